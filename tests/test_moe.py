"""The MoE decode references on the CPU: moe_route_ref against the model's
own routing formula and a stable sort, moe_ffn_ref against MoELayer.forward
in fp64.

An fp64 MoELayer still routes and applies SwiGLU in fp32 (router logits
``.float()``, swiglu_ref), so it matches the all-fp64 reference to fp32
rounding only: h is off by <= 2^-24 relative per element, which the down
projection (512 terms of size <= ~0.3) turns into <= ~1e-6 absolute on
outputs of size ~1. FWD_ATOL, FWD_RTOL are that with a factor of 5."""

import pytest
import torch

from metaflow_amd.models.mixtral import MixtralConfig, MoELayer
from metaflow_amd.ops import kernels as K


FWD_ATOL, FWD_RTOL = 5e-6, 1e-5


def gapped_logits(T, E, seed):
    """Rows whose entries differ by >= 1e-3: a random permutation of an
    E-point grid of step 0.05, jittered by less than 0.02."""
    g = torch.Generator().manual_seed(seed)
    grid = 0.05 * torch.arange(E, dtype=torch.float32)
    perm = torch.rand(T, E, generator=g).argsort(-1)
    return grid[perm] + 0.02 * torch.rand(T, E, generator=g)


@pytest.mark.parametrize("T,E,k", [(1, 4, 1), (33, 4, 2), (33, 64, 8)])
def test_route_ref_is_the_models_formula(T, E, k):
    logits = gapped_logits(T, E, seed=E + k)
    expert, weight, order, offset = K.moe_route_ref(logits, k)
    w, e = torch.softmax(logits, dim=-1).topk(k, dim=-1)
    w = w / w.sum(-1, keepdim=True)
    assert torch.equal(expert.long(), e)
    torch.testing.assert_close(weight, w, rtol=1e-5, atol=0)
    flat = e.reshape(-1)
    assert torch.equal(order.long(), torch.argsort(flat, stable=True))
    counts = torch.bincount(flat, minlength=E)
    assert offset[0] == 0
    assert torch.equal(offset[1:].long(), counts.cumsum(0))


def test_route_ref_ties_pick_the_lowest_index():
    logits = torch.tensor([[1.0, 2.0, 2.0, 2.0, 0.5],
                           [0.0, 0.0, 0.0, 0.0, 0.0]])
    expert, weight, _, _ = K.moe_route_ref(logits, 2)
    assert expert.tolist() == [[1, 2], [0, 1]]
    assert weight.tolist() == [[0.5, 0.5], [0.5, 0.5]]


def test_ffn_ref_is_the_layer_forward_in_fp64():
    torch.manual_seed(0)
    cfg = MixtralConfig.tiny()
    layer = MoELayer(cfg).double()
    for p in layer.parameters():
        torch.nn.init.normal_(p, std=0.1)
    x = torch.randn(7, cfg.hidden_size, dtype=torch.float64)
    with torch.no_grad():
        want = layer(x[None])[0]
        logits = layer.router(x)
        ws = [[getattr(e, n).weight for e in layer.local_experts]
              for n in ("gate_proj", "up_proj", "down_proj")]
        got = K.moe_ffn_ref(x, logits, *ws, cfg.top_k, dtype=torch.float64)
        # the CPU path of the public entries is the reference
        dec = layer.decode(x[None])[0]
    torch.testing.assert_close(got, want, rtol=FWD_RTOL, atol=FWD_ATOL)
    torch.testing.assert_close(dec, want, rtol=FWD_RTOL, atol=FWD_ATOL)


def test_ffn_is_inference_only():
    cfg = MixtralConfig.tiny()
    layer = MoELayer(cfg)
    x = torch.zeros(1, 1, cfg.hidden_size, dtype=torch.bfloat16)
    with pytest.raises(RuntimeError, match="inference-only"):
        layer.decode(x)
