"""The prefill-sized MoE entries on the CPU: the references and K.moe_ffn
accept T * top_k up to 65536, and a MoELayer with cfg.fused_moe_prefill
returns the reference's result from forward and leaves calls that need a
backward on the eager block."""

import pytest
import torch

from metaflow_amd.models.mixtral import MixtralConfig, MoELayer
from metaflow_amd.ops import kernels as K


def test_wide_shapes_are_accepted():
    T, E, k, hidden, inter = 1100, 64, 8, 128, 128   # 8800 entries
    g = torch.Generator().manual_seed(0)
    logits = torch.randn(T, E, generator=g)
    expert, weight, order, offset = K.moe_route_ref(logits, k)
    assert order.shape == (T * k,) and int(offset[-1]) == T * k
    assert torch.equal(order.long().sort().values, torch.arange(T * k))
    ws = [[0.05 * torch.randn(shape, generator=g) for _ in range(E)]
          for shape in ((inter, hidden), (inter, hidden), (hidden, inter))]
    x = torch.randn(T, hidden, generator=g)
    ref = K.moe_ffn_ref(x, logits, *ws, k)
    for path in (None, "tiled"):
        assert torch.equal(K.moe_ffn(x, logits, *ws, k, path=path), ref)
    with pytest.raises(ValueError, match="stream path"):
        K.moe_ffn(x, logits, *ws, k, path="stream")
    with pytest.raises(ValueError):
        K.moe_route_ref(torch.zeros(65537, 4), 1)
    with pytest.raises(RuntimeError, match="inference-only"):
        K.moe_ffn(x.requires_grad_(), logits, *ws, k, path="tiled")


def test_layer_forward_takes_the_fused_block():
    torch.manual_seed(0)
    cfg = MixtralConfig.tiny()
    cfg.fused_moe_prefill = True
    layer = MoELayer(cfg).float()
    for p in layer.parameters():
        torch.nn.init.normal_(p, std=0.1)
    x = torch.randn(1, 300, cfg.hidden_size)
    ws = [[getattr(e, n).weight for e in layer.local_experts]
          for n in ("gate_proj", "up_proj", "down_proj")]
    with torch.no_grad():
        got = layer(x)
        ref = K.moe_ffn_ref(x[0], layer.router(x[0]), *ws, cfg.top_k)
    assert torch.equal(got[0], ref)
    # a call that needs a backward is refused by the fused block and stays
    # on the eager one
    xg = x.clone().requires_grad_()
    out = layer(xg)
    out.sum().backward()
    assert xg.grad is not None and xg.grad.shape == x.shape
    torch.testing.assert_close(out.detach(), got, rtol=1e-4, atol=1e-5)
