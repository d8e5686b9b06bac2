"""The E4M3 kernels of moe.hip and moe_prefill.hip on the GPU: K.moe_ffn over
quantised experts against the fp64 reference on the exactly dequantised
weights (w8.double() * scale), at the smallest shapes that reach each branch
of the stream and the tiled kernels, and the captured serving step of a
Mixtral with quantised experts.

The bound is that of test_moe_gpu.py: the worst per-token relative L2 error
must come within 2x of what the eager block (Fp8Expert.forward, which
rounds the dequantised weights to bf16 as well as g, u, h, y) makes of the
same inputs. Row r of every weight is multiplied by 2 ** ((5 r) % 7 - 3)
before quantising, so the scales of neighbouring rows differ by up to 64x
and a wrong row-to-scale pairing through the C layout is a gross error.
Measured (kernel / eager) are printed and recorded in docs/KERNELS.md."""

import pytest
import torch

from metaflow_amd.models.mixtral import (
    MixtralConfig,
    MixtralForCausalLM,
    MoELayer,
)
from metaflow_amd.ops import kernels as K

from .test_moe_prefill_gpu import (
    _FixedRouter,
    _picked_logits,
    _picks,
    _worst_row_err,
)

pytestmark = pytest.mark.gpu


def setup_module():
    assert K.extension_loaded(), "_mfx_hip must be built for GPU tests"


@pytest.fixture
def dev():
    return torch.device("cuda:0")


# name: (path, hidden, E, k, inter, experts of each token, down_splits)
EMPTY = [(t % 3, (t + 1) % 3) for t in range(5)]   # expert 3 gets nothing
CASES = {
    # hidden 384: an odd number of chunks for gate/up
    "stream_odd_chunks_1": ("stream", 384, 4, 2, 384, EMPTY, 1),
    "stream_odd_chunks_3": ("stream", 384, 4, 2, 384, EMPTY, 3),
    # counts 32 / 8 / 5 / 35: a full group, and a ragged second group
    "stream_groups": ("stream", 256, 4, 2, 512,
                      [(0, 3)] * 32 + [(3, 1)] * 3 + [(1, 2)] * 5, None),
    "tiled_edges": ("tiled", 256, 6, 2, 384,
                    _picks([0, 1, 127, 128, 129, 257], 2), None),
    "tiled_one_token": ("tiled", 256, 4, 2, 384, _picks([0, 1, 0, 1], 2),
                        None),
}


@pytest.mark.parametrize("name", sorted(CASES))
def test_ffn_fp8(dev, name):
    path, hidden, E, k, inter, picks, splits = CASES[name]
    T = len(picks)
    logits = _picked_logits(picks, E)
    g = torch.Generator().manual_seed(T)
    layer = MoELayer(MixtralConfig(hidden_size=hidden, num_experts=E,
                                   intermediate_size=inter, top_k=k))
    for p in layer.local_experts.parameters():
        rows = 2.0 ** ((5 * torch.arange(p.size(0))) % 7 - 3)
        p.data = (0.05 * torch.randn(p.shape, generator=g) *
                  rows[:, None]).to(p.dtype)
    layer = layer.to(dev).quantize_experts_()
    table = layer._table()
    assert table.fp8 and tuple(table.tab.shape) == (6, E)
    big = torch.full((T + 2, hidden), float("nan"), dtype=torch.bfloat16)
    big[1:T + 1] = torch.randn(T, hidden, generator=g).to(torch.bfloat16)
    x = big.to(dev)[1:T + 1]   # inside a NaN-filled allocation
    exact = [[K.moe_dequant_ref(w.cpu(), s.cpu(), torch.float64)
              for w, s in zip(ws, ss)]
             for ws, ss in zip(table.weights, table.scales)]
    ref = K.moe_ffn_ref(x.cpu(), logits, *exact, k, dtype=torch.float64)

    def run(x, logits):
        return K.moe_ffn(x, logits.to(dev), table, top_k=k, path=path,
                         down_splits=splits)

    with torch.no_grad():
        out, again = run(x, logits), run(x, logits)
        layer.router = _FixedRouter(logits.to(dev))
        eager = layer(x[None])[0]
    assert out.shape == x.shape and out.dtype == torch.bfloat16
    assert torch.equal(out, again)
    err, eager_err = _worst_row_err(out, ref), _worst_row_err(eager, ref)
    print("%s T=%d worst per-token rel L2: kernel %.3e, eager %.3e"
          % (name, T, err, eager_err))
    assert err <= 2 * eager_err

    if path == "tiled" and T > 1:
        # the same tokens in another order (13 is coprime to 321): rows do
        # not depend on their place in the tiles
        perm = (13 * torch.arange(T) + 3) % T
        with torch.no_grad():
            moved = run(x[perm.to(dev)].contiguous(), logits[perm])
        assert torch.equal(moved, out[perm.to(dev)])


def test_serving_captures_fp8_mixtral(dev):
    torch.manual_seed(0)
    cfg = MixtralConfig.tiny(vocab=256, seq=256)
    cfg.fused_moe_prefill = cfg.fused_moe_decode = True
    m = MixtralForCausalLM(cfg).to(dev).eval().quantize_experts_()
    assert m.graph_safe_decode and all(la.moe.quantized for la in m.layers)
    from metaflow_amd.serving import ContinuousBatcher

    prompts = [([5, 9, 17, 4], 5), (list(range(2, 20)), 4)]
    outs = []
    for graph in (True, False):
        b = ContinuousBatcher(m, max_batch=2, max_len=64, graph=graph)
        assert (b._graph is not None) == graph
        reqs = [b.submit(p, n) for p, n in prompts]
        res = b.run()
        outs.append([res[r.id] for r in reqs])
    assert outs[0] == outs[1]
    assert [len(o) for o in outs[0]] == [n for _, n in prompts]
