"""moe.hip on the GPU: device routing against moe_route_ref, K.moe_ffn
against the fp64 reference at the shapes that take each path of the grouped
kernels, and the captured serving step of a fused-MoE Mixtral.

moe_ffn's bound is relative to the eager block: MoELayer.forward runs on
the same inputs and weights and its worst per-token relative L2 error
against the same fp64 reference is measured; the kernel must come within
2x of it. Eager rounds g, u, h, y and each contribution to bf16 and sums in
bf16, the kernel rounds h and the output only, so 2x is slack. Measured
(worst per-token, kernel / eager) are printed and recorded in
docs/KERNELS.md."""

import pytest
import torch

from metaflow_amd.models.mixtral import (
    MixtralConfig,
    MixtralForCausalLM,
    MoELayer,
)
from metaflow_amd.ops import kernels as K

pytestmark = pytest.mark.gpu
HIDDEN = 256


def setup_module():
    assert K.extension_loaded(), "_mfx_hip must be built for GPU tests"


@pytest.fixture
def dev():
    return torch.device("cuda:0")


def _route_logits(T, E, ties):
    g = torch.Generator().manual_seed(T * 100 + E)
    if ties:  # three distinct values: every row is full of equal logits
        return torch.randint(0, 3, (T, E), generator=g).float()
    return torch.randn(T, E, generator=g)


@pytest.mark.parametrize("T", [1, 33])
@pytest.mark.parametrize("E,k,ties", [
    (4, 1, False), (4, 2, False), (64, 1, False), (64, 2, False),
    (64, 8, False), (64, 8, True)])
def test_route(dev, T, E, k, ties):
    logits = _route_logits(T, E, ties)
    ref = K.moe_route_ref(logits, k)
    w64 = K.moe_route_ref(logits.double(), k)[1]
    expert, weight, order, offset = K.moe_route(logits.to(dev), k)
    for got, want in zip((expert, order, offset), (ref[0], ref[2], ref[3])):
        assert got.dtype == torch.int32
        assert torch.equal(got.cpu(), want)
    torch.testing.assert_close(weight.cpu().double(), w64, rtol=1e-6, atol=0)


def _picked_logits(picks, E):
    """Logits that send token t to the experts picks[t], in that order."""
    g = torch.Generator().manual_seed(len(picks))
    logits = 0.1 * torch.rand(len(picks), E, generator=g)
    for t, row in enumerate(picks):
        for j, e in enumerate(row):
            logits[t, e] += 2.0 - 0.7 * j
    return logits


# name: (E, k, inter, experts of each token, down_splits)
FFN_CASES = {
    # expert 3 receives nothing
    "empty_expert": (4, 2, 384, [(t % 3, (t + 1) % 3) for t in range(5)]),
    # one expert, groups of 32 + 1
    "groups_32_1": (2, 1, 256, [(0,)] * 33),
    # expert 0 holds exactly 32 entries, the last expert 35 (32 + 3)
    "full_and_ragged": (4, 2, 512, [(0, 3)] * 32 + [(3, 1)] * 3
                        + [(1, 2)] * 5),
}


class _FixedRouter(torch.nn.Module):
    def __init__(self, logits):
        super().__init__()
        self.logits = logits

    def forward(self, flat):
        return self.logits


def _worst_row_err(out, ref):
    out = out.double().cpu()
    assert torch.isfinite(out).all()
    return ((out - ref).norm(dim=-1) / ref.norm(dim=-1)).max().item()


@pytest.mark.parametrize("name,splits", [
    ("empty_expert", 1), ("empty_expert", 3), ("groups_32_1", None),
    ("full_and_ragged", None)])
def test_ffn(dev, name, splits):
    E, k, inter, picks = FFN_CASES[name]
    T = len(picks)
    logits = _picked_logits(picks, E)
    counts = torch.bincount(K.moe_route_ref(logits, k)[0].reshape(-1).long(),
                            minlength=E).tolist()
    print(name, "entries per expert", counts)
    g = torch.Generator().manual_seed(T)
    layer = MoELayer(MixtralConfig(hidden_size=HIDDEN, num_experts=E,
                                   intermediate_size=inter, top_k=k))
    for p in layer.parameters():
        p.data = (0.05 * torch.randn(p.shape, generator=g)).to(p.dtype)
    layer = layer.to(dev)
    ws = [[getattr(e, n).weight for e in layer.local_experts]
          for n in ("gate_proj", "up_proj", "down_proj")]
    big = torch.full((T + 2, HIDDEN), float("nan"), dtype=torch.bfloat16)
    big[1:T + 1] = torch.randn(T, HIDDEN, generator=g).to(torch.bfloat16)
    x = big.to(dev)[1:T + 1]
    ref = K.moe_ffn_ref(x.cpu(), logits, *[[w.cpu() for w in m] for m in ws],
                        k, dtype=torch.float64)

    with torch.no_grad():
        out = K.moe_ffn(x, logits.to(dev), *ws, k, down_splits=splits)
        again = K.moe_ffn(x, logits.to(dev), *ws, k, down_splits=splits)
        layer.router = _FixedRouter(logits.to(dev))
        eager = layer(x[None])[0]
    assert out.shape == x.shape and out.dtype == torch.bfloat16
    assert torch.equal(out, again)
    err, eager_err = _worst_row_err(out, ref), _worst_row_err(eager, ref)
    print("%s splits=%s worst per-token rel L2: kernel %.3e, eager %.3e"
          % (name, splits, err, eager_err))
    assert err <= 2 * eager_err


def test_serving_captures_fused_mixtral(dev):
    torch.manual_seed(0)
    cfg = MixtralConfig.tiny(vocab=256, seq=256)
    cfg.fused_moe_decode = True
    m = MixtralForCausalLM(cfg).to(dev).eval()
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
