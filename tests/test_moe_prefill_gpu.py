"""moe_prefill.hip on the GPU: the multi-block route against moe_route_ref,
K.moe_ffn(path="tiled") against the fp64 reference with per-expert counts
on the edges of the 128-entry tile, independence of a token's result from
its place in the tiles, hipGraph replay after the routing has changed, and
a Mixtral whose prefill takes the fused block.

The bound on moe_ffn is that of test_moe_gpu.py: the worst per-token
relative L2 error against the fp64 reference must come within 2x of what
the eager MoELayer.forward makes of the same inputs and weights. Measured
(kernel / eager) are printed and recorded in docs/KERNELS.md."""

import pytest
import torch

from metaflow_amd.models.mixtral import (
    MixtralConfig,
    MixtralForCausalLM,
    MoELayer,
)
from metaflow_amd.ops import kernels as K

pytestmark = pytest.mark.gpu
HIDDEN = 256   # four K chunks of 64: a prologue, steady steps, a last chunk
TM = 128       # the kernels' M tile


def setup_module():
    assert K.extension_loaded(), "_mfx_hip must be built for GPU tests"


@pytest.fixture
def dev():
    return torch.device("cuda:0")


# 300: two route blocks; 1100 x 8: five blocks of 2048 entries, 64 experts;
# 2049: the first T past the one-workgroup kernel. wide=True at (300, 4, 2)
# is the wide path where the old kernel also serves.
@pytest.mark.parametrize("T,E,k,ties", [
    (300, 4, 2, False), (1100, 64, 8, False), (1100, 64, 8, True),
    (2049, 8, 1, False)])
def test_route(dev, T, E, k, ties):
    g = torch.Generator().manual_seed(T * 100 + E)
    logits = (torch.randint(0, 3, (T, E), generator=g).float() if ties
              else torch.randn(T, E, generator=g))
    ref = K.moe_route_ref(logits, k)
    w64 = K.moe_route_ref(logits.double(), k)[1]
    expert, weight, order, offset = K.moe_route(logits.to(dev), k, wide=True)
    for got, want in zip((expert, order, offset), (ref[0], ref[2], ref[3])):
        assert got.dtype == torch.int32
        assert torch.equal(got.cpu(), want)
    torch.testing.assert_close(weight.cpu().double(), w64, rtol=1e-6, atol=0)


def _picks(counts, k):
    """Experts of each token, k distinct ones, with counts[e] entries for
    expert e: the sorted entry list cut into k runs, token t taking the
    t-th of each run (distinct as long as no count exceeds a run)."""
    flat = [e for e, c in enumerate(counts) for _ in range(c)]
    T = len(flat) // k
    assert T * k == len(flat) and max(counts) <= T
    return [tuple(flat[t + j * T] for j in range(k)) for t in range(T)]


def _picked_logits(picks, E):
    """Logits that send token t to the experts picks[t], in that order."""
    g = torch.Generator().manual_seed(len(picks))
    logits = 0.1 * torch.rand(len(picks), E, generator=g)
    for t, row in enumerate(picks):
        for j, e in enumerate(row):
            logits[t, e] += 2.0 - 0.7 * j
    return logits


# name: (k, inter, entries per expert)
FFN_CASES = {
    "tile_edges": (2, 384, [0, 1, TM - 1, TM, TM + 1, 2 * TM + 1]),
    "top1_inter128": (1, 128, [TM + 1, 0, TM, 1, TM - 1]),
    "one_token": (2, 384, [0, 1, 0, 1]),
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


@pytest.mark.parametrize("name", sorted(FFN_CASES))
def test_ffn(dev, name):
    k, inter, counts = FFN_CASES[name]
    E = len(counts)
    logits = _picked_logits(_picks(counts, k), E)
    T = logits.size(0)
    assert torch.bincount(K.moe_route_ref(logits, k)[0].reshape(-1).long(),
                          minlength=E).tolist() == counts
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
    x = big.to(dev)[1:T + 1]   # inside a NaN-filled allocation
    ref = K.moe_ffn_ref(x.cpu(), logits, *[[w.cpu() for w in m] for m in ws],
                        k, dtype=torch.float64)
    with torch.no_grad():
        out = K.moe_ffn(x, logits.to(dev), *ws, k, path="tiled")
        again = K.moe_ffn(x, logits.to(dev), *ws, k, path="tiled")
        layer.router = _FixedRouter(logits.to(dev))
        eager = layer(x[None])[0]
    assert out.shape == x.shape and out.dtype == torch.bfloat16
    assert torch.equal(out, again)
    err, eager_err = _worst_row_err(out, ref), _worst_row_err(eager, ref)
    print("%s T=%d worst per-token rel L2: kernel %.3e, eager %.3e"
          % (name, T, err, eager_err))
    assert err <= 2 * eager_err

    if T > 1:
        # the same tokens in another order: 13 is coprime to both T (321,
        # 385), so neighbours in a tile end up in different tiles and places
        perm = (13 * torch.arange(T) + 3) % T
        with torch.no_grad():
            moved = K.moe_ffn(x[perm.to(dev)].contiguous(),
                              logits[perm].to(dev), *ws, k, path="tiled")
        assert torch.equal(moved, out[perm.to(dev)])


def test_capture_replays_a_new_routing(dev):
    T, E, k, inter = 300, 4, 2, 384
    first = _picked_logits([(t % 4, (t + 1) % 4) for t in range(T)], E)
    # expert 3 goes from 150 entries to none, expert 0 from 150 to 300
    second = _picked_logits([(0, 1 + t % 2) for t in range(T)], E)
    g = torch.Generator().manual_seed(T)
    ws = [[(0.05 * torch.randn(shape, generator=g)).to(torch.bfloat16)
           .to(dev) for _ in range(E)]
          for shape in ((inter, HIDDEN), (inter, HIDDEN), (HIDDEN, inter))]
    table = K.MoeTable(*ws)
    xs = torch.randn(2, T, HIDDEN, generator=g).to(torch.bfloat16).to(dev)
    x, logits = xs[0].clone(), first.to(dev)
    with torch.no_grad():
        K.moe_ffn(x, logits, table, top_k=k, path="tiled")
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            out = K.moe_ffn(x, logits, table, top_k=k, path="tiled")
        x.copy_(xs[1])
        logits.copy_(second.to(dev))
        want = K.moe_ffn(xs[1], second.to(dev), table, top_k=k, path="tiled")
        for _ in range(3):
            out.zero_()
            graph.replay()
            torch.cuda.synchronize()
            assert torch.equal(out, want)


def test_model_prefill_takes_the_fused_block(dev):
    torch.manual_seed(0)
    cfg = MixtralConfig.tiny(vocab=256, seq=256)
    cfg.fused_moe_prefill = cfg.fused_moe_decode = True
    m = MixtralForCausalLM(cfg).to(dev).eval()
    from metaflow_amd.serving import ContinuousBatcher

    g = torch.Generator().manual_seed(1)
    long_prompt = torch.randint(0, 256, (200,), generator=g).tolist()
    prompts = [(long_prompt, 4), (list(range(2, 20)), 5)]
    for chunk in (64, None):
        b = ContinuousBatcher(m, max_batch=2, max_len=256, graph=True,
                              prefill_chunk=chunk)
        assert b._graph is not None
        reqs = [b.submit(p, n) for p, n in prompts]
        res = b.run()
        assert [len(res[r.id]) for r in reqs] == [n for _, n in prompts]

    # the block inside a plain forward: T = 200 takes the tiled kernels
    # (a mean expert run of 100 entries), seen on the layer's own input
    moe = m.layers[1].moe
    seen = {}
    hook = moe.register_forward_hook(
        lambda mod, args, out: seen.update(x=args[0], out=out))
    tokens = torch.tensor([long_prompt], device=dev)
    with torch.no_grad():
        m(tokens)
        hook.remove()
        x = seen["x"][0]
        cfg.fused_moe_prefill = False
        eager = moe(seen["x"])[0]
        cfg.fused_moe_prefill = True
        logits = moe.router(x).float()
    ws = [[getattr(e, n).weight.cpu() for e in moe.local_experts]
          for n in ("gate_proj", "up_proj", "down_proj")]
    ref = K.moe_ffn_ref(x.cpu(), logits.cpu(), *ws, cfg.top_k,
                        dtype=torch.float64)
    err = _worst_row_err(seen["out"][0], ref)
    eager_err = _worst_row_err(eager, ref)
    print("model block worst per-token rel L2: fused %.3e, eager %.3e"
          % (err, eager_err))
    assert err <= 2 * eager_err
    # a call that needs a backward stays on the eager block (the fused one
    # would raise)
    assert m(tokens).requires_grad
