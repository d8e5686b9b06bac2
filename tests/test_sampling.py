"""The sampler's semantics on the CPU path (sample_tokens_ref) against an
fp64 oracle, and per-request sampling in the serving engine against
generate(seed=...).

Tolerance: a returned token t must be kept and own u to within eps,
lo_t - eps <= u <= hi_t + eps, with eps = 16 * delta_ref, delta_ref the
largest shift of the fp32 reference's CDF boundaries from the oracle's on
the test's own inputs."""

import numpy as np
import pytest
import torch

from metaflow_amd.models.llama import LlamaConfig, LlamaForCausalLM
from metaflow_amd.ops import kernels as K
from metaflow_amd.serving import ContinuousBatcher

from .sampling_oracle import (EPS_FACTOR, GAP_MIN, RowOracle, assert_draws,
                              delta_ref, make_case, pick_top_p, random_row,
                              row64, settings_for)


def _run_case(case):
    logits, temp, k, p, u, oracles = case
    d = delta_ref(logits, temp, k, p, oracles)
    eps = EPS_FACTOR * d
    tok = K.sample_tokens(logits, temp, k, p, u)
    assert tok.dtype == torch.int64 and tok.shape == (logits.size(0),)
    worst = assert_draws(tok, u, oracles, eps,
                         greedy=logits.float().argmax(-1))
    print("delta_ref %.3g eps %.3g worst miss %.3g" % (d, eps, worst))


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("V", [5, 1000, 2048])
def test_interval_check(V, dtype):
    _run_case(make_case(V, dtype, settings_for(V), rows_per_setting=2,
                        n_u=32, seed=100 + V))


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_mixed_rows_strided_view(dtype):
    """Every row its own parameters, greedy rows among them, the rows a
    [B, 3, V][:, -1] view."""
    V = 1000
    settings = [(0.0, 0, 1.0), (1.0, 0, 1.0), (0.7, 50, 1.0),
                (-1.0, 7, 0.5), (1.3, 0, 0.9), (0.8, 40, 0.8),
                (0.5, 1, 1.0), (2.0, 999, 0.95)]
    case = make_case(V, dtype, settings, rows_per_setting=1, n_u=4,
                     seed=7, strided=True)
    assert not case[0].is_contiguous()
    _run_case(case)


def test_top_k_and_top_p_off_values():
    """top_k >= V, top_k <= 0 and top_p >= 1 all mean "off"."""
    V = 300
    g = torch.Generator().manual_seed(3)
    x = (torch.randn(V, generator=g) * 3).to(torch.bfloat16)
    u = torch.rand(24, generator=g)
    logits = x[None].expand(24, V).contiguous()
    temp = torch.full((24,), 0.9)
    base = K.sample_tokens(logits, temp, torch.zeros(24, dtype=torch.int32),
                           torch.ones(24), u)
    for k, p in ((V, 1.0), (V + 5, 1.5), (-3, 1.0), (0, 2.0)):
        out = K.sample_tokens(logits, temp,
                              torch.full((24,), k, dtype=torch.int32),
                              torch.full((24,), p), u)
        assert out.tolist() == base.tolist(), (k, p)
    o = RowOracle(row64(x), 0.9, 0, 1.0)
    d = delta_ref(logits[:1], temp[:1], torch.zeros(1, dtype=torch.int32),
                  torch.ones(1), [o])
    assert_draws(base, u, [o] * 24, EPS_FACTOR * d)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_neg_inf_entries_never_return(dtype):
    V = 257
    g = torch.Generator().manual_seed(5)
    x = random_row(V, dtype, g)
    dead = torch.rand(V, generator=g) < 0.6
    dead[:3] = True            # the row starts and ends on dropped tokens
    dead[-3:] = True
    x[dead] = float("-inf")
    n = 64
    u = torch.rand(n, generator=g)
    u[0] = 0.0
    u[1] = float(np.nextafter(np.float32(1), np.float32(0)))
    logits = x[None].expand(n, V).contiguous()
    # top_k beyond the finite count keeps every finite token, no more
    for k, p in ((0, 1.0), (200, 1.0), (0, 0.9), (20, 0.8)):
        q, o = pick_top_p(row64(x), 1.1, k, p)
        temp = torch.full((n,), 1.1)
        kk = torch.full((n,), k, dtype=torch.int32)
        pp = torch.full((n,), q)
        d = delta_ref(logits[:1], temp[:1], kk[:1], pp[:1], [o])
        out = K.sample_tokens(logits, temp, kk, pp, u)
        assert not dead[out].any(), (k, p)
        assert_draws(out, u, [o] * n, EPS_FACTOR * d)


def test_greedy_ties_equal_argmax():
    g = torch.Generator().manual_seed(11)
    for dtype in (torch.bfloat16, torch.float32):
        x = (torch.randn(6, 513, generator=g) * 3).to(dtype)
        top = x.max() + 1
        x[0, [400, 17, 300]] = top
        x[1, [512, 511]] = top
        x[2, [0, 512]] = top
        x[3, :] = 1.5                      # a constant row
        x[4, 100] = top
        x[5, [7, 8]] = 0.0                 # -0.0 ties with +0.0
        x[5, 7] = -0.0
        x[5].clamp_(max=0.0)
        out = K.sample_tokens(x, torch.tensor([0.0, 0.0, -1.0, 0.0, 0.0, 0.0]),
                              torch.full((6,), 5, dtype=torch.int32),
                              torch.full((6,), 0.5), torch.full((6,), 0.7))
        assert out.tolist() == x.float().argmax(-1).tolist()


def test_top_k_one_and_tiny_top_p_equal_argmax():
    g = torch.Generator().manual_seed(13)
    for dtype in (torch.bfloat16, torch.float32):
        x = (torch.randn(16, 777, generator=g) * 3).to(dtype)
        am = torch.randint(0, 777, (16,), generator=g)
        x[torch.arange(16), am] = x.max() + 2         # a unique maximum
        u = torch.rand(16, generator=g)
        temp = torch.full((16,), 1.7)
        k1 = K.sample_tokens(x, temp, torch.ones(16, dtype=torch.int32),
                             torch.ones(16), u)
        p0 = K.sample_tokens(x, temp, torch.zeros(16, dtype=torch.int32),
                             torch.full((16,), 1e-6), u)
        assert k1.tolist() == am.tolist()
        assert p0.tolist() == am.tolist()


def test_tiny_temperature_is_finite():
    """(x - max) * (1/T): a tiny T gives the argmax, not a NaN row."""
    g = torch.Generator().manual_seed(17)
    x = torch.randn(4, 100, generator=g)
    out = K.sample_tokens(x, torch.tensor([1e-30, 1e-38, 1e-42, 1e-10]),
                          torch.zeros(4, dtype=torch.int32), torch.ones(4),
                          torch.tensor([0.0, 0.3, 0.6, 0.99]))
    assert out.tolist() == x.argmax(-1).tolist()


def grid_case(dtype=torch.bfloat16):
    """One row of V = 2048 with (0.9, 64, 0.85), 4096 times, u on the
    grid (i + 1/2) / 4096."""
    V, n = 2048, 4096
    g = torch.Generator().manual_seed(23)
    x = (torch.randn(V, generator=g) * 3).to(dtype)
    p, o = pick_top_p(row64(x), 0.9, 64, 0.85)
    assert o.gap >= GAP_MIN
    u = ((torch.arange(n, dtype=torch.float64) + 0.5) / n).float()
    return (x[None].expand(n, V).contiguous(), torch.full((n,), 0.9),
            torch.full((n,), 64, dtype=torch.int32), torch.full((n,), p),
            u, o)


def assert_grid(tokens, o):
    n = tokens.numel()
    counts = np.bincount(tokens.cpu().numpy(), minlength=o.keep.shape[0])
    assert counts[~o.keep].sum() == 0, "a dropped token was returned"
    want = n * (o.hi - o.lo)
    dev = np.abs(counts - want)[o.keep].max()
    print("kept %d gap %.3g max count deviation %.3f"
          % (o.keep.sum(), o.gap, dev))
    assert dev <= 2.0, dev


def test_grid_counts():
    logits, temp, k, p, u, o = grid_case()
    assert_grid(K.sample_tokens(logits, temp, k, p, u), o)


# ------------------------------------------------------------------ engine
@pytest.fixture(scope="module")
def tiny_model():
    torch.manual_seed(0)
    cfg = LlamaConfig.tiny(vocab=128, seq=256)
    return LlamaForCausalLM(cfg).eval()


# (prompt, max_new, temperature, top_k, top_p, seed); the last is greedy
REQUESTS = [
    ([5, 9, 17, 4], 9, 0.9, 0, 1.0, 11),
    (list(range(2, 25)), 7, 1.2, 20, 1.0, 12),
    ([100, 101], 10, 0.7, 0, 0.9, 13),
    ([64, 3, 99, 12, 54, 23], 8, 1.0, 30, 0.8, 14),
    ([7] * 11, 6, 0.0, 0, 1.0, None),
]


def _generate_ref(model, req):
    prompt, n, T, k, p, seed = req
    if T <= 0:
        return model.generate(torch.tensor([prompt]),
                              n)[0, len(prompt):].tolist()
    return model.generate(torch.tensor([prompt]), n, temperature=T,
                          top_k=k or None, top_p=p,
                          seed=seed)[0, len(prompt):].tolist()


@pytest.fixture(scope="module")
def generate_refs(tiny_model):
    return [_generate_ref(tiny_model, r) for r in REQUESTS]


def _serve(model, requests, **kw):
    b = ContinuousBatcher(model, **kw)
    reqs = [b.submit(p, n, temperature=T, top_k=k, top_p=tp, seed=s)
            for (p, n, T, k, tp, s) in requests]
    out = b.run()
    assert all(r.done for r in reqs)
    return [out[r.id] for r in reqs]


@pytest.mark.parametrize("kw", [
    dict(max_batch=3, max_len=64),
    dict(max_batch=3, max_len=64, prefill_chunk=8),
    dict(max_batch=3, max_len=64, num_pages=6),
    dict(max_batch=2, max_len=64, prefill_chunk=5, num_pages=4),
], ids=["dense", "chunked", "paged", "chunked-paged"])
def test_engine_sampled_requests_equal_generate(tiny_model, generate_refs,
                                                kw):
    out = _serve(tiny_model, REQUESTS, **kw)
    for i, (got, ref) in enumerate(zip(out, generate_refs)):
        assert got == ref, (i, got, ref)


def test_engine_request_alone_in_one_slot(tiny_model, generate_refs):
    for req, ref in zip(REQUESTS, generate_refs):
        assert _serve(tiny_model, [req], max_batch=1, max_len=64) == [ref]


def test_engine_seeds(tiny_model, generate_refs):
    a = _serve(tiny_model, REQUESTS, max_batch=3, max_len=64)
    b = _serve(tiny_model, REQUESTS, max_batch=3, max_len=64)
    assert a == b
    other = [(p, n, T, k, tp, None if s is None else s + 1000)
             for (p, n, T, k, tp, s) in REQUESTS]
    c = _serve(tiny_model, other, max_batch=3, max_len=64)
    assert c[-1] == a[-1]                      # the greedy request
    assert any(x != y for x, y in zip(a[:-1], c[:-1]))


def test_engine_seed_none_follows_manual_seed(tiny_model):
    reqs = [([5, 9, 17], 8, 1.0, 0, 1.0, None)]
    torch.manual_seed(123)
    a = _serve(tiny_model, reqs, max_batch=2, max_len=32)
    torch.manual_seed(123)
    b = _serve(tiny_model, reqs, max_batch=2, max_len=32)
    assert a == b


def test_engine_default_requests_are_greedy(tiny_model, monkeypatch):
    """Default-argument requests carry the greedy parameters, draw
    nothing, decode what generate() decodes, and are selected by the
    sampler: one call per first token and one per decode step, each over
    all its rows."""
    calls = []
    real = K.sample_tokens

    def spy(logits, temperature, *rest):
        calls.append((logits.size(0), temperature.tolist()))
        return real(logits, temperature, *rest)

    monkeypatch.setattr(K, "sample_tokens", spy)
    prompts = [([5, 9, 17, 4], 6), ([100, 101], 8)]
    b = ContinuousBatcher(tiny_model, max_batch=2, max_len=64)
    state = torch.get_rng_state()
    reqs = [b.submit(p, n) for p, n in prompts]
    for r in reqs:
        assert (r.temperature, r.top_k, r.top_p, r.seed) == (0.0, 0, 1.0,
                                                             None)
    steps = 0
    while b.queue or any(r is not None for r in b.slots):
        steps += b.step() > 0
    out = {r.id: r.generated for r in reqs}
    assert torch.equal(torch.get_rng_state(), state)   # no draw was made
    # two first tokens (one row each), then one call per decode step over
    # both slots, every row greedy
    assert sorted(c[0] for c in calls) == [1, 1] + [2] * steps
    assert all(t == 0.0 for c in calls for t in c[1])
    for r, (p, n) in zip(reqs, prompts):
        ref = tiny_model.generate(torch.tensor([p]), n)[0, len(p):].tolist()
        assert out[r.id] == ref


def test_generate_seed_rows_are_seed_plus_row(tiny_model):
    """Row b of a seeded batch generate is the single-row generate with
    seed + b."""
    prompt = torch.tensor([[5, 9, 17, 4], [5, 9, 17, 4]])
    both = tiny_model.generate(prompt, 8, temperature=1.0, top_p=0.95,
                               seed=40)
    for b in range(2):
        one = tiny_model.generate(prompt[b:b + 1], 8, temperature=1.0,
                                  top_p=0.95, seed=40 + b)
        assert both[b].tolist() == one[0].tolist()
