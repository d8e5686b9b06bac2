"""The fused sampler kernel (ops/csrc/sampling.hip) at its edges, against
the fp64 oracle of sampling_oracle.py, and the engine's sampled decoding
on the GPU. Tolerance as in test_sampling.py: eps = 16 * delta_ref, with
delta_ref measured on each test's own inputs through the CPU reference."""

import pytest
import torch

from metaflow_amd.models.llama import LlamaConfig, LlamaForCausalLM
from metaflow_amd.ops import kernels as K
from metaflow_amd.serving import ContinuousBatcher

from .sampling_oracle import (EPS_FACTOR, assert_draws, delta_ref,
                              make_case, pick_top_p, random_row, row64,
                              settings_for)
from .test_sampling import assert_grid, grid_case

pytestmark = pytest.mark.gpu

DTYPES = [torch.bfloat16, torch.float32]
# elements one workgroup covers per tile: 1024 threads x one 16-byte vector
SPAN = {torch.bfloat16: 1024 * 8, torch.float32: 1024 * 4}


def _dev(case):
    logits, temp, k, p, u, oracles = case
    if logits.is_contiguous():
        dl = logits.cuda()
    else:
        # rebuild the [B, 3, V][:, -1] view on the device
        full = torch.zeros(logits.size(0), 3, logits.size(1),
                           dtype=logits.dtype, device="cuda")
        full[:, -1] = logits.cuda()
        dl = full[:, -1]
        assert dl.stride(0) == 3 * logits.size(1)
    return dl, temp.cuda(), k.cuda(), p.cuda(), u.cuda()


def _run_case(case):
    logits, temp, k, p, u, oracles = case
    d = delta_ref(logits, temp, k, p, oracles)
    eps = EPS_FACTOR * d
    args = _dev(case)
    tok = K.sample_tokens(*args)
    assert tok.is_cuda and tok.dtype == torch.int64
    worst = assert_draws(tok, u, oracles, eps,
                         greedy=logits.float().argmax(-1))
    print("V %d delta_ref %.3g eps %.3g worst miss %.3g"
          % (logits.size(1), d, eps, worst))
    # the same call twice is bit-equal
    assert torch.equal(tok, K.sample_tokens(*args))


def _mixed(V):
    """The four settings plus greedy rows, in one launch."""
    return settings_for(V) + [(0.0, 3, 0.5), (-1.0, 0, 1.0)]


@pytest.mark.parametrize("dtype", DTYPES)
def test_shorter_than_one_vector(dtype):
    _run_case(make_case(5, dtype, _mixed(5), 2, 16, seed=1))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("V", [1000, 1001])
def test_strided_view_rows(V, dtype):
    """[B, 3, V][:, -1]: V = 1001 puts every row base off the 16-byte
    grid, a different offset per row."""
    case = make_case(V, dtype, _mixed(V), 2, 8, seed=2, strided=True)
    _run_case(case)


@pytest.mark.parametrize("dtype", DTYPES)
def test_unaligned_base_pointer(dtype):
    """A contiguous batch whose first row starts one element past an
    aligned address."""
    V = 1003
    logits, temp, k, p, u, oracles = make_case(V, dtype, _mixed(V), 1, 8,
                                               seed=3)
    B = logits.size(0)
    flat = torch.zeros(B * V + 1, dtype=dtype, device="cuda")
    dl = flat[1:].view(B, V)
    dl.copy_(logits)
    assert dl.data_ptr() % 16 != 0
    d = delta_ref(logits, temp, k, p, oracles)
    tok = K.sample_tokens(dl, temp.cuda(), k.cuda(), p.cuda(), u.cuda())
    assert_draws(tok, u, oracles, EPS_FACTOR * d,
                 greedy=logits.float().argmax(-1))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("off", [-1, 0, 1])
def test_tile_span_edges(off, dtype):
    V = SPAN[dtype] + off
    _run_case(make_case(V, dtype, _mixed(V), 1, 6, seed=4 + off))


@pytest.mark.parametrize("dtype", DTYPES)
def test_llama3_vocab(dtype):
    """V = 128 256, B = 3: three rows, three settings, one launch."""
    V = 128256
    settings = [(0.8, 40, 0.8), (1.3, 0, 0.9), (0.7, 50, 1.0)]
    _run_case(make_case(V, dtype, settings, 1, 1, seed=9))


@pytest.mark.parametrize("dtype", DTYPES)
def test_llama3_vocab_more_draws(dtype):
    """The same vocabulary with a spread of u per row, plain sampling
    (the whole row carries weight) among the settings."""
    V = 128256
    _run_case(make_case(V, dtype, settings_for(V), 1, 6, seed=10))


def test_grid_counts_gpu():
    logits, temp, k, p, u, o = grid_case()
    tok = K.sample_tokens(logits.cuda(), temp.cuda(), k.cuda(), p.cuda(),
                          u.cuda())
    assert_grid(tok, o)


@pytest.mark.parametrize("dtype", DTYPES)
def test_ties_and_argmax(dtype):
    g = torch.Generator().manual_seed(11)
    V = SPAN[dtype] + 513
    x = (torch.randn(8, V, generator=g) * 3).to(dtype)
    top = x.max() + 1
    x[0, [V - 1, 17, 4000]] = top
    x[1, [V - 1, V - 2]] = top
    x[2, [0, V - 1]] = top
    x[3, :] = 1.5                          # a constant row
    x[4, 4097] = top
    x[5].clamp_(max=0.0)                   # many ties at zero, one -0.0
    x[5, 0] = -1.0
    x[5, 1] = -0.0
    x[6, :] = float("-inf")                # outside the contract: in range
    x[6, 77] = -3.0
    # rows 0-5 greedy (the other parameters are ignored), 6-7 top_k = 1
    temp = torch.tensor([0.0, 0.0, -1.0, 0.0, 0.0, 0.0, 1.0, 1.0])
    k = torch.tensor([5, 5, 5, 5, 5, 5, 1, 1], dtype=torch.int32)
    p = torch.tensor([0.5, 0.5, 0.5, 0.5, 0.5, 0.5, 1.0, 1.0])
    u = torch.full((8,), 0.7)
    want = x.float().argmax(-1)
    am7 = int(want[7])
    x[7, am7] = x[7, am7] + 2              # a unique maximum
    out = K.sample_tokens(x.cuda(), temp.cuda(), k.cuda(), p.cuda(),
                          u.cuda())
    assert out.cpu().tolist() == want.tolist()
    # top_p = 1e-6 on the rows with a unique maximum
    out = K.sample_tokens(x[[4, 6, 7]].cuda(), torch.ones(3).cuda(),
                          torch.zeros(3, dtype=torch.int32).cuda(),
                          torch.full((3,), 1e-6).cuda(),
                          torch.tensor([0.0, 0.5, 0.999]).cuda())
    assert out.cpu().tolist() == want[[4, 6, 7]].tolist()


@pytest.mark.parametrize("dtype", DTYPES)
def test_neg_inf_entries_never_return_gpu(dtype):
    V = 9001
    g = torch.Generator().manual_seed(5)
    x = random_row(V, dtype, g)
    dead = torch.rand(V, generator=g) < 0.6
    dead[:9] = True
    dead[-9:] = True
    x[dead] = float("-inf")
    n = 48
    u = torch.rand(n, generator=g)
    u[0] = 0.0
    u[1] = 1.0 - 2.0 ** -24
    logits = x[None].expand(n, V).contiguous().cuda()
    for k, p in ((0, 1.0), (5000, 1.0), (0, 0.9), (20, 0.8)):
        q, o = pick_top_p(row64(x), 1.1, k, p)
        temp = torch.full((n,), 1.1)
        kk = torch.full((n,), k, dtype=torch.int32)
        pp = torch.full((n,), q)
        d = delta_ref(x[None], temp[:1], kk[:1], pp[:1], [o])
        out = K.sample_tokens(logits, temp.cuda(), kk.cuda(), pp.cuda(),
                              u.cuda()).cpu()
        assert not dead[out].any(), (k, p)
        assert_draws(out, u, [o] * n, EPS_FACTOR * d)


def test_non_finite_rows_stay_in_range():
    """NaN rows and all -inf rows are outside the contract but return an
    index in [0, V)."""
    V = 3000
    x = torch.randn(4, V)
    x[0, ::7] = float("nan")
    x[1, :] = float("nan")
    x[2, :] = float("-inf")
    x[3, 5] = float("inf")
    for temp, k, p in ((0.0, 0, 1.0), (1.0, 0, 1.0), (1.0, 10, 0.5)):
        out = K.sample_tokens(x.cuda(), torch.full((4,), temp).cuda(),
                              torch.full((4,), k, dtype=torch.int32).cuda(),
                              torch.full((4,), p).cuda(),
                              torch.full((4,), 0.5).cuda()).cpu()
        assert ((out >= 0) & (out < V)).all(), out


def test_capturable():
    """No host read: the call records into a graph and replays on new
    inputs."""
    V = 2048
    case = make_case(V, torch.bfloat16, settings_for(V), 1, 4, seed=21)
    logits, temp, k, p, u, oracles = case
    args = [t.cuda() for t in (logits, temp, k, p, u)]
    want = K.sample_tokens(*args)
    static = [torch.zeros_like(t) for t in args]
    static[1].fill_(1.0)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        K.sample_tokens(*static)
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = K.sample_tokens(*static)
    for dst, src in zip(static, args):
        dst.copy_(src)
    g.replay()
    assert torch.equal(out, want)


# ------------------------------------------------------------------ engine
REQUESTS = [
    ([5, 9, 17, 4], 9, 0.9, 0, 1.0, 11),
    (list(range(2, 25)), 7, 1.2, 20, 1.0, 12),
    ([100, 101], 10, 0.7, 0, 0.9, 13),
    ([64, 3, 99, 12, 54, 23], 8, 1.0, 30, 0.8, 14),
    ([7] * 11, 6, 0.0, 0, 1.0, None),
]


@pytest.fixture(scope="module")
def tiny_gpu_model():
    torch.manual_seed(0)
    cfg = LlamaConfig.tiny(vocab=2048, seq=256)
    return LlamaForCausalLM(cfg).to("cuda:0").eval()


def _serve(model, **kw):
    b = ContinuousBatcher(model, **kw)
    reqs = [b.submit(p, n, temperature=T, top_k=k, top_p=tp, seed=s)
            for (p, n, T, k, tp, s) in REQUESTS]
    out = b.run()
    assert all(r.done and len(out[r.id]) == r.max_new for r in reqs)
    return [out[r.id] for r in reqs]


def test_engine_eager_and_graph_agree(tiny_gpu_model):
    # max_len 128 is one decode split under both, so both see the same
    # logits bit for bit
    eager = _serve(tiny_gpu_model, max_batch=3, max_len=128, graph=False)
    graph = _serve(tiny_gpu_model, max_batch=3, max_len=128, graph=True)
    assert eager == graph
    # the greedy request is what generate() decodes
    p, n = REQUESTS[-1][0], REQUESTS[-1][1]
    ref = tiny_gpu_model.generate(torch.tensor([p], device="cuda"),
                                  n)[0, len(p):].tolist()
    assert eager[-1] == ref


def test_engine_sampled_paged_run_completes(tiny_gpu_model):
    out = _serve(tiny_gpu_model, max_batch=3, max_len=128, graph=True,
                 num_pages=6)
    assert all(0 <= t < 2048 for toks in out for t in toks)
