"""append.hip's paged instantiation on the GPU: K.attn_append_paged
against the fp32 reference on the shapes that take each of the kernel's paths, against the
dense append kernel, under hipGraph capture, and the model wiring.

Pool setup as in test_paged_gpu.py: the pool is larger than what the
sequences own, owned pages are handed out in shuffled order, every
unowned page and every row past pos+Sq in a last page is NaN, and table
entries past the last needed page point at an all-NaN page. A wrong read
shows as a NaN or a numerical failure, never as a fault. The check is PER
ROW against fp32 attn_append_ref on rows assembled on the CPU: one
wrongly visible or hidden key at these horizons moves its row by more
than the tolerance (test_attn_append_gpu.py), which a whole-tensor norm
would hide. 2e-2 is the project's kernel tolerance (test_ops_gpu.py).
"""

import math

import pytest
import torch

pytestmark = pytest.mark.gpu

SCALE = 1.0 / math.sqrt(128)
TOL = 2e-2
PAGE = 64

# (B, H, Hkv, Sq, pos, max_len)
SHAPES = [
    # 1-wave kernel, partial last page, one sequence at pos 0
    (2, 4, 2, 5, [300, 0], None),
    # 4-wave kernel; second query tile holds 2 of 128 rows; G = 4; pos
    # differs per sequence; the prefetch crosses page lookups
    (2, 8, 2, 130, [0, 191], None),
    # the new rows fill exactly one page, pos on a page boundary
    (1, 2, 1, 64, [64], None),
    # split count from the capacity: mostly empty or fully masked splits
    (1, 2, 1, 128, [3], 2048),
    # long prefix, several live splits, the merge
    (1, 2, 1, 64, [1000], 2048),
]
# sequence 1 takes no part: exact zeros, its table row is never read (it
# holds out-of-pool indices only)
SKIP_SHAPE = (3, 4, 2, 5, [70, -1, 0], None)
# holes: entry 1 of sequence 0 is -1, entry 1 of sequence 1 is past the
# pool. Keys 64..127 of both are invisible; every row still sees page 0
HOLE_SHAPE = (2, 2, 1, 5, [150, 150], None)


def setup_module():
    from metaflow_amd.ops import kernels as K

    assert K.extension_loaded(), "_mfx_hip must be built for GPU tests"


@pytest.fixture
def dev():
    return torch.device("cuda:0")


def _paged_case(B, H, Hkv, Sq, pos, max_len, seed, num_pages=None):
    """CPU tensors: q, NaN-backed pools, the table (one spare column, so
    every row has an entry past its last needed page), and each
    participating sequence's contiguous rows [Hkv, pos+Sq, 128]."""
    g = torch.Generator().manual_seed(seed)
    cap = max_len if max_len is not None else max(pos) + Sq
    pps = -(-cap // PAGE) + 1
    owned = sum(-(-(p + Sq) // PAGE) for p in pos if p >= 0)
    if num_pages is None:
        num_pages = owned + 4
    assert num_pages > owned
    perm = torch.randperm(num_pages, generator=g).tolist()
    nan_page = perm.pop()
    q = torch.randn(B, H, Sq, 128, generator=g).to(torch.bfloat16)
    kp = torch.full((num_pages, Hkv, PAGE, 128), float("nan"),
                    dtype=torch.bfloat16)
    vp = torch.full_like(kp, float("nan"))
    table = torch.full((B, pps), nan_page, dtype=torch.int32)
    rows = []
    for b, p in enumerate(pos):
        if p < 0:
            rows.append(None)
            continue
        n = p + Sq
        k = torch.randn(Hkv, n, 128, generator=g).to(torch.bfloat16)
        v = torch.randn(Hkv, n, 128, generator=g).to(torch.bfloat16)
        rows.append((k, v))
        for j in range(-(-n // PAGE)):
            page = perm.pop()
            table[b, j] = page
            m = min(PAGE, n - j * PAGE)
            kp[page, :, :m] = k[:, j * PAGE:j * PAGE + m]
            vp[page, :, :m] = v[:, j * PAGE:j * PAGE + m]
    return q, kp, vp, table, rows


def _reference(q, rows, pos, hidden=()):
    """fp32 attn_append_ref per participating sequence -> {b: [H,Sq,128]}.
    ``hidden`` is a key range no row sees (a hole in the table). It must
    end at or before pos: then every query row would have seen all of it,
    and dropping those rows from the cache (with pos moved down by as
    many) is the same attention."""
    from metaflow_amd.ops import kernels as K

    refs = {}
    for b, p in enumerate(pos):
        if p < 0:
            continue
        k, v = rows[b]
        if hidden:
            lo, hi = hidden
            assert hi <= p
            keep = torch.cat([torch.arange(0, lo), torch.arange(hi, k.size(1))])
            k, v, p = k[:, keep], v[:, keep], p - (hi - lo)
        ref = K.attn_append_ref(q[b:b + 1].float(), k[None].float(),
                                v[None].float(), p, SCALE)[0]
        assert not torch.isnan(ref).any()
        refs[b] = ref
    return refs


def _check_rows(o, refs, what):
    """Per-row relative error of o [B,H,Sq,128] (fp32, CPU) on the
    sequences of ``refs``; prints and returns the worst row."""
    worst, where = 0.0, None
    for b, ref in refs.items():
        assert not torch.isnan(o[b]).any(), "read an unowned row"
        err = (o[b] - ref).norm(dim=-1) / ref.norm(dim=-1)     # [H, Sq]
        if err.max().item() >= worst:
            worst = err.max().item()
            where = (b,) + tuple((err == err.max()).nonzero()[0].tolist())
    print("%s worst per-row rel err %.3e at (b,h,i)=%s" % (what, worst,
                                                           where))
    return worst


@pytest.mark.parametrize("B,H,Hkv,Sq,pos,max_len", SHAPES)
def test_attn_append_paged_matches_reference(dev, B, H, Hkv, Sq, pos,
                                             max_len):
    from metaflow_amd.ops import kernels as K

    q, kp, vp, table, rows = _paged_case(B, H, Hkv, Sq, pos, max_len,
                                         seed=Sq)
    refs = _reference(q, rows, pos)
    pos_t = torch.tensor(pos, dtype=torch.int32, device=dev)
    o = K.attn_append_paged(q.to(dev), kp.to(dev), vp.to(dev),
                            table.to(dev), pos_t, SCALE, max_len=max_len)
    torch.cuda.synchronize()
    assert o.shape == q.shape and o.dtype == torch.bfloat16
    worst = _check_rows(o.float().cpu(), refs, "paged append %s" % (pos,))
    assert worst < TOL


def test_sequence_that_takes_no_part_is_zero(dev):
    from metaflow_amd.ops import kernels as K

    B, H, Hkv, Sq, pos, max_len = SKIP_SHAPE
    q, kp, vp, table, rows = _paged_case(B, H, Hkv, Sq, pos, max_len, seed=2)
    table[1] = kp.size(0) + 5
    refs = _reference(q, rows, pos)
    # a list pos and a computed max_len; then the split path (a capacity
    # of 1024 rows gives 4 splits here), where the merge writes the zeros
    wide = torch.full((B, 16), int(table[0, -1]), dtype=torch.int32)
    wide[:, :table.size(1)] = table
    wide[1] = kp.size(0) + 5
    for tbl, ml in ((table, None), (wide, 1024)):
        o = K.attn_append_paged(q.to(dev), kp.to(dev), vp.to(dev),
                                tbl.to(dev), pos, SCALE, max_len=ml)
        torch.cuda.synchronize()
        o = o.float().cpu()
        assert bool((o[1] == 0).all()), "pos < 0 must give exact zeros"
        assert _check_rows(o, refs, "pos -1, max_len %s" % ml) < TOL


def test_table_holes_contribute_no_key(dev):
    from metaflow_amd.ops import kernels as K

    B, H, Hkv, Sq, pos, max_len = HOLE_SHAPE
    q, kp, vp, table, rows = _paged_case(B, H, Hkv, Sq, pos, max_len, seed=3)
    table[0, 1] = -1
    table[1, 1] = kp.size(0) + 3
    refs = _reference(q, rows, pos, hidden=(PAGE, 2 * PAGE))
    o = K.attn_append_paged(q.to(dev), kp.to(dev), vp.to(dev),
                            table.to(dev), pos, SCALE)
    torch.cuda.synchronize()
    assert _check_rows(o.float().cpu(), refs, "holes") < TOL


def test_only_holes_gives_zeros_not_nan(dev):
    """A sequence whose every needed entry is a hole sees no key at all:
    zeros (the guard on 1 / l), no NaN."""
    from metaflow_amd.ops import kernels as K

    q, kp, vp, table, _rows = _paged_case(1, 2, 1, 5, [70], None, seed=4)
    table[:] = -1
    o = K.attn_append_paged(q.to(dev), kp.to(dev), vp.to(dev),
                            table.to(dev), [70], SCALE)
    torch.cuda.synchronize()
    assert bool((o.float().cpu() == 0).all())


@pytest.mark.parametrize("B,H,Hkv,Sq,pos,max_len", SHAPES)
def test_attn_append_paged_matches_dense_kernel(dev, B, H, Hkv, Sq, pos,
                                                max_len):
    """The dense append kernel on the same rows, contiguous, with the
    same capacity and max_len: same tile order and split rule. Gated at
    the kernel tolerance; bit equality is printed, not asserted (the
    compiler may contract the two kernels differently)."""
    from metaflow_amd.ops import kernels as K

    q, kp, vp, table, rows = _paged_case(B, H, Hkv, Sq, pos, max_len,
                                         seed=Sq)
    Lmax = table.size(1) * PAGE
    kc = torch.full((B, Hkv, Lmax, 128), float("nan"), dtype=torch.bfloat16)
    vc = torch.full_like(kc, float("nan"))
    for b, (k, v) in enumerate(rows):
        kc[b, :, :k.size(1)] = k
        vc[b, :, :v.size(1)] = v
    pos_t = torch.tensor(pos, dtype=torch.int32, device=dev)
    ml = max_len if max_len is not None else max(pos) + Sq
    gq = q.to(dev)
    o_p = K.attn_append_paged(gq, kp.to(dev), vp.to(dev), table.to(dev),
                              pos_t, SCALE, max_len=ml)
    o_d = K.attn_append(gq, kc.to(dev), vc.to(dev), pos_t, SCALE,
                        max_len=ml)
    torch.cuda.synchronize()
    print("paged vs dense %s bit-equal: %s" % (pos, torch.equal(o_p, o_d)))
    o_p, o_d = o_p.float().cpu(), o_d.float().cpu()
    assert not torch.isnan(o_p).any() and not torch.isnan(o_d).any()
    err = ((o_p - o_d).norm(dim=-1) / o_d.norm(dim=-1)).max().item()
    print("paged vs dense %s worst per-row rel diff %.3e" % (pos, err))
    assert err < TOL


def test_attn_append_paged_is_capturable(dev):
    """One captured call, pos on the device and max_len the capacity;
    pos, the table and the pool then change in place, and the replay
    equals an eager call on the new contents."""
    from metaflow_amd.ops import kernels as K

    B, H, Hkv, Sq, cap = 2, 4, 2, 5, 1024          # 4 splits + the merge
    first = _paged_case(B, H, Hkv, Sq, [300, 0], cap, seed=8, num_pages=24)
    second = _paged_case(B, H, Hkv, Sq, [10, 500], cap, seed=9,
                         num_pages=24)
    q, kp, vp, table = (t.to(dev) for t in first[:4])
    pos_t = torch.tensor([300, 0], dtype=torch.int32, device=dev)
    o_first = K.attn_append_paged(q, kp, vp, table, pos_t, SCALE,
                                  max_len=cap)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        o_g = K.attn_append_paged(q, kp, vp, table, pos_t, SCALE,
                                  max_len=cap)
    q.copy_(second[0])
    kp.copy_(second[1])
    vp.copy_(second[2])
    table.copy_(second[3])
    pos_t.copy_(torch.tensor([10, 500], dtype=torch.int32))
    graph.replay()
    torch.cuda.synchronize()
    o_e = K.attn_append_paged(q, kp, vp, table, pos_t, SCALE, max_len=cap)
    torch.cuda.synchronize()
    assert not torch.isnan(o_g.float()).any()
    assert not torch.equal(o_g, o_first)        # the replay saw the change
    assert torch.equal(o_g, o_e)
    refs = _reference(second[0], second[4], [10, 500])
    assert _check_rows(o_g.float().cpu(), refs, "graph replay") < TOL


def _rel_err(a, b):
    a, b = a.float(), b.float()
    return ((a - b).norm() / (b.norm() + 1e-8)).item()


def _wiring(model, cfg, dev, monkeypatch):
    from metaflow_amd.models.llama import PagedKVCache, PagedSlotView
    from metaflow_amd.ops import kernels as K

    calls = []
    real = K.attn_append_paged

    def counted(*a, **kw):
        calls.append(a[0].shape)
        return real(*a, **kw)

    monkeypatch.setattr(K, "attn_append_paged", counted)
    g = torch.Generator().manual_seed(0)
    tokens = torch.randint(0, cfg.vocab_size, (1, 47), generator=g).to(dev)
    with torch.no_grad():
        full = model(tokens)
        paged = PagedKVCache(cfg, 4, 2, 128, dev)
        assert paged.reserve(2)
        paged.ensure(0, 1)          # slot 1's page is not pool page 0
        paged.ensure(1, 47)
        paged.sync()
        for li in range(cfg.num_layers):
            paged.k_pages[li].fill_(float("nan"))
            paged.v_pages[li].fill_(float("nan"))
        view = PagedSlotView(paged, 1)
        model(tokens[:, :40], cache=view)
        assert calls == []          # prefill at pos 0 is the flash kernel
        block = model(tokens[:, 40:], cache=view)
    torch.cuda.synchronize()
    assert len(calls) == cfg.num_layers
    assert all(s[2] == 7 for s in calls)
    assert view.pos == 47
    assert not torch.isnan(block.float()).any()
    assert full[:, 40:47].float().abs().max() > 0     # not a 0 == 0 match
    err = _rel_err(block, full[:, 40:47])
    print("paged block vs uncached logits rel err %.3e" % err)
    assert err < TOL


def test_llama_paged_block_uses_paged_append_kernel(dev, monkeypatch):
    from metaflow_amd.models.llama import LlamaConfig, LlamaForCausalLM

    torch.manual_seed(0)
    cfg = LlamaConfig.tiny(vocab=128, seq=256)
    model = LlamaForCausalLM(cfg).to(dev).eval()
    _wiring(model, cfg, dev, monkeypatch)


def test_mixtral_paged_block_uses_paged_append_kernel(dev, monkeypatch):
    from metaflow_amd.models.mixtral import (MixtralConfig,
                                             MixtralForCausalLM)

    torch.manual_seed(0)
    cfg = MixtralConfig.tiny(vocab=128, seq=256)
    model = MixtralForCausalLM(cfg).to(dev).eval()
    _wiring(model, cfg, dev, monkeypatch)
