"""CPU path of K.attn_append: the fp32 reference, int / per-sequence
offsets, and independence from cache rows past the visible range."""

import torch

from metaflow_amd.ops import kernels as K

SCALE = 0.0883


def _inputs(B=2, H=4, Hkv=2, Sq=5, Lmax=24, seed=0):
    g = torch.Generator().manual_seed(seed)
    q = torch.randn(B, H, Sq, 128, generator=g).to(torch.bfloat16)
    kc = torch.randn(B, Hkv, Lmax, 128, generator=g).to(torch.bfloat16)
    vc = torch.randn(B, Hkv, Lmax, 128, generator=g).to(torch.bfloat16)
    return q, kc, vc


def test_int_pos_is_bit_identical_to_attn_with_cache():
    q, kc, vc = _inputs()
    pos, S = 9, q.size(2)
    o = K.attn_append(q, kc, vc, pos, SCALE)
    ref = K.attn_append_ref(q, kc[:, :, :pos + S], vc[:, :, :pos + S], pos,
                            SCALE)
    assert o.dtype == torch.bfloat16 and o.shape == q.shape
    assert torch.equal(o, ref)


def test_pos_list_equals_per_sequence_loop():
    q, kc, vc = _inputs()
    S = q.size(2)
    pos = [0, 7]
    o = K.attn_append(q, kc, vc, pos, SCALE)
    for b, p in enumerate(pos):
        ref = K.attn_append_ref(q[b:b + 1], kc[b:b + 1, :, :p + S],
                                vc[b:b + 1, :, :p + S], p, SCALE)
        assert torch.equal(o[b:b + 1], ref)
    # a tensor of offsets is the same call
    assert torch.equal(
        K.attn_append(q, kc, vc, torch.tensor(pos, dtype=torch.int32),
                      SCALE), o)


def test_pos_zero_is_causal_attention():
    q, kc, vc = _inputs()
    S = q.size(2)
    o = K.attn_append(q, kc, vc, 0, SCALE)
    ref = K.attention_ref(q, kc[:, :, :S], vc[:, :, :S], SCALE, causal=True)
    # the same fp32 operations in the same order: no tolerance needed
    assert torch.equal(o, ref)


def test_nan_past_visible_range_is_ignored():
    q, kc, vc = _inputs()
    S = q.size(2)
    for pos in (6, [3, 11]):
        o = K.attn_append(q, kc, vc, pos, SCALE)
        kn, vn = kc.clone(), vc.clone()
        ends = [pos + S] * 2 if isinstance(pos, int) else [p + S for p in pos]
        for b, e in enumerate(ends):
            kn[b, :, e:] = float("nan")
            vn[b, :, e:] = float("nan")
        on = K.attn_append(q, kn, vn, pos, SCALE)
        assert not torch.isnan(on.float()).any()
        assert torch.equal(on, o)
