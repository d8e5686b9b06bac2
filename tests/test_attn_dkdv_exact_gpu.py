"""Exact-integer check of the dK/dV backward kernel.

The kernel feeds the P and dS accumulators to the next MFMA as B operands
after a half exchange between the lane halves that puts their rows in
natural k order; the transposed reads of dO and Q must supply the same
rows in the same k slots, and a mismatch corrupts almost every element.
With crafted inputs the whole backward is an exact integer expression, so
the comparison is torch.equal, not a tolerance:

  k = 0, lse = 0, o = 0  ->  S = 0, delta = 0, P = 1 wherever unmasked
  scale = 0.125, q / v / dout sparse with entries in {-1, 0, 1}

  dV[kv] = sum_h sum_{q visible} dO[h, q]
  dK[kv] = 0.125 * sum_h sum_{q visible} (dO[h, q] . V[kv]) * Q[h, q]
  dQ     = 0

The test asserts, before it calls the kernel, that every dP entry is below
256 in magnitude (so dS = dP / 8 is exact in bf16) and that every expected
output is exactly representable in bf16.
"""

import pytest
import torch

pytestmark = pytest.mark.gpu

SCALE = 0.125
DENSITY = 0.1
SHAPES = [(1, 4, 2, 256), (2, 8, 2, 512)]


def _sparse(gen, *shape):
    keep = torch.rand(*shape, generator=gen) < DENSITY
    sign = torch.randint(0, 2, shape, generator=gen) * 2 - 1
    return (keep * sign).to(torch.float64)


def _bf16_exact(x):
    return torch.equal(x.to(torch.bfloat16).to(torch.float64), x)


def _expected(q, v, dout, Hkv, causal):
    """(dk, dv) in fp64 from integer-valued fp64 q, v, dout; every
    intermediate is an integer far below 2^53, so fp64 is exact."""
    B, H, S, D = q.shape
    G = H // Hkv
    vis = torch.ones(S, S, dtype=torch.float64)     # [q, kv]
    if causal:
        vis = vis.tril()
    vexp = v.repeat_interleave(G, dim=1)
    dp = torch.matmul(dout, vexp.transpose(-1, -2)) * vis   # [B,H,q,kv]
    assert dp.abs().max().item() < 256
    dv = torch.matmul(vis.t().expand(B, H, S, S), dout)
    dk = torch.matmul(dp.transpose(-1, -2), q) * SCALE
    dv = dv.view(B, Hkv, G, S, D).sum(2)
    dk = dk.view(B, Hkv, G, S, D).sum(2)
    return dk, dv


@pytest.mark.parametrize("causal", [True, False])
@pytest.mark.parametrize("shape", SHAPES)
def test_dkdv_exact(shape, causal):
    from metaflow_amd.ops.kernels import hip_ext

    B, H, Hkv, S = shape
    gen = torch.Generator().manual_seed(7 + S)
    q = _sparse(gen, B, H, S, 128)
    v = _sparse(gen, B, Hkv, S, 128)
    dout = _sparse(gen, B, H, S, 128)
    dk_exp, dv_exp = _expected(q, v, dout, Hkv, causal)
    assert _bf16_exact(dk_exp) and _bf16_exact(dv_exp)
    assert dk_exp.abs().max().item() > 0 and dv_exp.abs().max().item() > 0

    dev = torch.device("cuda:0")
    bf = lambda t: t.to(torch.bfloat16).to(dev)
    qd, vd, dd = bf(q), bf(v), bf(dout)
    kd = torch.zeros_like(vd)
    od = torch.zeros_like(qd)
    lse = torch.zeros(B, H, S, dtype=torch.float32, device=dev)
    dq, dk, dv = hip_ext().attn_bwd(qd, kd, vd, od, dd, lse, SCALE, causal)
    assert torch.equal(dv.cpu(), dv_exp.to(torch.bfloat16)), "dV"
    assert torch.equal(dk.cpu(), dk_exp.to(torch.bfloat16)), "dK"
    assert torch.equal(dq.cpu(), torch.zeros_like(od).cpu()), "dQ"
