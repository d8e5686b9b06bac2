"""fp64 numpy oracle of the sampler's semantics, shared by the CPU and the
GPU sampling tests. It shares no code with the product: kept set by a
sort, weights and CDF in float64."""

import numpy as np
import torch

GAP_MIN = 1e-4
EPS_FACTOR = 16.0


class RowOracle(object):
    """Kept mask and each token's half-open interval [lo, hi) of the
    renormalised kept CDF in index order, for one row; ``gap`` is the
    distance from top_p to the nearer of M(j*) and M(j* - 1) (None
    where top-p is off)."""

    def __init__(self, x, T, k, p):
        x = np.asarray(x, dtype=np.float64)
        V = x.shape[0]
        keep = x > -np.inf
        if 0 < k < V:
            kth = np.sort(x)[V - k]
            keep &= x >= kth
        w = np.where(keep, np.exp((x - x.max()) / T), 0.0)
        self.gap = None
        if p < 1:
            vals, inv = np.unique(x[keep], return_inverse=True)
            mass = np.bincount(inv, weights=w[keep], minlength=len(vals))
            vals = vals[::-1]                          # descending
            share = np.cumsum(mass[::-1]) / mass.sum()
            j = int(np.nonzero(share >= p)[0][0])
            below = share[j - 1] if j > 0 else 0.0
            self.gap = min(share[j] - p, p - below)
            keep &= x >= vals[j]
            w = np.where(keep, w, 0.0)
        c = np.cumsum(w)
        self.keep = keep
        self.hi = c / c[-1]
        self.lo = (c - w) / c[-1]


def pick_top_p(x, T, k, p):
    """A top_p at or just below ``p`` whose oracle gap on row x is at
    least GAP_MIN, and that row's oracle."""
    for step in range(50):
        q = float(np.float32(p - 2e-4 * step))
        o = RowOracle(x, T, k, q)
        if q >= 1 or o.gap >= GAP_MIN:
            return q, o
    raise AssertionError("no top_p with a gap >= %g near %g" % (GAP_MIN, p))


def row64(logits_row):
    """One row of a bf16 / fp32 tensor as float64 numpy (exact)."""
    return logits_row.detach().cpu().double().numpy()


def delta_ref(logits, temperature, top_k, top_p, oracles):
    """Largest shift of sample_tokens_ref's fp32 CDF boundaries from the
    oracle's, over the sampled rows (computed on the CPU). ``oracles``:
    one RowOracle (or None for a greedy row) per row."""
    from metaflow_amd.ops import kernels as K

    keep, csum, total = K.sample_dist_ref(
        logits.detach().cpu(), temperature.cpu(), top_k.cpu(), top_p.cpu())
    keep = keep.numpy()
    with np.errstate(invalid="ignore"):        # greedy rows: 0 / 0, unused
        cdf = csum.double().numpy() / total.double().numpy()[:, None]
    worst = 0.0
    done = {}
    for b, o in enumerate(oracles):
        if o is None:
            continue
        assert (keep[b] == o.keep).all(), \
            "row %d: the reference's kept set differs from the oracle's" % b
        if id(o) in done:       # repeated rows share their oracle
            continue
        done[id(o)] = True
        worst = max(worst, float(np.abs(cdf[b] - o.hi)[o.keep].max()))
    return worst


def assert_draws(tokens, u, oracles, eps, greedy=None):
    """Every returned token is kept and owns u to within eps; greedy rows
    (oracle None) equal ``greedy[b]``."""
    tokens = tokens.detach().cpu().tolist()
    u = u.detach().cpu().double().tolist()
    worst = 0.0
    for b, o in enumerate(oracles):
        t = tokens[b]
        if o is None:
            assert t == int(greedy[b]), (b, t, int(greedy[b]))
            continue
        assert 0 <= t < o.keep.shape[0], (b, t)
        assert o.keep[t], "row %d: token %d is not in the kept set" % (b, t)
        miss = max(o.lo[t] - u[b], u[b] - o.hi[t], 0.0)
        worst = max(worst, miss)
        assert miss <= eps, (
            "row %d: u=%.9g outside [%.9g, %.9g) of token %d by %.3g "
            "(eps %.3g)" % (b, u[b], o.lo[t], o.hi[t], t, miss, eps))
    return worst


def random_row(V, dtype, gen):
    """randn * 3 rounded to bf16. An fp32 row keeps those ties (with as
    many distinct values as an fp32 row of randn has, no top_p has a gap
    of GAP_MIN: every step of M is smaller) but is scaled by 1 + 2^-17,
    which fills the low mantissa bits and preserves order and ties."""
    x = (torch.randn(V, generator=gen) * 3).to(torch.bfloat16)
    if dtype == torch.float32:
        x = x.float() * (1.0 + 2.0 ** -17)
    return x.to(dtype)


def u_values(n, gen):
    """n uniforms in [0, 1); from n = 3 they include 0 and the largest
    fp32 below 1."""
    u = torch.rand(n, generator=gen, dtype=torch.float32)
    if n >= 3:
        u[0] = 0.0
        u[1] = float(np.nextafter(np.float32(1), np.float32(0)))
    return u


def make_case(V, dtype, settings, rows_per_setting, n_u, seed,
              strided=False):
    """A batch: for each (T, k, p) of ``settings`` (T <= 0: greedy),
    ``rows_per_setting`` random rows (randn * 3), each repeated for n_u
    values of u. strided=True places the rows at [:, -1] of a [B, 3, V]
    tensor. Returns (logits [B, V], temperature, top_k, top_p, u,
    oracles)."""
    g = torch.Generator()
    g.manual_seed(seed)
    rows, temps, ks, ps, us, oracles = [], [], [], [], [], []
    for (T, k, p) in settings:
        for _ in range(rows_per_setting):
            x = random_row(V, dtype, g)
            q, o = p, None
            if T > 0:
                q, o = pick_top_p(row64(x), T, k, p)
                assert o.gap is None or o.gap >= GAP_MIN, o.gap
            for uu in u_values(n_u, g).tolist():
                rows.append(x)
                temps.append(T)
                ks.append(k)
                ps.append(q)
                us.append(uu)
                oracles.append(o)
    logits = torch.stack(rows)
    if strided:
        full = (torch.randn(len(rows), 3, V, generator=g) * 3).to(dtype)
        full[:, -1] = logits
        logits = full[:, -1]
    return (logits, torch.tensor(temps, dtype=torch.float32),
            torch.tensor(ks, dtype=torch.int32),
            torch.tensor(ps, dtype=torch.float32),
            torch.tensor(us, dtype=torch.float32), oracles)


def settings_for(V):
    """The issue's four (T, k, p) settings; the smaller k where V is 5."""
    small = V <= 50
    return [(1.0, 0, 1.0), (0.7, 3 if small else 50, 1.0),
            (1.3, 0, 0.9), (0.8, 3 if small else 40, 0.8)]
