"""Bit-identity of the attention train kernels against recorded outputs.

The forward, dQ and dK/dV kernels are changed only in ways that move data
or control flow (LDS layouts, which tiles evaluate the causal mask), never
in ways that reorder or re-round a sum, so O, lse, dQ, dK and dV must stay
bit-for-bit what they were. tests/golden/attn_train_bits.json holds the
SHA-256 of each output and of the CPU-generated inputs, recorded on an
MI355X from the commit BEFORE the LDS-image change by
tools/record_attn_train_bits.py.

Cases:
* b1h4g2s512: causal, two q blocks, so every wave sees unmasked tiles,
  diagonal tiles and skipped tiles;
* b1h4g4s768: causal, three q / kv blocks, one kv head;
* b2h8g4s512_noncausal: the ring-attention chunk op, no mask at all;
* b1h4g2s257 / b1h4g2s100: padded lengths through K.attention.

A differing INPUT hash fails the test (the generator changed: re-record on
the parent commit). A differing OUTPUT hash is the failure this test
exists for.
"""

import hashlib
import json
import math
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden",
                      "attn_train_bits.json")

# case id -> (B, H, Hkv, S, causal, path)
CASES = {
    "b1h4g2s512": (1, 4, 2, 512, True, "raw"),
    "b1h4g4s768": (1, 4, 1, 768, True, "raw"),
    "b2h8g4s512_noncausal": (2, 8, 2, 512, False, "raw"),
    "b1h4g2s257": (1, 4, 2, 257, True, "autograd"),
    "b1h4g2s100": (1, 4, 2, 100, True, "autograd"),
}


def sha(t):
    t = t.detach().cpu().contiguous()
    return hashlib.sha256(t.view(torch.uint8).numpy().tobytes()).hexdigest()


def inputs(case):
    """Seeded CPU inputs: the same bits on every machine."""
    B, H, Hkv, S, _, _ = CASES[case]
    gen = torch.Generator().manual_seed(4321 + sorted(CASES).index(case))
    mk = lambda h: torch.randn(B, h, S, 128, generator=gen).to(torch.bfloat16)
    return {"q": mk(H), "k": mk(Hkv), "v": mk(Hkv), "dout": mk(H)}


def outputs(case):
    """O, lse, dQ, dK, dV of the train kernels on the case's inputs."""
    from metaflow_amd.ops import kernels as K

    causal, path = CASES[case][4:]
    scale = 1.0 / math.sqrt(128)
    q, k, v, dout = [t.cuda() for t in inputs(case).values()]
    o, lse = K.attn_fwd_raw(q, k, v, scale, causal=causal)
    if path == "autograd":
        qg, kg, vg = [t.clone().requires_grad_(True) for t in (q, k, v)]
        oa = K.attention(qg, kg, vg, scale, causal)
        oa.backward(dout)
        assert torch.equal(oa, o)
        dq, dk, dv = qg.grad, kg.grad, vg.grad
    else:
        dq, dk, dv = K.attn_bwd_raw(q, k, v, o, dout, lse, scale,
                                    causal=causal)
    torch.cuda.synchronize()
    return {"o": o, "lse": lse, "dq": dq, "dk": dk, "dv": dv}


def record():
    """{case: {"inputs": {name: sha}, "outputs": {name: sha}}}"""
    return {case: {"inputs": {n: sha(t) for n, t in inputs(case).items()},
                   "outputs": {n: sha(t) for n, t in outputs(case).items()}}
            for case in sorted(CASES)}


def setup_module():
    from metaflow_amd.ops import kernels as K

    assert K.extension_loaded(), "_mfx_hip must be built+loadable on GPU"


@pytest.mark.parametrize("case", sorted(CASES))
def test_attn_train_bits(case):
    with open(GOLDEN) as f:
        golden = json.load(f)[case]
    got_in = {n: sha(t) for n, t in inputs(case).items()}
    assert got_in == golden["inputs"], (
        "the seeded CPU inputs differ from the recorded ones: re-record "
        "with tools/record_attn_train_bits.py on the commit before the "
        "LDS-image change")
    got = {n: sha(t) for n, t in outputs(case).items()}
    bad = sorted(n for n in got if got[n] != golden["outputs"][n])
    assert not bad, "outputs no longer bit-identical: %s" % bad
