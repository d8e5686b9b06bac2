"""Guard on the forward and dQ kernels' tile loops, read from their gfx950
assembly.

Both loops once moved P / dS between lanes through the LDS crossbar (34
ds_bpermute_b32 per tile in the forward, 16 in dQ) to build A operands.
They now feed the accumulators to the transposed second product as B
operands, reordered in the register file (v_permlane32_swap). This test
cross-compiles the attention source (no GPU needed) and counts what each
loop really contains:

* the MFMAs of one kv tile: 32 in the forward (16 for S^T, 16 for O^T),
  48 in dQ (16 each for S^T, dP^T and dQ^T), which also shows that the
  loop found is the real one;
* no ds_bpermute_b32;
* no more global_load_dwordx4 than the K/V staging issues: 2 tiles x 1024
  vec8 slots over 512 threads are 4 loads per thread (the forward's open
  coded staging emits exactly 4, stage_panel in dQ 5, because the compiler
  splits one over its bounds-guard branch), and no other load from global
  or scratch memory at all: Q, dO, lse and delta stay in registers.
"""

import re

import pytest

from .kernel_remarks import compile_tu, hipcc

TU = """#include "attention.hip"
template __global__ void attn_fwd_v2_kernel<512>(
    const short*, const short*, const short*, short*, float*, int, int, int,
    int, float, int);
template __global__ void attn_bwd_dq_v2_kernel<512>(
    const short*, const short*, const short*, const short*, const float*,
    const float*, short*, int, int, int, int, float, int);
"""

# kernel -> (MFMAs per tile, staging global_load_dwordx4 allowed)
LOOPS = {
    "attn_fwd_v2_kernel": (32, 4),
    "attn_bwd_dq_v2_kernel": (48, 5),
}

_asm = {}


def _assembly(tmp_path_factory):
    """The translation unit's assembly, compiled once for both cases."""
    if "s" not in _asm:
        tmp = tmp_path_factory.mktemp("fwd_dq_asm")
        _asm["s"], _ = compile_tu(TU, tmp, "fwd_dq_tu")
    return _asm["s"]


def _loop_instructions(asm, kernel):
    """Mnemonics of every block of the kernel's one loop: the block the
    compiler marks "Inner Loop Header" and the blocks it marks
    "in Loop: Header=" (which include the back-branch)."""
    m = re.search(r"^_Z\d+%s\w*:.*\n" % kernel, asm, re.M)
    assert m, "kernel not found in the assembly"
    body = asm[m.end():asm.index(".Lfunc_end", m.end())]
    ins, in_loop, headers = [], False, 0
    for line in body.split("\n"):
        if re.match(r"(\.LBB\d+_\d+:|; %bb\.\d+:)", line):
            in_loop = "Loop" in line
            headers += "Inner Loop Header" in line
        elif in_loop and line.startswith("\t"):
            word = line.split()[0]
            if not word.startswith((";", ".")):
                ins.append(word)
    assert headers == 1, "expected exactly one loop, found %d" % headers
    return ins


@pytest.mark.skipif(hipcc() is None, reason="hipcc not installed")
@pytest.mark.parametrize("kernel", sorted(LOOPS))
def test_loop_has_no_lane_exchange_and_no_refetch(kernel, tmp_path_factory):
    mfmas, staging_loads = LOOPS[kernel]
    ins = _loop_instructions(_assembly(tmp_path_factory), kernel)
    count = lambda name: sum(1 for i in ins if i == name)
    print(kernel, "loop instructions:", len(ins),
          {n: count(n) for n in ("v_mfma_f32_32x32x16_bf16",
                                 "global_load_dwordx4", "ds_bpermute_b32",
                                 "ds_read_b64_tr_b16")})
    assert count("v_mfma_f32_32x32x16_bf16") == mfmas
    assert count("ds_bpermute_b32") == 0
    assert count("global_load_dwordx4") <= staging_loads
    others = [i for i in ins if i.startswith(("global_load", "buffer_load",
                                              "flat_load", "scratch_load"))
              and i != "global_load_dwordx4"]
    assert not others, others
