"""Guard on the dK/dV kernel's tile loop, read from its gfx950 assembly.

The loop once carried 32 global K/V fragment loads and 32 cross-lane
ds_bpermute_b32 per iteration under a source comment that claimed the K/V
rows were register-resident: the compiler had quietly put the loads back
inside the loop. This test cross-compiles the attention source (no GPU
needed) and counts what the loop really contains:

* no ds_bpermute_b32: P and dS feed the transposed products from the
  accumulators, reordered in the register file (v_permlane32_swap), not
  through the LDS crossbar;
* no more global_load_dwordx4 than the Q/dO staging issues. stage_panel
  moves 2 tiles x 1024 vec8 slots with 512 threads, 4 loads per thread;
  the compiler emits 5 because it splits one of them over its bounds-guard
  branch (the dq kernel's loop shows the same 5 for its K/V staging). A
  K or V re-fetch would add at least 8.
"""

import re

import pytest

from .kernel_remarks import compile_tu, hipcc

TU = """#include "attention.hip"
template __global__ void attn_bwd_dkdv_v2_kernel<512>(
    const short*, const short*, const short*, const short*, const float*,
    const float*, float*, float*, int, int, int, int, float, int);
"""

STAGING_LOADS = 5


def _loop_instructions(asm):
    """Mnemonics of every block of the kernel's one loop: the block the
    compiler marks "Inner Loop Header" and the blocks it marks
    "in Loop: Header=" (which include the back-branch)."""
    m = re.search(r"^_Z\d+attn_bwd_dkdv_v2_kernel\w*:.*\n", asm, re.M)
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
def test_dkdv_loop_has_no_lane_exchange_and_no_kv_refetch(tmp_path):
    asm, _ = compile_tu(TU, tmp_path, "dkdv_tu")
    ins = _loop_instructions(asm)
    count = lambda name: sum(1 for i in ins if i == name)
    print("loop instructions:", len(ins),
          {n: count(n) for n in ("v_mfma_f32_32x32x16_bf16",
                                 "global_load_dwordx4", "global_load_dword",
                                 "ds_bpermute_b32", "ds_read_b64_tr_b16")})
    # the loop was found and is the real one: 64 MFMAs per q tile
    assert count("v_mfma_f32_32x32x16_bf16") == 64
    assert count("ds_bpermute_b32") == 0
    assert count("global_load_dwordx4") <= STAGING_LOADS
    # nothing else reads global memory in the loop but lse and delta
    others = [i for i in ins if i.startswith(("global_load", "buffer_load",
                                              "flat_load", "scratch_load"))
              and i not in ("global_load_dwordx4", "global_load_dword")]
    assert not others, others
    assert count("global_load_dword") <= 2
