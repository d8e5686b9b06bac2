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

import os
import re
import shutil
import subprocess

import pytest

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                    "metaflow_amd", "ops", "csrc")

TU = """#include "attention.hip"
template __global__ void attn_bwd_dkdv_v2_kernel<512>(
    const short*, const short*, const short*, const short*, const float*,
    const float*, float*, float*, int, int, int, int, float, int);
"""

STAGING_LOADS = 5


def _hipcc():
    return shutil.which("hipcc") or (
        "/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc")
        else None)


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


@pytest.mark.skipif(_hipcc() is None, reason="hipcc not installed")
def test_dkdv_loop_has_no_lane_exchange_and_no_kv_refetch(tmp_path):
    src = tmp_path / "dkdv_tu.hip"
    src.write_text(TU)
    out = tmp_path / "dkdv_tu.s"
    proc = subprocess.run(
        [_hipcc(), "--offload-arch=gfx950", "--cuda-device-only", "-O3",
         "-std=c++17", "-S", "-I", CSRC, str(src), "-o", str(out)],
        capture_output=True, text=True)
    assert proc.returncode == 0, proc.stderr[-2000:]
    ins = _loop_instructions(out.read_text())
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
