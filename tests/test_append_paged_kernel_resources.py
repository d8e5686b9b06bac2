"""Register / LDS budget guard for the paged append attention kernel.

Same method as test_append_kernel_resources.py: cross-compile a
translation unit that instantiates both block sizes of
attn_append_paged_kernel for gfx950 (no GPU needed) and read the
compiler's resource remarks. The kernel is the dense append kernel's loop
plus a block-table lookup per tile; the page base must stay in scalar
registers and cost no vector register, because the dense loop already
sits at the limit of two waves per SIMD. A spill, or a drop to one wave
per SIMD, is a large silent slowdown.
"""

import os
import re
import shutil
import subprocess

import pytest

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                    "metaflow_amd", "ops", "csrc")

# the include order of mfx_hip.hip: append_paged.hip builds on
# attention.hip's helpers, append.hip's staging and paged.hip's constants
TU = """#include "attention.hip"
#include "append.hip"
#include "paged.hip"
#include "append_paged.hip"
template __global__ void attn_append_paged_kernel<1>(
    const short*, const short*, const short*, const int*, const int*,
    short*, float*, float*, int, int, int, int, int, int, int, float);
template __global__ void attn_append_paged_kernel<4>(
    const short*, const short*, const short*, const int*, const int*,
    short*, float*, float*, int, int, int, int, int, int, int, float);
"""

# mangled-name fragment of each instantiation (template argument Li<NW>E)
KERNELS = {
    "attn_append_paged_kernelILi1E": "1 wave, 32 query rows",
    "attn_append_paged_kernelILi4E": "4 waves, 128 query rows",
}
# declared __shared__ arrays: one K and one V panel tile, [64][128] bf16
LDS_BYTES = 2 * 64 * 128 * 2
# regression guard, not a target: what the build reports for both
OCCUPANCY = 2


def _hipcc():
    return shutil.which("hipcc") or (
        "/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc")
        else None)


@pytest.mark.skipif(_hipcc() is None, reason="hipcc not installed")
def test_append_paged_kernel_resources(tmp_path):
    src = tmp_path / "append_paged_tu.hip"
    src.write_text(TU)
    proc = subprocess.run(
        [_hipcc(), "--offload-arch=gfx950", "--cuda-device-only", "-O3",
         "-std=c++17", "-S", "-Rpass-analysis=kernel-resource-usage",
         "-I", CSRC, str(src), "-o", str(tmp_path / "append_paged_tu.s")],
        capture_output=True, text=True)
    assert proc.returncode == 0, proc.stderr[-2000:]

    # remarks come as one block per kernel, headed by "Function Name:"
    usage = {}
    cur = None
    for line in proc.stderr.splitlines():
        m = re.search(r"remark: (?:Function Name: (\S+)|\s*([^:]+): (\d+))",
                      line)
        if not m:
            continue
        if m.group(1):
            cur = usage.setdefault(m.group(1), {})
        elif cur is not None:
            cur[m.group(2).strip()] = int(m.group(3))

    for frag in KERNELS:
        names = [n for n in usage if frag in n]
        assert len(names) == 1, (frag, sorted(usage))
        u = usage[names[0]]
        print(frag, u)
        assert u["SGPRs Spill"] == 0, (frag, u)
        assert u["VGPRs Spill"] == 0, (frag, u)
        assert u["ScratchSize [bytes/lane]"] == 0, (frag, u)
        assert u["Occupancy [waves/SIMD]"] == OCCUPANCY, (frag, u)
        assert u["LDS Size [bytes/block]"] == LDS_BYTES, (frag, u)
