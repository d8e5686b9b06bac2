"""Register / LDS budget guard for the three MFMA attention kernels.

attn_bwd_dkdv_v2_kernel sits exactly at the 256-VGPR limit with zero
spills and dq is a few registers below it; a spill or a lost wave of
occupancy is a large silent slowdown. Cross-compiles the attention source
for gfx950 (no GPU needed) and reads the compiler's resource remarks.
"""

import os
import re
import shutil
import subprocess

import pytest

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                    "metaflow_amd", "ops", "csrc")

TU = """#include "attention.hip"
template __global__ void attn_fwd_v2_kernel<512>(
    const short*, const short*, const short*, short*, float*, int, int, int,
    int, float, int);
template __global__ void attn_bwd_dq_v2_kernel<512>(
    const short*, const short*, const short*, const short*, const float*,
    const float*, short*, int, int, int, int, float, int);
template __global__ void attn_bwd_dkdv_v2_kernel<512>(
    const short*, const short*, const short*, const short*, const float*,
    const float*, float*, float*, int, int, int, int, float, int);
"""

# kernel name fragment -> LDS bytes per block from the declared __shared__
# arrays: fwd 2x2 16 KiB tiles; dq 2 tiles; dkdv 2 tiles + 2x64 floats
LDS_BYTES = {
    "attn_fwd_v2_kernel": 4 * 16384,
    "attn_bwd_dq_v2_kernel": 2 * 16384,
    "attn_bwd_dkdv_v2_kernel": 2 * 16384 + 2 * 64 * 4,
}


def _hipcc():
    return shutil.which("hipcc") or (
        "/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc")
        else None)


@pytest.mark.skipif(_hipcc() is None, reason="hipcc not installed")
def test_attention_kernel_resources(tmp_path):
    src = tmp_path / "attn_tu.hip"
    src.write_text(TU)
    proc = subprocess.run(
        [_hipcc(), "--offload-arch=gfx950", "--cuda-device-only", "-O3",
         "-std=c++17", "-S", "-Rpass-analysis=kernel-resource-usage",
         "-I", CSRC, str(src), "-o", str(tmp_path / "attn_tu.s")],
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

    for frag, lds in LDS_BYTES.items():
        names = [n for n in usage if frag in n]
        assert len(names) == 1, (frag, sorted(usage))
        u = usage[names[0]]
        print(frag, u)
        assert u["SGPRs Spill"] == 0, (frag, u)
        assert u["VGPRs Spill"] == 0, (frag, u)
        assert u["Occupancy [waves/SIMD]"] == 2, (frag, u)
        assert u["LDS Size [bytes/block]"] == lds, (frag, u)
