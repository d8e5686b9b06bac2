"""Register / LDS budget guard for the three MFMA attention kernels.

attn_bwd_dkdv_v2_kernel sits exactly at the 256-VGPR limit with zero
spills and dq is a few registers below it; a spill or a lost wave of
occupancy is a large silent slowdown. Cross-compiles the attention source
for gfx950 (no GPU needed) and reads the compiler's resource remarks.
"""

import pytest

from .kernel_remarks import hipcc, kernel_usage, resource_usage

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


@pytest.mark.skipif(hipcc() is None, reason="hipcc not installed")
def test_attention_kernel_resources(tmp_path):
    usage = resource_usage(TU, tmp_path, "attn_tu")
    for frag, lds in LDS_BYTES.items():
        u = kernel_usage(usage, frag)
        assert u["SGPRs Spill"] == 0, (frag, u)
        assert u["VGPRs Spill"] == 0, (frag, u)
        assert u["Occupancy [waves/SIMD]"] == 2, (frag, u)
        assert u["LDS Size [bytes/block]"] == lds, (frag, u)
