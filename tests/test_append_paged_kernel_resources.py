"""Register / LDS budget guard for the paged append attention kernel.

Same method as test_append_kernel_resources.py: cross-compile a
translation unit that instantiates both block sizes of
attn_append_paged_kernel for gfx950 (no GPU needed) and read the
compiler's resource remarks. The kernel is the dense append kernel's body
plus a block-table lookup per tile; the page base must stay in scalar
registers and cost no vector register, because the dense loop already
sits at the limit of two waves per SIMD. A spill, or a drop to one wave
per SIMD, is a large silent slowdown.
"""

import pytest

from .kernel_remarks import hipcc, kernel_usage, resource_usage

# the include order of mfx_hip.hip: append.hip builds on attention.hip's
# helpers and paged.hip's constants
TU = """#include "attention.hip"
#include "paged.hip"
#include "append.hip"
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


@pytest.mark.skipif(hipcc() is None, reason="hipcc not installed")
def test_append_paged_kernel_resources(tmp_path):
    usage = resource_usage(TU, tmp_path, "append_paged_tu")
    for frag in KERNELS:
        u = kernel_usage(usage, frag)
        assert u["SGPRs Spill"] == 0, (frag, u)
        assert u["VGPRs Spill"] == 0, (frag, u)
        assert u["ScratchSize [bytes/lane]"] == 0, (frag, u)
        assert u["Occupancy [waves/SIMD]"] == OCCUPANCY, (frag, u)
        assert u["LDS Size [bytes/block]"] == LDS_BYTES, (frag, u)
