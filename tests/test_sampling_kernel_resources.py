"""Register / scratch guard for the sampler kernels.

Same method as test_paged_kernel_resources.py: cross-compile sampling.hip
for gfx950 (no GPU needed) and read the compiler's resource remarks. The
kernel streams a row from L2 several times; a spill to scratch would add
traffic to every pass, silently. One workgroup is 1024 threads, four waves
per SIMD, so a workgroup only fits a CU with at most 128 VGPRs per lane.
"""

import pytest

from .kernel_remarks import hipcc, kernel_usage, resource_usage

ARGS = ("(const {t}*, long long, int, float, const float*, const int*, "
        "const float*, const float*, long long*)")
TU = ('#include "sampling.hip"\n'
      + "".join("template __global__ void sample_tokens_kernel<{t}>%s;\n"
                .replace("%s", ARGS).format(t=t) for t in ("short", "float")))

# mangled template arguments: bf16 rows are passed as short
KERNELS = ("sample_tokens_kernelIsE", "sample_tokens_kernelIfE")
# the histogram (256 bins x 16 replicas x 8 bytes) and the reduction words
LDS_MAX_BYTES = 256 * 16 * 8 + 512


@pytest.mark.skipif(hipcc() is None, reason="hipcc not installed")
def test_sampling_kernel_resources(tmp_path):
    usage = resource_usage(TU, tmp_path, "sampling_tu")
    for frag in KERNELS:
        u = kernel_usage(usage, frag)
        assert u["SGPRs Spill"] == 0, (frag, u)
        assert u["VGPRs Spill"] == 0, (frag, u)
        assert u["ScratchSize [bytes/lane]"] == 0, (frag, u)
        assert u["VGPRs"] <= 128, (frag, u)
        assert u["Occupancy [waves/SIMD]"] >= 4, (frag, u)
        assert u["LDS Size [bytes/block]"] <= LDS_MAX_BYTES, (frag, u)
