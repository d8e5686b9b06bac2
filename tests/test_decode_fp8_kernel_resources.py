"""Register / LDS guard for the FP8 paged-cache kernels (decode_fp8.hip),
by the method of test_paged_kernel_resources.py. The decode kernel keeps a
page per wave in flight next to 64 accumulator registers; docs/KERNELS.md
states two waves per SIMD and 66 KiB of LDS (two blocks per CU)."""

import pytest

from .kernel_remarks import hipcc, kernel_usage, resource_usage

# decode_fp8.hip builds on attention.hip's helpers, paged.hip's constants
# and decode.hip's merge kernel, and is included after them
TU = ('#include "attention.hip"\n#include "paged.hip"\n'
      '#include "decode.hip"\n#include "decode_fp8.hip"\n')

# 4 per-wave V tiles [64][128] bf16 + 4 x 2 row-scale vectors [64] fp32
DECODE_LDS_BYTES = 4 * 64 * 128 * 2 + 4 * 2 * 64 * 4
# (LDS bytes, waves per SIMD) as the doc states them
EXPECT = {
    "attn_decode_paged_fp8_partial_kernel": (DECODE_LDS_BYTES, 2),
    "kv_page_write_fp8_kernel": (0, 8),
}


@pytest.mark.skipif(hipcc() is None, reason="hipcc not installed")
def test_decode_fp8_kernel_resources(tmp_path):
    usage = resource_usage(TU, tmp_path, "decode_fp8_tu")
    for frag, (lds, occupancy) in EXPECT.items():
        u = kernel_usage(usage, frag)
        assert u["SGPRs Spill"] == 0, (frag, u)
        assert u["VGPRs Spill"] == 0, (frag, u)
        assert u["ScratchSize [bytes/lane]"] == 0, (frag, u)
        assert u["LDS Size [bytes/block]"] == lds, (frag, u)
        assert u["Occupancy [waves/SIMD]"] == occupancy, (frag, u)
