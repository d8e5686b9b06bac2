"""Register / LDS guard for the FP8 paged append kernel (append_fp8.hip),
by the method of test_decode_fp8_kernel_resources.py. Both block sizes hold
a tile's raw bytes in registers next to 64 accumulator registers and the
score tile; docs/KERNELS.md states two waves per SIMD, no spill and the LDS
of each instantiation."""

import pytest

from .kernel_remarks import hipcc, kernel_usage, resource_usage

# append_fp8.hip is included after append.hip and decode_fp8.hip, with the
# files those build on in front
TU = ('#include "attention.hip"\n#include "paged.hip"\n'
      '#include "decode.hip"\n#include "append.hip"\n'
      '#include "decode_fp8.hip"\n#include "append_fp8.hip"\n'
      'template __global__ void attn_append_paged_fp8_kernel<1>(\n'
      '    const short*, const unsigned char*, const unsigned char*,\n'
      '    const float*, const float*, const int*, const int*, short*,\n'
      '    float*, float*, int, int, int, int, int, int, int, float);\n'
      'template __global__ void attn_append_paged_fp8_kernel<4>(\n'
      '    const short*, const unsigned char*, const unsigned char*,\n'
      '    const float*, const float*, const int*, const int*, short*,\n'
      '    float*, float*, int, int, int, int, int, int, int, float);\n')

# K and V tiles [64][128] bf16; the 4-wave kernel adds the k and v row
# scales [64] fp32, the 1-wave kernel keeps them in registers (lane = row)
LDS_BYTES = {1: 2 * 64 * 128 * 2, 4: 2 * 64 * 128 * 2 + 2 * 64 * 4}


@pytest.mark.skipif(hipcc() is None, reason="hipcc not installed")
@pytest.mark.parametrize("nw", [1, 4])
def test_append_fp8_kernel_resources(tmp_path, nw):
    usage = resource_usage(TU, tmp_path, "append_fp8_tu")
    u = kernel_usage(usage, "attn_append_paged_fp8_kernelILi%dE" % nw)
    assert u["SGPRs Spill"] == 0, u
    assert u["VGPRs Spill"] == 0, u
    assert u["ScratchSize [bytes/lane]"] == 0, u
    assert u["LDS Size [bytes/block]"] == LDS_BYTES[nw], u
    assert u["Occupancy [waves/SIMD]"] == 2, u
