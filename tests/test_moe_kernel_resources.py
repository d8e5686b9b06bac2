"""Register / LDS budget guard for the MoE decode kernels (moe.hip), by the
method of test_append_kernel_resources.py: cross-compile for gfx950 (no GPU
needed) and read the compiler's resource remarks. The two stream kernels
keep two chunks of weight fragments in registers; a spill there would put
scratch traffic into a loop whose only job is to keep loads in flight."""

import pytest

from .kernel_remarks import hipcc, kernel_usage, resource_usage

# moe.hip builds on attention.hip's helpers and is included after it, as in
# mfx_hip.hip
TU = """#include "attention.hip"
#include "moe.hip"
"""

KERNELS = ["moe_route_kernel", "moe_gate_up_kernel", "moe_down_kernel",
           "moe_combine_kernel"]
# two x-chunk images of [32 tokens][128 k] bf16
STREAM_LDS_BYTES = 2 * 32 * 128 * 2


@pytest.mark.skipif(hipcc() is None, reason="hipcc not installed")
def test_moe_kernel_resources(tmp_path):
    usage = resource_usage(TU, tmp_path, "moe_tu")
    for frag in KERNELS:
        u = kernel_usage(usage, frag)
        assert u["SGPRs Spill"] == 0, (frag, u)
        assert u["VGPRs Spill"] == 0, (frag, u)
        assert u["ScratchSize [bytes/lane]"] == 0, (frag, u)
        if frag in ("moe_gate_up_kernel", "moe_down_kernel"):
            assert u["LDS Size [bytes/block]"] == STREAM_LDS_BYTES, (frag, u)
