"""Register / LDS budget guard for the MoE prefill kernels
(moe_prefill.hip), by the method of test_moe_kernel_resources.py. The two
GEMM kernels hold a 64 x 64 accumulator tile per matrix and a whole staged
chunk in registers; a spill would put scratch traffic between the MFMAs."""

import pytest

from .kernel_remarks import hipcc, kernel_usage, resource_usage

# included after attention.hip and moe.hip, as in mfx_hip.hip
TU = """#include "attention.hip"
#include "moe.hip"
#include "moe_prefill.hip"
"""

TM, TN, KC, BF16 = 128, 128, 64, 2
assert TM == TN            # one image shape serves entries and weight rows
IMAGE_BYTES = TM * KC * BF16
BUFFERS = 2
# kernel: images per buffer (the entries, and one per weight matrix), or
# None for the kernels that are no GEMM
KERNELS = {"moep_topk_kernel": None, "moep_scan_kernel": None,
           "moep_scatter_kernel": None, "moep_gateup_kernel": 3,
           "moep_dn_kernel": 2}


@pytest.mark.skipif(hipcc() is None, reason="hipcc not installed")
def test_moe_prefill_kernel_resources(tmp_path):
    usage = resource_usage(TU, tmp_path, "moe_prefill_tu")
    for frag, images in KERNELS.items():
        u = kernel_usage(usage, frag)
        assert u["SGPRs Spill"] == 0, (frag, u)
        assert u["VGPRs Spill"] == 0, (frag, u)
        assert u["ScratchSize [bytes/lane]"] == 0, (frag, u)
        if images:
            lds = images * BUFFERS * IMAGE_BYTES
            assert lds <= 160 * 1024
            assert u["LDS Size [bytes/block]"] == lds, (frag, u)
