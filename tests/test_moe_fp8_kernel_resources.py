"""Register / LDS budget guard for the E4M3 MoE kernels (moe.hip,
moe_prefill.hip), by the method of their bf16 twins: no spill, no scratch,
and the LDS of the bf16 kernel each mirrors (the images are the same, only
the way the weights reach them differs). VGPRs and occupancy are recorded in
docs/KERNELS.md, "FP8 expert weights"."""

import pytest

from .kernel_remarks import hipcc, kernel_usage, resource_usage

TU = """#include "attention.hip"
#include "moe.hip"
#include "moe_prefill.hip"
"""

# E4M3 kernel: the bf16 kernel it mirrors
TWINS = {"moe8_gate_up_kernel": "moe_gate_up_kernel",
         "moe8_down_kernel": "moe_down_kernel",
         "moep8_gateup_kernel": "moep_gateup_kernel",
         "moep8_dn_kernel": "moep_dn_kernel"}


@pytest.mark.skipif(hipcc() is None, reason="hipcc not installed")
def test_moe_fp8_kernel_resources(tmp_path):
    usage = resource_usage(TU, tmp_path, "moe_fp8_tu")
    for frag, twin in TWINS.items():
        u = kernel_usage(usage, frag)
        assert u["SGPRs Spill"] == 0, (frag, u)
        assert u["VGPRs Spill"] == 0, (frag, u)
        assert u["ScratchSize [bytes/lane]"] == 0, (frag, u)
        assert u["LDS Size [bytes/block]"] == \
            kernel_usage(usage, twin)["LDS Size [bytes/block]"], (frag, u)
