"""Register / LDS budget guard for the dense stream kernels
(linear_fp8.hip), by the method of the MoE guards: no spill and no scratch in
any instantiation, and exactly the x image in LDS: two buffers of 32 NB rows
of 256 bytes. VGPRs and occupancy are recorded in docs/KERNELS.md, "FP8 dense
weights"."""

import pytest

from .kernel_remarks import hipcc, kernel_usage, resource_usage

TU = """#include "attention.hip"
#include "moe.hip"
#include "linear_fp8.hip"
"""

# kernel: LDS bytes per block
KERNELS = {"lin_stream_%s_nb%d%s_kernel" % (w, nb, sw): 2 * 32 * nb * 256
           for w in ("bf16", "fp8") for nb in (1, 2)
           for sw in ("", "_swiglu")}
KERNELS.update(lin_reduce_kernel=0, lin_dequant_kernel=0)


@pytest.mark.skipif(hipcc() is None, reason="hipcc not installed")
def test_linear_fp8_kernel_resources(tmp_path):
    usage = resource_usage(TU, tmp_path, "linear_fp8_tu")
    for frag, lds in KERNELS.items():
        u = kernel_usage(usage, frag)
        assert u["SGPRs Spill"] == 0, (frag, u)
        assert u["VGPRs Spill"] == 0, (frag, u)
        assert u["ScratchSize [bytes/lane]"] == 0, (frag, u)
        assert u["LDS Size [bytes/block]"] == lds, (frag, u)
