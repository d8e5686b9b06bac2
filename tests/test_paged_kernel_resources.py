"""Register / scratch guard for the decode kernels and the page write.

Same method as test_append_kernel_resources.py: cross-compile paged.hip
and decode.hip for gfx950 (no GPU needed) and read the compiler's resource
remarks. All three kernels are memory-bound streams: a spill to scratch
adds traffic on the very path they are bound by, silently. The two decode
kernels are one body (attn_decode_impl) instantiated for the dense cache
and for the page pool; both report three waves per SIMD, and a drop to two
takes a third of the loads in flight away from a kernel that lives on
them, so that figure is held too.
"""

import pytest

from .kernel_remarks import hipcc, kernel_usage, resource_usage

# decode.hip takes the page constants from paged.hip, as in mfx_hip.hip
TU = '#include "paged.hip"\n#include "decode.hip"\n'

DECODE_KERNELS = ("attn_decode_partial_kernel",
                  "attn_decode_paged_partial_kernel")
KERNELS = DECODE_KERNELS + ("kv_page_write_kernel",)
# declared __shared__ of the decode kernels: q row, 4 x (m, l), 4 x o row
DECODE_LDS_BYTES = (128 + 4 + 4 + 4 * 128) * 4
# regression guard, not a target: what the build reports for both
DECODE_OCCUPANCY = 3


@pytest.mark.skipif(hipcc() is None, reason="hipcc not installed")
def test_paged_kernel_resources(tmp_path):
    usage = resource_usage(TU, tmp_path, "paged_tu")
    for frag in KERNELS:
        u = kernel_usage(usage, frag)
        assert u["SGPRs Spill"] == 0, (frag, u)
        assert u["VGPRs Spill"] == 0, (frag, u)
        assert u["ScratchSize [bytes/lane]"] == 0, (frag, u)
    for frag in DECODE_KERNELS:
        u = kernel_usage(usage, frag)
        assert u["LDS Size [bytes/block]"] == DECODE_LDS_BYTES, (frag, u)
        assert u["Occupancy [waves/SIMD]"] == DECODE_OCCUPANCY, (frag, u)
