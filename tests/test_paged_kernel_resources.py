"""Register / scratch guard for the paged KV cache kernels.

Same method as test_append_kernel_resources.py: cross-compile paged.hip
for gfx950 (no GPU needed) and read the compiler's resource remarks. Both
kernels are memory-bound streams: a spill to scratch adds traffic on the
very path they are bound by, silently. The occupancy is printed, not
asserted — nothing in the docs depends on a particular figure.
"""

import os
import re
import shutil
import subprocess

import pytest

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                    "metaflow_amd", "ops", "csrc")

TU = '#include "paged.hip"\n'

KERNELS = ("attn_decode_paged_partial_kernel", "kv_page_write_kernel")
# declared __shared__ of the decode kernel: q row, 4 x (m, l), 4 x o row
DECODE_LDS_BYTES = (128 + 4 + 4 + 4 * 128) * 4


def _hipcc():
    return shutil.which("hipcc") or (
        "/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc")
        else None)


@pytest.mark.skipif(_hipcc() is None, reason="hipcc not installed")
def test_paged_kernel_resources(tmp_path):
    src = tmp_path / "paged_tu.hip"
    src.write_text(TU)
    proc = subprocess.run(
        [_hipcc(), "--offload-arch=gfx950", "--cuda-device-only", "-O3",
         "-std=c++17", "-S", "-Rpass-analysis=kernel-resource-usage",
         "-I", CSRC, str(src), "-o", str(tmp_path / "paged_tu.s")],
        capture_output=True, text=True)
    assert proc.returncode == 0, proc.stderr[-2000:]

    # remarks come as one block per kernel, headed by "Function Name:"
    usage = {}
    cur = None
    for line in proc.stderr.splitlines():
        m = re.search(r"remark: (?:Function Name: (\S+)|\s*([^:]+): (\d+))",
                      line)
        if not m:
            continue
        if m.group(1):
            cur = usage.setdefault(m.group(1), {})
        elif cur is not None:
            cur[m.group(2).strip()] = int(m.group(3))

    for frag in KERNELS:
        names = [n for n in usage if frag in n]
        assert len(names) == 1, (frag, sorted(usage))
        u = usage[names[0]]
        print(frag, u)
        assert u["SGPRs Spill"] == 0, (frag, u)
        assert u["VGPRs Spill"] == 0, (frag, u)
        assert u["ScratchSize [bytes/lane]"] == 0, (frag, u)
    lds = usage[[n for n in usage if KERNELS[0] in n][0]]
    assert lds["LDS Size [bytes/block]"] == DECODE_LDS_BYTES, lds
