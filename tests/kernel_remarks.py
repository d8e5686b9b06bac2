"""Cross-compile a HIP translation unit for gfx950 (no GPU needed) and read
what the compiler says about it: shared by the kernel resource guards and
the loop-assembly guards."""

import os
import re
import shutil
import subprocess

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                    "metaflow_amd", "ops", "csrc")


def hipcc():
    return shutil.which("hipcc") or (
        "/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc")
        else None)


def compile_tu(tu, tmp_path, stem, remarks=False):
    """Write ``tu`` to tmp_path/stem.hip and compile it to assembly with
    the kernel sources on the include path. Returns (assembly text,
    compiler stderr)."""
    src = tmp_path / (stem + ".hip")
    src.write_text(tu)
    out = tmp_path / (stem + ".s")
    extra = ["-Rpass-analysis=kernel-resource-usage"] if remarks else []
    proc = subprocess.run(
        [hipcc(), "--offload-arch=gfx950", "--cuda-device-only", "-O3",
         "-std=c++17", "-S"] + extra +
        ["-I", CSRC, str(src), "-o", str(out)],
        capture_output=True, text=True)
    assert proc.returncode == 0, proc.stderr[-2000:]
    return out.read_text(), proc.stderr


def resource_usage(tu, tmp_path, stem):
    """{mangled kernel name: {remark name: value}} of every kernel in the
    translation unit."""
    _, stderr = compile_tu(tu, tmp_path, stem, remarks=True)
    # remarks come as one block per kernel, headed by "Function Name:"
    usage = {}
    cur = None
    for line in stderr.splitlines():
        m = re.search(r"remark: (?:Function Name: (\S+)|\s*([^:]+): (\d+))",
                      line)
        if not m:
            continue
        if m.group(1):
            cur = usage.setdefault(m.group(1), {})
        elif cur is not None:
            cur[m.group(2).strip()] = int(m.group(3))
    return usage


def kernel_usage(usage, frag):
    """The remarks of the one kernel whose mangled name contains ``frag``."""
    names = [n for n in usage if frag in n]
    assert len(names) == 1, (frag, sorted(usage))
    u = usage[names[0]]
    print(frag, u)
    return u
