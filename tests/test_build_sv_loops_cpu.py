"""Build-time property of the kernel behind the SV screen's loops per level (orca_amd/csrc/screen.h: screen_paired_dot_follow_kernel), checked by
cross-compiling for gfx950 (no GPU needed): it uses no scratch memory.  Every lane keeps its best candidate (an index and an e) in registers, in
plain C++, and the bin lists live in LDS; a spill would mean they went to memory."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = ("screen_paired_dot_follow_kernel",)
UNIT = """#include <hip/hip_runtime.h>
typedef float f32x4 __attribute__((ext_vector_type(4)));
#include "screen.h"
const void* screen_kernels[] = {%s};
"""


def test_dot_follow_kernel_does_not_spill(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    src = os.path.join(ROOT, "orca_amd", "csrc")
    unit = tmp_path / "screen_dot_follow_unit.hip"
    unit.write_text(UNIT % ", ".join("(const void*)" + k for k in KERNELS))
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-I" + src, "-I" + os.path.join(ROOT, "include"), "-Wno-unused-function", "-c",
                        str(unit), "-o", str(tmp_path / "screen_dot_follow_unit.o"), "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    name, scratch = None, {}
    for line in r.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            continue
        m = re.search(r"ScratchSize \[bytes/lane\]: (\d+)", line)
        if m and name:
            scratch[name] = int(m.group(1))
    for k in KERNELS:
        hit = [n for n in scratch if k in n]
        assert len(hit) == 1, (k, sorted(scratch))          # the remark format changed, or the kernel was not emitted?
        assert scratch[hit[0]] == 0, (hit[0], scratch[hit[0]])
