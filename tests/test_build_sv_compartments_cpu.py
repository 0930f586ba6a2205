"""Build-time properties of the kernels behind the SV screen's compartments per level (orca_amd/csrc/screen.h: screen_eigenvectors_kernel,
screen_gc_tracks_kernel), checked by cross-compiling for gfx950 (no GPU needed): they compile, and they use no scratch memory.  The eigen kernel keeps
the packed upper triangle of its map and every vector in LDS and a handful of fp64 sums in registers; the GC kernel takes its windows' offsets by
value and picks its own by a select chain.  A spill, or a table indexed in private memory, would show as scratch."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = ("screen_eigenvectors_kernel", "screen_gc_tracks_kernel")
UNIT = """#include <hip/hip_runtime.h>
typedef float f32x4 __attribute__((ext_vector_type(4)));
#include "screen.h"
const void* screen_kernels[] = {%s};
"""


def test_compartment_kernels_compile_for_gfx950_without_scratch(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    src = os.path.join(ROOT, "orca_amd", "csrc")
    unit = tmp_path / "screen_compartments_unit.hip"
    unit.write_text(UNIT % ", ".join("(const void*)" + k for k in KERNELS))
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-I" + src, "-I" + os.path.join(ROOT, "include"), "-Wno-unused-function", "-c",
                        str(unit), "-o", str(tmp_path / "screen_compartments_unit.o"), "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    name, scratch, lds = None, {}, {}
    for line in r.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            continue
        m = re.search(r"ScratchSize \[bytes/lane\]: (\d+)", line)
        if m and name:
            scratch[name] = int(m.group(1))
        m = re.search(r"LDS Size \[bytes/block\]: (\d+)", line)
        if m and name:
            lds[name] = int(m.group(1))
    for k in KERNELS:
        hit = [n for n in scratch if k in n]
        assert len(hit) == 1, (k, sorted(scratch))          # the remark format changed, or the kernel was not emitted?
        assert scratch[hit[0]] == 0, (hit[0], scratch[hit[0]])
        assert lds.get(hit[0], 0) <= 160 * 1024, (hit[0], lds)           # the CU's LDS: the packed triangle of a 256-bin map has to fit
