"""Build-time properties of the kernels of the chromosome scan (orca_amd/csrc/scan.h), checked by cross-compiling the header by itself for gfx950 (no
GPU needed): each of the four kernels is emitted and uses no scratch memory.  The running sums and the two running maxima of a walk live in
registers, in plain C++; a spill would mean they went to memory.  None of them uses LDS."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = ("scan_stitch_band_kernel", "scan_band_finish_kernel", "scan_band_insulation_kernel", "scan_boundary_strength_kernel")
UNIT = """#include "scan.h"
const void* scan_kernels[] = {%s};
"""


def test_scan_kernels_are_emitted_and_do_not_spill(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    src = os.path.join(ROOT, "orca_amd", "csrc")
    unit = tmp_path / "scan_unit.hip"
    unit.write_text(UNIT % ", ".join("(const void*)" + k for k in KERNELS))
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-I" + src, "-I" + os.path.join(ROOT, "include"), "-Wall", "-Werror",
                        "-Wno-unused-function", "-c", str(unit), "-o", str(tmp_path / "scan_unit.o"), "-Rpass-analysis=kernel-resource-usage"],
                       capture_output=True, text=True, timeout=600)
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
        assert lds.get(hit[0]) == 0, (hit[0], lds)
