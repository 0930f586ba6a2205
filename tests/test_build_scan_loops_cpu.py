"""Build-time properties of the kernels behind the scan's loop (dot) calls (orca_amd/csrc/scan_loops.h), checked by cross-compiling for gfx950 (no
GPU needed): the four kernels are emitted and use no scratch memory - the five fp64 sums of a window, the ballots and the prefix stay in registers -
and the enrichment kernel's tile of band rows fits the 64 KB a workgroup may declare: (32 + 2 * 16) rows of 256 floats at w = 16, D = 256."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = ("scan_band_dot_enrich_kernel", "scan_band_dot_count_kernel", "scan_row_offsets_kernel", "scan_band_dot_list_kernel")
UNIT = """#include <hip/hip_runtime.h>
typedef float f32x4 __attribute__((ext_vector_type(4)));
#include "screen.h"
#include "scan_loops.h"
const void* scan_loop_kernels[] = {%s};
"""


def test_scan_loop_kernels_are_emitted_do_not_spill_and_fit_lds(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    src = os.path.join(ROOT, "orca_amd", "csrc")
    unit = tmp_path / "scan_loops_unit.hip"
    unit.write_text(UNIT % ", ".join("(const void*)" + k for k in KERNELS))
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-I" + src, "-I" + os.path.join(ROOT, "include"), "-Wno-unused-function", "-c",
                        str(unit), "-o", str(tmp_path / "scan_loops_unit.o"), "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True, timeout=600)
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
    tile = [v for n, v in lds.items() if "scan_band_dot_enrich_kernel" in n]
    assert len(tile) == 1 and 0 < tile[0] <= 65536, lds     # the tile and its halo rows
    assert tile[0] == (32 + 2 * 16) * 256 * 4, lds
