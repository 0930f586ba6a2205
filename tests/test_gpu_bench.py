"""-m gpu: a plain `bench.py` run - the headline figure alone, without the `--full` sections - and the maps its last timed step
returned, written with --dump-outputs: they must be the reference's own output for this sequence, weights and zoom position (G8)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tests.util import golden

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plain_bench_run_dumps_the_timed_maps(cuda, tmp_path):
    out = tmp_path / "outputs"
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1", "--dump-outputs", str(out)],
                       capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-1500:] + p.stderr[-1500:]
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    r = json.loads(lines[0])
    assert r["steps"] == 2 and r["warmup"] == 1 and r["unit"] == "Mb/s" and r["higher_is_better"] is True and r["dtype"].startswith("f16x2")
    assert r["metric"].startswith("Mb of sequence encoded+decoded per second") and r["ms_per_step"] > 0
    assert abs(r["value"] - 2 * 32 * 1e3 / r["ms_per_step"]) <= 1e-3 * r["value"]      # both 32 Mb strands per timed step
    assert not {"roofline", "parity", "exact_f32", "config5", "sharded_256mb", "cpu_baseline"} & set(r), sorted(r)
    g = golden("G8_full32m.npz")
    assert sorted(os.listdir(out)) == [f"pred_{j}.npy" for j in range(6)]
    for j in range(6):
        a = np.load(out / f"pred_{j}.npy")
        assert a.dtype == np.float32 and a.shape == (250, 250)
        assert np.abs(a.astype(np.float64) - g[f"pred_{j}"]).max() < 1e-4, j
