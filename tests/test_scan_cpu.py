"""The host side of the chromosome scan (orca_amd/scan.py), without a GPU: the window planner and its coverage bound by brute force, the two numpy
restatements against independent dense computations, and the argument checks of `scan_1m`, which raise before any device is touched."""
import itertools

import numpy as np
import pytest
import torch

from orca_amd import scan as C
from orca_amd import screen as S
from orca_amd._lib import OrcaHipError


def _cases():
    for n, trim in itertools.product((3, 8, 50), (0, 1, 5)):
        if n - 2 * trim < 1:
            continue
        for step in sorted({1, n // 3, n - 2 * trim}):
            if 1 <= step <= n - 2 * trim:
                for n_total in (n, n + 1, 3 * n + 7):
                    yield n, step, trim, n_total


def _covering(off, n, trim, i, d):
    """the number of windows that cover pixel (i, i + d), from the rule alone"""
    return sum(1 for o in off if trim <= i - o and i - o + d <= n - 1 - trim)


@pytest.mark.parametrize("n, step, trim, n_total", list(_cases()))
def test_the_plan_covers_every_pixel_down_to_full_depth_and_no_further(n, step, trim, n_total):
    off = C.plan_windows(n_total, n, step, trim)
    assert off.dtype == np.int64 and off[0] == 0 and off[-1] == n_total - n
    gaps = np.diff(off)
    assert np.all(gaps >= 1) and np.all(gaps <= step)
    assert all(o % step == 0 for o in off[:-1]) and off.size == (n_total - n + step - 1) // step + 1
    D = C.full_depth(n, step, trim)
    assert D == n - 2 * trim - step + 1 and D >= 1
    for d in range(D):
        for i in range(trim, n_total - trim - d):                      # trim <= i and i + d <= n_total - 1 - trim
            assert _covering(off, n, trim, i, d) >= 1, (i, d)
    if np.any(gaps == step):                                           # an interior gap of `step`: the bound is sharp
        legal = range(trim, n_total - trim - D)
        assert len(legal) and any(_covering(off, n, trim, i, D) == 0 for i in legal)


def test_the_planner_refuses_what_it_cannot_lay_out():
    for bad in ((10, 11, 1, 0), (10, 4, 0, 0), (10, 4, 1, -1), (10, 4, 1, 2)):
        with pytest.raises(ValueError):
            C.plan_windows(*bad)
    assert C.full_depth(250, 100, 10) == 131
    assert list(C.plan_windows(163, 50, 15, 5)) == [0, 15, 30, 45, 60, 75, 90, 105, 113]


def _dense_stitch(maps, off, trim, N, D):
    """written independently of `stitch_band_host`: a dense [N, N] accumulate-and-average, pixel by pixel, then the band read off it"""
    B, n = maps.shape[0], maps.shape[1]
    vals = {}
    for b in range(B):
        for r in range(trim, n - trim):
            for c in range(r, n - trim):
                if c - r < D:
                    vals.setdefault((int(off[b]) + r, int(off[b]) + c), []).append(maps[b, r, c])
    band, count, rng = np.full((N, D), np.nan, np.float32), np.zeros((N, D), np.int32), np.full((N, D), np.nan, np.float32)
    for (i, j), v in vals.items():
        s = np.float64(0.0)
        for x in v:
            s += np.float64(x)
        band[i, j - i] = np.float32(s / np.float64(len(v)))
        count[i, j - i] = len(v)
        rng[i, j - i] = np.float32(np.nan) if np.isnan(v).any() else np.float32(max(v)) - np.float32(min(v))
    return band, count, rng


def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(a[~np.isnan(a)], b[~np.isnan(b)])


@pytest.mark.parametrize("n, trim, D, off, N", [(8, 1, 6, (0, 3, 5, 14), 24), (8, 0, 8, (0,), 8), (8, 3, 2, (1, 2, 3), 12), (11, 2, 4, (0, 4, 8, 9), 20)])
def test_stitch_band_host_equals_a_dense_accumulate_and_average(n, trim, D, off, N):
    rs = np.random.RandomState(n * 100 + D)
    maps = rs.randn(len(off), n, n).astype(np.float32)
    band, count, rng = C.stitch_band_host(maps, off, trim, N, D)
    want = _dense_stitch(maps, off, trim, N, D)
    assert band.dtype == np.float32 and count.dtype == np.int32 and rng.dtype == np.float32
    assert _same(band, want[0]) and np.array_equal(count, want[1]) and _same(rng, want[2])
    assert np.array_equal(np.isnan(band), count == 0) and np.all(rng[count == 1] == 0) and np.all(rng[count > 1] >= 0)
    if len(off) > 1:
        assert count.max() >= 2
    # the lower triangle is never read
    low = maps.copy()
    low[:, np.tril_indices(n, -1)[0], np.tril_indices(n, -1)[1]] = np.nan
    again = C.stitch_band_host(low, off, trim, N, D)
    assert _same(again[0], band) and np.array_equal(again[1], count) and _same(again[2], rng)
    # a NaN pixel of one window: exactly one band pixel, band and range both, the count as before
    r, c = trim, trim + D - 1
    bad = maps.copy()
    bad[-1, r, c] = np.nan
    nb, nc, nr = C.stitch_band_host(bad, off, trim, N, D)
    want = _dense_stitch(bad, off, trim, N, D)
    assert _same(nb, want[0]) and _same(nr, want[2]) and np.array_equal(nc, count)
    hit = np.argwhere(np.isnan(nb) & ~np.isnan(band))
    assert hit.tolist() == [[off[-1] + r, c - r]] and np.isnan(nr[off[-1] + r, c - r])
    assert np.array_equal(np.isnan(nr) & ~np.isnan(rng), np.isnan(nb) & ~np.isnan(band))


def test_stitch_band_host_refuses_malformed_tables():
    maps = np.zeros((2, 8, 8), np.float32)
    for off, trim, N, D in (((3, 3), 0, 20, 4), ((0, 13), 0, 20, 4), ((-1, 3), 0, 20, 4), ((0, 3), 0, 20, 9), ((0, 3), 2, 20, 5), ((0, 3), -1, 20, 4)):
        with pytest.raises(ValueError):
            C.stitch_band_host(maps, off, trim, N, D)


@pytest.mark.parametrize("N, D", [(3, 3), (40, 9), (65, 27)])
def test_band_insulation_host_equals_insulation_host_on_the_dense_map(N, D):
    rs = np.random.RandomState(N + D)
    band = rs.randn(N, D).astype(np.float32)
    for i in range(N):
        band[i, max(0, N - i):] = np.nan                               # pixels the stretch does not have
    holes = N > 10
    if holes:
        band[N // 2, 2] = np.nan
    widths = list(range(1, (D - 1) // 2 + 1))
    got = C.band_insulation_host(band, widths)
    dense = C.dense_host(band, N)
    assert np.array_equal(dense, dense.T, equal_nan=True) and np.array_equal(np.diag(dense), band[:, 0])
    want = S.insulation_host(dense[None], widths)[0]                   # every diamond reaches distance 2 w <= D - 1: inside the band
    assert got.shape == want.shape == (len(widths), N)
    assert np.array_equal(np.isnan(got), np.isnan(want))
    f = ~np.isnan(want)
    assert np.all(np.abs(got[f] - want[f]) <= 2.0 * max(widths) ** 2 * 2.0 ** -53 * np.nanmax(np.abs(band)))
    for k, w in enumerate(widths):
        fits = np.zeros(N, bool)
        fits[w: max(w, N - w)] = True
        assert not np.isnan(got[k, ~fits]).size or np.isnan(got[k, ~fits]).all()
        if not holes:
            assert not np.isnan(got[k, fits]).any()
    if holes:                                                          # the hole shows in the diamonds that hold pixel (N // 2, N // 2 + 2), in no other
        r, c = N // 2, N // 2 + 2
        for k, w in enumerate(widths):
            held = np.array([w <= i < N - w and i - w <= r < i < c <= i + w for i in range(N)])
            assert np.array_equal(np.isnan(got[k]) & (np.arange(N) >= w) & (np.arange(N) < N - w), held), w
    with pytest.raises(ValueError):
        C.band_insulation_host(band, [(D - 1) // 2 + 1])


def test_scan_1m_checks_its_arguments_before_it_touches_a_device():
    codes = torch.zeros(400_000, dtype=torch.uint8)
    kw = dict(window_bp=200_000, step_bp=60_000, trim_bins=5)
    with pytest.raises(ValueError, match="step_bp"):
        C.scan_1m(None, codes, **dict(kw, step_bp=60_001))
    with pytest.raises(ValueError, match="window_bp"):
        C.scan_1m(None, codes, **dict(kw, window_bp=1_028_000))
    assert C.full_depth(50, 15, 5) == 26
    with pytest.raises(ValueError, match="depth"):
        C.scan_1m(None, codes, depth=27, **kw)
    with pytest.raises(ValueError, match="depth"):
        C.scan_1m(None, codes, depth=0, **kw)
    with pytest.raises(ValueError, match="step_bp"):
        C.scan_1m(None, codes, **dict(kw, step_bp=164_000))             # wider than the trimmed window: holes at every distance
    with pytest.raises(ValueError, match="boundaries"):
        C.scan_1m(None, codes, boundaries=True, **kw)
    with pytest.raises(ValueError, match="boundaries"):
        C.scan_1m(None, codes, insulation=3, boundaries=0.1, **kw)
    with pytest.raises(ValueError, match="insulation"):
        C.scan_1m(None, codes, insulation=13, **kw)                     # 2 w + 1 > D = 26
    with pytest.raises(ValueError, match="strands"):
        C.scan_1m(None, codes, strands="-", **kw)
    with pytest.raises(OrcaHipError, match="no CPU path"):
        C.scan_1m(None, codes, **kw)
    with pytest.raises(OrcaHipError, match="no CPU path"):
        C.scan_1m(None, codes, insulation=(3, 10), boundaries=True, spread=True, strands="both", **kw)


def test_result_helpers():
    band = np.arange(12, dtype=np.float32).reshape(4, 3)
    res = C.ScanResult(8_000, 4_000, np.array([0], np.int64), 4, 3, torch.from_numpy(band), torch.ones(4, 3, dtype=torch.int32))
    assert res.bin_of(8_000) == 0 and res.bin_of(23_999) == 3 and res.pos_of(3) == 20_000 and res.pos_of(4) == 24_000
    for bad in (7_999, 24_000):
        with pytest.raises(ValueError):
            res.bin_of(bad)
    d = res.dense(1, 4)
    assert d.shape == (3, 3) and np.array_equal(d, np.array([[3, 4, 5], [4, 6, 7], [5, 7, 9]], np.float32))
    d = res.dense(0, 4)
    assert np.isnan(d[0, 3]) and np.isnan(d[3, 0]) and d[0, 2] == 2 and d[3, 3] == 9
    lists = C.boundary_lists_host(np.array([[np.nan, 0.5, np.nan, 0.05, 0.1]], np.float32), 0.1)
    assert lists[0][0].tolist() == [1, 4] and lists[0][0].dtype == np.int64 and lists[0][1].dtype == np.float32
