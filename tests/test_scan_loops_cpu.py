"""The host side of the scan's loop (dot) calls, no GPU: `scan.band_dot_enrichment_host` and `scan.band_dot_calls_host`, which work on the band
itself, against `screen.dot_enrichment_host` and `screen.dot_calls_host` on the dense map the band stands for (`scan.dense_host`) - BIT FOR BIT: both
add the same fp64 terms in the same order, the band only addresses them as band[i + a, d + b - a]; `screen.check_band_loops`; and the ``loops=``
checks of `scan_1m`, which raise before any device is touched."""
import numpy as np
import pytest
import torch

from orca_amd import scan as C
from orca_amd import screen as S
from orca_amd._lib import OrcaHipError

SHAPES = [(40, 14, 0, 1), (60, 26, 1, 4), (23, 12, 1, 2), (18, 18, 1, 4), (100, 70, 15, 16)]          # (N, D, p, w); the last: w = 16, D = 70


def make_band(N, D, seed, quantum=None):
    """a band of a stretch of N bins: NaN where i + d >= N, two NaN rows at either end, one NaN pixel inside; multiples of ``quantum`` if given"""
    rs = np.random.RandomState(seed)
    b = rs.randn(N, D)
    if quantum:
        b = np.round(b / quantum) * quantum
    b = b.astype(np.float32)
    i, d = np.indices((N, D))
    b[i + d >= N] = np.nan
    b[:2] = b[-2:] = np.nan
    b[N // 2, D // 2] = np.nan
    return b


def along_diagonals(dense, N, D):
    """the dense [N, N] array read back as a band [N, D]: out[i, d] = dense[i, i + d], NaN where i + d >= N"""
    out = np.full((N, D), np.nan, dtype=dense.dtype)
    for d in range(min(D, N)):
        k = np.arange(N - d)
        out[k, d] = dense[k, k + d]
    return out


def same_f32(got, want):
    g, w = np.asarray(got), np.asarray(want)
    return g.dtype == w.dtype == np.float32 and g.shape == w.shape and np.array_equal(np.isnan(g), np.isnan(w)) and np.array_equal(g[~np.isnan(g)], w[~np.isnan(w)])


def dense_calls(band, q):
    """`screen.dot_calls_host` on the dense map with the largest list: (ij int64 [L, 2], enrich [L]); the old cap must not be reached"""
    N = band.shape[0]
    h = S.dot_calls_host(C.dense_host(band, N)[None], S.LoopParams(q.p, q.w, q.r, q.threshold, q.d_min, 4096, q.tol))
    L = int(h["count"][0])
    assert L <= 4096
    return h["ij"][0, :L].astype(np.int64), h["enrich"][0, :L]


@pytest.mark.parametrize("N,D,p,w", SHAPES)
def test_band_enrichment_equals_the_dense_restatement_bit_for_bit(N, D, p, w):
    band = make_band(N, D, 100 * N + D)
    for d_min in (None, 2 * w + 2):
        q = S.LoopParams(p=p, w=w, d_min=d_min)
        got = C.band_dot_enrichment_host(band, q)
        want = along_diagonals(S.dot_enrichment_host(C.dense_host(band, N)[None], q)[0], N, D)
        assert got.shape == (N, D) and same_f32(got, want), (N, D, p, w, d_min)
        dm = 2 * w + 1 if d_min is None else d_min
        i, d = np.indices((N, D))
        eligible = (i >= w) & (i + d <= N - 1 - w) & (d >= dm) & (d <= D - 1 - 2 * w)
        assert np.isnan(got[~eligible]).all()
        if (N, D) != (18, 18):                                                   # there the one eligible pixel's window meets the NaN rows
            assert np.isfinite(got[eligible]).any() and np.isnan(got[eligible]).any()        # the NaN pixel and the NaN ends take some windows
    clean = np.random.RandomState(N).randn(N, D).astype(np.float32)
    i, d = np.indices((N, D))
    clean[i + d >= N] = np.nan
    e = C.band_dot_enrichment_host(clean, S.LoopParams(p=p, w=w))
    assert np.array_equal(~np.isnan(e), (i >= w) & (i + d <= N - 1 - w) & (d >= 2 * w + 1) & (d <= D - 1 - 2 * w))       # NaN exactly where ineligible
    assert (~np.isnan(e)).sum() >= 1


@pytest.mark.parametrize("N,D,p,w", SHAPES)
def test_band_calls_equal_the_dense_calls(N, D, p, w):
    assert (N - 2 * w) * (D - 4 * w - 1) < 1500                                  # eligible pixels: far below the dense restatement's cap
    for quantum in (None, 0.125):                                                # multiples of 1/8: many equal enrichments, the tie rule decides
        band = make_band(N, D, 7 * N + D, quantum)
        e = C.band_dot_enrichment_host(band, S.LoopParams(p=p, w=w))
        cut = float(np.nanmedian(e)) if np.isfinite(e).any() else 0.0
        for r, T in ((1, -1e30), (2, 0.0), (2, cut), (16, -1e30)):
            q = S.LoopParams(p=p, w=w, r=r, threshold=T, max_calls=1)           # max_calls caps nothing on a band
            ij, enrich = C.band_dot_calls_host(e, q)
            want_ij, want_e = dense_calls(band, q)
            assert ij.dtype == np.int64 and enrich.dtype == np.float32 and ij.shape == (len(enrich), 2)
            assert np.array_equal(ij, want_ij) and np.array_equal(enrich, want_e), (N, D, p, w, quantum, r, T)
            assert np.array_equal(enrich, e[ij[:, 0], ij[:, 1] - ij[:, 0]])
            key = ij[:, 0] * D + (ij[:, 1] - ij[:, 0])
            assert np.all(np.diff(key) > 0)                                      # ascending (i, d)
        if quantum and w <= 2:                                                   # small sets: their means do coincide
            vals = e[np.isfinite(e)]
            assert len(np.unique(vals)) < len(vals)                              # ties did occur


@pytest.mark.parametrize("N,D,p,w", SHAPES)
def test_a_constant_band_has_exactly_one_dot(N, D, p, w):
    band = np.full((N, D), 1.5, dtype=np.float32)
    i, d = np.indices((N, D))
    band[i + d >= N] = np.nan
    for d_min in (2 * w + 1, 2 * w + 2):
        if D < d_min + 2 * w + 1:
            continue
        q = S.LoopParams(p=p, w=w, r=3, threshold=0.0, d_min=d_min)
        e = C.band_dot_enrichment_host(band, q)
        assert np.all(e[~np.isnan(e)] == 0.0)
        ij, enrich = C.band_dot_calls_host(e, q)
        assert ij.tolist() == [[w, w + d_min]] and enrich.tolist() == [0.0]
    none = C.band_dot_calls_host(e, S.LoopParams(p=p, w=w, threshold=1.0))
    assert none[0].shape == (0, 2) and none[0].dtype == np.int64 and none[1].shape == (0,) and none[1].dtype == np.float32


def test_the_smallest_band_with_an_eligible_pixel():
    w, d_min = 2, 6
    need = d_min + 2 * w + 1
    band = np.random.RandomState(0).randn(need, need).astype(np.float32)
    i, d = np.indices(band.shape)
    band[i + d >= need] = np.nan
    q = S.LoopParams(p=0, w=w, d_min=d_min, threshold=-1e30)
    e = C.band_dot_enrichment_host(band, q)
    assert np.argwhere(~np.isnan(e)).tolist() == [[w, d_min]]
    assert C.band_dot_calls_host(e, q)[0].tolist() == [[w, w + d_min]]
    for shape in ((need - 1, need), (need, need - 1)):                           # one row or one distance fewer: nothing
        assert np.isnan(C.band_dot_enrichment_host(np.zeros(shape, np.float32), q)).all()


def test_check_band_loops():
    q = S.check_band_loops(True, 163, 26)
    assert q == S.LoopParams(1, 4, 2, float(np.float32(0.25)), 9, 64, 1) and S.check_band_loops(q, 163, 26) == q
    assert S.check_band_loops(S.LoopParams(p=0, w=1), 6, 6).d_min == 3           # the smallest band: N = D = d_min + 2 w + 1
    with pytest.raises(ValueError, match=r"a band of 163 bins x 17 distances has no eligible pixel at w = 4, d_min = 9 .*18"):
        S.check_band_loops(True, 163, 17)
    with pytest.raises(ValueError, match=r"a band of 17 bins x 26 distances has no eligible pixel"):
        S.check_band_loops(True, 17, 26)
    with pytest.raises(ValueError, match="no eligible pixel"):
        S.check_band_loops(S.LoopParams(d_min=18), 163, 26)
    for bad, word in ((S.LoopParams(p=4, w=4), "p = 4, w = 4"), (S.LoopParams(w=17), "w = 17"), (S.LoopParams(r=0), "r = 0"), (S.LoopParams(r=17), "r = 17"),
                      (S.LoopParams(d_min=8), "d_min = 8"), (S.LoopParams(threshold=float("nan")), "NaN"), (S.LoopParams(max_calls=0), "max_calls"),
                      (S.LoopParams(tol=-1), "tol"), (S.LoopParams(w=4.0), "must be an int"), ("yes", "loops: True"), (0.25, "loops: True")):
        with pytest.raises(ValueError, match=word):
            S.check_band_loops(bad, 163, 131)
    assert S.check_band_loops(S.LoopParams(max_calls=1, tol=0), 163, 26).max_calls == 1           # accepted; the scan does not use them


def test_scan_1m_checks_loops_before_it_touches_a_device():
    codes = torch.zeros(400_000, dtype=torch.uint8)
    kw = dict(window_bp=200_000, step_bp=60_000, trim_bins=5)                   # D = 26
    with pytest.raises(ValueError, match="loops: True"):
        C.scan_1m(None, codes, loops="yes", **kw)
    with pytest.raises(ValueError, match="loops: r = 0"):
        C.scan_1m(None, codes, loops=S.LoopParams(r=0), **kw)
    with pytest.raises(ValueError, match="NaN"):
        C.scan_1m(None, codes, loops=S.LoopParams(threshold=float("nan")), **kw)
    with pytest.raises(ValueError, match=r"x 26 distances has no eligible pixel at w = 7, d_min = 15"):
        C.scan_1m(None, codes, loops=S.LoopParams(w=7), **kw)                   # d_min + 2 w + 1 = 30 > D; w = 6 asks for 26 and fits
    with pytest.raises(OrcaHipError, match="no CPU path"):
        C.scan_1m(None, codes, loops=S.LoopParams(w=6), **kw)
    with pytest.raises(ValueError, match="no eligible pixel"):
        C.scan_1m(None, codes, loops=True, depth=17, **kw)
    for ok in (True, S.LoopParams(threshold=-1e30, max_calls=1), None, False):  # a legal argument gets as far as the device question
        with pytest.raises(OrcaHipError, match="no CPU path"):
            C.scan_1m(None, codes, loops=ok, **kw)
    with pytest.raises(OrcaHipError, match="no CPU path"):
        C.scan_1m(None, codes, loops=True, depth=18, insulation=3, boundaries=True, strands="both", **kw)


def test_loop_positions():
    band = torch.zeros(4, 3)
    res = C.ScanResult(8_000, 4_000, np.array([0], np.int64), 4, 3, band, torch.ones(4, 3, dtype=torch.int32))
    with pytest.raises(ValueError, match="loops"):
        res.loop_positions()
    res.loops = (np.array([[0, 2], [1, 3]], dtype=np.int64), np.array([0.5, 0.25], dtype=np.float32))
    pos = res.loop_positions()
    assert pos.dtype == np.int64 and pos.tolist() == [[8_000, 16_000], [12_000, 20_000]]
    assert pos.tolist() == [[res.pos_of(i), res.pos_of(j)] for i, j in res.loops[0]]
    res.loops = (np.zeros((0, 2), np.int64), np.zeros(0, np.float32))
    assert res.loop_positions().shape == (0, 2)
