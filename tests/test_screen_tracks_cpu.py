"""The tracks of the 1 Mb mutagenesis screen on the host (no GPU): the fp64 restatements `screen.insulation_host`, `insulation_scores_host` and
`viewpoint_scores_host` against sums written out by hand, where the diamond fits, the aligned forms on a deletion's bin map, and the argument
checks `check_insulation` / `check_viewpoints`."""
import numpy as np
import pytest

from orca_amd import screen as S

M5 = np.array([[1, 2, 3, 4, 5],
               [6, 7, 8, 9, 10],
               [11, 12, 13, 14, 15],
               [16, 17, 18, 19, 20],
               [21, 22, 23, 24, 26]], dtype=np.float32)


def deletion_map(n=50):
    """bins 10 .. 14 deleted: the alt map closes up, the refill at its end is unmapped (the map of test_rectangles_in_reference_bins)"""
    i = np.arange(n)
    return np.where(i < 10, i, np.where(i + 5 < n, i + 5, -1))


def test_insulation_by_explicit_sums():
    t = S.insulation_host(M5[None], (1, 2))
    assert t.shape == (1, 2, 5) and t.dtype == np.float64
    # w = 1: the one pixel (i - 1, i + 1); bins 0 and 4 have no diamond
    assert np.array_equal(t[0, 0], [np.nan, 3.0, 9.0, 15.0, np.nan], equal_nan=True)
    # w = 2: rows 0, 1 x columns 3, 4 at bin 2, nothing else fits
    assert np.array_equal(t[0, 1], [np.nan, np.nan, (4 + 5 + 9 + 10) / 4.0, np.nan, np.nan], equal_nan=True)
    assert np.array_equal(S.insulation_host(M5[None], 1), t[:, :1], equal_nan=True)         # an int is one width
    # the lower triangle and the diagonal are never read
    m = M5.copy()
    m[np.tril_indices(5)] = np.nan
    assert np.array_equal(S.insulation_host(m[None], (1, 2)), t, equal_nan=True)
    # a NaN pixel shows in the bins whose diamond holds it and in no other: (1, 3) is in bin 2's diamond at w = 1 and w = 2
    m = M5.copy()
    m[1, 3] = np.nan
    u = S.insulation_host(m[None], (1, 2))
    assert np.isnan(u[0, :, 2]).all() and np.array_equal(u[0, 0, [1, 3]], [3.0, 15.0])


@pytest.mark.parametrize("n", [1, 3, 50, 250, 256])
def test_the_diamond_fits_at_n_minus_2w_bins(n):
    m = np.random.RandomState(n).randn(1, n, n).astype(np.float32)
    for w in (1, 2, 25, (n - 1) // 2):
        if w < 1:
            continue
        t = S.insulation_host(m, [w])[0, 0]
        assert int(np.isfinite(t).sum()) == max(0, n - 2 * w), (n, w)
        assert np.array_equal(np.flatnonzero(np.isfinite(t)), np.arange(w, n - w)), (n, w)
    if n % 2 == 0:
        assert int(np.isfinite(S.insulation_host(m, [(n - 1) // 2])).sum()) == 2         # the largest legal width on an even map
    w = (n - 1) // 2
    if w >= 1:                                                                          # one bin by hand, mean of the w x w block
        i = w
        want = m[0, :w, i + 1: i + 1 + w].astype(np.float64).sum() / (w * w)
        assert abs(S.insulation_host(m, [w])[0, 0, i] - want) <= 1e-12, (n, w)             # fp64 sums of at most 16 129 terms, in whatever order


def test_insulation_scores_bin_with_bin_and_aligned():
    n, w = 50, 3
    rs = np.random.RandomState(3)
    alt, ref = rs.randn(2, n, n).astype(np.float32), rs.randn(n, n).astype(np.float32)
    tr, dl, al = S.insulation_scores_host(alt, ref, [w])
    assert al is None and tr.shape == dl.shape == (2, 1, n)
    ia, ir = S.insulation_host(alt, [w]), S.insulation_host(ref[None], [w])
    assert np.array_equal(tr, ia, equal_nan=True) and np.array_equal(dl, ia - ir, equal_nan=True)
    # the deletion: alt bin i stands for reference bin i (i < 10) or i + 5; both diamonds must fit, the centre must be mapped
    bm = deletion_map(n)
    tr2, dl2, al = S.insulation_scores_host(alt, ref, [w], bm)
    assert np.array_equal(tr2, tr, equal_nan=True) and np.array_equal(dl2, dl, equal_nan=True)
    assert np.array_equal(np.flatnonzero(np.isfinite(al[0, 0])), np.arange(3, 42))
    assert np.array_equal(np.flatnonzero(np.isfinite(al[1, 0])), np.arange(3, 42))
    for i in (3, 9, 10, 41):
        r = int(bm[i])
        want = alt[0, i - w: i, i + 1: i + 1 + w].astype(np.float64).sum() / 9 - ref[r - w: r, r + 1: r + 1 + w].astype(np.float64).sum() / 9
        assert abs(al[0, 0, i] - want) <= 1e-15 * 9, i
    # per-item maps; the identity gives the bin-with-bin difference, the same expression
    ident = np.arange(n)
    tr3, dl3, al3 = S.insulation_scores_host(alt, ref, (1, w, 24), np.stack([ident, bm]))
    assert np.array_equal(al3[0], dl3[0], equal_nan=True) and not np.array_equal(al3[1], dl3[1], equal_nan=True)
    assert np.array_equal(al3[1, 1], al[1, 0], equal_nan=True)
    # a width that fits nowhere, and an unmapped map
    assert np.isnan(S.insulation_host(alt, [25])).all()
    assert np.isnan(S.insulation_scores_host(alt, ref, [w], np.full(n, -1))[2]).all()
    with pytest.raises(ValueError):
        S.insulation_scores_host(alt, ref, [w], np.full(n, n))


def test_viewpoint_scores():
    n = 50
    rs = np.random.RandomState(4)
    alt, ref = rs.randn(2, n, n).astype(np.float32), rs.randn(n, n).astype(np.float32)
    views = [0, 12, 20, 49]
    dl, al = S.viewpoint_scores_host(alt, ref, views)
    assert al is None and dl.dtype == np.float32 and dl.shape == (2, 4, n)
    assert np.array_equal(dl, alt[:, views] - ref[views][None])
    # item 0: the deletion (reference bin 12 is gone; 20 sits at alt bin 15; alt columns 45 .. 49 stand for nothing).  item 1: an insertion
    # next to bin 10 leaves alt bins 10 and 11 both standing for reference bin 10, and pushes bin 49 out
    i = np.arange(n)
    dup = np.where(i <= 10, i, i - 1)
    bm = np.stack([deletion_map(n), dup])
    dl2, al = S.viewpoint_scores_host(alt, ref, [12, 20, 10, 49], bm)
    assert al.dtype == np.float32 and al.shape == (2, 4, n)
    assert np.isnan(al[0, 0]).all()                                                      # the viewpoint was deleted
    cols = np.arange(45)
    assert np.isnan(al[0, 1, 45:]).all()                                                 # a -1 column
    assert np.array_equal(al[0, 1, cols], alt[0, 15, cols] - ref[20, bm[0, cols]])        # c = 1: the fp32 subtraction
    want = (alt[1, 10].astype(np.float64) + alt[1, 11].astype(np.float64)) / 2.0 - ref[10, dup].astype(np.float64)
    assert np.array_equal(al[1, 2], want.astype(np.float32))                             # two alt bins: the mean of their rows
    assert np.isnan(al[1, 3]).all() and np.isnan(al[0, 3, 45:]).all()                    # pushed out; reference 49 sits at alt 44 in item 0
    assert np.array_equal(al[0, 3, cols], alt[0, 44, cols] - ref[49, bm[0, cols]])
    # the identity map gives the bin-with-bin difference
    _, al_id = S.viewpoint_scores_host(alt, ref, views, np.arange(n))
    assert np.array_equal(al_id, dl)


def test_check_insulation():
    assert S.check_insulation(5, 50).tolist() == [5] and S.check_insulation((1, 3, 24), 50).dtype == np.int32
    assert S.check_insulation(range(1, 9), 50).tolist() == list(range(1, 9))
    assert S.check_insulation([127], 256).tolist() == [127] and S.check_insulation([1], 3).tolist() == [1]
    for bad, n in (([], 50), (range(1, 10), 50), ((3, 5, 3), 50), (0, 50), ([2, 0], 50), (25, 50), ([128], 256), (1, 2), (1, 1), ("x", 50), (None, 50),
                   (-1, 50)):
        with pytest.raises(ValueError):
            S.check_insulation(bad, n)


def test_check_viewpoints():
    assert S.check_viewpoints([0, 49, 12, 12], 50).tolist() == [0, 49, 12, 12] and S.check_viewpoints(range(64), 64).dtype == np.int32
    for bad, n in (([], 50), ([50], 50), ([-1], 50), (list(range(65)), 250), (7, 50), (["a"], 50), (None, 50)):
        with pytest.raises(ValueError):
            S.check_viewpoints(bad, n)
