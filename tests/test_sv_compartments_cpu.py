"""Compartments per level of the SV screen, the numpy side (no GPU): `sv.eigenvectors_host` on planted spectra Q diag(8, -4, 2) Q^T + 0.02 noise /
sqrt(n) of which only the upper triangle is stored, its sign rule (a phase, an anti-correlated phase, the fallback), its NaN rule, `sv.gc_tracks_host`
on a hand-written code string, `sv.paired_compartment_scores_host` on three hand-made bin maps, `sv.check_compartments_arg` and the argument checks
of `sv_screen` / `sv_scores` (they raise before any device work)."""
import numpy as np
import pytest

from orca_amd import sv

LAM = (8.0, -4.0, 2.0)


def planted(n, seed, noise=0.02):
    """(the map with its lower triangle zeroed, Q): Q diag(LAM) Q^T + noise * randn / sqrt(n)"""
    rs = np.random.RandomState(seed)
    q, _ = np.linalg.qr(rs.randn(n, len(LAM)))
    m = (q * np.array(LAM)) @ q.T + noise * rs.randn(n, n) / np.sqrt(n)
    return np.triu(m).astype(np.float32), q


def pearson(x, y):
    ex, ey = x - x.mean(), y - y.mean()
    return (ex * ex).sum(), (ey * ey).sum(), (ex * ey).sum()


@pytest.mark.parametrize("n", [5, 17, 64, 250])
def test_planted_spectrum_is_recovered_from_the_upper_triangle(n):
    m, q = planted(n, n)
    got = sv.eigenvectors_host(m[None], n_eigs=3, d_lo=0, center=False)
    assert got["E"].dtype == np.float32 and got["E"].shape == (1, 3, n) and got["eigenvalue"].dtype == np.float64 and got["n_valid"].tolist() == [n]
    # the noise moves an eigenvalue by at most its spectral norm: |noise|_2 <= 2 * 0.02 (a Gaussian n x n matrix / sqrt(n) has norm -> 2), doubled
    assert np.abs(got["eigenvalue"][0] - np.array(LAM)).max() <= 0.08
    E = got["E"][0].astype(np.float64)
    low_rank = (q * np.array(LAM)) @ q.T
    # sum_k sign(lambda_k) E_k E_k^T is the rank-3 part of the stored matrix: within the noise's norm of the planted one (and E E^T within it of Q |L| Q^T)
    assert np.abs((E.T * np.sign(got["eigenvalue"][0])) @ E - low_rank).max() <= 0.08
    assert np.linalg.norm(E.T @ E - (q * np.abs(LAM)) @ q.T, 2) <= 0.16
    assert got["residual"].max() <= 1e-12                                 # eigh's pairs
    # the lower triangle is never read
    junk = m + np.tril(np.full((n, n), 7.0, dtype=np.float32), -1)
    again = sv.eigenvectors_host(junk[None], n_eigs=3, d_lo=0, center=False)
    assert all(np.array_equal(got[k], again[k], equal_nan=True) for k in got)


def test_band_and_centering_make_the_matrix():
    m, _ = planted(16, 3)
    A, valid = sv.compartment_matrix_host(m, d_lo=2, center=True)
    S = np.triu(m.astype(np.float64)) + np.triu(m.astype(np.float64), 1).T
    i, j = np.indices((16, 16))
    keep = np.abs(i - j) >= 2
    assert valid.all() and np.array_equal(A == 0.0, ~keep) and np.allclose(A[keep], S[keep] - S[keep].mean(), rtol=0, atol=1e-15)
    assert abs(A[keep].mean()) <= 1e-15 and np.array_equal(A, A.T)
    A0, _ = sv.compartment_matrix_host(m, d_lo=0, center=False)
    assert np.array_equal(A0, S)


def test_sign_rule_with_a_phase_an_anti_phase_and_the_fallback():
    n = 64
    m, _ = planted(n, 1)
    free = sv.eigenvectors_host(m[None], n_eigs=3)
    for k in range(3):                                                    # the fallback: the largest |E_k| is positive
        e = free["E"][0, k]
        assert e[np.argmax(np.abs(e))] > 0
    phase = np.random.RandomState(2).rand(1, n).astype(np.float32)
    phase[0, 5] = np.nan                                                  # a bin without a phase is left out of the correlation
    with_p, anti = sv.eigenvectors_host(m[None], n_eigs=3, phase=phase), sv.eigenvectors_host(m[None], n_eigs=3, phase=-phase)
    use = np.isfinite(phase[0])
    for k in range(3):
        e, a = with_p["E"][0, k].astype(np.float64), anti["E"][0, k].astype(np.float64)
        assert pearson(e[use], phase[0, use].astype(np.float64))[2] > 0 and pearson(a[use], -phase[0, use].astype(np.float64))[2] > 0
        assert np.array_equal(a, -e)                                      # the opposite phase: the opposite vector, the same bits otherwise
        assert np.array_equal(np.abs(e).astype(np.float32), np.abs(free["E"][0, k]))
    assert np.array_equal(with_p["eigenvalue"], free["eigenvalue"])
    # a constant phase has no correlation: the fallback; so has a phase with one finite bin
    flat = sv.eigenvectors_host(m[None], n_eigs=3, phase=np.ones((1, n), dtype=np.float32))
    lone = np.full((1, n), np.nan, dtype=np.float32)
    lone[0, 9] = 1.0
    assert np.array_equal(flat["E"], free["E"]) and np.array_equal(sv.eigenvectors_host(m[None], n_eigs=3, phase=lone)["E"], free["E"])
    # the fallback's tie: two components of equal size, the LOWER index is made positive
    t = np.zeros((1, 4, 4), dtype=np.float32)
    t[0, 0, 3] = 1.0
    t[0, 1, 2] = 0.5
    e = sv.eigenvectors_host(t, n_eigs=2, d_lo=0, center=False)           # eigenvalues +-1 (bins 0, 3) and +-0.5: eigh orders -1, 1 or 1, -1 by |.|, stably
    for k in range(2):
        assert abs(e["E"][0, k, 0]) == abs(e["E"][0, k, 3]) and e["E"][0, k, 0] > 0 and np.all(e["E"][0, k, 1:3] == 0)
    assert sorted(e["eigenvalue"][0].tolist()) == [-1.0, 1.0]


def test_one_nan_pixel_invalidates_its_two_bins():
    m, _ = planted(64, 1)
    m[3, 40] = np.nan
    A, valid = sv.compartment_matrix_host(m)
    assert np.flatnonzero(~valid).tolist() == [3, 40] and not np.isnan(A).any() and not A[3].any() and not A[:, 40].any()
    got = sv.eigenvectors_host(m[None], n_eigs=2)
    assert got["n_valid"].tolist() == [62]
    assert np.flatnonzero(np.isnan(got["E"][0, 0])).tolist() == [3, 40] and np.flatnonzero(np.isnan(got["E"][0, 1])).tolist() == [3, 40]
    assert np.isfinite(got["eigenvalue"]).all()
    inside = m.copy()
    inside[3, 40] = 1.0
    inside[7, 8] = np.nan                                                 # |i - j| = 1 < d_lo: not a kept pixel, nobody is invalid
    inside[50, 10] = np.nan                                               # below the diagonal: never read
    assert sv.eigenvectors_host(inside[None], n_eigs=1)["n_valid"].tolist() == [64]
    assert sv.eigenvectors_host(inside[None], n_eigs=1, d_lo=1)["n_valid"].tolist() == [62]


def test_too_few_valid_bins_give_nan():
    m, _ = planted(5, 5)
    m[0, 1:] = np.nan                                                     # bin 0 and, through the symmetry, bins 1 .. 4: S[j][0] is NaN
    got = sv.eigenvectors_host(m[None], n_eigs=1, d_lo=0, center=False)
    assert got["n_valid"].tolist() == [0] and np.isnan(got["E"]).all() and np.isnan(got["eigenvalue"]).all() and np.isnan(got["residual"]).all()
    m, _ = planted(5, 5)
    m[0, 4] = np.nan                                                      # 3 valid bins
    three = sv.eigenvectors_host(m[None], n_eigs=3, d_lo=0, center=False)
    assert three["n_valid"].tolist() == [3] and np.isnan(three["E"]).all() and np.isnan(three["eigenvalue"]).all()
    two = sv.eigenvectors_host(m[None], n_eigs=2, d_lo=0, center=False)
    assert two["n_valid"].tolist() == [3] and np.isfinite(two["eigenvalue"]).all() and np.isfinite(two["E"][0][:, 1:4]).all()


def test_gc_tracks_on_a_hand_written_string():
    codes = np.array([1, 2, 0, 3,   4, 4, 4, 4,   2, 2, 4, 0,   4, 1, 4, 4,   0, 0, 3, 3,   1], dtype=np.uint8)     # C G A T | N N N N | G G N A | N C N N | A A T T | C
    got = sv.gc_tracks_host(codes, [0, 1, 16], [4, 2, 1], 5)
    assert got.dtype == np.float32 and got.shape == (3, 5)
    assert np.array_equal(got[0], np.array([0.5, np.nan, 2 / 3, 1.0, 0.0], dtype=np.float32), equal_nan=True)       # an all-N bin is NaN, N runs do not count
    assert np.array_equal(got[1], np.array([0.5, 0.0, np.nan, 1.0, 1.0], dtype=np.float32), equal_nan=True)         # G A | T N | N N | N G | G N
    assert np.array_equal(got[2], np.array([0.0, 0.0, 0.0, 0.0, 1.0], dtype=np.float32))
    assert got[0, 2] == np.float32(2.0 / 3.0)                             # one fp64 division, rounded once
    for off, bs in ((-1, 2), (0, 5), (18, 1), (0, 0)):
        with pytest.raises(ValueError):
            sv.gc_tracks_host(codes, [off], [bs], 5)


def test_paired_scores_through_three_bin_maps():
    n = 8
    ref = np.array([[1.0, 2.0, -1.0, -2.0, 3.0, np.nan, -3.0, 4.0]], dtype=np.float32)
    jump = np.array([0, 1, 2, 5, 6, 7, -1, -1])                           # a deletion of reference bins 3, 4; two unmapped bins behind
    twice = np.array([0, 1, 2, 2, 3, 4, -1, 6])                           # a duplication: bin 2 twice
    down = np.array([0, 6, 4, 3, 2, 1, -1, 7])                            # an inversion: 6 .. 1 descending (5 would be NaN in ref: left unmapped)
    for bm in (jump, twice, down):
        M = np.flatnonzero(bm >= 0)
        alt = np.full((1, n), np.nan, dtype=np.float32)
        alt[0, M] = ref[0, bm[M]]                                         # the alt vector IS the reference's, through the map
        same = sv.paired_compartment_scores_host(alt[None], ref[None], bm)
        assert same["delta"].dtype == np.float32 and same["delta"].shape == (1, 1, n) and same["corr"].dtype == np.float64 and same["flips"].dtype == np.int32
        fin = M[np.isfinite(ref[0, bm[M]])]
        assert np.flatnonzero(~np.isnan(same["delta"][0, 0])).tolist() == fin.tolist() and not same["delta"][0, 0, fin].any()
        assert same["corr"][0, 0] == pytest.approx(1.0, abs=1e-15) and same["flips"][0, 0] == 0
        flipped = sv.paired_compartment_scores_host(-alt[None], ref[None], bm)
        assert flipped["corr"][0, 0] == pytest.approx(-1.0, abs=1e-15) and flipped["flips"][0, 0] == fin.size
        assert np.array_equal(flipped["delta"][0, 0, fin], -2 * ref[0, bm[fin]])
    # by hand, through the deletion's map: pairs (alt bin -> ref bin) 0->0, 1->1, 2->2, 3->5 (NaN in ref), 4->6, 5->7
    alt = np.array([[1.5, -2.0, -1.0, 9.0, -3.0, np.nan, 5.0, 5.0]], dtype=np.float32)
    got = sv.paired_compartment_scores_host(alt[None], ref[None], jump)
    want = np.array([0.5, -4.0, 0.0, np.nan, 0.0, np.nan, np.nan, np.nan], dtype=np.float32)
    assert np.array_equal(got["delta"][0, 0], want, equal_nan=True)
    x, y = np.array([1.5, -2.0, -1.0, -3.0]), np.array([1.0, 2.0, -1.0, -3.0])       # both finite: alt bins 0, 1, 2, 4
    X, Y, C = pearson(x, y)
    assert got["corr"][0, 0] == pytest.approx(C / np.sqrt(X * Y), abs=1e-15) and got["flips"][0, 0] == 1
    # below 2 pairs, and a map with no mapped bin: no correlation
    for bm, flips in ((np.array([3, -1, -1, -1, -1, -1, -1, -1]), 1), (np.full(n, -1), 0)):      # the one pair: 1.5 against -2.0
        none = sv.paired_compartment_scores_host(alt[None], ref[None], bm)
        assert np.isnan(none["corr"]).all() and none["flips"][0, 0] == flips and np.isnan(none["delta"][0, 0, 1:]).all()
    with pytest.raises(ValueError):
        sv.paired_compartment_scores_host(alt[None], ref[None], np.full(n, n))


def test_check_compartments_arg():
    Q = sv.CompartmentParams
    assert sv.check_compartments_arg(None) is None and sv.check_compartments_arg(False) is None
    assert sv.check_compartments_arg(True) == Q(1, 2, True, 1e-8, 1000) == Q()
    q = sv.check_compartments_arg(Q(n_eigs=np.int64(3), d_lo=0, center=np.bool_(False), tol=1, max_iter=np.int32(7)))
    assert q == Q(3, 0, False, 1.0, 7) and type(q.n_eigs) is int and type(q.center) is bool and type(q.tol) is float and type(q.max_iter) is int
    assert sv.check_compartments_arg(Q(d_lo=249)).d_lo == 249 and sv.check_compartments_arg(Q(d_lo=3), n=4).d_lo == 3
    bad = [Q(n_eigs=0), Q(n_eigs=4), Q(n_eigs=1.0), Q(n_eigs=True), Q(d_lo=-1), Q(d_lo=250), Q(d_lo=2.0), Q(center=1), Q(center=None), Q(tol=0.0),
           Q(tol=-1e-8), Q(tol=float("nan")), Q(tol=float("inf")), Q(tol="x"), Q(tol=True), Q(max_iter=0), Q(max_iter=10.0), (1, 2, True, 1e-8, 1000), 1,
           "yes", {"n_eigs": 1}]
    for b in bad:
        with pytest.raises(ValueError):
            sv.check_compartments_arg(b)
    with pytest.raises(ValueError):
        sv.check_compartments_arg(Q(d_lo=4), n=4)


def test_the_screen_and_the_scores_check_their_arguments_before_any_device_work():
    v = [sv.SV("del", 18_000_000, 19_200_000)]
    with pytest.raises(ValueError, match="scores=True"):
        sv.sv_screen(None, None, v, 40_000_000, compartments=True)
    with pytest.raises(ValueError, match="n_eigs"):
        sv.sv_screen(None, None, v, 40_000_000, scores=True, compartments=sv.CompartmentParams(n_eigs=4))
    with pytest.raises(ValueError, match="compartments"):
        sv.sv_screen(None, None, v, 40_000_000, scores=True, compartments="E1")
    with pytest.raises(ValueError, match="tol"):
        sv.sv_scores(v[0], None, None, 40_000_000, compartments=sv.CompartmentParams(tol=0))
    with pytest.raises(ValueError, match="phase"):
        sv.sv_scores(v[0], None, None, 40_000_000, phase=(np.zeros((6, 250)), np.zeros((6, 250))))
    with pytest.raises(ValueError, match="phase"):
        sv.sv_scores(v[0], None, None, 40_000_000, compartments=True, phase=np.zeros((6, 250)))
