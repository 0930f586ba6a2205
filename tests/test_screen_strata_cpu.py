"""`screen.strata_scores_host` and `screen.check_strata` without a GPU: the host restatement of orca_screen_strata_scores against independent numpy
(`np.diagonal`, `np.corrcoef`, `np.var`) on random fp32 maps, with and without hand-made bin maps, and the rules of the definition: a constant
stratum, a stratum of fewer than two pairs, no pair at all, where a NaN pixel shows, and the identity bin map giving the bin-with-bin arrays."""
import numpy as np
import pytest

from orca_amd import screen as S

PER_STRATUM = ("dist_delta", "dist_abs", "dist_rms", "dist_corr")
PER_MAP = ("mse", "corr", "scc")


def maps_of(n, E=3, seed=0):
    rs = np.random.RandomState(seed + n)
    return rs.randn(E, n, n).astype(np.float32), rs.randn(n, n).astype(np.float32)


def bin_maps(n):
    i = np.arange(n)
    k = max(1, n // 5)
    return {"identity": i, "deletion": np.where(i < n // 3, i, np.where(i + k < n, i + k, -1)), "duplicate": np.maximum(i - 1, 0), "none": np.full(n, -1)}


def pairs_of(a, r, m, d):
    """x, y of stratum d by the definition, as lists in ascending i"""
    n = r.shape[0]
    idx = [i for i in range(n - d) if m is None or (m[i] >= 0 and m[i + d] >= 0)]
    x = np.array([a[i, i + d] for i in idx], dtype=np.float64)
    y = np.array([r[i, i + d] if m is None else r[m[i], m[i + d]] for i in idx], dtype=np.float64)
    return x, y


def independent(a, r, m, lo, hi):
    """the scores of one map from numpy's own mean, var and corrcoef"""
    n = r.shape[0]
    out = {k: np.full(n, np.nan) for k in PER_STRATUM}
    cnt = np.zeros(n, dtype=np.int64)
    num = den = 0.0
    xs, ys = [], []
    for d in range(n):
        x, y = pairs_of(a, r, m, d)
        cnt[d] = x.size
        if x.size == 0:
            continue
        out["dist_delta"][d], out["dist_abs"][d], out["dist_rms"][d] = (x - y).mean(), np.abs(x - y).mean(), np.sqrt(((x - y) ** 2).mean())
        if x.size >= 2 and x.var() > 0 and y.var() > 0:
            out["dist_corr"][d] = np.corrcoef(x, y)[0, 1]
        if lo <= d < hi:
            xs.append(x)
            ys.append(y)
            if x.size >= 2 and x.var() > 0 and y.var() > 0:                      # HiCRep: weights c_d sqrt(var_x var_y) on the strata's correlations
                w = x.size * np.sqrt(x.var() * y.var())
                num += w * np.corrcoef(x, y)[0, 1]
                den += w
    x, y = (np.concatenate(v) if v else np.zeros(0) for v in (xs, ys))
    out["mse"] = ((x - y) ** 2).mean() if x.size else np.nan
    out["corr"] = np.corrcoef(x, y)[0, 1] if x.size >= 2 and x.var() > 0 and y.var() > 0 else np.nan
    out["scc"] = num / den if den > 0 else np.nan
    out["dist_count"] = cnt
    return out


def close(got, want, tol, what):
    g, w = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert g.shape == w.shape and np.array_equal(np.isnan(g), np.isnan(w)), (what, g, w)
    f = ~np.isnan(w)
    assert np.all(np.abs(g[f] - w[f]) <= tol * np.maximum(1.0, np.abs(w[f]))), (what, np.abs(g[f] - w[f]).max())


@pytest.mark.parametrize("n", [1, 2, 3, 50])
def test_host_restatement_equals_independent_numpy(n):
    alt, ref = maps_of(n)
    ranges = [None, (0, n)] + ([(1, n - 1), (n // 2, n // 2 + 1)] if n >= 3 else [])
    for name, m in [("bin with bin", None)] + list(bin_maps(n).items()):
        for rg in ranges:
            got = S.strata_scores_host(alt, ref, m, rg)
            lo, hi = (0, n) if rg is None else rg
            for e in range(alt.shape[0]):
                want = independent(alt[e], ref, m, lo, hi)
                for k in PER_STRATUM + PER_MAP:
                    assert got[k].dtype == np.float64
                    close(got[k][e], want[k], 1e-9 if "corr" in k or k == "scc" else 1e-12, (n, name, rg, e, k))
                assert got["dist_count"].dtype == np.int32 and np.array_equal(got["dist_count"][e], want["dist_count"]), (n, name)
    # the means and the rms straight from np.diagonal
    got = S.strata_scores_host(alt, ref)
    for e in range(alt.shape[0]):
        for d in range(n):
            dl = np.diagonal(alt[e].astype(np.float64) - ref.astype(np.float64), d)
            close(got["dist_delta"][e, d], dl.mean(), 1e-12, (n, d))
            close(got["dist_rms"][e, d], np.sqrt((dl * dl).mean()), 1e-12, (n, d))
            assert got["dist_count"][e, d] == n - d
    # one [n] bin map for all maps is the [E, n] one repeated
    m = bin_maps(n)["deletion"]
    one, rep = S.strata_scores_host(alt, ref, m), S.strata_scores_host(alt, ref, np.repeat(m[None], alt.shape[0], axis=0))
    assert all(np.array_equal(one[k], rep[k], equal_nan=True) for k in one)


def test_identity_bin_map_gives_the_bin_with_bin_arrays_exactly():
    for n in (1, 2, 3, 50):
        alt, ref = maps_of(n, seed=3)
        plain, ident = S.strata_scores_host(alt, ref, None, (0, n)), S.strata_scores_host(alt, ref, np.arange(n), (0, n))
        for k in PER_STRATUM + PER_MAP + ("dist_count",):
            assert np.array_equal(plain[k].view(np.uint64 if plain[k].dtype == np.float64 else np.int32),
                                  ident[k].view(np.uint64 if ident[k].dtype == np.float64 else np.int32)), (n, k)


def test_constant_stratum_few_pairs_and_no_pairs():
    n = 50
    alt, ref = maps_of(n, seed=5)
    ref = ref.copy()
    i = np.arange(n - 7)
    ref[i, i + 7] = np.float32(0.3)                                               # stratum 7 constant in ref: Y_7 is exactly 0.0
    alt = alt.copy()
    j = np.arange(n - 9)
    alt[1, j, j + 9] = np.float32(-1.7)                                           # and stratum 9 constant in alt map 1
    got = S.strata_scores_host(alt, ref)
    assert np.isnan(got["dist_corr"][:, 7]).all() and np.isnan(got["dist_corr"][1, 9]) and np.isfinite(got["dist_corr"][0, 9])
    assert np.isnan(got["dist_corr"][:, n - 1]).all() and np.isfinite(got["dist_corr"][:, n - 2]).all()           # c_d = 1 and c_d = 2
    assert np.isfinite(got["dist_delta"]).all() and np.isfinite(got["scc"]).all() and np.isfinite(got["corr"]).all()
    want = independent(alt[1], ref, None, 0, n)                                  # the constant strata weigh nothing in the SCC
    close(got["scc"][1], want["scc"], 1e-9, "scc")
    only = S.strata_scores_host(alt, ref, None, (7, 8))                          # only the constant stratum: denominator 0.0, Y = 0.0
    assert np.isnan(only["scc"]).all() and np.isnan(only["corr"]).all() and np.isfinite(only["mse"]).all()
    last = S.strata_scores_host(alt, ref, None, (n - 1, n))                      # c = 1
    assert np.isnan(last["scc"]).all() and np.isnan(last["corr"]).all()
    close(last["mse"], (alt[:, 0, n - 1].astype(np.float64) - float(ref[0, n - 1])) ** 2, 1e-12, "mse of one pair")
    # a map equal to the reference: every difference exactly 0, X_d = Y_d = C_d to the bit, so a stratum's correlation is 1 up to the rounding of
    # the product and the root, and the SCC up to that of its two sums of n terms
    same = S.strata_scores_host(ref[None], ref)
    assert np.all(same["dist_delta"] == 0) and np.all(same["dist_rms"] == 0) and same["mse"][0] == 0
    f = ~np.isnan(same["dist_corr"][0])
    assert np.all(np.abs(same["dist_corr"][0][f] - 1.0) <= 4 * 2.0 ** -53) and abs(same["scc"][0] - 1.0) <= 2 * n * 2.0 ** -53
    # no pair at all
    none = S.strata_scores_host(alt, ref, np.full(n, -1))
    assert all(np.isnan(none[k]).all() for k in PER_STRATUM + PER_MAP) and not none["dist_count"].any()
    # a deletion of bins 10 .. 19: strata 30 .. 39 keep pairs, 40 .. 49 have none; a range of empty strata gives c = 0
    k = np.arange(n)
    dele = np.where(k < 10, k, np.where(k + 10 < n, k + 10, -1))
    got = S.strata_scores_host(alt, ref, dele, (40, 50))
    assert got["dist_count"][0].tolist() == [max(0, 40 - d) for d in range(n)]
    assert all(np.isnan(got[k_]).all() for k_ in PER_MAP) and np.isnan(got["dist_delta"][:, 40:]).all() and np.isfinite(got["dist_delta"][:, :40]).all()


def nan_sets(out):
    return {k: np.argwhere(np.isnan(out[k])).tolist() for k in PER_STRATUM + PER_MAP}


@pytest.mark.parametrize("rg", [(0, 50), (0, 8), (9, 50), (8, 9)])
def test_nan_rule(rg):
    """a NaN at a pair of P_d: every output of stratum d, and the three per-map scores if d_lo <= d < d_hi; nothing else"""
    n = 50
    alt, ref = maps_of(n, E=2, seed=9)
    k = np.arange(n)
    dele = np.where(k < 10, k, np.where(k + 10 < n, k + 10, -1))                  # alt bins 40 .. 49 unmapped
    for m in (None, dele):
        clean = S.strata_scores_host(alt, ref, m, rg)
        a2, r2 = alt.copy(), ref.copy()
        a2[:, 20, 12] = np.nan                                                    # below the diagonal
        r2[30, 3] = np.nan
        if m is not None:
            a2[0, 5, 45] = np.nan                                                 # an unmapped pair
            r2[12, 14] = np.nan                                                   # reference bins 10 .. 19 stand behind no alt bin
        quiet = S.strata_scores_host(a2, r2, m, rg)
        assert all(np.array_equal(clean[f], quiet[f], equal_nan=True) for f in clean)
        a3 = alt.copy()
        a3[1, 12, 20] = np.nan                                                    # stratum 8 of map 1, a mapped pair under both maps
        got = S.strata_scores_host(a3, ref, m, rg)
        want = nan_sets(clean)
        for f in PER_STRATUM:
            want[f] = sorted(want[f] + [[1, 8]])
        if rg[0] <= 8 < rg[1]:
            for f in PER_MAP:
                want[f] = sorted(want[f] + [[1]])
        assert nan_sets(got) == want, (rg, m is None)
        for f in PER_STRATUM + PER_MAP:                                           # and every other value keeps its bits
            keep = ~np.isnan(got[f])
            assert np.array_equal(got[f][keep], clean[f][keep]), f
        r3 = ref.copy()
        r3[12, 20] = np.nan                                                       # the reference pixel: every map's stratum 8 bin with bin;
        got = S.strata_scores_host(alt, r3, m, rg)                                # aligned, reference (12, 20) stands behind no alt pair
        hit = [[e, 8] for e in range(2)] if m is None else []
        assert nan_sets(got)["dist_delta"] == sorted(nan_sets(clean)["dist_delta"] + hit)


def test_check_strata():
    assert S.check_strata(True, 50) == (0, 50) and S.check_strata((0, 50), 50) == (0, 50) and S.check_strata([3, 4], 50) == (3, 4)
    assert S.check_strata((np.int64(2), np.int32(9)), 50) == (2, 9)
    for bad in ((0, 51), (-1, 5), (5, 5), (6, 5), (50, 51), (0, 0)):
        with pytest.raises(ValueError):
            S.check_strata(bad, 50)
    for bad in (False, None, 5, "ab", (1,), (1, 2, 3), (0.5, 3), (0, 2.5), (True, 5), ("a", "b")):
        with pytest.raises(ValueError):
            S.check_strata(bad, 50)
    with pytest.raises(ValueError):
        S.strata_scores_host(np.zeros((1, 4, 4)), np.zeros((4, 4)), None, (0, 5))
    with pytest.raises(ValueError):
        S.strata_scores_host(np.zeros((1, 4, 4)), np.zeros((4, 4)), np.array([0, 1, 2, 4]))
    with pytest.raises(ValueError):
        S.strata_scores_host(np.zeros((1, 4, 3)), np.zeros((4, 4)))
