"""The numpy restatements of the SV screen's readouts per level (`sv.paired_insulation_host`, `sv.paired_viewpoints_host`,
`sv.paired_strata_host`), `sv.viewpoint_bins` and the argument checks, without a GPU: against naive loops written from the definitions on
hand-made 12 x 12 and 30 x 30 maps, against the 1 Mb screen's restatements pair by pair where the bin map does not descend, and the min/max
rule of the strata on a descending map with a NON-symmetric reference."""
import numpy as np
import pytest

from orca_amd import screen as S
from orca_amd import sv
from tests.test_gpu_screen_aligned import kernel_maps

STRATA = ("dist_delta", "dist_abs", "dist_rms", "dist_corr", "mse", "corr", "scc")


def all_maps(n):
    return dict(kernel_maps(n), descending=np.arange(n)[::-1].copy())


def pairs(n, B, seed):
    rs = np.random.RandomState(seed)
    return rs.randn(B, n, n).astype(np.float32), rs.randn(B, n, n).astype(np.float32)


def same(x, y, exact=False):
    """equal with NaN in the same places; ``exact``: to the bit, else to 1e-12 of the larger magnitude (another order of the same fp64 terms)"""
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    if x.shape != y.shape or not np.array_equal(np.isnan(x), np.isnan(y)):
        return False
    f = ~np.isnan(x)
    return np.array_equal(x[f], y[f]) if exact else bool(np.all(np.abs(x[f] - y[f]) <= 1e-12 * np.maximum(1.0, np.abs(y[f]))))


def naive_ins(m, w, i):
    n = m.shape[0]
    if not w <= i < n - w:
        return np.nan
    return sum(float(m[r, c]) for r in range(i - w, i) for c in range(i + 1, i + w + 1)) / (w * w)


@pytest.mark.parametrize("n", [12, 30])
def test_insulation_and_viewpoints_equal_naive_loops(n):
    maps = all_maps(n)
    names = list(maps)
    alt, ref = pairs(n, len(names), n)
    bm = np.stack([maps[k] for k in names])
    widths = [1, 2, 5]
    track, ref_track, aligned = sv.paired_insulation_host(alt, ref, widths, bm)
    assert track.shape == ref_track.shape == aligned.shape == (len(names), 3, n)
    for b in range(len(names)):
        for k, w in enumerate(widths):
            for i in range(n):
                ia, ir = naive_ins(alt[b], w, i), naive_ins(ref[b], w, i)
                assert same(track[b, k, i], ia) and same(ref_track[b, k, i], ir)
                mi = bm[b, i]
                want = ia - naive_ins(ref[b], w, mi) if mi >= 0 else np.nan
                assert same(aligned[b, k, i], want), (names[b], w, i)
    views = np.stack([[-1, 0, n - 1, n // 2, 1]] * len(names))
    got, count = sv.paired_viewpoints_host(alt, ref, views, bm)
    assert got.dtype == np.float32 and count.dtype == np.int32 and got.shape == (len(names), 5, n) and count.shape == (len(names), 5)
    for b in range(len(names)):
        for k, v in enumerate(views[b]):
            R = [i for i in range(n) if v >= 0 and bm[b, i] == v]
            assert count[b, k] == len(R)
            for j in range(n):
                if not R or bm[b, j] < 0:
                    assert np.isnan(got[b, k, j])
                elif len(R) == 1:
                    assert got[b, k, j] == alt[b, R[0], j] - ref[b, v, bm[b, j]]
                else:
                    want = sum(float(alt[b, i, j]) for i in R) / len(R) - float(ref[b, v, bm[b, j]])
                    assert got[b, k, j] == np.float32(want)
    d = names.index("duplicate")
    assert count[d].tolist() == [0, 2, 0, 1, 1] and count[names.index("descending")].tolist() == [0, 1, 1, 1, 1]
    assert not count[names.index("none")].any() and np.isnan(got[names.index("none")]).all()


def naive_strata(a, r, bm, lo, hi):
    n = a.shape[0]
    out = {k: np.full(n, np.nan) for k in STRATA[:4]}
    cnt = np.zeros(n, dtype=np.int32)
    per = {}
    for d in range(n):
        xy = []
        for i in range(n - d):
            mi, mj = bm[i], bm[i + d]
            if mi >= 0 and mj >= 0:
                xy.append((float(a[i, i + d]), float(r[min(mi, mj), max(mi, mj)])))
        cnt[d] = c = len(xy)
        if c == 0:
            continue
        x, y = np.array(xy).T
        ex, ey, dl = x - x.mean(), y - y.mean(), x - y
        per[d] = (c, x, y)
        out["dist_delta"][d], out["dist_abs"][d], out["dist_rms"][d] = dl.mean(), np.abs(dl).mean(), np.sqrt((dl * dl).mean())
        X, Y, C = (ex * ex).sum(), (ey * ey).sum(), (ex * ey).sum()
        if c >= 2 and X != 0 and Y != 0:
            out["dist_corr"][d] = C / np.sqrt(X * Y)
    ds = [d for d in range(lo, hi) if d in per]
    out.update(mse=np.nan, corr=np.nan, scc=np.nan, dist_count=cnt)
    if ds:
        x, y = np.concatenate([per[d][1] for d in ds]), np.concatenate([per[d][2] for d in ds])
        out["mse"] = ((x - y) ** 2).mean()
        ex, ey = x - x.mean(), y - y.mean()
        if x.size >= 2 and (ex * ex).sum() != 0 and (ey * ey).sum() != 0:
            out["corr"] = (ex * ey).sum() / np.sqrt((ex * ex).sum() * (ey * ey).sum())        # the plain Pearson correlation over the pooled pairs
        num = sum(((per[d][1] - per[d][1].mean()) * (per[d][2] - per[d][2].mean())).sum() for d in ds)
        den = sum(np.sqrt(((per[d][1] - per[d][1].mean()) ** 2).sum() * ((per[d][2] - per[d][2].mean()) ** 2).sum()) for d in ds)
        if den != 0:
            out["scc"] = num / den
    return out


@pytest.mark.parametrize("n", [12, 30])
def test_strata_equal_naive_loops(n):
    maps = all_maps(n)
    names = list(maps)
    alt, ref = pairs(n, len(names), 7 * n)
    bm = np.stack([maps[k] for k in names])
    for rng in (None, (2, n - 3)):
        got = sv.paired_strata_host(alt, ref, bm, rng)
        lo, hi = (0, n) if rng is None else rng
        for b, name in enumerate(names):
            want = naive_strata(alt[b], ref[b], bm[b], lo, hi)
            assert np.array_equal(got["dist_count"][b], want["dist_count"]) and got["dist_count"].dtype == np.int32
            for k in STRATA:
                x, y = np.asarray(got[k][b], dtype=np.float64), np.asarray(want[k], dtype=np.float64)
                assert np.array_equal(np.isnan(x), np.isnan(y)), (name, k)
                f = ~np.isnan(y)
                assert np.all(np.abs(x[f] - y[f]) <= 1e-9 * np.maximum(1.0, np.abs(y[f]))), (name, rng, k)      # the pooled sums against the plain formula
    one = names.index("one")
    assert got["dist_count"][one].tolist() == [1] + [0] * (n - 1)


@pytest.mark.parametrize("n", [12, 30])
def test_identity_map_with_equal_maps_gives_zero_deltas(n):
    alt, _ = pairs(n, 2, 3 * n)
    ident = np.arange(n)
    track, ref_track, aligned = sv.paired_insulation_host(alt, alt, [1, 3], ident)
    assert same(track, ref_track, exact=True) and np.all(aligned[~np.isnan(aligned)] == 0.0) and np.array_equal(np.isnan(aligned), np.isnan(track))
    va, count = sv.paired_viewpoints_host(alt, alt, [0, n // 2, n - 1], ident)
    assert np.all(va == 0.0) and np.all(count == 1)
    st = sv.paired_strata_host(alt, alt, ident)
    assert np.all(st["dist_delta"] == 0.0) and np.all(st["dist_abs"] == 0.0) and np.all(st["dist_rms"] == 0.0) and np.all(st["mse"] == 0.0)
    assert np.all(st["scc"] == 1.0) and np.all(st["corr"] == 1.0)
    assert np.array_equal(st["dist_count"], np.tile(n - np.arange(n), (2, 1)))
    assert np.all(st["dist_corr"][:, : n - 1] == 1.0) and np.isnan(st["dist_corr"][:, n - 1]).all()         # the last stratum has one pair


@pytest.mark.parametrize("n", [12, 30])
def test_non_decreasing_maps_equal_the_unpaired_restatements_pair_by_pair(n):
    maps = kernel_maps(n)                                                    # every one of them is non-decreasing where it is mapped
    names = list(maps)
    alt, ref = pairs(n, len(names), 5 * n)
    bm = np.stack([maps[k] for k in names])
    widths, views, rng = [1, 2, 5], [0, n // 2, n - 1], (1, n - 2)
    track, ref_track, aligned = sv.paired_insulation_host(alt, ref, widths, bm)
    va, count = sv.paired_viewpoints_host(alt, ref, views, bm)
    st = sv.paired_strata_host(alt, ref, bm, rng)
    for b, name in enumerate(names):
        ht, _, ha = S.insulation_scores_host(alt[b: b + 1], ref[b], widths, bm[b])
        assert same(track[b], ht[0], exact=True) and same(aligned[b], ha[0], exact=True), name
        assert same(ref_track[b], S.insulation_host(ref[b: b + 1], widths)[0], exact=True)
        _, hv = S.viewpoint_scores_host(alt[b: b + 1], ref[b], views, bm[b])
        assert hv.dtype == np.float32 and same(va[b], hv[0], exact=True), name
        assert count[b].tolist() == [int((bm[b] == v).sum()) for v in views]
        hs = S.strata_scores_host(alt[b: b + 1], ref[b], bm[b], rng)
        assert np.array_equal(st["dist_count"][b], hs["dist_count"][0])
        for k in STRATA:
            assert same(st[k][b], hs[k][0]), (name, k)


@pytest.mark.parametrize("n", [12, 30])
def test_descending_map_reads_the_mirrored_reference_pixel(n):
    """Under a descending map (an inversion) the reference pair (map i, map (i + d)) lies below the diagonal.  With a NON-symmetric reference
    the rule shows: the result is that of the reference whose lower triangle is overwritten by its upper one, and NOT that of the transposed
    reference (which is what reading ref[map i][map (i + d)] as given would amount to)."""
    alt, ref = pairs(n, 1, 11 * n)
    desc = np.arange(n)[::-1].copy()
    desc[[2, n - 4]] = -1
    assert not np.allclose(ref[0], ref[0].T)
    got = sv.paired_strata_host(alt, ref, desc)
    upper = np.triu(ref[0]) + np.triu(ref[0], 1).T                           # symmetric: the upper triangle on both sides
    mirrored = sv.paired_strata_host(alt, upper[None], desc)
    transposed = sv.paired_strata_host(alt, np.ascontiguousarray(ref[0].T)[None], desc)
    lower = np.tril(ref[0]) + np.tril(ref[0], -1).T
    as_given = S.strata_scores_host(alt, lower, desc)                        # the unpaired rule on a descending map reads the LOWER triangle
    for k in STRATA:
        assert same(got[k], mirrored[k], exact=True), k
    assert not same(got["dist_delta"][:, 1:], transposed["dist_delta"][:, 1:]) and not same(got["scc"], transposed["scc"])
    assert same(got["dist_delta"][:, 0], transposed["dist_delta"][:, 0])    # the diagonal is its own mirror image
    assert same(transposed["dist_delta"], as_given["dist_delta"]) and not same(got["dist_delta"][:, 1:], as_given["dist_delta"][:, 1:])
    assert np.array_equal(got["dist_count"], transposed["dist_count"])


@pytest.mark.parametrize("name", ["identity", "duplicate", "descending", "holes"])
def test_nan_below_the_diagonal_changes_nothing(name):
    n = 30
    alt, ref = pairs(n, 1, 99)
    bm = all_maps(n)[name]
    low = np.tril(np.ones((n, n), dtype=bool), -1)
    a2, r2 = alt.copy(), ref.copy()
    a2[0][low] = np.nan
    r2[0][low] = np.nan
    for x, y in ((a2, ref), (alt, r2), (a2, r2)):
        clean, got = sv.paired_strata_host(alt, ref, bm, (1, n)), sv.paired_strata_host(x, y, bm, (1, n))
        assert all(same(got[k], clean[k], exact=True) for k in STRATA) and np.array_equal(got["dist_count"], clean["dist_count"])
        for c, g in zip(sv.paired_insulation_host(alt, ref, [1, 4], bm), sv.paired_insulation_host(x, y, [1, 4], bm)):
            assert same(g, c, exact=True)


def test_viewpoint_bins_against_genomic_positions():
    start = [3_000_000, 11_000_000, 15_000_000, 17_000_000, 18_000_000, 18_500_000]        # a 32 Mb window zooming in to 1 Mb
    ref_out = {"start_coords": start}
    inside_32_only = 5_000_000                                              # in the 32 Mb level, before the 16 Mb level's first base
    pos = [start[0], start[0] + 32_000_000 - 1, start[0] - 1, start[0] + 32_000_000, inside_32_only, 18_999_999, 19_500_000 - 1, 19_500_000, start[5] - 1]
    vb = sv.viewpoint_bins(pos, ref_out)
    assert vb.dtype == np.int32 and vb.shape == (6, len(pos))
    for k in range(6):
        size = 128000 >> k
        for j, p in enumerate(pos):
            lo, hi = start[k], start[k] + 250 * size                        # the level's window, half-open
            if lo <= p < hi:
                assert 0 <= vb[k, j] < 250 and lo + vb[k, j] * size <= p < lo + (vb[k, j] + 1) * size, (k, p)
            else:
                assert vb[k, j] == -1, (k, p)
    assert vb[:, 0].tolist() == [0, -1, -1, -1, -1, -1] and vb[0, 1] == 249 and vb[0, 2] == -1 and vb[0, 3] == -1
    assert vb[:, 4].tolist() == [15, -1, -1, -1, -1, -1]
    assert vb[5, 5] == 124 and vb[5, 6] == 249 and vb[5, 7] == -1 and vb[5, 8] == -1 and vb[4, 8] == 62
    assert sv.viewpoint_bins([], ref_out).shape == (6, 0)


def test_the_readouts_need_scores_and_checked_arguments():
    for kw in ({"insulation": (5,)}, {"viewpoints": [1_000_000]}, {"strata": True}):
        with pytest.raises(ValueError):
            sv.sv_screen([], None, [], 40_000_000, scores=False, **kw)
    for kw in ({"insulation": (0,)}, {"insulation": (125,)}, {"insulation": (5, 5)}, {"insulation": tuple(range(1, 10))}, {"viewpoints": []},
               {"viewpoints": list(range(65))}, {"viewpoints": ["x"]}, {"strata": (3, 3)}, {"strata": (0, 251)}, {"strata": False}):
        with pytest.raises(ValueError):
            sv.check_tracks(**kw)
    assert sv.check_tracks() is None
    spec = sv.check_tracks(insulation=(5, 10, 25), viewpoints=[7], strata=True)
    assert spec["insulation"].tolist() == [5, 10, 25] and spec["viewpoints"] == [7] and spec["strata"] == (0, 250)
    with pytest.raises(ValueError):
        sv.paired_strata_host(np.zeros((1, 4, 4)), np.zeros((1, 4, 4)), [0, 1, 2, 4])
    with pytest.raises(ValueError):
        sv.paired_viewpoints_host(np.zeros((1, 4, 4)), np.zeros((1, 4, 4)), [4], [0, 1, 2, 3])
