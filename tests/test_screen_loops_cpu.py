"""The host side of the screen's loop (dot) calls without a GPU: `screen.dot_enrichment_host`, `dot_calls_host`, `follow_loop`, `match_loops_host`,
`loop_scores_host` and `check_loops`.  The restatements are checked against a brute-force loop over pixels, offsets and neighbours written here
from the definitions of include/orca_hip.h (orca_screen_dot_calls).  The random maps are multiples of 2^-12 with |x| < 8: every fp64 sum of at
most 33^2 of them is exact whatever its order, so the two sides must agree bit for bit."""
import math

import numpy as np
import pytest

from orca_amd import screen as S
from tests.test_gpu_screen_aligned import kernel_maps

PW = [(0, 1), (1, 3), (1, 4)]


def quantised(rs, *shape):
    return (np.clip(np.round(rs.randn(*shape) * 4096.0), -32767, 32767) / 4096.0).astype(np.float32)


def eligible(i, j, n, w, d_min):
    return w <= i and j <= n - 1 - w and j - i >= d_min


def brute_enrichment(m, p, w, d_min):
    """e of one map [n, n] by the definition: five lists per pixel, math.fsum (exact), one division each"""
    n = m.shape[0]
    out = np.full((n, n), np.nan, dtype=np.float32)
    for i in range(n):
        for j in range(n):
            if not eligible(i, j, n, w, d_min):
                continue
            P, D, LL, H, V = [], [], [], [], []
            for a in range(-w, w + 1):
                for b in range(-w, w + 1):
                    x = float(m[i + a, j + b])
                    in_p = abs(a) <= p and abs(b) <= p
                    if in_p:
                        P.append(x)
                    if not in_p and a != 0 and b != 0:
                        D.append(x)
                    if not in_p and 1 <= a <= w and -w <= b <= -1:
                        LL.append(x)
                    if abs(a) <= 1 and p < abs(b) <= w:
                        H.append(x)
                    if abs(b) <= 1 and p < abs(a) <= w:
                        V.append(x)
            assert len(P) == (2 * p + 1) ** 2 and len(LL) == w * w - p * p and len(H) == len(V) == 6 * (w - p)
            assert len(D) == (2 * w + 1) ** 2 - (2 * p + 1) ** 2 - 4 * (w - p)
            means = [math.fsum(s) / len(s) for s in (P, D, LL, H, V)]
            if any(math.isnan(v) for v in means):
                continue
            out[i, j] = np.float32(means[0] - max(means[1:]))
    return out


def brute_calls(e, r, T, K):
    """the dots of one enrichment map [n, n] float32 by the definition: (count, ij [K, 2], enrich [K])"""
    n = e.shape[0]
    T = np.float32(T)
    dots = []
    for i in range(n):
        for j in range(n):
            v = e[i, j]
            if np.isnan(v) or not v >= T:
                continue
            ok = True
            for ii in range(max(0, i - r), min(n, i + r + 1)):
                for jj in range(max(0, j - r), min(n, j + r + 1)):
                    f = e[ii, jj]
                    if (ii, jj) == (i, j) or np.isnan(f):
                        continue
                    ok &= bool(v > f) if (ii, jj) < (i, j) else bool(v >= f)
            if ok:
                dots.append((i, j))
    ij = np.full((K, 2), -1, dtype=np.int32)
    en = np.full(K, np.nan, dtype=np.float32)
    for k, (i, j) in enumerate(dots[:K]):
        ij[k], en[k] = (i, j), e[i, j]
    return len(dots), ij, en


def same_f32(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype == np.float32 and a.shape == b.shape and np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(a[~np.isnan(a)], b[~np.isnan(b)])


@pytest.mark.parametrize("p,w", PW)
@pytest.mark.parametrize("n", [5, 6, 13, 50])
def test_restatements_equal_the_brute_force(n, p, w):
    rs = np.random.RandomState(100 * n + w)
    maps = quantised(rs, 2, n, n)
    for d_min in (None, 2 * w + 3):
        q = S.LoopParams(p=p, w=w, r=2, threshold=-0.5, d_min=d_min, max_calls=7)
        dm = 2 * w + 1 if d_min is None else d_min
        e = S.dot_enrichment_host(maps, q)
        assert e.dtype == np.float32 and e.shape == (2, n, n)
        n_elig = sum(eligible(i, j, n, w, dm) for i in range(n) for j in range(n))
        assert int((~np.isnan(e[0])).sum()) == n_elig
        if n < 4 * w + 2:
            assert n_elig == 0
        if (n, w, d_min) == (6, 1, None):
            assert np.argwhere(~np.isnan(e[0])).tolist() == [[1, 4]]
        calls = S.dot_calls_host(maps, q)
        for k in range(2):
            want = brute_enrichment(maps[k], p, w, dm)
            assert same_f32(e[k], want), (n, p, w, d_min, k)
            cnt, ij, en = brute_calls(want, 2, -0.5, 7)
            assert int(calls["count"][k]) == cnt and np.array_equal(calls["ij"][k], ij) and same_f32(calls["enrich"][k], en), (n, p, w, d_min, k)
        assert calls["count"].dtype == np.int32 and calls["ij"].dtype == np.int32 and same_f32(calls["e_map"], e)


def test_a_block_of_ones_is_one_dot():
    m = np.zeros((1, 30, 30), dtype=np.float32)
    m[0, 9:12, 19:22] = 1.0
    q = S.LoopParams(p=1, w=3, r=2, threshold=0.5)
    got = S.dot_calls_host(m, q)
    assert got["count"].tolist() == [1] and got["ij"][0, 0].tolist() == [10, 20] and got["enrich"][0, 0] == np.float32(1.0)
    assert (got["ij"][0, 1:] == -1).all() and np.isnan(got["enrich"][0, 1:]).all() and got["ij"].shape == (1, 64, 2)


@pytest.mark.parametrize("p,w,d_min", [(0, 1, None), (1, 4, None), (1, 3, 11)])
def test_a_constant_map_has_exactly_one_dot(p, w, d_min):
    q = S.LoopParams(p=p, w=w, r=2, threshold=0.0, d_min=d_min)
    got = S.dot_calls_host(np.full((1, 40, 40), 0.375, dtype=np.float32), q)
    dm = 2 * w + 1 if d_min is None else d_min
    assert got["count"].tolist() == [1] and got["ij"][0, 0].tolist() == [w, w + dm] and got["enrich"][0, 0] == 0.0


def test_a_nan_pixel_shows_in_the_windows_that_hold_it():
    n, p, w = 40, 1, 3
    q = S.LoopParams(p=p, w=w)
    maps = quantised(np.random.RandomState(3), 1, n, n)
    clean = S.dot_enrichment_host(maps, q)
    for (y, x) in ((10, 25), (30, 8), (20, 20), (3, 36)):               # above the diagonal, below it, on it, in a corner
        m = maps.copy()
        m[0, y, x] = np.nan
        e = S.dot_enrichment_host(m, q)
        want = {(i, j) for i in range(n) for j in range(n) if eligible(i, j, n, w, 2 * w + 1) and abs(i - y) <= w and abs(j - x) <= w}
        assert {tuple(v) for v in np.argwhere(np.isnan(e[0]) & ~np.isnan(clean[0]))} == want, (y, x)
        keep = ~np.isnan(e)
        assert np.array_equal(e[keep], clean[keep])
        if y >= x:
            assert not want                                             # nothing on or below the diagonal is read
        assert same_f32(e[0], brute_enrichment(m[0], p, w, 2 * w + 1))
    # a NaN neighbour neither wins nor loses: the dot beside it stays a dot
    m = np.zeros((1, 30, 30), dtype=np.float32)
    m[0, 9:12, 19:22] = 1.0
    m[0, 2, 27] = np.nan
    got = S.dot_calls_host(m, S.LoopParams(p=1, w=3, r=8, threshold=0.5))
    assert np.isnan(got["e_map"][0, 4, 25]) and got["count"].tolist() == [1] and got["ij"][0, 0].tolist() == [10, 20]


def test_truncation_at_max_calls():
    maps = quantised(np.random.RandomState(5), 2, 50, 50)
    full = S.dot_calls_host(maps, S.LoopParams(p=0, w=1, r=1, threshold=-100.0, max_calls=4096))
    cut = S.dot_calls_host(maps, S.LoopParams(p=0, w=1, r=1, threshold=-100.0, max_calls=5))
    assert (full["count"] > 20).all() and np.array_equal(cut["count"], full["count"])
    assert np.array_equal(cut["ij"], full["ij"][:, :5]) and same_f32(cut["enrich"], full["enrich"][:, :5])
    for k in range(2):
        c = int(full["count"][k])
        rows = full["ij"][k, :c].tolist()
        assert rows == sorted(rows) and (full["ij"][k, c:] == -1).all() and np.isnan(full["enrich"][k, c:]).all() and not np.isnan(full["enrich"][k, :c]).any()


def test_check_loops_refusals():
    q = S.check_loops(True, 50)
    assert q == S.LoopParams(1, 4, 2, 0.25, 9, 64, 1) and S.check_loops(S.LoopParams(d_min=12), 50).d_min == 12
    assert S.check_loops(S.LoopParams(p=0, w=1), 6).d_min == 3 and S.check_loops(S.LoopParams(p=15, w=16, r=16, max_calls=4096, tol=0), 256).w == 16
    bad = [dict(p=-1), dict(p=4), dict(p=5, w=4), dict(w=17, p=1), dict(w=0, p=0), dict(r=0), dict(r=17), dict(d_min=8), dict(d_min=-1), dict(max_calls=0),
           dict(max_calls=4097), dict(tol=-1), dict(threshold=float("nan")), dict(threshold="x"), dict(threshold=None), dict(p=1.0), dict(w=True), dict(r=2.5),
           dict(max_calls=64.0), dict(tol=None)]
    for kw in bad:
        with pytest.raises(ValueError):
            S.check_loops(S.LoopParams(**kw), 250)
    for other in (False, None, 1, (1, 4), "yes", {"p": 1}):
        with pytest.raises(ValueError):
            S.check_loops(other, 250)
    with pytest.raises(ValueError):
        S.check_loops(True, 17)                                         # n = 4 w + 1: no eligible pixel
    assert S.check_loops(True, 18).d_min == 9
    with pytest.raises(ValueError):
        S.check_loops(S.LoopParams(p=0, w=1), 5)
    with pytest.raises(ValueError):
        S.check_loops(S.LoopParams(d_min=100), 108)


def test_follow_and_match_on_hand_made_bin_maps():
    n = 50
    q = S.LoopParams(p=1, w=3)                                          # d_min 7
    maps = kernel_maps(n)
    assert S.follow_loop(maps["identity"], 10, 30, q) == (10, 30)
    assert S.follow_loop(maps["shift"], 10, 30, q) == (7, 27)           # map a = a + 3
    assert S.follow_loop(maps["shift"], 5, 30, q) == (-1, -1)           # alt row 2 < w: ineligible
    assert S.follow_loop(maps["shift"], 2, 30, q) == (-1, -1)           # reference bin 2 is behind no alt bin
    assert S.follow_loop(maps["duplicate"], 0, 30, q) == (-1, -1)       # alt bins 0 and 1 both stand for 0: the lowest, 0 < w
    assert S.follow_loop(maps["duplicate"], 10, 30, q) == (11, 31)
    assert S.follow_loop(maps["none"], 10, 30, q) == (-1, -1)
    assert S.follow_loop(maps["one"], n - 1, n - 1, q) == (-1, -1)      # one pixel, on the diagonal
    assert S.follow_loop(maps["identity"], 10, 16, q) == (-1, -1)       # closer than d_min
    holes = maps["holes"]
    i, j = [int(v) for v in np.flatnonzero(holes >= 0)[[3, -4]]]
    assert S.follow_loop(holes, i, j, q) == (i, j)
    gone = int(np.flatnonzero(holes < 0)[2])
    assert S.follow_loop(holes, gone, 45, q) == (-1, -1) or holes[45] < 0
    # an insertion next to the anchor: alt bins 20 and 21 both stand for reference bin 20 -> the lowest as a row, the highest as a column
    k = np.arange(n)
    ins = np.where(k <= 20, k, k - 1)
    assert S.follow_loop(ins, 20, 40, q) == (20, 41) and S.follow_loop(ins, 5, 20, q) == (5, 21)
    # every pair against the brute force
    for name, bm in maps.items():
        for ri in range(n):
            for rj in range(ri, n, 7):
                a = [x for x in range(n) if bm[x] == ri]
                b = [x for x in range(n) if bm[x] == rj]
                want = (a[0], b[-1]) if a and b and eligible(a[0], b[-1], n, 3, 7) else (-1, -1)
                assert S.follow_loop(bm, ri, rj, q) == want, (name, ri, rj)
        ref_ij = np.array([[ri, rj] for ri in range(0, n, 3) for rj in range(ri, n, 5)], dtype=np.int32)
        assert np.array_equal(S._follow_loops(bm[None], ref_ij, S.check_loops(q, n))[0], [S.follow_loop(bm, int(a), int(b), q) for a, b in ref_ij]), name

    ref = np.array([[10, 30], [12, 40], [20, 45]], dtype=np.int32)
    pad = [[-1, -1]] * 2
    # bin with bin: within tol = 1 matches, two bins away does not; padding is neither gained nor a match
    g, l = S.match_loops_host(np.array([[11, 29], [12, 42], [5, 20]] + pad), ref, 1)
    assert g.tolist() == [False, True, True, False, False] and l.tolist() == [False, True, True]
    g, l = S.match_loops_host(np.array([[11, 29], [12, 42], [5, 20]] + pad), ref, 2)
    assert g.tolist() == [False, False, True, False, False] and l.tolist() == [False, False, True]
    g, l = S.match_loops_host(np.array(pad), ref, 1)
    assert not g.any() and l.all()
    g, l = S.match_loops_host(np.array([[11, 29]] + pad), ref[:0], 1)
    assert g.tolist() == [True, False, False] and l.shape == (0,)
    # a deleted anchor -> lost: reference bins 10 .. 14 deleted, the dot at (12, 40) has nowhere to be; the others moved 5 bins and are kept when aligned
    dele = np.where(k < 10, k, np.where(k + 5 < n, k + 5, -1))
    alt = np.array([[9, 25], [15, 40]] + pad)                           # stands for (9, 30) and (20, 45)
    g, l = S.match_loops_host(alt, ref, 1, dele)
    assert g.tolist() == [False, False, False, False] and l.tolist() == [False, True, False]
    g, l = S.match_loops_host(alt, ref, 1)                              # bin with bin the shifted dots are gained, and the reference's lost
    assert g.tolist() == [True, True, False, False] and l.tolist() == [True, True, True]
    assert S.follow_loop(dele, 12, 40, q) == (-1, -1) and S.follow_loop(dele, 20, 45, q) == (15, 40)
    # an inserted anchor -> gained: alt bins 10, 11 are inserted bases; a dot on them stands for nothing
    insm = np.where(k < 10, k, np.where(k < 12, -1, k - 2))
    g, l = S.match_loops_host(np.array([[10, 32], [12, 32], [5, 11]] + pad), ref, 1, insm)      # (-1, 30), (10, 30), (5, -1)
    assert g.tolist() == [True, False, True, False, False] and l.tolist() == [False, True, True]
    # shift: kept under aligned, gained plus lost bin with bin
    sh = maps["shift"]
    g, l = S.match_loops_host(np.array([[7, 27], [9, 37], [17, 42]]), ref, 0, sh)
    assert not g.any() and not l.any()
    g, l = S.match_loops_host(np.array([[7, 27], [9, 37], [17, 42]]), ref, 1)
    assert g.all() and l.all()
    g, l = S.match_loops_host(np.array([[7, 27]]), ref, 1, maps["none"])
    assert g.all() and l.all()


def test_the_screens_batched_matching_equals_the_per_item_one():
    n, E, K = 50, 40, 6
    rs = np.random.RandomState(12)
    maps = list(kernel_maps(n).values())
    bm = np.stack([maps[e % len(maps)] for e in range(E)])
    alt = rs.randint(0, n, (E, K, 2))
    for e in range(E):
        alt[e, rs.randint(0, K + 1):] = -1                              # lists of every length, 0 included
    for R in (0, 1, 9):
        ref = rs.randint(0, n, (R, 2))
        for tol in (0, 1, 4):
            for m in (None, bm):
                g, l = S._match_loops(alt, ref, tol, m)
                assert g.shape == (E, K) and l.shape == (E, R) and g.dtype == l.dtype == bool
                for e in range(E):
                    hg, hl = S.match_loops_host(alt[e], ref, tol, None if m is None else m[e])
                    assert np.array_equal(g[e], hg) and np.array_equal(l[e], hl), (R, tol, m is None, e)
    g, l = S._match_loops(alt[:0], ref, 1, bm[:0])
    assert g.shape == (0, K) and l.shape == (0, 9)


def test_loop_scores_host_fields():
    n, K = 50, 6
    q = S.LoopParams(p=1, w=3, r=2, threshold=0.4, max_calls=K, tol=1)
    ref = np.zeros((n, n), dtype=np.float32)
    for (i, j) in ((10, 30), (12, 42), (20, 45)):
        ref[i - 1: i + 2, j - 1: j + 2] = 1.0
    ref = ref + ref.T
    k = np.arange(n)
    dele = np.where(k < 11, k, np.where(k + 3 < n, k + 3, -1))          # reference bins 11 .. 13 deleted: the anchor of (12, 42) goes
    alt_del = np.zeros((n, n), dtype=np.float32)
    for (i, j) in ((10, 27), (17, 42)):                                 # (10, 30) and (20, 45) as the deletion leaves them
        alt_del[i - 1: i + 2, j - 1: j + 2] = 1.0
    weak = ref.copy()
    weak[9:12, 29:32] = 0.75                                            # the first loop weakened by a quarter
    alt = np.stack([ref, alt_del + alt_del.T, weak])
    bm = np.stack([k, dele, k])
    out = S.loop_scores_host(alt, ref, q, bm)
    assert out["ref_loop_count"] == 3 and out["ref_loops"].tolist() == [[10, 30], [12, 42], [20, 45]] and out["ref_loop_enrichment"].tolist() == [1.0, 1.0, 1.0]
    assert out["loop_count"].tolist() == [3, 2, 3] and out["loops"].shape == (3, K, 2) and out["loops"][1, :3].tolist() == [[10, 27], [17, 42], [-1, -1]]
    assert out["loops_gained"].tolist() == [0, 2, 0] and out["loops_lost"].tolist() == [0, 3, 0]
    assert out["aligned_loops_gained"].tolist() == [0, 0, 0] and out["aligned_loops_lost"].tolist() == [0, 1, 0]
    assert out["aligned_ref_loop_is_lost"][1].tolist() == [False, True, False] and out["loop_is_gained"][1].tolist() == [True, True] + [False] * (K - 2)
    assert out["loop_delta"][0].tolist() == [0.0, 0.0, 0.0] and out["loop_delta"][2].tolist() == [-0.25, 0.0, 0.0]
    assert out["aligned_loop_delta"][1, 0] == 0.0 and np.isnan(out["aligned_loop_delta"][1, 1]) and out["aligned_loop_delta"][1, 2] == 0.0
    e1 = brute_enrichment(alt[1], 1, 3, 7)                             # bin with bin the deletion's map has no peak at any reference dot
    assert out["loop_delta"][1].tolist() == [float(e1[i, j] - np.float32(1.0)) for i, j in ((10, 30), (12, 42), (20, 45))] and (out["loop_delta"][1] <= -1.0).all()
    for f in S.LOOP_FIELDS:                                             # identity bin maps: the plain fields
        for e in (0, 2):
            assert np.array_equal(out["aligned_" + f][e], out[f][e], equal_nan=True), f
        assert out[f].dtype == out["aligned_" + f].dtype
    assert out["loop_delta"].dtype == np.float32 and out["loops_gained"].dtype == np.int32 and out["loop_is_gained"].dtype == bool
    plain = S.loop_scores_host(alt, ref, q)
    assert not any(key.startswith("aligned_") for key in plain) and all(np.array_equal(plain[key], out[key], equal_nan=True) for key in plain)
    none = S.loop_scores_host(alt, np.zeros((n, n), dtype=np.float32), S.LoopParams(p=1, w=3, threshold=0.4, max_calls=K), bm)
    assert none["ref_loop_count"] == 0 and none["loop_delta"].shape == (3, 0) and none["loops_gained"].tolist() == [3, 2, 3] and none["loops_lost"].tolist() == [0, 0, 0]
