"""Domain boundary calls from insulation tracks without a GPU (screen.boundary_calls_host, match_boundaries_host, boundary_scores_host;
sv.paired_boundary_scores_host): the numpy restatements that the device is held to, on hand-worked tracks, against an independent O(n^2) brute force
and against scipy's find_peaks + peak_prominences on -t, and the matching through hand-made bin maps - the identity, a deletion's jump, a
duplication's repeat, a descending map, a shifted boundary within and beyond ``tol``, an alt boundary on a -1 bin."""
import numpy as np
import pytest
import torch

from orca_amd import screen as S
from orca_amd import sv

NAN = np.nan


def f32(*v):
    return np.array(v, dtype=np.float32)


def same(a, b):
    """equal, NaN in the same slots; floats bit for bit"""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype.kind == "f":
        return bool(((a == b) | (np.isnan(a) & np.isnan(b))).all())
    return bool(np.array_equal(a, b))


def calls(track, min_strength=0.0, max_calls=None, tol=1):
    t = np.asarray(track, dtype=np.float32)
    return S.boundary_calls_host(t, S.BoundaryParams(min_strength, t.shape[-1] if max_calls is None else max_calls, tol)), None


def listed(got):
    k = min(int(got["count"]), got["bins"].shape[-1])
    return got["bins"][:k].tolist(), got["strength"][:k].tolist()


# ---- minima and strengths ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("track, bins, strengths", [
    ([5, 1, 4, NAN, 4, 0, 6, 2, 9], [1, 5, 7], [3.0, 4.0, 4.0]),             # the NaN ends the runs: bin 1 is measured against 4, not against 6
    ([3, 1, 1, 3], [1], [2.0]),                                              # the first bin of a plateau, and only that one
    ([3, 2, 2, 1, 4], [3], [2.0]),                                           # the shelf 2 2 is a minimum of strength 0: never a boundary
    ([1, 2, 3, 4, 5], [], []),
    ([5, 4, 3, 2, 1], [], []),
    ([NAN] * 6, [], []),
    ([NAN, 2, 1, 2, NAN], [2], [1.0]),
    ([2, 1, NAN, 1, 2], [], []),                                             # a dip beside a NaN has no right (left) neighbour: no minimum
])
def test_hand_worked_tracks(track, bins, strengths):
    got, _ = calls(track)
    b, s = listed(got)
    assert b == bins and s == strengths and int(got["count"]) == len(bins)
    n = len(track)
    st = np.full(n, NAN, dtype=np.float32)
    st[bins] = strengths
    assert same(got["strength_track"], st) and same(S.boundary_strength_host(f32(*track)), st)
    assert (got["bins"][len(bins):] == -1).all() and np.isnan(got["strength"][len(bins):]).all()


def test_truncation_keeps_the_full_count_and_min_strength_filters():
    t = f32(5, 1, 4, NAN, 4, 0, 6, 2, 9)
    got, _ = calls(t, max_calls=2)
    assert int(got["count"]) == 3 and got["bins"].tolist() == [1, 5] and got["strength"].tolist() == [3.0, 4.0]
    got, _ = calls(t, max_calls=1)
    assert int(got["count"]) == 3 and got["bins"].tolist() == [1]
    got, _ = calls(t, min_strength=3.5)
    assert int(got["count"]) == 2 and listed(got) == ([5, 7], [4.0, 4.0])
    assert same(got["strength_track"], f32(NAN, 3, NAN, NAN, NAN, 4, NAN, 4, NAN))          # the track does not depend on min_strength
    got, _ = calls(t, min_strength=4.0)                                                       # >=, compared in fp32
    assert listed(got) == ([5, 7], [4.0, 4.0])
    got, _ = calls(t, min_strength=4.0000005)
    assert int(got["count"]) == 0 and (got["bins"] == -1).all()
    # leading dimensions are kept
    got = S.boundary_calls_host(np.stack([t, t[::-1]])[None], S.BoundaryParams(0.0, 4, 1))
    assert got["count"].shape == (1, 2) and got["bins"].shape == (1, 2, 4) and got["strength_track"].shape == (1, 2, 9)
    assert got["bins"][0, 0].tolist() == [1, 5, 7, -1] and got["bins"][0, 1].tolist() == [1, 3, 7, -1]


def brute_force(t):
    """Independent of the walks: the strength of minimum i is min over the two sides of (the largest value of the longest stretch next to i that
    holds no NaN and nothing below t[i]) - t[i], every stretch tried, O(n^2) per bin."""
    n = t.shape[0]
    out = np.full(n, NAN, dtype=np.float32)
    for i in range(1, n - 1):
        if np.isnan(t[i - 1: i + 2]).any() or not (t[i] < t[i - 1] and t[i] <= t[i + 1]):
            continue
        sides = []
        for stretch in ([t[i - k: i] for k in range(1, i + 1)], [t[i + 1: i + 1 + k] for k in range(1, n - i)]):
            ok = [s for s in stretch if not np.isnan(s).any() and (s >= t[i]).all()]
            sides.append(max((s.max() for s in ok), default=t[i]))
        s = np.float32(min(sides)) - t[i]
        if s > 0:
            out[i] = s
    return out


def random_track(rs, n, kind):
    if kind == "quantised":
        t = rs.randint(0, 4, size=n).astype(np.float32) * np.float32(0.25)                 # many ties, plateaus and shelves
    elif kind == "walk":
        t = np.cumsum(rs.randn(n)).astype(np.float32)
    else:
        t = rs.randn(n).astype(np.float32)
    if rs.rand() < 0.7:                                                                    # edge NaNs, as the diamond leaves them
        w = rs.randint(0, max(1, n // 3))
        t[:w] = NAN
        t[n - w:] = NAN
    if rs.rand() < 0.4 and n > 4:
        t[rs.randint(0, n, size=rs.randint(1, 3))] = NAN                                   # interior NaNs
    return t


def test_restatement_equals_the_brute_force():
    rs = np.random.RandomState(11)
    seen = 0
    for trial in range(240):
        n = int(rs.choice([3, 4, 5, 9, 17, 40, 64, 65]))
        t = random_track(rs, n, ("quantised", "walk", "noise")[trial % 3])
        want = brute_force(t)
        assert same(S.boundary_strength_host(t), want), (trial, t)
        seen += int((want > 0).sum())
    assert seen > 300


def test_restatement_equals_scipy_prominences():
    sig = pytest.importorskip("scipy.signal")
    rs = np.random.RandomState(5)
    for trial in range(120):
        n = int(rs.randint(3, 257))
        t = rs.permutation(n).astype(np.float32) * np.float32(0.37) + np.float32(rs.randn())          # tie-free
        w = rs.randint(0, max(1, n // 3))
        t[:w] = NAN
        t[n - w:] = NAN
        run = t[w: n - w]
        want = np.full(n, NAN, dtype=np.float32)
        if run.size >= 3:
            peaks, _ = sig.find_peaks(-run)
            prom = sig.peak_prominences(-run, peaks)[0]
            want[peaks + w] = prom.astype(np.float32)
        got = S.boundary_strength_host(t)
        assert same(got, want), (trial, n, w)


# ---- matching ---------------------------------------------------------------------------------------------------------------------------------------
N = 12
FLAT = np.zeros(N, dtype=np.float32)
IDENT = np.arange(N)


def match(alt_bins, alt_s, ref_bins, ref_s, tol=1, bm=None, ta=FLAT, tr=FLAT):
    """`match_boundaries_host` on one pair, and the batched form the screens run gives the same."""
    K, R = 4, 4
    ab, rb = np.full(K, -1, dtype=np.int32), np.full(R, -1, dtype=np.int32)
    a_s, r_s = np.full(K, NAN, dtype=np.float32), np.full(R, NAN, dtype=np.float32)
    ab[: len(alt_bins)], a_s[: len(alt_bins)], rb[: len(ref_bins)], r_s[: len(ref_bins)] = alt_bins, alt_s, ref_bins, ref_s
    one = S.match_boundaries_host(ab, a_s, rb, r_s, ta, tr, tol, bm)
    many = S._match_boundaries(ab[None], a_s[None], rb[None], r_s[None], ta[None], tr[None], tol, None if bm is None else np.asarray(bm)[None])
    for k, v in one.items():
        assert same(many[k][0], v), k
    return one


def test_matching_under_the_identity_and_a_shift_within_and_beyond_tol():
    got = match([3, 9], [1.5, 0.5], [3, 8], [1.0, 2.0], tol=1)
    assert got["followed_at"].tolist() == [3, 9, -1, -1] and same(got["strength_delta"], f32(0.5, -1.5, NAN, NAN))
    assert not got["is_lost"].any() and not got["is_gained"].any() and not got["is_unmapped"].any() and not got["ref_is_unmapped"].any()
    got = match([3, 9], [1.5, 0.5], [3, 8], [1.0, 2.0], tol=0)                                # beyond tol: 8 is lost (-its strength), 9 is gained
    assert got["followed_at"].tolist() == [3, -1, -1, -1] and same(got["strength_delta"], f32(0.5, -2.0, NAN, NAN))
    assert got["is_lost"].tolist() == [False, True, False, False] and got["is_gained"].tolist() == [False, True, False, False]
    got = match([3, 10], [1.5, 0.5], [3, 8], [1.0, 2.0], tol=2)
    assert got["followed_at"].tolist() == [3, 10, -1, -1] and not got["is_lost"].any() and not got["is_gained"].any()
    got = match([], [], [], [])
    assert not any(got[k].any() for k in ("is_lost", "is_gained", "is_unmapped", "ref_is_unmapped")) and (got["followed_at"] == -1).all()


def test_a_reference_boundary_inside_a_deleted_span_is_unmapped_not_lost():
    bm = np.array([0, 1, 2, 3, 4, 8, 9, 10, 11, -1, -1, -1])                                  # reference bins 5 .. 7 deleted, three bins of refill
    got = match([6], [1.0], [6, 9], [2.0, 1.0], tol=1, bm=bm)                                 # alt bin 6 stands for reference bin 9
    assert got["ref_is_unmapped"].tolist() == [True, False, False, False] and not got["is_lost"].any()
    assert got["followed_at"].tolist() == [-1, 6, -1, -1] and same(got["strength_delta"], f32(NAN, 0.0, NAN, NAN))
    assert not got["is_gained"].any() and not got["is_unmapped"].any()
    got = match([6], [1.0], [5], [2.0], tol=1, bm=bm)                                         # reference bin 5 is within tol of bin 4, which alt bin 4 stands for: lost
    assert got["is_lost"].tolist() == [True, False, False, False] and same(got["strength_delta"], f32(-2.0, NAN, NAN, NAN))
    assert got["is_gained"].tolist() == [True, False, False, False]                           # alt bin 6 = reference bin 9, nothing listed near it
    ta = FLAT.copy()
    ta[3:6] = NAN                                                                             # ... unless the alt track cannot be read there
    got = match([6], [1.0], [5], [2.0], tol=1, bm=bm, ta=ta)
    assert got["ref_is_unmapped"].tolist() == [True, False, False, False] and not got["is_lost"].any()


def test_under_a_duplication_the_partner_is_the_stronger_copy():
    bm = np.array([0, 1, 2, 3, 4, 5, 2, 3, 4, 5, 6, 7])                                       # reference bins 2 .. 5 twice
    got = match([3, 7], [1.0, 2.5], [3], [2.0], tol=0, bm=bm)
    assert got["followed_at"].tolist() == [7, -1, -1, -1] and same(got["strength_delta"], f32(0.5, NAN, NAN, NAN))
    assert not got["is_gained"].any() and not got["is_lost"].any()                            # both copies match the reference boundary
    got = match([3, 7], [2.5, 2.5], [3], [2.0], tol=0, bm=bm)                                 # equal strengths: the lower alt bin
    assert got["followed_at"].tolist() == [3, -1, -1, -1]
    got = match([3, 6], [1.0, 2.5], [3], [2.0], tol=1, bm=bm)                                 # alt bin 6 stands for reference bin 2: within tol
    assert got["followed_at"].tolist() == [6, -1, -1, -1]
    got = match([6], [2.5], [9], [2.0], tol=1, bm=bm)                                         # the junction is a new boundary; reference bin 9 left the window
    assert got["is_gained"].tolist() == [True, False, False, False] and got["ref_is_unmapped"].tolist() == [True, False, False, False]


def test_a_descending_map_needs_no_special_case():
    bm = IDENT[::-1].copy()
    got = match([4, 9], [3.0, 1.0], [2, 6], [2.0, 1.0], tol=1, bm=bm)                         # alt 9 = reference 2; alt 4 = reference 7, one off 6
    assert got["followed_at"].tolist() == [9, 4, -1, -1] and same(got["strength_delta"], f32(-1.0, 2.0, NAN, NAN))
    assert not got["is_gained"].any() and not got["is_lost"].any()
    got = match([4, 9], [3.0, 1.0], [2, 6], [2.0, 1.0], tol=0, bm=bm)
    assert got["is_lost"].tolist() == [False, True, False, False] and got["is_gained"].tolist() == [True, False, False, False]


def test_an_alt_boundary_on_an_unmapped_bin_is_neither_gained_nor_a_match():
    bm = np.array([0, 1, 2, -1, -1, 3, 4, 5, 6, 7, 8, 9])                                     # two inserted bins
    got = match([3, 6], [5.0, 1.0], [4], [1.0], tol=1, bm=bm)
    assert got["is_unmapped"].tolist() == [True, False, False, False] and not got["is_gained"].any()
    assert got["followed_at"].tolist() == [6, -1, -1, -1]                                     # the unmapped one, though stronger, is no partner
    tr = FLAT.copy()
    tr[4] = NAN                                                                               # the reference track cannot be read where alt bin 6 stands
    got = match([6], [1.0], [], [], tol=1, bm=bm, tr=tr)
    assert got["is_unmapped"].tolist() == [True, False, False, False] and not got["is_gained"].any()
    # the -1 padding of the map is never taken for reference bin 0 (|-1 - 0| = 1 <= tol)
    got = match([], [], [0], [1.0], tol=1, bm=np.array([-1] * 6 + [4, 5, 6, 7, 8, 9]))
    assert got["ref_is_unmapped"].tolist() == [True, False, False, False]


def test_batched_matching_equals_the_plain_loops_on_random_pairs():
    rs = np.random.RandomState(3)
    n, K = 40, 6
    for trial in range(60):
        P = 5
        ta, tr = (rs.randint(0, 5, size=(P, n)).astype(np.float32) for _ in range(2))
        for t in (ta, tr):
            t[:, :3] = NAN
            t[:, -3:] = NAN
            t[rs.randint(0, P), rs.randint(3, n - 3)] = NAN
        q = S.BoundaryParams(0.0, K, int(rs.randint(0, 3)))
        ac, rc = S.boundary_calls_host(ta, q), S.boundary_calls_host(tr, q)
        bm = np.tile(np.arange(n), (P, 1))
        bm[1, 10:] = np.concatenate([np.arange(18, n), -np.ones(8, dtype=int)])               # a deletion
        bm[2, 20:] = np.arange(12, 32)                                                        # a duplication
        bm[3, 8:30] = np.arange(8, 30)[::-1]                                                  # an inversion
        bm[4, 5:9] = -1                                                                       # an insertion
        many = S._match_boundaries(ac["bins"], ac["strength"], rc["bins"], rc["strength"], ta, tr, q.tol, bm)
        for p in range(P):
            one = S.match_boundaries_host(ac["bins"][p], ac["strength"][p], rc["bins"][p], rc["strength"][p], ta[p], tr[p], q.tol, bm[p])
            for k, v in one.items():
                assert same(many[k][p], v), (trial, p, k)
            first = [int(np.flatnonzero(bm[p] == r)[0]) if r >= 0 and (bm[p] == r).any() else -1 for r in rc["bins"][p]]
            assert many["first_at"][p].tolist() == first


# ---- the fields of the two screens ------------------------------------------------------------------------------------------------------------------
def test_boundary_scores_host_fields():
    rs = np.random.RandomState(8)
    E, W, n = 4, 2, 30
    ref = rs.randint(0, 6, size=(W, n)).astype(np.float32)
    ref[:, :2] = ref[:, -2:] = NAN
    alt = np.repeat(ref[None], E, axis=0)
    alt[1, :, 10:20] = rs.randint(0, 6, size=(W, 10))
    alt[2] = np.roll(alt[2], 1, axis=-1)
    alt[3, :, 12:] = np.concatenate([ref[:, 16:], np.full((W, 4), NAN, dtype=np.float32)], axis=1)      # a deletion of reference bins 12 .. 15
    bm = np.tile(np.arange(n), (E, 1))
    bm[3, 12:] = np.concatenate([np.arange(16, n), [-1] * 4])
    delta, al = rs.randn(E, W, n).astype(np.float32), rs.randn(E, W, n).astype(np.float32)
    K = 16
    q = S.BoundaryParams(0.0, K, 1)
    got = S.boundary_scores_host(alt, ref, q, bm, delta, al)
    plain = S.boundary_scores_host(alt, ref, q, None, delta)
    names = ("ref_boundaries", "ref_boundary_strength", "ref_boundary_count", "boundaries", "boundary_strength", "boundary_count") + S.BOUNDARY_MATCH_FIELDS
    assert set(plain) == set(names) and set(got) == set(names) | {"aligned_" + k for k in S.BOUNDARY_MATCH_FIELDS}
    assert set(S.boundary_scores_host(alt, ref, q)) == set(names) - {"boundary_delta"}
    for k in plain:
        assert same(plain[k], got[k]), k
    assert int(got["ref_boundary_count"].max()) <= K and int(got["boundary_count"].max()) <= K
    assert got["ref_boundaries"].shape == (W, K) and got["boundaries"].shape == (E, W, K) and got["boundary_count"].shape == (E, W)
    assert got["boundaries_lost"].dtype == np.int32 and got["ref_boundary_is_lost"].dtype == bool and got["boundary_followed_at"].dtype == np.int32
    # the unchanged item keeps every boundary at strength delta 0; where the bin map is the identity the aligned forms are the plain ones
    lst = got["ref_boundaries"] >= 0
    assert same(got["boundary_followed_at"][0], got["ref_boundaries"]) and (got["boundary_strength_delta"][0][lst] == 0).all()
    assert got["boundaries_lost"][0].tolist() == [0] * W and got["boundaries_gained"][0].tolist() == [0] * W
    for k in S.BOUNDARY_MATCH_FIELDS:
        assert same(got["aligned_" + k][:3], plain[k][:3]) or k == "boundary_delta", k
    # boundary_delta gathers the given difference at the reference boundary's own bin; the aligned form at the alt bin that stands for it
    for e in range(E):
        for w in range(W):
            for k, r in enumerate(got["ref_boundaries"][w]):
                want = NAN if r < 0 else delta[e, w, r]
                assert same(got["boundary_delta"][e, w, k], np.float32(want))
                at = np.flatnonzero(bm[e] == r) if r >= 0 else []
                assert same(got["aligned_boundary_delta"][e, w, k], np.float32(al[e, w, at[0]] if len(at) else NAN))
    # the deletion: a reference boundary inside bins 13 .. 14 is unmapped through the bin map (12 and 15 are within tol of mapped bins)
    inside = lst & (got["ref_boundaries"] >= 13) & (got["ref_boundaries"] <= 14)
    assert got["aligned_ref_boundary_is_unmapped"][3][inside].all()
    assert not (got["aligned_ref_boundary_is_lost"][3] & inside).any()
    # behind the deletion every boundary of the shifted track is found again through the bin map, at strength delta 0 where the runs are whole
    moved = lst & (got["ref_boundaries"] >= 18) & (got["ref_boundaries"] <= n - 5)
    assert (got["aligned_boundary_followed_at"][3][moved] == got["ref_boundaries"][moved] - 4).all()


def test_paired_boundary_scores_host_is_the_same_rule_per_pair():
    rs = np.random.RandomState(9)
    B, W, n = 3, 2, 250
    tr = rs.randint(0, 7, size=(B, W, n)).astype(np.float32)
    ta = tr.copy()
    ta[:, :, 100:140] = rs.randint(0, 7, size=(B, W, 40))
    for t in (ta, tr):
        t[:, :, :5] = t[:, :, -5:] = NAN
    bm = np.tile(np.arange(n), (B, 1))
    bm[1, 120:] = np.concatenate([np.arange(150, n), [-1] * 30])
    bm[2, 60:200] = np.arange(60, 200)[::-1]
    dl = rs.randn(B, W, n).astype(np.float32)
    q = S.BoundaryParams(1.0, 16, 2)
    got = sv.paired_boundary_scores_host(ta, tr, dl, bm, q)
    assert set(got) == set(sv.BOUNDARY_SCORE_FIELDS) and len(sv.BOUNDARY_SCORE_FIELDS) == 15
    for b in range(B):
        for w in range(W):
            ac, rc = S.boundary_calls_host(ta[b, w], q), S.boundary_calls_host(tr[b, w], q)
            assert same(got["boundaries"][b, w], ac["bins"]) and same(got["ref_boundary_strength"][b, w], rc["strength"])
            assert got["boundary_count"][b, w] == ac["count"] and got["ref_boundary_count"][b, w] == rc["count"]
            one = S.match_boundaries_host(ac["bins"], ac["strength"], rc["bins"], rc["strength"], ta[b, w], tr[b, w], q.tol, bm[b])
            for k, name in (("followed_at", "boundary_followed_at"), ("strength_delta", "boundary_strength_delta"), ("is_lost", "ref_boundary_is_lost"),
                            ("is_gained", "boundary_is_gained"), ("is_unmapped", "boundary_is_unmapped"), ("ref_is_unmapped", "ref_boundary_is_unmapped")):
                assert same(got[name][b, w], one[k]), (b, w, name)
            assert got["boundaries_lost"][b, w] == one["is_lost"].sum() and got["boundaries_gained"][b, w] == one["is_gained"].sum()
    assert int(got["ref_boundary_count"].min()) > 0 and got["boundary_delta"].shape == (B, W, 16)
    one_map = sv.paired_boundary_scores_host(ta[:1], tr[:1], dl[:1], bm[0], q)
    for k in got:
        assert same(one_map[k][0], got[k][0]), k


# ---- refused arguments ------------------------------------------------------------------------------------------------------------------------------
def test_check_boundaries():
    assert S.check_boundaries(True, 250) == S.BoundaryParams(float(np.float32(0.1)), 32, 1)
    q = S.check_boundaries(S.BoundaryParams(0.0, 250, 0), 250)
    assert q == S.BoundaryParams(0.0, 250, 0) and isinstance(q.min_strength, float)
    for bad in (False, None, 1, "yes", (0.1, 32, 1), S.LoopParams()):
        with pytest.raises(ValueError, match="BoundaryParams"):
            S.check_boundaries(bad, 250)
    for bad in (dict(min_strength=-0.1), dict(min_strength=NAN), dict(min_strength="x"), dict(min_strength=True), dict(min_strength=None),
                dict(max_calls=0), dict(max_calls=251), dict(max_calls=1.0), dict(max_calls=True), dict(tol=-1), dict(tol=1.0), dict(tol=None)):
        with pytest.raises(ValueError, match="boundaries"):
            S.check_boundaries(S.BoundaryParams(**bad), 250)
    for n in (2, 257):
        with pytest.raises(ValueError, match="bins"):
            S.check_boundaries(True, n)
    assert S.check_boundaries(S.BoundaryParams(max_calls=3), 3).max_calls == 3


def test_boundaries_need_the_insulation_tracks():
    from orca_amd import orca_modules as pm
    net = pm.Net(num_1d=4).eval()
    win = torch.zeros(40_000, dtype=torch.uint8)
    for b in (True, S.BoundaryParams()):
        with pytest.raises(ValueError, match="insulation"):
            S.screen_1m(net, win, [S.Edit("mask", 0, 10)], boundaries=b)
    with pytest.raises(ValueError, match="insulation"):
        sv.check_readouts(boundaries=True)
    with pytest.raises(ValueError, match="insulation"):
        sv.check_readouts(viewpoints=[5], boundaries=S.BoundaryParams())
    rd = sv.check_readouts(insulation=(5, 10), boundaries=True)
    assert rd.boundaries == S.check_boundaries(True, 250) and rd.loops is None and rd.insulation.tolist() == [5, 10]
    assert sv.check_readouts(insulation=(5, 10)).boundaries is None and sv.check_readouts(insulation=5, boundaries=False).boundaries is None
    entry = sv.entry_readouts({"bin_map": np.zeros((6, 250), dtype=np.int32)}, rd)
    assert entry["boundary_params"] == rd.boundaries and "loop_params" not in entry
    assert "boundary_params" not in sv.entry_readouts({"bin_map": np.zeros((6, 250), dtype=np.int32)}, sv.check_readouts(insulation=5))
