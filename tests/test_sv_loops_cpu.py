"""Loops per level of the SV screen, the numpy side (no GPU): `sv.paired_dot_follow_host` on hand-worked cases at n = 14, w = 2, d_min = 5 -
eligible pixels are 2 <= i, j <= 11, j - i >= 5 - its agreement with `screen.follow_loop` + `screen.dot_enrichment_host` on bin maps that repeat
no reference bin, `sv.paired_match_loops_host`, `sv.paired_loop_scores_host`'s shapes, and the argument checks of `sv_screen` / `sv_scores`."""
import numpy as np
import pytest

from orca_amd import screen, sv

N = 14
Q = screen.LoopParams(p=0, w=2, r=1, threshold=-1e30, d_min=5, max_calls=8, tol=1)
IDENT = np.arange(N)
JUMP = np.array([0, 1, 2, 3, 4, 8, 9, 10, 11, 12, 13, -1, -1, -1])             # reference bins 5 .. 7 deleted
TWICE = np.array([0, 1, 2, 2, 3, 4, 5, 6, 7, 8, 8, 9, 10, 11])                 # reference bins 2 and 8 each behind two alt bins
DOWN = IDENT[::-1].copy()
HOLE = np.where(IDENT == 9, -1, IDENT)


def emap(fill=None):
    """an enrichment map with a value of its own at every pixel - also at the ineligible ones: eligibility is the rule's, not the map's NaN"""
    e = (np.arange(N * N, dtype=np.float32).reshape(1, N, N) * np.float32(0.25)) if fill is None else np.full((1, N, N), fill, dtype=np.float32)
    return e.copy()


def follow(e, dots, bm, ref_e=None):
    ij = np.asarray(dots, dtype=np.int32).reshape(1, -1, 2)
    re = np.full((1, ij.shape[1]), 1.5, dtype=np.float32) if ref_e is None else np.asarray(ref_e, dtype=np.float32).reshape(1, -1)
    got = sv.paired_dot_follow_host(e, ij, re, bm, Q)
    assert got["candidates"].dtype == np.int32 and got["at"].dtype == np.int32 and got["enrich"].dtype == np.float32 and got["delta"].dtype == np.float32
    assert got["candidates"].shape == (1, ij.shape[1]) and got["at"].shape == (1, ij.shape[1], 2)
    return {k: v[0] for k, v in got.items()}


def test_identity_jump_and_mirror():
    e = emap()
    got = follow(e, [(3, 9), (2, 7), (2, 6)], IDENT)
    assert got["candidates"].tolist() == [1, 1, 0] and got["at"].tolist() == [[3, 9], [2, 7], [-1, -1]]        # (2, 6): j - i = 4 < d_min
    assert got["enrich"][0] == e[0, 3, 9] and got["delta"][0] == e[0, 3, 9] - np.float32(1.5) and np.isnan(got["enrich"][2]) and np.isnan(got["delta"][2])
    got = follow(e, [(2, 10), (3, 6), (3, 13)], JUMP)                         # behind the deletion every bin sits 3 lower; anchor 6 is deleted
    assert got["candidates"].tolist() == [1, 0, 1] and got["at"].tolist() == [[2, 7], [-1, -1], [3, 10]]
    got = follow(e, [(3, 13)], np.array([0, 1, 2, 3, 4, 8, 9, 10, 11, 12, 13, 13, -1, -1]))
    assert got["candidates"].tolist() == [2] and got["at"].tolist() == [[3, 11]]                              # alt 10 and 11 stand for 13: the larger e, at (3, 11)
    got = follow(e, [(3, 9)], DOWN)                                           # reference 3 sits at alt 10, reference 9 at alt 4: the mirrored pixel
    assert got["candidates"].tolist() == [1] and got["at"].tolist() == [[4, 10]] and got["enrich"][0] == e[0, 4, 10]
    got = follow(e, [(3, 9), (3, 10)], HOLE)
    assert got["candidates"].tolist() == [0, 1] and got["at"].tolist() == [[-1, -1], [3, 10]]


def test_duplicated_anchors_two_and_four_candidates():
    e = emap()
    got = follow(e, [(2, 7), (2, 8), (2, 6), (1, 8)], TWICE)
    # (2, 7): A = {2, 3}, C = {8}: 2 candidates.  (2, 8): A = {2, 3}, C = {9, 10}: 4.  (2, 6): C = {7}: (3, 7) is too near the diagonal, 1 left.
    # (1, 8): A = {1}, below w: none
    assert got["candidates"].tolist() == [2, 4, 1, 0]
    assert got["at"].tolist() == [[3, 8], [3, 10], [2, 7], [-1, -1]]          # e grows along the map: the last candidate is the strongest
    assert got["enrich"][1] == e[0, 3, 10]


def test_total_order_ties_and_nans():
    cand = [(2, 9), (2, 10), (3, 9), (3, 10)]
    e = emap(1e30)
    for (i, j), v in zip(cand, (1.0, 5.0, 5.0, 2.0)):
        e[0, i, j] = v
    got = follow(e, [(2, 8)], TWICE, [0.5])
    assert got["candidates"].tolist() == [4] and got["at"].tolist() == [[2, 10]] and got["enrich"][0] == 5.0 and got["delta"][0] == 4.5       # the earlier of two equals
    e = emap(1e30)
    for (i, j), v in zip(cand, (np.nan, np.nan, np.nan, -7.0)):
        e[0, i, j] = v
    got = follow(e, [(2, 8)], TWICE, [0.5])
    assert got["candidates"].tolist() == [4] and got["at"].tolist() == [[3, 10]] and got["enrich"][0] == -7.0 and got["delta"][0] == -7.5    # a NaN loses
    for i, j in cand:
        e[0, i, j] = np.nan
    got = follow(e, [(2, 8)], TWICE, [0.5])
    assert got["candidates"].tolist() == [4] and got["at"].tolist() == [[2, 9]] and np.isnan(got["enrich"][0]) and np.isnan(got["delta"][0])   # all NaN: the first
    e = emap()
    got = follow(e, [(2, 8)], TWICE, [np.nan])
    assert got["at"].tolist() == [[3, 10]] and got["enrich"][0] == e[0, 3, 10] and np.isnan(got["delta"][0])                                # the subtraction propagates


def test_empty_slots_are_never_used_as_indices():
    got = follow(emap(), [(-1, -1), (9, 3), (4, 4), (3, 9999), (-5, 9), (3, 14), (3, 9)], IDENT)
    assert got["candidates"].tolist() == [0] * 6 + [1] and got["at"].tolist() == [[-1, -1]] * 6 + [[3, 9]]
    assert np.isnan(got["enrich"][:6]).all() and np.isnan(got["delta"][:6]).all()


def test_without_repeats_it_is_follow_loop():
    n = 30
    q = screen.LoopParams(p=0, w=2, r=1, threshold=-1e30, max_calls=40)
    rs = np.random.RandomState(3)
    alt, ref = rs.randn(3, n, n).astype(np.float32), rs.randn(3, n, n).astype(np.float32)
    i = np.arange(n)
    holes = i.copy()
    holes[[5, 11, 12, 25]] = -1
    bm = np.stack([i, np.where(i + 3 < n, i + 3, -1), holes])
    e = screen.dot_enrichment_host(alt, q)
    rc = screen.dot_calls_host(ref, q)
    got = sv.paired_dot_follow_host(e, rc["ij"], rc["enrich"], bm, q)
    seen = set()
    for b in range(3):
        assert rc["count"][b] >= 3
        for k in range(q.max_calls):
            ri, rj = rc["ij"][b, k]
            a, c = screen.follow_loop(bm[b], ri, rj, q) if ri >= 0 else (-1, -1)
            assert got["at"][b, k].tolist() == [a, c] and got["candidates"][b, k] == (a >= 0)
            seen.add(a >= 0)
            if a >= 0:
                assert got["enrich"][b, k] == e[b, a, c] and got["delta"][b, k] == e[b, a, c] - rc["enrich"][b, k]
            else:
                assert np.isnan(got["enrich"][b, k]) and np.isnan(got["delta"][b, k])
    assert seen == {True, False}


def test_match_through_an_inversion_and_unmapped_bins():
    ref = np.array([[3, 9], [2, 8], [-1, -1]])
    alt = np.array([[4, 10], [2, 9], [-1, -1], [-1, -1]])
    gained, lost = sv.paired_match_loops_host(alt, ref, DOWN, 0)
    # alt (4, 10) stands for (min(9, 3), max(9, 3)) = (3, 9): matched.  alt (2, 9) stands for (4, 11): gained.  Reference (2, 8): lost
    assert gained.tolist() == [False, True, False, False] and lost.tolist() == [False, True, False]
    assert screen.match_loops_host(alt, ref[:2], 0, DOWN)[0].tolist() == [True, True, False, False]              # the 1 Mb screen's rule does not mirror
    gained, lost = sv.paired_match_loops_host(alt, ref, DOWN, 1)
    assert gained.tolist() == [False, True, False, False] and lost.tolist() == [False, False, False]             # (2, 8) is within 1 of (3, 9)
    gained, lost = sv.paired_match_loops_host(np.array([[3, 9], [3, 10]]), np.array([[3, 9], [3, 10]]), HOLE, 0)
    assert gained.tolist() == [True, False] and lost.tolist() == [True, False]                                 # alt bin 9 is unmapped: its dot is gained
    gained, lost = sv.paired_match_loops_host(np.array([[3, 9], [3, 10]]), np.array([[3, 9], [9999, 3], [5, 5]]), HOLE, 1)
    assert gained.tolist() == [True, False] and lost.tolist() == [False, False, False]                         # (3, 10) is within 1 of (3, 9); empty slots are not lost
    gained, lost = sv.paired_match_loops_host(np.full((3, 2), -1), np.full((2, 2), -1), IDENT, 1)
    assert not gained.any() and not lost.any()


def test_loop_scores_host_fields():
    n = 22
    q = screen.LoopParams(p=0, w=2, r=1, threshold=-1e30, max_calls=6)
    rs = np.random.RandomState(8)
    ref = rs.randn(2, n, n).astype(np.float32)
    i = np.arange(n)
    bm = np.stack([i, np.maximum(i - 1, 0)])
    got = sv.paired_loop_scores_host(ref, ref, bm, q)
    assert sorted(got) == sorted(sv.LOOP_SCORE_FIELDS)
    K = 6
    shapes = {"ref_loops": (2, K, 2), "loops": (2, K, 2), "ref_loop_enrichment": (2, K), "loop_enrichment": (2, K), "ref_loop_count": (2,), "loop_count": (2,),
              "loop_candidates": (2, K), "loop_followed_at": (2, K, 2), "loop_followed_enrichment": (2, K), "loop_delta": (2, K), "loop_is_gained": (2, K),
              "ref_loop_is_lost": (2, K), "loops_gained": (2,), "loops_lost": (2,)}
    for k, s in shapes.items():
        want = np.bool_ if "_is_" in k else (np.float32 if "enrichment" in k or k == "loop_delta" else np.int32)
        assert got[k].shape == s and got[k].dtype == want, k
    assert (got["ref_loop_count"] > K).all()                                 # truncated lists
    # an allele equal to its reference under the identity: every dot found where it was, nothing gained or lost
    assert (got["loop_candidates"][0] == 1).all() and np.array_equal(got["loop_followed_at"][0], got["ref_loops"][0]) and (got["loop_delta"][0] == 0).all()
    assert got["loops_gained"][0] == 0 and got["loops_lost"][0] == 0
    assert np.array_equal(got["loops"], got["ref_loops"])


def test_argument_checks():
    with pytest.raises(ValueError, match="scores=True"):
        sv.sv_screen([], None, [], 40_000_000, loops=True)
    with pytest.raises(ValueError, match="scores=True"):
        sv.sv_screen([], None, [], 40_000_000, loops=screen.LoopParams())
    for bad in (screen.LoopParams(p=4, w=4), screen.LoopParams(w=17), screen.LoopParams(max_calls=0), screen.LoopParams(threshold=float("nan")),
                screen.LoopParams(w=16, d_min=250), "yes", 3):
        with pytest.raises(ValueError, match="loops"):
            sv.check_loops_arg(bad)
        with pytest.raises(ValueError, match="loops"):
            sv.sv_screen([], None, [], 40_000_000, scores=True, loops=bad)
        with pytest.raises(ValueError, match="loops"):
            sv.sv_scores(sv.SV("del", 1, 2), {"predictions": None}, {"predictions": None}, 40_000_000, "cpu", loops=bad)
    assert sv.check_loops_arg(None) is None and sv.check_loops_arg(False) is None
    q = sv.check_loops_arg(True)
    assert q == screen.check_loops(True, 250) and q.d_min == 9 and q.max_calls == 64
    with pytest.raises(ValueError):
        sv.paired_dot_follow_host(np.zeros((1, N, N), dtype=np.float32), np.zeros((1, 2, 2)), np.zeros((1, 3)), IDENT, Q)
    with pytest.raises(ValueError):
        sv.paired_dot_follow_host(np.zeros((1, N, N), dtype=np.float32), np.zeros((1, 2, 2)), np.zeros((1, 2)), np.full(N, N), Q)
