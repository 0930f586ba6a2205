"""Non-additivity scores of the 1 Mb mutagenesis screen on the MI355X: the two kernels alone on hand-made member tables against the numpy
restatement (`screen.epistasis_scores_host`), bit-for-bit invariance to the batch, where a NaN pixel shows, the entry points' argument checks
(return codes only: nothing malformed reaches a kernel), and `screen.epistasis_1m` end to end on a 200 000-base window (synthetic
H1esc_1M(synthetic_seed=0)) on every route and on both strands.

Tolerances.  Per pixel the kernel and the restatement evaluate the same fp64 expression in the same order - t = 0.0 + (A_0 - ref) + (A_1 - ref)
+ ..., r = (S - ref) - t, no multiplication, so nothing to contract - and get the same r and t.  ``epi_abs_max`` is the largest fp64 |r| rounded to
fp32 once on both sides: bit for bit.  Every other field is an fp64 sum of N terms (N = n^2 for the means over the map, n for a profile row,
the rectangle's area for a region score) divided once and rounded to fp32 once.  The two sides associate the sum differently; any order of
an fp64 sum of N terms of size <= max|r| is within (N - 1) 2^-53 N max|r| of the exact sum, so two orders differ by less than 2 N 2^-53 max|r|
after the division by N.  The final rounding adds at most one fp32 ulp on either side: RTOL = 2.4e-7, two fp32 ulps, the RTOL of
tests/test_gpu_screen_aligned.py.  So |got - want| <= RTOL |want| + 2 N 2^-53 max|r|, max|r| taken over the set's pixels that are not NaN (its
``epi_abs_max``, where none is); the second term matters only for the signed region mean, whose terms cancel (for ``additive_abs_mean`` the
terms are |t| >= 0, the sums' orders differ by 1e-11 relative, and the first term covers it).  NaN sits in the same places on both sides."""
import ctypes

import numpy as np
import pytest
import torch

from orca_amd import _lib, engine
from orca_amd import orca_models as M
from orca_amd import screen as S
from orca_amd._lib import OrcaHipError
from tests.test_gpu_screen_aligned import L, NB, REGIONS, RTOL, _alt, _dp, _hp, _rects, _refused
from tests.test_gpu_screen_sets import _window

pytestmark = pytest.mark.gpu

FIELDS = ("epi_profile", "epi_abs_mean", "epi_abs_max", "additive_abs_mean", "epi_region", "epi_region_abs")
SCREEN_FIELDS = ("ref_map", "ref_1d", "maps", "delta_profile", "delta_abs_mean", "delta_abs_max", "delta_1d", "delta_region", "delta_region_abs", "shift",
                 "strand_gap", "ref_strand_gap")
U_BANK = 6


def bits(t):
    a = t.cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)
    return np.ascontiguousarray(a).view(np.uint32)


def same_bits(a, b):
    return tuple(a.shape) == tuple(b.shape) and np.array_equal(bits(a), bits(b))


def close_sum(got, want, N, rmax, what=""):
    """got (float32, leading axis = sets) against want (fp64) within RTOL |want| + 2 N 2^-53 max|r| with max|r| per set; NaN in the same places.
    ``N``: the number of terms, a scalar or one per trailing column."""
    g = np.asarray(got.cpu().numpy() if isinstance(got, torch.Tensor) else got)
    assert g.dtype == np.float32, what
    g, h = g.astype(np.float64), np.asarray(want, dtype=np.float64)
    assert g.shape == h.shape, (what, g.shape, h.shape)
    assert np.array_equal(np.isnan(g), np.isnan(h)), (what, np.argwhere(np.isnan(g) != np.isnan(h))[:5])
    rm = np.nan_to_num(np.asarray(rmax, dtype=np.float64), nan=0.0).reshape((-1,) + (1,) * (h.ndim - 1))
    tol = RTOL * np.abs(h) + 2.0 * np.asarray(N, dtype=np.float64) * 2.0 ** -53 * rm
    f = ~np.isnan(h)
    err = np.abs(g - h)
    assert np.all(err[f] <= tol[f]), (what, float((err[f] / np.maximum(tol[f], 1e-300)).max()))


def _rmax(maps, bank, ref, off, mem):
    """max |r| per set over its pixels that are not NaN (the terms of the sums that are compared), from the definition"""
    out = np.zeros(len(off) - 1)
    rf = ref.astype(np.float64)
    for e in range(len(off) - 1):
        t = np.zeros_like(rf)
        for m in mem[off[e]: off[e + 1]]:
            t = t + (bank[m].astype(np.float64) - rf)
        r = np.abs((maps[e].astype(np.float64) - rf) - t)
        out[e] = np.nanmax(r) if not np.isnan(r).all() else 0.0
    return out


def equals_host(got, maps, bank, ref, off, mem, rects, what=""):
    """the six results of the kernels (or of an `EpistasisResult`) against `epistasis_scores_host` on the same maps (tensors or numpy)"""
    maps, bank, ref = (x.cpu().numpy() if isinstance(x, torch.Tensor) else x for x in (maps, bank, ref))
    n = ref.shape[0]
    hp, hm, hx, ha, hs, hb = S.epistasis_scores_host(maps, bank, ref, off, mem, rects)
    rmax = _rmax(maps, bank, ref, off, mem)
    assert np.array_equal(rmax[~np.isnan(hx)], hx[~np.isnan(hx)])                   # where no pixel is NaN it is the restatement's maximum
    prof, mean, amax, add, sg, ab = got
    g, w = amax.cpu().numpy(), hx.astype(np.float32)
    assert g.dtype == np.float32 and np.array_equal(np.isnan(g), np.isnan(w)) and np.array_equal(bits(g)[~np.isnan(g)], bits(w)[~np.isnan(w)]), (what, "max", g, w)
    close_sum(prof, hp, n, rmax, (what, "profile"))
    close_sum(mean, hm, n * n, rmax, (what, "mean"))
    close_sum(add, ha, n * n, rmax, (what, "additive mean"))
    if rects is None:
        assert sg is None and ab is None and hs is None and hb is None
        return
    area = np.array([(i1 - i0) * (j1 - j0) for i0, i1, j0, j1 in rects], dtype=np.float64)[None]
    close_sum(sg, hs, area, rmax, (what, "region"))
    close_sum(ab, hb, area, rmax, (what, "region abs"))


def _bank(rs, n, cuda, ref):
    """U_BANK maps near the reference with a batch stride above n * n"""
    buf = torch.from_numpy((0.3 * rs.randn(U_BANK, n * n + 5)).astype(np.float32)).to(cuda)
    bank = buf.as_strided((U_BANK, n, n), (n * n + 5, n, 1))
    bank += ref[None]
    return bank


def _table(sets):
    return np.cumsum([0] + [len(s) for s in sets]).astype(np.int64), np.array([m for s in sets for m in s], dtype=np.int32)


SETS = ([4], [1, 3], [0, 2, 5], [5, 0, 3, 1, 2])                                    # 1, 2, 3 and 5 members, a member list in any order


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("n", [1, 3, 50, 250, 256])
def test_kernels_equal_the_host_restatement(cuda, n, B):
    ctx = engine.get_context(cuda)
    rs = np.random.RandomState(77 * n + B)
    for g0 in range(0, len(SETS), B):
        group = SETS[g0: g0 + B]
        off, mem = _table(group)
        alt, ref = _alt(rs, len(group), n, cuda)                                    # a strided slice of a larger tensor
        bank = _bank(rs, n, cuda, ref)
        assert alt.stride(0) == n * n + 7 and bank.stride(0) == n * n + 5
        alt += ref[None]                                                            # alt - ref of the order of the members' effects
        if n >= 3:
            bank[group[0][0], 1, 2] = float("nan")                                  # one NaN pixel in the first set's first member
        got = engine.screen_epistasis_scores(ctx, alt, bank, ref, off, mem, _rects(n))
        assert tuple(got[0].shape) == (len(group), n) and tuple(got[4].shape) == (len(group), 3)
        equals_host(got, alt, bank, ref, off, mem, _rects(n), (n, group))
        if n >= 3:
            assert torch.isnan(got[1][0]) and torch.isnan(got[3][0]) and int(torch.isnan(got[0][0]).sum()) == 1
        plain = engine.screen_epistasis_scores(ctx, alt, bank, ref, off, mem)       # without rectangles: the same four, None twice
        assert plain[4] is None and plain[5] is None and all(same_bits(x, y) for x, y in zip(plain[:4], got[:4]))


@pytest.mark.parametrize("n", [50, 250, 256])
def test_a_sets_results_do_not_depend_on_the_batch(cuda, n):
    ctx = engine.get_context(cuda)
    rs = np.random.RandomState(13 * n)
    group = list(SETS[1:])
    off, mem = _table(group)
    alt, ref = _alt(rs, 3, n, cuda)
    bank = _bank(rs, n, cuda, ref)
    whole = engine.screen_epistasis_scores(ctx, alt, bank, ref, off, mem, _rects(n))
    for b in range(3):                                                              # the set alone (on a contiguous copy: another batch stride)
        o1, m1 = _table([group[b]])
        one = engine.screen_epistasis_scores(ctx, alt[b: b + 1].contiguous(), bank.contiguous(), ref, o1, m1, _rects(n))
        for w, o in zip(whole, one):
            assert same_bits(w[b], o[0]), (group[b], n)
    perm = [2, 0, 1]
    pt = torch.tensor(perm, device=cuda)
    o2, m2 = _table([group[k] for k in perm])
    moved = engine.screen_epistasis_scores(ctx, alt[pt], bank, ref, o2, m2, _rects(n))
    for w, m in zip(whole, moved):
        assert same_bits(w[pt], m), (group, n)


def test_nan_shows_in_the_sets_that_hold_the_member(cuda):
    """One NaN pixel (12, 20) in bank map 1: it shows in exactly the sets whose member list holds 1 - in their mean, maximum and additive mean, in
    row 12 of their profile and in the rectangles that hold the pixel - and changes no other bit.  One in a set's own map shows in that set
    only, and not in its additive mean."""
    ctx = engine.get_context(cuda)
    n = 50
    sets = ([0, 1], [2], [1, 3, 4], [0, 2], [4, 1], [3])
    off, mem = _table(sets)
    rects = [(0, n, 0, n), (10, 15, 18, 25), (0, 5, 0, 5), (12, 13, 20, 21), (13, 20, 20, 21)]
    rs = np.random.RandomState(9)
    alt, ref = _alt(rs, len(sets), n, cuda)
    bank = _bank(rs, n, cuda, ref)
    clean = engine.screen_epistasis_scores(ctx, alt, bank, ref, off, mem, rects)
    assert all(bool(torch.isfinite(c).all()) for c in clean)
    row, col = 12, 20
    hit = [e for e in range(len(sets)) if 1 in mem[off[e]: off[e + 1]]]
    boxes = [k for k, (i0, i1, j0, j1) in enumerate(rects) if i0 <= row < i1 and j0 <= col < j1]
    assert hit == [0, 2, 4] and boxes == [0, 1, 3]
    b2 = bank.clone()
    b2[1, row, col] = float("nan")
    got = engine.screen_epistasis_scores(ctx, alt, b2, ref, off, mem, rects)
    equals_host(got, alt, b2, ref, off, mem, rects, "bank NaN")
    for e in range(len(sets)):
        want_row = [row] if e in hit else []
        assert np.flatnonzero(np.isnan(got[0][e].cpu().numpy())).tolist() == want_row, e
        for f in (1, 2, 3):
            assert bool(torch.isnan(got[f][e])) == (e in hit), (e, f)
        for f in (4, 5):
            assert np.flatnonzero(np.isnan(got[f][e].cpu().numpy())).tolist() == (boxes if e in hit else []), (e, f)
    for g, c in zip(got, clean):                                                    # everything else keeps its bits
        keep = ~np.isnan(g.cpu().numpy())
        assert np.array_equal(bits(g)[keep], bits(c)[keep])
    a2 = alt.clone()
    a2[3, row, col] = float("nan")
    got = engine.screen_epistasis_scores(ctx, a2, bank, ref, off, mem, rects)
    equals_host(got, a2, bank, ref, off, mem, rects, "alt NaN")
    assert torch.isnan(got[1]).tolist() == [e == 3 for e in range(len(sets))] == torch.isnan(got[2]).tolist() and same_bits(got[3], clean[3])
    assert np.flatnonzero(np.isnan(got[4][3].cpu().numpy())).tolist() == boxes


# ---- argument checks: return codes only -----------------------------------------------------------------------------------------------------------------
def test_bad_arguments_are_refused_before_any_launch(cuda):
    """Every call below is refused by the host entry point's checks, so nothing of it reaches a kernel; the output buffers keep their fill."""
    lib = _lib.load()
    h = engine.get_context(cuda).handle
    null = ctypes.c_void_p(0)
    n, B, U, K = 6, 3, 4, 2
    alt = torch.zeros((B, n, n), dtype=torch.float32, device=cuda)
    bank = torch.zeros((U, n, n), dtype=torch.float32, device=cuda)
    ref = torch.zeros((n, n), dtype=torch.float32, device=cuda)
    dev = torch.zeros(512, dtype=torch.int64, device=cuda)                          # stands for every device table: never read
    outs = [torch.full((B * 64,), 7.0, dtype=torch.float32, device=cuda) for _ in range(6)]
    good_off, good_mem = np.array([0, 2, 3, 6], dtype=np.int64), np.array([0, 1, 3, 2, 0, 1], dtype=np.int32)
    good_rects = np.ascontiguousarray([[0, 2, 1, 6], [5, 6, 0, 1]] + [[0, 1, 0, 1]] * 78, dtype=np.int32)       # padded: a count above the two given reads only this array

    def ptrs(skip):
        p = {"a": _dp(alt), "bk": _dp(bank), "r": _dp(ref), "od": _dp(dev), "md": _dp(dev), "rd": _dp(dev)}
        p.update({f"o{k}": _dp(outs[k]) for k in range(6)})
        for s in skip:
            p[s] = null
        return p

    def scores(off=good_off, mem=good_mem, P=None, nb=B, nn=n, uu=U, bs=n * n, bbs=n * n, skip=(), off_host=True, mem_host=True):
        p = ptrs(skip)
        return lib.orca_screen_epistasis_scores(h, p["a"], bs, p["bk"], bbs, uu, p["r"], nb, nn, p["od"], _hp(off) if off_host else null, p["md"],
                                                _hp(mem) if mem_host else null, mem.size if P is None else P, p["o0"], p["o1"], p["o2"], p["o3"])

    def region(off=good_off, mem=good_mem, P=None, nb=B, nn=n, uu=U, bs=n * n, bbs=n * n, skip=(), off_host=True, mem_host=True, rects=good_rects, kk=K, rects_host=True):
        p = ptrs(skip)
        return lib.orca_screen_epistasis_region_scores(h, p["a"], bs, p["bk"], bbs, uu, p["r"], nb, nn, p["od"], _hp(off) if off_host else null, p["md"],
                                                       _hp(mem) if mem_host else null, mem.size if P is None else P, p["rd"], _hp(rects) if rects_host else null, kk,
                                                       p["o4"], p["o5"])

    def i64(*v):
        return np.array(v, dtype=np.int64)

    def i32(*v):
        return np.array(v, dtype=np.int32)
    for call in (scores, region):
        assert "start at" in _refused(call(off=i64(1, 2, 3, 6)))                    # offsets that do not start at 0
        assert "decrease" in _refused(call(off=i64(0, 3, 2, 6)))                    # ... are not non-decreasing
        assert "end at" in _refused(call(off=i64(0, 2, 3, 5)))                      # ... do not end at P
        assert "reach" in _refused(call(off=i64(0, 2, 3, 7)))
        assert "empty" in _refused(call(off=i64(0, 2, 2, 6)))                       # an empty set
        assert "empty" in _refused(call(off=i64(0, 0, 3, 6)))
        assert "member 5" in _refused(call(mem=i32(0, 1, 3, 2, 0, U)))              # an index outside [0, U)
        assert "member 0" in _refused(call(mem=i32(-1, 1, 3, 2, 0, 1)))
        _refused(call(nb=0))
        _refused(call(nn=0))
        _refused(call(uu=0))
        _refused(call(P=0))
        assert "strides" in _refused(call(bs=n * n - 1)) and "strides" in _refused(call(bbs=n * n - 1))
        for s in ("a", "bk", "r", "od", "md"):
            assert "NULL" in _refused(call(skip=(s,))), s
        assert "NULL" in _refused(call(off_host=False)) and "NULL" in _refused(call(mem_host=False))
    for s in ("o0", "o1", "o2", "o3"):
        assert "NULL" in _refused(scores(skip=(s,))), s
    for s in ("rd", "o4", "o5"):
        assert "NULL" in _refused(region(skip=(s,))), s
    assert "NULL" in _refused(region(rects_host=False))
    assert "rectangles" in _refused(region(kk=0)) and "rectangles" in _refused(region(kk=65))           # K outside 1 .. 64
    for bad in ([0, 2, 1, 7], [-1, 2, 1, 6], [2, 2, 1, 6], [0, 7, 0, 1]):                               # a rectangle outside [0, n), or empty
        r = good_rects.copy()
        r[1] = bad
        assert "rectangle 1" in _refused(region(rects=r))
    torch.cuda.synchronize()
    assert all(bool((o == 7).all()) for o in outs)
    # the wrapper turns the same refusals into OrcaHipError, and checks the shapes itself
    ctx = engine.get_context(cuda)
    with pytest.raises(OrcaHipError):
        engine.screen_epistasis_scores(ctx, alt, bank, ref, [0, 2, 2, 6], good_mem)
    with pytest.raises(OrcaHipError):
        engine.screen_epistasis_scores(ctx, alt, bank, ref, good_off, [0, 1, 3, 2, 0, U])
    with pytest.raises(OrcaHipError):
        engine.screen_epistasis_scores(ctx, alt, bank, ref, good_off, good_mem, [(0, 2, 1, 7)])
    with pytest.raises(ValueError):
        engine.screen_epistasis_scores(ctx, alt, bank, ref, good_off[:-1], good_mem)
    with pytest.raises(ValueError):
        engine.screen_epistasis_scores(ctx, alt, bank[:, :5, :5], ref, good_off, good_mem)


# ---- the screen ---------------------------------------------------------------------------------------------------------------------------------------
def _sets(c):
    a = S.tile_edits("mask", 800, 8_000, 40_000, 56_000)
    b = S.tile_edits("mask", 800, 8_000, 120_000, 144_000)
    assert len(a) == 2 and len(b) == 3
    pairs, index = S.pair_edits(a, b)
    pos = (50_001, 90_123, 141_000)
    assert all(c[p] < 4 for p in pos)
    hap = S.snv_set(c, [(p, int(c[p]), (int(c[p]) + 1) % 4) for p in pos], name="hap")
    return pairs + [hap, S.EditSet([b[1]])], len(pairs)


@pytest.fixture(scope="module")
def case(cuda):
    c = _window()
    assert c.size == L
    sets, n_pairs = _sets(c)
    model = M.H1esc_1M(synthetic_seed=0).to(cuda)
    win = torch.from_numpy(c).to(cuda)
    st = {}
    res = S.epistasis_1m(model, win, sets, batch=3, regions=REGIONS, keep_maps=True, stats=st)
    return c, sets, n_pairs, model, win, res, st


def _result_equals_host(res, what):
    U = res.n_singles
    maps, ref = res.screen.maps.cpu().numpy(), res.screen.ref_map.cpu().numpy()
    equals_host(tuple(getattr(res, f) for f in FIELDS), maps[U:], maps[:U], ref, res.member_off, res.members, REGIONS, what)


def test_epistasis_fields_equal_the_host_restatement(case, cuda):
    """Every new field against the numpy restatement on ``res.screen.maps`` and ``ref_map``.  Printed, not asserted (the weights are synthetic):
    the sizes of ``epi_abs_mean`` and ``additive_abs_mean`` of the pairs."""
    c, sets, n_pairs, model, win, res, st = case
    assert res.n_singles == 8 and len(res.singles) == 8 and len(sets) == 8 and tuple(res.screen.maps.shape) == (16, NB, NB)
    assert st["route"] == "two_part" and st["range_fallback_batches"] == 0 and st["two_part_batches"] == 6        # batch 3 of 16: items 6 .. 8 straddle
    assert st["epistasis_sets"] == 8 and st["epistasis_singles"] == 8 and st["bank_bytes"] == 8 * NB * NB * 4 and st["edits"] == 16
    s2, off, mem = S.epistasis_items(sets)
    assert np.array_equal(off, res.member_off) and np.array_equal(mem, res.members) and res.member_off.tolist() == [0, 2, 4, 6, 8, 10, 12, 15, 16]
    assert tuple(res.epi_profile.shape) == (8, NB) and tuple(res.epi_region.shape) == (8, len(REGIONS))
    _result_equals_host(res, "two-part")
    # the one-member set holds its single's bits, so it scores exactly zero
    k, u = 7, int(res.members[-1])
    assert torch.equal(res.screen.maps[res.n_singles + k], res.screen.maps[u])
    assert not res.epi_profile[k].any() and float(res.epi_abs_mean[k]) == 0.0 and float(res.epi_abs_max[k]) == 0.0 and float(res.additive_abs_mean[k]) > 0.0
    for e in range(n_pairs):
        print(f"pair {e} = singles {res.members[2 * e]}, {res.members[2 * e + 1]}: epi_abs_mean {float(res.epi_abs_mean[e]):.4e}, additive_abs_mean "
              f"{float(res.additive_abs_mean[e]):.4e}, ratio {float(res.epi_abs_mean[e] / res.additive_abs_mean[e]):.4e}, epi_abs_max {float(res.epi_abs_max[e]):.4e}")
    print(f"hap of three: epi_abs_mean {float(res.epi_abs_mean[6]):.4e}, additive_abs_mean {float(res.additive_abs_mean[6]):.4e}")


def test_the_screen_inside_is_screen_1m(case, cuda):
    c, sets, n_pairs, model, win, res, st = case
    st2 = {}
    plain = S.screen_1m(model, win, res.singles + sets, keep_maps=True, regions=REGIONS, stats=st2)
    for name in SCREEN_FIELDS:
        x, y = getattr(plain, name), getattr(res.screen, name)
        assert (x is None) == (y is None), name
        assert x is None or torch.equal(x, y), name
    assert plain.strand_gap is None and plain.maps is not None and plain.delta_region is not None
    for k in ("route", "edits", "set_items", "segments", "front_bases", "indel_items", "take_rows", "strands", "range_fallback_batches", "whole_window_batches"):
        assert st[k] == st2[k], k                       # what does not depend on the batch size
    assert st2["two_part_batches"] == 1 and "epistasis_sets" not in st2
    # every field has the same bits with batch = 64, and nothing is kept without keep_maps
    big = S.epistasis_1m(model, win, sets, batch=64, regions=REGIONS)
    assert big.screen.maps is None
    for f in FIELDS:
        assert same_bits(getattr(big, f), getattr(res, f)), f
    none = S.epistasis_1m(model, win, sets[:2])
    assert none.epi_region is None and none.epi_region_abs is None and none.n_singles == 3 and same_bits(none.epi_abs_mean, res.epi_abs_mean[:2])


def test_on_the_whole_window_route_and_on_both_strands(case, cuda):
    c, sets, n_pairs, model, win, res, st = case
    pick = [sets[0], sets[6], sets[7], sets[5]]
    st3 = {}
    with engine.force_safe_precision():
        ww = S.epistasis_1m(model, win, pick, batch=3, regions=REGIONS, keep_maps=True, stats=st3)
    assert st3["route"] == "whole_window" and st3["epistasis_sets"] == 4
    _result_equals_host(ww, "whole-window")
    st4 = {}
    both = S.epistasis_1m(model, win, pick, batch=3, regions=REGIONS, keep_maps=True, stats=st4, strands="both")
    assert st4["strands"] == "both" and both.screen.strand_gap is not None
    _result_equals_host(both, "both strands")                                      # on the merged maps against the merged reference
    assert not same_bits(both.epi_abs_mean, ww.epi_abs_mean)


def test_refusals(case, cuda):
    c, sets, n_pairs, model, win, res, st = case
    with pytest.raises(ValueError):
        S.epistasis_1m(model, win, [S.EditSet([S.Edit("mask", 40_000, 800), S.Edit("del", 90_000, 10)])])
    with pytest.raises(ValueError, match="split"):
        S.epistasis_1m(model, win, sets, bank_bytes=8 * NB * NB * 4 - 1)
    with pytest.raises(ValueError):
        S.epistasis_1m(model, win, [])
