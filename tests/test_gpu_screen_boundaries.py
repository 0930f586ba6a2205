"""Domain boundary calls on the MI355X (orca_screen_boundary_calls; screen.screen_1m(..., insulation=, boundaries=)).

The kernel alone, on synthetic tracks uploaded directly (it takes tracks, not maps): n at the wave seams and at the last thread, 1 to 8 widths, 1
and 5 maps, tracks with edge NaNs, an interior NaN, plateaus, shelves and quantised values (many ties), a minimum at bins 1 and n - 2, K = 0, 1,
count - 1 and n.  Every output equals `screen.boundary_calls_host` EXACTLY - the kernel only compares and subtracts once in fp32, so there is no
tolerance: integers equal, floats bit for bit, NaN in the same slots.  Then: a track's bits do not depend on the batch, a NULL strength_track
changes no list, every malformed call is refused before any launch.

The screen: 200 000 bases of synthetic H1esc_1M(synthetic_seed=0) with a handful of edits (a deletion and a tandem duplication among them),
``aligned=True``: every boundary field equals `screen.boundary_scores_host` on the returned ``insulation``, ``ref_insulation`` and ``bin_map``; unset,
nothing changes."""
import ctypes

import numpy as np
import pytest
import torch

from orca_amd import _lib, engine
from orca_amd import orca_models as M
from orca_amd import screen as S
from orca_amd._lib import OrcaHipError
from tests.test_gpu_screen_aligned import F, L, NB, REGIONS, _dp, _items, _refused
from tests.test_gpu_screen_sets import _window
from tests.test_gpu_screen_tracks import INS_FIELDS, OLD_FIELDS, same_f32
from tests.test_gpu_screen_tracks import same_bits as same_words
from tests.test_screen_indel_cpu import plan_flank

pytestmark = pytest.mark.gpu

NAN = np.float32(np.nan)
KINDS = ("quantised", "edges", "interior", "plateaus", "ends", "noise", "monotone", "all_nan", "shelf")


def same_bits(a, b):
    """the same shape, dtype and bits: `tests.test_gpu_screen_tracks.same_bits` for the 4- and 8-byte types, plain equality for the bool masks"""
    if a.dtype == torch.bool or b.dtype == torch.bool:
        return a.dtype == b.dtype and a.shape == b.shape and bool(torch.equal(a, b))
    return a.dtype == b.dtype and same_words(a, b)


def make_track(rs, n, kind):
    """one synthetic track [n] float32 of the given kind"""
    if kind == "quantised":
        t = rs.randint(0, 4, size=n).astype(np.float32) * np.float32(0.25)
    elif kind == "plateaus":
        t = np.repeat(rs.randint(0, 5, size=n).astype(np.float32), 3)[:n]
    elif kind == "shelf":
        t = np.array(([3, 2, 2, 1, 4, 4, 0] * (n // 7 + 1))[:n], dtype=np.float32)
    elif kind == "monotone":
        t = np.arange(n, dtype=np.float32)
    elif kind == "all_nan":
        t = np.full(n, NAN)
    else:
        t = rs.randn(n).astype(np.float32)
    if kind in ("edges", "interior", "quantised") and n >= 7:                # as the diamond leaves them
        w = int(rs.randint(1, max(2, n // 4)))
        t[:w] = NAN
        t[n - w:] = NAN
    if kind == "interior" and n >= 9:
        t[n // 2] = NAN
        t[rs.randint(0, n)] = NAN
    if kind == "ends" and n >= 4:                                            # minima at bins 1 and n - 2 (the same bin when n = 3)
        t[0], t[1], t[n - 2], t[n - 1] = 9.0, -9.0, -9.0, 9.0
        if n > 4:
            t[2] = t[n - 3] = 1.0
    return t


def make_tracks(n, B, W, seed=0):
    rs = np.random.RandomState(1000 * n + 10 * B + W + seed)
    t = np.stack([make_track(rs, n, KINDS[(b * W + w + seed) % len(KINDS)]) for b in range(B) for w in range(W)]).reshape(B, W, n)
    if n == 3:
        t[0, 0] = [2.0, 1.0, 3.0]                                            # the one minimum a track of 3 bins can have
    return t


def check(got, want, what):
    assert got["count"].dtype == torch.int32 and np.array_equal(got["count"].cpu().numpy(), want["count"]), (what, "count")
    assert got["bins"].dtype == torch.int32 and np.array_equal(got["bins"].cpu().numpy(), want["bins"]), (what, "bins")
    assert same_f32(got["strength"], want["strength"]), (what, "strength")
    if got["strength_track"] is not None:
        assert same_f32(got["strength_track"], want["strength_track"]), (what, "strength_track")


@pytest.mark.parametrize("B, W", [(1, 1), (5, 3), (1, 8), (5, 8)])
@pytest.mark.parametrize("n", [3, 4, 63, 64, 65, 250, 256])
def test_kernel_equals_the_host_restatement_bit_for_bit(cuda, n, B, W):
    ctx = engine.get_context(cuda)
    t = make_tracks(n, B, W)
    dev = torch.from_numpy(t).to(cuda)
    full = S.boundary_calls_host(t, S.BoundaryParams(0.0, n, 1))
    most = int(full["count"].max())
    assert most >= 1 or (B * W == 1 and n > 3)                               # every batch has a track with a boundary; the "all_nan" and "monotone" ones have none
    assert B * W < len(KINDS) or int(full["count"].min()) == 0
    for K in sorted({0, 1, max(most - 1, 1), n}):
        for ms in (0.0, 0.5, 1.0):
            got = engine.screen_boundary_calls(ctx, dev, ms, K)
            assert tuple(got["bins"].shape) == (B, W, K) and tuple(got["strength_track"].shape) == (B, W, n)
            if K == 0:
                want = S.boundary_calls_host(t, S.BoundaryParams(ms, 1, 1))
                assert np.array_equal(got["count"].cpu().numpy(), want["count"]) and same_f32(got["strength_track"], want["strength_track"])
                continue
            want = S.boundary_calls_host(t, S.BoundaryParams(ms, K, 1))
            check(got, want, (n, B, W, K, ms))
            none = engine.screen_boundary_calls(ctx, dev, ms, K, strength_track=False)              # the NULL pointer: the same lists
            assert none["strength_track"] is None
            for k in ("count", "bins", "strength"):
                assert same_bits(none[k], got[k]), (n, K, ms, k)
    if n > 4:
        ends = [(b, w) for b in range(B) for w in range(W) if KINDS[(b * W + w) % len(KINDS)] == "ends"]
        for b, w in ends:
            assert full["bins"][b, w, 0] == 1 and n - 2 in full["bins"][b, w].tolist()


def test_hand_worked_tracks_on_the_device(cuda):
    ctx = engine.get_context(cuda)
    t = np.full((1, 3, 9), NAN)
    t[0, 0] = [5, 1, 4, NAN, 4, 0, 6, 2, 9]
    t[0, 1, :4] = [3, 1, 1, 3]
    t[0, 2, :5] = [3, 2, 2, 1, 4]
    got = engine.screen_boundary_calls(ctx, torch.from_numpy(t).to(cuda), 0.0, 4)
    assert got["count"].tolist() == [[3, 1, 1]]
    assert got["bins"].tolist() == [[[1, 5, 7, -1], [1, -1, -1, -1], [3, -1, -1, -1]]]
    s = got["strength"].cpu().numpy()
    assert s[0, 0, :3].tolist() == [3.0, 4.0, 4.0] and s[0, 1, 0] == 2.0 and s[0, 2, 0] == 2.0 and np.isnan(s).sum() == 7
    st = got["strength_track"].cpu().numpy()
    assert np.flatnonzero(~np.isnan(st[0, 0])).tolist() == [1, 5, 7] and np.flatnonzero(~np.isnan(st[0, 2])).tolist() == [3]
    # fp32: the strength is ONE fp32 subtraction of two fp32 values, and min_strength is compared in fp32
    u = np.array([[[1.0, np.float32(0.1), np.float32(0.7), 0.0, 2.0]]], dtype=np.float32)
    got = engine.screen_boundary_calls(ctx, torch.from_numpy(u).to(cuda), 0.0, 5)
    assert got["bins"].tolist() == [[[1, 3, -1, -1, -1]]]
    assert same_f32(got["strength"][0, 0, :2], np.array([np.float32(0.7) - np.float32(0.1), np.float32(1.0)], dtype=np.float32))
    edge = float(np.float32(0.7) - np.float32(0.1))
    assert engine.screen_boundary_calls(ctx, torch.from_numpy(u).to(cuda), edge, 5)["count"].tolist() == [[2]]
    assert engine.screen_boundary_calls(ctx, torch.from_numpy(u).to(cuda), float(np.nextafter(np.float32(edge), np.float32(1))), 5)["count"].tolist() == [[1]]


@pytest.mark.parametrize("n", [65, 250, 256])
def test_a_tracks_bits_do_not_depend_on_the_batch(cuda, n):
    ctx = engine.get_context(cuda)
    t = make_tracks(n, 5, 3, seed=1)
    K = 7
    five = engine.screen_boundary_calls(ctx, torch.from_numpy(t).to(cuda), 0.25, K)
    for b in range(5):
        for w in range(3):
            one = engine.screen_boundary_calls(ctx, torch.from_numpy(np.ascontiguousarray(t[b: b + 1, w: w + 1])).to(cuda), 0.25, K)
            for k in ("count", "bins", "strength", "strength_track"):
                assert same_bits(one[k][0, 0], five[k][b, w]), (n, b, w, k)
    other = t[::-1].copy()                                                    # the same tracks at other places of the batch
    rev = engine.screen_boundary_calls(ctx, torch.from_numpy(other).to(cuda), 0.25, K)
    for k in ("count", "bins", "strength", "strength_track"):
        assert same_bits(rev[k].flip(0), five[k]), (n, k)


def test_bad_arguments_are_refused_before_any_launch(cuda):
    """Every call below is refused by the host entry point's checks with ORCA_EINVAL, so nothing of it reaches a kernel; the output buffers keep their
    fill."""
    lib = _lib.load()
    h = engine.get_context(cuda).handle
    null = ctypes.c_void_p(0)
    B, W, n, K = 2, 3, 20, 4
    tr = torch.from_numpy(make_tracks(257, 3, 9)).to(cuda)                      # room for every refused shape, had it been launched
    oi = [torch.full((3 * 9,), 7, dtype=torch.int32, device=cuda), torch.full((3 * 9 * 257,), 7, dtype=torch.int32, device=cuda)]
    of = [torch.full((3 * 9 * 257,), 7.0, dtype=torch.float32, device=cuda) for _ in range(2)]

    def call(ctx=h, tracks=None, nb=B, nw=W, nn=n, ms=0.1, k=K, count=None, bins=None, strength=None, st=None):
        p = lambda v, d: _dp(d) if v is None else v
        return lib.orca_screen_boundary_calls(ctx, p(tracks, tr), nb, nw, nn, ms, k, p(count, oi[0]), p(bins, oi[1]), p(strength, of[0]), p(st, of[1]))

    assert call() == 0 and call(st=null) == 0                                   # the well-formed calls are accepted (and overwrite the fill: refilled below)
    torch.cuda.synchronize()
    assert not bool((of[0][: B * W * K] == 7.0).any())
    for o in oi:
        o.fill_(7)
    for o in of:
        o.fill_(7.0)
    einval = -1                                                                 # include/orca_hip.h: ORCA_EINVAL
    for k in ("ctx", "tracks", "count", "bins", "strength"):
        rc = call(**{k: null})
        assert rc == einval and "NULL" in _refused(rc), k
    for kw, word in ((dict(nn=2), "bins"), (dict(nn=257), "bins"), (dict(nn=0), "bins"), (dict(nw=0), "W 1..8"), (dict(nw=9), "W 1..8"), (dict(nb=0), "B >= 1"),
                     (dict(nb=-1), "B >= 1"), (dict(k=-1), "K = "), (dict(k=n + 1), "K = "), (dict(ms=float("nan")), "min_strength"),
                     (dict(ms=-0.5), "min_strength"), (dict(ms=float("-inf")), "min_strength")):
        rc = call(**kw)
        assert rc == einval and word in _refused(rc), kw
    assert call(k=0) == 0 and call(k=n) == 0 and call(nn=3, k=3) == 0 and call(nn=256, nw=8, k=256) == 0 and call(ms=0.0) == 0      # the bounds themselves
    torch.cuda.synchronize()
    for o in oi:
        o.fill_(7)
    for o in of:
        o.fill_(7.0)
    for kw in (dict(nn=257), dict(nw=9), dict(k=n + 1), dict(ms=float("nan")), dict(count=null)):
        assert call(**kw) == einval
    torch.cuda.synchronize()
    assert all(bool((o == 7).all()) for o in oi + of)
    # the wrapper turns the same refusals into errors
    ctx = engine.get_context(cuda)
    good = tr[:2, :3, :20].contiguous()
    with pytest.raises(OrcaHipError, match="K = "):
        engine.screen_boundary_calls(ctx, good, 0.1, 21)
    with pytest.raises(OrcaHipError, match="min_strength"):
        engine.screen_boundary_calls(ctx, good, -1.0, 4)
    with pytest.raises(OrcaHipError, match="W 1..8"):
        engine.screen_boundary_calls(ctx, tr[:, :, :20].contiguous(), 0.1, 4)
    with pytest.raises(OrcaHipError):
        engine.screen_boundary_calls(ctx, good.cpu(), 0.1, 4)
    with pytest.raises(ValueError):
        engine.screen_boundary_calls(ctx, good[0], 0.1, 4)
    with pytest.raises(ValueError):
        engine.screen_boundary_calls(ctx, tr[:2, :3, :20], 0.1, 4)               # not contiguous


# ---- the screen ---------------------------------------------------------------------------------------------------------------------------------------
WIDTHS = (1, 3, 10)
PICK = ("snv", "inv", "del3", "del4000", "del40000", "dup8000")
CALL_FIELDS = ("ref_boundaries", "ref_boundary_strength", "ref_boundary_count", "boundaries", "boundary_strength", "boundary_count")
ALL_FIELDS = CALL_FIELDS + S.BOUNDARY_MATCH_FIELDS + tuple("aligned_" + k for k in S.BOUNDARY_MATCH_FIELDS)


@pytest.fixture(scope="module")
def case(cuda):
    c, fl = _window(), plan_flank(F)
    every = _items(c)
    items = {k: every[k] for k in PICK}
    model = M.H1esc_1M(synthetic_seed=0).to(cuda)
    win, flank = torch.from_numpy(c).to(cuda), torch.from_numpy(fl).to(cuda)
    kw = dict(regions=REGIONS, flank=flank, aligned=True, insulation=WIDTHS)
    st = {}
    res = S.screen_1m(model, win, list(items.values()), keep_maps=True, stats=st, boundaries=S.BoundaryParams(0.0, 12, 1), **kw)
    return items, model, win, kw, res, st


def equals_host(res, q, bm, what):
    want = S.boundary_scores_host(res.insulation.cpu().numpy(), res.ref_insulation.cpu().numpy(), q, bm, res.delta_insulation.cpu().numpy(),
                                  None if bm is None else res.aligned_insulation.cpu().numpy())
    assert res.boundary_params == S.check_boundaries(q, NB)
    for name in ALL_FIELDS:
        got = getattr(res, name)
        if name.startswith("aligned_") and bm is None:
            assert got is None, (what, name)
            continue
        g, w = got.cpu().numpy(), want[name]
        assert g.shape == w.shape and g.dtype == w.dtype, (what, name, g.shape, w.shape, g.dtype, w.dtype)
        assert same_f32(g, w) if g.dtype == np.float32 else np.array_equal(g, w), (what, name)


def test_screen_boundary_fields_equal_the_host_restatement(case, cuda):
    """Printed, not asserted (the weights are synthetic): the reference's boundaries and what the 40 000-base deletion and the duplication do to them."""
    items, model, win, kw, res, st = case
    lst = list(items.values())
    host = np.stack([S.bin_map(v, L, F) for v in lst])
    q = S.BoundaryParams(0.0, 12, 1)
    assert np.array_equal(res.bin_map.cpu().numpy(), host) and st["boundaries"] == 12 and st["insulation_widths"] == 3
    E, W, K = len(lst), len(WIDTHS), 12
    assert tuple(res.ref_boundaries.shape) == (W, K) and tuple(res.boundaries.shape) == (E, W, K) and tuple(res.boundary_count.shape) == (E, W)
    assert tuple(res.boundaries_lost.shape) == (E, W) and tuple(res.aligned_boundary_delta.shape) == (E, W, K)
    equals_host(res, q, host, "min_strength 0")
    assert int(res.ref_boundary_count.min()) >= 1                              # a track of 50 - 2 w bins of a random map has minima
    # where the bin map is the identity the aligned forms hold the plain fields' bits
    for name in ("snv", "inv", "del3"):
        k = list(items).index(name)
        for f in S.BOUNDARY_MATCH_FIELDS:
            assert same_bits(getattr(res, "aligned_" + f)[k], getattr(res, f)[k]), (name, f)
    # the deletion: reference boundaries well inside the deleted span (reference bins 15 .. 24) are unmapped through the bin map, never lost
    k40 = list(items).index("del40000")
    rb = res.ref_boundaries.cpu().numpy()
    inside = (rb >= 16) & (rb <= 23)
    assert (res.aligned_ref_boundary_is_unmapped[k40].cpu().numpy()[inside]).all() and not (res.aligned_ref_boundary_is_lost[k40].cpu().numpy() & inside).any()
    for name in ("del40000", "dup8000"):
        k = list(items).index(name)
        print(name, "ref boundaries (w = 3)", rb[1][rb[1] >= 0].tolist(), "strengths", [f"{x:.4f}" for x in res.ref_boundary_strength[1].tolist() if x == x],
              "followed at", res.aligned_boundary_followed_at[k, 1].tolist(), "lost", int(res.aligned_boundaries_lost[k, 1]), "gained",
              int(res.aligned_boundaries_gained[k, 1]), "unmapped", int(res.aligned_ref_boundary_is_unmapped[k, 1].sum()))
    # the defaults, in batches of 4, without aligned: the same rule, the aligned forms None
    small = S.screen_1m(model, win, lst, batch=4, flank=kw["flank"], insulation=WIDTHS, boundaries=True)
    equals_host(small, True, None, "defaults")
    assert small.boundary_params == S.BoundaryParams(float(np.float32(0.1)), 32, 1) and tuple(small.boundaries.shape) == (E, W, 32)
    assert same_bits(small.insulation, res.insulation)
    # a truncated list keeps the full count
    few = S.screen_1m(model, win, lst[:2], flank=kw["flank"], insulation=WIDTHS, boundaries=S.BoundaryParams(0.0, 1, 1))
    assert same_bits(few.boundary_count, res.boundary_count[:2]) and same_bits(few.boundaries[:, :, 0], res.boundaries[:2, :, 0])
    equals_host(few, S.BoundaryParams(0.0, 1, 1), None, "K = 1")


def test_boundaries_change_nothing_else(case, cuda):
    items, model, win, kw, res, st = case
    lst = list(items.values())
    st2 = {}
    plain = S.screen_1m(model, win, lst, keep_maps=True, stats=st2, **kw)
    for name in OLD_FIELDS + INS_FIELDS + ("insulation_widths",):
        x, y = getattr(plain, name), getattr(res, name)
        assert x is not None and y is not None and same_bits(x, y), name
    for name in S.ScreenResult.__dataclass_fields__:
        if "boundar" in name:
            assert getattr(plain, name) is None and getattr(res, name) is not None, name
        elif name != "edits":
            x, y = getattr(plain, name), getattr(res, name)
            assert (x is None) == (y is None) and (x is None or not isinstance(x, torch.Tensor) or same_bits(x, y)), name
    assert sorted(n for n in S.ScreenResult.__dataclass_fields__ if "boundar" in n) == sorted(ALL_FIELDS + ("boundary_params",))
    assert st2["boundaries"] == 0 and {k: v for k, v in st.items() if k != "boundaries"} == {k: v for k, v in st2.items() if k != "boundaries"}
    off = S.screen_1m(model, win, lst[:2], flank=kw["flank"], insulation=WIDTHS, boundaries=False)
    assert off.boundaries is None and off.boundary_params is None
    with pytest.raises(ValueError, match="insulation"):
        S.screen_1m(model, win, lst[:1], boundaries=True)
    with pytest.raises(ValueError, match="max_calls"):
        S.screen_1m(model, win, lst[:1], insulation=WIDTHS, boundaries=S.BoundaryParams(0.1, NB + 1, 1))


def test_boundaries_on_both_strands_come_from_the_merged_maps(case, cuda):
    items, model, win, kw, res, st = case
    it = [items[k] for k in ("del40000", "dup8000", "snv")]
    host = np.stack([S.bin_map(v, L, F) for v in it])
    q = S.BoundaryParams(0.0, 12, 1)
    both = S.screen_1m(model, win, it, flank=kw["flank"], aligned=True, strands="both", insulation=WIDTHS, boundaries=q)
    equals_host(both, q, host, "both strands")                                # on the merged maps' tracks
    assert not same_bits(both.ref_boundary_strength, res.ref_boundary_strength)
