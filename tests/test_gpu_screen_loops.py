"""Loop (dot) calls of the 1 Mb mutagenesis screen on the MI355X (orca_screen_dot_calls, orca_screen_dot_enrichment): the two entry points against
the numpy restatements `screen.dot_enrichment_host` / `dot_calls_host`, bit-for-bit invariance to the batch, where a NaN pixel shows, the entry
points' argument checks (return codes only: nothing malformed reaches a kernel), and ``screen_1m(..., loops=)`` end to end on a 200 000-base window
with 40 000 bases of flank (synthetic H1esc_1M(synthetic_seed=0)) on every route and on both strands.

Exact inputs: maps quantised to multiples of 2^-12 with |x| < 8.  Every fp64 sum of at most 33^2 such values is exact whatever its order, the one
division per set and the one rounding to fp32 are correctly rounded on both sides, so kernel and restatement must agree bit for bit: the same
``count``, the same (i, j) lists, the same bits of e.
Unquantised maps: |got - want| <= RTOL |want| + 2 (2 w + 1)^2 2^-53 max|pixel|.  RTOL = 2.4e-7, two fp32 ulps, is the RTOL of
tests/test_gpu_screen_aligned.py; the second term bounds what a different order of the at most (2 w + 1)^2 fp64 additions of a set can move a sum
(the bound tests/test_gpu_screen_tracks.py derives), both sides counted, and the division by the count only shrinks it."""
import ctypes

import numpy as np
import pytest
import torch

from orca_amd import _lib, engine
from orca_amd import orca_models as M
from orca_amd import screen as S
from orca_amd._lib import OrcaHipError
from tests.test_gpu_screen_aligned import F, L, NB, REGIONS, RTOL, _dp, _hp, _refused
from tests.test_gpu_screen_sets import _window
from tests.test_gpu_screen_tracks import INS_FIELDS, OLD_FIELDS, VIEW_FIELDS, same_bits
from tests.test_screen_indel_cpu import plan_flank
from tests.test_screen_sets_cpu import snv

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -53
PARAMS = [(0, 1), (1, 4), (3, 16)]
LOOP_RESULT_FIELDS = ("ref_loops", "ref_loop_enrichment", "loops", "loop_enrichment", "loop_count") + S.LOOP_FIELDS
ALIGNED_LOOP_FIELDS = tuple("aligned_" + k for k in S.LOOP_FIELDS)


def _np(t):
    return t.cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)


def strided(a, cuda):
    """maps [B, n, n] (numpy) on the device with batch stride n * n + 7"""
    B, n = a.shape[0], a.shape[1]
    buf = torch.zeros((B, n * n + 7), dtype=torch.float32, device=cuda)
    buf[:, : n * n] = torch.from_numpy(a.reshape(B, n * n)).to(cuda)
    return buf.as_strided((B, n, n), (n * n + 7, n, 1))


def quantised(rs, B, n):
    return (np.clip(np.round(rs.randn(B, n, n) * 4096.0), -32767, 32767) / 4096.0).astype(np.float32)


def same_f32(got, want):
    g, w = _np(got), _np(want)
    return g.dtype == w.dtype == np.float32 and g.shape == w.shape and np.array_equal(np.isnan(g), np.isnan(w)) and np.array_equal(g[~np.isnan(g)], w[~np.isnan(w)])


def pixel_lists(rs, host, n, Q):
    """Q pixels per map: the map's listed dots, (-1, -1), pixels on and below the diagonal, the corners, and random ones"""
    B = host["ij"].shape[0]
    px = rs.randint(0, n, (B, Q, 2)).astype(np.int32)
    k = min(Q // 2, host["ij"].shape[1])
    px[:, :k] = host["ij"][:, :k]
    px[:, k] = -1
    px[:, k + 1] = (n - 1, 0)
    px[:, k + 2] = (0, n - 1)
    px[:, k + 3] = (n // 2, n // 2)
    px[:, k + 4] = (-1, n - 1)
    return px


def tolerance(want, w, pix):
    return RTOL * np.abs(want) + 2 * (2 * w + 1) ** 2 * EPS * pix


def close(got, want, w, pix, what):
    g, h = _np(got).astype(np.float64), np.asarray(want, dtype=np.float64)
    assert g.shape == h.shape and np.array_equal(np.isnan(g), np.isnan(h)), what
    f = ~np.isnan(h)
    err, tol = np.abs(g[f] - h[f]), tolerance(h[f], w, pix)
    assert np.all(err <= tol), (what, float((err / tol).max()))
    return float((err / tol).max()) if err.size else 0.0


# ---- (a) exact inputs: bit for bit ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("n", [1, 5, 6, 50, 250, 256])
def test_kernels_equal_the_host_restatement_bit_for_bit(cuda, n, B):
    ctx = engine.get_context(cuda)
    rs = np.random.RandomState(31 * n + B)
    a = quantised(rs, B, n)
    a[0, n // 2:, : n // 2 + 1] = np.nan                                # below the diagonal: never read
    alt = strided(a, cuda)
    assert alt.stride(0) == n * n + 7 or B == 1
    for (p, w) in PARAMS:
        fits = n >= 4 * w + 2
        for r, T, K, d_min in ((2, 0.0, 4096, None), (1, -1.0, 16, 2 * w + 4), (16, 1.0, 64, None)):
            if r == 16 and not (fits and n <= 50 or (n == 256 and w == 4)):
                continue
            q = S.LoopParams(p=p, w=w, r=r, threshold=T, d_min=d_min, max_calls=K)
            host = S.dot_calls_host(a, q)
            got = engine.screen_dot_calls(ctx, alt, p, w, r, T, K, d_min)
            what = (n, B, p, w, r, T, K, d_min)
            assert got["count"].dtype == torch.int32 and got["ij"].dtype == torch.int32 and tuple(got["ij"].shape) == (B, K, 2)
            assert np.array_equal(_np(got["count"]), host["count"]), (what, _np(got["count"]), host["count"])
            assert np.array_equal(_np(got["ij"]), host["ij"]), what
            assert same_f32(got["enrich"], host["enrich"]) and same_f32(got["e_map"], host["e_map"]), what
            if not fits:
                assert not host["count"].any() and np.isnan(host["e_map"]).all()
            elif n >= 50 and w <= 4 and r == 1:
                assert (host["count"] > K).all()                        # truncated: count is still the total
            elif n >= 50 and w <= 4 and r == 2:
                assert (host["count"] > 0).all() and (host["count"] < K).all()
            if r == 16:
                continue
            Q = 257 if n >= 50 else 9
            px = pixel_lists(rs, host, n, Q)
            e = engine.screen_dot_enrichment(ctx, alt, px, p, w, d_min)
            want = np.full((B, Q), np.nan, dtype=np.float32)
            ok = (px >= 0).all(axis=2)
            bb = np.broadcast_to(np.arange(B)[:, None], (B, Q))
            want[ok] = host["e_map"][bb[ok], px[ok][:, 0], px[ok][:, 1]]
            assert same_f32(e, want), what
            listed = min(Q // 2, K, int(host["count"].min()))
            assert not np.isnan(want[:, :listed]).any()
    if n == 6:                                                          # the smallest map with an eligible pixel: exactly one, (1, 4)
        got = engine.screen_dot_calls(ctx, alt, 0, 1, 1, -100.0, 4)
        assert got["count"].tolist() == [1] * B and got["ij"][:, 0].tolist() == [[1, 4]] * B and torch.isnan(got["e_map"]).sum().item() == B * 35


def test_a_block_of_ones_and_a_constant_map(cuda):
    ctx = engine.get_context(cuda)
    m = torch.zeros((2, 30, 30), dtype=torch.float32, device=cuda)
    m[0, 9:12, 19:22] = 1.0
    m[1] = 0.375
    got = engine.screen_dot_calls(ctx, m, 1, 3, 2, 0.5, 8)
    assert got["count"].tolist() == [1, 0] and got["ij"][0, 0].tolist() == [10, 20] and float(got["enrich"][0, 0]) == 1.0
    assert (got["ij"][0, 1:] == -1).all() and (got["ij"][1] == -1).all() and torch.isnan(got["enrich"][0, 1:]).all() and torch.isnan(got["enrich"][1]).all()
    got = engine.screen_dot_calls(ctx, m, 1, 3, 2, 0.0, 8, 9)           # T = 0: the constant map has exactly one dot, (w, w + d_min)
    assert got["count"].tolist()[1] == 1 and got["ij"][1, 0].tolist() == [3, 12] and float(got["enrich"][1, 0]) == 0.0


# ---- (b) unquantised maps: the enrichment within the derived bound ------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("n", [50, 250, 256])
def test_enrichment_of_random_maps_is_within_the_bound(cuda, n, B):
    ctx = engine.get_context(cuda)
    rs = np.random.RandomState(77 * n + B)
    a = rs.randn(B, n, n).astype(np.float32)
    alt = strided(a, cuda)
    pix = float(np.abs(a).max())
    worst = 0.0
    for (p, w) in PARAMS:
        if n < 4 * w + 2:
            continue
        q = S.LoopParams(p=p, w=w)
        want = S.dot_enrichment_host(a, q)
        got = engine.screen_dot_calls(ctx, alt, p, w, 2, 0.5, 64)
        worst = max(worst, close(got["e_map"], want, w, pix, (n, B, p, w, "e_map")))
        px = rs.randint(-1, n, (B, 300, 2)).astype(np.int32)
        ok = (px >= 0).all(axis=2)
        h = np.full((B, 300), np.nan, dtype=np.float32)
        bb = np.broadcast_to(np.arange(B)[:, None], (B, 300))
        h[ok] = want[bb[ok], px[ok][:, 0], px[ok][:, 1]]
        e = engine.screen_dot_enrichment(ctx, alt, px, p, w)
        worst = max(worst, close(e, h, w, pix, (n, B, p, w, "listed pixels")))
        assert (~np.isnan(h)).sum() > 20
        g = _np(got["e_map"])                                           # one device function: the listed pixels hold the map's bits
        assert same_f32(e, np.where(ok, g[bb, np.maximum(px[..., 0], 0), np.maximum(px[..., 1], 0)], np.float32(np.nan)).astype(np.float32))
    print(f"n = {n}, B = {B}: largest error / tolerance {worst:.3g}")


# ---- (c) invariance to the batch -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [50, 250, 256])
def test_a_maps_results_do_not_depend_on_the_batch(cuda, n):
    """A map alone (contiguous) against the same map as row 0, 1 and 2 of a batch of three with batch stride n * n + 7 and other maps beside it."""
    ctx = engine.get_context(cuda)
    rs = np.random.RandomState(5 * n)
    one = torch.from_numpy(rs.randn(1, n, n).astype(np.float32)).to(cuda)
    batch = strided(rs.randn(3, n, n).astype(np.float32), cuda)
    px = rs.randint(-1, n, (1, 200, 2)).astype(np.int32)
    px3 = rs.randint(-1, n, (3, 200, 2)).astype(np.int32)
    for (p, w) in PARAMS:
        if n < 4 * w + 2:
            continue
        alone = engine.screen_dot_calls(ctx, one, p, w, 2, -0.25, 32)
        alone_e = engine.screen_dot_enrichment(ctx, one, px, p, w)
        assert int(alone["count"][0]) > 0 or w == 16
        for row in range(3):
            batch[row] = one[0]                                         # the rows written earlier stay, as other maps
            got = engine.screen_dot_calls(ctx, batch, p, w, 2, -0.25, 32)
            assert torch.equal(got["count"][row], alone["count"][0]) and torch.equal(got["ij"][row], alone["ij"][0]), (n, p, w, row)
            assert same_bits(got["enrich"][row], alone["enrich"][0]) and same_bits(got["e_map"][row], alone["e_map"][0]), (n, p, w, row)
            p3 = px3.copy()
            p3[row] = px[0]
            assert same_bits(engine.screen_dot_enrichment(ctx, batch, p3, p, w)[row], alone_e[0]), (n, p, w, row)


# ---- (d) NaN locality --------------------------------------------------------------------------------------------------------------------------------
def test_nan_shows_in_the_windows_that_hold_it(cuda):
    ctx = engine.get_context(cuda)
    n, p, w = 50, 1, 4
    rs = np.random.RandomState(9)
    alt = strided(rs.randn(2, n, n).astype(np.float32), cuda)
    clean = engine.screen_dot_calls(ctx, alt, p, w, 2, 0.3, 64)
    quiet = alt.clone()
    quiet[:, 30, 8] = float("nan")                                      # below the diagonal
    quiet[0, 20, 20] = float("nan")                                     # on it
    quiet[1, 40, 39] = float("nan")
    got = engine.screen_dot_calls(ctx, quiet, p, w, 2, 0.3, 64)
    for k in ("count", "ij", "enrich", "e_map"):
        assert same_bits(got[k], clean[k]), k
    a3 = alt.clone()
    a3[1, 12, 30] = float("nan")
    got = engine.screen_dot_calls(ctx, a3, p, w, 2, 0.3, 64)
    new = (torch.isnan(got["e_map"]) & ~torch.isnan(clean["e_map"])).cpu().numpy()
    want = {(1, i, j) for i in range(n) for j in range(n) if w <= i and j <= n - 1 - w and j - i >= 2 * w + 1 and abs(i - 12) <= w and abs(j - 30) <= w}
    assert {tuple(v) for v in np.argwhere(new)} == want and len(want) == 81
    keep = ~torch.isnan(got["e_map"])
    assert torch.equal(got["e_map"][keep], clean["e_map"][keep])        # every other value keeps its bits
    host = S.dot_calls_host(a3.cpu().numpy(), S.LoopParams(p=p, w=w, r=2, threshold=0.3))
    assert np.array_equal(np.isnan(host["e_map"]), np.isnan(_np(got["e_map"])))
    assert np.array_equal(_np(got["count"]), host["count"]) and np.array_equal(_np(got["ij"]), host["ij"])   # a NaN neighbour neither wins nor loses
    px = np.array([[[12, 30], [8, 26], [16, 34], [7, 30], [12, 35]]] * 2, dtype=np.int32)
    e = engine.screen_dot_enrichment(ctx, a3, px, p, w)
    assert torch.isnan(e[1]).tolist() == [True, True, True, False, False] and not torch.isnan(e[0]).any()


# ---- (e) argument checks: return codes only ------------------------------------------------------------------------------------------------------------
def test_bad_arguments_are_refused_before_any_launch(cuda):
    """Every call below is refused by the host entry point's checks, so nothing of it reaches a kernel; the output buffers keep their fill."""
    lib = _lib.load()
    h = engine.get_context(cuda).handle
    null = ctypes.c_void_p(0)
    n, B, K = 20, 2, 8
    maps = torch.zeros((B, n, n), dtype=torch.float32, device=cuda)
    big = 257 * 257
    e_map = torch.full((B * big,), 7.0, dtype=torch.float32, device=cuda)
    cnt = torch.full((B,), 7, dtype=torch.int32, device=cuda)
    ij = torch.full((B * 4096 * 2,), 7, dtype=torch.int32, device=cuda)
    en = torch.full((B * 4096,), 7.0, dtype=torch.float32, device=cuda)
    pxd = torch.zeros((B * 4096 * 2,), dtype=torch.int32, device=cuda)      # stands for the device pixel list: never read
    good = np.ascontiguousarray([[[4, 15], [-1, -1], [19, 0]]] * B, dtype=np.int32)

    def calls(m=_dp(maps), bs=n * n, nb=B, nn=n, p=1, w=4, d=9, r=2, T=0.25, k=K, em=_dp(e_map), c=_dp(cnt), i=_dp(ij), e=_dp(en)):
        return lib.orca_screen_dot_calls(h, m, bs, nb, nn, p, w, d, r, T, k, em, c, i, e)

    def listed(m=_dp(maps), bs=n * n, nb=B, nn=n, p=1, w=4, d=9, dev=_dp(pxd), host=good, Q=3, o=_dp(en)):
        return lib.orca_screen_dot_enrichment(h, m, bs, nb, nn, p, w, d, dev, null if host is None else _hp(host), Q, o)
    for c in (calls, listed):
        assert "0 <= p < w" in _refused(c(p=-1))
        assert "0 <= p < w" in _refused(c(p=4))
        assert "0 <= p < w" in _refused(c(p=5))
        assert "0 <= p < w" in _refused(c(p=0, w=0, d=1))
        assert "0 <= p < w" in _refused(c(w=17, d=35))
        assert "d_min" in _refused(c(d=8))
        assert "d_min" in _refused(c(d=-3))
        _refused(c(nn=257, bs=big))                                     # n = 257
        _refused(c(nn=0))
        _refused(c(nb=0))
        _refused(c(nb=-1))
        assert "batch stride" in _refused(c(bs=n * n - 1))              # map_bs < n * n
        assert "NULL" in _refused(c(m=null))
    for k in ("em", "c", "i", "e"):
        assert "NULL" in _refused(calls(**{k: null})), k
    for r in (0, -1, 17):
        assert "radius" in _refused(calls(r=r))
    for k in (0, -1, 4097):
        assert "K =" in _refused(calls(k=k))
    assert "NaN" in _refused(calls(T=float("nan")))
    assert "NULL" in _refused(listed(dev=null))
    assert "NULL" in _refused(listed(host=None))                        # a device list without its host copy
    assert "NULL" in _refused(listed(o=null))
    for Q in (0, -1, 4097):
        assert "Q =" in _refused(listed(Q=Q))
    for v in (n, -2, 300):                                              # a host list that holds a coordinate outside -1 .. n - 1
        bad = good.copy()
        bad[1, 2, 1] = v
        assert "outside -1" in _refused(listed(host=bad)), v
    torch.cuda.synchronize()
    assert bool((e_map == 7).all()) and bool((cnt == 7).all()) and bool((ij == 7).all()) and bool((en == 7).all())
    # the wrappers turn the same refusals into errors
    ctx = engine.get_context(cuda)
    for kw in (dict(p=4), dict(w=17), dict(r=0), dict(max_calls=0), dict(max_calls=4097), dict(d_min=8), dict(threshold=float("nan"))):
        a = dict(p=1, w=4, r=2, threshold=0.25, max_calls=8, d_min=None)
        a.update(kw)
        with pytest.raises(OrcaHipError):
            engine.screen_dot_calls(ctx, maps, **a)
    bad = good.copy()
    bad[0, 0, 0] = n
    with pytest.raises(OrcaHipError):
        engine.screen_dot_enrichment(ctx, maps, bad, 1, 4)
    with pytest.raises(ValueError):
        engine.screen_dot_enrichment(ctx, maps, good[:1], 1, 4)
    with pytest.raises(ValueError):
        engine.screen_dot_calls(ctx, maps[:0], 1, 4, 2, 0.25, 8)
    with pytest.raises(ValueError):
        engine.screen_dot_calls(ctx, maps[:, :, :10], 1, 4, 2, 0.25, 8)


# ---- (f) the screen -----------------------------------------------------------------------------------------------------------------------------------
W, P, R_MAX, K_CALLS = 3, 1, 2, 32


def _loop_items(c):
    tiles = S.tile_edits("mask", 2_000, 2_000, 100_000, 106_000)
    assert len(tiles) == 3
    return {"snv": snv(c, 77_777), "snv2": snv(c, 140_001, 2), "mask0": tiles[0], "mask1": tiles[1], "mask2": tiles[2], "inv": S.Edit("inv", 150_000, 1_300),
            "del40000": S.Edit("del", 60_000, 40_000), "del4000": S.Edit("del", 90_500, 4_000),
            "ins6000": S.Edit("ins", 30_100, np.random.RandomState(4).randint(0, 4, 6_000).astype(np.uint8)),
            "ins12000": S.Edit("ins", 120_000, np.random.RandomState(8).randint(0, 4, 12_000).astype(np.uint8))}


def pick_threshold(ref_map):
    """T from the host e of the reference map: the midpoint of the widest gap among its 20 largest local maxima - of the gaps that leave at
    least 3 maxima above them, since the comparison needs at least 3 reference dots (on the synthetic weights the widest gap of all is behind
    the second maximum)"""
    every = S.dot_calls_host(ref_map[None], S.LoopParams(p=P, w=W, r=R_MAX, threshold=-np.inf, max_calls=4096))
    c = int(every["count"][0])
    top = np.sort(every["enrich"][0, :c].astype(np.float64))[::-1][:20]
    assert top.size >= 4, top
    gaps = top[:-1] - top[1:]
    g = 2 + int(np.argmax(gaps[2:]))
    print("the largest local maxima of the reference's enrichment:", np.round(top, 4).tolist(), "-> the widest gap is behind", g + 1)
    return float(np.float32(0.5 * (top[g] + top[g + 1])))


def unsafe_items(maps, q, pix):
    """the maps with a host e within the tolerance of T, or a candidate dot within the tolerance of a neighbour it competes with"""
    e = S.dot_enrichment_host(maps, q).astype(np.float64)
    tol = tolerance(e, q.w, pix)
    T, r, n = float(np.float32(q.threshold)), q.r, e.shape[1]
    with np.errstate(invalid="ignore"):
        bad = (np.abs(e - T) <= tol).any(axis=(1, 2))
        cand = e >= T - tol
        pad = np.full((e.shape[0], n + 2 * r, n + 2 * r), np.nan)
        pad[:, r: r + n, r: r + n] = e
        for di in range(-r, r + 1):
            for dj in range(-r, r + 1):
                if (di, dj) != (0, 0):
                    f = pad[:, r + di: r + di + n, r + dj: r + dj + n]
                    bad |= (cand & (np.abs(e - f) <= tol + tolerance(f, q.w, pix))).any(axis=(1, 2))
    return bad


def equals_host(res, q, bm, what):
    """every loop field of ``res`` against `screen.loop_scores_host` of its own kept maps"""
    maps, ref = res.maps.cpu().numpy(), res.ref_map.cpu().numpy()
    E = maps.shape[0]
    pix = float(max(np.abs(maps).max(), np.abs(ref).max()))
    host = S.loop_scores_host(maps, ref, q, bm)
    assert host["ref_loop_count"] >= 3, (what, host["ref_loop_count"])
    skip = unsafe_items(maps, q, pix)
    assert not unsafe_items(ref[None], q, pix).any(), what
    assert skip.sum() * 10 <= E, (what, skip)
    ok = ~skip
    R = host["ref_loops"].shape[0]
    assert res.loop_params == q and res.ref_loop_count == host["ref_loop_count"] and R == min(res.ref_loop_count, q.max_calls)
    assert np.array_equal(_np(res.ref_loops), host["ref_loops"]) and res.ref_loops.dtype == torch.int32
    close(res.ref_loop_enrichment, host["ref_loop_enrichment"], q.w, pix, (what, "ref_loop_enrichment"))
    assert np.array_equal(_np(res.loops)[ok], host["loops"][ok]) and np.array_equal(_np(res.loop_count)[ok], host["loop_count"][ok]), what
    close(_np(res.loop_enrichment)[ok], host["loop_enrichment"][ok], q.w, pix, (what, "loop_enrichment"))
    for pre in ("", "aligned_") if bm is not None else ("",):
        d, hd = _np(getattr(res, pre + "loop_delta")).astype(np.float64), host[pre + "loop_delta"].astype(np.float64)
        assert d.shape == hd.shape == (E, R) and np.array_equal(np.isnan(d), np.isnan(hd)), (what, pre)
        f = ~np.isnan(hd)                                               # a difference of two enrichments: both tolerances
        tol = tolerance(hd + host["ref_loop_enrichment"][None], q.w, pix) + tolerance(host["ref_loop_enrichment"], q.w, pix)[None] + RTOL * np.abs(hd)
        assert np.all(np.abs(d - hd)[f] <= tol[f]), (what, pre, "loop_delta")
        for k in ("loops_gained", "loops_lost", "loop_is_gained", "ref_loop_is_lost"):
            g = _np(getattr(res, pre + k))
            assert g.shape == host[pre + k].shape and g.dtype == host[pre + k].dtype and np.array_equal(g[ok], host[pre + k][ok]), (what, pre + k)
    if bm is None:
        assert all(getattr(res, k) is None for k in ALIGNED_LOOP_FIELDS)
    return host, skip


@pytest.fixture(scope="module")
def case(cuda):
    c, fl = _window(), plan_flank(F)
    items = _loop_items(c)
    model = M.H1esc_1M(synthetic_seed=0).to(cuda)
    win, flank = torch.from_numpy(c).to(cuda), torch.from_numpy(fl).to(cuda)
    lst = list(items.values())
    st0 = {}
    plain = S.screen_1m(model, win, lst, keep_maps=True, stats=st0, regions=REGIONS, flank=flank, aligned=True, insulation=[3], viewpoints=[10])
    q = S.LoopParams(p=P, w=W, r=R_MAX, threshold=pick_threshold(plain.ref_map.cpu().numpy()), max_calls=K_CALLS, tol=1)
    st = {}
    res = S.screen_1m(model, win, lst, keep_maps=True, stats=st, regions=REGIONS, flank=flank, aligned=True, insulation=[3], viewpoints=[10], loops=q)
    return c, items, model, win, flank, plain, st0, q, res, st


def test_screen_loop_fields_equal_the_host_restatement(case, cuda):
    c, items, model, win, flank, plain, st0, q, res, st = case
    lst = list(items.values())
    bm = np.stack([S.bin_map(v, L, F) for v in lst])
    assert st["route"] == "two_part" and st["loops"] == K_CALLS
    q = S.check_loops(q, NB)
    host, skip = equals_host(res, q, bm, "two-part")
    assert st["loop_truncated_items"] == int((host["loop_count"] > K_CALLS).sum())
    for name in ("snv", "snv2", "mask0", "mask1", "mask2", "inv"):      # identity bin maps: the aligned fields hold the plain fields' bits
        k = list(items).index(name)
        assert np.array_equal(bm[k], np.arange(NB))
        assert same_bits(res.aligned_loop_delta[k], res.loop_delta[k]) and torch.equal(res.aligned_loop_is_gained[k], res.loop_is_gained[k]), name
        assert torch.equal(res.aligned_ref_loop_is_lost[k], res.ref_loop_is_lost[k]) and int(res.aligned_loops_lost[k]) == int(res.loops_lost[k]), name
    k40 = list(items).index("del40000")                                 # reference bins 15 .. 24 deleted: a reference dot anchored there has no alt pixel
    ref_ij = host["ref_loops"]
    gone = ((ref_ij >= 15) & (ref_ij < 25)).any(axis=1)
    assert torch.isnan(res.aligned_loop_delta[k40])[torch.from_numpy(gone).to(cuda)].all()
    print("reference dots:", ref_ij.tolist(), "e", np.round(host["ref_loop_enrichment"], 4).tolist(), "T", q.threshold, "skipped items", int(skip.sum()))
    print("per item (count, gained, lost | aligned gained, lost):", {k: (int(res.loop_count[i]), int(res.loops_gained[i]), int(res.loops_lost[i]),
                                                                        int(res.aligned_loops_gained[i]), int(res.aligned_loops_lost[i])) for i, k in enumerate(items)})
    # batches of 3: the same bits
    small = S.screen_1m(model, win, lst, batch=3, flank=flank, aligned=True, loops=q)
    for k in LOOP_RESULT_FIELDS + ALIGNED_LOOP_FIELDS:
        x, y = getattr(small, k), getattr(res, k)
        assert (same_bits(x, y) if x.dtype == torch.float32 else torch.equal(x, y)), k
    # without aligned: the aligned fields are None, the others the same bits; truncation is counted
    st2 = {}
    cut = S.screen_1m(model, win, lst, keep_maps=True, stats=st2, flank=flank, loops=S.LoopParams(p=P, w=W, r=R_MAX, threshold=-10.0, max_calls=2, tol=1))
    assert st2["loops"] == 2 and st2["loop_truncated_items"] == len(lst) and (cut.loop_count > 2).all() and cut.ref_loop_count > 2 and tuple(cut.ref_loops.shape) == (2, 2)
    assert all(getattr(cut, k) is None for k in ALIGNED_LOOP_FIELDS) and tuple(cut.loops.shape) == (len(lst), 2, 2) and (cut.loops >= 0).all()


def test_loops_change_nothing_else(case, cuda):
    c, items, model, win, flank, plain, st0, q, res, st = case
    lst = list(items.values())
    none = S.screen_1m(model, win, lst, keep_maps=True, regions=REGIONS, flank=flank, aligned=True, insulation=[3], viewpoints=[10], loops=None)
    for other in (none, res):
        for name in OLD_FIELDS + INS_FIELDS + VIEW_FIELDS:
            x, y = getattr(plain, name), getattr(other, name)
            assert x is not None and y is not None, name
            assert same_bits(x, y), name
    for name in ("loop_params", "ref_loop_count") + LOOP_RESULT_FIELDS + ALIGNED_LOOP_FIELDS:
        assert getattr(plain, name) is None and getattr(none, name) is None and getattr(res, name) is not None, name
    assert st0["loops"] == 0 and st0["loop_truncated_items"] == 0
    assert {k: v for k, v in st.items() if not k.startswith("loop")} == {k: v for k, v in st0.items() if not k.startswith("loop")}
    assert S.screen_1m(model, win, lst[:1], loops=False).loops is None
    dflt = S.screen_1m(model, win, lst[:1], loops=True)
    assert dflt.loop_params == S.LoopParams(1, 4, 2, 0.25, 9, 64, 1) and tuple(dflt.loops.shape) == (1, 64, 2)
    for bad in (S.LoopParams(p=4), S.LoopParams(w=13), 3, "yes", S.LoopParams(r=0), S.LoopParams(threshold=float("nan"))):     # w = 13: no eligible pixel in 50 bins
        with pytest.raises(ValueError):
            S.screen_1m(model, win, lst[:1], loops=bad)


def test_loops_on_the_whole_window_route_and_on_both_strands(case, cuda):
    c, items, model, win, flank, plain, st0, q, res, st = case
    pick = ["del40000", "ins6000", "snv", "mask1", "inv"]
    it = [items[k] for k in pick]
    bm = np.stack([S.bin_map(v, L, F) for v in it])
    with engine.force_safe_precision():
        first = S.screen_1m(model, win, it[:1], flank=flank)
        qw = S.check_loops(S.LoopParams(p=P, w=W, r=R_MAX, threshold=pick_threshold(first.ref_map.cpu().numpy()), max_calls=K_CALLS), NB)
        st3 = {}
        ww = S.screen_1m(model, win, it, keep_maps=True, stats=st3, flank=flank, aligned=True, loops=qw)
    assert st3["route"] == "whole_window" and st3["loops"] == K_CALLS
    equals_host(ww, qw, bm, "whole-window")
    first = S.screen_1m(model, win, it[:1], flank=flank, strands="both")
    qb = S.check_loops(S.LoopParams(p=P, w=W, r=R_MAX, threshold=pick_threshold(first.ref_map.cpu().numpy()), max_calls=K_CALLS), NB)
    st4 = {}
    both = S.screen_1m(model, win, it, keep_maps=True, stats=st4, flank=flank, aligned=True, strands="both", loops=qb)
    assert st4["strands"] == "both" and both.strand_gap is not None
    equals_host(both, qb, bm, "both strands")                          # on the merged maps against the merged reference
