"""Distance-stratified scores of the 1 Mb mutagenesis screen on the MI355X (orca_screen_strata_scores): the kernel alone against the numpy
restatement `screen.strata_scores_host` with and without hand-made bin maps, bit-for-bit invariance to the batch, where a NaN pixel shows, the
entry point's argument checks (return codes only: nothing malformed reaches a kernel), and the screen end to end on a 200 000-base window with
40 000 bases of flank (synthetic H1esc_1M(synthetic_seed=0)) on every route and on both strands.

Tolerances, derived and not measured.  Both sides add the same fp64 terms in the same order; they differ in how a product and the addition that
takes it are rounded (one rounding on the device, two in numpy), in the last bit of a root or a quotient, and in the final rounding to fp32.
  fp32 outputs   |got - want| <= RTOL |want| + 2 c 2^-53 max|pixel|^p, p = 1 for ``dist_delta`` and ``dist_abs``, p = 2 for ``mse``; c = the pairs
                 summed (c_d, or the c of the range).  RTOL = 2.4e-7, two fp32 ulps, is the RTOL of tests/test_gpu_screen_aligned.py.
                 ``dist_rms`` gets the tolerance t of its square carried through the root: sqrt(want^2 + t) - want.
  fp64 outputs   ``dist_corr``, ``corr``, ``scc``: |got - want| <= 8 (c + 4) 2^-53.  Each centred sum of c terms carries at most (c + 4) 2^-53 of
                 the sum of its terms' magnitudes; for C_d that magnitude is at most sqrt(X Y) (Cauchy-Schwarz), so each sum moves r by at most
                 (c + 4) 2^-53; two such errors enter r on each side, and both sides count.  With c <= 32 896 the bound is at most 3e-11.
NaN sits in the same places on both sides and ``dist_count`` matches exactly.  Every comparison prints nothing unless it fails; WORST keeps the
largest error / tolerance seen per field and the last test of the file prints it."""
import ctypes

import numpy as np
import pytest
import torch

from orca_amd import _lib, engine
from orca_amd import orca_models as M
from orca_amd import screen as S
from orca_amd._lib import OrcaHipError
from tests.test_gpu_screen_aligned import F, L, NB, REGIONS, RTOL, _alt, _dp, _hp, _items, _refused, kernel_maps
from tests.test_gpu_screen_sets import _window
from tests.test_gpu_screen_tracks import OLD_FIELDS, same_bits
from tests.test_screen_indel_cpu import plan_flank

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -53
PER_STRATUM = ("dist_delta", "dist_abs", "dist_rms", "dist_corr")
PER_MAP = ("mse", "corr", "scc")
F64 = ("dist_corr", "corr", "scc")
ALIGNED_FIELDS = tuple("aligned_" + k for k in PER_STRATUM + PER_MAP) + ("aligned_dist_count",)
WORST = {}


def _np(t):
    return t.cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)


def _pix(*arrays):
    return max(float(np.nanmax(np.abs(_np(a)))) if _np(a).size else 0.0 for a in arrays)


def check(got, want, pix, rng, what):
    """a dict of device results (engine.screen_strata_scores, or the fields of a ScreenResult) against `screen.strata_scores_host`'s, within the
    tolerances of the module docstring; ``dist_count`` exactly when present"""
    cnt = want["dist_count"].astype(np.float64)
    tot = cnt[:, rng[0]: rng[1]].sum(axis=1)
    with np.errstate(invalid="ignore"):
        w2 = want["dist_rms"] * want["dist_rms"]
        tols = {"dist_delta": RTOL * np.abs(want["dist_delta"]) + 2 * cnt * EPS * pix,
                "dist_abs": RTOL * np.abs(want["dist_abs"]) + 2 * cnt * EPS * pix,
                "dist_rms": np.sqrt(w2 + RTOL * w2 + 2 * cnt * EPS * pix * pix) - want["dist_rms"],
                "mse": RTOL * np.abs(want["mse"]) + 2 * tot * EPS * pix * pix,
                "dist_corr": 8 * (cnt + 4) * EPS, "corr": 8 * (tot + 4) * EPS, "scc": 8 * (tot + 4) * EPS}
    for k in PER_STRATUM + PER_MAP:
        assert got[k].dtype == (torch.float64 if k in F64 else torch.float32), (what, k, got[k].dtype)
        g, h = _np(got[k]).astype(np.float64), want[k]
        assert g.shape == h.shape, (what, k, g.shape, h.shape)
        assert np.array_equal(np.isnan(g), np.isnan(h)), (what, k, np.argwhere(np.isnan(g) != np.isnan(h))[:5])
        f = ~np.isnan(h)
        err, tol = np.abs(g[f] - h[f]), np.broadcast_to(tols[k], h.shape)[f]
        ratio = float((err / np.maximum(tol, 1e-300)).max()) if err.size else 0.0
        WORST[k] = max(WORST.get(k, 0.0), ratio)
        assert np.all(err <= tol), (what, k, ratio, float(err.max()))
    if got.get("dist_count") is not None:
        assert got["dist_count"].dtype == torch.int32 and np.array_equal(_np(got["dist_count"]), want["dist_count"]), (what, "dist_count")


def inputs(kind, rs, B, n, cuda):
    """alt [B, n, n] with a batch stride above n * n and ref [n, n]: alt independent of ref / alt = ref + 1e-4 noise (r within 1e-8 of 1) / one
    stratum constant in ref"""
    alt, ref = _alt(rs, B, n, cuda)
    if kind == "near":
        alt.copy_(ref[None] + 1e-4 * alt)
    if kind == "constant":
        i = torch.arange(n - min(2, n - 1), device=cuda)
        ref[i, i + min(2, n - 1)] = 0.375
    return alt, ref


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("n", [1, 2, 3, 50, 250, 256])
def test_kernel_equals_the_host_restatement(cuda, n, B):
    ctx = engine.get_context(cuda)
    maps = kernel_maps(n)
    names = list(maps)
    rs = np.random.RandomState(2000 * n + B)
    sub = (n // 3, max(n // 3 + 1, n - 2))
    for kind in ("independent", "near", "constant"):
        alt, ref = inputs(kind, rs, B, n, cuda)
        assert alt.stride(0) == n * n + 7
        a, r = alt.cpu().numpy(), ref.cpu().numpy()
        pix = _pix(a, r)
        plain = engine.screen_strata_scores(ctx, alt, ref)
        assert plain["dist_count"] is None and tuple(plain["dist_corr"].shape) == (B, n) and tuple(plain["scc"].shape) == (B,)
        host = S.strata_scores_host(a, r)
        check(plain, host, pix, (0, n), (kind, n, B, "bin with bin"))
        if kind == "near" and n >= 50:                                  # the case fp64 is there for: 1 - r is small and is not lost
            assert 0 < float((1 - plain["scc"]).max()) < 1e-7 and float((1 - plain["scc"]).min()) > 1e-9
        if kind == "constant":
            d = min(2, n - 1)
            assert torch.isnan(plain["dist_corr"][:, d]).all() and torch.isfinite(plain["dist_delta"][:, d]).all()
        if kind == "independent":
            check(engine.screen_strata_scores(ctx, alt, ref, None, sub), S.strata_scores_host(a, r, None, sub), pix, sub, (n, B, "bin with bin", sub))
        for g0 in range(0, len(names), B):
            group = names[g0: g0 + B]
            bm = np.stack([maps[k] for k in group]).astype(np.int32)
            got = engine.screen_strata_scores(ctx, alt[: len(group)], ref, bm)
            host = S.strata_scores_host(a[: len(group)], r, bm)
            check(got, host, pix, (0, n), (kind, n, B, group))
            if kind == "independent":
                check(engine.screen_strata_scores(ctx, alt[: len(group)], ref, bm, sub), S.strata_scores_host(a[: len(group)], r, bm, sub), pix, sub, (n, B, group, sub))
            for b, k in enumerate(group):
                if k == "identity":                                     # the same expressions: the same bits
                    assert all(same_bits(got[f][b], plain[f][b]) for f in PER_STRATUM + PER_MAP), (kind, n, B)
                    assert got["dist_count"][b].tolist() == [n - d for d in range(n)]
                if k == "none":
                    assert all(torch.isnan(got[f][b]).all() for f in PER_STRATUM + PER_MAP) and not got["dist_count"][b].any()
                if k == "one":                                          # one mapped bin: stratum 0 has one pair, every other none
                    x = float(alt[b, n // 2, n // 2]) - float(ref[n - 1, n - 1])
                    assert got["dist_count"][b].tolist() == [1] + [0] * (n - 1) and float(got["dist_delta"][b, 0]) == np.float32(x)
                    assert float(got["mse"][b]) == np.float32(x * x) and torch.isnan(got["corr"][b]) and torch.isnan(got["scc"][b])


@pytest.mark.parametrize("n", [50, 250, 256])
def test_a_maps_results_do_not_depend_on_the_batch(cuda, n):
    """A map alone against the same map as row 0, 1 and 2 of a batch of three (another batch stride, other maps and bin maps beside it), under no
    bin map and under every map of `kernel_maps`; the identity bin map gives the bin-with-bin bits."""
    ctx = engine.get_context(cuda)
    maps = kernel_maps(n)
    rs = np.random.RandomState(13 * n)
    alt, ref = _alt(rs, 1, n, cuda)
    one = alt.contiguous()
    others, _ = _alt(rs, 3, n, cuda)
    sub = (3, n - 5)
    fields = PER_STRATUM + PER_MAP
    for name in [None] + list(maps):
        bm1 = None if name is None else maps[name].astype(np.int32)[None]
        for rng in (None, sub):
            alone = engine.screen_strata_scores(ctx, one, ref, bm1, rng)
            for row in range(3):
                batch = others                                          # batch stride n * n + 7; the rows written earlier stay, as other maps
                batch[row] = one[0]
                bm3 = None
                if name is not None:
                    bm3 = np.stack([maps["holes"], maps["shift"], maps["duplicate"]]).astype(np.int32)
                    bm3[row] = bm1[0]
                got = engine.screen_strata_scores(ctx, batch, ref, bm3, rng)
                for f in fields + (() if name is None else ("dist_count",)):
                    assert same_bits(got[f][row], alone[f][0]) if f != "dist_count" else torch.equal(got[f][row], alone[f][0]), (name, rng, row, f)
            if name == "identity":
                plain = engine.screen_strata_scores(ctx, one, ref, None, rng)
                assert all(same_bits(plain[f], alone[f]) for f in fields), rng


def nan_sets(out):
    return {k: np.argwhere(np.isnan(_np(out[k]))).tolist() for k in PER_STRATUM + PER_MAP}


@pytest.mark.parametrize("rng", [(0, 50), (0, 8), (9, 50), (8, 9)])
def test_nan_shows_in_its_stratum_only(cuda, rng):
    """n = 50.  A NaN below the diagonal and one at an unmapped pair change no bit; one above the diagonal, at alt (12, 20), makes every output of
    stratum 8 NaN and the three per-map scores exactly when 8 is inside the range - computed here from the definition, and equal to the host's."""
    ctx = engine.get_context(cuda)
    n = 50
    k = np.arange(n)
    dele = np.where(k < 10, k, np.where(k + 10 < n, k + 10, -1)).astype(np.int32)       # alt bins 40 .. 49 unmapped, reference bins 10 .. 19 behind no alt bin
    alt, ref = _alt(np.random.RandomState(17), 2, n, cuda)
    alt, ref = alt.contiguous(), ref.contiguous()
    for m in (None, np.stack([dele, dele])):
        clean = engine.screen_strata_scores(ctx, alt, ref, m, rng)
        a2, r2 = alt.clone(), ref.clone()
        a2[:, 20, 12] = float("nan")                                    # below the diagonal
        r2[30, 3] = float("nan")
        if m is not None:
            a2[0, 5, 45] = float("nan")                                 # unmapped pairs
            a2[1, 44, 47] = float("nan")
            r2[12, 14] = float("nan")
        quiet = engine.screen_strata_scores(ctx, a2, r2, m, rng)
        for f in PER_STRATUM + PER_MAP:
            assert same_bits(quiet[f], clean[f]), (f, m is None)
        a3 = alt.clone()
        a3[1, 12, 20] = float("nan")                                    # stratum 8 of map 1; mapped under both
        got = engine.screen_strata_scores(ctx, a3, ref, m, rng)
        want = nan_sets(clean)
        for f in PER_STRATUM:
            want[f] = sorted(want[f] + [[1, 8]])
        if rng[0] <= 8 < rng[1]:
            for f in PER_MAP:
                want[f] = sorted(want[f] + [[1]])
        assert nan_sets(got) == want == nan_sets(S.strata_scores_host(a3.cpu().numpy(), ref.cpu().numpy(), m, rng)), (rng, m is None)
        for f in PER_STRATUM + PER_MAP:                                 # every other value keeps its bits
            keep = ~np.isnan(_np(got[f]))
            assert np.array_equal(_np(got[f])[keep], _np(clean[f])[keep]), f
        r3 = ref.clone()
        r3[12, 20] = float("nan")                                       # the reference pixel: both maps' stratum 8 bin with bin; aligned, behind no alt pair
        got = engine.screen_strata_scores(ctx, alt, r3, m, rng)
        hit = [[0, 8], [1, 8]] if m is None else []
        assert nan_sets(got)["dist_corr"] == sorted(nan_sets(clean)["dist_corr"] + hit)
        assert nan_sets(got) == nan_sets(S.strata_scores_host(alt.cpu().numpy(), r3.cpu().numpy(), m, rng))


# ---- argument checks: return codes only -----------------------------------------------------------------------------------------------------------------
def test_bad_arguments_are_refused_before_any_launch(cuda):
    """Every call below is refused by the host entry point's checks, so nothing of it reaches a kernel; the output buffers keep their fill."""
    lib = _lib.load()
    h = engine.get_context(cuda).handle
    null = ctypes.c_void_p(0)
    n, B = 6, 2
    alt = torch.zeros((B, n, n), dtype=torch.float32, device=cuda)
    ref = torch.zeros((n, n), dtype=torch.float32, device=cuda)
    dev = torch.zeros(B * 257, dtype=torch.int32, device=cuda)                  # stands for the device bin map: never read
    o32 = [torch.full((B * 257,), 7.0, dtype=torch.float32, device=cuda) for _ in range(4)]
    o64 = [torch.full((B * 257,), 7.0, dtype=torch.float64, device=cuda) for _ in range(3)]
    cnt = torch.full((B * 257,), 7, dtype=torch.int32, device=cuda)
    good = np.ascontiguousarray([[0, 1, -1, 2, 3, 5], [-1] * 6], dtype=np.int32)
    big = np.zeros((B, 257), dtype=np.int32)

    def call(bm=good, a=_dp(alt), r=_dp(ref), bm_dev=_dp(dev), host=True, nb=B, nn=n, bs=n * n, lo=0, hi=n, dd=_dp(o32[0]), da=_dp(o32[1]), dr=_dp(o32[2]),
             dc=_dp(o64[0]), dn=_dp(cnt), ms=_dp(o32[3]), co=_dp(o64[1]), sc=_dp(o64[2])):
        return lib.orca_screen_strata_scores(h, a, bs, r, nb, nn, bm_dev, _hp(bm) if host else null, lo, hi, dd, da, dr, dc, dn, ms, co, sc)

    def plain(**kw):
        return call(bm_dev=null, host=False, dn=null, **kw)
    for c in (call, plain):
        _refused(c(nn=257, bs=257 * 257, hi=257, **({"bm": big} if c is call else {})))      # n = 257
        _refused(c(nn=0, hi=0))
        _refused(c(nb=0))
        _refused(c(nb=-1))
        _refused(c(bs=n * n - 1))                                                  # map_bs < n * n
        for lo, hi in ((-1, n), (0, n + 1), (3, 3), (4, 3), (n, n + 1), (0, 0)):
            assert "d_lo < d_hi" in _refused(c(lo=lo, hi=hi)), (lo, hi)
        for k in ("a", "r", "dd", "da", "dr", "dc", "ms", "co", "sc"):
            assert "NULL" in _refused(c(**{k: null})), k
    bad = good.copy()
    bad[1, 4] = n
    assert "outside -1" in _refused(call(bm=bad))                                  # a bin-map entry of n
    bad[1, 4] = -2
    assert "outside -1" in _refused(call(bm=bad))
    assert "together" in _refused(call(host=False))                                # a device bin map without its host copy
    assert "together" in _refused(call(bm_dev=null))                               # ... and the other way round
    assert "together" in _refused(call(dn=null))                                   # a bin map without dist_count
    assert "together" in _refused(call(bm_dev=null, host=False))                   # dist_count without a bin map
    torch.cuda.synchronize()
    assert all(bool((o == 7).all()) for o in o32 + o64 + [cnt])
    # the wrapper turns the same refusals into errors
    ctx = engine.get_context(cuda)
    for rng in ((0, n + 1), (2, 2), (-1, 3)):
        with pytest.raises(OrcaHipError):
            engine.screen_strata_scores(ctx, alt, ref, None, rng)
    with pytest.raises(OrcaHipError):
        engine.screen_strata_scores(ctx, alt, ref, bad)
    with pytest.raises(ValueError):
        engine.screen_strata_scores(ctx, alt, ref, good[:1])
    with pytest.raises(ValueError):
        engine.screen_strata_scores(ctx, alt, ref, None, 3)
    with pytest.raises(ValueError):
        engine.screen_strata_scores(ctx, alt[:0], ref)


# ---- the screen ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def case(cuda):
    c, fl = _window(), plan_flank(F)
    assert c.size == L
    items = _items(c)
    model = M.H1esc_1M(synthetic_seed=0).to(cuda)
    win, flank = torch.from_numpy(c).to(cuda), torch.from_numpy(fl).to(cuda)
    st = {}
    res = S.screen_1m(model, win, list(items.values()), keep_maps=True, stats=st, regions=REGIONS, flank=flank, aligned=True, strata=True)
    return c, fl, items, model, win, flank, res, st


def _equals_host(res, bm, rng, what):
    """every strata field of ``res`` against the host restatement on its own maps"""
    maps, ref = res.maps.cpu().numpy(), res.ref_map.cpu().numpy()
    pix = _pix(maps, ref)
    assert res.strata_range == rng
    check({k: getattr(res, k) for k in PER_STRATUM + PER_MAP}, S.strata_scores_host(maps, ref, None, rng), pix, rng, (what, "bin with bin"))
    assert tuple(res.dist_corr.shape) == (maps.shape[0], NB) and tuple(res.scc.shape) == (maps.shape[0],)
    if bm is None:
        assert all(getattr(res, k) is None for k in ALIGNED_FIELDS)
    else:
        check({k: getattr(res, "aligned_" + k) for k in PER_STRATUM + PER_MAP + ("dist_count",)}, S.strata_scores_host(maps, ref, bm, rng), pix, rng, (what, "aligned"))


def test_screen_strata_fields_equal_the_host_restatement(case, cuda):
    """Every new field against the numpy restatement on ``res.maps``, ``res.ref_map`` and `screen.bin_map`.  Printed, not asserted (the weights are
    synthetic): 1 - aligned_scc and 1 - scc of the 40 000-base deletion."""
    c, fl, items, model, win, flank, res, st = case
    lst = list(items.values())
    host = np.stack([S.bin_map(v, L, F) for v in lst])
    assert np.array_equal(res.bin_map.cpu().numpy(), host) and st["route"] == "two_part" and st["strata"] == NB
    _equals_host(res, host, (0, NB), "two-part")
    for name in ("snv", "inv", "del3"):                                 # length-preserving items: the identity bin map, the same bits
        k = list(items).index(name)
        assert np.array_equal(host[k], np.arange(NB))
        for f in PER_STRATUM + PER_MAP:
            assert same_bits(getattr(res, "aligned_" + f)[k], getattr(res, f)[k]), (name, f)
        assert res.aligned_dist_count[k].tolist() == [NB - d for d in range(NB)]
    k40 = list(items).index("del40000")
    m = host[k40]
    assert m.tolist() == list(range(15)) + list(range(25, 50)) + [-1] * 10
    assert res.aligned_dist_count[k40].tolist() == [int(((m[: NB - d] >= 0) & (m[d:] >= 0)).sum()) for d in range(NB)] == [max(0, 40 - d) for d in range(NB)]
    assert torch.isnan(res.aligned_dist_delta[k40, 40:]).all() and torch.isfinite(res.aligned_dist_delta[k40, :40]).all() and torch.isfinite(res.dist_delta[k40]).all()
    print(f"del40000: 1 - aligned_scc {1 - float(res.aligned_scc[k40]):.6e}, 1 - scc (bin with bin) {1 - float(res.scc[k40]):.6e}; "
          f"1 - aligned_corr {1 - float(res.aligned_corr[k40]):.6e}, 1 - corr {1 - float(res.corr[k40]):.6e}; aligned_mse {float(res.aligned_mse[k40]):.4e}, mse {float(res.mse[k40]):.4e}")
    print("1 - scc per item:", {k: f"{1 - float(v):.3e}" for k, v in zip(items, res.scc)})
    print("1 - aligned_scc per item:", {k: f"{1 - float(v):.3e}" for k, v in zip(items, res.aligned_scc)})


def test_strata_change_nothing_else(case, cuda):
    c, fl, items, model, win, flank, res, st = case
    lst = list(items.values())
    st2 = {}
    plain = S.screen_1m(model, win, lst, keep_maps=True, stats=st2, regions=REGIONS, flank=flank, aligned=True)
    for name in OLD_FIELDS:
        x, y = getattr(plain, name), getattr(res, name)
        assert x is not None and y is not None, name
        assert torch.equal(x, y) or (x.dtype == torch.float32 and torch.isnan(x).any() and same_bits(x, y)), name      # NaN rows: the same bits
    for name in ("strata_range",) + PER_STRATUM + PER_MAP + ALIGNED_FIELDS:
        assert getattr(plain, name) is None and getattr(res, name) is not None, name
    assert st2["strata"] == 0 and {k: v for k, v in st.items() if k != "strata"} == {k: v for k, v in st2.items() if k != "strata"}
    assert S.screen_1m(model, win, lst[:1], strata=False).scc is None
    # a range, without aligned, in batches of 3: the per-stratum fields are the same bits, the per-map ones run over the range
    st3 = {}
    part = S.screen_1m(model, win, lst, batch=3, keep_maps=True, stats=st3, flank=flank, strata=(2, 40))
    assert st3["strata"] == 38
    _equals_host(part, None, (2, 40), "range")
    for f in PER_STRATUM:
        assert same_bits(getattr(part, f), getattr(res, f)), f
    assert not same_bits(part.scc, res.scc)
    small = S.screen_1m(model, win, lst, batch=3, flank=flank, aligned=True, strata=True)
    for f in PER_STRATUM + PER_MAP:
        assert same_bits(getattr(small, f), getattr(res, f)) and same_bits(getattr(small, "aligned_" + f), getattr(res, "aligned_" + f)), f
    assert torch.equal(small.aligned_dist_count, res.aligned_dist_count)
    for bad in ((0, NB + 1), (5, 5), 7, (1, 2, 3)):
        with pytest.raises(ValueError):
            S.screen_1m(model, win, lst[:1], strata=bad)


def test_strata_on_the_whole_window_route_and_on_both_strands(case, cuda):
    c, fl, items, model, win, flank, res, st = case
    pick = ["del40000", "dup8000", "snv"]
    it = [items[k] for k in pick]
    host = np.stack([S.bin_map(v, L, F) for v in it])
    st3 = {}
    with engine.force_safe_precision():
        ww = S.screen_1m(model, win, it, keep_maps=True, stats=st3, flank=flank, aligned=True, strata=True)
    assert st3["route"] == "whole_window" and st3["strata"] == NB
    _equals_host(ww, host, (0, NB), "whole-window")
    st4 = {}
    both = S.screen_1m(model, win, it, keep_maps=True, stats=st4, flank=flank, aligned=True, strands="both", strata=True)
    assert st4["strands"] == "both" and both.strand_gap is not None
    _equals_host(both, host, (0, NB), "both strands")                           # on the merged maps against the merged reference
    assert not same_bits(both.dist_delta, ww.dist_delta)


def test_print_the_worst_error_over_tolerance():
    print("largest error / tolerance per field over this file's comparisons:", {k: f"{v:.3g}" for k, v in WORST.items()})
