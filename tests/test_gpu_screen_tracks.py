"""Insulation tracks and viewpoint profiles of the 1 Mb mutagenesis screen on the MI355X: the two kernels alone on hand-made bin maps against the
numpy restatements (`screen.insulation_scores_host`, `screen.viewpoint_scores_host`), bit-for-bit invariance to the batch, where a NaN pixel
shows, the entry points' argument checks (return codes only: nothing malformed reaches a kernel), and the screen end to end on a 200 000-base
window with 40 000 bases of flank (synthetic H1esc_1M(synthetic_seed=0)) on every route and on both strands.

Tolerances.  An insulation value is a mean of w^2 pixels summed in fp64 and rounded to fp32 once, or the fp64 difference of two such means
rounded once: |got - want| <= RTOL |want| + 2 w^2 2^-53 max|pixel|.  RTOL = 2.4e-7 is two fp32 ulps for the final rounding (the RTOL of
tests/test_gpu_screen_aligned.py); the second term is the worst reordering error of an fp64 sum of at most 2 w^2 terms, and matters only where
the alt and the reference means cancel.  ``delta_viewpoint`` is an fp32 subtraction and ``aligned_viewpoint`` one too where a single alt bin
stands for the viewpoint: bit for bit numpy's.  Where c > 1 alt bins stand for it the rows are added in fp64 in ascending order on both sides,
then one division, one subtraction and one rounding; asserted within RTOL |want| + 2 c 2^-53 max|pixel| in the kernel test.  NaN sits in the
same places on both sides."""
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
from tests.test_screen_indel_cpu import plan_flank

pytestmark = pytest.mark.gpu

WIDTHS = (1, 3, 10)
VIEWS = [0, 12, 20, 49]
OLD_FIELDS = ("ref_map", "ref_1d", "maps", "delta_profile", "delta_abs_mean", "delta_abs_max", "delta_1d", "delta_region", "delta_region_abs", "shift",
              "bin_map", "aligned_bins", "aligned_profile", "aligned_abs_mean", "aligned_abs_max", "aligned_region", "aligned_region_abs")
INS_FIELDS = ("ref_insulation", "insulation", "delta_insulation", "aligned_insulation")
VIEW_FIELDS = ("delta_viewpoint", "aligned_viewpoint")


def bits(t):
    a = t.cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype.itemsize == 4 else np.uint64)


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def same_f32(got, want):
    """kernel against numpy: NaN in the same places (whatever its payload), every other value the same bits"""
    g, w = (x.cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x) for x in (got, want))
    if g.shape != w.shape or g.dtype != np.float32 or w.dtype != np.float32 or not np.array_equal(np.isnan(g), np.isnan(w)):
        return False
    return np.array_equal(bits(g)[~np.isnan(g)], bits(w)[~np.isnan(w)])


def close_ins(got, want, widths, pix, what=""):
    """got [.., W, n] float32 against want (fp64) within RTOL |want| + 2 w^2 2^-53 max|pixel| per width, NaN in the same places"""
    g, h = np.asarray(got.cpu().numpy() if isinstance(got, torch.Tensor) else got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert g.shape == h.shape and g.shape[-2] == len(widths), (what, g.shape, h.shape)
    assert np.array_equal(np.isnan(g), np.isnan(h)), (what, np.argwhere(np.isnan(g) != np.isnan(h))[:5])
    for k, w in enumerate(widths):
        gk, hk = g[..., k, :], h[..., k, :]
        f = ~np.isnan(hk)
        err, tol = np.abs(gk[f] - hk[f]), RTOL * np.abs(hk[f]) + 2.0 * w * w * 2.0 ** -53 * pix
        assert np.all(err <= tol), (what, w, float((err / tol).max()))


def widths_of(n):
    return [w for w in (1, 2, 25, (n - 1) // 2, 128) if w >= 1]


def views_of(n):
    return [0, n // 2, n - 1]


def _pix(*arrays):
    return max(float(np.nanmax(np.abs(a))) for a in arrays)


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("n", [1, 3, 50, 250, 256])
def test_kernels_equal_the_host_restatements(cuda, n, B):
    ctx = engine.get_context(cuda)
    maps = kernel_maps(n)
    names = list(maps)
    ws, vs = widths_of(n), views_of(n)
    rs = np.random.RandomState(1000 * n + B)
    for g0 in range(0, len(names), B):
        group = names[g0: g0 + B]
        bm = np.stack([maps[k] for k in group]).astype(np.int32)
        alt, ref = _alt(rs, len(group), n, cuda)
        assert alt.stride(0) == n * n + 7
        a, r = alt.cpu().numpy(), ref.cpu().numpy()
        pix = _pix(a, r)
        track, delta, aligned = engine.screen_insulation(ctx, alt, ref, ws, bm)
        ht, hd, ha = S.insulation_scores_host(a, r, ws, bm)
        assert tuple(track.shape) == (len(group), len(ws), n)
        close_ins(track, ht, ws, pix, (group, "track"))
        close_ins(delta, hd, ws, pix, (group, "delta"))
        close_ins(aligned, ha, ws, pix, (group, "aligned"))
        assert torch.isnan(track[:, ws.index(128)]).all() and torch.isnan(aligned[:, ws.index(128)]).all()       # 2 w + 1 > n: legal, all NaN
        for k, w in enumerate(ws):
            assert int(torch.isfinite(track[0, k]).sum()) == max(0, n - 2 * w)
        # without the bin map the same bits and no aligned output; without the reference the track alone
        t2, d2, a2 = engine.screen_insulation(ctx, alt, ref, ws)
        assert a2 is None and same_bits(t2, track) and same_bits(d2, delta)
        t3, d3, a3 = engine.screen_insulation(ctx, alt, None, ws)
        assert d3 is None and a3 is None and same_bits(t3, track)
        dv, av = engine.screen_viewpoints(ctx, alt, ref, vs, bm)
        hv, hav = S.viewpoint_scores_host(a, r, vs, bm)
        assert same_f32(dv, hv), (group, "delta_viewpoint")
        g = av.cpu().numpy()
        assert np.array_equal(np.isnan(g), np.isnan(hav)), (group, "aligned_viewpoint NaN")
        for b in range(len(group)):
            for k, v in enumerate(vs):
                c = int((bm[b] == v).sum())
                if c <= 1:
                    assert same_f32(g[b, k], hav[b, k]), (group[b], v, c)
                else:
                    f = ~np.isnan(hav[b, k])
                    err = np.abs(g[b, k][f].astype(np.float64) - hav[b, k][f].astype(np.float64))
                    assert np.all(err <= RTOL * np.abs(hav[b, k][f]) + 2.0 * c * 2.0 ** -53 * pix), (group[b], v, c)
                if c == 0:
                    assert np.isnan(g[b, k]).all()
        dv2, av2 = engine.screen_viewpoints(ctx, alt, ref, vs)
        assert av2 is None and same_bits(dv2, dv)
        for b, k in enumerate(group):
            if k == "identity":                                            # the same expression: the same bits
                assert same_bits(aligned[b], delta[b]) and same_bits(av[b], dv[b])
            if k == "none":
                assert torch.isnan(aligned[b]).all() and torch.isnan(av[b]).all()


@pytest.mark.parametrize("n", [50, 250, 256])
def test_a_maps_results_do_not_depend_on_the_batch(cuda, n):
    ctx = engine.get_context(cuda)
    maps = kernel_maps(n)
    ws, vs = widths_of(n), views_of(n)
    rs = np.random.RandomState(11 * n)

    def run(a, ref, bm):
        return engine.screen_insulation(ctx, a, ref, ws, bm) + engine.screen_viewpoints(ctx, a, ref, vs, bm)
    for group in (["identity", "shift", "holes"], ["duplicate", "none", "one"]):
        bm = np.stack([maps[k] for k in group]).astype(np.int32)
        alt, ref = _alt(rs, 3, n, cuda)
        whole = run(alt, ref, bm)
        for b in range(3):                                              # three B = 1 calls (on a contiguous copy: another batch stride)
            one = run(alt[b: b + 1].contiguous(), ref, bm[b: b + 1])
            for w, o in zip(whole, one):
                assert same_bits(w[b], o[0]), (group[b], n)
        perm = [2, 0, 1]
        pt = torch.tensor(perm, device=cuda)
        moved = run(alt[pt], ref, bm[perm])
        for w, m in zip(whole, moved):
            assert same_bits(w[pt], m), (group, n)


def _holding(n, w, row, col):
    """the bins whose diamond at width w fits and holds pixel (row, col), from the definition: rows [i - w, i) x columns (i, i + w]"""
    return [i for i in range(n) if w <= i < n - w and i - w <= row < i and i < col <= i + w]


def test_nan_shows_in_the_diamonds_that_hold_it(cuda):
    """n = 50, w = 3, a NaN at alt (12, 20).  By the definition no diamond of width 3 holds that pixel (row 12 needs i <= 15, column 20 needs
    i >= 17), so at w = 3 it must change no bit; the same pixel at w = 8, and the pixel (12, 16) at w = 3, are held by non-empty sets of bins,
    and the NaN must show exactly there - in the track, in delta and, through the map, in aligned."""
    ctx = engine.get_context(cuda)
    n, ws = 50, [3, 8]
    i = np.arange(n)
    shift = np.where(i + 3 < n, i + 3, -1).astype(np.int32)[None]
    ident = i.astype(np.int32)[None]
    alt, ref = _alt(np.random.RandomState(5), 1, n, cuda)
    alt, ref = alt.contiguous(), ref.contiguous()
    clean = {k: engine.screen_insulation(ctx, alt, ref, ws, m) for k, m in (("ident", ident), ("shift", shift))}
    for row, col in ((12, 20), (12, 16)):
        a2 = alt.clone()
        a2[0, row, col] = float("nan")
        for name, bm in (("ident", ident), ("shift", shift)):
            got = engine.screen_insulation(ctx, a2, ref, ws, bm)
            host = S.insulation_scores_host(a2.cpu().numpy(), ref.cpu().numpy(), ws, bm)
            host_clean = S.insulation_scores_host(alt.cpu().numpy(), ref.cpu().numpy(), ws, bm)
            for k, w in enumerate(ws):
                hold = _holding(n, w, row, col)
                for f, (g, c, h, hc) in enumerate(zip(got, clean[name], host, host_clean)):
                    new = np.flatnonzero(np.isnan(g[0, k].cpu().numpy()) & ~np.isnan(c[0, k].cpu().numpy())).tolist()
                    host_new = np.flatnonzero(np.isnan(h[0, k]) & ~np.isnan(hc[0, k])).tolist()
                    # aligned: the alt diamond is at the alt bin itself, so the same bins - where the centre is mapped and the reference diamond fits
                    want = hold if f < 2 else [b for b in hold if bm[0, b] >= w and bm[0, b] < n - w]
                    assert new == want == host_new, (row, col, name, w, f, new, want, host_new)
                    keep = np.setdiff1d(np.arange(n), want)
                    assert np.array_equal(bits(g[0, k])[keep], bits(c[0, k])[keep]), (row, col, name, w, f)
        assert _holding(n, 3, 12, 20) == [] and _holding(n, 8, 12, 20) == list(range(13, 20)) and _holding(n, 3, 12, 16) == [13, 14, 15]
    # the diagonal and the lower triangle are never read
    a3, r3 = alt.clone(), ref.clone()
    low = torch.tril(torch.ones(n, n, dtype=torch.bool, device=cuda))
    a3[0][low] = float("nan")
    r3[low] = float("nan")
    for name, bm in (("ident", ident), ("shift", shift)):
        for g, c in zip(engine.screen_insulation(ctx, a3, r3, ws, bm), clean[name]):
            assert same_bits(g, c), name
    # a NaN in the reference at a diamond pixel: delta at the reference bins that hold it, aligned at the alt bins that stand for them
    r4 = ref.clone()
    r4[12, 14] = float("nan")
    for name, bm in (("ident", ident), ("shift", shift)):
        track, delta, aligned = engine.screen_insulation(ctx, alt, r4, ws, bm)
        ht, hd, ha = S.insulation_scores_host(alt.cpu().numpy(), r4.cpu().numpy(), ws, bm)
        assert same_bits(track, clean[name][0])
        for k, w in enumerate(ws):
            hold = _holding(n, w, 12, 14)
            assert hold, w
            new_d = np.flatnonzero(np.isnan(delta[0, k].cpu().numpy()) & ~np.isnan(clean[name][1][0, k].cpu().numpy())).tolist()
            new_a = np.flatnonzero(np.isnan(aligned[0, k].cpu().numpy()) & ~np.isnan(clean[name][2][0, k].cpu().numpy())).tolist()
            assert new_d == hold, (name, w, new_d, hold)
            assert new_a == [b for b in range(n) if w <= b < n - w and bm[0, b] in hold], (name, w, new_a)
            assert np.array_equal(np.isnan(delta[0, k].cpu().numpy()), np.isnan(hd[0, k])) and np.array_equal(np.isnan(aligned[0, k].cpu().numpy()), np.isnan(ha[0, k]))
    assert _holding(n, 3, 12, 14) == [13]


def test_viewpoints_read_their_rows_and_columns_only(cuda):
    ctx = engine.get_context(cuda)
    n, vs = 50, [20, 5]
    i = np.arange(n)
    shift = np.where(i + 3 < n, i + 3, -1).astype(np.int32)[None]           # reference 20 sits at alt 17, reference 5 at alt 2; alt columns 47 .. 49 unmapped
    alt, ref = _alt(np.random.RandomState(6), 1, n, cuda)
    alt, ref = alt.contiguous(), ref.contiguous()
    clean = engine.screen_viewpoints(ctx, alt, ref, vs, shift)
    a2, r2 = alt.clone(), ref.clone()
    rows = torch.ones(n, dtype=torch.bool, device=cuda)
    rows[[20, 5, 17, 2]] = False
    a2[0][rows] = float("nan")                                              # neither a viewpoint's own row nor a row that stands for one
    a2[0, 17, 47:] = float("nan")                                           # a row that stands for viewpoint 20 (and is no viewpoint), at unmapped columns
    rrows = torch.ones(n, dtype=torch.bool, device=cuda)
    rrows[[20, 5]] = False
    r2[rrows] = float("nan")
    quiet = engine.screen_viewpoints(ctx, a2, r2, vs, shift)
    for c, q in zip(clean, quiet):
        assert same_bits(c, q)
    # ... and one that is read shows where the definition says: alt (17, 30) in aligned viewpoint 20 at column 30 only
    a3 = alt.clone()
    a3[0, 17, 30] = float("nan")
    dv, av = engine.screen_viewpoints(ctx, a3, ref, vs, shift)
    assert same_bits(dv, clean[0])
    assert np.flatnonzero(np.isnan(av[0, 0].cpu().numpy())).tolist() == [30, 47, 48, 49] and same_bits(av[0, 1], clean[1][0, 1])
    hv, hav = S.viewpoint_scores_host(a3.cpu().numpy(), ref.cpu().numpy(), vs, shift)
    assert same_f32(dv, hv) and same_f32(av, hav)


# ---- argument checks: return codes only -----------------------------------------------------------------------------------------------------------------
def test_bad_arguments_are_refused_before_any_launch(cuda):
    """Every call below is refused by the host entry point's checks, so nothing of it reaches a kernel; the output buffers keep their fill."""
    lib = _lib.load()
    h = engine.get_context(cuda).handle
    null = ctypes.c_void_p(0)
    n, B = 6, 2
    alt = torch.zeros((B, n, n), dtype=torch.float32, device=cuda)
    ref = torch.zeros((n, n), dtype=torch.float32, device=cuda)
    dev = torch.zeros(256, dtype=torch.int32, device=cuda)                      # stands for every device table: never read
    outs = [torch.full((B * 8 * n,), 7.0, dtype=torch.float32, device=cuda) for _ in range(5)]
    good = np.ascontiguousarray([[0, 1, -1, 2, 3, 5], [-1] * 6], dtype=np.int32)
    big = np.zeros((B, 257), dtype=np.int32)

    def tab(*v):
        return np.ascontiguousarray(list(v) + [1] * (80 - len(v)), dtype=np.int32)       # padded: a count above the entries given reads only this array

    def ins(w=tab(1, 2), W=2, bm=good, a=_dp(alt), r=_dp(ref), w_dev=_dp(dev), w_host=True, bm_dev=_dp(dev), host=True, nb=B, nn=n, bs=n * n,
            t=_dp(outs[0]), d=_dp(outs[1]), al=_dp(outs[2])):
        return lib.orca_screen_insulation(h, a, bs, r, nb, nn, w_dev, _hp(w) if w_host else null, W, bm_dev, _hp(bm) if host else null, t, d, al)

    def view(v=tab(0, 5), V=2, bm=good, a=_dp(alt), r=_dp(ref), v_dev=_dp(dev), v_host=True, bm_dev=_dp(dev), host=True, nb=B, nn=n, bs=n * n,
             d=_dp(outs[3]), al=_dp(outs[4])):
        return lib.orca_screen_viewpoints(h, a, bs, r, nb, nn, v_dev, _hp(v) if v_host else null, V, bm_dev, _hp(bm) if host else null, d, al)
    assert "widths" in _refused(ins(W=0)) and "widths" in _refused(ins(W=9))
    assert "width 1" in _refused(ins(w=tab(1, 0))) and "width 0" in _refused(ins(w=tab(129, 1)))
    assert "viewpoints" in _refused(view(V=0)) and "viewpoints" in _refused(view(V=65))
    assert "viewpoint 1" in _refused(view(v=tab(0, -1))) and "viewpoint 0" in _refused(view(v=tab(n, 1)))
    bad = good.copy()
    bad[1, 4] = n
    for call in (ins, view):
        _refused(call(nn=257, bm=big, bs=257 * 257))                               # n = 257
        _refused(call(nn=0))
        _refused(call(bs=n * n - 1))                                               # map_bs < n * n
        _refused(call(nb=0))
        assert "outside -1" in _refused(call(bm=bad))                              # a bin-map entry of n
        assert "together" in _refused(call(bm_dev=null, host=False))               # aligned without a bin map
        assert "together" in _refused(call(al=null))                               # a bin map without aligned
        assert "NULL" in _refused(call(host=False))                                # no host copy of the map
        assert "NULL" in _refused(call(a=null))
    assert "NULL" in _refused(ins(w_host=False)) and "NULL" in _refused(ins(w_dev=null)) and "NULL" in _refused(ins(t=null))
    assert "NULL" in _refused(view(v_host=False)) and "NULL" in _refused(view(v_dev=null)) and "NULL" in _refused(view(d=null)) and "NULL" in _refused(view(r=null))
    assert "without ref" in _refused(ins(r=null, bm_dev=null, host=False, al=null))          # ref == NULL with delta
    assert "without ref" in _refused(ins(r=null, d=null))                                     # ref == NULL with aligned and a bin map
    torch.cuda.synchronize()
    assert all(bool((o == 7).all()) for o in outs)
    # the wrappers turn the same refusals into OrcaHipError
    ctx = engine.get_context(cuda)
    with pytest.raises(OrcaHipError):
        engine.screen_insulation(ctx, alt, ref, [0])
    with pytest.raises(OrcaHipError):
        engine.screen_insulation(ctx, alt, ref, list(range(1, 10)))
    with pytest.raises(OrcaHipError):
        engine.screen_viewpoints(ctx, alt, ref, [n])
    with pytest.raises(OrcaHipError):
        engine.screen_viewpoints(ctx, alt, ref, [0], bad)
    with pytest.raises(ValueError):
        engine.screen_insulation(ctx, alt, ref, [1], good[:1])
    with pytest.raises(ValueError):
        engine.screen_insulation(ctx, alt, None, [1], good)


# ---- the screen ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def case(cuda):
    c, fl = _window(), plan_flank(F)
    assert c.size == L
    items = _items(c)
    model = M.H1esc_1M(synthetic_seed=0).to(cuda)
    win, flank = torch.from_numpy(c).to(cuda), torch.from_numpy(fl).to(cuda)
    st = {}
    res = S.screen_1m(model, win, list(items.values()), keep_maps=True, stats=st, regions=REGIONS, flank=flank, aligned=True, insulation=WIDTHS, viewpoints=VIEWS)
    return c, fl, items, model, win, flank, res, st


def _equals_host(res, bm, what):
    """every track field of ``res`` against the host restatements on its own maps: the insulation ones within the tolerance, the viewpoint ones bit for bit"""
    maps, ref = res.maps.cpu().numpy(), res.ref_map.cpu().numpy()
    pix = _pix(maps, ref)
    E = maps.shape[0]
    ht, hd, ha = S.insulation_scores_host(maps, ref, WIDTHS, bm)
    assert tuple(res.insulation.shape) == (E, len(WIDTHS), NB) and tuple(res.ref_insulation.shape) == (len(WIDTHS), NB)
    close_ins(res.ref_insulation, S.insulation_host(ref[None], WIDTHS)[0], WIDTHS, pix, (what, "ref_insulation"))
    close_ins(res.insulation, ht, WIDTHS, pix, (what, "insulation"))
    close_ins(res.delta_insulation, hd, WIDTHS, pix, (what, "delta_insulation"))
    hv, hav = S.viewpoint_scores_host(maps, ref, VIEWS, bm)
    assert tuple(res.delta_viewpoint.shape) == (E, len(VIEWS), NB) and same_f32(res.delta_viewpoint, hv), (what, "delta_viewpoint")
    if bm is None:
        assert res.aligned_insulation is None and res.aligned_viewpoint is None
    else:
        close_ins(res.aligned_insulation, ha, WIDTHS, pix, (what, "aligned_insulation"))
        assert same_f32(res.aligned_viewpoint, hav), (what, "aligned_viewpoint")
    assert res.insulation_widths.dtype == torch.int32 and res.insulation_widths.tolist() == list(WIDTHS) and res.viewpoint_bins.tolist() == VIEWS


def test_screen_track_fields_equal_the_host_restatements(case, cuda):
    """Every new field against the numpy restatement on ``res.maps``, ``res.ref_map`` and `screen.bin_map`.  Printed, not asserted (the weights are
    synthetic): the sign and size of ``aligned_insulation`` at the junction of the 40 000-base deletion."""
    c, fl, items, model, win, flank, res, st = case
    lst = list(items.values())
    host = np.stack([S.bin_map(v, L, F) for v in lst])
    assert np.array_equal(res.bin_map.cpu().numpy(), host) and st["route"] == "two_part" and st["insulation_widths"] == 3 and st["viewpoints"] == 4
    _equals_host(res, host, "two-part")
    k40 = list(items).index("del40000")
    assert host[k40].tolist() == list(range(15)) + list(range(25, 50)) + [-1] * 10
    assert torch.isnan(res.aligned_viewpoint[k40, VIEWS.index(20)]).all() and torch.isfinite(res.delta_viewpoint[k40, VIEWS.index(20)]).all()
    assert torch.isnan(res.aligned_insulation[k40, :, 40:]).all()
    for k, w in enumerate(WIDTHS):                     # finite where the centre is mapped and both diamonds fit: alt w .. 14 and 15 .. min(39, 49 - w - 10)
        fin = [i for i in range(NB) if w <= i < NB - w and host[k40, i] >= w and host[k40, i] < NB - w]
        assert np.flatnonzero(torch.isfinite(res.aligned_insulation[k40, k]).cpu().numpy()).tolist() == fin and 15 in fin
    for name in ("snv", "inv", "del3"):
        k = list(items).index(name)
        assert same_bits(res.aligned_insulation[k], res.delta_insulation[k]) and same_bits(res.aligned_viewpoint[k], res.delta_viewpoint[k]), name
    # the junction: alt bin 15 is the first bin behind the deletion (reference bin 25); alt bin 14 the last before it
    for k, w in enumerate(WIDTHS):
        print(f"del40000 aligned_insulation at the junction, w = {w}: alt bin 14 {float(res.aligned_insulation[k40, k, 14]):+.4e}, alt bin 15 "
              f"{float(res.aligned_insulation[k40, k, 15]):+.4e}; ref_insulation there {float(res.ref_insulation[k, 14]):+.4e}, {float(res.ref_insulation[k, 25]):+.4e}; "
              f"largest |aligned_insulation| of the item {float(np.nanmax(np.abs(res.aligned_insulation[k40, k].cpu().numpy()))):.4e}")


def test_tracks_change_nothing_else(case, cuda):
    c, fl, items, model, win, flank, res, st = case
    lst = list(items.values())
    st2 = {}
    plain = S.screen_1m(model, win, lst, keep_maps=True, stats=st2, regions=REGIONS, flank=flank, aligned=True)
    for name in OLD_FIELDS:
        x, y = getattr(plain, name), getattr(res, name)
        assert x is not None and y is not None, name
        assert torch.equal(x, y) or (x.dtype == torch.float32 and torch.isnan(x).any() and same_bits(x, y)), name      # NaN rows: the same bits
    for name in ("insulation_widths", "viewpoint_bins") + INS_FIELDS + VIEW_FIELDS:
        assert getattr(plain, name) is None and getattr(res, name) is not None, name
    new = ("insulation_widths", "viewpoints")
    assert st2["insulation_widths"] == 0 and st2["viewpoints"] == 0
    assert {k: v for k, v in st.items() if k not in new} == {k: v for k, v in st2.items() if k not in new}
    # one of the two alone, and without aligned: the aligned forms are None
    only = S.screen_1m(model, win, [items["del4000"]], flank=flank, insulation=3)
    assert only.delta_viewpoint is None and only.aligned_insulation is None and tuple(only.delta_insulation.shape) == (1, 1, NB)
    k = list(items).index("del4000")
    assert same_bits(only.delta_insulation[0, 0], res.delta_insulation[k, 1]) and same_bits(only.ref_insulation[0], res.ref_insulation[1])
    # batches of 3: every batch's tracks come from that batch's maps and its rows of the bin map
    small = S.screen_1m(model, win, lst, batch=3, regions=REGIONS, flank=flank, aligned=True, insulation=WIDTHS, viewpoints=VIEWS)
    for name in INS_FIELDS + VIEW_FIELDS:
        assert same_bits(getattr(small, name), getattr(res, name)), name
    with pytest.raises(ValueError):
        S.screen_1m(model, win, lst[:1], insulation=25)
    with pytest.raises(ValueError):
        S.screen_1m(model, win, lst[:1], viewpoints=[50])


def test_tracks_on_the_whole_window_route_and_on_both_strands(case, cuda):
    c, fl, items, model, win, flank, res, st = case
    pick = ["del40000", "dup8000", "snv"]
    it = [items[k] for k in pick]
    host = np.stack([S.bin_map(v, L, F) for v in it])
    st3 = {}
    with engine.force_safe_precision():
        ww = S.screen_1m(model, win, it, keep_maps=True, stats=st3, flank=flank, aligned=True, insulation=WIDTHS, viewpoints=VIEWS)
    assert st3["route"] == "whole_window" and st3["insulation_widths"] == 3
    _equals_host(ww, host, "whole-window")
    st4 = {}
    both = S.screen_1m(model, win, it, keep_maps=True, stats=st4, flank=flank, aligned=True, strands="both", insulation=WIDTHS, viewpoints=VIEWS)
    assert st4["strands"] == "both" and both.strand_gap is not None
    _equals_host(both, host, "both strands")                                  # on the merged maps against the merged reference
    assert not same_bits(both.delta_insulation, ww.delta_insulation)
    plus = S.screen_1m(model, win, it, keep_maps=True, flank=flank, insulation=WIDTHS, viewpoints=VIEWS)
    _equals_host(plus, None, "no aligned")
