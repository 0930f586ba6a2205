"""Aligned scores of the 1 Mb mutagenesis screen on the MI355X: the two kernels alone on hand-made bin maps against the numpy restatements
(`screen.aligned_scores_host`, `screen.aligned_region_scores_host`), NaN handling, bit-for-bit invariance to the batch, the screen end to end
on a 200 000-base window with 40 000 bases of flank (synthetic H1esc_1M(synthetic_seed=0)), ``flank_bp``, and the entry points' argument
checks (return codes only: nothing malformed reaches a kernel).

Tolerances.  The maximum is exact: the largest fp64 difference rounded to fp32, on both sides.  A sum has at most 65 536 fp64 terms; the two
sides associate them differently, which moves it at the 1e-11 level, so only the final rounding to fp32 can differ: RTOL = 2.4e-7, two fp32
ulps.  NaN sits in the same places on both sides."""
import ctypes

import numpy as np
import pytest
import torch

from orca_amd import _lib, engine
from orca_amd import orca_models as M
from orca_amd import screen as S
from orca_amd._lib import OrcaHipError
from tests.test_gpu_screen_sets import _window
from tests.test_screen_indel_cpu import plan_flank
from tests.test_screen_sets_cpu import snv

pytestmark = pytest.mark.gpu

RTOL = 2.4e-7
L, F = 200_000, 40_000
NB = L // 4000
REGIONS = [(5, 15, 20, 35), (30, 45, 30, 45)]


def close(got, want, what=""):
    g, h = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert g.shape == h.shape, (what, g.shape, h.shape)
    assert np.array_equal(np.isnan(g), np.isnan(h)), (what, g, h)
    f = ~np.isnan(h)
    err = np.abs(g[f] - h[f])
    assert np.all(err <= RTOL * np.abs(h[f])), (what, float((err / np.maximum(np.abs(h[f]), 1e-300)).max()))


def same_max(got, want, what=""):
    assert np.array_equal(np.asarray(got), np.asarray(want, dtype=np.float64).astype(np.float32), equal_nan=True), (what, got, want)


def kernel_maps(n):
    """name -> bin map [n]: the cases a screen produces (a deletion's constant shift, an insertion's holes, a shared reference bin) and the
    degenerate ones."""
    i = np.arange(n)
    s = min(3, n - 1)
    holes = i.copy()
    holes[np.random.RandomState(n).rand(n) < 0.3] = -1
    one = np.full(n, -1)
    one[n // 2] = n - 1
    return {"identity": i, "shift": np.where(i + s < n, i + s, -1), "holes": holes, "duplicate": np.maximum(i - 1, 0), "none": np.full(n, -1), "one": one}


def _alt(rs, B, n, cuda):
    """B random maps with a batch stride above n * n, and a reference map."""
    buf = torch.from_numpy(rs.randn(B, n * n + 7).astype(np.float32)).to(cuda)
    return buf.as_strided((B, n, n), (n * n + 7, n, 1)), torch.from_numpy(rs.randn(n, n).astype(np.float32)).to(cuda)


def _rects(n):
    return [(0, n, 0, n), (n // 3, n // 3 + max(1, n // 4), n // 2, n), (0, 1, n - 1, n)]


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("n", [1, 50, 250, 256])
def test_kernels_equal_the_host_restatements(cuda, n, B):
    ctx = engine.get_context(cuda)
    maps = kernel_maps(n)
    names = list(maps)
    rs = np.random.RandomState(100 * n + B)
    for g0 in range(0, len(names), B):
        group = names[g0: g0 + B]
        bm = np.stack([maps[k] for k in group]).astype(np.int32)
        alt, ref = _alt(rs, len(group), n, cuda)
        assert alt.stride(0) > n * n
        prof, mean, amax = engine.screen_aligned_scores(ctx, alt, ref, bm)
        hp, hm, hx = S.aligned_scores_host(alt.cpu().numpy(), ref.cpu().numpy(), bm)
        close(prof.cpu().numpy(), hp, (group, "profile"))
        close(mean.cpu().numpy(), hm, (group, "mean"))
        same_max(amax.cpu().numpy(), hx, (group, "max"))
        sg, ab = engine.screen_aligned_region_scores(ctx, alt, ref, bm, _rects(n))
        hs, ha = S.aligned_region_scores_host(alt.cpu().numpy(), ref.cpu().numpy(), bm, _rects(n))
        close(sg.cpu().numpy(), hs, (group, "region"))
        close(ab.cpu().numpy(), ha, (group, "region abs"))
        for b, k in enumerate(group):                                   # the degenerate maps give what the table of the entry point says
            if k == "none":
                assert torch.isnan(prof[b]).all() and torch.isnan(mean[b]) and torch.isnan(amax[b]) and torch.isnan(sg[b]).all() and torch.isnan(ab[b]).all()
            if k == "one":
                d = abs(float(alt[b, n // 2, n // 2]) - float(ref[n - 1, n - 1]))
                assert int(torch.isfinite(prof[b]).sum()) == 1 and float(amax[b]) == np.float32(d) and float(mean[b]) == np.float32(d)


@pytest.mark.parametrize("n", [1, 50, 250, 256])
def test_a_maps_results_do_not_depend_on_the_batch(cuda, n):
    ctx = engine.get_context(cuda)
    maps = kernel_maps(n)
    rs = np.random.RandomState(7 * n)
    for group in (["identity", "shift", "holes"], ["duplicate", "none", "one"]):
        bm = np.stack([maps[k] for k in group]).astype(np.int32)
        alt, ref = _alt(rs, 3, n, cuda)
        whole = engine.screen_aligned_scores(ctx, alt, ref, bm) + engine.screen_aligned_region_scores(ctx, alt, ref, bm, _rects(n))
        for b in range(3):                                              # three B = 1 calls (on a contiguous copy: another batch stride)
            one = (engine.screen_aligned_scores(ctx, alt[b: b + 1].contiguous(), ref, bm[b: b + 1])
                   + engine.screen_aligned_region_scores(ctx, alt[b: b + 1].contiguous(), ref, bm[b: b + 1], _rects(n)))
            for w, o in zip(whole, one):
                assert np.array_equal(w[b].cpu().numpy().view(np.uint32), o[0].cpu().numpy().view(np.uint32)), (group[b], n)
        perm = [2, 0, 1]
        pt = torch.tensor(perm, device=cuda)
        moved = engine.screen_aligned_scores(ctx, alt[pt], ref, bm[perm]) + engine.screen_aligned_region_scores(ctx, alt[pt], ref, bm[perm], _rects(n))
        for w, m in zip(whole, moved):
            assert np.array_equal(w[pt].cpu().numpy().view(np.uint32), m.cpu().numpy().view(np.uint32)), (group, n)


def test_nan_shows_at_a_mapped_pair_only(cuda):
    ctx = engine.get_context(cuda)
    n = 50
    bm = np.arange(n, dtype=np.int32)
    bm[[4, 17, 30]] = -1
    bm = bm[None]
    alt, ref = _alt(np.random.RandomState(1), 1, n, cuda)
    alt, ref = alt.contiguous(), ref.contiguous()
    rects = [(0, n, 0, n), (10, 20, 25, 40), (0, 4, 0, 4)]
    clean = engine.screen_aligned_scores(ctx, alt, ref, bm) + engine.screen_aligned_region_scores(ctx, alt, ref, bm, rects)
    # unmapped pairs: an alt row, an alt column and the reference rows / columns nobody stands for
    a2, r2 = alt.clone(), ref.clone()
    a2[0, 4, :] = float("nan")
    a2[0, :, 17] = float("nan")
    a2[0, 30, 30] = float("inf")
    r2[4, :] = float("nan")
    r2[:, 30] = float("nan")
    quiet = engine.screen_aligned_scores(ctx, a2, r2, bm) + engine.screen_aligned_region_scores(ctx, a2, r2, bm, rects)
    for c, q in zip(clean, quiet):
        assert np.array_equal(c.cpu().numpy().view(np.uint32), q.cpu().numpy().view(np.uint32))
    # one mapped pair, alt (12, 33): row 12 of the profile, the mean, the max and the rectangles that hold it
    a3 = alt.clone()
    a3[0, 12, 33] = float("nan")
    prof, mean, amax = engine.screen_aligned_scores(ctx, a3, ref, bm)
    sg, ab = engine.screen_aligned_region_scores(ctx, a3, ref, bm, rects)
    hp, hm, hx = S.aligned_scores_host(a3.cpu().numpy(), ref.cpu().numpy(), bm)
    close(prof.cpu().numpy(), hp)
    keep = torch.ones(n, dtype=torch.bool, device=cuda)
    keep[12] = False
    assert torch.isnan(prof[0, 12]) and torch.equal(prof[0, keep].isnan(), clean[0][0, keep].isnan()) and int(prof[0].isnan().sum()) == 4
    assert np.isnan(hm[0]) and np.isnan(hx[0]) and torch.isnan(mean[0]) and torch.isnan(amax[0])
    assert torch.isnan(sg[0, 0]) and torch.isnan(sg[0, 1]) and torch.isnan(ab[0, 1]) and sg[0, 2] == clean[3][0, 2] and ab[0, 2] == clean[4][0, 2]
    # ... and a NaN in the reference at a pair some alt pair stands for
    r3 = ref.clone()
    r3[12, 33] = float("nan")
    prof, mean, amax = engine.screen_aligned_scores(ctx, alt, r3, bm)
    assert torch.isnan(prof[0, 12]) and int(prof[0].isnan().sum()) == 4 and torch.isnan(mean[0]) and torch.isnan(amax[0])


def test_rectangles_in_reference_bins(cuda):
    """A deletion of bins 10 .. 14 (the alt map closes up, the refill is unmapped), an insertion of two bins at bin 10, and a shared bin."""
    ctx = engine.get_context(cuda)
    n = 50
    i = np.arange(n)
    dele = np.where(i < 10, i, np.where(i + 5 < n, i + 5, -1))
    ins = np.where(i < 10, i, np.where(i < 12, -1, i - 2))
    bm = np.stack([dele, ins, np.maximum(i - 1, 0)]).astype(np.int32)
    rects = [(20, 30, 25, 40), (8, 17, 5, 20), (10, 15, 10, 15), (10, 15, 0, n), (48, 50, 0, 10)]      # inside; across the hole; deleted; deleted rows; pushed out
    alt, ref = _alt(np.random.RandomState(2), 3, n, cuda)
    sg, ab = engine.screen_aligned_region_scores(ctx, alt, ref, bm, rects)
    hs, ha = S.aligned_region_scores_host(alt.cpu().numpy(), ref.cpu().numpy(), bm, rects)
    close(sg.cpu().numpy(), hs)
    close(ab.cpu().numpy(), ha)
    assert torch.isnan(sg[0, 2:4]).all() and torch.isnan(ab[0, 2:4]).all() and torch.isfinite(sg[0, :2]).all() and torch.isfinite(sg[0, 4])
    assert torch.isnan(sg[1, 4]) and torch.isfinite(sg[1, :4]).all() and torch.isfinite(sg[2]).all()
    # the deleted region by hand: rectangle 1 of map 0 is alt rows {8, 9, 10, 11} (reference 8, 9, 15, 16) x alt columns 5 .. 14
    a, r = alt[0].cpu().numpy().astype(np.float64), ref.cpu().numpy().astype(np.float64)
    rows, cols = [8, 9, 10, 11], list(range(5, 15))
    d = a[np.ix_(rows, cols)] - r[np.ix_([8, 9, 15, 16], [5, 6, 7, 8, 9, 15, 16, 17, 18, 19])]
    close(sg[0, 1].cpu().numpy(), d.mean())
    close(ab[0, 1].cpu().numpy(), np.abs(d).mean())


# ---- the screen ---------------------------------------------------------------------------------------------------------------------------------------
def _items(c):
    return {
        "snv": snv(c, 77_777),
        "inv": S.Edit("inv", 150_000, 1_300),
        "del3": S.Edit("del", 50_001, 3),
        "del4000": S.Edit("del", 90_500, 4_000),
        "del40000": S.Edit("del", 60_000, 40_000),
        "ins6000": S.Edit("ins", 30_100, np.random.RandomState(4).randint(0, 4, 6_000).astype(np.uint8)),
        "dup8000": S.tandem_dup(c, 110_000, 8_000),
        "balanced": S.EditSet([S.Edit("del", 100_000, 4_000), S.Edit("ins", 120_000, np.random.RandomState(6).randint(0, 4, 4_000).astype(np.uint8))]),
    }


@pytest.fixture(scope="module")
def case(cuda):
    c, fl = _window(), plan_flank(F)
    assert c.size == L
    items = _items(c)
    model = M.H1esc_1M(synthetic_seed=0).to(cuda)
    win, flank = torch.from_numpy(c).to(cuda), torch.from_numpy(fl).to(cuda)
    st = {}
    res = S.screen_1m(model, win, list(items.values()), keep_maps=True, stats=st, regions=REGIONS, flank=flank, aligned=True)
    return c, fl, items, model, win, flank, res, st


def test_screen_aligned_fields_equal_the_host_restatements(case, cuda):
    """Every aligned field against the numpy restatement on ``res.maps``, ``res.ref_map`` and `screen.bin_map`.  Printed, not asserted (on synthetic
    weights nobody knows which is smaller): the aligned and the bin-with-bin mean score of the 40 000-base deletion."""
    c, fl, items, model, win, flank, res, st = case
    lst = list(items.values())
    host = np.stack([S.bin_map(v, L, F) for v in lst])
    assert res.bin_map.dtype == torch.int32 and np.array_equal(res.bin_map.cpu().numpy(), host)
    assert res.aligned_bins.dtype == torch.int64 and res.aligned_bins.tolist() == (host >= 0).sum(axis=1).tolist()
    ident = [k for k, m in zip(items, host) if np.array_equal(m, np.arange(NB))]
    assert ident == ["snv", "inv", "del3"] and st["aligned_items"] == len(items) - 3 == 5 and st["route"] == "two_part"
    k40 = list(items).index("del40000")
    assert host[k40].tolist() == list(range(15)) + list(range(25, 50)) + [-1] * 10 and int(res.aligned_bins[k40]) == 40
    maps, ref = res.maps.cpu().numpy(), res.ref_map.cpu().numpy()
    hp, hm, hx = S.aligned_scores_host(maps, ref, host)
    close(res.aligned_profile.cpu().numpy(), hp, "aligned_profile")
    close(res.aligned_abs_mean.cpu().numpy(), hm, "aligned_abs_mean")
    same_max(res.aligned_abs_max.cpu().numpy(), hx, "aligned_abs_max")
    hs, ha = S.aligned_region_scores_host(maps, ref, host, REGIONS)
    close(res.aligned_region.cpu().numpy(), hs, "aligned_region")
    close(res.aligned_region_abs.cpu().numpy(), ha, "aligned_region_abs")
    assert tuple(res.aligned_profile.shape) == (len(items), NB) and tuple(res.aligned_region.shape) == (len(items), len(REGIONS))
    assert torch.isfinite(res.aligned_abs_mean).all() and torch.isnan(res.aligned_profile[k40, 40:]).all() and torch.isfinite(res.aligned_profile[k40, :40]).all()
    print("del40000: aligned_abs_mean", float(res.aligned_abs_mean[k40]), "delta_abs_mean (bin with bin)", float(res.delta_abs_mean[k40]),
          "aligned_abs_max", float(res.aligned_abs_max[k40]), "delta_abs_max", float(res.delta_abs_max[k40]))
    print("aligned_abs_mean per item:", {k: float(v) for k, v in zip(items, res.aligned_abs_mean)})
    print("delta_abs_mean per item:", {k: float(v) for k, v in zip(items, res.delta_abs_mean)})


def test_identity_maps_give_the_bin_with_bin_scores(case, cuda):
    """Where the bin map is the identity the aligned scores are the ``delta_*`` scores up to the rounding of the differences (fp32 there, fp64
    here: one more fp32 ulp, still inside RTOL)."""
    c, fl, items, model, win, flank, res, st = case
    for name in ("snv", "inv", "del3"):
        k = list(items).index(name)
        close(res.aligned_profile[k].cpu().numpy(), res.delta_profile[k].cpu().numpy(), name)
        close(res.aligned_abs_mean[k].cpu().numpy(), res.delta_abs_mean[k].cpu().numpy(), name)
        close(res.aligned_abs_max[k].cpu().numpy(), res.delta_abs_max[k].cpu().numpy(), name)
        close(res.aligned_region[k].cpu().numpy(), res.delta_region[k].cpu().numpy(), name)
        close(res.aligned_region_abs[k].cpu().numpy(), res.delta_region_abs[k].cpu().numpy(), name)


def test_aligned_changes_nothing_else(case, cuda):
    c, fl, items, model, win, flank, res, st = case
    st2 = {}
    plain = S.screen_1m(model, win, list(items.values()), keep_maps=True, stats=st2, regions=REGIONS, flank=flank)
    for name in ("ref_map", "ref_1d", "maps", "delta_profile", "delta_abs_mean", "delta_abs_max", "delta_1d", "delta_region", "delta_region_abs", "shift"):
        assert torch.equal(getattr(plain, name), getattr(res, name)), name
    for name in ("bin_map", "aligned_bins", "aligned_profile", "aligned_abs_mean", "aligned_abs_max", "aligned_region", "aligned_region_abs"):
        assert getattr(plain, name) is None and getattr(res, name) is not None, name
    assert st2["aligned_items"] == 0 and {k: v for k, v in st.items() if k != "aligned_items"} == {k: v for k, v in st2.items() if k != "aligned_items"}
    no_regions = S.screen_1m(model, win, [items["del4000"]], flank=flank, aligned=True)
    assert no_regions.aligned_region is None and no_regions.aligned_region_abs is None and tuple(no_regions.aligned_profile.shape) == (1, NB)
    # batches of 3: every batch's scores come from that batch's maps and its rows of the bin map
    small = S.screen_1m(model, win, list(items.values()), batch=3, keep_maps=True, regions=REGIONS, flank=flank, aligned=True)
    assert torch.equal(small.bin_map, res.bin_map) and torch.equal(small.aligned_bins, res.aligned_bins)
    hp, hm, hx = S.aligned_scores_host(small.maps.cpu().numpy(), small.ref_map.cpu().numpy(), small.bin_map.cpu().numpy())
    hs, ha = S.aligned_region_scores_host(small.maps.cpu().numpy(), small.ref_map.cpu().numpy(), small.bin_map.cpu().numpy(), REGIONS)
    close(small.aligned_profile.cpu().numpy(), hp, "batch 3 profile")
    close(small.aligned_abs_mean.cpu().numpy(), hm, "batch 3 mean")
    same_max(small.aligned_abs_max.cpu().numpy(), hx, "batch 3 max")
    close(small.aligned_region.cpu().numpy(), hs, "batch 3 region")
    close(small.aligned_region_abs.cpu().numpy(), ha, "batch 3 region abs")
    for name in ("aligned_profile", "aligned_abs_mean", "aligned_abs_max", "aligned_region", "aligned_region_abs"):     # the maps are the same bits, so are these
        assert np.array_equal(getattr(small, name).cpu().numpy(), getattr(res, name).cpu().numpy(), equal_nan=True), name
    # the aligned scores of the whole-window route come from that route's maps
    st3 = {}
    with engine.force_safe_precision():
        ww = S.screen_1m(model, win, [items["del40000"], items["dup8000"]], keep_maps=True, stats=st3, regions=REGIONS, flank=flank, aligned=True)
    assert st3["route"] == "whole_window" and st3["aligned_items"] == 2
    host = np.stack([S.bin_map(items[k], L, F) for k in ("del40000", "dup8000")])
    hp, hm, hx = S.aligned_scores_host(ww.maps.cpu().numpy(), ww.ref_map.cpu().numpy(), host)
    close(ww.aligned_profile.cpu().numpy(), hp)
    close(ww.aligned_abs_mean.cpu().numpy(), hm)
    same_max(ww.aligned_abs_max.cpu().numpy(), hx)


def test_flank_bp_reads_the_flank_from_the_genome(case, cuda):
    from orca_amd.genome import PackedGenome
    c, fl, items, model, win, flank, res, st = case
    genome = PackedGenome({"chrS": np.concatenate([c, fl, fl[:10_000]])}).to(cuda)
    pick = ["del40000", "ins6000"]
    it = [items[k] for k in pick]
    idx = torch.tensor([list(items).index(k) for k in pick], device=cuda)
    a = S.screen_1m(model, (genome, "chrS", 0, L), it, keep_maps=True, flank_bp=F, aligned=True)
    assert torch.equal(a.maps, res.maps[idx]) and torch.equal(a.bin_map, res.bin_map[idx])
    assert np.array_equal(a.aligned_profile.cpu().numpy(), res.aligned_profile[idx].cpu().numpy(), equal_nan=True)
    default = S.screen_1m(model, (genome, "chrS", 0, L), it, keep_maps=True)                   # FLANK_BP bases, as before
    today = S.screen_1m(model, win, it, keep_maps=True, flank=flank[: S.FLANK_BP].clone())
    assert torch.equal(default.maps, today.maps) and not torch.equal(default.maps[0], a.maps[0])
    more = S.screen_1m(model, (genome, "chrS", 0, L), it, keep_maps=True, flank_bp=L)           # fewer at the chromosome's end: F + 10 000 are there
    assert torch.equal(more.maps, S.screen_1m(model, win, it, keep_maps=True, flank=torch.cat([flank, flank[:10_000]])).maps)
    none = S.screen_1m(model, (genome, "chrS", 0, L), it, keep_maps=True, flank_bp=0)
    assert torch.equal(none.maps, S.screen_1m(model, win, it, keep_maps=True).maps)
    with pytest.raises(ValueError):
        S.screen_1m(model, (genome, "chrS", 0, L), it, flank=flank, flank_bp=F)
    with pytest.raises(ValueError):
        S.screen_1m(model, win, it, flank_bp=F)
    with pytest.raises(ValueError):
        S.screen_1m(model, (genome, "chrS", 0, L), it, flank_bp=L + 1)
    with pytest.raises(ValueError):
        S.screen_1m(model, (genome, "chrS", 0, L), it, flank_bp=-1)


# ---- argument checks: return codes only -----------------------------------------------------------------------------------------------------------------
def _hp(a):
    return ctypes.c_void_p(a.ctypes.data)


def _dp(t):
    return ctypes.c_void_p(t.data_ptr())


def _refused(rc):
    msg = _lib.load().orca_last_error()
    assert rc != 0 and msg and len(msg) > 20, (rc, msg)
    return msg.decode()


def test_bad_arguments_are_refused_before_any_launch(cuda):
    """Every call below is refused by the host entry point's checks, so nothing of it reaches a kernel; the output buffers keep their fill."""
    lib = _lib.load()
    h = engine.get_context(cuda).handle
    null = ctypes.c_void_p(0)
    n, B = 6, 2
    alt = torch.zeros((B, n, n), dtype=torch.float32, device=cuda)
    ref = torch.zeros((n, n), dtype=torch.float32, device=cuda)
    dev = torch.zeros(256, dtype=torch.int32, device=cuda)                      # stands for every device table: never read
    outs = [torch.full((B * n,), 7.0, dtype=torch.float32, device=cuda) for _ in range(5)]
    good = np.ascontiguousarray([[0, 1, -1, 2, 3, 5], [-1] * 6], dtype=np.int32)
    good_r = np.ascontiguousarray([[0, 6, 0, 6], [2, 3, 4, 5]], dtype=np.int32)

    def bad_map(v):
        m = good.copy()
        m[1, 4] = v
        return m

    def scores(bm=good, a=_dp(alt), r=_dp(ref), bm_dev=_dp(dev), host=True, nb=B, nn=n, bs=n * n, o=(_dp(outs[0]), _dp(outs[1]), _dp(outs[2]))):
        return lib.orca_screen_aligned_scores(h, a, bs, r, nb, nn, bm_dev, _hp(bm) if host else null, *o)

    def regions(bm=good, rc=good_r, K=2, a=_dp(alt), r=_dp(ref), bm_dev=_dp(dev), host=True, rc_dev=_dp(dev), rc_host=True, nb=B, nn=n,
                o=(_dp(outs[3]), _dp(outs[4]))):
        return lib.orca_screen_aligned_region_scores(h, a, n * n, r, nb, nn, bm_dev, _hp(bm) if host else null, rc_dev, _hp(rc) if rc_host else null, K, *o)
    for call in (scores, regions):
        assert "outside -1" in _refused(call(bm=bad_map(n)))                       # a map value n
        assert "outside -1" in _refused(call(bm=bad_map(-2)))                      # a map value -2
        assert "NULL" in _refused(call(host=False))                                # no host copy of the map
        assert "NULL" in _refused(call(bm_dev=null)) and "NULL" in _refused(call(a=null)) and "NULL" in _refused(call(r=null))
        _refused(call(nb=-1))
        _refused(call(nn=0))
        _refused(call(nn=257))
    assert "NULL" in _refused(scores(o=(null, _dp(outs[1]), _dp(outs[2])))) and "NULL" in _refused(regions(o=(_dp(outs[3]), null)))
    _refused(scores(bs=-1))
    assert "rectangles" in _refused(regions(K=0)) and "rectangles" in _refused(regions(K=65))
    assert "NULL" in _refused(regions(rc_host=False)) and "NULL" in _refused(regions(rc_dev=null))
    assert "rectangle 1" in _refused(regions(rc=np.ascontiguousarray([[0, 6, 0, 6], [2, 2, 4, 5]], dtype=np.int32)))      # empty
    assert "rectangle 0" in _refused(regions(rc=np.ascontiguousarray([[0, 7, 0, 6], [2, 3, 4, 5]], dtype=np.int32)))      # leaves the map
    torch.cuda.synchronize()
    assert all(bool((o == 7).all()) for o in outs)
    # the wrappers turn the same refusals into OrcaHipError
    ctx = engine.get_context(cuda)
    with pytest.raises(OrcaHipError):
        engine.screen_aligned_scores(ctx, alt, ref, bad_map(n))
    with pytest.raises(OrcaHipError):
        engine.screen_aligned_region_scores(ctx, alt, ref, bad_map(-2), good_r)
    with pytest.raises(OrcaHipError):
        engine.screen_aligned_region_scores(ctx, alt, ref, good, np.zeros((0, 4), dtype=np.int32))
    with pytest.raises(ValueError):
        engine.screen_aligned_scores(ctx, alt, ref, good[:1])
