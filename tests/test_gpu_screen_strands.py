"""``screen_1m(..., strands="both")`` on the MI355X: orca_screen_merge_strands alone against torch, orca_strand_merge and the fp64 host restatement
(`screen.merge_strands_host`), then the screen on a 200 000-base window (synthetic H1esc_1M(synthetic_seed=0)) with 8 000 bases of flank: every merged
map and 1-D head against model.net on the alt window and on its reverse complement merged on the host, the mirror symmetry, bit-for-bit invariance to
the batch, the unchanged default, the scores against the host functions, and the fallbacks.

Tolerances.  The merge is exact up to the one rounding of the sum, and the kernel's expression is orca_strand_merge's: ``torch.equal``.  The gap is a
sum of at most 65 536 fp64 terms that the two sides associate differently (1e-11 level), so only the final rounding to fp32 can differ: RTOL = 2.4e-7,
two fp32 ulps, the bound of tests/test_gpu_screen_aligned.py.  Maps against model.net: TOL of tests/test_gpu_screen.py, over the scale."""
import ctypes

import numpy as np
import pytest
import torch

from orca_amd import _lib, engine
from orca_amd import orca_models as M
from orca_amd import orca_modules as pm
from orca_amd import screen as S
from orca_amd import synth
from orca_amd._lib import OrcaHipError
from tests.encoder_ref import revcomp
from tests.test_gpu_screen import TOL, _net_on
from tests.test_gpu_screen_aligned import close, same_max
from tests.test_gpu_screen_sets import _check_regions, _window
from tests.test_screen_indel_cpu import plan_flank
from tests.test_screen_sets_cpu import snv
from tests.util import maxabs

pytestmark = pytest.mark.gpu

L, F = 200_000, 8_000
NB = L // 4000
REGIONS = [(5, 15, 20, 35), (30, 45, 30, 45)]
FIELDS = ("maps", "delta_profile", "delta_abs_mean", "delta_abs_max", "delta_1d", "strand_gap")


# ---- the kernel ---------------------------------------------------------------------------------------------------------------------------------------
def _maps(rs, B, n, cuda, pad=7):
    """B random maps (the same values whatever ``pad``) with a batch stride of n * n + pad."""
    buf = torch.zeros((B, n * n + pad), dtype=torch.float32, device=cuda)
    buf[:, : n * n] = torch.from_numpy(rs.randn(B, n * n).astype(np.float32)).to(cuda)
    return buf.as_strided((B, n, n), (n * n + pad, n, 1))


def _bits(t):
    return t.cpu().numpy().view(np.uint32)


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("n", [1, 2, 5, 50, 250, 256])
def test_merge_kernel_equals_torch_strand_merge_and_the_host(cuda, n, B):
    """Odd n pairs the centre element with itself, 250 is the row that is only 8-byte aligned, 256 the cap; the batch strides are n * n + 7 (odd: the
    scalar accesses) and n * n + 8 (the float2 ones where n is even) - the same bits either way."""
    ctx = engine.get_context(cuda)
    rs = np.random.RandomState(1000 * n + B)
    ref_p, ref_m = (torch.from_numpy(rs.randn(n, n).astype(np.float32)).to(cuda) for _ in range(2))
    results = []
    for pad in (7, 8):
        rs2 = np.random.RandomState(n + B)
        a, b = _maps(rs2, B, n, cuda, pad), _maps(rs2, B, n, cuda, pad)
        assert a.stride(0) > n * n
        out, gap = engine.screen_merge_strands(ctx, a, b, ref_p, ref_m)
        assert torch.equal(out, 0.5 * a + 0.5 * b.flip(-1, -2))
        for k in range(B):
            assert torch.equal(out[k], engine.strand_merge(a[k].contiguous(), b[k].contiguous())), k
        hm, hg = S.merge_strands_host(a.cpu().numpy(), b.cpu().numpy(), ref_p.cpu().numpy(), ref_m.cpu().numpy())
        assert np.array_equal(out.cpu().numpy(), hm.astype(np.float32))
        close(gap.cpu().numpy(), hg, ("gap", n, B, pad))
        plain, none = engine.screen_merge_strands(ctx, a, b)                       # the form without references: the same maps, no gap
        assert none is None and torch.equal(plain, out)
        for k in range(B):                                                        # a map alone (contiguous: another stride) and inside the batch
            o1, g1 = engine.screen_merge_strands(ctx, a[k: k + 1].contiguous(), b[k: k + 1].contiguous(), ref_p, ref_m)
            assert np.array_equal(_bits(g1[0]), _bits(gap[k])) and torch.equal(o1[0], out[k])
        a2 = a.clone()                                                            # out aliased to fwd: the same bits
        o2, g2 = engine.screen_merge_strands(ctx, a2, b, ref_p, ref_m, out=a2)
        assert o2.data_ptr() == a2.data_ptr() and torch.equal(a2, out) and np.array_equal(_bits(g2), _bits(gap))
        results.append((out.clone(), gap.clone()))
    assert torch.equal(results[0][0], results[1][0]) and np.array_equal(_bits(results[0][1]), _bits(results[1][1]))     # scalar and float2 accesses


def test_merge_kernel_nan_shows_in_its_two_mirrored_elements(cuda):
    ctx = engine.get_context(cuda)
    n, B = 50, 3
    rs = np.random.RandomState(5)
    a, b = _maps(rs, B, n, cuda), _maps(rs, B, n, cuda)
    ref_p, ref_m = (torch.from_numpy(rs.randn(n, n).astype(np.float32)).to(cuda) for _ in range(2))
    clean, cgap = engine.screen_merge_strands(ctx, a, b, ref_p, ref_m)
    a2, b2 = a.clone(), b.clone()
    a2[1, 12, 33] = float("nan")                                   # shows at (12, 33)
    b2[1, 12, 33] = float("nan")                                   # shows at the mirrored place (37, 16)
    out, gap = engine.screen_merge_strands(ctx, a2, b2, ref_p, ref_m)
    nan = torch.isnan(out)
    assert int(nan.sum()) == 2 and bool(nan[1, 12, 33]) and bool(nan[1, n - 1 - 12, n - 1 - 33])
    assert torch.equal(out[~nan], clean[~nan])
    assert torch.isnan(gap[1]) and np.array_equal(_bits(gap[[0, 2]]), _bits(cgap[[0, 2]]))
    r2 = ref_m.clone()                                              # a NaN in a reference: every gap, no map
    r2[3, 4] = float("nan")
    out, gap = engine.screen_merge_strands(ctx, a, b, ref_p, r2)
    assert torch.equal(out, clean) and torch.isnan(gap).all()


def _refused(rc):
    msg = _lib.load().orca_last_error()
    assert rc != 0 and msg and len(msg) > 20, (rc, msg)
    return msg.decode()


def test_merge_bad_arguments_are_refused_before_any_launch(cuda):
    lib = _lib.load()
    h = engine.get_context(cuda).handle
    null = ctypes.c_void_p(0)
    n, B = 6, 2
    fwd, rev, out = (torch.full((B, n, n), v, dtype=torch.float32, device=cuda) for v in (1.0, 2.0, 7.0))
    ref = torch.zeros((n, n), dtype=torch.float32, device=cuda)
    gap = torch.full((B,), 7.0, dtype=torch.float32, device=cuda)

    def dp(t):
        return ctypes.c_void_p(t.data_ptr())

    def call(f=dp(fwd), fbs=n * n, r=dp(rev), rbs=n * n, rf=dp(ref), rr=dp(ref), nb=B, nn=n, o=dp(out), obs=n * n, g=dp(gap), ctx=h):
        return lib.orca_screen_merge_strands(ctx, f, fbs, r, rbs, rf, rr, nb, nn, o, obs, g)
    for kw in (dict(f=null), dict(r=null), dict(o=null), dict(ctx=null)):
        assert "NULL" in _refused(call(**kw))
    for kw in (dict(nn=0), dict(nn=257), dict(nn=-3), dict(nb=0), dict(nb=-1)):
        assert "bins" in _refused(call(**kw))
    for kw in (dict(fbs=n * n - 1), dict(rbs=0), dict(obs=-1)):
        assert "stride" in _refused(call(**kw))
    assert "ref_rev" in _refused(call(rr=null))
    assert "overlaps" in _refused(call(o=dp(rev)))
    assert "overlaps" in _refused(call(o=ctypes.c_void_p(rev.data_ptr() + 4 * n * n)))          # the second map of rev
    torch.cuda.synchronize()
    assert bool((out == 7).all()) and bool((gap == 7).all()) and bool((rev == 2).all())
    ctx = engine.get_context(cuda)
    with pytest.raises(OrcaHipError):
        engine.screen_merge_strands(ctx, fwd, rev, out=rev)
    with pytest.raises(ValueError):
        engine.screen_merge_strands(ctx, fwd, rev, ref)
    with pytest.raises(ValueError):
        engine.screen_merge_strands(ctx, fwd, rev[:1])
    # ref_fwd == NULL with a gap buffer: the gap is skipped, the maps are merged
    assert call(rf=null) == 0
    torch.cuda.synchronize()
    assert bool((out == 1.5).all()) and bool((gap == 7).all())


# ---- the screen ---------------------------------------------------------------------------------------------------------------------------------------
SNVS = ("snv0", "snv1", "snvL2", "snvL1")


def _lp_items(c):
    """Length-preserving items: masks and inversions at both window ends, in the middle and across an N run, the four SNVs at the window's ends, a set
    with two clusters."""
    return {
        "mask_start": S.Edit("mask", 0, 2_000), "mask_end": S.Edit("mask", L - 2_000, 2_000), "inv_start": S.Edit("inv", 0, 3_000),
        "inv_end": S.Edit("inv", L - 3_000, 3_000), "mask_mid": S.Edit("mask", 60_000, 2_000), "inv_mid": S.Edit("inv", 140_000, 3_000),
        "inv_n": S.Edit("inv", 99_000, 2_000), "mask_n": S.Edit("mask", 2_500, 1_500),
        "snv0": snv(c, 0), "snv1": snv(c, 1), "snvL2": snv(c, L - 2), "snvL1": snv(c, L - 1),
        "two": S.EditSet([S.Edit("mask", 30_000, 1_200), S.Edit("inv", 150_000, 1_500)], name="two clusters"),
    }


def _indel_items(c):
    rs = np.random.RandomState(8)
    return {
        "del": S.Edit("del", 50_001, 4_300), "ins": S.Edit("ins", 30_100, rs.randint(0, 4, 6_000).astype(np.uint8)),
        "unbalanced": S.EditSet([S.Edit("del", 100_000, 2_000), S.Edit("ins", 120_000, rs.randint(0, 4, 500).astype(np.uint8))]),
        # an insertion at base 0: behind it the takes begin one row later than on the '+' strand alone (`item_sources`, both_strands)
        "ins_start": S.EditSet([S.Edit("ins", 0, rs.randint(0, 4, 177).astype(np.uint8)), S.Edit("mask", 160_000, 2_000)]),
    }


def _mirrored(item):
    """The item that does to revcomp(window) what ``item`` does to the window (length-preserving members only)."""
    out = []
    for e in S.members_of(item):
        out.append(S.Edit(e.kind, L - e.end, e.length, revcomp(e.seq) if e.kind == "sub" else None))
    return out[0] if isinstance(item, S.Edit) else S.EditSet(out, item.name)


def _both_on_net(net, wins, dev):
    """The reference side, without the screen: model.net on the windows and on their reverse complements, merged on the host (fp64)."""
    plus, hp = _net_on(net, wins, dev)
    minus, hm = _net_on(net, np.stack([revcomp(w) for w in wins]), dev)
    merged, _ = S.merge_strands_host(plus, minus)
    return merged, 0.5 * hp.astype(np.float64) + 0.5 * hm.astype(np.float64)[..., ::-1], plus, minus


@pytest.fixture(scope="module")
def case(cuda):
    c, fl = _window(), plan_flank(F)
    assert c.size == L
    lp, ind = _lp_items(c), _indel_items(c)
    items = {**lp, **ind}
    model = M.H1esc_1M(synthetic_seed=0).to(cuda)
    win, flank = torch.from_numpy(c).to(cuda), torch.from_numpy(fl).to(cuda)
    st = {}
    res = S.screen_1m(model, win, list(items.values()), keep_maps=True, stats=st, regions=REGIONS, flank=flank, aligned=True, strands="both")
    return c, fl, lp, ind, items, model, win, flank, res, st


def test_merged_maps_equal_the_model_on_both_strands(case, cuda):
    """Every merged map, ``ref_map`` and the merged 1-D heads against model.net on `apply_edit`'s window and on its reverse complement, merged on the
    host: within TOL of max-abs over the scale.  Every item but the four SNVs moves the reference side's merged map by at least 10 x TOL x scale,
    so the bound means something.  Every item's '-' strand runs two-part, the ``del`` / ``ins`` items' from the '-' strand's stage-4 cache entries.
    Measured on the MI355X (scale 1.0): ref_map 2.5e-7, worst map 3.0e-7, worst head 2.1e-7; the smallest move is inv_start's, 31.8 x TOL x scale
    (the SNVs: 0.5 to 0.6)."""
    c, fl, lp, ind, items, model, win, flank, res, st = case
    wins = np.stack([c] + [S.apply_edit(c, it, fl) for it in items.values()])
    merged, heads, plus, minus = _both_on_net(model.net, wins, cuda)
    scale = max(1.0, float(np.abs(merged).max()))
    err_ref = maxabs(res.ref_map.cpu().numpy(), merged[0]) / scale
    errs = {k: maxabs(res.maps[i].cpu().numpy(), merged[1 + i]) / scale for i, k in enumerate(items)}
    moves = {k: float(np.abs(merged[1 + i] - merged[0]).max()) / (TOL * scale) for i, k in enumerate(items)}
    err_h = max(maxabs(res.ref_1d.cpu().numpy(), heads[0]), maxabs(res.delta_1d.cpu().numpy() + res.ref_1d.cpu().numpy()[None], heads[1:]))
    print("strands=both: scale", scale, "ref_map error / scale", err_ref, "worst map error / scale", max(errs.values()), "worst head error", err_h)
    print("moves / (TOL x scale):", {k: round(v, 1) for k, v in moves.items()})
    assert err_ref < TOL and err_h < TOL
    for k, v in errs.items():
        assert v < TOL, (k, v)
    for k, v in moves.items():
        assert k in SNVS or v >= 10, (k, v)
    # the gaps are what the host restatement makes of the reference side's strands, up to the maps' own error
    _, gaps = S.merge_strands_host(plus[1:], minus[1:], plus[0], minus[0])
    assert maxabs(res.strand_gap.cpu().numpy(), gaps) < 4 * TOL * scale
    assert abs(float(res.ref_strand_gap) - float(np.abs(plus[0] - minus[0][::-1, ::-1]).mean())) < 2 * TOL * scale
    assert res.ref_strand_gap.dim() == 0 and tuple(res.strand_gap.shape) == (len(items),)
    assert st["route"] == "two_part" and st["strands"] == "both" and st["range_fallback_batches"] == 0 and st["two_part_batches"] == 1
    assert st["reverse_two_part_items"] == len(items) and st["reverse_whole_items"] == 0 and st["indel_items"] == len(ind) and st["take_rows"] > 0
    plus = S.needed_phases(list(ind.values()), L, F, both_strands=True)
    assert st["cache_phases"] == 5 * (len({ph % 16 for ph in plus}) + len({ph % 16 for ph in S.mirror_phases(plus, L + F)}))        # both strands' entries


def test_scores_equal_the_host_functions_on_the_merged_maps(case, cuda):
    c, fl, lp, ind, items, model, win, flank, res, st = case
    maps, ref = res.maps.cpu().numpy(), res.ref_map.cpu().numpy()
    prof, mean, amax = S.scores_host(maps, ref)
    for got, want in ((res.delta_profile, prof), (res.delta_abs_mean, mean), (res.delta_abs_max, amax)):
        g = got.cpu().numpy().astype(np.float64)
        assert np.all(np.abs(g - want) <= 1e-6 * np.maximum(np.abs(want), 1e-30)), float(np.abs(g - want).max())
    _check_regions(res.delta_region, res.delta_region_abs, maps, ref, REGIONS)
    host = np.stack([S.bin_map(v, L, F) for v in items.values()])
    assert np.array_equal(res.bin_map.cpu().numpy(), host)
    hp, hm, hx = S.aligned_scores_host(maps, ref, host)
    close(res.aligned_profile.cpu().numpy(), hp, "aligned_profile")
    close(res.aligned_abs_mean.cpu().numpy(), hm, "aligned_abs_mean")
    same_max(res.aligned_abs_max.cpu().numpy(), hx, "aligned_abs_max")
    hs, ha = S.aligned_region_scores_host(maps, ref, host, REGIONS)
    close(res.aligned_region.cpu().numpy(), hs, "aligned_region")
    close(res.aligned_region_abs.cpu().numpy(), ha, "aligned_region_abs")
    assert torch.equal(res.shift.cpu(), torch.tensor([S.shift_of(v) for v in items.values()]))


def test_mirror_symmetry(case, cuda):
    """strands="both" on revcomp(window) with the mirrored items gives the flipped maps of the original call, within TOL: the two calls reach the same
    two strands by different routes (what was the front's reverse run is now its forward run), so equal bits are not promised (on the MI355X
    they did come out equal)."""
    c, fl, lp, ind, items, model, win, flank, res, st = case
    rwin = torch.from_numpy(revcomp(c)).to(cuda)
    for k, it in lp.items():                                                   # the mirrored item does do the mirrored thing
        assert np.array_equal(S.apply_edit(revcomp(c), _mirrored(it)), revcomp(S.apply_edit(c, it))), k
    st2 = {}
    mir = S.screen_1m(model, rwin, [_mirrored(v) for v in lp.values()], keep_maps=True, stats=st2, strands="both")
    assert st2["route"] == "two_part" and st2["reverse_two_part_items"] == len(lp) and st2["reverse_whole_items"] == 0
    n_lp = len(lp)
    scale = max(1.0, float(res.maps.abs().max()))
    assert maxabs(mir.ref_map.flip(-1, -2).cpu().numpy(), res.ref_map.cpu().numpy()) / scale < TOL
    assert maxabs(mir.maps.flip(-1, -2).cpu().numpy(), res.maps[:n_lp].cpu().numpy()) / scale < TOL
    assert maxabs(mir.ref_1d.flip(-1).cpu().numpy(), res.ref_1d.cpu().numpy()) < TOL
    assert maxabs(mir.delta_1d.flip(-1).cpu().numpy(), res.delta_1d[:n_lp].cpu().numpy()) < 2 * TOL


def test_both_strands_are_batch_invariant(case, cuda):
    """Bit for bit whatever the batch size and the order (``del`` / ``ins`` items included), and a length-preserving item keeps its bits when an
    indel item joins its batch."""
    c, fl, lp, ind, items, model, win, flank, res, st = case
    lst = list(lp.values())
    base = S.screen_1m(model, win, lst, batch=64, keep_maps=True, strands="both")
    for name in FIELDS:                                                        # alone against beside the three indel items (the fixture's batch)
        assert torch.equal(getattr(base, name), getattr(res, name)[: len(lst)]), name
    assert torch.equal(base.ref_map, res.ref_map) and torch.equal(base.ref_strand_gap, res.ref_strand_gap)
    for b in (1, 7):
        r2 = S.screen_1m(model, win, lst, batch=b, keep_maps=True, strands="both")
        for name in FIELDS:
            assert torch.equal(getattr(r2, name), getattr(base, name)), (b, name)
    perm = np.random.RandomState(3).permutation(len(items))                    # every batch of 5 mixes the kinds: the indel items too keep their bits
    all_items = list(items.values())
    r3 = S.screen_1m(model, win, [all_items[i] for i in perm], batch=5, keep_maps=True, flank=flank, strands="both")
    pt = torch.from_numpy(perm).to(cuda)
    for name in FIELDS:
        assert torch.equal(getattr(r3, name), getattr(res, name)[pt]), name


def test_the_default_is_unchanged(case, cuda):
    c, fl, lp, ind, items, model, win, flank, res, st = case
    lst = list(items.values())
    st1, st2 = {}, {}
    today = S.screen_1m(model, win, lst, keep_maps=True, stats=st1, regions=REGIONS, flank=flank, aligned=True)
    plus = S.screen_1m(model, win, lst, keep_maps=True, stats=st2, regions=REGIONS, flank=flank, aligned=True, strands="+")
    for name in S.ScreenResult.__dataclass_fields__:
        a, b = getattr(today, name), getattr(plus, name)
        if isinstance(a, torch.Tensor):
            assert np.array_equal(a.cpu().numpy(), b.cpu().numpy(), equal_nan=True) and a.dtype == b.dtype, name
        elif name != "edits":
            assert a is None and b is None, name
    assert plus.strand_gap is None and plus.ref_strand_gap is None and st1 == st2 and st1["strands"] == "+"
    assert st1["reverse_two_part_items"] == 0 and st1["reverse_whole_items"] == 0
    assert not torch.equal(plus.maps, res.maps)                                # the model is not strand-symmetric: the merged maps are other maps
    with pytest.raises(ValueError, match="strands"):
        S.screen_1m(model, win, lst, strands="-")


def test_fallbacks_take_both_strands_through_the_whole_window_route(case, cuda):
    c, fl, lp, ind, items, model, win, flank, res, st = case
    pick = ["mask_start", "inv_n", "snvL1", "two", "del"]
    idx = torch.tensor([list(items).index(k) for k in pick], device=cuda)
    it = [items[k] for k in pick]
    scale = max(1.0, float(res.maps.abs().max()))
    st2 = {}
    with engine.force_safe_precision():
        safe = S.screen_1m(model, win, it, batch=3, keep_maps=True, stats=st2, flank=flank, strands="both")
    assert st2["route"] == "whole_window" and st2["whole_window_batches"] == 2 and st2["two_part_batches"] == 0
    assert st2["reverse_whole_items"] == len(pick) and st2["reverse_two_part_items"] == 0
    assert maxabs(safe.maps.cpu().numpy(), res.maps[idx].cpu().numpy()) / scale < TOL
    assert maxabs(safe.ref_map.cpu().numpy(), res.ref_map.cpu().numpy()) / scale < TOL
    assert maxabs(safe.strand_gap.cpu().numpy(), res.strand_gap[idx].cpu().numpy()) < 4 * TOL * scale
    other = M.H1esc_1M(synthetic_seed=0).to(cuda)
    other.net.precision = "bf16x3"
    st3 = {}
    r3 = S.screen_1m(other, win, it, keep_maps=True, stats=st3, flank=flank, strands="both")
    assert st3["route"] == "whole_window" and st3["reverse_whole_items"] == len(pick)
    assert maxabs(r3.maps.cpu().numpy(), res.maps[idx].cpu().numpy()) / scale < TOL


def test_range_fallback_when_the_fp16_check_fires_on_both_strands(case, cuda):
    """tests/test_gpu_screen.py's range-trip test with strands="both": Encoder weights x 2.0 trip the deferred check on the reference, every batch is
    redone whole, both strands, in the range-safe arithmetic, and the merged maps still equal model.net on both strands."""
    c, fl, lp, ind, items, model, win, flank, res, st = case
    net = pm.Net(num_1d=32)
    shapes = {k: tuple(v.shape) for k, v in net.state_dict().items()}
    hot = synth.synth_state_dict(shapes, seed=0, relu_gain=2.0)
    cold = synth.synth_state_dict(shapes, seed=0)
    enc_keys = {k for k in shapes if k.startswith(("lconv", "conv"))}
    net.load_state_dict({k: torch.from_numpy(np.asarray(hot[k] if k in enc_keys else cold[k])) for k in shapes}, strict=True)
    net = net.eval().to(cuda)
    pick = ["mask_mid", "snv1", "two"]
    it = [items[k] for k in pick]
    st2 = {}
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        r = S.screen_1m(net, win, it, keep_maps=True, stats=st2, strands="both")
        assert st2["range_fallback_reference"] and st2["range_fallback_batches"] == 1 and st2["two_part_batches"] == 0
        assert st2["reverse_whole_items"] == len(pick) and st2["reverse_two_part_items"] == 0
        wins = np.stack([c] + [S.apply_edit(c, v) for v in it])
        merged, heads, _, _ = _both_on_net(net, wins, cuda)
    scale = max(1.0, float(np.abs(merged).max()))
    assert maxabs(r.ref_map.cpu().numpy(), merged[0]) / scale < TOL and maxabs(r.maps.cpu().numpy(), merged[1:]) / scale < TOL
    assert maxabs(r.delta_1d.cpu().numpy() + r.ref_1d.cpu().numpy()[None], heads[1:]) < TOL
