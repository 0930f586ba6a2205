"""Compound edits (screen.EditSet) and region scores of the 1 Mb mutagenesis screen on the MI355X.  The window is 200 000 bases (50 bins, 500
stage-5 rows) with N runs, the model synthetic H1esc_1M(synthetic_seed=0): the multi-span and multi-segment kernels alone (exact), a
single-member set against the bare edit (bit for bit), the sets' maps against model.net on the edited windows, batch / order / member-order
invariance (bit for bit), the region scores against the fp64 host restatement, the whole-window routes, and the entry points' argument checks
(through return codes only: nothing malformed reaches a kernel)."""
import ctypes

import numpy as np
import pytest
import torch

from orca_amd import _lib, engine
from orca_amd import orca_models as M
from orca_amd import screen as S
from orca_amd._lib import OrcaHipError
from tests.test_gpu_screen import TOL, _net_on
from tests.test_screen_sets_cpu import plan_items, snv
from tests.util import maxabs

pytestmark = pytest.mark.gpu

L = 200_000
N5, NB = L // 400, L // 4000
NAMES = ("maps", "delta_profile", "delta_abs_mean", "delta_abs_max", "delta_1d", "delta_region", "delta_region_abs")
REGIONS = [(12, 17, 30, 35), (0, NB, 0, NB), (7, 8, 9, 10), (NB - 3, NB, NB - 6, NB), (0, 1, 0, NB)]


def _window():
    rs = np.random.RandomState(2025)
    c = rs.randint(0, 4, L).astype(np.uint8)
    for a, b in ((3_000, 3_400), (12_500, 12_620), (20_000, 20_040), (99_700, 100_300), (198_500, 198_900)):
        c[a:b] = 4
    return c


def _items(c):
    it = plan_items(L, c)
    it["snvs300"] = plan_items(L, c, n_snv=300, seed=9)["snvs"]
    return it


@pytest.fixture(scope="module")
def case(cuda):
    c = _window()
    items = _items(c)
    model = M.H1esc_1M(synthetic_seed=0).to(cuda)
    win = torch.from_numpy(c).to(cuda)
    st = {}
    res = S.screen_1m(model, win, list(items.values()), batch=64, keep_maps=True, stats=st, regions=REGIONS)
    return c, items, model, win, res, st


# ---- the kernels alone ----------------------------------------------------------------------------------------------------------------------------
def test_edit_codes_multi_equals_apply_edit(cuda):
    c = _window()
    items = list(_items(c).values())
    win = torch.from_numpy(c).to(cuda)
    ctx = engine.get_context(cuda)
    wins = [S.apply_edit(c, it) for it in items]
    for run_max in (S.RUN_MAX_BP, 20_000):                            # the packed-snippet form
        p = S.plan_batch(items, L, run_max=run_max)
        want = np.concatenate([wins[p.item_of[i]][p.snippet[i, 0]: p.snippet[i, 0] + p.snippet[i, 1]] for i in p.order])
        out = torch.full((want.size,), 9, dtype=torch.uint8, device=cuda)
        engine.screen_edit_codes_multi(ctx, win, p.snippet_table, p.span_table, torch.from_numpy(p.payload).to(cuda), out)
        assert np.array_equal(out.cpu().numpy(), want), run_max
    table, spans, payload = S.whole_window_set_tables(items, L)      # the whole-window form
    out = torch.full((len(items) * L,), 9, dtype=torch.uint8, device=cuda)
    engine.screen_edit_codes_multi(ctx, win, table, spans, torch.from_numpy(payload).to(cuda), out)
    assert np.array_equal(out.cpu().numpy().reshape(len(items), L), np.stack(wins))
    # no span at all (and no payload): the window's own bases
    out = torch.full((8_000,), 9, dtype=torch.uint8, device=cuda)
    engine.screen_edit_codes_multi(ctx, win, np.array([[0, 1_000, 8_000, 0, 0, 0, 0, 0]]), np.zeros((0, 4), np.int64), None, out)
    assert np.array_equal(out.cpu().numpy(), c[1_000:9_000])


@pytest.mark.parametrize("B,nseg", [(1, [0]), (1, [1]), (1, [7]), (5, [7, 0, 1, 2, 7]), (5, [0, 0, 0, 0, 0])])
def test_splice_rows_multi_equals_numpy(cuda, B, nseg):
    rs = np.random.RandomState(B + sum(nseg))
    n5, nfresh = 70, 90
    ref = rs.randn(n5, 128).astype(np.float32)
    fresh = rs.randn(nfresh, 128).astype(np.float32)
    segs, off, want = [], [0], np.repeat(ref[None], B, axis=0)
    for b in range(B):
        if nseg[b] == 7:                                                # rows 0 and n5 - 1 among them, two segments touching
            rows = [(0, 1), (3, 4), (7, 2), (9, 5), (20, 1), (40, 11), (n5 - 1, 1)]
        elif nseg[b] == 2:
            rows = [(0, n5 - 1), (n5 - 1, 1)]
        else:
            rows = [(n5 - 6, 6)][:nseg[b]]
        for r0, cnt in rows:
            src = int(rs.randint(0, nfresh - cnt + 1))
            segs.append((r0, cnt, src))
            want[b, r0: r0 + cnt] = fresh[src: src + cnt]
        off.append(len(segs))
    out = torch.full((B, n5, 128), np.nan, dtype=torch.float32, device=cuda)
    engine.screen_splice_rows_multi(engine.get_context(cuda), torch.from_numpy(ref).to(cuda), torch.from_numpy(fresh).to(cuda),
                                    np.array(segs, dtype=np.int64).reshape(-1, 3), np.array(off), out)
    assert np.array_equal(out.cpu().numpy(), want)


# ---- the screen -------------------------------------------------------------------------------------------------------------------------------------
def test_single_member_set_equals_bare_edit(case, cuda):
    c, items, model, win, res, st = case
    edits = [snv(c, 77_777), S.Edit("mask", 99_500, 700), S.Edit("inv", 150_000, 1_300)]
    a = S.screen_1m(model, win, edits, keep_maps=True, regions=REGIONS)
    b = S.screen_1m(model, win, [S.EditSet([e]) for e in edits], keep_maps=True, regions=REGIONS)
    for name in NAMES:
        assert torch.equal(getattr(a, name), getattr(b, name)), name
    assert torch.equal(a.ref_map, b.ref_map)


def test_sets_match_model_net_on_the_edited_windows(case, cuda):
    c, items, model, win, res, st = case
    assert st["route"] == "two_part" and st["two_part_batches"] == 1 and st["range_fallback_batches"] == 0 and st["whole_window_batches"] == 0
    assert st["edits"] == len(items) and st["set_items"] == sum(isinstance(v, S.EditSet) for v in items.values()) == len(items) - 2
    assert st["segments"] == sum(len(S.set_clusters(v, L)) for v in items.values()) > len(items)
    wins = np.stack([S.apply_edit(c, v) for v in items.values()])
    ref_map, ref_1d = _net_on(model.net, c[None], cuda)
    maps, heads = _net_on(model.net, wins, cuda)
    scale = max(1.0, float(np.abs(maps).max()))
    assert tuple(res.maps.shape) == (len(items), NB, NB)
    assert maxabs(res.ref_map.cpu().numpy(), ref_map[0]) / scale < TOL
    for k, name in enumerate(items):
        assert maxabs(res.maps[k].cpu().numpy(), maps[k]) / scale < TOL, name
        assert float(res.delta_abs_max[k]) > 0, name
    assert maxabs(res.delta_1d.cpu().numpy(), heads - res.ref_1d.cpu().numpy()[None]) < TOL
    st2 = {}
    r2 = S.screen_1m(model, win, [items["far_apart"]], keep_maps=True, stats=st2)
    assert st2["route"] == "two_part" and st2["segments"] == 2 and st2["set_items"] == 1
    assert torch.equal(r2.maps[0], res.maps[list(items).index("far_apart")])


def test_sets_are_invariant_to_batch_order_and_member_order(case, cuda):
    c, items, model, win, res, st = case
    lst = list(items.values())
    for b in (1, 7):
        r = S.screen_1m(model, win, lst, batch=b, keep_maps=True, regions=REGIONS)
        for name in NAMES:
            assert torch.equal(getattr(r, name), getattr(res, name)), (b, name)
    perm = np.random.RandomState(0).permutation(len(lst))
    pt = torch.from_numpy(perm).to(cuda)
    r = S.screen_1m(model, win, [lst[i] for i in perm], batch=64, keep_maps=True, regions=REGIONS)
    for name in NAMES:
        assert torch.equal(getattr(r, name), getattr(res, name)[pt]), name
    rev = [S.EditSet(list(v)[::-1]) if isinstance(v, S.EditSet) else v for v in lst]
    r = S.screen_1m(model, win, rev, batch=64, keep_maps=True, regions=REGIONS)
    for name in NAMES:
        assert torch.equal(getattr(r, name), getattr(res, name)), name


# ---- region scores ----------------------------------------------------------------------------------------------------------------------------------
def _check_regions(got_s, got_a, maps, ref, regions):
    """|got - want| <= 1e-6 |want| + 1e-12 mean|d|: the fp32 rounding of an fp64 sum, plus the sum's own rounding."""
    ws, wa = S.region_scores_host(maps, ref, regions)
    gs, ga = got_s.cpu().numpy().astype(np.float64), got_a.cpu().numpy().astype(np.float64)
    assert gs.shape == ws.shape and ga.shape == wa.shape
    for g, w in ((gs, ws), (ga, wa)):
        err, bound = np.abs(g - w), 1e-6 * np.abs(w) + 1e-12 * wa
        print("region scores: worst |got - want| / bound", float((err / np.maximum(bound, 1e-300)).max()))
        assert np.all(err <= bound), (float(err.max()), np.argwhere(err > bound)[:4].tolist())


def test_region_scores_against_the_host_function(case, cuda):
    c, items, model, win, res, st = case
    maps, ref = res.maps.cpu().numpy(), res.ref_map.cpu().numpy()
    assert tuple(res.delta_region.shape) == tuple(res.delta_region_abs.shape) == (len(items), len(REGIONS)) and res.delta_region.dtype == torch.float32
    _check_regions(res.delta_region, res.delta_region_abs, maps, ref, REGIONS)
    assert S.screen_1m(model, win, [items["one_row"]]).delta_region is None
    ctx = engine.get_context(cuda)
    one = [(NB - 1, NB, NB - 1, NB)]                                                       # K = 1: a 1 x 1 rectangle at the last row and column
    _check_regions(*engine.screen_region_scores(ctx, res.maps, res.ref_map, one), maps, ref, one)
    rs = np.random.RandomState(3)
    many = [(0, NB, 0, NB), (0, 1, 0, 1), (NB - 7, NB, NB - 2, NB)]
    while len(many) < 64:
        i0, j0 = rs.randint(0, NB, 2)
        many.append((int(i0), int(rs.randint(i0 + 1, NB + 1)), int(j0), int(rs.randint(j0 + 1, NB + 1))))
    sg, ab = engine.screen_region_scores(ctx, res.maps, res.ref_map, many)                 # K = 64
    _check_regions(sg, ab, maps, ref, many)
    r64 = S.screen_1m(model, win, list(items.values())[:3], regions=many)
    assert torch.equal(r64.delta_region, sg[:3]) and torch.equal(r64.delta_region_abs, ab[:3])
    # a NaN in one alt map: NaN in that map's rectangles that hold it, nowhere else
    bad = res.maps.clone()
    bad[2, 8, 3] = float("nan")
    sg2, ab2 = engine.screen_region_scores(ctx, bad, res.ref_map, many)
    holds = torch.tensor([i0 <= 8 < i1 and j0 <= 3 < j1 for i0, i1, j0, j1 in many], device=cuda)
    assert holds[0] and not holds.all()
    for got, clean in ((sg2, sg), (ab2, ab)):
        assert torch.equal(torch.isnan(got[2]), holds)
        keep = torch.ones_like(got, dtype=torch.bool)
        keep[2] = ~holds
        assert torch.equal(got[keep], clean[keep]) and not torch.isnan(got[keep]).any()
    with pytest.raises(ValueError):
        S.screen_1m(model, win, [items["one_row"]], regions=[(0, NB + 1, 0, 1)])
    with pytest.raises(ValueError):
        S.screen_1m(model, win, [items["one_row"]], regions=[(0, 1, 0, 1)] * 65)


# ---- fallbacks ----------------------------------------------------------------------------------------------------------------------------------------
def test_other_precision_takes_the_whole_window_route(case, cuda):
    c, items, model, win, res, st = case
    other = M.H1esc_1M(synthetic_seed=0).to(cuda)
    other.net.precision = "bf16x3"
    st2 = {}
    r = S.screen_1m(other, win, list(items.values()), batch=5, keep_maps=True, stats=st2, regions=REGIONS)
    assert st2["route"] == "whole_window" and st2["whole_window_batches"] == -(-len(items) // 5) and st2["two_part_batches"] == 0 and st2["segments"] == 0
    assert st2["set_items"] == st["set_items"]
    scale = max(1.0, float(res.maps.abs().max()))
    worst = float((r.maps - res.maps).abs().max()) / scale
    print("whole-window bf16x3 maps against two-part f16x2 maps, relative to the scale:", worst)
    assert worst < TOL
    assert float((r.delta_region - res.delta_region).abs().max()) / scale < TOL


def test_forced_safe_precision_takes_the_whole_window_route(case, cuda):
    c, items, model, win, res, st = case
    st2 = {}
    pick = ["far_apart", "bare_snv", "inv_next_to_sub"]
    with engine.force_safe_precision():
        r = S.screen_1m(model, win, [items[k] for k in pick], batch=2, keep_maps=True, stats=st2)
    assert st2["route"] == "whole_window" and st2["whole_window_batches"] == 2 and st2["two_part_batches"] == 0 and st2["range_fallback_batches"] == 0
    assert st2["segments"] == 0 and st2["set_items"] == 2 and not st2["range_fallback_reference"]
    scale = max(1.0, float(res.maps.abs().max()))
    idx = torch.tensor([list(items).index(k) for k in pick], device=cuda)
    assert float((r.maps - res.maps[idx]).abs().max()) / scale < TOL


# ---- argument checks: return codes only -----------------------------------------------------------------------------------------------------------------
def _i64(a):
    return np.ascontiguousarray(a, dtype=np.int64)


def _hp(a):
    return ctypes.c_void_p(a.ctypes.data)


def _dp(t):
    return ctypes.c_void_p(t.data_ptr())


def _refused(rc):
    msg = _lib.load().orca_last_error()
    assert rc != 0 and msg and len(msg) > 20, (rc, msg)
    return msg.decode()


def test_bad_arguments_are_refused_before_any_launch(cuda):
    """Every call below is refused by the host entry point's checks, so no table of these reaches a kernel; the output buffers keep their fill."""
    lib = _lib.load()
    h = engine.get_context(cuda).handle
    null = ctypes.c_void_p(0)
    win = torch.zeros(1_000, dtype=torch.uint8, device=cuda)
    out = torch.full((600,), 9, dtype=torch.uint8, device=cuda)
    dev = torch.zeros(64, dtype=torch.int64, device=cuda)                      # stands for every device table: never read
    good_t, good_s = _i64([[0, 0, 300, 0, 1, 0, 0, 0], [300, 100, 300, 1, 1, 0, 0, 0]]), _i64([[1, 10, 5, 0], [2, 200, 50, 0]])

    def edit(table=good_t, spans=good_s, window=_dp(win), o=_dp(out), ns=2, nspans=2, npay=0, total=600, tab_dev=_dp(dev), host=True):
        return lib.orca_screen_edit_codes_multi(h, window, 1_000, tab_dev, _hp(table) if host else null, ns, _dp(dev), _hp(spans), nspans, null, npay, o, total)
    assert "NULL" in _refused(edit(window=null)) and "NULL" in _refused(edit(o=null)) and "NULL" in _refused(edit(tab_dev=null)) and "NULL" in _refused(edit(host=False))
    _refused(edit(ns=-1))
    _refused(edit(nspans=-2))
    _refused(edit(npay=-1))
    _refused(edit(total=-600))
    assert "no gaps" in _refused(edit(table=_i64([[0, 0, 300, 0, 1, 0, 0, 0], [310, 100, 290, 1, 1, 0, 0, 0]])))       # a gap
    assert "no gaps" in _refused(edit(table=_i64([[300, 0, 300, 0, 1, 0, 0, 0], [0, 100, 300, 1, 1, 0, 0, 0]])))       # not ascending
    _refused(edit(total=601))                                                                                          # out is not what the snippets hold
    _refused(edit(table=_i64([[0, 800, 300, 0, 1, 0, 0, 0], [300, 100, 300, 1, 1, 0, 0, 0]])))                         # a snippet leaves the window
    _refused(edit(table=_i64([[0, 0, 300, 1, 2, 0, 0, 0], [300, 100, 300, 1, 1, 0, 0, 0]])))                           # a span range past the table
    _refused(edit(spans=_i64([[0, 10, 5, 0], [2, 200, 50, 0]])))                                                       # a payload that is not there
    _refused(edit(spans=_i64([[1, 990, 50, 0], [2, 200, 50, 0]])))                                                     # a span leaves the window
    _refused(edit(table=_i64([[0, 0, 600, 0, 2, 0, 0, 0]]), ns=1, spans=_i64([[1, 200, 50, 0], [1, 220, 5, 0]])))      # overlapping spans
    assert bool((out == 9).all())

    ref = torch.zeros((20, 128), dtype=torch.float32, device=cuda)
    fresh = torch.zeros((8, 128), dtype=torch.float32, device=cuda)
    rows = torch.full((2, 20, 128), 7.0, dtype=torch.float32, device=cuda)
    good_g, good_o = _i64([[0, 3, 0], [10, 4, 3], [19, 1, 7]]), _i64([0, 2, 3])

    def splice(seg=good_g, off=good_o, r=_dp(ref), o=_dp(rows), nseg=3, B=2, n5=20, nfresh=8, off_dev=_dp(dev)):
        return lib.orca_screen_splice_rows_multi(h, r, n5, _dp(fresh), nfresh, _dp(dev), _hp(seg), nseg, off_dev, _hp(off), B, o)
    assert "NULL" in _refused(splice(r=null)) and "NULL" in _refused(splice(o=null)) and "NULL" in _refused(splice(off_dev=null))
    _refused(splice(B=-1))
    _refused(splice(n5=-20))
    _refused(splice(nfresh=-8))
    _refused(splice(nseg=-3))
    assert "decrease" in _refused(splice(off=_i64([0, 4, 3])))                              # not monotone
    assert "offsets" in _refused(splice(off=_i64([0, 2, 2])))                               # the last entry is not the segment count
    assert "offsets" in _refused(splice(off=_i64([1, 2, 3])))
    _refused(splice(seg=_i64([[0, 3, 0], [10, 11, 3], [19, 1, 7]])))                        # a segment leaves the image
    _refused(splice(seg=_i64([[0, 3, 6], [10, 4, 3], [19, 1, 7]])))                         # ... or the fresh rows
    _refused(splice(seg=_i64([[10, 4, 3], [0, 3, 0], [19, 1, 7]])))                         # not sorted by row_lo
    assert bool((rows == 7).all())

    alt = torch.zeros((2, 10, 10), dtype=torch.float32, device=cuda)
    ref2 = torch.zeros((10, 10), dtype=torch.float32, device=cuda)
    sg = torch.full((2, 2), 5.0, dtype=torch.float32, device=cuda)
    ab = torch.full((2, 2), 5.0, dtype=torch.float32, device=cuda)

    def region(rects, a=_dp(alt), K=2, B=2, n=10, rd=_dp(dev)):
        r = np.ascontiguousarray(rects, dtype=np.int32)
        return lib.orca_screen_region_scores(h, a, 100, _dp(ref2), B, n, rd, _hp(r), K, _dp(sg), _dp(ab))
    ok = [(0, 10, 0, 10), (9, 10, 9, 10)]
    assert "NULL" in _refused(region(ok, a=null)) and "NULL" in _refused(region(ok, rd=null))
    _refused(region(ok, B=-2))
    _refused(region(ok, K=0))
    _refused(region(ok, K=-1))
    _refused(region([(0, 1, 0, 1)] * 65, K=65))
    for bad in ((0, 11, 0, 10), (0, 10, -1, 10), (5, 5, 0, 10), (0, 10, 7, 3), (10, 11, 0, 1)):
        assert "rectangle 1" in _refused(region([ok[0], bad]))
    assert bool((sg == 5).all()) and bool((ab == 5).all())
    # the wrappers turn the same refusals into OrcaHipError
    with pytest.raises(OrcaHipError):
        engine.screen_region_scores(engine.get_context(cuda), alt, ref2, [(0, 11, 0, 10)])
    with pytest.raises(OrcaHipError):
        engine.screen_splice_rows_multi(engine.get_context(cuda), ref, fresh, good_g, _i64([0, 3, 2]), rows)
