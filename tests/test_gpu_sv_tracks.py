"""Readouts per level of the SV screen on the MI355X (orca_screen_paired_insulation, orca_screen_paired_viewpoints,
orca_screen_paired_strata_scores; sv.sv_screen(..., scores=True, insulation=, viewpoints=, strata=), sv.sv_scores): the three kernels alone
against the numpy restatements `sv.paired_insulation_host`, `sv.paired_viewpoints_host`, `sv.paired_strata_host` on hand-made bin maps,
bit-for-bit invariance to the batch, bit-for-bit agreement with the unpaired kernels of the 1 Mb screen where both are defined, where a NaN
pixel shows, the entry points' argument checks (return codes only: nothing malformed reaches a kernel), and the screen end to end on the
first three variants of tests/test_gpu_sv_incremental.py - a deletion, a duplication and an inversion (synthetic H1esc(synthetic_seed=0)).

Tolerances are not new numbers: the arithmetic is that of the unpaired kernels, so the bounds are theirs, imported.  Insulation:
`close_ins` of tests/test_gpu_screen_tracks.py, |got - want| <= RTOL |want| + 2 w^2 2^-53 max|pixel|.  Viewpoints: the fp32 subtraction bit for
bit where at most one alt bin stands for the viewpoint (`same_f32`), else RTOL |want| + 2 c 2^-53 max|pixel| as asserted there.  Strata: `check`
of tests/test_gpu_screen_strata.py (its module docstring derives the bounds).  NaN sits in the same places on both sides; ``count`` and
``dist_count`` are exact."""
import ctypes

import numpy as np
import pytest
import torch

from orca_amd import _lib, engine, orca_models, sv
from orca_amd._lib import OrcaHipError
from tests import test_gpu_screen_strata as TS
from tests.test_gpu_screen_aligned import RTOL, _dp, _hp, _refused, kernel_maps
from tests.test_gpu_screen_tracks import _holding, close_ins, same_f32
from tests.test_gpu_sv_incremental import CHR, VARIANTS
from tests.test_gpu_sv_scores import FIELDS as OLD_FIELDS
from tests.test_gpu_sv_scores import all_maps, dict_maps, pairs, same_bits, scores_same_bits

pytestmark = pytest.mark.gpu

WIDTHS = [w for w in (1, 8, 9, 127, 128) if w <= 128]
STRATA = TS.PER_STRATUM + TS.PER_MAP
WORST = {}


def _np(t):
    return t.cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)


def views_of(n, B):
    """[B, 5]: -1, the first and the last bin, a bin two alt bins stand for under `duplicate` (0) or none does under `shift` (1), the middle -
    rotated from pair to pair, so that every pair has a list of its own"""
    base = np.array([-1, 0, n - 1, min(1, n - 1), n // 2], dtype=np.int32)
    return np.stack([np.roll(base, b) for b in range(B)])


def pix_of(*arrays):
    return max(float(np.nanmax(np.abs(_np(a)))) for a in arrays)


def check_viewpoints(got, count, alt, ref, views, bm, what):
    want, wc = sv.paired_viewpoints_host(alt, ref, views, bm)
    g = _np(got)
    assert _np(count).dtype == np.int32 and np.array_equal(_np(count), wc), (what, "count")
    assert g.dtype == np.float32 and g.shape == want.shape and np.array_equal(np.isnan(g), np.isnan(want)), (what, "NaN")
    pix = pix_of(alt, ref)
    for b in range(g.shape[0]):
        for k in range(g.shape[1]):
            c = int(wc[b, k])
            if c <= 1:
                assert same_f32(g[b, k], want[b, k]), (what, b, k, c)
            else:
                f = ~np.isnan(want[b, k])
                err = np.abs(g[b, k][f].astype(np.float64) - want[b, k][f].astype(np.float64))
                tol = RTOL * np.abs(want[b, k][f]) + 2.0 * c * 2.0 ** -53 * pix
                WORST["viewpoint_delta"] = max(WORST.get("viewpoint_delta", 0.0), float((err / tol).max()) if err.size else 0.0)
                assert np.all(err <= tol), (what, b, k, c)
            if c == 0:
                assert np.isnan(g[b, k]).all()


def check_insulation(got, alt, ref, widths, bm, what):
    want = sv.paired_insulation_host(alt, ref, widths, bm)
    pix = pix_of(alt, ref)
    for g, h, name in zip(got, want, ("insulation", "ref_insulation", "insulation_delta")):
        assert _np(g).dtype == np.float32
        close_ins(g, h, widths, pix, (what, name))
        f = ~np.isnan(h)
        for k, w in enumerate(widths):
            fk = f[..., k, :]
            err = np.abs(_np(g).astype(np.float64)[..., k, :][fk] - h[..., k, :][fk])
            tol = RTOL * np.abs(h[..., k, :][fk]) + 2.0 * w * w * 2.0 ** -53 * pix
            WORST[name] = max(WORST.get(name, 0.0), float((err / tol).max()) if err.size else 0.0)


def check_strata(got, alt, ref, bm, rng, what):
    """a dict of device tensors against `sv.paired_strata_host` with the bounds of tests/test_gpu_screen_strata.py"""
    n = bm.shape[1]
    want = sv.paired_strata_host(alt, ref, bm, rng)
    TS.check(got, want, pix_of(alt, ref), (0, n) if rng is None else rng, what)
    assert got["dist_count"].dtype == torch.int32 and np.array_equal(_np(got["dist_count"]), want["dist_count"])


# ---- the kernels against the restatements ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("n", [1, 2, 3, 63, 64, 65, 250, 256])
def test_kernels_equal_the_host_restatements(cuda, n, B):
    ctx = engine.get_context(cuda)
    maps = all_maps(n)
    names = list(maps)
    rs = np.random.RandomState(5000 * n + B)
    sub = (n // 3, max(n // 3 + 1, n - 2))
    for g0 in range(0, len(names), B):
        group = names[g0: g0 + B]
        G = len(group)
        bm = np.stack([maps[k] for k in group]).astype(np.int32)
        alt, ref = pairs(rs, G, n, cuda, near=(g0 // B) % 2 == 1)
        if G > 1:
            assert alt.stride(0) == n * n + 7 and ref.stride(0) == n * n + 3
        a, r = alt.cpu().numpy(), ref.cpu().numpy()
        got = engine.screen_paired_insulation(ctx, alt, ref, WIDTHS, bm)
        assert all(tuple(t.shape) == (G, len(WIDTHS), n) for t in got)
        check_insulation(got, a, r, WIDTHS, bm, (n, B, group))
        for k, w in enumerate(WIDTHS):
            assert int(torch.isfinite(got[0][0, k]).sum()) == int(torch.isfinite(got[1][0, k]).sum()) == max(0, n - 2 * w)
        if n == 3:
            assert torch.isfinite(got[0][0, 0]).nonzero().flatten().tolist() == [1]                # w = 1, n = 3: exactly one bin fits
        if n == 256:
            assert torch.isnan(got[0][:, WIDTHS.index(128)]).all() and torch.isnan(got[2][:, WIDTHS.index(128)]).all()
        views = views_of(n, G)
        va, count = engine.screen_paired_viewpoints(ctx, alt, ref, views, bm)
        assert tuple(va.shape) == (G, views.shape[1], n) and tuple(count.shape) == (G, views.shape[1])
        check_viewpoints(va, count, a, r, views, bm, (n, B, group))
        for rng in (None, sub):
            st = engine.screen_paired_strata_scores(ctx, alt, ref, bm, rng)
            assert tuple(st["dist_corr"].shape) == (G, n) and tuple(st["scc"].shape) == (G,)
            check_strata(st, a, r, bm, rng, (n, B, group, rng))
        for b, k in enumerate(group):
            if k == "none":
                assert torch.isnan(got[2][b]).all() and torch.isnan(va[b]).all() and not count[b].any() and not st["dist_count"][b].any()
            if k == "duplicate" and n > 2:
                assert 2 in count[b].tolist() and 0 in count[b].tolist()
            if k == "descending":
                full = engine.screen_paired_strata_scores(ctx, alt[b: b + 1], ref[b: b + 1], bm[b: b + 1])
                assert full["dist_count"][0].tolist() == [n - d for d in range(n)]


@pytest.mark.parametrize("n", [65, 250, 256])
def test_a_pairs_results_do_not_depend_on_the_batch(cuda, n):
    """A pair alone (contiguous) against the same pair as row 0, 1 and 2 of a batch of three - other batch strides, other pairs, bin maps and
    view lists beside it - under every bin map: the same bits."""
    ctx = engine.get_context(cuda)
    maps = all_maps(n)
    rs = np.random.RandomState(17 * n)
    alt1, ref1 = pairs(rs, 1, n, cuda)
    alt1, ref1 = alt1.contiguous(), ref1.contiguous()
    alt3, ref3 = pairs(rs, 3, n, cuda)
    v1 = views_of(n, 1)
    sub = (3, n - 5)

    def run(a, r, bm, views):
        st = engine.screen_paired_strata_scores(ctx, a, r, bm, sub)
        return engine.screen_paired_insulation(ctx, a, r, WIDTHS, bm) + engine.screen_paired_viewpoints(ctx, a, r, views, bm) + tuple(st[k] for k in STRATA + ("dist_count",))
    for name in maps:
        bm1 = maps[name].astype(np.int32)[None]
        alone = run(alt1, ref1, bm1, v1)
        for row in range(3):
            alt3[row], ref3[row] = alt1[0], ref1[0]                         # the rows written earlier stay, as other pairs
            bm3 = np.stack([maps["holes"], maps["shift"], maps["duplicate"]]).astype(np.int32)
            bm3[row] = bm1[0]
            v3 = views_of(n, 3)[::-1].copy()
            v3[row] = v1[0]
            for g, o in zip(run(alt3, ref3, bm3, v3), alone):
                assert same_bits(g[row], o[0]), (name, row)


@pytest.mark.parametrize("n", [65, 250])
def test_one_reference_replicated_gives_the_unpaired_kernels_bits(cuda, n):
    """B pairs that share ONE reference map (replicated, batch stride n * n + 3) against the 1 Mb screen's kernels on that reference: insulation
    and viewpoints under every map of `kernel_maps`, the strata under the same maps (all non-decreasing where mapped)."""
    ctx = engine.get_context(cuda)
    maps = kernel_maps(n)
    names = list(maps)
    B = len(names)
    bm = np.stack([maps[k] for k in names]).astype(np.int32)
    rs = np.random.RandomState(23 * n)
    alt, refs = pairs(rs, B, n, cuda)
    refs[:] = refs[0].clone()
    ref = refs[0].contiguous()
    assert refs.stride(0) == n * n + 3
    ws = [1, 8, 9, 25]
    track, ref_track, aligned = engine.screen_paired_insulation(ctx, alt, refs, ws, bm)
    t1, _, a1 = engine.screen_insulation(ctx, alt, ref, ws, bm)
    assert same_bits(track, t1) and same_bits(aligned, a1)
    rt, _, _ = engine.screen_insulation(ctx, ref[None], None, ws)
    assert all(same_bits(ref_track[b], rt[0]) for b in range(B))
    vs = [0, n - 1, 1, n // 2]
    va, count = engine.screen_paired_viewpoints(ctx, alt, refs, np.array(vs, dtype=np.int32), bm)
    _, v1 = engine.screen_viewpoints(ctx, alt, ref, vs, bm)
    assert same_bits(va, v1) and np.array_equal(_np(count), np.stack([[(bm[b] == v).sum() for v in vs] for b in range(B)]))
    for rng in (None, (2, n - 7)):
        st = engine.screen_paired_strata_scores(ctx, alt, refs, bm, rng)
        s1 = engine.screen_strata_scores(ctx, alt, ref, bm, rng)
        for k in STRATA:
            assert same_bits(st[k], s1[k]), (k, rng)
        assert torch.equal(st["dist_count"], s1["dist_count"])


# ---- where a NaN shows --------------------------------------------------------------------------------------------------------------------------------------
def test_nan_shows_in_the_diamonds_that_hold_it(cuda):
    """n = 50, widths 3 and 8, two pairs through a descending map with holes.  A NaN at alt (12, 20) of pair 1 is held by no diamond of width 3
    and by bins 13 .. 19 at width 8; one at the reference's (12, 14) is in the reference diamonds of bins `_holding`, and shows in ``aligned`` at
    the alt bins that stand for them.  Pair 0 and every other value keep their bits; nothing below the diagonal is read."""
    ctx = engine.get_context(cuda)
    n, ws = 50, [3, 8]
    m = np.arange(n, dtype=np.int32)[::-1].copy()
    m[[4, 17, 30]] = -1
    bm = np.stack([m, m])
    alt, ref = pairs(np.random.RandomState(2), 2, n, cuda)
    alt, ref = alt.contiguous(), ref.contiguous()
    clean = engine.screen_paired_insulation(ctx, alt, ref, ws, bm)
    low = torch.tril(torch.ones(n, n, dtype=torch.bool, device=cuda))
    a2, r2 = alt.clone(), ref.clone()
    a2[:, low] = float("nan")
    r2[:, low] = float("nan")
    for g, c in zip(engine.screen_paired_insulation(ctx, a2, r2, ws, bm), clean):
        assert same_bits(g, c)
    a3 = alt.clone()
    a3[1, 12, 20] = float("nan")
    got = engine.screen_paired_insulation(ctx, a3, ref, ws, bm)
    check_insulation(got, a3.cpu().numpy(), ref.cpu().numpy(), ws, bm, "alt NaN")
    assert same_bits(got[1], clean[1])
    for f in (0, 2):
        assert same_bits(got[f][0], clean[f][0])
        for k, w in enumerate(ws):
            hold = [i for i in _holding(n, w, 12, 20) if f == 0 or (m[i] >= w and m[i] < n - w)]
            new = np.flatnonzero(np.isnan(_np(got[f][1, k])) & ~np.isnan(_np(clean[f][1, k]))).tolist()
            assert new == hold, (f, w, new, hold)
            keep = np.setdiff1d(np.arange(n), hold)
            assert same_bits(got[f][1, k][keep], clean[f][1, k][keep])
    assert _holding(n, 3, 12, 20) == [] and _holding(n, 8, 12, 20) == list(range(13, 20))
    r3 = ref.clone()
    r3[1, 12, 14] = float("nan")
    got = engine.screen_paired_insulation(ctx, alt, r3, ws, bm)
    check_insulation(got, alt.cpu().numpy(), r3.cpu().numpy(), ws, bm, "ref NaN")
    assert same_bits(got[0], clean[0]) and same_bits(got[1][0], clean[1][0]) and same_bits(got[2][0], clean[2][0])
    for k, w in enumerate(ws):
        hold = _holding(n, w, 12, 14)
        assert hold and np.flatnonzero(np.isnan(_np(got[1][1, k])) & ~np.isnan(_np(clean[1][1, k]))).tolist() == hold
        new = np.flatnonzero(np.isnan(_np(got[2][1, k])) & ~np.isnan(_np(clean[2][1, k]))).tolist()
        assert new == [i for i in range(n) if w <= i < n - w and m[i] in hold], (w, new)


@pytest.mark.parametrize("rng", [(0, 50), (0, 8), (9, 50), (8, 9)])
def test_nan_shows_in_its_stratum_only(cuda, rng):
    """n = 50, a descending bin map with three unmapped bins (an inversion: every reference pair is mirrored).  A NaN below the diagonal of
    either map and one at an unmapped pair change no bit; one at alt (12, 20) of pair 1, or at the reference pixel that pair stands for -
    (min, max) of (49 - 12, 49 - 20) = (29, 37) - makes stratum 8 of pair 1 NaN and its per-map scores exactly when 8 is inside the range."""
    ctx = engine.get_context(cuda)
    n = 50
    m = np.arange(n, dtype=np.int32)[::-1].copy()
    m[[4, 17, 30]] = -1
    bm = np.stack([m, m])
    alt, ref = pairs(np.random.RandomState(19), 2, n, cuda)
    alt, ref = alt.contiguous(), ref.contiguous()
    clean = engine.screen_paired_strata_scores(ctx, alt, ref, bm, rng)
    low = torch.tril(torch.ones(n, n, dtype=torch.bool, device=cuda), -1)
    a2, r2 = alt.clone(), ref.clone()
    a2[:, low] = float("nan")                                               # below the diagonal of both maps
    r2[:, low] = float("nan")
    a2[0, 4, 45] = float("nan")                                             # unmapped pairs: alt row 4, alt column 30, the reference bins behind no alt bin
    a2[1, 12, 30] = float("nan")
    r2[0, 19, 32:] = float("nan")                                           # reference bin 49 - 30 = 19
    r2[1, :32, 32] = float("nan")                                           # reference bin 49 - 17 = 32
    quiet = engine.screen_paired_strata_scores(ctx, a2, r2, bm, rng)
    for f in STRATA:
        assert same_bits(quiet[f], clean[f]), f
    assert torch.equal(quiet["dist_count"], clean["dist_count"])
    for where in ("alt", "ref"):
        a3, r3 = alt.clone(), ref.clone()
        if where == "alt":
            a3[1, 12, 20] = float("nan")
        else:
            r3[1, 29, 37] = float("nan")
        got = engine.screen_paired_strata_scores(ctx, a3, r3, bm, rng)
        want = TS.nan_sets(clean)
        for f in TS.PER_STRATUM:
            want[f] = sorted(want[f] + [[1, 8]])
        if rng[0] <= 8 < rng[1]:
            for f in TS.PER_MAP:
                want[f] = sorted(want[f] + [[1]])
        assert TS.nan_sets(got) == want == TS.nan_sets(sv.paired_strata_host(a3.cpu().numpy(), r3.cpu().numpy(), bm, rng)), (where, rng)
        for f in STRATA:                                                    # every other value keeps its bits
            keep = ~np.isnan(_np(got[f]))
            assert np.array_equal(_np(got[f])[keep], _np(clean[f])[keep]), f


def test_viewpoints_read_their_rows_and_mapped_columns_only(cuda):
    ctx = engine.get_context(cuda)
    n = 50
    i = np.arange(n)
    shift = np.where(i + 3 < n, i + 3, -1).astype(np.int32)                 # reference 20 sits at alt 17, reference 5 at alt 2; alt columns 47 .. 49 unmapped
    bm = np.stack([shift, shift])
    views = np.array([[20, 5, -1], [-1, 20, 2]], dtype=np.int32)           # reference 2: behind no alt bin
    alt, ref = pairs(np.random.RandomState(6), 2, n, cuda)
    alt, ref = alt.contiguous(), ref.contiguous()
    clean, count = engine.screen_paired_viewpoints(ctx, alt, ref, views, bm)
    assert count.tolist() == [[1, 1, 0], [0, 1, 0]] and torch.isnan(clean[0, 2]).all() and torch.isnan(clean[1, 0]).all() and torch.isnan(clean[1, 2]).all()
    a2, r2 = alt.clone(), ref.clone()
    rows = torch.ones(n, dtype=torch.bool, device=cuda)
    rows[[17, 2]] = False
    a2[0][rows] = float("nan")                                              # rows that stand for no viewpoint of pair 0
    a2[0, 17, 47:] = float("nan")                                           # a row that does, at unmapped columns
    a2[1, 2] = float("nan")                                                 # pair 1 has no viewpoint behind alt row 2
    rrows = torch.ones(n, dtype=torch.bool, device=cuda)
    rrows[[20, 5]] = False
    r2[0][rrows] = float("nan")
    r2[1, 2] = float("nan")                                                 # the reference row of a viewpoint nothing stands for
    quiet, _ = engine.screen_paired_viewpoints(ctx, a2, r2, views, bm)
    assert same_bits(quiet, clean)
    a3 = alt.clone()
    a3[0, 17, 30] = float("nan")
    got, _ = engine.screen_paired_viewpoints(ctx, a3, ref, views, bm)
    assert np.flatnonzero(np.isnan(_np(got[0, 0]))).tolist() == [30, 47, 48, 49] and same_bits(got[0, 1], clean[0, 1]) and same_bits(got[1], clean[1])


# ---- argument checks: return codes only -----------------------------------------------------------------------------------------------------------------
def test_bad_arguments_are_refused_before_any_launch(cuda):
    """Every call below is refused by the host entry points' checks, so nothing of it reaches a kernel; the output buffers keep their fill."""
    lib = _lib.load()
    h = engine.get_context(cuda).handle
    null = ctypes.c_void_p(0)
    n, B, W, V = 6, 2, 2, 3
    alt = torch.zeros((B, n, n), dtype=torch.float32, device=cuda)
    ref = torch.zeros((B, n, n), dtype=torch.float32, device=cuda)
    dev = torch.zeros(B * 257, dtype=torch.int32, device=cuda)                  # stands for every device table: never read
    o32 = [torch.full((B * 9 * 257,), 7.0, dtype=torch.float32, device=cuda) for _ in range(4)]
    o64 = [torch.full((B * 257,), 7.0, dtype=torch.float64, device=cuda) for _ in range(3)]
    cnt = torch.full((B * 257,), 7, dtype=torch.int32, device=cuda)
    good = np.ascontiguousarray([[0, 1, -1, 2, 3, 5], [5, 4, 3, -1, 1, 1]], dtype=np.int32)
    big = np.zeros((B, 257), dtype=np.int32)
    widths = np.array([1, 2], dtype=np.int32)
    views = np.array([[0, -1, 5], [5, 5, 2]], dtype=np.int32)

    def ins(bm=good, w=widths, nw=W, nb=B, nn=n, abs_=n * n, rbs=n * n, host=True, whost=True, **p):
        q = dict(a=_dp(alt), r=_dp(ref), wd=_dp(dev), md=_dp(dev), o0=_dp(o32[0]), o1=_dp(o32[1]), o2=_dp(o32[2]))
        q.update(p)
        return lib.orca_screen_paired_insulation(h, q["a"], abs_, q["r"], rbs, nb, nn, q["wd"], _hp(w) if whost else null, nw, q["md"], _hp(bm) if host else null,
                                                 q["o0"], q["o1"], q["o2"])

    def vws(bm=good, v=views, nv=V, nb=B, nn=n, abs_=n * n, rbs=n * n, host=True, vhost=True, **p):
        q = dict(a=_dp(alt), r=_dp(ref), vd=_dp(dev), md=_dp(dev), o0=_dp(o32[0]), ct=_dp(cnt))
        q.update(p)
        return lib.orca_screen_paired_viewpoints(h, q["a"], abs_, q["r"], rbs, nb, nn, q["vd"], _hp(v) if vhost else null, nv, q["md"], _hp(bm) if host else null,
                                                 q["o0"], q["ct"])

    def stra(bm=good, lo=0, hi=n, nb=B, nn=n, abs_=n * n, rbs=n * n, host=True, **p):
        q = dict(a=_dp(alt), r=_dp(ref), md=_dp(dev), o0=_dp(o32[0]), o1=_dp(o32[1]), o2=_dp(o32[2]), c0=_dp(o64[0]), ct=_dp(cnt), o3=_dp(o32[3]), c1=_dp(o64[1]),
                 c2=_dp(o64[2]))
        q.update(p)
        return lib.orca_screen_paired_strata_scores(h, q["a"], abs_, q["r"], rbs, nb, nn, q["md"], _hp(bm) if host else null, lo, hi, q["o0"], q["o1"], q["o2"],
                                                    q["c0"], q["ct"], q["o3"], q["c1"], q["c2"])
    dev.zero_()
    assert ins() == 0 and vws() == 0 and stra() == 0                            # the well-formed calls are accepted (and overwrite the fill: refilled below)
    torch.cuda.synchronize()
    for o in o32 + o64:
        o.fill_(7.0)
    cnt.fill_(7)
    for call in (ins, vws, stra):
        _refused(call(nn=0))
        _refused(call(nn=257, abs_=257 * 257, rbs=257 * 257, bm=big))
        _refused(call(nb=0))
        _refused(call(nb=-1))
        assert ">= n * n" in _refused(call(abs_=n * n - 1))                    # a stride below n^2, either map
        assert ">= n * n" in _refused(call(rbs=n * n - 1))
        bad = good.copy()
        bad[1, 4] = n
        assert "outside -1" in _refused(call(bm=bad))                           # a bin-map entry of n
        bad[1, 4] = -2
        assert "outside -1" in _refused(call(bm=bad))
        assert "NULL" in _refused(call(host=False))                             # a NULL host table
        for k in ("a", "r", "md", "o0"):
            assert "NULL" in _refused(call(**{k: null})), k
    for w in (0, 129, -1):
        assert "outside 1" in _refused(ins(w=np.array([1, w], dtype=np.int32)))
    _refused(ins(nw=9, w=np.ones(9, dtype=np.int32)))
    _refused(ins(nw=0))
    assert "NULL" in _refused(ins(whost=False)) and "NULL" in _refused(ins(wd=null)) and "NULL" in _refused(ins(o1=null)) and "NULL" in _refused(ins(o2=null))
    for x in (-2, n):
        bad_v = views.copy()
        bad_v[1, 2] = x
        assert "outside -1" in _refused(vws(v=bad_v))
    _refused(vws(nv=65, v=np.zeros((B, 65), dtype=np.int32)))
    _refused(vws(nv=0))
    assert "NULL" in _refused(vws(vhost=False)) and "NULL" in _refused(vws(vd=null)) and "NULL" in _refused(vws(ct=null))
    for lo, hi in ((3, 3), (4, 3), (-1, 3), (0, n + 1)):
        assert "d_lo" in _refused(stra(lo=lo, hi=hi))
    for k in ("o1", "o2", "o3", "c0", "c1", "c2", "ct"):
        assert "NULL" in _refused(stra(**{k: null})), k
    torch.cuda.synchronize()
    assert all(bool((o == 7).all()) for o in o32 + o64 + [cnt])
    # the wrappers turn the same refusals into errors
    ctx = engine.get_context(cuda)
    with pytest.raises(OrcaHipError):
        engine.screen_paired_insulation(ctx, alt, ref, [0], good)
    with pytest.raises(OrcaHipError):
        engine.screen_paired_viewpoints(ctx, alt, ref, [n], good)
    with pytest.raises(OrcaHipError):
        engine.screen_paired_strata_scores(ctx, alt, ref, good, (2, 2))
    with pytest.raises(ValueError):
        engine.screen_paired_strata_scores(ctx, alt, ref[:1], good)
    with pytest.raises(ValueError):
        engine.screen_paired_viewpoints(ctx, alt, ref, np.zeros((3, 2), dtype=np.int32), good)
    with pytest.raises(ValueError):
        engine.screen_paired_insulation(ctx, alt, ref, [1], good[:1])


# ---- the screen ---------------------------------------------------------------------------------------------------------------------------------------
THREE = VARIANTS[:3]                                                        # a deletion, a duplication, an inversion
KW = dict(insulation=(5, 10), viewpoints=[21_250_000, 30_000_000], strata=(2, 250))       # inside the duplication; outside every 1 Mb window
TOP_KEYS = ["bin_map", "count", "dist_count", "insulation_widths", "junction_bins", "models", "strata_range", "viewpoint_bins", "viewpoint_count"]
NEW_FIELDS = ("insulation", "ref_insulation", "insulation_delta", "viewpoint_delta", "dist_delta", "dist_abs", "dist_rms", "dist_corr", "mse", "strata_corr", "scc")


@pytest.fixture(scope="module")
def case(cuda):
    g = torch.Generator(device=cuda).manual_seed(11)
    genome = torch.randint(0, 4, (CHR,), device=cuda, generator=g, dtype=torch.uint8)
    genome[7_000_000:7_003_000] = 4                                     # an N run inside the windows
    model = orca_models.H1esc(synthetic_seed=0)
    tracked = sv.sv_screen([model], genome, THREE, CHR, min_uses=1, scores=True, **KW)
    return model, genome, tracked


def tracks_same_bits(x, y):
    return (scores_same_bits(x, y) and sorted(x) == sorted(y) and all(np.array_equal(x[k], y[k]) for k in TOP_KEYS if k != "models")
            and all(sorted(a) == sorted(b) and all(same_bits(a[k], b[k]) for k in NEW_FIELDS) for a, b in zip(x["models"], y["models"])))


def equals_host(entry, what):
    """an entry's readouts against the restatements on the entry's own maps"""
    s = entry["scores"]
    assert sorted(s) == TOP_KEYS
    bm = sv.level_bin_maps(entry["sv"], CHR, entry["ref"], entry["alt"])
    vb = sv.viewpoint_bins(KW["viewpoints"], entry["ref"])
    assert np.array_equal(s["bin_map"], bm) and s["insulation_widths"].tolist() == [5, 10] and s["strata_range"] == (2, 250)
    assert s["viewpoint_bins"].dtype == np.int32 and np.array_equal(s["viewpoint_bins"], vb) and vb[5, 1] == -1 and (vb[0] >= 0).all()
    for m, got in enumerate(s["models"]):
        assert sorted(got) == sorted(OLD_FIELDS + NEW_FIELDS)
        alt, ref = dict_maps(entry["alt"], m), dict_maps(entry["ref"], m)
        C = alt.shape[1]
        a, r, bmc = alt.reshape(6 * C, 250, 250), ref.reshape(6 * C, 250, 250), np.repeat(bm, C, axis=0)
        assert all(got[k].shape == (6, C, 2, 250) and got[k].dtype == np.float32 for k in ("insulation", "ref_insulation", "insulation_delta", "viewpoint_delta"))
        check_insulation([got[k].reshape(6 * C, 2, 250) for k in ("insulation", "ref_insulation", "insulation_delta")], a, r, [5, 10], bmc, (what, m))
        wc = sv.paired_viewpoints_host(a, r, np.repeat(vb, C, axis=0), bmc)[1]
        assert s["viewpoint_count"].dtype == np.int32 and np.array_equal(np.repeat(s["viewpoint_count"], C, axis=0), wc)
        check_viewpoints(got["viewpoint_delta"].reshape(6 * C, 2, 250), wc, a, r, np.repeat(vb, C, axis=0), bmc, (what, m))
        flat = {k: torch.from_numpy(np.ascontiguousarray(got["strata_corr" if k == "corr" else k]).reshape((6 * C, 250) if k.startswith("dist_") else (6 * C,)))
                for k in STRATA}
        flat["dist_count"] = torch.from_numpy(np.repeat(s["dist_count"], C, axis=0))
        assert s["dist_count"].dtype == np.int32 and s["dist_count"].shape == (6, 250)
        check_strata(flat, a, r, bmc, (2, 250), (what, m))


def test_screen_readouts_equal_the_host_restatements(case):
    """Printed, not asserted (the weights are synthetic): the insulation change at the junctions and 1 - scc per level."""
    model, genome, tracked = case
    for i, v in enumerate(THREE):
        e = tracked[i]
        assert sorted(e) == ["alt", "ref", "scores", "sv"] and e["sv"] == v
        equals_host(e, v)
        s = e["scores"]
        jb = s["junction_bins"][:, 0]
        print(v, "viewpoint_count", s["viewpoint_count"].tolist(), "insulation_delta at the first junction (w = 5)",
              [f"{s['models'][0]['insulation_delta'][k, 0, 0, jb[k]]:.4f}" if jb[k] >= 0 else None for k in range(6)],
              "1 - scc", [f"{1 - x:.3e}" for x in s["models"][0]["scc"][:, 0]])
    dup, inv = tracked[1]["scores"], tracked[2]["scores"]
    assert 2 in dup["viewpoint_count"][:, 0].tolist()                       # the position inside the duplication: two alt bins stand for it somewhere
    assert all(tracked[i]["scores"]["viewpoint_count"][5, 1] == 0 and tracked[i]["scores"]["viewpoint_count"][0, 1] == 1 for i in range(3))
    assert any((np.diff(inv["bin_map"][k][inv["bin_map"][k] >= 0]) < 0).any() for k in range(6))          # the inversion's maps do descend
    assert (tracked[0]["scores"]["dist_count"][5] == 0).all()               # the deletion's finest level: nothing in common


def test_readouts_change_nothing_else_and_maps_can_stay_on_the_device(case):
    model, genome, tracked = case
    plain = sv.sv_screen([model], genome, THREE, CHR, min_uses=1, scores=True)
    bare = sv.sv_screen([model], genome, THREE, CHR, min_uses=1, scores=True, keep_maps=False, **KW)
    for i in range(3):
        assert sorted(plain[i]["scores"]) == ["bin_map", "count", "junction_bins", "models"] and sorted(plain[i]["scores"]["models"][0]) == sorted(OLD_FIELDS)
        assert scores_same_bits(plain[i]["scores"], tracked[i]["scores"]), i
        for allele in ("ref", "alt"):
            assert bare[i][allele]["predictions"] is None
            for j in range(6):
                assert np.array_equal(plain[i][allele]["predictions"][0][j], tracked[i][allele]["predictions"][0][j]), (i, allele, j)
        assert tracks_same_bits(bare[i]["scores"], tracked[i]["scores"]), i
    only = sv.sv_screen([model], genome, THREE[:1], CHR, min_uses=1, scores=True, keep_maps=False, insulation=5)
    assert sorted(only[0]["scores"]) == ["bin_map", "count", "insulation_widths", "junction_bins", "models"]
    assert same_bits(only[0]["scores"]["models"][0]["insulation_delta"][:, :, 0], tracked[0]["scores"]["models"][0]["insulation_delta"][:, :, 0])
    with pytest.raises(ValueError):
        sv.sv_screen([model], genome, THREE[:1], CHR, insulation=(5,))


def test_sv_scores_of_two_genomepredict_calls(case, cuda):
    model, genome, tracked = case
    full = sv.sv_screen([model], genome, THREE, CHR, incremental=False, scores=True, **KW)
    for i, v in enumerate(THREE):
        equals_host(full[i], ("full", v))
        again = sv.sv_scores(v, full[i]["ref"], full[i]["alt"], CHR, cuda, **KW)
        assert tracks_same_bits(again, full[i]["scores"])
        for k in ("viewpoint_bins", "viewpoint_count", "dist_count"):
            assert np.array_equal(full[i]["scores"][k], tracked[i]["scores"][k]), k


def test_an_allele_equal_to_the_reference_gives_zero_deltas(case, cuda):
    model, genome, tracked = case
    ref = tracked[1]["ref"]
    none = sv.SV("del", 20_000_000, 20_000_000)
    s = sv.sv_scores(none, ref, ref, CHR, cuda, **KW)
    got = s["models"][0]
    assert np.array_equal(s["dist_count"], np.tile(250 - np.arange(250, dtype=np.int32), (6, 1)))
    assert np.array_equal(s["viewpoint_count"], (s["viewpoint_bins"] >= 0).astype(np.int32))
    assert same_bits(got["insulation"], got["ref_insulation"])
    for k in ("insulation_delta", "viewpoint_delta", "dist_delta", "dist_abs", "dist_rms"):
        f = ~np.isnan(got[k])
        assert f.any() and (got[k][f] == 0).all(), k
    assert np.array_equal(np.isnan(got["insulation_delta"]), np.isnan(got["insulation"]))
    assert np.array_equal(np.isnan(got["viewpoint_delta"]).all(axis=-1)[:, 0], s["viewpoint_bins"] < 0)
    assert (got["mse"] == 0).all() and (got["scc"] == 1.0).all() and (got["strata_corr"] == 1.0).all()


def test_print_the_worst_error_over_tolerance():
    print("largest error / tolerance per field over this file's comparisons:", {k: f"{v:.3g}" for k, v in dict(WORST, **TS.WORST).items()})
