"""Loop (dot) calls along the scan's band on the MI355X (orca_scan_band_dot_enrichment, orca_scan_band_dot_offsets, orca_scan_band_dot_list;
scan.scan_1m(..., loops=)) against the numpy restatements `scan.band_dot_enrichment_host` / `scan.band_dot_calls_host`.

Exact inputs: bands quantised to multiples of 2^-12 with |x| < 8, the convention of tests/test_gpu_screen_loops.py - every fp64 sum of at most 33^2
such values is exact whatever its order, the one division per set and the one rounding to fp32 are correctly rounded on both sides, so kernel and
restatement agree bit for bit.  Unquantised bands: that file's bound, |got - want| <= RTOL |want| + 2 (2 w + 1)^2 2^-53 max|pixel|, RTOL imported
from it.  The dots are called from the DEVICE's enrichment band, so only fp32 comparisons separate kernel and restatement: the lists are equal
exactly, in order.  N runs over the seams of the enrichment kernel's tiles of R = engine.SCAN_LOOP_ROWS rows, D over the wave seams and the limit.

End to end: synthetic H1esc_1M(synthetic_seed=0) on a random chromosome of 654 321 bases with a run of N, 200 000-base windows every 60 000 bases,
trim 5: 163 bins, 9 windows, depth 26 - the shape of tests/test_gpu_scan.py, made here."""
import ctypes

import numpy as np
import pytest
import torch

from orca_amd import _lib, engine
from orca_amd import orca_models as M
from orca_amd import scan as C
from orca_amd import screen as S
from orca_amd._lib import OrcaHipError
from tests.test_gpu_screen_aligned import _dp, _refused
from tests.test_gpu_screen_loops import RTOL, close, same_f32
from tests.test_gpu_screen_tracks import same_bits

pytestmark = pytest.mark.gpu

NAN = np.float32(np.nan)
EINVAL = -1                                                                     # include/orca_hip.h: ORCA_EINVAL
R = engine.SCAN_LOOP_ROWS
PARAMS = [(0, 1), (1, 4), (15, 16)]
assert RTOL == 2.4e-7


def make_band(rs, N, D, quantised=True, ends=0):
    """a band of a stretch of N bins, NaN where i + d >= N and in ``ends`` rows at either end; multiples of 2^-12 with |x| < 8 if ``quantised``"""
    b = rs.randn(N, D)
    if quantised:
        b = np.clip(np.round(b * 4096.0), -32767, 32767) / 4096.0
    b = b.astype(np.float32)
    i, d = np.indices((N, D))
    b[i + d >= N] = NAN
    if ends:
        b[:ends] = b[-ends:] = NAN
    return b


def eligible(N, D, w, d_min):
    i, d = np.indices((N, D))
    return (i >= w) & (i + d <= N - 1 - w) & (d >= d_min) & (d <= D - 1 - 2 * w)


def enrich(ctx, band, p, w, d_min=None, cuda=None):
    dev = band if isinstance(band, torch.Tensor) else torch.from_numpy(band).to(cuda)
    return engine.scan_band_dot_enrichment(ctx, dev, p, w, d_min)


# ---- the enrichment band ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p,w", PARAMS)
@pytest.mark.parametrize("D", ["smallest", 27, 131, 256])
def test_enrichment_equals_the_host_restatement_bit_for_bit(cuda, D, p, w):
    ctx = engine.get_context(cuda)
    lib = _lib.load()
    d_min = 2 * w + 1
    need = d_min + 2 * w + 1
    D = need if D == "smallest" else D
    some = 0
    for N in (need, R - 1, R, R + 1, 2 * R + 1, 300):
        rs = np.random.RandomState(1000 * N + 10 * D + w)
        band = make_band(rs, N, D)
        q = S.LoopParams(p=p, w=w)
        want = C.band_dot_enrichment_host(band, q)
        dev = torch.from_numpy(band).to(cuda)
        out = torch.full((N + 1, D), 7.0, dtype=torch.float32, device=cuda)      # pre-filled: an unwritten element shows, and so does one too many
        assert lib.orca_scan_band_dot_enrichment(ctx.handle, _dp(dev), N, D, p, w, d_min, _dp(out)) == 0
        got = out.cpu().numpy()
        assert (got[N] == 7.0).all(), (N, D, p, w)
        assert same_f32(got[:N], want), (N, D, p, w)
        ok = eligible(N, D, w, d_min)
        assert np.array_equal(~np.isnan(want), ok), (N, D, p, w)                # no NaN but at the ineligible pixels
        some += int(ok.sum())
        if ok.any():                                                            # one NaN pixel: exactly the windows that hold it turn NaN
            ei, ed = np.argwhere(ok)[ok.sum() // 2]
            a, b = (0, 0) if N == need else (min(w, 1), -w)
            pi, pd = ei + a, ed + b - a
            bad = band.copy()
            bad[pi, pd] = NAN
            g2 = enrich(ctx, bad, p, w, None, cuda).cpu().numpy()
            i, d = np.indices((N, D))
            holds = ok & (np.abs(pi - i) <= w) & (np.abs(pd - d + (pi - i)) <= w)
            assert holds[ei, ed] and np.array_equal(np.isnan(g2), ~ok | holds), (N, D, p, w)
            assert np.array_equal(g2[ok & ~holds], got[:N][ok & ~holds]), (N, D, p, w)
            assert same_f32(g2, C.band_dot_enrichment_host(bad, q)), (N, D, p, w)
        if D >= d_min + 1 + 2 * w + 1:                                           # a larger d_min moves the first eligible distance
            g3 = enrich(ctx, dev, p, w, d_min + 1)
            assert same_f32(g3, C.band_dot_enrichment_host(band, S.LoopParams(p=p, w=w, d_min=d_min + 1))), (N, D, p, w)
    assert (some > 0) == (D >= need)
    if D == need:                                                               # the smallest band with an eligible pixel: exactly one, (w, d_min)
        e = enrich(ctx, make_band(np.random.RandomState(5), need, need), p, w, None, cuda)
        assert (~torch.isnan(e)).nonzero().tolist() == [[w, d_min]]


@pytest.mark.parametrize("p,w", PARAMS)
def test_enrichment_of_unquantised_bands_within_the_bound(cuda, p, w):
    ctx = engine.get_context(cuda)
    for N, D in ((2 * R + 13, 131), (300, 256), (150, 70)):
        rs = np.random.RandomState(N + D + w)
        band = make_band(rs, N, D, quantised=False, ends=3)
        band[N // 2, D // 2] = NAN
        got = enrich(ctx, band, p, w, None, cuda)
        want = C.band_dot_enrichment_host(band, S.LoopParams(p=p, w=w))
        assert got.dtype == torch.float32 and tuple(got.shape) == (N, D)
        close(got, want, w, float(np.nanmax(np.abs(band))), (N, D, p, w))
        assert np.isfinite(want).any() and np.isnan(want[eligible(N, D, w, 2 * w + 1)]).any()
        assert same_bits(enrich(ctx, band, p, w, None, cuda), got)               # the same bits on every run


@pytest.mark.parametrize("p,w", PARAMS)
def test_a_tiles_result_does_not_depend_on_where_it_starts(cuda, p, w):
    """Rows [a, b) of a band run alone - other tiles, another halo - against the same rows of the whole band, wherever both are eligible."""
    ctx = engine.get_context(cuda)
    N, D = 4 * R + 9, 131
    rs = np.random.RandomState(w)
    band = (rs.randn(N, D) * 10.0 ** rs.randint(-3, 4, size=(N, 1))).astype(np.float32)       # magnitudes that make the order of a sum matter
    i, d = np.indices((N, D))
    band[i + d >= N] = NAN
    dev = torch.from_numpy(band).to(cuda)
    whole = enrich(ctx, dev, p, w)
    seen = 0
    for a, b in ((13, 13 + 2 * R + 13), (R + 1, N), (0, 3 * R - 5), (R - 1, 2 * R + 2 * w + 12)):
        assert a % R or b % R
        part = enrich(ctx, dev[a:b].contiguous(), p, w)
        both = torch.from_numpy(eligible(b - a, D, w, 2 * w + 1) & eligible(N, D, w, 2 * w + 1)[a:b]).to(cuda)
        assert int(both.sum()) > 0, (a, b)
        assert not bool(torch.isnan(part[both]).any()) and same_bits(part[both], whole[a:b][both]), (a, b, p, w)
        seen += int(both.sum())
    assert seen > 100


# ---- the dots ------------------------------------------------------------------------------------------------------------------------------
def raw_calls(ctx, e_band, r, T, cap=None, extra=16):
    """the two entry points by hand, into pre-filled lists of ``cap`` + ``extra`` slots (cap: L by default): (L, row_start, ij, enrich)"""
    lib = _lib.load()
    N, D = e_band.shape
    row_start = torch.full((N + 2,), -7, dtype=torch.int64, device=e_band.device)
    assert lib.orca_scan_band_dot_offsets(ctx.handle, _dp(e_band), N, D, r, T, _dp(row_start)) == 0
    rs = row_start.cpu().numpy()
    L = int(rs[N])
    cap = L if cap is None else cap
    ij = torch.full((cap + extra, 2), -7, dtype=torch.int64, device=e_band.device)
    en = torch.full((cap + extra,), 7.0, dtype=torch.float32, device=e_band.device)
    assert lib.orca_scan_band_dot_list(ctx.handle, _dp(e_band), N, D, r, T, _dp(row_start), cap, _dp(ij), _dp(en)) == 0
    return L, rs, ij.cpu().numpy(), en.cpu().numpy()


def check_dots(ctx, e_band, r, T, what):
    e = e_band.cpu().numpy()
    N, D = e.shape
    want_ij, want_e = C.band_dot_calls_host(e, S.LoopParams(r=r, threshold=T))
    L, rs, ij, en = raw_calls(ctx, e_band, r, T)
    assert L == len(want_e), (what, L, len(want_e))
    assert rs[N + 1] == -7 and rs[0] == 0 and np.all(np.diff(rs[: N + 1]) >= 0), what
    assert np.array_equal(rs[: N + 1], np.searchsorted(want_ij[:, 0], np.arange(N + 1))), what      # row_start[i] = the dots in rows < i
    assert np.array_equal(ij[:L], want_ij) and np.array_equal(en[:L], want_e), what
    assert (ij[L:] == -7).all() and (en[L:] == 7.0).all(), what                 # nothing beyond L
    gi, ge = engine.scan_band_dot_calls(ctx, e_band, r, T)
    assert gi.dtype == torch.int64 and ge.dtype == torch.float32 and tuple(gi.shape) == (L, 2) and tuple(ge.shape) == (L,) and gi.device == e_band.device
    assert np.array_equal(gi.cpu().numpy(), want_ij) and np.array_equal(ge.cpu().numpy(), want_e), what
    return L


@pytest.mark.parametrize("r", [1, 2, 16])
@pytest.mark.parametrize("case", ["random", "ties", "long", "deep"])
def test_dot_lists_equal_the_host_restatement_exactly(cuda, case, r):
    ctx = engine.get_context(cuda)
    N, D, p, w, quantum = {"random": (300, 131, 1, 4, None), "ties": (2 * R + 1, 27, 0, 1, 0.125), "long": (4097, 27, 1, 4, None),
                           "deep": (300, 256, 1, 4, None)}[case]
    rs = np.random.RandomState(len(case) + r)
    band = make_band(rs, N, D, quantised=False, ends=2)
    if quantum:
        band = (np.round(band / quantum) * quantum).astype(np.float32)          # few distinct values: many equal enrichments, the tie rule decides
    band[N // 3, D // 2] = NAN
    e_band = enrich(ctx, band, p, w, None, cuda)
    e = e_band.cpu().numpy()
    vals = e[np.isfinite(e)]
    assert vals.size > 100
    if quantum:
        assert len(np.unique(vals)) < vals.size // 2
    counts = [check_dots(ctx, e_band, r, T, (case, r, T)) for T in (-1e30, 0.0, float(np.median(vals)))]
    assert counts[0] >= counts[1] >= 1 and counts[0] >= counts[2] >= 1
    if case == "deep":                                                          # dots at distances in each of the row's four waves
        at = C.band_dot_calls_host(e, S.LoopParams(r=r, threshold=-1e30))[0]
        assert len(np.unique((at[:, 1] - at[:, 0]) // 64)) == 4
    if case == "long":                                                          # dots in many row tiles and in many chunks of the prefix kernel
        rows = C.band_dot_calls_host(e, S.LoopParams(r=r, threshold=-1e30))[0][:, 0]
        assert len(np.unique(rows // R)) > 20 and len(np.unique(rows // -(-N // 256))) > 50
    assert check_dots(ctx, e_band, r, 1e30, (case, r, "none")) == 0             # an empty result
    gi, ge = engine.scan_band_dot_calls(ctx, e_band, r, 1e30)
    assert tuple(gi.shape) == (0, 2) and tuple(ge.shape) == (0,)


def test_a_constant_band_and_a_short_list(cuda):
    ctx = engine.get_context(cuda)
    N, D, p, w = 70, 40, 1, 4
    band = np.full((N, D), 1.5, dtype=np.float32)
    i, d = np.indices((N, D))
    band[i + d >= N] = NAN
    e_band = enrich(ctx, band, p, w, None, cuda)
    assert bool((e_band[torch.from_numpy(eligible(N, D, w, 9)).to(cuda)] == 0).all())
    gi, ge = engine.scan_band_dot_calls(ctx, e_band, 2, 0.0)
    assert gi.tolist() == [[w, w + 9]] and ge.tolist() == [0.0]                 # of equal neighbours exactly the first is a dot
    # a list shorter than the table says: only the slots below cap are written
    rs = np.random.RandomState(3)
    e_band = enrich(ctx, make_band(rs, 3 * R, 60), p, w, None, cuda)
    L, _, ij, en = raw_calls(ctx, e_band, 1, -1e30)
    assert L > 20
    L2, _, ij2, en2 = raw_calls(ctx, e_band, 1, -1e30, cap=L - 9, extra=32)
    assert L2 == L and np.array_equal(ij2[: L - 9], ij[: L - 9]) and np.array_equal(en2[: L - 9], en[: L - 9])
    assert (ij2[L - 9:] == -7).all() and (en2[L - 9:] == 7.0).all()


def test_malformed_calls_are_refused_before_any_launch(cuda):
    lib = _lib.load()
    h, null = engine.get_context(cuda).handle, ctypes.c_void_p(0)
    N, D = 40, 30
    band = torch.zeros((300, 300), dtype=torch.float32, device=cuda)             # room for every refused shape, had it been launched
    e_out = torch.full((300, 300), 7.0, dtype=torch.float32, device=cuda)
    rows = torch.full((400,), 7, dtype=torch.int64, device=cuda)
    ij = torch.full((400, 2), 7, dtype=torch.int64, device=cuda)
    en = torch.full((400,), 7.0, dtype=torch.float32, device=cuda)

    def enr(ctx=h, b=None, nt=N, nd=D, p=1, w=4, dm=9, out=None):
        return lib.orca_scan_band_dot_enrichment(ctx, _dp(band) if b is None else b, nt, nd, p, w, dm, _dp(e_out) if out is None else out)

    def off(ctx=h, e=None, nt=N, nd=D, r=2, T=0.0, out=None):
        return lib.orca_scan_band_dot_offsets(ctx, _dp(band) if e is None else e, nt, nd, r, T, _dp(rows) if out is None else out)

    def lst(ctx=h, e=None, nt=N, nd=D, r=2, T=0.0, rs=None, cap=10, i=None, o=None):
        return lib.orca_scan_band_dot_list(ctx, _dp(band) if e is None else e, nt, nd, r, T, _dp(rows) if rs is None else rs, cap, _dp(ij) if i is None else i,
                                           _dp(en) if o is None else o)

    for fn, kws in ((enr, (dict(ctx=null), dict(b=null), dict(out=null))), (off, (dict(ctx=null), dict(e=null), dict(out=null))),
                    (lst, (dict(ctx=null), dict(e=null), dict(rs=null), dict(i=null), dict(o=null)))):
        for kw in kws:
            rc = fn(**kw)
            assert rc == EINVAL and "NULL" in _refused(rc), (fn.__name__, kw)
    for fn in (enr, off, lst):
        for kw, word in ((dict(nd=1), "distances"), (dict(nd=257), "distances"), (dict(nd=0), "distances"), (dict(nt=0), "bins"), (dict(nt=-3), "bins"),
                         (dict(nt=(1 << 24) + 1), "bins")):
            rc = fn(**kw)
            assert rc == EINVAL and word in _refused(rc), (fn.__name__, kw)
    for kw, word in ((dict(p=4), "p = 4"), (dict(p=-1), "p = -1"), (dict(w=17, dm=35), "w = 17"), (dict(p=0, w=0, dm=1), "w = 0"), (dict(dm=8), "d_min = 8")):
        rc = enr(**kw)
        assert rc == EINVAL and word in _refused(rc), kw
    for fn in (off, lst):
        for kw, word in ((dict(r=0), "r = 0"), (dict(r=17), "r = 17"), (dict(T=float("nan")), "NaN")):
            rc = fn(**kw)
            assert rc == EINVAL and word in _refused(rc), (fn.__name__, kw)
    rc = lst(cap=-1)
    assert rc == EINVAL and "cap" in _refused(rc)
    torch.cuda.synchronize()
    assert all(bool((t == 7).all()) for t in (e_out, rows, ij, en))             # nothing was written
    assert enr() == 0 and enr(nd=2, p=0, w=1, dm=3) == 0 and enr(nd=256, nt=300) == 0 and off(e=_dp(e_out), T=1.0) == 0 and lst(e=_dp(e_out), cap=0) == 0      # the bounds themselves
    torch.cuda.synchronize()
    assert bool(torch.isnan(e_out[0, :2]).all()) and int(rows[N]) == 0 and bool((ij == 7).all()) and bool((en == 7.0).all())
    # the wrappers turn the same refusals into errors
    ctx = engine.get_context(cuda)
    good = torch.zeros((N, D), dtype=torch.float32, device=cuda)
    with pytest.raises(OrcaHipError, match="p = 4"):
        engine.scan_band_dot_enrichment(ctx, good, 4, 4)
    with pytest.raises(OrcaHipError, match="d_min = 8"):
        engine.scan_band_dot_enrichment(ctx, good, 1, 4, 8)
    with pytest.raises(OrcaHipError, match="distances"):
        engine.scan_band_dot_enrichment(ctx, good[:, :1].contiguous(), 0, 1)
    with pytest.raises(OrcaHipError, match="r = 0"):
        engine.scan_band_dot_calls(ctx, good, 0, 0.0)
    with pytest.raises(OrcaHipError, match="NaN"):
        engine.scan_band_dot_calls(ctx, good, 2, float("nan"))
    with pytest.raises(OrcaHipError):
        engine.scan_band_dot_enrichment(ctx, good.cpu(), 1, 4)
    with pytest.raises(ValueError):
        engine.scan_band_dot_calls(ctx, good[0], 2, 0.0)


# ---- end to end ----------------------------------------------------------------------------------------------------------------------------
CHR_BP, WINDOW_BP, STEP_BP, TRIM = 654_321, 200_000, 60_000, 5
EVERY = S.LoopParams(threshold=-1e30)                                           # every local maximum of the enrichment


@pytest.fixture(scope="module")
def case(cuda):
    rs = np.random.RandomState(2026)
    c = rs.randint(0, 4, CHR_BP).astype(np.uint8)
    c[301_000:301_700] = 4
    codes = torch.from_numpy(c).to(cuda)
    model = M.H1esc_1M(synthetic_seed=0).to(cuda)
    kw = dict(window_bp=WINDOW_BP, step_bp=STEP_BP, trim_bins=TRIM)
    st = {}
    res = C.scan_1m(model, codes, spread=True, insulation=(3, 10), boundaries=True, loops=EVERY, stats=st, **kw)
    return model, codes, kw, res, st


def test_scan_loops_equal_the_host_restatements(case, cuda):
    model, codes, kw, res, st = case
    assert (res.n_bins, res.depth) == (163, 26) and st["windows"] == 9
    q = res.loop_params
    assert q == S.LoopParams(1, 4, 2, float(np.float32(-1e30)), 9, 64, 1)
    band = res.band.cpu().numpy()
    assert res.loop_enrichment.dtype == torch.float32 and tuple(res.loop_enrichment.shape) == (163, 26) and res.loop_enrichment.device == res.band.device
    close(res.loop_enrichment, C.band_dot_enrichment_host(band, q), q.w, float(np.nanmax(np.abs(band))), "scan loop enrichment")
    e = res.loop_enrichment.cpu().numpy()
    i, d = np.indices((163, 26))
    assert np.array_equal(~np.isnan(e), (i >= TRIM + q.w) & (i + d <= 163 - 1 - TRIM - q.w) & (d >= 9) & (d <= 26 - 1 - 8))      # the trimmed ends are NaN in the band
    ij, enrich = res.loops
    want_ij, want_e = C.band_dot_calls_host(e, q)
    assert ij.dtype == np.int64 and enrich.dtype == np.float32
    assert np.array_equal(ij, want_ij) and np.array_equal(enrich, want_e)
    L = len(enrich)
    assert L >= 1 and st["loops"] == L
    pos = res.loop_positions()
    assert pos.dtype == np.int64 and pos.tolist() == [[res.pos_of(a), res.pos_of(b)] for a, b in ij]
    assert np.isfinite(res.band_range.cpu().numpy()[ij[:, 0], ij[:, 1] - ij[:, 0]]).all()          # how far the windows disagree at every dot


def test_scan_loops_change_nothing_else_and_do_not_depend_on_the_batch(case, cuda):
    model, codes, kw, res, st = case
    s0 = {}
    plain = C.scan_1m(model, codes, spread=True, insulation=(3, 10), boundaries=True, stats=s0, **kw)
    assert plain.loops is None and plain.loop_enrichment is None and plain.loop_params is None and "loops" not in s0
    for k in ("band", "coverage", "band_range", "insulation", "boundary_strength"):
        assert same_bits(getattr(plain, k), getattr(res, k)), k
    for a, b in zip(plain.boundaries, res.boundaries):
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    for batch in (2, 4):
        other = C.scan_1m(model, codes, batch=batch, loops=EVERY, **kw)
        assert same_bits(other.loop_enrichment, res.loop_enrichment), batch
        assert np.array_equal(other.loops[0], res.loops[0]) and np.array_equal(other.loops[1], res.loops[1]), batch
    s1 = {}
    one = C.scan_1m(model, codes, loops=S.LoopParams(threshold=-1e30, max_calls=1, tol=0), stats=s1, **kw)      # max_calls caps nothing here
    assert np.array_equal(one.loops[0], res.loops[0]) and np.array_equal(one.loops[1], res.loops[1]) and s1["loops"] == st["loops"]
    cut = float(np.median(res.loops[1]))
    fewer = C.scan_1m(model, codes, loops=S.LoopParams(threshold=cut), **kw)
    want = C.band_dot_calls_host(fewer.loop_enrichment.cpu().numpy(), fewer.loop_params)
    assert np.array_equal(fewer.loops[0], want[0]) and np.array_equal(fewer.loops[1], want[1]) and 1 <= len(want[1]) <= len(res.loops[1])
    with pytest.raises(ValueError, match="no eligible pixel"):
        C.scan_1m(model, codes, loops=True, depth=17, **kw)
