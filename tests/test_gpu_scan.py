"""The chromosome scan on the MI355X (orca_scan_*; scan.scan_1m).

The kernels alone, on random data uploaded directly.  Stitch + finish: n at the wave seams and at the limit, D at the wave seams and at n - 2 trim,
trim 0 / 1 / the largest, 1 and 5 windows with a batch stride above n * n, offsets regular, irregular with a gap wider than a window (holes) and
ending exactly at N - n, one window with N = n: ``count`` equal as integers, ``band`` and ``range`` equal `scan.stitch_band_host` BIT FOR BIT (both
sides add the same fp64 terms in the same order and round once), whatever the split into launches; a NaN pixel shows in exactly one band pixel and the
lower triangle is never read.  Band insulation against `scan.band_insulation_host` within the project's insulation tolerance
(tests/test_gpu_screen_tracks.py: RTOL |want| + 2 w^2 2^-53 max|pixel|), NaN in the same places, the same bits on every run, and against
orca_screen_insulation on one window.  Boundary strengths against `screen.boundary_strength_host` EXACTLY for tracks of 1 to 4097 bins, and against
orca_screen_boundary_calls' strength track bit for bit up to its 256 bins.  Every malformed call is refused before any launch.

End to end: synthetic H1esc_1M(synthetic_seed=0) on a random chromosome of 654 321 bases with a run of N, 200 000-base windows every 60 000 bases,
trim 5: 163 bins, 9 windows (the last clamped to bin 113), depth 26."""
import ctypes

import numpy as np
import pytest
import torch

from orca_amd import _lib, engine
from orca_amd import orca_models as M
from orca_amd import scan as C
from orca_amd import screen as S
from orca_amd._lib import OrcaHipError
from tests.test_gpu_screen_aligned import RTOL, _dp, _hp, _refused
from tests.test_gpu_screen_boundaries import KINDS, make_track
from tests.test_gpu_screen_tracks import close_ins, same_bits, same_f32

pytestmark = pytest.mark.gpu

NAN = np.float32(np.nan)
EINVAL = -1                                                                     # include/orca_hip.h: ORCA_EINVAL


def upload_maps(m, cuda):
    """[B, n, n] float32 numpy on the device with a batch stride of n * n + 7"""
    B, n = m.shape[0], m.shape[1]
    buf = torch.zeros((B, n * n + 7), dtype=torch.float32, device=cuda)
    buf[:, : n * n] = torch.from_numpy(m.reshape(B, n * n)).to(cuda)
    return buf.as_strided((B, n, n), (n * n + 7, n, 1))


def stitch(ctx, maps, off, trim, N, D, splits=None, spread=True):
    """maps through orca_scan_stitch_band in the launches ``splits`` (lists of window indices, one launch by default), then orca_scan_band_finish"""
    acc = engine.scan_accumulators(maps.device, N, D)
    off = np.asarray(off, dtype=np.int64)
    for idx in splits or [list(range(len(off)))]:
        engine.scan_stitch_band(ctx, maps[idx[0]: idx[-1] + 1], off[idx[0]: idx[-1] + 1], trim, acc)
    band, rng = engine.scan_band_finish(ctx, acc, spread)
    return band, acc["count"], rng


def offsets_of(n, trim, B):
    """(name, offsets, N): regular and ending exactly at N - n; irregular with a gap wider than a window and rows behind the last one"""
    if B == 1:
        return [("one window", [0], n), ("one window inside", [2], n + 5)]
    s = max(1, (n - 2 * trim) // 2)
    reg = [k * s for k in range(B)]
    irr = [0, 1, 3, 2 * n + 4, 2 * n + 5]
    return [("regular", reg, reg[-1] + n), ("irregular", irr, irr[-1] + n + 2)]


@pytest.mark.parametrize("B", [1, 5])
@pytest.mark.parametrize("n", [3, 50, 64, 65, 256])
def test_stitch_and_finish_equal_the_host_restatement_bit_for_bit(cuda, n, B):
    ctx = engine.get_context(cuda)
    rs = np.random.RandomState(10 * n + B)
    m = rs.randn(B, n, n).astype(np.float32)
    dev = upload_maps(m, cuda)
    assert dev.stride(0) == n * n + 7
    seen = 0
    for trim in sorted({0, 1, (n - 1) // 2}):
        for D in sorted({d for d in (1, 63, 64, 65, n - 2 * trim) if 1 <= d <= n - 2 * trim}):
            for name, off, N in offsets_of(n, trim, B):
                what = (n, B, trim, D, name)
                band, count, rng = stitch(ctx, dev, off, trim, N, D)
                hb, hc, hr = C.stitch_band_host(m, off, trim, N, D)
                assert count.dtype == torch.int32 and np.array_equal(count.cpu().numpy(), hc), what
                assert same_f32(band, hb), what
                assert same_f32(rng, hr), what
                g = band.cpu().numpy()
                assert np.array_equal(np.isnan(g), hc == 0), what                # NaN exactly where no window covers the pixel
                i, d = np.indices((N, D))
                assert np.isnan(g[i + d >= N]).all(), what
                assert bool((rng[count == 1] == 0).all()), what
                if name == "irregular":                                          # the gap: rows no window reaches
                    assert (hc[n + 3: 2 * n + 4] == 0).all() and (hc[-2:] == 0).all(), what
                if name == "regular":
                    assert hc[N - 1 - trim, 0] >= 1 and (trim == 0 or hc[N - trim, 0] == 0), what
                none, c2, r2 = stitch(ctx, dev, off, trim, N, D, spread=False)  # range is optional: the same band
                assert r2 is None and same_bits(none, band) and same_bits(c2, count), what
                seen += 1
    assert seen >= 4


def test_the_split_into_launches_changes_no_bit(cuda):
    ctx = engine.get_context(cuda)
    n, trim, D = 65, 2, 40
    off, N = [0, 7, 20, 21, 50], 120
    rs = np.random.RandomState(7)
    m = (rs.randn(5, n, n) * 10.0 ** rs.randint(-3, 4, size=(5, 1, 1))).astype(np.float32)        # magnitudes that make the order of a sum matter
    dev = upload_maps(m, cuda)
    one = stitch(ctx, dev, off, trim, N, D)
    assert int(one[1].max()) >= 4
    for splits in ([[0, 1], [2, 3, 4]], [[0], [1], [2], [3], [4]], [[0, 1, 2, 3], [4]]):
        got = stitch(ctx, dev, off, trim, N, D, splits)
        for a, b, k in zip(got, one, ("band", "count", "range")):
            assert same_bits(a, b), (splits, k)
    want = C.stitch_band_host(m, off, trim, N, D)
    assert same_f32(one[0], want[0]) and np.array_equal(one[1].cpu().numpy(), want[1]) and same_f32(one[2], want[2])


def test_nan_pixels_and_the_lower_triangle(cuda):
    ctx = engine.get_context(cuda)
    n, trim, D = 50, 3, 20
    off, N = [0, 10, 30], 85
    rs = np.random.RandomState(11)
    m = rs.randn(3, n, n).astype(np.float32)
    base = stitch(ctx, upload_maps(m, cuda), off, trim, N, D)
    low = m.copy()
    r, c = np.tril_indices(n, -1)
    low[:, r, c] = NAN
    got = stitch(ctx, upload_maps(low, cuda), off, trim, N, D)
    for a, b in zip(got, base):
        assert same_bits(a, b)                                                   # the lower triangle is never read
    out = m.copy()
    out[:, :trim] = out[:, :, -trim:] = NAN                                      # nor the trimmed rows and columns
    out[:, np.triu_indices(n, D)[0], np.triu_indices(n, D)[1]] = NAN             # nor a distance beyond the band
    got = stitch(ctx, upload_maps(out, cuda), off, trim, N, D)
    for a, b in zip(got, base):
        assert same_bits(a, b)
    for b, r, c in ((1, 12, 15), (0, trim, trim + D - 1), (2, n - 1 - trim, n - 1 - trim)):
        bad = m.copy()
        bad[b, r, c] = NAN
        band, count, rng = stitch(ctx, upload_maps(bad, cuda), off, trim, N, D)
        hb, hc, hr = C.stitch_band_host(bad, off, trim, N, D)
        assert same_f32(band, hb) and same_f32(rng, hr) and same_bits(count, base[1])
        hit = torch.isnan(band) & ~torch.isnan(base[0])
        assert hit.nonzero().tolist() == [[off[b] + r, c - r]]                   # one band pixel, however many windows cover it
        assert torch.equal(torch.isnan(rng) & ~torch.isnan(base[2]), hit)
    assert int(base[1][10 + 12, 3]) == 2                                         # the first of them lies under two windows


def test_malformed_stitch_calls_are_refused_before_any_launch(cuda):
    lib = _lib.load()
    h = engine.get_context(cuda).handle
    null = ctypes.c_void_p(0)
    n, B, N, D, trim = 8, 3, 30, 4, 1
    maps = torch.zeros((B, 300 * 300), dtype=torch.float32, device=cuda)         # room for every refused shape, had it been launched
    acc = {"sum": torch.full((400 * 300,), 7.0, dtype=torch.float64, device=cuda), "count": torch.full((400 * 300,), 7, dtype=torch.int32, device=cuda),
           "lo": torch.full((400 * 300,), 7.0, dtype=torch.float32, device=cuda), "hi": torch.full((400 * 300,), 7.0, dtype=torch.float32, device=cuda)}
    out = [torch.full((400 * 300,), 7.0, dtype=torch.float32, device=cuda) for _ in range(2)]
    off_dev = torch.zeros(8, dtype=torch.int64, device=cuda)                     # stands for the device table: never read

    def call(ctx=h, mp=None, bs=300 * 300, nb=B, nn=n, off=(0, 5, 22), od=None, oh=None, tr=trim, nt=N, nd=D, **ptr):
        o = np.asarray(off, dtype=np.int64)
        p = lambda k: ptr.get(k, _dp(acc[k]))
        return lib.orca_scan_stitch_band(ctx, _dp(maps) if mp is None else mp, bs, nb, nn, _dp(off_dev) if od is None else od, _hp(o) if oh is None else oh, tr,
                                         nt, nd, p("sum"), p("count"), p("lo"), p("hi"))

    def untouched():
        torch.cuda.synchronize()
        return all(bool((t == 7).all()) for t in list(acc.values()) + out)

    bad = [(dict(off=(0, 5, 5)), "ascending"), (dict(off=(5, 0, 22)), "ascending"), (dict(off=(0, 5, 23)), "N - n"), (dict(off=(-1, 5, 22)), "N - n"),
           (dict(nd=7), "D = "), (dict(nd=0), "D = "), (dict(nn=257, nt=400, bs=300 * 300), "bins"), (dict(nn=0), "bins"), (dict(nb=0), "maps"),
           (dict(nb=-2), "maps"), (dict(tr=-1), "trim"), (dict(tr=4), "trim"), (dict(bs=63), "stride"), (dict(nt=7), "stretch")]
    for kw, word in bad:
        rc = call(**kw)
        assert rc == EINVAL and word in _refused(rc), kw
    for kw in (dict(ctx=null), dict(mp=null), dict(od=null), dict(oh=null), dict(sum=null), dict(count=null), dict(lo=null), dict(hi=null)):
        rc = call(**kw)
        assert rc == EINVAL and "NULL" in _refused(rc), kw
    fin = lambda nt=N, nd=D, **ptr: lib.orca_scan_band_finish(ptr.get("ctx", h), ptr.get("sum", _dp(acc["sum"])), _dp(acc["count"]), _dp(acc["lo"]), _dp(acc["hi"]),
                                                               nt, nd, ptr.get("band", _dp(out[0])), _dp(out[1]))
    for kw in (dict(nt=0), dict(nd=0), dict(nd=257), dict(band=null), dict(sum=null), dict(ctx=null)):
        assert fin(**kw) == EINVAL, kw
    assert untouched()
    assert call() == 0 and call(nd=n - 2 * trim) == 0 and call(off=(0, 5, N - n)) == 0 and call(nn=256, nt=300, off=(0, 5, 44), tr=127, nd=2) == 0      # the bounds themselves
    torch.cuda.synchronize()
    assert not untouched()
    # the wrappers turn the same refusals into errors
    ctx = engine.get_context(cuda)
    good = torch.zeros((2, n, n), dtype=torch.float32, device=cuda)
    fresh = engine.scan_accumulators(cuda, N, D)
    with pytest.raises(OrcaHipError, match="ascending"):
        engine.scan_stitch_band(ctx, good, [4, 4], trim, fresh)
    with pytest.raises(OrcaHipError, match="N - n"):
        engine.scan_stitch_band(ctx, good, [4, N - n + 1], trim, fresh)
    with pytest.raises(OrcaHipError, match="D = "):
        engine.scan_stitch_band(ctx, good, [0, 4], 3, fresh)
    with pytest.raises(OrcaHipError):
        engine.scan_stitch_band(ctx, good.cpu(), [0, 4], trim, fresh)
    with pytest.raises(ValueError):
        engine.scan_stitch_band(ctx, good, [0, 4, 8], trim, fresh)
    with pytest.raises(ValueError):
        engine.scan_stitch_band(ctx, good, [0, 4], trim, dict(fresh, count=fresh["count"].long()))
    torch.cuda.synchronize()
    assert int(fresh["count"].sum()) == 0 and float(fresh["sum"].abs().sum()) == 0.0


# ---- band insulation -----------------------------------------------------------------------------------------------------------------------
def widths_of(D):
    top = (D - 1) // 2
    return sorted({w for w in (1, 2, 3, top // 2, 25, top - 1, top) if 1 <= w <= top})


def make_band(rs, N, D):
    """a random band of a stretch of N bins: NaN where i + d >= N, and holes"""
    b = rs.randn(N, D).astype(np.float32)
    i, d = np.indices((N, D))
    b[i + d >= N] = NAN
    for _ in range(max(1, N // 20)):
        b[rs.randint(0, N), rs.randint(0, D)] = NAN
    if N >= 64:
        b[40:43] = NAN                                                           # rows no window reached
    return b


@pytest.mark.parametrize("D", [3, 27, 131])
@pytest.mark.parametrize("N", [3, 64, 65, 300])
def test_band_insulation_equals_the_host_restatement(cuda, N, D):
    ctx = engine.get_context(cuda)
    band = make_band(np.random.RandomState(1000 * N + D), N, D)
    ws = widths_of(D)
    assert 1 <= len(ws) <= 8 and ws[0] == 1 and ws[-1] == (D - 1) // 2
    dev = torch.from_numpy(band).to(cuda)
    got = engine.scan_band_insulation(ctx, dev, ws)
    want = C.band_insulation_host(band, ws)
    assert tuple(got.shape) == (len(ws), N) and got.dtype == torch.float32
    close_ins(got, want, ws, float(np.nanmax(np.abs(band))), (N, D))
    if N >= 64:
        assert np.isfinite(want[0]).any() and np.isnan(want[0, 1: N - 1]).any()  # the holes take some diamonds and leave others standing
    assert same_bits(engine.scan_band_insulation(ctx, dev, ws), got)             # the same bits on every run
    for k, w in enumerate(ws):                                                   # a width's track does not depend on the others
        assert same_bits(engine.scan_band_insulation(ctx, dev, [w])[0], got[k]), w
    for bad in ([(D - 1) // 2 + 1], [0], [1, 1], list(range(1, 10))):
        with pytest.raises(OrcaHipError, match="width"):
            engine.scan_band_insulation(ctx, dev, bad)


def test_band_insulation_of_one_window_is_the_screens_insulation(cuda):
    ctx = engine.get_context(cuda)
    n = 50
    ws = [1, 3, 10, 24]
    m = np.random.RandomState(3).randn(1, n, n).astype(np.float32)
    dev = upload_maps(m, cuda)
    band, count, _ = stitch(ctx, dev, [0], 0, n, n)
    assert int(count.min()) == 0 and int(count.max()) == 1 and same_f32(band[:, 0], np.diag(m[0]).copy())
    got = engine.scan_band_insulation(ctx, band, ws)
    ref = engine.screen_insulation(ctx, dev, None, ws)[0][0]
    close_ins(got, ref.double().cpu().numpy(), ws, float(np.abs(m).max()), "one window")
    close_ins(got, S.insulation_host(m, ws)[0], ws, float(np.abs(m).max()), "one window, host")
    lib, h, null = _lib.load(), ctx.handle, ctypes.c_void_p(0)
    out = torch.full((4 * n,), 7.0, dtype=torch.float32, device=cuda)
    w = np.array(ws, dtype=np.int32)
    wd = torch.from_numpy(w).to(cuda)
    for args in ((h, _dp(band), n, n, _dp(wd), _hp(np.array([1, 3, 10, 25], dtype=np.int32)), 4, _dp(out)), (h, null, n, n, _dp(wd), _hp(w), 4, _dp(out)),
                 (h, _dp(band), n, n, null, _hp(w), 4, _dp(out)), (h, _dp(band), n, n, _dp(wd), null, 4, _dp(out)), (h, _dp(band), n, n, _dp(wd), _hp(w), 4, null),
                 (h, _dp(band), 0, n, _dp(wd), _hp(w), 4, _dp(out)), (h, _dp(band), n, 257, _dp(wd), _hp(w), 4, _dp(out)),
                 (h, _dp(band), n, n, _dp(wd), _hp(w), 0, _dp(out)), (null, _dp(band), n, n, _dp(wd), _hp(w), 4, _dp(out))):
        rc = lib.orca_scan_band_insulation(*args)
        assert rc == EINVAL and _refused(rc)
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())


# ---- boundary strength ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W", [1, 8])
@pytest.mark.parametrize("N", [1, 2, 3, 63, 64, 65, 255, 256, 257, 1000, 4097])
def test_boundary_strength_equals_the_host_restatement_exactly(cuda, N, W):
    ctx = engine.get_context(cuda)
    rs = np.random.RandomState(100 * N + W)
    t = np.stack([make_track(rs, N, KINDS[(w + N + W) % len(KINDS)]) for w in range(W)])
    if N == 3:
        t[0] = [2.0, 1.0, 3.0]                                                   # the one minimum a track of 3 bins can have
    dev = torch.from_numpy(t).to(cuda)
    got = engine.scan_boundary_strength(ctx, dev)
    want = np.stack([S.boundary_strength_host(x) for x in t])
    assert tuple(got.shape) == (W, N) and same_f32(got, want), (N, W)
    if N == 3:
        assert got[0].tolist()[1] == 1.0
    if W == 8 and N >= 63:
        assert np.isfinite(want).any() and np.isnan(want).any()
    if 3 <= N <= 256:
        calls = engine.screen_boundary_calls(ctx, dev[None], 0.0, 1)["strength_track"][0]
        assert same_bits(got, calls), (N, W)
    assert same_bits(engine.scan_boundary_strength(ctx, dev), got)


def test_malformed_boundary_strength_calls_are_refused(cuda):
    lib = _lib.load()
    h, null = engine.get_context(cuda).handle, ctypes.c_void_p(0)
    t = torch.zeros(64, dtype=torch.float32, device=cuda)
    out = torch.full((64,), 7.0, dtype=torch.float32, device=cuda)
    for args in ((null, _dp(t), 2, 32, _dp(out)), (h, null, 2, 32, _dp(out)), (h, _dp(t), 2, 32, null), (h, _dp(t), 0, 32, _dp(out)), (h, _dp(t), 2, 0, _dp(out)),
                 (h, _dp(t), 65536, 1, _dp(out))):
        rc = lib.orca_scan_boundary_strength(*args)
        assert rc == EINVAL and _refused(rc)
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())
    with pytest.raises(OrcaHipError):
        engine.scan_boundary_strength(engine.get_context(cuda), t.cpu().view(2, 32))
    with pytest.raises(ValueError):
        engine.scan_boundary_strength(engine.get_context(cuda), t)


# ---- end to end ----------------------------------------------------------------------------------------------------------------------------
CHR_BP, WINDOW_BP, STEP_BP, TRIM = 654_321, 200_000, 60_000, 5
WIDTHS = (3, 10)


@pytest.fixture(scope="module")
def case(cuda):
    rs = np.random.RandomState(2026)
    c = rs.randint(0, 4, CHR_BP).astype(np.uint8)
    c[301_000:301_700] = 4
    codes = torch.from_numpy(c).to(cuda)
    model = M.H1esc_1M(synthetic_seed=0).to(cuda)
    net = S._net_of(model)
    off = C.plan_windows(CHR_BP // 4000, WINDOW_BP // 4000, STEP_BP // 4000, TRIM)
    plus, minus = [], []
    with torch.no_grad():
        for a in off:                                                            # one window at a time: a map does not depend on its batch
            w = codes[int(a) * 4000: int(a) * 4000 + WINDOW_BP][None]
            plus.append(net._dec(net._enc.forward_codes(w))[0, 0].cpu().numpy())
            minus.append(net._dec(net._enc.forward_codes(w, reverse=True))[0, 0].cpu().numpy())
    kw = dict(window_bp=WINDOW_BP, step_bp=STEP_BP, trim_bins=TRIM)
    st = {}
    res = C.scan_1m(model, codes, spread=True, insulation=WIDTHS, boundaries=S.BoundaryParams(min_strength=0.0), stats=st, **kw)
    return model, codes, off, np.stack(plus), np.stack(minus), kw, res, st


def test_scan_equals_the_host_stitch_of_the_windows_maps(case, cuda):
    model, codes, off, plus, minus, kw, res, st = case
    assert off.tolist() == [0, 15, 30, 45, 60, 75, 90, 105, 113] and np.array_equal(res.offsets, off)
    assert (res.n_bins, res.depth, res.start, res.binsize) == (163, 26, 0, 4000) and C.full_depth(50, 15, 5) == 26
    assert st["windows"] == 9 and st["decoded_windows"] == 9 and st["batches"] == 1 and st["strands"] == "+"
    band, count, rng = C.stitch_band_host(plus, off, TRIM, 163, 26)
    assert np.isfinite(plus).all()
    assert same_f32(res.band, band) and same_f32(res.band_range, rng)
    assert res.coverage.dtype == torch.int32 and np.array_equal(res.coverage.cpu().numpy(), count)
    i, d = np.indices((163, 26))
    inside = (i >= TRIM) & (i + d <= 163 - 1 - TRIM)
    assert (count[inside] >= 1).all() and (count[~inside] == 0).all() and count.max() >= 3        # no holes but the trimmed ends
    assert float(np.nanmax(rng)) > 0
    for batch in (2, 4):
        s2 = {}
        other = C.scan_1m(model, codes, batch=batch, spread=True, stats=s2, **kw)
        assert s2["batches"] == -(-9 // batch) and s2["decoded_windows"] == 9
        assert same_bits(other.band, res.band) and same_bits(other.coverage, res.coverage) and same_bits(other.band_range, res.band_range), batch
        assert other.insulation is None and other.boundary_strength is None and other.boundaries is None
    plain = C.scan_1m(model, codes, **kw)
    assert plain.band_range is None and same_bits(plain.band, res.band)
    sub = C.scan_1m(model, codes, start=60_000, end=60_000 + 263_999, depth=7, **kw)              # a stretch: bins 15 .. 80, the tail dropped
    assert (sub.n_bins, sub.depth, sub.start) == (65, 7, 60_000) and sub.offsets.tolist() == [0, 15]
    hb = C.stitch_band_host(plus[[1, 2]], [0, 15], TRIM, 65, 7)[0]
    assert same_f32(sub.band, hb)
    assert sub.bin_of(60_000) == 0 and sub.pos_of(65) == 320_000
    dense = res.dense(20, 60)
    assert dense.shape == (40, 40) and np.array_equal(dense, dense.T, equal_nan=True)
    assert same_f32(dense[0, :26], band[20]) and np.isnan(dense[0, 26:]).all()


def test_scan_tracks_and_boundaries_equal_the_host_restatements(case, cuda):
    model, codes, off, plus, minus, kw, res, st = case
    band = res.band.cpu().numpy()
    assert res.insulation_widths.tolist() == list(WIDTHS) and tuple(res.insulation.shape) == (2, 163)
    close_ins(res.insulation, C.band_insulation_host(band, WIDTHS), WIDTHS, float(np.nanmax(np.abs(band))), "scan insulation")
    tracks = res.insulation.cpu().numpy()
    for k, w in enumerate(WIDTHS):
        assert np.flatnonzero(~np.isnan(tracks[k])).tolist() == list(range(TRIM + w, 163 - TRIM - w))
    want = np.stack([S.boundary_strength_host(t) for t in tracks])
    assert same_f32(res.boundary_strength, want)
    assert len(res.boundaries) == 2 and res.boundary_params.min_strength == 0.0
    for k in range(2):
        bins, strength = res.boundaries[k]
        at = np.flatnonzero(~np.isnan(want[k]))
        assert bins.dtype == np.int64 and strength.dtype == np.float32 and at.size >= 1
        assert np.array_equal(bins, at) and np.array_equal(strength, want[k][at])
    cut = float(np.nanmedian(want))
    res2 = C.scan_1m(model, codes, insulation=WIDTHS, boundaries=S.BoundaryParams(min_strength=cut, max_calls=1), **kw)
    assert same_bits(res2.boundary_strength, res.boundary_strength)
    for k in range(2):
        with np.errstate(invalid="ignore"):
            at = np.flatnonzero(want[k] >= np.float32(cut))
        assert np.array_equal(res2.boundaries[k][0], at) and np.array_equal(res2.boundaries[k][1], want[k][at])        # max_calls caps nothing
    assert sum(len(b[0]) for b in res2.boundaries) < sum(len(b[0]) for b in res.boundaries)


def test_scan_on_both_strands(case, cuda):
    model, codes, off, plus, minus, kw, res, st = case
    s2 = {}
    both = C.scan_1m(model, codes, strands="both", spread=True, stats=s2, batch=4, **kw)
    assert s2["decoded_windows"] == 18 and s2["windows"] == 9 and s2["strands"] == "both"
    merged = S.merge_strands_host(plus, minus)[0]
    band, count, rng = C.stitch_band_host(merged, off, TRIM, 163, 26)
    g = both.band.cpu().numpy().astype(np.float64)
    assert np.array_equal(np.isnan(g), np.isnan(band)) and np.array_equal(both.coverage.cpu().numpy(), count)
    f = ~np.isnan(band)
    assert np.all(np.abs(g[f] - band[f].astype(np.float64)) <= RTOL * np.abs(band[f].astype(np.float64)))
    assert not same_bits(both.band, res.band)


def test_scan_refuses_what_it_cannot_run(case, cuda):
    model, codes, off, plus, minus, kw, res, st = case
    with pytest.raises(OrcaHipError, match="no CPU path"):
        C.scan_1m(model, codes.cpu(), **kw)
    with pytest.raises(ValueError, match="holds no window"):
        C.scan_1m(model, codes, end=199_999, **kw)
    with pytest.raises(ValueError, match="depth"):
        C.scan_1m(model, codes, depth=27, **kw)
    with pytest.raises(ValueError):
        C.scan_1m(model, codes.view(1, -1), **kw)
    with pytest.raises(TypeError):
        C.scan_1m(object(), codes, **kw)
