"""Compartments per level of the SV screen on the MI355X (orca_screen_eigenvectors, orca_screen_gc_tracks; sv.sv_screen(..., scores=True,
compartments=), sv.sv_scores(..., compartments=, phase=)).

The eigen kernel alone, through raw ctypes and through `engine`, on planted spectra Q diag(8, -4, 2) Q^T + 0.02 noise / sqrt(n) whose upper triangle
alone is stored.  For n < 64: d_lo = 0, center = False (the band and the centering destroy the planted gaps of tiny matrices); for n >= 64: d_lo = 2,
center = True.  B = 3 with a batch stride above n * n, K = 3, tol = 1e-8.  The bounds are derived from `numpy.linalg.eigh` of the numpy-prepared A
(`sv.compartment_matrix_host`), lambda_k in descending |lambda|, u_k its unit vectors, gap_k = the distance from lambda_k to the rest of the spectrum:
  (1) the residual recomputed in numpy from the returned fp32 E, |A v - lambda v|_2 / |lambda| with v = E / |E|_2 and the returned eigenvalue, is at
      most tol + 2 * 2^-24 * |lambda_1| / |lambda_k|: the second term is the rounding of v to fp32, |A dv| <= |lambda_1| 2^-24, on both sides;
  (2) |eigenvalue - lambda_k| <= tol |lambda_k|;
  (3) |v - u_k|_2 <= sqrt(2) residual |lambda_k| / gap_k + 2^-23 (Davis-Kahan: sin(angle) <= |r| / gap, |v - u| <= sqrt(2) sin; `residual` is the
      kernel's own report).
Every figure is printed before it is asserted.  Then the NaN rule, the sign rule, a tied spectrum (the only cap on iterations relied on: max_iter = 50),
bit-for-bit independence of the batch, the refused arguments; the GC kernel against `sv.gc_tracks_host` exactly; and the screen end to end on a
synthetic model and chromosome with a deletion, a duplication, an inversion and a deletion larger than the finest window."""
import ctypes

import numpy as np
import pytest
import torch

from orca_amd import _lib, engine, orca_models, sv
from orca_amd._lib import OrcaHipError

pytestmark = pytest.mark.gpu

LAM = (8.0, -4.0, 2.0)
TOL = 1e-8
EINVAL = -1                                                      # ORCA_EINVAL (include/orca_hip.h)


def planted(n, seed, noise=0.02):
    rs = np.random.RandomState(seed)
    q, _ = np.linalg.qr(rs.randn(n, len(LAM)))
    m = (q * np.array(LAM)) @ q.T + noise * rs.randn(n, n) / np.sqrt(n)
    return np.triu(m).astype(np.float32)


def strided(maps, pad, cuda):
    """[B, n, n] numpy -> a device view with batch stride n * n + pad (the padding holds NaN: never read)"""
    B, n = maps.shape[0], maps.shape[1]
    buf = torch.full((B, n * n + pad), float("nan"), dtype=torch.float32, device=cuda)
    buf[:, :n * n] = torch.from_numpy(maps.reshape(B, n * n)).to(cuda)
    return torch.as_strided(buf, (B, n, n), (n * n + pad, n, 1))


def _dp(t):
    return ctypes.c_void_p(t.data_ptr() if t is not None else 0)


def raw_eigenvectors(cuda, maps, K, d_lo, center, tol, max_iter, phase=None):
    """orca_screen_eigenvectors through ctypes: (rc, dict of numpy arrays)"""
    ctx = engine.get_context(cuda)
    ctx.sync_stream()
    B, n = maps.shape[0], maps.shape[1]
    k = max(K, 1)
    E = torch.full((B, k, n), 7.0, dtype=torch.float32, device=cuda)
    lam, res = (torch.full((B, k), 7.0, dtype=torch.float64, device=cuda) for _ in range(2))
    it, nv = torch.full((B, k), 7, dtype=torch.int32, device=cuda), torch.full((B,), 7, dtype=torch.int32, device=cuda)
    rc = _lib.load().orca_screen_eigenvectors(ctx.handle, _dp(maps), maps.stride(0) if B > 1 else n * n, B, n, K, d_lo, center, tol, max_iter, _dp(phase), _dp(E),
                                              _dp(lam), _dp(res), _dp(it), _dp(nv))
    torch.cuda.synchronize(cuda)
    return rc, {"E": E.cpu().numpy(), "eigenvalue": lam.cpu().numpy(), "residual": res.cpu().numpy(), "iterations": it.cpu().numpy(), "n_valid": nv.cpu().numpy()}


def eigenvectors(cuda, route, maps, K, d_lo, center, tol=TOL, max_iter=1000, phase=None):
    if route == "raw":
        rc, got = raw_eigenvectors(cuda, maps, K, d_lo, int(center), tol, max_iter, phase)
        assert rc == 0, _lib.load().orca_last_error()
        return got
    got = engine.screen_eigenvectors(engine.get_context(cuda), maps, K, d_lo, center, tol, max_iter, phase)
    assert got["E"].dtype == torch.float32 and got["eigenvalue"].dtype == torch.float64 and got["residual"].dtype == torch.float64
    assert got["iterations"].dtype == torch.int32 and got["n_valid"].dtype == torch.int32
    return {k: v.cpu().numpy() for k, v in got.items()}


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def spectrum(m, d_lo, center):
    A, valid = sv.compartment_matrix_host(m, d_lo, center)
    lam, U = np.linalg.eigh(A)
    o = np.argsort(-np.abs(lam), kind="stable")
    return A, valid, lam[o], U[:, o]


def check_planted(got, b, m, d_lo, center, K, what):
    A, valid, lam, U = spectrum(m, d_lo, center)
    assert valid.all() and got["n_valid"][b] == m.shape[0]
    for k in range(K):
        E = got["E"][b, k].astype(np.float64)
        ev, res, it = got["eigenvalue"][b, k], got["residual"][b, k], got["iterations"][b, k]
        v = E / np.linalg.norm(E)
        again = np.linalg.norm(A @ v - ev * v) / abs(ev)
        b1 = TOL + 2.0 * 2.0 ** -24 * abs(lam[0]) / abs(lam[k])
        gap = np.abs(lam[k] - np.delete(lam, k)).min()
        u = U[:, k] * (1.0 if U[:, k] @ v >= 0 else -1.0)
        b3 = np.sqrt(2.0) * res * abs(lam[k]) / gap + 2.0 ** -23
        print(what, "map", b, "k", k, f"lambda {ev:.6f} (eigh {lam[k]:.6f}, relative gap {gap / abs(lam[k]):.3f}) iterations {it} residual {res:.2e}"
              f" | recomputed {again:.2e} <= {b1:.2e} | eigenvalue {abs(ev - lam[k]):.1e} <= {TOL * abs(lam[k]):.1e} | vector {np.linalg.norm(v - u):.2e} <= {b3:.2e}")
        assert res <= TOL and it >= 1, (what, b, k)
        assert again <= b1, (what, b, k)
        assert abs(ev - lam[k]) <= TOL * abs(lam[k]), (what, b, k)
        assert np.linalg.norm(v - u) <= b3, (what, b, k)
        assert abs(E @ E - abs(ev)) <= 4 * 2.0 ** -24 * abs(ev), (what, b, k)                # E = v sqrt(|lambda|), rounded to fp32 per component
        assert E[np.argmax(np.abs(got["E"][b, k]))] > 0, (what, b, k)                        # no phase: the largest component is positive


# ---- the eigen kernel alone -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("route", ["raw", "engine"])
@pytest.mark.parametrize("n", [4, 5, 17, 64, 250, 256])
def test_planted_spectra_within_the_bounds_derived_from_eigh(cuda, n, route):
    d_lo, center = (0, False) if n < 64 else (2, True)
    maps = np.stack([planted(n, 1000 * b + n) for b in range(3)])
    dev = strided(maps, 5, cuda)
    assert dev.stride(0) == n * n + 5
    got = eigenvectors(cuda, route, dev, 3, d_lo, center)
    assert got["E"].shape == (3, 3, n) and got["eigenvalue"].shape == (3, 3) and got["n_valid"].shape == (3,)
    for b in range(3):
        check_planted(got, b, maps[b], d_lo, center, 3, (n, route))
    if n >= 64:                                                  # the lower triangle is never read
        junk = maps + np.tril(np.full((n, n), np.nan, dtype=np.float32), -1)
        assert all(same_bits(got[k], v) for k, v in eigenvectors(cuda, route, strided(junk, 5, cuda), 3, d_lo, center).items())


def test_nan_pixel_and_too_few_valid_bins(cuda):
    n = 64
    hole = planted(n, 1)
    hole[3, 40] = np.nan
    few = planted(n, 2)
    few[0, 2:] = np.nan                                          # S[0][j] is NaN for every j >= 2: bin 0 and bins 2 .. 63 are invalid, bin 1 is left
    inside = planted(n, 3)
    inside[7, 8] = np.nan                                        # |i - j| < d_lo: not a kept pixel
    maps = np.stack([hole, few, inside, planted(n, 4)])
    for route in ("raw", "engine"):
        got = eigenvectors(cuda, route, strided(maps, 3, cuda), 2, 2, True)
        assert got["n_valid"].tolist() == [62, 1, 64, 64]
        for k in range(2):
            assert np.flatnonzero(np.isnan(got["E"][0, k])).tolist() == [3, 40]
        assert np.isnan(got["E"][1]).all() and np.isnan(got["eigenvalue"][1]).all() and np.isnan(got["residual"][1]).all() and got["iterations"][1].tolist() == [0, 0]
        assert np.isfinite(got["E"][2:]).all() and np.isfinite(got["eigenvalue"][[0, 2, 3]]).all() and (got["residual"][[0, 2, 3]] <= TOL).all()
        want = sv.eigenvectors_host(maps, 2, 2, True)
        assert np.array_equal(want["n_valid"], got["n_valid"]) and np.array_equal(np.isnan(want["E"]), np.isnan(got["E"]))
        for b in (0, 2, 3):
            A, valid, lam, U = spectrum(maps[b], 2, True)
            for k in range(2):
                assert abs(got["eigenvalue"][b, k] - lam[k]) <= TOL * abs(lam[k]), (b, k)
                gap = np.abs(lam[k] - np.delete(lam, k)).min()
                d = np.nan_to_num(got["E"][b, k].astype(np.float64) - want["E"][b, k].astype(np.float64))
                # the vectors' bound (3) scaled by sqrt(|lambda|), both sides rounded to fp32
                assert np.linalg.norm(d) <= np.sqrt(abs(lam[k])) * (np.sqrt(2.0) * got["residual"][b, k] * abs(lam[k]) / gap + 2.0 ** -22), (b, k)
    # n_valid = K + 1 is computed, n_valid = K is not
    m = planted(5, 5)
    m[0, 4] = np.nan                                             # bins 0 and 4 invalid: 3 valid bins
    three = eigenvectors(cuda, "engine", strided(m[None], 0, cuda), 3, 0, False)
    two = eigenvectors(cuda, "engine", strided(m[None], 0, cuda), 2, 0, False)
    assert three["n_valid"].tolist() == [3] and np.isnan(three["E"]).all() and three["iterations"].tolist() == [[0, 0, 0]]
    assert two["n_valid"].tolist() == [3] and np.isfinite(two["E"][0][:, 1:4]).all() and np.isnan(two["E"][0][:, [0, 4]]).all() and (two["residual"] <= TOL).all()


@pytest.mark.parametrize("route", ["raw", "engine"])
def test_sign_follows_the_phase_or_the_largest_component(cuda, route):
    n = 250
    maps = np.stack([planted(n, 10 + b) for b in range(2)])
    dev = strided(maps, 2, cuda)
    rs = np.random.RandomState(3)
    phase = rs.rand(2, n).astype(np.float32)
    phase[0, 5] = np.nan                                         # left out of the correlation
    phase[1, 7] = np.inf
    flat = np.ones((2, n), dtype=np.float32)                     # no correlation: the fallback
    lone = np.full((2, n), np.nan, dtype=np.float32)
    lone[:, 9] = 1.0                                             # fewer than 2 bins: the fallback
    up = lambda p: torch.from_numpy(p).to(cuda)
    free = eigenvectors(cuda, route, dev, 3, 2, True)
    with_p, anti = eigenvectors(cuda, route, dev, 3, 2, True, phase=up(phase)), eigenvectors(cuda, route, dev, 3, 2, True, phase=up(-phase))
    for b in range(2):
        use = np.isfinite(phase[b])
        for k in range(3):
            e = with_p["E"][b, k].astype(np.float64)
            p = phase[b, use].astype(np.float64)
            c = ((e[use] - e[use].mean()) * (p - p.mean())).sum()
            print("phase", b, k, "centred cross sum", c)
            assert c > 0, (b, k)
            f = free["E"][b, k]
            assert f[np.argmax(np.abs(f))] > 0
    assert same_bits(anti["E"], -with_p["E"]) and same_bits(np.abs(free["E"]), np.abs(with_p["E"]))
    for k in ("eigenvalue", "residual", "iterations", "n_valid"):
        assert same_bits(free[k], with_p[k]) and same_bits(free[k], anti[k])
    assert same_bits(eigenvectors(cuda, route, dev, 3, 2, True, phase=up(flat))["E"], free["E"])
    assert same_bits(eigenvectors(cuda, route, dev, 3, 2, True, phase=up(lone))["E"], free["E"])
    # the fallback's tie: [[1, -1], [-1, 1]] has the leading vector (1, -1) / sqrt(2), and w = A v has w_1 = -w_0 exactly - two components of equal
    # size: the one with the lower index is made positive
    t = np.array([[[1.0, -1.0], [0.0, 1.0]]], dtype=np.float32)
    got = eigenvectors(cuda, route, strided(t, 0, cuda), 1, 0, False)
    assert got["E"][0, 0, 0] > 0 and got["E"][0, 0, 1] == -got["E"][0, 0, 0] and abs(got["E"][0, 0, 0] - 1.0) <= 2.0 ** -22 and abs(got["eigenvalue"][0, 0] - 2.0) <= 2e-8


@pytest.mark.parametrize("route", ["raw", "engine"])
def test_a_tied_spectrum_stops_at_max_iter(cuda, route):
    t = np.zeros((1, 6, 6), dtype=np.float32)
    t[0, 0, 1] = t[0, 1, 0] = 1.0                                # eigenvalues +1 and -1: power iteration cannot separate them
    got = eigenvectors(cuda, route, strided(t, 0, cuda), 1, 0, False, tol=TOL, max_iter=50)
    print("tie", {k: v.tolist() for k, v in got.items()})
    assert got["residual"][0, 0] > TOL and got["iterations"][0, 0] == 50 and got["n_valid"][0] == 6
    assert not any(np.isnan(got[k].astype(np.float64)).any() for k in got)


def test_a_maps_bits_do_not_depend_on_the_batch(cuda):
    n = 250
    maps = np.stack([planted(n, 20 + b) for b in range(5)])
    maps[1, 3, 40] = np.nan
    phase = np.random.RandomState(4).rand(5, n).astype(np.float32)
    ctx = engine.get_context(cuda)
    batch = engine.screen_eigenvectors(ctx, strided(maps, 11, cuda), 3, 2, True, TOL, 1000, torch.from_numpy(phase).to(cuda))
    for b in (1, 3):
        alone = engine.screen_eigenvectors(ctx, strided(maps[b:b + 1], 0, cuda), 3, 2, True, TOL, 1000, torch.from_numpy(phase[b:b + 1]).to(cuda))
        for k in batch:
            assert same_bits(batch[k][b:b + 1].cpu().numpy(), alone[k].cpu().numpy()), (b, k)
    again = engine.screen_eigenvectors(ctx, strided(maps, 11, cuda), 3, 2, True, TOL, 1000, torch.from_numpy(phase).to(cuda))
    assert all(same_bits(batch[k].cpu().numpy(), again[k].cpu().numpy()) for k in batch)


def test_bad_arguments_are_refused_before_any_launch(cuda):
    """Every call below is refused by the host entry point's checks (return codes only: nothing reaches a kernel); the outputs keep their fill."""
    big = torch.zeros((2, 257, 257), dtype=torch.float32, device=cuda)
    ok = torch.zeros((2, 6, 6), dtype=torch.float32, device=cuda)
    cases = [(big, 1, 2, 1, TOL, 10), (ok, 4, 2, 1, TOL, 10), (ok, 0, 2, 1, TOL, 10), (ok, 1, 6, 1, TOL, 10), (ok, 1, -1, 1, TOL, 10), (ok, 1, 2, 1, 0.0, 10),
             (ok, 1, 2, 1, -1.0, 10), (ok, 1, 2, 1, float("nan"), 10), (ok, 1, 2, 1, TOL, 0), (ok, 1, 2, 2, TOL, 10)]
    for maps, K, d_lo, center, tol, max_iter in cases:
        rc, got = raw_eigenvectors(cuda, maps, K, d_lo, center, tol, max_iter)
        msg = _lib.load().orca_last_error()
        assert rc == EINVAL and msg and b"orca_screen_eigenvectors" in msg, (K, d_lo, center, tol, max_iter, rc, msg)
        assert (got["E"] == 7.0).all() and (got["eigenvalue"] == 7.0).all() and (got["iterations"] == 7).all() and (got["n_valid"] == 7).all()
    ctx = engine.get_context(cuda)
    for kw in (dict(n_eigs=4), dict(d_lo=6), dict(tol=0.0), dict(max_iter=0)):
        with pytest.raises(OrcaHipError):
            engine.screen_eigenvectors(ctx, ok, **kw)
    with pytest.raises(ValueError):
        engine.screen_eigenvectors(ctx, ok, phase=torch.zeros((2, 5), dtype=torch.float32, device=cuda))
    with pytest.raises(ValueError):
        engine.screen_eigenvectors(ctx, ok[0])


# ---- the GC kernel ------------------------------------------------------------------------------------------------------------------------------------------
def test_gc_tracks_equal_the_host_restatement_exactly(cuda):
    L = 200_001
    rs = np.random.RandomState(6)
    codes = rs.randint(0, 4, L).astype(np.uint8)
    for s in rs.randint(0, L - 3000, 12):
        codes[s:s + int(rs.randint(1, 3000))] = 4                # N runs
    codes[100_000:100_016] = 4                                   # all-N bins at the small bin sizes
    ctx = engine.get_context(cuda)
    dev = torch.from_numpy(codes).to(cuda)
    n = 250
    sizes = [400, 100, 4, 3, 2, 1]                               # six nested windows around base 100 000, at odd offsets
    offs = [100_000 - n * bs // 2 + k for k, bs in enumerate(sizes)]
    assert all(offs[k] <= offs[k + 1] and offs[k + 1] + n * sizes[k + 1] <= offs[k] + n * sizes[k] for k in range(5))
    for view, host in ((dev, codes), (dev[1:], codes[1:]), (dev[13:], codes[13:])):             # every alignment of the first base
        got = engine.gc_tracks(ctx, view, offs, sizes, n)
        want = sv.gc_tracks_host(host, offs, sizes, n)
        assert got.dtype == torch.float32 and tuple(got.shape) == (6, n) and same_bits(got.cpu().numpy(), want)
        assert np.isnan(want[5]).any() and not np.isnan(want).all(axis=1).any()              # all-N bins are among them
    for offs1, sizes1, n1 in (([7], [128_000], 1), ([0], [L], 1), ([1], [100_000], 2), ([3, 0], [128_000, 66_667], 1), ([L - 1], [1], 1)):
        assert same_bits(engine.gc_tracks(ctx, dev, offs1, sizes1, n1).cpu().numpy(), sv.gc_tracks_host(codes, offs1, sizes1, n1)), (offs1, sizes1)
    many = list(range(0, 20 * 37, 37))                           # more windows than one launch takes
    assert same_bits(engine.gc_tracks(ctx, dev, many, [9] * 20, 17).cpu().numpy(), sv.gc_tracks_host(codes, many, [9] * 20, 17))
    allg = torch.full((64,), 2, dtype=torch.uint8, device=cuda)
    assert engine.gc_tracks(ctx, allg, [0], [16], 4).cpu().numpy().tolist() == [[1.0] * 4]
    for off, bs in ((L - 250 * 4 + 1, 4), (-1, 4), (0, 0), (L, 1), (0, L // 250 + 1)):          # a window past L (or before 0) is refused
        with pytest.raises(OrcaHipError, match="orca_screen_gc_tracks"):
            engine.gc_tracks(ctx, dev, [0, off], [1, bs], n)
        with pytest.raises(ValueError):
            sv.gc_tracks_host(codes, [0, off], [1, bs], n)


# ---- the screen ---------------------------------------------------------------------------------------------------------------------------------------------
CHR = 40_000_000
# a deletion, a duplication, an inversion, and a deletion larger than the finest (1 Mb) window: its finest level shares no locus with the reference's
VARIANTS = [sv.SV("del", 17_001_234, 17_803_210), sv.SV("dup", 21_004_000, 21_500_000), sv.SV("inv", 15_000_000, 18_000_000), sv.SV("del", 18_000_000, 19_200_000)]
Q = sv.CompartmentParams(n_eigs=2)
TOP_NEW = ["compartment_params", "gc", "ref_gc"]
PLAIN_TOP = ["bin_map", "count", "junction_bins", "models"]


@pytest.fixture(scope="module")
def case(cuda):
    g = torch.Generator(device=cuda).manual_seed(11)
    genome = torch.randint(0, 4, (CHR,), device=cuda, generator=g, dtype=torch.uint8)
    genome[7_000_000:7_003_000] = 4                              # an N run inside the windows
    genome[16_000_000:17_000_000:3] = 0                          # a GC-poor megabase: the GC track is not flat
    model = orca_models.H1esc(synthetic_seed=0)
    screened = sv.sv_screen([model], genome, VARIANTS, CHR, min_uses=1, scores=True, compartments=Q, keep_maps=True)
    return model, genome, screened


def dict_maps(out, m):
    return np.stack([np.asarray(p, dtype=np.float32).reshape((-1, 250, 250)) for p in out["predictions"][m]])          # [6, C, 250, 250]


def compartments_same_bits(x, y):
    return (sorted(x) == sorted(y) and all(same_bits(x[k], y[k]) for k in ("bin_map", "count", "junction_bins", "ref_gc", "gc"))
            and x["compartment_params"] == y["compartment_params"] and len(x["models"]) == len(y["models"])
            and all(sorted(a) == sorted(b) and all(same_bits(a[k], b[k]) for k in a) for a, b in zip(x["models"], y["models"])))


def test_screen_fields_equal_the_kernels_on_the_kept_maps(case, cuda):
    model, genome, screened = case
    ctx = engine.get_context(cuda)
    assert sorted(screened) == [0, 1, 2, 3]
    for i, v in enumerate(VARIANTS):
        e = screened[i]
        s = e["scores"]
        assert sorted(s) == sorted(PLAIN_TOP + TOP_NEW) and s["compartment_params"] == Q
        # the GC tracks: the restatement on the assembled windows, exactly
        rp, rw, rm, ap, aw, am = sv.sv_windows(v, CHR)
        for key, pieces, wpos, out in (("ref_gc", rp, rw, e["ref"]), ("gc", ap, aw, e["alt"])):
            codes = sv.assemble_codes(genome, pieces).cpu().numpy()
            off = [out["start_coords"][k] - (wpos - 16_000_000) for k in range(6)]
            assert s[key].dtype == np.float32 and same_bits(s[key], sv.gc_tracks_host(codes, off, [128_000 >> k for k in range(6)], 250)), (v, key)
        assert s["ref_gc"].std() > 0 and not np.isnan(s["ref_gc"]).any()
        bm = s["bin_map"]
        for m, got in enumerate(s["models"]):
            assert set(sv.COMPARTMENT_SCORE_FIELDS) <= set(got)
            C = got["compartment"].shape[1]
            bmc = np.repeat(bm, C, axis=0)
            for side, out, gc in (("ref_", e["ref"], s["ref_gc"]), ("", e["alt"], s["gc"])):
                maps = torch.from_numpy(dict_maps(out, m).reshape(6 * C, 250, 250)).to(cuda)
                ph = torch.from_numpy(np.repeat(gc, C, axis=0)).to(cuda)
                want = {k: t.cpu().numpy() for k, t in engine.screen_eigenvectors(ctx, maps, Q.n_eigs, Q.d_lo, Q.center, Q.tol, Q.max_iter, ph).items()}
                assert got[side + "compartment"].dtype == np.float32 and got[side + "compartment"].shape == (6, C, 2, 250)
                assert same_bits(got[side + "compartment"], want["E"].reshape(6, C, 2, 250)), (v, m, side)
                assert same_bits(got[side + "compartment_eigenvalue"], want["eigenvalue"].reshape(6, C, 2)), (v, m, side)
                assert same_bits(got[side + "compartment_residual"], want["residual"].reshape(6, C, 2)), (v, m, side)
                assert same_bits(got[side + "compartment_iterations"], want["iterations"].reshape(6, C, 2)), (v, m, side)
                assert got[side + "compartment_converged"].dtype == np.bool_ and np.array_equal(got[side + "compartment_converged"], got[side + "compartment_residual"] <= Q.tol)
                assert (want["n_valid"] == 250).all() and not np.isnan(want["E"]).any()
                # wherever the kernel took the phase rule (2 or more valid bins with a finite phase), the vector does not anti-correlate with its GC
                E = got[side + "compartment"].astype(np.float64)
                for lv in range(6):
                    p = gc[lv].astype(np.float64)
                    use = np.isfinite(p)
                    if use.sum() < 2:
                        continue
                    for c in range(C):
                        for k in range(2):
                            x = E[lv, c, k, use]
                            assert ((x - x.mean()) * (p[use] - p[use].mean())).sum() >= 0, (v, m, side, lv, c, k)
                print(v, side or "alt_", "iterations", got[side + "compartment_iterations"][:, 0].tolist(), "converged", got[side + "compartment_converged"][:, 0].tolist())
            want = sv.paired_compartment_scores_host(got["compartment"].reshape(6 * C, 2, 250), got["ref_compartment"].reshape(6 * C, 2, 250), bmc)
            assert same_bits(got["compartment_delta"], want["delta"].reshape(6, C, 2, 250)) and same_bits(got["compartment_corr"], want["corr"].reshape(6, C, 2))
            assert same_bits(got["compartment_flips"], want["flips"].reshape(6, C, 2)) and got["compartment_flips"].dtype == np.int32
            for lv in range(6):
                assert np.array_equal(np.isnan(got["compartment_delta"][lv]), np.broadcast_to(bm[lv] < 0, got["compartment_delta"][lv].shape))
                if s["count"][lv] == 0:
                    assert np.isnan(got["compartment_delta"][lv]).all() and np.isnan(got["compartment_corr"][lv]).all() and not got["compartment_flips"][lv].any()
    big = screened[3]["scores"]
    assert big["count"][5] == 0 and np.isnan(big["models"][0]["compartment_corr"][5]).all()          # the deletion larger than the finest window
    assert all((screened[i]["scores"]["count"] > 0).all() for i in range(3))
    inv = screened[2]["scores"]["bin_map"]
    assert any((np.diff(inv[k][inv[k] >= 0]) < 0).any() for k in range(6))                          # the inversion's maps do descend


def test_sv_scores_with_the_gc_as_phase_gives_the_same_fields(case, cuda):
    model, genome, screened = case
    for i, v in enumerate(VARIANTS):
        e = screened[i]
        s = e["scores"]
        again = sv.sv_scores(v, e["ref"], e["alt"], CHR, cuda, compartments=Q, phase=(s["ref_gc"], s["gc"]))
        assert compartments_same_bits(again, s), v
    # without a phase: the reference's largest component is positive, the alt vector does not point against it through the bin map, and |E| is the same
    e = screened[1]
    s = e["scores"]
    free = sv.sv_scores(VARIANTS[1], e["ref"], e["alt"], CHR, cuda, compartments=Q)
    assert sorted(free) == sorted(PLAIN_TOP + ["compartment_params"])
    for got, had in zip(free["models"], s["models"]):
        assert same_bits(np.abs(got["ref_compartment"]), np.abs(had["ref_compartment"])) and same_bits(np.abs(got["compartment"]), np.abs(had["compartment"]))
        assert same_bits(got["compartment_eigenvalue"], had["compartment_eigenvalue"])
        r = got["ref_compartment"]
        assert (np.take_along_axis(r, np.abs(r).argmax(axis=-1)[..., None], axis=-1) > 0).all()
        for lv in range(6):
            M = np.flatnonzero(s["bin_map"][lv] >= 0)
            dot = (got["compartment"][lv][..., M].astype(np.float64) * r[lv][..., s["bin_map"][lv, M]].astype(np.float64)).sum(axis=-1)
            assert (dot >= 0).all(), lv


def test_maps_can_stay_on_the_device_and_nothing_else_changes(case):
    model, genome, screened = case
    bare = sv.sv_screen([model], genome, VARIANTS, CHR, min_uses=1, scores=True, compartments=Q, keep_maps=False)
    plain = sv.sv_screen([model], genome, VARIANTS, CHR, min_uses=1, scores=True)
    for i in range(len(VARIANTS)):
        assert bare[i]["ref"]["predictions"] is None and bare[i]["alt"]["predictions"] is None
        assert compartments_same_bits(bare[i]["scores"], screened[i]["scores"]), i
        p, s = plain[i]["scores"], screened[i]["scores"]
        assert sorted(p) == PLAIN_TOP and sorted(s) == sorted(PLAIN_TOP + TOP_NEW)
        assert all(same_bits(p[k], s[k]) for k in PLAIN_TOP if k != "models")
        for a, b in zip(p["models"], s["models"]):
            assert sorted(a) == sorted(set(b) - set(sv.COMPARTMENT_SCORE_FIELDS)) and all(same_bits(a[k], b[k]) for k in a)
        for allele in ("ref", "alt"):
            for j in range(6):
                assert same_bits(plain[i][allele]["predictions"][0][j], screened[i][allele]["predictions"][0][j]), (i, allele, j)
    with pytest.raises(ValueError):
        sv.sv_screen([model], genome, VARIANTS[:1], CHR, compartments=True)


def test_two_genomepredict_calls_pass_the_gc_of_their_windows(case, cuda):
    model, genome, screened = case
    full = sv.sv_screen([model], genome, VARIANTS[1:2], CHR, incremental=False, scores=True, compartments=Q)
    s, had = full[0]["scores"], screened[1]["scores"]                  # (the result is keyed by the index into the list that was passed)
    assert sorted(s) == sorted(PLAIN_TOP + TOP_NEW) and same_bits(s["ref_gc"], had["ref_gc"]) and same_bits(s["gc"], had["gc"])
    again = sv.sv_scores(VARIANTS[1], full[0]["ref"], full[0]["alt"], CHR, cuda, compartments=Q, phase=(s["ref_gc"], s["gc"]))
    assert compartments_same_bits(again, s)
