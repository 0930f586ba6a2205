"""Impact scores of the SV screen on the MI355X (orca_screen_paired_aligned_scores; sv.sv_screen(..., scores=), sv.sv_scores): the kernel alone
against the numpy restatement `sv.paired_aligned_scores_host` on hand-made bin maps, bit-for-bit invariance to the batch, where a NaN pixel
shows, the entry point's argument checks (return codes only: nothing malformed reaches a kernel), and the screen end to end on the variants of
tests/test_gpu_sv_incremental.py (synthetic H1esc(synthetic_seed=0), a 40 Mb random chromosome) - one and two models, a two-target model.

Tolerances, derived and not measured.  Both sides compute every term in fp64 from the same fp32 pixels; they add the terms in different orders,
round a product and the addition that takes it once (device) or twice (numpy), may differ in the last bit of a root or a quotient, and round to
fp32 at the end.  A sum of N fp64 terms in ANY order is within N 2^-53 sum |term| of the exact sum, so with c the mapped bins of the pair:
  ``abs_mean``, ``delta_mean``   N = c^2 terms of magnitude |dl|, sum |dl| = c^2 abs_mean:  |got - want| <= RTOL |want| + c^2 2^-53 abs_mean
  ``profile``                    N = c terms per row, sum |dl| = c profile:                 |got - want| <= RTOL |want| + c 2^-53 |want|
  ``rms``                        the mean of dl^2 moves by at most t = c^2 2^-53 rms^2, carried through the root:
                                                                                            |got - want| <= RTOL |want| + sqrt(want^2 + t) - want
  ``corr``                       |got - want| <= 8 (c^2 + 4) 2^-53, the bound of tests/test_gpu_screen_strata.py with c^2 pairs: each centred sum
                                 of N terms carries at most (N + 4) 2^-53 of the sum of its terms' magnitudes, for C that is at most sqrt(X Y)
                                 (Cauchy-Schwarz), so each sum moves r by at most (N + 4) 2^-53; two such errors enter r per side, two sides
  ``abs_max``                    the largest fp64 difference rounded to fp32 on both sides: equal
  ``count``                      exact
RTOL = 2.4e-7 is the project's two fp32 ulps (tests/test_gpu_screen_aligned.py).  NaN sits in the same places on both sides.  The screen's
scores are checked against the restatement on the maps the same call returned, with the same bounds."""
import ctypes

import numpy as np
import pytest
import torch

from orca_amd import _lib, engine, orca_models, sv
from orca_amd._lib import OrcaHipError
from tests.test_gpu_screen_aligned import RTOL, _dp, _hp, _refused, kernel_maps
from tests.test_gpu_sv_incremental import CHR, VARIANTS

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -53
SCALARS = ("abs_mean", "abs_max", "delta_mean", "rms", "corr")
FIELDS = SCALARS + ("profile",)
WORST = {}


def _np(t):
    return t.cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)


def bits(t):
    a = _np(t)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def same_bits(x, y):
    return _np(x).shape == _np(y).shape and _np(x).dtype == _np(y).dtype and np.array_equal(bits(x), bits(y))


def check(got, want, what):
    """device results (a dict of tensors or arrays, any leading shape) against `sv.paired_aligned_scores_host`'s on the same maps, within the
    tolerances of the module docstring"""
    c = want["count"].astype(np.float64)
    assert _np(got["count"]).dtype == np.int32 and np.array_equal(_np(got["count"]), want["count"]), (what, "count")
    with np.errstate(invalid="ignore"):
        w = want["rms"]
        tols = {"abs_mean": RTOL * np.abs(want["abs_mean"]) + c * c * EPS * want["abs_mean"],
                "delta_mean": RTOL * np.abs(want["delta_mean"]) + c * c * EPS * want["abs_mean"],
                "profile": RTOL * np.abs(want["profile"]) + c[..., None] * EPS * np.abs(want["profile"]),
                "rms": RTOL * np.abs(w) + np.sqrt(w * w + c * c * EPS * w * w) - w,
                "corr": 8 * (c * c + 4) * EPS}
    for k in FIELDS:
        g = _np(got[k])
        assert g.dtype == (np.float64 if k == "corr" else np.float32), (what, k, g.dtype)
        g, h = g.astype(np.float64), want[k]
        assert g.shape == h.shape, (what, k, g.shape, h.shape)
        assert np.array_equal(np.isnan(g), np.isnan(h)), (what, k, np.argwhere(np.isnan(g) != np.isnan(h))[:5])
        f = ~np.isnan(h)
        if k == "abs_max":
            assert np.array_equal(g[f], h[f].astype(np.float32).astype(np.float64)), (what, k)
            continue
        err, tol = np.abs(g[f] - h[f]), np.broadcast_to(tols[k], h.shape)[f]
        ratio = float((err / np.maximum(tol, 1e-300)).max()) if err.size else 0.0
        WORST[k] = max(WORST.get(k, 0.0), ratio)
        assert np.all(err <= tol), (what, k, ratio, float(err.max()))


def all_maps(n):
    return dict(kernel_maps(n), descending=np.arange(n)[::-1].copy())


def pairs(rs, B, n, cuda, near=False):
    """B random pairs of maps, alt with batch stride n * n + 7 and ref with n * n + 3 (``near``: alt = ref + 1e-4 noise, r within 1e-8 of 1)"""
    a = torch.from_numpy(rs.randn(B, n * n + 7).astype(np.float32)).to(cuda).as_strided((B, n, n), (n * n + 7, n, 1))
    r = torch.from_numpy(rs.randn(B, n * n + 3).astype(np.float32)).to(cuda).as_strided((B, n, n), (n * n + 3, n, 1))
    if near:
        a.copy_(r + 1e-4 * a)
    return a, r


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 250, 256])
def test_kernel_equals_the_host_restatement(cuda, n, B):
    ctx = engine.get_context(cuda)
    maps = all_maps(n)
    names = list(maps)
    rs = np.random.RandomState(3000 * n + B)
    for near in (False, True):
        for g0 in range(0, len(names), B):
            group = names[g0: g0 + B]
            bm = np.stack([maps[k] for k in group]).astype(np.int32)
            alt, ref = pairs(rs, len(group), n, cuda, near)
            if len(group) > 1:
                assert alt.stride(0) == n * n + 7 and ref.stride(0) == n * n + 3
            got = engine.screen_paired_aligned_scores(ctx, alt, ref, bm)
            assert tuple(got["profile"].shape) == (len(group), n) and all(tuple(got[k].shape) == (len(group),) for k in SCALARS + ("count",))
            check(got, sv.paired_aligned_scores_host(alt.cpu().numpy(), ref.cpu().numpy(), bm), (n, B, near, group))
            for b, k in enumerate(group):                                   # the degenerate maps give what the table of the entry point says
                if k == "none":
                    assert int(got["count"][b]) == 0 and all(torch.isnan(got[f][b]).all() for f in FIELDS)
                if k == "one":
                    d = np.float32(abs(float(alt[b, n // 2, n // 2]) - float(ref[b, n - 1, n - 1])))
                    assert int(got["count"][b]) == 1 and float(got["abs_mean"][b]) == float(got["abs_max"][b]) == d and torch.isnan(got["corr"][b])
                    assert int(torch.isfinite(got["profile"][b]).sum()) == 1
                if k == "identity" and near and n >= 63:                    # the case fp64 is there for: 1 - r is small and is not lost
                    assert 1e-9 < 1 - float(got["corr"][b]) < 1e-7


@pytest.mark.parametrize("n", [65, 250, 256])
def test_a_pairs_results_do_not_depend_on_the_batch(cuda, n):
    """A pair alone (contiguous) against the same pair as row 0, 1 and 2 of a batch of three - other batch strides, other pairs and bin maps beside
    it - under every bin map: the same bits."""
    ctx = engine.get_context(cuda)
    maps = all_maps(n)
    rs = np.random.RandomState(13 * n)
    alt1, ref1 = pairs(rs, 1, n, cuda)
    alt1, ref1 = alt1.contiguous(), ref1.contiguous()
    alt3, ref3 = pairs(rs, 3, n, cuda)
    for name in maps:
        bm1 = maps[name].astype(np.int32)[None]
        alone = engine.screen_paired_aligned_scores(ctx, alt1, ref1, bm1)
        for row in range(3):
            alt3[row], ref3[row] = alt1[0], ref1[0]                         # the rows written earlier stay, as other pairs
            bm3 = np.stack([maps["holes"], maps["shift"], maps["duplicate"]]).astype(np.int32)
            bm3[row] = bm1[0]
            got = engine.screen_paired_aligned_scores(ctx, alt3, ref3, bm3)
            for f in FIELDS:
                assert same_bits(got[f][row], alone[f][0]), (name, row, f)
            assert int(got["count"][row]) == int(alone["count"][0])


def test_nan_shows_at_a_mapped_pair_only(cuda):
    ctx = engine.get_context(cuda)
    n = 50
    m = np.arange(n, dtype=np.int32)[::-1].copy()                           # a descending map with three unmapped bins
    m[[4, 17, 30]] = -1
    bm = np.stack([m, m])
    alt, ref = pairs(np.random.RandomState(1), 2, n, cuda)
    alt, ref = alt.contiguous(), ref.contiguous()
    clean = engine.screen_paired_aligned_scores(ctx, alt, ref, bm)
    # unmapped pairs: an alt row, an alt column, and the reference rows / columns no alt bin stands for (reference bin 49 - 4 = 45, ..)
    a2, r2 = alt.clone(), ref.clone()
    a2[0, 4, :] = float("nan")
    a2[1, :, 17] = float("nan")
    a2[0, 30, 30] = float("inf")
    r2[0, 45, :] = float("nan")
    r2[1, :, 19] = float("nan")
    quiet = engine.screen_paired_aligned_scores(ctx, a2, r2, bm)
    assert all(same_bits(quiet[f], clean[f]) for f in FIELDS) and torch.equal(quiet["count"], clean["count"])
    # one mapped pair of pair 1, alt (12, 33): its scalars and row 12 of its profile; pair 0 and every other row keep their bits
    for where in ("alt", "ref"):
        a3, r3 = alt.clone(), ref.clone()
        if where == "alt":
            a3[1, 12, 33] = float("nan")
        else:
            r3[1, 49 - 12, 49 - 33] = float("nan")                          # the reference pixel alt (12, 33) stands for
        got = engine.screen_paired_aligned_scores(ctx, a3, r3, bm)
        check(got, sv.paired_aligned_scores_host(a3.cpu().numpy(), r3.cpu().numpy(), bm), where)
        for f in SCALARS:
            assert torch.isnan(got[f][1]) and same_bits(got[f][0], clean[f][0]), (where, f)
        keep = torch.ones(n, dtype=torch.bool, device=cuda)
        keep[12] = False
        assert torch.isnan(got["profile"][1, 12]) and same_bits(got["profile"][1, keep], clean["profile"][1, keep]) and same_bits(got["profile"][0], clean["profile"][0])
        assert int(torch.isnan(got["profile"][1]).sum()) == 4


def test_bad_arguments_are_refused_before_any_launch(cuda):
    """Every call below is refused by the host entry point's checks, so nothing of it reaches a kernel; the output buffers keep their fill."""
    lib = _lib.load()
    h = engine.get_context(cuda).handle
    null = ctypes.c_void_p(0)
    n, B = 6, 2
    alt = torch.zeros((B, n, n), dtype=torch.float32, device=cuda)
    ref = torch.zeros((B, n, n), dtype=torch.float32, device=cuda)
    dev = torch.zeros(B * 257, dtype=torch.int32, device=cuda)                  # stands for the device bin map: never read
    o32 = [torch.full((B * 257,), 7.0, dtype=torch.float32, device=cuda) for _ in range(5)]
    o64 = torch.full((B,), 7.0, dtype=torch.float64, device=cuda)
    cnt = torch.full((B,), 7, dtype=torch.int32, device=cuda)
    good = np.ascontiguousarray([[0, 1, -1, 2, 3, 5], [5, 4, 3, -1, 1, 1]], dtype=np.int32)
    big = np.zeros((B, 257), dtype=np.int32)

    def call(bm=good, a=_dp(alt), r=_dp(ref), bm_dev=_dp(dev), host=True, nb=B, nn=n, abs_=n * n, rbs=n * n, pr=_dp(o32[0]), am=_dp(o32[1]), ax=_dp(o32[2]),
             dm=_dp(o32[3]), rm=_dp(o32[4]), co=_dp(o64), ct=_dp(cnt)):
        return lib.orca_screen_paired_aligned_scores(h, a, abs_, r, rbs, nb, nn, bm_dev, _hp(bm) if host else null, pr, am, ax, dm, rm, co, ct)
    assert call() == 0                                                          # the well-formed call is accepted (and overwrites the fill: refilled below)
    torch.cuda.synchronize()
    for o in o32:
        o.fill_(7.0)
    o64.fill_(7.0)
    cnt.fill_(7)
    _refused(call(nn=0))
    _refused(call(nn=257, abs_=257 * 257, rbs=257 * 257, bm=big))
    _refused(call(nb=0))
    _refused(call(nb=-1))
    assert ">= n * n" in _refused(call(abs_=n * n - 1))                        # a stride below n^2, either map
    assert ">= n * n" in _refused(call(rbs=n * n - 1))
    bad = good.copy()
    bad[1, 4] = n
    assert "outside -1" in _refused(call(bm=bad))                               # a bin-map entry of n
    bad[1, 4] = -2
    assert "outside -1" in _refused(call(bm=bad))
    assert "NULL" in _refused(call(host=False))
    for k in ("a", "r", "bm_dev", "pr", "am", "ax", "dm", "rm", "co", "ct"):
        assert "NULL" in _refused(call(**{k: null})), k
    assert "NULL" in _refused(lib.orca_screen_paired_aligned_scores(null, _dp(alt), n * n, _dp(ref), n * n, B, n, _dp(dev), _hp(good), *(_dp(o) for o in o32), _dp(o64),
                                                                   _dp(cnt)))
    torch.cuda.synchronize()
    assert all(bool((o == 7).all()) for o in o32 + [o64, cnt])
    # the wrapper turns the same refusals into errors
    ctx = engine.get_context(cuda)
    with pytest.raises(OrcaHipError):
        engine.screen_paired_aligned_scores(ctx, alt, ref, bad)
    with pytest.raises(ValueError):
        engine.screen_paired_aligned_scores(ctx, alt, ref, good[:1])
    with pytest.raises(ValueError):
        engine.screen_paired_aligned_scores(ctx, alt, ref[:1], good)
    with pytest.raises(ValueError):
        engine.screen_paired_aligned_scores(ctx, alt[:0], ref[:0], good[:0])
    with pytest.raises(ValueError):
        engine.screen_paired_aligned_scores(ctx, alt.transpose(1, 2), ref, good)


# ---- the screen ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def case(cuda):
    g = torch.Generator(device=cuda).manual_seed(11)
    genome = torch.randint(0, 4, (CHR,), device=cuda, generator=g, dtype=torch.uint8)
    genome[7_000_000:7_003_000] = 4                                     # an N run inside the windows
    model = orca_models.H1esc(synthetic_seed=0)
    scored = sv.sv_screen([model], genome, VARIANTS, CHR, min_uses=1, scores=True)
    return model, genome, scored


def dict_maps(out, m=0):
    """model m's maps of an output dict as [6, C, 250, 250]"""
    return np.stack([np.asarray(p).reshape(-1, 250, 250) for p in out["predictions"][m]])


def equals_host(entry, what):
    """an entry's scores against the restatement on the entry's own maps, and its bin maps against `level_bin_maps`"""
    s = entry["scores"]
    assert sorted(s) == ["bin_map", "count", "junction_bins", "models"] and len(s["models"]) == len(entry["alt"]["predictions"])
    bm = sv.level_bin_maps(entry["sv"], CHR, entry["ref"], entry["alt"])
    assert s["bin_map"].dtype == np.int32 and np.array_equal(s["bin_map"], bm)
    assert s["count"].dtype == np.int32 and np.array_equal(s["count"], (bm >= 0).sum(axis=1))
    assert np.array_equal(s["junction_bins"], sv.junction_bins(entry["sv"], CHR, entry["alt"]))
    for m, got in enumerate(s["models"]):
        assert sorted(got) == sorted(FIELDS)
        alt, ref = dict_maps(entry["alt"], m), dict_maps(entry["ref"], m)
        C = alt.shape[1]
        want = sv.paired_aligned_scores_host(alt.reshape(6 * C, 250, 250), ref.reshape(6 * C, 250, 250), np.repeat(bm, C, axis=0))
        assert np.array_equal(want["count"].reshape(6, C), np.repeat(s["count"][:, None], C, axis=1))
        for k in SCALARS:
            assert got[k].shape == (6, C), (what, m, k)
        assert got["profile"].shape == (6, C, 250)
        flat = {k: got[k].reshape((6 * C, 250) if k == "profile" else (6 * C,)) for k in FIELDS}
        flat["count"] = want["count"]
        check(flat, want, (what, m))


def scores_same_bits(x, y):
    return (all(np.array_equal(x[k], y[k]) for k in ("bin_map", "count", "junction_bins")) and len(x["models"]) == len(y["models"])
            and all(same_bits(a[k], b[k]) for a, b in zip(x["models"], y["models"]) for k in FIELDS))


def test_screen_scores_equal_the_host_restatement(case):
    """Printed, not asserted (the weights are synthetic): abs_mean and 1 - corr per level of every variant."""
    model, genome, scored = case
    assert sorted(scored) == list(range(len(VARIANTS)))
    for i, v in enumerate(VARIANTS):
        e = scored[i]
        assert sorted(e) == ["alt", "ref", "scores", "sv"] and e["sv"] == v
        equals_host(e, v)
        print(v, "count", e["scores"]["count"].tolist(), "abs_mean", [f"{x:.4f}" for x in e["scores"]["models"][0]["abs_mean"][:, 0]],
              "1 - corr", [f"{1 - x:.3e}" for x in e["scores"]["models"][0]["corr"][:, 0]])
    counts = [scored[i]["scores"]["count"].tolist() for i in range(len(VARIANTS))]
    assert counts[0] == [240, 232, 212, 175, 100, 0] and counts[2] == [250, 250, 250, 250, 248, 248] and counts[4] == [244, 238, 224, 200, 150, 50]
    zero = scored[0]["scores"]["models"][0]                             # the 1.2 Mb deletion's finest level: no locus in common, NaN scores
    assert all(np.isnan(zero[k][5]).all() for k in FIELDS) and all(np.isfinite(zero[k][:5]).all() for k in SCALARS)
    assert (scored[0]["scores"]["junction_bins"][:, 0] == [125, 126, 126, 126, 126, 126]).all()


def test_scores_change_nothing_else_and_maps_can_stay_on_the_device(case):
    model, genome, scored = case
    plain = sv.sv_screen([model], genome, VARIANTS, CHR, min_uses=1)
    bare = sv.sv_screen([model], genome, VARIANTS, CHR, min_uses=1, scores=True, keep_maps=False)
    for i in range(len(VARIANTS)):
        assert sorted(plain[i]) == ["alt", "ref", "sv"]
        for allele in ("ref", "alt"):
            a, b, c = plain[i][allele], scored[i][allele], bare[i][allele]
            assert sorted(a) == sorted(b) == sorted(c)
            for k in ("start_coords", "end_coords", "chr", "experiments", "annos"):
                assert a[k] == b[k] == c[k], k
            assert c["predictions"] is None and len(c["normmats"]) == 1 and all(np.array_equal(x, y) for x, y in zip(c["normmats"][0], b["normmats"][0]))
            for j in range(6):
                assert np.array_equal(a["predictions"][0][j], b["predictions"][0][j]), (i, allele, j)
        assert scores_same_bits(bare[i]["scores"], scored[i]["scores"]), i
    with pytest.raises(ValueError):
        sv.sv_screen([model], genome, VARIANTS[:1], CHR, keep_maps=False)


def test_scores_do_not_depend_on_the_group_or_the_streams(case):
    model, genome, scored = case
    got = {}
    sv.sv_screen([model], genome, VARIANTS[:3], CHR, min_uses=1, group=1, scores=True, keep_maps=False, on_result=lambda i, e: got.__setitem__(i, e))
    three = sv.sv_screen([model], genome, VARIANTS[:3], CHR, min_uses=1, group=3, streams=0, scores=True, rank=0, world=1)
    for i in range(3):
        assert scores_same_bits(got[i]["scores"], scored[i]["scores"]) and scores_same_bits(three[i]["scores"], scored[i]["scores"]), i
    half = sv.sv_screen([model], genome, VARIANTS, CHR, min_uses=1, scores=True, keep_maps=False, rank=1, world=2)
    assert half and all(scores_same_bits(e["scores"], scored[i]["scores"]) for i, e in half.items()) and len(half) < len(VARIANTS)


def test_scores_of_a_unit_redone_in_the_range_safe_arithmetic_are_those_of_its_final_maps(case, monkeypatch):
    """The forced retry of tests/test_gpu_sv_incremental.py (the pool reports a raised fp16-range flag once, for the second variant's encodes):
    that unit's maps are recomputed, and its scores come from the recomputed maps - the restatement on the returned maps; the others' bits stay."""
    model, genome, scored = case
    calls = {"n": 0}
    real = engine.ContextPool.take_overflow

    def fake(self):
        calls["n"] += 1
        return bool(real(self)) or calls["n"] == 2
    monkeypatch.setattr(engine.ContextPool, "take_overflow", fake)
    with pytest.warns(UserWarning, match="fp16 range"):
        redo = sv.sv_screen([model], genome, VARIANTS[:3], CHR, min_uses=1, streams=4, group=1, scores=True)
    for i in range(3):
        equals_host(redo[i], ("retry", i))
        same = scores_same_bits(redo[i]["scores"], scored[i]["scores"])
        assert same == (i != 1) and np.array_equal(redo[i]["alt"]["predictions"][0][0], scored[i]["alt"]["predictions"][0][0]) == (i != 1), i


def test_sv_scores_of_two_genomepredict_calls(case, cuda):
    """`incremental=False` scores the returned host maps through `sv_scores`: the restatement on those maps, and as close to the incremental
    screen's scores as the maps are.  With da, dr the largest differences of an alt and of a reference pixel between the two calls at a level
    (measured here; tests/test_gpu_sv_incremental.py caps each at 2e-5), every dl = x - y moves by at most da + dr and so does their mean of
    absolute values; each side rounds it to fp32 once (half an ulp each, RTOL covers both): |abs_mean difference| <= da + dr + RTOL |abs_mean|."""
    model, genome, scored = case
    full = sv.sv_screen([model], genome, VARIANTS, CHR, incremental=False, scores=True)
    for i, v in enumerate(VARIANTS):
        equals_host(full[i], ("full", v))
        again = sv.sv_scores(v, full[i]["ref"], full[i]["alt"], CHR, cuda)
        assert scores_same_bits(again, full[i]["scores"])
        assert np.array_equal(full[i]["scores"]["bin_map"], scored[i]["scores"]["bin_map"])
        for j in range(6):
            da = float(np.abs(full[i]["alt"]["predictions"][0][j] - scored[i]["alt"]["predictions"][0][j]).max())
            dr = float(np.abs(full[i]["ref"]["predictions"][0][j] - scored[i]["ref"]["predictions"][0][j]).max())
            assert da <= 2e-5 and dr <= 2e-5
            x, y = full[i]["scores"]["models"][0]["abs_mean"][j, 0], scored[i]["scores"]["models"][0]["abs_mean"][j, 0]
            if scored[i]["scores"]["count"][j] == 0:
                assert np.isnan(x) and np.isnan(y)
            else:
                print(v, "level", j, "abs_mean", float(x), float(y), "da", da, "dr", dr)
                assert abs(float(x) - float(y)) <= da + dr + RTOL * abs(float(y)), (v, j, x, y, da, dr)
    lean = sv.sv_screen([model], genome, VARIANTS[:1], CHR, incremental=False, scores=True, keep_maps=False)
    assert lean[0]["ref"]["predictions"] is None and lean[0]["alt"]["predictions"] is None and scores_same_bits(lean[0]["scores"], full[0]["scores"])
    with pytest.raises(ValueError):
        sv.sv_scores(VARIANTS[0], lean[0]["ref"], lean[0]["alt"], CHR, cuda)


def test_an_allele_equal_to_the_reference_scores_zero(case, cuda):
    """The reference allele against itself through the identity map (alt_out == ref_out, no variant: an empty deletion): abs_max == 0 and
    corr == 1.0 exactly - X, Y and C are the same bits where the two maps are."""
    model, genome, scored = case
    ref = scored[1]["ref"]
    none = sv.SV("del", 20_000_000, 20_000_000)
    s = sv.sv_scores(none, ref, ref, CHR, cuda)
    assert np.array_equal(s["bin_map"], np.tile(np.arange(250, dtype=np.int32), (6, 1))) and s["count"].tolist() == [250] * 6
    got = s["models"][0]
    assert (got["abs_max"] == 0).all() and (got["abs_mean"] == 0).all() and (got["rms"] == 0).all() and (got["delta_mean"] == 0).all() and (got["profile"] == 0).all()
    assert (got["corr"] == 1.0).all()
    flat = {"predictions": [[np.full((250, 250), 0.25, dtype=np.float32)] * 6], "start_coords": ref["start_coords"]}
    assert np.isnan(sv.sv_scores(none, flat, flat, CHR, cuda)["models"][0]["corr"]).all()          # X == 0: no correlation


def test_two_models_and_a_two_target_model(case, cuda):
    """Units of the screen are (variants, model): every model's scores, in model order, [6, C] / [6, C, 250] for a model of C targets; every
    channel equals the restatement on its own maps, and a model's scores do not depend on the models beside it."""
    from orca_amd import orca_leukemia
    model, genome, scored = case
    two = orca_leukemia.OrcaLeukemiaA(synthetic_seed=4)
    got = sv.sv_screen([model, two], genome, VARIANTS[:2], CHR, min_uses=1, scores=True)
    for i in range(2):
        ms = got[i]["scores"]["models"]
        assert len(ms) == 2 and ms[0]["corr"].shape == (6, 1) and ms[1]["corr"].shape == (6, 2) and ms[1]["profile"].shape == (6, 2, 250)
        assert got[i]["alt"]["predictions"][1][0].shape == (2, 250, 250)
        equals_host(got[i], ("two models", i))
        assert all(same_bits(ms[0][k], scored[i]["scores"]["models"][0][k]) for k in FIELDS)
        assert not same_bits(ms[1]["abs_mean"][:, 0], ms[1]["abs_mean"][:, 1])
    bare = sv.sv_screen([model, two], genome, VARIANTS[:2], CHR, min_uses=1, scores=True, keep_maps=False)
    for i in range(2):
        assert bare[i]["alt"]["predictions"] is None and len(bare[i]["alt"]["normmats"]) == 2 and scores_same_bits(bare[i]["scores"], got[i]["scores"])


def test_print_the_worst_error_over_tolerance():
    print("largest error / tolerance per field over this file's comparisons:", {k: f"{v:.3g}" for k, v in WORST.items()})
