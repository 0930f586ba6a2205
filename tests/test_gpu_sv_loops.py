"""Loops per level of the SV screen on the MI355X (orca_screen_paired_dot_follow; sv.sv_screen(..., scores=True, loops=), sv.sv_scores).

The kernel alone: random fp32 maps, their enrichment maps and reference dot lists from the device's own `engine.screen_dot_calls` (threshold -1e30
fills the lists), hand-made bin maps - identity, a jump, a repeated segment, a descending segment, holes, a descending map with holes, and a
degenerate one (first half -> one bin, second half -> another) with a hand-made reference dot on those two bins - and hand-made list slots
(-1, ri >= rj, 9999, rj = n).  Every output equals `sv.paired_dot_follow_host` on the same device e map EXACTLY: the kernel only compares and
subtracts once in fp32, so there is no tolerance - integers equal, floats bit for bit, NaN in the same places.  Then: ``enrich`` holds the bits of
``alt_e`` at ``at``; overwriting every non-candidate pixel with 1e30 changes nothing; a pair's outputs do not depend on B, its place in the batch or
the batch stride; every malformed call is refused before any launch.

The screen: the first three variants of tests/test_gpu_sv_incremental.py (a deletion, a duplication, an inversion; synthetic H1esc), every field of
an entry against the engine calls and the host matching on the entry's own kept maps, bit for bit, with the maps kept or not, incremental or not,
and through `sv_scores`."""
import ctypes

import numpy as np
import pytest
import torch

from orca_amd import _lib, engine, orca_models, screen, sv
from orca_amd._lib import OrcaHipError
from tests.test_gpu_screen_aligned import _dp, _hp, _refused
from tests.test_gpu_sv_incremental import CHR, VARIANTS
from tests.test_gpu_sv_scores import FIELDS as OLD_FIELDS
from tests.test_gpu_sv_scores import bits, dict_maps, same_bits, scores_same_bits

pytestmark = pytest.mark.gpu

SHAPES = [(10, 1), (22, 3), (40, 5), (250, 2)]                              # n = 10 = 4 w + 2: the smallest map with an eligible pixel at w = 2
FOLLOW = ("candidates", "at", "enrich", "delta")


def params_of(n):
    return screen.check_loops(screen.LoopParams(p=0, w=2, r=1, threshold=-1e30, max_calls=12) if n < 250 else screen.LoopParams(threshold=-1e30), n)


def _np(t):
    return t.cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)


def segment(n):
    """the reference bins [s0, s1) that the map "repeat" holds twice"""
    return n // 4, n // 4 + max(2, 2 * n // 5)


def follow_maps(n):
    """name -> bin map [n]"""
    i = np.arange(n)
    s0, s1 = segment(n)
    down = i.copy()
    down[n // 4: 3 * n // 4] = down[n // 4: 3 * n // 4][::-1]
    holes = i.copy()
    holes[np.random.RandomState(n).rand(n) < 0.2] = -1
    down_holes = np.where(holes >= 0, n - 1 - i, -1)
    deg = np.where(i < n // 2, n // 4, n // 2 + 1)
    return {"identity": i, "jump": np.where(i < n // 3, i, np.where(i + max(1, n // 8) < n, i + max(1, n // 8), -1)),
            "repeat": np.concatenate([i[:s1], i[s0:s1], i[s1:]])[:n], "down": down, "holes": holes, "down_holes": down_holes, "degenerate": deg}


def device_case(ctx, cuda, n, names, seed, e_pad=0):
    """For the bin maps ``names``: (alt_e [G, n, n] on the device with batch stride n * n + e_pad, ref_ij, ref_enrich on the device, bin maps, q).  The
    lists are the device's calls on random reference maps, with hand-made slots: the last five are 9999 / i == j / -1 / ri > rj / rj == n, slot 1 is
    the dot (w, n - 1 - w), slots 2 and 3 are dots with both anchors resp. one anchor in the segment that "repeat" holds twice, and slot 0 of a
    degenerate pair is the dot on its two bins."""
    q = params_of(n)
    G = len(names)
    maps = follow_maps(n)
    bm = np.stack([maps[k] for k in names]).astype(np.int32)
    rs = np.random.RandomState(seed)
    alt = torch.from_numpy(rs.randn(G, n, n).astype(np.float32)).to(cuda)
    ref = torch.from_numpy(rs.randn(G, n, n).astype(np.float32)).to(cuda)
    args = (q.p, q.w, q.r, q.threshold, q.max_calls, q.d_min)
    ac, rc = engine.screen_dot_calls(ctx, alt, *args), engine.screen_dot_calls(ctx, ref, *args)
    assert int(rc["count"].min()) >= 1
    ij, en = rc["ij"].cpu().numpy().copy(), rc["enrich"].cpu().numpy().copy()
    K = q.max_calls
    ij[:, K - 5:] = np.array([[3, n], [5, 2], [-1, -1], [7, 7], [9999, 3]], dtype=np.int32)[None]
    s0 = segment(n)[0]
    ij[:, 1], en[:, 1] = (q.w, n - 1 - q.w), 0.25
    ij[:, 2], en[:, 2] = (s0, s0 + q.d_min), -0.125
    ij[:, 3], en[:, 3] = (q.w, s0 + q.d_min), 3.0
    for b, k in enumerate(names):
        if k == "degenerate":
            ij[b, 0], en[b, 0] = (n // 4, n // 2 + 1), -0.5
    e = ac["e_map"]
    if e_pad:
        buf = torch.full((G, n * n + e_pad), 1e30, dtype=torch.float32, device=cuda)
        e = buf.as_strided((G, n, n), (n * n + e_pad, n, 1))
        e.copy_(ac["e_map"])
    return e, torch.from_numpy(ij).to(cuda), torch.from_numpy(en).to(cuda), bm, q


def equal_exactly(got, want, what):
    for k in FOLLOW:
        g, w = _np(got[k]), _np(want[k])
        assert g.dtype == w.dtype and g.shape == w.shape, (what, k)
        if g.dtype == np.int32:
            assert np.array_equal(g, w), (what, k)
        else:
            assert np.array_equal(np.isnan(g), np.isnan(w)), (what, k, "NaN")
            f = ~np.isnan(w)
            assert np.array_equal(bits(g)[f], bits(w)[f]), (what, k)


def candidate_mask(ij, bm, q, n):
    """bool [B, n, n]: the pixels that are a candidate of some listed dot"""
    mask = np.zeros((ij.shape[0], n, n), dtype=bool)
    for b in range(ij.shape[0]):
        for ri, rj in ij[b]:
            if not 0 <= ri < rj <= n - 1:
                continue
            a, c = np.flatnonzero(bm[b] == ri), np.flatnonzero(bm[b] == rj)
            i, j = np.minimum(a[:, None], c[None, :]).ravel(), np.maximum(a[:, None], c[None, :]).ravel()
            ok = (i >= q.w) & (j <= n - 1 - q.w) & (j - i >= q.d_min)
            mask[b, i[ok], j[ok]] = True
    return mask


# ---- the kernel against the restatement -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,B", SHAPES)
def test_kernel_equals_the_host_restatement_exactly(cuda, n, B):
    ctx = engine.get_context(cuda)
    names = list(follow_maps(n))
    seen = set()
    for g0 in range(0, len(names), B):
        group = names[g0: g0 + B]
        e, ij, en, bm, q = device_case(ctx, cuda, n, group, 7000 * n + g0, e_pad=5 if g0 else 0)
        got = engine.screen_paired_dot_follow(ctx, e, ij, en, bm, q.w, q.d_min)
        G, K = len(group), q.max_calls
        assert tuple(got["candidates"].shape) == (G, K) and tuple(got["at"].shape) == (G, K, 2) and got["candidates"].dtype == torch.int32 and got["at"].dtype == torch.int32
        assert tuple(got["enrich"].shape) == (G, K) == tuple(got["delta"].shape) and got["enrich"].dtype == torch.float32 == got["delta"].dtype
        eh, ijh, enh = e.cpu().numpy(), ij.cpu().numpy(), en.cpu().numpy()
        want = sv.paired_dot_follow_host(eh, ijh, enh, bm, q)
        equal_exactly(got, want, (n, group))
        cand, at, enrich = _np(got["candidates"]), _np(got["at"]), _np(got["enrich"])
        # the hand-made empty slots, and `enrich` = the bits of alt_e at `at`
        assert not cand[:, K - 5:].any() and (at[:, K - 5:] == -1).all() and np.isnan(enrich[:, K - 5:]).all() and np.isnan(_np(got["delta"])[:, K - 5:]).all()
        assert np.array_equal(at[..., 0] >= 0, cand > 0) and np.array_equal(at[..., 1] >= 0, cand > 0)
        for b, k in np.argwhere(cand > 0):
            assert bits(enrich[b, k: k + 1])[0] == bits(eh[b, at[b, k, 0], at[b, k, 1]][None])[0], (n, group, b, k)
        seen.update(cand.ravel().tolist())
        for b, name in enumerate(group):
            if name == "degenerate" and n >= 22:
                m = candidate_mask(ijh[b: b + 1, :1], bm[b: b + 1], q, n)
                assert cand[b, 0] == m.sum() and (cand[b, 0] > 256 or n < 40)                  # n = 40: 314 candidates, more than one pass of any workgroup
            if name == "identity":
                assert (cand[b][(ijh[b, :, 0] >= 0) & (ijh[b, :, 0] < ijh[b, :, 1]) & (ijh[b, :, 1] < n)] == 1).all() and np.array_equal(at[b, 0], ijh[b, 0])
        # every pixel that is no candidate overwritten: nothing may change (a wrong min / max or stride would read one)
        mask = torch.from_numpy(candidate_mask(ijh, bm, q, n)).to(cuda)
        e2 = torch.where(mask, e, torch.full_like(e, 1e30))
        again = engine.screen_paired_dot_follow(ctx, e2.contiguous(), ij, en, bm, q.w, q.d_min)
        for k in FOLLOW:
            assert same_bits(again[k], got[k]), (n, group, k, "1e30")
    if n >= 22:                                                                 # deleted / ordinary / one anchor repeated / both (n = 22: one of the four is too near the diagonal)
        assert {0, 1, 2} <= seen and (4 in seen if n >= 40 else 3 in seen), seen


@pytest.mark.parametrize("n", [22, 40, 250])
def test_a_pairs_outputs_do_not_depend_on_the_batch(cuda, n):
    """A pair alone (contiguous e map) against the same pair as row 0, 1 and 2 of a batch of three with another batch stride, other pairs, lists and
    bin maps beside it - under every bin map: the same bits."""
    ctx = engine.get_context(cuda)
    names = list(follow_maps(n))
    e3, ij3, en3, bm3, q = device_case(ctx, cuda, n, ["repeat", "down_holes", "jump"], 31 * n, e_pad=9)
    assert e3.stride(0) == n * n + 9
    for name in names:
        e1, ij1, en1, bm1, _ = device_case(ctx, cuda, n, [name], 37 * n)
        alone = engine.screen_paired_dot_follow(ctx, e1, ij1, en1, bm1, q.w, q.d_min)
        for row in range(3):
            e3[row], ij3[row], en3[row] = e1[0], ij1[0], en1[0]               # the rows written earlier stay, as other pairs
            bm = bm3.copy()
            bm[:row + 1] = bm1[0]
            got = engine.screen_paired_dot_follow(ctx, e3, ij3, en3, bm, q.w, q.d_min)
            for k in FOLLOW:
                assert same_bits(got[k][row], alone[k][0]), (name, row, k)


def test_bad_arguments_are_refused_before_any_launch(cuda):
    """Every call below is refused by the host entry point's checks, so nothing of it reaches a kernel; the output buffers keep their fill."""
    lib = _lib.load()
    h = engine.get_context(cuda).handle
    null = ctypes.c_void_p(0)
    n, B, R = 12, 2, 3
    e = torch.zeros((B, n, n), dtype=torch.float32, device=cuda)
    ij = torch.full((B, 4097, 2), -1, dtype=torch.int32, device=cuda)
    en = torch.zeros((B, 4097), dtype=torch.float32, device=cuda)
    dev = torch.zeros(B * 257, dtype=torch.int32, device=cuda)                  # stands for the device bin map
    oi = [torch.full((B * 4097 * 2,), 7, dtype=torch.int32, device=cuda) for _ in range(2)]
    of = [torch.full((B * 4097,), 7.0, dtype=torch.float32, device=cuda) for _ in range(2)]
    good = np.ascontiguousarray([list(range(n)), [-1] * n], dtype=np.int32)
    big = np.zeros((B, 257), dtype=np.int32)

    def call(bm=good, nb=B, nn=n, ebs=n * n, w=2, d_min=5, nr=R, host=True, **p):
        a = dict(e=_dp(e), ij=_dp(ij), en=_dp(en), md=_dp(dev), cand=_dp(oi[0]), at=_dp(oi[1]), enrich=_dp(of[0]), delta=_dp(of[1]), ctx=h)
        a.update(p)
        return lib.orca_screen_paired_dot_follow(a["ctx"], a["e"], ebs, nb, nn, w, d_min, a["ij"], a["en"], nr, a["md"], _hp(bm) if host else null, a["cand"], a["at"],
                                                 a["enrich"], a["delta"])
    assert call() == 0                                                          # the well-formed call is accepted (and overwrites the fill: refilled below)
    torch.cuda.synchronize()
    assert not oi[0][: B * R].any() and (oi[1][: B * R * 2] == -1).all() and bool(torch.isnan(of[0][: B * R]).all())
    for o in oi:
        o.fill_(7)
    for o in of:
        o.fill_(7.0)
    for k in ("ctx", "e", "ij", "en", "md", "cand", "at", "enrich", "delta"):
        assert "NULL" in _refused(call(**{k: null})), k
    assert "NULL" in _refused(call(host=False))
    _refused(call(nb=0))
    _refused(call(nb=-1))
    _refused(call(nn=0))
    _refused(call(nn=257, ebs=257 * 257, bm=big))
    assert ">= n * n" in _refused(call(ebs=n * n - 1))
    for w in (0, 17, -1):
        assert "half-width" in _refused(call(w=w, d_min=40))
    assert "d_min" in _refused(call(d_min=4)) and "d_min" in _refused(call(w=16, d_min=32))
    for nr in (0, 4097, -1):
        assert "R = " in _refused(call(nr=nr))
    for x in (n, -2):
        bad = good.copy()
        bad[1, 4] = x
        assert "outside -1" in _refused(call(bm=bad))
    torch.cuda.synchronize()
    assert all(bool((o == 7).all()) for o in oi + of)
    # the wrapper turns the same refusals into errors
    ctx = engine.get_context(cuda)
    with pytest.raises(OrcaHipError):
        engine.screen_paired_dot_follow(ctx, e, ij[:, :R].contiguous(), en[:, :R].contiguous(), good, 2, 4)
    with pytest.raises(OrcaHipError):
        engine.screen_paired_dot_follow(ctx, e, ij.contiguous(), en.contiguous(), good, 2)
    with pytest.raises(ValueError):
        engine.screen_paired_dot_follow(ctx, e, ij[:1, :R].contiguous(), en[:1, :R].contiguous(), good, 2)
    with pytest.raises(ValueError):
        engine.screen_paired_dot_follow(ctx, e, ij[:, :R].contiguous(), en[:, :R].contiguous(), good[:1], 2)
    with pytest.raises(OrcaHipError):
        engine.screen_paired_dot_follow(ctx, e.cpu(), ij[:, :R].contiguous(), en[:, :R].contiguous(), good, 2)


# ---- the screen ---------------------------------------------------------------------------------------------------------------------------------------
THREE = VARIANTS[:3]                                                        # a deletion, a duplication, an inversion
K_SMALL = 5
TOP_KEYS = ["bin_map", "count", "junction_bins", "loop_params", "models"]
LOOP_FIELDS = sv.LOOP_SCORE_FIELDS


@pytest.fixture(scope="module")
def case(cuda):
    """(model, genome, q, looped, filled): ``filled`` = the screen with threshold -1e30 and K = 5 (every list truncated); ``q``'s threshold is chosen
    from the device e map of variant 0's 32 Mb reference level, the midpoint between the 8th and the 9th largest local-maximum enrichment: being a
    local maximum does not depend on the threshold, so that level has exactly 8 dots; ``looped`` = the screen with q."""
    g = torch.Generator(device=cuda).manual_seed(11)
    genome = torch.randint(0, 4, (CHR,), device=cuda, generator=g, dtype=torch.uint8)
    genome[7_000_000:7_003_000] = 4                                     # an N run inside the windows
    model = orca_models.H1esc(synthetic_seed=0)
    fill = screen.LoopParams(threshold=-1e30, max_calls=K_SMALL)
    filled = sv.sv_screen([model], genome, THREE, CHR, min_uses=1, scores=True, loops=fill)
    d = screen.LoopParams()
    ref0 = torch.from_numpy(dict_maps(filled[0]["ref"])[0, :1]).to(cuda)
    got = engine.screen_dot_calls(engine.get_context(cuda), ref0, d.p, d.w, d.r, -1e30, 4096)
    count = int(got["count"][0])
    assert 9 <= count <= 4096, count
    es = np.sort(got["enrich"][0, :count].cpu().numpy().astype(np.float64))[::-1]
    t = np.float32((es[7] + es[8]) / 2)
    assert es[7] >= t > es[8], (es[7], t, es[8])
    q = screen.LoopParams(threshold=float(t))
    looped = sv.sv_screen([model], genome, THREE, CHR, min_uses=1, scores=True, loops=q)
    assert looped[0]["scores"]["models"][0]["ref_loop_count"][0, 0] == 8
    return model, genome, q, looped, filled


def field_same(a, b):
    return (a.dtype == b.dtype and np.array_equal(a, b)) if a.dtype == np.bool_ else same_bits(a, b)


def loops_same_bits(x, y, old=True):
    return ((not old or scores_same_bits(x, y)) and sorted(x) == sorted(y) and x["loop_params"] == y["loop_params"] and len(x["models"]) == len(y["models"])
            and all(sorted(a) == sorted(b) and all(field_same(a[k], b[k]) for k in LOOP_FIELDS) for a, b in zip(x["models"], y["models"])))


def equals_engine(entry, q, cuda, what):
    """an entry's loop fields against the engine calls and the host matching on the entry's own maps: bit for bit"""
    ctx = engine.get_context(cuda)
    s = entry["scores"]
    qq = screen.check_loops(q, 250)
    assert sorted(s) == TOP_KEYS and s["loop_params"] == qq
    bm = sv.level_bin_maps(entry["sv"], CHR, entry["ref"], entry["alt"])
    assert np.array_equal(s["bin_map"], bm)
    K = qq.max_calls
    for m, got in enumerate(s["models"]):
        assert sorted(got) == sorted(OLD_FIELDS + LOOP_FIELDS)
        alt, ref = dict_maps(entry["alt"], m), dict_maps(entry["ref"], m)
        C = alt.shape[1]
        bmc = np.repeat(bm, C, axis=0)
        a, r = (torch.from_numpy(np.ascontiguousarray(x.reshape(6 * C, 250, 250))).to(cuda) for x in (alt, ref))
        args = (qq.p, qq.w, qq.r, qq.threshold, K, qq.d_min)
        ac, rc = engine.screen_dot_calls(ctx, a, *args), engine.screen_dot_calls(ctx, r, *args)
        fl = engine.screen_paired_dot_follow(ctx, ac["e_map"], rc["ij"], rc["enrich"], bmc, qq.w, qq.d_min)
        want = {"ref_loops": rc["ij"], "loops": ac["ij"], "ref_loop_enrichment": rc["enrich"], "loop_enrichment": ac["enrich"], "ref_loop_count": rc["count"],
                "loop_count": ac["count"], "loop_candidates": fl["candidates"], "loop_followed_at": fl["at"], "loop_followed_enrichment": fl["enrich"],
                "loop_delta": fl["delta"]}
        want = {k: _np(v) for k, v in want.items()}
        gl = [sv.paired_match_loops_host(want["loops"][b], want["ref_loops"][b], bmc[b], qq.tol) for b in range(6 * C)]
        want["loop_is_gained"], want["ref_loop_is_lost"] = np.stack([x[0] for x in gl]), np.stack([x[1] for x in gl])
        want["loops_gained"], want["loops_lost"] = (want[k].sum(axis=1).astype(np.int32) for k in ("loop_is_gained", "ref_loop_is_lost"))
        shapes = {"ref_loops": (K, 2), "loops": (K, 2), "loop_followed_at": (K, 2), "ref_loop_count": (), "loop_count": (), "loops_gained": (), "loops_lost": ()}
        for k in LOOP_FIELDS:
            dt = np.bool_ if "_is_" in k else (np.float32 if "enrichment" in k or k == "loop_delta" else np.int32)
            assert got[k].dtype == dt and got[k].shape == (6, C) + shapes.get(k, (K,)), (what, k)
            w = want[k].reshape(got[k].shape)
            assert np.array_equal(got[k], w) if dt == np.bool_ else same_bits(got[k], w), (what, m, k)
        # and the follow against the restatement on the device's e map
        host = sv.paired_dot_follow_host(_np(ac["e_map"]), want["ref_loops"], want["ref_loop_enrichment"], bmc, qq)
        equal_exactly({k: got[f].reshape(host[k].shape) for k, f in zip(FOLLOW, ("loop_candidates", "loop_followed_at", "loop_followed_enrichment", "loop_delta"))},
                      host, (what, m))
        listed = want["ref_loops"][..., 0] >= 0
        assert np.array_equal(listed.sum(axis=1), np.minimum(want["ref_loop_count"], K))
        assert not want["loop_candidates"][~listed].any() and not want["ref_loop_is_lost"][~listed].any()


def test_screen_loops_equal_the_engine_and_the_host_matching(case, cuda):
    """Printed, not asserted (the weights are synthetic): per variant and level (ref_loop_count, loop_count, loops_gained, loops_lost, max candidates)."""
    model, genome, q, looped, filled = case
    for res, qq, name in ((looped, q, "chosen"), (filled, screen.LoopParams(threshold=-1e30, max_calls=K_SMALL), "filled")):
        for i, v in enumerate(THREE):
            e = res[i]
            assert sorted(e) == ["alt", "ref", "scores", "sv"] and e["sv"] == v
            equals_engine(e, qq, cuda, (name, v))
            g = e["scores"]["models"][0]
            print(name, v, [(int(g["ref_loop_count"][k, 0]), int(g["loop_count"][k, 0]), int(g["loops_gained"][k, 0]), int(g["loops_lost"][k, 0]),
                             int(g["loop_candidates"][k, 0].max())) for k in range(6)])
    f0 = filled[0]["scores"]["models"][0]
    assert (f0["ref_loop_count"] > K_SMALL).all() and (f0["ref_loops"][..., 0] >= 0).all()          # truncated: every slot of every list holds a dot
    assert 3 <= looped[0]["scores"]["models"][0]["ref_loop_count"][0, 0] <= q.max_calls
    dup, inv = looped[1]["scores"], looped[2]["scores"]
    assert any(np.bincount(dup["bin_map"][k][dup["bin_map"][k] >= 0]).max() >= 2 for k in range(6))     # the duplication: some reference bin has two alt bins
    assert any((np.diff(inv["bin_map"][k][inv["bin_map"][k] >= 0]) < 0).any() for k in range(6))        # the inversion's maps do descend


def test_loops_change_nothing_else_and_maps_can_stay_on_the_device(case):
    model, genome, q, looped, filled = case
    plain = sv.sv_screen([model], genome, THREE, CHR, min_uses=1, scores=True)
    bare = sv.sv_screen([model], genome, THREE, CHR, min_uses=1, scores=True, keep_maps=False, loops=q)
    for i in range(3):
        assert sorted(plain[i]["scores"]) == ["bin_map", "count", "junction_bins", "models"] and sorted(plain[i]["scores"]["models"][0]) == sorted(OLD_FIELDS)
        assert scores_same_bits(plain[i]["scores"], looped[i]["scores"]) and scores_same_bits(plain[i]["scores"], filled[i]["scores"]), i
        for allele in ("ref", "alt"):
            assert bare[i][allele]["predictions"] is None
            for j in range(6):
                assert np.array_equal(plain[i][allele]["predictions"][0][j], looped[i][allele]["predictions"][0][j]), (i, allele, j)
        assert loops_same_bits(bare[i]["scores"], looped[i]["scores"]), i
    with pytest.raises(ValueError):
        sv.sv_screen([model], genome, THREE[:1], CHR, loops=True)
    with pytest.raises(ValueError):
        sv.sv_screen([model], genome, THREE[:1], CHR, scores=True, loops=screen.LoopParams(w=17))


def test_sv_scores_of_two_genomepredict_calls(case, cuda):
    model, genome, q, looped, filled = case
    full = sv.sv_screen([model], genome, THREE, CHR, incremental=False, scores=True, loops=q)
    for i, v in enumerate(THREE):
        equals_engine(full[i], q, cuda, ("full", v))
        again = sv.sv_scores(v, full[i]["ref"], full[i]["alt"], CHR, cuda, loops=q)
        assert loops_same_bits(again, full[i]["scores"])
        assert np.array_equal(full[i]["scores"]["bin_map"], looped[i]["scores"]["bin_map"])
        redo = sv.sv_scores(v, looped[i]["ref"], looped[i]["alt"], CHR, cuda, loops=q)             # two calls of the dot kernels instead of one: the same bits
        assert loops_same_bits(redo, looped[i]["scores"], old=False)


def test_an_allele_equal_to_the_reference_keeps_every_loop(case, cuda):
    model, genome, q, looped, filled = case
    ref = looped[0]["ref"]                                                    # (q gives its 32 Mb level 8 dots)
    none = sv.SV("del", 20_000_000, 20_000_000)
    for qq in (q, screen.LoopParams(threshold=-1e30, max_calls=K_SMALL)):
        s = sv.sv_scores(none, ref, ref, CHR, cuda, loops=qq)
        got = s["models"][0]
        listed = got["ref_loops"][..., 0] >= 0
        assert listed.any() and (got["loop_candidates"][listed] == 1).all() and not got["loop_candidates"][~listed].any()
        assert np.array_equal(got["loop_followed_at"], got["ref_loops"]) and same_bits(got["loop_followed_enrichment"], got["ref_loop_enrichment"])
        assert (got["loop_delta"][listed] == 0).all() and np.isnan(got["loop_delta"][~listed]).all()
        assert not got["loop_is_gained"].any() and not got["ref_loop_is_lost"].any() and not got["loops_gained"].any() and not got["loops_lost"].any()
        assert np.array_equal(got["loops"], got["ref_loops"]) and np.array_equal(got["loop_count"], got["ref_loop_count"])
