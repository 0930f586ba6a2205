"""-m gpu: every entry point that works inside the per-context workspace arena (and the edge-fix scratch slabs), run on an arena filled with
0x00, 0xFF, 0x3C and 0x7B (tests/arena.py; `engine.Context.fill_workspace`): the result must be finite, the same bits under every fill, and no fill may
raise the fp16-range flag.  The planar Encoder zeroes the guards and tails of every tensor BEHIND its producer (about twenty separate launches over
five stage-1 variants, the joint two-strand layout, the part hand-overs and the chunked path); one forgotten launch, or a kernel that reads one unit
past the zeroed tail, makes a result depend on what an earlier call left there - and a fresh allocation (what most tests meet: tests/conftest.py
releases the arenas after every module) is very often zero pages.

Every call goes to the engine layer directly, below the modules' range-guard retry: a flag raised by arena contents must be seen, not consumed.

Lengths: 12 000 bases (3 bins, n3 = 750: one ragged tile per launch everywhere, all ends within one tile), 264 000 (66 bins; n2 = 66 000 >= 65 536
puts the 96-cout layers on the 512-position kernels, several tiles per strand at stages 3-4, stage 5 on the short-row kernel) and 1 000 000
(n5 = 2 500 > 2 048: stages 5-6 on the tiled channel-last kernel; default arithmetic and the two-strand call only)."""
import functools

import numpy as np
import pytest
import torch

from orca_amd import _lib, engine
from orca_amd import screen as S
from orca_amd import selene_utils2 as SU
from orca_amd import synth
from orca_amd.genome import PackedGenome, TwoBitGenome
from tests import arena
from tests import decoder_ref as DR
from tests.arena import EDGE_BYTES, as_bits, assert_arena_independent, nan_outputs
from tests.encoder_ref import pack_p16
from tests.test_gpu_encoder_two_strands import _codes
from tests.util import product_module

pytestmark = pytest.mark.gpu

LENGTHS = (12_000, 264_000, 1_000_000)
ENC_PRECISIONS = ("f16x2", "bf16", "bf16x2", "bf16x3", "f32")
SENTINEL = 1234.5
NAN = float("nan")


# ---- the Encoder --------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def enc(cuda):
    return product_module("Encoder", 0, device=cuda)


def _net(enc, cuda, precision, form="default"):
    """The module's engine handle in ``precision`` and ``form`` (the `_net` / `_apply_precision` pattern of the stage tests)."""
    enc.form = form
    try:
        net = enc._net(cuda)
    finally:
        enc.form = "default"
    enc._apply_precision(net, precision)
    return net


def _bins_out(cuda, B, bins):
    return torch.full((B, 128, bins), NAN, dtype=torch.float32, device=cuda)


def _check_codes(net, cuda, codes, what, reverse=False, bin_lo=0, bin_hi=0, chunk_bp=0):
    B, L = codes.shape
    bins = (bin_hi if bin_hi > 0 else engine.encoder_num_bins(L)) - bin_lo

    def fn():
        return engine.encoder_forward_codes(net, codes, reverse, bin_lo, bin_hi, chunk_bp, out=_bins_out(cuda, B, bins))
    return assert_arena_independent(net.ctx, fn, what=what)


@pytest.mark.parametrize("L", LENGTHS[:2])
@pytest.mark.parametrize("reverse", (False, True))
@pytest.mark.parametrize("precision", ENC_PRECISIONS)
def test_encoder_from_codes(enc, cuda, precision, reverse, L):
    _check_codes(_net(enc, cuda, precision), cuda, _codes(L, L % 97, cuda), (precision, reverse, L), reverse)


@pytest.mark.parametrize("L", (8_000, 16_000))
@pytest.mark.parametrize("precision", ("f16x2", "bf16"))
def test_encoder_lengths_whose_last_pool5_tile_ends_past_its_planes(enc, cuda, precision, L):
    """n3 = 500 and 1 000: the last 320-position tile of stage 3's pooled conv (conv_p16p5.h) ends at unit 656 / 1 296 of planes of
    p16_plen(n3) = 544 / 1 056 units - its unstored lanes read the next plane and, behind the last plane, the rest of the arena buffer, and the
    range guard sees those lanes (12 000 and 264 000 bases keep that tile inside the plane).  Both strands, and the two-strand call."""
    codes = _codes(L, L % 97, cuda)
    net = _net(enc, cuda, precision)
    for reverse in (False, True):
        _check_codes(net, cuda, codes, (precision, reverse, L), reverse)
    bins = engine.encoder_num_bins(L)
    assert_arena_independent(net.ctx, lambda: engine.encoder_forward_two_strands(net, codes, _bins_out(cuda, 2, bins)), what=(precision, L, "two strands"))


@pytest.mark.parametrize("reverse", (False, True))
def test_encoder_from_codes_1mb(enc, cuda, reverse):
    L = LENGTHS[2]
    _check_codes(_net(enc, cuda, "f16x2"), cuda, _codes(L, L % 97, cuda), ("f16x2", reverse, L), reverse)


@pytest.mark.parametrize("precision", ENC_PRECISIONS)
def test_encoder_batch_of_two(enc, cuda, precision):
    L = LENGTHS[1]
    codes = torch.cat([_codes(L, 1, cuda), _codes(L, 2, cuda)])
    _check_codes(_net(enc, cuda, precision), cuda, codes, (precision, "B = 2"), reverse=True)


@pytest.mark.parametrize("L", LENGTHS[:2])
@pytest.mark.parametrize("precision", ("f16x2", "bf16"))
@pytest.mark.parametrize("form", sorted(_lib.ENCODER_FORMS))
def test_encoder_forms(enc, cuda, form, precision, L):
    """Every forced form of stage 1-3's linear groups: with the default they walk the five stage-1 variants (fuse1, stored first layer, compose,
    compose25, residual from the bases / the fused B16 stage) and both forms of stages 2-3."""
    codes = _codes(L, L % 97, cuda)
    for reverse in (False, True):
        _check_codes(_net(enc, cuda, precision, form), cuda, codes, (form, precision, reverse, L), reverse)


def _float_rows(codes):
    """[1, L] base codes -> [1, L, 4] float32 one-hot rows (N = 0.25 everywhere), contiguous"""
    table = torch.cat([torch.eye(4), torch.full((1, 4), 0.25)]).to(codes.device)
    return table[codes.long()].contiguous()


@pytest.mark.parametrize("L", LENGTHS[:2])
@pytest.mark.parametrize("layout", ("flat", "strided"))
@pytest.mark.parametrize("form", ("default", "two_conv"))
@pytest.mark.parametrize("precision", ("f16x2", "f32"))
def test_encoder_from_float_rows(enc, cuda, precision, form, layout, L):
    """`engine.encoder_forward`: the transposed view of [1, L, 4] is the flat path; a contiguous [1, 4, L] the strided one - gathered by
    seq_to_rows_kernel into buf[kS], or (two-conv form on P16 planes) read by conv1d_first_p16_kernel."""
    rows = _float_rows(_codes(L, L % 97, cuda))
    x = rows.transpose(1, 2)
    if layout == "strided":
        x = x.contiguous()
    assert (x.stride(1) == 1) == (layout == "flat")
    net = _net(enc, cuda, precision, form)
    bins = engine.encoder_num_bins(L)
    assert_arena_independent(net.ctx, lambda: engine.encoder_forward(net, x, out=_bins_out(cuda, 1, bins)), what=(precision, form, layout, L))


@pytest.mark.parametrize("L", LENGTHS[:2])
@pytest.mark.parametrize("precision", ("f16x2", "bf16"))
def test_encoder_from_the_two_bit_genome(enc, cuda, precision, L):
    g = TwoBitGenome.from_packed(PackedGenome.random({"chrA": 300_003}, seed=4, n_runs=5)).to(cuda)
    two, nmask = g.planes("chrA")
    net = _net(enc, cuda, precision)
    bins = engine.encoder_num_bins(L)
    for reverse in (False, True):
        assert_arena_independent(net.ctx, lambda: engine.encoder_forward_2bit(net, two, nmask, 4001, L, reverse, out=_bins_out(cuda, 1, bins)),
                                 what=(precision, L, reverse))


@pytest.mark.parametrize("precision", ("f16x2", "bf16", "bf16x3"))
def test_encoder_bin_range(enc, cuda, precision):
    L = LENGTHS[1]
    codes = _codes(L, L % 97, cuda)
    for reverse in (False, True):
        _check_codes(_net(enc, cuda, precision), cuda, codes, (precision, reverse, "bins 11..29"), reverse, bin_lo=11, bin_hi=29)


@pytest.mark.parametrize("precision", ENC_PRECISIONS)
def test_encoder_chunked(enc, cuda, precision):
    """264 000 bases in chunks of 100 000 (three chunks with their 112 kb halos) and whole: each chunking on its own is bit-identical across the
    fills (the two chunkings tile the sequence differently and are not compared with each other)."""
    L = LENGTHS[1]
    codes = _codes(L, L % 97, cuda)
    net = _net(enc, cuda, precision)
    for chunk_bp in (100_000, 0):
        _check_codes(net, cuda, codes, (precision, "chunk", chunk_bp), chunk_bp=chunk_bp)
        _check_codes(net, cuda, codes, (precision, "chunk", chunk_bp, "reverse"), reverse=True, chunk_bp=chunk_bp)


@pytest.mark.parametrize("L", LENGTHS)
@pytest.mark.parametrize("joint", (True, False))
@pytest.mark.parametrize("precision", ("f16x2", "bf16"))
def test_encoder_two_strands(enc, cuda, precision, joint, L):
    """`engine.encoder_forward_two_strands` with the joint pass (one set of planes for both strands, a zero gap between them) on and off"""
    net = _net(enc, cuda, precision)
    codes = _codes(L, L % 97, cuda)
    bins = engine.encoder_num_bins(L)
    net.set_encoder_two_strands(joint)
    try:
        assert_arena_independent(net.ctx, lambda: engine.encoder_forward_two_strands(net, codes, _bins_out(cuda, 2, bins)), what=(precision, L, joint))
    finally:
        net.set_encoder_two_strands(True)


# ---- the Encoder's parts (f16x2; inputs as test_gpu_encoder_stages.py builds them) ---------------------------------------------------------------
def _part_codes(L, seed, cuda):
    return _codes(L, seed, cuda)[0].contiguous()


def _sentinel(cuda, *shape):
    return torch.full(shape, SENTINEL, dtype=torch.float32, device=cuda)


@pytest.mark.parametrize("L", (16 * 515, 264_000))
def test_part_stage3_planes(enc, cuda, L):
    net = _net(enc, cuda, "f16x2")
    codes = _part_codes(L, 3, cuda)
    for reverse in (False, True):
        assert_arena_independent(net.ctx, lambda: engine.encoder_stage3_planes(net, codes, reverse), what=("stage3_planes", L, reverse))


@pytest.fixture(scope="module")
def s4_planes(cuda):
    """a stage-4 input of 500 positions as P16 planes (values as a pooled stage 3 has them: non-negative, O(1)), zero guards and tail"""
    v = (np.random.RandomState(31).rand(500, 128) * 2.0).astype(np.float32)
    return torch.from_numpy(pack_p16(v, engine.p16_plane_units(500))).to(cuda)


def test_part_front_snippet(enc, cuda):
    net = _net(enc, cuda, "f16x2")
    L, n_dst = 12_000, 90
    codes = _part_codes(L, 21, cuda)
    units = engine.p16_plane_units(n_dst)
    for reverse in (False, True):
        for base0, nbases, skip, count, dst_pos0 in [(0, 4000, 0, 50, 0), (2416, 3200, 3, 37, 53), (L - 4800, 4800, 20, 40, n_dst - 40)]:
            def fn():
                dst = _sentinel(cuda, 32, units, 4)
                engine.encoder_front_snippet(net, codes, reverse, base0, nbases, skip, count, dst, dst_pos0)
                return dst
            assert_arena_independent(net.ctx, fn, what=("front_snippet", reverse, base0))


def test_part_back_and_stage4_rows(enc, cuda, s4_planes):
    net = _net(enc, cuda, "f16x2")

    def back():
        return engine.encoder_back(net, s4_planes, 500, torch.full((128, 10), NAN, dtype=torch.float32, device=cuda))
    assert_arena_independent(net.ctx, back, what="back")
    assert_arena_independent(net.ctx, lambda: engine.encoder_stage4_rows(net, s4_planes, 500), what="stage4_rows")


def test_part_front4(enc, cuda):
    net = _net(enc, cuda, "f16x2")
    L, n_dst = 24_000, 60
    codes = _part_codes(L, 22, cuda)
    run = _part_codes(16_000, 23, cuda)
    ranges = [(0, 6, 0), (34, 6, n_dst - 6)]
    for reverse in (False, True):
        for base0, nbases, skip, count, dst_pos0 in [(0, 8000, 0, 20, 0), (4000, 8000, 2, 15, 5), (L - 9200, 9200, 3, 20, n_dst - 20)]:
            def snippet():
                dst = _sentinel(cuda, n_dst, 128)
                engine.encoder_front4_snippet(net, codes, reverse, base0, nbases, skip, count, dst, dst_pos0)
                return dst
            assert_arena_independent(net.ctx, snippet, what=("front4_snippet", reverse, base0))

        def two_ranges():
            dst = _sentinel(cuda, n_dst, 128)
            engine.encoder_front4_ranges(net, run, reverse, ranges, dst)
            return dst
        assert_arena_independent(net.ctx, two_ranges, what=("front4_ranges", reverse))


@pytest.mark.parametrize("n5", (100, 2_500))
def test_part_back5(enc, cuda, n5):
    """n5 = 100: the short-row kernel; 2 500: the tiled channel-last kernel"""
    net = _net(enc, cuda, "f16x2")
    rows = torch.from_numpy((np.random.RandomState(n5).rand(3, n5, 128) * 2.0).astype(np.float32)).to(cuda)

    def one():
        return engine.encoder_back5(net, rows[0], torch.full((128, n5 // 10), NAN, dtype=torch.float32, device=cuda))
    assert_arena_independent(net.ctx, one, what=("back5", n5))
    assert_arena_independent(net.ctx, lambda: engine.encoder_back5_batch(net, rows, _bins_out(cuda, 3, n5 // 10)), what=("back5_batch", n5))


# ---- the U-net encoders ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ("f16x2", "bf16x3", "f32"))
@pytest.mark.parametrize("kind,nlev", (("Encoder2", 5), ("Encoder2b", 5), ("Encoder3", 3)))
def test_unet_forward(cuda, kind, nlev, precision):
    """B = 2 at n = 64 and 4 096 (levels on both sides of the 2 048 boundary between the short-row and the tiled kernels), the input contiguous
    and with a channel stride of 1 (the two staging kernels)."""
    m = product_module(kind, 0, device=cuda, precision=precision)
    net = m._net(cuda)
    m._apply_precision(net, precision)
    for n in (64, 4096):
        nlc = torch.from_numpy((np.random.RandomState(n).rand(2, n, 128) * 0.5).astype(np.float32)).to(cuda)
        for x in (nlc.transpose(1, 2).contiguous(), nlc.transpose(1, 2)):
            assert_arena_independent(net.ctx, lambda: engine.unet_forward(net, x, nlev), what=(kind, precision, n, x.stride()))


# ---- the Decoders ------------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _dec_inputs(n, B, T):
    return DR.inputs(n, B, T)


def _dec_net(cuda, kind, precision, T=1, **kw):
    m = product_module(kind, 0, device=cuda, precision=precision, num_2d=T, **kw)
    net = m._net(cuda)
    m._apply_precision(net, precision)
    return net


@pytest.mark.parametrize("T", (1, 3))
@pytest.mark.parametrize("mode", ("bilinear", "nearest"))
@pytest.mark.parametrize("precision", ("f16x2", "f32"))
def test_decoder_forward(cuda, precision, mode, T):
    """n = 250 and 30, B = 2 (the even batch: two streams) and 3 (odd), with and without the coarse prediction"""
    net = _dec_net(cuda, "Decoder", precision, T, upsample_mode=mode)
    for n in (250, 30):
        for B in (2, 3):
            x, de, y = (t.to(cuda) for t in _dec_inputs(n, B, T))
            for yy in (y, None):
                assert_arena_independent(net.ctx, lambda: engine.decoder_forward(net, x, de, yy), what=(precision, mode, T, n, B, yy is not None))


@pytest.mark.parametrize("precision", ("f16x2", "f32"))
def test_decoder_rows_and_accumulate(cuda, precision):
    net = _dec_net(cuda, "Decoder", precision, 1, upsample_mode="bilinear")
    for n, B in ((250, 3), (30, 2)):
        x, de, y = (t.to(cuda) for t in _dec_inputs(n, B, 1))
        xs, des, ys = [x[b] for b in range(B)], [de[b] for b in range(B)], [y[b] for b in range(B)]
        assert_arena_independent(net.ctx, lambda: engine.decoder_forward_rows(net, xs, des, ys), what=("rows", precision, n, B))
        base = torch.from_numpy(np.random.RandomState(n).randn(B, 1, n, n).astype(np.float32)).to(cuda)
        assert_arena_independent(net.ctx, lambda: engine.decoder_forward(net, x, de, y, out=base.clone(), accumulate=True), what=("accumulate", precision, n, B))


@pytest.mark.parametrize("precision", ("f16x2", "f32"))
def test_decoder_1m(cuda, precision):
    net = _dec_net(cuda, "Decoder_1m", precision)
    for n, B in ((250, 3), (30, 2)):
        x = _dec_inputs(n, B, 1)[0].to(cuda)
        xs = [x[b] for b in range(B)]
        base = torch.from_numpy(np.random.RandomState(n).randn(B, 1, n, n).astype(np.float32)).to(cuda)
        assert_arena_independent(net.ctx, lambda: engine.decoder1m_forward(net, x), what=("1m", precision, n, B))
        assert_arena_independent(net.ctx, lambda: engine.decoder1m_forward_rows(net, xs), what=("1m rows", precision, n, B))
        assert_arena_independent(net.ctx, lambda: engine.decoder1m_forward(net, x, out=base.clone(), accumulate=True), what=("1m accumulate", precision, n, B))


# ---- the observed-data path: the pyramid lives in the arena --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,cutoff,levels", [(40, 50, 8), (513, 3, 12)])
def test_adaptive_coarsegrain(cuda, n, cutoff, levels):
    a, c = synth.synth_hic(n, 100 + n, nan_frac=0.05, depth=4.0)
    a, c = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(cuda), torch.from_numpy(np.ascontiguousarray(c, dtype=np.float32)).to(cuda)
    ctx = engine.get_context(cuda)
    bits = assert_arena_independent(ctx, lambda: SU.adaptive_coarsegrain_gpu(a, c, cutoff=cutoff, max_levels=levels), finite=False, what=("coarsegrain", n))
    assert np.isfinite(bits.view(np.float32)).any()


# ---- kernel test entries that stage their operands in the arena: the references of their own tests do not lean on its contents either -------------
def _conv1d_case(cin, cout, n, k=9):
    rs = np.random.RandomState(cin + cout + n)
    w = (rs.randn(cout, cin, k) / np.sqrt(cin * k)).astype(np.float32)
    b = (rs.randn(cout) * 0.1).astype(np.float32)
    return rs.randn(n, cin).astype(np.float32), w, b, rs.randn(n, cout).astype(np.float32)


@pytest.mark.parametrize("fmt", ("p16", "b16"))
@pytest.mark.parametrize("cin,cout,n,out_mode", [(64, 96, 1500, 0), (96, 128, 1030, 1), (128, 128, 323, 3)])
def test_entry_conv1d_p16(cuda, cin, cout, n, out_mode, fmt):
    x, w, b, r = _conv1d_case(cin, cout, n)
    x, r = torch.from_numpy(x).to(cuda), torch.from_numpy(r).to(cuda)
    ctx = engine.get_context(cuda)
    assert_arena_independent(ctx, lambda: engine.conv1d_p16(x, w, b, True, r, out_mode, fmt=fmt), what=("conv1d_p16", cin, cout, n, out_mode, fmt))
    assert_arena_independent(ctx, lambda: engine.conv1d_p16(x, w, b, False, None, out_mode, fmt=fmt), what=("conv1d_p16 plain", cin, cout, n, out_mode, fmt))


def test_entry_conv1d_nlc(cuda):
    ctx = engine.get_context(cuda)
    for cin, cout, n in ((128, 128, 2049), (96, 64, 513)):
        x, w, b, r = _conv1d_case(cin, cout, n)
        x, r = torch.from_numpy(np.stack([x, x[::-1]])).to(cuda), torch.from_numpy(np.stack([r, r[::-1]])).to(cuda)
        for precision in ("f16x2", "bf16x3"):
            assert_arena_independent(ctx, lambda: engine.conv1d_nlc(x, w, b, precision, True, r), what=("conv1d_nlc", cin, cout, n, precision))


def _conv2d_case(cin, cout, n, B):
    rs = np.random.RandomState(cin * 100 + cout + n)
    w = (rs.randn(cout, cin, 3, 3) / np.sqrt(cin * 9)).astype(np.float32)
    b = (rs.randn(cout) * 0.1).astype(np.float32)
    return torch.from_numpy(rs.randn(B, cin, n, n).astype(np.float32)), w, b, torch.from_numpy(rs.randn(B, cout, n, n).astype(np.float32))


def test_entry_conv2d(cuda):
    ctx = engine.get_context(cuda)
    x, w, b, r = _conv2d_case(64, 32, 126, 2)
    x, r = x.to(cuda), r.to(cuda)
    assert_arena_independent(ctx, lambda: engine.conv2d(x, w, b, 16, True, r), what="conv2d")
    assert_arena_independent(ctx, lambda: engine.conv2d(x, w, b, 16, False, None), what="conv2d plain")


@pytest.mark.parametrize("precision", ("f16x2", "bf16", "f16"))
def test_entry_conv2d_m16_and_dblock(cuda, precision):
    ctx = engine.get_context(cuda)
    for B in (2, 1):                                   # the four-row and the one-row kernel
        x, w, b, r = _conv2d_case(64, 32, 126, B)
        x, r = x.to(cuda), r.to(cuda)
        assert_arena_independent(ctx, lambda: engine.conv2d_m16(x, w, b, 8, True, r, precision=precision), what=("conv2d_m16", precision, B))
    xb = torch.from_numpy(np.random.RandomState(126).randn(3, 64, 126, 126).astype(np.float32)).to(cuda)
    convs = DR.dense_block(116)
    assert_arena_independent(ctx, lambda: engine.conv2d_dblock(xb, convs, 16, precision), what=("conv2d_dblock", precision))


# ---- one module-level case: the 1 Mb screen, on every context of the thread -----------------------------------------------------------------------------
def _thread_contexts():
    """every context of this thread and of its pools, enumerated as tests/conftest.py does"""
    ctxs = list(getattr(engine._tls, "ctxs", {}).values())
    for pool in engine._thread_pools().values():
        ctxs += list(pool.ctxs)
    return ctxs


def test_screen_1m_both_strands(cuda, monkeypatch):
    """`screen.screen_1m` with a substitution, a deletion and an insertion, ``strands="both"``, two batches: every workspace of the thread is filled
    before the reference run and again before each batch; every field of the result is identical across the fills, no batch falls back."""
    from orca_amd import orca_models as M
    from tests.test_gpu_screen_sets import _window
    from tests.test_screen_indel_cpu import plan_flank
    from tests.test_screen_sets_cpu import snv
    c, fl = _window(), plan_flank(8_000)
    model = M.H1esc_1M(synthetic_seed=0).to(cuda)
    win, flank = torch.from_numpy(c).to(cuda), torch.from_numpy(fl).to(cuda)
    edits = [snv(c, 100_003), S.Edit("del", 50_001, 4_300), S.Edit("ins", 30_100, np.random.RandomState(8).randint(0, 4, 6_000).astype(np.uint8))]
    state = {"byte": None, "fills": 0}

    def fill_all():
        if state["byte"] is None:
            return
        for ctx in _thread_contexts():
            size = ctx.workspace_bytes()
            assert ctx.fill_workspace(state["byte"]) == size + EDGE_BYTES
            state["fills"] += size > 0

    real = S._Screen.two_part

    def two_part(self, *a, **k):
        fill_all()
        return real(self, *a, **k)
    monkeypatch.setattr(S._Screen, "two_part", two_part)

    def run():
        fill_all()
        st = {}
        with nan_outputs():
            res = S.screen_1m(model, win, edits, batch=2, keep_maps=True, stats=st, regions=[(5, 15, 20, 35)], flank=flank, aligned=True, strands="both")
        torch.cuda.synchronize()
        assert st["route"] == "two_part" and st["two_part_batches"] == 2 and st["range_fallback_batches"] == 0 and not st["range_fallback_reference"]
        return {k: as_bits(v) for k, v in sorted(vars(res).items()) if isinstance(v, torch.Tensor) and v.numel()}

    run()                                               # sizes every arena
    sizes = [ctx.workspace_bytes() for ctx in _thread_contexts()]
    results = {}
    for byte in arena.FILLS:
        state["byte"], state["fills"] = byte, 0
        results[byte] = run()
        assert state["fills"] >= 3                      # the reference and two batches, on at least one non-empty arena
        assert [ctx.workspace_bytes() for ctx in _thread_contexts()] == sizes, "an arena was regrown: the fill is gone"
    base = results[0x00]
    assert {"ref_map", "maps", "delta_profile", "delta_abs_mean", "delta_abs_max", "strand_gap", "aligned_profile"} <= set(base)
    for k in ("ref_map", "maps", "delta_profile", "strand_gap"):
        assert np.isfinite(base[k].view(np.float32)).all(), k
    for byte in arena.FILLS[1:]:
        assert set(results[byte]) == set(base)
        for k, bits in base.items():
            assert np.array_equal(results[byte][k], bits), (f"fill 0x{byte:02X}", k, int((results[byte][k] != bits).sum()))
