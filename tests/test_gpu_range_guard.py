"""-m gpu: the fp16-range guard of the f16x2 arithmetic, kernel by kernel (cases and fp64 references: tests/range_guard_ref.py; their
preconditions: tests/test_range_guard_cpu.py).  Every case drains the context's flag, makes ONE call and reads the flag.  A "must flag" case
stores a value of 66000 somewhere; its twin stores 65000 there, must not flag, and - where the call returns values - must agree with the
fp64 reference within 2e-5 + 2^-22 relative (the bound of the kernels' own tests in test_gpu_kernels.py).  Device tensors are made once per
shape; a placement changes single elements."""
import warnings

import numpy as np
import pytest
import torch

from orca_amd import engine
from orca_amd import orca_modules as pm
from tests import encoder_ref as R
from tests import range_guard_ref as G
from tests.util import synth_sd

pytestmark = pytest.mark.gpu
REL = 2.0 ** -22


def _flag_of(cuda, fn):
    ctx = engine.get_context(cuda)
    ctx.take_overflow()
    out = fn()
    return out, ctx.take_overflow()


def _excess(y, ref):
    """max of |y - ref| - (2e-5 + 2^-22 |ref|) on the device (<= 0: within the bound)."""
    ref = ref.to(y.device)
    return float(((y.double() - ref).abs() - (2e-5 + REL * ref.abs())).max())


class _Dev1d:
    """A `Conv1dSpike` with its background on the device: `run(p, co, V)` puts the spike in, calls the kernel once and takes it out again."""

    def __init__(self, cuda, case, fmt="p16"):
        self.c, self.cuda, self.fmt = case, cuda, fmt
        self.x = torch.from_numpy(case.x0).to(cuda)
        self.r = None if case.r0 is None else torch.from_numpy(case.r0).to(cuda)
        self.ref = torch.from_numpy(case.stored0).to(cuda)

    def run(self, p, co, V, r_at=None, check=True):
        c = self.c
        x, w, r1, q, t = c.place(p, co, V, r_at)
        self.x[q, G.CI] = G.XS
        if r1 is not None:
            self.r[p, co] = float(r1[p, co])
        y, flag = _flag_of(self.cuda, lambda: engine.conv1d_p16(self.x, w, c.b, c.relu, self.r, c.out_mode, fmt=self.fmt))
        self.x[q, G.CI] = 0.0
        if r1 is not None:
            self.r[p, co] = float(c.r0[p, co])
        exc = None
        if check:
            o0, rows = c.reference_patch(x, w, r1, q)
            keep = self.ref[o0: o0 + rows.shape[0]].clone()
            self.ref[o0: o0 + rows.shape[0]] = torch.from_numpy(rows).to(self.cuda)
            exc = _excess(y, self.ref)
            self.ref[o0: o0 + rows.shape[0]] = keep
        return flag, exc


def _run_pairs(dev, places, scrub=False):
    """``scrub``: one more in-range call between the pair (see test_p16p5_kernel_guard_in_every_pool_slot); its flag is returned as "stale"."""
    bad = []
    for p, co in places:
        r_at = 0.0 if dev.c.r0 is not None else None
        flag, _ = dev.run(p, co, G.V_FLAG, r_at, check=False)
        if not flag:
            bad.append(("missed", p, co))
        if scrub and dev.run(p, co, G.V_OK, r_at, check=False)[0]:
            dev.stale = getattr(dev, "stale", []) + [(p, co)]
        flag, exc = dev.run(p, co, G.V_OK, r_at)
        if flag:
            bad.append(("false alarm", p, co))
        if exc > 0.0:
            bad.append(("value", p, co, exc))
    return bad


MODES = [(0, False, False), (0, True, True), (1, False, False), (1, True, True)]


@pytest.mark.parametrize("cin,cout,k,tile", [(64, 64, 9, 512), (128, 128, 9, 512), (64, 96, 9, 256), (64, 96, 17, 256)])
def test_p16_tiled_kernel_guard_by_position_and_channel(cuda, cin, cout, k, tile):
    """conv1d_k9_p16_kernel (conv_p16.h:760), n = 600: the 64-cout tile (512 positions, 8 waves of 64 positions x all 64 couts, wave tile
    2 x 2 accumulator tiles of 32 x 32; 128 couts = two cout blocks) and the 96-cout tile (256 positions, 8 waves of 32 x 96, 1 x 3 tiles), k = 9 and
    the 17-tap form, out_mode 0 and 1 (MaxPool1d(4)), each plain and with ReLU + residual.  A wave owns a position slice and every cout of
    the tile, so `conv1d_placements` takes one position in every 32-position slice of the first tile (every wave, both position halves of a
    2 x 2 wave tile) and walks the channel through ALL octets over the set (every cout block, every 32-cout accumulator tile, every 4-cout
    register group of it), plus positions 0, n - 1 (= the last valid position of the ragged last tile) and both sides of every tile boundary."""
    bad = []
    for out_mode, relu, res in MODES:
        dev = _Dev1d(cuda, G.Conv1dSpike(cin, cout, 600, k, relu, res, out_mode))
        bad += [(out_mode, res) + b for b in _run_pairs(dev, G.conv1d_placements(600, cout, tile))]
    assert not bad, bad


@pytest.mark.parametrize("out_mode,relu,res", [(0, False, False), (1, True, True)])
def test_p16x_kernel_guard_by_position_and_channel(cuda, out_mode, relu, res):
    """conv1d_k9_p16x_kernel (conv_p16x.h:305; 96 couts from 65 536 positions on), n = 65 600 = 128 tiles of 512 + 64: `p16x_placements` - the ends,
    511 | 512, 65 535 | 65 536, n - 1 in the ragged last tile, and one placement in each of the 16 waves (8 position groups x 2 cout groups) of an
    interior tile, moving through the 4 x 3 accumulator tiles of the wave tile and all 12 octets."""
    dev = _Dev1d(cuda, G.Conv1dSpike(96, 96, 65600, 9, relu, res, out_mode))
    bad = _run_pairs(dev, G.p16x_placements(65600))
    assert not bad, bad


@pytest.mark.parametrize("n", [323, 2000])
def test_p16p5_kernel_guard_in_every_pool_slot(cuda, n):
    """conv1d_k9_p16p5_kernel (conv_p16p5.h:282; 128 couts, ReLU + residual + MaxPool1d(5), 320-position tiles, positions dealt to the lanes with
    stride 5; 8 waves = 2 position groups x 4 cout groups): `pool5_placements` - the spike in each of the five slots of windows in both position
    groups, on both sides of the tile boundary at 320 and in the last stored window; the octets move so that every wave and octet is hit.
    This kernel reads input units beyond the end of its planes for lanes whose results are never stored, and its guard sees those lanes too:
    behind the last input plane the test entry keeps zero units of its own (as the Encoder's buffers do: tests/test_gpu_arena.py), so an in-range
    call right behind a flagged one (which left inf in the output buffer next door) does not flag: each pair still runs its in-range call twice,
    and neither may flag."""
    dev = _Dev1d(cuda, G.Conv1dSpike(128, 128, n, 9, True, True, 3))
    bad = _run_pairs(dev, G.pool5_placements(n), scrub=True)
    assert not bad, bad
    assert not getattr(dev, "stale", []), dev.stale


def test_p16_guard_sits_behind_residual_and_relu(cuda):
    """40000 from the conv + 40000 of residual: only the sum leaves the range (twin: + 25000); -66000 in front of the ReLU is stored as 0."""
    for out_mode in (0, 1):
        dev = _Dev1d(cuda, G.Conv1dSpike(64, 64, 600, 9, True, True, out_mode))
        flag, _ = dev.run(300, 21, 40000.0, r_at=40000.0, check=False)
        assert flag, out_mode
        flag, exc = dev.run(300, 21, 40000.0, r_at=25000.0)
        assert not flag and exc <= 0.0, (out_mode, flag, exc)
        flag, exc = dev.run(300, 21, -G.V_FLAG, r_at=0.0)
        assert not flag and exc <= 0.0, (out_mode, flag, exc)


def test_p16_outputs_that_are_not_fp16_planes_never_flag(cuda):
    """out_mode 2 (fp32 rows) and B16 planes hold 1e5: no flag; the fp32 rows are correct."""
    for cin, cout in ((64, 64), (64, 96), (128, 128)):
        dev = _Dev1d(cuda, G.Conv1dSpike(cin, cout, 600, 9, False, False, 2))
        for p, co in ((0, 3), (511, cout - 1), (599, 40)):
            flag, exc = dev.run(p, co, 1.0e5)
            assert not flag and exc <= 0.0, (cin, cout, p, co, flag, exc)
    for cin, cout, out_mode in ((64, 64, 0), (64, 96, 1), (128, 128, 3)):
        dev = _Dev1d(cuda, G.Conv1dSpike(cin, cout, 600, 9, True, True, out_mode), fmt="b16")
        for p, co in ((0, 3), (511, cout - 1), (599, 40)):
            flag, _ = dev.run(p, co, 1.0e5, r_at=0.0, check=False)
            assert not flag, (cin, cout, out_mode, p, co)


def test_values_that_are_never_stored_are_reported_only(cuda, capsys):
    """The guard may fire for values a kernel computes and does not store: positions >= n of a ragged tile, the dropped remainder of a
    MaxPool1d(5).  That direction is conservative; printed, nothing asserted."""
    n = 65600
    c = G.Conv1dSpike(96, 96, n, 9, False, False, 0)
    x = torch.from_numpy(c.x0).to(cuda)
    x[n - 1, G.CI] = G.XS
    w = c.w0.copy()
    w[17, G.CI, 1] = G.V_FLAG / G.XS                   # tap 1 of position n + 2 reads position n - 1
    _, flag = _flag_of(cuda, lambda: engine.conv1d_p16(x, w, c.b, False, None, 0))
    with capsys.disabled():
        print(f"\n  conv_p16x.h, 66000 at virtual position n + 2 of the ragged last tile: flag = {flag}")
    dev = _Dev1d(cuda, G.Conv1dSpike(128, 128, 323, 9, True, True, 3))
    flag, exc = dev.run(321, 50, G.V_FLAG, r_at=0.0)
    with capsys.disabled():
        print(f"  conv_p16p5.h, 66000 at position 321 of 323 (dropped by the pool): flag = {flag}, stored values within the bound: {exc <= 0.0}")


# ---- channel-last kernels: the guard is on the input split -------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [55, 2048, 2049, 4100])
def test_channel_last_kernels_guard_their_input(cuda, n):
    """conv_small.h:102 (rows of <= 2048 positions) and conv_bf16s.h:317 (longer rows), 128 -> 128, B = 3 with the value in batch row 2: an
    input of 7e4 at one (position, channel) flags in f16x2 and never in bf16x3 / bf16x2 / bf16; 6.5e4 there does not flag and the output is
    right; an in-range input whose OUTPUT is 1e5 does not flag either (the consumer checks that value) and is right."""
    c = G.NlcCase(128, 128, n)
    xd = torch.from_numpy(c.x0).to(cuda)
    bad = []
    for p, ci in ((0, 0), (n // 2, 77), (n - 1, 127), (min(n - 1, 2047), 40), (n - 2, 9)):
        for value, want in ((c.X_BAD, True), (G.V_OK, False)):
            x, ref = c.with_input(p, ci, value)
            keep = float(c.x0[2, p, ci])
            xd[2, p, ci] = value
            y, flag = _flag_of(cuda, lambda: engine.conv1d_nlc(xd, c.w0, c.b, "f16x2"))
            if flag != want:
                bad.append(("f16x2", p, ci, value, flag))
            if not want and _excess(y, torch.from_numpy(ref)) > 0.0:
                bad.append(("value", p, ci))
            if want:
                for prec in ("bf16x3", "bf16x2", "bf16"):
                    if _flag_of(cuda, lambda: engine.conv1d_nlc(xd, c.w0, c.b, prec))[1]:
                        bad.append((prec, p, ci))
            xd[2, p, ci] = keep
    x, w, ref = c.big_output(n - 1, 77)
    y, flag = _flag_of(cuda, lambda: engine.conv1d_nlc(torch.from_numpy(x).to(cuda), w, c.b, "f16x2"))
    assert not flag and _excess(y, torch.from_numpy(ref)) <= 0.0
    assert not bad, bad


# ---- Decoder convs on M16 maps -------------------------------------------------------------------------------------------------------------
def _m16_pairs(cuda, c, xd, rd, refd, precision="f16x2", check=True):
    """Every pixel of `conv2d_pixels` in map B - 1: [(what, pixel, ...)] of the placements that flag wrongly or store wrong values."""
    bad = []
    bm = c.B - 1
    for k, (i, j) in enumerate(G.conv2d_pixels(c.n, c.dil, c.B)):
        co = (9 * k) % c.cout
        xd[bm, G.CI, i, j] = G.XS
        for V, want in ((G.V_FLAG, True), (G.V_OK, False)):
            w = c.weight(bm, i, j, co, V)
            y, flag = _flag_of(cuda, lambda: engine.conv2d_m16(xd, w, c.b, c.dil, c.relu, rd, precision=precision))
            if flag != want:
                bad.append(("missed" if want else "false alarm", (i, j), co))
            if check and not want:
                patch = c.reference_patch(w, bm, i, j)
                keep = [refd[bm, :, pi, pj].clone() for (pi, pj), _ in patch]
                for (pi, pj), v in patch:
                    refd[bm, :, pi, pj] = torch.from_numpy(v).to(cuda)
                exc = _excess(y, refd)
                for ((pi, pj), _), kv in zip(patch, keep):
                    refd[bm, :, pi, pj] = kv
                if exc > 0.0:
                    bad.append(("value", (i, j), co, exc))
        xd[bm, G.CI, i, j] = 0.0
    return bad


@pytest.mark.parametrize("n,B", G.CONV2D_MAPS)
def test_conv2d_m16_guard_by_pixel(cuda, n, B):
    """conv2d_3x3_m16_kernel (B = 1: one output row per workgroup, conv2d_m16.h:647 / :688) and conv2d_3x3_m16q_kernel (B = 2: four rows x 128 pixels,
    conv2d_m16q.h:413; the spike in map 1), dilation 1 and 8, 64 -> 32 and 32 -> 64, plain and with ReLU + residual: the four corners, the last
    row and column, a pixel on each side of a row-group boundary and of the 128-pixel column-tile boundary; the channel moves by 9 per pixel
    (octets 0, 1, 2, ... and every lane group of an accumulator tile)."""
    bad = []
    for dil, cin, cout, res in G.CONV2D_LAYERS:
        c = G.Conv2dSpike(cin, cout, n, dil, B, relu=res, residual=res)
        xd = torch.from_numpy(c.x0).to(cuda)
        rd = None if c.r0 is None else torch.from_numpy(c.r0).to(cuda)
        refd = torch.from_numpy(c.stored0).to(cuda)
        bad += [(dil, cin, cout, res) + b for b in _m16_pairs(cuda, c, xd, rd, refd)]
    assert not bad, bad


@pytest.mark.parametrize("B", [1, 2])
def test_conv2d_m16_single_plane_modes(cuda, B):
    """The same spike through the single-plane instantiations (the NS / DT switches of the epilogues): "f16" (one fp16 plane, DT = 1) guards like
    f16x2 - its stores have the same range; "bf16" (DT = 0) has fp32's exponent range and never flags.  (Flags only: the operands of these
    modes are rounded to 11 / 8 bits, the weight that makes 66000 / 65000 included - 64 x fp16(1031.2) = 65984, 64 x fp16(1015.6) = 65024.)"""
    for cin, cout in ((64, 32), (32, 64)):
        c = G.Conv2dSpike(cin, cout, 30, 1, B, relu=True, residual=True)
        xd, rd = torch.from_numpy(c.x0).to(cuda), torch.from_numpy(c.r0).to(cuda)
        assert not _m16_pairs(cuda, c, xd, rd, None, precision="f16", check=False)
        bm = B - 1
        for k, (i, j) in enumerate(G.conv2d_pixels(30, 1, B)):
            xd[bm, G.CI, i, j] = G.XS
            w = c.weight(bm, i, j, (9 * k) % cout, G.V_FLAG)
            assert not _flag_of(cuda, lambda: engine.conv2d_m16(xd, w, c.b, 1, True, rd, precision="bf16"))[1], (cin, cout, i, j)
            xd[bm, G.CI, i, j] = 0.0


@pytest.mark.parametrize("d", G.DBLOCK_DILS)
def test_dblock_guard_by_pixel(cuda, d):
    """conv2d_dblock_kernel (conv2d_dblock.h:366) with zero weights and biases summing to 6000: out = x + 6000 exactly, so one pixel of 60000 in map 1
    leaves the range there only (twin: 59000) - at the corners and on both sides of a sub-image boundary (pixels d - 1 | d)."""
    c = G.DBlockCase(G.DBLOCK_N, G.DBLOCK_B)
    xd = torch.from_numpy(c.x0).to(cuda)
    for k, (i, j) in enumerate(c.pixels(d)):
        ch = (9 * k + 5) % 64
        for xv, want in ((c.X_HI, True), (c.X_LO, False)):
            xd[1, ch, i, j] = xv
            y, flag = _flag_of(cuda, lambda: engine.conv2d_dblock(xd, c.convs, d))
            assert flag == want, (d, i, j, ch, xv, flag)
            if not want:
                assert _excess(y, xd.double() + c.bias_sum) <= 0.0, (d, i, j)
        xd[1, ch, i, j] = float(c.x0[1, ch, i, j])


# ---- the edge-fix kernels ------------------------------------------------------------------------------------------------------------------
def _encoder(sd, cuda):
    enc = pm.Encoder(precision="f16x2")
    enc.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, strict=True)
    enc.eval()
    net = enc._net(cuda)
    enc._apply_precision(net, "f16x2")
    return enc, net


@pytest.mark.parametrize("reverse", [False, True])
@pytest.mark.parametrize("stage", [1, 2])
def test_edge_fix_kernels_raise_the_flag(cuda, stage, reverse):
    """lconv_edge_layer_kernel / lconv_edge_pool_kernel overwrite the end positions of a composed linear group with the reference's exact values
    and store them as fp16 hi / lo.  `edge_sd` hides +-1e5 exactly there (test_range_guard_cpu.py: every value a main kernel stores or checks is
    in range): stage 2 through the layer kernel (lout2's first / last four positions), stage 1 - on the default route from packed bases - through
    the pool kernel alone (the pooled end windows).  The flag must be up after `encoder_forward_codes` and after `encoder_stage3_planes`; the
    module must warn, fall back and match the fp64 oracle within 1e-4 of max |ref| (the bound of test_f16x2_overflow_guard_falls_back)."""
    L = 16 * 300
    codes = np.random.RandomState(5).randint(0, 4, L).astype(np.uint8)
    cd = torch.from_numpy(codes).to(cuda)
    # the unmodified Encoder on the same bases: nothing to flag
    enc0, net0 = _encoder(synth_sd("Encoder", 0), cuda)
    assert not _flag_of(cuda, lambda: engine.encoder_forward_codes(net0, cd[None], reverse))[1]
    assert not _flag_of(cuda, lambda: engine.encoder_stage3_planes(net0, cd, reverse))[1]
    sd = G.edge_sd(synth_sd("Encoder", 0), stage)
    enc, net = _encoder(sd, cuda)
    y, flag = _flag_of(cuda, lambda: engine.encoder_forward_codes(net, cd[None], reverse))
    print(f"\n  stage {stage}, reverse {reverse}: flag after encoder_forward_codes = {flag}; f16x2 output finite: {bool(torch.isfinite(y).all())}, "
          f"max |y| = {float(y.abs().nan_to_num(nan=-1.0).max()):.4g}")
    assert flag
    assert _flag_of(cuda, lambda: engine.encoder_stage3_planes(net, cd, reverse))[1]
    ref = R.stages(sd, R.strand_codes(codes, reverse), upto=7)[7].T[None]          # [1, 128, bins]
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        out = enc.forward_codes(cd[None], reverse=reverse).cpu().numpy()
    assert any("fp16 range" in str(m.message) for m in w)
    s = float(np.abs(ref).max())
    err = float(np.abs(out.astype(np.float64) - ref).max()) / s
    print(f"  module after the fallback: max |out - ref| / max |ref| = {err:.3g} (max |ref| = {s:.4g})")
    assert np.isfinite(out).all() and err < 1e-4


# ---- Decoder heads: the outer sum, the distance encoding, the up-sampled coarse prediction ---------------------------------------------------------
def _decoder(kind, cuda, **kw):
    from tests.util import shapes_of
    from orca_amd import synth
    sd = {k: np.array(v, copy=True) for k, v in synth.synth_state_dict(shapes_of(kind, **kw), seed=0).items()}
    if kind == "Decoder":
        # A Decoder never stores x_i + x_j (it enters lcombinerD's first conv through fp32 tables), so the spike in x can only show in that conv's
        # OUTPUT.  With this column zeroed the output stays O(1) and can be held to the oracle; a non-zero column would put ~1e3 x the weights
        # there and flag, if at all, through the conv's own epilogue - the guard test_conv2d_m16_guard_by_pixel already covers.
        sd["lcombinerD.0.weight"][:, G.HEAD_C] = 0.0
    dec = getattr(pm, kind)(precision="f16x2", **kw)
    dec.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, strict=True)
    dec.eval()
    net = dec._net(cuda)
    dec._apply_precision(net, "f16x2")
    return sd, net


@pytest.mark.parametrize("B", [1, 2])
def test_decoder_heads_guard_the_outer_sum(cuda, B):
    """x[b, c, i] = 40000 with everything else O(1): x_i + x_j leaves the range at pixel (i, i) alone (twin: 32500 -> 65000), i = 0, 64, n - 1, in
    the last map of the batch.  Decoder_1m stores the sum (outer_sum_m16_body): stopped behind stage 0, the flag asserted and the twin compared
    exactly (x lives on a grid of 1/4).  A Decoder does NOT store it: x_i + x_j enters lcombinerD's first conv through the separable fp32
    tables of its epilogue (sep_tables_kernel), so with zero weights on the spike's channel nothing out of range is ever stored; the assertion
    for it is that neither value flags and both stage-1 maps match the fp64 oracle.  (What a Decoder's head does store and guard - the distance
    encoding and the up-sampled prediction - is the next test.)"""
    from oracle import orca_oracle as O
    x0, de0, _ = G.head_inputs(B)
    de = torch.from_numpy(de0)
    sd1, net1 = _decoder("Decoder_1m", cuda)
    sdd, netd = _decoder("Decoder", cuda, upsample_mode="bilinear")
    xd = torch.from_numpy(x0).to(cuda)
    for i in G.HEAD_SUM_PIXELS:
        for v, want in ((G.HEAD_X_BAD, True), (G.HEAD_X_OK, False)):
            xd[B - 1, G.HEAD_C, i] = v
            y, flag = _flag_of(cuda, lambda: engine.decoder_probe(net1, xd, None, None, 0))
            assert flag == want, ("Decoder_1m", i, v)
            if not want:
                xx = xd.double()
                assert _excess(y, xx[:, :, :, None] + xx[:, :, None, :]) <= 0.0
            y, flag = _flag_of(cuda, lambda: engine.decoder_probe(netd, xd, de.to(cuda), None, 1))
            assert not flag, ("Decoder", i, v)
            in0 = O._pad_channels(de.double().expand(B, -1, -1, -1), O.DECODER_IN_CHANNELS)
            assert _excess(y, O.decoder_first(sdd, xd.cpu(), in0, torch.float64)) <= 0.0, ("Decoder", i, v)
        xd[B - 1, G.HEAD_C, i] = float(x0[B - 1, G.HEAD_C, i])


@pytest.mark.parametrize("B", [1, 2])
@pytest.mark.parametrize("mode", ["bilinear", "nearest"])
def test_decoder_head_guards_distenc_and_the_upsampled_prediction(cuda, mode, B):
    """A `distenc` entry of -inf (log 0) must flag (stage 0: the distance encoding in its M16 map); 7e4 in the coarse prediction `y` (map B - 1)
    must flag in the up-sample body, in both up-sample modes (stage 2); 6.5e4 there must not, and stage 2 then matches the fp64 oracle."""
    from oracle import orca_oracle as O
    x0, de0, y0 = G.head_inputs(B, seed=7)
    x = torch.from_numpy(x0).to(cuda)
    sd, net = _decoder("Decoder", cuda, upsample_mode=mode)
    de = torch.from_numpy(de0).to(cuda)
    out, flag = _flag_of(cuda, lambda: engine.decoder_probe(net, x, de, None, 0))
    assert not flag and _excess(out[:, :1], de.double().expand(B, -1, -1, -1)) <= 0.0
    for i, j in G.HEAD_DE_PIXELS:
        de[0, 0, i, j] = float("-inf")
        assert _flag_of(cuda, lambda: engine.decoder_probe(net, x, de, None, 0))[1], (i, j)
        de[0, 0, i, j] = float(de0[0, 0, i, j])
    yd = torch.from_numpy(y0).to(cuda)
    in0 = O._pad_channels(de.cpu().double().expand(B, -1, -1, -1), O.DECODER_IN_CHANNELS)
    s1 = O.decoder_first(sd, x.cpu(), in0, torch.float64)
    for i, j in G.head_y_pixels(mode):
        for v, want in ((G.HEAD_Y_BAD, True), (G.HEAD_Y_OK, False)):
            yd[B - 1, 0, i, j] = v
            out, flag = _flag_of(cuda, lambda: engine.decoder_probe(net, x, de, yd, 2))
            assert flag == want, (mode, i, j, v)
            if not want:
                up = torch.from_numpy(G.upsampled(yd.cpu().numpy(), mode))
                assert _excess(out, O.decoder_mat(sd, s1, up, torch.float64)) <= 0.0, (mode, i, j)
        yd[B - 1, 0, i, j] = float(y0[B - 1, 0, i, j])


# ---- Encoder stage 1 in every form -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", G.ENCODER_FORMS)
def test_encoder_stage1_forms_guard(cuda, form):
    """Every form `Net.set_encoder_form` accepts, from packed codes and from float rows (flat [L, 4] rows and strided [4, L] rows), L = 16 x 600.
    The routes run conv1d_first_mfma_p16_kernel with 9, 17 and 25 taps, conv1d_first_p16_kernel, the fused first layer (F1) and the residual
    from the bases (RL).  The synthetic Encoder must not flag; the same Encoder with lconv1's channel 9 scaled out of range through its last
    BatchNorm (weight x 100, bias + 1e5) must flag; float rows with one base scaled by 3e6 at position 0, 256 or L - 1 must flag.  This holds
    each ROUTE to the contract, not each of its kernels: the out-of-range value is seen by every kernel downstream of the first one too."""
    from orca_amd import synth
    L = G.STAGE1_L
    seq = synth.synth_sequence(L, seed=4, n_frac=0.01)                               # [1, L, 4]
    flat = torch.from_numpy(seq).to(cuda).transpose(1, 2)                            # [1, 4, L] view of flat rows
    strided = flat.contiguous()
    codes, ok = engine.pack_sequence(flat)
    assert ok
    enc0, net0 = _encoder(synth_sd("Encoder", 0), cuda)
    enc1, net1 = _encoder(G.stage1_scaled_sd(synth_sd("Encoder", 0)), cuda)
    net0.set_encoder_form(form)
    net1.set_encoder_form(form)
    runs = {"codes": lambda net: engine.encoder_forward_codes(net, codes), "flat rows": lambda net: engine.encoder_forward(net, flat),
            "strided rows": lambda net: engine.encoder_forward(net, strided)}
    for name, run in runs.items():
        assert not _flag_of(cuda, lambda: run(net0))[1], (form, name, "unscaled")
        assert _flag_of(cuda, lambda: run(net1))[1], (form, name, "scaled lconv1")
    for pos in G.STAGE1_POSITIONS:
        for name, x in (("flat rows", flat), ("strided rows", strided)):
            keep = x[0, :, pos].clone()
            x[0, :, pos] = keep * G.STAGE1_BASE_GAIN
            assert _flag_of(cuda, lambda: engine.encoder_forward(net0, x))[1], (form, name, pos)
            x[0, :, pos] = keep
