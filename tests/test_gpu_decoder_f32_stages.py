"""-m gpu: the exact-fp32 Decoders kernel by kernel against fp64 at EVERY pixel and channel - `conv2d_3x3_kernel` alone (engine.conv2d) and
the production chain of a `precision="f32"` net stopped behind each stage (engine.decoder_probe; an f32 net hands out its fp32 planes: stage 0
of a Decoder is the whole 136-channel input map, A with y has 72 channels): `outer_sum_kernel`, `upsample2d_x2_kernel`, `conv2d_3x3_kernel<32|64>`
layer by layer and `final_sym_kernel`.  This is the arithmetic every Decoder call is redone in when the fp16-range guard fires, and the
reference that test_decoder_size_sweep_split_fp16_vs_exact_fp32 judges the 16-bit path by.  The counterpart of test_gpu_decoder_stages.py.

ISOLATION: a stage's fp64 reference is applied to what the GPU handed out for the stage before, so a stage's error is its own.
Metric: `rel_err` = max |d| / max(1, max |ref|) unless an elementwise bound is stated.

BOUNDS.  None is taken from the kernels' output.  A convolution stage is held to YARD_FACTOR = 16 x its YARDSTICK - the same stage on the same
input in torch fp32 on the CPU against fp64, computed inside each test (decoder_ref.py; test_decoder_stages_cpu.py proves that a plain
sequential fp32 chain stays within it and that fp16-rounded operands exceed it hundreds of times).  The pointwise stages have derived bounds:
outer sum |d| <= 2^-24 |ref| + 2^-149 (one fp32 addition); distenc channels and nearest up-sampling bit-equal; pad channels exactly 0; bilinear
|d| <= 8 x 2^-24 x (the same interpolation of |y|) (the weights 0, 1/4, 3/4, 1 are exact, each term passes at most four roundings);
accumulate |acc - (pre + out)| <= 2^-23 |pre + out| + 2^-126.  Every test prints its figures (`pytest -s`); the docstrings record the worst
ratio to the yardstick observed on the MI355X - a record, not the limit."""
import functools

import numpy as np
import pytest
import torch

from orca_amd import engine
from tests import decoder_ref as R
from tests.decoder_ref import rel_err
from tests.util import product_module

pytestmark = pytest.mark.gpu

_modules = {}


def _module(cuda, kind, seed, precision="f32", num_2d=1, mode="bilinear"):
    key = (kind, seed, precision, num_2d, mode)
    if key not in _modules:
        kw = {"upsample_mode": mode} if kind == "Decoder" else {}
        _modules[key] = product_module(kind, seed, device=cuda, precision=precision, num_2d=num_2d, **kw)
    return _modules[key]


def _net(m, cuda):
    net = m._net(cuda)
    m._apply_precision(net, m.precision)
    return net


def _probe(m, cuda, x, de, y, stage):
    net = _net(m, cuda)
    out = engine.decoder_probe(net, x, de, y, stage).cpu().numpy()
    assert not net.ctx.take_overflow()
    return out


def _dev(cuda, *ts):
    return [None if t is None else t.to(cuda) for t in ts]


@pytest.fixture(autouse=True, scope="module")
def _drop_what_the_module_kept():
    """The modules (their nets' weight uploads) and the kept chain maps go with the file: later files find the device and the host as they
    would without it."""
    yield
    _modules.clear()
    _chain_stage.cache_clear()


_worst = {}


def _held(group, label, got, stage, *args):
    """rel_err of ``got`` against the fp64 ``stage(*args)`` <= YARD_FACTOR x the yardstick of that stage; prints both and the group's worst ratio."""
    ref, yard = R.yardstick(stage, *args)
    err = rel_err(got, ref)
    ratio = err / yard if yard > 0 else (0.0 if err == 0 else float("inf"))
    _worst[group] = max(_worst.get(group, 0.0), ratio)
    print(f"{label}: rel_err {err:.3g}, yardstick {yard:.3g}, ratio {ratio:.2f} (worst of '{group}' so far {_worst[group]:.2f}; bound {R.YARD_FACTOR})")
    return got.shape == ref.shape and err <= R.YARD_FACTOR * yard


# ---- the conv kernel alone, exact case --------------------------------------------------------------------------------------------------------
CONV_SHAPES = [(136, 64, 1, 250, 1),     # the Decoder's first layer: 17 chunks, 2 garbage columns in the last float4
               (72, 64, 1, 30, 2),       # the lcombiner input with y
               (65, 64, 1, 17, 2),       # a padded chunk, odd n
               (64, 32, 64, 250, 1),     # the edge waves' tap skipping
               (32, 64, 32, 33, 3),      # one column into the second wave, d ~ n, B = 3
               (64, 32, 16, 2, 2),       # every off-centre tap outside the map
               (32, 64, 8, 1, 1),        # n = 1
               (64, 64, 4, 256, 1),      # no pad column, dilation 4
               (64, 32, 2, 255, 1),      # odd n at the top of the range
               (128, 32, 1, 64, 2),      # wave boundary
               (64, 64, 1, 65, 2)]       # wave boundary


@pytest.mark.parametrize("cin,cout,d,n,B", CONV_SHAPES)
def test_conv_kernel_exact_case(cuda, cin, cout, d, n, B):
    """conv2d_3x3_kernel<32|64> through orca_conv2d_forward on data that fp32 sums exactly in ANY order (decoder_ref.exact_conv_case: integers
    in [-8, 8], weights and bias k / 8; test_decoder_stages_cpu.py): the output EQUALS the fp64 reference, plain and with ReLU + residual - a
    wrong border tap, chunk, wave skip or batch stride is an O(1) difference at some pixel."""
    x, w, b, r = R.exact_conv_case(cin, cout, n, B)
    xd, rd = _dev(cuda, x, r)
    for relu, res, resd in ((False, None, None), (True, r, rd)):
        got = engine.conv2d(xd, w, b, d, relu=relu, r=resd).cpu().numpy()
        ref = R.conv_ref(x, w, b, d, relu, res)
        bad = int((got.astype(np.float64) != ref).sum())
        print(f"conv exact cin={cin} cout={cout} d={d} n={n} B={B} relu={relu}: {bad} of {ref.size} values differ")
        assert got.shape == ref.shape and bad == 0


# ---- the head: outer_sum_kernel, upsample2d_x2_kernel -------------------------------------------------------------------------------------------
def _outer_sum_ok(got, ref):
    d = np.abs(got.astype(np.float64) - ref)
    bound = 2.0 ** -24 * np.abs(ref) + 2.0 ** -149
    return bool((d <= bound).all()), float((d / bound).max())


@pytest.mark.parametrize("n", [250, 30, 2])
@pytest.mark.parametrize("T", [1, 3, 8])
@pytest.mark.parametrize("mode", ["bilinear", "nearest"])
def test_head_input_map_and_upsampled_prediction(cuda, mode, T, n):
    """The per-map `outer_sum_kernel` and `upsample2d_x2_kernel` loops at B = 2 (every row different): stage 0 = x_i + x_j in 128 channels
    (one fp32 addition), distenc bit-equal in the next T, zeros to 135; channels 64..71 of stage 2 = the up-sampled coarse prediction
    (nearest: bit-equal; bilinear: the derived bound, which an unclamped last row or column breaks), zeros behind its T planes.  x is a
    transposed view (channel stride 1); the contiguous x gives the same bits.
    Worst observed fraction of the elementwise bounds: 1.0 (outer sum: the half ulp of a correctly rounded sum), 0.38 (bilinear, T = 8,
    n = 250)."""
    m = _module(cuda, "Decoder", 0, num_2d=T, mode=mode)
    x, de, y = R.inputs(n, 2, T)
    xd = x.transpose(1, 2).contiguous().to(cuda).transpose(1, 2)
    assert not xd.is_contiguous()
    ded, yd = _dev(cuda, de, y)
    in0, up = R.head_f32(x, de, y, mode)
    g0 = _probe(m, cuda, xd, ded, yd, 0)
    g2 = _probe(m, cuda, xd, ded, yd, 2)
    assert g0.shape == (2, 136, n, n) and g2.shape == (2, 72, n, n)
    ok0, w0 = _outer_sum_ok(g0[:, :128], in0[:, :128])
    assert ok0
    assert np.array_equal(g0[:, 128: 128 + T], de.numpy()) and not g0[:, 128 + T:].any()
    gu = g2[:, 64: 64 + T].astype(np.float64)
    if mode == "nearest":
        w2 = 0.0
        assert np.array_equal(gu, up[:, :T])
    else:
        bound = 8 * 2.0 ** -24 * R.head_f32(x, de, y.abs(), mode)[1][:, :T]
        w2 = float((np.abs(gu - up[:, :T]) / np.maximum(bound, 2.0 ** -149)).max())
        assert (np.abs(gu - up[:, :T]) <= bound).all()
    assert not g2[:, 64 + T:].any()
    print(f"f32 head {mode} T={T} n={n}: worst fraction of the elementwise bound {w0:.3g} (outer sum), {w2:.3g} (up-sampled y)")
    xc = x.to(cuda)
    assert xc.is_contiguous()
    assert np.array_equal(_probe(m, cuda, xc, ded, yd, 0), g0) and np.array_equal(_probe(m, cuda, xc, ded, yd, 2), g2)


def test_head_outer_sum_of_the_decoder_1m(cuda):
    """Stage 0 of an exact-fp32 Decoder_1m: x_i + x_j in 128 channels, n = 250 and 2, B = 2, one fp32 addition per value.
    Worst observed fraction of the bound: 1.0 (the half ulp of a correctly rounded sum)."""
    m = _module(cuda, "Decoder_1m", 2)
    for n in (250, 2):
        x, _, _ = R.inputs(n, 2)
        g = _probe(m, cuda, x.to(cuda), None, None, 0)
        ok, w = _outer_sum_ok(g, R.outer_sum(x))
        print(f"f32 outer sum n={n}: worst fraction of the elementwise bound {w:.3g}")
        assert g.shape == (2, 128, n, n) and ok


# ---- first conv, combinerD, block 0 -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [250, 256, 30, 2])
@pytest.mark.parametrize("with_y", [True, False])
@pytest.mark.parametrize("seed", R.SEEDS)
def test_first_conv_combinerD_and_block0(cuda, seed, with_y, n):
    """Stage 1 (the 136-channel first layer, 17 chunks) from the GPU's stage 0; stage 2 channels 0..63 (three convs, residual) from the GPU's
    stage 1; stage 3 (block 0: lcombiner / combiner on the 72-channel map with y, lconvtwos.0 / convtwos.0 without) from the GPU's stage 2.
    B = 2.  Worst observed ratio to the yardstick: first conv 6.34, combinerD 4.42, block 0 2.54 (bound 16)."""
    m = _module(cuda, "Decoder", seed)
    sd = R.decoder_sd("Decoder", seed)
    x, de, y = R.inputs(n, 2)
    y = y if with_y else None
    xd, ded, yd = _dev(cuda, x, de, y)
    g = [_probe(m, cuda, xd, ded, yd, k) for k in range(4)]
    assert g[0].shape[1] == 136 and g[2].shape[1] == (72 if with_y else 64)
    tag = f"f32 seed {seed} y={with_y} n={n}"
    ok = [_held("first conv", f"{tag} first conv", g[1], R.first_map, sd, g[0]),
          _held("combinerD", f"{tag} combinerD", g[2][:, :64], R.mat, sd, g[1]),
          _held("block 0", f"{tag} block 0", g[3], R.block, sd, "Decoder", 0, g[2])]
    assert all(ok), ok


# ---- every block of the chain -----------------------------------------------------------------------------------------------------------------
CHAINS = {"dec30": ("Decoder", 0, 30, 2), "dec1m30": ("Decoder_1m", 2, 30, 2), "dec250": ("Decoder", 2, 250, 1), "dec256": ("Decoder", 0, 256, 1),
          "dec2": ("Decoder", 2, 2, 3)}
BLOCKS = ([("dec30", i) for i in range(1, 28)] + [("dec1m30", i) for i in range(19)] + [("dec250", i) for i in list(range(1, 8)) + [27]] +
          [("dec256", i) for i in range(1, 8)] + [("dec2", i) for i in range(1, 8)])


@functools.lru_cache(maxsize=2)
def _chain_stage(cuda, chain, stage):
    """The GPU's map behind ``stage`` of a chain (the map a block test checks is what the next block's test reads: kept for it)."""
    kind, seed, n, B = CHAINS[chain]
    x, de, y = R.inputs(n, B)
    xd, ded, yd = _dev(cuda, x, de, y) if kind == "Decoder" else (x.to(cuda), None, None)
    return _probe(_module(cuda, kind, seed), cuda, xd, ded, yd, stage)


@pytest.mark.parametrize("chain,i", BLOCKS)
def test_every_block_of_the_chain(cuda, chain, i):
    """Block i of the exact-fp32 chain (four conv2d_3x3_kernel launches, two residuals): fp64 `decoder_block` on the GPU's stage 2 + i against
    the GPU's stage 3 + i.  Decoder with y at n = 30, B = 2: blocks 1..27; Decoder_1m at n = 30, B = 2: 0..18; Decoder at n = 250, B = 1:
    1..7 and 27; at n = 256 (no pad column), B = 1: 1..7; at n = 2 (every off-centre tap of d >= 2 outside the map), B = 3: 1..7.
    Worst observed ratio to the yardstick per chain: Decoder n = 30 1.99, Decoder_1m 2.22, n = 250 1.77, n = 256 1.84, n = 2 1.36 (bound 16)."""
    kind, seed, n, B = CHAINS[chain]
    sd = R.decoder_sd(kind, seed)
    src = _chain_stage(cuda, chain, 2 + i if i > 0 else 0)
    got = _chain_stage(cuda, chain, 3 + i)
    assert src.shape[0] == B and got.shape == (B, 64, n, n)
    assert _held(f"blocks {chain}", f"f32 {chain} block {i} d={R.DIL[kind][i]}", got, R.block, sd, kind, i, src)


# ---- final ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [250, 30, 2])
@pytest.mark.parametrize("precision,T", [("f32", 1), ("f32", 3), ("f32", 8), ("f16x2", 8)])
def test_final_head_symmetrisation_and_accumulate(cuda, precision, T, n):
    """final_sym_kernel (f32) on the forward's output against fp64 `final` + symmetrisation of the GPU's last-stage probe, B = 2,
    64 -> max(5, T) -> T; T = 8 = ORCA_MAX_TARGETS fills the head's LDS arrays, so the f16x2 net's final_sym_m16_kernel gets the same case
    under the same bound.  The output equals its transpose exactly; accumulate adds into a pre-filled `out` within one fp32 addition.
    Worst observed ratio to the yardstick: f32 1.12, f16x2 1.10 (bound 16); accumulate 0.5 of its elementwise bound."""
    m = _module(cuda, "Decoder", 2, precision=precision, num_2d=T)
    sd = R.decoder_sd("Decoder", 2, num_2d=T)
    x, de, y = R.inputs(n, 2, T)
    xd, ded, yd = _dev(cuda, x, de, y)
    last = _probe(m, cuda, xd, ded, yd, 30)
    net = _net(m, cuda)
    out = engine.decoder_forward(net, xd, ded, yd)
    assert not net.ctx.take_overflow() and out.shape == (2, T, n, n)
    assert _held(f"final {precision}", f"{precision} final T={T} n={n}", out.cpu().numpy(), R.final, sd, last)
    assert torch.equal(out, out.transpose(2, 3))
    pre = torch.from_numpy(np.random.RandomState(n).randn(2, T, n, n).astype(np.float32)).to(cuda)
    acc = engine.decoder_forward(net, xd, ded, yd, out=pre.clone(), accumulate=True)
    want = pre.double() + out.double()
    frac = float(((acc.double() - want).abs() / (2.0 ** -23 * want.abs() + 2.0 ** -126)).max())
    print(f"{precision} final T={T} n={n}: accumulate, worst fraction of the elementwise bound {frac:.3g}")
    assert frac <= 1.0


# ---- call forms -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_y", [True, False])
def test_decoder_rows_form_equals_the_strided_form(cuda, with_y):
    """decoder_forward_rows (one device pointer per batch row) against the strided form on an exact-fp32 Decoder at n = 30, B = 3: the per-map
    outer_sum / upsample2d loops take their rows from `RowSrc::at` either way - the same bits."""
    m = _module(cuda, "Decoder", 0)
    net = _net(m, cuda)
    x, de, y = _dev(cuda, *R.inputs(30, 3))
    y = y if with_y else None
    want = engine.decoder_forward(net, x, de, y)
    got = engine.decoder_forward_rows(net, [x[b].clone() for b in range(3)], [de[b].clone() for b in range(3)],
                                      None if y is None else [y[b].clone() for b in range(3)])
    assert bool(torch.isfinite(want).all()) and not torch.equal(want[0], want[1]) and torch.equal(got, want)


def test_decoder1m_rows_form_equals_the_strided_form(cuda):
    """decoder1m_forward_rows against decoder1m_forward on an exact-fp32 Decoder_1m at n = 30, B = 3: the same bits."""
    m = _module(cuda, "Decoder_1m", 2)
    net = _net(m, cuda)
    (x,) = _dev(cuda, R.inputs(30, 3)[0])
    want = engine.decoder1m_forward(net, x)
    got = engine.decoder1m_forward_rows(net, [x[b].clone() for b in range(3)])
    assert bool(torch.isfinite(want).all()) and not torch.equal(want[0], want[1]) and torch.equal(got, want)


# ---- stale workspace --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["f32", "f16x2"])
def test_forward_does_not_read_what_an_earlier_forward_left_in_the_workspace(cuda, precision):
    """A forward at n = 250, B = 2; then, on the same context, one at n = 256 whose x is NaN (the input map and the residual stream, with no
    pad column at that size, are NaN all over, in a layout whose planes start elsewhere); then the first again: finite and the same bits.  The fp32 planes' pad columns 250..255 are never written at
    n = 250 (the conv masks them on the read), and the M16 block kernel gathers out-of-map taps from a pad pixel that the kernel in front
    must have left zero."""
    m = _module(cuda, "Decoder", 0, precision=precision)
    net = _net(m, cuda)
    x, de, y = _dev(cuda, *R.inputs(250, 2))
    a = engine.decoder_forward(net, x, de, y).clone()
    assert not net.ctx.take_overflow()
    x2, de2, y2 = _dev(cuda, *R.inputs(256, 2))
    engine.decoder_forward(net, torch.full_like(x2, float("nan")), de2, y2)
    net.ctx.take_overflow()                                     # (NaN is out of the fp16 range: clear the flag)
    b =engine.decoder_forward(net, x, de, y)
    assert not net.ctx.take_overflow()
    assert bool(torch.isfinite(a).all()) and torch.equal(a, b)
