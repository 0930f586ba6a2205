"""-m gpu: the Decoders' kernels one at a time against fp64 at EVERY pixel and channel - the residual block of dilation 16 / 32 / 64 on its
own (engine.conv2d_dblock) and the production chain stopped behind each stage (engine.decoder_probe: stage numbering in
oracle/orca_oracle.py) - not after ~110 convolutions and the 64 -> 5 -> 1 head, where tests/test_gpu_nets.py allows 1e-4 on an O(1) map.

ISOLATION: a stage's reference is fp64 applied to what the GPU produced for the stage before (two probes; the decoded hi + lo values are exact
in fp32), so a stage's error is its own.  Metric: `rel_err` = max |d| / max(1, max |ref|) unless an elementwise bound is stated.

BOUNDS.  Each is 4 x the worst value observed on the MI355X, rounded up to one digit (every test prints its figure: `pytest -s`); the
docstrings record "worst observed ...; bound ...".  All f16x2 bounds are below the 2e-5 that test_conv2d_m16_dilated holds one M16
convolution to.  The head's elementwise bound follows from the storage format and the accumulate bound from fp32 addition."""
import numpy as np
import pytest
import torch

from orca_amd import engine
from orca_amd._lib import OrcaHipError
from tests import decoder_ref as R
from tests.decoder_ref import rel_err
from tests.util import product_module

pytestmark = pytest.mark.gpu

KERNEL_BOUND = 3e-6                  # the block kernel alone on dense weights: worst observed 6.33e-7
BLOCK_BOUND = R.BLOCK_BOUND          # one residual block of the chain: worst observed 1.26e-6 (decoder_ref.py)
FIRST_BOUND = 3e-6                   # the separable first conv: worst observed 7.2e-7
MAT_BOUND = 7e-6                     # combinerD (three convs and a residual): worst observed 1.54e-6
BLOCK0_BOUND = 4e-6                  # block 0: worst observed 9.45e-7
FINAL_BOUND = 2e-6                   # final + symmetrisation: worst observed 4.69e-7
# one residual block on single 16-bit planes against fp64 on the same (rounded) input: worst observed 5.67e-4 (f16), 5.21e-3 (bf16)
PLANE_BOUND = {"f16": 3e-3, "bf16": 3e-2}


_modules = {}


def _module(cuda, kind, seed, precision="f16x2", num_2d=1, mode="bilinear"):
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


# ---- the block kernel alone -----------------------------------------------------------------------------------------------------------------
SHAPES = [(250, 2), (256, 1), (254, 1), (126, 3), (30, 2), (17, 1), (2, 1)]


@pytest.mark.parametrize("n,B", SHAPES)
@pytest.mark.parametrize("d", [16, 32, 64])
def test_block_kernel_dense_f16x2(cuda, d, n, B):
    """conv2d_dblock_kernel<2, 1> in one launch with the Decoder's grid, dense normal weights (1 / sqrt(9 cin)), every pixel and channel: ragged
    sub-images (250, 126), no pad column (256), one pad column pair (254), n < d (one-pixel sub-images, the early exit), odd n, B = 3.
    Worst observed 6.33e-7 (d = 16), 6.25e-7 (d = 32), 5.57e-7 (d = 64); bound KERNEL_BOUND = 3e-6."""
    convs = R.dense_block(100 + d)
    x = R.m16_exact(torch.from_numpy(np.random.RandomState(n + d).randn(B, 64, n, n).astype(np.float32)))
    got = engine.conv2d_dblock(x.to(cuda), convs, d).cpu().numpy()
    err = rel_err(got, R.block_ref(convs, d, x))
    print(f"block kernel f16x2 d={d} n={n} B={B}: rel_err {err:.3g}")
    assert err <= KERNEL_BOUND


@pytest.mark.parametrize("n", [250, 30])
@pytest.mark.parametrize("d", [16, 32, 64])
@pytest.mark.parametrize("precision", ["f16x2", "f16", "bf16"])
def test_block_kernel_exact_case(cuda, precision, d, n):
    """Sparse weights in {0, +-1, +-0.5}, each through a different off-centre tap, integer biases, integer impulses at the corners, on row and
    column n - 1 and on both sides of a sub-image border (decoder_ref.exact_block / exact_input; exactly representable in every format,
    test_decoder_stages_cpu.py): the output EQUALS the fp64 reference - a swapped tap, channel half, residual or sub-image index is an O(1)
    difference here, in all three arithmetic modes."""
    x = R.exact_input(n, 2, d)
    got = engine.conv2d_dblock(x.to(cuda), R.exact_block(), d, precision).cpu().numpy()
    assert np.array_equal(got.astype(np.float64), R.exact_ref(n, 2, d))


@pytest.mark.parametrize("n,B", [(250, 2), (30, 2)])
@pytest.mark.parametrize("precision", ["f16", "bf16"])
def test_block_kernel_dense_single_plane(cuda, precision, n, B):
    """The single-plane modes on the dense weights, input rounded to the plane's type; the kernel rounds the weights and the three
    intermediate maps to 11 (8) bits.  Worst observed, f16: 5.67e-4 (n = 250), 5.42e-4 (n = 30); bf16: 4.86e-3 (n = 250), 5.21e-3 (n = 30);
    bound PLANE_BOUND = 3e-3 (f16), 3e-2 (bf16)."""
    worst = 0.0
    for d in (16, 32, 64):
        convs = R.dense_block(100 + d)
        x = R.m16_exact(torch.from_numpy(np.random.RandomState(n + d).randn(B, 64, n, n).astype(np.float32)), precision)
        got = engine.conv2d_dblock(x.to(cuda), convs, d, precision).cpu().numpy()
        err = rel_err(got, R.block_ref(convs, d, x))
        print(f"block kernel {precision} d={d} n={n} B={B}: rel_err {err:.3g}")
        worst = max(worst, err)
    assert worst <= PLANE_BOUND[precision]


# ---- the head launch ------------------------------------------------------------------------------------------------------------------------
def _elementwise(got, ref):
    """|d| <= 2^-20 |ref| + 2^-22: two fp16 planes keep 22 bits above a subnormal floor of 2^-24; fp32 round-off of the interpolation."""
    d = np.abs(got.astype(np.float64) - ref)
    return bool((d <= 2.0 ** -20 * np.abs(ref) + 2.0 ** -22).all()), float((d / (2.0 ** -20 * np.abs(ref) + 2.0 ** -22)).max())


@pytest.mark.parametrize("n", [250, 30, 2])
@pytest.mark.parametrize("T", [1, 3])
@pytest.mark.parametrize("mode", ["bilinear", "nearest"])
def test_head_distenc_chunk_and_upsampled_prediction(cuda, mode, T, n):
    """decoder_head_m16_kernel's two map roles at B = 2: stage 0 = distenc in channels 0..T-1, channels 64..79 of stage 2 = the up-sampled
    coarse prediction; x is a transposed view (channel stride 1).  Elementwise bound above; padding channels exactly 0.
    Worst observed: 0.12 of the bound (distenc), 0.40 of it (up-sampled y)."""
    m = _module(cuda, "Decoder", 0, num_2d=T, mode=mode)
    x, de, y = R.inputs(n, 2, T)
    xd = x.transpose(1, 2).contiguous().to(cuda).transpose(1, 2)
    assert not xd.is_contiguous() or n == 1
    ded, yd = _dev(cuda, de, y)
    in0, up = R.head(x, de, y, mode)
    g0 = _probe(m, cuda, xd, ded, yd, 0)
    g2 = _probe(m, cuda, xd, ded, yd, 2)
    assert g0.shape == (2, 16, n, n) and g2.shape == (2, 80, n, n)
    ok0, w0 = _elementwise(g0[:, :T], in0[:, :T])
    ok2, w2 = _elementwise(g2[:, 64: 64 + T], up[:, :T])
    print(f"head {mode} T={T} n={n}: worst fraction of the elementwise bound {w0:.3g} (distenc), {w2:.3g} (up-sampled y)")
    assert ok0 and ok2
    assert not g0[:, T:].any() and not g2[:, 64 + T:].any()
    # the same stage-2 map from a contiguous x: the strides are the only difference
    assert np.array_equal(_probe(m, cuda, x.to(cuda), ded, yd, 2), g2)


def test_head_outer_sum_of_the_decoder_1m(cuda):
    """Stage 0 of a Decoder_1m: x_i + x_j in 128 channels (the outer-sum role), n = 250 and 2, B = 2; same elementwise bound.
    Worst observed: 0.12 of the bound."""
    m = _module(cuda, "Decoder_1m", 2)
    for n in (250, 2):
        x, _, _ = R.inputs(n, 2)
        g = _probe(m, cuda, x.to(cuda), None, None, 0)
        ok, w = _elementwise(g, R.outer_sum(x))
        print(f"outer sum n={n}: worst fraction of the elementwise bound {w:.3g}")
        assert g.shape == (2, 128, n, n) and ok


# ---- separable first conv, combinerD, block 0 -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [250, 254, 30, 2])
@pytest.mark.parametrize("with_y", [True, False])
@pytest.mark.parametrize("seed", R.SEEDS)
def test_first_conv_combinerD_and_block0(cuda, seed, with_y, n):
    """Stage 1 (sep_tables_body + the `tab` epilogue of the per-layer kernel on the distenc chunk alone) from the encoding and the GPU's
    stage 0; stage 2 channels 0..63 (three convs, residual) from the GPU's stage 1; stage 3 (block 0: lcombiner / combiner on the 80-channel
    map with y, lconvtwos.0 / convtwos.0 without) from the GPU's stage 2.  B = 2.  Worst observed: first conv 7.2e-7 (bound FIRST_BOUND = 3e-6),
    combinerD 1.54e-6 (bound MAT_BOUND = 7e-6), block 0 9.45e-7 (bound BLOCK0_BOUND = 4e-6); all three at n = 250 or 254."""
    m = _module(cuda, "Decoder", seed)
    sd = R.decoder_sd("Decoder", seed)
    x, de, y = R.inputs(n, 2)
    y = y if with_y else None
    xd, ded, yd = _dev(cuda, x, de, y)
    g = [_probe(m, cuda, xd, ded, yd, k) for k in range(4)]
    assert g[2].shape[1] == (80 if with_y else 64)
    errs = (rel_err(g[1], R.first(sd, x, g[0])), rel_err(g[2][:, :64], R.mat(sd, g[1])), rel_err(g[3], R.block(sd, "Decoder", 0, g[2])))
    print(f"seed {seed} y={with_y} n={n}: first conv {errs[0]:.3g}, combinerD {errs[1]:.3g}, block 0 {errs[2]:.3g}")
    assert errs[0] <= FIRST_BOUND and errs[1] <= MAT_BOUND and errs[2] <= BLOCK0_BOUND


# ---- every block of the chain ---------------------------------------------------------------------------------------------------------------
CHAINS = {"dec250": ("Decoder", 0, 250, 2), "dec1m": ("Decoder_1m", 2, 250, 1), "dec254": ("Decoder", 2, 254, 1), "dec30": ("Decoder", 2, 30, 2)}
BLOCKS = ([("dec250", i) for i in range(1, 28)] + [("dec1m", i) for i in range(19)] +
          [(c, i) for c in ("dec254", "dec30") for i in list(range(1, 8)) + [27]])
_worst = {}


@pytest.mark.parametrize("chain,i", BLOCKS)
def test_every_block_of_the_chain(cuda, chain, i):
    """Block i of the production chain: fp64 `decoder_block` on the GPU's stage 2 + i against the GPU's stage 3 + i.  Decoder with y at
    n = 250, B = 2 (the four-row kernel and the block kernel): blocks 1..27; Decoder_1m at n = 250, B = 1 (the one-row kernel): 0..18;
    Decoder at n = 254 (B = 1) and 30 (B = 2): 1..7 and 27.  At n = 254 a block kernel's out-of-map pixels are gathered from pad pixel 255
    of row 0, which the per-layer kernel in front must have left zero.  Prints the worst block per dilation so far.
    Worst observed per dilation 1 / 2 / 4 / 8 / 16 / 32 / 64 (x 1e-7) - Decoder n = 250: 6.2, 7.1, 7.5, 6.0, 6.6, 5.8, 5.3; Decoder_1m:
    12.6, 6.5, 6.3, 7.0, 7.4, 7.8, 7.2; n = 254: 6.2, 9.0, 6.2, 6.2, 4.3, 4.9, 4.5; n = 30: 6.2, 7.2, 6.0, 4.4, 2.6, 2.0, 2.4.
    Worst of all 1.26e-6 (Decoder_1m, d = 1); bound BLOCK_BOUND = 6e-6."""
    kind, seed, n, B = CHAINS[chain]
    m = _module(cuda, kind, seed)
    sd = R.decoder_sd(kind, seed)
    x, de, y = R.inputs(n, B)
    xd, ded, yd = _dev(cuda, x, de, y) if kind == "Decoder" else (x.to(cuda), None, None)
    src = _probe(m, cuda, xd, ded, yd, 2 + i if i > 0 else 0)
    got = _probe(m, cuda, xd, ded, yd, 3 + i)
    err = rel_err(got, R.block(sd, kind, i, src))
    d = R.DIL[kind][i]
    if err > _worst.get((chain, d), (-1.0, 0))[0]:
        _worst[(chain, d)] = (err, i)
    print(f"{chain} block {i} d={d}: rel_err {err:.3g}; worst at this dilation so far {_worst[(chain, d)][0]:.3g} (block {_worst[(chain, d)][1]})")
    assert err <= BLOCK_BOUND


# ---- final ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [250, 254, 18, 2])
@pytest.mark.parametrize("T", [1, 3])
def test_final_head_symmetrisation_and_accumulate(cuda, T, n):
    """final_sym_m16_kernel (136 tile pairs, ragged last tiles): the forward's output against fp64 `final` + symmetrisation of the GPU's
    last-stage probe, B = 2, 64 -> max(5, T) -> T; the output is exactly symmetric; accumulate adds into a pre-filled `out`.
    Worst observed 4.69e-7 (T = 3, n = 250); bound FINAL_BOUND = 2e-6.  Accumulate, elementwise: |acc - (pre + out)| <= 2^-23 |pre + out|
    (+ 2^-126), twice the half ulp of the one fp32 addition; worst observed 0.5 of it."""
    m = _module(cuda, "Decoder", 2, num_2d=T)
    sd = R.decoder_sd("Decoder", 2, num_2d=T)
    x, de, y = R.inputs(n, 2, T)
    xd, ded, yd = _dev(cuda, x, de, y)
    last = _probe(m, cuda, xd, ded, yd, 30)
    net = _net(m, cuda)
    out = engine.decoder_forward(net, xd, ded, yd)
    assert not net.ctx.take_overflow() and out.shape == (2, T, n, n)
    err = rel_err(out.cpu().numpy(), R.final(sd, last))
    print(f"final T={T} n={n}: rel_err {err:.3g}")
    assert err <= FINAL_BOUND
    assert torch.equal(out, out.transpose(2, 3))
    pre = torch.from_numpy(np.random.RandomState(n).randn(2, T, n, n).astype(np.float32)).to(cuda)
    acc = engine.decoder_forward(net, xd, ded, yd, out=pre.clone(), accumulate=True)
    # elementwise: the kernel adds the same fp32 value to what `out` held, one rounding of the sum (half an ulp; a factor of 2 allowed)
    want = pre.double() + out.double()
    frac = float(((acc.double() - want).abs() / (2.0 ** -23 * want.abs() + 2.0 ** -126)).max())
    print(f"final T={T} n={n}: accumulate, worst fraction of the elementwise bound {frac:.3g}")
    assert frac <= 1.0


# ---- argument checks --------------------------------------------------------------------------------------------------------------------------
def test_probe_and_block_entry_refuse_what_they_cannot_run(cuda):
    from orca_amd import _lib
    m = _module(cuda, "Decoder", 0)
    m1 = _module(cuda, "Decoder_1m", 0)
    x, de, y = _dev(cuda, *R.inputs(30, 1))
    net, net1 = _net(m, cuda), _net(m1, cuda)
    out = torch.empty((1, 128, 30, 30), device=cuda)

    def raw(n_, dp, yp, stage, channels):
        return _lib.load().orca_decoder_probe(n_.ctx.handle, n_.handle, x.data_ptr(), x.stride(0), x.stride(1), x.stride(2), dp, 0, 900, 30, 1, yp,
                                              225, 225, 15, 1, 1, 30, stage, channels, out.data_ptr())
    assert raw(net, de.data_ptr(), y.data_ptr(), 3, 64) == 0
    for stage, ch in ((31, 64), (-1, 64), (0, 64), (1, 80), (2, 64), (5, 32)):           # no such stage / a channel mismatch
        assert raw(net, de.data_ptr(), y.data_ptr(), stage, ch) == -1, (stage, ch)
    assert raw(net, de.data_ptr(), None, 2, 80) == -1 and raw(net, de.data_ptr(), None, 2, 64) == 0
    assert raw(net1, None, None, 0, 128) == 0 and raw(net1, None, None, 21, 64) == 0
    for stage, ch in ((1, 64), (2, 64), (22, 64), (0, 16)):
        assert raw(net1, None, None, stage, ch) == -1, (stage, ch)
    assert raw(net1, de.data_ptr(), None, 3, 64) == -1                                     # a Decoder_1m takes no distenc
    # an exact-fp32 net hands out its fp32 planes: the whole 136-channel input map, A with the 8 planes of the up-sampled y
    netf, netf1 = _net(_module(cuda, "Decoder", 0, precision="f32"), cuda), _net(_module(cuda, "Decoder_1m", 0, precision="f32"), cuda)
    assert [tuple(engine.decoder_probe(netf, x, de, yy, k).shape[1:]) for k, yy in ((0, y), (1, y), (2, y), (2, None), (3, y), (30, y))] == \
        [(136, 30, 30), (64, 30, 30), (72, 30, 30), (64, 30, 30), (64, 30, 30), (64, 30, 30)]
    assert [tuple(engine.decoder_probe(netf1, x, None, None, k).shape) for k in (0, 3, 21)] == [(1, 128, 30, 30), (1, 64, 30, 30), (1, 64, 30, 30)]
    for stage, ch in ((31, 64), (-1, 64), (0, 16), (0, 128), (1, 72), (2, 80), (2, 64), (5, 32)):   # no such stage / a channel mismatch
        assert raw(netf, de.data_ptr(), y.data_ptr(), stage, ch) == -1, (stage, ch)
    assert raw(netf, de.data_ptr(), None, 2, 72) == -1
    for stage, ch in ((1, 64), (2, 64), (22, 64), (0, 136)):
        assert raw(netf1, None, None, stage, ch) == -1, (stage, ch)
    # the block entry
    convs = R.dense_block(1)
    xb = torch.zeros((1, 64, 30, 30), device=cuda)
    assert engine.conv2d_dblock(xb, convs, 16).shape == xb.shape
    for dil in (8, 1, 128, 48):
        with pytest.raises(OrcaHipError):
            engine.conv2d_dblock(xb, convs, dil)

    def raw_block(dils):                                                                   # one dilation per conv
        descs = engine.make_descs([{"w": w, "b": b, "cout": w.shape[0], "cin": w.shape[1], "k": 3, "dil": dl} for (w, b), dl in zip(convs, dils)])
        return _lib.load().orca_conv2d_dblock_forward(engine.get_context(cuda).handle, descs, _lib.PRECISIONS["f16x2"], xb.data_ptr(),
                                                      torch.empty_like(xb).data_ptr(), 1, 30)
    assert raw_block((16, 16, 16, 16)) == 0 and raw_block((16, 16, 32, 16)) == -1 and raw_block((32, 16, 16, 16)) == -1
    with pytest.raises(OrcaHipError):
        engine.conv2d_dblock(xb, convs, 16, precision="f32")
    with pytest.raises(OrcaHipError):
        engine.conv2d_dblock(xb, convs, 16, precision="bf16x3")
    with pytest.raises(OrcaHipError):
        engine.conv2d_dblock(xb, [convs[1], convs[0], convs[2], convs[3]], 16)
    with pytest.raises(OrcaHipError):
        engine.conv2d_dblock(torch.zeros((1, 64, 257, 257), device=cuda), convs, 16)
