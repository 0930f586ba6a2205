"""-m gpu: a run of Decoder blocks of dilation 16, 32, 64 in ONE launch (conv2d_dblock_run_kernel, f16x2) against the per-block launches of
conv2d_dblock_kernel it replaces.  The yardstick is BIT equality: the per-block path is bounded against fp64 by
tests/test_gpu_decoder_stages.py, and equality carries that bound over - no new numeric bound is introduced here."""
import numpy as np
import pytest
import torch

from orca_amd import engine
from orca_amd._lib import OrcaHipError
from tests import decoder_ref as R
from tests.decoder_ref import rel_err
from tests.util import product_module

pytestmark = pytest.mark.gpu

RUNS = [(16, 3), (16, 2), (32, 2)]                       # (first dilation, blocks); production: (16, 3)
# ragged sub-images (250, 126, 130), no pad column (256), one pad column pair (254), dilation 64 reaching across the map (130), n < d (30,
# 17, 2: one-pixel sub-images, the early exit), odd n and odd batches
SHAPES = [(250, 2), (256, 1), (254, 1), (130, 1), (30, 2), (17, 1), (2, 1), (126, 3)]


def _run_convs(d0, nblk):
    return [c for b in range(nblk) for c in R.dense_block(1000 + 10 * d0 + b)]


def _chain_ref(convs, d0, x):
    for b in range(len(convs) // 4):
        x = R.block_ref(convs[4 * b: 4 * b + 4], d0 << b, x)
    return x


@pytest.mark.parametrize("n,B", SHAPES)
@pytest.mark.parametrize("d0,nblk", RUNS)
def test_run_kernel_equals_per_block_launches(cuda, d0, nblk, n, B):
    """One fused launch == nblk per-block launches on the same M16 buffer, bit for bit; dense weights (a different seed per block), inputs
    exact in two fp16 planes.  Prints the fused result's rel_err against the fp64 chain for the record (no bound: equality carries the
    per-block bound of test_gpu_decoder_stages.py over)."""
    convs = _run_convs(d0, nblk)
    x = R.m16_exact(torch.from_numpy(np.random.RandomState(7 * n + d0 + nblk).randn(B, 64, n, n).astype(np.float32)))
    xd = x.to(cuda)
    fused = engine.conv2d_dblock_run(xd, convs, d0, fused=True)
    chain = engine.conv2d_dblock_run(xd, convs, d0, fused=False)
    assert not engine.get_context(cuda).take_overflow()
    print(f"block run d0={d0} nblk={nblk} n={n} B={B}: fused rel_err vs fp64 chain {rel_err(fused.cpu().numpy(), _chain_ref(convs, d0, x)):.3g}")
    assert torch.equal(fused, chain)


@pytest.mark.parametrize("n", [250, 30])
@pytest.mark.parametrize("d0,nblk", RUNS)
def test_run_kernel_exact_case(cuda, d0, nblk, n):
    """decoder_ref.exact_block chained nblk times on exact_input in fp64: every intermediate is first confirmed (CPU) to be exactly representable
    in two fp16 planes, then the fused run's output EQUALS the fp64 result - a wrong neighbour stride, tap or sub-image index is an O(1)
    difference here."""
    convs = R.exact_block() * nblk
    x = R.exact_input(n, 2, d0)
    cur = x.numpy().astype(np.float64)
    for b in range(nblk):
        cur = R.block_ref(convs[:4], d0 << b, cur)
        assert np.array_equal(R.m16_exact(cur.astype(np.float32)).numpy().astype(np.float64), cur), f"block {b}: not exact in two fp16 planes"
    got = engine.conv2d_dblock_run(x.to(cuda), convs, d0, fused=True).cpu().numpy()
    assert not engine.get_context(cuda).take_overflow()
    assert np.array_equal(got.astype(np.float64), cur)


def test_run_kernel_raises_the_flag_for_an_intermediate_block(cuda):
    """Block 0's last conv is scaled until its output leaves the fp16 range; blocks 1 and 2 have zero weights and biases, so behind block 0
    nothing but 0 and NaN exists (0 x inf) and no later range check can fire: the flag comes from the intermediate block's own check, in the
    fused launch as in the per-block ones, and the (invalid) results still agree bit for bit."""
    convs = R.dense_block(5)
    convs[3] = (convs[3][0] * 1.0e5, convs[3][1])
    convs += [(np.zeros_like(w), np.zeros_like(b)) for w, b in R.dense_block(5)] * 2
    x = R.m16_exact(torch.from_numpy(np.random.RandomState(3).randn(2, 64, 30, 30).astype(np.float32))).to(cuda)
    ctx = engine.get_context(cuda)
    assert not ctx.take_overflow()
    outs = []
    for fused in (True, False):
        outs.append(engine.conv2d_dblock_run(x, convs, 16, fused=fused))
        assert ctx.take_overflow(), f"fused={fused}"
    assert torch.equal(outs[0].view(torch.int32), outs[1].view(torch.int32))
    # below the range: no flag
    engine.conv2d_dblock_run(x, R.dense_block(5) * 3, 16)
    assert not ctx.take_overflow()


# ---- the whole forward ------------------------------------------------------------------------------------------------------------------------
_modules = {}


def _module(cuda, kind, seed=0, precision="f16x2"):
    key = (kind, seed, precision)
    if key not in _modules:
        kw = {"upsample_mode": "bilinear"} if kind == "Decoder" else {}
        _modules[key] = product_module(kind, seed, device=cuda, precision=precision, **kw)
    return _modules[key]


def _net(m, cuda, runs):
    net = m._net(cuda)
    m._apply_precision(net, m.precision)
    net.set_decoder_block_runs(runs)
    return net


def _args(cuda, kind, with_y, n, B):
    x, de, y = R.inputs(n, B)
    if kind == "Decoder_1m":
        return x.to(cuda), None, None
    return x.to(cuda), de.to(cuda), y.to(cuda) if with_y else None


@pytest.mark.parametrize("n,B", [(250, 2), (130, 1)])
@pytest.mark.parametrize("kind,with_y", [("Decoder", True), ("Decoder", False), ("Decoder_1m", False)])
def test_forward_and_probes_equal_with_runs_on_and_off(cuda, kind, with_y, n, B):
    """The forward's output, and the probes behind the 16, 32 and 64 blocks of the first run (blocks 4, 5, 6 of both Decoders: stages 7, 8,
    9 - a probe at 7 or 8 breaks the run), are bit-identical with orca_net_set_decoder_block_runs on and off."""
    m = _module(cuda, kind)
    x, de, y = _args(cuda, kind, with_y, n, B)
    got = {}
    try:
        for runs in (True, False):
            net = _net(m, cuda, runs)
            out = engine.decoder1m_forward(net, x) if kind == "Decoder_1m" else engine.decoder_forward(net, x, de, y)
            got[runs] = [out] + [engine.decoder_probe(net, x, de, y, st) for st in (7, 8, 9)]
            assert not net.ctx.take_overflow()
    finally:
        m._net(cuda).set_decoder_block_runs(True)
    assert got[True][0].shape == (B, 1, n, n) and bool(torch.isfinite(got[True][0]).all())
    for a, b in zip(got[True], got[False]):
        assert torch.equal(a, b)


def test_forward_overflow_flag_of_an_intermediate_block(cuda):
    """convtwos.4 (dilation 16, the first block of the first run) with its last BatchNorm scaled by 1e5: its output, which the fused launch
    never stores, leaves the fp16 range - the flag fires with block runs on and off; with the unscaled weights it does not."""
    sd = {k: np.array(v, copy=True) for k, v in R.decoder_sd("Decoder", 0).items()}
    sd["convtwos.4.4.weight"] *= 1.0e5
    sd["convtwos.4.4.bias"] *= 1.0e5
    from orca_amd import orca_modules as pm
    m = pm.Decoder(upsample_mode="bilinear")
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    m.eval().to(cuda)
    m.precision = "f16x2"
    x, de, y = _args(cuda, "Decoder", True, 130, 1)
    for runs in (True, False):
        net = _net(m, cuda, runs)
        engine.decoder_forward(net, x, de, y)
        assert net.ctx.take_overflow(), f"runs={runs}"
    net = _net(_module(cuda, "Decoder"), cuda, True)
    engine.decoder_forward(net, x, de, y)
    assert not net.ctx.take_overflow()


# ---- option plumbing --------------------------------------------------------------------------------------------------------------------------
def test_option_is_refused_on_an_encoder_and_leaves_the_single_plane_modes_alone(cuda):
    enc = product_module("Encoder", 0, device=cuda)
    with pytest.raises(OrcaHipError, match="not a Decoder"):
        enc._net(cuda).set_decoder_block_runs(True)
    x, de, y = _args(cuda, "Decoder", True, 130, 1)
    for precision in ("bf16", "f16"):
        m = _module(cuda, "Decoder", 0, precision)
        try:
            outs = [engine.decoder_forward(_net(m, cuda, runs), x, de, y) for runs in (True, False)]
        finally:
            m._net(cuda).set_decoder_block_runs(True)
        assert torch.equal(outs[0], outs[1]), precision
    with pytest.raises(OrcaHipError):
        engine.conv2d_dblock_run(torch.zeros((1, 64, 30, 30), device=cuda), R.dense_block(1) * 3, 16, precision="bf16")
    with pytest.raises(OrcaHipError):
        engine.conv2d_dblock_run(torch.zeros((1, 64, 30, 30), device=cuda), R.dense_block(1) * 3, 32)      # 32, 64, 128
    with pytest.raises(OrcaHipError):
        engine.conv2d_dblock_run(torch.zeros((1, 64, 30, 30), device=cuda), R.dense_block(1) * 2, 64)
