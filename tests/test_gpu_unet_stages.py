"""-m gpu: Encoder2 / Encoder3 / Encoder2b (`orca_unet_forward`) level by level - every level, every position, all 128 channels - against
the oracle's fp64 walk (tests/unet_ref.py), weight seeds 0 and 1.

Paths, from orca_encoder.hip.  "f32": the exact fp32-MFMA kernels on channel-major rows (`launch_conv1d`, `upsample1d_x2_kernel`,
`launch_pool`).  Every other precision: `unet_forward_nlc` - the input staged channel-last by `transpose2d_kernel` (unit position stride)
or `copy2d_flat_kernel` (a position-strided view); per level `maxpool1d_nlc_kernel<2>` over the B * n rows of all batch entries, four
`launch_conv1d_b16` convs (levels of <= 2 048 positions: conv1d_k9_small_kernel; longer ones: conv1d_k9_bf16s_kernel, for f16x2 with
64-position tiles while ceil(n / 256) * B < 200); on the expanding path `upsample1d_x2_nlc_kernel` (row m reads row m >> 1) and the last conv
with r2 = y = `encs[lev]` (the skip connection, read and overwritten in one launch); every output handed over by `transpose2d_kernel`
(32 x 32 tiles: ragged at level sizes that are no multiples of 32).

BOUND.  Not fixed in advance: for each case E32 = max over the levels of rel_err(fp32 walk, fp64 walk) on the CPU (rel_err normalises by
max(1, max |ref|); 3.7e-7 at n = 8 .. 1.5e-6 at n >= 800), and every level must stay within 4 E32 for "f32" (the fp32 MFMA chain differs from
torch only in summation order) and 8 E32 for "f16x2" and "bf16x3" (an fp64 walk on operands rounded to hi + lo fp16 stayed under 2.5 E32:
about three times that is left for the summation order).  bf16 is left out: lossy by design, pinned by rounding-point emulation in
test_gpu_config3.py.

Observed on the MI355X, worst rel_err / E32 over all levels, sizes, seeds, batches and layouts:
             f32    f16x2   bf16x3
  Encoder2   3.43   3.50    1.98
  Encoder3   3.61   3.03    2.44
  Encoder2b  3.07   3.02    1.61     (the same on Encoder2's contracting weights)
The largest ratios belong to the smallest inputs (f32 3.61 at Encoder3 n = 24, 3.43 and f16x2 3.50 at Encoder2 n = 32; n >= 800: f32 <= 3.07,
f16x2 <= 3.03), where E32 is a maximum over few values: "f32" comes within 10 % of its factor of 4 there, the 16-bit modes use less than half of
their 8."""
import ctypes

import numpy as np
import pytest
import torch

from orca_amd import _lib
from orca_amd import orca_modules as pm
from orca_amd._lib import OrcaHipError
from tests import unet_ref as R
from tests.unet_ref import rel_err
from tests.util import product_module

pytestmark = pytest.mark.gpu
PRECISIONS = ["f32", "f16x2", "bf16x3"]
FACTOR = {"f32": 4.0, "f16x2": 8.0, "bf16x3": 8.0}

CASES = ([("Encoder2", n) for n in (32, 96, 800, 2048, 2080, 4160)] + [("Encoder3", n) for n in (8, 24, 2000, 4112)]
         + [("Encoder2b", n) for n in (32, 800, 4160)] + [("Encoder2b<-Encoder2", n) for n in (32, 800, 4160)])


def _module(kind, seed, precision):
    if kind == "Encoder2b<-Encoder2":
        m = pm.Encoder2b(precision=precision)
        m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in R.unet_sd(kind, seed).items()}, strict=True)
        return m.eval()
    return product_module(kind, seed, precision=precision)


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("seed", R.SEEDS)
@pytest.mark.parametrize("kind,n", CASES)
def test_every_level_against_the_fp64_walk(cuda, kind, n, seed, precision):
    """Every level of every network against the fp64 walk, B = 1 and 3, input contiguous, a `[:, :, ::2]` view, and a batch-and-position slice
    of a larger tensor (odd offset); the tensor that owns the input is bit-unchanged afterwards.
    Encoder2 (5 levels, n % 32 == 0): n = 32 and 96 end in levels of 1 and 3 positions (one workgroup column of conv_small.h, ragged
    32 x 32 transposes); 800 and 2 048 run every conv on conv1d_k9_small_kernel (n <= 2048 at every level); 2 080 has only the last expanding
    level (2 080 positions) on conv1d_k9_bf16s_kernel - its r2 = y launch included; 4 160 has level 0 (4 160) and level 1 (2 080) beyond
    2 048 on both paths.  Encoder3 (3 levels, n % 8 == 0): 8, 24 (levels of 1 and 3), 2 000, 4 112 (levels 4 112 and 2 056 beyond).
    Encoder2b (the contracting path as output): 32, 800, 4 160 - also on Encoder2's contracting weights ("Encoder2b<-Encoder2"), which checks
    Encoder2's contracting levels 1..4 one by one (its own outputs show only the expanding path's).
    For f16x2 the long levels take 64-position tiles (ceil(4160 / 256) * 3 = 51 < 200); bf16x3 always the 256-position ones.
    Observed on the MI355X: see the module docstring."""
    _, w64 = R.walks(kind, seed, n)
    mod = _module(kind, seed, precision)
    sizes = R.level_sizes(kind, n)
    worst = 0.0
    for B in (1, 3):
        e32 = R.e32(kind, seed, n, B)
        bound = FACTOR[precision] * e32
        x = R.values(n)[:B]
        for layout in R.LAYOUTS:
            owner, view = R.device_input(x, layout, cuda)
            keep = owner.clone()
            ys = mod(view)
            assert torch.equal(owner, keep), (layout, "the input was written")
            assert [tuple(y.shape) for y in ys] == [(B, 128, m) for m in sizes]
            for lev, y in enumerate(ys):
                err = rel_err(y.cpu().numpy(), w64[lev][:B])
                worst = max(worst, err / e32)
                assert err <= bound, (kind, n, seed, precision, B, layout, lev, err, e32)
    print(f"{kind} n = {n} seed {seed} {precision}: worst rel_err / E32 = {worst:.3g} (bound {FACTOR[precision]:g})")


@pytest.mark.parametrize("precision", ["f16x2", "bf16x3"])
@pytest.mark.parametrize("kind,n", [("Encoder2", 96), ("Encoder2", 2048), ("Encoder3", 2000), ("Encoder2b", 800)])
def test_row_of_a_batch_is_the_row_alone(cuda, kind, n, precision):
    """n <= 2 048: every conv runs conv1d_k9_small_kernel (one workgroup per 32 positions x 32 couts of ONE row: grid.y = B), the pool and
    the upsample work on B * n rows with n even: row 1 of B = 3 is bit-equal to that row run alone, at every level."""
    mod = _module(kind, 0, precision)
    x = R.values(n).to(cuda)
    for a, b in zip(mod(x), mod(x[1:2])):
        assert torch.equal(a[1:2], b)


def test_batch_flips_the_tile_rule_at_the_last_level(cuda):
    """Encoder2, f16x2, n = 2 336: level 0 (2 336 positions, conv1d_k9_bf16s_kernel) is 10 tiles of 256 per row - B = 20 makes 200 and takes
    the 256-position tile, B = 1 the 64-position one; every other level (<= 1 168) runs conv1d_k9_small_kernel.  Every row of B = 20 within
    8 E32 at every level, and bit-equal to the row run alone (rows 0, 7 and 19; the two tile shapes add their products in one order,
    test_gpu_conv1d_nlc.py).
    Observed on the MI355X: E32 = 1.45e-6, worst row 2.67 E32; the rows were bit-equal."""
    n, B = 2336, 20
    sd = R.unet_sd("Encoder2", 0)
    x = torch.from_numpy((np.random.RandomState(2336).rand(B, 128, n) * 0.5).astype(np.float32))
    w32, w64 = R.walk("Encoder2", sd, x, torch.float32), R.walk("Encoder2", sd, x, torch.float64)
    e32 = max(rel_err(a, b) for a, b in zip(w32, w64))
    mod = _module("Encoder2", 0, "f16x2")
    xd = x.to(cuda)
    ys = mod(xd)
    worst = 0.0
    for lev, y in enumerate(ys):
        got = y.cpu().numpy()
        for row in range(B):
            worst = max(worst, rel_err(got[row], w64[lev][row]) / e32)
    print(f"Encoder2 n = {n} B = {B} f16x2: E32 = {e32:.3g}, worst row rel_err / E32 = {worst:.3g} (bound 8)")
    assert worst <= 8.0
    for row in (0, 7, 19):
        for a, b in zip(ys, mod(xd[row:row + 1])):
            assert torch.equal(a[row:row + 1], b), (row, a.shape)


def test_position_strided_input_of_65568_bins(cuda):
    """The staging of a position-strided input (`copy2d_flat_kernel`: its rows are not a grid dimension, where `copy2d_kernel` had the n
    positions in gridDim.y and was refused from 65 536 on): Encoder2, f16x2, B = 1, n = 65 568 as a `[:, :, ::2]` view is bit-equal, at every
    level, to the contiguous copy of the same data (which `transpose2d_kernel` stages)."""
    n = 65568
    mod = _module("Encoder2", 0, "f16x2")
    gen = torch.Generator(device=cuda)
    gen.manual_seed(65568)
    big = torch.rand((1, 128, 2 * n), device=cuda, generator=gen) * 0.5
    view = big[:, :, ::2]
    assert view.stride(2) == 2
    ys = mod(view)
    for a, b in zip(ys, mod(view.contiguous())):
        assert tuple(a.shape) == tuple(b.shape) and torch.equal(a, b)
    assert float(ys[0].abs().max()) > 0


def test_argument_checks(cuda):
    """ORCA_EINVAL with nothing launched (no conv launch counted, the outputs still hold their sentinel): n not a multiple of 32 (Encoder2) or
    8 (Encoder3), a wrong number of output pointers, a decoder net."""
    lib = _lib.load()

    def refused(net, n, n_outs):
        x = torch.zeros((1, 128, max(n, 1)), dtype=torch.float32, device=cuda)
        outs = [torch.full((1, 128, max(n, 1)), -777.0, dtype=torch.float32, device=cuda) for _ in range(n_outs)]
        ptrs = (ctypes.c_void_p * n_outs)(*[o.data_ptr() for o in outs])
        before = net.ctx.launch_counts()
        rc = lib.orca_unet_forward(net.ctx.handle, net.handle, ctypes.c_void_p(x.data_ptr()), x.stride(0), x.stride(1), x.stride(2), 1, n, ptrs, n_outs)
        torch.cuda.synchronize()
        assert rc == -1, (n, n_outs, rc)                         # ORCA_EINVAL
        assert net.ctx.launch_counts() == before
        assert all(float(o.min()) == float(o.max()) == -777.0 for o in outs)

    for precision in ("f16x2", "f32"):
        e2, e3 = _module("Encoder2", 0, precision), _module("Encoder3", 0, precision)
        n2, n3 = e2._net(cuda), e3._net(cuda)
        e2._apply_precision(n2, precision)
        e3._apply_precision(n3, precision)
        for n in (0, 16, 48, 2047, 2049):
            refused(n2, n, 6)
        for n in (0, 4, 12, 2001):
            refused(n3, n, 4)
        refused(n2, 64, 5)
        refused(n2, 64, 7)
        refused(n3, 64, 6)
        with pytest.raises(OrcaHipError, match="orca_unet_forward"):
            e2(torch.zeros((1, 128, 48), device=cuda))
    dec = product_module("Decoder", 0, upsample_mode="bilinear")
    refused(dec._net(cuda), 64, 6)
