"""-m gpu: the channel-last split-operand conv1d launcher (`launch_conv1d_b16`: conv_small.h up to 2 048 positions, conv_bf16s.h beyond and
whenever MaxPool1d(4) is fused) with every argument the nets give it - second residual (also in place), fused pool, tile rule, persistent
walk - through `orca_conv1d_nlc_forward_full` (`engine.conv1d_nlc`), against `F.conv1d` in fp64 on the same fp32 operands.

Inputs as the sibling tests of test_gpu_kernels.py: randn, weights / sqrt(cin 9), bias 0.1 randn.  Bounds, max-abs, the project's own for
these kernels on these inputs: f16x2 and bf16x3 2e-5, bf16x2 3e-4, bf16 5e-2.

Dispatch, from orca_encoder.hip (`launch_conv1d_b16`, `launch_conv1d_b16_ns`):
  n <= 2048 and no pool4                       -> conv1d_k9_small_kernel (conv_small.h), whatever B, cout, fixed_tile
  else cout 64 / 96                            -> conv1d_k9_bf16s_kernel, 256-position tiles
  else cout 128, bf16x3                        -> 256-position tiles (launch_b16_t<128, 2, 2, 4, 2>)
  else cout 128, f16x2 / bf16x2 / bf16         -> 64-position tiles (launch_b16_t<128, 1, 2, 2, 2>) if fixed_tile != 1 and
                                                  ceil(n / 256) * (fixed_tile == 2 ? 1 : B) < 200, else the 256-position tiles.
                                                  fixed_tile = 1 reaches the rule for f16x2 only: for bf16x2 and bf16 the launcher hands on
                                                  `fixed_tile == 2 ? 2 : 0`, so there the 256-position tile is taken by the automatic rule alone."""
import ctypes
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from orca_amd import _lib, engine

pytestmark = pytest.mark.gpu
TOLS = {"f16x2": 2e-5, "bf16x3": 2e-5, "bf16x2": 3e-4, "bf16": 5e-2}
PRECISIONS = list(TOLS)


@functools.lru_cache(maxsize=None)
def _case(cin, cout, n, B):
    """(x [B,cin,n], w, b, r1, r2 [B,cout,n], fp64 conv + bias [B,cout,n]) - computed once and left unchanged."""
    rs = np.random.RandomState(cin * 1000 + cout + n + B)
    x = torch.from_numpy(rs.randn(B, cin, n).astype(np.float32))
    w = (rs.randn(cout, cin, 9) / np.sqrt(cin * 9)).astype(np.float32)
    b = rs.randn(cout).astype(np.float32) * 0.1
    r1 = torch.from_numpy(rs.randn(B, cout, n).astype(np.float32))
    r2 = torch.from_numpy(rs.randn(B, cout, n).astype(np.float32))
    conv = F.conv1d(x.double(), torch.from_numpy(w).double(), torch.from_numpy(b).double(), padding=4)
    return x, w, b, r1, r2, conv


def _nlc(t, cuda):
    return t.transpose(1, 2).contiguous().to(cuda)


def _ref(conv, relu, *res):
    y = F.relu(conv) if relu else conv
    for r in res:
        if r is not None:
            y = y + r.double()
    return y


def _err(y, ref):
    """max-abs of a channel-last device result against a channel-major fp64 reference."""
    return float((y.cpu().double().transpose(1, 2) - ref).abs().max())


# ---- 128 couts, 256-position tile ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["f16x2", "bf16x2", "bf16"])
@pytest.mark.parametrize("n", [2049, 2309])
def test_tile256_fixed_tile_and_batch_rows(cuda, precision, n):
    """conv_bf16s.h, launch_b16_t<128, 2, 2, 4, 2, NS <= 2, DT> (128 couts, 256-position tile) next to launch_b16_t<128, 1, 2, 2, 2> (64):
    (128, 128), B = 3, n = 2 049 (8 tiles of 256 + 1 position) and 2 309 (10 tiles, the last of 5 positions), with and without ReLU + r1.
    fixed_tile = 1: the 256-position tile for f16x2 (for bf16x2 / bf16 the launcher drops the request: 27 / 30 < 200 tiles give the
    64-position one); fixed_tile = 0: the 64-position tile (9 x 3, 10 x 3 < 200); fixed_tile = 2 ("what a B = 1 call takes"): the 64-position
    one, for all three.  Every position within the bound; a row of the batch is bit-equal to the row run alone; fixed_tile = 2 at B = 3 is
    bit-equal, row by row, to B = 1 calls with fixed_tile = 0; and the two tile shapes are bit-equal to each other (both walk chunks, taps
    and products in one order into one accumulator per output) - for f16x2 here, for bf16x2 / bf16 in the automatic-rule test below.
    Observed on the MI355X: see `test_tile256_automatic_rule`."""
    x, w, b, r1, _, conv = _case(128, 128, n, 3)
    xd, rd = _nlc(x, cuda), _nlc(r1, cuda)
    worst = 0.0
    for relu, ra, rad in [(False, None, None), (True, r1, rd)]:
        ref = _ref(conv, relu, ra)
        y1 = engine.conv1d_nlc(xd, w, b, precision, relu, rad, fixed_tile=1)
        y0 = engine.conv1d_nlc(xd, w, b, precision, relu, rad, fixed_tile=0)
        y2 = engine.conv1d_nlc(xd, w, b, precision, relu, rad, fixed_tile=2)
        for y in (y1, y0, y2):
            assert tuple(y.shape) == (3, n, 128)
            worst = max(worst, _err(y, ref))
        for row in range(3):
            ra1 = None if rad is None else rad[row:row + 1].contiguous()
            alone1 = engine.conv1d_nlc(xd[row:row + 1].contiguous(), w, b, precision, relu, ra1, fixed_tile=1)
            alone0 = engine.conv1d_nlc(xd[row:row + 1].contiguous(), w, b, precision, relu, ra1, fixed_tile=0)
            assert torch.equal(alone1, y1[row:row + 1]), (precision, n, relu, row, "batch row != row alone (fixed_tile 1)")
            assert torch.equal(alone0, y2[row:row + 1]), (precision, n, relu, row, "fixed_tile 2 != B = 1 call")
        assert torch.equal(y0, y1), (precision, n, relu, "64- and 256-position tiles differ")
    print(f"tile256 fixed {precision} n = {n}: worst max-abs {worst:.3g} (bound {TOLS[precision]:.1g})")
    assert worst < TOLS[precision]


@pytest.mark.parametrize("precision", ["f16x2", "bf16x2", "bf16"])
def test_tile256_automatic_rule(cuda, precision):
    """The automatic rule of `launch_conv1d_b16_ns`: (128, 128), n = 2 309, B = 20 makes ceil(2309 / 256) x 20 = 200 tiles, the threshold, so
    f16x2, bf16x2 and bf16 all take the 256-position tile (what the screen's `orca_encoder_back5_batch` and the SV batches run); 200 tiles
    are fewer than the resident workgroups, one tile per workgroup.  Every position of every row within the bound, with and without
    ReLU + r1; row b is bit-equal to that row run alone with fixed_tile = 1 (f16x2: the 256-position tile again; bf16x2 / bf16: a B = 1
    call has 10 < 200 tiles and takes the 64-position tile, so for them this IS the comparison of the two tile shapes); and B = 20 under
    fixed_tile = 2 (64-position tiles) is bit-equal to the automatic call.
    Observed on the MI355X (worst max-abs over both tests): f16x2 5.2e-6, bf16x2 2.4e-5, bf16 1.2e-2; the two tile shapes were bit-equal in
    every comparison."""
    n, B = 2309, 20
    x, w, b, r1, _, conv = _case(128, 128, n, B)
    xd, rd = _nlc(x, cuda), _nlc(r1, cuda)
    worst = 0.0
    for relu, ra, rad in [(False, None, None), (True, r1, rd)]:
        y = engine.conv1d_nlc(xd, w, b, precision, relu, rad)
        worst = max(worst, _err(y, _ref(conv, relu, ra)))
        for row in (0, 7, 19):
            alone = engine.conv1d_nlc(xd[row:row + 1].contiguous(), w, b, precision, relu, None if rad is None else rad[row:row + 1].contiguous(),
                                      fixed_tile=1)
            assert torch.equal(alone, y[row:row + 1]), (precision, relu, row)
        assert torch.equal(engine.conv1d_nlc(xd, w, b, precision, relu, rad, fixed_tile=2), y), (precision, relu, "64- and 256-position tiles differ")
    print(f"tile256 automatic {precision}: worst max-abs {worst:.3g} (bound {TOLS[precision]:.1g})")
    assert worst < TOLS[precision]


# ---- second residual, also in place ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("n", [1, 33, 2048, 2049, 2309])
@pytest.mark.parametrize("cout", [64, 96, 128])
def test_second_residual_and_in_place(cuda, cout, n, precision):
    """r2, the U-net encoders' skip connection, and r2 aliasing y (`encs[lev]` is read and overwritten in one launch of unet_forward_nlc):
    relu(conv) + r1 + r2 at every position, (cout, cout) channels, B = 2.  n = 1, 33, 2 048: conv1d_k9_small_kernel (n <= 2048, no pool4;
    its `a.r2` add); n = 2 049, 2 309: conv1d_k9_bf16s_kernel (its `rb2` add; fixed_tile 0 and 9 x 2, 10 x 2 < 200 tiles: 64-position tiles
    for 128 couts below bf16x3, 256-position ones otherwise).  The in-place call (r2 copied into the output buffer, that buffer passed as y
    and r2) is bit-equal to the out-of-place one, whose r2 tensor is unchanged afterwards.
    Observed on the MI355X, worst max-abs: f16x2 4.6e-6, bf16x3 5.2e-6, bf16x2 2.3e-5, bf16 1.2e-2."""
    x, w, b, r1, r2, conv = _case(cout, cout, n, 2)
    xd, r1d, r2d = _nlc(x, cuda), _nlc(r1, cuda), _nlc(r2, cuda)
    keep = r2d.clone()
    y = engine.conv1d_nlc(xd, w, b, precision, True, r1d, r2=r2d)
    assert tuple(y.shape) == (2, n, cout) and torch.equal(r2d, keep)
    err = _err(y, _ref(conv, True, r1, r2))
    print(f"r2 {precision} cout {cout} n = {n}: max-abs {err:.3g} (bound {TOLS[precision]:.1g})")
    assert err < TOLS[precision]
    # a dropped r2 is an error of |r2| ~ 1, a dropped r1 likewise: both far above every bound (also the bf16 one)
    assert _err(y, _ref(conv, True, r1)) > 1.0 and _err(y, _ref(conv, True, r2)) > 1.0
    z = engine.conv1d_nlc(xd, w, b, precision, True, r1d, r2=r2d, inplace=True)
    assert torch.equal(z, y) and torch.equal(r2d, keep)
    # r2 alone, no ReLU
    y3 = engine.conv1d_nlc(xd, w, b, precision, False, None, r2=r2d)
    assert _err(y3, _ref(conv, False, r2)) < TOLS[precision]


# ---- fused MaxPool1d(4) ----------------------------------------------------------------------------------------------------------------------
def _pool4_direct(cuda, xd, w, b, precision, relu, r1d, n, cout):
    """The export on a caller-owned output with one sentinel row behind its B * (n // 4) rows."""
    B, _, cin = xd.shape
    d = engine.make_descs([{"w": w, "b": b, "cout": cout, "cin": cin, "k": 9, "dil": 1}])
    buf = torch.full((B * (n // 4) + 1, cout), -777.0, dtype=torch.float32, device=cuda)
    ctx = engine.get_context(cuda)
    ctx.sync_stream()
    _lib.check(_lib.load().orca_conv1d_nlc_forward_full(ctx.handle, d, _lib.PRECISIONS[precision], ctypes.c_void_p(xd.data_ptr()),
                                                        ctypes.c_void_p(buf.data_ptr()), ctypes.c_void_p(r1d.data_ptr()) if r1d is not None else None,
                                                        None, B, n, 1 if relu else 0, 1, 0), "orca_conv1d_nlc_forward_full")
    return buf


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("n", [3, 7, 256, 1030, 2051])
@pytest.mark.parametrize("cin,cout", [(64, 64), (64, 96), (96, 128), (128, 128)])
def test_fused_maxpool4(cuda, cin, cout, n, precision):
    """pool4, the fused MaxPool1d(4) epilogue of conv1d_k9_bf16s_kernel (quad shuffles `__shfl_xor` 1, 2; `r_bs` the UN-pooled batch stride of
    r1 while y is pooled; the ragged last window dropped by `pos + 3 < n`).  pool4 keeps every n on conv_bf16s.h (the short-row kernel is
    taken only if !pool4); n = 3, 7, 256, 1 030, 2 051 are n mod 4 = 3, 3, 0, 2, 3 and 0, 1, 64, 257, 512 pooled rows - one tile to nine of 256
    (64 for 128 couts below bf16x3: fixed_tile 0 and at most 9 x 2 < 200 tiles).  B = 2, with and without ReLU + r1, against `max_pool1d(., 4, 4)`
    of the fp64 result.  The output has exactly n // 4 rows per batch entry (n = 3: none, and no launch), and on a caller-owned buffer the
    sentinel row behind the last one is untouched.
    Observed on the MI355X, worst max-abs: f16x2 4.4e-6, bf16x3 6.1e-6, bf16x2 2.4e-5, bf16 1.2e-2."""
    x, w, b, r1, _, conv = _case(cin, cout, n, 2)
    xd, r1d = _nlc(x, cuda), _nlc(r1, cuda)
    ctx = engine.get_context(cuda)
    worst = 0.0
    for relu, ra, rad in [(False, None, None), (True, r1, r1d)]:
        before = ctx.launch_counts()
        y = engine.conv1d_nlc(xd, w, b, precision, relu, rad, pool4=True)
        assert tuple(y.shape) == (2, n // 4, cout)
        launched = ctx.launch_counts()
        assert launched["conv_small"] == before["conv_small"] and launched["conv_bf16s"] == before["conv_bf16s"] + (1 if n >= 4 else 0)
        buf = _pool4_direct(cuda, xd, w, b, precision, relu, rad, n, cout)
        assert float(buf[-1].min()) == float(buf[-1].max()) == -777.0, "the row behind the output was written"
        if n < 4:
            continue
        ref = F.max_pool1d(_ref(conv, relu, ra), 4, 4)
        assert ref.shape[2] == n // 4
        worst = max(worst, _err(y, ref))
        assert torch.equal(buf[:-1].view(2, n // 4, cout), y)
    print(f"pool4 {precision} ({cin}, {cout}) n = {n}: worst max-abs {worst:.3g} (bound {TOLS[precision]:.1g})")
    assert worst < TOLS[precision]


# ---- persistent walk ---------------------------------------------------------------------------------------------------------------------------
def _window_ref(x_nlc, w, b, lo, hi):
    """fp64 conv + bias on positions [lo, hi) of a channel-last device row batch [B, n, cin]: the reach is 4 positions, so the slice with
    its halo (zeros beyond the row's ends) is exact.  -> [B, hi - lo, cout]"""
    n = x_nlc.shape[1]
    a, z = max(lo - 4, 0), min(hi + 4, n)
    xs = x_nlc[:, a:z].cpu().double().transpose(1, 2)
    xs = F.pad(xs, (4 - (lo - a), 4 - (z - hi)))
    return F.conv1d(xs, torch.from_numpy(w).double(), torch.from_numpy(b).double()).transpose(1, 2)


@pytest.mark.parametrize("cin,cout,precision", [(128, 128, "f16x2"), (64, 64, "bf16x3")])
def test_persistent_walk(cuda, cin, cout, precision):
    """The persistent walk of conv1d_k9_bf16s_kernel (`tile += gridDim.x`, with the prefetch of the next tile's chunk 0 under the current
    tile's last chunk - also across a batch seam): n = 150 016 = 586 x 256, B = 2 is 1 172 tiles of 256 positions ((128, 128) f16x2: 1 172 >= 200
    takes launch_b16_t<128, 2, 2, 4, 2, 2, 1>; (64, 64) bf16x3: launch_b16_t<64, 2, 2, 4, 1, 3, 0>), more than the grid of
    `resident_workgroups` (CUs x 1 or 2 workgroups of 80 - 91 KB LDS), so every workgroup walks several tiles and some walk from row 0 into row 1.
    No ReLU, r1 added.  fp64 on windows (a slice with a 4-position halo is exact): the first and the last 300 positions of each row and
    +-150 around positions 65 536 and 131 072; ALL positions against the exact-fp32 kernel (`engine.conv1d`, test_conv1d_k9) at 2e-5.
    Observed on the MI355X: windows against fp64 4.2e-6 (f16x2), 4.4e-6 (bf16x3); all positions against the fp32 kernel 1.1e-5, 8.6e-6."""
    n, B = 150016, 2
    gen = torch.Generator(device=cuda)
    gen.manual_seed(cin + cout)
    x = torch.randn((B, n, cin), device=cuda, generator=gen)
    r1 = torch.randn((B, n, cout), device=cuda, generator=gen)
    rs = np.random.RandomState(cin + cout + n)
    w = (rs.randn(cout, cin, 9) / np.sqrt(cin * 9)).astype(np.float32)
    b = rs.randn(cout).astype(np.float32) * 0.1
    y = engine.conv1d_nlc(x, w, b, precision, False, r1)
    assert tuple(y.shape) == (B, n, cout)
    worst = 0.0
    for lo, hi in [(0, 300), (n - 300, n), (65536 - 150, 65536 + 150), (131072 - 150, 131072 + 150)]:
        ref = _window_ref(x, w, b, lo, hi) + r1[:, lo:hi].cpu().double()
        worst = max(worst, float((y[:, lo:hi].cpu().double() - ref).abs().max()))
    exact = engine.conv1d(x.transpose(1, 2).contiguous(), w, b, False, r1.transpose(1, 2).contiguous())
    diff = float((exact.transpose(1, 2) - y).abs().max())
    print(f"persistent walk {precision} ({cin}, {cout}): windows against fp64 {worst:.3g}, all positions against the fp32 kernel {diff:.3g} (bound 2e-5)")
    assert worst < TOLS[precision] and diff < 2e-5
