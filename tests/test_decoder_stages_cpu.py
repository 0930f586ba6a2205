"""CPU: the oracle's Decoder stages (oracle/orca_oracle.py `decoder_stages`, `decoder_1m_stages`, `decoder_block`) that
tests/test_gpu_decoder_stages.py holds the HIP kernels to - they compose to the forward the golden fixtures pin, fp32 and fp64 agree, the exact
case of the block kernel is exact in every storage format, and a per-stage comparison sees a defect that the end-to-end tolerance hides.
For the exact-fp32 nets (tests/test_gpu_decoder_f32_stages.py): the yardstick bound holds a sequential fp32 chain and fails fp16-rounded
operands, the 136- / 72-channel stage references are the pieces above, and the integer conv case is exact in fp32."""
import functools

import numpy as np
import pytest
import torch

from oracle import orca_oracle as O
from tests import decoder_ref as R
from tests.decoder_ref import rel_err

N = 30


def _inputs(B=2):
    return R.inputs(N, B)


@pytest.mark.parametrize("with_y,mode", [(False, "bilinear"), (True, "bilinear"), (True, "nearest")])
def test_decoder_blocks_compose_to_the_forward(with_y, mode):
    """first -> mat -> decoder_block 0..27 -> final_sym, each on the previous one's output, is `decoder_forward` (what
    test_oracle_golden.py pins against the reference's own modules); the stage mapping has the shapes the probe hands out."""
    sd = R.decoder_sd("Decoder", 0)
    x, de, y = _inputs()
    y = y if with_y else None
    ref = O.decoder_forward(sd, x, de, y, mode)
    st = O.decoder_stages(sd, x, de, y, mode)
    assert list(st) == list(range(31)) + ["out"]
    assert st[0].shape == (2, 16, N, N) and st[1].shape == (2, 64, N, N) and st[2].shape == (2, 80 if with_y else 64, N, N)
    assert torch.equal(st[0][:, :1], de) and not st[0][:, 1:].any()
    in0, up = R.head(x, de, y, mode)
    cur = O.decoder_first(sd, x, torch.from_numpy(in0).float())
    assert torch.equal(cur, st[1])
    cur = O.decoder_mat(sd, cur, None if up is None else torch.from_numpy(up[:, :1]).float())
    assert rel_err(cur.numpy(), st[2].numpy()) < 1e-6          # (`up` was interpolated in fp64)
    if with_y:
        assert not cur[:, 65:].any() and rel_err(cur[:, 64].numpy(), up[:, 0]) < 1e-6
    for i in range(28):
        cur = O.decoder_block(sd, "Decoder", i, cur)
        assert cur.shape == (2, 64, N, N)
        assert rel_err(cur.numpy(), st[3 + i].numpy()) < 1e-6, i
    assert rel_err(O.final_sym(sd, cur).numpy(), ref.numpy()) < 1e-6
    assert torch.equal(st["out"], ref)


def test_decoder_1m_blocks_compose_to_the_forward():
    sd = R.decoder_sd("Decoder_1m", 2)
    x, _, _ = _inputs()
    ref = O.decoder_1m_forward(sd, x)
    st = O.decoder_1m_stages(sd, x)
    assert list(st) == [0] + list(range(3, 22)) + ["out"]
    cur = st[0]
    assert cur.shape == (2, 128, N, N) and torch.equal(cur[1, 5, 3, 7], x[1, 5, 3] + x[1, 5, 7])
    for i in range(19):
        cur = O.decoder_block(sd, "Decoder_1m", i, cur)
        assert rel_err(cur.numpy(), st[3 + i].numpy()) < 1e-6, i
    assert rel_err(O.final_sym(sd, cur).numpy(), ref.numpy()) < 1e-6


@pytest.mark.parametrize("kind", ["Decoder", "Decoder_1m"])
def test_fp32_stages_agree_with_fp64_stages(kind):
    """Every stage of the fp32 oracle against the fp64 one on the same input, n = 30, B = 2.  A conv's fp32 round-off is ~2^-24 sqrt(K) of
    its output's scale (K = 9 cin <= 1224 products) and the residual stream carries it on unamplified, so the stages' errors add up like a
    random walk, far below the linear 116 x 35 x 2^-24.  Worst observed 6.4e-7 (Decoder), 4.5e-7 (Decoder_1m); bound 4 x that, 3e-6."""
    sd = R.decoder_sd(kind, 2)
    x, de, y = _inputs()
    a = R.stages(sd, kind, x, de, y, dtype=torch.float32)
    b = R.stages(sd, kind, x, de, y)
    worst = max(rel_err(a[k], b[k]) for k in b)
    print(f"{kind}: fp32 against fp64 stages, worst rel_err {worst:.3g}")
    assert list(a) == list(b) and worst <= 3e-6


@pytest.mark.parametrize("n", [250, 30])
@pytest.mark.parametrize("d", [16, 32, 64])
def test_exact_case_is_exact_in_every_storage_format(d, n):
    """What lets test_gpu_decoder_stages.py ask for EQUALITY, at the (d, n) it asks it at: in the exact case the input, the three intermediate
    maps of the block and its output are unchanged by a round trip through bf16 (8 significant bits; fp16 and fp16 pairs keep more), and all
    are multiples of 1/16."""
    import torch.nn.functional as F
    convs, x = R.exact_block(), R.exact_input(n, 2, d).double()
    W = [(torch.from_numpy(w).double(), torch.from_numpy(b).double()) for w, b in convs]
    assert all(set(np.unique(np.abs(w))) <= {0.0, 0.5, 1.0} and np.count_nonzero(w[:, :, 1, 1]) == 0 for w, _ in convs)
    t = F.conv2d(x, *W[0], padding=d, dilation=d)
    o = F.conv2d(t, *W[1], padding=d, dilation=d) + x
    u = F.relu(F.conv2d(o, *W[2], padding=d, dilation=d))
    out = F.relu(F.conv2d(u, *W[3], padding=d, dilation=d)) + o
    for m in (x, t, o, u, out):
        assert torch.equal(m.to(torch.bfloat16).double(), m) and torch.equal((m * 16).round(), m * 16)
    assert np.array_equal(out.numpy(), R.exact_ref(n, 2, d))
    # ... and it is not a trivial map (at n <= d every off-centre tap reads padding: biases, ReLU and the residuals alone give 8 values)
    assert len(np.unique(out.numpy())) >= (8 if n <= d else 9)


@functools.lru_cache(maxsize=1)
def _stages_130():
    """fp64 stages of the seed-0 Decoder at n = 130 (dilation 64 still reaches across the map), one map."""
    x, de, y = R.inputs(130, 1)
    return R.stages(R.decoder_sd("Decoder", 0), "Decoder", x, de, y)


@pytest.mark.parametrize("i", [7, 4, 6])
def test_one_dropped_lo_weight_plane_shows_per_stage_but_not_end_to_end(i):
    """SENSITIVITY.  The f16x2 kernels add three products per tap (hi.lo, lo.hi, hi.hi of the fp16 pairs).  Losing the weights' lo plane in ONE
    conv of ONE block (i = 7: d = 1, i = 4: d = 16, i = 6: d = 64; the conv is m.a, then lm.b) leaves that conv with the fp16 rounding of
    its weights - here in the fp64 reference of that block, on the fp64 stream in front of it.  The block's output then differs from the
    unmodified reference by >= 3 x BLOCK_BOUND (the per-block bound of test_gpu_decoder_stages.py), the mutation of the issue's first choice: it
    holds for the synthetic weights in all six cases (stage rel_err 2.4e-5 .. 7.0e-5).  Printed, not asserted: what the same defect does to the
    network's output, next to the 1e-4 that the end-to-end tests allow (5.1e-5 .. 3.2e-4 max-abs here: under that tolerance in two of the
    six cases and within a factor of 3.2 of it in all)."""
    sd = R.decoder_sd("Decoder", 0)
    st = _stages_130()
    for name in (f"convtwos.{i}.0", f"lconvtwos.{i}.2"):
        bad = dict(sd)
        bad[name + ".weight"] = np.asarray(sd[name + ".weight"]).astype(np.float16).astype(np.float32)
        got = R.block(bad, "Decoder", i, st[2 + i])
        err = rel_err(got, st[3 + i])
        cur = got
        for k in range(i + 1, 28):
            cur = R.block(sd, "Decoder", k, cur)
        end = float(np.abs(R.final(sd, cur) - st["out"]).max())
        print(f"block {i} (d = {O.DECODER_DILATIONS[i]}), {name} without its lo plane: stage rel_err {err:.3g} "
              f"(per-block bound {R.BLOCK_BOUND:.1g}); final output max-abs {end:.3g} (end-to-end tolerance 1e-4)")
        assert err >= 3 * R.BLOCK_BOUND, (name, err)


# ---- the yardstick of tests/test_gpu_decoder_f32_stages.py ------------------------------------------------------------------------------------
def _seq_conv(x, w, b, d, relu=False, r=None):
    """A 3x3 conv as a plain sequential float32 chain, one term at a time (numpy float32: the product and the sum each round): channel-major,
    the nine taps inside, bias last - the order of conv2d_3x3_kernel's chunks.  x [B,cin,n,n], w [cout,cin,3,3] (BN folded), b [cout]."""
    x, w = np.asarray(x, np.float32), np.asarray(w, np.float32)
    n = x.shape[-1]
    xp = np.pad(x, ((0, 0), (0, 0), (d, d), (d, d)))
    acc = np.zeros((x.shape[0], w.shape[0], n, n), np.float32)
    for ci in range(x.shape[1]):
        for ky in range(3):
            for kx in range(3):
                acc += w[None, :, ci, ky, kx, None, None] * xp[:, ci, None, ky * d: ky * d + n, kx * d: kx * d + n]
    acc += np.asarray(b, np.float32)[None, :, None, None]
    if relu:
        acc = np.maximum(acc, np.float32(0))
    return acc if r is None else acc + r


def _folded(sd, pairs):
    from orca_amd import engine
    return [engine.fold_conv(sd, c, bn) for c, bn in pairs]


def _seq_stage(sd, i, x, half=False):
    """The first conv (i = None, x = the 136-channel stage 0) or residual block i >= 1 (x = the stream in front of it) of the seed's Decoder
    as `_seq_conv` chains on the library's BN-folded fp32 weights; ``half``: x and every w rounded to fp16 first."""
    def h(v):
        return np.asarray(v, np.float32).astype(np.float16).astype(np.float32) if half else np.asarray(v, np.float32)
    if i is None:
        (c,) = _folded(sd, [("lcombinerD.0", "lcombinerD.1")])
        return _seq_conv(h(x)[:, : c["cin"]], h(c["w"]), c["b"], 1)
    d = O.DECODER_DILATIONS[i]
    la, lb, ma, mb = _folded(sd, [(f"lconvtwos.{i}.0", f"lconvtwos.{i}.1"), (f"lconvtwos.{i}.2", f"lconvtwos.{i}.3"),
                                  (f"convtwos.{i}.0", f"convtwos.{i}.1"), (f"convtwos.{i}.3", f"convtwos.{i}.4")])
    x = h(x)
    o = _seq_conv(_seq_conv(x, h(la["w"]), la["b"], d), h(lb["w"]), lb["b"], d, r=x)
    return _seq_conv(_seq_conv(o, h(ma["w"]), ma["b"], d, relu=True), h(mb["w"]), mb["b"], d, relu=True, r=o)


@functools.lru_cache(maxsize=1)
def _f32_stage_inputs():
    """fp32 stages of the seed-0 Decoder at n = 30, B = 2, with stage 0 as an exact-fp32 net holds it (136 channels)."""
    sd = R.decoder_sd("Decoder", 0)
    x, de, y = _inputs()
    st = R.stages(sd, "Decoder", x, de, y, dtype=torch.float32)
    st[0] = R.head_f32(x, de, y)[0].astype(np.float32)
    return sd, st


@pytest.mark.parametrize("i", [None, 7, 4, 6])
def test_fp32_yardstick_holds_a_sequential_chain_and_sees_fp16_operands(i):
    """What lets test_gpu_decoder_f32_stages.py hold conv2d_3x3_kernel to YARD_FACTOR x the yardstick (torch fp32 against fp64 on the same
    input, in `rel_err`), at n = 30: the first conv (K = 9 x 136) and one block per dilation 1, 16 and 64 (i = 7, 4, 6) as a plain sequential
    float32 chain - the worst order a correct fp32 kernel can sum in - stay within the bound, and the same stage with x and w rounded to fp16
    (an 11-bit operand path) exceeds it."""
    sd, st = _f32_stage_inputs()
    if i is None:
        ref, yard = R.yardstick(R.first_map, sd, st[0])
        src = st[0]
    else:
        ref, yard = R.yardstick(R.block, sd, "Decoder", i, st[2 + i])
        src = st[2 + i]
    seq, half = rel_err(_seq_stage(sd, i, src), ref), rel_err(_seq_stage(sd, i, src, half=True), ref)
    print(f"stage {'first conv' if i is None else f'block {i}'}: yardstick {yard:.3g}; sequential fp32 chain {seq:.3g} ({seq / yard:.2f} x), "
          f"fp16 operands {half:.3g} ({half / yard:.0f} x); bound {R.YARD_FACTOR} x")
    assert yard > 0 and seq <= R.YARD_FACTOR * yard < half
    assert ref.shape == (2, 64, N, N)


def test_head_f32_is_the_whole_input_map_and_the_72_channel_A():
    """`head_f32`: x_i + x_j in channels 0..127, distenc behind them, zeros to 135; the up-sampled y in 8 planes - the pieces the 16-bit
    file's `head` and `outer_sum` give, and what `first_map` reads is `decoder_first`'s input."""
    sd = R.decoder_sd("Decoder", 0)
    x, de, y = _inputs()
    in0, up = R.head_f32(x, de, y)
    h0, hup = R.head(x, de, y)
    assert in0.shape == (2, 136, N, N) and up.shape == (2, 8, N, N)
    assert np.array_equal(in0[:, :128], R.outer_sum(x)) and np.array_equal(in0[:, 128:], h0[:, :8]) and np.array_equal(up, hup[:, :8])
    assert not in0[:, 129:].any() and not up[:, 1:].any()
    assert np.array_equal(R.first_map(sd, in0), R.first(sd, x, h0))
    assert R.head_f32(x, de, None)[1] is None


@pytest.mark.parametrize("cin,cout,d,n,B", [(136, 64, 1, 30, 1), (65, 64, 1, 17, 2), (64, 32, 16, 2, 2), (32, 64, 8, 1, 1)])
def test_exact_conv_case_is_exact_in_fp32(cin, cout, d, n, B):
    """What lets the GPU test ask conv2d_3x3_kernel for EQUALITY: on `exact_conv_case` data torch fp32 equals fp64 (with and without ReLU and
    residual), every value is a multiple of 1/8 below 2^17 such units, and the result is no trivial map."""
    x, w, b, r = R.exact_conv_case(cin, cout, n, B)
    for relu, res in ((False, None), (True, r)):
        ref = R.conv_ref(x, w, b, d, relu, res)
        assert np.array_equal(R.conv_ref(x, w, b, d, relu, res, torch.float32).astype(np.float64), ref)
        assert np.array_equal(np.round(ref * 8), ref * 8) and np.abs(ref * 8).max() < 2 ** 17
        assert len(np.unique(ref)) > min(16, ref.size // 4)
