"""fp64 references for the Decoders stage by stage (oracle `decoder_stages` and its pieces, as numpy), the residual block of dilation
16 / 32 / 64 on its own, what the exact-fp32 nets' maps add (the 136-channel stage 0, the 72-channel A, the torch-fp32 yardstick, an exactly
summable conv case), and the inputs the GPU tests share.  The counterpart of tests/encoder_ref.py."""
import functools

import numpy as np
import torch
import torch.nn.functional as F

from oracle import orca_oracle as O
from orca_amd import synth
from tests.encoder_ref import rel_err  # noqa: F401  (max |got - ref| / max(1, max |ref|), shared with the Encoder's tests)
from tests.util import synth_sd

F64 = torch.float64
SEEDS = (0, 2)                                       # synth_sd seeds the GPU tests run on
# rel_err bound of ONE residual block of the production chain in f16x2 against fp64 on the same input (test_gpu_decoder_stages.py): 4 x the
# worst observed on the MI355X over every block of both Decoders, 1.26e-6, rounded up to one digit.  test_decoder_stages_cpu.py proves a
# dropped weight plane exceeds it threefold.
BLOCK_BOUND = 6e-6
DIL = {"Decoder": O.DECODER_DILATIONS, "Decoder_1m": O.DECODER1M_DILATIONS}


def decoder_sd(kind, seed=0, num_2d=1):
    kw = {"upsample_mode": "bilinear"} if kind == "Decoder" else {}
    return synth_sd(kind, seed, num_2d=num_2d, **kw)


# ---- inputs -------------------------------------------------------------------------------------------------------------------------------
def inputs(n, B, T=1, seed=31):
    """As test_decoders_vs_golden builds them, every batch row different: x [B,128,n] uniform in [0, 0.5), distenc [B,T,n,n] a log
    distance-decay background (one curve per row and target), y [B,T,n/2,n/2] normal.  float32 CPU tensors."""
    rs = np.random.RandomState(seed + 1000 * n + B)
    x = (rs.rand(B, 128, n) * 0.5).astype(np.float32)
    idx = np.abs(np.arange(n)[None, :] - np.arange(n)[:, None]) * 8
    de = np.stack([np.stack([synth.synth_expected_log(8000, seed=T * b + t)[idx] for t in range(T)]) for b in range(B)]).astype(np.float32)
    y = rs.randn(B, T, max(n // 2, 1), max(n // 2, 1)).astype(np.float32)
    return torch.from_numpy(x), torch.from_numpy(de), torch.from_numpy(y)


def m16_exact(v, precision="f16x2"):
    """float32 values as the M16 storage keeps them: hi + lo of two fp16 planes (f16x2; exact in fp32), one fp16 / bf16 plane."""
    v = torch.as_tensor(v, dtype=torch.float32)
    if precision == "bf16":
        return v.to(torch.bfloat16).float()
    hi = v.half().float()
    return hi if precision == "f16" else hi + (v - hi).half().float()


# ---- stages (fp64, numpy out) -------------------------------------------------------------------------------------------------------------
def _np(t):
    return t.numpy()


def head(x, distenc, y=None, upsample_mode="bilinear"):
    """(stage 0 [B,16,n,n], channels 64..79 of stage 2 [B,16,n,n] or None) of a Decoder."""
    de = O._t(distenc, F64)
    in0 = O._pad_channels(de.expand(x.shape[0], -1, -1, -1), O.DECODER_IN_CHANNELS)
    up = None if y is None else O._pad_channels(F.interpolate(O._t(y, F64), scale_factor=(2, 2), mode=upsample_mode), 16)
    return _np(in0), None if up is None else _np(up)


def outer_sum(x):
    x = O._t(x, F64)
    return _np(x[:, :, :, None] + x[:, :, None, :])


def first(sd, x, in0):
    return _np(O.decoder_first(sd, x, in0, F64))


def mat(sd, s1, dtype=F64):
    """Channels 0..63 of stage 2 from stage 1."""
    return _np(O.decoder_mat(sd, s1, None, dtype))


def block(sd, kind, i, cur, dtype=F64):
    return _np(O.decoder_block(sd, kind, i, cur, dtype))


def final(sd, cur, dtype=F64):
    return _np(O.final_sym(sd, cur, dtype))


def stages(sd, kind, x, distenc=None, y=None, upsample_mode="bilinear", dtype=F64):
    st = O.decoder_1m_stages(sd, x, dtype) if kind == "Decoder_1m" else O.decoder_stages(sd, x, distenc, y, upsample_mode, dtype)
    return {k: _np(v) for k, v in st.items()}


# ---- the exact-fp32 nets (tests/test_gpu_decoder_f32_stages.py) ------------------------------------------------------------------------------
# Their probe hands out what the fp32 planes hold: stage 0 of a Decoder is the WHOLE 136-channel input map (x_i + x_j in 0..127, distenc in
# 128..128+T-1, zeros), A with y has 72 channels (64 + the 8 planes of the up-sampled coarse prediction).
F32_IN_CHANNELS, F32_A_CHANNELS = 136, 72
# A convolution stage's bound is YARD_FACTOR x its YARDSTICK: the rel_err of the same stage on the same input in torch fp32 on the CPU against
# the fp64 reference.  5.5 (a plain sequential K-term fp32 chain - what the kernel's fmaf chain is - has 1.2 .. 5.5 x the error of torch's
# blocked sum: 1.47e-6 against 2.67e-7 at cin 136, d 1) x 3 (order, fmaf, the extreme-value spread between shapes).
# test_decoder_stages_cpu.py proves that such a chain stays within it and that fp16-rounded operands do not.
YARD_FACTOR = 16


def head_f32(x, distenc, y=None, upsample_mode="bilinear"):
    """(stage 0 [B,136,n,n], channels 64..71 of stage 2 [B,8,n,n] or None) of an exact-fp32 Decoder."""
    in0, up = head(x, distenc, y, upsample_mode)
    return np.concatenate([outer_sum(x), in0[:, : F32_IN_CHANNELS - 128]], axis=1), None if up is None else up[:, : F32_A_CHANNELS - 64]


def first_map(sd, in_map, dtype=F64):
    """Stage 1 from the 136-channel stage 0 of an exact-fp32 Decoder: lcombinerD's conv 0 + BN on its first 128 + T channels."""
    sd = O._as_sd(sd, dtype)
    T = sd["lcombinerD.0.weight"].shape[1] - 128
    with torch.no_grad():
        return _np(O._bn(sd, "lcombinerD.1", O._conv(sd, "lcombinerD.0", O._t(in_map, dtype)[:, : 128 + T])))


def yardstick(stage, *args):
    """(fp64 reference, YARDSTICK) of a convolution stage: ``stage(*args, dtype)`` is one of `first_map`, `mat`, `block`, `final`."""
    ref = stage(*args, F64)
    return ref, rel_err(stage(*args, torch.float32), ref)


def exact_conv_case(cin, cout, n, B, seed=0):
    """One 3x3 conv that fp32 computes EXACTLY in any order: x integers in [-8, 8], w = k / 8 with integer |k| <= 8, bias k / 8, residual
    integers - every partial sum is a multiple of 1/8 below 2^17 such units (9 * 136 * 64 + 8 + 64 = 78 408).  (x, w, b, r), float32."""
    rs = np.random.RandomState(1000 * cin + 10 * n + B + seed)
    x = rs.randint(-8, 9, (B, cin, n, n)).astype(np.float32)
    w = (rs.randint(-8, 9, (cout, cin, 3, 3)) / 8.0).astype(np.float32)
    b = (rs.randint(-8, 9, cout) / 8.0).astype(np.float32)
    r = rs.randint(-8, 9, (B, cout, n, n)).astype(np.float32)
    return torch.from_numpy(x), w, b, torch.from_numpy(r)


def conv_ref(x, w, b, d, relu=False, r=None, dtype=F64):
    """act(conv3x3(x; w, b), dilation = padding = d) + r in ``dtype``."""
    with torch.no_grad():
        out = F.conv2d(O._t(x, dtype), O._t(w, dtype), O._t(b, dtype), padding=d, dilation=d)
        out = F.relu(out) if relu else out
        return _np(out if r is None else out + O._t(r, dtype))


# ---- one residual block of dilation 16 / 32 / 64 on its own ---------------------------------------------------------------------------------
BLOCK_SHAPES = ((32, 64), (64, 32), (32, 64), (64, 32))      # (cout, cin) of lm.a, lm.b, m.a, m.b


def dense_block(seed):
    """Dense normal weights scaled 1 / sqrt(9 cin), biases normal x 0.1: [(w [cout,cin,3,3], b [cout])] * 4, float32."""
    rs = np.random.RandomState(seed)
    return [((rs.randn(co, ci, 3, 3) / np.sqrt(9.0 * ci)).astype(np.float32), (0.1 * rs.randn(co)).astype(np.float32)) for co, ci in BLOCK_SHAPES]


def block_ref(convs, d, x, drop=None):
    """fp64: o = lm.b(lm.a(x)) + x; relu(m.b(relu(m.a(o)))) + o, zero padding d, weights as given.  ``drop`` = (conv, mutation) replaces that
    conv's weights: "lo" - by their fp16 rounding (what a dropped lo weight plane computes)."""
    x = O._t(x, F64)
    W = []
    for k, (w, b) in enumerate(convs):
        w = torch.from_numpy(np.asarray(w, dtype=np.float64))
        if drop is not None and drop[0] == k:
            assert drop[1] == "lo"
            w = w.half().double()
        W.append((w, torch.from_numpy(np.asarray(b, dtype=np.float64))))

    def conv(k, t):
        return F.conv2d(t, W[k][0], W[k][1], padding=d, dilation=d)

    with torch.no_grad():
        o = conv(1, conv(0, x)) + x
        return _np(F.relu(conv(3, F.relu(conv(2, o)))) + o)


def exact_block():
    """Sparse weights in {0, +-1, +-0.5} - every output channel of every conv reads one or two input channels, each through ONE tap that is
    never the centre and differs from conv to conv and channel to channel - and integer biases in -1..2: with `exact_input` every
    intermediate is a small multiple of 1/16, exactly representable in bf16, fp16 and fp16 pairs (test_decoder_stages_cpu.py checks it)."""
    vals = (1.0, -1.0, 0.5, -0.5)
    taps = (0, 1, 2, 3, 5, 6, 7, 8)                      # all but the centre
    convs = []
    for k, (co, ci) in enumerate(BLOCK_SHAPES):
        w = np.zeros((co, ci, 9), np.float32)
        for o in range(co):
            w[o, (5 * o + 3 * k) % ci, taps[(o + 3 * k) % 8]] = vals[(o + k) % 4]
            if o % 3 == k % 3:
                w[o, (7 * o + k + 1) % ci, taps[(o + 3 * k + 5) % 8]] = vals[(o + k + 1) % 2]       # a second term, +-1
        b = ((np.arange(co) + k) % 4 - 1).astype(np.float32)
        convs.append((w.reshape(co, ci, 3, 3), b))
    return convs


def exact_input(n, B, d):
    """Integer impulses 1..3 on a zero map [B,64,n,n]: the four corners, row and column n - 1, the last pixel of a sub-image (rows and
    columns congruent mod d) next to the first of the following one, and both sides of row / column d."""
    x = np.zeros((B, 64, n, n), np.float32)
    last = (n - 1) // d * d                                # last row / column of the sub-images that start at 0
    pts = [(0, 0), (0, n - 1), (n - 1, 0), (n - 1, n - 1), (n - 1, n // 2), (n // 3, n - 1), (last, last), (0, 1), (last, min(last + 1, n - 1)),
           (min(d - 1, n - 1), min(d - 1, n - 1)), (min(d, n - 1), min(d, n - 1)), (n // 2, n // 2)]
    for b in range(B):
        for q, (i, j) in enumerate(pts):
            x[b, (11 * q + 29 * b) % 64, i, j] += 1 + (q + b) % 3
            x[b, (11 * q + 29 * b + 32) % 64, j, i] -= 1 + (q + 2 * b) % 2
    return torch.from_numpy(x)


@functools.lru_cache(maxsize=6)
def exact_ref(n, B, d):
    return block_ref(exact_block(), d, exact_input(n, B, d))
