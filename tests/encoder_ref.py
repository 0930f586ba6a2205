"""fp64 references for the Encoder in two parts (sv.Stage3Cache / sv.Stage4Cache and the C exports behind them): the oracle's stages on
packed bases, MaxPool1d(5), and the P16 plane layout of conv_p16.h / p16_planes.h decoded and encoded on the host."""
import numpy as np
import torch

from oracle import orca_oracle as O
from orca_amd import synth
from tests.util import shapes_of

# (seed, conv gain) of the synthetic Encoder weights the tests run on
WEIGHTS = [(0, 1.0), (1, 1.0), (0, 1.6)]


def encoder_sd(seed=0, gain=1.0):
    return synth.synth_state_dict(shapes_of("Encoder"), seed=seed, relu_gain=gain)


def revcomp(codes):
    """Reverse complement of uint8 codes (0..3 = ACGT, 4 = N)."""
    c = np.asarray(codes)[::-1]
    return np.where(c < 4, 3 - c, c).astype(np.uint8)


def strand_codes(codes, reverse):
    return revcomp(codes) if reverse else np.asarray(codes, dtype=np.uint8)


def onehot(codes, dtype=torch.float64):
    """[B, L] (or [L]) codes -> [B, 4, L] one-hot, N = 0.25 x 4 (selene_utils2.py:216-222, :272)."""
    c = np.atleast_2d(np.asarray(codes, dtype=np.int64))
    x = np.zeros((c.shape[0], 4, c.shape[1]), dtype=np.float64)
    for k in range(4):
        x[:, k, :] = (c == k)
    x[np.broadcast_to((c == 4)[:, None, :], x.shape)] = 0.25
    return torch.from_numpy(x).to(dtype)


def stages(sd, codes, upto, first=1):
    """fp64 stage outputs of the Encoder run on ``codes`` alone (zero padded at its own ends): {k: [n_k, C_k] (or [B, n_k, C_k]) numpy},
    stage k after its residual (stage 7 without), k = first..upto.  ``first`` > 1: ``codes`` is instead what stage ``first`` reads, [n, 128]
    values (the pooled output of stage ``first`` - 1)."""
    if first == 1:
        batched = np.asarray(codes).ndim == 2
        x = onehot(codes)
    else:
        batched = False
        x = torch.from_numpy(np.asarray(codes, dtype=np.float64).T[None].copy())
    outs = O.encoder_stages(sd, x, upto=upto, dtype=torch.float64, first=first)
    res = {}
    for k, o in enumerate(outs, start=first):
        v = o.numpy().transpose(0, 2, 1)
        res[k] = v if batched else v[0]
    return res


def pool5(v):
    """MaxPool1d(5) along axis 0 of [n, C] (a tail of fewer than 5 rows is dropped)."""
    n = v.shape[0] // 5
    return v[: 5 * n].reshape(n, 5, *v.shape[1:]).max(1)


# ---- a synthetic chromosome and windows on it for the stage-cache route (sv.s3_plan) -----------------------------------------------------
C = 64_000


def chromosome():
    rs = np.random.RandomState(77)
    codes = rs.randint(0, 4, C).astype(np.uint8)
    codes[23_500: 24_700] = 4                                            # N runs (one inside the inverted piece below)
    codes[51_000: 51_300] = 4
    return codes


# (pieces, region): windows of 4 - 48 kb (multiples of 400) from off-grid pieces
WINDOWS = [
    ([(5_003, 10_000, "+"), (21_117, 14_000, "+")], None),                           # a deletion
    ([(20_001, 12_000, "+"), (28_001, 12_000, "+")], None),                          # a duplication (bases 28 001 - 32 001 twice)
    ([(8_007, 10_000, "+"), (18_007, 9_000, "-"), (27_007, 9_000, "+")], None),       # an inversion (with an N run)
    ([(C - 15_000, 15_000, "+"), (3_000, 9_000, "-")], None),                        # a piece that ends at the chromosome's end
    ([(0, 8_800, "+"), (40_011, 3_200, "+")], None),                                 # ... and one that starts at its start
    ([(33_333, 4_000, "+")], None),                                                  # a few kb
    ([(2_011, 48_000, "+")], None),                                                  # 48 kb
    ([(6_003, 40_000, "+")], (10_000, 40_000)),                                      # partly outside the cached region
    ([(4_005, 14_000, "+"), (30_021, 10_000, "-")], (12_000, 45_000)),               # ... and an inversion across its edge
]


# ---- P16 planes: [32, units, 4] float32 = 16 octets of channels x 2 splits (hi, lo); plane 2 o + s; a 16-byte unit holds the fp16 values of
# channels 8 o .. 8 o + 7 of ONE position; position j at unit 8 + j (P16_GUARD = 8 zero units on the left) ----
P16_GUARD = 8


def unpack_p16(planes, n):
    """Planes (torch or numpy [32, units, 4] float32) -> values [n, 128] float64 (hi + lo of positions 0..n-1)."""
    a = planes.detach().cpu().numpy() if isinstance(planes, torch.Tensor) else np.asarray(planes)
    h = np.ascontiguousarray(a).view(np.float16).reshape(16, 2, a.shape[1], 8).astype(np.float64)
    v = h[:, 0] + h[:, 1]                                     # [16 octets, units, 8]
    return v[:, P16_GUARD: P16_GUARD + n, :].transpose(1, 0, 2).reshape(n, 128)


def pack_p16(values, units, fill=0.0):
    """values [n, 128] -> planes [32, units, 4] float32 (numpy): hi = fp16(v), lo = fp16(v - hi); every other unit = ``fill`` (float32 bits)."""
    v = np.asarray(values, dtype=np.float32)
    n = v.shape[0]
    out = np.full((32, units, 4), fill, dtype=np.float32)
    h = out.view(np.float16).reshape(16, 2, units, 8)
    hi = v.astype(np.float16)
    lo = (v - hi.astype(np.float32)).astype(np.float16)
    for s, part in enumerate((hi, lo)):
        h[:, s, P16_GUARD: P16_GUARD + n, :] = part.reshape(n, 16, 8).transpose(1, 0, 2)
    return out


def rel_err(got, ref):
    """max |got - ref| / max(1, max |ref|)."""
    ref = np.asarray(ref, dtype=np.float64)
    return float(np.abs(np.asarray(got, dtype=np.float64) - ref).max() / max(1.0, float(np.abs(ref).max())))
