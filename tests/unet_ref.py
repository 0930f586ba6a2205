"""References for the U-net encoders (Encoder2 / Encoder3 / Encoder2b, `orca_unet_forward`): synthetic state dicts, inputs in the three layouts
the C entry stages, and the oracle's walk (oracle/orca_oracle.py `encoder_unet_forward`, `encoder2b_forward`) in fp32 and fp64, computed once per
(network, weights, n) on a batch of `BMAX` rows and shared by the tests - a row of a conv network does not depend on the other rows, so the
B = 1 case of a test is row 0 of the same walk."""
import functools

import numpy as np
import torch

from oracle import orca_oracle as O
from tests.encoder_ref import rel_err  # noqa: F401  (max |got - ref| / max(1, max |ref|): what the stage tests bound)
from tests.util import synth_sd

NLEV = {"Encoder2": 5, "Encoder3": 3, "Encoder2b": 5}
SEEDS = (0, 1)
BMAX = 3
LAYOUTS = ("contiguous", "strided", "slice")


@functools.lru_cache(maxsize=None)
def unet_sd(kind, seed):
    """State dict of ``kind``; "Encoder2b<-Encoder2": the contracting half of the Encoder2 dict of that seed (`encoder2b_of`)."""
    if kind == "Encoder2b<-Encoder2":
        return encoder2b_of(unet_sd("Encoder2", seed))
    return synth_sd(kind, seed)


def encoder2b_of(sd2):
    """An Encoder2b state dict cut out of an Encoder2 one: the two share the key names ``lblocks.i`` / ``blocks.i`` of the contracting path."""
    return {k: v for k, v in sd2.items() if k.startswith(("lblocks.", "blocks."))}


def module_kind(kind):
    return "Encoder2b" if kind.startswith("Encoder2b") else kind


def level_sizes(kind, n):
    """Positions of the nlev + 1 encodings of an n-position input, fine to coarse."""
    return [n >> i for i in range(NLEV[module_kind(kind)] + 1)]


@functools.lru_cache(maxsize=None)
def values(n, seed=0):
    """The input values [BMAX, 128, n] float32 (uniform in [0, 0.5), as the sibling tests of test_gpu_nets.py)."""
    return torch.from_numpy((np.random.RandomState(1000 * seed + n).rand(BMAX, 128, n) * 0.5).astype(np.float32))


def device_input(x, layout, device):
    """``x`` [B, 128, n] on ``device`` as (the tensor that owns the memory, the view of it that holds x): contiguous, every second position of a
    [B, 128, 2 n] tensor, or rows 1..B and positions 17..17 + n of a [B + 2, 128, n + 40] tensor (an odd offset: no 16-byte alignment).  What
    surrounds x is a sentinel."""
    B, C, n = x.shape
    if layout == "contiguous":
        owner = x.clone().to(device)
        return owner, owner
    if layout == "strided":
        owner = torch.full((B, C, 2 * n), 7.5, dtype=torch.float32)
        owner[:, :, ::2] = x
        owner = owner.to(device)
        return owner, owner[:, :, ::2]
    if layout == "slice":
        owner = torch.full((B + 2, C, n + 40), 7.5, dtype=torch.float32)
        owner[1: B + 1, :, 17: 17 + n] = x
        owner = owner.to(device)
        return owner, owner[1: B + 1, :, 17: 17 + n]
    raise ValueError(layout)


def walk(kind, sd, x, dtype=torch.float64):
    """The oracle's encodings of ``x`` as numpy arrays, fine to coarse, weights and arithmetic in ``dtype``."""
    k = module_kind(kind)
    outs = O.encoder2b_forward(sd, x, dtype=dtype) if k == "Encoder2b" else O.encoder_unet_forward(sd, x, NLEV[k], dtype=dtype)
    return [o.numpy() for o in outs]


@functools.lru_cache(maxsize=None)
def walks(kind, seed, n, xseed=0):
    """(fp32 walk, fp64 walk) of `values(n, xseed)` through the seed-``seed`` weights of ``kind``, BMAX rows."""
    sd, x = unet_sd(kind, seed), values(n, xseed)
    return walk(kind, sd, x, torch.float32), walk(kind, sd, x, torch.float64)


def e32(kind, seed, n, B, xseed=0):
    """E32 of a case: max over the levels of rel_err(fp32 walk, fp64 walk) on rows 0..B-1 - the reference's own fp32 rounding, which the
    bounds of the GPU tests are multiples of."""
    w32, w64 = walks(kind, seed, n, xseed)
    return max(rel_err(a[:B], b[:B]) for a, b in zip(w32, w64))
