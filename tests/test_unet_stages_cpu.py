"""CPU: the oracle's walk of the U-net encoders (oracle/orca_oracle.py `encoder_unet_forward`, `encoder2b_forward` with ``dtype=``) that
tests/test_gpu_unet_stages.py holds `orca_unet_forward` to - in fp32 it is still what the golden fixtures pin, bit for bit; fp64 agrees with it
to fp32 rounding; Encoder2b on Encoder2's contracting weights is Encoder2's contracting path; and the ctypes prototype of the full channel-last
conv entry loads."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import orca_oracle as O
from orca_amd import _lib
from tests import unet_ref as R
from tests.unet_ref import rel_err
from tests.util import golden, maxabs, synth_sd


def _walk_before_dtype(sd, x, nlev, expanding=True):
    """`encoder_unet_forward` / `encoder2b_forward` as they stood before they took ``dtype=`` (fp32 `_SD`, fp32 input), restated."""
    sd = O._SD(sd)
    out = O._t(x)
    with torch.no_grad():
        encs = [out]
        for i in range(nlev):
            lout = O._lin2(sd, f"lblocks.{i}", 1, F.max_pool1d(out, 2, 2))
            out = O._relu2(sd, f"blocks.{i}", lout) + lout
            encs.append(out)
        if not expanding:
            return encs
        encs2 = [out]
        for i, enc in enumerate(reversed(encs[:-1])):
            lout = O._lin2(sd, f"downlblocks.{i}", 1, F.interpolate(out, scale_factor=2, mode="nearest"))
            out = O._relu2(sd, f"downblocks.{i}", lout, second_bn=False) + lout
            out = enc + out
            encs2.append(out)
    return encs2[::-1]


G3_G15_INPUTS = [("Encoder2", 21, 800), ("Encoder2", 22, 8000), ("Encoder3", 23, 2000), ("Encoder2b", 33, 2048)]


@pytest.mark.parametrize("kind,xseed,n", G3_G15_INPUTS)
def test_fp32_walk_is_the_old_oracle_bit_for_bit(kind, xseed, n):
    """On the inputs of the G3 (Encoder2 at 800 and 8 000 bins, Encoder3 at 2 000) and G15 (Encoder2b at 2 048) fixtures: the walk with
    dtype=torch.float32, the default call and the pre-``dtype`` form are the same bits, so test_oracle_golden.py still pins all three."""
    sd = synth_sd(kind, 0)
    x = torch.from_numpy((np.random.RandomState(xseed).rand(1, 128, n) * 0.5).astype(np.float32))
    nlev = R.NLEV[kind]
    old = _walk_before_dtype(sd, x, nlev, expanding=kind != "Encoder2b")
    new = O.encoder2b_forward(sd, x) if kind == "Encoder2b" else O.encoder_unet_forward(sd, x, nlev)
    explicit = R.walk(kind, sd, x, torch.float32)
    assert [o.shape[2] for o in new] == R.level_sizes(kind, n) and len(old) == len(new) == len(explicit)
    for a, b, c in zip(old, new, explicit):
        assert a.dtype == b.dtype == torch.float32 and torch.equal(a, b) and np.array_equal(b.numpy(), c)
    if kind == "Encoder2" and n == 800:
        g = golden("G3_encoder23.npz")
        assert max(maxabs(y[0].numpy(), g[f"e2_{i}"]) for i, y in enumerate(new)) < 2e-5


@pytest.mark.parametrize("kind,n", [("Encoder2", 800), ("Encoder2", 32), ("Encoder3", 2000), ("Encoder3", 8), ("Encoder2b", 800)])
@pytest.mark.parametrize("seed", R.SEEDS)
def test_fp64_walk_is_within_the_fp32_walks_rounding(kind, n, seed):
    """Every level of the fp32 walk against the fp64 one (E32 of tests/unet_ref.py, the unit of the GPU tests' bounds).  A conv's fp32
    round-off is ~2^-24 sqrt(K) of its output's scale (K = 9 x 128 = 1 152 products: 2e-6) and the residual streams carry it on unamplified,
    so the 40 (24, 20) convs add up like a random walk: sqrt(40) x 2e-6 = 1.3e-5 at most - observed 3.7e-7 (n = 8) .. 1.5e-6 (n >= 800).
    Bound 1e-5.  The fp64 walk returns float64 and does not come out of the fp32 weights' rounding alone: it differs from the fp32 walk."""
    w32, w64 = R.walks(kind, seed, n)
    assert all(a.dtype == np.float32 and b.dtype == np.float64 and a.shape == b.shape == (R.BMAX, 128, m)
               for a, b, m in zip(w32, w64, R.level_sizes(kind, n)))
    worst = R.e32(kind, seed, n, R.BMAX)
    print(f"{kind} n = {n} seed {seed}: fp32 against fp64 walk, E32 = {worst:.3g}")
    assert 0 < worst <= 1e-5
    assert 0 < R.e32(kind, seed, n, 1) <= 1e-5         # row 0 of the same walk: the B = 1 case of the GPU tests


@pytest.mark.parametrize("seed", R.SEEDS)
def test_encoder2b_on_encoder2_weights_is_encoder2s_contracting_path(seed):
    """What lets the GPU test check Encoder2's contracting levels one by one through an Encoder2b: in fp64 the Encoder2b walk on the
    ``lblocks`` / ``blocks`` entries of an Encoder2 state dict IS the contracting path inside the Encoder2 walk, exactly (same ops on the
    same values), and its last level is Encoder2's coarsest output."""
    sd2 = R.unet_sd("Encoder2", seed)
    sdb = R.encoder2b_of(sd2)
    assert sorted(sdb) == sorted(synth_sd("Encoder2b", seed)) and all(sdb[k].shape == v.shape for k, v in synth_sd("Encoder2b", seed).items())
    x = R.values(96)
    outs, contracting = O.encoder_unet_forward(sd2, x, 5, dtype=torch.float64, contracting=True)
    b = O.encoder2b_forward(sdb, x, dtype=torch.float64)
    assert len(b) == len(contracting) == 6 and torch.equal(b[0], x.double())
    for lev in range(6):
        assert b[lev].dtype == torch.float64 and torch.equal(b[lev], contracting[lev]), lev
    assert torch.equal(b[5], outs[5])
    assert not torch.equal(b[4], outs[4])              # ... while the expanding path's levels are something else
    for a, c in zip(R.walks("Encoder2b<-Encoder2", seed, 96)[1], contracting):
        assert np.array_equal(a, c.numpy())


def test_full_conv1d_nlc_entry_prototype_loads():
    """orca_conv1d_nlc_forward_full: declared in include/orca_hip.h (test_abi.py checks export and prototype list), twelve arguments, and it
    refuses a NULL context with ORCA_EINVAL before touching a device."""
    lib = _lib.load()
    res, args = _lib.SIGNATURES["orca_conv1d_nlc_forward_full"]
    old = _lib.SIGNATURES["orca_conv1d_nlc_forward"][1]
    assert res is ctypes.c_int and len(args) == len(old) + 3
    assert args[:6] == old[:6] and args[6] is ctypes.c_void_p and args[7:10] == old[6:] and args[10:] == [ctypes.c_int, ctypes.c_int]
    fn = lib.orca_conv1d_nlc_forward_full
    assert fn.argtypes == args
    assert fn(None, None, _lib.PRECISIONS["f16x2"], None, None, None, None, 1, 32, 0, 0, 0) == -1      # ORCA_EINVAL
    assert b"NULL argument" in lib.orca_last_error()
