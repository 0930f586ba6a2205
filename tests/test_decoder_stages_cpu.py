"""CPU: the oracle's Decoder stages (oracle/orca_oracle.py `decoder_stages`, `decoder_1m_stages`, `decoder_block`) that
tests/test_gpu_decoder_stages.py holds the HIP kernels to - they compose to the forward the golden fixtures pin, fp32 and fp64 agree, the exact
case of the block kernel is exact in every storage format, and a per-stage comparison sees a defect that the end-to-end tolerance hides."""
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
