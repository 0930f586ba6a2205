"""-m gpu: the Encoder's two-strand call (orca_encoder_forward_two_strands) - stages 1-2 per strand, stages 3-7 as ONE pass over both strands,
which share one set of planes with a zero gap between them (stages 3-4) and run as a batch of two rows (stages 5-7).  Every position reads the
inputs and does the arithmetic it would in a call of its own, so everything here is BIT identity against the two per-strand calls
(`Net.set_encoder_two_strands(False)`: the same entry point, the route it replaces)."""
import warnings

import numpy as np
import pytest
import torch

from orca_amd import engine
from orca_amd import orca_predict as P
from tests.arena import assert_arena_independent
from tests.util import product_module

pytestmark = pytest.mark.gpu

# 12 kb: n3 = 750, the second strand at 1 000 - the seam inside a 512-position tile and a 320-position pooled workgroup, four ends close together
# 260 kb: n3 = 16 250 - several tiles per strand at stages 3 and 4, stage 5 (n5 = 650) on the short-row kernel
# 1 Mb: n5 = 2 500 > 2 048 - stages 5 and 6 on the tiled channel-last kernel (both tile shapes are taken at 32 Mb: test_cascade_32m_maps_equal)
LENGTHS = (12_000, 260_000, 1_000_000)


def _codes(L, seed, device):
    """[1,L] uint8: random bases with N runs at both ends and across the middle (the reverse complement's first bases are not the forward's last)."""
    c = np.random.RandomState(seed).randint(0, 4, L).astype(np.uint8)
    c[:37] = 4
    c[L - 91:] = 4
    c[L // 2 - 150:L // 2 + 213] = 4
    c[L // 3:L // 3 + 16] = 4
    return torch.from_numpy(c)[None].to(device)


def _bits(t):
    return t.cpu().numpy().view(np.int32)


def _run(enc, codes, joint):
    """both strands through Encoder.forward_two_strands with the joint pass on / off -> ([2,128,bins] tensor, planar launches it took)"""
    net = enc._net(codes.device)
    net.set_encoder_two_strands(joint)
    assert net.encoder_two_strands() == joint
    out = torch.full((2, 128, engine.encoder_num_bins(codes.shape[1])), float("nan"), dtype=torch.float32, device=codes.device)
    before = net.ctx.launch_counts()["planar"]
    enc.forward_two_strands(codes, out)
    torch.cuda.synchronize()
    net.set_encoder_two_strands(True)
    return out, net.ctx.launch_counts()["planar"] - before


@pytest.fixture(scope="module")
def enc(cuda):
    return product_module("Encoder", 0, device=cuda)


@pytest.fixture(scope="module")
def split(enc, cuda):
    """the per-strand route's results, computed once per (precision, length)"""
    cache = {}

    def get(precision, L):
        if (precision, L) not in cache:
            enc.precision = precision
            cache[(precision, L)] = _run(enc, _codes(L, L % 97, cuda), False)
        return cache[(precision, L)]
    return get


@pytest.mark.parametrize("L", LENGTHS)
@pytest.mark.parametrize("precision", ("f16x2", "bf16"))
def test_joint_pass_is_bit_identical(enc, split, cuda, precision, L):
    ref, n_split = split(precision, L)
    enc.precision = precision
    out, n_joint = _run(enc, _codes(L, L % 97, cuda), True)
    assert n_joint < n_split                      # it IS the joint route: stages 3-4 launched once
    assert np.isfinite(ref.cpu().numpy()).all()
    assert np.array_equal(_bits(out), _bits(ref))
    # and the per-strand route of this entry point is the two calls everyone else makes
    for k, rev in enumerate((False, True)):
        assert np.array_equal(_bits(enc.forward_codes(_codes(L, L % 97, cuda), reverse=rev)[0]), _bits(ref[k]))


@pytest.mark.parametrize("precision", ("f16x2", "bf16"))
def test_gap_does_not_rely_on_a_fresh_workspace(enc, split, cuda, precision):
    """the 12 kb case twice in one process with a 1 Mb call in between: the second time its gap, guards and tails lie where the longer call
    kept activations; then the same call on an arena filled with 0x00, 0xFF and 0x3C (tests/arena.py): the per-strand route's bits under every
    fill, and no fill raises the range flag"""
    ref, _ = split(precision, LENGTHS[0])
    enc.precision = precision
    for L in (LENGTHS[0], LENGTHS[2], LENGTHS[0]):
        out, _ = _run(enc, _codes(L, L % 97, cuda), True)
        if L == LENGTHS[0]:
            assert np.array_equal(_bits(out), _bits(ref))
    L = LENGTHS[0]
    net, codes = enc._net(cuda), _codes(L, L % 97, cuda)
    enc._apply_precision(net, precision)
    assert net.encoder_two_strands()

    def joint():      # the engine call itself: the module's range-guard retry would consume a flag that arena contents raised
        return engine.encoder_forward_two_strands(net, codes, torch.full((2, 128, engine.encoder_num_bins(L)), float("nan"), dtype=torch.float32, device=cuda))
    bits = assert_arena_independent(net.ctx, joint, what=("two strands", precision))
    assert np.array_equal(bits, _bits(ref).reshape(-1))


def test_guard_fires_on_the_reverse_strand_only(cuda):
    """A sequence of A / C only: its forward strand never multiplies the first layer's G / T columns, its reverse complement (G / T only) reads
    nothing else.  With those columns scaled up the fp16-range flag is raised by the reverse strand alone; the joint call must raise it too, and
    its range-safe retry must give what the per-strand calls' retries give."""
    L = 12_000
    enc = product_module("Encoder", 0)
    sd = {k: v.clone() for k, v in enc.state_dict().items()}
    sd["lconv1.0.weight"][:, 2:4, :] *= 4.0e4
    enc.load_state_dict(sd)
    enc = enc.to(cuda)
    enc.precision = "f16x2"
    codes = torch.from_numpy(np.random.RandomState(9).randint(0, 2, L).astype(np.uint8))[None].to(cuda)

    def warned(fn):
        with warnings.catch_warnings(record=True) as w:
            warnings.simplefilter("always")
            out = fn()
        return out, any("fp16 range" in str(m.message) for m in w)

    fwd, w_f = warned(lambda: enc.forward_codes(codes, reverse=False))
    rev, w_r = warned(lambda: enc.forward_codes(codes, reverse=True))
    assert not w_f and w_r
    (out, _), w_j = warned(lambda: _run(enc, codes, True))
    assert w_j
    (ref, _), w_s = warned(lambda: _run(enc, codes, False))
    assert w_s
    assert np.isfinite(out.cpu().numpy()).all()
    assert np.array_equal(_bits(out), _bits(ref))
    assert np.array_equal(_bits(out[1]), _bits(rev[0]))      # the retried strand: bf16x3, as its own call retried it
    assert not enc._net(cuda).ctx.take_overflow()            # the flag was consumed by the retry


def test_routing(enc, cuda, monkeypatch):
    L = LENGTHS[0]
    codes = _codes(L, L % 97, cuda)
    enc.precision = "f16x2"
    assert P._joint_encode(enc, codes) is not None
    # what keeps its two calls: float strands, a batch, ragged or chunked lengths, the range-safe arithmetic, a forced form, two streams
    assert P._joint_encode(enc, torch.zeros((1, 4, L), device=cuda)) is None
    assert P._joint_encode(enc, torch.cat([codes, codes])) is None
    assert P._joint_encode(enc, codes[:, :L - 16]) is None
    monkeypatch.setenv("ORCA_ENCODER_CHUNK_BP", "8000")
    assert P._joint_encode(enc, codes) is None
    monkeypatch.delenv("ORCA_ENCODER_CHUNK_BP")
    monkeypatch.setenv("ORCA_STRAND_STREAMS", "1")
    assert P._joint_encode(enc, codes) is None
    monkeypatch.delenv("ORCA_STRAND_STREAMS")
    enc.form = "two_conv"
    assert P._joint_encode(enc, codes) is None
    enc.form = "default"
    for precision in ("bf16x3", "bf16x2", "f32"):
        enc.precision = precision
        assert P._joint_encode(enc, codes) is None
    # ... and the library agrees where the call reaches it all the same: bf16x3 runs no planar launch, the forced form as many as two calls
    enc.precision = "bf16x3"
    out, n = _run(enc, codes, True)
    assert n == 0
    for k, rev in enumerate((False, True)):
        assert np.array_equal(_bits(out[k]), _bits(enc.forward_codes(codes, reverse=rev)[0]))
    enc.precision = "f16x2"
    enc.form = "two_conv"
    _, n_on = _run(enc, codes, True)
    _, n_off = _run(enc, codes, False)
    enc.form = "default"
    assert n_on == n_off
    # a bin range is a per-strand call of its own and gives the joint call's bins
    full, _ = _run(enc, codes, True)
    part = enc.forward_codes(codes, reverse=True, bin_lo=1, bin_hi=3)
    assert np.array_equal(_bits(part[0]), _bits(full[1][:, 1:3]))
    # _encode_two_strands: the joint call for one sequence, the two calls for a batch
    calls = []
    enc0 = torch.empty((2, 128, 3), dtype=torch.float32, device=cuda)
    P._encode_two_strands(lambda rev, out: calls.append(rev), enc0, 1, lambda out: calls.append("joint"))
    P._encode_two_strands(lambda rev, out: calls.append(rev), torch.empty((4, 128, 3), device=cuda), 2, lambda out: calls.append("joint"))
    P._encode_two_strands(lambda rev, out: calls.append(rev), enc0, 1)
    assert calls == ["joint", False, True, False, True]


def test_cascade_32m_maps_equal(cuda):
    """cascade_32m on both strands of a packed 32 Mb window (the shape whose stage 5 takes the 256-position tiles and stage 6 the 64-position
    ones; a 1 Mb window has too few bins for the 32 Mb cascade): every map with the joint pass equals the map without it."""
    from orca_amd import orca_models as M
    model = M.H1esc(synthetic_seed=0)
    L = 32_000_000
    codes = torch.randint(0, 4, (1, L), dtype=torch.uint8, device=cuda, generator=torch.Generator(device=cuda).manual_seed(7))
    codes[:, :500] = 4
    codes[:, L - 777:] = 4
    codes[:, L // 2 - 3000:L // 2 + 5000] = 4
    net = model.net0._net(cuda)
    res = {}
    for joint in (True, False):
        net.set_encoder_two_strands(joint)
        before = net.ctx.launch_counts()["planar"]
        preds, starts, merged = P.cascade_32m(model, [codes, codes], 16_000_000 + 1_234_567, 16_000_000, [False, True], merge=True)
        torch.cuda.synchronize()
        res[joint] = (preds, merged, net.ctx.launch_counts()["planar"] - before)
    net.set_encoder_two_strands(True)
    assert res[True][2] < res[False][2]
    for a, b in zip(res[True][0] + res[True][1], res[False][0] + res[False][1]):
        assert torch.equal(a, b)
