"""-m gpu: `orca_encoder_probe` - the production route of every arithmetic (f16x2 planes, bf16x3 / bf16x2 channel-last, exact fp32, bf16 planes)
stopped behind a stage - against the fp64 oracle at EVERY position and channel of that stage, not behind the 4 000x of MaxPools where only a
window's argmax survives.  Two references per case: (a) the fp64 chain from the bases (the end-to-end error at that stage) and (b) stage k in
fp64 from the probe's own stage k - 1 (one stage isolated, as test_every_block_of_the_chain isolates a Decoder block).  The error measure is
`rel_err` (max |diff| / max(1, max |ref|)) over everything, and the same over the first and last 40 positions (the edge zones that the edge
chains recompute), held to the SAME bound.  Bounds: tests/encoder_probe_ref.py BOUNDS; measurements in the docstrings below.  The preconditions
(host pooling, the oracle's restart, how large the faults are that this file exists for) are tests/test_encoder_probe_cpu.py."""
import numpy as np
import pytest
import torch

from orca_amd import engine
from orca_amd._lib import OrcaHipError
from tests.encoder_probe_ref import (BOUNDS, EDGE, FP32_CLASS, PRECISIONS, PROBE_WEIGHTS, errs, interior_err, oracle, pool, probe_codes, restart,
                                     stages_rows)
from tests.encoder_ref import encoder_sd, onehot, rel_err, strand_codes
from tests.range_guard_ref import ENCODER_FORMS

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def mods(cuda):
    from orca_amd import orca_modules as pm
    res = {}
    for w in PROBE_WEIGHTS:
        m = pm.Encoder()
        m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in encoder_sd(*w).items()}, strict=True)
        res[w] = m.eval().to(cuda)
    return res


def _net(m, cuda, precision, form="default"):
    """The module's engine net in ``precision`` and ``form`` (what Encoder.forward sets before it calls the library)."""
    m.form = form
    net = m._net(cuda)
    m._apply_precision(net, precision)
    return net


def _dev(a, cuda):
    return torch.from_numpy(np.ascontiguousarray(a)).to(cuda)


def _held(what, precision, stage, kind, allp, edge, interior=float("nan")):
    """Print the figure, then hold it - and its edge zones - to the bound of (precision, stage, reference kind)."""
    bound = BOUNDS[precision][stage][kind]
    print(f"PROBE {precision} stage {stage} ({'ab'[kind]}) {what}: {allp:.3g} edge {edge:.3g} interior {interior:.3g} bound {bound}")
    if bound is not None:
        assert allp <= bound and edge <= bound, (what, precision, stage, "ab"[kind], allp, edge, bound)


# ---- lengths: default form, packed codes, both strands ----------------------------------------------------------------------------------------
LENGTHS = [(80, 4), (4000, 7), (16 * 255, 7), (16 * 260, 7), (8240, 7), (4000 * 3 + 777, 7)]     # (L, stages probed)


@pytest.mark.parametrize("L,upto", LENGTHS)
@pytest.mark.parametrize("precision", PRECISIONS)
def test_every_stage_of_every_pipeline(mods, cuda, precision, L, upto):
    """Stages 1..7 (L = 80: one stage-4 position, stages 1..4, and the refusal of stage 5) of the default form from packed codes with N runs
    (one at position 0), both strands, both weight sets, at L = 4 000 (one bin), 16 x 255 / 16 x 260 (stage 3 either side of a 256-position tile,
    stage 2 at 1 020 / 1 040), 8 240 (stage 2 at 2 060 positions: above the n <= 2 048 switch from conv_small.h to conv_bf16s.h) and 12 777 (no
    pool divides it).
    Worst observed on the MI355X over every case of this file (this test, the long launches, the forms x sources), stages 1..7; "edge": the worst
    inside the edge zones alone; (a) from the bases, (b) from the probe's own previous stage (stages 2..7); bounds = 3.5 x, BOUNDS:
      f16x2  (a) 8.16e-7 1.57e-6 2.00e-6 2.41e-6 2.55e-6 1.65e-6 1.69e-6   edge 6.83e-7 1.43e-6 2.00e-6 2.05e-6 2.55e-6 1.65e-6 1.69e-6
             (b)         1.56e-6 1.20e-6 1.79e-6 1.15e-6 9.22e-7 9.07e-7   edge         1.25e-6 1.16e-6 1.78e-6 1.15e-6 9.22e-7 9.07e-7
      bf16x3 (a) 1.02e-6 1.29e-6 1.40e-6 1.54e-6 1.15e-6 1.08e-6 9.27e-7   edge 7.79e-7 1.22e-6 1.10e-6 1.54e-6 1.15e-6 1.08e-6 9.27e-7
             (b)         1.20e-6 4.51e-7 6.62e-7 4.68e-7 3.08e-7 2.00e-7   edge         1.08e-6 4.25e-7 6.62e-7 4.68e-7 3.08e-7 2.00e-7
      bf16x2 (a) 8.72e-6 1.57e-5 1.68e-5 2.55e-5 1.86e-5 2.32e-5 1.74e-5   edge 7.78e-6 1.57e-5 1.54e-5 2.55e-5 1.86e-5 2.32e-5 1.74e-5
             (b)         1.29e-5 1.21e-5 1.37e-5 1.15e-5 1.17e-5 9.48e-6   edge         1.16e-5 1.21e-5 1.37e-5 1.15e-5 1.17e-5 9.48e-6
      f32    (a) 1.17e-6 1.83e-6 1.87e-6 3.17e-6 2.22e-6 2.03e-6 1.40e-6   edge 9.77e-7 1.54e-6 1.76e-6 2.89e-6 2.22e-6 2.03e-6 1.40e-6
             (b)         1.85e-6 1.64e-6 2.01e-6 1.54e-6 1.08e-6 8.43e-7   edge         1.33e-6 1.30e-6 2.01e-6 1.54e-6 1.08e-6 8.43e-7
      bf16   (a) 5.79e-3 7.24e-3 7.87e-3 1.27e-2 8.71e-3 1.01e-2 8.12e-3   edge 4.74e-3 6.97e-3 7.87e-3 1.27e-2 8.71e-3 1.01e-2 8.12e-3
             (b)         6.62e-3 6.01e-3 6.98e-3 5.02e-3 6.01e-3 4.58e-3   edge         6.27e-3 5.71e-3 6.98e-3 5.02e-3 6.01e-3 4.58e-3
    (behind stage 4 a probed tensor has at most 159 positions: the edge zones are half of it or all of it.)  No edge zone measures worse than
    its interior by more than the spread between the weight sets: edge / interior per case has a median of 0.6 - 1.09 and is at most 1.31 at
    the stages with edge chains (1 - 3; 1.40 at stage 4 of L = 8 240, where 80 of the 103 positions are edge zone).  f32 measures 1.05 - 1.3 x f16x2 at stages 1 - 5 (median per case; below it at stages 6 - 7), bf16x3 1.2 x at stage 1 and
    0.4 - 0.8 x behind it: all of it fp32 accumulation round-off of 7 - 25 units of 2^-23, inside the spread between the two weight sets (up to
    1.8 x at one stage) - the fp32 matrix instruction rounds after every 2 products of a K = 576 .. 1 152 sum, the 16-bit ones after every 16, and
    the f32 pipeline's stages 1 - 3 are measured unpooled, small values included."""
    for w, m in mods.items():
        sd = encoder_sd(*w)
        net = _net(m, cuda, precision)
        codes = probe_codes(L, 500 + L % 1000)
        dcodes = _dev(codes, cuda)
        for rev in (False, True):
            ref = oracle(w, L, 500 + L % 1000, rev, upto)
            prev = None
            for k in range(1, upto + 1):
                t, pl = engine.encoder_probe(net, codes=dcodes, reverse=rev, stage=k)
                got = t.cpu().numpy()
                want = pool(ref[k], pl)
                assert got.shape == want.shape, (k, got.shape, want.shape)
                _held(f"L={L} w={w} rev={rev}", precision, k, 0, *errs(got, want), interior_err(got, want))
                if prev is not None:
                    want = pool(restart(sd, prev[0], prev[1], k), pl)
                    _held(f"L={L} w={w} rev={rev}", precision, k, 1, *errs(got, want), interior_err(got, want))
                prev = (got, pl)
            if upto < 7:
                with pytest.raises(OrcaHipError, match="orca_encoder_probe"):
                    engine.encoder_probe(net, codes=dcodes, reverse=rev, stage=upto + 1)


# ---- one long launch per pipeline -----------------------------------------------------------------------------------------------------------------
LONG = [(16 * 2050, ()), (70_000, (32_768, 65_536)), (4 * 65_800, (4 * 32_768, 4 * 65_536))]     # (L, the bases the inner windows lie around)


@pytest.mark.parametrize("L,anchors", LONG)
@pytest.mark.parametrize("precision", PRECISIONS)
def test_long_launches_in_windows(mods, cuda, precision, L, anchors):
    """Stages 1..3 of one long sequence.  L = 16 x 2 050 puts stage 3 of the channel-last pipeline on conv_bf16s.h (2 050 > 2 048 positions);
    L = 70 000 makes every stage-1 launch (and the probe's own copy-out) one of more than 65 535 positions; L = 4 x 65 800 puts stage 2 of the
    planar pipelines on their >= 65 536-position kernels, conv_p16x.h on P16 and conv_p16w1.h on B16 planes (asserted on the launch records).
    Compared in windows: the first and last 40 positions of the probed tensor and 40 around the anchors - positions 32 768 and 65 536 of the
    stage-1 grid (L = 70 000) / of the stage-2 grid (L = 263 200) - against the oracle on slices of +-512 bases around them (cut on the 80-base
    grid, so that every pool window of the slice is one of the sequence's): exact, the reach of a stage-3 position is 336 bases
    (test_encoder_stages_cpu.py).  Reference (a) only.  Held to BOUNDS like every case."""
    w = PROBE_WEIGHTS[0]
    sd = encoder_sd(*w)
    net = _net(mods[w], cuda, precision)
    codes = probe_codes(L, 9)
    dcodes = _dev(codes, cuda)
    for rev in (False, True):
        sc = strand_codes(codes, rev)
        slices = {}
        for k in (1, 2, 3):
            net.ctx.set_timing(k == 2)
            try:
                t, pl = engine.encoder_probe(net, codes=dcodes, reverse=rev, stage=k)
                tags = {(cout, tile) for cout, cin, tile, batch, n, ms, ksize in net.ctx.get_timing()} if k == 2 else set()
            finally:
                net.ctx.set_timing(False)
            if k == 2 and L >= 4 * 65_536 and precision in ("f16x2", "bf16"):
                assert (96, -14 if precision == "f16x2" else -10) in tags, sorted(tags)
            got = t.cpu().numpy()
            g = (1, 4, 16)[k - 1] * pl                                                   # bases per position of the probed tensor
            n = got.shape[0]
            assert n == (L // (1, 4, 16)[k - 1]) // pl
            assert n >= 2 * EDGE
            for a in sorted({0, n - EDGE} | {p // g - EDGE // 2 for p in anchors if p + 40 * g < L}):
                b0, b1 = max(0, (a * g - 512) // 80 * 80), min(L, (a + EDGE) * g + 512)
                if (b0, b1) not in slices:
                    slices[(b0, b1)] = stages_rows(sd, onehot(sc[b0: b1])[0].numpy(), 3)
                want = pool(slices[(b0, b1)][k], pl)[a - b0 // g: a - b0 // g + EDGE]
                allp = rel_err(got[a: a + EDGE], want)                                   # (relative to the window's own max |ref|)
                _held(f"L={L} rev={rev} window {a}", precision, k, 0, allp, allp if a in (0, n - EDGE) else 0.0)


# ---- forms x sources --------------------------------------------------------------------------------------------------------------------------------
def _sources(codes, cuda, precision):
    """name -> (probe keyword arguments, the float rows [4, L] the oracle reads)."""
    L = len(codes)
    rows = onehot(codes)[0].numpy().astype(np.float32)                                   # [4, L]
    flat = _dev(rows.T, cuda)                                                             # [L, 4] contiguous
    res = {"codes": (dict(codes=_dev(codes, cuda)), rows),
           "flat rows": (dict(x=flat.t()), rows),                                         # strides (1, 4): read in place
           "channel-major rows": (dict(x=_dev(rows, cuda)), rows)}                        # strides (L, 1): gathered first
    if precision in ("bf16x3", "bf16x2", "f32"):                                          # these promise fp32 range for ANY float rows
        arb = np.random.RandomState(14).rand(4, L).astype(np.float32)
        res["arbitrary rows"] = (dict(x=_dev(arb.T, cuda).t()), arb)
    return res


# the forms that run the same launches, per pipeline and source (orca_encoder.hip: enc_route)
def _route_classes(precision, source):
    packed = source == "codes"
    if precision in ("f16x2", "bf16"):
        return [["default"], ["stored_residual"], ["lconv1_only"], ["two_conv"]] if packed else [["default", "stored_residual"], ["lconv1_only"], ["two_conv"]]
    if precision == "f32" or packed:
        return [["default", "stored_residual"], ["lconv1_only", "two_conv"]]
    return [list(ENCODER_FORMS)]                                                          # channel-last from float rows: stage 1 never composed


@pytest.mark.parametrize("precision", PRECISIONS)
def test_forms_and_sources(mods, cuda, precision):
    """Stages 1 and 2 at L = 16 x 260 in every form of range_guard_ref.ENCODER_FORMS - two_conv, lconv1_only and stored_residual are what
    extreme weights and float rows fall back to - from packed codes, flat [L, 4] rows seen as a transposed view, contiguous [4, L] rows (gathered
    first) and, in the modes that promise fp32 range for them, arbitrary float rows (uniform in [0, 1)); both weight sets.  Held to BOUNDS.
    That a form did take its own route is asserted on the launch records (get_timing: launches over >= 65 536 positions, so on a stage-1
    probe of 70 000 positions of the same net and source kind): forms the route treats alike leave the same records, all others differ."""
    L = 16 * 260
    ctx = engine.get_context(cuda)
    for w, m in mods.items():
        sd = encoder_sd(*w)
        codes = probe_codes(L, 260)
        try:
            for name, (kw, rows) in _sources(codes, cuda, precision).items():
                ref = stages_rows(sd, rows, 2)
                for form in ENCODER_FORMS:
                    net = _net(m, cuda, precision, form)
                    prev = None
                    for k in (1, 2):
                        t, pl = engine.encoder_probe(net, stage=k, **kw)
                        got = t.cpu().numpy()
                        want = pool(ref[k], pl)
                        _held(f"{form} / {name} w={w}", precision, k, 0, *errs(got, want), interior_err(got, want))
                        if prev is not None:
                            want = pool(restart(sd, prev[0], prev[1], k), pl)
                            _held(f"{form} / {name} w={w}", precision, k, 1, *errs(got, want), interior_err(got, want))
                        prev = (got, pl)
            if w != PROBE_WEIGHTS[0]:
                continue
            long_codes = probe_codes(70_000, 11)
            for name, (kw, _) in _sources(long_codes, cuda, precision).items():
                sig = {}
                for form in ENCODER_FORMS:
                    net = _net(m, cuda, precision, form)
                    ctx.set_timing(True)
                    try:
                        engine.encoder_probe(net, stage=1, **kw)
                        sig[form] = sorted((cout, cin, tile, n, ksize) for cout, cin, tile, batch, n, ms, ksize in ctx.get_timing())
                    finally:
                        ctx.set_timing(False)
                classes = _route_classes(precision, name)
                for c in classes:
                    assert all(sig[f] == sig[c[0]] for f in c), (name, c, sig)
                firsts = [sig[c[0]] for c in classes]
                assert all(firsts[i] != firsts[j] for i in range(len(firsts)) for j in range(i)), (name, sig)
        finally:
            m.form = "default"


# ---- the probe is the production route ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", [4000, 4000 * 3 + 777])
@pytest.mark.parametrize("precision", PRECISIONS)
def test_stage7_is_the_forward_bit_for_bit(mods, cuda, precision, L):
    """Stage 7 of the probe IS `encoder_forward_codes` (both strands) / `encoder_forward` (flat and channel-major float rows) of the same input:
    torch.equal.  The probe is the production route with an early return, not a look-alike."""
    w = PROBE_WEIGHTS[0]
    net = _net(mods[w], cuda, precision)
    codes = probe_codes(L, 70 + L % 100)
    dcodes = _dev(codes, cuda)
    for rev in (False, True):
        t, pl = engine.encoder_probe(net, codes=dcodes, reverse=rev, stage=7)
        out = engine.encoder_forward_codes(net, dcodes[None], reverse=rev)
        assert pl == 1 and tuple(t.shape) == (L // 4000, 128) and torch.equal(t.t(), out[0]), (rev,)
    rows = onehot(codes)[0].numpy().astype(np.float32)
    for x in (_dev(rows.T, cuda).t(), _dev(rows, cuda)):
        t, _ = engine.encoder_probe(net, x=x, stage=7)
        assert torch.equal(t.t(), engine.encoder_forward(net, x[None])[0])
    assert not net.ctx.take_overflow()


def test_arguments_and_the_part_exports_still_refuse(mods, cuda):
    """Both or neither input, a stage outside 1..7 and a stage with no position left are refused (ORCA_EINVAL, before any launch); the part
    exports still refuse a net that is not in the f16x2 arithmetic."""
    m = mods[PROBE_WEIGHTS[0]]
    codes = _dev(probe_codes(4000, 1), cuda)
    net = _net(m, cuda, "bf16x3")
    for bad in (dict(), dict(codes=codes, x=torch.zeros(4, 4000, device=cuda))):
        with pytest.raises(ValueError):
            engine.encoder_probe(net, stage=1, **bad)
    for stage in (0, 8):
        with pytest.raises(OrcaHipError, match="orca_encoder_probe"):
            engine.encoder_probe(net, codes=codes, stage=stage)
    with pytest.raises(OrcaHipError, match="no position"):
        engine.encoder_probe(net, codes=codes[:79], stage=4)
    for precision in ("bf16x3", "bf16x2", "f32", "bf16"):
        with pytest.raises(OrcaHipError, match="f16x2"):
            engine.encoder_stage3_planes(_net(m, cuda, precision), codes)
    _net(m, cuda, "f16x2")


def test_recorded_faults_exceed_the_recorded_bounds():
    """The smallest fault measured by test_encoder_probe_cpu.py::test_faults_exceed_the_bounds (0.100: stage 1's composed groups without their
    exact ends, gain 1.6, pooled) is more than 10 x the largest stage-1 bound of the fp32-class modes (4.1e-6) and of bf16x2 (3.1e-5), and
    more than 3 x the stage-1 bound of bf16 (2.1e-2): every mode's bound catches every one of the three faults."""
    assert 0.100 > 10 * max(BOUNDS[p][1][0] for p in FP32_CLASS + ("bf16x2",))
    assert 0.100 > 3 * BOUNDS["bf16"][1][0]
