"""The cases of tests/range_guard_ref.py judged without a GPU, from their fp64 references alone: a "must flag" case stores |v| >= 66000
somewhere, a "must not flag" case nothing above 65000, a single spike leaves every other stored value below 16384, and every input,
residual and weight is inside the fp16 range (the test entries' converters raise nothing)."""
import numpy as np
import pytest

from tests import range_guard_ref as G
from tests.util import synth_sd


def _inputs_in_range(*arrays):
    return all(a is None or float(np.abs(a).max()) <= G.F16_MAX for a in arrays)


def _check_spike(ref, at, V):
    """ref: every stored value; ``at``: the spike's index in it."""
    v = float(ref[at])
    assert abs(v - V) < 8.0, (v, V)                   # the spike's weight is a multiple of 1/8: V is met to within 64 / 8, on V's side of the limit
    rest = np.abs(ref).copy()
    rest[at] = 0.0
    assert float(rest.max()) <= G.V_QUIET, float(rest.max())
    if V >= G.V_FLAG:
        assert abs(v) >= G.V_FLAG
    else:
        assert float(np.abs(ref).max()) <= G.V_OK


SHAPES_1D = [(64, 64, 600, 9, 512), (128, 128, 600, 9, 512), (64, 96, 600, 9, 256), (64, 96, 600, 17, 256)]
MODES_1D = [(0, False, False), (0, True, True), (1, False, False), (1, True, True)]
CASES_1D = [s + m for s in SHAPES_1D for m in MODES_1D] + [(96, 96, 65600, 9, 0, 0, False, False), (96, 96, 65600, 9, 0, 1, True, True)]


@pytest.mark.parametrize("cin,cout,n,k,tile,out_mode,relu,residual", CASES_1D)
def test_conv1d_spike_cases(cin, cout, n, k, tile, out_mode, relu, residual):
    c = G.Conv1dSpike(cin, cout, n, k, relu, residual, out_mode)
    if tile:
        places = G.conv1d_placements(n, cout, tile)
        assert {0, n - 1, tile - 1, tile} <= {p for p, _ in places}
        assert {p // 32 for p, _ in places} >= set(range(min(tile, n) // 32))      # every 32-position slice of a tile
    else:
        places = G.p16x_placements(n)
        assert {0, 511, 512, 65535, 65536, n - 1} <= {p for p, _ in places}
        inner = places[6:]
        assert {((p % 512) // 64, co // 48) for p, co in inner} == {(k, cg) for k in range(8) for cg in range(2)}      # every wave
        assert {((p % 64) // 16) for p, _ in inner} == set(range(4)) and {(co % 48) // 16 for _, co in inner} == set(range(3))
    assert {co // 8 for _, co in places} == set(range(cout // 8))             # every octet
    for i, (p, co) in enumerate(places):
        for V in (G.V_FLAG, G.V_OK):
            x, w, r1, q, t = c.place(p, co, V, r_at=0.0 if residual else None)
            assert _inputs_in_range(x, w, r1)
            ref = c.reference(x, w, r1, q)
            _check_spike(ref, (p // c.pool, co), V)
            if i == 0 and n < 10000:
                assert float(np.abs(ref - c.full_reference(x, w, r1)).max()) < 1e-9


@pytest.mark.parametrize("n", [323, 2000])
def test_conv1d_pool5_spike_cases(n):
    c = G.Conv1dSpike(128, 128, n, 9, True, True, 3)
    places = G.pool5_placements(n)
    assert {co // 8 for _, co in places} == set(range(16))
    assert {((p % 320) // 160, co // 32) for p, co in places} == {(pg, cg) for pg in range(2) for cg in range(4)}      # every wave
    assert {p % 5 for p, _ in places} == set(range(5)) and all(p < 5 * (n // 5) for p, _ in places)
    for p, co in places:
        for V in (G.V_FLAG, G.V_OK):
            x, w, r1, q, t = c.place(p, co, V, r_at=0.0)
            assert _inputs_in_range(x, w, r1)
            _check_spike(c.reference(x, w, r1, q), (p // 5, co), V)


def test_conv1d_residual_and_relu_cases():
    c = G.Conv1dSpike(64, 64, 600, 9, True, True, 0)
    for r_at, want in ((40000.0, 80000.0), (25000.0, 65000.0)):
        x, w, r1, q, t = c.place(300, 21, 40000.0, r_at=r_at)           # conv 40000 + residual: only the sum leaves the range
        assert _inputs_in_range(x, w, r1)
        ref = c.reference(x, w, r1, q)
        assert abs(ref[300, 21] - want) < 8.0
        assert float(np.abs(ref).max()) == abs(ref[300, 21])
    x, w, r1, q, t = c.place(300, 21, -G.V_FLAG, r_at=0.0)                # -66000 in front of the ReLU: 0 stored
    assert _inputs_in_range(x, w, r1)
    assert float(np.abs(c.reference(x, w, r1, q)).max()) <= G.V_QUIET
    assert float(np.abs(c.full_reference(x, w, r1) - c.reference(x, w, r1, q)).max()) < 1e-9


@pytest.mark.parametrize("n,B", G.CONV2D_MAPS)
def test_conv2d_spike_cases(n, B):
    for dil, cin, cout, res in G.CONV2D_LAYERS:
        c = G.Conv2dSpike(cin, cout, n, dil, B, relu=res, residual=res)
        for k, (i, j) in enumerate(G.conv2d_pixels(n, dil, B)):
            co = (9 * k) % cout
            for V in (G.V_FLAG, G.V_OK):
                w = c.weight(B - 1, i, j, co, V)
                assert _inputs_in_range(c.x0, w, c.r0)
                patch = dict(c.reference_patch(w, B - 1, i, j))
                r = 0.0 if c.r0 is None else float(c.r0[B - 1, co, i, j])
                v = float(patch[(i, j)][co])
                assert abs(v - (V + r)) < 8.0
                rest = max(float(np.abs(np.delete(vec, co) if px == (i, j) else vec).max()) for px, vec in patch.items())
                assert max(rest, float(np.abs(c.stored0).max())) <= G.V_QUIET
                assert v >= G.V_FLAG - 3.0 if V == G.V_FLAG else v <= G.V_OK + 3.0       # (+- the residual's own O(1) value at the pixel)
                if k == 0 and n <= 30:
                    assert float(np.abs(c.reference(w, B - 1, i, j) - c.full_reference(w, B - 1, i, j)).max()) < 1e-9


def test_dblock_cases():
    c = G.DBlockCase(G.DBLOCK_N, G.DBLOCK_B)
    for d in G.DBLOCK_DILS:
        pixels = c.pixels(d)
        assert (d, d) in pixels and (d - 1, d) in pixels                  # the map has a sub-image boundary at this dilation
        for i, j in pixels:
            for xv, flag in ((c.X_HI, True), (c.X_LO, False)):
                x = c.x0.copy()
                x[1, 9, i, j] = xv
                assert _inputs_in_range(x, *[w for w, _ in c.convs], *[b for _, b in c.convs])
                ref = c.reference(x)
                assert (float(np.abs(ref).max()) >= G.V_FLAG) if flag else (float(np.abs(ref).max()) <= G.V_OK)
                rest = np.abs(ref).copy()
                rest[1, 9, i, j] = 0.0
                assert float(rest.max()) <= G.V_QUIET


@pytest.mark.parametrize("B", [1, 2])
def test_decoder_head_cases(B):
    x0, de0, y0 = G.head_inputs(B)
    assert _inputs_in_range(x0, de0, y0)
    for i in G.HEAD_SUM_PIXELS:
        for v, flag in ((G.HEAD_X_BAD, True), (G.HEAD_X_OK, False)):
            x = x0.astype(np.float64)
            x[B - 1, G.HEAD_C, i] = v
            assert v <= G.F16_MAX
            s = x[:, :, :, None] + x[:, :, None, :]
            if flag:
                assert s[B - 1, G.HEAD_C, i, i] >= G.V_FLAG
                s[B - 1, G.HEAD_C, i, i] = 0.0
                assert float(np.abs(s).max()) <= G.V_OK           # the pixel (i, i) alone
            else:
                assert float(np.abs(s).max()) <= G.V_OK
    for mode in ("bilinear", "nearest"):
        for i, j in G.head_y_pixels(mode):
            for v, flag in ((G.HEAD_Y_BAD, True), (G.HEAD_Y_OK, False)):
                y = y0.copy()
                y[B - 1, 0, i, j] = v
                up = np.abs(G.upsampled(y, mode))
                assert (float(up.max()) >= G.V_FLAG) if flag else (float(up.max()) <= G.V_OK), (mode, i, j, v)
                assert float(up[: B - 1].max() if B > 1 else 0.0) <= 16.0
    for i, j in G.HEAD_DE_PIXELS:
        assert max(i, j) < G.HEAD_N                                # -inf there: |v| = inf >= 66000 in the stored distance encoding


def test_encoder_stage1_form_cases():
    from orca_amd import synth
    seq = synth.synth_sequence(G.STAGE1_L, seed=4, n_frac=0.01)                      # [1, L, 4]
    x = np.ascontiguousarray(seq.transpose(0, 2, 1))
    sd0 = synth_sd("Encoder", 0)
    for t in G.stage1_tensors(sd0, x):
        assert float(np.abs(t).max()) <= 64.0                      # the synthetic Encoder: nothing near the range
    mid, l1, a1, o1 = G.stage1_tensors(G.stage1_scaled_sd(sd0), x)
    assert float(np.abs(l1[G.STAGE1_CH]).min()) >= G.V_FLAG        # scaled lconv1: out of range at every position of the channel
    assert float(np.abs(o1[G.STAGE1_CH]).min()) >= G.V_FLAG        # ... in the stored residual and in the stage output that carries it
    for pos in G.STAGE1_POSITIONS:
        xs = x.copy()
        xs[0, :, pos] *= G.STAGE1_BASE_GAIN
        mid, l1, a1, o1 = G.stage1_tensors(sd0, xs)
        assert float(np.abs(mid).max()) >= G.V_FLAG and float(np.abs(l1).max()) >= G.V_FLAG, pos


def test_nlc_big_output_case_is_in_range_on_the_input_side():
    c = G.NlcCase(128, 128, 55)
    x, w, ref = c.big_output(54, 77)
    assert _inputs_in_range(x, w)
    assert abs(ref[2, 54, 77] - 1.0e5) < 8.0
    assert c.X_BAD > G.V_FLAG


@pytest.mark.parametrize("stage", [1, 2])
def test_edge_fix_constructions(stage):
    """The weights of `edge_sd` put +-1e5 where ONLY the edge-fix kernels store it.  Checked by the padded-composition emulation: the conv
    pair on the stage input padded by 8 zeros per side, read back at offset 8, is what a composed 17-tap conv computes."""
    L = 16 * 300
    sd = G.edge_sd(synth_sd("Encoder", 0), stage)
    for k, v in sd.items():
        if k.endswith((".weight", ".bias")) and not (k.endswith(".bias") and np.abs(v).max() > 9e4):
            assert float(np.abs(v).max()) <= G.F16_MAX, k
    codes = np.random.RandomState(5).randint(0, 4, L).astype(np.uint8)
    v = G.edge_views(sd, codes, stage)
    lt, lc = v["lout_true"], v["lout_composed"]
    n = lt.shape[0]
    assert n == (L if stage == 1 else L // 4)
    # the reference's lout: +1e5 at the first four positions of channel EDGE_OUT, -1e5 at the last four, O(1) everywhere else
    assert (lt[:4, G.EDGE_OUT] >= G.V_FLAG).all() and (lt[-4:, G.EDGE_OUT] <= -G.V_FLAG).all()
    rest = np.abs(lt).copy()
    rest[:4, G.EDGE_OUT] = rest[-4:, G.EDGE_OUT] = 0.0
    assert float(rest.max()) <= 16.0
    # what the main kernels see and store: the composed lout, everything in front of it, conv<stage>.a's output, the pooled stage output with
    # the composed residual - all in range, so no main kernel has anything to flag
    assert float(np.abs(lc).max()) <= 16.0
    assert float(np.abs(lt[8:-8] - lc[8:-8]).max()) < 1e-6
    for t in v["stored_before"] + [v["a"], v["out_main"]]:
        assert float(np.abs(t).max()) <= G.V_OK
    ot = v["out_true"]
    if stage == 1:
        # the pool kernel's windows carry it: window 0 and the last window of channel EDGE_OUT; the layer kernel stores conv1.a's ends only (O(1))
        assert ot[0, G.EDGE_OUT] >= G.V_FLAG and ot[-1, G.EDGE_OUT] <= -G.V_FLAG
        assert float(np.abs(v["a"]).max()) <= 16.0
        rest = np.abs(ot).copy()
        rest[[0, -1], G.EDGE_OUT] = 0.0
        assert float(rest.max()) <= 16.0
    else:
        inner = np.abs(ot[1:-1])
        assert float(inner.max()) <= G.V_OK            # stage 2's output outside the end windows (1e4 class: conv2.a reads the 1e5 ends)
