"""The 1 Mb mutagenesis screen (orca_amd/screen.py) without a GPU: edits against a numpy restatement, their validation, the generators, the
batch plan against the fp64 oracle's Encoder stages (the rows an edit changes are among the rows the plan recomputes, and the plan's front runs
give them exactly), the score formulas, and no silent CPU path."""
import numpy as np
import pytest
import torch

from orca_amd import screen as S
from orca_amd._lib import OrcaHipError
from tests.encoder_ref import encoder_sd, pool5, stages


def _restate(codes, kind, pos, length, seq=None):
    out = [int(c) for c in codes]
    comp = {0: 3, 1: 2, 2: 1, 3: 0, 4: 4}
    if kind == "sub":
        for k in range(length):
            out[pos + k] = "ACGTN".index(seq[k].upper()) if isinstance(seq, str) else int(seq[k])
    elif kind == "mask":
        for k in range(length):
            out[pos + k] = 4
    else:
        span = out[pos: pos + length]
        for k in range(length):
            out[pos + k] = comp[span[length - 1 - k]]
    return np.array(out, dtype=np.uint8)


def test_apply_edit_matches_restatement():
    rs = np.random.RandomState(3)
    codes = rs.randint(0, 4, 400).astype(np.uint8)
    codes[100:110] = 4
    cases = [("sub", 5, 4, "ACGT"), ("sub", 0, 3, "nNa"), ("sub", 397, 3, [4, 0, 3]), ("mask", 50, 17, None), ("mask", 0, 400, None),
             ("inv", 95, 30, None), ("inv", 103, 4, None), ("inv", 0, 400, None), ("inv", 399, 1, None)]
    for kind, pos, ln, seq in cases:
        got = S.apply_edit(codes, S.Edit(kind, pos, ln, seq))
        assert np.array_equal(got, _restate(codes, kind, pos, ln, seq)), (kind, pos, ln)
    # N inside an inverted span stays N, at the mirrored place
    inv = S.apply_edit(codes, S.Edit("inv", 95, 30))
    assert np.all(inv[95 + 125 - 110: 95 + 125 - 100] == 4)
    # an inversion twice is the identity
    e = S.Edit("inv", 37, 201)
    assert np.array_equal(S.apply_edit(S.apply_edit(codes, e), e), codes)


def test_edit_validation():
    with pytest.raises(ValueError):
        S.Edit("del", 0, 1)
    with pytest.raises(ValueError):
        S.Edit("mask", 0, 0)
    with pytest.raises(ValueError):
        S.Edit("inv", 5, -3)
    with pytest.raises(ValueError):
        S.Edit("mask", -1, 3)
    with pytest.raises(ValueError):
        S.Edit("sub", 0, 2, "A")            # payload length
    with pytest.raises(ValueError):
        S.Edit("sub", 0, 1)                 # no payload
    with pytest.raises(ValueError):
        S.Edit("sub", 0, 1, "X")
    with pytest.raises(ValueError):
        S.Edit("sub", 0, 1, [5])
    with pytest.raises(ValueError):
        S.Edit("mask", 0, 2, "AC")          # payload on a mask
    with pytest.raises(ValueError):
        S.Edit("inv", 399, 2).check(400)    # leaves the window
    with pytest.raises(ValueError):
        S.plan_batch([S.Edit("mask", 7990, 20)], 8000)
    with pytest.raises(ValueError):
        S.apply_edit(np.zeros(10, np.uint8), S.Edit("mask", 5, 6))
    S.Edit("inv", 398, 2).check(400)


def test_generators():
    rs = np.random.RandomState(4)
    codes = rs.randint(0, 4, 1000).astype(np.uint8)
    codes[[10, 11, 500]] = 4
    ed = S.saturation_edits(codes, 0, 1000)
    assert len(ed) == 3 * 997 + 4 * 3
    assert all(e.kind == "sub" and e.length == 1 and int(e.seq[0]) != int(codes[e.pos]) for e in ed)
    per = np.bincount([e.pos for e in ed], minlength=1000)
    assert per[10] == per[11] == per[500] == 4 and sorted({int(v) for v in per}) == [3, 4]
    assert {int(e.seq[0]) for e in ed if e.pos == 10} == {0, 1, 2, 3}
    assert len(S.saturation_edits(torch.from_numpy(codes), 200, 210)) == 30
    t = S.tile_edits("mask", 4000, 4000, 0, 1_000_000)
    assert len(t) == 250 and t[0].pos == 0 and t[-1].end == 1_000_000
    t = S.tile_edits("inv", 100, 50, 10, 400)
    assert [e.pos for e in t] == list(range(10, 301, 50)) and all(e.end <= 400 for e in t)
    with pytest.raises(ValueError):
        S.tile_edits("sub", 1, 1, 0, 10)


# ---- the plan against the fp64 oracle -------------------------------------------------------------------------------------------------------
L_PLAN = 48_000


def _plan_edits(L, codes):
    return [S.Edit("sub", 0, 1, [(int(codes[0]) + 1) % 4]), S.Edit("sub", 1, 1, [4]), S.Edit("sub", L - 2, 1, [(int(codes[L - 2]) + 2) % 4]),
            S.Edit("sub", L - 1, 1, [(int(codes[L - 1]) + 3) % 4]), S.Edit("sub", 1_500, 1, [(int(codes[1_500]) + 1) % 4]),
            S.Edit("sub", L - 1_900, 1, [(int(codes[L - 1_900]) + 1) % 4]), S.Edit("sub", 20_011, 1, [(int(codes[20_011]) + 2) % 4]),
            S.Edit("sub", 31_999, 1, [(int(codes[31_999]) + 1) % 4]), S.Edit("inv", 12_345, 900), S.Edit("mask", 39_600, 800)]


@pytest.mark.parametrize("run_max", [S.RUN_MAX_BP, 20_000])
def test_plan_against_oracle_stages(run_max):
    """fp64, synthetic weights at gain 1.6: for every edit the stage-5 rows that change are inside the plan's rows, and the plan's front runs
    (edited snippets concatenated, window ends first / last) give the edited window's rows to 1e-10."""
    sd = encoder_sd(0, 1.6)
    rs = np.random.RandomState(11)
    codes = rs.randint(0, 4, L_PLAN).astype(np.uint8)
    codes[20_000:20_040] = 4
    codes[12_500:12_620] = 4                                         # inside the inverted span
    edits = _plan_edits(L_PLAN, codes)
    plan = S.plan_batch(edits, L_PLAN, run_max=run_max)
    assert len(plan.runs) >= (2 if run_max == S.RUN_MAX_BP else 4)
    wins = np.stack([codes] + [S.apply_edit(codes, e) for e in edits])
    rows = pool5(np.moveaxis(stages(sd, wins, 4)[4], 0, 1))            # [n5, B, 128]
    ref, alt = rows[:, 0], rows[:, 1:]
    n5 = L_PLAN // 400
    assert rows.shape[0] == n5
    for i, e in enumerate(edits):
        changed = np.nonzero(np.abs(alt[:, i] - ref).max(axis=1) > 0)[0]
        r0, r1 = plan.rows[i]
        assert changed.size and r0 <= changed.min() and changed.max() < r1, (e, changed.min(), changed.max(), r0, r1)
    # the packed snippet buffer and the front runs, restated on the host
    buf = np.concatenate([S.apply_edit(codes, edits[i])[plan.snippet[i, 0]: plan.snippet[i, 0] + plan.snippet[i, 1]] for i in plan.order])
    tab = plan.edit_table
    assert tab[0, 0] == 0 and np.all(tab[1:, 0] == tab[:-1, 0] + tab[:-1, 2]) and tab[-1, 0] + tab[-1, 2] == buf.size
    fresh = np.full((plan.n_fresh, 128), np.nan)
    for o0, nb, ranges in plan.runs:
        run_rows = pool5(stages(sd, buf[o0: o0 + nb], 4)[4])
        for skip, count, dst in ranges:
            fresh[dst: dst + count] = run_rows[skip: skip + count]
    assert not np.isnan(fresh).any()
    scale = max(1.0, float(np.abs(alt).max()))
    for i in range(len(edits)):
        r0, r1 = plan.rows[i]
        f0 = plan.fresh[i]
        assert tuple(plan.splice_table[i]) == (r0, r1 - r0, f0)
        assert np.abs(fresh[f0: f0 + r1 - r0] - alt[r0:r1, i]).max() / scale <= 1e-10, edits[i]


def test_plan_runs_respect_window_ends():
    L = 1_000_000
    edits = [S.Edit("sub", p, 1, "A") for p in (0, 5, 999_999, 999_000, 500_000, 1_200)] + [S.Edit("inv", 100_000, 50_000), S.Edit("mask", 0, L)]
    plan = S.plan_batch(edits, L, run_max=100_000)
    for o0, nb, ranges in plan.runs:
        members = [i for i in plan.order if o0 <= plan.edit_table[plan.order.index(i), 0] < o0 + nb]
        for k, i in enumerate(members):
            b0, sn = plan.snippet[i]
            if b0 == 0:
                assert k == 0
            if b0 + sn == L:
                assert k == len(members) - 1
        assert nb <= 100_000 or len(members) == 1
    assert plan.snippet[7].tolist() == [0, L]


def test_score_formulas_against_host_function():
    rs = np.random.RandomState(5)
    n, E = 37, 6
    ref = rs.randn(n, n).astype(np.float32)
    maps = (ref[None] + 0.1 * rs.randn(E, n, n)).astype(np.float32)
    maps[2] = ref
    prof, mean, amax = S.scores_host(maps, ref)
    for e in range(E):
        d = [[abs(float(maps[e, i, j]) - float(ref[i, j])) for j in range(n)] for i in range(n)]
        assert np.allclose(prof[e], [sum(r) / n for r in d], rtol=1e-12, atol=0)
        assert mean[e] == pytest.approx(sum(map(sum, d)) / (n * n), rel=1e-12, abs=0)
        assert amax[e] == max(map(max, d))
    assert mean[2] == 0 and amax[2] == 0


def test_no_silent_cpu_path():
    """A window that is not on the MI355X is an error (on a machine without a GPU every window is), never a CPU computation."""
    from orca_amd import orca_modules as pm
    net = pm.Net(num_1d=4).eval()
    with pytest.raises(OrcaHipError):
        S.screen_1m(net, torch.zeros(40_000, dtype=torch.uint8), [S.Edit("mask", 0, 10)])
