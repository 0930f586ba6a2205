"""``screen_1m(..., strands="both")`` without a GPU: the mirrored plan of the '-' strand against the fp64 oracle's Encoder stages (the front run on
the reverse complement of every packed run, read by the mirrored ranges and spliced by the mirrored segments, gives ALL stage-5 rows of the reverse
complement of the edited window), `mirror_plan` as its own inverse and as a pure transform, the host restatement of the merge, and the argument
checks.  A batch with a ``del`` / ``ins`` item is planned with ``both_strands`` and mirrored too: every one of the n5 rows of every item's '-' image,
whether fresh, a reference row or pooled from a '-' cache entry, against the oracle's rows of the reverse-complemented alt window."""
import copy

import numpy as np
import pytest
import torch

from orca_amd import engine
from orca_amd import screen as S
from orca_amd._lib import OrcaHipError
from tests.encoder_ref import encoder_sd, pool5, revcomp, stages
from tests.test_screen_cpu import L_PLAN, _plan_edits
from tests.test_screen_indel_cpu import indel_items, plan_flank, restate_buffer


def _window():
    rs = np.random.RandomState(11)
    codes = rs.randint(0, 4, L_PLAN).astype(np.uint8)
    codes[20_000:20_040] = 4
    codes[12_500:12_620] = 4                                         # inside the inverted span
    return codes


def _items(codes):
    L = L_PLAN
    two = S.EditSet([S.Edit("sub", 5_003, 2, "NA"), S.Edit("mask", 5_900, 450), S.Edit("inv", 27_000, 700), S.Edit("sub", 27_900, 1, [(int(codes[27_900]) + 1) % 4])],
                    name="two clusters")
    assert len(S.set_clusters(two, L)) == 2
    return _plan_edits(L, codes) + [two]


def _tables_equal(a, b):
    for f in a.__dataclass_fields__:
        x, y = getattr(a, f), getattr(b, f)
        if isinstance(x, np.ndarray):
            assert isinstance(y, np.ndarray) and x.dtype == y.dtype and np.array_equal(x, y), f
        else:
            assert x == y, f


@pytest.mark.parametrize("run_max", [S.RUN_MAX_BP, 20_000])
def test_mirror_plan_against_oracle_stages(run_max):
    """fp64, synthetic weights at gain 1.6.  The '-' strand restated on the host: the reverse complement of every packed run buffer through stages
    1-4 and the pool, read by the MIRRORED ranges; every mirrored fresh segment equals the oracle's stage-5 rows of revcomp(apply_edit(codes, e)) to
    1e-10 over the scale (the bound of the '+' strand's proof), and every row outside the mirrored segments equals the '-' reference row, which
    is the oracle's row of the reverse-complemented edited window too (so the whole row image is proven, not only its fresh part)."""
    sd = encoder_sd(0, 1.6)
    codes = _window()
    items = _items(codes)
    plan = S.plan_batch(items, L_PLAN, run_max=run_max)
    mir = S.mirror_plan(plan)
    assert mir.reverse and not plan.reverse
    assert len(plan.runs) >= (2 if run_max == S.RUN_MAX_BP else 4)
    n5 = L_PLAN // 400
    wins = np.stack([revcomp(codes)] + [revcomp(S.apply_edit(codes, e)) for e in items])
    rows = pool5(np.moveaxis(stages(sd, wins, 4)[4], 0, 1))            # [n5, B, 128], '-' row order
    ref, alt = rows[:, 0], rows[:, 1:]
    assert rows.shape[0] == n5
    # the packed buffer is the '+' strand's: one buffer, in forward coordinates, for both strands
    buf = np.concatenate([S.apply_edit(codes, items[plan.item_of[i]])[plan.snippet[i, 0]: plan.snippet[i, 0] + plan.snippet[i, 1]] for i in plan.order])
    assert mir.order == plan.order and np.array_equal(mir.snippet_table, plan.snippet_table) and np.array_equal(mir.span_table, plan.span_table)
    assert [(o0, nb) for o0, nb, _ in mir.runs] == [(o0, nb) for o0, nb, _ in plan.runs]
    fresh = np.full((mir.n_fresh, 128), np.nan)
    for o0, nb, ranges in mir.runs:
        run_rows = pool5(stages(sd, revcomp(buf[o0: o0 + nb]), 4)[4])          # what the front does with reverse=True: the whole run reverse-complemented
        for skip, count, dst in ranges:
            assert 0 <= skip and skip + count <= nb // 400
            assert np.isnan(fresh[dst: dst + count]).all()                     # no two ranges share a fresh row
            fresh[dst: dst + count] = run_rows[skip: skip + count]
    assert not np.isnan(fresh).any()
    scale = max(1.0, float(np.abs(alt).max()))
    assert mir.seg_off.tolist() == plan.seg_off.tolist()
    for i, item in enumerate(items):
        seg = mir.segments[mir.seg_off[i]: mir.seg_off[i + 1]]
        assert np.all(seg[1:, 0] >= seg[:-1, 0] + seg[:-1, 1])                  # sorted by row_lo, disjoint: what the splice kernel searches
        assert sorted((int(n5 - a - c), int(n5 - a)) for a, c, _ in seg) == S.set_clusters(item, L_PLAN)
        outside = np.ones(n5, dtype=bool)
        for row_lo, cnt, src in seg:
            assert np.abs(fresh[src: src + cnt] - alt[row_lo: row_lo + cnt, i]).max() / scale <= 1e-10, (item, row_lo)
            outside[row_lo: row_lo + cnt] = False
        assert np.abs(alt[outside, i] - ref[outside]).max() / scale <= 1e-10, item
        assert np.abs(alt[~outside, i] - ref[~outside]).max() > 0, item        # the fresh rows do differ from the reference: the check above has teeth


def test_mirror_plan_is_its_own_inverse_and_pure():
    codes = _window()
    for items in (_plan_edits(L_PLAN, codes), _items(codes)):
        for run_max in (S.RUN_MAX_BP, 20_000):
            plan = S.plan_batch(items, L_PLAN, run_max=run_max)
            before = copy.deepcopy(plan)
            mir = S.mirror_plan(plan)
            _tables_equal(plan, before)                                        # the argument is left as it was
            _tables_equal(S.mirror_plan(mir), before)
            n5 = L_PLAN // 400
            assert np.array_equal(mir.rows, np.stack([n5 - plan.rows[:, 1], n5 - plan.rows[:, 0]], axis=1))
            if plan.splice_table is not None:                                  # bare edits: one segment per item, the single-span kernels' table
                assert np.array_equal(mir.splice_table, mir.segments)
                assert np.array_equal(mir.splice_table[:, 0], n5 - plan.splice_table[:, 0] - plan.splice_table[:, 1])
                assert np.array_equal(mir.edit_table, plan.edit_table)


def test_mirrored_runs_respect_window_ends():
    """A run that a window-start snippet opens is, reversed, a run that a window-end snippet closes: in the mirrored ranges the snippet that holds the
    window's start is read LAST in its run and the one that holds its end FIRST."""
    L = 1_000_000
    edits = [S.Edit("sub", p, 1, "A") for p in (0, 5, 999_999, 999_000, 500_000, 1_200)] + [S.Edit("inv", 100_000, 50_000)]
    plan = S.plan_batch(edits, L, run_max=100_000)
    mir = S.mirror_plan(plan)
    fresh_of = {int(plan.fresh[i]): i for i in range(len(edits))}
    for o0, nb, ranges in mir.runs:
        by_skip = sorted(ranges)
        for k, (skip, count, dst) in enumerate(by_skip):
            b0, sn = plan.snippet[fresh_of[dst]]
            if b0 == 0:
                assert k == len(by_skip) - 1
            if b0 + sn == L:
                assert k == 0


def _take_spans(segs):
    return {(r, ph) for a, cnt, ph, _ in segs if ph >= 0 for r in range(a, a + cnt)}


def test_defaults_unchanged_and_the_both_strands_rule():
    """`plan_batch` and `item_sources` without the new argument return what they return with it off; with it on, a take survives only where the
    '-' entry's run holds its cone too: the '-' run may start one stage-4 row later in context coordinates, so the rule bites at the context's
    start (an insertion of 177 bases at base 0: the takes begin at row 6, not 5)."""
    codes = _window()
    plan = S.plan_batch(_plan_edits(L_PLAN, codes), L_PLAN)
    assert plan.reverse is False and plan.both_strands is False and not plan.indel
    _tables_equal(plan, S.plan_batch(_plan_edits(L_PLAN, codes), L_PLAN, both_strands=True))        # no del / ins: the same plan either way
    items = [S.Edit("del", 9_000, 37), S.Edit("mask", 30_000, 500), S.Edit("ins", 700, "ACGTT"), S.Edit("del", L_PLAN - 900, 30), S.Edit("ins", 0, "A" * 177)]
    fewer = 0
    for F in (0, 4_000, 4_037, 1_999):
        C = L_PLAN + F
        ind = S.plan_batch(items, L_PLAN, flank=F)
        assert ind.indel and ind.reverse is False and ind.both_strands is False
        _tables_equal(ind, S.plan_batch(items, L_PLAN, flank=F, both_strands=False))
        with pytest.raises(ValueError, match="mirror_plan"):
            S.mirror_plan(ind)                                                                      # not planned for both strands: no mirror
        for it in items:
            pcs = S.item_pieces(it, L_PLAN, F)[0]
            plain, both = S.item_sources(pcs, L_PLAN, F), S.item_sources(pcs, L_PLAN, F, both_strands=True)
            assert plain == S.item_sources(pcs, L_PLAN, F, S.MARGIN_BP, False)
            assert _take_spans(both[0]) <= _take_spans(plain[0])
            assert [g for g in both[0] if g[2] < 0] == [g for g in plain[0] if g[2] < 0]              # reference sources are the same
            fewer += len(_take_spans(plain[0])) - len(_take_spans(both[0]))
            for a, cnt, ph, src in both[0]:                                                         # the cone inside the run of both entries
                if ph >= 0:
                    x0, x1 = 80 * src + ph - S.MARGIN_BP, 80 * src + ph + 400 * cnt + S.MARGIN_BP
                    pm = (C - ph) % 80
                    assert ph <= x0 and x1 <= ph + 80 * S.entry_rows(C, ph)
                    assert pm <= C - x1 and C - x0 <= pm + 80 * S.entry_rows(C, pm)
        assert S.mirror_phases(S.mirror_phases(ind.phases, C), C) == ind.phases
    assert fewer > 0                                                                                # the rule has teeth
    pcs = S.item_pieces(items[-1], L_PLAN, 0)[0]
    assert S.item_sources(pcs, L_PLAN, 0)[0][0][:2] == (5, 110) and S.item_sources(pcs, L_PLAN, 0, both_strands=True)[0][0][:2] == (6, 109)


@pytest.mark.parametrize("F", [0, 8_000, 4_037])
def test_indel_mirror_plan_against_oracle_stages(F):
    """The '-' strand of a batch with ``del`` / ``ins`` items (the item list of tests/test_screen_indel_cpu.py: deletions, insertions, sets, items
    next to both window ends, a deletion refilled past the flank), fp64 at gain 1.6.  The '-' reference rows, the oracle front on the reverse
    complement of every planned run read by the mirrored ranges, and the pooled rows of the oracle's '-' phase entries (its stage 4 on the
    reverse-complemented context from the phase on), put together by the mirrored gather segments, give ALL n5 rows of
    revcomp(apply_edit(codes, item, flank)) to 1e-10 of the scale.  F = 4 037: a context that is no multiple of 80, where the two strands'
    entries end at different places."""
    sd = encoder_sd(0, 1.6)
    codes, flank = _window(), plan_flank(F)
    context = np.concatenate([codes, flank])
    C, n5 = context.size, L_PLAN // 400
    named = indel_items(L_PLAN, codes, F)
    named["ins177_at_start"] = S.Edit("ins", 0, np.random.RandomState(5).randint(0, 4, 177).astype(np.uint8))      # where the both-strands rule bites
    items = list(named.values())
    wins = np.stack([codes] + [S.apply_edit(codes, e, flank) for e in items])
    rows = pool5(np.moveaxis(stages(sd, np.stack([revcomp(w) for w in wins]), 4)[4], 0, 1))         # [n5, B, 128], '-' row order
    ref, alt = rows[:, 0], rows[:, 1:]
    assert rows.shape[0] == n5
    scale = max(1.0, float(np.abs(alt).max()))
    entries = {}
    near_start = near_end = False
    for run_max in ((S.RUN_MAX_BP, 20_000) if F == 8_000 else (S.RUN_MAX_BP,)):
        plan = S.plan_batch(items, L_PLAN, run_max=run_max, flank=F, both_strands=True)
        mir = S.mirror_plan(plan)
        assert plan.indel and plan.both_strands and mir.reverse and mir.phases == S.mirror_phases(plan.phases, C)
        back = S.mirror_plan(mir)
        _tables_equal(back, plan)
        assert mir.entry_rows == [S.entry_rows(C, ph) for ph in mir.phases] and mir.take_rows == plan.take_rows > 0
        for ph in mir.phases:                                                  # the '-' cache: stage 4 on the reverse-complemented context
            if ph not in entries:
                entries[ph] = stages(sd, revcomp(context)[ph: ph + 80 * S.entry_rows(C, ph)], 4)[4]
                assert entries[ph].shape[0] == S.entry_rows(C, ph)
        buf = restate_buffer(plan, context)                                    # one buffer, in alt coordinates, for both strands
        fresh = np.full((mir.n_fresh, 128), np.nan)
        for o0, nb, ranges in mir.runs:
            run_rows = pool5(stages(sd, revcomp(buf[o0: o0 + nb]), 4)[4])
            for skip, count, dst in ranges:
                assert np.isnan(fresh[dst: dst + count]).all()
                fresh[dst: dst + count] = run_rows[skip: skip + count]
        assert not np.isnan(fresh).any()
        takes = 0
        for i, (name, item) in enumerate(named.items()):
            seg = mir.gather_segments[mir.gather_off[i]: mir.gather_off[i + 1]]
            assert np.all(seg[1:, 0] >= seg[:-1, 0] + seg[:-1, 1]) and np.all(seg[:, 1] > 0)      # sorted by row_lo, disjoint: what the kernel searches
            img = ref.copy()                                                                       # rows in no segment: the '-' reference at their own index
            for r0, cnt, source, src in seg:
                if source == engine.SCREEN_SRC_FRESH:
                    img[r0: r0 + cnt] = fresh[src: src + cnt]
                elif source == engine.SCREEN_SRC_REF:
                    assert 0 <= src and src + cnt <= n5
                    img[r0: r0 + cnt] = ref[src: src + cnt]
                else:
                    e = entries[mir.phases[source]]
                    assert 0 <= src and src + 5 * cnt <= e.shape[0]
                    img[r0: r0 + cnt] = pool5(e[src: src + 5 * cnt])
                    takes += cnt
                    x0, x1 = 80 * src + mir.phases[source] - S.MARGIN_BP, 80 * src + mir.phases[source] + 400 * cnt + S.MARGIN_BP
                    near_start |= x0 - mir.phases[source] < 480                                    # a take whose cone reaches the start of the '-' entry's run
                    near_end |= mir.phases[source] + 80 * e.shape[0] - x1 < 480                    # ... and one that reaches its end (within a row + a stage-4 row)
            err = np.abs(img - alt[:, i]).max() / scale
            assert err <= 1e-10, (F, name, err, np.nonzero(np.abs(img - alt[:, i]).max(axis=1) / scale > 1e-10)[0][:8])
            if not S.changes_length(item):                                                         # a length-preserving item plans as it does alone
                assert sorted((int(n5 - a - c), int(n5 - a)) for a, c, _, _ in seg) == S.set_clusters(item, L_PLAN) and np.all(seg[:, 2] == engine.SCREEN_SRC_FRESH)
        assert takes == mir.take_rows
    assert near_start and near_end


def test_merge_strands_host_against_a_direct_loop():
    rs = np.random.RandomState(7)
    n, E = 5, 3
    plus, minus = rs.randn(E, n, n).astype(np.float32), rs.randn(E, n, n).astype(np.float32)
    rp, rm = rs.randn(n, n).astype(np.float32), rs.randn(n, n).astype(np.float32)
    merged, gap = S.merge_strands_host(plus, minus, rp, rm)
    for e in range(E):
        tot = 0.0
        for i in range(n):
            for j in range(n):
                assert merged[e, i, j] == 0.5 * float(plus[e, i, j]) + 0.5 * float(minus[e, n - 1 - i, n - 1 - j])
                tot += abs((float(plus[e, i, j]) - float(rp[i, j])) - (float(minus[e, n - 1 - i, n - 1 - j]) - float(rm[n - 1 - i, n - 1 - j])))
        assert gap[e] == pytest.approx(tot / (n * n), rel=1e-12, abs=0)
    m2, g2 = S.merge_strands_host(plus[0], minus[0])
    assert g2 is None and np.array_equal(m2, merged[0])
    # the centre element of an odd map pairs with itself; equal strands with mirrored maps merge to the '+' map and have no gap
    m3, g3 = S.merge_strands_host(plus, plus[:, ::-1, ::-1], rp, rp[::-1, ::-1])
    assert np.array_equal(m3, plus.astype(np.float64)) and np.all(g3 == 0)


def test_strands_validation():
    from orca_amd import orca_modules as pm
    net = pm.Net(num_1d=4).eval()
    win = torch.zeros(40_000, dtype=torch.uint8)
    for bad in ("x", "-", "", None, True):
        with pytest.raises(ValueError, match="strands"):
            S.screen_1m(net, win, [S.Edit("mask", 0, 10)], strands=bad)
    for ok in ("+", "both"):                                                   # a CPU window is still an error, never a CPU computation
        with pytest.raises(OrcaHipError):
            S.screen_1m(net, win, [S.Edit("mask", 0, 10)], strands=ok)
