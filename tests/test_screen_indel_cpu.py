"""Insertions and deletions in the 1 Mb mutagenesis screen without a GPU: validation of the new edit kinds, `indel`, `apply_edit` with a flank, the
row-source plan against the fp64 oracle's Encoder stages (the 80 phase entries from the oracle's stage 4 on the phase-shifted context, the
oracle front on every planned run, every row of every item filled from its segments), the shape of the plan, and no silent CPU path."""
import functools

import numpy as np
import pytest
import torch

from orca_amd import engine
from orca_amd import screen as S
from orca_amd._lib import OrcaHipError
from tests.encoder_ref import encoder_sd, pool5, stages
from tests.test_screen_sets_cpu import plan_window, snv

L_PLAN, F_PLAN = 48_000, 4_000


def plan_flank(F=F_PLAN):
    f = np.random.RandomState(12).randint(0, 4, F).astype(np.uint8)
    f[F // 2: F // 2 + 30] = 4
    return f


def indel_items(L, codes, F=F_PLAN):
    """The item list of the plan tests (CPU oracle and GPU): name -> item.  Rows are 400 bases, the margin is 1 760, the pad 2 400; positions are
    given for L = 48 000 and scale with L."""
    u = L // 48_000
    ref4 = codes[33_000 * u: 33_000 * u + 4]
    return {
        "del1": S.Edit("del", 20_000 * u, 1),
        "ins1": S.Edit("ins", 24_001 * u, "G"),
        "del400": S.Edit("del", 20_000 * u, 400),                                               # 400 | s: reference rows one index further on
        "del80": S.Edit("del", 20_000 * u, 80),                                                 # 80 | s: phase entry 0
        "del37": S.Edit("del", 20_011 * u, 37),
        "ins_near_start": S.Edit("ins", 700, "ACGTT"),
        "del_near_start": S.Edit("del", 1_000, 12),
        "ins_at_start": S.Edit("ins", 0, "TTGAC"),
        "del_near_end": S.Edit("del", L - 900, 30),
        "ins_near_end": S.Edit("ins", L - 1_200, "TTG"),
        "del_past_flank": S.Edit("del", 30_000 * u, F + 1_000),                                 # refilled from the flank, then N
        "balanced": S.EditSet([S.Edit("del", 12_000 * u, 3), S.Edit("ins", 12_000 * u + 10_000, "CAT")]),
        "mixed": S.EditSet([snv(codes, 9_000 * u), S.Edit("inv", 12_345 * u, 900), S.Edit("del", 13_245 * u, 17), S.Edit("ins", 15_000 * u, "ACGTNACGT"),
                            S.Edit("mask", 30_000 * u, 50), S.Edit("ins", 30_050 * u, [3, 3])]),
        "vcf": S.indel(codes, 33_000 * u, ref4, "".join("ACGTN"[k] for k in ref4[:2]) + "TTGACCA"),
        "bare_snv": snv(codes, 31_999 * u),                                                     # length-preserving items ride along
        "set_inv": S.EditSet([S.Edit("inv", 39_000 * u, 800), snv(codes, 5_000 * u, 2)]),
    }


# ---- validation ---------------------------------------------------------------------------------------------------------------------------------
def test_new_kinds_validation():
    d, i = S.Edit("del", 5, 3), S.Edit("ins", 5, "ACN")
    assert (d.pos, d.length, d.end, d.removed, d.inserted, d.seq) == (5, 3, 8, 3, 0, None)
    assert (i.pos, i.length, i.end, i.removed, i.inserted) == (5, 0, 5, 0, 3) and i.seq.tolist() == [0, 1, 4] and i.seq.dtype == np.uint8
    assert S.Edit("ins", 5, [0, 1, 4]).seq.tolist() == [0, 1, 4] and S.Edit("ins", 5, 3, "ACN").inserted == 3
    assert "ins" in repr(i) and "ACN" in repr(i) and "del" in repr(d)
    for bad in (lambda: S.Edit("del", 5, 0), lambda: S.Edit("del", -1, 3), lambda: S.Edit("del", 5, 3, "ACG"), lambda: S.Edit("del", 0, 3),
                lambda: S.Edit("ins", 5, ""), lambda: S.Edit("ins", -1, "A"), lambda: S.Edit("ins", 5, "AXG"), lambda: S.Edit("ins", 5, [7]),
                lambda: S.Edit("ins", 5, 2, "ACG"), lambda: S.Edit("dup", 5, 3)):
        with pytest.raises(ValueError):
            bad()
    d.check(8)
    with pytest.raises(ValueError):
        d.check(7)
    S.Edit("ins", 8, "A").check(8)                                    # 0 <= pos <= L
    S.Edit("ins", 0, "A").check(8)
    with pytest.raises(ValueError):
        S.Edit("ins", 9, "A").check(8)
    assert S.changes_length(d) and S.changes_length(i) and not S.changes_length(S.Edit("mask", 0, 3))
    assert S.shift_of(d) == 3 and S.shift_of(i) == -3 and S.shift_of(S.EditSet([d, S.Edit("ins", 20, "ACGTA")])) == -2


def test_editset_membership():
    span, inv = S.Edit("mask", 10, 5), S.Edit("inv", 20, 5)
    s = S.EditSet([inv, S.Edit("ins", 20, "AC"), S.Edit("del", 15, 5), span, S.Edit("ins", 10, "T"), S.Edit("ins", 25, "G")])
    assert [(e.kind, e.pos) for e in s] == [("ins", 10), ("mask", 10), ("del", 15), ("ins", 20), ("inv", 20), ("ins", 25)]     # an ins before a span at its pos
    assert (s.pos, s.end) == (10, 25) and S.changes_length(s) and S.shift_of(s) == 5 - 4
    S.EditSet([S.Edit("ins", 7, "A")])
    for bad in ([span, S.Edit("ins", 12, "A")],                      # an ins strictly inside a span
                [S.Edit("del", 10, 5), S.Edit("ins", 14, "A")],
                [S.Edit("ins", 12, "A"), S.Edit("ins", 12, "C")],    # two ins at one pos
                [S.Edit("del", 10, 5), S.Edit("mask", 14, 2)],       # spans overlap
                [S.Edit("del", 10, 5), S.Edit("del", 12, 1)]):
        with pytest.raises(ValueError):
            S.EditSet(bad)
    with pytest.raises(ValueError):
        s.check(24)
    s.check(25)
    with pytest.raises(ValueError):
        S.plan_batch([S.Edit("del", 7_990, 20)], 8_000)
    with pytest.raises(ValueError):
        S.plan_batch([S.Edit("del", 10, 20)], 8_000, flank=8_001)


def test_indel_helper():
    c = np.array([0, 1, 2, 3, 3, 0, 1, 4, 2, 2], dtype=np.uint8)           # ACGTTACNGG
    e = S.indel(c, 2, "GTT", "G")                                           # VCF deletion with its anchor base
    assert (e.kind, e.pos, e.length) == ("del", 3, 2)
    e = S.indel(c, 2, "G", "GAC")                                           # insertion behind the anchor
    assert (e.kind, e.pos, e.seq.tolist()) == ("ins", 3, [0, 1])
    e = S.indel(c, 3, "TTA", "TGA")                                         # prefix and suffix trimmed: an SNV
    assert (e.kind, e.pos, e.length, e.seq.tolist()) == ("sub", 4, 1, [2])
    e = S.indel(c, 1, "CGTT", "CAAT")                                       # equal lengths: one sub
    assert (e.kind, e.pos, e.length, e.seq.tolist()) == ("sub", 2, 2, [0, 0])
    e = S.indel(c, 5, "ACN", "GG", name="v")                                # a sub plus a del
    assert isinstance(e, S.EditSet) and e.name == "v" and [(m.kind, m.pos, m.length) for m in e] == [("sub", 5, 2), ("del", 7, 1)] and e[0].seq.tolist() == [2, 2]
    e = S.indel(c, 0, "A", "TCC")                                           # a sub plus an ins
    assert [(m.kind, m.pos) for m in e] == [("sub", 0), ("ins", 1)] and e[0].seq.tolist() == [3] and e[1].seq.tolist() == [1, 1]
    e = S.indel(c, 4, "", "AC")                                             # an empty ref: a plain insertion in front of pos
    assert (e.kind, e.pos, e.seq.tolist()) == ("ins", 4, [0, 1])
    e = S.indel(torch.from_numpy(c), 3, [3, 3], [3])                        # codes, a tensor window; TT -> T
    assert (e.kind, e.pos, e.length) == ("del", 4, 1)
    assert np.array_equal(S.apply_edit(c, S.indel(c, 5, "ACN", "GG")), [0, 1, 2, 3, 3, 2, 2, 2, 2, 4])
    for bad in (lambda: S.indel(c, 2, "CTT", "G"), lambda: S.indel(c, 8, "GGA", "G"), lambda: S.indel(c, 2, "GT", "GT"), lambda: S.indel(c, -1, "A", "C"),
                lambda: S.indel(c, 2, "GX", "G")):
        with pytest.raises(ValueError):
            bad()


def test_apply_edit_with_and_without_flank():
    rs = np.random.RandomState(3)
    c = rs.randint(0, 4, 400).astype(np.uint8)
    c[100:110] = 4
    fl = rs.randint(0, 4, 25).astype(np.uint8)
    cx = np.concatenate([c, fl, np.full(400, 4, np.uint8)])
    n = np.full(400, 4, np.uint8)
    d = S.Edit("del", 50, 30)
    assert np.array_equal(S.apply_edit(c, d, fl), np.concatenate([c[:50], c[80:], fl, n])[:400])            # refilled from the flank, then N
    assert np.array_equal(S.apply_edit(c, d), np.concatenate([c[:50], c[80:], n])[:400])                    # no flank: N
    assert np.array_equal(S.apply_edit(c, S.Edit("del", 50, 10), fl), np.concatenate([c[:50], c[60:], fl[:10]]))
    i = S.Edit("ins", 50, "ACGTN")
    want = np.concatenate([c[:50], [0, 1, 2, 3, 4], c[50:395]])
    assert np.array_equal(S.apply_edit(c, i, fl), want) and np.array_equal(S.apply_edit(c, i), want)       # the tail is pushed out
    assert np.array_equal(S.apply_edit(c, S.Edit("ins", 0, "TT")), np.concatenate([[3, 3], c[:398]]))
    assert np.array_equal(S.apply_edit(c, S.Edit("ins", 400, "TT"), fl), c)                                 # behind the last base: pushed out whole
    assert np.array_equal(S.apply_edit(c, S.Edit("ins", 399, "TT"), fl), np.concatenate([c[:399], [3]]))
    s = S.EditSet([S.Edit("inv", 95, 30), S.Edit("del", 130, 7), S.Edit("ins", 130, "GG"), S.Edit("sub", 200, 2, "NN"), S.Edit("mask", 390, 10), S.Edit("ins", 400, "A")])
    r = c[95:125][::-1]
    want = np.concatenate([c[:95], np.where(r < 4, 3 - r, r), c[125:130], [2, 2], c[137:200], [4, 4], c[202:390], np.full(10, 4), [0], fl])[:400]
    got = S.apply_edit(c, s, fl)
    assert got.dtype == np.uint8 and got.shape == (400,) and np.array_equal(got, want)
    for item in (d, i, s, S.Edit("del", 1, 399)):
        for f in (None, fl, fl[:0], torch.from_numpy(fl)):
            assert S.apply_edit(c, item, f).shape == (400,)
    assert np.array_equal(S.apply_edit(c, S.Edit("del", 1, 399), fl), cx[np.r_[0, 400:799]])
    # length-preserving items: the flank changes nothing
    for item in (S.Edit("inv", 95, 30), S.EditSet([S.Edit("mask", 0, 7), S.Edit("sub", 396, 4, "ACGT")])):
        assert np.array_equal(S.apply_edit(c, item, fl), S.apply_edit(c, item))
    for bad in (np.zeros(401, np.uint8), np.zeros((2, 3), np.uint8), np.array([5], np.uint8), np.zeros(3, np.float32)):
        with pytest.raises(ValueError):
            S.apply_edit(c, S.Edit("mask", 0, 3), bad)                                                      # validated all the same
        with pytest.raises(ValueError):
            S.apply_edit(c, d, bad)


# ---- the plan against the fp64 oracle -----------------------------------------------------------------------------------------------------------
def restate_buffer(plan, context, npay_check=True):
    """The packed codes buffer from the two device tables (orca_screen_assemble_codes restated): per snippet, per alt base, the piece that holds it."""
    tab, pcs = plan.snippet_table, plan.piece_table
    assert tab[0, 0] == 0 and np.all(tab[1:, 0] == tab[:-1, 0] + tab[:-1, 2])
    C = context.size
    buf = np.full(int(tab[-1, 0] + tab[-1, 2]), 4, dtype=np.uint8)
    for off, a0, nb, lo, cnt in tab[:, :5]:
        mine = pcs[lo: lo + cnt]
        assert np.all(mine[1:, 0] >= mine[:-1, 0] + mine[:-1, 3])                                  # sorted by dst, disjoint
        for dst, kind, src, ln in mine:
            t = np.arange(max(dst, a0), min(dst + ln, a0 + nb))                                    # the alt bases of this piece inside the snippet
            if kind == 0 or kind == 1:
                at = src + (t - dst) if kind == 0 else src + ln - 1 - (t - dst)
                v = np.where((at >= 0) & (at < C), context[np.clip(at, 0, C - 1)], 4)
                v = v if kind == 0 else np.where(v < 4, 3 - v, v)
            elif kind == 2:
                assert src >= 0 and src + ln <= plan.payload.size
                v = plan.payload[src + (t - dst)]
            else:
                assert kind == 3
                v = np.full(t.size, 4)
            buf[off + t - a0] = v
    return buf


def oracle_entries(sd, context):
    """All 80 phase entries: the oracle's stage 4 on context bases [phase, phase + 80 rows), entries of one length in one batch."""
    C = context.size
    by_len = {}
    for ph in range(80):
        by_len.setdefault(S.entry_rows(C, ph), []).append(ph)
    out = {}
    for n4, phs in by_len.items():
        got = stages(sd, np.stack([context[ph: ph + 80 * n4] for ph in phs]), 4)[4]
        assert got.shape[1] == n4
        for k, ph in enumerate(phs):
            out[ph] = got[k]
    return out


def test_entry_rows_is_the_cache_arithmetic():
    from orca_amd import sv
    for C in (52_000, 48_000, 208_000, 1_008_000, 1_000_037, 2_000):
        for ph in range(80):
            p16, k = ph % 16, ph // 16
            n3 = (C - p16) // 80 * 80 // sv.S3_GRID                                      # sv.Stage3Cache._planes3 / Stage4Cache._build_group, region (0, C)
            assert S.entry_rows(C, ph) == min((C - ph) // sv.S4_GRID, (n3 - k) // sv.S3_POOL), (C, ph)
            assert ph + 80 * S.entry_rows(C, ph) <= C


@functools.lru_cache(maxsize=None)
def oracle_case():
    """Computed once for both parametrisations (the plan's run packing does not enter): the oracle's rows of the reference and of every
    apply_edit window, and its 80 phase entries.  Read only."""
    sd = encoder_sd(0, 1.6)
    codes, flank = plan_window(), plan_flank()
    named = indel_items(L_PLAN, codes)
    wins = np.stack([codes] + [S.apply_edit(codes, e, flank) for e in named.values()])
    rows = pool5(np.moveaxis(stages(sd, wins, 4)[4], 0, 1))            # [n5, B, 128]
    return sd, codes, flank, named, wins, rows, oracle_entries(sd, np.concatenate([codes, flank]))


@pytest.mark.parametrize("run_max", [S.RUN_MAX_BP, 20_000])
def test_indel_plan_against_oracle_stages(run_max):
    """fp64, synthetic weights at gain 1.6: the reference rows, the oracle front on every planned run of the restated buffer, and the pooled
    rows of the oracle's phase entries, put together by the plan's segments, give ALL rows of apply_edit's window to 1e-10 of the scale."""
    sd, codes, flank, named, wins, rows, entries = oracle_case()
    context = np.concatenate([codes, flank])
    items = list(named.values())
    plan = S.plan_batch(items, L_PLAN, run_max=run_max, flank=F_PLAN)
    n5 = L_PLAN // 400
    assert plan.indel and plan.flank == F_PLAN and plan.edit_table is None and plan.splice_table is None and plan.span_table is None
    assert plan.gather_off.shape == (len(items) + 1,) and plan.gather_off[0] == 0 and plan.gather_off[-1] == len(plan.gather_segments)
    assert plan.shift.tolist() == [S.shift_of(e) for e in items]
    ref, alt = rows[:, 0], rows[:, 1:]
    assert rows.shape[0] == n5
    assert plan.entry_rows == [entries[ph].shape[0] for ph in plan.phases] and plan.phases == S.needed_phases(items, L_PLAN, F_PLAN)
    buf = restate_buffer(plan, context)
    for k, i in enumerate(plan.order):                                  # the buffer is apply_edit's window, snippet by snippet
        off, a0, nb = (int(v) for v in plan.snippet_table[k, :3])
        assert (a0, nb) == tuple(plan.snippet[i])
        assert np.array_equal(buf[off: off + nb], wins[1 + plan.item_of[i]][a0: a0 + nb]), (k, items[plan.item_of[i]])
    fresh = np.full((plan.n_fresh, 128), np.nan)
    for o0, nb, ranges in plan.runs:
        assert nb <= run_max or len(ranges) == 1
        run_rows = pool5(stages(sd, buf[o0: o0 + nb], 4)[4])
        for skip, count, dst in ranges:
            fresh[dst: dst + count] = run_rows[skip: skip + count]
    assert not np.isnan(fresh).any()
    scale = max(1.0, float(np.abs(alt).max()))
    takes = 0
    for i, (name, item) in enumerate(named.items()):
        seg = plan.gather_segments[plan.gather_off[i]: plan.gather_off[i + 1]]
        assert np.all(seg[1:, 0] >= seg[:-1, 0] + seg[:-1, 1]) and np.all(seg[:, 1] > 0)          # sorted by row_lo, disjoint
        img = ref.copy()                                                                           # rows in no segment: ref at their own index
        for r0, cnt, source, src in seg:
            if source == engine.SCREEN_SRC_FRESH:
                img[r0: r0 + cnt] = fresh[src: src + cnt]
            elif source == engine.SCREEN_SRC_REF:
                img[r0: r0 + cnt] = ref[src: src + cnt]
            else:
                e = entries[plan.phases[source]]
                assert 0 <= src and src + 5 * cnt <= e.shape[0]
                img[r0: r0 + cnt] = pool5(e[src: src + 5 * cnt])
                takes += cnt
        err = np.abs(img - alt[:, i]).max() / scale
        assert err <= 1e-10, (name, err, np.nonzero(np.abs(img - alt[:, i]).max(axis=1) / scale > 1e-10)[0][:8])
        if not S.changes_length(item):                                                             # ... and plans as it does alone
            assert [(int(a), int(a + c)) for a, c, s_, _ in seg] == S.set_clusters(item, L_PLAN) and np.all(seg[:, 2] == engine.SCREEN_SRC_FRESH)
    assert takes == plan.take_rows > 0
    src_of = {n: plan.gather_segments[plan.gather_off[i]: plan.gather_off[i + 1]] for i, n in enumerate(named)}
    assert (src_of["del400"][:, 2] == engine.SCREEN_SRC_REF).any() and (src_of["del80"][:, 2] >= 0).any()
    assert [plan.phases[s_] for s_ in src_of["del80"][:, 2] if s_ >= 0] == [0] and [plan.phases[s_] for s_ in src_of["del37"][:, 2] if s_ >= 0] == [37]
    # the balanced set: behind its second member the rows are the reference's own, and there is no end snippet
    bal = src_of["balanced"]
    assert bal[-1, 0] + bal[-1, 1] <= (22_000 + 1_760) // 400 + 1 and (bal[:, 2] == engine.SCREEN_SRC_FRESH).sum() == 2
    assert S.apply_edit(codes, named["del_past_flank"], flank)[-1_000:].tolist() == [4] * 1_000


def test_plan_shape():
    """Deterministic on the host: an isolated indel further than 6 kb from both window ends has exactly two fresh segments, its junction and the
    window's right end; every other row is a ref copy (in no segment, or source -2) or a take."""
    L, F = 200_000, 8_000
    n5 = L // 400
    for item in (S.Edit("del", 6_001, 1), S.Edit("ins", L - 6_001, "ACGT"), S.Edit("del", 100_000, 37), S.Edit("ins", 77_777, "A" * 50), S.Edit("del", 50_000, 800),
                 S.indel(np.zeros(L, np.uint8), 120_000, "AAAA", "AC")):
        p = S.plan_batch([item], L, flank=F)
        g = p.gather_segments
        fresh = g[g[:, 2] == engine.SCREEN_SRC_FRESH]
        assert len(fresh) == 2 == len(p.segments) and fresh[1, 0] + fresh[1, 1] == n5, item
        pos = S.members_of(item)[0].pos
        assert fresh[0, 0] * 400 <= pos < (fresh[0, 0] + fresh[0, 1]) * 400 and fresh[0, 1] <= 11 and fresh[1, 1] <= 6, item
        between = g[(g[:, 2] != engine.SCREEN_SRC_FRESH)]
        assert between[:, 1].sum() == n5 - fresh[0, 0] - fresh[:, 1].sum()                     # everything behind the junction: ref copies and takes
        assert fresh[0, 0] + fresh[0, 1] == between[0, 0] and between[-1, 0] + between[-1, 1] == fresh[1, 0]
        assert p.take_rows == between[between[:, 2] >= 0][:, 1].sum() and len(p.runs) == 1
    # no flank: the same shape, more of the end is N
    assert len(S.plan_batch([S.Edit("del", 100_000, 37)], L).segments) == 2


def test_plan_of_an_insertion_behind_the_last_base_is_empty():
    """``Edit("ins", L, seq)`` leaves the alt window as it is: every row is the reference's own, and the batch has no snippet, run or segment."""
    L = 48_000
    for items in ([S.Edit("ins", L, "AC")], [S.Edit("ins", L, "AC"), S.indel(np.zeros(L, np.uint8), L - 1, "A", "AT")]):
        p = S.plan_batch(items, L, flank=F_PLAN)
        assert p.indel and p.snippet_table.shape == (0, 8) and p.n_fresh == 0 and p.runs == [] and p.order == [] and p.phases == []
        assert p.gather_segments.shape == (0, 4) and p.gather_off.tolist() == [0] * (len(items) + 1) and p.segments.shape == (0, 3)
        assert p.shift.tolist() == [-2, -1][:len(items)] and p.piece_table[:, 1:].tolist() == [[0, 0, L]] * len(items)


def test_plan_without_length_changes_is_what_it_was():
    """A list without del / ins goes down the unchanged code path (tests/test_screen_sets_cpu.py pins that path's fields); the general planner,
    made to plan the same list, gives the same snippets, rows, runs and fresh rows - which is why a length-preserving item in a batch with
    indels is computed from the very bases and front runs it is computed from alone."""
    from tests.test_screen_sets_cpu import plan_items
    codes = plan_window()
    items = list(plan_items(L_PLAN, codes).values())
    for flank in (0, F_PLAN):
        p = S.plan_batch(items, L_PLAN, flank=flank)
        assert not p.indel and p.piece_table is None and p.gather_segments is None and p.phases is None and p.take_rows == 0 and p.span_table is not None
    q = S._plan_indels(items, L_PLAN, F_PLAN, S.PAD_BP, S.MARGIN_BP, S.MIN_SNIPPET_BP, S.RUN_MAX_BP)
    for name in ("snippet", "rows", "fresh", "item_of", "payload", "segments", "seg_off"):
        assert np.array_equal(getattr(p, name), getattr(q, name)), name
    assert (p.L, p.order, p.runs, p.n_fresh) == (q.L, q.order, q.runs, q.n_fresh) and q.phases == [] and q.take_rows == 0
    assert np.array_equal(p.snippet_table[:, :3], q.snippet_table[:, :3])
    assert q.gather_segments[:, [0, 1, 3]].tolist() == p.segments.tolist() and np.all(q.gather_segments[:, 2] == engine.SCREEN_SRC_FRESH)
    buf = restate_buffer(q, np.concatenate([codes, plan_flank()]))
    want = np.concatenate([S.apply_edit(codes, items[p.item_of[i]])[p.snippet[i, 0]: p.snippet[i, 0] + p.snippet[i, 1]] for i in p.order])
    assert np.array_equal(buf, want)
    bare = [S.Edit("sub", 20_011, 2, "AC"), S.Edit("mask", L_PLAN - 300, 300)]
    assert S.plan_batch(bare, L_PLAN, flank=F_PLAN).edit_table is not None


def test_whole_window_piece_tables():
    codes, flank = plan_window(), plan_flank()
    items = list(indel_items(L_PLAN, codes).values())
    table, pieces, payload = S.whole_window_piece_tables(items, L_PLAN, F_PLAN)
    assert table[:, :3].tolist() == [[i * L_PLAN, 0, L_PLAN] for i in range(len(items))] and table[-1, 3] + table[-1, 4] == len(pieces)

    class P:
        pass
    P.snippet_table, P.piece_table, P.payload = table, pieces, payload
    buf = restate_buffer(P, np.concatenate([codes, flank]))
    assert np.array_equal(buf.reshape(len(items), L_PLAN), np.stack([S.apply_edit(codes, e, flank) for e in items]))
    for lo, cnt in table[:, 3:5]:
        mine = pieces[lo: lo + cnt]
        assert mine[0, 0] == 0 and np.all(mine[1:, 0] == mine[:-1, 0] + mine[:-1, 3]) and mine[-1, 0] + mine[-1, 3] == L_PLAN        # the pieces tile [0, L)


# ---- no silent CPU path -------------------------------------------------------------------------------------------------------------------------
def test_no_silent_cpu_path():
    from orca_amd import orca_modules as pm
    net = pm.Net(num_1d=4).eval()
    with pytest.raises(OrcaHipError):
        S.screen_1m(net, torch.zeros(40_000, dtype=torch.uint8), [S.Edit("del", 100, 10)], flank=torch.zeros(100, dtype=torch.uint8))
    u8, f32 = torch.zeros(400, dtype=torch.uint8), torch.zeros((10, 128))
    with pytest.raises(OrcaHipError):
        engine.screen_assemble_codes(None, u8, np.array([[0, 0, 400, 0, 1, 0, 0, 0]]), np.array([[0, 0, 0, 400]]), None, torch.zeros(400, dtype=torch.uint8))
    with pytest.raises(OrcaHipError):
        engine.screen_gather_rows(None, f32, f32, [torch.zeros((50, 128))], np.array([[0, 1, 0, 0]]), np.array([0, 1]), torch.zeros((1, 10, 128)))
