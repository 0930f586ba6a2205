"""Compound edits (screen.EditSet) and region scores of the 1 Mb mutagenesis screen without a GPU: validation, the generators, apply_edit on a
set, the cluster plan against the fp64 oracle's Encoder stages (the oracle front on every planned snippet, then the splice, gives the rows of
the fully edited window), the plan of bare edits restated from the documented rules, the region score formulas, and no silent CPU path."""
import itertools

import numpy as np
import pytest
import torch

from orca_amd import engine
from orca_amd import screen as S
from orca_amd._lib import OrcaHipError
from tests.encoder_ref import encoder_sd, pool5, stages

L_PLAN = 48_000


def snv(codes, p, k=1):
    return S.Edit("sub", p, 1, [(int(codes[p]) + k) % 4 if codes[p] < 4 else k % 4])


def plan_window(L=L_PLAN):
    rs = np.random.RandomState(11)
    codes = rs.randint(0, 4, L).astype(np.uint8)
    codes[20_000:20_040] = 4
    codes[12_500:12_620] = 4
    return codes


def plan_items(L, codes, n_snv=60, seed=7):
    """The mixed list of the plan tests (CPU oracle and GPU): name -> item.  Rows are 400 bases, the margin is 1 760, the pad 2 400."""
    rs = np.random.RandomState(seed)
    h = n_snv // 2                                          # two clumps, so the set keeps more than one cluster
    many = np.sort(np.concatenate([L // 50 + rs.choice(L // 5 - L // 50, h, replace=False), 3 * L // 5 + rs.choice(3 * L // 10, n_snv - h, replace=False)]))
    return {
        "one_row": S.EditSet([snv(codes, 20_011), snv(codes, 20_150, 2)]),                        # both in row 50
        "touching": S.EditSet([snv(codes, 10_000), snv(codes, 13_800)]),                         # rows [20, 30) and [30, 39)
        "far_apart": S.EditSet([snv(codes, 5_000), S.Edit("mask", L - 8_000, 300)]),              # two segments
        "both_ends": S.EditSet([snv(codes, L - 1), snv(codes, 0)]),
        "pad_zone": S.EditSet([snv(codes, 10_000), snv(codes, 14_200, 3)]),                      # 14 200: in the first snippet's pad, past its margin
        "inv_next_to_sub": S.EditSet([S.Edit("inv", 12_345, 900), S.Edit("sub", 13_245, 3, "NAC"), S.Edit("mask", 30_000, 50)]),
        "snvs": S.EditSet([snv(codes, int(p), 1 + int(p) % 3) for p in many], name="haplotype"),
        "bare_inv": S.Edit("inv", 39_000, 800),
        "bare_snv": snv(codes, 31_999),
        "single": S.EditSet([S.Edit("mask", 25_000, 120)]),
    }


# ---- EditSet ----------------------------------------------------------------------------------------------------------------------------------
def test_editset_validation():
    a, b, c = S.Edit("mask", 10, 5), S.Edit("inv", 15, 5), S.Edit("sub", 12, 2, "AC")
    s = S.EditSet([b, a], name="x")
    assert [e.pos for e in s] == [10, 15] and len(s) == 2 and s[0] is a and s.name == "x"          # touching but disjoint: allowed, sorted by pos
    assert (s.pos, s.end) == (10, 20)
    with pytest.raises(ValueError) as ei:
        S.EditSet([a, c])
    assert repr(a) in str(ei.value) and repr(c) in str(ei.value)                                  # the message names both members
    with pytest.raises(ValueError):
        S.EditSet([a, a])
    with pytest.raises(ValueError):
        S.EditSet([])
    with pytest.raises(TypeError):
        S.EditSet([a, ("mask", 30, 2)])
    with pytest.raises(TypeError):
        S.EditSet([s])                                                                            # sets do not nest
    with pytest.raises(AttributeError):
        s.edits = ()
    s.check(20)
    with pytest.raises(ValueError):
        s.check(19)                                                                               # a member leaves the window
    with pytest.raises(ValueError):
        S.apply_edit(np.zeros(19, np.uint8), s)
    with pytest.raises(ValueError):
        S.plan_batch([S.EditSet([S.Edit("mask", 0, 4), S.Edit("mask", 7_990, 20)])], 8_000)


def test_snv_set():
    codes = np.array([0, 1, 2, 3, 4, 0, 1], dtype=np.uint8)
    s = S.snv_set(codes, [(5, "A", "T"), (1, "c", "G"), (4, "N", 2)], name="h")
    assert [(e.kind, e.pos, e.length, int(e.seq[0])) for e in s] == [("sub", 1, 1, 2), ("sub", 4, 1, 2), ("sub", 5, 1, 3)] and s.name == "h"
    assert np.array_equal(S.apply_edit(codes, s), [0, 2, 2, 3, 2, 3, 1])
    assert len(S.snv_set(torch.from_numpy(codes), [(0, 0, 1)])) == 1
    with pytest.raises(ValueError):
        S.snv_set(codes, [(1, "A", "G")])                     # ref disagrees with the window
    with pytest.raises(ValueError):
        S.snv_set(codes, [(1, "C", "G"), (1, "C", "T")])      # two variants at one position
    with pytest.raises(ValueError):
        S.snv_set(codes, [(7, "A", "G")])                     # outside the window
    with pytest.raises(ValueError):
        S.snv_set(codes, [])


def test_pair_edits():
    a = [S.Edit("mask", 0, 100), S.Edit("mask", 100, 100), S.Edit("mask", 250, 100)]
    b = [S.Edit("inv", 50, 100), S.Edit("mask", 350, 10), S.Edit("mask", 200, 50)]
    sets, index = S.pair_edits(a, b)
    want = [(i, j) for i in range(3) for j in range(3) if a[i].end <= b[j].pos or b[j].end <= a[i].pos]
    assert index == want and (0, 0) not in index and (1, 0) not in index and (2, 2) in index and len(index) == 7
    for s, (i, j) in zip(sets, index):
        assert isinstance(s, S.EditSet) and {id(e) for e in s} == {id(a[i]), id(b[j])}
    assert S.pair_edits([], b) == ([], [])


def test_apply_edit_on_a_set_is_the_members_in_any_order():
    rs = np.random.RandomState(3)
    codes = rs.randint(0, 4, 400).astype(np.uint8)
    codes[100:110] = 4
    members = [S.Edit("inv", 95, 30), S.Edit("sub", 125, 4, "ACGN"), S.Edit("sub", 91, 4, [3, 3, 4, 0]), S.Edit("mask", 0, 7), S.Edit("inv", 399, 1),
               S.Edit("inv", 200, 100)]
    want = S.apply_edit(codes, S.EditSet(members))
    for perm in itertools.permutations(range(len(members)), len(members)):
        if perm[0] > 1:
            continue                                                       # 240 of the 720 orders are plenty
        c = codes
        for k in perm:
            c = S.apply_edit(c, members[k])                              # disjoint members: one after another is the same window
        assert np.array_equal(c, want), perm
        assert np.array_equal(S.apply_edit(codes, S.EditSet([members[k] for k in perm])), want)
    assert np.array_equal(S.apply_edit(codes, S.EditSet(members[:1])), S.apply_edit(codes, members[0]))
    # the inversion read the unedited window: its neighbours' payloads are not mirrored into it
    assert np.array_equal(want[95:125], S.apply_edit(codes, members[0])[95:125]) and want[125:129].tolist() == [0, 1, 2, 4]


# ---- the plan against the fp64 oracle -----------------------------------------------------------------------------------------------------------
def test_clusters_of_the_plan_items():
    codes = plan_window()
    it = plan_items(L_PLAN, codes)
    rows = {k: [S.edit_rows(e, L_PLAN) for e in S.members_of(v)] for k, v in it.items()}
    assert rows["one_row"][0] == rows["one_row"][1] and 20_011 // 400 == 20_150 // 400
    assert rows["touching"] == [(20, 30), (30, 39)] and S.set_clusters(it["touching"], L_PLAN) == [(20, 39)]
    assert S.set_clusters(it["far_apart"], L_PLAN) == [(8, 17), (95, 106)]
    assert S.set_clusters(it["both_ends"], L_PLAN) == [(0, 5), (115, 120)]
    # 14 200 lies inside the snippet of rows [20, 30) (its pad reaches 14 400) but past that cluster's margin: a cluster of its own
    assert S.set_clusters(it["pad_zone"], L_PLAN) == [(20, 30), (31, 40)] and S.edit_snippet(20, 30, L_PLAN) == (5_600, 14_400)
    assert len(it["snvs"]) == 60 and len(S.set_clusters(it["snvs"], L_PLAN)) == 2
    assert S.set_clusters(it["bare_snv"], L_PLAN) == [S.edit_rows(it["bare_snv"], L_PLAN)]


@pytest.mark.parametrize("run_max", [S.RUN_MAX_BP, 20_000])
def test_set_plan_against_oracle_stages(run_max):
    """fp64, synthetic weights at gain 1.6: the oracle front on every planned run (the packed snippets with every span that meets them applied),
    spliced into the reference rows by the plan's segments, gives ALL rows of the fully edited window to 1e-10 - the rows between clusters
    included."""
    sd = encoder_sd(0, 1.6)
    codes = plan_window()
    items = list(plan_items(L_PLAN, codes).values())
    plan = S.plan_batch(items, L_PLAN, run_max=run_max)
    n5 = L_PLAN // 400
    S_ = len(plan.order)
    assert plan.edit_table is None and plan.splice_table is None
    assert plan.seg_off.shape == (len(items) + 1,) and plan.seg_off[0] == 0 and plan.seg_off[-1] == S_ == len(plan.segments) and S_ > len(items)
    assert np.all(np.diff(plan.seg_off) >= 1)
    wins = np.stack([codes] + [S.apply_edit(codes, e) for e in items])
    rows = pool5(np.moveaxis(stages(sd, wins, 4)[4], 0, 1))            # [n5, B, 128]
    ref, alt = rows[:, 0], rows[:, 1:]
    assert rows.shape[0] == n5
    # the packed buffer restated from the device tables: per snippet the window's bases with the snippet's span range applied
    tab, spans = plan.snippet_table, plan.span_table
    assert tab[0, 0] == 0 and np.all(tab[1:, 0] == tab[:-1, 0] + tab[:-1, 2])
    buf = np.zeros(int(tab[-1, 0] + tab[-1, 2]), dtype=np.uint8)
    for k, i in enumerate(plan.order):
        off, b0, nb, lo, cnt = (int(v) for v in tab[k, :5])
        assert (b0, nb) == tuple(plan.snippet[i])
        item = items[plan.item_of[i]]
        sp = spans[lo: lo + cnt]
        assert np.all(sp[1:, 1] >= sp[:-1, 1] + sp[:-1, 2])                                        # sorted by pos, disjoint
        meets = [e for e in S.members_of(item) if e.pos < b0 + nb and e.end > b0]
        assert [(int(a), int(b)) for a, b in sp[:, 1:3]] == [(e.pos, e.length) for e in meets]     # every member that meets the snippet, no other
        assert [int(a) for a in sp[:, 0]] == [engine.SCREEN_KINDS[e.kind] for e in meets]
        for (kind, pos, ln, po), e in zip(sp, meets):
            if e.kind == "sub":
                assert np.array_equal(plan.payload[po: po + ln], e.seq)
        buf[off: off + nb] = S.apply_edit(codes, item)[b0: b0 + nb]
    fresh = np.full((plan.n_fresh, 128), np.nan)
    for o0, nb, ranges in plan.runs:
        assert nb <= run_max or len(ranges) == 1
        run_rows = pool5(stages(sd, buf[o0: o0 + nb], 4)[4])
        for skip, count, dst in ranges:
            fresh[dst: dst + count] = run_rows[skip: skip + count]
    assert not np.isnan(fresh).any()
    scale = max(1.0, float(np.abs(alt).max()))
    for i, item in enumerate(items):
        seg = plan.segments[plan.seg_off[i]: plan.seg_off[i + 1]]
        assert [(int(a), int(a + c)) for a, c, _ in seg] == S.set_clusters(item, L_PLAN)
        img = ref.copy()
        for r0, cnt, src in seg:
            img[r0: r0 + cnt] = fresh[src: src + cnt]
        assert np.abs(img - alt[:, i]).max() / scale <= 1e-10, item
        changed = np.nonzero(np.abs(alt[:, i] - ref).max(axis=1) > 0)[0]
        assert changed.size and all(any(a <= r < a + c for a, c, _ in seg) for r in changed), item


def test_thousand_snv_set_plans():
    L = 1_000_000
    rs = np.random.RandomState(1)
    codes = rs.randint(0, 4, L).astype(np.uint8)
    pos = np.sort(rs.choice(L, 1_000, replace=False))
    s = S.snv_set(codes, [(int(p), int(codes[p]), (int(codes[p]) + 1) % 4) for p in pos])
    plan = S.plan_batch([s], L)
    assert len(plan.span_table) == 1_000 and plan.seg_off.tolist() == [0, len(plan.segments)]
    seg = plan.segments
    assert np.all(seg[1:, 0] > seg[:-1, 0] + seg[:-1, 1]) and seg[:, 1].sum() == plan.n_fresh          # sorted, apart, every fresh row used once
    covered = np.zeros(L // 400, dtype=bool)
    for r0, cnt, _ in seg:
        covered[r0: r0 + cnt] = True
    for p in pos:
        r0, r1 = S.edit_rows(S.Edit("mask", int(p), 1), L)
        assert covered[r0:r1].all()
    table, spans, payload = S.whole_window_set_tables([s, S.Edit("mask", 5, 10)], L)
    assert table[:, :5].tolist() == [[0, 0, L, 0, 1_000], [L, 0, L, 1_000, 1]] and len(spans) == 1_001 and payload.size == 1_000


def test_plan_of_bare_edits_is_what_it_was():
    """A list of bare Edits: every field restated here from the documented rules (rows = the cone of 1 760 bases in 400-base rows; snippet = rows
    +- 2 400 bases clipped to the window and grown to 8 000, towards the end first; a snippet at the window's start opens its run, one at its end
    closes it, the others follow in list order; tables in buffer order)."""
    L = 48_000
    edits = [S.Edit("sub", 20_011, 2, "AC"), S.Edit("mask", L - 300, 300), S.Edit("inv", 12_345, 900), S.Edit("sub", 0, 1, "N"), S.Edit("sub", 31_999, 1, "T")]
    p = S.plan_batch(edits, L)
    rows, snip = [], []
    for e in edits:
        r0, r1 = max(0, (e.pos - 1_760) // 400), min(L // 400, -(-(e.pos + e.length + 1_760) // 400))
        b0, b1 = max(0, r0 * 400 - 2_400), min(L, r1 * 400 + 2_400)
        while b1 - b0 < 8_000:
            if b1 < L:
                b1 = min(L, b1 + 400)
            else:
                b0 -= 400
        rows.append((r0, r1))
        snip.append((b0, b1 - b0))
    assert rows == [(45, 55), (114, 120), (26, 38), (0, 5), (75, 85)]
    order = [3, 0, 2, 4, 1]                              # the start's snippet, the middle ones in list order, the end's: one run of 43 600 bases
    off, fresh, o, f = {}, {}, 0, 0
    for i in order:
        off[i], fresh[i] = o, f
        o += snip[i][1]
        f += rows[i][1] - rows[i][0]
    assert p.L == L and p.snippet.tolist() == [list(s) for s in snip] and p.rows.tolist() == [list(r) for r in rows] and p.order == order
    assert p.fresh.tolist() == [fresh[i] for i in range(5)] and p.n_fresh == f == 43
    assert p.runs == [(0, o, [((off[i] + rows[i][0] * 400 - snip[i][0]) // 400, rows[i][1] - rows[i][0], fresh[i]) for i in order])]
    pay_off = {0: 0, 3: 2, 4: 3}
    kinds = {"sub": 0, "mask": 1, "inv": 2}
    want = [[off[i], snip[i][0], snip[i][1], kinds[edits[i].kind], edits[i].pos, edits[i].length, pay_off.get(i, 0), 0] for i in order]
    assert p.edit_table.dtype == np.int64 and p.edit_table.tolist() == want
    assert p.splice_table.dtype == np.int64 and p.splice_table.tolist() == [[rows[i][0], rows[i][1] - rows[i][0], fresh[i]] for i in range(5)]
    assert p.payload.dtype == np.uint8 and p.payload.tolist() == [0, 1, 4, 3]
    # the new fields say the same thing: one snippet, one span and one segment per edit
    assert p.item_of.tolist() == [0, 1, 2, 3, 4] and p.seg_off.tolist() == [0, 1, 2, 3, 4, 5] and p.segments.tolist() == p.splice_table.tolist()
    assert p.span_table.tolist() == [[kinds[e.kind], e.pos, e.length, pay_off.get(i, 0)] for i, e in enumerate(edits)]
    assert p.snippet_table.tolist() == [[off[i], snip[i][0], snip[i][1], i, 1, 0, 0, 0] for i in order]
    # single-member sets plan as their members do
    q = S.plan_batch([S.EditSet([e]) for e in edits], L)
    assert q.edit_table.tolist() == want and q.runs == p.runs and q.segments.tolist() == p.segments.tolist()


# ---- region scores ------------------------------------------------------------------------------------------------------------------------------
def test_region_scores_host_against_a_direct_loop():
    rs = np.random.RandomState(5)
    n, E = 23, 4
    ref = rs.randn(n, n).astype(np.float32)
    maps = (ref[None] + 0.1 * rs.randn(E, n, n)).astype(np.float32)
    maps[2] = ref
    regions = [(0, n, 0, n), (3, 4, 7, 8), (n - 5, n, n - 2, n), (0, 1, 0, n), (4, 9, 2, 3)]
    sg, ab = S.region_scores_host(maps, ref, regions)
    assert sg.shape == ab.shape == (E, len(regions)) and sg.dtype == np.float64
    for e in range(E):
        for k, (i0, i1, j0, j1) in enumerate(regions):
            d = [float(maps[e, i, j]) - float(ref[i, j]) for i in range(i0, i1) for j in range(j0, j1)]
            assert sg[e, k] == pytest.approx(sum(d) / len(d), rel=1e-12, abs=1e-17)
            assert ab[e, k] == pytest.approx(sum(abs(v) for v in d) / len(d), rel=1e-12, abs=0)
    assert np.all(sg[2] == 0) and np.all(ab[2] == 0) and np.all(np.abs(sg) <= ab)
    assert ab[:, 0] == pytest.approx(S.scores_host(maps, ref)[1], rel=1e-12)
    maps[1, 3, 7] = np.nan
    sg, ab = S.region_scores_host(maps, ref, regions)
    assert np.isnan(sg[1, :2]).all() and np.isnan(ab[1, :2]).all() and not np.isnan(sg[1, 2:]).any() and not np.isnan(sg[[0, 2, 3]]).any()


@pytest.mark.parametrize("bad", [[], [(0, 1, 0, 1)] * 65, [(0, 0, 0, 1)], [(2, 1, 0, 1)], [(0, 1, 0, 11)], [(-1, 1, 0, 1)], [(0, 1, 3, 3)], [(0, 1, 0)], 5])
def test_regions_validation(bad):
    with pytest.raises(ValueError):
        S.check_regions(bad, 10)


def test_regions_accepted():
    assert S.check_regions([(0, 10, 9, 10)] * 64, 10).shape == (64, 4) and S.check_regions([[0, 1, 0, 1]], 10).dtype == np.int32


# ---- no silent CPU path -------------------------------------------------------------------------------------------------------------------------
def test_no_silent_cpu_path():
    from orca_amd import orca_modules as pm
    net = pm.Net(num_1d=4).eval()
    item = S.EditSet([S.Edit("mask", 0, 10), S.Edit("inv", 20, 10)])
    with pytest.raises(OrcaHipError):
        S.screen_1m(net, torch.zeros(40_000, dtype=torch.uint8), [item], regions=[(0, 1, 0, 1)])
    u8, f32 = torch.zeros(400, dtype=torch.uint8), torch.zeros((10, 128))
    with pytest.raises(OrcaHipError):
        engine.screen_edit_codes_multi(None, u8, np.array([[0, 0, 400, 0, 1, 0, 0, 0]]), np.array([[1, 5, 5, 0]]), None, torch.zeros(400, dtype=torch.uint8))
    with pytest.raises(OrcaHipError):
        engine.screen_splice_rows_multi(None, f32, f32, np.array([[0, 1, 0]]), np.array([0, 1]), torch.zeros((1, 10, 128)))
    with pytest.raises(OrcaHipError):
        engine.screen_region_scores(None, torch.zeros((1, 10, 10)), torch.zeros((10, 10)), [(0, 1, 0, 1)])
