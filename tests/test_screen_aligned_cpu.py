"""Aligned bins of the 1 Mb mutagenesis screen, host side (orca_amd/screen.py): `bin_map` against a brute-force restatement that carries a label
per context base through the item, the two generators for large edits, and the numpy restatements of the aligned scores (against
`scores_host` / `region_scores_host` on an identity map, and against values worked out by hand).  No GPU."""
import numpy as np
import pytest

from orca_amd import screen as S

L = 40_000
N = L // 4000
FLANKS = (0, 8_000)
SIZES = (1, 1_999, 2_000, 2_001, 4_000, 12_000)


def brute_bin_map(item, L, F):
    """Label the context bases 0 .. L + F - 1, apply the item to the labels (an inserted base and the N fill are -1; ``sub`` / ``mask`` / ``inv``
    spans keep their labels in place), cut to L and read the labels at the bins' midpoints: a label below L is a window base, its bin label // 4000."""
    lab = np.arange(L + F, dtype=np.int64)
    parts, p = [], 0
    for e in S.members_of(item):
        parts.append(lab[p: e.pos])
        if e.kind == "ins":
            parts.append(np.full(e.seq.size, -1, dtype=np.int64))
        elif e.kind != "del":
            parts.append(lab[e.pos: e.end])
        p = e.end
    parts += [lab[p:], np.full(L, -1, dtype=np.int64)]
    at = np.concatenate(parts)[:L][2000::4000]
    return np.where((at >= 0) & (at < L), at // 4000, -1).astype(np.int32)


def _codes(seed=3, n=L):
    return np.random.RandomState(seed).randint(0, 4, n).astype(np.uint8)


def _seq(n, seed=0):
    return np.random.RandomState(seed).randint(0, 4, n).astype(np.uint8)


def named_items():
    c = _codes()
    items = {"sub": S.Edit("sub", 777, 3, "ACG"), "mask": S.Edit("mask", 3_000, 9_000), "inv": S.Edit("inv", 17_000, 6_001)}
    for k in SIZES:
        items[f"del{k}"] = S.Edit("del", 9_500, k)
        items[f"ins{k}"] = S.Edit("ins", 9_500, _seq(k, k))
    items["ins_at_0"] = S.Edit("ins", 0, _seq(5_000, 1))
    items["ins_at_L"] = S.Edit("ins", L, _seq(5_000, 2))
    items["del_into_last_bin"] = S.Edit("del", 30_500, 8_000)
    items["del_to_the_end"] = S.Edit("del", 33_000, 7_000)
    items["balanced"] = S.EditSet([S.Edit("del", 6_000, 3_000), S.Edit("ins", 15_000, _seq(3_000, 3))])
    items["inv_del_ins"] = S.EditSet([S.Edit("inv", 2_000, 5_000), S.Edit("del", 11_000, 6_500), S.Edit("ins", 25_000, _seq(2_500, 4)), S.Edit("sub", 25_000, 2, "TT")])
    items["tandem_dup"] = S.tandem_dup(c, 12_000, 8_000)
    return items


def random_items(count=300, seed=11):
    rs = np.random.RandomState(seed)
    out = []
    for _ in range(count):
        k = int(rs.randint(1, 5))
        pos = np.sort(rs.choice(np.arange(1, L), k, replace=False))
        members = []
        for m, p in enumerate(pos):
            room = int(pos[m + 1] if m + 1 < k else L) - int(p)
            kind = S.KINDS[rs.randint(len(S.KINDS))]
            if kind == "ins":
                members.append(S.Edit("ins", int(p), _seq(int(rs.randint(1, 9_000)), int(p))))
                continue
            n = int(rs.randint(1, min(room, 9_000) + 1))
            members.append(S.Edit(kind, int(p), n, _seq(n, int(p))) if kind == "sub" else S.Edit(kind, int(p), n))
        out.append(members[0] if k == 1 and rs.rand() < 0.5 else S.EditSet(members))
    return out


def _monotone(m):
    v = m[m >= 0]
    return bool(np.all(np.diff(v) >= 0))


@pytest.mark.parametrize("F", FLANKS)
def test_bin_map_equals_the_brute_force_restatement(F):
    ident = np.arange(N, dtype=np.int32)
    items = named_items()
    for name, it in items.items():
        m = S.bin_map(it, L, F)
        assert m.dtype == np.int32 and m.shape == (N,), name
        assert np.array_equal(m, brute_bin_map(it, L, F)), (name, m)
        assert _monotone(m), (name, m)
    for name in ("sub", "mask", "inv", "ins_at_L"):                   # length-preserving (and an insertion pushed out whole): the identity
        assert np.array_equal(S.bin_map(items[name], L, F), ident), name
    assert np.array_equal(S.bin_map(S.EditSet([items["sub"], items["mask"], items["inv"]]), L, F), ident)
    # a shift below 2 000 bases moves no midpoint across a bin edge here; 2 000 does, for every bin behind the deletion
    assert np.array_equal(S.bin_map(items["del1"], L, F), ident) and np.array_equal(S.bin_map(items["del1999"], L, F), ident)
    assert S.bin_map(items["del2000"], L, F).tolist() == [0, 1, 3, 4, 5, 6, 7, 8, 9, -1]          # bin 2 = bases 8 000 .. holds the cut; the refill is -1
    assert S.bin_map(items["del4000"], L, F).tolist() == [0, 1, 3, 4, 5, 6, 7, 8, 9, -1]
    assert S.bin_map(items["del12000"], L, F).tolist() == [0, 1, 5, 6, 7, 8, 9, -1, -1, -1]
    assert np.array_equal(S.bin_map(items["ins1"], L, F), ident)
    assert S.bin_map(items["ins1999"], L, F).tolist() == [0, 1, -1, 3, 4, 5, 6, 7, 8, 9]           # alt base 10 000 is inserted; behind it the identity
    assert S.bin_map(items["ins2001"], L, F).tolist() == [0, 1, -1, 2, 3, 4, 5, 6, 7, 8]           # alt base 10 000 is inserted
    assert S.bin_map(items["ins4000"], L, F).tolist() == [0, 1, -1, 2, 3, 4, 5, 6, 7, 8]
    assert S.bin_map(items["ins_at_0"], L, F).tolist() == [-1, 0, 1, 2, 3, 4, 5, 6, 7, 8]          # 5 000 bases in front: bin 1's midpoint is base 1 000
    # balanced: the identity behind the set (and in front of it); in between the bins are displaced
    b = S.bin_map(items["balanced"], L, F)
    assert np.array_equal(b[:1], ident[:1]) and np.array_equal(b[4:], ident[4:]) and b.tolist()[1:4] == [2, 3, -1]
    # a tandem duplication: the inserted copy [20 000, 28 000) is -1, the source keeps its bins, the tail is displaced by two bins
    assert S.bin_map(items["tandem_dup"], L, F).tolist() == [0, 1, 2, 3, 4, -1, -1, 5, 6, 7]
    assert np.array_equal(S.bin_map(items["del_to_the_end"], L, F)[:8], ident[:8]) and S.bin_map(items["del_to_the_end"], L, F)[9] == -1


@pytest.mark.parametrize("F", FLANKS)
def test_bin_map_of_random_items(F):
    shared = 0
    for it in random_items():
        m = S.bin_map(it, L, F)
        assert np.array_equal(m, brute_bin_map(it, L, F)), (it, m)
        assert _monotone(m) and m.min() >= -1 and m.max() < N, (it, m)
        if not S.changes_length(it):
            assert np.array_equal(m, np.arange(N)), it
        v = m[m >= 0]
        shared += int(np.any(np.diff(v) == 0))
    assert shared > 0                                                   # two alt bins that share a reference bin do occur


def test_bin_map_refuses_bad_arguments():
    with pytest.raises(ValueError):
        S.bin_map(S.Edit("del", 5, 10), L + 1)
    with pytest.raises(ValueError):
        S.bin_map(S.Edit("del", 5, 10), L, L + 1)
    with pytest.raises(ValueError):
        S.bin_map(S.Edit("del", L - 5, 10), L)
    with pytest.raises(TypeError):
        S.bin_map("del", L)


def test_deletion_scan_bounds():
    sc = S.deletion_scan(4_000, 2_000, 0, 20_000)
    assert [e.pos for e in sc] == [1] + list(range(2_001, 16_001, 2_000)) and all(e.kind == "del" and e.length == 4_000 and e.end <= 20_000 for e in sc)
    sc = S.deletion_scan(4_000, 2_000, 8_000, 20_000)
    assert [e.pos for e in sc] == [8_000, 10_000, 12_000, 14_000, 16_000] and sc[-1].end == 20_000
    assert [e.pos for e in S.deletion_scan(100, 50, 10, 111)] == [10] and S.deletion_scan(100, 50, 10, 109) == []
    assert [e.pos for e in S.deletion_scan(3, 1, 0, 5)] == [1, 2]
    for w, s in ((0, 5), (5, 0), (-1, 5)):
        with pytest.raises(ValueError):
            S.deletion_scan(w, s, 0, 100)


def test_tandem_dup_is_the_insertion_of_the_copy():
    c = _codes()
    d = S.tandem_dup(c, 12_000, 8_000)
    assert (d.kind, d.pos, d.length) == ("ins", 20_000, 0) and np.array_equal(d.seq, c[12_000:20_000])
    hand = S.Edit("ins", 20_000, c[12_000:20_000])
    want = np.concatenate([c[:20_000], c[12_000:20_000], c[20_000:]])[:L]
    assert np.array_equal(S.apply_edit(c, d), want) and np.array_equal(S.apply_edit(c, d), S.apply_edit(c, hand))
    assert S.shift_of(d) == -8_000
    end = S.tandem_dup(c, L - 100, 100)                                 # a copy behind the last base is pushed out whole
    assert end.pos == L and np.array_equal(S.apply_edit(c, end), c)
    for pos, n in ((-1, 10), (L - 5, 10), (10, 0)):
        with pytest.raises(ValueError):
            S.tandem_dup(c, pos, n)
    with pytest.raises(ValueError):
        S.Edit("dup", 10, 10)                                           # still no kind of its own


def test_host_restatements_on_an_identity_map():
    rs = np.random.RandomState(5)
    n, E = 13, 4
    maps, ref = rs.randn(E, n, n).astype(np.float32), rs.randn(n, n).astype(np.float32)
    rects = [(0, n, 0, n), (2, 5, 7, 13), (12, 13, 0, 1)]
    ident = np.arange(n, dtype=np.int32)
    for bm in (ident, np.repeat(ident[None], E, axis=0)):
        for got, want in zip(S.aligned_scores_host(maps, ref, bm), S.scores_host(maps, ref)):
            assert got.dtype == np.float64 and np.allclose(got, want, rtol=1e-12, atol=0)
        for got, want in zip(S.aligned_region_scores_host(maps, ref, bm, rects), S.region_scores_host(maps, ref, rects)):
            assert got.dtype == np.float64 and np.allclose(got, want, rtol=1e-12, atol=1e-15)
    with pytest.raises(ValueError):
        S.aligned_scores_host(maps, ref, np.full(n, n))
    with pytest.raises(ValueError):
        S.aligned_scores_host(maps, ref, np.full((E, n + 1), 0))
    with pytest.raises(ValueError):
        S.aligned_region_scores_host(maps, ref, ident, [(0, 0, 0, 1)])


def test_host_restatements_on_a_hand_made_case():
    """alt[i, j] = 10 i + j, ref[i, j] = i + 2 j, map = [0, 2, -1, 3]: M = {0, 1, 3}, c = 3, and with the reference bins (0, 2, 3)
         i = 0: |0 - 0|, |1 - 4|, |3 - 6|      = 0, 3, 3      sum 6
         i = 1: |10 - 2|, |11 - 6|, |13 - 8|   = 8, 5, 5      sum 18
         i = 3: |30 - 3|, |31 - 7|, |33 - 9|   = 27, 24, 24   sum 75
    so profile = (2, 6, NaN, 25), mean = 99 / 9 = 11, max = 27.  Alt row 2 and column 2 hold NaN: they are not mapped and must not show."""
    alt = (10.0 * np.arange(4)[:, None] + np.arange(4)[None]).astype(np.float32)
    ref = (np.arange(4)[:, None] + 2.0 * np.arange(4)[None]).astype(np.float32)
    alt[2, :] = np.nan
    alt[:, 2] = np.nan
    bm = np.array([0, 2, -1, 3], dtype=np.int32)
    prof, mean, amax = S.aligned_scores_host(alt[None], ref, bm)
    assert np.array_equal(prof[0, [0, 1, 3]], [2.0, 6.0, 25.0]) and np.isnan(prof[0, 2]) and mean[0] == 11.0 and amax[0] == 27.0
    # rectangles in reference bins: rows {2, 3} x column {0} = alt rows {1, 3} x alt column {0}: (10 - 2, 30 - 3); row {0} x columns {2, 3} = alt
    # row 0 x alt columns {1, 3}: (1 - 4, 3 - 6); reference bin 1 stands behind no alt bin: NaN
    sg, ab = S.aligned_region_scores_host(alt[None], ref, bm, [(2, 4, 0, 1), (0, 1, 2, 4), (1, 2, 0, 4), (0, 4, 1, 2)])
    assert sg[0, :2].tolist() == [17.5, -3.0] and ab[0, :2].tolist() == [17.5, 3.0] and np.isnan(sg[0, 2:]).all() and np.isnan(ab[0, 2:]).all()
    # a NaN at a mapped pair does show, in the row's profile, the mean and the max
    alt[1, 3] = np.nan
    prof, mean, amax = S.aligned_scores_host(alt[None], ref, bm)
    assert prof[0, 0] == 2.0 and np.isnan(prof[0, 1]) and prof[0, 3] == 25.0 and np.isnan(mean[0]) and np.isnan(amax[0])
    # nothing mapped: NaN everywhere
    prof, mean, amax = S.aligned_scores_host(alt[None], ref, np.full(4, -1))
    assert np.isnan(prof).all() and np.isnan(mean[0]) and np.isnan(amax[0])
