"""The host side of the screen's non-additivity scores (orca_amd/screen.py: `epistasis_items`, `epistasis_scores_host`): the member table of a list
of sets, and the fp64 restatement against a per-pixel Python formula on hand-made maps.  No GPU."""
import numpy as np
import pytest

from orca_amd import screen as S


def _key(e):
    return (e.kind, e.pos, e.length, None if e.seq is None else e.seq.tobytes())


def test_items_dedupe_and_reproduce_the_pair_index():
    a = S.tile_edits("mask", 500, 4_000, 10_000, 30_000)
    b = S.tile_edits("mask", 500, 4_000, 100_000, 112_000) + [S.Edit("sub", 150_000, 2, "AC")]
    sets, index = S.pair_edits(a, b)
    assert len(sets) == len(a) * len(b)
    singles, off, mem = S.epistasis_items(sets)
    assert len(singles) == len(a) + len(b) and len({_key(e) for e in singles}) == len(singles)
    assert off.dtype == np.int64 and mem.dtype == np.int32 and off.tolist() == list(range(0, 2 * len(sets) + 1, 2)) and mem.size == 2 * len(sets)
    for k, (i, j) in enumerate(index):
        got = [singles[m] for m in mem[off[k]: off[k + 1]]]
        assert [_key(e) for e in got] == [_key(e) for e in sets[k].edits]                     # the set's own sorted order
        assert {_key(e) for e in got} == {_key(a[i]), _key(b[j])}
    # order of first appearance: the first set's members first
    assert [_key(e) for e in singles[:2]] == [_key(e) for e in sets[0].edits]
    # equal edits built apart are one single; another payload is another single
    s2, o2, m2 = S.epistasis_items([S.EditSet([S.Edit("sub", 5, 1, "A"), S.Edit("mask", 9, 2)]), S.EditSet([S.Edit("sub", 5, 1, [0])]), S.EditSet([S.Edit("sub", 5, 1, "C")])])
    assert len(s2) == 3 and o2.tolist() == [0, 2, 3, 4] and m2.tolist() == [0, 1, 0, 2]


def test_a_bare_edit_is_a_one_member_set():
    e = S.Edit("inv", 1_000, 300)
    singles, off, mem = S.epistasis_items([e, S.EditSet([e, S.Edit("mask", 5_000, 10)]), S.EditSet([e])])
    assert len(singles) == 2 and singles[0] is e and off.tolist() == [0, 1, 3, 4] and mem.tolist() == [0, 0, 1, 0]
    with pytest.raises(TypeError):
        S.epistasis_items(["mask"])


def test_length_changing_members_are_refused():
    for bad in (S.Edit("del", 10, 5), S.Edit("ins", 10, "ACG")):
        with pytest.raises(ValueError):
            S.epistasis_items([S.EditSet([S.Edit("mask", 100, 10), bad])])
        with pytest.raises(ValueError):
            S.epistasis_items([bad])


def _hand_made():
    rs = np.random.RandomState(3)
    n = 3
    ref = rs.randn(n, n).astype(np.float32)
    bank = (ref[None] + 0.1 * rs.randn(4, n, n)).astype(np.float32)
    maps = (ref[None] + 0.2 * rs.randn(4, n, n)).astype(np.float32)
    maps[2] = bank[3]                                                              # set 2 = {single 3}: its map holds the single's bits
    off, mem = np.array([0, 2, 5, 6, 7]), np.array([0, 1, 2, 0, 3, 3, 1])
    return n, ref, bank, maps, off, mem


def test_host_scores_equal_the_per_pixel_formula():
    n, ref, bank, maps, off, mem = _hand_made()
    regions = [(0, 2, 1, 3), (2, 3, 0, 1), (0, 3, 0, 3)]
    prof, mean, amax, add, sg, ab = S.epistasis_scores_host(maps, bank, ref, off, mem, regions)
    assert prof.shape == (4, n) and mean.shape == amax.shape == add.shape == (4,) and sg.shape == ab.shape == (4, 3)
    for e in range(4):
        r, t = np.zeros((n, n)), np.zeros((n, n))
        for i in range(n):
            for j in range(n):
                s = 0.0
                for m in mem[off[e]: off[e + 1]]:
                    s = s + (float(bank[m, i, j]) - float(ref[i, j]))
                t[i, j] = s
                r[i, j] = (float(maps[e, i, j]) - float(ref[i, j])) - s
        tol = 4 * 2.0 ** -53 * n * n * max(np.abs(r).max(), np.abs(t).max())       # the sums' order only; every pixel is the same expression
        assert amax[e] == np.abs(r).max()
        assert abs(mean[e] - sum(abs(v) for v in r.ravel()) / (n * n)) <= tol and abs(add[e] - sum(abs(v) for v in t.ravel()) / (n * n)) <= tol
        for i in range(n):
            assert abs(prof[e, i] - sum(abs(v) for v in r[i]) / n) <= tol
        for k, (i0, i1, j0, j1) in enumerate(regions):
            box = r[i0:i1, j0:j1].ravel()
            assert abs(sg[e, k] - sum(box) / box.size) <= tol and abs(ab[e, k] - sum(abs(v) for v in box) / box.size) <= tol
    # without regions: the same four, and None twice
    again = S.epistasis_scores_host(maps, bank, ref, off, mem)
    assert again[4] is None and again[5] is None and all(np.array_equal(x, y) for x, y in zip(again[:4], (prof, mean, amax, add)))


def test_a_one_member_set_that_holds_its_singles_bits_scores_zero():
    n, ref, bank, maps, off, mem = _hand_made()
    prof, mean, amax, add, sg, ab = S.epistasis_scores_host(maps, bank, ref, off, mem, [(0, n, 0, n)])
    assert mean[2] == 0.0 and amax[2] == 0.0 and not prof[2].any() and sg[2, 0] == 0.0 and ab[2, 0] == 0.0
    assert add[2] == np.abs(bank[3].astype(np.float64) - ref.astype(np.float64)).mean() and add[2] > 0.0
    assert mean[3] > 0.0                                                           # set 3 = {single 1} with another map


def test_region_scores_are_signed():
    n = 3
    ref = np.zeros((n, n), dtype=np.float32)
    bank = np.stack([np.full((n, n), 0.25, dtype=np.float32), np.full((n, n), 0.5, dtype=np.float32)])
    maps = np.stack([np.full((n, n), 0.5, dtype=np.float32), np.full((n, n), 1.0, dtype=np.float32)])      # below and above the additive 0.75
    off, mem = np.array([0, 2, 4]), np.array([0, 1, 0, 1])
    prof, mean, amax, add, sg, ab = S.epistasis_scores_host(maps, bank, ref, off, mem, [(0, 1, 0, 2)])
    assert sg[:, 0].tolist() == [-0.25, 0.25] and ab[:, 0].tolist() == [0.25, 0.25] and add.tolist() == [0.75, 0.75] and mean.tolist() == [0.25, 0.25]


def test_a_nan_propagates_and_bad_tables_are_refused():
    n, ref, bank, maps, off, mem = _hand_made()
    bank = bank.copy()
    bank[1, 0, 2] = np.nan                                                         # single 1: in sets 0 and 3
    prof, mean, amax, add, sg, ab = S.epistasis_scores_host(maps, bank, ref, off, mem, [(0, 1, 0, 2), (0, 1, 2, 3)])
    assert np.isnan(mean).tolist() == [True, False, False, True] == np.isnan(amax).tolist() == np.isnan(add).tolist()
    assert np.isnan(prof[0]).tolist() == [True, False, False] and np.isnan(sg[0]).tolist() == [False, True] and not np.isnan(sg[1]).any()
    for bad_off, bad_mem in (([1, 2, 5, 6, 7], mem), ([0, 2, 2, 6, 7], mem), ([0, 2, 5, 6, 6], mem), (off, [0, 1, 2, 0, 3, 3, 4]), (off, [0, 1, 2, 0, 3, 3, -1]), (off[:-1], mem)):
        with pytest.raises(ValueError):
            S.epistasis_scores_host(maps, bank, ref, bad_off, bad_mem)
