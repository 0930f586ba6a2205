"""The host side of the SV screen's impact scores without a GPU (orca_amd/sv.py): `allele_bin_map` against a per-base brute force on a toy
chromosome, its properties per kind of variant, `level_bin_maps` / `junction_bins` on the variants the GPU tests screen, and
`paired_aligned_scores_host` - the numpy restatement the kernel is tested against - against naive Python loops."""
import math

import numpy as np
import pytest

from orca_amd import orca_predict as OP
from orca_amd import sv
from tests.test_gpu_screen_aligned import kernel_maps
from tests.test_gpu_sv_incremental import CHR, VARIANTS

TOY = 400


def ref_coordinates(pieces):
    """per base of the allele: the reference base it is a copy of"""
    return np.concatenate([np.arange(s, s + ln) if st == "+" else np.arange(s + ln - 1, s - 1, -1) for s, ln, st in pieces])


def brute_bin_map(pieces, alt_start, ref_start, binsize, n):
    coord = ref_coordinates(pieces)
    out = []
    for i in range(n):
        x = alt_start + i * binsize + binsize // 2
        if not 0 <= x < len(coord):
            out.append(-1)
            continue
        m = math.floor((int(coord[x]) - ref_start) / binsize)
        out.append(m if 0 <= m < n else -1)
    return out


TOY_SVS = [sv.SV("del", 100, 160), sv.SV("dup", 100, 160), sv.SV("inv", 100, 160), sv.SV("del", 3, 391), sv.SV("inv", 1, 399), sv.SV("dup", 190, 193),
           sv.SV("inv", 200, 201), sv.SV("del", 0, 50), sv.SV("dup", 350, 400)]


@pytest.mark.parametrize("binsize", [4, 6])
def test_bin_map_equals_brute_force_on_a_toy_chromosome(binsize):
    n = 16
    seen = set()
    for v in TOY_SVS:
        pieces = sv.allele_pieces(v, TOY)
        alt_len = sum(p[1] for p in pieces)
        assert len(ref_coordinates(pieces)) == alt_len
        # windows inside the allele, hanging over its start (negative coordinates) and over its end, reference windows shifted either way
        for alt_start in (-3 * binsize - 1, 0, 60, 97, 101, 130, alt_len - n * binsize, alt_len - 5 * binsize + 2):
            for ref_start in (alt_start, alt_start - 2 * binsize - 1, alt_start + 3 * binsize + 2, 58, 160):
                got = sv.allele_bin_map(pieces, alt_start, ref_start, binsize, n)
                assert got.dtype == np.int32 and got.shape == (n,)
                assert got.tolist() == brute_bin_map(pieces, alt_start, ref_start, binsize, n), (v, alt_start, ref_start)
                seen.update(np.sign(np.diff(got[got >= 0])).tolist())
                seen.add("hole" if (got < 0).any() else "full")
                if np.unique(got[got >= 0]).size < (got >= 0).sum():
                    seen.add("shared")
    assert seen >= {-1, 1, "shared", "hole", "full"}                          # descending, shared, ascending entries, with and without unmapped bins


def test_bin_map_properties():
    n, bs = 16, 4
    whole = [(0, TOY, "+")]
    for start in (0, 100, 333):
        assert sv.allele_bin_map(whole, start, start, bs, n).tolist() == list(range(n))          # no variant, equal starts: the identity
    assert sv.allele_bin_map(whole, 100, 100 + 3 * bs, bs, n).tolist() == [-1] * 3 + list(range(n - 3))
    assert sv.allele_bin_map([], 0, 0, bs, n).tolist() == [-1] * n
    d = sv.allele_bin_map(sv.allele_pieces(sv.SV("del", 120, 140), TOY), 100, 100, bs, n)
    assert d.tolist() == [0, 1, 2, 3, 4] + list(range(10, 16)) + [-1] * 5                        # never descends; a jump of the deleted 5 bins
    assert (np.diff(d[d >= 0]) > 0).all()
    i = sv.allele_bin_map(sv.allele_pieces(sv.SV("inv", 120, 140), TOY), 100, 100, bs, n)
    assert i.tolist() == [0, 1, 2, 3, 4, 9, 8, 7, 6, 5] + list(range(10, 16))                     # descends inside the inversion, and only there
    u = sv.allele_bin_map(sv.allele_pieces(sv.SV("dup", 120, 140), TOY), 100, 100, bs, n)
    assert u.tolist() == list(range(10)) + [5, 6, 7, 8, 9] + [10]                                 # the second copy shares reference bins 5 .. 9
    # general in the bin size and in n
    assert sv.allele_bin_map(sv.allele_pieces(sv.SV("del", 120, 140), TOY), 100, 100, 10, 5).tolist() == [0, 1, 4, -1, -1]


def outputs(v):
    """the two output dicts' start coordinates of a variant, forward strand, as `run_cascade` advances them"""
    rp, rw, rm, ap, aw, am = sv.sv_windows(v, CHR)
    starts = []
    for mpos, wpos in ((rm, rw), (am, aw)):
        st = [0]
        for level in (32, 16, 8, 4, 2, 1):
            st.append(st[-1] + OP.zoom_index_32m(level, st[-1], mpos, wpos, False) * level)
        starts.append({"start_coords": [wpos - 16_000_000 + s * 4000 for s in st[:-1]]})
    return starts


def shared(row):
    m = row[row >= 0]
    return int(m.size - np.unique(m).size)


def test_level_bin_maps_of_the_screened_variants():
    maps = [sv.level_bin_maps(v, CHR, *outputs(v)) for v in VARIANTS]
    for m in maps:
        assert m.dtype == np.int32 and m.shape == (6, 250) and m.min() >= -1 and m.max() <= 249
    counts = [(m >= 0).sum(axis=1).tolist() for m in maps]
    dele, dup, inv, small, dele2 = maps
    assert counts[0] == [240, 232, 212, 175, 100, 0]                       # the finest level of the 1.2 Mb deletion: no locus in common
    assert all((np.diff(r[r >= 0]) > 0).all() for r in dele) and all((np.diff(r[r >= 0]) > 0).all() for r in dele2)
    assert counts[1] == [250] * 6 and [shared(r) for r in dup] == [4, 8, 16, 31, 62, 124]
    assert counts[2] == [250, 250, 250, 250, 248, 248]
    assert [int((np.diff(r[r >= 0]) < 0).sum()) for r in inv] == [23, 45, 93, 187, 247, 247]      # levels 4, 5 lie inside the inversion: descending throughout
    assert counts[3] == [250] * 6 and [int((np.diff(r) < 0).sum()) for r in small] == [0, 0, 0, 0, 1, 2]
    assert counts[4] == [244, 238, 224, 200, 150, 50]
    # each row is `allele_bin_map` at the level's bin size, and a reference allele against itself is the identity at every level
    v = VARIANTS[4]
    ro, ao = outputs(v)
    for k in range(6):
        assert np.array_equal(dele2[k], sv.allele_bin_map(sv.allele_pieces(v, CHR), ao["start_coords"][k], ro["start_coords"][k], 128000 >> k))
        assert np.array_equal(sv.allele_bin_map([(0, CHR, "+")], ro["start_coords"][k], ro["start_coords"][k], 128000 >> k), np.arange(250))


def test_junction_bins():
    for v in VARIANTS:
        ro, ao = outputs(v)
        jb = sv.junction_bins(v, CHR, ao)
        at = {"del": [v.start], "dup": [v.end, 2 * v.end - v.start], "inv": [v.start, v.end]}[v.kind]      # alt coordinates of the first base behind a junction
        assert jb.dtype == np.int32 and jb.shape == (6, len(at))
        for k in range(6):
            for q, p in enumerate(at):
                b = (p - ao["start_coords"][k]) // (128000 >> k)
                assert jb[k, q] == (b if 0 <= b < 250 else -1), (v, k, q)
    assert sv.junction_bins(VARIANTS[0], CHR, outputs(VARIANTS[0])[1])[:, 0].tolist() == [125, 126, 126, 126, 126, 126]
    assert sv.junction_bins(VARIANTS[2], CHR, outputs(VARIANTS[2])[1])[4:].tolist() == [[-1, -1], [-1, -1]]


def naive_scores(a, r, m):
    """the definitions of include/orca_hip.h (orca_screen_paired_aligned_scores) as Python loops over one pair"""
    n = len(m)
    M = [i for i in range(n) if m[i] >= 0]
    c = len(M)
    nan = float("nan")
    out = {"count": c, "profile": [nan] * n, "abs_mean": nan, "abs_max": nan, "delta_mean": nan, "rms": nan, "corr": nan}
    if c == 0:
        return out
    xs = [float(a[i][j]) for i in M for j in M]
    ys = [float(r[m[i]][m[j]]) for i in M for j in M]
    dl = [x - y for x, y in zip(xs, ys)]
    for i in M:
        out["profile"][i] = math.fsum(abs(float(a[i][j]) - float(r[m[i]][m[j]])) for j in M) / c
    out["abs_mean"], out["abs_max"] = math.fsum(abs(d) for d in dl) / c ** 2, max(abs(d) for d in dl)
    out["delta_mean"], out["rms"] = math.fsum(dl) / c ** 2, math.sqrt(math.fsum(d * d for d in dl) / c ** 2)
    mx, my = math.fsum(xs) / c ** 2, math.fsum(ys) / c ** 2
    X, Y, C = math.fsum((x - mx) ** 2 for x in xs), math.fsum((y - my) ** 2 for y in ys), math.fsum((x - mx) * (y - my) for x, y in zip(xs, ys))
    if c >= 2 and X != 0.0 and Y != 0.0:
        out["corr"] = C / math.sqrt(X * Y)
    return out


def test_host_restatement_equals_naive_loops():
    n = 7
    maps = dict(kernel_maps(n), descending=np.arange(n)[::-1].copy())
    names = list(maps)
    rs = np.random.RandomState(5)
    B = len(names)
    alt, ref = rs.randn(B, n, n).astype(np.float32), rs.randn(B, n, n).astype(np.float32)
    bm = np.stack([maps[k] for k in names]).astype(np.int32)
    got = sv.paired_aligned_scores_host(alt, ref, bm)
    assert got["count"].dtype == np.int32 and got["profile"].shape == (B, n) and all(got[k].dtype == np.float64 for k in sv.SCORE_FIELDS)
    for b, name in enumerate(names):
        want = naive_scores(alt[b], ref[b], bm[b].tolist())
        assert got["count"][b] == want["count"], name
        for k in sv.SCORE_FIELDS:
            np.testing.assert_allclose(got[k][b], want[k], rtol=1e-13, atol=1e-15, equal_nan=True, err_msg=f"{name} {k}")
    k = names.index("none")
    assert got["count"][k] == 0 and all(np.isnan(got[f][k]).all() for f in sv.SCORE_FIELDS)
    k = names.index("one")
    d = abs(float(alt[k, n // 2, n // 2]) - float(ref[k, n - 1, n - 1]))
    assert got["count"][k] == 1 and got["abs_mean"][k] == got["abs_max"][k] == got["rms"][k] == d and np.isnan(got["corr"][k])
    assert int(np.isfinite(got["profile"][k]).sum()) == 1
    # one bin map for all pairs; every pair against the reference of its own
    one = sv.paired_aligned_scores_host(alt[:3], ref[:3], maps["shift"])
    for b in range(3):
        assert one["abs_mean"][b] == sv.paired_aligned_scores_host(alt[b: b + 1], ref[b: b + 1], maps["shift"][None])["abs_mean"][0]
    assert len({float(v) for v in one["abs_mean"]}) == 3
    # a map against itself; a constant map has no correlation
    same = sv.paired_aligned_scores_host(ref[:1], ref[:1], np.arange(n))
    assert same["abs_max"][0] == 0.0 and same["rms"][0] == 0.0 and same["corr"][0] == 1.0
    flat = sv.paired_aligned_scores_host(np.full((1, n, n), 0.375, dtype=np.float32), ref[:1], np.arange(n))
    assert np.isnan(flat["corr"][0]) and np.isfinite(flat["abs_mean"][0])
    # NaN: at a mapped pair in that pair's scalars and that row of the profile; at an unmapped pair nowhere
    holes = maps["holes"]
    un, mp = int(np.flatnonzero(holes < 0)[0]), np.flatnonzero(holes >= 0)
    a2 = alt[:2].copy()
    a2[0, un, :] = np.nan
    a2[0, :, un] = np.nan
    quiet, clean = sv.paired_aligned_scores_host(a2, ref[:2], holes), sv.paired_aligned_scores_host(alt[:2], ref[:2], holes)
    assert all(np.array_equal(quiet[f], clean[f], equal_nan=True) for f in sv.SCORE_FIELDS)
    a2 = alt[:2].copy()
    a2[1, mp[1], mp[0]] = np.nan
    loud = sv.paired_aligned_scores_host(a2, ref[:2], holes)
    for f in ("abs_mean", "abs_max", "delta_mean", "rms", "corr"):
        assert np.isnan(loud[f][1]) and loud[f][0] == clean[f][0], f
    assert np.isnan(loud["profile"][1, mp[1]]) and np.array_equal(np.delete(loud["profile"], mp[1], axis=1), np.delete(clean["profile"], mp[1], axis=1), equal_nan=True)
    for bad in (np.full(n, n), np.full(n, -2), np.zeros((3, n)), np.zeros(n - 1)):
        with pytest.raises(ValueError):
            sv.paired_aligned_scores_host(alt[:2], ref[:2], bad)


def test_keep_maps_false_needs_scores():
    with pytest.raises(ValueError):
        sv.sv_screen([], None, [], CHR, keep_maps=False)
