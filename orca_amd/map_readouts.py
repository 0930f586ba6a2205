"""What the screens read from finished maps, restated in numpy: the leaf module under `screen`, `sv`, `sv_readouts` and `scan`.

The parameter classes of the readouts (`LoopParams`, `BoundaryParams`), the checks of the readout arguments (``check_*``; `check_loops_arg` and
`check_boundaries_arg` also say when an argument is unset), the ``*_host`` restatements that the tests hold the kernels to (include/orca_hip.h
defines what each kernel computes), and the host matching that the screens themselves run after their last batch (`_follow_loops`,
`_match_loops`, `_match_boundaries`, `_boundary_fields`).  Nothing here touches a device: numpy and the standard library only, so every other
module of the screens may build on it.  `screen` re-exports every name, and the docstrings speak of them as ``screen.NAME``.
"""
from dataclasses import dataclass
from typing import Optional

import numpy as np

BIN_BP = 4000


def _bin_maps(bin_map_, E, n):
    m = np.asarray(bin_map_)
    if m.ndim == 1:
        m = np.repeat(m[None], E, axis=0)
    if m.shape != (E, n) or not np.issubdtype(m.dtype, np.integer) or (m.size and (m.min() < -1 or m.max() >= n)):
        raise ValueError(f"bin_map: [{E}, {n}] integers -1 .. {n - 1}")
    return m.astype(np.int64)


# ---- scores ---------------------------------------------------------------------------------------------------------------------------------
def scores_host(maps, ref_map):
    """The scores of `ScreenResult` from alt maps [E, n, n] and the reference map [n, n] (fp64 host restatement of orca_screen_scores):
    d = |alt - ref|; delta_profile[e, i] = mean_j d[e, i, j]; delta_abs_mean[e] = mean_ij d[e, i, j]; delta_abs_max[e] = max_ij d[e, i, j]."""
    d = np.abs(np.asarray(maps, dtype=np.float64) - np.asarray(ref_map, dtype=np.float64)[None])
    return d.mean(axis=2), d.mean(axis=(1, 2)), d.max(axis=(1, 2))


def check_regions(regions, n):
    """``regions`` as a [K, 4] int32 array of half-open bin rectangles (i0, i1, j0, j1), 0 <= i0 < i1 <= n and the same for j, 1 <= K <= 64."""
    try:
        r = np.array([[int(v) for v in rect] for rect in regions], dtype=np.int64)
    except (TypeError, ValueError):
        raise ValueError("regions: a list of (i0, i1, j0, j1) bin rectangles") from None
    if r.ndim != 2 or r.shape[1] != 4 or not 1 <= r.shape[0] <= 64:
        raise ValueError("regions: 1 to 64 rectangles (i0, i1, j0, j1)")
    for k, (i0, i1, j0, j1) in enumerate(r):
        if not (0 <= i0 < i1 <= n and 0 <= j0 < j1 <= n):
            raise ValueError(f"region {k} = rows [{i0}, {i1}) x columns [{j0}, {j1}): half open, non-empty, inside the map's {n} bins")
    return r.astype(np.int32)


def region_scores_host(maps, ref_map, regions):
    """The region scores of `ScreenResult` from alt maps [E, n, n] and the reference map [n, n] (fp64 host restatement of
    orca_screen_region_scores): with d = alt - ref, (delta_region [E, K], delta_region_abs [E, K]) = the means of d and of |d| over rows
    [i0, i1) x columns [j0, j1) of every rectangle (i0, i1, j0, j1)."""
    ref = np.asarray(ref_map, dtype=np.float64)
    d = np.asarray(maps, dtype=np.float64) - ref[None]
    r = check_regions(regions, ref.shape[0])
    sg = np.stack([d[:, i0:i1, j0:j1].mean(axis=(1, 2)) for i0, i1, j0, j1 in r], axis=1)
    ab = np.stack([np.abs(d[:, i0:i1, j0:j1]).mean(axis=(1, 2)) for i0, i1, j0, j1 in r], axis=1)
    return sg, ab


def aligned_scores_host(maps, ref_map, bin_map):
    """The aligned scores of `ScreenResult` from alt maps [E, n, n], the reference map [n, n] and the bin maps [E, n] (or one [n] for all; fp64 host
    restatement of orca_screen_aligned_scores).  With M = the alt bins whose ``bin_map`` is >= 0, c = |M| and d[i, j] = |alt[i, j] - ref[map i,
    map j]| for i, j in M: (aligned_profile [E, n], aligned_abs_mean [E], aligned_abs_max [E]) = (sum_j d[i, j] / c, NaN outside M;
    sum_ij d / c^2; max d), all NaN for an item with c = 0."""
    alt, ref = np.asarray(maps, dtype=np.float64), np.asarray(ref_map, dtype=np.float64)
    E, n = alt.shape[0], ref.shape[0]
    bm = _bin_maps(bin_map, E, n)
    prof, mean, amax = np.full((E, n), np.nan), np.full(E, np.nan), np.full(E, np.nan)
    for e in range(E):
        M = np.flatnonzero(bm[e] >= 0)
        if M.size:
            r = bm[e, M]
            d = np.abs(alt[e][np.ix_(M, M)] - ref[np.ix_(r, r)])
            prof[e, M], mean[e], amax[e] = d.sum(axis=1) / M.size, d.sum() / M.size ** 2, d.max()
    return prof, mean, amax


def aligned_region_scores_host(maps, ref_map, bin_map, regions):
    """The aligned region scores of `ScreenResult` (fp64 host restatement of orca_screen_aligned_region_scores): the rectangles are in REFERENCE
    bins, and rectangle (i0, i1, j0, j1) takes the alt pairs (i, j) with map i in [i0, i1) and map j in [j0, j1).  (aligned_region [E, K],
    aligned_region_abs [E, K]) = the means of alt[i, j] - ref[map i, map j] and of its absolute value over them, NaN where no pair qualifies."""
    alt, ref = np.asarray(maps, dtype=np.float64), np.asarray(ref_map, dtype=np.float64)
    E, n = alt.shape[0], ref.shape[0]
    bm = _bin_maps(bin_map, E, n)
    rects = check_regions(regions, n)
    sg, ab = np.full((E, len(rects)), np.nan), np.full((E, len(rects)), np.nan)
    for e in range(E):
        for k, (i0, i1, j0, j1) in enumerate(rects):
            rows, cols = np.flatnonzero((bm[e] >= i0) & (bm[e] < i1)), np.flatnonzero((bm[e] >= j0) & (bm[e] < j1))
            if rows.size and cols.size:
                d = alt[e][np.ix_(rows, cols)] - ref[np.ix_(bm[e, rows], bm[e, cols])]
                sg[e, k], ab[e, k] = d.mean(), np.abs(d).mean()
    return sg, ab


def check_insulation(widths, n):
    """``insulation`` as an int32 array of 1 to 8 distinct diamond widths in bins (an int stands for one width), each 1 <= w <= (n - 1) // 2: the
    widths at which at least one bin of an n-bin map has a diamond."""
    try:
        w = _widths(widths)
    except (TypeError, ValueError):
        raise ValueError("insulation: a width in bins or a sequence of widths") from None
    if not 1 <= len(w) <= 8 or len(set(w)) != len(w):
        raise ValueError("insulation: 1 to 8 distinct widths")
    for v in w:
        if not 1 <= v <= (n - 1) // 2:
            raise ValueError(f"insulation width {v}: 1 .. {(n - 1) // 2} bins on a map of {n} bins (the diamond must fit somewhere)")
    return np.array(w, dtype=np.int32)


def check_viewpoints(views, n):
    """``viewpoints`` as an int32 array of 1 to 64 bins in [0, n)."""
    try:
        v = [int(x) for x in views]
    except (TypeError, ValueError):
        raise ValueError("viewpoints: a sequence of bins") from None
    if not 1 <= len(v) <= 64:
        raise ValueError("viewpoints: 1 to 64 bins")
    for x in v:
        if not 0 <= x < n:
            raise ValueError(f"viewpoint {x}: inside the map's {n} bins")
    return np.array(v, dtype=np.int32)


def _widths(widths):
    return [int(widths)] if np.ndim(widths) == 0 else [int(v) for v in widths]


def insulation_host(maps, widths):
    """Insulation tracks of maps [E, n, n] at ``widths`` (bins): fp64 [E, W, n].  The diamond of bin i at width w is rows [i - w, i) x columns
    (i, i + w] - bin i's own row and column left out, centred on bin i; it fits when w <= i < n - w.  ins_w(m)[i] = the mean of m over the diamond
    (w^2 terms, fp64), NaN where it does not fit; lower = more insulated.  Every diamond is summed on its own, so a NaN pixel shows in the bins
    whose diamond holds it and in no other."""
    m = np.asarray(maps, dtype=np.float64)
    E, n = m.shape[0], m.shape[1]
    ws = _widths(widths)
    out = np.full((E, len(ws), n), np.nan)
    for k, w in enumerate(ws):
        for i in range(w, n - w):
            out[:, k, i] = m[:, i - w: i, i + 1: i + w + 1].sum(axis=(1, 2)) / float(w * w)
    return out


def insulation_scores_host(maps, ref_map, widths, bin_map=None):
    """The insulation fields of `ScreenResult` from alt maps [E, n, n] and the reference map [n, n] (fp64 host restatement of
    orca_screen_insulation), with ins = `insulation_host`: (insulation [E, W, n] = ins(alt), delta_insulation [E, W, n] = ins(alt)[i] - ins(ref)[i],
    aligned_insulation [E, W, n] or None without ``bin_map``).  aligned[e, k, i], with r = bin_map[e, i] ([E, n], or one [n] for all): ins(alt_e)[i] -
    ins(ref)[r] if r >= 0, the alt diamond fits at i and the reference diamond fits at r, else NaN; indexed by ALT bin; only the centre bin has to
    be mapped.  Where the bin map is the identity it is delta_insulation."""
    alt = insulation_host(maps, widths)
    ref = insulation_host(np.asarray(ref_map)[None], widths)[0]
    E, n = alt.shape[0], alt.shape[2]
    if bin_map is None:
        return alt, alt - ref[None], None
    bm = _bin_maps(bin_map, E, n)
    at = np.full(alt.shape, np.nan)
    for e in range(E):
        M = np.flatnonzero(bm[e] >= 0)
        at[e][:, M] = alt[e][:, M] - ref[:, bm[e, M]]
    return alt, alt - ref[None], at


def viewpoint_scores_host(maps, ref_map, views, bin_map=None):
    """The viewpoint fields of `ScreenResult` from alt maps [E, n, n] and the reference map [n, n] (host restatement of orca_screen_viewpoints):
    (delta_viewpoint [E, V, n] float32 = alt[view, j] - ref[view, j], the fp32 subtraction; aligned_viewpoint [E, V, n] float32 or None without
    ``bin_map``).  For the aligned form the viewpoint is a REFERENCE bin: with R = the alt bins i with bin_map[e, i] == view (ascending) and
    c = |R|, aligned[e, v, j] = fp32((sum_{i in R} alt[i, j]) / c - ref[view, bin_map[e, j]]) in fp64, the rows added in ascending i, where c >= 1
    and bin_map[e, j] >= 0, else NaN (the viewpoint was deleted, or column j stands for nothing); for c = 1 it is the fp32 subtraction."""
    alt, ref = np.asarray(maps, dtype=np.float32), np.asarray(ref_map, dtype=np.float32)
    E, n = alt.shape[0], ref.shape[0]
    vs = [int(v) for v in views]
    delta = alt[:, vs, :] - ref[None, vs, :]
    if bin_map is None:
        return delta, None
    bm = _bin_maps(bin_map, E, n)
    at = np.full((E, len(vs), n), np.nan, dtype=np.float32)
    for e in range(E):
        cols = np.flatnonzero(bm[e] >= 0)
        for k, v in enumerate(vs):
            R = np.flatnonzero(bm[e] == v)
            if R.size == 1:
                at[e, k, cols] = alt[e, R[0], cols] - ref[v, bm[e, cols]]
            elif R.size > 1:
                s = np.zeros(cols.size)
                for i in R:
                    s = s + alt[e, i, cols].astype(np.float64)
                at[e, k, cols] = (s / float(R.size) - ref[v, bm[e, cols]].astype(np.float64)).astype(np.float32)
    return delta, at


STRATA_FIELDS = ("dist_delta", "dist_abs", "dist_rms", "dist_corr", "mse", "corr", "scc")


def check_strata(strata, n):
    """``strata`` as the stratum range (d_lo, d_hi) of the per-map scores on a map of n bins: True stands for every stratum, (0, n); a pair of
    ints must satisfy 0 <= d_lo < d_hi <= n.  Anything else is a ValueError."""
    if strata is True:
        return 0, n
    try:
        lo, hi = strata
        if isinstance(lo, (bool, np.bool_)) or isinstance(hi, (bool, np.bool_)) or int(lo) != lo or int(hi) != hi:
            raise ValueError
        lo, hi = int(lo), int(hi)
    except (TypeError, ValueError):
        raise ValueError("strata: True (every stratum) or a pair (d_lo, d_hi) of ints") from None
    if not 0 <= lo < hi <= n:
        raise ValueError(f"strata ({lo}, {hi}): 0 <= d_lo < d_hi <= {n} on a map of {n} bins")
    return lo, hi


def strata_scores_host(maps, ref_map, bin_map=None, d_range=None):
    """The distance-stratified scores of `ScreenResult` from alt maps [E, n, n] and the reference map [n, n] (fp64 host restatement of
    orca_screen_strata_scores): a dict of fp64 arrays ``dist_delta``, ``dist_abs``, ``dist_rms``, ``dist_corr`` [E, n], ``mse``, ``corr``, ``scc``
    [E], and ``dist_count`` [E, n] int32 (also without ``bin_map``: n - d then).  Stratum d is the pairs (i, i + d); x = the alt pixel, y =
    ref[i, i + d] or, with ``bin_map`` ([E, n], or one [n] for all), ref[map i, map (i + d)] over the pairs whose two bins are mapped - the stratum
    is the ALT distance, an unmapped pair is never read.  The same two passes as the kernel, each for i ascending from 0.0: the means mx_d, my_d
    (one division by c_d), then X_d = sum (x - mx_d)^2, Y_d = sum (y - my_d)^2, C_d = sum (x - mx_d)(y - my_d) and sum dl, sum |dl|, sum dl^2 of
    dl = x - y.  dist_delta / dist_abs / dist_rms = the mean of dl, of |dl|, and the root of the mean of dl^2; dist_corr = C_d / sqrt(X_d Y_d), NaN
    when c_d < 2, X_d == 0 or Y_d == 0; all NaN where c_d = 0.  Over the strata ``d_range`` = (d_lo, d_hi) (all by default), serially for d
    ascending, c = sum c_d: mse = sum sum dl^2 / c; scc = sum C_d / sum sqrt(X_d Y_d) (HiCRep's stratum-adjusted correlation on raw values), NaN
    when the denominator is 0; corr = the Pearson correlation of all those pairs from the pooled sums, mx = (sum c_d mx_d) / c,
    X = sum [X_d + c_d (mx_d - mx)^2], C = sum [C_d + c_d (mx_d - mx)(my_d - my)], NaN when X or Y is 0 or c < 2; all three NaN when c = 0."""
    a, r = np.asarray(maps, dtype=np.float64), np.asarray(ref_map, dtype=np.float64)
    E, n = a.shape[0], r.shape[0]
    if a.shape != (E, n, n) or r.shape != (n, n):
        raise ValueError("maps [E, n, n], ref_map [n, n]")
    lo, hi = check_strata(True if d_range is None else d_range, n)
    bm = None if bin_map is None else _bin_maps(bin_map, E, n)

    def pairs(i):                                        # row i's pairs (i, i + d), d = 0 .. n - 1 - i: x [E, w], y [E, w], whether the pair counts
        x = a[:, i, i:]
        if bm is None:
            return x, np.broadcast_to(r[i, i:], x.shape), np.ones(x.shape, dtype=bool)
        mi, mj = bm[:, i: i + 1], bm[:, i:]
        ok = (mi >= 0) & (mj >= 0)
        return x, r[np.where(ok, mi, 0), np.where(ok, mj, 0)], ok
    cnt = np.zeros((E, n), dtype=np.int64)
    sx, sy = np.zeros((E, n)), np.zeros((E, n))
    for i in range(n):                                   # adding 0.0 for a pair that does not count leaves a sum as it is
        x, y, ok = pairs(i)
        sx[:, : n - i] += np.where(ok, x, 0.0)
        sy[:, : n - i] += np.where(ok, y, 0.0)
        cnt[:, : n - i] += ok
    X, Y, C, sd, sa, sq = (np.zeros((E, n)) for _ in range(6))
    with np.errstate(invalid="ignore", divide="ignore"):
        c = cnt.astype(np.float64)
        mx, my = sx / c, sy / c
        for i in range(n):
            x, y, ok = pairs(i)
            ex, ey, dl = x - mx[:, : n - i], y - my[:, : n - i], x - y
            for acc, v in ((X, ex * ex), (Y, ey * ey), (C, ex * ey), (sd, dl), (sa, np.abs(dl)), (sq, dl * dl)):
                acc[:, : n - i] += np.where(ok, v, 0.0)
        out = {"dist_delta": sd / c, "dist_abs": sa / c, "dist_rms": np.sqrt(sq / c), "dist_count": cnt.astype(np.int32)}
        out["dist_corr"] = np.where((cnt < 2) | (X == 0.0) | (Y == 0.0), np.nan, C / np.sqrt(X * Y))
        some = cnt > 0                                   # empty strata are skipped
        tot = np.zeros(E, dtype=np.int64)
        q, num, den, wx, wy = (np.zeros(E) for _ in range(5))
        for d in range(lo, hi):
            tot += cnt[:, d]
            for acc, v in ((q, sq[:, d]), (num, C[:, d]), (den, np.sqrt(X[:, d] * Y[:, d])), (wx, c[:, d] * mx[:, d]), (wy, c[:, d] * my[:, d])):
                acc += np.where(some[:, d], v, 0.0)
        t = tot.astype(np.float64)
        pmx, pmy = wx / t, wy / t
        PX, PY, PC = (np.zeros(E) for _ in range(3))
        for d in range(lo, hi):
            ex, ey = mx[:, d] - pmx, my[:, d] - pmy
            for acc, v in ((PX, X[:, d] + c[:, d] * (ex * ex)), (PY, Y[:, d] + c[:, d] * (ey * ey)), (PC, C[:, d] + c[:, d] * (ex * ey))):
                acc += np.where(some[:, d], v, 0.0)
        out["mse"] = q / t
        out["scc"] = np.where((tot == 0) | (den == 0.0), np.nan, num / den)
        out["corr"] = np.where((tot < 2) | (PX == 0.0) | (PY == 0.0), np.nan, PC / np.sqrt(PX * PY))
    return out


# ---- loops: dot calls (orca_screen_dot_calls, orca_screen_dot_enrichment) ---------------------------------------------------------------------
LOOP_MAX_W, LOOP_MAX_R, LOOP_MAX_CALLS = 16, 16, 4096
LOOP_FIELDS = ("loop_delta", "loops_gained", "loops_lost", "loop_is_gained", "ref_loop_is_lost")


@dataclass(frozen=True)
class LoopParams:
    """The parameters of the dot (loop) calls of ``screen_1m(..., loops=)``; include/orca_hip.h (orca_screen_dot_calls) defines what they mean.
      p          peak half-width: the peak set P is the (2 p + 1)^2 pixels around (i, j)
      w          window half-width of the HiCCUPS sets D, LL, H, V; 0 <= p < w <= 16
      r          a dot is the local maximum of the enrichment within Chebyshev distance r; 1 <= r <= 16
      threshold  a dot has enrichment e >= threshold (compared in fp32).  The maps are log observed / expected, so e is a log fold enrichment
                 of the peak over its strongest local background.  The default, 0.25, is NOT calibrated on the published checkpoints - nobody
                 on this project has them; choose it from ``ref_loop_enrichment`` and known loops of the cell type
      d_min      the smallest distance j - i of a pixel that can be called; None = 2 w + 1, the smallest at which every set lies strictly
                 above the diagonal
      max_calls  K, the dots listed per map (row-major order; ``loop_count`` still counts all); 1 <= K <= 4096
      tol        an alt dot matches a reference dot when their Chebyshev distance is <= tol bins (``loops_gained`` / ``loops_lost``)"""
    p: int = 1
    w: int = 4
    r: int = 2
    threshold: float = 0.25
    d_min: Optional[int] = None
    max_calls: int = 64
    tol: int = 1


def _loop_params(params):
    """``params`` (a `LoopParams`) validated, with ``d_min`` resolved and ``threshold`` as the fp32 the kernel compares with."""
    if not isinstance(params, LoopParams):
        raise ValueError("loops: True (the defaults) or a screen.LoopParams")
    vals = {}
    for k in ("p", "w", "r", "d_min", "max_calls", "tol"):
        v = getattr(params, k)
        if k == "d_min" and v is None:
            continue
        if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, np.integer)):
            raise ValueError(f"loops: {k} = {v!r} must be an int")
        vals[k] = int(v)
    p, w = vals["p"], vals["w"]
    if not 0 <= p < w <= LOOP_MAX_W:
        raise ValueError(f"loops: p = {p}, w = {w}: 0 <= p < w <= {LOOP_MAX_W}")
    if not 1 <= vals["r"] <= LOOP_MAX_R:
        raise ValueError(f"loops: r = {vals['r']}: 1 .. {LOOP_MAX_R}")
    d_min = vals.get("d_min", 2 * w + 1)
    if d_min < 2 * w + 1:
        raise ValueError(f"loops: d_min = {d_min} below 2 w + 1 = {2 * w + 1} (the sets must stay above the diagonal)")
    if not 1 <= vals["max_calls"] <= LOOP_MAX_CALLS:
        raise ValueError(f"loops: max_calls = {vals['max_calls']}: 1 .. {LOOP_MAX_CALLS}")
    if vals["tol"] < 0:
        raise ValueError(f"loops: tol = {vals['tol']} must not be negative")
    try:
        t = float(np.float32(params.threshold))
    except (TypeError, ValueError):
        raise ValueError("loops: threshold must be a number") from None
    if isinstance(params.threshold, (bool, np.bool_)) or t != t:
        raise ValueError("loops: threshold must be a number, not NaN")
    return LoopParams(p, w, vals["r"], t, d_min, vals["max_calls"], vals["tol"])


def check_loops(loops, n):
    """``loops`` as a validated `LoopParams` for a map of n bins: True stands for the defaults, ``d_min=None`` becomes 2 w + 1.  A ValueError
    for anything that is not True or a `LoopParams`, for values outside their ranges (0 <= p < w <= 16, 1 <= r <= 16, d_min >= 2 w + 1,
    1 <= max_calls <= 4096, tol >= 0, threshold not NaN) and when no pixel of an n-bin map is eligible (n < 2 w + 1 + d_min)."""
    q = _loop_params(LoopParams() if loops is True else loops)
    if n < 2 * q.w + 1 + q.d_min:
        raise ValueError(f"loops: a map of {n} bins has no eligible pixel at w = {q.w}, d_min = {q.d_min} (n >= 2 w + 1 + d_min = {2 * q.w + 1 + q.d_min})")
    return q


def check_band_loops(loops, N, D):
    """``loops`` as a validated `LoopParams` for a band of N bins x D distances (``scan.scan_1m(..., loops=)``): `check_loops`' ranges, and a
    ValueError when no band pixel is eligible - pixel (i, d) needs w <= i, i + d <= N - 1 - w and d_min <= d <= D - 1 - 2 w, so D >= d_min + 2 w + 1
    and N >= d_min + 2 w + 1.  ``max_calls`` and ``tol`` are checked and unused: nothing is capped or matched on a band."""
    q = _loop_params(LoopParams() if loops is True else loops)
    need = q.d_min + 2 * q.w + 1
    if int(D) < need or int(N) < need:
        raise ValueError(f"loops: a band of {int(N)} bins x {int(D)} distances has no eligible pixel at w = {q.w}, d_min = {q.d_min} "
                         f"(N >= d_min + 2 w + 1 = {need} and D >= {need})")
    return q


def check_loops_arg(loops, n):
    """A screen's ``loops`` argument, checked for maps of n bins: None when unset (None or False), else `check_loops`' validated `LoopParams`."""
    return None if loops is None or loops is False else check_loops(loops, n)


def _dot_enrichment_of(view, p, w):
    """e (float32) of a block of pixels whose windows are all readable: ``view(a, b)`` is the fp64 array of the block's pixels shifted by the window
    offset (a, b), |a|, |b| <= w.  The one numpy statement of the sets and of the order of the sums (a ascending, then b ascending), for a dense map
    (`dot_enrichment_host`) and for a band (`scan.band_dot_enrichment_host`)."""
    sums, cnt = dict.fromkeys("PDLHV", 0.0), dict.fromkeys("PDLHV", 0)
    for a in range(-w, w + 1):
        for b in range(-w, w + 1):
            x = view(a, b)
            sets = []
            if abs(a) <= p and abs(b) <= p:
                sets.append("P")
            else:
                if a != 0 and b != 0:
                    sets.append("D")
                if a >= 1 and b <= -1:
                    sets.append("L")
            if abs(a) <= 1 and abs(b) > p:
                sets.append("H")
            if abs(b) <= 1 and abs(a) > p:
                sets.append("V")
            for k in sets:
                sums[k] = sums[k] + x
                cnt[k] += 1
    mean = {k: sums[k] / float(cnt[k]) for k in "PDLHV"}
    nan = np.isnan(mean["P"])
    for k in "DLHV":
        nan = nan | np.isnan(mean[k])
    with np.errstate(invalid="ignore"):
        bg = mean["D"]
        for k in "LHV":
            bg = np.where(mean[k] > bg, mean[k], bg)
        return np.where(nan, np.nan, mean["P"] - bg).astype(np.float32)


def dot_enrichment_host(maps, params):
    """The enrichment e of maps [E, n, n] at every pixel (host restatement of the device function behind orca_screen_dot_calls): float32
    [E, n, n], NaN at the ineligible pixels.  Pixel (i, j) is eligible when w <= i, j <= n - 1 - w and j - i >= d_min.  Over the offsets (a, b),
    |a|, |b| <= w: P = |a| <= p and |b| <= p; D = not P, a != 0 and b != 0; LL = 1 <= a, b <= -1, not P; H = |a| <= 1 and |b| > p; V = |b| <= 1
    and |a| > p.  e = mean P - max(mean D, mean LL, mean H, mean V), every set summed on its own in fp64 (a ascending, then b ascending), one
    division by its count, rounded to fp32 once; NaN when any set holds a NaN.  Nothing on or below the diagonal enters an eligible pixel."""
    q = _loop_params(params)
    m = np.asarray(maps, dtype=np.float32)
    if m.ndim != 3 or m.shape[1] != m.shape[2]:
        raise ValueError("maps: [E, n, n]")
    E, n = m.shape[0], m.shape[1]
    p, w, d_min = q.p, q.w, q.d_min
    out = np.full((E, n, n), np.nan, dtype=np.float32)
    c = n - 2 * w                                        # the pixels whose window is inside the map: rows and columns w .. n - 1 - w
    if c <= 0 or n < 2 * w + 1 + d_min:
        return out
    m64 = m.astype(np.float64)
    e = _dot_enrichment_of(lambda a, b: m64[:, w + a: w + a + c, w + b: w + b + c], p, w)
    i = np.arange(w, n - w)
    e[:, ~(i[None, :] - i[:, None] >= d_min)] = np.nan
    out[:, w: n - w, w: n - w] = e
    return out


def dot_calls_host(maps, params):
    """The dot calls of maps [E, n, n] (host restatement of orca_screen_dot_calls): a dict of ``count`` [E] int32 (all dots), ``ij`` [E, K, 2] int32
    and ``enrich`` [E, K] float32 (the first K = max_calls dots in row-major order, -1 / NaN behind them) and ``e_map`` = `dot_enrichment_host`.
    (i, j) is a dot when e is not NaN, e >= threshold and, for every pixel within Chebyshev distance r whose e' is not NaN,
    e > e' where that pixel precedes (i, j) in row-major order and e >= e' where it follows; all in fp32."""
    q = _loop_params(params)
    e = dot_enrichment_host(maps, q)
    E, n = e.shape[0], e.shape[1]
    r, K, T = q.r, q.max_calls, np.float32(q.threshold)
    pad = np.full((E, n + 2 * r, n + 2 * r), np.nan, dtype=np.float32)
    pad[:, r: r + n, r: r + n] = e
    with np.errstate(invalid="ignore"):
        dot = ~np.isnan(e) & (e >= T)
        for di in range(-r, r + 1):
            for dj in range(-r, r + 1):
                if di == 0 and dj == 0:
                    continue
                f = pad[:, r + di: r + di + n, r + dj: r + dj + n]
                wins = (e > f) if (di < 0 or (di == 0 and dj < 0)) else (e >= f)
                dot &= np.isnan(f) | wins
    count = dot.reshape(E, -1).sum(axis=1).astype(np.int32)
    ij = np.full((E, K, 2), -1, dtype=np.int32)
    enrich = np.full((E, K), np.nan, dtype=np.float32)
    for k in range(E):
        at = np.argwhere(dot[k])[:K]                     # row-major
        ij[k, : len(at)] = at
        enrich[k, : len(at)] = e[k, at[:, 0], at[:, 1]]
    return {"count": count, "ij": ij, "enrich": enrich, "e_map": e}


def follow_loop(bin_map_row, i, j, params):
    """Where the reference pixel (i, j) went in an alt map with bin map ``bin_map_row`` [n]: (a, b) with a the LOWEST alt bin that stands for
    reference bin i and b the HIGHEST that stands for j - the anchors' outer edges, should an insertion have left two alt bins on one reference
    bin.  (-1, -1) when either reference bin is behind no alt bin (the anchor was deleted or pushed out) or (a, b) is not an eligible pixel."""
    q = _loop_params(params)
    bm = np.asarray(bin_map_row)
    n = bm.shape[0]
    ia, jb = np.flatnonzero(bm == i), np.flatnonzero(bm == j)
    if i < 0 or j < 0 or not ia.size or not jb.size:
        return -1, -1
    a, b = int(ia[0]), int(jb[-1])
    if not (a >= q.w and b <= n - 1 - q.w and b - a >= q.d_min):
        return -1, -1
    return a, b


def _follow_loops(bin_maps, ref_ij, q):
    """`follow_loop` of every reference dot ``ref_ij`` [R, 2] under every row of ``bin_maps`` [E, n]: int32 [E, R, 2]."""
    bm = np.asarray(bin_maps)
    E, n = bm.shape
    out = np.full((E, ref_ij.shape[0], 2), -1, dtype=np.int32)
    if not ref_ij.shape[0]:
        return out
    ident = (bm == np.arange(n)[None]).all(axis=1)       # most items of a screen keep their length: every dot stays where it is
    ri, rj = ref_ij[:, 0].astype(np.int64), ref_ij[:, 1].astype(np.int64)
    out[ident] = np.where(((ri >= q.w) & (rj <= n - 1 - q.w) & (rj - ri >= q.d_min))[:, None], ref_ij, -1)[None]
    for e in np.flatnonzero(~ident):
        idx = np.flatnonzero(bm[e] >= 0)
        first, last = np.full(n, -1), np.full(n, -1)
        first[bm[e, idx[::-1]]] = idx[::-1]              # written in descending order: the lowest alt bin stays
        last[bm[e, idx]] = idx
        a, b = first[ref_ij[:, 0]], last[ref_ij[:, 1]]
        ok = (a >= q.w) & (b >= 0) & (b <= n - 1 - q.w) & (b - a >= q.d_min)
        out[e, ok, 0], out[e, ok, 1] = a[ok], b[ok]
    return out


def match_loops_host(alt_ij, ref_ij, tol, bin_map_row=None):
    """Match the listed dots of an alt map, ``alt_ij`` [K, 2] (-1 rows are padding), to the reference's, ``ref_ij`` [R, 2]: (is_gained [K] bool,
    is_lost [R] bool).  An alt dot matches a reference dot when their Chebyshev distance is <= ``tol``; gained = a listed alt dot that matches
    none, lost = a reference dot that no alt dot matches.  With ``bin_map_row`` [n] an alt dot (a, b) stands for (map a, map b) before it is
    compared; if either bin is unmapped it is gained and matches nothing."""
    alt, ref = np.asarray(alt_ij, dtype=np.int64).reshape(-1, 2), np.asarray(ref_ij, dtype=np.int64).reshape(-1, 2)
    listed = alt[:, 0] >= 0
    ok = listed.copy()
    if bin_map_row is not None:
        bm = np.asarray(bin_map_row, dtype=np.int64)
        alt = np.where(listed[:, None], bm[np.where(listed[:, None], alt, 0)], -1)
        ok = listed & (alt >= 0).all(axis=1)
    near = (np.abs(alt[:, None, :] - ref[None, :, :]).max(axis=2) <= int(tol)) & ok[:, None]       # [K, R]
    return listed & ~near.any(axis=1), ~near.any(axis=0)


def _match_loops(alt_ij, ref_ij, tol, bin_maps=None):
    """`match_loops_host` of every item at once: ``alt_ij`` [E, K, 2], ``ref_ij`` [R, 2], ``bin_maps`` [E, n] or None -> (is_gained [E, K], is_lost [E, R])."""
    alt, ref = np.asarray(alt_ij, dtype=np.int32), np.asarray(ref_ij, dtype=np.int32).reshape(-1, 2)
    E, K, R = alt.shape[0], alt.shape[1], ref.shape[0]
    listed = alt[:, :, 0] >= 0
    ok = listed
    if bin_maps is not None:
        bm = np.asarray(bin_maps, dtype=np.int32)
        alt = np.where(listed[:, :, None], np.take_along_axis(bm, np.where(listed[:, :, None], alt, 0).reshape(E, 2 * K), axis=1).reshape(E, K, 2), -1)
        ok = listed & (alt >= 0).all(axis=2)
    if not R or not E:
        return listed.copy(), np.zeros((E, R), dtype=bool) if not R else np.ones((E, R), dtype=bool)
    gained, lost = np.zeros((E, K), dtype=bool), np.zeros((E, R), dtype=bool)
    step = max(1, (1 << 22) // (K * R))                  # items per pass: [step, K, R] temporaries of a few MB
    for e0 in range(0, E, step):
        a = alt[e0: e0 + step]
        near = ok[e0: e0 + step, :, None]
        for c in range(2):                               # Chebyshev distance <= tol, coordinate by coordinate
            near = near & (np.abs(a[:, :, c, None] - ref[None, None, :, c]) <= int(tol))
        gained[e0: e0 + step], lost[e0: e0 + step] = listed[e0: e0 + step] & ~near.any(axis=2), ~near.any(axis=1)
    return gained, lost


def loop_scores_host(maps, ref_map, params, bin_map=None):
    """Every loop field of `ScreenResult` from alt maps [E, n, n] and the reference map [n, n] (host restatement of ``screen_1m(..., loops=)``): a
    dict of ``ref_loop_count`` (int, all dots of the reference), ``ref_loops`` [R, 2] int32 and ``ref_loop_enrichment`` [R] float32 (the listed
    ones, R = min(count, K)), ``loops`` [E, K, 2] int32, ``loop_enrichment`` [E, K] float32, ``loop_count`` [E] int32, ``loop_delta`` [E, R] float32
    (e of the alt map at the reference dot's pixel minus the reference's e there, an fp32 subtraction; NaN where the alt e is), ``loops_gained``,
    ``loops_lost`` [E] int32 and the masks ``loop_is_gained`` [E, K], ``ref_loop_is_lost`` [E, R] (`match_loops_host`); with ``bin_map`` ([E, n],
    or one [n] for all) also their ``aligned_`` forms: the reference dot followed to its alt pixel (`follow_loop`; NaN when it has none) and the
    alt dots matched through the bin map."""
    q = _loop_params(params)
    alt = np.asarray(maps, dtype=np.float32)
    E, n = alt.shape[0], alt.shape[1]
    rc = dot_calls_host(np.asarray(ref_map, dtype=np.float32)[None], q)
    R = min(int(rc["count"][0]), q.max_calls)
    ref_ij, ref_e = rc["ij"][0, :R], rc["enrich"][0, :R]
    ac = dot_calls_host(alt, q)
    out = {"ref_loop_count": int(rc["count"][0]), "ref_loops": ref_ij, "ref_loop_enrichment": ref_e, "loops": ac["ij"], "loop_enrichment": ac["enrich"],
           "loop_count": ac["count"]}
    bms = None if bin_map is None else _bin_maps(bin_map, E, n)
    for pre in ("", "aligned_") if bms is not None else ("",):
        delta = np.full((E, R), np.nan, dtype=np.float32)
        gained, lost = np.zeros((E, q.max_calls), dtype=bool), np.zeros((E, R), dtype=bool)
        for e in range(E):
            for k in range(R):
                a, b = (int(ref_ij[k, 0]), int(ref_ij[k, 1])) if not pre else follow_loop(bms[e], int(ref_ij[k, 0]), int(ref_ij[k, 1]), q)
                if a >= 0:
                    delta[e, k] = ac["e_map"][e, a, b] - ref_e[k]
            gained[e], lost[e] = match_loops_host(ac["ij"][e], ref_ij, q.tol, bms[e] if pre else None)
        out[pre + "loop_delta"], out[pre + "loop_is_gained"], out[pre + "ref_loop_is_lost"] = delta, gained, lost
        out[pre + "loops_gained"], out[pre + "loops_lost"] = gained.sum(axis=1).astype(np.int32), lost.sum(axis=1).astype(np.int32)
    return out


# ---- boundaries: domain boundary calls from the insulation tracks (orca_screen_boundary_calls) --------------------------------------------------
BOUNDARY_MIN_BINS, BOUNDARY_MAX_BINS = 3, 256
BOUNDARY_MATCH_FIELDS = ("boundary_followed_at", "boundary_strength_delta", "boundary_delta", "boundary_is_gained", "ref_boundary_is_lost",
                         "boundary_is_unmapped", "ref_boundary_is_unmapped", "boundaries_gained", "boundaries_lost")


@dataclass(frozen=True)
class BoundaryParams:
    """The parameters of the boundary calls of ``screen_1m(..., insulation=, boundaries=)`` and ``sv_screen(..., insulation=, boundaries=)``;
    include/orca_hip.h (orca_screen_boundary_calls) defines a minimum, its strength and a call.
      min_strength  a boundary is a minimum of the insulation track whose strength - the prominence of the dip, in the track's unit, mean log
                    observed / expected - is > 0 and >= min_strength (compared in fp32); >= 0.  The default, 0.1, is NOT calibrated on the
                    published checkpoints - nobody on this project has them; choose it from ``ref_boundary_strength`` (run once with
                    ``min_strength=0.0``) and known boundaries of the cell type
      max_calls     K, the boundaries listed per track, in ascending bin order (``boundary_count`` still counts all); 1 <= K <= n
      tol           an alt boundary matches a reference boundary when the reference bin it stands for is within tol bins of it; >= 0"""
    min_strength: float = 0.1
    max_calls: int = 32
    tol: int = 1


def check_boundaries(boundaries, n):
    """``boundaries`` as a validated `BoundaryParams` for tracks of n bins (3 <= n <= 256): True stands for the defaults; ``min_strength`` comes back
    as the fp32 the kernel compares with.  A ValueError for anything that is not True or a `BoundaryParams` and for values outside their ranges
    (min_strength a number >= 0 and not NaN, 1 <= max_calls <= n, tol >= 0, both ints)."""
    q = BoundaryParams() if boundaries is True else boundaries
    if not isinstance(q, BoundaryParams):
        raise ValueError("boundaries: True (the defaults) or a screen.BoundaryParams")
    if not BOUNDARY_MIN_BINS <= int(n) <= BOUNDARY_MAX_BINS:
        raise ValueError(f"boundaries: tracks of {n} bins ({BOUNDARY_MIN_BINS} .. {BOUNDARY_MAX_BINS})")
    for k in ("max_calls", "tol"):
        v = getattr(q, k)
        if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, np.integer)):
            raise ValueError(f"boundaries: {k} = {v!r} must be an int")
    if not 1 <= q.max_calls <= int(n):
        raise ValueError(f"boundaries: max_calls = {q.max_calls}: 1 .. {int(n)} on tracks of {int(n)} bins")
    if q.tol < 0:
        raise ValueError(f"boundaries: tol = {q.tol} must not be negative")
    try:
        s = float(np.float32(q.min_strength))
    except (TypeError, ValueError):
        raise ValueError("boundaries: min_strength must be a number") from None
    if isinstance(q.min_strength, (bool, np.bool_)) or not s >= 0.0:
        raise ValueError(f"boundaries: min_strength = {q.min_strength!r} must be a number >= 0, not NaN")
    return BoundaryParams(s, int(q.max_calls), int(q.tol))


def check_boundaries_arg(boundaries, n, insulation):
    """A screen's ``boundaries`` argument, checked for tracks of n bins: None when unset (None or False), else `check_boundaries`' validated
    `BoundaryParams`.  ``insulation``: the screen's insulation argument - the boundaries are called on the insulation tracks, so without them
    (None) it is a ValueError."""
    if boundaries is None or boundaries is False:
        return None
    if insulation is None:
        raise ValueError("boundaries: called on the insulation tracks (insulation=widths)")
    return check_boundaries(boundaries, n)


def boundary_strength_host(track):
    """The strength track of one insulation track [n] (host restatement of orca_screen_boundary_calls' ``strength_track``): float32 [n], the strength
    at every minimum with strength > 0, NaN elsewhere.  Bin i is a minimum when 1 <= i <= n - 2, t[i - 1], t[i], t[i + 1] are not NaN, t[i] <
    t[i - 1] and t[i] <= t[i + 1]; walking left from i - 1 while the bin exists, is not NaN and is >= t[i], L = the largest value met (t[i] if none),
    R the same to the right; strength = min(L, R) - t[i], one fp32 subtraction.  A NaN ends a walk: nothing is bridged across it."""
    t = np.asarray(track, dtype=np.float32)
    if t.ndim != 1:
        raise ValueError("track: [n]")
    n = t.shape[0]
    out = np.full(n, np.nan, dtype=np.float32)
    ok = ~np.isnan(t)
    for i in range(1, n - 1):
        v = t[i]
        if not (ok[i - 1] and ok[i] and ok[i + 1] and v < t[i - 1] and v <= t[i + 1]):
            continue
        side = []
        for step in (-1, 1):
            best, j = v, i + step
            while 0 <= j < n and t[j] >= v:              # False for a NaN
                if t[j] > best:
                    best = t[j]
                j += step
            side.append(best)
        s = np.float32(min(side[0], side[1])) - v
        if s > 0:
            out[i] = s
    return out


def boundary_calls_host(tracks, params):
    """The boundary calls of insulation tracks [..., n] (host restatement of orca_screen_boundary_calls; ``params``: a `BoundaryParams` or True): a
    dict of ``count`` [...] int32 (all boundaries of the track), ``bins`` [..., K] int32 and ``strength`` [..., K] float32 (the first K = max_calls
    boundaries in ascending bin order, -1 / NaN behind them) and ``strength_track`` [..., n] float32 (`boundary_strength_host`).  A boundary is a
    minimum with strength > 0 and strength >= min_strength, compared in fp32."""
    t = np.asarray(tracks, dtype=np.float32)
    if t.ndim < 1:
        raise ValueError("tracks: [..., n]")
    lead, n = t.shape[:-1], t.shape[-1]
    q = check_boundaries(params, n)
    K, T = q.max_calls, np.float32(q.min_strength)
    flat = t.reshape(-1, n)
    P = flat.shape[0]
    count, bins = np.zeros(P, dtype=np.int32), np.full((P, K), -1, dtype=np.int32)
    strength, st = np.full((P, K), np.nan, dtype=np.float32), np.full((P, n), np.nan, dtype=np.float32)
    for p in range(P):
        st[p] = boundary_strength_host(flat[p])
        with np.errstate(invalid="ignore"):
            at = np.flatnonzero(st[p] >= T)              # the track holds strengths > 0 only; NaN compares False
        count[p] = at.size
        bins[p, : min(at.size, K)] = at[:K]
        strength[p, : min(at.size, K)] = st[p, at[:K]]
    return {"count": count.reshape(lead), "bins": bins.reshape(lead + (K,)), "strength": strength.reshape(lead + (K,)),
            "strength_track": st.reshape(lead + (n,))}


def match_boundaries_host(alt_bins, alt_strength, ref_bins, ref_strength, alt_track, ref_track, tol, bin_map_row=None):
    """Match the listed boundaries of ONE alt track to its reference track's, plainly (the loops below state the rule; `_match_boundaries` is the
    batched form the screens run).  ``alt_bins`` [K] / ``ref_bins`` [R] int32 (-1 = an empty slot) with their strengths, ``alt_track`` /
    ``ref_track`` [n] the insulation tracks the lists were called on, ``bin_map_row`` [n] the reference bin every alt bin stands for, -1 for none
    (None = the identity).  With map = the bin map:
      - an alt boundary at alt bin a stands for reference bin map[a]; it is MAPPED when map[a] >= 0 and ref_track[map[a]] is not NaN;
      - a reference boundary r is MAPPED when some alt bin a has map[a] >= 0, |map[a] - r| <= tol and alt_track[a] not NaN - something of the alt
        allele stands where it was, and the alt track can be read there;
      - r MATCHES a listed alt boundary a when map[a] >= 0 and |map[a] - r| <= tol (symmetric: a descending map needs no special case); its PARTNER
        is the matching alt boundary of largest strength, the lower alt bin of equals;
      - lost = a mapped reference boundary without a partner; gained = a mapped alt boundary that matches no listed reference boundary; an
        unmapped one is neither - a boundary that left the window, or sits in inserted sequence, is not a false call.
    A dict of ``followed_at`` [R] int32 (the partner's alt bin, -1 without), ``strength_delta`` [R] float32 (the partner's strength - the reference
    strength, one fp32 subtraction; -the reference strength when lost; NaN when unmapped or the slot is empty), ``is_lost``, ``ref_is_unmapped``
    [R] bool, ``is_gained``, ``is_unmapped`` [K] bool."""
    ab, rb = np.asarray(alt_bins, dtype=np.int64).reshape(-1), np.asarray(ref_bins, dtype=np.int64).reshape(-1)
    a_s, r_s = np.asarray(alt_strength, dtype=np.float32).reshape(-1), np.asarray(ref_strength, dtype=np.float32).reshape(-1)
    ta, tr = np.asarray(alt_track, dtype=np.float32), np.asarray(ref_track, dtype=np.float32)
    n, tol = ta.shape[0], int(tol)
    bm = np.arange(n, dtype=np.int64) if bin_map_row is None else np.asarray(bin_map_row, dtype=np.int64)
    K, R = ab.shape[0], rb.shape[0]
    out = {"followed_at": np.full(R, -1, dtype=np.int32), "strength_delta": np.full(R, np.nan, dtype=np.float32), "is_lost": np.zeros(R, dtype=bool),
           "ref_is_unmapped": np.zeros(R, dtype=bool), "is_gained": np.zeros(K, dtype=bool), "is_unmapped": np.zeros(K, dtype=bool)}
    matched = np.zeros(K, dtype=bool)
    for k in range(R):
        r = int(rb[k])
        if r < 0:
            continue
        best = -1
        for j in range(K):
            a = int(ab[j])
            if a >= 0 and bm[a] >= 0 and abs(int(bm[a]) - r) <= tol:
                matched[j] = True
                if best < 0 or a_s[j] > a_s[best] or (a_s[j] == a_s[best] and a < int(ab[best])):
                    best = j
        mapped = any(bm[a] >= 0 and abs(int(bm[a]) - r) <= tol and not np.isnan(ta[a]) for a in range(n))
        if best >= 0:
            out["followed_at"][k], out["strength_delta"][k] = ab[best], a_s[best] - r_s[k]
        elif mapped:
            out["is_lost"][k], out["strength_delta"][k] = True, -r_s[k]
        else:
            out["ref_is_unmapped"][k] = True
    for j in range(K):
        a = int(ab[j])
        if a < 0:
            continue
        mapped = bm[a] >= 0 and not np.isnan(tr[bm[a]])
        out["is_unmapped"][j] = not mapped
        out["is_gained"][j] = mapped and not matched[j]
    return out


def _match_boundaries(alt_bins, alt_strength, ref_bins, ref_strength, alt_track, ref_track, tol, bin_map=None):
    """`match_boundaries_host` of P pairs at once: ``alt_bins`` / ``alt_strength`` [P, K], ``ref_bins`` / ``ref_strength`` [P, R], ``alt_track`` /
    ``ref_track`` [P, n], ``bin_map`` [P, n] or None (the identity) -> its dict with a leading P, plus ``first_at`` [P, R] int32: the lowest alt bin
    that stands for the reference boundary's own bin, -1 for none."""
    ab, rb = np.asarray(alt_bins, dtype=np.int32), np.asarray(ref_bins, dtype=np.int32)
    a_s, r_s = np.asarray(alt_strength, dtype=np.float32), np.asarray(ref_strength, dtype=np.float32)
    ta, tr = np.asarray(alt_track, dtype=np.float32), np.asarray(ref_track, dtype=np.float32)
    (P, K), R, n, tol = ab.shape, rb.shape[1], ta.shape[1], int(tol)
    rows = np.arange(P)[:, None]
    a_listed, r_listed = ab >= 0, rb >= 0
    r_safe = np.where(r_listed, rb, 0)
    has = np.zeros((P, n + 2 * tol), dtype=bool)                                                  # per reference bin (offset tol): a readable alt bin stands for it
    if bin_map is None:                                                                           # the identity: every bin stands for itself
        m, first_at = np.where(a_listed, ab, -1), np.where(r_listed, rb, -1)
        has[:, tol: tol + n] = ~np.isnan(ta)
    else:
        bm = np.asarray(bin_map, dtype=np.int32)
        m = np.where(a_listed, bm[rows, np.where(a_listed, ab, 0)], -1)                           # the reference bin every listed alt boundary stands for
        pr, pa = np.nonzero((bm >= 0) & ~np.isnan(ta))                                            # readable: stands for a reference bin and has a track value
        has[pr, bm[pr, pa] + tol] = True
        first = np.full((P, n), -1, dtype=np.int32)
        pr, pa = np.nonzero(bm >= 0)
        first[pr[::-1], bm[pr[::-1], pa[::-1]]] = pa[::-1]                                        # written in descending order: the lowest alt bin stays
        first_at = np.where(r_listed, first[rows, r_safe], -1)
    a_mapped = a_listed & (m >= 0) & ~np.isnan(tr[rows, np.where(m >= 0, m, 0)])
    near = np.zeros((P, n), dtype=bool)
    for d in range(2 * tol + 1):
        near |= has[:, d: d + n]
    r_mapped = r_listed & near[rows, r_safe]
    with np.errstate(invalid="ignore"):                                                           # what holds without a single match
        out = {"followed_at": np.full((P, R), -1, dtype=np.int32), "strength_delta": np.where(r_mapped, -r_s, np.float32(np.nan)).astype(np.float32),
               "is_gained": a_mapped.copy(), "first_at": first_at.astype(np.int32)}
    has_partner = np.zeros((P, R), dtype=bool)
    Ku, Ru = (int(np.flatnonzero(x.any(axis=0)).max(initial=-1)) + 1 for x in (a_listed, r_listed))      # the slots that some pair uses: the lists are mostly short
    step = max(1, (1 << 21) // max(1, Ku * Ru))                                                   # pairs per pass: [step, Ru, Ku] temporaries of a few MB
    for p0 in range(0, P if Ku and Ru else 0, step):
        s = slice(p0, p0 + step)
        mk, rk, sk = m[s, None, :Ku], rb[s, :Ru, None], a_s[s, :Ku]
        match = (r_listed[s, :Ru, None] & (mk >= 0)) & (np.abs(mk - rk) <= tol)                   # [p, Ru, Ku]
        with np.errstate(invalid="ignore"):
            best = np.where(match, sk[:, None, :], -np.inf).argmax(axis=2)                        # the first of equals: the lists ascend, so the lower alt bin
        hp = match.any(axis=2)
        pk = np.arange(match.shape[0])[:, None]
        has_partner[s, :Ru] = hp
        out["followed_at"][s, :Ru] = np.where(hp, ab[s][pk, best], -1)
        with np.errstate(invalid="ignore"):
            out["strength_delta"][s, :Ru] = np.where(hp, sk[pk, best] - r_s[s, :Ru], out["strength_delta"][s, :Ru])
        out["is_gained"][s, :Ku] = a_mapped[s, :Ku] & ~match.any(axis=1)
    out["is_lost"], out["ref_is_unmapped"] = r_mapped & ~has_partner, r_listed & ~r_mapped
    out["is_unmapped"] = a_listed & ~a_mapped
    return out


def _boundary_fields(alt, ref, alt_track, ref_track, tol, bin_map=None, delta=None):
    """The matched boundary fields (`BOUNDARY_MATCH_FIELDS`) of P pairs of tracks, a dict of [P, ...] numpy arrays, from the calls of the alt tracks
    ``alt`` and of the reference tracks ``ref`` (``bins``, ``strength`` [P, K]), the tracks themselves [P, n], and ``bin_map`` [P, n] (None = the
    identity).  ``delta`` [P, n] float32 or None: the signed insulation difference by ALT bin; ``boundary_delta`` gathers it at the lowest alt bin
    that stands for each reference boundary's own bin (NaN where there is none, or the slot is empty) and is left out without it; that bin is
    ``first_at`` [P, R] int32 of the dict (-1 for none), for a caller that gathers on the device - not a field."""
    got = _match_boundaries(alt["bins"], alt["strength"], ref["bins"], ref["strength"], alt_track, ref_track, tol, bin_map)
    out = {"boundary_followed_at": got["followed_at"], "boundary_strength_delta": got["strength_delta"], "boundary_is_gained": got["is_gained"],
           "ref_boundary_is_lost": got["is_lost"], "boundary_is_unmapped": got["is_unmapped"], "ref_boundary_is_unmapped": got["ref_is_unmapped"],
           "boundaries_gained": got["is_gained"].sum(axis=1).astype(np.int32), "boundaries_lost": got["is_lost"].sum(axis=1).astype(np.int32),
           "first_at": got["first_at"]}
    if delta is not None:
        at = got["first_at"]
        d = np.asarray(delta, dtype=np.float32)
        out["boundary_delta"] = np.where(at >= 0, d[np.arange(d.shape[0])[:, None], np.where(at >= 0, at, 0)], np.float32(np.nan))
    return out


def boundary_scores_host(tracks, ref_tracks, params, bin_map=None, delta=None, aligned_delta=None):
    """Every boundary field of `ScreenResult` from the insulation tracks of the alt maps ``tracks`` [E, W, n] and of the reference ``ref_tracks``
    [W, n] (host restatement of ``screen_1m(..., insulation=, boundaries=)`` on `ScreenResult.insulation` and ``ref_insulation``): a dict of
    ``ref_boundaries``, ``ref_boundary_strength`` [W, K], ``ref_boundary_count`` [W], ``boundaries``, ``boundary_strength`` [E, W, K],
    ``boundary_count`` [E, W] (`boundary_calls_host`) and the matched fields `BOUNDARY_MATCH_FIELDS` bin with bin (`match_boundaries_host` under the
    identity); with ``bin_map`` ([E, n], or one [n] for all) also their ``aligned_`` forms through it.  ``boundary_delta`` /
    ``aligned_boundary_delta`` need ``delta`` / ``aligned_delta`` [E, W, n] (`ScreenResult.delta_insulation` / ``aligned_insulation``: fp64
    differences rounded once, which the fp32 tracks cannot give back) and are left out without them."""
    t, r = np.asarray(tracks, dtype=np.float32), np.asarray(ref_tracks, dtype=np.float32)
    if t.ndim != 3 or r.shape != t.shape[1:]:
        raise ValueError("tracks: [E, W, n], ref_tracks: [W, n]")
    E, W, n = t.shape
    q = check_boundaries(params, n)
    rc, ac = boundary_calls_host(r, q), boundary_calls_host(t, q)
    out = {"ref_boundaries": rc["bins"], "ref_boundary_strength": rc["strength"], "ref_boundary_count": rc["count"], "boundaries": ac["bins"],
           "boundary_strength": ac["strength"], "boundary_count": ac["count"]}
    flat = lambda a: np.ascontiguousarray(a).reshape((E * W,) + a.shape[2:])
    alt = {k: flat(ac[k]) for k in ("bins", "strength")}
    ref = {k: flat(np.broadcast_to(rc[k], (E,) + rc[k].shape)) for k in ("bins", "strength")}
    rt = flat(np.broadcast_to(r, (E, W, n)))
    bms = None if bin_map is None else np.repeat(_bin_maps(bin_map, E, n), W, axis=0)
    for pre, bm, dl in (("", None, delta), ("aligned_", bms, aligned_delta)) if bms is not None else (("", None, delta),):
        got = _boundary_fields(alt, ref, flat(t), rt, q.tol, bm, None if dl is None else flat(np.asarray(dl, dtype=np.float32)))
        out.update((pre + k, v.reshape((E, W) + v.shape[1:])) for k, v in got.items() if k != "first_at")
    return out


def merge_strands_host(plus, minus, ref_plus=None, ref_minus=None):
    """The merged maps of ``strands="both"`` (fp64 host restatement of orca_screen_merge_strands): ``plus``, ``minus`` [E, n, n] (or [n, n]) the two
    strands' maps, ``minus`` in the '-' strand's own orientation.  (merged, gap) with merged = 0.5 plus + 0.5 flip(minus), flip reversing both bin
    axes, and - with the two strands' reference maps [n, n] - gap[e] = mean |(plus[e] - ref_plus) - flip(minus[e] - ref_minus)|, else None."""
    p, m = np.asarray(plus, dtype=np.float64), np.asarray(minus, dtype=np.float64)
    merged = 0.5 * p + 0.5 * m[..., ::-1, ::-1]
    if ref_plus is None or ref_minus is None:
        return merged, None
    d = (p - np.asarray(ref_plus, dtype=np.float64)) - (m - np.asarray(ref_minus, dtype=np.float64))[..., ::-1, ::-1]
    return merged, np.abs(d).mean(axis=(-1, -2))


def _member_table(member_off, members, E, U):
    off, mem = np.asarray(member_off, dtype=np.int64), np.asarray(members, dtype=np.int64)
    if off.shape != (E + 1,) or mem.ndim != 1 or off[0] != 0 or off[-1] != mem.size or np.any(np.diff(off) < 1) or (mem.size and (mem.min() < 0 or mem.max() >= U)):
        raise ValueError(f"member table: offsets [{E + 1}] from 0 to P, strictly increasing, and [P] indices in [0, {U})")
    return off, mem


def epistasis_scores_host(maps, bank, ref, member_off, members, regions=None):
    """The scores of `EpistasisResult` from the sets' maps [E, n, n], the singles' maps ``bank`` [U, n, n], the reference map [n, n] and the member
    table of `epistasis_items` (fp64 host restatement of orca_screen_epistasis_scores and orca_screen_epistasis_region_scores, in their order:
    every pixel converted to fp64 first, no multiplication).  Per set, t = sum_m (bank[member m] - ref) added sequentially for m ascending
    from 0.0, r = (maps[e] - ref) - t: (epi_profile [E, n] = mean_j |r|, epi_abs_mean [E] = mean |r|, epi_abs_max [E] = max |r|,
    additive_abs_mean [E] = mean |t|, epi_region [E, K], epi_region_abs [E, K]) - the last two the means of r and of |r| over the rectangles
    of ``regions``, None without them."""
    alt, bk, rf = np.asarray(maps, dtype=np.float64), np.asarray(bank, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    E, n = alt.shape[0], rf.shape[0]
    off, mem = _member_table(member_off, members, E, bk.shape[0])
    r, t = np.empty((E, n, n)), np.empty((E, n, n))
    for e in range(E):
        s = np.zeros((n, n))
        for m in mem[off[e]: off[e + 1]]:
            s = s + (bk[m] - rf)
        r[e], t[e] = (alt[e] - rf) - s, s
    with np.errstate(invalid="ignore"):
        a = np.abs(r)
        out = (a.mean(axis=2), a.mean(axis=(1, 2)), a.max(axis=(1, 2)), np.abs(t).mean(axis=(1, 2)))
        if regions is None:
            return out + (None, None)
        rects = check_regions(regions, n)
        sg = np.stack([r[:, i0:i1, j0:j1].mean(axis=(1, 2)) for i0, i1, j0, j1 in rects], axis=1)
        ab = np.stack([a[:, i0:i1, j0:j1].mean(axis=(1, 2)) for i0, i1, j0, j1 in rects], axis=1)
    return out + (sg, ab)
