"""Readouts of the structural-variant screen: what compares a pair of finished maps through a bin map.

`sv.sv_screen(..., scores=True)` and `sv.sv_scores` hand this module the six levels' reference and alt maps of a variant, [6, C, 250, 250] per model,
with the levels' bin maps (int32 [6, 250]: the reference bin every alt bin stands for, or -1) and the bins of the positions that the readouts are asked
about.  It knows maps, bin maps, bins and checked parameters - not variants, pieces or coordinates; its public names are also reachable as ``sv.NAME``.
Every kernel has a ``*_host`` restatement in numpy here, which the tests compare the device against.

THE FIELDS of ``entry["scores"]``.  Every entry of a screen with ``scores=True`` has
    {"bin_map": int32 [6, 250], "count": int32 [6] (the mapped bins per level), "junction_bins": int32 [6, J] (`sv.junction_bins`),
     "models": [{"abs_mean", "abs_max", "delta_mean", "rms": float32 [6, C], "corr": float64 [6, C], "profile": float32 [6, C, 250]} per model]}
- how far the alt maps are from the variant's OWN reference maps, level by level, on aligned bins (`sv.level_bin_maps`;
orca_screen_paired_aligned_scores, include/orca_hip.h has the definitions) - indexed by level (32 Mb first) and target channel, ``profile`` also by ALT
bin.  A level whose two windows share no locus has count 0 and NaN scores - the finest levels of a deletion larger than their window, since
`sv.sv_windows` centres the reference window on the deleted span.
``insulation``, ``viewpoints``, ``strata``: readouts of WHAT changed, per level, from the same final maps through the same bin maps - one more launch
per readout and (variant, model) over the 6 C pairs, on the decoders' stream (orca_screen_paired_insulation / _viewpoints / _strata_scores;
`paired_insulation_host`, `paired_viewpoints_host`, `paired_strata_host` restate them in numpy).  Unset, ``entry["scores"]`` has exactly the keys and
bits above.
  ``insulation=(5, 10, 25)``: diamond widths in bins, the same at every level (`screen.check_insulation` on 250 bins).  Adds ``insulation_widths`` and
    per model ``insulation``, ``ref_insulation``, ``insulation_delta`` float32 [6, C, W, 250]: ins(alt)[i], ins(ref)[i] at the reference's own bin, and
    ins(alt)[i] - ins(ref)[map i] by alt bin (NaN where bin i is unmapped or a diamond does not fit); ``insulation_delta[k, c, w, junction_bins[k]]``
    is the change at the breakpoint - a lost boundary reads positive.
  ``viewpoints=[pos, ...]``: 1 to 64 base positions on the ORIGINAL chromosome (`sv.viewpoint_bins`: a reference bin per level, -1 outside the
    level's window).  Adds ``viewpoint_bins``, ``viewpoint_count`` int32 [6, V] (the alt bins that stand for the viewpoint: 0 deleted or outside, 2
    duplicated) and per model ``viewpoint_delta`` float32 [6, C, V, 250] by alt bin: the mean alt row of those bins minus the reference's row of the
    viewpoint, column j against reference column map j.
  ``strata=True`` or ``(d_lo, d_hi)`` (`screen.check_strata` on 250 bins).  Adds ``strata_range``, ``dist_count`` int32 [6, 250] and per model
    ``dist_delta``, ``dist_abs``, ``dist_rms`` float32 [6, C, 250], ``dist_corr`` float64 [6, C, 250], ``mse`` float32 [6, C], ``strata_corr``, ``scc``
    float64 [6, C] (the strata kernel's pooled Pearson and HiCRep's stratum-adjusted correlation over the range; ``corr`` keeps its meaning).  Inside
    an inversion the reference pixel is read mirrored into the upper triangle.
``loops=True`` or a `screen.LoopParams` (`screen.check_loops` on 250 bins, one parameter set for all six levels; the default threshold is NOT
  calibrated on the published checkpoints): dot (loop) calls per level and target on the variant's own reference map and on its alt map
  (orca_screen_dot_calls), every listed reference dot followed through the level's bin map to EVERY eligible alt pixel that stands for it, the
  strongest reported (orca_screen_paired_dot_follow; `paired_loop_scores_host` restates all of it in numpy).  Adds ``loop_params`` (the validated
  parameters) and per model, with K = max_calls: ``ref_loops``, ``loops`` int32 [6, C, K, 2] (the first K dots, row-major, -1 behind them),
  ``ref_loop_enrichment``, ``loop_enrichment`` float32 [6, C, K], ``ref_loop_count``, ``loop_count`` int32 [6, C] (ALL dots), ``loop_candidates`` int32
  [6, C, K] (the eligible alt pixels that stand for reference dot k: 0 = an anchor deleted, outside the alt window or too near the diagonal or the
  edge, 1 ordinarily, 2 to 4 under a tandem duplication), ``loop_followed_at`` int32 [6, C, K, 2] (the one with the largest enrichment, (-1, -1)
  without one), ``loop_followed_enrichment``, ``loop_delta`` float32 [6, C, K] (its e, and its e minus the reference dot's; NaN without one),
  ``loop_is_gained``, ``ref_loop_is_lost`` bool [6, C, K] (a listed alt dot whose reference pixel (min(map a, map c), max(map a, map c)) has no listed
  reference dot within ``tol`` - one with an unmapped bin is gained; a listed reference dot that no listed alt dot matches) and their sums
  ``loops_gained``, ``loops_lost`` int32 [6, C].  Unset, nothing is launched.
``boundaries=True`` or a `screen.BoundaryParams` (with ``insulation=``, else a ValueError; `check_boundaries_arg`, one parameter set for all six levels
  and every width; the default ``min_strength`` is NOT calibrated on the published checkpoints - choose it from ``ref_boundary_strength``): domain
  boundary calls per level, target and width on the variant's own reference track and on its alt track (orca_screen_boundary_calls on the tracks the
  insulation readout holds on the device - two launches, the maps are not needed again; include/orca_hip.h defines a minimum, its strength - the
  prominence of the dip, in mean log observed / expected, nothing bridged across a NaN - and a call), matched through the level's bin map on the host
  (`paired_boundary_scores_host` restates all of it in numpy).  Adds ``boundary_params`` and per model, with K = max_calls: ``ref_boundaries``,
  ``boundaries`` int32 [6, C, W, K] (ascending bins, -1 behind them), ``ref_boundary_strength``, ``boundary_strength`` float32 [6, C, W, K],
  ``ref_boundary_count``, ``boundary_count`` int32 [6, C, W] (ALL boundaries); per REFERENCE boundary ``boundary_followed_at`` int32 (the alt bin of
  its partner: the listed alt boundary a with |map a - r| <= tol of largest strength, the lower bin of equals; -1 without), ``boundary_strength_delta``
  float32 (the partner's strength - the reference's; -the reference's when lost; NaN when unmapped), ``boundary_delta`` float32 (``insulation_delta``
  at the lowest alt bin that stands for the boundary's own bin; NaN without one), ``ref_boundary_is_lost`` (some alt bin with a track value stands
  within tol of it, but no listed alt boundary does) and ``ref_boundary_is_unmapped`` (no such alt bin: deleted, or outside the alt window - not
  lost); per ALT boundary ``boundary_is_gained`` (its bin stands for a reference bin where the reference track is not NaN, and no listed reference
  boundary is within tol) and ``boundary_is_unmapped`` (its bin stands for no such reference bin - inserted sequence or refill: not gained) - all
  [6, C, W, K] - and the sums ``boundaries_gained``, ``boundaries_lost`` int32 [6, C, W].  Under a tandem duplication both copies of a boundary match
  the reference boundary and the stronger is its partner; inside an inversion the bin map descends and |map a - r| needs no special case.  Unset,
  nothing is launched.
``compartments=True`` or a `CompartmentParams` (`check_compartments_arg`, one parameter set for all six levels): the compartment signal per level and
  target - the K = n_eigs leading eigenvectors of the variant's own reference map and of its alt map (orca_screen_eigenvectors: one launch per
  (variant, model) over the 12 C maps; include/orca_hip.h has the definition, `eigenvectors_host` restates it through numpy's eigh), scaled by
  sqrt(|eigenvalue|) and oriented by the GC content of the window's own bins (orca_screen_gc_tracks on the assembled codes, one call per window: A
  compartment = GC-rich = positive) - compared through the level's bin map on the host (`paired_compartment_scores_host`).  Adds
  ``compartment_params``, ``ref_gc``, ``gc`` float32 [6, 250] and per model ``ref_compartment``, ``compartment`` float32 [6, C, K, 250] (by reference
  bin, by alt bin; NaN on a bin with a NaN pixel), ``compartment_delta`` float32 [6, C, K, 250] (E_alt[i] - E_ref[map i]; NaN where bin i is unmapped
  or either value is NaN), ``ref_compartment_eigenvalue``, ``compartment_eigenvalue``, ``ref_compartment_residual``, ``compartment_residual`` float64
  [6, C, K], ``ref_compartment_converged``, ``compartment_converged`` bool [6, C, K] (residual <= tol), ``ref_compartment_iterations``,
  ``compartment_iterations`` int32 [6, C, K], ``compartment_corr`` float64 [6, C, K] (Pearson of E_alt[i] against E_ref[map i] over the pairs where
  both are finite; NaN below 2 pairs) and ``compartment_flips`` int32 [6, C, K] (the pairs whose two values have opposite sign).  CAVEATS: only the
  coarse levels (128 kb and 64 kb bins) have a compartment meaning - the fine levels (4-16 kb bins) get the same numbers without one; and where the
  spectrum reorders between reference and alt (E1 <-> E2) ``compartment_delta`` is meaningless - ``compartment_corr`` near 0 shows it.  A vector that
  did not converge is returned as it stands (``*_converged`` False), never NaN for that.  Unset, nothing is launched.
"""
from collections import namedtuple

import numpy as np
import torch

from . import engine, map_readouts
from .map_readouts import STRATA_FIELDS, _boundary_fields, _loop_params, boundary_calls_host, check_boundaries, check_insulation, check_loops, check_strata, dot_calls_host, insulation_host

LEVELS = 6
LEVEL_BINS = 250
SCORE_FIELDS = ("abs_mean", "abs_max", "delta_mean", "rms", "corr", "profile")


def _ref_bins_host(table, B, n, bin_map=True):
    """A table of reference bins, one row per pair (or one row for all B pairs), as int64 [B, k], checked: every entry is 0 .. n - 1, or -1.  A bin map
    has k = n entries per row; a list of viewpoints (``bin_map=False``) any number V."""
    t = np.asarray(table, dtype=np.int64)
    t = np.broadcast_to(t, (B, n if bin_map else t.shape[0])) if t.ndim == 1 else t
    if t.ndim != 2 or t.shape[0] != B or (bin_map and t.shape[1] != n) or t.min(initial=0) < -1 or t.max(initial=0) >= n:
        name, k = ("bin map", n) if bin_map else ("views", "V")
        raise ValueError(f"{name}: [{B}, {k}] (or [{k}]) with values -1 .. {n - 1}")
    return t


def _pairs_host(alt, ref, bin_map, dtype):
    """The pairs and the bin map of a paired restatement, checked: (alt, ref as ``dtype`` [B, n, n], bin map int64 [B, n], B, n)."""
    a, r = np.asarray(alt, dtype=dtype), np.asarray(ref, dtype=dtype)
    if a.ndim != 3 or a.shape[1] != a.shape[2] or r.shape != a.shape:
        raise ValueError("alt, ref: [B, n, n]")
    B, n = a.shape[0], a.shape[1]
    return a, r, _ref_bins_host(bin_map, B, n), B, n


def paired_aligned_scores_host(alt, ref, bin_map):
    """fp64 numpy restatement of orca_screen_paired_aligned_scores: alt [B, n, n] against ref [B, n, n], pair b through ``bin_map`` [B, n] (or one
    [n] for all).  With M = the alt bins whose map is >= 0, c = |M|, and over M x M: x = alt[i, j], y = ref[map i, map j], dl = x - y.  A dict of
    ``profile`` [B, n] = sum_j |dl| / c (NaN outside M), ``abs_mean`` = sum |dl| / c^2, ``abs_max`` = max |dl|, ``delta_mean`` = sum dl / c^2,
    ``rms`` = sqrt(sum dl^2 / c^2), ``corr`` = the Pearson correlation over the c^2 pairs from two-pass centred sums (the means first, then X, Y,
    C; NaN when c^2 < 2 or X or Y is exactly 0) - all float64 [B] - and ``count`` [B] int32 = c.  Every float is NaN for a pair with c = 0."""
    a, r, bm, B, n = _pairs_host(alt, ref, bin_map, np.float64)
    out = {k: np.full(B, np.nan) for k in ("abs_mean", "abs_max", "delta_mean", "rms", "corr")}
    out["profile"], out["count"] = np.full((B, n), np.nan), np.zeros(B, dtype=np.int32)
    with np.errstate(invalid="ignore"):
        for b in range(B):
            M = np.flatnonzero(bm[b] >= 0)
            c = out["count"][b] = M.size
            if c == 0:
                continue
            x, y = a[b][np.ix_(M, M)], r[b][np.ix_(bm[b, M], bm[b, M])]
            dl = x - y
            out["profile"][b, M] = np.abs(dl).sum(axis=1) / c
            out["abs_mean"][b], out["abs_max"][b] = np.abs(dl).sum() / c ** 2, np.abs(dl).max()
            out["delta_mean"][b], out["rms"][b] = dl.sum() / c ** 2, np.sqrt((dl * dl).sum() / c ** 2)
            ex, ey = x - x.sum() / c ** 2, y - y.sum() / c ** 2
            X, Y, C = (ex * ex).sum(), (ey * ey).sum(), (ex * ey).sum()
            if c >= 2 and X != 0.0 and Y != 0.0:
                out["corr"][b] = C / np.sqrt(X * Y)
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
# Readouts per level: what changed, not only how much.  The 1 Mb screen's insulation tracks, viewpoint profiles (virtual 4C) and distance
# strata (orca_amd/screen_readouts.py), in their paired forms: every (level, target) alt map against the variant's own reference map through the
# level's bin map.  A genomic position is a different bin at every level, or none; inside an inversion the bin map descends, and the strata
# read the reference pixel mirrored into the upper triangle (the min/max rule).
# ---------------------------------------------------------------------------------------------------------------------------------
def paired_insulation_host(alt, ref, widths, bin_map):
    """fp64 numpy restatement of orca_screen_paired_insulation: alt [B, n, n] against ref [B, n, n], pair b through ``bin_map`` [B, n] (or one
    [n] for all), at ``widths`` (bins).  ins_w(m)[i] = the mean of m over rows [i - w, i) x columns (i, i + w], NaN unless w <= i < n - w
    (`screen.insulation_host`).  (track, ref_track, aligned), each fp64 [B, W, n]: track = ins(alt b)[i], ref_track = ins(ref b)[i] at the
    reference's own bin i, aligned = ins(alt b)[i] - ins(ref b)[map i] where map i >= 0 and both diamonds fit, else NaN."""
    a, r, bm, B, n = _pairs_host(alt, ref, bin_map, np.float64)
    track, ref_track = insulation_host(a, widths), insulation_host(r, widths)
    aligned = np.full(track.shape, np.nan)
    for b in range(B):
        M = np.flatnonzero(bm[b] >= 0)
        aligned[b][:, M] = track[b][:, M] - ref_track[b][:, bm[b, M]]
    return track, ref_track, aligned


def paired_viewpoints_host(alt, ref, views, bin_map):
    """Numpy restatement of orca_screen_paired_viewpoints: alt [B, n, n] against ref [B, n, n] (float32), pair b through ``bin_map`` [B, n] (or
    one [n]) at its own viewpoints ``views`` [B, V] (or one [V] for all): REFERENCE bins, -1 = none.  With R = the alt bins i with map i ==
    view (ascending), c = |R|: (aligned float32 [B, V, n], count int32 [B, V] = c; 0 for view -1).  aligned[b, v, j] = fp32((sum_{i in R}
    alt[i, j]) / c - ref_b[view, map j]) in fp64, the rows added in ascending i, where c >= 1 and map j >= 0, else NaN; for c = 1 it is the fp32
    subtraction alt[R0, j] - ref_b[view, map j]."""
    a, r, bm, B, n = _pairs_host(alt, ref, bin_map, np.float32)
    vs = _ref_bins_host(views, B, n, bin_map=False)
    V = vs.shape[1]
    aligned, count = np.full((B, V, n), np.nan, dtype=np.float32), np.zeros((B, V), dtype=np.int32)
    for b in range(B):
        cols = np.flatnonzero(bm[b] >= 0)
        for k in range(V):
            v = int(vs[b, k])
            if v < 0:
                continue
            R = np.flatnonzero(bm[b] == v)
            count[b, k] = R.size
            if R.size == 1:
                aligned[b, k, cols] = a[b, R[0], cols] - r[b, v, bm[b, cols]]
            elif R.size > 1:
                s = np.zeros(cols.size)
                for i in R:
                    s = s + a[b, i, cols].astype(np.float64)
                aligned[b, k, cols] = (s / float(R.size) - r[b, v, bm[b, cols]].astype(np.float64)).astype(np.float32)
    return aligned, count


def _seq(v):
    """the sum of v added sequentially from 0.0, in order"""
    return float(np.cumsum(v)[-1]) if v.size else 0.0


def paired_strata_host(alt, ref, bin_map, d_range=None):
    """fp64 numpy restatement of orca_screen_paired_strata_scores: alt [B, n, n] against ref [B, n, n], pair b through ``bin_map`` [B, n] (or
    one [n] for all).  Stratum d is the alt pairs (i, i + d) with mi = map i >= 0 and mj = map (i + d) >= 0, c_d of them; x = alt[i, i + d],
    y = ref_b[min(mi, mj), max(mi, mj)] - the reference pixel mirrored into the upper triangle where the bin map descends, so that nothing below
    the diagonal of either map is read.  Per stratum, two passes, each for i ascending from 0.0: the means mx_d, my_d, then X_d = sum (x - mx_d)^2,
    Y_d, C_d = sum (x - mx_d)(y - my_d) and sum dl, sum |dl|, sum dl^2 of dl = x - y.  A dict of ``dist_delta``, ``dist_abs``, ``dist_rms``,
    ``dist_corr`` [B, n] (the mean of dl, of |dl|, the root of the mean of dl^2, C_d / sqrt(X_d Y_d); NaN where c_d = 0, dist_corr also where
    c_d < 2 or X_d or Y_d is 0), ``dist_count`` [B, n] int32, and over the strata ``d_range`` = (d_lo, d_hi) (all by default), serially for d
    ascending, empty strata skipped, c = sum c_d: ``mse`` = sum sum dl^2 / c, ``scc`` = sum C_d / sum sqrt(X_d Y_d) (NaN when the denominator
    is 0), ``corr`` = the Pearson correlation from the pooled sums, mx = (sum c_d mx_d) / c, X = sum [X_d + c_d (mx_d - mx)^2], C = sum [C_d +
    c_d (mx_d - mx)(my_d - my)] (NaN when X or Y is 0 or c < 2); all three NaN when c = 0."""
    a, r, bm, B, n = _pairs_host(alt, ref, bin_map, np.float64)
    lo, hi = check_strata(True if d_range is None else d_range, n)
    out = {k: np.full((B, n), np.nan) for k in ("dist_delta", "dist_abs", "dist_rms", "dist_corr")}
    out.update({k: np.full(B, np.nan) for k in ("mse", "corr", "scc")})
    out["dist_count"] = np.zeros((B, n), dtype=np.int32)
    with np.errstate(invalid="ignore"):
        for b in range(B):
            cnt = np.zeros(n, dtype=np.int64)
            mx, my, X, Y, C, Q = (np.zeros(n) for _ in range(6))
            for d in range(n):
                i = np.arange(n - d)
                mi, mj = bm[b, i], bm[b, i + d]
                ok = (mi >= 0) & (mj >= 0)
                i, mi, mj = i[ok], mi[ok], mj[ok]
                c = cnt[d] = i.size
                if c == 0:
                    continue
                x, y = a[b, i, i + d], r[b, np.minimum(mi, mj), np.maximum(mi, mj)]
                mx[d], my[d] = _seq(x) / c, _seq(y) / c
                ex, ey, dl = x - mx[d], y - my[d], x - y
                X[d], Y[d], C[d], Q[d] = _seq(ex * ex), _seq(ey * ey), _seq(ex * ey), _seq(dl * dl)
                out["dist_delta"][b, d], out["dist_abs"][b, d], out["dist_rms"][b, d] = _seq(dl) / c, _seq(np.abs(dl)) / c, np.sqrt(Q[d] / c)
                if c >= 2 and X[d] != 0.0 and Y[d] != 0.0:
                    out["dist_corr"][b, d] = C[d] / np.sqrt(X[d] * Y[d])
            out["dist_count"][b] = cnt
            ds = [d for d in range(lo, hi) if cnt[d] > 0]
            tot = int(sum(cnt[d] for d in ds))
            if tot == 0:
                continue
            q = num = den = wx = wy = 0.0
            for d in ds:
                q, num, den = q + Q[d], num + C[d], den + np.sqrt(X[d] * Y[d])
                wx, wy = wx + cnt[d] * mx[d], wy + cnt[d] * my[d]
            pmx, pmy = wx / tot, wy / tot
            PX = PY = PC = 0.0
            for d in ds:
                ex, ey = mx[d] - pmx, my[d] - pmy
                PX, PY, PC = PX + (X[d] + cnt[d] * (ex * ex)), PY + (Y[d] + cnt[d] * (ey * ey)), PC + (C[d] + cnt[d] * (ex * ey))
            out["mse"][b] = q / tot
            if den != 0.0 and not np.isnan(den):
                out["scc"][b] = num / den
            if tot >= 2 and PX != 0.0 and PY != 0.0:
                out["corr"][b] = PC / np.sqrt(PX * PY)
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
# Loops per level.  The dot calls are the 1 Mb screen's (orca_screen_dot_calls on the reference maps and on the alt maps; `screen.LoopParams`); what
# is new is the way from a reference dot into the alt map.  Under a duplication two alt bins stand for one reference bin, so a reference dot has up
# to four alt pixels: it is followed to EVERY one that is eligible and the strongest is reported - "does this loop survive anywhere in the allele" -
# with their number beside it (orca_screen_paired_dot_follow; include/orca_hip.h and DESIGN 3d have the rule).
# ---------------------------------------------------------------------------------------------------------------------------------
LOOP_SCORE_FIELDS = ("ref_loops", "loops", "ref_loop_enrichment", "loop_enrichment", "ref_loop_count", "loop_count", "loop_candidates", "loop_followed_at",
                     "loop_followed_enrichment", "loop_delta", "loop_is_gained", "ref_loop_is_lost", "loops_gained", "loops_lost")


def check_loops_arg(loops):
    """The ``loops`` argument of `sv_screen` / `sv_scores`, checked: None when unset (None or False), else the validated `screen.LoopParams`
    (`screen.check_loops` on the levels' 250 bins; True = the defaults).  One parameter set serves all six levels."""
    return map_readouts.check_loops_arg(loops, LEVEL_BINS)


def _is_dot_slot(ij, n):
    """bool [...]: the slots of a dot list [..., 2] that hold a dot, 0 <= i < j <= n - 1 (the -1 padding and anything else is an empty slot)."""
    return (ij[..., 0] >= 0) & (ij[..., 0] < ij[..., 1]) & (ij[..., 1] <= n - 1)


def _follow_beats(v, at, w, other):
    """The total order of the follow: is candidate (e = v at pixel ``at``) better than (w at ``other``)?  A non-NaN e beats a NaN e, a larger e a
    smaller one (fp32), and of two equals the earlier pixel in row-major order."""
    vn, wn = bool(np.isnan(v)), bool(np.isnan(w))
    if vn != wn:
        return wn
    if not vn and v != w:
        return bool(v > w)
    return at < other


def paired_dot_follow_host(alt_e, ref_ij, ref_enrich, bin_map, params):
    """Numpy restatement of orca_screen_paired_dot_follow, brute force over A x C: ``alt_e`` [B, n, n] float32 (the alt maps' enrichment map,
    `screen.dot_calls_host`'s or the device's ``e_map``), ``ref_ij`` [B, R, 2] and ``ref_enrich`` [B, R] (the reference maps' dot lists), pair b
    through ``bin_map`` [B, n] (or one [n] for all); ``params``: a `screen.LoopParams` (w and d_min are used).  For reference dot (ri, rj), 0 <= ri <
    rj <= n - 1 (any other slot is empty): A = the alt bins a with map a = ri, C = those with map c = rj, the candidates are the pixels (min(a, c),
    max(a, c)) over A x C with w <= i, j <= n - 1 - w and j - i >= d_min.  A dict of ``candidates`` [B, R] int32 (their number), ``at`` [B, R, 2]
    int32 (the best: a non-NaN e beats a NaN e, a larger e a smaller one, the earlier pixel of two equals), ``enrich`` [B, R] float32 (alt_e there)
    and ``delta`` [B, R] float32 = enrich - ref_enrich (fp32); (-1, -1), NaN, NaN without a candidate."""
    q = _loop_params(params)
    e = np.asarray(alt_e, dtype=np.float32)
    if e.ndim != 3 or e.shape[1] != e.shape[2]:
        raise ValueError("alt_e: [B, n, n]")
    B, n = e.shape[0], e.shape[1]
    ij, re = np.asarray(ref_ij, dtype=np.int64), np.asarray(ref_enrich, dtype=np.float32)
    if ij.ndim != 3 or ij.shape[0] != B or ij.shape[2] != 2 or re.shape != ij.shape[:2]:
        raise ValueError(f"ref_ij: [{B}, R, 2], ref_enrich: [{B}, R]")
    bm = _ref_bins_host(bin_map, B, n)
    R = ij.shape[1]
    out = {"candidates": np.zeros((B, R), dtype=np.int32), "at": np.full((B, R, 2), -1, dtype=np.int32),
           "enrich": np.full((B, R), np.nan, dtype=np.float32), "delta": np.full((B, R), np.nan, dtype=np.float32)}
    dot = _is_dot_slot(ij, n)
    for b, k in zip(*np.nonzero(dot)):
        ri, rj = int(ij[b, k, 0]), int(ij[b, k, 1])
        best, cnt = None, 0
        for a in np.flatnonzero(bm[b] == ri):
            for c in np.flatnonzero(bm[b] == rj):
                i, j = int(min(a, c)), int(max(a, c))
                if not (i >= q.w and j <= n - 1 - q.w and j - i >= q.d_min):
                    continue
                cnt += 1
                if best is None or _follow_beats(e[b, i, j], i * n + j, e[b, best[0], best[1]], best[0] * n + best[1]):
                    best = (i, j)
        out["candidates"][b, k] = cnt
        if best is not None:
            out["at"][b, k] = best
            out["enrich"][b, k] = e[b, best[0], best[1]]
            with np.errstate(invalid="ignore"):
                out["delta"][b, k] = e[b, best[0], best[1]] - re[b, k]
    return out


def paired_match_loops_host(alt_ij, ref_ij, bin_map_row, tol):
    """Match the listed dots of an alt map, ``alt_ij`` [K, 2], to its reference map's, ``ref_ij`` [R, 2], through the pair's bin map ``bin_map_row``
    [n]: (is_gained [K] bool, is_lost [R] bool).  An alt dot (a, c) stands for the reference pixel (min(map a, map c), max(map a, map c)) - the mirror
    rule: inside an inversion the bin map descends - or for nothing if either bin is unmapped; it matches a listed reference dot within Chebyshev
    distance ``tol``.  gained = a listed alt dot that matches none, lost = a listed reference dot that none matches; both False in the empty slots
    (-1 padding, or anything but 0 <= i < j <= n - 1)."""
    alt, ref = np.asarray(alt_ij, dtype=np.int64).reshape(-1, 2), np.asarray(ref_ij, dtype=np.int64).reshape(-1, 2)
    bm = np.asarray(bin_map_row, dtype=np.int64)
    n = bm.shape[0]
    listed, ref_listed = _is_dot_slot(alt, n), _is_dot_slot(ref, n)
    m = bm[np.where(listed[:, None], alt, 0)]
    ok = listed & (m >= 0).all(axis=1)
    px = np.stack([m.min(axis=1), m.max(axis=1)], axis=1)
    near = (np.abs(px[:, None, :] - ref[None, :, :]).max(axis=2) <= int(tol)) & ok[:, None] & ref_listed[None, :]       # [K, R]
    return listed & ~near.any(axis=1), ref_listed & ~near.any(axis=0)


def _loop_fields(rc, ac, fl, bin_map, tol):
    """The loop fields of B pairs, [B, ...] numpy arrays, from the dot calls of the reference maps ``rc`` and of the alt maps ``ac`` (``count``,
    ``ij``, ``enrich``), the follow ``fl`` and the matching on the host."""
    B, K = ac["ij"].shape[0], ac["ij"].shape[1]
    gained, lost = np.zeros((B, K), dtype=bool), np.zeros((B, K), dtype=bool)
    for b in range(B):
        gained[b], lost[b] = paired_match_loops_host(ac["ij"][b], rc["ij"][b], bin_map[b], tol)
    return {"ref_loops": rc["ij"], "loops": ac["ij"], "ref_loop_enrichment": rc["enrich"], "loop_enrichment": ac["enrich"],
            "ref_loop_count": rc["count"], "loop_count": ac["count"], "loop_candidates": fl["candidates"], "loop_followed_at": fl["at"],
            "loop_followed_enrichment": fl["enrich"], "loop_delta": fl["delta"], "loop_is_gained": gained, "ref_loop_is_lost": lost,
            "loops_gained": gained.sum(axis=1).astype(np.int32), "loops_lost": lost.sum(axis=1).astype(np.int32)}


def paired_loop_scores_host(alt, ref, bin_map, params):
    """Numpy restatement of the loop fields of ``sv_screen(..., scores=True, loops=)`` for B pairs: alt [B, n, n] against ref [B, n, n], pair b through
    ``bin_map`` [B, n] (or one [n] for all), ``params`` a `screen.LoopParams` (or True).  `screen.dot_calls_host` on both, `paired_dot_follow_host`
    from the reference's list into the alt maps' enrichment map, `paired_match_loops_host` per pair: a dict of `LOOP_SCORE_FIELDS`, each [B, ...]
    (K = max_calls): ``ref_loops``, ``loops`` int32 [B, K, 2]; ``ref_loop_enrichment``, ``loop_enrichment`` float32 [B, K]; ``ref_loop_count``,
    ``loop_count`` int32 [B] (all dots); ``loop_candidates`` int32 [B, K]; ``loop_followed_at`` int32 [B, K, 2]; ``loop_followed_enrichment``,
    ``loop_delta`` float32 [B, K]; ``loop_is_gained``, ``ref_loop_is_lost`` bool [B, K]; ``loops_gained``, ``loops_lost`` int32 [B]."""
    a, r, bm, B, n = _pairs_host(alt, ref, bin_map, np.float32)
    q = check_loops(params, n)
    rc, ac = dot_calls_host(r, q), dot_calls_host(a, q)
    return _loop_fields(rc, ac, paired_dot_follow_host(ac["e_map"], rc["ij"], rc["enrich"], bm, q), bm, q.tol)


# ---------------------------------------------------------------------------------------------------------------------------------
# Compartments per level.  The compartment signal of a map is its leading eigenvector (orca_screen_eigenvectors; include/orca_hip.h and DESIGN 3d
# have the definition): the K leading eigenpairs of every level's reference and alt map, oriented by the GC content of the window's own bins
# (orca_screen_gc_tracks on the assembled codes: A compartment = GC-rich = positive), compared through the level's bin map on the host.  Only
# the coarse levels (128 kb, 64 kb bins) have a compartment meaning; the fine levels get the same numbers without one.
# ---------------------------------------------------------------------------------------------------------------------------------
CompartmentParams = namedtuple("CompartmentParams", "n_eigs d_lo center tol max_iter", defaults=(1, 2, True, 1e-8, 1000))
COMPARTMENT_MAX_EIGS = 3
COMPARTMENT_SCORE_FIELDS = ("ref_compartment", "compartment", "compartment_delta", "ref_compartment_eigenvalue", "compartment_eigenvalue",
                            "ref_compartment_residual", "compartment_residual", "ref_compartment_converged", "compartment_converged",
                            "ref_compartment_iterations", "compartment_iterations", "compartment_corr", "compartment_flips")


def check_compartments_arg(compartments, n=LEVEL_BINS):
    """The ``compartments`` argument of `sv_screen` / `sv_scores`, checked for maps of ``n`` bins: None when unset (None or False), else the validated
    `CompartmentParams` (True = the defaults).  A ValueError for anything else and for values outside their ranges: 1 <= n_eigs <= 3, 0 <= d_lo
    <= n - 1, center a bool, tol > 0 (finite), max_iter >= 1.  One parameter set serves all six levels."""
    if compartments is None or compartments is False:
        return None
    q = CompartmentParams() if compartments is True else compartments
    if not isinstance(q, CompartmentParams):
        raise ValueError("compartments: True (the defaults) or an sv.CompartmentParams")
    vals = {}
    for k in ("n_eigs", "d_lo", "max_iter"):
        v = getattr(q, k)
        if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, np.integer)):
            raise ValueError(f"compartments: {k} = {v!r} must be an int")
        vals[k] = int(v)
    if not 1 <= vals["n_eigs"] <= COMPARTMENT_MAX_EIGS:
        raise ValueError(f"compartments: n_eigs = {vals['n_eigs']}: 1 .. {COMPARTMENT_MAX_EIGS}")
    if not 0 <= vals["d_lo"] <= n - 1:
        raise ValueError(f"compartments: d_lo = {vals['d_lo']}: 0 .. {n - 1} on maps of {n} bins")
    if vals["max_iter"] < 1:
        raise ValueError(f"compartments: max_iter = {vals['max_iter']} must be at least 1")
    if not isinstance(q.center, (bool, np.bool_)):
        raise ValueError(f"compartments: center = {q.center!r} must be a bool")
    try:
        tol = float(q.tol)
    except (TypeError, ValueError):
        raise ValueError("compartments: tol must be a number") from None
    if isinstance(q.tol, (bool, np.bool_)) or not (tol > 0.0 and np.isfinite(tol)):
        raise ValueError(f"compartments: tol = {q.tol!r} must be a finite number > 0")
    return CompartmentParams(vals["n_eigs"], vals["d_lo"], bool(q.center), tol, vals["max_iter"])


def compartment_matrix_host(m, d_lo=2, center=True):
    """(A float64 [n, n], valid bool [n]) of one map ``m`` [n, n], as orca_screen_eigenvectors prepares it: S[i][j] = m[min(i,j)][max(i,j)] (the lower
    triangle of ``m`` is never read); bin i is invalid when S[i][j] is NaN for some j with |i - j| >= d_lo; a pixel is kept when |i - j| >= d_lo
    and both bins are valid; A = S - mu on the kept pixels (mu = their fp64 mean, 0 without ``center`` or without a kept pixel) and 0 elsewhere."""
    m = np.asarray(m, dtype=np.float64)
    if m.ndim != 2 or m.shape[0] != m.shape[1]:
        raise ValueError("a map: [n, n]")
    n = m.shape[0]
    S = np.triu(m)
    S = S + np.triu(S, 1).T
    i, j = np.indices((n, n))
    band = np.abs(i - j) >= int(d_lo)
    valid = ~(np.isnan(S) & band).any(axis=1)
    keep = band & valid[:, None] & valid[None, :]
    mu = S[keep].mean() if center and keep.any() else 0.0
    return np.where(keep, S - mu, 0.0), valid


def _compartment_sign(v, scale, valid, phase):
    """The sign rule of orca_screen_eigenvectors for one unit vector ``v`` [n] (fp64) with E = v * scale: +1.0 or -1.0."""
    if phase is not None:
        p = np.asarray(phase, dtype=np.float32)
        use = valid & np.isfinite(p)
        if use.sum() >= 2:
            ex, ey = v[use] - v[use].mean(), p[use].astype(np.float64) - p[use].astype(np.float64).mean()
            X, Y, C = (ex * ex).sum(), (ey * ey).sum(), (ex * ey).sum()
            if X > 0.0 and Y > 0.0 and C != 0.0 and C == C:
                return -1.0 if C < 0.0 else 1.0
    e = (v * scale).astype(np.float32)
    return -1.0 if e[int(np.argmax(np.where(valid, np.abs(e), np.float32(-1.0))))] < 0.0 else 1.0      # argmax: the lowest index of equals


def eigenvectors_host(maps, n_eigs=1, d_lo=2, center=True, phase=None):
    """Numpy restatement of orca_screen_eigenvectors through `numpy.linalg.eigh` on the prepared A (`compartment_matrix_host`): ``maps`` [B, n, n],
    ``phase`` [B, n] or None.  The ``n_eigs`` eigenpairs of largest |lambda| (descending |lambda|), E_k = v_k sqrt(|lambda_k|) with NaN on the invalid
    bins, the sign by the same rule: with a phase, the Pearson correlation with it over the valid bins whose phase is finite is non-negative; without
    one (or below 2 such bins, or with a zero or NaN correlation) the component of largest |E_k| (as fp32) is positive, the lowest index of equals.
    A dict of ``E`` float32 [B, K, n], ``eigenvalue`` float64 [B, K], ``residual`` float64 [B, K] (|A v - lambda v| / |lambda| of eigh's pair) and
    ``n_valid`` int32 [B]; a map with n_valid <= K is all NaN.  eigh is exact where the device iterates: the two agree to the device's ``residual``
    (times |lambda| / gap for the vectors), not bit for bit."""
    m = np.asarray(maps, dtype=np.float32)
    if m.ndim != 3 or m.shape[1] != m.shape[2]:
        raise ValueError("maps: [B, n, n]")
    B, n, K = m.shape[0], m.shape[1], int(n_eigs)
    if not 1 <= K <= COMPARTMENT_MAX_EIGS or not 0 <= int(d_lo) <= n - 1:
        raise ValueError(f"n_eigs: 1 .. {COMPARTMENT_MAX_EIGS}, d_lo: 0 .. n - 1")
    ph = None if phase is None else np.asarray(phase, dtype=np.float32)
    if ph is not None and ph.shape != (B, n):
        raise ValueError(f"phase: [{B}, {n}]")
    out = {"E": np.full((B, K, n), np.nan, dtype=np.float32), "eigenvalue": np.full((B, K), np.nan), "residual": np.full((B, K), np.nan),
           "n_valid": np.zeros(B, dtype=np.int32)}
    for b in range(B):
        A, valid = compartment_matrix_host(m[b], d_lo, center)
        out["n_valid"][b] = valid.sum()
        if valid.sum() <= K:
            continue
        lam, U = np.linalg.eigh(A)
        order = np.argsort(-np.abs(lam), kind="stable")[:K]
        for k, o in enumerate(order):
            v = np.where(valid, U[:, o], 0.0)
            v = v / np.linalg.norm(v)
            scale = np.sqrt(abs(lam[o]))
            rn = np.linalg.norm(A @ v - lam[o] * v)
            out["eigenvalue"][b, k] = lam[o]
            out["residual"][b, k] = 0.0 if rn == 0.0 else (rn / abs(lam[o]) if lam[o] != 0.0 else np.inf)
            sgn = _compartment_sign(v, scale, valid, None if ph is None else ph[b])
            out["E"][b, k] = np.where(valid, (sgn * v * scale).astype(np.float32), np.float32(np.nan))
    return out


def gc_tracks_host(codes, offsets, binsizes, n):
    """Numpy restatement of orca_screen_gc_tracks: float32 [W, n], out[w][i] = #{C, G} / #{A, C, G, T} (one fp64 division, rounded once) over the
    bases [off_w + i bs_w, off_w + (i + 1) bs_w) of ``codes`` [L] uint8 (0..3 = A, C, G, T; anything above is N), NaN where the bin holds no
    A/C/G/T.  A ValueError for a window that leaves [0, L)."""
    c = np.asarray(codes, dtype=np.uint8).reshape(-1)
    off, bs, n = np.asarray(offsets, dtype=np.int64).reshape(-1), np.asarray(binsizes, dtype=np.int64).reshape(-1), int(n)
    if off.size < 1 or bs.size != off.size or n < 1:
        raise ValueError("offsets, binsizes: one each per window, at least one window; n >= 1")
    L = c.size
    ct = np.int32 if L < 2 ** 31 else np.int64
    acgt, cg = np.zeros(L + 1, dtype=ct), np.zeros(L + 1, dtype=ct)
    np.cumsum(c < 4, dtype=ct, out=acgt[1:])
    np.cumsum((c == 1) | (c == 2), dtype=ct, out=cg[1:])
    out = np.full((off.size, n), np.nan, dtype=np.float32)
    for w in range(off.size):
        if off[w] < 0 or bs[w] < 1 or off[w] + n * bs[w] > L:
            raise ValueError(f"window {w}: {n} bins of {bs[w]} bases from base {off[w]} leave the {L} codes")
        edges = off[w] + np.arange(n + 1, dtype=np.int64) * bs[w]
        a, g = np.diff(acgt[edges]), np.diff(cg[edges])
        ok = a > 0
        out[w, ok] = (g[ok].astype(np.float64) / a[ok].astype(np.float64)).astype(np.float32)
    return out


def paired_compartment_scores_host(alt_E, ref_E, bin_map):
    """The compartment vectors of B alt maps against their reference maps' through the bin maps, in numpy - what `sv_screen` runs on the host:
    ``alt_E``, ``ref_E`` [B, K, n] (or [K, n]), ``bin_map`` [B, n] (or one [n] for all).  The PAIRS of (b, k) are the alt bins i with map i >= 0
    whose two values alt_E[i] and ref_E[map i] are both finite.  A dict of ``delta`` float32 [B, K, n] = alt_E[i] - ref_E[map i] by alt bin (one
    fp32 subtraction; NaN where bin i is unmapped or either value is NaN), ``corr`` float64 [B, K] = the Pearson correlation over the pairs (fp64,
    the means first, then the centred sums; NaN below 2 pairs or where either side is constant) and ``flips`` int32 [B, K] = the pairs whose two
    values have opposite sign (a bin that changed compartment, where the vectors are oriented alike)."""
    a, r = np.asarray(alt_E, dtype=np.float32), np.asarray(ref_E, dtype=np.float32)
    if a.ndim == 2:
        a, r = a[None], r[None] if r.ndim == 2 else r
    if a.ndim != 3 or r.shape != a.shape:
        raise ValueError("alt_E, ref_E: [B, K, n]")
    B, K, n = a.shape
    bm = _ref_bins_host(bin_map, B, n)
    out = {"delta": np.full((B, K, n), np.nan, dtype=np.float32), "corr": np.full((B, K), np.nan), "flips": np.zeros((B, K), dtype=np.int32)}
    for b in range(B):
        M = np.flatnonzero(bm[b] >= 0)
        for k in range(K):
            x, y = a[b, k, M], r[b, k, bm[b, M]]
            with np.errstate(invalid="ignore"):
                out["delta"][b, k, M] = x - y
            ok = np.isfinite(x) & np.isfinite(y)
            x, y = x[ok].astype(np.float64), y[ok].astype(np.float64)
            out["flips"][b, k] = int((x * y < 0.0).sum())
            if x.size >= 2:
                ex, ey = x - x.mean(), y - y.mean()
                X, Y = (ex * ex).sum(), (ey * ey).sum()
                if X > 0.0 and Y > 0.0:
                    out["corr"][b, k] = (ex * ey).sum() / np.sqrt(X * Y)
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
# Boundaries per level.  Domain boundary calls on the insulation tracks of every level's reference and alt map (orca_screen_boundary_calls on
# the tracks the insulation readout already holds on the device; `screen.BoundaryParams`; include/orca_hip.h and DESIGN 3d / 3e have the
# definitions), matched through the level's bin map on the host: which reference boundaries the allele keeps, weakens or loses, which it creates.
# ---------------------------------------------------------------------------------------------------------------------------------
BOUNDARY_SCORE_FIELDS = ("ref_boundaries", "boundaries", "ref_boundary_strength", "boundary_strength", "ref_boundary_count", "boundary_count",
                         "boundary_followed_at", "boundary_strength_delta", "boundary_delta", "boundary_is_gained", "ref_boundary_is_lost",
                         "boundary_is_unmapped", "ref_boundary_is_unmapped", "boundaries_gained", "boundaries_lost")


def check_boundaries_arg(boundaries, insulation=None):
    """The ``boundaries`` argument of `sv_screen` / `sv_scores`, checked: None when unset (None or False), else the validated
    `screen.BoundaryParams` (`screen.check_boundaries` on the levels' 250 bins; True = the defaults).  ``insulation``: the checked widths - the
    boundaries are called on the insulation tracks, so without them it is a ValueError.  One parameter set serves all six levels and every width."""
    return map_readouts.check_boundaries_arg(boundaries, LEVEL_BINS, insulation)


def _paired_boundary_fields(rc, ac, track, ref_track, delta, bin_map, tol):
    """The boundary fields (`BOUNDARY_SCORE_FIELDS`, numpy [B, W, ...]) of B pairs from the calls of the reference tracks ``rc`` and of the alt
    tracks ``ac`` (``count`` [B, W], ``bins``, ``strength`` [B, W, K]), the tracks [B, W, n], ``insulation_delta`` ``delta`` [B, W, n] and
    ``bin_map`` [B, n] (one row per pair, every width): the matching on the host (`screen._boundary_fields`)."""
    B, W, n = track.shape
    flat = lambda a: np.ascontiguousarray(a).reshape((B * W,) + a.shape[2:])
    got = _boundary_fields({k: flat(ac[k]) for k in ("bins", "strength")}, {k: flat(rc[k]) for k in ("bins", "strength")}, flat(track), flat(ref_track),
                           tol, np.repeat(np.asarray(bin_map), W, axis=0), flat(delta))
    out = {"ref_boundaries": rc["bins"], "boundaries": ac["bins"], "ref_boundary_strength": rc["strength"], "boundary_strength": ac["strength"],
           "ref_boundary_count": rc["count"], "boundary_count": ac["count"]}
    out.update((k, v.reshape((B, W) + v.shape[1:])) for k, v in got.items() if k != "first_at")
    return out


def paired_boundary_scores_host(track, ref_track, insulation_delta, bin_map, params):
    """Numpy restatement of the boundary fields of ``sv_screen(..., scores=True, insulation=, boundaries=)`` for B pairs of tracks: ``track``,
    ``ref_track``, ``insulation_delta`` [B, W, n] (an entry's ``insulation``, ``ref_insulation``, ``insulation_delta`` with [6, C] flattened to B),
    pair b through ``bin_map`` [B, n] (or one [n] for all), ``params`` a `screen.BoundaryParams` (or True).  `screen.boundary_calls_host` on both
    tracks, `screen.match_boundaries_host`'s rule per (pair, width): a dict of `BOUNDARY_SCORE_FIELDS`, with K = max_calls: ``ref_boundaries``,
    ``boundaries`` int32 [B, W, K] (ascending, -1 behind them); ``ref_boundary_strength``, ``boundary_strength`` float32 [B, W, K];
    ``ref_boundary_count``, ``boundary_count`` int32 [B, W] (all); per reference boundary ``boundary_followed_at`` int32 (the partner's alt bin or
    -1), ``boundary_strength_delta`` float32 (partner - reference; -reference when lost; NaN when unmapped), ``boundary_delta`` float32
    (``insulation_delta`` at the lowest alt bin that stands for the boundary's own bin, NaN without one), ``ref_boundary_is_lost``,
    ``ref_boundary_is_unmapped`` bool; per alt boundary ``boundary_is_gained``, ``boundary_is_unmapped`` bool - all [B, W, K]; ``boundaries_gained``,
    ``boundaries_lost`` int32 [B, W]."""
    t, r, d = (np.asarray(x, dtype=np.float32) for x in (track, ref_track, insulation_delta))
    if t.ndim != 3 or r.shape != t.shape or d.shape != t.shape:
        raise ValueError("track, ref_track, insulation_delta: [B, W, n]")
    B, n = t.shape[0], t.shape[2]
    q = check_boundaries(params, n)
    return _paired_boundary_fields(boundary_calls_host(r, q), boundary_calls_host(t, q), t, r, d, _ref_bins_host(bin_map, B, n), q.tol)


# The arguments, checked once, and what they add to an entry before any model is scored.
def check_tracks(insulation=None, viewpoints=None, strata=None):
    """The three readout arguments of `sv_screen` / `sv_scores`, checked: None when all are unset, else {"insulation": int32 widths or None,
    "viewpoints": [positions] or None, "strata": (d_lo, d_hi) or None}.  ``insulation`` as `screen.check_insulation` takes it, ``strata`` as
    `screen.check_strata`, on the levels' 250 bins; ``viewpoints``: 1 to 64 base positions on the original chromosome."""
    if insulation is None and viewpoints is None and strata is None:
        return None
    spec = {"insulation": None, "viewpoints": None, "strata": None}
    if insulation is not None:
        spec["insulation"] = check_insulation(insulation, LEVEL_BINS)
    if viewpoints is not None:
        try:
            pos = [int(p) for p in viewpoints]
        except (TypeError, ValueError):
            raise ValueError("viewpoints: a sequence of base positions") from None
        if not 1 <= len(pos) <= 64 or min(pos) < 0:
            raise ValueError("viewpoints: 1 to 64 base positions >= 0")
        spec["viewpoints"] = pos
    if strata is not None:
        spec["strata"] = check_strata(strata, LEVEL_BINS)
    return spec


Readouts = namedtuple("Readouts", "insulation viewpoints strata loops compartments boundaries", defaults=(None,))


def check_readouts(insulation=None, viewpoints=None, strata=None, loops=None, compartments=None, boundaries=None):
    """The six readout arguments of `sv_screen` / `sv_scores`, checked (`check_tracks`, `check_loops_arg`, `check_compartments_arg`,
    `check_boundaries_arg`, in that order): None when all are unset, else a `Readouts` of the six checked values, each None where unset."""
    tracks = check_tracks(insulation, viewpoints, strata) or {}
    rd = Readouts(tracks.get("insulation"), tracks.get("viewpoints"), tracks.get("strata"), check_loops_arg(loops), check_compartments_arg(compartments),
                  check_boundaries_arg(boundaries, tracks.get("insulation")))
    return None if all(v is None for v in rd) else rd


def _strata_counts(bm):
    """int32 [n]: the alt pairs (i, i + d) of a bin map [n] whose two bins are mapped, per d."""
    ok = (bm >= 0).astype(np.int64)
    return np.correlate(ok, ok, "full")[ok.size - 1:].astype(np.int32)


def entry_readouts(entry, rd, view_bins=None, phase=None):
    """The model-independent keys that the readouts ``rd`` (`check_readouts`' value or None) add to ``entry``, an entry's ``scores`` with its ``bin_map``
    [6, 250]; returns ``entry``.  ``view_bins``: int32 [6, V], the reference bin of every viewpoint per level (with ``rd.viewpoints``); ``phase`` =
    (ref_gc, gc), each [6, 250], or None (with ``rd.compartments``)."""
    bm = entry["bin_map"]
    if rd is None:
        return entry
    if rd.loops is not None:
        entry["loop_params"] = rd.loops
    if rd.compartments is not None:
        entry["compartment_params"] = rd.compartments
        if phase is not None:
            entry["ref_gc"], entry["gc"] = (np.ascontiguousarray(p, dtype=np.float32) for p in phase)
            if entry["ref_gc"].shape != (LEVELS, LEVEL_BINS) or entry["gc"].shape != (LEVELS, LEVEL_BINS):
                raise ValueError(f"phase: (ref_phase, alt_phase), each [{LEVELS}, {LEVEL_BINS}]")
    if rd.insulation is not None:
        entry["insulation_widths"] = rd.insulation.copy()
    if rd.boundaries is not None:
        entry["boundary_params"] = rd.boundaries
    if rd.viewpoints is not None:
        vb = entry["viewpoint_bins"] = view_bins
        entry["viewpoint_count"] = np.where(vb >= 0, (bm[:, None, :] == vb[:, :, None]).sum(axis=2), 0).astype(np.int32)
    if rd.strata is not None:
        entry["strata_range"] = tuple(rd.strata)
        entry["dist_count"] = np.stack([_strata_counts(bm[k]) for k in range(LEVELS)])
    return entry


# One model's maps of one variant on the device.  Every readout is a launch over the same B = 6 C pairs that returns numpy arrays [B, ...].
def _to_host(d):
    return {k: v.cpu().numpy() for k, v in d.items()}


def _joint_maps(ref, alt):
    """The reference maps followed by the alt maps as ONE [2B, n, n] view where the alt maps [B, n, n] lie right behind the reference maps [B, n, n] in
    one allocation, as the screen's do - else None."""
    B, n = alt.shape[0], alt.shape[1]
    if (ref.is_contiguous() and alt.is_contiguous() and ref.untyped_storage().data_ptr() == alt.untyped_storage().data_ptr()
            and alt.storage_offset() == ref.storage_offset() + ref.numel()):
        return ref.as_strided((2 * B, n, n), (n * n, n, 1))
    return None


def _ref_and_alt(launch, ref, alt, fetch=dict):
    """(the reference maps' dict, the alt maps' dict) of ``launch(maps, lo, hi)``, a batched launch that returns a dict of [batch, ...] arrays and whose
    result for a map does not depend on the batch it is in: ONE launch over `_joint_maps` (rows lo = 0 .. hi = 2B) where there is such a view, else two
    (rows 0 .. B, then B .. 2B).  ``fetch`` is applied to every launch's dict (`_to_host`: one copy per array, not one per half)."""
    B = alt.shape[0]
    both = _joint_maps(ref, alt)
    if both is None:
        rc, ac = launch(ref, 0, B), launch(alt, B, 2 * B)
        return fetch(rc), fetch(ac)
    got = fetch(launch(both, 0, 2 * B))
    return {k: v[:B] for k, v in got.items()}, {k: v[B:] for k, v in got.items()}


def _model_loops(ctx, alt, ref, bin_map, q):
    """The loop fields (`LOOP_SCORE_FIELDS`, numpy [B, ...]) of B pairs of maps on the device, alt [B, n, n] against ref [B, n, n] (contiguous) through
    ``bin_map`` [B, n], on the current stream: orca_screen_dot_calls over the reference and the alt maps (`_ref_and_alt`: ONE call for the screen's maps),
    then orca_screen_paired_dot_follow from the reference's device lists into the alt maps' enrichment map, the small copies back and the matching in
    numpy."""
    rc, ac = _ref_and_alt(lambda maps, lo, hi: engine.screen_dot_calls(ctx, maps, q.p, q.w, q.r, q.threshold, q.max_calls, q.d_min), ref, alt)
    fl = engine.screen_paired_dot_follow(ctx, ac["e_map"], rc["ij"], rc["enrich"], bin_map, q.w, q.d_min)
    host = [{k: d[k].cpu().numpy() for k in d if k != "e_map"} for d in (rc, ac, fl)]
    return _loop_fields(*host, bin_map, q.tol)


def _model_compartments(ctx, alt, ref, bin_map, q, ref_phase=None, alt_phase=None):
    """The compartment fields (`COMPARTMENT_SCORE_FIELDS`, numpy [B, ...]) of B pairs of maps on the device, alt [B, n, n] against ref [B, n, n]
    (contiguous) through ``bin_map`` [B, n], on the current stream: orca_screen_eigenvectors over the reference and the alt maps (`_ref_and_alt`: ONE
    launch for the screen's maps), phased by ``ref_phase`` / ``alt_phase`` [B, n] (numpy).  Without them the reference takes the kernel's fallback
    orientation and every alt vector is flipped so that its dot product with the reference's through the bin map is not negative.  The small arrays
    come back and `paired_compartment_scores_host` compares them."""
    B = alt.shape[0]
    phased = ref_phase is not None and alt_phase is not None
    ph = torch.from_numpy(np.ascontiguousarray(np.concatenate([ref_phase, alt_phase]), dtype=np.float32)).to(alt.device) if phased else None
    rc, ac = _ref_and_alt(lambda maps, lo, hi: engine.screen_eigenvectors(ctx, maps, q.n_eigs, q.d_lo, q.center, q.tol, q.max_iter,
                                                                          phase=None if ph is None else ph[lo:hi]), ref, alt, _to_host)
    if not phased:
        ac["E"] = ac["E"].copy()
        for b in range(B):
            M = np.flatnonzero(bin_map[b] >= 0)
            prod = ac["E"][b][:, M].astype(np.float64) * rc["E"][b][:, bin_map[b, M]].astype(np.float64)
            ac["E"][b][np.nansum(prod, axis=1) < 0.0] *= np.float32(-1.0)
    sc = paired_compartment_scores_host(ac["E"], rc["E"], bin_map)
    return {"ref_compartment": rc["E"], "compartment": ac["E"], "compartment_delta": sc["delta"],
            "ref_compartment_eigenvalue": rc["eigenvalue"], "compartment_eigenvalue": ac["eigenvalue"],
            "ref_compartment_residual": rc["residual"], "compartment_residual": ac["residual"],
            "ref_compartment_converged": rc["residual"] <= q.tol, "compartment_converged": ac["residual"] <= q.tol,
            "ref_compartment_iterations": rc["iterations"], "compartment_iterations": ac["iterations"], "compartment_corr": sc["corr"], "compartment_flips": sc["flips"]}


def _model_scores(ctx, ref_maps, alt_maps, bin_map, entry=None):
    """One model's scores of one variant: ``ref_maps``, ``alt_maps`` [6, C, n, n] contiguous on the device, ``bin_map`` [6, n] (repeated per
    target channel here) - one launch of 6 C pairs on the current stream; a dict of numpy arrays [6, C] (``profile`` [6, C, n]).  ``entry``
    (an entry's ``scores`` after `entry_readouts`): one more launch per readout it names, over the same pairs; each gives arrays [6 C, ...], and all
    of them leave here as [6, C, ...]."""
    lv, C, n = alt_maps.shape[0], alt_maps.shape[1], alt_maps.shape[2]
    alt, ref, bmc = alt_maps.reshape(lv * C, n, n), ref_maps.reshape(lv * C, n, n), np.repeat(bin_map, C, axis=0)
    entry = {} if entry is None else entry
    got = engine.screen_paired_aligned_scores(ctx, alt, ref, bmc)
    out = {k: got[k].cpu().numpy() for k in SCORE_FIELDS}
    if "insulation_widths" in entry:
        tracks = engine.screen_paired_insulation(ctx, alt, ref, entry["insulation_widths"], bmc)
        out.update((k, t.cpu().numpy()) for k, t in zip(("insulation", "ref_insulation", "insulation_delta"), tracks))
        if "boundary_params" in entry:                   # two launches over the tracks that are on the device; the maps are not needed again
            q = entry["boundary_params"]
            ac, rc = (_to_host({k: v for k, v in engine.screen_boundary_calls(ctx, t, q.min_strength, q.max_calls, strength_track=False).items() if v is not None})
                      for t in tracks[:2])
            out.update(_paired_boundary_fields(rc, ac, out["insulation"], out["ref_insulation"], out["insulation_delta"], bmc, q.tol))
    if "viewpoint_bins" in entry:
        aligned, _ = engine.screen_paired_viewpoints(ctx, alt, ref, np.repeat(entry["viewpoint_bins"], C, axis=0), bmc)
        out["viewpoint_delta"] = aligned.cpu().numpy()
    if "strata_range" in entry:
        st = engine.screen_paired_strata_scores(ctx, alt, ref, bmc, entry["strata_range"])
        out.update(("strata_corr" if k == "corr" else k, st[k].cpu().numpy()) for k in STRATA_FIELDS)       # the strata kernel's ``corr`` is ``strata_corr`` in an entry
    if "loop_params" in entry:
        out.update(_model_loops(ctx, alt, ref, bmc, entry["loop_params"]))
    if "compartment_params" in entry:
        rp, ap = (np.repeat(entry[k], C, axis=0) if k in entry else None for k in ("ref_gc", "gc"))
        out.update(_model_compartments(ctx, alt, ref, bmc, entry["compartment_params"], rp, ap))
    return {k: v.reshape((lv, C) + v.shape[1:]) for k, v in out.items()}
