"""The readouts of the 1 Mb screen on the device: the result classes, and one unit per readout (the counterpart of sv_readouts.py).

`screen._run_screen` owns the routes - how a batch's final maps come about.  What is read from them is a list of `Readout` units, each with its
own fields of the `ScreenResult`: `MapScores`, `Insulation` (with the boundary calls on its tracks), `Viewpoints`, `Strata`, `Loops`, and the
`EpistasisBank` that `epistasis_1m` appends.  `readout_units` checks the screen's readout arguments and builds the list; `Run` is what the units
share.  The units are independent launches on the same maps, so a screen with several readouts gives every one of them the bits it gives alone.
map_readouts.py restates every readout in numpy.
"""
from collections import namedtuple
from dataclasses import dataclass, field
from typing import Optional

import numpy as np
import torch

from . import engine
from .map_readouts import (STRATA_FIELDS, BoundaryParams, LoopParams, _boundary_fields, _follow_loops, _match_loops, check_boundaries_arg, check_insulation,
                           check_loops_arg, check_regions, check_strata, check_viewpoints)


@dataclass
class EpistasisResult:
    """Result of `epistasis_1m` (device tensors unless said otherwise).  U singles, E sets; S_e the map of set e, A_m the map of its member m applied
    alone (both from ``screen``, so with ``strands="both"`` the merged maps), ref = ``screen.ref_map``.  Per pixel, every operand converted to fp64
    first: t = sum_m (A_m - ref), the additive expectation; r = (S_e - ref) - t, the residual.  Every field is rounded to fp32 once:
      screen            the `ScreenResult` of ``singles + sets`` (items [0, U) the singles, item U + e set e)
      singles           list of `Edit`, n_singles = U; member_off [E + 1] int64 and members [P] int32 (numpy): `epistasis_items`' table
      epi_profile       [E, n]  mean_j |r[i, j]|
      epi_abs_mean      [E]     mean_ij |r|
      epi_abs_max       [E]     max_ij |r|
      additive_abs_mean [E]     mean_ij |t|: the scale to set ``epi_abs_mean`` against
      epi_region        [E, K]  with ``regions``: the mean of r over rectangle k (signed; positive = more contact than the members' effects add up to)
      epi_region_abs    [E, K]  the mean of |r| over rectangle k
    A one-member set scores exactly 0 wherever its map holds its single's bits (on the two-part route it does).  `epistasis_scores_host` computes
    the same from maps on the host."""
    screen: "ScreenResult"
    singles: list
    n_singles: int
    member_off: np.ndarray
    members: np.ndarray
    epi_profile: torch.Tensor
    epi_abs_mean: torch.Tensor
    epi_abs_max: torch.Tensor
    additive_abs_mean: torch.Tensor
    epi_region: Optional[torch.Tensor] = None
    epi_region_abs: Optional[torch.Tensor] = None


@dataclass
class ScreenResult:
    """Result of `screen_1m` (device tensors).  Maps are the model's output, the log observed / expected map of ``_Orca1M.forward`` (the
    background cancels in the differences).  With d = |alt map - ref_map|:
      ref_map          [n, n]         the unedited window's map;  ref_1d [num_1d, n] its 1-D head (None without one)
      delta_profile    [E, n]         delta_profile[e, i] = mean_j d[e, i, j]  (mean |alt - ref| of map row i)
      delta_abs_mean   [E]            delta_abs_mean[e] = mean_ij d[e, i, j]
      delta_abs_max    [E]            delta_abs_max[e] = max_ij d[e, i, j]
      delta_1d         [E, num_1d, n] alt 1-D head - ref_1d (signed; None without a 1-D head)
      maps             [E, n, n]      the alt maps (``keep_maps=True`` only)
      delta_region     [E, K]         mean of alt - ref (signed) over rectangle k of ``regions`` (None without regions)
      delta_region_abs [E, K]         mean of |alt - ref| over rectangle k (None without regions)
      shift            [E] int64      bases removed minus bases inserted by the item (0 without ``del`` / ``ins``).  The alt window is anchored at
                                      the window's first base, so what lies behind the item's last member sits ``shift`` bases (shift / 4000
                                      bins) earlier in the alt map than in ``ref_map``.  The ``delta_*`` scores above compare bin with bin all the
                                      same, so behind an unbalanced indel they also hold that displacement; the ``aligned_*`` fields below do not
    With ``aligned=True`` (None otherwise), all indexed by ALT bin; M = the alt bins of item e that stand for a reference bin, c = |M|,
    d[i, j] = |alt map[i, j] - ref_map[map i, map j]| for i, j in M:
      bin_map            [E, n] int32 the reference bin alt bin i stands for, -1 for none (`bin_map` states the rule)
      aligned_bins       [E] int64    c, the number of mapped bins
      aligned_profile    [E, n]       sum_{j in M} d[i, j] / c; NaN for i outside M
      aligned_abs_mean   [E]          sum_{i, j in M} d / c^2 (NaN when c = 0)
      aligned_abs_max    [E]          max over M x M (NaN when c = 0)
      aligned_region     [E, K]       with ``regions``, read as REFERENCE bins: the mean of alt[i, j] - ref[map i, map j] (signed) over the alt
                                      pairs with map i in [i0, i1) and map j in [j0, j1); NaN when none qualifies (the region was deleted)
      aligned_region_abs [E, K]       the mean of its absolute value over the same pairs
    With ``strands="both"`` every map above is the MERGED map 0.5 plus + 0.5 flip(minus) (minus = the model's map of the reverse complement of the
    item's alt window, flip reverses both bin axes; forward orientation, so bins, regions and `bin_map` keep their meaning), every score is taken
    from merged maps against the merged ``ref_map``, the 1-D heads are 0.5 h_plus + 0.5 h_minus.flip(-1), and (None with ``strands="+"``):
      strand_gap         [E]          mean over the map of |(alt+ - ref+) - flip(alt- - ref-)|: how far the two strands disagree about the item's
                                      effect - set it beside ``delta_abs_mean``: an effect well above its gap is one both strands see
      ref_strand_gap     0-dim        mean |ref+ - flip(ref-)|: the model's strand asymmetry on the unedited window
    With ``insulation=`` (None otherwise; W widths).  The diamond of bin i at width w is rows [i - w, i) x columns (i, i + w] of a map - bin i's own
    row and column left out; it fits when w <= i < n - w.  ins_w(m)[i] = the mean of m over it (fp64), NaN where it does not fit; lower = more
    insulated, so a boundary is a dip, and a positive difference at a bin says the boundary there weakened:
      insulation_widths  [W] int32    the widths, in bins
      ref_insulation     [W, n]       ins_w(ref_map)
      insulation         [E, W, n]    ins_w(alt map)
      delta_insulation   [E, W, n]    ins(alt)[i] - ins(ref)[i] (signed; the difference of the fp64 means, rounded once)
      aligned_insulation [E, W, n]    with ``aligned=True``: ins(alt)[i] - ins(ref)[map i], indexed by ALT bin; NaN where alt bin i stands for no reference
                                      bin or a diamond does not fit.  Only the centre bin has to be mapped - the alt diamond may hold inserted bases or
                                      refill.  Where the bin map is the identity it is ``delta_insulation`` bit for bit
    With ``viewpoints=`` (None otherwise; V bins) - a virtual 4C, the signed row of a bin:
      viewpoint_bins     [V] int32    the viewpoint bins
      delta_viewpoint    [E, V, n]    alt map[view, j] - ref_map[view, j] (fp32)
      aligned_viewpoint  [E, V, n]    with ``aligned=True``: the viewpoint is a REFERENCE bin.  R = the alt bins that stand for it, c = |R|:
                                      (sum_{i in R} alt map[i, j]) / c - ref_map[view, map j], indexed by ALT column j; NaN when c = 0 (the viewpoint was
                                      deleted) or column j stands for nothing
    With ``strata=`` (None otherwise) - how similar the alt map is to ``ref_map``, by genomic distance.  Stratum d is the pairs (i, i + d) of the upper
    triangle, x = the alt pixel, y = the reference pixel, dl = x - y, all in fp64; mx_d, my_d the stratum's means, X_d, Y_d, C_d its centred sums
    of squares and of products (two passes), c_d = n - d its pairs:
      strata_range       (d_lo, d_hi) the strata the three per-map scores run over
      dist_delta         [E, n]       the mean of dl over stratum d: the change of the distance-decay curve (a deletion lifts whole bands)
      dist_abs           [E, n]       the mean of |dl|
      dist_rms           [E, n]       sqrt(mean of dl^2)
      dist_corr          [E, n] f64   C_d / sqrt(X_d Y_d), the Pearson correlation within the stratum: a uniform shift of the band leaves it at 1, a
                                      re-patterning lowers it.  NaN when c_d < 2 or either side is constant there.  fp64: 1 - r of a small edit survives
      mse                [E]          sum_d sum dl^2 / c over d_lo <= d < d_hi, c = sum_d c_d
      corr               [E] f64      the Pearson correlation over all pairs of those strata (from the pooled centred sums)
      scc                [E] f64      sum_d C_d / sum_d sqrt(X_d Y_d): HiCRep's stratum-adjusted correlation (its weights c_d sqrt(var_x var_y)) on raw
                                      values - no smoothing, no rank transform; read an effect as 1 - scc
    and with ``aligned=True`` the same over the pairs whose two alt bins stand for reference bins, y = ref_map[map i, map (i + d)] (the stratum is
    the ALT distance; where the bin map is the identity they are the fields above bit for bit):
      aligned_dist_delta, aligned_dist_abs, aligned_dist_rms, aligned_dist_corr [E, n];  aligned_mse, aligned_corr, aligned_scc [E]
      aligned_dist_count [E, n] int32 c_d, the mapped pairs of stratum d; every per-stratum value is NaN where it is 0
    A NaN pixel at a pair of stratum d makes that stratum's values NaN and, if d_lo <= d < d_hi, the three per-map scores; nothing else.
    With ``loops=`` (None otherwise) - dot calls (`LoopParams`; include/orca_hip.h, orca_screen_dot_calls, defines eligible pixels, the
    enrichment e and a dot).  K = max_calls, R = min(ref_loop_count, K):
      loop_params        LoopParams   the validated parameters (d_min resolved)
      ref_loops          [R, 2] int32 the reference map's dots (i, j), row-major;  ref_loop_enrichment [R] their e;  ref_loop_count (int) all of them
      loops              [E, K, 2] int32  the first K dots of every alt map, row-major, -1 behind them;  loop_enrichment [E, K] their e, NaN behind
      loop_count         [E] int32    all dots of the alt map (above K the list is truncated)
      loop_delta         [E, R]       e of the alt map at reference dot k's pixel minus the reference's e there: "this loop weakened by x";
                                      NaN where the alt e is (a NaN pixel in the window)
      loop_is_gained     [E, K] bool  a listed alt dot with no reference dot within Chebyshev distance tol;  loops_gained [E] int32 their number
      ref_loop_is_lost   [E, R] bool  a reference dot with no listed alt dot within tol;  loops_lost [E] int32 their number
    and with ``aligned=True`` aligned_loop_delta, aligned_loop_is_gained, aligned_loops_gained, aligned_ref_loop_is_lost, aligned_loops_lost:
    reference dot (i, j) is followed to alt pixel (lowest a with map a = i, highest b with map b = j) - NaN when either bin does not exist or
    the pixel is ineligible - and an alt dot (a, b) stands for (map a, map b), gained if either bin is unmapped; where the bin map is the
    identity they hold the plain fields' bits.
    With ``insulation=`` and ``boundaries=`` (None otherwise) - domain boundary calls on the insulation tracks above, per width (`BoundaryParams`;
    include/orca_hip.h, orca_screen_boundary_calls, defines a minimum, its strength - the prominence of the dip, in mean log observed / expected -
    and a call).  K = max_calls; a list slot beyond a track's boundaries holds -1 / NaN / False:
      boundary_params          BoundaryParams  the validated parameters
      ref_boundaries           [W, K] int32    the boundaries of ``ref_insulation``, ascending;  ref_boundary_strength [W, K] their strengths;
                                               ref_boundary_count [W] int32 all of them (above K the list is truncated)
      boundaries               [E, W, K] int32 the boundaries of ``insulation``;  boundary_strength [E, W, K];  boundary_count [E, W] int32
      boundary_followed_at     [E, W, K] int32 per REFERENCE boundary k: the alt bin of its partner - the matching alt boundary (within tol bins) of
                                               largest strength, the lower bin of equals - or -1
      boundary_strength_delta  [E, W, K]       the partner's strength - the reference strength: "this boundary weakened by x"; -the reference
                                               strength when lost; NaN when unmapped
      boundary_delta           [E, W, K]       ``delta_insulation`` at the reference boundary's own bin (positive = less insulated there)
      ref_boundary_is_lost     [E, W, K] bool  a mapped reference boundary without a partner;  boundaries_lost [E, W] int32 their number
      boundary_is_gained       [E, W, K] bool  per ALT boundary: mapped, and no listed reference boundary within tol;  boundaries_gained [E, W] int32
      boundary_is_unmapped, ref_boundary_is_unmapped [E, W, K] bool  neither lost nor gained: an alt boundary whose bin stands for no reference bin
                                               or for one where ``ref_insulation`` is NaN; a reference boundary with no alt bin within tol whose
                                               ``insulation`` can be read
    and with ``aligned=True`` the ``aligned_`` forms of the nine matched fields (`BOUNDARY_MATCH_FIELDS`) through ``bin_map``: an alt boundary at
    alt bin a stands for reference bin map a, so a boundary that a deletion merely shifted is kept, one inside the deleted span is unmapped (not
    lost), and ``aligned_boundary_delta`` is ``aligned_insulation`` at the lowest alt bin that stands for the reference boundary's bin (NaN without
    one); where the bin map is the identity they hold the plain fields' bits.  The default ``min_strength`` is NOT calibrated.
    `scores_host` computes the three map scores from maps on the host, `region_scores_host` the two region scores, `aligned_scores_host` and
    `aligned_region_scores_host` the aligned ones, `insulation_scores_host` and `viewpoint_scores_host` the tracks, `strata_scores_host` the
    distance-stratified scores, `loop_scores_host` the loop fields, `boundary_scores_host` the boundary fields."""
    ref_map: torch.Tensor
    ref_1d: Optional[torch.Tensor]
    delta_profile: torch.Tensor
    delta_abs_mean: torch.Tensor
    delta_abs_max: torch.Tensor
    delta_1d: Optional[torch.Tensor] = None
    maps: Optional[torch.Tensor] = None
    edits: list = field(default_factory=list)
    delta_region: Optional[torch.Tensor] = None
    delta_region_abs: Optional[torch.Tensor] = None
    shift: Optional[torch.Tensor] = None
    bin_map: Optional[torch.Tensor] = None
    aligned_bins: Optional[torch.Tensor] = None
    aligned_profile: Optional[torch.Tensor] = None
    aligned_abs_mean: Optional[torch.Tensor] = None
    aligned_abs_max: Optional[torch.Tensor] = None
    aligned_region: Optional[torch.Tensor] = None
    aligned_region_abs: Optional[torch.Tensor] = None
    strand_gap: Optional[torch.Tensor] = None
    ref_strand_gap: Optional[torch.Tensor] = None
    insulation_widths: Optional[torch.Tensor] = None
    ref_insulation: Optional[torch.Tensor] = None
    insulation: Optional[torch.Tensor] = None
    delta_insulation: Optional[torch.Tensor] = None
    aligned_insulation: Optional[torch.Tensor] = None
    viewpoint_bins: Optional[torch.Tensor] = None
    delta_viewpoint: Optional[torch.Tensor] = None
    aligned_viewpoint: Optional[torch.Tensor] = None
    strata_range: Optional[tuple] = None
    dist_delta: Optional[torch.Tensor] = None
    dist_abs: Optional[torch.Tensor] = None
    dist_rms: Optional[torch.Tensor] = None
    dist_corr: Optional[torch.Tensor] = None
    mse: Optional[torch.Tensor] = None
    corr: Optional[torch.Tensor] = None
    scc: Optional[torch.Tensor] = None
    aligned_dist_delta: Optional[torch.Tensor] = None
    aligned_dist_abs: Optional[torch.Tensor] = None
    aligned_dist_rms: Optional[torch.Tensor] = None
    aligned_dist_corr: Optional[torch.Tensor] = None
    aligned_dist_count: Optional[torch.Tensor] = None
    aligned_mse: Optional[torch.Tensor] = None
    aligned_corr: Optional[torch.Tensor] = None
    aligned_scc: Optional[torch.Tensor] = None
    loop_params: Optional[LoopParams] = None
    ref_loops: Optional[torch.Tensor] = None
    ref_loop_enrichment: Optional[torch.Tensor] = None
    ref_loop_count: Optional[int] = None
    loops: Optional[torch.Tensor] = None
    loop_enrichment: Optional[torch.Tensor] = None
    loop_count: Optional[torch.Tensor] = None
    loop_delta: Optional[torch.Tensor] = None
    loops_gained: Optional[torch.Tensor] = None
    loops_lost: Optional[torch.Tensor] = None
    loop_is_gained: Optional[torch.Tensor] = None
    ref_loop_is_lost: Optional[torch.Tensor] = None
    aligned_loop_delta: Optional[torch.Tensor] = None
    aligned_loops_gained: Optional[torch.Tensor] = None
    aligned_loops_lost: Optional[torch.Tensor] = None
    aligned_loop_is_gained: Optional[torch.Tensor] = None
    aligned_ref_loop_is_lost: Optional[torch.Tensor] = None
    boundary_params: Optional[BoundaryParams] = None
    ref_boundaries: Optional[torch.Tensor] = None
    ref_boundary_strength: Optional[torch.Tensor] = None
    ref_boundary_count: Optional[torch.Tensor] = None
    boundaries: Optional[torch.Tensor] = None
    boundary_strength: Optional[torch.Tensor] = None
    boundary_count: Optional[torch.Tensor] = None
    boundary_followed_at: Optional[torch.Tensor] = None
    boundary_strength_delta: Optional[torch.Tensor] = None
    boundary_delta: Optional[torch.Tensor] = None
    boundary_is_gained: Optional[torch.Tensor] = None
    ref_boundary_is_lost: Optional[torch.Tensor] = None
    boundary_is_unmapped: Optional[torch.Tensor] = None
    ref_boundary_is_unmapped: Optional[torch.Tensor] = None
    boundaries_gained: Optional[torch.Tensor] = None
    boundaries_lost: Optional[torch.Tensor] = None
    aligned_boundary_followed_at: Optional[torch.Tensor] = None
    aligned_boundary_strength_delta: Optional[torch.Tensor] = None
    aligned_boundary_delta: Optional[torch.Tensor] = None
    aligned_boundary_is_gained: Optional[torch.Tensor] = None
    aligned_ref_boundary_is_lost: Optional[torch.Tensor] = None
    aligned_boundary_is_unmapped: Optional[torch.Tensor] = None
    aligned_ref_boundary_is_unmapped: Optional[torch.Tensor] = None
    aligned_boundaries_gained: Optional[torch.Tensor] = None
    aligned_boundaries_lost: Optional[torch.Tensor] = None


# ---- the readout units ----------------------------------------------------------------------------------------------------------------------
UNSET_STATS = {"insulation_widths": 0, "viewpoints": 0, "strata": 0, "loops": 0, "loop_truncated_items": 0, "boundaries": 0}      # the units' ``stats`` of a screen that sets none of them
ReadoutArgs = namedtuple("ReadoutArgs", "regions insulation viewpoints strata loops boundaries", defaults=(None,) * 6)          # `screen_1m`'s readout arguments as given


class Run:
    """What every unit of one screen reads, built once after the reference: ``ctx``, ``dev``, ``E`` items, ``n`` bins, the final ``ref_map``
    (merged with ``strands="both"``), ``upload(array, dtype)``, and with ``aligned`` the items' bin maps on the host and on the device
    (``bin_maps`` int32 [E, n], ``bin_maps_dev``; both None without) and ``moved``: the items whose bin map is not the identity, ascending -
    the only ones an aligned matching on the host has to look at again."""

    def __init__(self, sc, E, ref_map, bin_maps=None):
        self.ctx, self.dev, self.E, self.n, self.ref_map, self.upload = sc.ctx, sc.dev, E, sc.n, ref_map, sc._upload
        self.aligned, self.bin_maps = bin_maps is not None, bin_maps
        self.bin_maps_dev = self.upload(bin_maps, torch.int32) if self.aligned else None
        self.moved = np.flatnonzero((bin_maps != np.arange(self.n, dtype=np.int32)[None]).any(axis=1)) if self.aligned else np.zeros(0, dtype=np.int64)

    def maps_of(self, i0, i1):
        """The bin maps of items [i0, i1) as the engine's wrappers take them, (host slice, device slice); (None, None) without ``aligned``."""
        return (self.bin_maps[i0:i1], self.bin_maps_dev[i0:i1]) if self.aligned else (None, None)

    def zeros(self, *shape, dtype=torch.float32):
        return torch.zeros(shape, dtype=dtype, device=self.dev)

    def full(self, shape, value, dtype):
        return torch.full(shape, value, dtype=dtype, device=self.dev)


class Readout:
    """One readout of the 1 Mb screen.  ``start(res, run)`` allocates its fields of the `ScreenResult`, computes the reference's own values and
    returns its ``stats`` entries; ``batch(res, run, i0, i1, maps)`` launches on the FINAL maps [i1 - i0, n, n] of items [i0, i1) - after the
    strand merge and any range fallback; the buffer is the batch's own, so it is read before the call returns - and writes its rows of the
    fields on the device; ``finish(res, run)`` is the host work after the last batch and returns ``stats`` entries too.  A readout that is
    not asked for is not in the list: nothing of it is launched."""

    def start(self, res, run):
        return {}

    def batch(self, res, run, i0, i1, maps):
        pass

    def finish(self, res, run):
        return {}


class MapScores(Readout):
    """The three map scores of every screen (orca_screen_scores) and, with ``regions`` / ``aligned``, the region scores and the aligned forms."""

    def __init__(self, rects=None):
        self.rects = rects

    def start(self, res, run):
        E, n, K = run.E, run.n, 0 if self.rects is None else len(self.rects)
        res.delta_profile, res.delta_abs_mean, res.delta_abs_max = run.zeros(E, n), run.zeros(E), run.zeros(E)
        if K:
            res.delta_region, res.delta_region_abs = run.zeros(E, K), run.zeros(E, K)
        if run.aligned:
            res.aligned_profile, res.aligned_abs_mean, res.aligned_abs_max = run.zeros(E, n), run.zeros(E), run.zeros(E)
            if K:
                res.aligned_region, res.aligned_region_abs = run.zeros(E, K), run.zeros(E, K)
        return {}

    def batch(self, res, run, i0, i1, maps):
        bm, bm_dev = run.maps_of(i0, i1)
        res.delta_profile[i0:i1], res.delta_abs_mean[i0:i1], res.delta_abs_max[i0:i1] = engine.screen_scores(run.ctx, maps, run.ref_map)
        if self.rects is not None:
            res.delta_region[i0:i1], res.delta_region_abs[i0:i1] = engine.screen_region_scores(run.ctx, maps, run.ref_map, self.rects)
        if run.aligned:
            res.aligned_profile[i0:i1], res.aligned_abs_mean[i0:i1], res.aligned_abs_max[i0:i1] = engine.screen_aligned_scores(run.ctx, maps, run.ref_map, bm, bm_dev)
            if self.rects is not None:
                res.aligned_region[i0:i1], res.aligned_region_abs[i0:i1] = engine.screen_aligned_region_scores(run.ctx, maps, run.ref_map, bm, self.rects, bm_dev)


class Insulation(Readout):
    """The insulation tracks (orca_screen_insulation) and, with ``bp`` (a checked `BoundaryParams`), the boundary calls on the tracks a batch has
    just produced (orca_screen_boundary_calls), matched on the host after the last batch."""

    def __init__(self, widths, bp=None):
        self.widths, self.bp = widths, bp

    def start(self, res, run):                           # the reference's own tracks once, from the final (merged) reference map, and its boundaries from them
        E, n, W, bp = run.E, run.n, len(self.widths), self.bp
        res.insulation_widths = run.upload(self.widths, torch.int32)
        res.ref_insulation = engine.screen_insulation(run.ctx, run.ref_map[None], None, self.widths)[0][0]
        res.insulation, res.delta_insulation = run.zeros(E, W, n), run.zeros(E, W, n)
        if run.aligned:
            res.aligned_insulation = run.zeros(E, W, n)
        if bp is not None:
            got = engine.screen_boundary_calls(run.ctx, res.ref_insulation[None], bp.min_strength, bp.max_calls, strength_track=False)
            res.boundary_params = bp
            res.ref_boundaries, res.ref_boundary_strength, res.ref_boundary_count = got["bins"][0], got["strength"][0], got["count"][0]
            res.boundaries = run.full((E, W, bp.max_calls), -1, torch.int32)
            res.boundary_strength = run.full((E, W, bp.max_calls), float("nan"), torch.float32)
            res.boundary_count = run.zeros(E, W, dtype=torch.int32)
        return {"insulation_widths": W, "boundaries": 0 if bp is None else bp.max_calls}

    def batch(self, res, run, i0, i1, maps):
        bp = self.bp
        tr, dl, al = engine.screen_insulation(run.ctx, maps, run.ref_map, self.widths, *run.maps_of(i0, i1))
        res.insulation[i0:i1], res.delta_insulation[i0:i1] = tr, dl
        if run.aligned:
            res.aligned_insulation[i0:i1] = al
        if bp is not None:
            got = engine.screen_boundary_calls(run.ctx, tr, bp.min_strength, bp.max_calls, strength_track=False)
            res.boundaries[i0:i1], res.boundary_strength[i0:i1], res.boundary_count[i0:i1] = got["bins"], got["strength"], got["count"]

    def finish(self, res, run):
        """The matched boundary fields (`BOUNDARY_MATCH_FIELDS`, and with ``aligned`` their ``aligned_`` forms): `_boundary_fields` on the lists and
        the tracks' NaN pattern, copied to the host once; ``boundary_delta`` is gathered on the device."""
        if self.bp is None:
            return {}
        (E, W, n), K, tol = res.insulation.shape, self.bp.max_calls, self.bp.tol
        host = lambda t: t.cpu().numpy().reshape((E * W,) + tuple(t.shape[2:]))
        alt = {"bins": host(res.boundaries), "strength": host(res.boundary_strength)}
        ref = {k: np.ascontiguousarray(np.broadcast_to(v.cpu().numpy(), (E, W, K))).reshape(E * W, K)
               for k, v in (("bins", res.ref_boundaries), ("strength", res.ref_boundary_strength))}
        ta, tr = host(res.insulation), np.ascontiguousarray(np.broadcast_to(res.ref_insulation.cpu().numpy(), (E, W, n))).reshape(E * W, n)
        nan = run.full((), float("nan"), torch.float32)
        got = None
        for pre in ("", "aligned_") if run.aligned else ("",):
            if not pre:
                got = _boundary_fields(alt, ref, ta, tr, tol)
            else:                                        # an identity bin map changes nothing: only the other items are matched again
                moved = (run.moved[:, None] * W + np.arange(W)[None]).reshape(-1)
                got = {k: v.copy() for k, v in got.items()}
                if moved.size:
                    sub = lambda d: {k: v[moved] for k, v in d.items()}
                    for k, v in _boundary_fields(sub(alt), sub(ref), ta[moved], tr[moved], tol, np.repeat(run.bin_maps, W, axis=0)[moved]).items():
                        got[k][moved] = v
            for k, v in got.items():
                if k != "first_at":
                    setattr(res, pre + k, run.upload(v.reshape((E, W) + v.shape[1:]), {"b": torch.bool, "i": torch.int32, "f": torch.float32}[v.dtype.kind]))
            at_dev = run.upload(got["first_at"].reshape(E, W, K), torch.int64)
            src = res.aligned_insulation if pre else res.delta_insulation
            setattr(res, pre + "boundary_delta", torch.where(at_dev >= 0, torch.gather(src, 2, at_dev.clamp(min=0)), nan))
        return {}


class Viewpoints(Readout):
    """The viewpoint profiles (orca_screen_viewpoints)."""

    def __init__(self, views):
        self.views = views

    def start(self, res, run):
        res.viewpoint_bins = run.upload(self.views, torch.int32)
        res.delta_viewpoint = run.zeros(run.E, len(self.views), run.n)
        if run.aligned:
            res.aligned_viewpoint = run.zeros(run.E, len(self.views), run.n)
        return {"viewpoints": len(self.views)}

    def batch(self, res, run, i0, i1, maps):
        dl, al = engine.screen_viewpoints(run.ctx, maps, run.ref_map, self.views, *run.maps_of(i0, i1))
        res.delta_viewpoint[i0:i1] = dl
        if run.aligned:
            res.aligned_viewpoint[i0:i1] = al


class Strata(Readout):
    """The distance-stratified scores (orca_screen_strata_scores): bin with bin, then with ``aligned`` a second call through the bin maps."""

    def __init__(self, drange):
        self.drange = drange

    def start(self, res, run):
        res.strata_range = self.drange
        for pre in ("", "aligned_") if run.aligned else ("",):
            for name in STRATA_FIELDS:
                setattr(res, pre + name, run.zeros(*((run.E, run.n) if name.startswith("dist_") else (run.E,)),
                                                   dtype=torch.float64 if name in ("dist_corr", "corr", "scc") else torch.float32))
        if run.aligned:
            res.aligned_dist_count = run.zeros(run.E, run.n, dtype=torch.int32)
        return {"strata": self.drange[1] - self.drange[0]}

    def batch(self, res, run, i0, i1, maps):
        got = engine.screen_strata_scores(run.ctx, maps, run.ref_map, None, self.drange)
        for name in STRATA_FIELDS:
            getattr(res, name)[i0:i1] = got[name]
        if run.aligned:
            bm, bm_dev = run.maps_of(i0, i1)
            got = engine.screen_strata_scores(run.ctx, maps, run.ref_map, bm, self.drange, bm_dev)
            for name in STRATA_FIELDS + ("dist_count",):
                getattr(res, "aligned_" + name)[i0:i1] = got[name]


class Loops(Readout):
    """The dot calls (orca_screen_dot_calls), the change of the enrichment at the reference's dots - with ``aligned`` also at the pixels they were
    followed to (orca_screen_dot_enrichment) - and the matching of the lists on the host after the last batch."""

    def __init__(self, lp):
        self.lp = lp

    def start(self, res, run):                           # the reference's dots once, from the final (merged) reference map
        lp, E = self.lp, run.E
        got = engine.screen_dot_calls(run.ctx, run.ref_map[None], lp.p, lp.w, lp.r, lp.threshold, lp.max_calls, lp.d_min)
        res.loop_params, res.ref_loop_count = lp, int(got["count"][0])
        R, K = min(res.ref_loop_count, lp.max_calls), lp.max_calls
        res.ref_loops, res.ref_loop_enrichment = got["ij"][0, :R].contiguous(), got["enrich"][0, :R].contiguous()
        self.ref_ij, self.ref_pix, self.followed = res.ref_loops.cpu().numpy(), res.ref_loops.long(), None
        res.loops = run.full((E, K, 2), -1, torch.int32)
        res.loop_enrichment = run.full((E, K), float("nan"), torch.float32)
        res.loop_count = run.zeros(E, dtype=torch.int32)
        res.loop_delta = run.zeros(E, R)
        if run.aligned:                                  # every reference dot followed to its alt pixel, per item: (-1, -1) where it has none
            res.aligned_loop_delta = run.full((E, R), float("nan"), torch.float32)
            self.followed = _follow_loops(run.bin_maps, self.ref_ij, lp)
        return {"loops": K}

    def batch(self, res, run, i0, i1, maps):
        lp, pix = self.lp, self.ref_pix
        got = engine.screen_dot_calls(run.ctx, maps, lp.p, lp.w, lp.r, lp.threshold, lp.max_calls, lp.d_min)
        res.loops[i0:i1], res.loop_enrichment[i0:i1], res.loop_count[i0:i1] = got["ij"], got["enrich"], got["count"]
        if pix.shape[0]:
            res.loop_delta[i0:i1] = got["e_map"][:, pix[:, 0], pix[:, 1]] - res.ref_loop_enrichment[None]
            if run.aligned:
                res.aligned_loop_delta[i0:i1] = engine.screen_dot_enrichment(run.ctx, maps, self.followed[i0:i1], lp.p, lp.w, lp.d_min) - res.ref_loop_enrichment[None]

    def finish(self, res, run):                          # the lists are tiny: one copy to the host, the matching in numpy
        lp, moved = self.lp, run.moved
        alt_ij = res.loops.cpu().numpy()
        for pre in ("", "aligned_") if run.aligned else ("",):
            if not pre:
                gained, lost = _match_loops(alt_ij, self.ref_ij, lp.tol)
            else:                                        # an identity bin map changes nothing: only the other items are matched again
                gained, lost = gained.copy(), lost.copy()
                gained[moved], lost[moved] = _match_loops(alt_ij[moved], self.ref_ij, lp.tol, run.bin_maps[moved])
            setattr(res, pre + "loop_is_gained", run.upload(gained, torch.bool))
            setattr(res, pre + "ref_loop_is_lost", run.upload(lost, torch.bool))
            setattr(res, pre + "loops_gained", run.upload(gained.sum(axis=1), torch.int32))
            setattr(res, pre + "loops_lost", run.upload(lost.sum(axis=1), torch.int32))
        return {"loop_truncated_items": int((res.loop_count > lp.max_calls).sum())}


class EpistasisBank(Readout):
    """The unit `epistasis_1m` appends to a screen of ``singles + sets``: the singles' final maps go into a device bank [U, n, n], and every set's
    map is scored against it in the batch that holds it (orca_screen_epistasis_scores, orca_screen_epistasis_region_scores) into ``out``, the
    `EpistasisResult` that carries the member table.  The singles come first, so every member is banked before a set needs it."""

    def __init__(self, out, rects=None):
        self.out, self.rects = out, rects

    def start(self, res, run):
        out, E, n = self.out, len(self.out.member_off) - 1, run.n
        self.bank = torch.empty((out.n_singles, n, n), dtype=torch.float32, device=run.dev)
        out.epi_profile, out.epi_abs_mean, out.epi_abs_max, out.additive_abs_mean = run.zeros(E, n), run.zeros(E), run.zeros(E), run.zeros(E)
        if self.rects is not None:
            out.epi_region, out.epi_region_abs = run.zeros(E, len(self.rects)), run.zeros(E, len(self.rects))
        return {}

    def batch(self, res, run, i0, i1, maps):
        out, U, member_off = self.out, self.out.n_singles, self.out.member_off
        if i0 < U:                                       # the batch's singles into the bank, before its sets are scored
            self.bank[i0: min(i1, U)] = maps[: min(i1, U) - i0]
        if i1 <= U:
            return
        s0 = max(i0, U)
        e0, e1 = s0 - U, i1 - U
        off = member_off[e0: e1 + 1] - member_off[e0]
        got = engine.screen_epistasis_scores(run.ctx, maps[s0 - i0:], self.bank, res.ref_map, off, out.members[member_off[e0]: member_off[e1]], self.rects)
        out.epi_profile[e0:e1], out.epi_abs_mean[e0:e1], out.epi_abs_max[e0:e1], out.additive_abs_mean[e0:e1] = got[:4]
        if self.rects is not None:
            out.epi_region[e0:e1], out.epi_region_abs[e0:e1] = got[4:]


def readout_units(args, n):
    """The units of a screen on maps of n bins from its readout arguments as given (a `ReadoutArgs`), in their launch order within a batch.  The
    arguments are checked here, in the order of the fields, before anything is launched; an unset one gives no unit.  A new readout is one more
    class above, one more field and one more line here."""
    rects = None if args.regions is None else check_regions(args.regions, n)
    widths = None if args.insulation is None else check_insulation(args.insulation, n)
    views = None if args.viewpoints is None else check_viewpoints(args.viewpoints, n)
    drange = None if args.strata is None or args.strata is False else check_strata(args.strata, n)
    lp = check_loops_arg(args.loops, n)
    bp = check_boundaries_arg(args.boundaries, n, args.insulation)
    units = [MapScores(rects), None if widths is None else Insulation(widths, bp), None if views is None else Viewpoints(views),
             None if drange is None else Strata(drange), None if lp is None else Loops(lp)]
    return [u for u in units if u is not None]
