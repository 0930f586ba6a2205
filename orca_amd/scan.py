"""A whole chromosome through the 1 Mb model (``H1esc_1M`` / ``Hff_1M``, ``Net``), stitched on the device.

The screens (`screen.screen_1m`, `sv.sv_screen`) are relative: an edit or a structural variant against its own reference window.  `scan_1m`
answers the absolute question: what does the model predict along this chromosome, and where are its domain boundaries?  The 1 Mb model gives
one n x n map per call (n = 250), so a chromosome is hundreds of overlapping windows.  `scan_1m` predicts them in batches through the same
Encoder and Decoder_1m as `Net.forward` and never brings a window map to the host: every batch is accumulated into ONE banded map of the
chromosome stretch,

    band[i, d] = the mean over the windows that cover it of pixel (i, i + d),     0 <= i < N,  0 <= d < D

(orca_scan_stitch_band, orca_scan_band_finish), the insulation diamond runs on that band (orca_scan_band_insulation) and the boundary strengths
on the chromosome-long tracks (orca_scan_boundary_strength); include/orca_hip.h has the definitions.  The ordered boundary lists are made on the
host from the strength array, which is small.  ``loops=`` calls the dots (`screen.LoopParams`, the screens' third readout) on the band itself: the
enrichment of every band pixel (orca_scan_band_dot_enrichment) and ALL its local maxima as one ordered list made on the device
(orca_scan_band_dot_offsets, orca_scan_band_dot_list).

*Coverage.*  A window is trusted on its bins [trim, n - trim): window b, which starts at chromosome bin off[b], covers pixel (i, d) when
r = i - off[b] has trim <= r and r + d <= n - 1 - trim.  `plan_windows` lays the windows out and `full_depth` says how many distances have no
holes; `scan_1m` refuses a deeper band, so the only uncovered pixels are the ``trim`` bins at either end of the stretch.

*Mean and range.*  Where windows overlap the band holds their mean - every window saw the pixel with a different context, and none is
privileged - summed in fp64 in ascending window order, so the bits do not depend on ``batch``.  ``spread=True`` adds ``band_range`` = the largest
minus the smallest of the values a pixel got: how far the overlapping windows disagree, the scan's confidence readout as ``strand_gap`` is the
strands'.  A NaN from the model stays a NaN in mean and range.

`stitch_band_host` and `band_insulation_host` restate the kernels in numpy; `screen.boundary_strength_host` is the restatement of the fourth, and
`band_dot_enrichment_host` / `band_dot_calls_host` of the loop kernels.

The defaults of ``trim_bins``, of `screen.BoundaryParams.min_strength` and of `screen.LoopParams.threshold` are NOT calibrated on the published
checkpoints - nobody on this project has them."""
from dataclasses import dataclass
from typing import Optional

import numpy as np
import torch

from . import engine
from ._lib import OrcaHipError
from .map_readouts import BIN_BP, BoundaryParams, LoopParams, _dot_enrichment_of, _loop_params, _widths, check_band_loops
from .screen import _net_of

MAX_BINS = 256                      # bins of a window map (Net.forward's limit)


# ---- the window planner ----------------------------------------------------------------------------------------------------------------------
def _check_plan(n, step, trim):
    n, step, trim = int(n), int(step), int(trim)
    if n < 1 or step < 1 or trim < 0 or n - 2 * trim < 1:
        raise ValueError(f"windows of {n} bins every {step} bins, trimmed by {trim}: n >= 1, step >= 1, trim >= 0 and n - 2 trim >= 1")
    return n, step, trim


def plan_windows(n_total, n, step, trim):
    """The chromosome bins at which the windows of a scan start, int64, strictly ascending: 0, step, 2 step, ... while the offset is <= n_total - n,
    plus a final n_total - n if it is not already the last - so the last window ends with the stretch, and consecutive offsets differ by at most
    ``step``.  ``n_total``: bins of the stretch (>= n); ``n``: bins of a window map; ``trim`` only has to be legal for n (`full_depth` uses it)."""
    n, step, trim = _check_plan(n, step, trim)
    n_total = int(n_total)
    if n_total < n:
        raise ValueError(f"a stretch of {n_total} bins holds no window of {n} bins")
    off = list(range(0, n_total - n + 1, step))
    if off[-1] != n_total - n:
        off.append(n_total - n)
    return np.array(off, dtype=np.int64)


def full_depth(n, step, trim):
    """n - 2 trim - step + 1: the number D of distances at which EVERY pixel (i, d), d < D, with trim <= i and i + d <= n_total - 1 - trim is covered
    by at least one window of `plan_windows(n_total, n, step, trim)`, whatever n_total >= n.  May be <= 0: then ``step`` is too wide for the trim.

    Proof.  Window o covers (i, d) when trim <= i - o and i - o + d <= n - 1 - trim, that is when o lies in I = [i + d - n + 1 + trim, i - trim], an
    interval of n - 2 trim - d integers, which is >= step for d < D.  The offsets are a subset of [0, n_total - n] that holds both ends and whose
    consecutive members differ by at most ``step``.  Because trim <= i, I does not end below 0; because i + d <= n_total - 1 - trim, it does not begin
    above n_total - n.  So either I holds 0, or it holds n_total - n - both are offsets - or it lies inside [0, n_total - n], and >= step consecutive
    integers there cannot fit strictly between two offsets at most ``step`` apart.  The bound is sharp: at d = D the interval has step - 1 integers and
    fits between two offsets exactly ``step`` apart (the pixel i = o + step - 1 + trim behind such an offset o is then covered by no window)."""
    n, step, trim = _check_plan(n, step, trim)
    return n - 2 * trim - step + 1


# ---- host restatements ---------------------------------------------------------------------------------------------------------------------------
def stitch_band_host(maps, off, trim, N, D):
    """Host restatement of orca_scan_stitch_band + orca_scan_band_finish: window maps [B, n, n] (float32) that start at the chromosome bins ``off``
    [B] (strictly ascending, 0 <= off <= N - n), stitched into (band [N, D] float32, count [N, D] int32, range [N, D] float32).  Window b covers
    pixel (i, d) when r = i - off[b] has trim <= r and r + d <= n - 1 - trim; only maps[b, r, r + d], the upper triangle, is read.  Per pixel the
    covering values are added in fp64 in ascending b - the kernel's order, so the same bits - and band = float32(sum / count), range = hi - lo in
    fp32 (0 under one window); both NaN where count = 0.  A NaN value makes the pixel's band and range NaN."""
    m = np.asarray(maps, dtype=np.float32)
    o = np.asarray(off, dtype=np.int64).reshape(-1)
    if m.ndim != 3 or m.shape[1] != m.shape[2] or o.size != m.shape[0] or m.shape[0] < 1:
        raise ValueError("maps: [B, n, n] with one offset each")
    B, n = m.shape[0], m.shape[1]
    trim, N, D = int(trim), int(N), int(D)
    if trim < 0 or not 1 <= D <= n - 2 * trim:
        raise ValueError(f"trim = {trim}, D = {D}: trim >= 0 and 1 <= D <= n - 2 trim = {n - 2 * trim}")
    if o[0] < 0 or o[-1] > N - n or np.any(np.diff(o) <= 0):
        raise ValueError("off: strictly ascending inside 0 .. N - n")
    s, c = np.zeros((N, D), dtype=np.float64), np.zeros((N, D), dtype=np.int32)
    lo, hi = np.full((N, D), np.inf, dtype=np.float32), np.full((N, D), -np.inf, dtype=np.float32)
    for b in range(B):
        for d in range(D):
            r = np.arange(trim, n - trim - d)                   # trim <= r and r + d <= n - 1 - trim
            if r.size == 0:
                continue
            v, i = m[b, r, r + d], o[b] + r
            s[i, d] += v.astype(np.float64)
            c[i, d] += 1
            bad = np.isnan(v)
            with np.errstate(invalid="ignore"):
                lo[i, d] = np.where(bad, v, np.where(v < lo[i, d], v, lo[i, d]))         # a NaN already there fails the comparison and stays
                hi[i, d] = np.where(bad, v, np.where(v > hi[i, d], v, hi[i, d]))
    have = c > 0
    band, rng = np.full((N, D), np.nan, dtype=np.float32), np.full((N, D), np.nan, dtype=np.float32)
    with np.errstate(invalid="ignore"):
        band[have] = (s[have] / c[have].astype(np.float64)).astype(np.float32)
        rng[have] = hi[have] - lo[have]
    return band, c, rng


def band_insulation_host(band, widths):
    """Host restatement of orca_scan_band_insulation: insulation tracks [W, N] (fp64) of a band [N, D] at ``widths`` (1 <= w, 2 w + 1 <= D).
    track[k, i] = the mean of the w^2 pixels rows r in [i - w, i) x columns c in (i, i + w], read as band[r, c - r] and added in fp64; NaN where
    the diamond does not fit (i < w or i >= N - w) or holds a NaN - `screen.insulation_host` on the dense map the band stands for.  The terms are
    the kernel's, added here row by row and there 64 lanes at a time: equal within 2 w^2 2^-53 max|pixel|, not bit for bit."""
    b = np.asarray(band, dtype=np.float64)
    if b.ndim != 2:
        raise ValueError("band: [N, D]")
    N, D = b.shape
    ws = _widths(widths)
    out = np.full((len(ws), N), np.nan)
    for k, w in enumerate(ws):
        if w < 1 or 2 * w + 1 > D:
            raise ValueError(f"insulation width {w}: 1 <= w and 2 w + 1 <= D = {D}")
        i = np.arange(w, N - w)
        if i.size == 0:
            continue
        acc = np.zeros(i.size)
        for r in range(w):
            for c in range(w):
                acc += b[i - w + r, w - r + 1 + c]
        out[k, i] = acc / float(w * w)
    return out


def band_dot_enrichment_host(band, params):
    """Host restatement of orca_scan_band_dot_enrichment: the enrichment band [N, D] float32 of a band [N, D] under ``params`` (a
    `screen.LoopParams`), NaN at the ineligible pixels.  Pixel (i, d) is eligible when w <= i, i + d <= N - 1 - w and d_min <= d <= D - 1 - 2 w; its
    window pixel (a, b) - dense pixel (i + a, i + d + b) - is band[i + a, d + b - a], the flattened band at (i D + d) + a (D - 1) + b.  So the block of
    pixels shifted by (a, b) is a slice of the band itself: no dense map is made, and a 10 000 x 131 band is a few hundred slices of it.  The sets, the
    order of the fp64 sums (a ascending, then b ascending), the one division per set and the one rounding are `screen.dot_enrichment_host`'s - one
    function computes both - so e is, bit for bit, its e of the dense map the band stands for."""
    q = _loop_params(params)
    f = np.asarray(band, dtype=np.float32)
    if f.ndim != 2:
        raise ValueError("band: [N, D]")
    N, D = f.shape
    p, w, d_min = q.p, q.w, q.d_min
    out = np.full((N, D), np.nan, dtype=np.float32)
    rows, cols = N - 2 * w, D - 2 * w - d_min              # the block: rows w .. N - 1 - w, distances d_min .. D - 1 - 2 w
    if cols <= 0 or N < d_min + 2 * w + 1:
        return out
    f64 = f.astype(np.float64)
    e = _dot_enrichment_of(lambda a, b: f64[w + a: w + a + rows, d_min + b - a: d_min + b - a + cols], p, w)
    i, d = np.arange(w, N - w)[:, None], np.arange(d_min, D - 2 * w)[None, :]
    e[i + d > N - 1 - w] = np.nan                          # the column i + d needs w bins behind it too (those windows met the band's NaN end anyway)
    out[w: N - w, d_min: D - 2 * w] = e
    return out


def band_dot_calls_host(e_band, params):
    """Host restatement of orca_scan_band_dot_offsets + orca_scan_band_dot_list: ALL dots of an enrichment band [N, D] (float32) in ascending (i, d)
    order, as (ij int64 [L, 2] = (i, i + d), enrich float32 [L]).  (i, d) is a dot when e is not NaN, e >= threshold and, for every (di, dj) with
    |di|, |dj| <= r, not both 0, whose neighbour e' = e_band[i + di, d + dj - di] exists and is not NaN: e > e' where di < 0 or (di = 0 and dj < 0),
    e >= e' otherwise; all in fp32.  Only ``r`` and ``threshold`` of ``params`` are used: ``max_calls`` caps nothing here."""
    q = _loop_params(params)
    e = np.asarray(e_band, dtype=np.float32)
    if e.ndim != 2:
        raise ValueError("e_band: [N, D]")
    N, D = e.shape
    r, T = q.r, np.float32(q.threshold)
    pad = np.full((N + 2 * r, D + 4 * r), np.nan, dtype=np.float32)
    pad[r: r + N, 2 * r: 2 * r + D] = e
    with np.errstate(invalid="ignore"):
        dot = ~np.isnan(e) & (e >= T)
        for di in range(-r, r + 1):
            for dj in range(-r, r + 1):
                if di == 0 and dj == 0:
                    continue
                f = pad[r + di: r + di + N, 2 * r + dj - di: 2 * r + dj - di + D]
                wins = (e > f) if (di < 0 or (di == 0 and dj < 0)) else (e >= f)
                dot &= np.isnan(f) | wins
    at = np.argwhere(dot).astype(np.int64)                 # row-major: ascending (i, d)
    return np.stack([at[:, 0], at[:, 0] + at[:, 1]], axis=1), e[at[:, 0], at[:, 1]].copy()


# ---- the result -----------------------------------------------------------------------------------------------------------------------------------
@dataclass
class ScanResult:
    """What `scan_1m` returns.  The stretch is bases [start, start + n_bins * binsize) of the codes it was given; bin i is bases
    [start + i * binsize, start + (i + 1) * binsize).
      start, binsize     first base of bin 0; 4 000
      offsets            int64 numpy [windows]: the bin every window started at (`plan_windows`)
      n_bins, depth      N and D
      band               [N, D] float32 on the device: band[i, d] = the mean prediction of pixel (i, i + d); NaN where no window covers it (the
                         ``trim`` bins at either end) and where i + d >= N
      coverage           [N, D] int32 on the device: the number of windows that cover the pixel
      band_range         with ``spread=True``: [N, D] float32, largest minus smallest of the covering windows' values; 0 under one window
      insulation_widths  the widths, int32 numpy [W]
      insulation         [W, N] float32 on the device; NaN where the diamond does not fit or reaches an uncovered pixel
      boundary_strength  [W, N] float32 on the device: the strength at every minimum with strength > 0, NaN elsewhere
      boundaries         per width a pair (bins int64 numpy, strength float32 numpy), ascending in the bin: the minima whose strength is >=
                         ``min_strength`` - ALL of them
      boundary_params    the validated `screen.BoundaryParams` (``min_strength`` as the fp32 it was compared in)
      loop_params        with ``loops=``: the validated `screen.LoopParams` (``d_min`` resolved, ``threshold`` as the fp32 it was compared in)
      loop_enrichment    [N, D] float32 on the device: the enrichment e of band pixel (i, d), NaN where the pixel is ineligible or its window
                         holds a NaN
      loops              a pair (ij int64 numpy [L, 2], enrichment float32 numpy [L]): ALL dots (i, j = i + d) in ascending (i, d) order and
                         their e; `loop_positions` gives the anchors in bases"""
    start: int
    binsize: int
    offsets: np.ndarray
    n_bins: int
    depth: int
    band: torch.Tensor
    coverage: torch.Tensor
    band_range: Optional[torch.Tensor] = None
    insulation_widths: Optional[np.ndarray] = None
    insulation: Optional[torch.Tensor] = None
    boundary_strength: Optional[torch.Tensor] = None
    boundaries: Optional[list] = None
    boundary_params: Optional[BoundaryParams] = None
    loop_params: Optional[LoopParams] = None
    loop_enrichment: Optional[torch.Tensor] = None
    loops: Optional[tuple] = None

    def bin_of(self, pos):
        """The bin that holds base ``pos`` (in the coordinates of ``start``)."""
        i = (int(pos) - self.start) // self.binsize
        if not 0 <= i < self.n_bins:
            raise ValueError(f"base {pos} is outside the scanned stretch [{self.start}, {self.start + self.n_bins * self.binsize})")
        return i

    def pos_of(self, bin):
        """The first base of bin ``bin``."""
        if not 0 <= int(bin) <= self.n_bins:
            raise ValueError(f"bin {bin} is outside 0 .. {self.n_bins}")
        return self.start + int(bin) * self.binsize

    def loop_positions(self):
        """int64 numpy [L, 2]: the first base of the two anchor bins of every dot of ``loops`` (`pos_of`)."""
        if self.loops is None:
            raise ValueError("the scan called no loops (loops=)")
        return self.start + self.loops[0].astype(np.int64) * self.binsize

    def dense(self, i0, i1):
        """The stretch of bins [i0, i1) as a symmetric [m, m] float32 numpy map, m = i1 - i0: pixel (a, b) = band[i0 + min(a, b), |a - b|], NaN
        beyond the band (|a - b| >= depth) and wherever the band is NaN."""
        i0, i1 = int(i0), int(i1)
        if not 0 <= i0 < i1 <= self.n_bins:
            raise ValueError(f"bins [{i0}, {i1}) outside 0 .. {self.n_bins}")
        return dense_host(self.band[i0:i1].cpu().numpy(), i1 - i0)


def dense_host(band_rows, m):
    """Rows [i0, i0 + m) of a band as the symmetric [m, m] float32 map of those bins (`ScanResult.dense`)."""
    b = np.asarray(band_rows, dtype=np.float32)
    out = np.full((m, m), np.nan, dtype=np.float32)
    for d in range(min(b.shape[1], m)):
        k = np.arange(m - d)
        out[k, k + d] = out[k + d, k] = b[k, d]
    return out


# ---- the scan ----------------------------------------------------------------------------------------------------------------------------------
def _check_band_widths(insulation, D):
    try:
        w = _widths(insulation)
    except (TypeError, ValueError):
        raise ValueError("insulation: a width in bins or a sequence of widths") from None
    if not 1 <= len(w) <= 8 or len(set(w)) != len(w):
        raise ValueError("insulation: 1 to 8 distinct widths")
    for v in w:
        if v < 1 or 2 * v + 1 > D:
            raise ValueError(f"insulation width {v}: 1 .. {(D - 1) // 2} bins on a band of {D} distances (the diamond reaches distance 2 w)")
    return np.array(w, dtype=np.int32)


def _check_min_strength(boundaries):
    q = BoundaryParams() if boundaries is True else boundaries
    if not isinstance(q, BoundaryParams):
        raise ValueError("boundaries: True (the defaults) or a screen.BoundaryParams")
    try:
        s = float(np.float32(q.min_strength))
    except (TypeError, ValueError):
        raise ValueError("boundaries: min_strength must be a number") from None
    if isinstance(q.min_strength, (bool, np.bool_)) or not s >= 0.0:
        raise ValueError(f"boundaries: min_strength = {q.min_strength!r} must be a number >= 0, not NaN")
    return BoundaryParams(s, q.max_calls, q.tol)


def _stretch_codes(codes, start, end, window_bp):
    """(resident codes [>= stretch] uint8 on the device, first base of the stretch inside them, start in the caller's coordinates, N bins)."""
    start = int(start)
    if isinstance(codes, tuple):
        if len(codes) != 2:
            raise ValueError("codes: a [chrlen] uint8 codes tensor or (genome, chrom)")
        genome, chrom = codes
        length = dict(genome.get_chr_lens())[chrom]
    elif isinstance(codes, torch.Tensor):
        if not codes.is_cuda:
            raise OrcaHipError(f"scan_1m: the codes are on '{codes.device}': orca_amd runs on MI355X only, there is no CPU path")
        if codes.dtype != torch.uint8 or codes.dim() != 1:
            raise ValueError("codes: a [chrlen] uint8 codes tensor")
        length = codes.numel()
    else:
        raise TypeError("codes: a [chrlen] uint8 codes tensor or (genome, chrom)")
    end = length if end is None else int(end)
    if not 0 <= start <= end <= length:
        raise ValueError(f"bases [{start}, {end}) outside the chromosome's {length}")
    if end - start < window_bp:
        raise ValueError(f"a stretch of {end - start} bases holds no window of {window_bp}")
    N = (end - start) // BIN_BP                               # a tail shorter than a bin is dropped
    if isinstance(codes, tuple):
        got = genome.get_codes_from_coords(chrom, start, start + N * BIN_BP)
        if not isinstance(got, torch.Tensor):
            raise OrcaHipError("scan_1m: the genome is not resident on the MI355X (genome.to('cuda') first); there is no CPU path")
        return got.contiguous(), 0, start, N
    return codes.contiguous(), start, start, N


def scan_1m(model, codes, start=0, end=None, window_bp=1_000_000, step_bp=400_000, trim_bins=10, depth=None, batch=32, strands="+", insulation=None,
            boundaries=None, spread=False, stats=None, loops=None):
    """Predict bases [start, end) of a chromosome with the 1 Mb model, window by window, and stitch the maps into one band on the device: a
    `ScanResult`.

    ``model``: an ``H1esc_1M`` / ``Hff_1M`` container or a bare ``orca_modules.Net``.  ``codes``: the chromosome's base codes, a [chrlen] uint8 tensor
    on the MI355X, or ``(genome, chrom)`` for a `genome.PackedGenome` / `TwoBitGenome` resident there (read through ``get_codes_from_coords``).  A CPU
    tensor is an `OrcaHipError`: there is no CPU path.  ``end=None``: the chromosome's end.  end - start >= window_bp; a tail shorter than 4 kb is
    dropped, so the stretch has N = (end - start) // 4000 bins.

    ``window_bp`` and ``step_bp`` are multiples of 4 000, window_bp // 4000 = n <= 256 bins (1 000 000 and n = 250 in the reference); the windows
    start every ``step_bp`` and a last one ends with the stretch (`plan_windows`).  ``trim_bins``: a window is trusted on its bins [trim, n - trim) -
    the outer bins see less context; the default, 10, is NOT calibrated on the published checkpoints (nobody on this project has them).  ``depth``:
    D, the distances the band keeps; None means `full_depth` = n - 2 trim - step + 1, and a larger value is a ValueError - so the band has no holes
    except the ``trim`` bins at either end of the stretch.

    Per batch of ``batch`` windows the code windows are taken from the resident codes, the maps come from ``net._enc.forward_codes`` and ``net._dec``
    (the modules' fp16-range guards apply as in ``Net.forward``), and orca_scan_stitch_band adds them to the band; window maps never go to the host.
    ``strands="both"``: every window is also predicted on its reverse complement and the two maps are merged as ``genomepredict`` merges them
    (orca_screen_merge_strands) before they are stitched.  The band's bits do not depend on ``batch``.

    ``insulation``: a diamond width in bins or 1 to 8 distinct widths, 1 <= w and 2 w + 1 <= D, for `ScanResult.insulation`
    (orca_scan_band_insulation).  ``boundaries`` (with ``insulation``; without it a ValueError): True or a `screen.BoundaryParams`, for
    ``boundary_strength`` (orca_scan_boundary_strength) and the lists ``boundaries``.  Only ``min_strength`` is used - its default is NOT calibrated
    either; choose it from ``boundary_strength`` - and ``max_calls`` does NOT cap the lists: a chromosome has as many boundaries as it has.
    ``spread=True`` adds ``band_range``.  ``stats``: a dict that receives ``windows``, ``decoded_windows`` (twice the windows on both strands),
    ``batches``, ``bins``, ``depth`` and ``strands``, and with ``loops=`` ``loops``, the number of dots.

    ``loops``: True or a `screen.LoopParams` (`screen.check_band_loops`: a ValueError, before any device work, for a value outside its range and when
    the band has no eligible pixel, D < d_min + 2 w + 1), for ``loop_enrichment`` (orca_scan_band_dot_enrichment) and the list ``loops``
    (orca_scan_band_dot_offsets, orca_scan_band_dot_list): the screens' dot calls on the band, without their limit of 256 bins - a pixel at distance
    d_min <= d <= D - 1 - 2 w is called with its whole window, wherever the windows' seams lie.  ``max_calls`` and ``tol`` are accepted and unused:
    ``max_calls`` caps nothing here, a chromosome has as many loops as it has.  The default ``threshold`` is NOT calibrated on the published
    checkpoints; choose it from ``loop_enrichment``.  The calls run on the stitched MEAN, so ``band_range`` (``spread=True``) at a dot says how far the
    overlapping windows disagree there.  ``strands="both"`` needs nothing more: the band is already the merged one."""
    window_bp, step_bp, trim, batch = int(window_bp), int(step_bp), int(trim_bins), int(batch)
    if window_bp % BIN_BP or not 1 <= window_bp // BIN_BP <= MAX_BINS:
        raise ValueError(f"window_bp = {window_bp}: a multiple of {BIN_BP} with at most {MAX_BINS} bins (Net.forward's limit)")
    if step_bp % BIN_BP or step_bp < BIN_BP:
        raise ValueError(f"step_bp = {step_bp}: a positive multiple of {BIN_BP}")
    n, step = window_bp // BIN_BP, step_bp // BIN_BP
    if trim < 0 or n - 2 * trim < 1:
        raise ValueError(f"trim_bins = {trim} on windows of {n} bins: trim >= 0 and n - 2 trim >= 1")
    deepest = full_depth(n, step, trim)
    if deepest < 1:
        raise ValueError(f"step_bp = {step_bp} leaves holes at every distance: at most {(n - 2 * trim) * BIN_BP} with trim_bins = {trim}")
    D = deepest if depth is None else int(depth)
    if not 1 <= D <= deepest:
        raise ValueError(f"depth = {D}: 1 .. full_depth = {deepest} (a deeper band has holes between the windows)")
    if strands not in ("+", "both"):
        raise ValueError(f"strands must be '+' or 'both', got {strands!r}")
    if batch < 1:
        raise ValueError("batch must be positive")
    want_b = boundaries is not None and boundaries is not False
    if want_b and insulation is None:
        raise ValueError("boundaries: called on the insulation tracks (insulation=widths)")
    widths = None if insulation is None else _check_band_widths(insulation, D)
    bp = _check_min_strength(boundaries) if want_b else None
    lp = None if loops is None or loops is False else check_band_loops(loops, n, D)      # the stretch has N >= n >= D bins: D decides
    codes, base, start, N = _stretch_codes(codes, start, end, window_bp)
    net = _net_of(model)
    both = strands == "both"
    dev = codes.device
    ctx = engine.get_context(dev)
    off = plan_windows(N, n, step, trim)
    off_dev = torch.from_numpy(off).to(dev)
    st = {"windows": int(off.size), "decoded_windows": 0, "batches": 0, "bins": N, "depth": D, "strands": strands}
    with torch.no_grad():
        acc = engine.scan_accumulators(dev, N, D)
        for k0 in range(0, off.size, batch):
            o = off[k0: k0 + batch]
            win = torch.stack([codes[base + int(a) * BIN_BP: base + int(a) * BIN_BP + window_bp] for a in o])
            maps = net._dec(net._enc.forward_codes(win))[:, 0]
            st["decoded_windows"] += len(o)
            if both:
                minus = net._dec(net._enc.forward_codes(win, reverse=True))[:, 0]
                st["decoded_windows"] += len(o)
                maps, _ = engine.screen_merge_strands(ctx, maps, minus, out=maps)
            engine.scan_stitch_band(ctx, maps, o, trim, acc, off_dev[k0: k0 + batch])
            st["batches"] += 1
        band, rng = engine.scan_band_finish(ctx, acc, spread=bool(spread))
        res = ScanResult(start, BIN_BP, off, N, D, band, acc["count"], rng)
        if widths is not None:
            res.insulation_widths = widths
            res.insulation = engine.scan_band_insulation(ctx, band, widths)
            if bp is not None:
                res.boundary_params = bp
                res.boundary_strength = engine.scan_boundary_strength(ctx, res.insulation)
                res.boundaries = boundary_lists_host(res.boundary_strength.cpu().numpy(), bp.min_strength)
        if lp is not None:
            res.loop_params = lp
            res.loop_enrichment = engine.scan_band_dot_enrichment(ctx, band, lp.p, lp.w, lp.d_min)
            ij, enrich = engine.scan_band_dot_calls(ctx, res.loop_enrichment, lp.r, lp.threshold)
            res.loops = (ij.cpu().numpy(), enrich.cpu().numpy())
            st["loops"] = int(ij.shape[0])
    if stats is not None:
        stats.update(st)
    return res


def boundary_lists_host(strength, min_strength):
    """Per track of ``strength`` [W, N] (float32: the strength at every minimum with strength > 0, NaN elsewhere) the pair (bins int64, strength
    float32) of the minima with strength >= ``min_strength`` (compared in fp32), ascending in the bin."""
    s = np.asarray(strength, dtype=np.float32)
    out = []
    for t in s.reshape(-1, s.shape[-1]):
        with np.errstate(invalid="ignore"):
            at = np.flatnonzero(t >= np.float32(min_strength))           # NaN compares False
        out.append((at.astype(np.int64), t[at].copy()))
    return out
