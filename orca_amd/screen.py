"""In-silico mutagenesis screens on the 1 Mb model (``H1esc_1M`` / ``Hff_1M``, ``Net``): the "virtual genetic screens" use case of the
reference's README, for structure below 1 Mb.

An `Edit` is a LENGTH-PRESERVING change of one window - a substitution, an N-mask or an in-place reverse complement.  Such an edit keeps the
4 kb grid, and the Encoder is translation-covariant on it: only the stage-5 input rows (400 bases each, after stage 4 and its MaxPool1d(5))
whose dependency cone meets the edit change - stages 1-4 reach 1 631 bases past a row's 400 (``sv.S4_MARGIN_BP``).  `screen_1m` therefore
encodes the window ONCE (front + stage 4 over the whole window, stages 5-7, Decoder_1m), and per edit only

  * the front + stage 4 on a snippet of a few kb around the edit (many snippets concatenated into one run),
  * stages 5-7 on a copy of the reference rows with the snippet's rows spliced in (a batch of edits in one launch chain),
  * Decoder_1m on the batch, and the scores against the reference map.

The edited snippets, the row images, the batched stages 5-7 and the scores are HIP kernels (include/orca_hip.h: orca_screen_*,
orca_encoder_back5_batch).  The route needs the Encoder's two-part form (default f16x2 arithmetic, `Encoder.two_part_ok`); otherwise - another
precision or Encoder form, `engine.force_safe_precision()` - every batch goes through the whole-window route (the edited windows through
`Net`'s own Encoder and Decoder_1m), with the same API and results.  The fp16-range check is deferred to the end of the reference and of each
batch; when it fires, that batch (or, for the reference, the whole screen) is redone on the whole-window route in the range-safe arithmetic.

An `EditSet` is a compound edit: several pairwise disjoint `Edit`s of the same window applied together (a haplotype's SNVs, two sites knocked
out at once, `pair_edits` for epistasis).  It is still length-preserving, so the same argument holds: the rows inside some member's cone
change, and no others.  The rows of the members are merged into clusters, each cluster is one snippet, and the item's row image takes one
row range per cluster (orca_screen_edit_codes_multi, orca_screen_splice_rows_multi).  ``regions`` adds the signed and the absolute mean of
alt - ref over chosen bin rectangles (orca_screen_region_scores).

``Edit("del", ...)`` and ``Edit("ins", ...)`` change the length.  The alt window is still L bases and starts where the window starts: it is the
first L bases of (edited window ++ right flank ++ N ...), so a net deletion is refilled from the flank and a net insertion pushes the tail
out.  Behind a length change the same bases sit at another offset s (context position - alt position).  Stage 4 is translation-covariant on
the 80-base grid, so their rows are the MaxPool1d(5) of stage 4's output on the CONTEXT (window ++ flank) at phase s mod 80
(`sv.Stage4Cache`), or plainly the reference's rows s / 400 further on when 400 divides s; only the junctions and the alt window's right
end go through the front again.  A batch that holds such an item takes its bases from piece lists (orca_screen_assemble_codes) and its rows
from a table of sources (orca_screen_gather_rows); `plan_batch` states the rule.

Behind an unbalanced indel the alt map is displaced against the reference map, and the bin-with-bin scores hold that displacement.
``screen_1m(..., aligned=True)`` adds scores on ALIGNED bins: `bin_map` says which reference bin an alt bin stands for, and alt pair (i, j) is
compared with reference pair (map i, map j) (orca_screen_aligned_scores, orca_screen_aligned_region_scores).  `deletion_scan` and `tandem_dup`
generate the large edits this is for, and ``flank_bp`` reads enough genome behind the window to refill them.

``screen_1m(..., strands="both")`` scores every item on both strands, merged as ``genomepredict`` merges them: every map returned or scored is
0.5 plus + 0.5 flip(minus), minus being the model's map of the reverse complement of the item's alt window.  The snippets are generated once, in
forward coordinates; the front reads the same buffer reverse-complemented, and the '-' strand's plan is the mirror of the '+' strand's
(`mirror_plan`: '+' row r is '-' row n5 - 1 - r).  One kernel merges a batch's two strands and measures how far they disagree
(orca_screen_merge_strands, `ScreenResult.strand_gap`); the scores then run unchanged on the merged maps.

The scores above are means and maxima of |alt - ref|: they say that something changed, not what.  ``screen_1m(..., insulation=widths)`` adds
the insulation track of every alt map - the mean contact across each bin, over a diamond of the given width - and its signed difference to
the reference's, and ``viewpoints=bins`` the signed row alt - ref of chosen bins (a virtual 4C); with ``aligned=True`` both also come on aligned
bins, through the same `bin_map` (orca_screen_insulation, orca_screen_viewpoints; `insulation_scores_host`, `viewpoint_scores_host`).  Both are
1-D tracks per item, so a deletion scan can ask "which deletion fuses the two domains" without ``keep_maps``.

``screen_1m(..., strata=True)`` adds how similar every alt map is to the reference map, by genomic distance: per stratum d - the pairs
(i, i + d) - the mean, mean absolute and root-mean-square difference and the fp64 correlation, and per map the mean squared difference, the
Pearson correlation and HiCRep's stratum-adjusted correlation, bin with bin and, with ``aligned=True``, through `bin_map`
(orca_screen_strata_scores; `strata_scores_host`).  A uniform shift of a distance band and a re-patterning inside it, which a mean of
|alt - ref| cannot tell apart, separate there.

``screen_1m(..., loops=True)`` (or a `LoopParams`) calls loops - the focal peaks between two anchors - on every alt map and on the reference
map: the enrichment of a pixel's peak over HiCCUPS' donut, lower-left, horizontal and vertical backgrounds as a difference of fp64 means of
log observed / expected, thresholded and reduced to local maxima on the device (orca_screen_dot_calls, orca_screen_dot_enrichment), then the
change of the enrichment at every reference dot and which dots were gained or lost, bin with bin and, with ``aligned=True``, through `bin_map`
(`loop_scores_host` restates it all).  "Which CTCF-site knock-out removes this loop" needs no ``keep_maps``.

``screen_1m(..., insulation=widths, boundaries=True)`` (or a `BoundaryParams`) calls domain boundaries on the insulation tracks: the minima of a
track whose strength - the prominence of the dip, in mean log observed / expected - reaches ``min_strength``, listed on the device
(orca_screen_boundary_calls), then which reference boundaries an item keeps, weakens or loses and which it creates, bin with bin and, with
``aligned=True``, through `bin_map` (`boundary_scores_host` restates it all).  "Which deletion fuses the two domains" is ``boundaries_lost``.

Every score above compares an item with the unedited window.  `epistasis_1m` asks whether the effect of an `EditSet` is the sum of its members'
effects: it screens the distinct members and the sets in one pass, keeps the members' maps in a device bank, and scores per set the residual
r = (alt_set - ref) - sum_m (alt_m - ref), every pixel in fp64 (orca_screen_epistasis_scores, orca_screen_epistasis_region_scores;
`epistasis_items`, `epistasis_scores_host`) - the readout of a `pair_edits` screen, and of "is this haplotype more than its SNVs".
"""
from contextlib import nullcontext

import numpy as np
import torch

from . import engine, sv
from ._lib import OrcaHipError
# the screen is four modules; every name that lives in one of the other three stays reachable as screen.NAME
from .map_readouts import (  # noqa: F401
    BIN_BP, _bin_maps, scores_host, check_regions, region_scores_host, aligned_scores_host, aligned_region_scores_host, check_insulation,
    check_viewpoints, _widths, insulation_host, insulation_scores_host, viewpoint_scores_host, STRATA_FIELDS, check_strata, strata_scores_host,
    LOOP_MAX_W, LOOP_MAX_R, LOOP_MAX_CALLS, LOOP_FIELDS, LoopParams, _loop_params, check_loops, check_band_loops, check_loops_arg, dot_enrichment_host, dot_calls_host,
    follow_loop, _follow_loops, match_loops_host, _match_loops, loop_scores_host, BOUNDARY_MIN_BINS, BOUNDARY_MAX_BINS, BOUNDARY_MATCH_FIELDS,
    BoundaryParams, check_boundaries, check_boundaries_arg, boundary_strength_host, boundary_calls_host, match_boundaries_host, _match_boundaries,
    _boundary_fields, boundary_scores_host, merge_strands_host, _member_table, epistasis_scores_host)
from .screen_plan import (  # noqa: F401
    ROW_BP, MARGIN_BP, PAD_BP, MIN_SNIPPET_BP, RUN_MAX_BP, N_CODE, KINDS, LEN_KINDS, FLANK_BP, _ACGTN, _codes_of, Edit, EditSet, members_of,
    changes_length, shift_of, _flank_host, apply_edit, saturation_edits, tile_edits, pair_edits, snv_set, indel, deletion_scan, tandem_dup, bin_map,
    BatchPlan, edit_rows, edit_snippet, _runs, set_clusters, _item_table, _item_spans, _span_table, _spans_meeting, entry_rows, item_pieces,
    item_sources, needed_phases, mirror_phases, _pieces_meeting, _piece_table, _pack, _layout, _plan_indels, plan_batch, mirror_plan, _whole_window,
    whole_window_table, whole_window_piece_tables, whole_window_set_tables, epistasis_items)
from .screen_readouts import (  # noqa: F401
    EpistasisResult, ScreenResult, UNSET_STATS, ReadoutArgs, Run, Readout, MapScores, Insulation, Viewpoints, Strata, Loops, EpistasisBank,
    readout_units)


# ---- the screen -----------------------------------------------------------------------------------------------------------------------------
def _window_codes(window):
    if isinstance(window, tuple):
        if len(window) not in (3, 4):
            raise ValueError("window: a [L] uint8 codes tensor or (genome, chrom, start[, L])")
        genome, chrom, start = window[:3]
        L = int(window[3]) if len(window) == 4 else 1_000_000
        codes = genome.get_codes_from_coords(chrom, int(start), int(start) + L)
        if not isinstance(codes, torch.Tensor):
            raise OrcaHipError("screen_1m: the genome is not resident on the MI355X (genome.to('cuda') first); there is no CPU path")
        window = codes
    if not isinstance(window, torch.Tensor):
        raise TypeError("window: a [L] uint8 codes tensor or (genome, chrom, start[, L])")
    if not window.is_cuda:
        raise OrcaHipError(f"screen_1m: the window is on '{window.device}': orca_amd runs on MI355X only, there is no CPU path")
    if window.dtype != torch.uint8 or window.dim() != 1:
        raise ValueError("window: a [L] uint8 codes tensor")
    L = window.numel()
    if L % 4000 or not 0 < L // 4000 <= 256:
        raise ValueError(f"window of {L} bases: a multiple of 4 000 with at most 256 bins (Net.forward's limit)")
    return window.contiguous()


def _net_of(model):
    net = getattr(model, "net", model)
    if not (hasattr(net, "_enc") and hasattr(net, "_dec")):
        raise TypeError("screen_1m: an H1esc_1M / Hff_1M container or an orca_modules.Net")
    return net


def _flank_codes(window, flank, win, flank_bp=None):
    """The right flank of the window as a [F] uint8 tensor on the window's device (0 <= F <= L): ``flank`` as given, else read from the genome
    of a ``(genome, chrom, start[, L])`` window (``flank_bp`` bases, `FLANK_BP` by default, fewer at the chromosome's end), else empty."""
    L = win.numel()
    if flank is None:
        if not isinstance(window, tuple) or flank_bp == 0:
            return win[:0]
        genome, chrom, start = window[:3]
        n = dict(genome.get_chr_lens())[chrom]
        flank = genome.get_codes_from_coords(chrom, int(start) + L, min(int(start) + L + (min(FLANK_BP, L) if flank_bp is None else flank_bp), n))
    if not isinstance(flank, torch.Tensor):
        raise TypeError("flank: a [F] uint8 codes tensor on the MI355X")
    if not flank.is_cuda:
        raise OrcaHipError(f"screen_1m: the flank is on '{flank.device}': orca_amd runs on MI355X only, there is no CPU path")
    if flank.dtype != torch.uint8 or flank.dim() != 1 or flank.numel() > L or flank.device != win.device:
        raise ValueError(f"flank: a [F] uint8 codes tensor beside the window, 0 <= F <= {L}")
    return flank.contiguous()


class _Screen:
    def __init__(self, net, window, stats, flank=None):
        self.net, self.window, self.stats = net, window, stats
        self.F = 0 if flank is None else flank.numel()
        self.context = window if not self.F else torch.cat([window, flank])       # what the pieces of an indel batch read
        self.cache = None
        self.dev = window.device
        self.L = window.numel()
        self.n5, self.n = self.L // ROW_BP, self.L // 4000
        self.ctx = engine.get_context(self.dev)
        self.num_1d = net.num_1d or 0

    # decode an encoding [B,128,n]: (maps [B,n,n], 1-D head [B,num_1d,n] or None)
    def _decode(self, enc):
        maps = self.net._dec(enc)[:, 0]
        h = None
        if self.num_1d:
            w1, b1, w2, b2 = self.net._head1d_weights(self.dev)
            h = engine.pointwise1d(engine.pointwise1d(enc, w1, b1, "relu"), w2, b2, "sigmoid")
        return maps, h

    def _upload(self, a, dtype):
        return torch.from_numpy(np.ascontiguousarray(a)).to(self.dev, dtype)

    def whole(self, edits, reverse=False):
        """Maps of the edited windows through Net's own Encoder and Decoder_1m (the module guards apply as in Net.forward); ``reverse``: of their
        reverse complements (the '-' strand's maps, in its own orientation)."""
        if not edits:
            return self._decode(self.net._enc.forward_codes(self.window[None], reverse=reverse))
        codes = torch.empty(len(edits) * self.L, dtype=torch.uint8, device=self.dev)
        if any(changes_length(e) for e in edits):
            table, pieces, payload = whole_window_piece_tables(edits, self.L, self.F)
            pay = self._upload(payload, torch.uint8) if payload.size else None
            engine.screen_assemble_codes(self.ctx, self.context, table, pieces, pay, codes)
        elif all(isinstance(e, Edit) for e in edits):
            table, payload = whole_window_table(edits, self.L)
            pay = self._upload(payload, torch.uint8) if payload.size else None
            engine.screen_edit_codes(self.ctx, self.window, table, self._upload(table, torch.int64), pay, codes)
        else:
            table, spans, payload = whole_window_set_tables(edits, self.L)
            pay = self._upload(payload, torch.uint8) if payload.size else None
            engine.screen_edit_codes_multi(self.ctx, self.window, table, spans, pay, codes)
        return self._decode(self.net._enc.forward_codes(codes.view(len(edits), self.L), reverse=reverse))

    def reference_rows(self, reverse=False):
        enc = self.net._enc
        s5 = torch.empty((self.n5, 128), dtype=torch.float32, device=self.dev)
        enc.front4_ranges(self.window, reverse, [(0, self.n5, 0)], s5)
        return s5

    def build_entries(self, phases, strand="+"):
        """The stage-4 cache entries of ``phases`` over the context on ``strand`` ('-': over its reverse complement; `sv.Stage4Cache` builds a
        phase's group of five)."""
        if self.cache is None:
            self.cache = sv.Stage4Cache(self.net._enc, self.context)
        out = []
        for ph in phases:
            e = self.cache.get(strand, ph)
            if e is None:
                raise OrcaHipError(f"screen_1m: stage-4 cache entry {ph} unavailable (fp16 range)")
            if e.shape[0] != entry_rows(self.L + self.F, ph):
                raise OrcaHipError(f"screen_1m: stage-4 cache entry {ph} holds {e.shape[0]} rows, the plan expects {entry_rows(self.L + self.F, ph)}")
            out.append(e)
        self.stats["cache_phases"] = self.cache.builds
        return out

    def _snippet_codes(self, p, edits):
        """The packed buffer of the plan's edited snippets, in forward coordinates (both strands read it)."""
        total = int(p.snippet[:, 1].sum())
        codes = torch.empty(total, dtype=torch.uint8, device=self.dev)
        pay = self._upload(p.payload, torch.uint8) if p.payload.size else None
        if p.indel:
            if total:                                    # no snippet at all: every row of every item is served (an ``ins`` behind the last base)
                engine.screen_assemble_codes(self.ctx, self.context, p.snippet_table, p.piece_table, pay, codes)
        elif p.edit_table is not None and all(isinstance(e, Edit) for e in edits):
            engine.screen_edit_codes(self.ctx, self.window, p.edit_table, self._upload(p.edit_table, torch.int64), pay, codes)
        else:
            engine.screen_edit_codes_multi(self.ctx, self.window, p.snippet_table, p.span_table, pay, codes)
        return codes

    def _strand_enc(self, p, edits, codes, s5_ref, reverse=False):
        """The encodings [B, 128, n] of one strand of a batch from the snippets' bases: the front on every run, the row images, stages 5-7.
        ``reverse``: ``p`` is the mirrored plan, ``s5_ref`` the '-' strand's reference rows, and the front reverse-complements every run."""
        enc = self.net._enc
        fresh = torch.empty((p.n_fresh, 128), dtype=torch.float32, device=self.dev)
        for o0, nb, ranges in p.runs:
            enc.front4_ranges(codes[o0: o0 + nb], reverse, ranges, fresh)
        rows = torch.empty((len(edits), self.n5, 128), dtype=torch.float32, device=self.dev)
        if p.indel:
            engine.screen_gather_rows(self.ctx, s5_ref, fresh, self.build_entries(p.phases, "-" if reverse else "+"), p.gather_segments, p.gather_off, rows)
        elif p.splice_table is not None and all(isinstance(e, Edit) for e in edits):
            engine.screen_splice_rows(self.ctx, s5_ref, fresh, self._upload(p.splice_table, torch.int64), rows)
        else:
            engine.screen_splice_rows_multi(self.ctx, s5_ref, fresh, p.segments, p.seg_off, rows)
        return enc.back5_batch(rows)

    def two_part(self, edits, s5_ref, plan=None, s5_ref_minus=None):
        """Maps of a batch on the two-part route.  ``plan``: the batch's plan if it holds a length-changing item (`screen_1m` made it with the
        reference, and for both strands if they are wanted) - then the bases of every snippet come from the items' pieces and the row images
        from the reference rows, the recomputed rows and the cache entries; a list of bare `Edit`s runs the single-span kernels, as ever.  With
        ``s5_ref_minus`` (the '-' strand's reference rows) the result is the pair ('+' strand, '-' strand) of (maps, 1-D head), the second in
        the '-' strand's own orientation: the front reads the same buffer reverse-complemented, run by run, and the mirrored plan
        (`mirror_plan`) says where its rows go."""
        p = plan_batch(edits, self.L) if plan is None else plan
        codes = self._snippet_codes(p, edits)
        out = self._strand_enc(p, edits, codes, s5_ref)
        self.stats["segments"] += len(p.segments)
        self.stats["front_runs"] += len(p.runs)
        self.stats["front_bases"] += int(codes.numel())
        self.stats["take_rows"] += p.take_rows
        if s5_ref_minus is None:
            return self._decode(out)
        return self._decode(out), self._decode(self._strand_enc(mirror_plan(p), edits, codes, s5_ref_minus, True))

    def reference(self, edits, batch, both):
        """The unedited window's (final map [n, n], 1-D head or None, strand gap or None), and what the batches need of it: whether they take the
        two-part route (``use_two_part``), the reference rows of the strands, the plans of the batches that hold a length-changing item with the
        stage-4 cache entries they pool from - all under ONE deferred range check; when it fires, the reference is redone on the whole-window
        route in the range-safe arithmetic and every batch goes that way.  With ``both`` the map is the merged one, as every batch's will be."""
        net, st, n, dev = self.net, self.stats, self.n, self.dev
        self.both, self.plans, self.use_two_part = both, {}, net._enc.two_part_ok()
        self.s5_ref = self.s5_ref_minus = self.ref_plus = self.ref_minus = ref_minus = None
        if self.use_two_part:
            with engine.defer_overflow_guard():
                self.s5_ref = self.reference_rows()
                enc_ref = torch.empty((1, 128, n), dtype=torch.float32, device=dev)
                net._enc.back5(self.s5_ref, enc_ref[0])
                ref_map, ref_1d = self._decode(enc_ref)
                if both:                                 # the '-' strand's reference, under the same range check
                    self.s5_ref_minus = self.reference_rows(True)
                    enc_minus = torch.empty((1, 128, n), dtype=torch.float32, device=dev)
                    net._enc.back5(self.s5_ref_minus, enc_minus[0])
                    ref_minus = self._decode(enc_minus)
                if st["indel_items"]:                    # the cache entries the batches will pool from, under the reference's range check
                    for i0 in range(0, len(edits), batch):       # every indel batch is planned once, here; the phases built are the phases used
                        if any(changes_length(e) for e in edits[i0: i0 + batch]):
                            self.plans[i0] = plan_batch(edits[i0: i0 + batch], self.L, flank=self.F, both_strands=both)
                    phases = sorted({ph for p in self.plans.values() for ph in p.phases})
                    self.build_entries(phases)
                    if both:
                        self.build_entries(mirror_phases(phases, self.L + self.F), "-")
            if self.ctx.take_overflow():
                self.use_two_part = False
                st["range_fallback_reference"] = True
        if not self.use_two_part:
            with engine.force_safe_precision() if st["range_fallback_reference"] else nullcontext():
                ref_map, ref_1d = self.whole([])
                ref_minus = self.whole([], reverse=True) if both else None
        st["route"] = "two_part" if self.use_two_part else "whole_window"
        ref_map = ref_map[0].contiguous()
        ref_1d = None if ref_1d is None else ref_1d[0].contiguous()
        if not both:
            return ref_map, ref_1d, None
        # the reference merged as every batch will be; zero "references" make the gap mean |ref+ - flip(ref-)|
        self.ref_plus, self.ref_minus, ref_1d_minus = ref_map, ref_minus[0][0].contiguous(), ref_minus[1]
        zero = torch.zeros_like(self.ref_plus)
        merged, ref_gap = engine.screen_merge_strands(self.ctx, self.ref_plus[None], self.ref_minus[None], zero, zero)
        if ref_1d is not None:
            ref_1d = 0.5 * ref_1d + 0.5 * ref_1d_minus[0].flip(-1)
        return merged[0], ref_1d, ref_gap[0]

    def _whole_strands(self, chunk):
        """A batch on the whole-window route: the '+' strand's (maps, 1-D head), or the pair of strands'."""
        if not self.both:
            return self.whole(chunk)
        self.stats["reverse_whole_items"] += len(chunk)
        return self.whole(chunk), self.whole(chunk, reverse=True)

    def final_maps(self, i0, chunk):
        """The FINAL (maps [B, n, n], 1-D head or None, strand gap [B] or None) of the batch ``chunk`` = items [i0, i0 + B), after `reference`: on
        the two-part route under one deferred range check for both strands - when it fires the batch is redone on the whole-window route in the
        range-safe arithmetic - or on the whole-window route; with both strands merged as the reference was."""
        st = self.stats
        if self.use_two_part:
            with engine.defer_overflow_guard():
                out = self.two_part(chunk, self.s5_ref, self.plans.get(i0), self.s5_ref_minus)
            if self.ctx.take_overflow():
                st["range_fallback_batches"] += 1
                with engine.force_safe_precision():
                    out = self._whole_strands(chunk)
            else:
                st["two_part_batches"] += 1
                if self.both:
                    st["reverse_two_part_items"] += len(chunk)
        elif st["range_fallback_reference"]:
            st["range_fallback_batches"] += 1
            with engine.force_safe_precision():
                out = self._whole_strands(chunk)
        else:
            st["whole_window_batches"] += 1
            out = self._whole_strands(chunk)
        if not self.both:
            return out + (None,)
        (maps, h), (maps_minus, h_minus) = out
        maps, gap = engine.screen_merge_strands(self.ctx, maps, maps_minus, self.ref_plus, self.ref_minus, out=maps)
        return maps, (None if h is None else 0.5 * h + 0.5 * h_minus.flip(-1)), gap


def screen_1m(model, window, edits, batch=64, keep_maps=False, stats=None, regions=None, flank=None, aligned=False, flank_bp=None, strands="+",
              insulation=None, viewpoints=None, strata=None, loops=None, boundaries=None):
    """Score ``edits`` (a list of `Edit` and `EditSet`, one row of every result tensor each) of one window with the 1 Mb model: a `ScreenResult`.

    ``model``: an ``H1esc_1M`` / ``Hff_1M`` container or a bare ``orca_modules.Net``.  ``window``: the window's base codes, a [L] uint8 tensor on
    the MI355X, or ``(genome, chrom, start)`` / ``(genome, chrom, start, L)`` for a `genome.PackedGenome` / `TwoBitGenome` resident there
    (L = 1 000 000 by default, as the reference's 1 Mb model).  L: a multiple of 4 000 with at most 256 bins.  Forward strand only (as the
    reference's ``pred_1m``) by default; ``strands`` below.  ``batch``: edits per batch.  ``keep_maps``: also return every alt map.  ``stats``: a dict that receives
    counters - ``route`` ("two_part" / "whole_window"), ``two_part_batches``, ``whole_window_batches``, ``range_fallback_batches`` (batches
    redone on the whole-window route in the range-safe arithmetic after the fp16-range check fired), ``range_fallback_reference`` (the
    reference itself tripped: every batch went that way), ``front_runs``, ``front_bases``, ``edits``, ``set_items`` (items that are an
    `EditSet`), ``segments`` ((snippet, row range) segments planned on the two-part route: one per bare edit, one per cluster of a set).
    ``regions``: up to 64 half-open bin rectangles (i0, i1, j0, j1) for `ScreenResult.delta_region` / ``delta_region_abs``.

    ``del`` / ``ins`` members: the alt window is the first L bases of (edited window ++ flank ++ N ...).  ``flank``: a [F] uint8 tensor on the
    MI355X with the bases that follow the window, 0 <= F <= L; for a ``(genome, chrom, start[, L])`` window it is read from the genome
    (`FLANK_BP` bases, fewer at the chromosome's end); bases beyond it are N.  It is validated and otherwise ignored when no item changes
    length.  `ScreenResult.shift` says how far each item displaces what follows it.  More ``stats``: ``indel_items`` (items with a ``del`` /
    ``ins`` member), ``take_rows`` (stage-5 rows pooled from stage-4 cache entries on the two-part route), ``cache_phases`` (entries built: 512
    bytes per context base for all 80; they are built with the reference, inside its deferred range check).

    ``flank_bp``: for a ``(genome, chrom, start[, L])`` window without ``flank``, the number of bases to read behind the window, 0 <= flank_bp <= L
    (`FLANK_BP` by default; fewer at the chromosome's end).  Without it a 100 kb deletion is refilled with 8 kb of genome and 92 kb of N.  Given
    together with ``flank`` or with a tensor window it is a ValueError.

    ``aligned=True`` adds the scores on aligned bins (`ScreenResult.bin_map`, ``aligned_bins``, ``aligned_profile``, ``aligned_abs_mean``,
    ``aligned_abs_max`` and, with ``regions``, ``aligned_region`` / ``aligned_region_abs``): alt pair (i, j) against reference pair (map i, map j)
    with map = `bin_map` of the item, taken from the batch's maps whichever route produced them.  The rectangles of ``regions`` keep their
    meaning for ``delta_region`` and are read as REFERENCE bins for the aligned pair.  With ``aligned=False`` nothing more is launched and those
    fields are None.  ``stats`` gains ``aligned_items``: the items whose bin map is not the identity (0 without ``aligned``).

    ``strands``: "+" (the default: nothing below is launched, every field is what it ever was) or "both": every map returned or scored is the
    merged map 0.5 plus + 0.5 flip(minus), as ``genomepredict`` merges its two strands - minus is the model's map of the REVERSE COMPLEMENT of the
    item's alt window (for a ``del`` / ``ins`` item the L-base alt window with its refill and N fill applied), flip reverses both bin axes.  Merged
    maps are in forward orientation, so ``ref_map``, ``maps``, every ``delta_*`` and ``aligned_*`` field, ``regions``, `bin_map` and ``shift`` keep
    their meaning, now on merged maps against the merged reference (orca_screen_merge_strands, then the same score kernels); the 1-D heads are
    0.5 h_plus + 0.5 h_minus.flip(-1).  `ScreenResult.strand_gap` and ``ref_strand_gap`` say how far the strands disagree.  On the two-part route
    the snippets are generated once and the front reads them a second time reverse-complemented (`mirror_plan`); a ``del`` / ``ins`` item
    pools its '-' rows from the '-' strand's stage-4 cache entries (built with the reference too; ``cache_phases`` counts both strands').  One
    deferred range check covers both strands of a batch (and of the reference).  The screen is decode-bound, so expect about twice the time
    per item.  More ``stats``: ``strands``, ``reverse_two_part_items`` / ``reverse_whole_items`` (items whose '-' strand ran two-part /
    through the whole-window Encoder: the whole-window route and the range-safe redo).

    ``insulation``: a diamond width in bins or 1 to 8 distinct widths, each 1 <= w <= (n - 1) // 2, for the insulation tracks
    `ScreenResult.insulation`, ``ref_insulation``, ``delta_insulation`` and, with ``aligned=True``, ``aligned_insulation`` (orca_screen_insulation):
    the mean contact across every bin, the readout for "did a boundary weaken or appear".  ``viewpoints``: 1 to 64 bins for
    `ScreenResult.delta_viewpoint` and, with ``aligned=True``, ``aligned_viewpoint`` (orca_screen_viewpoints): the signed row alt - ref of a bin, a
    virtual 4C; in the aligned form the viewpoint is a REFERENCE bin, followed to wherever the item moved it.  Both are taken from the batch's
    maps whichever route made them, with ``strands="both"`` from the merged maps against the merged ``ref_map``.  With both None nothing more is
    launched and every other field is what it was.  ``stats`` gains ``insulation_widths`` and ``viewpoints``: their numbers (0 when absent).

    ``strata``: True, or a pair (d_lo, d_hi) with 0 <= d_lo < d_hi <= n (`check_strata`), for the similarity of every alt map to ``ref_map`` by
    genomic distance (orca_screen_strata_scores): per stratum d - the pairs (i, i + d) - `ScreenResult.dist_delta`, ``dist_abs``, ``dist_rms`` and the
    fp64 correlation ``dist_corr``; per map, over the strata d_lo <= d < d_hi (all of them with True), ``mse``, the Pearson ``corr`` and the
    stratum-adjusted correlation ``scc`` (HiCRep's), both fp64, so that 1 - scc of a small edit is not lost; with ``aligned=True`` also the
    ``aligned_dist_*`` fields, ``aligned_mse``, ``aligned_corr`` and ``aligned_scc`` through `bin_map` (a second call).  The means of |alt - ref| above
    cannot tell a uniform shift of a distance band (``dist_delta`` moves, ``dist_corr`` stays 1) from a re-patterning inside it (``dist_corr`` drops).
    Taken from the batch's final maps whichever route made them, with ``strands="both"`` from the merged maps against the merged ``ref_map``.  With
    None (or False) nothing more is launched and every other field is what it was.  ``stats`` gains ``strata``: the number of strata the per-map
    scores run over (0 when absent).

    ``loops``: True (the defaults) or a `LoopParams` (`check_loops`), for dot calls on every alt map and on ``ref_map`` (orca_screen_dot_calls):
    `ScreenResult.ref_loops`, ``ref_loop_enrichment``, ``ref_loop_count``, ``loops``, ``loop_enrichment``, ``loop_count``, the change of the enrichment
    at every reference dot ``loop_delta``, and ``loops_gained`` / ``loops_lost`` with their masks; with ``aligned=True`` also the ``aligned_`` forms
    of the last five, through `bin_map` (the followed pixels go through orca_screen_dot_enrichment).  The default threshold is NOT calibrated on the
    published checkpoints.  Taken from the batch's final maps whichever route made them, with ``strands="both"`` from the merged maps; the
    reference's dots are called once from the final ``ref_map``; the lists are matched on the host after the last batch.  With None (or False)
    nothing more is launched and every other field is what it was.  ``stats`` gains ``loops`` (K, 0 when absent) and ``loop_truncated_items``
    (items with more than K dots).

    ``boundaries`` (with ``insulation``; without it a ValueError): True (the defaults) or a `BoundaryParams` (`check_boundaries`), for domain
    boundary calls on the insulation tracks the screen already computes (orca_screen_boundary_calls: one launch over the reference's tracks, one per
    batch over its items' tracks, every width at once): `ScreenResult.ref_boundaries`, ``ref_boundary_strength``, ``ref_boundary_count``,
    ``boundaries``, ``boundary_strength``, ``boundary_count``, and which reference boundaries an item keeps, weakens or loses and which it creates -
    ``boundary_followed_at``, ``boundary_strength_delta``, ``boundary_delta``, ``ref_boundary_is_lost`` / ``boundaries_lost``, ``boundary_is_gained`` /
    ``boundaries_gained`` and the two ``*_is_unmapped`` masks; with ``aligned=True`` also their ``aligned_`` forms through `bin_map`.  A boundary's
    strength is the prominence of the dip in mean log observed / expected; the default ``min_strength`` is NOT calibrated on the published
    checkpoints - choose it from ``ref_boundary_strength``.  With ``strands="both"`` the tracks are the merged maps'.  The lists are matched on the
    host after the last batch.  With None (or False) nothing more is launched and every other field is what it was.  ``stats`` gains ``boundaries``
    (K, 0 when absent)."""
    return _run_screen(model, window, edits, batch=batch, keep_maps=keep_maps, stats=stats, flank=flank, aligned=aligned, flank_bp=flank_bp, strands=strands,
                       readouts=ReadoutArgs(regions, insulation, viewpoints, strata, loops, boundaries))


def _run_screen(model, window, edits, batch=64, keep_maps=False, stats=None, flank=None, aligned=False, flank_bp=None, strands="+", readouts=ReadoutArgs(), units=()):
    """The body of `screen_1m` (its arguments, its result; ``readouts``: its readout arguments as given, checked here in their turn): the routes
    of one screen.  What is read from a batch's final maps is the list of units of ``readouts`` (`readout_units`) followed by ``units``, more
    `Readout`s of the caller's (`epistasis_1m`'s bank).  Without them nothing is launched that `screen_1m` did not launch."""
    if strands not in ("+", "both"):
        raise ValueError(f"strands must be '+' or 'both', got {strands!r}")
    if readouts.boundaries is not None and readouts.boundaries is not False and readouts.insulation is None:
        raise ValueError("boundaries: called on the insulation tracks (insulation=widths)")
    both = strands == "both"
    net = _net_of(model)
    if flank_bp is not None:
        if flank is not None or not isinstance(window, tuple):
            raise ValueError("flank_bp: for a (genome, chrom, start[, L]) window without an explicit flank")
    win = _window_codes(window)
    if flank_bp is not None:
        flank_bp = int(flank_bp)
        if not 0 <= flank_bp <= win.numel():
            raise ValueError(f"flank_bp of {flank_bp}: 0 .. {win.numel()} bases")
    edits = list(edits)
    for e in edits:
        if not isinstance(e, (Edit, EditSet)):
            raise TypeError("edits: a list of screen.Edit and screen.EditSet")
        e.check(win.numel())
    if batch <= 0:
        raise ValueError("batch must be positive")
    units = readout_units(readouts, win.numel() // 4000) + list(units)
    st = {"route": None, "two_part_batches": 0, "whole_window_batches": 0, "range_fallback_batches": 0, "range_fallback_reference": False,
          "front_runs": 0, "front_bases": 0, "edits": len(edits), "set_items": sum(isinstance(e, EditSet) for e in edits), "segments": 0,
          "indel_items": sum(changes_length(e) for e in edits), "take_rows": 0, "cache_phases": 0, "aligned_items": 0,
          "strands": strands, "reverse_two_part_items": 0, "reverse_whole_items": 0, **UNSET_STATS}
    fl = _flank_codes(window, flank, win, flank_bp) if (flank is not None or st["indel_items"]) else None
    sc = _Screen(net, win, st, fl if st["indel_items"] else None)
    E, n, dev = len(edits), sc.n, sc.dev
    with torch.no_grad():
        ref_map, ref_1d, ref_gap = sc.reference(edits, batch, both)
        res = ScreenResult(ref_map, ref_1d, None, None, None, edits=edits)
        if sc.num_1d:
            res.delta_1d = torch.zeros((E, sc.num_1d, n), dtype=torch.float32, device=dev)
        if keep_maps:
            res.maps = torch.zeros((E, n, n), dtype=torch.float32, device=dev)
        if both:
            res.ref_strand_gap, res.strand_gap = ref_gap, torch.zeros(E, dtype=torch.float32, device=dev)
        res.shift = torch.tensor([shift_of(e) for e in edits], dtype=torch.int64, device=dev)
        bmaps = None
        if aligned:
            bmaps = np.stack([bin_map(e, sc.L, sc.F) for e in edits]) if E else np.zeros((0, n), dtype=np.int32)
        run = Run(sc, E, ref_map, bmaps)
        if aligned:
            st["aligned_items"] = len(run.moved)
            res.bin_map, res.aligned_bins = run.bin_maps_dev, sc._upload((bmaps >= 0).sum(axis=1), torch.int64)
        for u in units:
            st.update(u.start(res, run))
        for i0 in range(0, E, batch):
            chunk = edits[i0: i0 + batch]
            i1 = i0 + len(chunk)
            maps, h, gap = sc.final_maps(i0, chunk)
            if both:
                res.strand_gap[i0:i1] = gap
            for u in units:
                u.batch(res, run, i0, i1, maps)
            if h is not None:
                torch.sub(h, ref_1d[None], out=res.delta_1d[i0:i1])
            if keep_maps:
                res.maps[i0:i1] = maps
        for u in units:
            st.update(u.finish(res, run))
    if stats is not None:
        stats.update(st)
    return res


def epistasis_1m(model, window, sets, batch=64, regions=None, strands="+", keep_maps=False, stats=None, bank_bytes=4 << 30):
    """Non-additivity scores of ``sets`` (a list of `EditSet`; a bare `Edit` counts as a one-member set) on one window with the 1 Mb model: is the
    effect of a set the sum of its members' effects?  An `EpistasisResult`.

    ``singles, member_off, members = epistasis_items(sets)``, and ``singles + sets`` go through ONE screen (`screen_1m`'s arguments ``model``,
    ``window``, ``batch``, ``regions``, ``strands``, ``keep_maps``, ``stats`` mean what they mean there): one reference, one plan.  The singles'
    final maps - after the strand merge and after any range fallback, whichever route made them - are kept in a device bank [U, n, n], and in
    the same batch loop every set's map is scored against the bank (orca_screen_epistasis_scores, orca_screen_epistasis_region_scores): per
    pixel in fp64, t = sum_m (A_m - ref) and r = (S - ref) - t, `EpistasisResult` has the fields.  The singles come first, so every member is
    banked before a set needs it; a batch may hold the last singles and the first sets.  No set's map is kept unless ``keep_maps``.

    r is a small difference of four nearly equal maps.  An fp32 pixel is exact in fp64, so here every difference is exact up to fp64
    rounding whatever the maps hold, the sums keep their accuracy under cancellation, and only the final results are rounded to fp32
    (DESIGN 3e says what that did and did not change on the workload measured).

    ``del`` / ``ins`` members are a ValueError (`epistasis_items`).  ``bank_bytes``: the most the bank may take (U n^2 4 bytes; 4 GiB by
    default) - a larger one is a ValueError: split the set list.  ``stats`` gains ``epistasis_sets``, ``epistasis_singles`` and ``bank_bytes``
    (the bank's size)."""
    sets = list(sets)
    for s in sets:
        if not isinstance(s, (Edit, EditSet)):
            raise TypeError("sets: a list of screen.EditSet (and screen.Edit)")
    if not sets:
        raise ValueError("epistasis_1m: at least one set")
    singles, member_off, members = epistasis_items(sets)
    win = _window_codes(window)
    U, n = len(singles), win.numel() // 4000
    need = U * n * n * 4
    if need > bank_bytes:
        raise ValueError(f"epistasis_1m: the bank of {U} single-edit maps takes {need} bytes, above bank_bytes = {bank_bytes}: split the set list")
    rects = None if regions is None else check_regions(regions, n)
    out = EpistasisResult(None, singles, U, member_off, members, None, None, None, None)
    st = {}
    out.screen = _run_screen(model, win, singles + sets, batch=batch, keep_maps=keep_maps, stats=st, strands=strands, readouts=ReadoutArgs(regions=rects),
                             units=[EpistasisBank(out, rects)])
    st.update(epistasis_sets=len(sets), epistasis_singles=U, bank_bytes=need)
    if stats is not None:
        stats.update(st)
    return out
