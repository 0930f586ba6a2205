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
"""
from dataclasses import dataclass, field
from typing import Optional

import numpy as np
import torch

from . import engine, sv
from ._lib import OrcaHipError

ROW_BP = sv.S4_GRID * sv.S3_POOL          # 400 bases per stage-5 input row
MARGIN_BP = sv.S4_MARGIN_BP               # >= 1 616: reach of stages 1-4 beyond a row's bases
PAD_BP = sv.S4_PAD_BP                     # a snippet extends this far beyond the rows it is run for (>= MARGIN_BP, a multiple of 400)
MIN_SNIPPET_BP = sv.S4_MIN_SNIPPET_BP
# snippets are concatenated into front runs of at most this many bases.  Below 262 144 bases (65 536 stage-2 positions) a run's convs use the
# same kernels whatever its length, so a snippet's rows are bit for bit the same in whichever run (batch, order) it lands; a longer snippet
# runs alone
RUN_MAX_BP = 256_000
N_CODE = 4
KINDS = ("sub", "mask", "inv")
_ACGTN = {c: i for i, c in enumerate("ACGTN")}


def _codes_of(seq):
    if isinstance(seq, str):
        try:
            return np.array([_ACGTN[c] for c in seq.upper()], dtype=np.uint8)
        except KeyError:
            raise ValueError("a substitution's seq: letters A, C, G, T, N only") from None
    a = np.asarray(seq)
    if a.ndim != 1 or not np.issubdtype(a.dtype, np.integer) or (a.size and (a.min() < 0 or a.max() > 4)):
        raise ValueError("a substitution's seq: an ACGTN string or a 1-D sequence of codes 0..4")
    return a.astype(np.uint8)


class Edit:
    """A length-preserving edit of a window, ``pos`` relative to the window's first base:
      ``Edit("sub", pos, length, seq)``  bases [pos, pos + length) replaced by ``seq`` (an ACGTN string or codes 0..4 = A, C, G, T, N)
      ``Edit("mask", pos, length)``      the span set to N (code 4: the reference's 0.25 row)
      ``Edit("inv", pos, length)``       the span reverse-complemented in place (N stays N)"""

    __slots__ = ("kind", "pos", "length", "seq")

    def __init__(self, kind, pos, length, seq=None):
        if kind not in KINDS:
            raise ValueError(f"edit kind must be one of {KINDS}, got {kind!r}")
        pos, length = int(pos), int(length)
        if length <= 0:
            raise ValueError(f"edit length must be positive, got {length}")
        if pos < 0:
            raise ValueError(f"edit position must be >= 0, got {pos}")
        if kind == "sub":
            if seq is None:
                raise ValueError("a substitution needs seq")
            seq = _codes_of(seq)
            if seq.size != length:
                raise ValueError(f"substitution of {length} bases with a payload of {seq.size}")
        elif seq is not None:
            raise ValueError(f"a '{kind}' edit takes no seq")
        self.kind, self.pos, self.length, self.seq = kind, pos, length, seq

    @property
    def end(self):
        return self.pos + self.length

    def check(self, L):
        if self.end > L:
            raise ValueError(f"edit [{self.pos}, {self.end}) leaves the window of {L} bases")

    def __repr__(self):
        s = "" if self.seq is None else ", " + "".join("ACGTN"[c] for c in self.seq[:16]) + ("..." if self.length > 16 else "")
        return f"Edit({self.kind!r}, {self.pos}, {self.length}{s})"


def apply_edit(codes, edit):
    """The edited window as numpy uint8 (host restatement of the device kernel; ``codes``: [L] codes 0..4)."""
    c = np.array(codes, dtype=np.uint8, copy=True)
    edit.check(c.size)
    s = slice(edit.pos, edit.end)
    if edit.kind == "sub":
        c[s] = edit.seq
    elif edit.kind == "mask":
        c[s] = N_CODE
    else:
        r = c[s][::-1]
        c[s] = np.where(r < 4, 3 - r, r)
    return c


# ---- generators ----------------------------------------------------------------------------------------------------------------------------
def saturation_edits(codes, start, end):
    """Every single-base substitution of window bases [start, end): 3 per position (the other bases), 4 where the reference base is N."""
    c = np.asarray(codes.cpu() if isinstance(codes, torch.Tensor) else codes)
    if not 0 <= start <= end <= c.size:
        raise ValueError(f"[{start}, {end}) outside the window of {c.size} bases")
    return [Edit("sub", p, 1, [b]) for p in range(start, end) for b in range(4) if b != int(c[p])]


def tile_edits(kind, width, step, start, end):
    """``mask`` or ``inv`` tiles of ``width`` bases every ``step`` bases, each inside [start, end)."""
    if kind not in ("mask", "inv"):
        raise ValueError("tile_edits: kind 'mask' or 'inv'")
    if width <= 0 or step <= 0:
        raise ValueError("tile_edits: width and step must be positive")
    return [Edit(kind, p, width) for p in range(start, end - width + 1, step)]


# ---- planning (pure; tests/test_screen_cpu.py checks it against the fp64 oracle) -----------------------------------------------------------
@dataclass
class BatchPlan:
    """The two-part route's work for one batch of edits on an L-base window.  Per edit i: snippet[i] = (b0, nb) window bases through the front,
    rows[i] = (r0, r1) the stage-5 rows it replaces (pooled rows (r0 - b0 / 400) .. of its run); ``order``: the edits' snippets in the packed
    codes buffer; ``runs``: (first base in the buffer, bases, [(skip, count, fresh_row0)]) - one front run each; ``fresh[i]``: edit i's first
    row in the recomputed rows [R, 128]; ``edit_table`` / ``splice_table``: the device tables of orca_screen_edit_codes / _splice_rows."""
    L: int
    snippet: np.ndarray
    rows: np.ndarray
    order: list
    runs: list
    fresh: np.ndarray
    n_fresh: int
    edit_table: np.ndarray
    splice_table: np.ndarray
    payload: np.ndarray


def edit_rows(edit, L, margin=MARGIN_BP):
    """Stage-5 rows [r0, r1) whose cone (the row's 400 bases +- margin) meets the edit."""
    n5 = L // ROW_BP
    return max(0, (edit.pos - margin) // ROW_BP), min(n5, -(-(edit.end + margin) // ROW_BP))


def edit_snippet(r0, r1, L, pad=PAD_BP, min_snippet=MIN_SNIPPET_BP):
    """Window bases [b0, b1) that give rows [r0, r1) exactly: pad bases either side, clipped to the window (a snippet that reaches an end then
    starts / ends there, and its zero padding is the window's), at least ``min_snippet`` long."""
    b0, b1 = max(0, r0 * ROW_BP - pad), min(L, r1 * ROW_BP + pad)
    while b1 - b0 < min_snippet and (b0 > 0 or b1 < L):
        if b1 < L:
            b1 = min(L, b1 + ROW_BP)
        else:
            b0 = max(0, b0 - ROW_BP)
    return b0, b1


def _runs(snips, L, run_max):
    """Group snippets into front runs: a snippet at the window's start must open its run, one at the end close it (the run's ends are then the
    window's); runs stay <= run_max bases, longer snippets and snippets that span the whole window run alone."""
    alone, lefts, rights, mids = [], [], [], []
    for i, (b0, b1) in enumerate(snips):
        left, right = b0 == 0, b1 == L
        (alone if (left and right) or b1 - b0 > run_max else lefts if left else rights if right else mids).append(i)
    runs = [[i] for i in lefts]
    size = [snips[i][1] - snips[i][0] for i in lefts]
    closed = [False] * len(runs)

    def place(i, close):
        nb = snips[i][1] - snips[i][0]
        for k in range(len(runs)):
            if not closed[k] and size[k] + nb <= run_max:
                runs[k].append(i)
                size[k] += nb
                closed[k] = close
                return
        runs.append([i])
        size.append(nb)
        closed.append(close)
    for i in mids:
        place(i, False)
    for i in rights:
        place(i, True)
    return runs + [[i] for i in alone]


def plan_batch(edits, L, pad=PAD_BP, margin=MARGIN_BP, min_snippet=MIN_SNIPPET_BP, run_max=RUN_MAX_BP):
    """The `BatchPlan` of ``edits`` on an L-base window (L a multiple of 400)."""
    if L % ROW_BP:
        raise ValueError(f"window length must be a multiple of {ROW_BP}")
    if pad < margin or pad % ROW_BP:
        raise ValueError("pad must cover the margin and be a multiple of 400")
    E = len(edits)
    rows = np.zeros((E, 2), dtype=np.int64)
    snips = []
    for i, e in enumerate(edits):
        e.check(L)
        r0, r1 = edit_rows(e, L, margin)
        rows[i] = r0, r1
        snips.append(edit_snippet(r0, r1, L, pad, min_snippet))
    runs_idx = _runs(snips, L, run_max)
    order = [i for r in runs_idx for i in r]
    out_off = {}
    off = 0
    for i in order:
        out_off[i] = off
        off += snips[i][1] - snips[i][0]
    fresh = np.zeros(E, dtype=np.int64)
    n_fresh = 0
    for i in order:
        fresh[i] = n_fresh
        n_fresh += int(rows[i, 1] - rows[i, 0])
    runs = []
    for r in runs_idx:
        o0 = out_off[r[0]]
        nb = sum(snips[i][1] - snips[i][0] for i in r)
        ranges = [(int(out_off[i] - o0 + rows[i, 0] * ROW_BP - snips[i][0]) // ROW_BP, int(rows[i, 1] - rows[i, 0]), int(fresh[i])) for i in r]
        runs.append((o0, nb, ranges))
    payload, pay_off = [], {}
    npay = 0
    for i, e in enumerate(edits):
        if e.kind == "sub":
            pay_off[i] = npay
            payload.append(e.seq)
            npay += e.length
    table = np.zeros((E, engine.SCREEN_EDIT_FIELDS), dtype=np.int64)
    for k, i in enumerate(order):
        e = edits[i]
        table[k, :7] = (out_off[i], snips[i][0], snips[i][1] - snips[i][0], engine.SCREEN_KINDS[e.kind], e.pos, e.length, pay_off.get(i, 0))
    splice = np.stack([rows[:, 0], rows[:, 1] - rows[:, 0], fresh], axis=1).astype(np.int64)
    return BatchPlan(L, np.array([(b0, b1 - b0) for b0, b1 in snips], dtype=np.int64).reshape(E, 2), rows, order, runs, fresh, n_fresh, table, splice,
                     np.concatenate(payload) if payload else np.zeros(0, dtype=np.uint8))


def whole_window_table(edits, L):
    """Edit table of the whole-window route: edit i's complete edited window at bases [i L, (i + 1) L) of the output."""
    payload, npay, table = [], 0, np.zeros((len(edits), engine.SCREEN_EDIT_FIELDS), dtype=np.int64)
    for i, e in enumerate(edits):
        e.check(L)
        po = 0
        if e.kind == "sub":
            po = npay
            payload.append(e.seq)
            npay += e.length
        table[i, :7] = (i * L, 0, L, engine.SCREEN_KINDS[e.kind], e.pos, e.length, po)
    return table, (np.concatenate(payload) if payload else np.zeros(0, dtype=np.uint8))


# ---- scores ---------------------------------------------------------------------------------------------------------------------------------
def scores_host(maps, ref_map):
    """The scores of `ScreenResult` from alt maps [E, n, n] and the reference map [n, n] (fp64 host restatement of orca_screen_scores):
    d = |alt - ref|; delta_profile[e, i] = mean_j d[e, i, j]; delta_abs_mean[e] = mean_ij d[e, i, j]; delta_abs_max[e] = max_ij d[e, i, j]."""
    d = np.abs(np.asarray(maps, dtype=np.float64) - np.asarray(ref_map, dtype=np.float64)[None])
    return d.mean(axis=2), d.mean(axis=(1, 2)), d.max(axis=(1, 2))


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
    `scores_host` computes the three map scores from maps on the host."""
    ref_map: torch.Tensor
    ref_1d: Optional[torch.Tensor]
    delta_profile: torch.Tensor
    delta_abs_mean: torch.Tensor
    delta_abs_max: torch.Tensor
    delta_1d: Optional[torch.Tensor] = None
    maps: Optional[torch.Tensor] = None
    edits: list = field(default_factory=list)


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


class _Screen:
    def __init__(self, net, window, stats):
        self.net, self.window, self.stats = net, window, stats
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

    def whole(self, edits):
        """Maps of the edited windows through Net's own Encoder and Decoder_1m (the module guards apply as in Net.forward)."""
        if not edits:
            return self._decode(self.net._enc.forward_codes(self.window[None]))
        table, payload = whole_window_table(edits, self.L)
        codes = torch.empty(len(edits) * self.L, dtype=torch.uint8, device=self.dev)
        pay = self._upload(payload, torch.uint8) if payload.size else None
        engine.screen_edit_codes(self.ctx, self.window, table, self._upload(table, torch.int64), pay, codes)
        return self._decode(self.net._enc.forward_codes(codes.view(len(edits), self.L)))

    def reference_rows(self):
        enc = self.net._enc
        s5 = torch.empty((self.n5, 128), dtype=torch.float32, device=self.dev)
        enc.front4_ranges(self.window, False, [(0, self.n5, 0)], s5)
        return s5

    def two_part(self, edits, s5_ref):
        enc = self.net._enc
        p = plan_batch(edits, self.L)
        total = int(p.snippet[:, 1].sum())
        codes = torch.empty(total, dtype=torch.uint8, device=self.dev)
        pay = self._upload(p.payload, torch.uint8) if p.payload.size else None
        engine.screen_edit_codes(self.ctx, self.window, p.edit_table, self._upload(p.edit_table, torch.int64), pay, codes)
        fresh = torch.empty((p.n_fresh, 128), dtype=torch.float32, device=self.dev)
        for o0, nb, ranges in p.runs:
            enc.front4_ranges(codes[o0: o0 + nb], False, ranges, fresh)
        rows = torch.empty((len(edits), self.n5, 128), dtype=torch.float32, device=self.dev)
        engine.screen_splice_rows(self.ctx, s5_ref, fresh, self._upload(p.splice_table, torch.int64), rows)
        out = enc.back5_batch(rows)
        self.stats["front_runs"] += len(p.runs)
        self.stats["front_bases"] += total
        return self._decode(out)


def screen_1m(model, window, edits, batch=64, keep_maps=False, stats=None):
    """Score ``edits`` (a list of `Edit`) of one window with the 1 Mb model: a `ScreenResult`.

    ``model``: an ``H1esc_1M`` / ``Hff_1M`` container or a bare ``orca_modules.Net``.  ``window``: the window's base codes, a [L] uint8 tensor on
    the MI355X, or ``(genome, chrom, start)`` / ``(genome, chrom, start, L)`` for a `genome.PackedGenome` / `TwoBitGenome` resident there
    (L = 1 000 000 by default, as the reference's 1 Mb model).  L: a multiple of 4 000 with at most 256 bins.  Forward strand only (as the
    reference's ``pred_1m``).  ``batch``: edits per batch.  ``keep_maps``: also return every alt map.  ``stats``: a dict that receives
    counters - ``route`` ("two_part" / "whole_window"), ``two_part_batches``, ``whole_window_batches``, ``range_fallback_batches`` (batches
    redone on the whole-window route in the range-safe arithmetic after the fp16-range check fired), ``range_fallback_reference`` (the
    reference itself tripped: every batch went that way), ``front_runs``, ``front_bases``, ``edits``."""
    net = _net_of(model)
    win = _window_codes(window)
    edits = list(edits)
    for e in edits:
        if not isinstance(e, Edit):
            raise TypeError("edits: a list of screen.Edit")
        e.check(win.numel())
    if batch <= 0:
        raise ValueError("batch must be positive")
    st = {"route": None, "two_part_batches": 0, "whole_window_batches": 0, "range_fallback_batches": 0, "range_fallback_reference": False,
          "front_runs": 0, "front_bases": 0, "edits": len(edits)}
    sc = _Screen(net, win, st)
    E, n, dev = len(edits), sc.n, sc.dev
    two_part = net._enc.two_part_ok()
    with torch.no_grad():
        s5_ref = None
        if two_part:
            with engine.defer_overflow_guard():
                s5_ref = sc.reference_rows()
                enc_ref = torch.empty((1, 128, n), dtype=torch.float32, device=dev)
                net._enc.back5(s5_ref, enc_ref[0])
                ref_map, ref_1d = sc._decode(enc_ref)
            if sc.ctx.take_overflow():
                two_part = False
                st["range_fallback_reference"] = True
        if not two_part and not st["range_fallback_reference"]:
            ref_map, ref_1d = sc.whole([])
        elif st["range_fallback_reference"]:
            with engine.force_safe_precision():
                ref_map, ref_1d = sc.whole([])
        st["route"] = "two_part" if two_part else "whole_window"
        ref_map = ref_map[0].contiguous()
        ref_1d = None if ref_1d is None else ref_1d[0].contiguous()
        res = ScreenResult(ref_map, ref_1d, torch.zeros((E, n), dtype=torch.float32, device=dev), torch.zeros(E, dtype=torch.float32, device=dev),
                           torch.zeros(E, dtype=torch.float32, device=dev),
                           torch.zeros((E, sc.num_1d, n), dtype=torch.float32, device=dev) if sc.num_1d else None,
                           torch.zeros((E, n, n), dtype=torch.float32, device=dev) if keep_maps else None, edits)
        for i0 in range(0, E, batch):
            chunk = edits[i0: i0 + batch]
            if two_part:
                with engine.defer_overflow_guard():
                    maps, h = sc.two_part(chunk, s5_ref)
                if sc.ctx.take_overflow():
                    st["range_fallback_batches"] += 1
                    with engine.force_safe_precision():
                        maps, h = sc.whole(chunk)
                else:
                    st["two_part_batches"] += 1
            elif st["range_fallback_reference"]:
                st["range_fallback_batches"] += 1
                with engine.force_safe_precision():
                    maps, h = sc.whole(chunk)
            else:
                st["whole_window_batches"] += 1
                maps, h = sc.whole(chunk)
            i1 = i0 + len(chunk)
            prof, mean, amax = engine.screen_scores(sc.ctx, maps, ref_map)
            res.delta_profile[i0:i1] = prof
            res.delta_abs_mean[i0:i1] = mean
            res.delta_abs_max[i0:i1] = amax
            if h is not None:
                torch.sub(h, ref_1d[None], out=res.delta_1d[i0:i1])
            if keep_maps:
                res.maps[i0:i1] = maps
    if stats is not None:
        stats.update(st)
    return res
