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
from dataclasses import dataclass, field, replace
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
KINDS = ("sub", "mask", "inv", "del", "ins")
LEN_KINDS = ("del", "ins")                # the kinds that change the length
FLANK_BP = 8_000                          # bases read behind a (genome, chrom, start) window for the refill after deletions
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
    """An edit of a window, ``pos`` relative to the window's first base:
      ``Edit("sub", pos, length, seq)``  bases [pos, pos + length) replaced by ``seq`` (an ACGTN string or codes 0..4 = A, C, G, T, N)
      ``Edit("mask", pos, length)``      the span set to N (code 4: the reference's 0.25 row)
      ``Edit("inv", pos, length)``       the span reverse-complemented in place (N stays N)
      ``Edit("del", pos, length)``       bases [pos, pos + length) removed, pos >= 1: the alt window keeps the window's first base (it is anchored
                                         there, and refilled from the right flank)
      ``Edit("ins", pos, seq)``          ``seq`` inserted in front of base ``pos`` (0 <= pos <= L); it consumes no base: ``length`` is 0
    The first three keep the length; ``removed`` / ``inserted`` are the bases a ``del`` / ``ins`` takes out / puts in."""

    __slots__ = ("kind", "pos", "length", "seq")

    def __init__(self, kind, pos, length, seq=None):
        if kind not in KINDS:
            raise ValueError(f"edit kind must be one of {KINDS}, got {kind!r}")
        if kind == "ins":
            if seq is None:
                seq, length = length, 0                                   # Edit("ins", pos, seq)
            seq = _codes_of(seq)
            if seq.size == 0:
                raise ValueError("an insertion needs a non-empty seq")
            if int(length) not in (0, seq.size):
                raise ValueError(f"insertion of {seq.size} bases with a length of {length}")
            if int(pos) < 0:
                raise ValueError(f"edit position must be >= 0, got {pos}")
            self.kind, self.pos, self.length, self.seq = kind, int(pos), 0, seq
            return
        pos, length = int(pos), int(length)
        if kind == "del" and pos == 0 and length > 0:
            raise ValueError("a deletion starts at base 1 or later: the alt window keeps the window's first base")
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

    @property
    def removed(self):
        return self.length if self.kind == "del" else 0

    @property
    def inserted(self):
        return int(self.seq.size) if self.kind == "ins" else 0

    def check(self, L):
        if self.end > L:
            raise ValueError(f"edit [{self.pos}, {self.end}) leaves the window of {L} bases")

    def __repr__(self):
        s = "" if self.seq is None else ", " + "".join("ACGTN"[c] for c in self.seq[:16]) + ("..." if self.seq.size > 16 else "")
        if self.kind == "ins":
            return f"Edit('ins', {self.pos}{s})"
        return f"Edit({self.kind!r}, {self.pos}, {self.length}{s})"


class EditSet:
    """A compound edit: ``EditSet(edits, name=None)``, a non-empty immutable sequence of pairwise disjoint `Edit`s of one window that are applied
    together.  All positions are in the unedited window's coordinates (an ``inv`` member reads its source from the unedited window - the members
    are disjoint, so nothing else could be meant).  The members are kept sorted by ``pos``, an ``ins`` before a span that starts at its ``pos``:
    the order they are given in changes nothing.  An ``ins`` may sit at a span's first base or right behind its last one, not strictly inside
    it, and no two ``ins`` share a ``pos``."""

    __slots__ = ("edits", "name")

    def __init__(self, edits, name=None):
        edits = list(edits)
        if not edits:
            raise ValueError("an EditSet needs at least one Edit")
        for e in edits:
            if not isinstance(e, Edit):
                raise TypeError(f"an EditSet's members are screen.Edit, got {e!r}")
        edits.sort(key=lambda e: (e.pos, e.kind != "ins"))
        for a, b in zip(edits, edits[1:]):
            if b.pos < a.end:
                raise ValueError(f"an EditSet's members must be disjoint: {a!r} and {b!r} overlap")
            if a.kind == "ins" and b.kind == "ins" and a.pos == b.pos:
                raise ValueError(f"an EditSet takes one insertion per position: {a!r} and {b!r}")
        object.__setattr__(self, "edits", tuple(edits))
        object.__setattr__(self, "name", name)

    def __setattr__(self, key, value):
        raise AttributeError("an EditSet is immutable")

    def __len__(self):
        return len(self.edits)

    def __getitem__(self, i):
        return self.edits[i]

    def __iter__(self):
        return iter(self.edits)

    @property
    def pos(self):
        return self.edits[0].pos

    @property
    def end(self):
        return max(e.end for e in self.edits)

    def check(self, L):
        for e in self.edits:
            e.check(L)

    def __repr__(self):
        head = ", ".join(repr(e) for e in self.edits[:3]) + (f", ... {len(self.edits)} members" if len(self.edits) > 3 else "")
        return f"EditSet([{head}]" + ("" if self.name is None else f", name={self.name!r}") + ")"


def members_of(item):
    """The `Edit`s of a screen item (an `Edit` or an `EditSet`), sorted by ``pos``."""
    if isinstance(item, Edit):
        return (item,)
    if isinstance(item, EditSet):
        return item.edits
    raise TypeError(f"a screen item is a screen.Edit or a screen.EditSet, got {item!r}")


def changes_length(item):
    """True if a member of the item is a ``del`` or an ``ins`` (a balanced set included)."""
    return any(e.kind in LEN_KINDS for e in members_of(item))


def shift_of(item):
    """Bases removed minus bases inserted: what lies behind the item's last member is displaced by that much towards the window's start."""
    return sum(e.removed - e.inserted for e in members_of(item))


def _flank_host(flank, L):
    """``flank`` (None, numpy or a tensor) as numpy uint8 codes [F], 0 <= F <= L."""
    if flank is None:
        return np.zeros(0, dtype=np.uint8)
    f = np.asarray(flank.cpu() if isinstance(flank, torch.Tensor) else flank)
    if f.ndim != 1 or not np.issubdtype(f.dtype, np.integer) or f.size > L or (f.size and (f.min() < 0 or f.max() > 4)):
        raise ValueError(f"flank: [F] codes 0..4 with 0 <= F <= {L}, the bases that follow the window")
    return f.astype(np.uint8)


def apply_edit(codes, edit, flank=None):
    """The alt window as numpy uint8, always L bases (host restatement of the device kernels; ``codes``: [L] codes 0..4; ``edit``: an `Edit` or
    an `EditSet`, whose members all read the unedited window).  With a ``del`` / ``ins`` member it is the first L bases of (edited window ++
    ``flank`` ++ N ...); ``flank`` ([F] codes, the bases that follow the window) changes nothing otherwise."""
    src = np.asarray(codes, dtype=np.uint8)
    c = np.array(src, dtype=np.uint8, copy=True)
    edit.check(c.size)
    fl = _flank_host(flank, c.size)
    if changes_length(edit):
        cx, parts, p = np.concatenate([src, fl]), [], 0
        for e in members_of(edit):
            parts.append(cx[p: e.pos])
            if e.kind in ("sub", "ins"):
                parts.append(e.seq)
            elif e.kind == "mask":
                parts.append(np.full(e.length, N_CODE, dtype=np.uint8))
            elif e.kind == "inv":
                r = src[e.pos: e.end][::-1]
                parts.append(np.where(r < 4, 3 - r, r).astype(np.uint8))
            p = e.end
        parts += [cx[p:], np.full(c.size, N_CODE, dtype=np.uint8)]
        return np.concatenate(parts)[: c.size].astype(np.uint8)
    for e in members_of(edit):
        s = slice(e.pos, e.end)
        if e.kind == "sub":
            c[s] = e.seq
        elif e.kind == "mask":
            c[s] = N_CODE
        else:
            r = src[s][::-1]
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


def pair_edits(a, b):
    """Every pair from two edit lists applied together (epistasis screens): ``(sets, index)`` - one `EditSet` per (x, y) in a x b whose spans are
    disjoint, and ``index[k] = (i, j)``: sets[k] = {a[i], b[j]}, to line the rows up with those of the single edits."""
    sets, index = [], []
    for i, x in enumerate(a):
        for j, y in enumerate(b):
            if x.end <= y.pos or y.end <= x.pos:
                sets.append(EditSet([x, y]))
                index.append((i, j))
    return sets, index


def snv_set(codes, variants, name=None):
    """One `EditSet` of 1-base substitutions from ``variants`` = [(pos, ref, alt)] (bases as ACGTN letters or codes 0..4), e.g. a haplotype
    inside one window.  A ``ref`` that is not the window's base at ``pos``, or two variants at one position, is a ValueError."""
    c = np.asarray(codes.cpu() if isinstance(codes, torch.Tensor) else codes)
    seen, edits = set(), []
    for pos, ref, alt in variants:
        pos = int(pos)
        if not 0 <= pos < c.size:
            raise ValueError(f"variant at {pos} outside the window of {c.size} bases")
        if pos in seen:
            raise ValueError(f"two variants at position {pos}")
        seen.add(pos)
        r, a = _codes_of(ref if isinstance(ref, str) else [ref]), _codes_of(alt if isinstance(alt, str) else [alt])
        if r.size != 1 or a.size != 1:
            raise ValueError(f"variant at {pos}: ref and alt are single bases")
        if int(r[0]) != int(c[pos]):
            raise ValueError(f"variant at {pos}: ref {'ACGTN'[int(r[0])]} but the window has {'ACGTN'[int(c[pos])]}")
        edits.append(Edit("sub", pos, 1, a))
    return EditSet(edits, name)


def indel(codes, pos, ref, alt, name=None):
    """The minimal item of a VCF-style variant: at window base ``pos`` the bases ``ref`` (checked against ``codes``) become ``alt`` (ACGTN strings or
    codes, either may be empty).  The common prefix, then the common suffix, are trimmed; what is left is an `Edit` ``sub`` (equal lengths),
    ``del`` or ``ins`` (one side empty), or an `EditSet` of a ``sub`` of the shorter side's length followed by the ``del`` / ``ins`` of the rest.
    A deletion that is left starting at window base 0 (a VCF line without an anchor base there) is refused like any ``Edit("del", 0, ...)``:
    the alt window keeps the window's first base.  An insertion anchored at the window's last base gives ``Edit("ins", L, ...)``, which leaves
    the L-base alt window as it is."""
    c = np.asarray(codes.cpu() if isinstance(codes, torch.Tensor) else codes)
    pos = int(pos)
    r, a = _codes_of(ref), _codes_of(alt)
    if not 0 <= pos <= pos + r.size <= c.size:
        raise ValueError(f"variant [{pos}, {pos + r.size}) outside the window of {c.size} bases")
    if not np.array_equal(c[pos: pos + r.size], r):
        raise ValueError(f"variant at {pos}: ref {''.join('ACGTN'[k] for k in r[:16])} but the window has {''.join('ACGTN'[int(k)] for k in c[pos: pos + min(r.size, 16)])}")
    m = min(r.size, a.size)
    pre = 0
    while pre < m and r[pre] == a[pre]:
        pre += 1
    suf = 0
    while suf < m - pre and r[r.size - 1 - suf] == a[a.size - 1 - suf]:
        suf += 1
    r, a, pos = r[pre: r.size - suf], a[pre: a.size - suf], pos + pre
    if r.size == 0 and a.size == 0:
        raise ValueError(f"variant at {pos}: ref and alt are the same")
    m = min(r.size, a.size)
    rest = None if r.size == a.size else Edit("del", pos + m, r.size - m) if r.size > a.size else Edit("ins", pos + m, a[m:])
    if m == 0:
        return rest
    sub = Edit("sub", pos, m, a[:m])
    return sub if rest is None else EditSet([sub, rest], name)


def deletion_scan(width, step, start, end):
    """Deletions of ``width`` bases every ``step`` bases, each inside [start, end): ``Edit("del", p, width)`` for p = max(start, 1), p + step, ...
    (a deletion starts at base 1 or later: the alt window keeps the window's first base).  Score them with ``screen_1m(..., aligned=True)``."""
    if width <= 0 or step <= 0:
        raise ValueError("deletion_scan: width and step must be positive")
    return [Edit("del", p, width) for p in range(max(int(start), 1), int(end) - width + 1, step)]


def tandem_dup(codes, pos, length):
    """A tandem duplication of window bases [pos, pos + length) as the insertion of their copy right behind them:
    ``Edit("ins", pos + length, codes[pos: pos + length])``.  In `bin_map` the inserted copy stands for no reference bin (-1)."""
    c = np.asarray(codes.cpu() if isinstance(codes, torch.Tensor) else codes)
    pos, length = int(pos), int(length)
    if length <= 0 or not 0 <= pos <= pos + length <= c.size:
        raise ValueError(f"duplication of [{pos}, {pos + length}): non-empty and inside the window of {c.size} bases")
    return Edit("ins", pos + length, c[pos: pos + length])


# ---- aligned bins ---------------------------------------------------------------------------------------------------------------------------
BIN_BP = 4000


def bin_map(item, L, F=0):
    """The reference bin every bin of the item's alt map stands for: np.int32 [n], n = L // 4000, -1 for none.  An alt bin is placed by its
    midpoint base a = 4000 i + 2000.  Walking the item's members in their sorted order with cum = bases inserted - removed so far, a surviving
    reference base p sits at alt position p + cum.  If a is a surviving base of the window (p < L), ``bin_map[i] = p // 4000``; ``sub``, ``mask``
    and ``inv`` spans stand where they stood (p = a - cum, not mirrored for ``inv``).  -1: a is an inserted base, was refilled from the flank
    (p >= L; ``F``, the flank's length, 0 <= F <= L, therefore changes nothing: the refill stands for no reference bin whatever fills it) or is
    N fill beyond the context.

    A length-preserving item maps every bin to itself, and a shift below 2 000 bases leaves the map the identity wherever no midpoint crosses a
    bin edge.  All pieces are forward and in order, so the mapped values never decrease with i; next to an insertion two alt bins may share a
    reference bin, which is why every aligned result is indexed by ALT bin.  A mapped bin's midpoint lies inside its reference bin by
    construction; what remains is a misregistration below half a bin, inherent to a 4 kb map: behind a shift that is no multiple of 4 000 the
    aligned score of an otherwise silent edit is not zero."""
    members = members_of(item)
    if L % BIN_BP or not 0 <= int(F) <= L:
        raise ValueError(f"bin_map: a window of {L} bases (a multiple of {BIN_BP}) with a flank of {F} (0 .. {L})")
    item.check(L)
    mid = BIN_BP * np.arange(L // BIN_BP, dtype=np.int64) + BIN_BP // 2
    out = np.full(mid.size, -1, dtype=np.int32)
    p, cum = 0, 0
    runs = []                                            # (first surviving base, one past the last, cum): alt [p0 + cum, p1 + cum)
    for e in members:
        if e.kind in LEN_KINDS:
            runs.append((p, e.pos, cum))
            cum += e.inserted - e.removed
            p = e.end
    runs.append((p, L, cum))
    for p0, p1, s in runs:
        m = (mid >= p0 + s) & (mid < p1 + s)
        out[m] = (mid[m] - s) // BIN_BP
    return out


def _bin_maps(bin_map_, E, n):
    m = np.asarray(bin_map_)
    if m.ndim == 1:
        m = np.repeat(m[None], E, axis=0)
    if m.shape != (E, n) or not np.issubdtype(m.dtype, np.integer) or (m.size and (m.min() < -1 or m.max() >= n)):
        raise ValueError(f"bin_map: [{E}, {n}] integers -1 .. {n - 1}")
    return m.astype(np.int64)


# ---- planning (pure; tests/test_screen_cpu.py checks it against the fp64 oracle) -----------------------------------------------------------
@dataclass
class BatchPlan:
    """The two-part route's work for one batch of items (`Edit` / `EditSet`) on an L-base window.  A bare `Edit` is one snippet; an `EditSet` is
    one snippet per CLUSTER of its members' rows (row intervals that overlap or touch are merged).  For a list of bare `Edit`s snippet k is
    edit k.  Per snippet k: ``item_of[k]`` its item, snippet[k] = (b0, nb) window bases through the front, rows[k] = (r0, r1) the stage-5
    rows it replaces (pooled rows (r0 - b0 / 400) .. of its run); ``order``: the snippets in the packed codes buffer; ``runs``: (first base in
    the buffer, bases, [(skip, count, fresh_row0)]) - one front run each; ``fresh[k]``: snippet k's first row in the recomputed rows [R, 128].
    Device tables: ``edit_table`` / ``splice_table`` of orca_screen_edit_codes / _splice_rows (None when an item has more than one member);
    ``snippet_table`` [S, 8] = [out_off, b0, nb, span_lo, span_cnt, 0, 0, 0] in ``order``, ``span_table`` [n, 4] = [kind, pos, len, pay_off]
    (item by item, sorted by pos within an item; a snippet applies every span of its item that meets it, whichever cluster the span
    belongs to), ``segments`` [S, 3] = [row_lo, row_cnt, src_row] item by item, sorted by row_lo, item i's at
    [seg_off[i], seg_off[i + 1]) - the tables of orca_screen_edit_codes_multi / _splice_rows_multi.

    A batch with a length-changing item (``indel`` True; `plan_batch` states the row-source rule): snippets are in ALT coordinates,
    ``snippet_table`` [S, 8] = [out_off, a0, nb, piece_lo, piece_cnt, 0, 0, 0] and ``piece_table`` [n, 4] = [dst, kind, src, len] (item by item,
    item i's at [piece_off[i], piece_off[i + 1]), sorted by dst; kind 0 context forward, 1 context reverse complement, 2 payload, 3 N) are the
    tables of orca_screen_assemble_codes; ``gather_segments`` [G, 4] = [row_lo, row_cnt, source, src_row] with offsets ``gather_off`` [E + 1]
    those of orca_screen_gather_rows (source -1 fresh, -2 ref, p >= 0 entry ``phases[p]`` of the stage-4 cache, which must hold
    ``entry_rows[p]`` rows); ``segments`` keeps the fresh ones; ``take_rows`` counts the pooled rows, ``shift[i]`` = bases removed - inserted.
    The single-span and span tables are None."""
    L: int
    snippet: np.ndarray
    rows: np.ndarray
    order: list
    runs: list
    fresh: np.ndarray
    n_fresh: int
    edit_table: Optional[np.ndarray]
    splice_table: Optional[np.ndarray]
    payload: np.ndarray
    item_of: np.ndarray = None
    snippet_table: np.ndarray = None
    span_table: np.ndarray = None
    segments: np.ndarray = None
    seg_off: np.ndarray = None
    indel: bool = False
    flank: int = 0
    piece_table: np.ndarray = None
    piece_off: np.ndarray = None
    gather_segments: np.ndarray = None
    gather_off: np.ndarray = None
    phases: list = None
    entry_rows: list = None
    take_rows: int = 0
    shift: np.ndarray = None
    reverse: bool = False                     # `mirror_plan`: the row tables are the '-' strand's (the codes tables never change)
    both_strands: bool = False                # a ``del`` / ``ins`` batch planned so that `mirror_plan` applies (`item_sources`)


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


def set_clusters(item, L, margin=MARGIN_BP):
    """The row clusters of an item: `edit_rows` of every member, intervals that overlap or touch merged - [(r0, r1)] ascending.  Rows between
    two clusters are outside every member's cone, so they keep the reference's values."""
    out = []
    for e in members_of(item):                       # sorted by pos: r0 ascends
        r0, r1 = edit_rows(e, L, margin)
        if out and r0 <= out[-1][1]:
            out[-1][1] = max(out[-1][1], r1)
        else:
            out.append([r0, r1])
    return [(a, b) for a, b in out]


def _item_table(items, rows_of):
    """Every item's rows of a 4-field sub-table (spans / pieces), item by item: (table [n, 4] int64, first row of every item [E + 1], payload,
    per-item row lists).  ``rows_of(item, pay_off)`` = (the item's rows, its payload codes), ``pay_off`` its first code's place in the payload."""
    rows, lists, pay, npay = [], [], [], 0
    base = np.zeros(len(items) + 1, dtype=np.int64)
    for i, it in enumerate(items):
        mine, py = rows_of(it, npay)
        lists.append(mine)
        rows += mine
        pay.append(py)
        npay += py.size
        base[i + 1] = len(rows)
    return np.array(rows, dtype=np.int64).reshape(-1, 4), base, (np.concatenate(pay) if pay else np.zeros(0, dtype=np.uint8)), lists


def _item_spans(item, pay_off=0):
    """The members of ``item`` as spans: ([(kind, pos, len, pay_off)], payload codes)."""
    out, pay = [], [np.zeros(0, dtype=np.uint8)]
    for e in members_of(item):
        out.append((engine.SCREEN_KINDS[e.kind], e.pos, e.length, pay_off if e.kind == "sub" else 0))
        if e.kind == "sub":
            pay.append(e.seq)
            pay_off += e.length
    return out, np.concatenate(pay)


def _span_table(items):
    """(span table [n, 4] int64, first span of every item [E + 1], payload): every item's members, item by item."""
    return _item_table(items, _item_spans)[:3]


def _spans_meeting(spans, lo, hi, b0, b1):
    """Of spans [lo, hi) (sorted by pos, disjoint) those that meet bases [b0, b1): (first, count)."""
    pos, end = spans[lo:hi, 1], spans[lo:hi, 1] + spans[lo:hi, 2]
    a, b = int(np.searchsorted(end, b0, side="right")), int(np.searchsorted(pos, b1, side="left"))
    return lo + a, max(0, b - a)


# ---- insertions and deletions: piece lists and row sources -----------------------------------------------------------------------------------
def entry_rows(C, phase):
    """Rows of entry ``phase`` (0..79) of `sv.Stage4Cache` over a context of C bases: stage 4's output on context bases [phase, phase + 80 rows)
    (the entry's run).  The five entries of a phase mod 16 share stage-3 planes that end at a multiple of 80 from that phase."""
    p16, k = phase % sv.S3_GRID, phase // sv.S3_GRID
    return max(0, min((C - phase) // sv.S4_GRID, ((C - p16) // sv.S4_GRID * sv.S3_POOL - k) // sv.S3_POOL))


def item_pieces(item, L, F, pay_off=0):
    """The alt window of ``item`` as pieces over the context (window ++ flank, C = L + F): ([(dst, kind, src, len)], payload codes).  The pieces
    tile alt bases [0, L) in order.  kind 0: context [src, src + len) forward; 1: its reverse complement; 2: payload codes [src, src + len)
    (``pay_off`` = the first code's place in the batch's payload); 3: N."""
    C, out, pay, d, p = L + F, [], [], 0, 0

    def put(kind, src, ln, back=False):
        nonlocal d
        n = min(ln, L - d)
        if n > 0:
            out.append((d, kind, src + (ln - n if back else 0), n))         # a reverse complement cut at L keeps its FIRST alt bases: the span's last
            d += n
    npay = pay_off
    for e in members_of(item):
        put(0, p, e.pos - p)
        if e.kind in ("sub", "ins"):
            put(2, npay, int(e.seq.size))
            pay.append(e.seq)
            npay += int(e.seq.size)
        elif e.kind == "mask":
            put(3, 0, e.length)
        elif e.kind == "inv":
            put(1, e.pos, e.length, back=True)
        p = e.end
    put(0, p, C - p)
    put(3, 0, L - d)
    return out, (np.concatenate(pay) if pay else np.zeros(0, dtype=np.uint8))


def item_sources(pieces, L, F, margin=MARGIN_BP, both_strands=False):
    """Where the stage-5 rows of an alt window come from: (segments, fresh) with segments = [(row_lo, row_cnt, source, src_row)] for source -2
    (reference rows [src_row, ..)) and source = a phase 0..79 (pooled from that cache entry's stage-4 row src_row on), and fresh = [(r0, r1)]
    the maximal runs of rows that go through the front.  Rows in neither keep the reference's row of their own index.  The rule, with the
    cone of row r = alt bases [400 r - margin, 400 r + 400 + margin) and s = context position - alt position of a context-forward piece:
      * a row is served without the front only if its cone lies inside ONE context-forward piece (the alt window's start counts as inside for
        a piece with s = 0 that starts there, its end for a piece with s = 0 that ends there: these ends are the window's own);
      * s = 0: the reference's row r.  400 | s: the reference's row r + s / 400 if that row's cone lies inside the window [0, L) (the
        reference rows saw zero padding there).  Otherwise entry s mod 80, stage-4 rows (400 r + s - phase) / 80 .. + 4, if the cone in
        context coordinates lies inside the entry's run (the cache saw zero padding at its ends);
      * everything else is fresh: junctions, payload, inversions, N fill, and the alt window's right end whenever s != 0 there.
    ``both_strands`` (``strands="both"``; off by default, and then every plan is what it ever was): the '-' strand serves the same rows from the
    '-' cache - on that strand the row is pooled from entry (C - s) mod 80 of the reverse-complemented context, whose run ends elsewhere, within
    a few rows of the context's ends - so a take is kept only where the cone lies inside the run of BOTH entries (`mirror_plan` then is a
    pure table transform); the rest is fresh."""
    n5, C = L // ROW_BP, L + F
    segs, served = [], np.zeros(n5, dtype=bool)
    for d0, kind, src, ln in pieces:
        if kind != 0:
            continue
        d1, s = d0 + ln, src - d0
        lo = 0 if (d0 == 0 and s == 0) else -(-(d0 + margin) // ROW_BP)
        hi = n5 if (d1 == L and s == 0) else (d1 - margin) // ROW_BP
        lo, hi = max(lo, 0), min(hi, n5)
        if hi <= lo:
            continue
        if s == 0:
            served[lo:hi] = True
            continue
        cuts = [(lo, hi)]
        if s % ROW_BP == 0:
            q = s // ROW_BP
            a, b = max(lo, -(-margin // ROW_BP) - q), min(hi, (L - margin) // ROW_BP - q)
            if b > a:
                segs.append((a, b - a, engine.SCREEN_SRC_REF, a + q))
                served[a:b] = True
                cuts = [(lo, a), (b, hi)]
        ph = s % sv.S4_GRID
        run0, run1 = ph, ph + sv.S4_GRID * entry_rows(C, ph)
        if both_strands:                                 # the '-' entry's run, in context coordinates
            pm = (C - s) % sv.S4_GRID
            run0, run1 = max(run0, C - pm - sv.S4_GRID * entry_rows(C, pm)), min(run1, C - pm)
        for x, y in cuts:
            a, b = max(x, -(-(run0 + margin - s) // ROW_BP)), min(y, (run1 - margin - s) // ROW_BP)
            if b > a:
                segs.append((a, b - a, ph, (ROW_BP * a + s - ph) // sv.S4_GRID))
                served[a:b] = True
    edge = np.flatnonzero(np.diff(np.concatenate([[False], ~served, [False]]).astype(np.int8)))
    return sorted(segs), [(int(a), int(b)) for a, b in zip(edge[0::2], edge[1::2])]


def needed_phases(items, L, F, margin=MARGIN_BP, both_strands=False):
    """The stage-4 cache entries (phases 0..79, ascending) the two-part route of ``items`` pools rows from on the '+' strand (`mirror_phases`
    gives the '-' strand's)."""
    ph = set()
    for it in items:
        if changes_length(it):
            ph.update(g[2] for g in item_sources(item_pieces(it, L, F)[0], L, F, margin, both_strands)[0] if g[2] >= 0)
    return sorted(ph)


def mirror_phases(phases, C):
    """The '-' strand's cache entries for the '+' strand's ``phases`` over a context of C bases: a row that starts at context base x = phase mod 80
    starts at base C - x - 400 of the reverse-complemented context, phase (C - phase) mod 80.  Ascending; its own inverse."""
    return sorted({(C - ph) % sv.S4_GRID for ph in phases})


def _pieces_meeting(pieces, lo, hi, a0, a1):
    """Of pieces [lo, hi) (sorted by dst, disjoint) those that meet alt bases [a0, a1): (first, count)."""
    dst, end = pieces[lo:hi, 0], pieces[lo:hi, 0] + pieces[lo:hi, 3]
    a, b = int(np.searchsorted(end, a0, side="right")), int(np.searchsorted(dst, a1, side="left"))
    return lo + a, max(0, b - a)


def _piece_table(items, L, F):
    """(piece table [n, 4] int64, first piece of every item [E + 1], payload, per-item piece lists): every item's pieces, item by item."""
    return _item_table(items, lambda it, pay_off: item_pieces(it, L, F, pay_off))


def _pack(snips, rows, L, run_max):
    """Snippets into front runs (`_runs`): (runs_idx, order, out_off {snippet: first base in the buffer}, fresh [S], n_fresh, runs)."""
    runs_idx = _runs(snips, L, run_max)
    order = [i for r in runs_idx for i in r]
    out_off, off = {}, 0
    for i in order:
        out_off[i] = off
        off += snips[i][1] - snips[i][0]
    fresh = np.zeros(len(snips), dtype=np.int64)
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
    return order, out_off, fresh, n_fresh, runs


def _layout(fresh_runs, L, pad, min_snippet, run_max, sub, base, meeting):
    """The layout both planners share, from every item's runs of rows that go through the front (``fresh_runs[i]`` = [(r0, r1)] ascending): one
    snippet per run, item by item, packed into front runs (`_pack`); the snippet table in buffer order, snippet k carrying the rows of ``sub``
    (item i's at [base[i], base[i + 1])) that ``meeting`` finds on its bases; and the fresh segments.  The `BatchPlan` fields of all that."""
    rows_l = [r for mine in fresh_runs for r in mine]
    item_of = [i for i, mine in enumerate(fresh_runs) for _ in mine]
    snips = [edit_snippet(r0, r1, L, pad, min_snippet) for r0, r1 in rows_l]
    S = len(snips)
    rows = np.array(rows_l, dtype=np.int64).reshape(S, 2)
    order, out_off, fresh, n_fresh, runs = _pack(snips, rows, L, run_max)
    snippet_table = np.zeros((S, engine.SCREEN_EDIT_FIELDS), dtype=np.int64)
    for k, i in enumerate(order):
        it = item_of[i]
        lo, cnt = meeting(sub, int(base[it]), int(base[it + 1]), snips[i][0], snips[i][1])
        snippet_table[k, :5] = (out_off[i], snips[i][0], snips[i][1] - snips[i][0], lo, cnt)
    return dict(L=L, snippet=np.array([(b0, b1 - b0) for b0, b1 in snips], dtype=np.int64).reshape(S, 2), rows=rows, order=order, runs=runs, fresh=fresh,
                n_fresh=n_fresh, item_of=np.array(item_of, dtype=np.int64), snippet_table=snippet_table,
                segments=np.stack([rows[:, 0], rows[:, 1] - rows[:, 0], fresh], axis=1).astype(np.int64).reshape(S, 3),
                seg_off=np.cumsum([0] + [len(mine) for mine in fresh_runs], dtype=np.int64))


def _plan_indels(edits, L, F, pad, margin, min_snippet, run_max, both_strands=False):
    """`plan_batch` for a batch that holds a length-changing item: every item, the length-preserving ones too, as pieces and row sources.  A
    length-preserving item gets the clusters, snippets and fresh rows it gets alone (its pieces all have s = 0, so the rows outside every
    member's cone are served and the others are not: `set_clusters`' rule), and the front runs give a snippet's rows bit for bit in
    whichever run it lands."""
    E = len(edits)
    pieces, piece_off, payload, lists = _piece_table(edits, L, F)
    sources = [item_sources(pcs, L, F, margin, both_strands) for pcs in lists]
    served = [segs for segs, _ in sources]
    p = _layout([mine for _, mine in sources], L, pad, min_snippet, run_max, pieces, piece_off, _pieces_meeting)
    phases = sorted({g[2] for segs in served for g in segs if g[2] >= 0})
    index = {ph: k for k, ph in enumerate(phases)}
    gather, gather_off, take_rows = [], np.zeros(E + 1, dtype=np.int64), 0
    for i in range(E):
        mine = [(int(r0), int(cnt), engine.SCREEN_SRC_FRESH, int(src)) for r0, cnt, src in p["segments"][p["seg_off"][i]: p["seg_off"][i + 1]]]
        for r0, cnt, source, src in served[i]:
            mine.append((r0, cnt, index[source] if source >= 0 else source, src))
            take_rows += cnt if source >= 0 else 0
        gather += sorted(mine)
        gather_off[i + 1] = len(gather)
    return BatchPlan(edit_table=None, splice_table=None, payload=payload, indel=True, flank=F, piece_table=pieces, piece_off=piece_off,
                     gather_segments=np.array(gather, dtype=np.int64).reshape(-1, engine.SCREEN_GATHER_FIELDS), gather_off=gather_off, phases=phases,
                     entry_rows=[entry_rows(L + F, ph) for ph in phases], take_rows=take_rows, shift=np.array([shift_of(e) for e in edits], dtype=np.int64), both_strands=both_strands, **p)


def plan_batch(edits, L, pad=PAD_BP, margin=MARGIN_BP, min_snippet=MIN_SNIPPET_BP, run_max=RUN_MAX_BP, flank=0, both_strands=False):
    """The `BatchPlan` of ``edits`` (`Edit`s and `EditSet`s) on an L-base window (L a multiple of 400) followed by ``flank`` bases of right flank
    (only a batch with a ``del`` / ``ins`` member looks at it; such a batch is planned by the row-source rule of `item_sources`, with
    ``both_strands`` in the form that `mirror_plan` can mirror; a batch without such a member plans the same either way)."""
    if L % ROW_BP:
        raise ValueError(f"window length must be a multiple of {ROW_BP}")
    if pad < margin or pad % ROW_BP:
        raise ValueError("pad must cover the margin and be a multiple of 400")
    if not 0 <= int(flank) <= L:
        raise ValueError(f"flank of {flank} bases: 0 .. {L}")
    indel = any(changes_length(e) for e in edits)
    for e in edits:
        e.check(L)
    if indel:
        return _plan_indels(edits, L, int(flank), pad, margin, min_snippet, run_max, both_strands)
    spans, span_base, payload = _span_table(edits)
    p = _layout([set_clusters(e, L, margin) for e in edits], L, pad, min_snippet, run_max, spans, span_base, _spans_meeting)
    table = splice = None
    if len(spans) == len(edits):                     # one member per item: the tables of the single-span kernels, snippet i = item i with its span
        table, splice = p["snippet_table"].copy(), p["segments"].copy()
        table[:, 3:7] = spans[p["order"]]
    return BatchPlan(edit_table=table, splice_table=splice, payload=payload, span_table=spans, **p)


def mirror_plan(plan):
    """The plan of the same batch on the '-' strand (``strands="both"``): a pure table transform, its own inverse.  The edited snippets are
    generated once, in forward coordinates - ``edit_table``, ``snippet_table``, ``span_table``, ``payload``, ``order`` and the buffer offsets in
    ``runs`` stay as they are - and the front reads the same buffer with ``reverse=True``: it reverse-complements the whole run, so the pooled
    rows come out in '-' order.  L is a multiple of 400 and every snippet bound is a multiple of 400 or a window end, so the '-' strand's
    400-base grid is the mirror of the '+' grid and '+' row r is '-' row n5 - 1 - r:
      * a run of nr pooled rows sends the range (skip, count, dst) to (nr - skip - count, count, dst): a snippet keeps its place in the
        recomputed rows, and its rows lie there ascending in '-' row index;
      * a segment (row_lo, cnt, src_row) becomes (n5 - row_lo - cnt, cnt, src_row), each item's segments re-sorted by row_lo;
      * ``rows`` and ``snippet`` are restated in '-' coordinates ((n5 - r1, n5 - r0) and (L - b0 - nb, nb)).
    A run that a window-start snippet opens is, reversed, a run that a window-end snippet closes: `_runs`' rule holds on the '-' strand.
    A plan with row sources (``indel``; it must have been made with ``both_strands``, so that every take lies inside the run of the '-' entry
    too) mirrors its gather segments [row_lo, row_cnt, source, src_row] the same way, with C = L + flank: a fresh source keeps src_row; a
    reference source (-2) reads the '-' reference rows [n5 - src_row - cnt, ..); a take from entry ``phases[p]`` starts at context base
    x = 80 src_row + phase and becomes a take from the '-' entry of phase (C - phase) mod 80 (`mirror_phases`) at stage-4 row
    (C - x - 400 cnt - that phase) / 80.  ``phases`` and ``entry_rows`` are then the '-' cache's."""
    if plan.indel and not plan.both_strands:
        raise ValueError("mirror_plan: a del / ins batch must be planned with both_strands=True (its takes must lie inside the '-' entries' runs too)")
    L, n5 = plan.L, plan.L // ROW_BP
    more = {}
    if plan.indel:
        C = L + plan.flank
        phases = mirror_phases(plan.phases, C)
        index = {ph: k for k, ph in enumerate(phases)}
        g = plan.gather_segments.copy()
        for k, (a, cnt, source, src) in enumerate(plan.gather_segments):
            if source == engine.SCREEN_SRC_REF:
                src = n5 - src - cnt
            elif source >= 0:
                ph = plan.phases[source]
                pm = (C - ph) % sv.S4_GRID
                source, src = index[pm], (C - (sv.S4_GRID * src + ph) - ROW_BP * cnt - pm) // sv.S4_GRID
            g[k] = (n5 - a - cnt, cnt, source, src)
        for i in range(len(plan.gather_off) - 1):
            a, b = int(plan.gather_off[i]), int(plan.gather_off[i + 1])
            g[a:b] = g[a:b][::-1]
        more = dict(gather_segments=g, phases=phases, entry_rows=[entry_rows(C, ph) for ph in phases])

    def seg(t):
        return None if t is None else np.stack([n5 - t[:, 0] - t[:, 1], t[:, 1], t[:, 2]], axis=1).astype(np.int64).reshape(-1, 3)
    segments = seg(plan.segments)
    for i in range(len(plan.seg_off) - 1):
        a, b = int(plan.seg_off[i]), int(plan.seg_off[i + 1])
        segments[a:b] = segments[a:b][::-1]              # ascending and disjoint before: descending after the mirror
    runs = [(o0, nb, [(nb // ROW_BP - skip - count, count, dst) for skip, count, dst in ranges]) for o0, nb, ranges in plan.runs]
    return replace(plan, reverse=not plan.reverse, runs=runs, segments=segments, splice_table=seg(plan.splice_table), **more,
                   rows=np.stack([n5 - plan.rows[:, 1], n5 - plan.rows[:, 0]], axis=1).astype(np.int64).reshape(-1, 2),
                   snippet=np.stack([L - plan.snippet[:, 0] - plan.snippet[:, 1], plan.snippet[:, 1]], axis=1).astype(np.int64).reshape(-1, 2))


def _whole_window(items, L, sub_table):
    """The tables of the whole-window route: item i's complete edited window at bases [i L, (i + 1) L) of the output, one [0, L) snippet with all of
    the item's rows of ``sub_table(items)`` = (sub-table, first row of every item, payload, ..) - (snippet table, sub-table, payload)."""
    for it in items:
        it.check(L)
    sub, base, payload = sub_table(items)[:3]
    table = np.zeros((len(items), engine.SCREEN_EDIT_FIELDS), dtype=np.int64)
    table[:, 0], table[:, 2], table[:, 3], table[:, 4] = L * np.arange(len(items)), L, base[:-1], np.diff(base)
    return table, sub, payload


def whole_window_table(edits, L):
    """Edit table of the whole-window route: edit i's complete edited window at bases [i L, (i + 1) L) of the output."""
    table, spans, payload = _whole_window(edits, L, _span_table)
    table[:, 3:7] = spans                            # bare edits: the one span in the snippet's own row
    return table, payload


def whole_window_piece_tables(items, L, F):
    """`whole_window_set_tables` for a batch with a length-changing item: (snippet table, piece table, payload) of orca_screen_assemble_codes."""
    return _whole_window(items, L, lambda its: _piece_table(its, L, F))


def whole_window_set_tables(items, L):
    """`whole_window_table` for `Edit`s and `EditSet`s: (snippet table, span table, payload) of orca_screen_edit_codes_multi."""
    return _whole_window(items, L, _span_table)


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
    sums = {k: np.zeros((E, c, c)) for k in "PDLHV"}
    cnt = dict.fromkeys("PDLHV", 0)
    for a in range(-w, w + 1):
        for b in range(-w, w + 1):
            x = m64[:, w + a: w + a + c, w + b: w + b + c]
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
    nan = np.zeros((E, c, c), dtype=bool)
    for k in "PDLHV":
        nan |= np.isnan(mean[k])
    with np.errstate(invalid="ignore"):
        bg = mean["D"]
        for k in "LHV":
            bg = np.where(mean[k] > bg, mean[k], bg)
        e = np.where(nan, np.nan, mean["P"] - bg).astype(np.float32)
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


def epistasis_items(sets):
    """What `epistasis_1m` screens for a list of `EditSet`s (a bare `Edit` counts as a one-member set): ``(singles, member_off, members)``.
    ``singles``: the distinct members of all sets as `Edit`s, in order of first appearance - two `Edit`s are the same when kind, pos, length and
    the bytes of seq agree.  Set e has members ``singles[members[m]]`` for m in [member_off[e], member_off[e + 1]), in the set's own sorted
    order: ``member_off`` np.int64 [E + 1], ``members`` np.int32 [P] - the member table of orca_screen_epistasis_scores.  A ``del`` or ``ins``
    member is a ValueError: behind a displacement "bin with bin" additivity is not defined."""
    singles, index, off, members = [], {}, [0], []
    for item in sets:
        for e in members_of(item):
            if e.kind in LEN_KINDS:
                raise ValueError(f"epistasis: {e!r} changes the length; the sum of the members' effects is defined for length-preserving members only")
            key = (e.kind, e.pos, e.length, None if e.seq is None else e.seq.tobytes())
            if key not in index:
                index[key] = len(singles)
                singles.append(e)
            members.append(index[key])
        off.append(len(members))
    return singles, np.array(off, dtype=np.int64), np.array(members, dtype=np.int32)


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
    return _run_screen(model, window, edits, batch, keep_maps, stats, regions, flank, aligned, flank_bp, strands, insulation, viewpoints, strata=strata, loops=loops,
                       boundaries=boundaries)


def _run_screen(model, window, edits, batch, keep_maps, stats, regions, flank, aligned, flank_bp, strands, insulation, viewpoints, hook=None, strata=None,
                loops=None, boundaries=None):
    """The body of `screen_1m` (its arguments, its result).  ``hook``: called as ``hook(res, i0, i1, maps)`` at the end of every batch, on every
    route, with the `ScreenResult` under construction (``res.ref_map`` is final) and the FINAL maps [i1 - i0, n, n] of items [i0, i1) - after the
    strand merge and after any range fallback; the buffer is the batch's own, so the hook reads it before it returns.  Without a hook nothing
    is launched that `screen_1m` did not launch."""
    if strands not in ("+", "both"):
        raise ValueError(f"strands must be '+' or 'both', got {strands!r}")
    if boundaries is not None and boundaries is not False and insulation is None:
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
    rects = None if regions is None else check_regions(regions, win.numel() // 4000)
    widths = None if insulation is None else check_insulation(insulation, win.numel() // 4000)
    views = None if viewpoints is None else check_viewpoints(viewpoints, win.numel() // 4000)
    drange = None if strata is None or strata is False else check_strata(strata, win.numel() // 4000)
    lp = None if loops is None or loops is False else check_loops(loops, win.numel() // 4000)
    bp = None if boundaries is None or boundaries is False else check_boundaries(boundaries, win.numel() // 4000)
    st = {"route": None, "two_part_batches": 0, "whole_window_batches": 0, "range_fallback_batches": 0, "range_fallback_reference": False,
          "front_runs": 0, "front_bases": 0, "edits": len(edits), "set_items": sum(isinstance(e, EditSet) for e in edits), "segments": 0,
          "indel_items": sum(changes_length(e) for e in edits), "take_rows": 0, "cache_phases": 0, "aligned_items": 0,
          "strands": strands, "reverse_two_part_items": 0, "reverse_whole_items": 0,
          "insulation_widths": 0 if widths is None else len(widths), "viewpoints": 0 if views is None else len(views),
          "strata": 0 if drange is None else drange[1] - drange[0], "loops": 0 if lp is None else lp.max_calls, "loop_truncated_items": 0,
          "boundaries": 0 if bp is None else bp.max_calls}
    fl = _flank_codes(window, flank, win, flank_bp) if (flank is not None or st["indel_items"]) else None
    sc = _Screen(net, win, st, fl if st["indel_items"] else None)
    E, n, dev = len(edits), sc.n, sc.dev
    two_part = net._enc.two_part_ok()
    plans = {}
    with torch.no_grad():
        s5_ref = s5_ref_minus = ref_minus = None
        if two_part:
            with engine.defer_overflow_guard():
                s5_ref = sc.reference_rows()
                enc_ref = torch.empty((1, 128, n), dtype=torch.float32, device=dev)
                net._enc.back5(s5_ref, enc_ref[0])
                ref_map, ref_1d = sc._decode(enc_ref)
                if both:                                 # the '-' strand's reference, under the same range check
                    s5_ref_minus = sc.reference_rows(True)
                    enc_minus = torch.empty((1, 128, n), dtype=torch.float32, device=dev)
                    net._enc.back5(s5_ref_minus, enc_minus[0])
                    ref_minus = sc._decode(enc_minus)
                if st["indel_items"]:                    # the cache entries the batches will pool from, under the reference's range check
                    for i0 in range(0, E, batch):        # every indel batch is planned once, here; the phases built are the phases used
                        if any(changes_length(e) for e in edits[i0: i0 + batch]):
                            plans[i0] = plan_batch(edits[i0: i0 + batch], sc.L, flank=sc.F, both_strands=both)
                    phases = sorted({ph for p in plans.values() for ph in p.phases})
                    sc.build_entries(phases)
                    if both:
                        sc.build_entries(mirror_phases(phases, sc.L + sc.F), "-")
            if sc.ctx.take_overflow():
                two_part = False
                st["range_fallback_reference"] = True
        if not two_part and not st["range_fallback_reference"]:
            ref_map, ref_1d = sc.whole([])
            ref_minus = sc.whole([], reverse=True) if both else None
        elif st["range_fallback_reference"]:
            with engine.force_safe_precision():
                ref_map, ref_1d = sc.whole([])
                ref_minus = sc.whole([], reverse=True) if both else None
        st["route"] = "two_part" if two_part else "whole_window"
        ref_map = ref_map[0].contiguous()
        ref_1d = None if ref_1d is None else ref_1d[0].contiguous()
        ref_gap = ref_plus = None
        if both:                                         # the reference merged as every batch will be; zero "references" make the gap mean |ref+ - flip(ref-)|
            ref_plus, ref_minus, ref_1d_minus = ref_map, ref_minus[0][0].contiguous(), ref_minus[1]
            zero = torch.zeros_like(ref_plus)
            merged, ref_gap = engine.screen_merge_strands(sc.ctx, ref_plus[None], ref_minus[None], zero, zero)
            ref_map = merged[0]
            if ref_1d is not None:
                ref_1d = 0.5 * ref_1d + 0.5 * ref_1d_minus[0].flip(-1)
        res = ScreenResult(ref_map, ref_1d, torch.zeros((E, n), dtype=torch.float32, device=dev), torch.zeros(E, dtype=torch.float32, device=dev),
                           torch.zeros(E, dtype=torch.float32, device=dev),
                           torch.zeros((E, sc.num_1d, n), dtype=torch.float32, device=dev) if sc.num_1d else None,
                           torch.zeros((E, n, n), dtype=torch.float32, device=dev) if keep_maps else None, edits)
        if both:
            res.ref_strand_gap = ref_gap[0]
            res.strand_gap = torch.zeros(E, dtype=torch.float32, device=dev)
        res.shift = torch.tensor([shift_of(e) for e in edits], dtype=torch.int64, device=dev)
        if rects is not None:
            res.delta_region = torch.zeros((E, len(rects)), dtype=torch.float32, device=dev)
            res.delta_region_abs = torch.zeros((E, len(rects)), dtype=torch.float32, device=dev)
        bmaps = None
        if aligned:
            bmaps = np.stack([bin_map(e, sc.L, sc.F) for e in edits]) if E else np.zeros((0, n), dtype=np.int32)
            st["aligned_items"] = int((bmaps != np.arange(n, dtype=np.int32)[None]).any(axis=1).sum())
            res.bin_map = sc._upload(bmaps, torch.int32)
            res.aligned_bins = sc._upload((bmaps >= 0).sum(axis=1), torch.int64)
            res.aligned_profile = torch.zeros((E, n), dtype=torch.float32, device=dev)
            res.aligned_abs_mean = torch.zeros(E, dtype=torch.float32, device=dev)
            res.aligned_abs_max = torch.zeros(E, dtype=torch.float32, device=dev)
            if rects is not None:
                res.aligned_region = torch.zeros((E, len(rects)), dtype=torch.float32, device=dev)
                res.aligned_region_abs = torch.zeros((E, len(rects)), dtype=torch.float32, device=dev)
        if widths is not None:                           # the reference's own track once, from the final (merged) reference map
            res.insulation_widths = sc._upload(widths, torch.int32)
            res.ref_insulation = engine.screen_insulation(sc.ctx, ref_map[None], None, widths)[0][0]
            res.insulation = torch.zeros((E, len(widths), n), dtype=torch.float32, device=dev)
            res.delta_insulation = torch.zeros((E, len(widths), n), dtype=torch.float32, device=dev)
            if aligned:
                res.aligned_insulation = torch.zeros((E, len(widths), n), dtype=torch.float32, device=dev)
            if bp is not None:                           # the reference's boundaries once, from its own tracks
                got = engine.screen_boundary_calls(sc.ctx, res.ref_insulation[None], bp.min_strength, bp.max_calls, strength_track=False)
                res.boundary_params = bp
                res.ref_boundaries, res.ref_boundary_strength, res.ref_boundary_count = got["bins"][0], got["strength"][0], got["count"][0]
                res.boundaries = torch.full((E, len(widths), bp.max_calls), -1, dtype=torch.int32, device=dev)
                res.boundary_strength = torch.full((E, len(widths), bp.max_calls), float("nan"), dtype=torch.float32, device=dev)
                res.boundary_count = torch.zeros((E, len(widths)), dtype=torch.int32, device=dev)
        if views is not None:
            res.viewpoint_bins = sc._upload(views, torch.int32)
            res.delta_viewpoint = torch.zeros((E, len(views), n), dtype=torch.float32, device=dev)
            if aligned:
                res.aligned_viewpoint = torch.zeros((E, len(views), n), dtype=torch.float32, device=dev)
        if drange is not None:
            res.strata_range = drange
            for pre in ("", "aligned_") if aligned else ("",):
                for name in STRATA_FIELDS:
                    setattr(res, pre + name, torch.zeros((E, n) if name.startswith("dist_") else (E,), device=dev,
                                                         dtype=torch.float64 if name in ("dist_corr", "corr", "scc") else torch.float32))
            if aligned:
                res.aligned_dist_count = torch.zeros((E, n), dtype=torch.int32, device=dev)
        ref_ij = ref_pix = followed = None
        if lp is not None:                               # the reference's dots once, from the final (merged) reference map
            got = engine.screen_dot_calls(sc.ctx, ref_map[None], lp.p, lp.w, lp.r, lp.threshold, lp.max_calls, lp.d_min)
            res.loop_params, res.ref_loop_count = lp, int(got["count"][0])
            R, K = min(res.ref_loop_count, lp.max_calls), lp.max_calls
            res.ref_loops, res.ref_loop_enrichment = got["ij"][0, :R].contiguous(), got["enrich"][0, :R].contiguous()
            ref_ij = res.ref_loops.cpu().numpy()
            ref_pix = res.ref_loops.long()
            res.loops = torch.full((E, K, 2), -1, dtype=torch.int32, device=dev)
            res.loop_enrichment = torch.full((E, K), float("nan"), dtype=torch.float32, device=dev)
            res.loop_count = torch.zeros(E, dtype=torch.int32, device=dev)
            res.loop_delta = torch.zeros((E, R), dtype=torch.float32, device=dev)
            if aligned:                                  # every reference dot followed to its alt pixel, per item: (-1, -1) where it has none
                res.aligned_loop_delta = torch.full((E, R), float("nan"), dtype=torch.float32, device=dev)
                followed = _follow_loops(bmaps, ref_ij, lp)
        def whole(chunk):                                # a batch on the whole-window route: the '+' strand, or the pair of strands
            if not both:
                return sc.whole(chunk)
            st["reverse_whole_items"] += len(chunk)
            return sc.whole(chunk), sc.whole(chunk, reverse=True)
        for i0 in range(0, E, batch):
            chunk = edits[i0: i0 + batch]
            if two_part:
                with engine.defer_overflow_guard():      # one check for both strands of the batch
                    out = sc.two_part(chunk, s5_ref, plans.get(i0), s5_ref_minus)
                if sc.ctx.take_overflow():
                    st["range_fallback_batches"] += 1
                    with engine.force_safe_precision():
                        out = whole(chunk)
                else:
                    st["two_part_batches"] += 1
                    if both:
                        st["reverse_two_part_items"] += len(chunk)
            elif st["range_fallback_reference"]:
                st["range_fallback_batches"] += 1
                with engine.force_safe_precision():
                    out = whole(chunk)
            else:
                st["whole_window_batches"] += 1
                out = whole(chunk)
            i1 = i0 + len(chunk)
            if both:
                (maps, h), (maps_minus, h_minus) = out
                maps, res.strand_gap[i0:i1] = engine.screen_merge_strands(sc.ctx, maps, maps_minus, ref_plus, ref_minus, out=maps)
                if h is not None:
                    h = 0.5 * h + 0.5 * h_minus.flip(-1)
            else:
                maps, h = out
            prof, mean, amax = engine.screen_scores(sc.ctx, maps, ref_map)
            res.delta_profile[i0:i1] = prof
            res.delta_abs_mean[i0:i1] = mean
            res.delta_abs_max[i0:i1] = amax
            if rects is not None:
                res.delta_region[i0:i1], res.delta_region_abs[i0:i1] = engine.screen_region_scores(sc.ctx, maps, ref_map, rects)
            if aligned:
                res.aligned_profile[i0:i1], res.aligned_abs_mean[i0:i1], res.aligned_abs_max[i0:i1] = engine.screen_aligned_scores(
                    sc.ctx, maps, ref_map, bmaps[i0:i1], res.bin_map[i0:i1])
                if rects is not None:
                    res.aligned_region[i0:i1], res.aligned_region_abs[i0:i1] = engine.screen_aligned_region_scores(
                        sc.ctx, maps, ref_map, bmaps[i0:i1], rects, res.bin_map[i0:i1])
            if widths is not None:
                tr, dl, al = engine.screen_insulation(sc.ctx, maps, ref_map, widths, bmaps[i0:i1] if aligned else None, res.bin_map[i0:i1] if aligned else None)
                res.insulation[i0:i1], res.delta_insulation[i0:i1] = tr, dl
                if aligned:
                    res.aligned_insulation[i0:i1] = al
                if bp is not None:
                    got = engine.screen_boundary_calls(sc.ctx, tr, bp.min_strength, bp.max_calls, strength_track=False)
                    res.boundaries[i0:i1], res.boundary_strength[i0:i1], res.boundary_count[i0:i1] = got["bins"], got["strength"], got["count"]
            if views is not None:
                dl, al = engine.screen_viewpoints(sc.ctx, maps, ref_map, views, bmaps[i0:i1] if aligned else None, res.bin_map[i0:i1] if aligned else None)
                res.delta_viewpoint[i0:i1] = dl
                if aligned:
                    res.aligned_viewpoint[i0:i1] = al
            if drange is not None:
                got = engine.screen_strata_scores(sc.ctx, maps, ref_map, None, drange)
                for name in STRATA_FIELDS:
                    getattr(res, name)[i0:i1] = got[name]
                if aligned:
                    got = engine.screen_strata_scores(sc.ctx, maps, ref_map, bmaps[i0:i1], drange, res.bin_map[i0:i1])
                    for name in STRATA_FIELDS + ("dist_count",):
                        getattr(res, "aligned_" + name)[i0:i1] = got[name]
            if lp is not None:
                got = engine.screen_dot_calls(sc.ctx, maps, lp.p, lp.w, lp.r, lp.threshold, lp.max_calls, lp.d_min)
                res.loops[i0:i1], res.loop_enrichment[i0:i1], res.loop_count[i0:i1] = got["ij"], got["enrich"], got["count"]
                if ref_pix.shape[0]:
                    res.loop_delta[i0:i1] = got["e_map"][:, ref_pix[:, 0], ref_pix[:, 1]] - res.ref_loop_enrichment[None]
                    if aligned:
                        res.aligned_loop_delta[i0:i1] = engine.screen_dot_enrichment(sc.ctx, maps, followed[i0:i1], lp.p, lp.w, lp.d_min) - res.ref_loop_enrichment[None]
            if h is not None:
                torch.sub(h, ref_1d[None], out=res.delta_1d[i0:i1])
            if keep_maps:
                res.maps[i0:i1] = maps
            if hook is not None:
                hook(res, i0, i1, maps)
        if lp is not None:                               # the lists are tiny: one copy to the host, the matching in numpy
            alt_ij = res.loops.cpu().numpy()
            st["loop_truncated_items"] = int((res.loop_count > lp.max_calls).sum())
            for pre in ("", "aligned_") if aligned else ("",):
                if not pre:
                    gained, lost = _match_loops(alt_ij, ref_ij, lp.tol)
                else:                                    # an identity bin map changes nothing: only the other items are matched again
                    moved = np.flatnonzero((bmaps != np.arange(n, dtype=np.int32)[None]).any(axis=1))
                    gained, lost = gained.copy(), lost.copy()
                    gained[moved], lost[moved] = _match_loops(alt_ij[moved], ref_ij, lp.tol, bmaps[moved])
                setattr(res, pre + "loop_is_gained", sc._upload(gained, torch.bool))
                setattr(res, pre + "ref_loop_is_lost", sc._upload(lost, torch.bool))
                setattr(res, pre + "loops_gained", sc._upload(gained.sum(axis=1), torch.int32))
                setattr(res, pre + "loops_lost", sc._upload(lost.sum(axis=1), torch.int32))
        if bp is not None:                               # the lists and the tracks' NaN pattern on the host, the matching in numpy
            _screen_boundaries(res, sc, bp, bmaps if aligned else None)
    if stats is not None:
        stats.update(st)
    return res


def _screen_boundaries(res, sc, bp, bmaps):
    """The matched boundary fields of a finished `ScreenResult` (`BOUNDARY_MATCH_FIELDS`, and their ``aligned_`` forms with the items' bin maps
    ``bmaps`` [E, n]): `_boundary_fields` on the lists and tracks copied to the host once; ``boundary_delta`` is gathered on the device."""
    E, W, n = res.insulation.shape
    K = bp.max_calls
    host = lambda t: t.cpu().numpy().reshape((E * W,) + tuple(t.shape[2:]))
    alt = {"bins": host(res.boundaries), "strength": host(res.boundary_strength)}
    ref = {k: np.ascontiguousarray(np.broadcast_to(v.cpu().numpy(), (E, W, K))).reshape(E * W, K)
           for k, v in (("bins", res.ref_boundaries), ("strength", res.ref_boundary_strength))}
    ta, tr = host(res.insulation), np.ascontiguousarray(np.broadcast_to(res.ref_insulation.cpu().numpy(), (E, W, n))).reshape(E * W, n)
    nan = torch.full((), float("nan"), dtype=torch.float32, device=sc.dev)
    got = None
    for pre in ("", "aligned_") if bmaps is not None else ("",):
        if not pre:
            got = _boundary_fields(alt, ref, ta, tr, bp.tol)
        else:                                            # an identity bin map changes nothing: only the other items are matched again
            moved = np.flatnonzero(np.repeat((bmaps != np.arange(n, dtype=np.int32)[None]).any(axis=1), W))
            got = {k: v.copy() for k, v in got.items()}
            if moved.size:
                sub = lambda d: {k: v[moved] for k, v in d.items()}
                for k, v in _boundary_fields(sub(alt), sub(ref), ta[moved], tr[moved], bp.tol, np.repeat(bmaps, W, axis=0)[moved]).items():
                    got[k][moved] = v
        for k, v in got.items():
            if k != "first_at":
                setattr(res, pre + k, sc._upload(v.reshape((E, W) + v.shape[1:]), {"b": torch.bool, "i": torch.int32, "f": torch.float32}[v.dtype.kind]))
        at_dev = sc._upload(got["first_at"].reshape(E, W, K), torch.int64)
        src = res.aligned_insulation if pre else res.delta_insulation
        setattr(res, pre + "boundary_delta", torch.where(at_dev >= 0, torch.gather(src, 2, at_dev.clamp(min=0)), nan))


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
    U, E, n, dev = len(singles), len(sets), win.numel() // 4000, win.device
    need = U * n * n * 4
    if need > bank_bytes:
        raise ValueError(f"epistasis_1m: the bank of {U} single-edit maps takes {need} bytes, above bank_bytes = {bank_bytes}: split the set list")
    rects = None if regions is None else check_regions(regions, n)
    ctx = engine.get_context(dev)
    bank = torch.empty((U, n, n), dtype=torch.float32, device=dev)
    out = EpistasisResult(None, singles, U, member_off, members, torch.zeros((E, n), dtype=torch.float32, device=dev),
                          *(torch.zeros(E, dtype=torch.float32, device=dev) for _ in range(3)))
    if rects is not None:
        out.epi_region, out.epi_region_abs = (torch.zeros((E, len(rects)), dtype=torch.float32, device=dev) for _ in range(2))

    def score(res, i0, i1, maps):
        if i0 < U:                                       # the batch's singles into the bank, before its sets are scored
            bank[i0: min(i1, U)] = maps[: min(i1, U) - i0]
        if i1 <= U:
            return
        s0 = max(i0, U)
        e0, e1 = s0 - U, i1 - U
        off = member_off[e0: e1 + 1] - member_off[e0]
        got = engine.screen_epistasis_scores(ctx, maps[s0 - i0:], bank, res.ref_map, off, members[member_off[e0]: member_off[e1]], rects)
        out.epi_profile[e0:e1], out.epi_abs_mean[e0:e1], out.epi_abs_max[e0:e1], out.additive_abs_mean[e0:e1] = got[:4]
        if rects is not None:
            out.epi_region[e0:e1], out.epi_region_abs[e0:e1] = got[4:]
    st = {}
    out.screen = _run_screen(model, win, singles + sets, batch, keep_maps, st, rects, None, False, None, strands, None, None, hook=score)
    st.update(epistasis_sets=E, epistasis_singles=U, bank_bytes=need)
    if stats is not None:
        stats.update(st)
    return out
