"""The edits of the 1 Mb screen and the plans of its two-part route (`screen` says what they are for, and re-exports every name).

`Edit`, `EditSet` and the generators; `apply_edit`, the host restatement of the edited window; `bin_map`, the reference bin behind every alt
bin; `plan_batch` / `mirror_plan` and the tables of the whole-window route, which tests/test_screen_cpu.py checks against the fp64 oracle;
`epistasis_items`, the member table of an epistasis screen.  All of it is host work: it fills the tables the kernels read and launches nothing.
"""
from dataclasses import dataclass, replace
from typing import Optional

import numpy as np
import torch

from . import engine, sv
from .map_readouts import BIN_BP

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
