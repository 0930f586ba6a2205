"""The three table formats of the screen's edited bases and of its row images against each other and against numpy, kernel by kernel, on hand-built
tables (not `plan_batch`'s): one batch stated as the single-span table, as snippet + span tables and as snippet + piece tables gives the same bytes
from orca_screen_edit_codes, _edit_codes_multi and _assemble_codes; one set of row segments gives the same bits from orca_screen_splice_rows,
_splice_rows_multi and _gather_rows.  The kernels share their bodies (orca_amd/csrc/screen.h); a format's adapter is where a mistake would sit."""
import numpy as np
import pytest
import torch

from orca_amd import engine
from orca_amd import screen as S

pytestmark = pytest.mark.gpu

L = 4_000
# (snippet [b0, b1), its bare edit): a sub that starts at base 0; an inv that starts before its snippet and ends inside it; a mask that runs to the
# window's last base; a 1-base sub on its snippet's last base
CASES = [((0, 1_500), ("sub", 0, 7)), ((1_200, 2_600), ("inv", 1_100, 300)), ((3_000, 4_000), ("mask", 3_900, 100)), ((2_000, 2_800), ("sub", 2_799, 1))]


def _window(rs):
    c = rs.randint(0, 4, L).astype(np.uint8)
    for a, b in ((0, 3), (1_150, 1_230), (1_390, 1_405), (2_795, 2_800), (3_950, 3_960)):       # N runs across the edits' and the snippets' ends
        c[a:b] = 4
    return c


def _code_case():
    """(window, the expected bytes, single-span table, snippet + span tables, snippet + piece tables, payload) of CASES"""
    rs = np.random.RandomState(11)
    c = _window(rs)
    edits = [S.Edit(k, p, n, rs.randint(0, 5, n).astype(np.uint8)) if k == "sub" else S.Edit(k, p, n) for _, (k, p, n) in CASES]
    snips = [s for s, _ in CASES]
    off = np.concatenate([[0], np.cumsum([b1 - b0 for b0, b1 in snips])])
    want = np.concatenate([S.apply_edit(c, e)[b0:b1] for e, (b0, b1) in zip(edits, snips)])
    assert want.size == off[-1] == 4_700 and not np.array_equal(want, np.concatenate([c[b0:b1] for b0, b1 in snips]))

    single = np.zeros((len(edits), engine.SCREEN_EDIT_FIELDS), dtype=np.int64)
    table = np.zeros_like(single)                                       # one span per snippet
    spans = np.zeros((len(edits), engine.SCREEN_SPAN_FIELDS), dtype=np.int64)
    ptable, pieces, payload, npay = np.zeros_like(single), [], [], 0
    for i, (e, (b0, b1)) in enumerate(zip(edits, snips)):
        spans[i] = (engine.SCREEN_KINDS[e.kind], e.pos, e.length, npay if e.kind == "sub" else 0)
        single[i, :7] = (off[i], b0, b1 - b0, *spans[i])
        table[i, :5] = (off[i], b0, b1 - b0, i, 1)
        pcs, py = S.item_pieces(e, L, 0, npay)                          # the item's whole alt window; the snippet takes the pieces that meet it
        lo, cnt = S._pieces_meeting(np.array(pcs, dtype=np.int64), 0, len(pcs), b0, b1)
        ptable[i, :5] = (off[i], b0, b1 - b0, len(pieces) + lo, cnt)
        pieces += pcs
        payload.append(py)
        npay += py.size
    pieces = np.array(pieces, dtype=np.int64)
    assert {int(k) for k in pieces[:, 1]} == {0, 1, 2, 3}                 # every piece kind takes part
    return c, want, single, table, spans, ptable, pieces, np.concatenate(payload)


def test_three_code_formats_give_the_same_bytes(cuda):
    c, want, single, table, spans, ptable, pieces, payload = _code_case()
    ctx = engine.get_context(cuda)
    win, pay = torch.from_numpy(c).to(cuda), torch.from_numpy(payload).to(cuda)
    outs = [torch.full((want.size,), 9, dtype=torch.uint8, device=cuda) for _ in range(3)]
    engine.screen_edit_codes(ctx, win, single, torch.from_numpy(single).to(cuda), pay, outs[0])
    engine.screen_edit_codes_multi(ctx, win, table, spans, pay, outs[1])
    engine.screen_assemble_codes(ctx, win, ptable, pieces, pay, outs[2])
    for name, out in zip(("edit_codes", "edit_codes_multi", "assemble_codes"), outs):
        assert np.array_equal(out.cpu().numpy(), want), name


def _row_case(n5=10, nfresh=7, B=3):
    """(ref rows, fresh rows, the B segments, their offsets, the same as gather segments, the expected images)"""
    rs = np.random.RandomState(12)
    ref, fresh = rs.randn(n5, 128).astype(np.float32), rs.randn(nfresh, 128).astype(np.float32)
    ref[0, 5], ref[9, 127], ref[4, 0] = np.nan, -0.0, -0.0
    fresh[2, 0], fresh[6, 64], fresh[0, 3] = -0.0, np.nan, np.nan
    segs = np.array([[0, 3, 2], [7, 3, 4], [5, 1, 0]], dtype=np.int64)   # one that starts at row 0, one that ends at row n5, one of a single row
    want = np.repeat(ref[None], B, axis=0)
    for b, (r0, cnt, src) in enumerate(segs):
        want[b, r0: r0 + cnt] = fresh[src: src + cnt]
    seg_off = np.arange(B + 1, dtype=np.int64)
    gather = np.stack([segs[:, 0], segs[:, 1], np.full(B, engine.SCREEN_SRC_FRESH), segs[:, 2]], axis=1)
    return ref, fresh, segs, seg_off, gather, want


def test_three_row_formats_give_the_same_bits(cuda):
    ref, fresh, segs, seg_off, gather, want = _row_case()
    B, n5 = want.shape[:2]
    ctx = engine.get_context(cuda)
    r, f = torch.from_numpy(ref).to(cuda), torch.from_numpy(fresh).to(cuda)
    outs = [torch.full((B, n5, 128), 7.0, dtype=torch.float32, device=cuda) for _ in range(3)]
    engine.screen_splice_rows(ctx, r, f, torch.from_numpy(segs).to(cuda), outs[0])
    engine.screen_splice_rows_multi(ctx, r, f, segs, seg_off, outs[1])
    engine.screen_gather_rows(ctx, r, f, [], gather, seg_off, outs[2])
    bits = want.view(np.int32)
    assert np.isnan(want).sum() >= 3 and (bits == np.int32(-2 ** 31)).sum() >= 3          # the NaNs and the -0.0s are in the images
    for name, out in zip(("splice_rows", "splice_rows_multi", "gather_rows"), outs):
        assert np.array_equal(out.cpu().numpy().view(np.int32), bits), name
