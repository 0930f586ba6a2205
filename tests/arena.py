"""The workspace arena as a test input (`engine.Context.fill_workspace`, orca_ctx_fill_workspace): every call of the library works inside one
per-context arena that is reused, grown and never cleared, plus four edge-fix scratch slabs.  The contract: no call reads arena or scratch bytes
it has not written in the same call, every output is written in full, and the fp16-range flag does not depend on what was there before.  So the
same call on an arena filled with different bytes gives the same bits and the same flag.

FILLS, and what each byte reads as (pinned by tests/test_arena_cpu.py):
  0x00  zero in every format: what a fresh allocation usually holds - the baseline
  0xFF  NaN as fp32, as both fp16 halves of a P16 unit and as bf16; -1 / 255 as an integer or a base code
  0x3C  0.011489 as fp32, 1.059 per fp16 half, 0.011475 as bf16: `fmaxf` drops a NaN, so a NaN read in front of a ReLU or a max-pool vanishes
        where 1.059 in a zero pad does not; far inside the fp16 range, so it cannot raise the range flag legitimately
  0x7B  61 280 per fp16 half (the largest byte pattern that is finite there), 1.3e36 as fp32 and as bf16: the range guards take their maximum
        with `fmaxf` too, so NaN never raises the flag and 1.059 cannot - a guard that sees lanes fed from the arena shows under this fill"""
import contextlib

import numpy as np
import torch

FILLS = (0x00, 0xFF, 0x3C, 0x7B)
EDGE_BYTES = 4 * 40 * 128 * 4          # orca_ctx::d_edge: four scratch slabs of 40 x 128 floats


@contextlib.contextmanager
def nan_outputs():
    """While active, every floating-point ROCm tensor from `torch.empty` / `torch.empty_like` starts as NaN: the engine wrappers allocate their
    outputs that way, and torch's allocator would otherwise hand back the block that still holds the previous run's result - an element the
    library does not write would then look written."""
    real_empty, real_like = torch.empty, torch.empty_like

    def poisoned(t):
        if t.is_cuda and t.is_floating_point():
            t.fill_(float("nan"))
        return t

    torch.empty = lambda *a, **k: poisoned(real_empty(*a, **k))
    torch.empty_like = lambda *a, **k: poisoned(real_like(*a, **k))
    try:
        yield
    finally:
        torch.empty, torch.empty_like = real_empty, real_like


def as_bits(out):
    """A tensor / numpy array or a (nested) list / tuple of them -> one flat int32 array of their bits (None entries are skipped)."""
    parts = []

    def walk(o):
        if o is None:
            return
        if isinstance(o, (list, tuple)):
            for v in o:
                walk(v)
            return
        a = o.detach().cpu().contiguous().numpy() if isinstance(o, torch.Tensor) else np.ascontiguousarray(o)
        if a.dtype.itemsize % 4:
            a = a.astype(np.int32)
        parts.append(a.reshape(-1).view(np.int32))

    walk(out)
    assert parts, "the call returned no output"
    return np.concatenate(parts)


def bits_on_fills(ctx, fn, fills=None):
    """``fn()`` once to size the arena of ``ctx`` (result discarded), then once per fill byte on the arena and edge scratch filled with it ->
    [(bits as int32, range flag)].  fn returns its output(s); outputs it owns it prefills itself (NaN, or a sentinel where the call writes a
    part only), the ones the engine wrappers allocate are NaN through `nan_outputs`."""
    fills = FILLS if fills is None else fills
    with nan_outputs():
        fn()
    torch.cuda.synchronize()
    res = []
    for byte in fills:
        ctx.take_overflow()
        size = ctx.workspace_bytes()
        filled = ctx.fill_workspace(byte)
        assert size > 0 and filled == size + EDGE_BYTES, (byte, size, filled)
        with nan_outputs():
            out = fn()
        torch.cuda.synchronize()
        flag = ctx.take_overflow()
        assert ctx.workspace_bytes() == size, (byte, "the arena was regrown: the fill is gone")
        res.append((as_bits(out), flag))
    return res


def assert_arena_independent(ctx, fn, fills=None, finite=True, what=""):
    """The result under 0x00 is finite everywhere (``finite=False``: outputs that hold NaN by design or are no fp32 - then only the bits are
    compared), every fill gives the bits of 0x00, no fill raises the range flag.  -> the bits."""
    fills = FILLS if fills is None else fills
    assert fills[0] == 0x00
    res = bits_on_fills(ctx, fn, fills)
    base, _ = res[0]
    if finite:
        assert np.isfinite(base.view(np.float32)).all(), (what, "not finite on a zeroed arena", int((~np.isfinite(base.view(np.float32))).sum()))
    for byte, (bits, flag) in zip(fills, res):
        assert not flag, (what, f"fill 0x{byte:02X} raised the fp16-range flag")
        differ = bits != base
        assert not differ.any(), (what, f"fill 0x{byte:02X}: {int(differ.sum())} of {bits.size} words differ, first at {int(np.argmax(differ))}")
    return base
