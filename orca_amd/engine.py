"""Thin host layer over the C ABI: contexts, BatchNorm folding, net handles and
forward wrappers that take torch ROCm tensors purely as device containers
(``data_ptr()`` + strides).  No arithmetic on the data path happens in torch.
"""
import ctypes
import threading
import weakref

import numpy as np
import torch

from . import _lib
from ._lib import ConvDesc, OrcaHipError, check

BN_EPS = 1e-5  # nn.BatchNorm1d/2d default used throughout orca_modules.py


# ---------------------------------------------------------------------------
# contexts: one per (host thread, device)
# ---------------------------------------------------------------------------
_tls = threading.local()


class Context:
    def __init__(self, device_index):
        lib = _lib.load()
        self.device_index = device_index
        self.handle = ctypes.c_void_p()
        stream = torch.cuda.current_stream(device_index).cuda_stream
        check(lib.orca_ctx_create(device_index, ctypes.c_void_p(stream), ctypes.byref(self.handle)), "orca_ctx_create")
        self._finalizer = weakref.finalize(self, lib.orca_ctx_destroy, self.handle)

    def sync_stream(self):
        """Point the context at torch's current stream for this device."""
        stream = torch.cuda.current_stream(self.device_index).cuda_stream
        check(_lib.load().orca_ctx_set_stream(self.handle, ctypes.c_void_p(stream)), "orca_ctx_set_stream")

    def workspace_bytes(self):
        n = ctypes.c_size_t()
        check(_lib.load().orca_ctx_workspace_bytes(self.handle, ctypes.byref(n)))
        return n.value

    def take_overflow(self):
        """f16x2 mode: True if an activation left the fp16 range since the last call (syncs the stream)."""
        f = ctypes.c_int()
        check(_lib.load().orca_ctx_take_overflow(self.handle, ctypes.byref(f)), "orca_ctx_take_overflow")
        return bool(f.value)

    def set_timing(self, enable):
        check(_lib.load().orca_ctx_set_timing(self.handle, 1 if enable else 0))

    def get_timing(self, max_records=4096):
        """[(cout, cin, tile, batch, n, ms, ksize)] of the conv1d launches timed since the last call."""
        buf = (_lib.KernelTime * max_records)()
        n = ctypes.c_int()
        check(_lib.load().orca_ctx_get_timing(self.handle, buf, max_records, ctypes.byref(n)))
        return [(r.cout, r.cin, r.tile, r.batch, r.n, r.ms, r.ksize) for r in buf[: min(n.value, max_records)]]

    def launch_counts(self):
        """{"conv_small": n, "conv_bf16s": n, "planar": n, "decoder_pairs": n} launches on this context since it was created."""
        c = (ctypes.c_int64 * 4)()
        check(_lib.load().orca_ctx_launch_counts(self.handle, c), "orca_ctx_launch_counts")
        return dict(zip(("conv_small", "conv_bf16s", "planar", "decoder_pairs"), [int(x) for x in c]))

    def release_workspace(self):
        check(_lib.load().orca_ctx_release_workspace(self.handle))

    def fill_workspace(self, byte):
        """Test hook: set every byte of the arena and of the edge-fix scratch to ``byte`` (syncs) -> bytes filled."""
        n = ctypes.c_size_t()
        check(_lib.load().orca_ctx_fill_workspace(self.handle, int(byte) & 0xFF, ctypes.byref(n)), "orca_ctx_fill_workspace")
        return n.value


def get_context(device):
    if isinstance(device, torch.device):
        if device.type != "cuda":
            raise OrcaHipError(f"orca_amd runs on MI355X only; got a tensor on '{device}'. There is no CPU path.")
        idx = device.index if device.index is not None else torch.cuda.current_device()
    else:
        idx = int(device)
    ctx = getattr(_tls, "override", None)          # ContextPool.run: an auxiliary context is current on this thread
    if ctx is None or ctx.device_index != idx:
        ctxs = getattr(_tls, "ctxs", None)
        if ctxs is None:
            ctxs = _tls.ctxs = {}
        if idx not in ctxs:
            ctxs[idx] = Context(idx)
        ctx = ctxs[idx]
    ctx.sync_stream()
    return ctx


# ---------------------------------------------------------------------------
# fp16-range guard policy (see orca_modules._HipModule._run_guarded)
#   immediate (default): every module forward in "f16x2" checks the device flag right away (one stream sync)
#   deferred: a caller that runs a whole cascade checks ONCE at the end and reruns it under force_safe()
# ---------------------------------------------------------------------------
import contextlib


class _GuardState(threading.local):
    """Per-THREAD policy (contexts, streams and overflow flags are per thread too, see _tls): one thread's deferred scope
    must not switch off another thread's immediate checks."""
    defer = False
    force_safe = False

    def __getitem__(self, key):      # dict-style access kept for the modules
        return getattr(self, key)

    def __setitem__(self, key, value):
        setattr(self, key, value)


_guard = _GuardState()


@contextlib.contextmanager
def _guard_scope(key, value):
    old = _guard[key]
    _guard[key] = value
    try:
        yield
    finally:
        _guard[key] = old


def defer_overflow_guard():
    return _guard_scope("defer", True)


def immediate_overflow_guard():
    """Inside a deferred scope: check (and retry) right away again.  Used around rank-LOCAL work that is followed by a
    collective (dist.ShardedEncoder): a retry decided after the collective would re-enter it on one rank only."""
    return _guard_scope("defer", False)


def force_safe_precision():
    return _guard_scope("force_safe", True)


class ContextPool:
    """K auxiliary contexts on one device, each with its own HIP stream, workspace arena, edge-fix scratch, fp16-range flag and weight
    upload (a context's arena is reused by every call, so calls that are to overlap need a context each) - for INDEPENDENT short calls
    whose launches fill a fraction of the chip each: the local re-encodes of an SV allele window (sv.encode_windows: 14 calls of ~50
    dependent launches, 0.65 ms of GPU time each in stream order against 0.15 ms of host time to issue one).  All issued from the
    CALLER's thread: run(i, fn) makes context i the thread's current context (get_context) and its stream torch's current stream while
    fn() runs.  fork() orders the pool's streams behind a stream of the caller's, host_join() marks the end of what has been issued,
    wait_join() orders a stream behind those marks (join() = both, now); `side` is one more stream of the caller's for preparation
    work.  (Worker THREADS per context were measured too: 42.0 against 40.6 ms per variant - the host is not the bound.)"""

    def __init__(self, device, k):
        self.index = device.index if isinstance(device, torch.device) and device.index is not None else torch.cuda.current_device()
        self.streams = [torch.cuda.Stream(device=self.index) for _ in range(k)]
        self.ctxs = []
        for s in self.streams:
            with torch.cuda.stream(s):
                self.ctxs.append(Context(self.index))
        self._fork = torch.cuda.Event()
        self._join = [torch.cuda.Event() for _ in range(k)]
        self.side = torch.cuda.Stream(device=self.index)     # a stream beside the caller's current one (preparation work)
        self._dirty = set()                                   # contexts that ran something since their range flag was last read

    def __len__(self):
        return len(self.ctxs)

    def fork(self, stream=None):
        """The pool's streams continue behind ``stream`` (default: the caller's current stream)."""
        self._fork.record(stream or torch.cuda.current_stream(self.index))
        for s in self.streams:
            s.wait_event(self._fork)

    def run(self, i, fn):
        i %= len(self.ctxs)
        self._dirty.add(i)
        prev = getattr(_tls, "override", None)
        _tls.override = self.ctxs[i]
        try:
            with torch.cuda.stream(self.streams[i]):
                return fn()
        finally:
            _tls.override = prev

    def host_join(self):
        """Mark the end of the work issued so far on the pool's streams (wait_join orders a stream behind those marks - now or later,
        e.g. after more work has been issued on it: sv.sv_screen issues a variant's local encodes under the previous variant's decoders)."""
        for s, ev in zip(self.streams, self._join):
            ev.record(s)

    def wait_join(self, stream=None):
        cur = stream or torch.cuda.current_stream(self.index)
        for ev in self._join:
            cur.wait_event(ev)

    def join(self):
        self.host_join()
        self.wait_join()

    def release_workspaces(self):
        """Free the contexts' workspace arenas (they grow again on demand): a whole-strand Encoder call leaves 25 GB in its context."""
        for c in self.ctxs:
            c.release_workspace()

    def take_overflow(self):
        """True if an activation left the fp16 range in a call run on one of the pool's contexts since the last check (reads - stream
        sync - and clears the flags of the contexts used since then)."""
        dirty, self._dirty = sorted(self._dirty), set()
        return any([self.ctxs[i].take_overflow() for i in dirty])      # a list: every flag is read (and cleared)


def _thread_pools():
    pools = getattr(_tls, "pools", None)
    if pools is None:
        pools = _tls.pools = {}
    return pools


def context_pool(device, k):
    """THE pool of k auxiliary contexts of a device FOR THE CALLING THREAD (made once per thread: modules cache a weight upload per
    context they ran on).  Per thread like every other context (`_tls.ctxs`): a pool's workspace arenas, edge scratch, streams, `_dirty`
    set and fork / join events belong to one chain of calls; two threads sharing them would overwrite each other's workspace and drain
    each other's fp16-range flags."""
    idx = device.index if isinstance(device, torch.device) and device.index is not None else torch.cuda.current_device()
    pools = _thread_pools()
    if (idx, k) not in pools:
        pools[(idx, k)] = ContextPool(torch.device("cuda", idx), k)
    return pools[(idx, k)]


def strand_streams():
    """$ORCA_STRAND_STREAMS=1: `genomepredict` / `cascade_32m` encode the reverse strand on an auxiliary context while the forward strand
    runs on the caller's stream.  The two Encoders' launches then share the chip (two persistent kernels side by side, each about twice as
    long): a first layer bound by HBM writes runs beside a conv bound by the matrix pipe, the small launches of stages 5-7 beside full ones -
    63.8 against 65.4 ms per step (same box, alternating).  Opt-in: a kernel's duration no longer says what the kernel can do (the bench's
    per-kernel roofline is defined on launches that have the chip to themselves), and the second context holds its own 25 GB workspace."""
    import os
    return os.environ.get("ORCA_STRAND_STREAMS", "0") == "1"


def batch_streams():
    """The bf16-plane Encoder (config 3's throughput mode) runs a batch of >= 2 sequences as two halves on two contexts / HIP streams
    (`orca_modules.Encoder.forward_codes`): stage 1's HBM-bound launch of one half beside the matrix-bound convs of the other - 74.7 -> 71.8 ms
    per 8 strands (tools/scratch measurement, late round 5), same bits.  $ORCA_BATCH_STREAMS=0: one context (a kernel's HIP-event time then
    measures the kernel, not its share of the chip - bench.py's config-3 roofline pass).  The fp32-class default arithmetic does not gain
    (197.3 -> 197.6 ms) and stays on one context."""
    import os
    return os.environ.get("ORCA_BATCH_STREAMS", "1") != "0"


def in_pool_run():
    """True while the calling thread is inside ContextPool.run (its current context is one of a pool's)."""
    return getattr(_tls, "override", None) is not None


def tentative(undo):
    """A result computed in the fp16-split arithmetic was just put where LATER calls will find it (a cached Encoder output, a
    chromosome encoding of the SV drivers' store) while the range check of the pass that produced it is still pending
    (`run_with_overflow_retry`: one check at the end of the chain).  ``undo()`` takes it out again; it runs if and only if that
    check fires, before the range-safe retry.  Outside such a pass (immediate checks: the module's own retry has already
    happened; the retry itself: range-safe arithmetic) nothing is registered."""
    lst = getattr(_tls, "tentative", None)
    if lst is not None and _guard.defer and not _guard.force_safe:
        lst.append(undo)


def run_with_overflow_retry(fn, device, pool=None):
    """Run fn() (a chain of module forwards on ``device``) with ONE fp16-range check at the end instead of one
    per module; if an activation left the fp16 range anywhere, redo the whole chain in the range-safe arithmetic.
    ``pool``: a ContextPool fn() also launched on (its contexts carry their own range flags).
    Whatever fn() cached for later calls on the way (`tentative`) is dropped first when the check fires."""
    if not (isinstance(device, torch.device) and device.type == "cuda"):
        return fn()
    ctx = get_context(device)
    outer, _tls.tentative = getattr(_tls, "tentative", None), []
    try:
        with defer_overflow_guard():
            out = fn()
        over = ctx.take_overflow()
        for p in ([pool] if pool is not None else []) + [q for q in _thread_pools().values() if q is not pool and q.index == ctx.device_index]:
            over = p.take_overflow() or over          # THIS thread's auxiliary contexts fn() ran on (e.g. the reverse strand's Encoder, strand_streams())
        if over:
            import warnings
            warnings.warn("orca_amd: an activation left the fp16 range; recomputing with range-safe arithmetic (bf16x3 / f32)")
            for undo in _tls.tentative:
                undo()
            _tls.tentative = []
            with force_safe_precision():
                out = fn()
    finally:
        _tls.tentative = outer
    return out


# ---------------------------------------------------------------------------
# BatchNorm folding (host, float64) - checkpoint format of orca_models.py:53-123
# ---------------------------------------------------------------------------
def _np64(v):
    if isinstance(v, torch.Tensor):
        return v.detach().cpu().double().numpy()
    return np.asarray(v, dtype=np.float64)


def fold_conv(sd, conv, bn=None, dilation=1):
    """(weight, bias[, BN running stats]) -> folded fp32 (w, b) + shape info.
    Eval-mode BN is the per-channel affine y = (x-mean)/sqrt(var+eps)*gamma+beta."""
    w = _np64(sd[conv + ".weight"])
    b = _np64(sd[conv + ".bias"])
    if bn is not None:
        s = _np64(sd[bn + ".weight"]) / np.sqrt(_np64(sd[bn + ".running_var"]) + BN_EPS)
        w = w * s.reshape((-1,) + (1,) * (w.ndim - 1))
        b = (b - _np64(sd[bn + ".running_mean"])) * s + _np64(sd[bn + ".bias"])
    return {"w": np.ascontiguousarray(w, dtype=np.float32), "b": np.ascontiguousarray(b, dtype=np.float32),
            "cout": w.shape[0], "cin": w.shape[1], "k": w.shape[2], "dil": int(dilation)}


def make_descs(convs):
    arr = (ConvDesc * len(convs))()
    for i, c in enumerate(convs):
        arr[i].weight_host = c["w"].ctypes.data
        arr[i].bias_host = c["b"].ctypes.data
        arr[i].cout, arr[i].cin, arr[i].ksize, arr[i].dilation = c["cout"], c["cin"], c["k"], c["dil"]
    return arr


class Net:
    """Device-resident weights of one reference module (orca_net)."""

    def __init__(self, ctx, kind, convs, upsample_mode=_lib.ORCA_UPSAMPLE_BILINEAR):
        lib = _lib.load()
        self.ctx, self.kind = ctx, kind
        self.precision = "f32"          # what orca_net_create leaves; `set_precision` keeps it current
        self.handle = ctypes.c_void_p()
        descs = make_descs(convs)  # `convs` keeps the numpy arrays alive during the call
        check(lib.orca_net_create(ctx.handle, kind, descs, len(convs), upsample_mode, ctypes.byref(self.handle)), "orca_net_create")
        self._finalizer = weakref.finalize(self, lib.orca_net_free, self.handle)

    def num_targets(self):
        """Maps per prediction of a Decoder / Decoder_1m net (num_2d); 1 for the other kinds."""
        if getattr(self, "_num_targets", None) is None:
            t = ctypes.c_int(0)
            check(_lib.load().orca_net_num_targets(self.handle, ctypes.byref(t)), "orca_net_num_targets")
            self._num_targets = int(t.value)
        return self._num_targets

    def set_precision(self, name):
        if name not in _lib.PRECISIONS:
            raise ValueError(f"precision must be one of {sorted(_lib.PRECISIONS)}, got {name!r}")
        check(_lib.load().orca_net_set_precision(self.handle, _lib.PRECISIONS[name]), "orca_net_set_precision")
        self.precision = name

    def set_encoder_form(self, name):
        """Encoder nets: force a less composed form of stage 1-3's linear groups (include/orca_hip.h: ORCA_ENCODER_FORM_*; the parity suite's handle)."""
        if name not in _lib.ENCODER_FORMS:
            raise ValueError(f"form must be one of {sorted(_lib.ENCODER_FORMS)}, got {name!r}")
        check(_lib.load().orca_net_set_encoder_form(self.handle, _lib.ENCODER_FORMS[name]), "orca_net_set_encoder_form")

    def set_decoder_block_runs(self, on):
        """Decoder nets, f16x2: run each dilation 16-32-64 block run as one launch (default) or block by block (bit-identical; conv2d_dblock.h)."""
        check(_lib.load().orca_net_set_decoder_block_runs(self.handle, 1 if on else 0), "orca_net_set_decoder_block_runs")

    def set_encoder_two_strands(self, on):
        """Encoder nets: `encoder_forward_two_strands` runs stages 3-7 of both strands as one joint pass (default) or as the two per-strand calls
        (bit-identical)."""
        check(_lib.load().orca_net_set_encoder_two_strands(self.handle, 1 if on else 0), "orca_net_set_encoder_two_strands")

    def encoder_two_strands(self):
        on = ctypes.c_int(0)
        check(_lib.load().orca_net_get_encoder_two_strands(self.handle, ctypes.byref(on)), "orca_net_get_encoder_two_strands")
        return bool(on.value)


# ---------------------------------------------------------------------------
# forward wrappers
# ---------------------------------------------------------------------------
def _f32_cuda(t, name):
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name} must be a torch.Tensor")
    if not t.is_cuda:
        raise OrcaHipError(f"{name} is on '{t.device}': orca_amd has no CPU path (move it to the MI355X with .cuda())")
    if t.dtype != torch.float32:
        t = t.float()
    return t


def _p(t):
    return ctypes.c_void_p(t.data_ptr())


def encoder_num_bins(L):
    return int(_lib.load().orca_encoder_num_bins(int(L)))


def encoder_forward(net, x, bin_lo=0, bin_hi=0, chunk_bp=0, out=None):
    x = _f32_cuda(x, "x")
    if x.dim() != 3 or x.shape[1] != 4:
        raise ValueError(f"Encoder input must be [B,4,L], got {tuple(x.shape)}")
    B, _, L = x.shape
    total = encoder_num_bins(L)
    hi = total if bin_hi <= 0 else bin_hi
    if out is None:
        out = torch.empty((B, 128, hi - bin_lo), dtype=torch.float32, device=x.device)
    net.ctx.sync_stream()
    check(_lib.load().orca_encoder_forward(net.ctx.handle, net.handle, _p(x), x.stride(0), x.stride(1), x.stride(2), B, L,
                                           bin_lo, hi, _p(out), out.stride(0), out.stride(1), chunk_bp), "orca_encoder_forward")
    return out


def pack_sequence(x):
    """x: [B,4,L] float ROCm tensor (any strides) -> (codes uint8 [B,L], packable).  ``packable`` is False if some
    row is neither one-hot nor the 0.25 'N' row; the codes are then meaningless and the float path must be used."""
    x = _f32_cuda(x, "x")
    B, C, L = x.shape
    if C != 4:
        raise ValueError(f"sequence must be [B,4,L], got {tuple(x.shape)}")
    codes = torch.empty((B, L), dtype=torch.uint8, device=x.device)
    ctx = get_context(x.device)
    ok = True
    for b in range(B):
        flag = ctypes.c_int()
        check(_lib.load().orca_pack_sequence(ctx.handle, ctypes.c_void_p(x[b].data_ptr()), x.stride(1), x.stride(2), L,
                                             ctypes.c_void_p(codes[b].data_ptr()), ctypes.byref(flag)), "orca_pack_sequence")
        ok = ok and bool(flag.value)
    return codes, ok


class CodeWindow:
    """A rank's share of a packed sequence: ``codes`` [B, n] = bases [origin, origin + n) of an L-base sequence (see
    `code_window_range` for what a bin range needs).  Accepted wherever the Encoder takes packed bases."""

    def __init__(self, codes, origin, L):
        self.codes, self.origin, self.L = codes, int(origin), int(L)

    @property
    def shape(self):
        return (self.codes.shape[0], self.L)

    device = property(lambda self: self.codes.device)
    dtype = property(lambda self: self.codes.dtype)


def code_window_range(L, bin_lo, bin_hi, reverse=False, halo=112000, binsize=4000):
    """[b0, b1): bases of the FORWARD sequence the Encoder reads for bins [bin_lo, bin_hi) of the forward strand / of the reverse
    complement (input halo of orca_modules.py:929-980 included; the last bin range runs to the end of the sequence)."""
    total = encoder_num_bins(L)
    lo = max(0, bin_lo * binsize - halo)
    hi = L if bin_hi >= total else min(L, bin_hi * binsize + halo)
    return (L - hi, L - lo) if reverse else (lo, hi)


def encoder_forward_codes(net, codes, reverse=False, bin_lo=0, bin_hi=0, chunk_bp=0, out=None):
    win = codes if isinstance(codes, CodeWindow) else None
    if win is not None:
        codes = win.codes
    if not (isinstance(codes, torch.Tensor) and codes.is_cuda and codes.dtype == torch.uint8 and codes.dim() == 2):
        raise ValueError("codes must be a [B,L] uint8 ROCm tensor")
    if codes.stride(1) != 1:
        codes = codes.contiguous()
    B, L = codes.shape
    if win is not None:
        L = win.L
    total = encoder_num_bins(L)
    hi = total if bin_hi <= 0 else bin_hi
    if out is None:
        out = torch.empty((B, 128, hi - bin_lo), dtype=torch.float32, device=codes.device)
    elif tuple(out.shape) != (B, 128, hi - bin_lo) or out.stride(2) != 1:
        raise ValueError(f"out must be a [{B},128,{hi - bin_lo}] view with unit stride along the bins")
    net.ctx.sync_stream()
    if win is not None:
        check(_lib.load().orca_encoder_forward_codes_window(net.ctx.handle, net.handle, _p(codes), codes.stride(0), win.origin, codes.shape[1],
                                                            1 if reverse else 0, B, L, bin_lo, hi, _p(out), out.stride(0), out.stride(1), chunk_bp),
              "orca_encoder_forward_codes_window")
        return out
    check(_lib.load().orca_encoder_forward_codes(net.ctx.handle, net.handle, _p(codes), codes.stride(0), 1 if reverse else 0, B, L,
                                                 bin_lo, hi, _p(out), out.stride(0), out.stride(1), chunk_bp), "orca_encoder_forward_codes")
    return out


def encoder_forward_two_strands(net, codes, out):
    """Forward strand and reverse complement of ONE packed sequence (``codes`` [1,L] uint8) into rows 0 and 1 of ``out`` [2,128,bins]: stages 1-2
    per strand, stages 3-7 once for both (include/orca_hip.h: orca_encoder_forward_two_strands) - the bits of two `encoder_forward_codes` calls."""
    if not (isinstance(codes, torch.Tensor) and codes.is_cuda and codes.dtype == torch.uint8 and codes.dim() == 2 and codes.shape[0] == 1):
        raise ValueError("codes must be a [1,L] uint8 ROCm tensor")
    if codes.stride(1) != 1:
        codes = codes.contiguous()
    L = codes.shape[1]
    if tuple(out.shape) != (2, 128, encoder_num_bins(L)) or out.stride(2) != 1 or out.dtype != torch.float32:
        raise ValueError(f"out must be a float32 [2,128,{encoder_num_bins(L)}] view with unit stride along the bins")
    net.ctx.sync_stream()
    check(_lib.load().orca_encoder_forward_two_strands(net.ctx.handle, net.handle, _p(codes), L, _p(out[0]), _p(out[1]), out.stride(1)),
          "orca_encoder_forward_two_strands")
    return out


# ---- the Encoder in two parts (include/orca_hip.h: orca_encoder_stage3_planes ...; sv.Stage3Cache is the user) -------------------------------------
def p16_plane_units(n):
    """16-byte units per plane of a P16 sequence tensor of n positions (guards and tile padding included)."""
    return int(_lib.load().orca_p16_plane_units(int(n)))


def _codes1d(codes):
    if not (isinstance(codes, torch.Tensor) and codes.is_cuda and codes.dtype == torch.uint8 and codes.dim() == 1 and codes.is_contiguous()):
        raise ValueError("codes must be a contiguous [L] uint8 ROCm tensor")
    return codes


def _planes(t, units, name):
    if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and tuple(t.shape) == (32, units, 4)):
        raise ValueError(f"{name}: a contiguous [32,{units},4] float32 ROCm tensor (32 P16 planes of {units} 16-byte units)")
    return t


def encoder_stage3_planes(net, codes, reverse=False):
    """Stage 3's output (before MaxPool1d(5)) of the bases ``codes`` [L] (L % 80 == 0; ``reverse``: of their reverse complement) as 32 P16
    planes: a [32, units, 4] float32 tensor, position j at unit 8 + j."""
    codes = _codes1d(codes)
    L = codes.numel()
    if L <= 0 or L % 80:
        raise ValueError("stage-3 planes: the number of bases must be a positive multiple of 80")
    units = p16_plane_units(L // 16)
    planes = torch.empty((32, units, 4), dtype=torch.float32, device=codes.device)
    net.ctx.sync_stream()
    check(_lib.load().orca_encoder_stage3_planes(net.ctx.handle, net.handle, _p(codes), L, 1 if reverse else 0, _p(planes), units), "orca_encoder_stage3_planes")
    return planes


def p16_pool5_into(ctx, src, src_pos0, dst, dst_pos0, count):
    """MaxPool1d(5) of positions [src_pos0, src_pos0 + 5 count) of the planes ``src`` into positions [dst_pos0, dst_pos0 + count) of ``dst``."""
    _planes(src, src.shape[1], "src")
    _planes(dst, dst.shape[1], "dst")
    ctx.sync_stream()
    check(_lib.load().orca_p16_pool5_into(ctx.handle, _p(src), src.shape[1], int(src_pos0), _p(dst), dst.shape[1], int(dst_pos0), int(count)), "orca_p16_pool5_into")


def encoder_front_snippet(net, codes, reverse, base0, nbases, skip, count, dst, dst_pos0):
    """Stages 1-3 + MaxPool1d(5) on strand positions [base0, base0 + nbases) of ``codes`` [L]; pooled positions [skip, skip + count) go to
    positions [dst_pos0, ..) of the stage-4 input planes ``dst``."""
    codes = _codes1d(codes)
    _planes(dst, dst.shape[1], "dst")
    net.ctx.sync_stream()
    check(_lib.load().orca_encoder_front_snippet(net.ctx.handle, net.handle, _p(codes), codes.numel(), 1 if reverse else 0, int(base0), int(nbases), int(skip), int(count),
                                                 _p(dst), dst.shape[1], int(dst_pos0)), "orca_encoder_front_snippet")


def encoder_back(net, s4, n4, out):
    """Stages 4-7 from the stage-4 input planes ``s4`` ([32, p16_plane_units(n4), 4]) into ``out`` [128, n4 / 50] (unit stride along the bins)."""
    _planes(s4, p16_plane_units(n4), "s4")
    if not (out.is_cuda and out.dtype == torch.float32 and tuple(out.shape) == (128, n4 // 50) and out.stride(1) == 1):
        raise ValueError(f"out must be a [128,{n4 // 50}] float32 view with unit stride along the bins")
    net.ctx.sync_stream()
    check(_lib.load().orca_encoder_back(net.ctx.handle, net.handle, _p(s4), s4.shape[1], int(n4), _p(out), out.stride(0)), "orca_encoder_back")
    return out


def _rows(t, name):
    if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and t.dim() == 2 and t.shape[1] == 128):
        raise ValueError(f"{name}: a contiguous [n,128] float32 ROCm tensor")
    return t


def encoder_stage4_rows(net, s4, n4):
    """Stage 4 alone: stage-4 input planes ``s4`` ([32, p16_plane_units(n4), 4]) -> its output rows [n4, 128] (before the MaxPool1d(5) in front of stage 5)."""
    _planes(s4, p16_plane_units(n4), "s4")
    rows = torch.empty((n4, 128), dtype=torch.float32, device=s4.device)
    net.ctx.sync_stream()
    check(_lib.load().orca_encoder_stage4_rows(net.ctx.handle, net.handle, _p(s4), s4.shape[1], int(n4), _p(rows)), "orca_encoder_stage4_rows")
    return rows


def rows_pool5_into(ctx, src, src_pos0, dst, dst_pos0, count):
    """MaxPool1d(5) of rows [src_pos0, src_pos0 + 5 count) of ``src`` [n,128] into rows [dst_pos0, dst_pos0 + count) of ``dst`` [m,128]."""
    _rows(src, "src")
    _rows(dst, "dst")
    ctx.sync_stream()
    check(_lib.load().orca_rows_pool5_into(ctx.handle, _p(src), src.shape[0], int(src_pos0), _p(dst), dst.shape[0], int(dst_pos0), int(count)), "orca_rows_pool5_into")


def encoder_front4_snippet(net, codes, reverse, base0, nbases, skip, count, dst, dst_pos0):
    """Stages 1-4 + MaxPool1d(5) on strand positions [base0, base0 + nbases) of ``codes`` [L] (multiples of 400); pooled rows [skip, skip + count)
    go to rows [dst_pos0, ..) of the stage-5 input ``dst`` [n5,128]."""
    codes = _codes1d(codes)
    _rows(dst, "dst")
    net.ctx.sync_stream()
    check(_lib.load().orca_encoder_front4_snippet(net.ctx.handle, net.handle, _p(codes), codes.numel(), 1 if reverse else 0, int(base0), int(nbases), int(skip), int(count),
                                                  _p(dst), dst.shape[0], int(dst_pos0)), "orca_encoder_front4_snippet")


def encoder_front4_ranges(net, codes, reverse, ranges, dst):
    """Stages 1-4 + MaxPool1d(5) on ALL of ``codes`` [L] (the snippets of one window strand, concatenated); ranges = [(skip, count, dst_pos0)]: pooled
    rows [skip, skip + count) of that run go to rows [dst_pos0, ..) of ``dst`` [n5,128]."""
    codes = _codes1d(codes)
    _rows(dst, "dst")
    flat = (ctypes.c_int64 * (3 * len(ranges)))(*[int(v) for r in ranges for v in r])
    net.ctx.sync_stream()
    check(_lib.load().orca_encoder_front4_ranges(net.ctx.handle, net.handle, _p(codes), codes.numel(), 1 if reverse else 0, len(ranges), flat, _p(dst), dst.shape[0]),
          "orca_encoder_front4_ranges")


def encoder_back5(net, rows, out):
    """Stages 5-7 from the stage-5 input ``rows`` [n5,128] into ``out`` [128, n5 / 10] (unit stride along the bins)."""
    _rows(rows, "rows")
    n5 = rows.shape[0]
    if not (out.is_cuda and out.dtype == torch.float32 and tuple(out.shape) == (128, n5 // 10) and out.stride(1) == 1):
        raise ValueError(f"out must be a [128,{n5 // 10}] float32 view with unit stride along the bins")
    net.ctx.sync_stream()
    check(_lib.load().orca_encoder_back5(net.ctx.handle, net.handle, _p(rows), n5, _p(out), out.stride(0)), "orca_encoder_back5")
    return out


# ---- the 1 Mb mutagenesis screen (include/orca_hip.h: orca_screen_*; orca_amd/screen.py is the user) ------------------------------------------
SCREEN_EDIT_FIELDS = 8          # int64 per snippet of an edit table: out_off, b0, nb, kind, pos, len, pay_off, 0
SCREEN_KINDS = {"sub": 0, "mask": 1, "inv": 2}


def _i64_cuda(t, name, cols):
    if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.int64 and t.is_contiguous() and t.dim() == 2 and t.shape[1] == cols):
        raise ValueError(f"{name}: a contiguous [k,{cols}] int64 ROCm tensor")
    return t


def screen_edit_codes(ctx, window, table_host, table, payload, out):
    """Edited snippets of ``window`` [L] uint8 into ``out`` [total] (orca_screen_edit_codes).  ``table_host``: the same [k, 8] int64 table as numpy,
    checked here (the kernel also clamps every read); ``table``: its device copy."""
    window, out = _codes1d(window), _codes1d(out)
    _i64_cuda(table, "table", SCREEN_EDIT_FIELDS)
    t = np.asarray(table_host, dtype=np.int64)
    L, npay = window.numel(), (0 if payload is None else payload.numel())
    if t.shape != tuple(table.shape) or t.shape[0] == 0:
        raise ValueError("edit table: host and device copies differ or are empty")
    off, b0, nb, kind, pos, ln, po = (t[:, k] for k in range(7))
    if (off[0] != 0 or np.any(off[1:] != (off + nb)[:-1]) or int((off + nb)[-1]) != out.numel() or np.any(nb <= 0) or np.any(b0 < 0)
            or np.any(b0 + nb > L) or np.any(pos < 0) or np.any(ln <= 0) or np.any(pos + ln > L) or np.any((kind < 0) | (kind > 2))
            or np.any((kind == 0) & ((po < 0) | (po + ln > npay)))):
        raise ValueError("edit table: snippets must be packed back to back inside the window, edits inside it, payloads inside the payload buffer")
    if payload is not None:
        payload = _codes1d(payload)
    ctx.sync_stream()
    check(_lib.load().orca_screen_edit_codes(ctx.handle, _p(window), L, _p(table), t.shape[0], ctypes.c_void_p(0) if payload is None else _p(payload), npay,
                                             _p(out), out.numel()), "orca_screen_edit_codes")
    return out


def screen_splice_rows(ctx, ref, fresh, table, out):
    """B stage-5 row images ``out`` [B, n5, 128]: ``ref`` [n5, 128] with rows [row_lo, row_lo + row_cnt) of image b taken from rows [src_row, ..) of
    ``fresh`` [R, 128]; ``table`` [B, 3] int64 on the device."""
    _rows(ref, "ref")
    _rows(fresh, "fresh")
    _i64_cuda(table, "table", 3)
    n5 = ref.shape[0]
    if not (out.is_cuda and out.dtype == torch.float32 and out.is_contiguous() and out.dim() == 3 and tuple(out.shape[1:]) == (n5, 128)
            and out.shape[0] == table.shape[0]):
        raise ValueError(f"out: a contiguous [B,{n5},128] float32 ROCm tensor, B = the table's rows")
    ctx.sync_stream()
    check(_lib.load().orca_screen_splice_rows(ctx.handle, _p(ref), n5, _p(fresh), fresh.shape[0], _p(table), out.shape[0], _p(out)), "orca_screen_splice_rows")
    return out


def encoder_back5_batch(net, rows, out=None):
    """Stages 5-7 of B windows from their stage-5 rows ``rows`` [B, n5, 128] into ``out`` [B, 128, n5 / 10] (unit stride along the bins)."""
    if not (isinstance(rows, torch.Tensor) and rows.is_cuda and rows.dtype == torch.float32 and rows.is_contiguous() and rows.dim() == 3 and rows.shape[2] == 128):
        raise ValueError("rows: a contiguous [B,n5,128] float32 ROCm tensor")
    B, n5 = rows.shape[0], rows.shape[1]
    if out is None:
        out = torch.empty((B, 128, n5 // 10), dtype=torch.float32, device=rows.device)
    elif not (out.is_cuda and out.dtype == torch.float32 and tuple(out.shape) == (B, 128, n5 // 10) and out.stride(2) == 1):
        raise ValueError(f"out must be a [{B},128,{n5 // 10}] float32 view with unit stride along the bins")
    net.ctx.sync_stream()
    check(_lib.load().orca_encoder_back5_batch(net.ctx.handle, net.handle, _p(rows), B, n5, _p(out), out.stride(0), out.stride(1)), "orca_encoder_back5_batch")
    return out


def _maps_args(alt, ref):
    """alt [B, n, n] (any batch stride, rows contiguous) and ref [n, n] of the score entry points: (alt, ref, n)."""
    alt, ref = _f32_cuda(alt, "alt"), _f32_cuda(ref, "ref").contiguous()
    n = ref.shape[0]
    if alt.dim() != 3 or ref.dim() != 2 or tuple(alt.shape[1:]) != (n, n) or alt.stride(2) != 1 or alt.stride(1) != n or tuple(ref.shape) != (n, n):
        raise ValueError(f"alt [B,{n},{n}] with contiguous maps, ref [{n},{n}]")
    return alt, ref, n


def _f32_outputs(device, *shapes):
    return tuple(torch.empty(s, dtype=torch.float32, device=device) for s in shapes)


def _map_batch(t, name):
    """The map-batch rule of the readouts: ``t`` is [B, n, n] float32 on the device with contiguous maps (any batch stride) and at least one map.
    (t, B, n, batch stride) - for B = 1 a stride of at least n * n: torch may report any stride for the one map."""
    t = _f32_cuda(t, name)
    if t.dim() != 3 or t.shape[0] < 1 or t.shape[1] != t.shape[2] or t.stride(2) != 1 or t.stride(1) != t.shape[1]:
        raise ValueError(f"{name}: [B,n,n] with B >= 1 and contiguous maps, got {tuple(t.shape)}")
    B, n = t.shape[0], t.shape[1]
    return t, B, n, t.stride(0) if B > 1 else max(t.stride(0), n * n)


def _host_list(a, name):
    """A short list of ints (widths, viewpoints) as a contiguous int32 [k] numpy table."""
    return _host_table(np.asarray(a).reshape(-1, 1), np.int32, 1, name)[:, 0]


def screen_scores(ctx, alt, ref):
    """alt [B, n, n] (any batch stride, rows contiguous) against ref [n, n]: (profile [B, n], mean [B], max [B]) of |alt - ref|."""
    alt, ref, n = _maps_args(alt, ref)
    B = alt.shape[0]
    profile, mean, amax = _f32_outputs(alt.device, (B, n), (B,), (B,))
    ctx.sync_stream()
    check(_lib.load().orca_screen_scores(ctx.handle, _p(alt), alt.stride(0), _p(ref), B, n, _p(profile), _p(mean), _p(amax)), "orca_screen_scores")
    return profile, mean, amax


# compound edits and region scores (orca_screen_*_multi, orca_screen_region_scores).  The small tables are numpy on the host; the wrappers upload the
# device copies, and the library checks the host copies before it launches anything (a malformed table is an OrcaHipError, never a launch)
SCREEN_SPAN_FIELDS = 4          # int64 per span: kind, pos, len, pay_off


def _on_device(t, name, dtype):
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name} must be a torch.Tensor")
    if not t.is_cuda:
        raise OrcaHipError(f"{name} is on '{t.device}': orca_amd has no CPU path (move it to the MI355X with .cuda())")
    if t.dtype != dtype or not t.is_contiguous():
        raise ValueError(f"{name}: a contiguous {dtype} ROCm tensor")
    return t


def _host_table(a, dtype, cols, name):
    a = np.ascontiguousarray(a, dtype=dtype)
    if a.ndim != 2 or a.shape[1] != cols:
        raise ValueError(f"{name}: a [k,{cols}] table")
    return a


def _np_p(a):
    return ctypes.c_void_p(a.ctypes.data if a.size else 0)


def _dev_p(t):
    return ctypes.c_void_p(t.data_ptr() if t.numel() else 0)


def _screen_codes(entry, ctx, src, name, size, table_host, sub_host, sub_name, payload, out):
    """The call of orca_screen_edit_codes_multi / _assemble_codes: bases of ``src`` (``name``, [``size``] uint8) into ``out`` by the snippet table and its
    4-field sub-table ``sub_name``, both numpy on the host and uploaded here."""
    src, out = _on_device(src, name, torch.uint8), _on_device(out, "out", torch.uint8)
    if src.dim() != 1 or out.dim() != 1:
        raise ValueError(f"{name}, out: [{size}] and [total] uint8")
    if payload is not None:
        payload = _on_device(payload, "payload", torch.uint8)
    t, s = _host_table(table_host, np.int64, SCREEN_EDIT_FIELDS, "snippet table"), _host_table(sub_host, np.int64, 4, sub_name)
    td, sd = torch.from_numpy(t).to(src.device), torch.from_numpy(s).to(src.device)
    ctx.sync_stream()
    check(getattr(_lib.load(), entry)(ctx.handle, _dev_p(src), src.numel(), _dev_p(td), _np_p(t), t.shape[0], _dev_p(sd), _np_p(s), s.shape[0],
                                      ctypes.c_void_p(0) if payload is None else _dev_p(payload), 0 if payload is None else payload.numel(),
                                      _dev_p(out), out.numel()), entry)
    return out


def screen_edit_codes_multi(ctx, window, table_host, spans_host, payload, out):
    """Edited snippets of ``window`` [L] uint8 into ``out`` [total] with any number of spans per snippet (orca_screen_edit_codes_multi).
    ``table_host`` [k, 8] int64 numpy = [out_off, b0, nb, span_lo, span_cnt, 0, 0, 0]; ``spans_host`` [s, 4] int64 numpy = [kind, pos, len, pay_off]."""
    return _screen_codes("orca_screen_edit_codes_multi", ctx, window, "window", "L", table_host, spans_host, "span table", payload, out)


def _segment_args(segments_host, cols, seg_off_host, out, n5):
    """A segment table of ``cols`` fields with its offsets, and the images ``out`` they describe: (table, offsets, B)."""
    g = _host_table(segments_host, np.int64, cols, "segment table")
    o = np.ascontiguousarray(seg_off_host, dtype=np.int64)
    if o.ndim != 1 or o.size < 1:
        raise ValueError("segment offsets: [B + 1] int64")
    B = o.size - 1
    if out.dim() != 3 or tuple(out.shape) != (B, n5, 128):
        raise ValueError(f"out: a contiguous [{B},{n5},128] float32 ROCm tensor, B + 1 = the number of segment offsets")
    return g, o, B


def screen_splice_rows_multi(ctx, ref, fresh, segments_host, seg_off_host, out):
    """B stage-5 row images ``out`` [B, n5, 128]: ``ref`` [n5, 128] with, for every segment [row_lo, row_cnt, src_row] of image b (``segments_host``
    [s, 3] int64 numpy, image b's at [seg_off_host[b], seg_off_host[b + 1])), rows [row_lo, row_lo + row_cnt) from rows [src_row, ..) of ``fresh``."""
    ref, fresh, out = _on_device(ref, "ref", torch.float32), _on_device(fresh, "fresh", torch.float32), _on_device(out, "out", torch.float32)
    if ref.dim() != 2 or ref.shape[1] != 128 or fresh.dim() != 2 or fresh.shape[1] != 128:
        raise ValueError("ref, fresh: [n,128] float32")
    n5 = ref.shape[0]
    g, o, B = _segment_args(segments_host, 3, seg_off_host, out, n5)
    gd, od = torch.from_numpy(g).to(ref.device), torch.from_numpy(o).to(ref.device)
    ctx.sync_stream()
    check(_lib.load().orca_screen_splice_rows_multi(ctx.handle, _dev_p(ref), n5, _dev_p(fresh), fresh.shape[0], _dev_p(gd), _np_p(g), g.shape[0], _dev_p(od), _np_p(o),
                                                    B, _dev_p(out)), "orca_screen_splice_rows_multi")
    return out


# insertions and deletions (orca_screen_assemble_codes, orca_screen_gather_rows)
SCREEN_PIECE_FIELDS = 4         # int64 per piece: dst (alt base), kind, src, len
SCREEN_PIECE_KINDS = {"fwd": 0, "rc": 1, "payload": 2, "n": 3}
SCREEN_GATHER_FIELDS = 4        # int64 per segment: row_lo, row_cnt, source, src_row
SCREEN_SRC_FRESH, SCREEN_SRC_REF = -1, -2


def screen_assemble_codes(ctx, context, table_host, pieces_host, payload, out):
    """Alt bases from piece lists over ``context`` [C] uint8 (the window followed by its right flank) into ``out`` [total]
    (orca_screen_assemble_codes).  ``table_host`` [k, 8] int64 numpy = [out_off, a0, nb, piece_lo, piece_cnt, 0, 0, 0] (a0 in alt coordinates);
    ``pieces_host`` [n, 4] int64 numpy = [dst, kind, src, len], kind 0 context forward, 1 its reverse complement, 2 payload, 3 N."""
    return _screen_codes("orca_screen_assemble_codes", ctx, context, "context", "C", table_host, pieces_host, "piece table", payload, out)


def screen_gather_rows(ctx, ref, fresh, entries, segments_host, seg_off_host, out):
    """B stage-5 row images ``out`` [B, n5, 128] (orca_screen_gather_rows): for every segment [row_lo, row_cnt, source, src_row] of image b
    (``segments_host`` [s, 4] int64 numpy, image b's at [seg_off_host[b], seg_off_host[b + 1])) rows [row_lo, row_lo + row_cnt) come from rows
    [src_row, ..) of ``fresh`` [R, 128] (source -1) or of ``ref`` [n5, 128] (-2), or are the MaxPool1d(5) of rows src_row + 5 t .. + 4 of
    ``entries[source]`` (a list of [n, 128] float32 tensors: stage-4 phase entries); every other row is ``ref`` at its own index."""
    ref, fresh, out = _on_device(ref, "ref", torch.float32), _on_device(fresh, "fresh", torch.float32), _on_device(out, "out", torch.float32)
    if ref.dim() != 2 or ref.shape[1] != 128 or fresh.dim() != 2 or fresh.shape[1] != 128:
        raise ValueError("ref, fresh: [n,128] float32")
    entries = [_on_device(e, "a phase entry", torch.float32) for e in entries]
    if any(e.dim() != 2 or e.shape[1] != 128 or e.data_ptr() % 16 for e in entries):
        raise ValueError("phase entries: [n,128] float32, 16-byte aligned")
    n5 = ref.shape[0]
    g, o, B = _segment_args(segments_host, SCREEN_GATHER_FIELDS, seg_off_host, out, n5)
    ptrs = np.array([e.data_ptr() for e in entries], dtype=np.int64)
    cnts = np.array([e.shape[0] for e in entries], dtype=np.int64)
    gd, od, pd, cd = (torch.from_numpy(a).to(ref.device) for a in (g, o, ptrs, cnts))
    ctx.sync_stream()
    check(_lib.load().orca_screen_gather_rows(ctx.handle, _dev_p(ref), n5, _dev_p(fresh), fresh.shape[0], _dev_p(pd), _dev_p(cd), _np_p(cnts), len(entries),
                                              _dev_p(gd), _np_p(g), g.shape[0], _dev_p(od), _np_p(o), B, _dev_p(out)), "orca_screen_gather_rows")
    return out


def screen_region_scores(ctx, alt, ref, rects_host):
    """alt [B, n, n] (any batch stride, rows contiguous) against ref [n, n] over the K rectangles ``rects_host`` [K, 4] = (i0, i1, j0, j1), half open:
    (mean of alt - ref [B, K], mean of |alt - ref| [B, K]) (orca_screen_region_scores)."""
    alt, ref, n = _maps_args(alt, ref)
    r = _host_table(rects_host, np.int32, 4, "rectangles")
    B, K = alt.shape[0], r.shape[0]
    rd = torch.from_numpy(r).to(alt.device)
    sg, ab = _f32_outputs(alt.device, (B, K), (B, K))
    ctx.sync_stream()
    check(_lib.load().orca_screen_region_scores(ctx.handle, _dev_p(alt), alt.stride(0), _p(ref), B, n, _dev_p(rd), _np_p(r), K, _dev_p(sg), _dev_p(ab)),
          "orca_screen_region_scores")
    return sg, ab


# non-additivity (orca_screen_epistasis_scores, orca_screen_epistasis_region_scores): the member table is two more small tables
def screen_epistasis_scores(ctx, alt, bank, ref, member_off_host, members_host, rects_host=None):
    """The B set maps alt [B, n, n] against the sum of their members' effects (orca_screen_epistasis_scores): ``bank`` [U, n, n] holds every single
    edit's map (both any batch stride, rows contiguous), ref [n, n] the unedited map; set b has members ``members_host[member_off_host[b]:
    member_off_host[b + 1]]`` ([B + 1] int64 from 0, strictly increasing; [P] int32 bank indices in [0, U)).  Per pixel in fp64 t = sum_m (bank[m] - ref),
    r = (alt - ref) - t: (profile [B, n] = mean_j |r|, mean [B] = mean |r|, max [B] = max |r|, additive mean [B] = mean |t|, region [B, K], region abs
    [B, K]) - the last two the means of r and of |r| over the K rectangles ``rects_host`` [K, 4] = (i0, i1, j0, j1), half open
    (orca_screen_epistasis_region_scores), None without them."""
    alt, ref, n = _maps_args(alt, ref)
    bank = _f32_cuda(bank, "bank")
    if bank.dim() != 3 or bank.shape[0] < 1 or tuple(bank.shape[1:]) != (n, n) or bank.stride(2) != 1 or bank.stride(1) != n or bank.device != alt.device:
        raise ValueError(f"bank: [U,{n},{n}] beside alt with U >= 1 and contiguous maps")
    o = np.ascontiguousarray(member_off_host, dtype=np.int64)
    m = np.ascontiguousarray(members_host, dtype=np.int32)
    B, U = alt.shape[0], bank.shape[0]
    if o.ndim != 1 or o.size != B + 1 or m.ndim != 1 or B < 1:
        raise ValueError(f"member table: offsets [{B + 1}] int64 (one set per alt map, at least one), members [P] int32")
    bs, bank_bs = _map_batch(alt, "alt")[3], _map_batch(bank, "bank")[3]
    od, md = torch.from_numpy(o).to(alt.device), torch.from_numpy(m).to(alt.device)
    head = (ctx.handle, _dev_p(alt), bs, _dev_p(bank), bank_bs, U, _p(ref), B, n, _dev_p(od), _np_p(o), _dev_p(md), _np_p(m), m.size)
    profile, mean, amax, add = _f32_outputs(alt.device, (B, n), (B,), (B,), (B,))
    ctx.sync_stream()
    check(_lib.load().orca_screen_epistasis_scores(*head, _dev_p(profile), _dev_p(mean), _dev_p(amax), _dev_p(add)), "orca_screen_epistasis_scores")
    if rects_host is None:
        return profile, mean, amax, add, None, None
    r = _host_table(rects_host, np.int32, 4, "rectangles")
    rd = torch.from_numpy(r).to(alt.device)
    sg, ab = _f32_outputs(alt.device, (B, r.shape[0]), (B, r.shape[0]))
    check(_lib.load().orca_screen_epistasis_region_scores(*head, _dev_p(rd), _np_p(r), r.shape[0], _dev_p(sg), _dev_p(ab)), "orca_screen_epistasis_region_scores")
    return profile, mean, amax, add, sg, ab


# aligned scores (orca_screen_aligned_scores, orca_screen_aligned_region_scores): the bin map is one more small table
SCREEN_ALIGNED_MAX_BINS = 256


def _aligned_args(alt, ref, bin_map_host, bin_map):
    alt, ref, n = _maps_args(alt, ref)
    m = _host_table(bin_map_host, np.int32, n, "bin map")
    if m.shape[0] != alt.shape[0]:
        raise ValueError(f"bin map: [{alt.shape[0]},{n}] int32, one row per alt map")
    md = torch.from_numpy(m).to(alt.device) if bin_map is None else _on_device(bin_map, "bin_map", torch.int32)
    if tuple(md.shape) != m.shape or md.device != alt.device:
        raise ValueError("bin map: host and device copies differ in shape")
    return alt, ref, m, md


def screen_aligned_scores(ctx, alt, ref, bin_map_host, bin_map=None):
    """alt [B, n, n] (any batch stride, rows contiguous) against ref [n, n] on aligned bins (orca_screen_aligned_scores): ``bin_map_host`` [B, n] int32
    numpy, the reference bin of every alt bin or -1 (``bin_map``: its device copy, uploaded here when None).  (profile [B, n], mean [B], max [B]) of
    |alt[i, j] - ref[map i, map j]| over the mapped bins, NaN where nothing is mapped."""
    alt, ref, m, md = _aligned_args(alt, ref, bin_map_host, bin_map)
    B, n = m.shape
    profile, mean, amax = _f32_outputs(alt.device, (B, n), (B,), (B,))
    ctx.sync_stream()
    check(_lib.load().orca_screen_aligned_scores(ctx.handle, _dev_p(alt), alt.stride(0), _p(ref), B, n, _dev_p(md), _np_p(m), _dev_p(profile), _dev_p(mean),
                                                 _dev_p(amax)), "orca_screen_aligned_scores")
    return profile, mean, amax


def screen_aligned_region_scores(ctx, alt, ref, bin_map_host, rects_host, bin_map=None):
    """`screen_region_scores` on aligned bins (orca_screen_aligned_region_scores): the K rectangles ``rects_host`` [K, 4] = (i0, i1, j0, j1) are in
    REFERENCE bins, and rectangle k takes the alt pairs (i, j) with map i in [i0, i1) and map j in [j0, j1): (mean of alt[i, j] - ref[map i, map j]
    [B, K], mean of its absolute value [B, K]), NaN where no pair qualifies."""
    alt, ref, m, md = _aligned_args(alt, ref, bin_map_host, bin_map)
    B, n = m.shape
    r = _host_table(rects_host, np.int32, 4, "rectangles")
    K = r.shape[0]
    rd = torch.from_numpy(r).to(alt.device)
    sg, ab = _f32_outputs(alt.device, (B, K), (B, K))
    ctx.sync_stream()
    check(_lib.load().orca_screen_aligned_region_scores(ctx.handle, _dev_p(alt), alt.stride(0), _p(ref), B, n, _dev_p(md), _np_p(m), _dev_p(rd), _np_p(r), K,
                                                        _dev_p(sg), _dev_p(ab)), "orca_screen_aligned_region_scores")
    return sg, ab


# tracks (orca_screen_insulation, orca_screen_viewpoints): 1-D readouts per map; the widths / viewpoints are one more small table, the bin map is optional
def _track_args(alt, ref, table_host, name, bin_map_host, bin_map):
    """The arguments the two track entry points share: (alt, ref, batch stride, table [k] int32 on the host, its device copy, bin map host / device or
    None / None)."""
    if bin_map_host is None:
        if bin_map is not None:
            raise ValueError("bin_map: the device copy of bin_map_host, which is None")
        (alt, ref, _), m, md = _maps_args(alt, ref), None, None
    else:
        alt, ref, m, md = _aligned_args(alt, ref, bin_map_host, bin_map)
    alt, _, _, bs = _map_batch(alt, "alt")
    t = _host_list(table_host, name)
    return alt, ref, bs, t, torch.from_numpy(t).to(alt.device), m, md


def screen_insulation(ctx, alt, ref, widths_host, bin_map_host=None, bin_map=None):
    """Insulation tracks of alt [B, n, n] (any batch stride, rows contiguous) at the W widths ``widths_host`` (1 to 8 ints, each 1 .. 128 bins), against
    ref [n, n] (orca_screen_insulation): (track [B, W, n], delta [B, W, n], aligned [B, W, n] or None).  The diamond of bin i at width w is rows
    [i - w, i) x columns (i, i + w]; ins_w(m)[i] is its fp64 mean, NaN where it does not fit (i < w or i >= n - w).  track = ins(alt), delta = ins(alt)[i] -
    ins(ref)[i], and with ``bin_map_host`` [B, n] int32 (``bin_map``: its device copy, uploaded here when None) aligned = ins(alt)[i] - ins(ref)[map i],
    NaN where alt bin i stands for no reference bin or the reference diamond does not fit there.  ``ref=None``: the track alone, (track, None, None)."""
    if ref is None:
        if bin_map_host is not None or bin_map is not None:
            raise ValueError("ref=None computes the track alone: no bin map")
        alt = _f32_cuda(alt, "alt")
        if alt.dim() != 3:
            raise ValueError("alt: [B,n,n]")
        alt, _, bs, w, wd, m, md = _track_args(alt, alt[0], widths_host, "widths", None, None)       # ref only says n here; it is not passed on
    else:
        alt, ref, bs, w, wd, m, md = _track_args(alt, ref, widths_host, "widths", bin_map_host, bin_map)
    B, n, W = alt.shape[0], alt.shape[1], w.shape[0]
    null = ctypes.c_void_p(0)
    track, = _f32_outputs(alt.device, (B, W, n))
    delta = None if ref is None else _f32_outputs(alt.device, (B, W, n))[0]
    aligned = None if m is None else _f32_outputs(alt.device, (B, W, n))[0]
    ctx.sync_stream()
    check(_lib.load().orca_screen_insulation(ctx.handle, _dev_p(alt), bs, null if ref is None else _p(ref), B, n, _dev_p(wd), _np_p(w), W,
                                             null if m is None else _dev_p(md), null if m is None else _np_p(m), _dev_p(track),
                                             null if delta is None else _dev_p(delta), null if aligned is None else _dev_p(aligned)), "orca_screen_insulation")
    return track, delta, aligned


def screen_viewpoints(ctx, alt, ref, views_host, bin_map_host=None, bin_map=None):
    """Viewpoint profiles (virtual 4C) of alt [B, n, n] (any batch stride, rows contiguous) against ref [n, n] at the V viewpoint bins ``views_host`` (1 to
    64 ints in [0, n)) (orca_screen_viewpoints): (delta [B, V, n], aligned [B, V, n] or None).  delta = alt[view, j] - ref[view, j] in fp32.  With
    ``bin_map_host`` [B, n] int32 (``bin_map``: its device copy) the viewpoint is a REFERENCE bin: aligned = the mean of the alt rows i with map i == view,
    at column j, minus ref[view, map j]; NaN where no alt bin stands for the viewpoint or column j stands for nothing."""
    alt, ref, bs, v, vd, m, md = _track_args(alt, ref, views_host, "viewpoints", bin_map_host, bin_map)
    B, n, V = alt.shape[0], alt.shape[1], v.shape[0]
    null = ctypes.c_void_p(0)
    delta, = _f32_outputs(alt.device, (B, V, n))
    aligned = None if m is None else _f32_outputs(alt.device, (B, V, n))[0]
    ctx.sync_stream()
    check(_lib.load().orca_screen_viewpoints(ctx.handle, _dev_p(alt), bs, _p(ref), B, n, _dev_p(vd), _np_p(v), V, null if m is None else _dev_p(md),
                                             null if m is None else _np_p(m), _dev_p(delta), null if aligned is None else _dev_p(aligned)), "orca_screen_viewpoints")
    return delta, aligned


# distance strata (orca_screen_strata_scores): similarity scores per genomic distance and per map; the bin map is optional
def _strata_args(d_range, B, n, dev, counts=True):
    """What the two strata entry points share: (d_lo, d_hi, the dict of the eight outputs) - ``d_range`` = (d_lo, d_hi), every stratum of the ``n`` by
    default; ``dist_count`` is None without ``counts``."""
    try:
        d_lo, d_hi = (0, n) if d_range is None else (int(v) for v in d_range)
    except (TypeError, ValueError):
        raise ValueError("d_range: (d_lo, d_hi)") from None
    out = dict(zip(("dist_delta", "dist_abs", "dist_rms", "mse"), _f32_outputs(dev, (B, n), (B, n), (B, n), (B,))))
    out["dist_corr"] = torch.empty((B, n), dtype=torch.float64, device=dev)
    out["corr"], out["scc"] = (torch.empty(B, dtype=torch.float64, device=dev) for _ in range(2))
    out["dist_count"] = torch.empty((B, n), dtype=torch.int32, device=dev) if counts else None
    return d_lo, d_hi, out


def screen_strata_scores(ctx, alt, ref, bin_map=None, d_range=None, bin_map_dev=None):
    """Distance-stratified similarity of alt [B, n, n] (any batch stride, rows contiguous) to ref [n, n] (orca_screen_strata_scores; include/orca_hip.h
    has the definitions): a dict of ``dist_delta``, ``dist_abs``, ``dist_rms`` [B, n] float32 (the mean of alt - ref, of its absolute value and its root
    mean square over stratum d, the pairs (i, i + d)), ``dist_corr`` [B, n] float64 (the Pearson correlation within stratum d), ``mse`` [B] float32,
    ``corr`` and ``scc`` [B] float64 (mean squared difference, Pearson and stratum-adjusted correlation over the strata ``d_range`` = (d_lo, d_hi),
    0 <= d_lo < d_hi <= n; all of them by default) and ``dist_count`` [B, n] int32, the pairs per stratum, or None without a bin map.  ``bin_map``
    [B, n] int32 numpy on the host (``bin_map_dev``: its device copy, uploaded here when None): the aligned form, alt pair (i, i + d) against
    reference pair (map i, map (i + d)) where both are mapped."""
    if bin_map is None:
        if bin_map_dev is not None:
            raise ValueError("bin_map_dev: the device copy of bin_map, which is None")
        (alt, ref, _), m, md = _maps_args(alt, ref), None, None
    else:
        alt, ref, m, md = _aligned_args(alt, ref, bin_map, bin_map_dev)
    alt, B, n, bs = _map_batch(alt, "alt")
    d_lo, d_hi, out = _strata_args(d_range, B, n, alt.device, counts=m is not None)
    null = ctypes.c_void_p(0)
    ctx.sync_stream()
    check(_lib.load().orca_screen_strata_scores(ctx.handle, _dev_p(alt), bs, _p(ref), B, n, null if m is None else _dev_p(md), null if m is None else _np_p(m),
                                                d_lo, d_hi, _dev_p(out["dist_delta"]), _dev_p(out["dist_abs"]), _dev_p(out["dist_rms"]), _dev_p(out["dist_corr"]),
                                                null if m is None else _dev_p(out["dist_count"]), _dev_p(out["mse"]), _dev_p(out["corr"]), _dev_p(out["scc"])),
          "orca_screen_strata_scores")
    return out


# paired aligned scores (orca_screen_paired_aligned_scores): every alt map against a reference map of its own - the readout of the SV screen
PAIRED_SCORE_FIELDS = ("profile", "abs_mean", "abs_max", "delta_mean", "rms", "corr", "count")


def _pair_bin_map(bin_map_host, B, n, device):
    """The bin maps of B pairs: (``bin_map_host`` as [B, n] int32 on the host, its device copy)."""
    m = _host_table(bin_map_host, np.int32, n, "bin map")
    if m.shape[0] != B:
        raise ValueError(f"bin map: [{B},{n}] int32, one row per pair")
    return m, torch.from_numpy(m).to(device)


def _pair_args(alt, ref, bin_map_host):
    """What the paired entry points share: (alt, alt batch stride, ref, ref batch stride, bin map [B, n] int32 on the host, its device copy)."""
    alt, ref = _f32_cuda(alt, "alt"), _f32_cuda(ref, "ref")
    if ref.shape != alt.shape or ref.device != alt.device:
        raise ValueError(f"alt, ref: [B,n,n] with B >= 1 on one device, got {tuple(alt.shape)} and {tuple(ref.shape)}")
    (alt, B, n, alt_bs), (ref, _, _, ref_bs) = _map_batch(alt, "alt"), _map_batch(ref, "ref")
    return (alt, alt_bs, ref, ref_bs) + _pair_bin_map(bin_map_host, B, n, alt.device)


def screen_paired_aligned_scores(ctx, alt, ref, bin_map_host):
    """B pairs of maps, alt [B, n, n] against ref [B, n, n] (both any batch stride, rows contiguous), pair b through row b of ``bin_map_host`` [B, n]
    int32 numpy: the reference bin alt bin i stands for, or -1 (orca_screen_paired_aligned_scores; include/orca_hip.h has the definitions).  A dict of
    device tensors: ``profile`` [B, n], ``abs_mean``, ``abs_max``, ``delta_mean``, ``rms`` [B] float32, ``corr`` [B] float64 and ``count`` [B] int32,
    the mapped bins; every float is NaN for a pair with none."""
    alt, alt_bs, ref, ref_bs, m, md = _pair_args(alt, ref, bin_map_host)
    (B, n), dev = m.shape, alt.device
    out = dict(zip(PAIRED_SCORE_FIELDS[:5], _f32_outputs(dev, (B, n), (B,), (B,), (B,), (B,))))
    out["corr"] = torch.empty(B, dtype=torch.float64, device=dev)
    out["count"] = torch.empty(B, dtype=torch.int32, device=dev)
    ctx.sync_stream()
    check(_lib.load().orca_screen_paired_aligned_scores(ctx.handle, _dev_p(alt), alt_bs, _dev_p(ref), ref_bs, B, n, _dev_p(md), _np_p(m),
                                                        *(_dev_p(out[k]) for k in PAIRED_SCORE_FIELDS)), "orca_screen_paired_aligned_scores")
    return out


# paired tracks and strata (orca_screen_paired_insulation / _viewpoints / _strata_scores): the 1 Mb screen's readouts, every alt map against a reference
# map of its own through its bin map
def screen_paired_insulation(ctx, alt, ref, widths_host, bin_map_host):
    """Insulation tracks of B pairs of maps, alt [B, n, n] against ref [B, n, n] (both any batch stride, rows contiguous) at the W widths ``widths_host``
    (1 to 8 ints, each 1 .. 128 bins) through ``bin_map_host`` [B, n] int32 numpy (orca_screen_paired_insulation): (track, ref_track, aligned), each
    [B, W, n] float32.  track = ins(alt b)[i], ref_track = ins(ref b)[i] at the reference's own bin i, aligned = ins(alt b)[i] - ins(ref b)[map i],
    NaN where alt bin i stands for no reference bin or either diamond does not fit."""
    alt, alt_bs, ref, ref_bs, m, md = _pair_args(alt, ref, bin_map_host)
    B, n = m.shape
    w = _host_list(widths_host, "widths")
    W = w.shape[0]
    wd = torch.from_numpy(w).to(alt.device)
    track, ref_track, aligned = _f32_outputs(alt.device, (B, W, n), (B, W, n), (B, W, n))
    ctx.sync_stream()
    check(_lib.load().orca_screen_paired_insulation(ctx.handle, _dev_p(alt), alt_bs, _dev_p(ref), ref_bs, B, n, _dev_p(wd), _np_p(w), W, _dev_p(md), _np_p(m),
                                                    _dev_p(track), _dev_p(ref_track), _dev_p(aligned)), "orca_screen_paired_insulation")
    return track, ref_track, aligned


def screen_paired_viewpoints(ctx, alt, ref, views_host, bin_map_host):
    """Viewpoint profiles (virtual 4C) of B pairs of maps, alt [B, n, n] against ref [B, n, n], at ``views_host`` [B, V] int32 numpy (or one [V] list for
    every pair): REFERENCE bins in -1 .. n - 1, 1 <= V <= 64, -1 = not in that pair's window (orca_screen_paired_viewpoints): (aligned [B, V, n] float32,
    count [B, V] int32).  count = the alt bins that stand for the viewpoint; aligned[b, v, j] = their mean alt row at column j minus
    ref[b][view, map j], NaN where count is 0 or column j stands for nothing."""
    alt, alt_bs, ref, ref_bs, m, md = _pair_args(alt, ref, bin_map_host)
    B, n = m.shape
    v = np.asarray(views_host)
    if v.ndim == 1:
        v = np.broadcast_to(v, (B, v.shape[0]))
    if v.ndim != 2 or v.shape[0] != B:
        raise ValueError(f"viewpoints: [{B},V] int32 (or one [V] list for all {B} pairs)")
    v = np.ascontiguousarray(v, dtype=np.int32)
    V = v.shape[1]
    vd = torch.from_numpy(v).to(alt.device)
    aligned, = _f32_outputs(alt.device, (B, V, n))
    count = torch.empty((B, V), dtype=torch.int32, device=alt.device)
    ctx.sync_stream()
    check(_lib.load().orca_screen_paired_viewpoints(ctx.handle, _dev_p(alt), alt_bs, _dev_p(ref), ref_bs, B, n, _dev_p(vd), _np_p(v), V, _dev_p(md), _np_p(m),
                                                    _dev_p(aligned), _dev_p(count)), "orca_screen_paired_viewpoints")
    return aligned, count


PAIRED_STRATA_FIELDS = ("dist_delta", "dist_abs", "dist_rms", "dist_corr", "dist_count", "mse", "corr", "scc")


def screen_paired_strata_scores(ctx, alt, ref, bin_map_host, d_range=None):
    """Distance-stratified similarity of B pairs of maps, alt [B, n, n] against ref [B, n, n] through ``bin_map_host`` [B, n] int32 numpy
    (orca_screen_paired_strata_scores): `screen_strata_scores`' dict in its aligned form - ``dist_delta``, ``dist_abs``, ``dist_rms`` [B, n] float32,
    ``dist_corr`` [B, n] float64, ``dist_count`` [B, n] int32, ``mse`` [B] float32, ``corr``, ``scc`` [B] float64 over the strata ``d_range`` =
    (d_lo, d_hi), all by default.  The reference pixel of alt pair (i, i + d) is ref[b][min(mi, mj), max(mi, mj)], mi = map i, mj = map (i + d): the
    lower side of the diagonal of neither map is read, whichever way the bin map runs."""
    alt, alt_bs, ref, ref_bs, m, md = _pair_args(alt, ref, bin_map_host)
    B, n = m.shape
    d_lo, d_hi, out = _strata_args(d_range, B, n, alt.device)
    ctx.sync_stream()
    check(_lib.load().orca_screen_paired_strata_scores(ctx.handle, _dev_p(alt), alt_bs, _dev_p(ref), ref_bs, B, n, _dev_p(md), _np_p(m), d_lo, d_hi,
                                                       *(_dev_p(out[k]) for k in PAIRED_STRATA_FIELDS)), "orca_screen_paired_strata_scores")
    return out


# loops (orca_screen_dot_calls, orca_screen_dot_enrichment): dot calls per map and the enrichment at listed pixels
def _dot_args(maps, p, w, d_min):
    return _map_batch(maps, "maps") + (int(p), int(w), 2 * int(w) + 1 if d_min is None else int(d_min))


def screen_dot_calls(ctx, maps, p, w, r, threshold, max_calls, d_min=None):
    """Dot (loop) calls on maps [B, n, n] (any batch stride, rows contiguous) of log observed / expected (orca_screen_dot_calls; include/orca_hip.h has the
    definitions): a dict of ``count`` [B] int32 (all dots of the map), ``ij`` [B, K, 2] int32 and ``enrich`` [B, K] float32 (the first K = ``max_calls``
    dots in row-major order, -1 / NaN behind them) and ``e_map`` [B, n, n] float32, the enrichment at every pixel (NaN where ineligible).  0 <= p < w <= 16,
    1 <= r <= 16, ``d_min`` >= 2 w + 1 (its default), 1 <= K <= 4096."""
    maps, B, n, bs, p, w, d_min = _dot_args(maps, p, w, d_min)
    K, dev = int(max_calls), maps.device
    e_map, enrich = _f32_outputs(dev, (B, n, n), (B, max(K, 0)))
    count = torch.empty(B, dtype=torch.int32, device=dev)
    ij = torch.empty((B, max(K, 0), 2), dtype=torch.int32, device=dev)
    ctx.sync_stream()
    check(_lib.load().orca_screen_dot_calls(ctx.handle, _dev_p(maps), bs, B, n, p, w, d_min, int(r), float(threshold), K, _dev_p(e_map), _dev_p(count), _dev_p(ij),
                                            _dev_p(enrich)), "orca_screen_dot_calls")
    return {"count": count, "ij": ij, "enrich": enrich, "e_map": e_map}


def screen_dot_enrichment(ctx, maps, pixels_host, p, w, d_min=None):
    """The enrichment e of maps [B, n, n] at the listed pixels ``pixels_host`` [B, Q, 2] int32 numpy, (i, j) per pixel, 1 <= Q <= 4096
    (orca_screen_dot_enrichment): [B, Q] float32, NaN for (-1, -1) and every other ineligible pixel, otherwise the bits of `screen_dot_calls`' ``e_map``."""
    maps, B, n, bs, p, w, d_min = _dot_args(maps, p, w, d_min)
    px = np.ascontiguousarray(pixels_host, dtype=np.int32)
    if px.ndim != 3 or px.shape[0] != B or px.shape[2] != 2:
        raise ValueError(f"pixels: [{B},Q,2] int32, one list per map")
    Q = px.shape[1]
    out, = _f32_outputs(maps.device, (B, Q))
    pd = torch.from_numpy(px).to(maps.device)
    ctx.sync_stream()
    check(_lib.load().orca_screen_dot_enrichment(ctx.handle, _dev_p(maps), bs, B, n, p, w, d_min, _dev_p(pd), _np_p(px), Q, _dev_p(out)), "orca_screen_dot_enrichment")
    return out


def screen_paired_dot_follow(ctx, alt_e, ref_ij, ref_enrich, bin_map_host, w, d_min=None):
    """The reference dots of B pairs followed through each pair's bin map into the alt map (orca_screen_paired_dot_follow; include/orca_hip.h has the
    rule).  ``alt_e`` [B, n, n] float32 (any batch stride, rows contiguous): `screen_dot_calls`' ``e_map`` of the alt maps; ``ref_ij`` [B, R, 2] int32 and
    ``ref_enrich`` [B, R] float32: its ``ij`` and ``enrich`` of the reference maps, device tensors as it returned them (a slot that is no dot, 0 <= ri < rj
    <= n - 1, is empty); ``bin_map_host`` [B, n] int32 numpy.  A dict of device tensors: ``candidates`` [B, R] int32 (the eligible alt pixels that stand for
    the dot), ``at`` [B, R, 2] int32 (the one with the largest e, the earlier of equals; (-1, -1) without a candidate), ``enrich`` [B, R] float32 (e there)
    and ``delta`` [B, R] float32 (e there minus the reference dot's e), NaN without a candidate."""
    alt_e, B, n, e_bs = _map_batch(alt_e, "alt_e")
    ref_ij, ref_enrich = _on_device(ref_ij, "ref_ij", torch.int32), _on_device(ref_enrich, "ref_enrich", torch.float32)
    if ref_ij.dim() != 3 or ref_ij.shape[0] != B or ref_ij.shape[2] != 2 or ref_enrich.shape != ref_ij.shape[:2] or ref_ij.device != alt_e.device \
            or ref_enrich.device != alt_e.device:
        raise ValueError(f"ref_ij: [{B},R,2] int32 and ref_enrich: [{B},R] float32 on the maps' device")
    R, dev = ref_ij.shape[1], alt_e.device
    m, md = _pair_bin_map(bin_map_host, B, n, dev)
    w = int(w)
    d_min = 2 * w + 1 if d_min is None else int(d_min)
    enrich, delta = _f32_outputs(dev, (B, R), (B, R))
    candidates = torch.empty((B, R), dtype=torch.int32, device=dev)
    at = torch.empty((B, R, 2), dtype=torch.int32, device=dev)
    ctx.sync_stream()
    check(_lib.load().orca_screen_paired_dot_follow(ctx.handle, _dev_p(alt_e), e_bs, B, n, w, d_min, _dev_p(ref_ij), _dev_p(ref_enrich), R, _dev_p(md), _np_p(m),
                                                    _dev_p(candidates), _dev_p(at), _dev_p(enrich), _dev_p(delta)), "orca_screen_paired_dot_follow")
    return {"candidates": candidates, "at": at, "enrich": enrich, "delta": delta}


# boundaries (orca_screen_boundary_calls): domain boundary calls from insulation tracks that are on the device already
def screen_boundary_calls(ctx, tracks, min_strength, max_calls, strength_track=True):
    """Domain boundary calls on insulation tracks [B, W, n] float32 on the device (`screen_insulation`'s or `screen_paired_insulation`'s, contiguous;
    orca_screen_boundary_calls, include/orca_hip.h has the definitions): a dict of ``count`` [B, W] int32 (all boundaries of the track), ``bins`` [B, W, K]
    int32 and ``strength`` [B, W, K] float32 (the first K = ``max_calls`` boundaries in ascending bin order, -1 / NaN behind them) and, unless
    ``strength_track`` is False (then None), ``strength_track`` [B, W, n] float32: the strength at every minimum with strength > 0, NaN elsewhere.
    B >= 1, 1 <= W <= 8, 3 <= n <= 256, ``min_strength`` >= 0, 0 <= K <= n."""
    tracks = _on_device(_f32_cuda(tracks, "tracks"), "tracks", torch.float32)
    if tracks.dim() != 3:
        raise ValueError(f"tracks: [B,W,n] float32, got {tuple(tracks.shape)}")
    (B, W, n), K, dev = tracks.shape, int(max_calls), tracks.device
    count = torch.empty((B, W), dtype=torch.int32, device=dev)
    bins = torch.empty((B, W, max(K, 0)), dtype=torch.int32, device=dev)
    strength, = _f32_outputs(dev, (B, W, max(K, 0)))
    st = _f32_outputs(dev, (B, W, n))[0] if strength_track else None
    spare = torch.empty(2, dtype=torch.int32, device=dev)    # K = 0: the lists are empty, and the entry point takes no NULL for them
    ctx.sync_stream()
    check(_lib.load().orca_screen_boundary_calls(ctx.handle, _dev_p(tracks), B, W, n, float(min_strength), K, _dev_p(count), _dev_p(bins if K else spare[:1]),
                                                 _dev_p(strength if K else spare[1:]), ctypes.c_void_p(0) if st is None else _dev_p(st)),
          "orca_screen_boundary_calls")
    return {"count": count, "bins": bins, "strength": strength, "strength_track": st}


# compartments (orca_screen_eigenvectors, orca_screen_gc_tracks): the leading eigenpairs of maps and the GC track that phases them
def screen_eigenvectors(ctx, maps, n_eigs=1, d_lo=2, center=True, tol=1e-8, max_iter=1000, phase=None):
    """The ``n_eigs`` (1..3) leading eigenpairs of maps [B, n, n] (any batch stride, rows contiguous; n <= 256), one map per workgroup
    (orca_screen_eigenvectors; include/orca_hip.h has the definition: the symmetrised upper triangle, the valid bins, A = S - mean on the kept pixels
    |i - j| >= ``d_lo``, E_k = v_k sqrt(|lambda_k|), descending |lambda|).  ``phase``: [B, n] float32 on the device (or None) - the sign makes E_k's
    correlation with it non-negative; without it the component of largest |E_k| is positive.  A dict of device tensors: ``E`` [B, K, n] float32 (NaN on
    invalid bins), ``eigenvalue``, ``residual`` [B, K] float64 (the relative residual reached: converged means <= ``tol``), ``iterations`` [B, K] int32
    and ``n_valid`` [B] int32; a map with n_valid <= K is all NaN."""
    maps, B, n, bs = _map_batch(maps, "maps")
    K, dev = int(n_eigs), maps.device
    if phase is not None:
        phase = _on_device(phase, "phase", torch.float32)
        if tuple(phase.shape) != (B, n) or phase.device != dev:
            raise ValueError(f"phase: [{B},{n}] float32 on the maps' device")
    E, = _f32_outputs(dev, (B, max(K, 0), n))
    eigenvalue, residual = (torch.empty((B, max(K, 0)), dtype=torch.float64, device=dev) for _ in range(2))
    iterations = torch.empty((B, max(K, 0)), dtype=torch.int32, device=dev)
    n_valid = torch.empty(B, dtype=torch.int32, device=dev)
    ctx.sync_stream()
    check(_lib.load().orca_screen_eigenvectors(ctx.handle, _dev_p(maps), bs, B, n, K, int(d_lo), int(bool(center)), float(tol), int(max_iter),
                                               None if phase is None else _dev_p(phase), _dev_p(E), _dev_p(eigenvalue), _dev_p(residual), _dev_p(iterations),
                                               _dev_p(n_valid)), "orca_screen_eigenvectors")
    return {"E": E, "eigenvalue": eigenvalue, "residual": residual, "iterations": iterations, "n_valid": n_valid}


def gc_tracks(ctx, codes, offsets, binsizes, n):
    """GC content per bin of W windows of ``codes`` [L] uint8 on the device (0..3 = A, C, G, T, 4 = N): window w has ``n`` bins of ``binsizes[w]`` bases
    from base ``offsets[w]`` (host sequences of W ints).  [W, n] float32 on the device: #{C, G} / #{A, C, G, T} per bin, NaN where the bin holds no
    A/C/G/T (orca_screen_gc_tracks).  A window that leaves [0, L) is an OrcaHipError."""
    codes = _on_device(codes, "codes", torch.uint8)
    if codes.dim() != 1:
        raise ValueError("codes: [L] uint8")
    off, bs = np.ascontiguousarray(offsets, dtype=np.int64).reshape(-1), np.ascontiguousarray(binsizes, dtype=np.int64).reshape(-1)
    if off.size < 1 or bs.size != off.size:
        raise ValueError("offsets, binsizes: one int64 each per window, at least one window")
    W, n = off.size, int(n)
    out, = _f32_outputs(codes.device, (W, max(n, 0)))
    ctx.sync_stream()
    check(_lib.load().orca_screen_gc_tracks(ctx.handle, _dev_p(codes), codes.numel(), _np_p(off), _np_p(bs), W, n, _dev_p(out)), "orca_screen_gc_tracks")
    return out


# both strands (orca_screen_merge_strands)
def screen_merge_strands(ctx, fwd, rev, ref_fwd=None, ref_rev=None, out=None):
    """The '+' strand's maps ``fwd`` [B, n, n] and the '-' strand's ``rev`` [B, n, n] (any batch stride, rows contiguous) merged as genomepredict merges
    them (orca_screen_merge_strands): (out [B, n, n] = 0.5 fwd + 0.5 rev.flip(-1, -2), gap [B] or None).  With both strands' reference maps ``ref_fwd``,
    ``ref_rev`` [n, n], gap[b] = mean |(fwd[b] - ref_fwd) - (rev[b] - ref_rev).flip(-1, -2)|; without them it is None.  ``out`` may be ``fwd`` itself (merged
    in place); it must not overlap ``rev``."""
    if (ref_fwd is None) != (ref_rev is None):
        raise ValueError("ref_fwd and ref_rev: both strands' reference maps, or neither")
    fwd, rev = _f32_cuda(fwd, "fwd"), _f32_cuda(rev, "rev")
    if fwd.dim() != 3 or fwd.shape[0] < 1 or fwd.shape[1] != fwd.shape[2] or not 1 <= fwd.shape[1] <= SCREEN_ALIGNED_MAX_BINS:
        raise ValueError(f"fwd: [B,n,n] with B >= 1 and 1 <= n <= {SCREEN_ALIGNED_MAX_BINS}, got {tuple(fwd.shape)}")
    B, n = fwd.shape[0], fwd.shape[1]
    if out is None:
        out = torch.empty((B, n, n), dtype=torch.float32, device=fwd.device)
    elif not (isinstance(out, torch.Tensor) and out.dtype == torch.float32):
        raise ValueError("out: a float32 tensor (it is written in place)")
    for t, name in ((fwd, "fwd"), (rev, "rev"), (out, "out")):
        if tuple(t.shape) != (B, n, n) or t.stride(2) != 1 or t.stride(1) != n or (B > 1 and t.stride(0) < n * n) or t.device != fwd.device:
            raise ValueError(f"{name}: [{B},{n},{n}] float32 beside fwd with contiguous maps and a batch stride >= {n * n}")
    refs = []
    for t, name in ((ref_fwd, "ref_fwd"), (ref_rev, "ref_rev")):
        if t is not None:
            t = _f32_cuda(t, name).contiguous()
            if tuple(t.shape) != (n, n) or t.device != fwd.device:
                raise ValueError(f"{name}: [{n},{n}] beside fwd")
        refs.append(t)
    gap = None if refs[0] is None else torch.empty(B, dtype=torch.float32, device=fwd.device)
    bs = [_map_batch(t, name)[3] for t, name in ((fwd, "fwd"), (rev, "rev"), (out, "out"))]
    null = ctypes.c_void_p(0)
    ctx.sync_stream()
    check(_lib.load().orca_screen_merge_strands(ctx.handle, _p(fwd), bs[0], _p(rev), bs[1], null if refs[0] is None else _p(refs[0]),
                                                null if refs[1] is None else _p(refs[1]), B, n, _p(out), bs[2], null if gap is None else _p(gap)),
          "orca_screen_merge_strands")
    return out, gap


# the chromosome scan (orca_scan_*; scan.scan_1m): window maps stitched into a band [N, D] - band[i, d] stands for pixel (i, i + d) - the band's insulation
# tracks, and boundary strengths on tracks of any length.  include/orca_hip.h has the definitions; no arena, every buffer is a torch tensor
def scan_accumulators(device, N, D):
    """Fresh accumulators of a band of ``N`` bins x ``D`` distances for `scan_stitch_band`: a dict of ``sum`` [N, D] float64 = 0, ``count`` [N, D]
    int32 = 0, ``lo`` [N, D] float32 = +inf and ``hi`` [N, D] float32 = -inf on ``device``."""
    N, D = int(N), int(D)
    if N < 1 or D < 1:
        raise ValueError(f"a band of {N} bins x {D} distances: at least one of each")
    return {"sum": torch.zeros((N, D), dtype=torch.float64, device=device), "count": torch.zeros((N, D), dtype=torch.int32, device=device),
            "lo": torch.full((N, D), float("inf"), dtype=torch.float32, device=device),
            "hi": torch.full((N, D), float("-inf"), dtype=torch.float32, device=device)}


def _scan_acc(acc, device=None):
    """The four accumulators of a band as (sum, count, lo, hi, N, D), each a contiguous [N, D] tensor of its type on one device."""
    try:
        ts = [_on_device(acc[k], k, d) for k, d in (("sum", torch.float64), ("count", torch.int32), ("lo", torch.float32), ("hi", torch.float32))]
    except (KeyError, TypeError, IndexError):
        raise ValueError("acc: the dict of sum, count, lo and hi that scan_accumulators made") from None
    if ts[0].dim() != 2 or any(t.shape != ts[0].shape or t.device != ts[0].device for t in ts) or (device is not None and ts[0].device != device):
        raise ValueError("acc: sum, count, lo and hi are [N, D] on the maps' device")
    return ts + [ts[0].shape[0], ts[0].shape[1]]


def scan_stitch_band(ctx, maps, off_host, trim, acc, off=None):
    """One batch of window maps [B, n, n] (any batch stride, rows contiguous; n <= 256) accumulated into the band ``acc`` (`scan_accumulators`;
    orca_scan_stitch_band): ``off_host`` [B] int64 numpy, the chromosome bin every window starts at, strictly ascending, 0 <= off <= N - n (``off``: its
    device copy, uploaded here when None); window b covers band pixel (i, d) when r = i - off[b] has ``trim`` <= r and r + d <= n - 1 - trim, and adds
    maps[b, r, r + d] to ``sum`` in fp64, 1 to ``count`` and the value to the running ``lo`` / ``hi``; a NaN stays.  1 <= D <= n - 2 trim.  Calls
    continue the same accumulators: a window list split into batches at any point gives the same bits as one call."""
    maps, B, n, bs = _map_batch(maps, "maps")
    s, c, lo, hi, N, D = _scan_acc(acc, maps.device)
    o = np.ascontiguousarray(off_host, dtype=np.int64).reshape(-1)
    if o.size != B:
        raise ValueError(f"off_host: one int64 per map ({B}), got {o.size}")
    od = torch.from_numpy(o).to(maps.device) if off is None else _on_device(off, "off", torch.int64)
    if tuple(od.shape) != (B,) or od.device != maps.device:
        raise ValueError("off: the device copy of off_host")
    ctx.sync_stream()
    check(_lib.load().orca_scan_stitch_band(ctx.handle, _dev_p(maps), bs, B, n, _dev_p(od), _np_p(o), int(trim), N, D, _dev_p(s), _dev_p(c), _dev_p(lo),
                                            _dev_p(hi)), "orca_scan_stitch_band")


def scan_band_finish(ctx, acc, spread=True):
    """The accumulators ``acc`` of a band into (band [N, D], range [N, D] or None) float32 (orca_scan_band_finish): band = (float)(sum / count), the
    fp64 quotient rounded once, NaN where no window covers the pixel and where i + d >= N; with ``spread`` range = hi - lo, how far the overlapping
    windows disagree about the pixel (0 under one window, NaN under none)."""
    s, c, lo, hi, N, D = _scan_acc(acc)
    band, = _f32_outputs(s.device, (N, D))
    rng = _f32_outputs(s.device, (N, D))[0] if spread else None
    ctx.sync_stream()
    check(_lib.load().orca_scan_band_finish(ctx.handle, _dev_p(s), _dev_p(c), _dev_p(lo), _dev_p(hi), N, D, _dev_p(band),
                                            ctypes.c_void_p(0) if rng is None else _dev_p(rng)), "orca_scan_band_finish")
    return band, rng


def scan_band_insulation(ctx, band, widths_host):
    """Insulation tracks [W, N] float32 of a band [N, D] (`scan_band_finish`'s) at the W widths ``widths_host`` (1 to 8 distinct ints, 1 <= w and
    2 w + 1 <= D; orca_scan_band_insulation): track[k, i] = the fp64 mean of the w^2 pixels rows [i - w, i) x columns (i, i + w] of the dense map the band
    stands for, read as band[r, c - r]; NaN where the diamond does not fit (i < w or i >= N - w) or holds a NaN - `screen_insulation`'s definition."""
    band = _on_device(_f32_cuda(band, "band"), "band", torch.float32)
    if band.dim() != 2 or band.shape[0] < 1 or band.shape[1] < 1:
        raise ValueError(f"band: [N, D] float32, got {tuple(band.shape)}")
    N, D = band.shape
    w = _host_list(widths_host, "widths")
    wd = torch.from_numpy(w).to(band.device)
    track, = _f32_outputs(band.device, (w.shape[0], N))
    ctx.sync_stream()
    check(_lib.load().orca_scan_band_insulation(ctx.handle, _dev_p(band), N, D, _dev_p(wd), _np_p(w), w.shape[0], _dev_p(track)), "orca_scan_band_insulation")
    return track


def scan_boundary_strength(ctx, tracks):
    """Boundary strengths [W, N] float32 of insulation tracks [W, N] float32 on the device, contiguous, of ANY length N >= 1
    (orca_scan_boundary_strength): `screen_boundary_calls`' ``strength_track`` bit for bit - the prominence of the dip at every minimum where it is > 0,
    NaN elsewhere; a NaN ends a walk - without its limit of 256 bins.  The ordered lists are made from it on the host."""
    tracks = _on_device(_f32_cuda(tracks, "tracks"), "tracks", torch.float32)
    if tracks.dim() != 2:
        raise ValueError(f"tracks: [W, N] float32, got {tuple(tracks.shape)}")
    W, N = tracks.shape
    out, = _f32_outputs(tracks.device, (W, N))
    ctx.sync_stream()
    check(_lib.load().orca_scan_boundary_strength(ctx.handle, _dev_p(tracks), W, N, _dev_p(out)), "orca_scan_boundary_strength")
    return out


# loops along the band (orca_scan_band_dot_*; scan.scan_1m(..., loops=)): the enrichment band, then ALL its dots as one ordered list
SCAN_LOOP_ROWS = 32             # band rows per workgroup of the enrichment kernel (orca_amd/csrc/scan_loops.h); no result depends on it


def _band(t, name):
    t = _on_device(_f32_cuda(t, name), name, torch.float32)
    if t.dim() != 2 or t.shape[0] < 1 or t.shape[1] < 1:
        raise ValueError(f"{name}: [N, D] float32, got {tuple(t.shape)}")
    return t, t.shape[0], t.shape[1]


def scan_band_dot_enrichment(ctx, band, p, w, d_min=None):
    """The enrichment band [N, D] float32 of a band [N, D] (`scan_band_finish`'s; 2 <= D <= 256; orca_scan_band_dot_enrichment): e[i, d] =
    `screen_dot_calls`' enrichment of the dense map the band stands for at pixel (i, i + d), NaN where any pixel of the window is NaN and at every
    ineligible pixel - eligible: w <= i, i + d <= N - 1 - w and ``d_min`` <= d <= D - 1 - 2 w.  0 <= p < w <= 16, ``d_min`` >= 2 w + 1 (its default)."""
    band, N, D = _band(band, "band")
    p, w = int(p), int(w)
    d_min = 2 * w + 1 if d_min is None else int(d_min)
    e_band, = _f32_outputs(band.device, (N, D))
    ctx.sync_stream()
    check(_lib.load().orca_scan_band_dot_enrichment(ctx.handle, _dev_p(band), N, D, p, w, d_min, _dev_p(e_band)), "orca_scan_band_dot_enrichment")
    return e_band


def scan_band_dot_calls(ctx, e_band, r, threshold):
    """ALL dots of an enrichment band [N, D] (`scan_band_dot_enrichment`'s) in ascending (i, d) order, on the device: (ij [L, 2] int64, the pixel
    (i, i + d); enrich [L] float32, its e).  (i, d) is a dot when e is not NaN, e >= ``threshold`` and e wins against every neighbour
    e_band[i + di, d + dj - di], |di|, |dj| <= ``r``, that exists and is not NaN: e > e' where the neighbour comes first in (i, d) order, e >= e' where
    it follows (include/orca_hip.h).  orca_scan_band_dot_offsets counts the dots per row and prefixes the counts, L comes to the host (one 8-byte
    copy), and orca_scan_band_dot_list writes the lists; with L = 0 nothing more is launched."""
    e_band, N, D = _band(e_band, "e_band")
    dev = e_band.device
    row_start = torch.empty(N + 1, dtype=torch.int64, device=dev)
    ctx.sync_stream()
    check(_lib.load().orca_scan_band_dot_offsets(ctx.handle, _dev_p(e_band), N, D, int(r), float(threshold), _dev_p(row_start)), "orca_scan_band_dot_offsets")
    L = int(row_start[N].item())
    ij = torch.empty((L, 2), dtype=torch.int64, device=dev)
    enrich, = _f32_outputs(dev, (L,))
    if L:
        check(_lib.load().orca_scan_band_dot_list(ctx.handle, _dev_p(e_band), N, D, int(r), float(threshold), _dev_p(row_start), L, _dev_p(ij), _dev_p(enrich)),
              "orca_scan_band_dot_list")
    return ij, enrich


def encoder_forward_2bit(net, two, nmask, start, L, reverse=False, bin_lo=0, bin_hi=0, chunk_bp=0, out=None):
    """Encoder on bases [start, start + L) of a chromosome stored as 2 bits per base + N mask in HBM (genome.TwoBitGenome planes): no
    unpacked window is made (orca_encoder_forward_2bit).  Returns [1,128,bins]."""
    if not (two.is_cuda and nmask.is_cuda and two.dtype == torch.uint8 and nmask.dtype == torch.uint8 and two.is_contiguous() and nmask.is_contiguous()):
        raise ValueError("two / nmask: contiguous uint8 ROCm tensors")
    if start < 0 or (start + L + 3) // 4 > two.numel() or (start + L + 7) // 8 > nmask.numel():
        raise ValueError("2-bit window outside the chromosome")
    total = encoder_num_bins(L)
    hi = total if bin_hi <= 0 else bin_hi
    if out is None:
        out = torch.empty((1, 128, hi - bin_lo), dtype=torch.float32, device=two.device)
    elif tuple(out.shape) != (1, 128, hi - bin_lo) or out.stride(2) != 1:
        raise ValueError(f"out must be a [1,128,{hi - bin_lo}] view with unit stride along the bins")
    net.ctx.sync_stream()
    check(_lib.load().orca_encoder_forward_2bit(net.ctx.handle, net.handle, _p(two), _p(nmask), int(start), 1 if reverse else 0, int(L), bin_lo, hi,
                                                _p(out), out.stride(1), chunk_bp), "orca_encoder_forward_2bit")
    return out


def unet_forward(net, x, nlev):
    x = _f32_cuda(x, "x")
    if x.dim() != 3 or x.shape[1] != 128:
        raise ValueError(f"Encoder2/3 input must be [B,128,n], got {tuple(x.shape)}")
    B, _, n = x.shape
    outs = [torch.empty((B, 128, n >> i), dtype=torch.float32, device=x.device) for i in range(nlev + 1)]
    ptrs = (ctypes.c_void_p * (nlev + 1))(*[o.data_ptr() for o in outs])
    net.ctx.sync_stream()
    check(_lib.load().orca_unet_forward(net.ctx.handle, net.handle, _p(x), x.stride(0), x.stride(1), x.stride(2), B, n, ptrs,
                                        nlev + 1), "orca_unet_forward")
    return outs


def decoder_forward(net, x, distenc, y=None, out=None, accumulate=False):
    """x [B,128,n]; distenc [B or 1, T, n, n]; y None or [B,T,n/2,n/2]; returns / fills [B,T,n,n]
    (T = the net's number of target maps: 1 for the Orca models, num_2d for the orca_leukemia decoders)."""
    x = _f32_cuda(x, "x")
    distenc = _f32_cuda(distenc, "distenc")
    B, C, n = x.shape
    T = net.num_targets()
    if C != 128:
        raise ValueError(f"Decoder input must be [B,128,n], got {tuple(x.shape)}")
    if distenc.dim() != 4 or distenc.shape[1] != T or distenc.shape[2] != n or distenc.shape[3] != n:
        raise ValueError(f"distenc must be [B,{T},{n},{n}], got {tuple(distenc.shape)}")
    if distenc.shape[0] not in (1, B):
        raise ValueError("distenc batch mismatch")
    sd_b = distenc.stride(0) if distenc.shape[0] == B else 0
    yp, sy = ctypes.c_void_p(0), (0, 0, 0, 0)
    if y is not None:
        y = _f32_cuda(y, "y")
        if tuple(y.shape) != (B, T, n // 2, n // 2):
            raise ValueError(f"coarse prediction must be [{B},{T},{n // 2},{n // 2}], got {tuple(y.shape)}")
        yp, sy = _p(y), (y.stride(0), y.stride(1), y.stride(2), y.stride(3))
    if out is None:
        out = torch.empty((B, T, n, n), dtype=torch.float32, device=x.device)
        accumulate = False
    elif tuple(out.shape) != (B, T, n, n) or not out.is_contiguous():
        raise ValueError(f"out must be a contiguous [{B},{T},{n},{n}] tensor")
    net.ctx.sync_stream()
    if T == 1:
        check(_lib.load().orca_decoder_forward(net.ctx.handle, net.handle, _p(x), x.stride(0), x.stride(1), x.stride(2), _p(distenc),
                                               sd_b, distenc.stride(2), distenc.stride(3), yp, sy[0], sy[2], sy[3], B, n, _p(out),
                                               1 if accumulate else 0), "orca_decoder_forward")
    else:
        check(_lib.load().orca_decoder_forward_mt(net.ctx.handle, net.handle, _p(x), x.stride(0), x.stride(1), x.stride(2),
                                                  _p(distenc), sd_b, distenc.stride(1), distenc.stride(2), distenc.stride(3), yp,
                                                  sy[0], sy[1], sy[2], sy[3], B, n, _p(out), 1 if accumulate else 0),
              "orca_decoder_forward_mt")
    return out


def _row_ptrs(rows):
    return (ctypes.c_void_p * len(rows))(*[r.data_ptr() for r in rows])


def _same_strides(rows, name):
    st = rows[0].stride()
    if any(r.stride() != st or r.shape != rows[0].shape for r in rows):
        raise ValueError(f"{name}: the rows of a batch must share one shape and one set of strides")
    return st


def decoder_forward_rows(net, xs, des, ys=None, out=None, accumulate=False):
    """Decoder on a batch given ROW BY ROW: xs = B views [128,n], des = B views [T,n,n] (the same view may repeat),
    ys = None or B views [T,n/2,n/2] - any strides, no copies (orca_decoder_forward_rows)."""
    xs = [_f32_cuda(t, "x") for t in xs]
    des = [_f32_cuda(t, "distenc") for t in des]
    B, T = len(xs), net.num_targets()
    C, n = xs[0].shape
    if C != 128 or tuple(des[0].shape) != (T, n, n) or len(des) != B:
        raise ValueError(f"decoder rows: x [128,n] and distenc [{T},n,n] per row, got {tuple(xs[0].shape)} / {tuple(des[0].shape)}")
    sx, sd = _same_strides(xs, "x"), _same_strides(des, "distenc")
    yp, sy = None, (0, 0, 0)
    if ys is not None:
        ys = [_f32_cuda(t, "y") for t in ys]
        if len(ys) != B or tuple(ys[0].shape) != (T, n // 2, n // 2):
            raise ValueError(f"coarse prediction rows must be [{T},{n // 2},{n // 2}]")
        yp, sy = _row_ptrs(ys), _same_strides(ys, "y")
    if out is None:
        out = torch.empty((B, T, n, n), dtype=torch.float32, device=xs[0].device)
        accumulate = False
    net.ctx.sync_stream()
    check(_lib.load().orca_decoder_forward_rows(net.ctx.handle, net.handle, _row_ptrs(xs), sx[0], sx[1], _row_ptrs(des), sd[0], sd[1], sd[2],
                                                yp, sy[0], sy[1], sy[2], B, n, _p(out), 1 if accumulate else 0), "orca_decoder_forward_rows")
    return out


def decoder1m_forward_rows(net, xs, out=None, accumulate=False):
    xs = [_f32_cuda(t, "x") for t in xs]
    B, T = len(xs), net.num_targets()
    C, n = xs[0].shape
    sx = _same_strides(xs, "x")
    if out is None:
        out = torch.empty((B, T, n, n), dtype=torch.float32, device=xs[0].device)
        accumulate = False
    net.ctx.sync_stream()
    check(_lib.load().orca_decoder1m_forward_rows(net.ctx.handle, net.handle, _row_ptrs(xs), sx[0], sx[1], B, n, _p(out), 1 if accumulate else 0),
          "orca_decoder1m_forward_rows")
    return out


def decoder1m_forward(net, x, out=None, accumulate=False):
    x = _f32_cuda(x, "x")
    B, C, n = x.shape
    T = net.num_targets()
    if C != 128:
        raise ValueError(f"Decoder_1m input must be [B,128,n], got {tuple(x.shape)}")
    if out is None:
        out = torch.empty((B, T, n, n), dtype=torch.float32, device=x.device)
        accumulate = False
    elif tuple(out.shape) != (B, T, n, n) or not out.is_contiguous():
        raise ValueError(f"out must be a contiguous [{B},{T},{n},{n}] tensor")
    net.ctx.sync_stream()
    check(_lib.load().orca_decoder1m_forward(net.ctx.handle, net.handle, _p(x), x.stride(0), x.stride(1), x.stride(2), B, n,
                                             _p(out), 1 if accumulate else 0), "orca_decoder1m_forward")
    return out


def decoder_probe(net, x, distenc, y, stage):
    """Test entry (orca_decoder_probe): the Decoder / Decoder_1m forward of ``net`` stopped behind the launches that complete ``stage``;
    returns that feature map as fp32 [B,C,n,n].  Stages: 0 = IN (16 channels; Decoder_1m 128), 1 = after lcombinerD's first conv, 2 = A
    (80 channels with y, else 64), 3 + i = the residual stream after block i.  A Decoder_1m takes distenc = y = None.  An exact-fp32 net hands
    out what its fp32 maps hold: stage 0 of a Decoder is the whole 136-channel input map (x_i + x_j, distenc, zeros), A with y has 72."""
    x = _f32_cuda(x, "x")
    B, C, n = x.shape
    if C != 128:
        raise ValueError(f"Decoder input must be [B,128,n], got {tuple(x.shape)}")
    is1m = net.kind == _lib.ORCA_NET_DECODER_1M
    T = net.num_targets()
    dp, sd, yp, sy = ctypes.c_void_p(0), (0, 0, 0, 0), ctypes.c_void_p(0), (0, 0, 0, 0)
    if distenc is not None:
        distenc = _f32_cuda(distenc, "distenc")
        if distenc.dim() != 4 or tuple(distenc.shape[1:]) != (T, n, n) or distenc.shape[0] not in (1, B):
            raise ValueError(f"distenc must be [B or 1,{T},{n},{n}], got {tuple(distenc.shape)}")
        dp, sd = _p(distenc), (distenc.stride(0) if distenc.shape[0] == B else 0, distenc.stride(1), distenc.stride(2), distenc.stride(3))
    if y is not None:
        y = _f32_cuda(y, "y")
        if tuple(y.shape) != (B, T, n // 2, n // 2):
            raise ValueError(f"coarse prediction must be [{B},{T},{n // 2},{n // 2}], got {tuple(y.shape)}")
        yp, sy = _p(y), (y.stride(0), y.stride(1), y.stride(2), y.stride(3))
    f32 = net.precision == "f32"
    channels = (128 if is1m else 136 if f32 else 16) if stage == 0 else ((72 if f32 else 80) if stage == 2 and y is not None else 64)
    out = torch.empty((B, channels, n, n), dtype=torch.float32, device=x.device)
    net.ctx.sync_stream()
    check(_lib.load().orca_decoder_probe(net.ctx.handle, net.handle, _p(x), x.stride(0), x.stride(1), x.stride(2), dp, *sd, yp, *sy, B, n,
                                         int(stage), channels, _p(out)), "orca_decoder_probe")
    return out


def encoder_probe(net, codes=None, x=None, reverse=False, stage=7):
    """Test entry (orca_encoder_probe): stages 1..``stage`` of the route `encoder_forward` / `encoder_forward_codes` take for ``net`` (its
    precision and form decide it) on ONE whole sequence - ``codes`` [L] uint8 (``reverse``: its reverse complement) or float rows ``x`` [4, L]
    (any strides) - and what the route leaves behind that stage: (fp32 [n_out, C], pool), pool = the MaxPool1d already applied to it (1, 4, 5)."""
    if (codes is None) == (x is None):
        raise ValueError("encoder_probe: exactly one of codes and x")
    if codes is not None:
        codes = _codes1d(codes)
        L, dev, cp, xp, sx = codes.numel(), codes.device, _p(codes), ctypes.c_void_p(0), (0, 0)
    else:
        x = _f32_cuda(x, "x")
        if x.dim() != 2 or x.shape[0] != 4:
            raise ValueError(f"encoder_probe: float rows must be [4,L], got {tuple(x.shape)}")
        L, dev, cp, xp, sx = x.shape[1], x.device, ctypes.c_void_p(0), _p(x), (x.stride(0), x.stride(1))
    n = L
    for pool in (4, 4, 5, 5, 5, 2)[: max(0, int(stage) - 1)]:
        n //= pool
    buf = torch.empty(max(1, n * 128), dtype=torch.float32, device=dev)
    n_out, C, pl = ctypes.c_int64(0), ctypes.c_int(0), ctypes.c_int(0)
    net.ctx.sync_stream()
    check(_lib.load().orca_encoder_probe(net.ctx.handle, net.handle, cp, 1 if reverse else 0, xp, *sx, L, int(stage), _p(buf), buf.numel(),
                                         ctypes.byref(n_out), ctypes.byref(C), ctypes.byref(pl)), "orca_encoder_probe")
    return buf[: n_out.value * C.value].view(n_out.value, C.value), int(pl.value)


def strand_merge(fwd, rev):
    """0.5*fwd + 0.5*rev[::-1, ::-1] for contiguous [n,n] maps (orca_predict.py:514-523)."""
    fwd, rev = _f32_cuda(fwd, "fwd").contiguous(), _f32_cuda(rev, "rev").contiguous()
    n = fwd.shape[-1]
    out = torch.empty_like(fwd)
    ctx = get_context(fwd.device)
    check(_lib.load().orca_strand_merge(ctx.handle, _p(fwd), _p(rev), _p(out), n), "orca_strand_merge")
    return out


def block_mean(normmat, start, nb, npix=250, flip=False, want_mean=True):
    """Background of one level of the 256 Mb cascade on the device (orca_predict.py:724-737, :692-703): block means of the
    window [start, start + npix*nb)^2 of a float64 CUDA matrix -> (float64 [npix,npix] means or None, float32 [1,1,npix,npix]
    log-background, flipped in both axes if ``flip``).  The means are bit-identical to numpy's nanmean-of-nanmean."""
    if not (normmat.is_cuda and normmat.dtype == torch.float64 and normmat.dim() == 2 and normmat.stride(1) == 1):
        raise OrcaHipError("block_mean: a float64 [n,n] ROCm tensor with unit column stride is required")
    if start < 0 or start + npix * nb > min(normmat.shape):
        raise ValueError(f"block_mean: window [{start}, {start + npix * nb}) outside the {tuple(normmat.shape)} background")
    ctx = get_context(normmat.device)
    ctx.sync_stream()
    mean = torch.empty((npix, npix), dtype=torch.float64, device=normmat.device) if want_mean else None
    logt = torch.empty((1, 1, npix, npix), dtype=torch.float32, device=normmat.device)
    check(_lib.load().orca_block_mean_f64(ctx.handle, _p(normmat), normmat.stride(0), int(start), int(start), int(nb), int(npix),
                                          _p(mean) if mean is not None else None, _p(logt), 1 if flip else 0), "orca_block_mean_f64")
    return mean, logt


# ---- single layers (kernel unit tests) -------------------------------------
def conv1d(x, w, b, relu=False, r1=None, r2=None, tile=0):
    """y = [relu](conv1d_k9(x, w) + b) [+ r1] [+ r2]; x [B,cin,n] contiguous cuda."""
    x = _f32_cuda(x, "x").contiguous()
    B, cin, n = x.shape
    w = np.ascontiguousarray(w, dtype=np.float32)
    b = np.ascontiguousarray(b, dtype=np.float32)
    cout = w.shape[0]
    d = make_descs([{"w": w, "b": b, "cout": cout, "cin": cin, "k": 9, "dil": 1}])
    y = torch.empty((B, cout, n), dtype=torch.float32, device=x.device)
    ctx = get_context(x.device)
    r1 = r1.contiguous() if r1 is not None else None
    r2 = r2.contiguous() if r2 is not None else None
    check(_lib.load().orca_conv1d_forward(ctx.handle, d, _p(x), cin * n, n, _p(y), cout * n, n,
                                          _p(r1) if r1 is not None else None, _p(r2) if r2 is not None else None, B, n,
                                          1 if relu else 0, tile), "orca_conv1d_forward")
    return y


def conv1d_nlc(x, w, b, precision="bf16x3", relu=False, r1=None, r2=None, inplace=False, pool4=False, fixed_tile=0):
    """channel-last split-operand conv: x [B,n,cin] -> [B,n,cout] (pool4: MaxPool1d(4) fused, [B,n//4,cout]).  r2: a second residual
    [B,n,cout]; inplace: it is copied into the output buffer and that buffer is passed as both (the U-net encoders' skip connection).
    fixed_tile: the tile rule of the long 128-cout layers (include/orca_hip.h).  Any of the last four: the full test entry."""
    x = _f32_cuda(x, "x").contiguous()
    B, n, cin = x.shape
    w = np.ascontiguousarray(w, dtype=np.float32)
    b = np.ascontiguousarray(b, dtype=np.float32)
    cout = w.shape[0]
    d = make_descs([{"w": w, "b": b, "cout": cout, "cin": cin, "k": 9, "dil": 1}])
    if inplace and r2 is None:
        raise ValueError("conv1d_nlc: inplace needs r2")
    y = torch.empty((B, n // 4 if pool4 else n, cout), dtype=torch.float32, device=x.device)
    if y.numel() == 0:
        return y
    ctx = get_context(x.device)
    r1 = r1.contiguous() if r1 is not None else None
    if r2 is None and not pool4 and not fixed_tile:
        check(_lib.load().orca_conv1d_nlc_forward(ctx.handle, d, _lib.PRECISIONS[precision], _p(x), _p(y),
                                                  _p(r1) if r1 is not None else None, B, n, 1 if relu else 0), "orca_conv1d_nlc_forward")
        return y
    if r2 is not None:
        if tuple(r2.shape) != tuple(y.shape):
            raise ValueError(f"conv1d_nlc: r2 must be {tuple(y.shape)}, got {tuple(r2.shape)}")
        r2 = _f32_cuda(r2, "r2").contiguous()
        if inplace:
            y.copy_(r2)
            r2 = y
    ctx.sync_stream()       # the copy above was enqueued on torch's stream
    check(_lib.load().orca_conv1d_nlc_forward_full(ctx.handle, d, _lib.PRECISIONS[precision], _p(x), _p(y), _p(r1) if r1 is not None else None,
                                                   _p(r2) if r2 is not None else None, B, n, 1 if relu else 0, 1 if pool4 else 0,
                                                   int(fixed_tile)), "orca_conv1d_nlc_forward_full")
    return y


def conv1d_p16(x, w, b, relu=False, r1=None, out_mode=0, fmt="p16"):
    """P16 / LDS-DMA conv (test wrapper): x [n,cin] channel-last fp32 -> [n, n/4 (out_mode 1) or n/5 (out_mode 3: 128 couts), cout].
    fmt="b16": the same kernel on single-plane bf16 activations (cin % 32 == 0)."""
    x = _f32_cuda(x, "x").contiguous()
    n, cin = x.shape
    w = np.ascontiguousarray(w, dtype=np.float32)
    b = np.ascontiguousarray(b, dtype=np.float32)
    cout = w.shape[0]
    d = make_descs([{"w": w, "b": b, "cout": cout, "cin": cin, "k": int(w.shape[2]), "dil": 1}])     # 9 taps, or 17 (the composed-pair form)
    y = torch.empty((n // 4 if out_mode == 1 else n // 5 if out_mode == 3 else n, cout), dtype=torch.float32, device=x.device)
    if y.numel() == 0:
        return y
    ctx = get_context(x.device)
    r1 = r1.contiguous() if r1 is not None else None
    fn = _lib.load().orca_conv1d_b16_forward if fmt == "b16" else _lib.load().orca_conv1d_p16_forward
    check(fn(ctx.handle, d, _p(x), _p(y), _p(r1) if r1 is not None else None, n, 1 if relu else 0, out_mode), f"orca_conv1d_{fmt}_forward")
    return y


def conv2d(x, w, b, dilation=1, relu=False, r=None):
    x = _f32_cuda(x, "x").contiguous()
    B, cin, n, _ = x.shape
    w = np.ascontiguousarray(w, dtype=np.float32)
    b = np.ascontiguousarray(b, dtype=np.float32)
    cout = w.shape[0]
    d = make_descs([{"w": w, "b": b, "cout": cout, "cin": cin, "k": 3, "dil": dilation}])
    y = torch.empty((B, cout, n, n), dtype=torch.float32, device=x.device)
    ctx = get_context(x.device)
    r = r.contiguous() if r is not None else None
    check(_lib.load().orca_conv2d_forward(ctx.handle, d, _p(x), _p(y), _p(r) if r is not None else None, B, n,
                                          1 if relu else 0), "orca_conv2d_forward")
    return y


def conv2d_m16(x, w, b, dilation=1, relu=False, r=None, precision="f16x2"):
    """The Decoders' 16-bit 3x3 conv on M16 maps (test wrapper): x [B,cin,n,n] -> [B,cout,n,n]; dilation 1..8."""
    x = _f32_cuda(x, "x").contiguous()
    B, cin, n, _ = x.shape
    w = np.ascontiguousarray(w, dtype=np.float32)
    b = np.ascontiguousarray(b, dtype=np.float32)
    cout = w.shape[0]
    d = make_descs([{"w": w, "b": b, "cout": cout, "cin": cin, "k": 3, "dil": dilation}])
    y = torch.empty((B, cout, n, n), dtype=torch.float32, device=x.device)
    ctx = get_context(x.device)
    r = r.contiguous() if r is not None else None
    check(_lib.load().orca_conv2d_m16_forward(ctx.handle, d, _lib.PRECISIONS[precision], _p(x), _p(y), _p(r) if r is not None else None, B, n,
                                              1 if relu else 0), "orca_conv2d_m16_forward")
    return y


def conv2d_dblock(x, convs, dilation, precision="f16x2"):
    """One whole residual block of the Decoders at dilation 16 / 32 / 64 in one launch (conv2d_dblock.h; test wrapper): x [B,64,n,n],
    convs = [(w, b)] * 4 for lm.a (64 -> 32), lm.b (32 -> 64), m.a, m.b -> lm(x) + x =: o, m(o) + o, [B,64,n,n]; 1 <= n <= 256."""
    x = _f32_cuda(x, "x").contiguous()
    B, _, n, _ = x.shape
    layers = []
    for w, b in convs:
        w = np.ascontiguousarray(w, dtype=np.float32)
        layers.append({"w": w, "b": np.ascontiguousarray(b, dtype=np.float32), "cout": w.shape[0], "cin": w.shape[1], "k": w.shape[2],
                       "dil": int(dilation)})
    if len(layers) != 4:
        raise ValueError("conv2d_dblock: four convs (lm.a, lm.b, m.a, m.b)")
    d = make_descs(layers)
    y = torch.empty_like(x)
    ctx = get_context(x.device)
    check(_lib.load().orca_conv2d_dblock_forward(ctx.handle, d, _lib.PRECISIONS[precision], _p(x), _p(y), B, n), "orca_conv2d_dblock_forward")
    return y


def conv2d_dblock_run(x, convs, d0, fused=True, precision="f16x2"):
    """A run of 2 or 3 consecutive Decoder blocks of dilations d0, 2 d0 (, 4 d0) <= 64 (test wrapper): convs = [(w, b)] * 4 per block.  One
    round trip through the M16 storage; fused: one conv2d_dblock_run_kernel launch, else one conv2d_dblock_kernel launch per block on the
    same M16 buffer."""
    x = _f32_cuda(x, "x").contiguous()
    B, _, n, _ = x.shape
    if len(convs) not in (8, 12):
        raise ValueError("conv2d_dblock_run: four convs (lm.a, lm.b, m.a, m.b) for each of 2 or 3 blocks")
    layers = []
    for k, (w, b) in enumerate(convs):
        w = np.ascontiguousarray(w, dtype=np.float32)
        layers.append({"w": w, "b": np.ascontiguousarray(b, dtype=np.float32), "cout": w.shape[0], "cin": w.shape[1], "k": w.shape[2],
                       "dil": int(d0) << (k // 4)})
    d = make_descs(layers)
    y = torch.empty_like(x)
    ctx = get_context(x.device)
    check(_lib.load().orca_conv2d_dblock_run_forward(ctx.handle, d, len(convs) // 4, _lib.PRECISIONS[precision], _p(x), _p(y), B, n,
                                                     1 if fused else 0), "orca_conv2d_dblock_run_forward")
    return y


def maxpool1d(x, k):
    x = _f32_cuda(x, "x").contiguous()
    B, C, n = x.shape
    y = torch.empty((B, C, n // k), dtype=torch.float32, device=x.device)
    ctx = get_context(x.device)
    check(_lib.load().orca_maxpool1d_forward(ctx.handle, _p(x), n, _p(y), n // k, B * C, n // k, k), "orca_maxpool1d_forward")
    return y


def pointwise1d(x, w_dev, b_dev, act="none"):
    """Kernel-size-1 Conv1d + activation (Net.final_1d layers): x [B,cin,n] ROCm fp32, w_dev [cout,cin] / b_dev [cout]
    ROCm tensors (folded weights).  act: "none" | "relu" | "sigmoid"."""
    x = _f32_cuda(x, "x").contiguous()
    B, cin, n = x.shape
    cout = w_dev.shape[0]
    if tuple(w_dev.shape) != (cout, cin) or not w_dev.is_cuda or not w_dev.is_contiguous():
        raise ValueError("w_dev must be a contiguous [cout,cin] ROCm tensor")
    y = torch.empty((B, cout, n), dtype=torch.float32, device=x.device)
    ctx = get_context(x.device)
    check(_lib.load().orca_pointwise1d_forward(ctx.handle, _p(w_dev), _p(b_dev), cout, cin, _p(x), cin * n, n, _p(y), cout * n, n, B, n,
                                               {"none": 0, "relu": 1, "sigmoid": 2}[act]), "orca_pointwise1d_forward")
    return y
