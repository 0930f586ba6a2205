"""Cases for the fp16-range guard of the f16x2 arithmetic (tests/test_range_guard_cpu.py checks them, tests/test_gpu_range_guard.py runs them).

A case is the inputs and weights of ONE call, the fp64 reference of every value that call stores to a 16-bit plane, and the flag the call
must leave behind.  The guard's contract: every value stored to a P16 / M16 plane has |v| <= 65504, else the context's flag goes
up.  "Must flag" cases store at least one |v| >= V_FLAG, "must not flag" cases store nothing above V_OK: both margins are ~0.7 % of the
limit, four orders of magnitude above the 2^-22 relative error of the arithmetic, so neither side of a pair depends on rounding.

Single-conv spike (1-D and 2-D): a small random background; input channel CI is zero except for one value XS = 64 at position q; ONE weight
w[co, CI, t] is set so that the output at (p, co), p = q + half - t, is V.  Every other output stays O(1): the other weights of channel CI are
background weights (|w| < 0.2 -> a contribution below 13).  By linearity the reference of a placement is the background's conv (computed
once, in fp64) plus the spike's column of weights scattered around q: `reference()` costs O(cout) per placement, `full_reference()` does
the whole conv again and the CPU test compares the two.

The backgrounds live on a dyadic grid: inputs are multiples of 1/4, weights of 1/32 (the spike's weight of 1/8), biases and residuals of
1/128.  Every product is then a multiple of 2^-7 and every partial sum below 2^17 is exactly representable in fp32, so the kernels' fp32
accumulation is exact and the fp64 reference is what they hold before the final rounding to the 22-bit storage: the twin's values can be
held to 2e-5 + 2^-22 |ref| AT the 65000 spike.  (With a generic background the fp32 accumulation of the ~10^3 terms added behind the spike
is off by ~10 half-ulps there - 2^-21 relative - as any fp32-accumulating conv is, torch's included.)  The price
is that V is met to within 8: "must flag" placements round the weight up (V' in [66000, 66008)), the twins down (V' in (64992, 65000])."""
import numpy as np
import torch
import torch.nn.functional as F

F16_MAX = 65504.0
V_FLAG = 66000.0      # what a "must flag" case stores (at least)
V_OK = 65000.0        # what a "must not flag" twin stores (at most)
V_QUIET = 16384.0     # single-spike cases: every stored value but the spike stays below this
XS = 64.0             # the spike's input value
CI = 3                # the spike's input channel


def _t64(a):
    return torch.from_numpy(np.asarray(a, dtype=np.float64))


def _grid(a, step):
    """``a`` rounded to multiples of ``step`` (a power of two), float32."""
    return (np.round(np.asarray(a) / step) * step).astype(np.float32)


def spike_weight(V, base):
    """The weight w (a multiple of 1/8) with base + XS w on V's side of the limit: >= V for a "must flag" V, <= V otherwise (for negative V mirrored)."""
    w = (V - base) / XS * 8.0
    up = abs(V) >= F16_MAX
    if V < 0:
        up = not up
    return np.float32((np.ceil(w) if up else np.floor(w)) / 8.0)


# ---- 1-D: engine.conv1d_p16 (x [n, cin] channel-last, w [cout, cin, k]) --------------------------------------------------------------------
class Conv1dSpike:
    """One layer shape of `engine.conv1d_p16`: relu, residual (r1 [n, cout] or None) and out_mode 0 (every position), 1 (MaxPool1d(4)),
    2 (fp32 rows, nothing stored to a plane) or 3 (MaxPool1d(5))."""

    def __init__(self, cin, cout, n, k=9, relu=False, residual=False, out_mode=0, seed=0):
        rs = np.random.RandomState(1000 * seed + cin + cout + n + k)
        self.cin, self.cout, self.n, self.k, self.relu, self.out_mode = cin, cout, n, k, relu, out_mode
        self.x0 = _grid(rs.randn(n, cin) * 0.5, 0.25)
        self.x0[:, CI] = 0.0
        self.w0 = _grid(rs.randn(cout, cin, k) / np.sqrt(cin * k) * 1.5, 1.0 / 32)
        self.b = _grid(rs.randn(cout) * 0.1, 1.0 / 128)
        self.r0 = _grid(rs.randn(n, cout) * 0.5, 1.0 / 128) if residual else None
        with torch.no_grad():
            self.base = F.conv1d(_t64(self.x0.T[None]), _t64(self.w0), _t64(self.b), padding=k // 2)[0].numpy().T.copy()   # [n, cout], before the ReLU

    @property
    def pool(self):
        return {0: 1, 1: 4, 2: 1, 3: 5}[self.out_mode]

    def place(self, p, co, V, r_at=None):
        """Inputs of the placement: the conv's output (before ReLU and residual) at (p, co) is V.  ``r_at``: the residual's value at (p, co).
        Returns (x, w, r1, q, t): numpy float32 arrays (r1 None without a residual), the spike's input position and tap."""
        h = self.k // 2
        t = (p * 5 + co) % self.k                    # the tap moves with the placement ...
        q = p - h + t
        if not 0 <= q < self.n:                      # ... and stays inside the sequence
            t = h
            q = p
        x = self.x0.copy()
        x[q, CI] = XS
        w = self.w0.copy()
        w[co, CI, t] = spike_weight(V, self.base[p, co])
        r1 = None
        if self.r0 is not None:
            r1 = self.r0.copy()
            if r_at is not None:
                r1[p, co] = np.float32(r_at)
        return x, w, r1, q, t

    def _epilogue(self, y, r1):
        if self.relu:
            y = np.maximum(y, 0.0)
        if r1 is not None:
            y = y + r1.astype(np.float64)
        if self.pool > 1:
            m = y.shape[0] // self.pool
            y = y[: m * self.pool].reshape(m, self.pool, self.cout).max(1)
        return y

    @property
    def stored0(self):
        """What the background alone stores (no spike, the residual as drawn): [n / pool, cout] fp64, computed once."""
        if getattr(self, "_stored0", None) is None:
            self._stored0 = self._epilogue(self.base, self.r0)
        return self._stored0

    def reference_patch(self, x, w, r1, q):
        """(o0, rows): the placement's stored values are `stored0` with rows [o0, o0 + len(rows)) replaced by ``rows`` (the windows that read
        the spike or hold the changed residual value)."""
        h, P = self.k // 2, self.pool
        lo = max(0, q - h) // P * P
        hi = min(self.n // P * P, -(-(min(self.n, q + h + 1)) // P) * P)
        if hi <= lo:
            return lo // P, np.zeros((0, self.cout))
        y = self.base[lo:hi].copy()
        for t in range(self.k):
            p = q + h - t
            if lo <= p < hi:
                y[p - lo] += float(x[q, CI]) * w[:, CI, t].astype(np.float64)
        return lo // P, self._epilogue(y, None if r1 is None else r1[lo:hi])

    def reference(self, x, w, r1, q):
        """fp64 values the call stores / returns, [n / pool, cout]: background + the spike's weights around q."""
        o0, rows = self.reference_patch(x, w, r1, q)
        out = self.stored0.copy()
        out[o0: o0 + rows.shape[0]] = rows
        return out

    def full_reference(self, x, w, r1):
        with torch.no_grad():
            y = F.conv1d(_t64(x.T[None]), _t64(w), _t64(self.b), padding=self.k // 2)[0].numpy().T
        return self._epilogue(y, r1)


def conv1d_placements(n, cout, tile, wave_positions=32):
    """[(p, co)]: the ends, both sides of every tile boundary, the last position of the ragged last tile (= n - 1), and one position in every
    `wave_positions`-wide slice of the first tile; the channel walks through the octets (co = 8 i + i % 8 for placement i) so that the set
    covers every octet of the layer at least once."""
    ps = [0, n - 1]
    for b in range(tile, n, tile):
        ps += [b - 1, b]
    for s in range(0, min(tile, n), wave_positions):
        ps.append(min(n - 1, s + (7 * (s // wave_positions) + 3) % wave_positions))
    ps = sorted(set(ps))
    noct = cout // 8
    while len(ps) < noct:                                   # at least one placement per octet
        ps.append((ps[-1] * 7 + 13) % n)
    return [(p, 8 * (i % noct) + (i + i // noct) % 8) for i, p in enumerate(ps)]


def pool5_placements(n):
    """conv_p16p5.h (128 couts, 320-position tiles = 64 windows of 5; 8 waves = 2 position groups of 32 windows x 4 cout groups of 32): the
    spike in each of the five slots of windows 0, 13 (first position group), 32, 47, 63 (second; 63 = the last of a tile), 64 (the next tile)
    and the last stored window; the octet moves by 3 per placement, so both position groups meet all four cout groups and every octet occurs."""
    wins = sorted({w for w in (0, 13, 32, 47, 63, 64, n // 5 - 1) if 0 <= w < n // 5})
    return [(5 * w + slot, 8 * ((3 * i) % 16) + (i // 16 + slot) % 8) for i, (w, slot) in enumerate((w, s) for w in wins for s in range(5))]


def p16x_placements(n):
    """conv_p16x.h (96 couts, 512-position tiles, 16 waves = 8 position groups of 64 x 2 cout groups of 48, wave tile 4 x 3 tiles of 16 x 16):
    the ends, both sides of the first tile boundary and of position 65 536 (the length from which the launcher takes this kernel), the last
    position of the ragged last tile (= n - 1), and in one interior tile one position
    per wave: position group k, cout group c -> all 16 waves; the position's 16-wide sub-tile and the cout tile inside the group move with k,
    so that over the set every one of the 4 x 3 accumulator tiles of a wave's tile and all 12 octets occur."""
    out = [(0, 5), (511, 14), (512, 23), (65535, 32), (65536, 41), (n - 1, 95)]
    t0 = 64 * 512
    for k in range(8):
        for c in range(2):
            i = 2 * k + c
            out.append((t0 + 64 * k + 16 * ((k + c) % 4) + (5 * i) % 16, 48 * c + 16 * (i % 3) + 8 * ((k >> 1) & 1) + i % 8))
    return out


# ---- 2-D: engine.conv2d_m16 (x [B, cin, n, n], w [cout, cin, 3, 3], dilation d) -------------------------------------------------------------
class Conv2dSpike:
    def __init__(self, cin, cout, n, dil, B, relu=False, residual=False, seed=0):
        rs = np.random.RandomState(2000 * seed + cin + cout + n + dil + B)
        self.cin, self.cout, self.n, self.dil, self.B, self.relu = cin, cout, n, dil, B, relu
        self.x0 = _grid(rs.randn(B, cin, n, n) * 0.5, 0.25)
        self.x0[:, CI] = 0.0
        self.w0 = _grid(rs.randn(cout, cin, 3, 3) / np.sqrt(cin * 9) * 1.5, 1.0 / 32)
        self.b = _grid(rs.randn(cout) * 0.1, 1.0 / 128)
        self.r0 = _grid(rs.randn(B, cout, n, n) * 0.5, 1.0 / 128) if residual else None
        with torch.no_grad():
            self.base = F.conv2d(_t64(self.x0), _t64(self.w0), _t64(self.b), padding=dil, dilation=dil).numpy()

    def weight(self, bm, i, j, co, V):
        """w with the centre tap of (co, CI) set so that the conv's output at map bm, pixel (i, j), channel co is V (the spike sits at the same pixel)."""
        w = self.w0.copy()
        w[co, CI, 1, 1] = spike_weight(V, self.base[bm, co, i, j])
        return w

    def _epilogue(self, y, r):
        if self.relu:
            y = np.maximum(y, 0.0)
        return y if r is None else y + r.astype(np.float64)

    @property
    def stored0(self):
        """What the background alone stores: [B, cout, n, n] fp64, computed once."""
        if getattr(self, "_stored0", None) is None:
            self._stored0 = self._epilogue(self.base, self.r0)
        return self._stored0

    def reference_patch(self, w, bm, i, j):
        """[((pi, pj), values [cout])]: the pixels of map bm whose stored values differ from `stored0` (those that read the spike)."""
        d, n = self.dil, self.n
        out = []
        for a in range(3):
            for c in range(3):
                pi, pj = i - (a - 1) * d, j - (c - 1) * d          # the output pixel that reads the spike through tap (a, c)
                if 0 <= pi < n and 0 <= pj < n:
                    y = self.base[bm, :, pi, pj] + XS * w[:, CI, a, c].astype(np.float64)
                    out.append(((pi, pj), self._epilogue(y, None if self.r0 is None else self.r0[bm, :, pi, pj])))
        return out

    def reference(self, w, bm, i, j):
        y = self.stored0.copy()
        for (pi, pj), v in self.reference_patch(w, bm, i, j):
            y[bm, :, pi, pj] = v
        return y

    def full_reference(self, w, bm, i, j):
        x = self.x0.copy()
        x[bm, CI, i, j] = XS
        with torch.no_grad():
            y = F.conv2d(_t64(x), _t64(w), _t64(self.b), padding=self.dil, dilation=self.dil).numpy()
        if self.relu:
            y = np.maximum(y, 0.0)
        if self.r0 is not None:
            y = y + self.r0.astype(np.float64)
        return y


def conv2d_pixels(n, dil, B):
    """Spike pixels: the four corners, the last row / column, a pixel on each side of the first row-group boundary (the four-row kernel's
    groups hold rows 4 d q + r + {0, d, 2d, 3d}: rows 4d - 1 | 4d; the one-row kernel's bands are 8 rows: 7 | 8) and of the 128-pixel
    column-tile boundary (127 | 128), where the map has them."""
    px = [(0, 0), (0, n - 1), (n - 1, 0), (n - 1, n - 1), (n // 2, n - 1), (n - 1, n // 2)]
    rb = 4 * dil if B >= 2 else 8
    if rb < n:
        px += [(rb - 1, 5 % n), (rb, 5 % n)]
    if n > 128:
        px += [(n // 3, 127), (n // 3, 128)]
    return px


# ---- channel-last: engine.conv1d_nlc (x [B, n, cin]); the guard sits on the INPUT split -----------------------------------------------------
class NlcCase:
    X_BAD = 7.0e4     # an input value outside the fp16 range

    def __init__(self, cin, cout, n, B=3, seed=0):
        rs = np.random.RandomState(3000 * seed + cin + cout + n)
        self.cin, self.cout, self.n, self.B = cin, cout, n, B
        self.x0 = _grid(rs.randn(B, n, cin) * 0.5, 0.25)
        self.x0[:, :, CI] = 0.0
        self.w0 = _grid(rs.randn(cout, cin, 9) / np.sqrt(cin * 9) * 1.5, 1.0 / 32)
        self.b = _grid(rs.randn(cout) * 0.1, 1.0 / 128)

    @property
    def base(self):
        if getattr(self, "_base", None) is None:
            with torch.no_grad():
                self._base = F.conv1d(_t64(self.x0.transpose(0, 2, 1)), _t64(self.w0), _t64(self.b), padding=4).numpy().transpose(0, 2, 1).copy()
        return self._base          # [B, n, cout]

    def with_input(self, p, ci, value, w=None):
        """(x, ref): x0 with x[B - 1, p, ci] = value, and the fp64 output [B, n, cout] of the conv with weights ``w`` (default w0; it may
        differ from w0 in channel CI only, which is zero in x0)."""
        w = self.w0 if w is None else w
        x = self.x0.copy()
        x[self.B - 1, p, ci] = np.float32(value)
        ref = self.base.copy()
        dx = float(x[self.B - 1, p, ci]) - float(self.x0[self.B - 1, p, ci])
        for t in range(9):
            o = p + 4 - t
            if 0 <= o < self.n:
                ref[self.B - 1, o] += dx * w[:, ci, t].astype(np.float64)
        return x, ref

    def big_output(self, p, co, V=1.0e5):
        """In-range inputs (one value XS in batch row B - 1) whose OUTPUT at (B - 1, p, co) is V: nothing to flag here, the consumer checks it."""
        w = self.w0.copy()
        w[co, CI, 4] = spike_weight(V, self.base[self.B - 1, p, co])
        x, ref = self.with_input(p, CI, XS, w)
        return x, w, ref


# ---- Decoder blocks: engine.conv2d_dblock with zero weights: out = x + b_lm + b_m exactly ----------------------------------------------------
class DBlockCase:
    X_HI, X_LO = 60000.0, 59000.0        # + 6000 of biases: 66000 / 65000

    def __init__(self, n, B, seed=0):
        rs = np.random.RandomState(4000 * seed + n + B)
        self.n, self.B = n, B
        self.x0 = (np.round(rs.randn(B, 64, n, n) * 32.0) / 64.0).astype(np.float32)     # multiples of 1/64: x + 6000 is exact in the 22-bit storage
        z = lambda co, ci: np.zeros((co, ci, 3, 3), dtype=np.float32)
        b_lm = np.full(64, 2500.0, dtype=np.float32)
        b_m = np.full(64, 3500.0, dtype=np.float32)
        # lm.a, lm.b, m.a, m.b: lm(x) = b_lm, o = x + b_lm; m(o) = relu(b_m) = b_m, out = o + b_m
        self.convs = [(z(32, 64), np.zeros(32, np.float32)), (z(64, 32), b_lm), (z(32, 64), np.zeros(32, np.float32)), (z(64, 32), b_m)]
        self.bias_sum = 6000.0

    def reference(self, x):
        return x.astype(np.float64) + self.bias_sum

    def pixels(self, d):
        """Corners and both sides of the sub-image boundaries (a block kernel's workgroup holds the pixels (i % d, j % d) = const:
        neighbours i = d - 1 | d belong to different workgroups)."""
        n = self.n
        px = [(0, 0), (0, n - 1), (n - 1, 0), (n - 1, n - 1)]
        if d < n:
            px += [(d - 1, d), (d, d - 1), (d, d)]
        return px


# ---- the edge-fix kernels (conv_p16.h: lconv_edge_layer_kernel, lconv_edge_pool_kernel) --------------------------------------------------------
BN_EPS = 1e-5
EDGE_MID, EDGE_OUT = 5, 7        # the intermediate channel that carries 1e5, the output channel that shows it at the ends
EDGE_BIAS = 1.0e5


def _fold_scale(sd, bn, ch):
    return float(sd[bn + ".weight"][ch]) / float(np.sqrt(np.float64(sd[bn + ".running_var"][ch]) + BN_EPS))


def edge_sd(sd, stage):
    """A copy of the Encoder state dict ``sd`` whose linear group lconv<stage> (1 or 2) hides +-1e5 at the sequence ends: the intermediate's
    channel EDGE_MID gets +1e5 through its BatchNorm bias; the second conv reads that channel only into output channel EDGE_OUT, through taps
    0 and 8 with weights -1/s and +1/s (s: the folded scale of the group's last BatchNorm).  In the interior the two taps cancel (the
    intermediate is 1e5 + O(1) at both); at the first four positions tap 0 reads the zero padding (output +1e5), at the last four tap 8 does
    (-1e5).  A composed 17-tap conv sees the intermediate's VIRTUAL values beyond the ends - 1e5 there too - and cancels everywhere.
    Stage 1 also zeroes conv1.a's weights on channel EDGE_OUT: lout1 then reaches the stage output through the residual only, i.e. through
    the pooled end windows that lconv_edge_pool_kernel rewrites, and through no value that lconv_edge_layer_kernel stores on the default route."""
    sd = {k: np.array(v, copy=True) for k, v in sd.items()}
    c1, bn1, c2, bn2 = ("lconv1.0", "lconv1.1", "lconv1.2", "lconv1.3") if stage == 1 else ("lconv2.1", "lconv2.2", "lconv2.3", "lconv2.4")
    sd[bn1 + ".bias"][EDGE_MID] += np.float32(EDGE_BIAS)
    s = _fold_scale(sd, bn2, EDGE_OUT)
    w = sd[c2 + ".weight"]
    w[:, EDGE_MID, :] = 0.0
    w[EDGE_OUT, EDGE_MID, 0] = np.float32(-1.0 / s)
    w[EDGE_OUT, EDGE_MID, 8] = np.float32(1.0 / s)
    if stage == 1:
        sd["conv1.0.weight"][:, EDGE_OUT, :] = 0.0
    return sd


def edge_views(sd, codes, stage):
    """fp64, from the oracle's layers, for the Encoder ``sd`` on the bases ``codes`` [L]:
      "lout_true"      lconv<stage>'s output as the reference computes it (every intermediate zero-padded): what the edge-fix kernels store at the ends
      "lout_composed"  the same conv pair on the stage input padded by 8 zeros per side, read back at offset 8: what a 17-tap composed conv
                       computes (and what the main kernel's guard sees) at every position
      "stored_before"  every tensor the chain stores BEFORE that stage's edge fix runs (earlier stage outputs and their layers), as a list
      "out_true"       the stage's output after the residual and its MaxPool1d(4): [n / 4, C]
      "out_main"       the same with the COMPOSED lout as residual: what the main kernel's epilogue holds where the edge fix has not been applied
    all [n, C]."""
    from oracle import orca_oracle as O
    from tests import encoder_ref as R
    s = O._SD(sd, "", torch.float64)
    with torch.no_grad():
        x = R.onehot(codes)
        before = []
        if stage == 2:
            l1 = O._lin2(s, "lconv1", 0, x)
            a1 = F.relu(O._bn(s, "conv1.1", O._conv(s, "conv1.0", l1)))
            o1 = O._relu2(s, "conv1", l1) + l1
            x = F.max_pool1d(o1, 4, 4)
            before = [l1, a1, x]
        name, i0 = ("lconv1", 0) if stage == 1 else ("lconv2", 1)
        lt = O._lin2(s, name, i0, x)
        lc = O._lin2(s, name, i0, F.pad(x, (8, 8)))[:, :, 8:-8]
        cname = f"conv{stage}"
        a = F.relu(O._bn(s, cname + ".1", O._conv(s, cname + ".0", lt)))               # conv<stage>.a reads the edge-fixed (true) lout
        c = F.relu(O._bn(s, cname + ".4", O._conv(s, cname + ".3", a)))
        out_true = F.max_pool1d(c + lt, 4, 4)
        out_main = F.max_pool1d(c + lc, 4, 4)
    f = lambda t: t[0].numpy().T
    return {"lout_true": f(lt), "lout_composed": f(lc), "stored_before": [f(t) for t in before], "a": f(a), "out_true": f(out_true), "out_main": f(out_main)}


# ---- what both test files loop over -----------------------------------------------------------------------------------------------------------
CONV2D_MAPS = [(30, 1), (30, 2), (250, 1), (250, 2)]                 # (n, B): B = 1 the one-row kernel, B = 2 the four-row kernel
CONV2D_LAYERS = [(dil, cin, cout, res) for dil in (1, 8) for cin, cout in ((64, 32), (32, 64)) for res in (False, True)]
DBLOCK_N, DBLOCK_B, DBLOCK_DILS = 70, 2, (16, 64)


# ---- Decoder heads ---------------------------------------------------------------------------------------------------------------------------
HEAD_C, HEAD_N = 37, 130
HEAD_X_BAD, HEAD_X_OK = 40000.0, 32500.0          # x_i + x_j at (i, i): 80000 / 65000
HEAD_SUM_PIXELS = (0, 64, HEAD_N - 1)
HEAD_DE_PIXELS = ((0, 0), (64, 129), (129, 3))
HEAD_Y_BAD, HEAD_Y_OK = 7.0e4, 6.5e4


def head_inputs(B, seed=None):
    """(x [B, 128, n], distenc [1, 1, n, n], y [B, 1, n / 2, n / 2]) on the dyadic grids, O(1)."""
    rs = np.random.RandomState(B if seed is None else seed)
    return (_grid(rs.randn(B, 128, HEAD_N) * 0.5, 0.25), _grid(rs.randn(1, 1, HEAD_N, HEAD_N) * 0.5, 1.0 / 128),
            _grid(rs.randn(B, 1, HEAD_N // 2, HEAD_N // 2) * 0.5, 0.25))


def head_y_pixels(mode):
    """Pixels of y for the up-sample spike.  Bilinear: only a corner pixel of y reaches an output pixel with weight 1 (elsewhere 7e4 arrives
    as <= 0.75 x 7e4, in range); nearest: any pixel."""
    return ((0, 0), (0, 64), (64, 0), (64, 64)) + (((32, 31), (17, 64)) if mode == "nearest" else ())


def upsampled(y, mode):
    with torch.no_grad():
        return F.interpolate(_t64(y), scale_factor=(2, 2), mode=mode).numpy()


# ---- Encoder stage 1 in every form ---------------------------------------------------------------------------------------------------------------
STAGE1_L = 16 * 600
STAGE1_CH = 9
STAGE1_POSITIONS = (0, 256, STAGE1_L - 1)
STAGE1_BASE_GAIN = 3.0e6
ENCODER_FORMS = ("default", "stored_residual", "lconv1_only", "two_conv")


def stage1_scaled_sd(sd):
    """``sd`` with lconv1's channel STAGE1_CH scaled out of range through its last BatchNorm (weight x 100, bias + 1e5)."""
    sd = {k: np.array(v, copy=True) for k, v in sd.items()}
    sd["lconv1.3.weight"][STAGE1_CH] *= 100.0
    sd["lconv1.3.bias"][STAGE1_CH] += 1.0e5
    return sd


def stage1_tensors(sd, x):
    """fp64 [first conv + BN, lout1, conv1.a's output, the stage output before its pool] of the Encoder ``sd`` on rows ``x`` [1, 4, L]."""
    from oracle import orca_oracle as O
    s = O._SD(sd, "", torch.float64)
    with torch.no_grad():
        x = _t64(x)
        mid = O._bn(s, "lconv1.1", O._conv(s, "lconv1.0", x))
        l1 = O._lin2(s, "lconv1", 0, x)
        a1 = F.relu(O._bn(s, "conv1.1", O._conv(s, "conv1.0", l1)))
        o1 = O._relu2(s, "conv1", l1) + l1
    return [t[0].numpy() for t in (mid, l1, a1, o1)]
