// scan.h - kernels of the chromosome scan (orca_amd/scan.py: scan_1m; entry points orca_scan_* in orca_screen.hip).  include/orca_hip.h has the definitions
// word for word.  A chromosome stretch has N bins; a window map has n <= SCAN_MAX_BINS bins and window b starts at chromosome bin off[b]; the band keeps
// D distances per bin, band[i][d] = pixel (i, i + d).  Only the upper triangle of a window map is read.  No atomics, no LDS, no workspace: every output
// element has ONE thread (or one wave), the order of every sum is fixed, and nothing depends on how the windows were batched.
// The header stands alone (tests/test_build_scan_cpu.py compiles it by itself).
#pragma once
#include <hip/hip_runtime.h>

#define SCAN_MAX_BINS 256            // bins of a window map (Net.forward's limit)
#define SCAN_MAX_WIDTHS 8            // insulation widths per call
#define SCAN_INSULATION_BINS 32      // bins per workgroup of scan_band_insulation_kernel: 8 per wave

// one batch of window maps [B][n][n] (batch stride map_bs) into the accumulators [N][D].  Thread t of the launch owns band pixel (i, d) = (i0 + t / D,
// t % D) - d fastest, so a wave reads a run of a window row and writes a run of the accumulators - for the rows [i0, i0 + rows) the batch can touch
// (the host passes i0 = off[0] and rows = off[B - 1] + n - off[0] from its copy of the table), clipped to N.  Window b covers the pixel when r = i - off[b]
// has trim <= r and r + d <= n - 1 - trim: with trim >= 0 both indices are inside map b whatever the device copy of `off` holds, so a table that differs
// from the host's cannot make a read leave the maps.  b ascends, the fp64 sum of a pixel continues the one an earlier launch left: one launch of a window
// list and any split of it add the same terms in the same order.  A NaN makes sum NaN by the addition and lo / hi NaN by the branch; the comparisons
// that follow are false, so they stay NaN.  The caller starts the accumulators at sum = 0, count = 0, lo = +inf, hi = -inf.
static __global__ void __launch_bounds__(256) scan_stitch_band_kernel(const float* __restrict__ maps, long map_bs, int B, int n, const long long* __restrict__ off,
                                                                      int trim, long N, int D, long i0, long rows, double* __restrict__ sum,
                                                                      int* __restrict__ count, float* __restrict__ lo, float* __restrict__ hi) {
  const long t = (long)blockIdx.x * 256 + threadIdx.x;
  if (D < 1 || t >= rows * D) return;
  const long i = i0 + t / D;
  const int d = (int)(t % D);
  if (i < 0 || i >= N) return;
  n = n > SCAN_MAX_BINS ? SCAN_MAX_BINS : n;
  trim = trim < 0 ? 0 : trim;
  const long at = i * D + d;
  double s = sum[at];
  int c = count[at];
  float l = lo[at], h = hi[at];
  bool any = false;
  for (int b = 0; b < B; ++b) {                          // wave-uniform loads of the table
    const long r = i - (long)off[b];
    if (r < trim || r + d > (long)(n - 1 - trim)) continue;
    const float v = maps[(long)b * map_bs + r * n + (r + d)];
    s += (double)v;
    ++c;
    if (v != v) l = h = v;
    else {
      l = v < l ? v : l;
      h = v > h ? v : h;
    }
    any = true;
  }
  if (any) {
    sum[at] = s;
    count[at] = c;
    lo[at] = l;
    hi[at] = h;
  }
}

// the accumulators into results, one thread per band pixel: band = (float)(sum / count) - the fp64 quotient, rounded once - and range = hi - lo, one fp32
// subtraction (0 where one window covers the pixel); NaN where no window covers the pixel, and where i + d >= N (a pixel the stretch does not have).
// range may be NULL.
static __global__ void __launch_bounds__(256) scan_band_finish_kernel(const double* __restrict__ sum, const int* __restrict__ count, const float* __restrict__ lo,
                                                                      const float* __restrict__ hi, long N, int D, float* __restrict__ band,
                                                                      float* __restrict__ range) {
  const long at = (long)blockIdx.x * 256 + threadIdx.x;
  if (D < 1 || at >= N * D) return;
  const long i = at / D;
  const int d = (int)(at % D);
  const int c = count[at];
  const bool have = c > 0 && i + d < N;
  const float nan = __int_as_float(0x7fc00000);
  band[at] = have ? (float)(sum[at] / (double)c) : nan;
  if (range) range[at] = have ? hi[at] - lo[at] : nan;
}

// insulation tracks [W][N] of the band [N][D] at W widths (int32; the host entry point checks 1 <= w and 2 w + 1 <= D - any other width reads as one
// that fits nowhere): track[k][i] = the fp64 mean, rounded once, of the w^2 pixels rows r in [i - w, i) x columns c in (i, i + w], read as band[r][c - r]
// (1 <= c - r <= 2 w < D), NaN where i < w or i >= N - w.  Every diamond is summed on its own, so a NaN pixel (a hole of the band) shows in the bins
// whose diamond holds it and in no other.  One workgroup of four waves per (SCAN_INSULATION_BINS bins, width), one wave per bin at a time: lane l adds
// elements l, l + 64, ... of the diamond (row-major) in fp64, then the shuffles - a fixed order, the same bits on every run.
static __global__ void __launch_bounds__(256) scan_band_insulation_kernel(const float* __restrict__ band, long N, int D, const int* __restrict__ widths, int W,
                                                                          float* __restrict__ track) {
  const int k = blockIdx.y, lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  if (k >= W || D < 1) return;
  int w = widths[k];
  const bool legal = w >= 1 && 2 * (long)w + 1 <= D;
  w = legal ? w : 1;
  const long b0 = (long)blockIdx.x * SCAN_INSULATION_BINS;
  const float nan = __int_as_float(0x7fc00000);
  for (long i = b0 + wv; i < b0 + SCAN_INSULATION_BINS && i < N; i += 4) {       // wave-uniform
    const bool fits = legal && i >= w && i < N - w;
    double s = 0.0;
    if (fits) {
      for (int e = lane; e < w * w; e += 64) {
        const int r = e / w, c = e - r * w;
        s += (double)band[(i - w + r) * D + (w - r + 1 + c)];
      }
      for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    }
    if (lane == 0) track[(long)k * N + i] = fits ? (float)(s / ((double)w * (double)w)) : nan;
  }
}

// boundary strengths of W tracks [W][N] of any length: orca_screen_boundary_calls' strength_track, bit for bit, without its limit of 256 bins.  Thread
// (bin i, track k) on a grid of (ceil(N / 256), W): bin i is a minimum when 1 <= i <= N - 2, t[i - 1], t[i], t[i + 1] are not NaN, t[i] < t[i - 1] and
// t[i] <= t[i + 1]; it walks left from i - 1 and right from i + 1 in global memory while the bin exists, is not NaN and is >= t[i], its two running maxima
// in registers; strength = min(L, R) - t[i], ONE fp32 subtraction, written where it is > 0, NaN elsewhere.  A NaN ends a walk.  The walks diverge by
// design; the neighbours of a wave's bins share cache lines.
static __global__ void __launch_bounds__(256) scan_boundary_strength_kernel(const float* __restrict__ tracks, long N, float* __restrict__ strength) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= N) return;
  const float* t = tracks + (long)blockIdx.y * N;
  float s = __int_as_float(0x7fc00000);
  if (i >= 1 && i <= N - 2) {
    const float v = t[i], a = t[i - 1], b = t[i + 1];
    if (v == v && a == a && b == b && v < a && v <= b) {
      float L = v, R = v;
      for (long j = i - 1; j >= 0; --j) {
        const float f = t[j];
        if (!(f >= v)) break;                            // lower, or NaN
        L = f > L ? f : L;
      }
      for (long j = i + 1; j < N; ++j) {
        const float f = t[j];
        if (!(f >= v)) break;
        R = f > R ? f : R;
      }
      s = (L < R ? L : R) - v;
    }
  }
  strength[(long)blockIdx.y * N + i] = s > 0.f ? s : __int_as_float(0x7fc00000);
}
