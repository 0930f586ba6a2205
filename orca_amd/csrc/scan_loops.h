// scan_loops.h - loop (dot) calls along a whole chromosome, on the band (orca_amd/scan.py: scan_1m(..., loops=); entry points orca_scan_band_dot_* in
// orca_screen.hip).  include/orca_hip.h has the definitions word for word.  Included after screen.h: the enrichment is screen_dot_enrich, the one device
// function that computes e anywhere in the project, called on the band as a strided image.  Dense pixel (i + a, j + b) with j = i + d sits at
// band[(i + a) * D + d + b - a] = (&band[i * D + d])[a * (D - 1) + b]: the band is an image with row stride D - 1, so the sums are screen_dot_enrich's own,
// in its order, with its bits.  No atomics, no workspace: every output element has one thread, and the list's order comes from ballots and a prefix.
#pragma once
#include <hip/hip_runtime.h>

#define SCAN_LOOP_MAX_DEPTH 256      // D: distances of a band (SCAN_MAX_BINS)
#define SCAN_LOOP_ROWS 32            // R: band rows per workgroup of scan_band_dot_enrich_kernel; (R + 2 * 16) * 256 floats = 64 KB of LDS

// The enrichment band e[N][D] of a band [N][D]: NaN at every ineligible pixel, every element stored.  One workgroup of 256 threads per tile of R
// consecutive rows [i0, i0 + R).  Rows [i0 - w, i0 + R - 1 + w] go to LDS once, as they lie in memory (row pitch D, so the copy is flat: consecutive
// lanes on consecutive addresses on both sides); a row outside [0, N) is not read, and no eligible pixel needs one.  Element t, t + 256, ... of the
// tile (row-major, d fastest) is then summed from LDS: pixel (i, d) is eligible when w <= i, i + d <= N - 1 - w and d_min <= d <= D - 1 - 2 w, and its
// window is rows i - w .. i + w (inside [0, N) and inside the staged rows) at distances d - 2 w .. d + 2 w (inside [1, D - 1]).  At a fixed (a, b) the
// element's LDS word is e + w * D + a * (D - 1) + b: the lanes of a wave read consecutive words, also across a row's end - no bank conflict.  A pixel's
// result depends on the band alone, not on R or on where its tile starts.
static __global__ void __launch_bounds__(256) scan_band_dot_enrich_kernel(const float* __restrict__ band, long N, int D, int p, int w, int d_min,
                                                                          float* __restrict__ e_band) {
  __shared__ float s_rows[(SCAN_LOOP_ROWS + 2 * SCREEN_DOT_MAX_W) * SCAN_LOOP_MAX_DEPTH];
  if (D < 1 || D > SCAN_LOOP_MAX_DEPTH || N < 1) return;
  w = w > SCREEN_DOT_MAX_W ? SCREEN_DOT_MAX_W : (w < 1 ? 1 : w);
  p = p >= w ? w - 1 : (p < 0 ? 0 : p);
  d_min = d_min < 2 * w + 1 ? 2 * w + 1 : d_min;
  const long i0 = (long)blockIdx.x * SCAN_LOOP_ROWS;
  if (i0 >= N) return;
  const long first = (i0 - w) * D, all = N * D;                           // the flat index of the first staged element; may be negative
  const int staged = (SCAN_LOOP_ROWS + 2 * w) * D;
  for (int k = threadIdx.x; k < staged; k += 256) {
    const long at = first + k;
    if (at >= 0 && at < all) s_rows[k] = band[at];
  }
  __syncthreads();
  const float qnan = __int_as_float(0x7fc00000);
  const int d_hi = D - 1 - 2 * w;
  for (int e = threadIdx.x; e < SCAN_LOOP_ROWS * D; e += 256) {
    const int row = e / D, d = e - row * D;
    const long i = i0 + row;
    if (i >= N) break;                                                      // e ascends with the row
    const bool ok = i >= w && i + d <= N - 1 - w && d >= d_min && d <= d_hi;
    e_band[i0 * D + e] = ok ? screen_dot_enrich(&s_rows[e + w * D], D - 1, p, w) : qnan;
  }
}

// Whether band pixel (i, d) is a dot, and its e in *v: e not NaN, e >= T, and against every neighbour (i + di, d + dj - di), |di|, |dj| <= r, not both
// 0, that exists (row in [0, N), distance in [0, D)) and is not NaN: e > e' where the neighbour precedes the pixel in row-major order (di < 0, or
// di = 0 and dj < 0), e >= e' where it follows.  fp32 comparisons of values read from the enrichment band; ineligible pixels hold NaN there.  The one
// statement of the rule: the counting and the listing kernel both call it.
static __device__ __forceinline__ bool scan_band_is_dot(const float* __restrict__ e_band, long N, int D, long i, int d, int r, float T, float* v) {
  const float e = e_band[i * D + d];
  *v = e;
  if (!(e == e && e >= T)) return false;
  for (int di = -r; di <= r; ++di) {
    const long ii = i + di;
    if (ii < 0 || ii >= N) continue;
    const float* row = e_band + ii * D;
    for (int dj = -r; dj <= r; ++dj) {
      const int dd = d + dj - di;
      if ((di == 0 && dj == 0) || dd < 0 || dd >= D) continue;
      const float f = row[dd];
      if (f != f) continue;
      const bool before = di < 0 || (di == 0 && dj < 0);
      if (before ? !(e > f) : !(e >= f)) return false;
    }
  }
  return true;
}

// One workgroup per band row i, thread d at distance d (the host launches the waves that D needs, at most four): is_dot, one ballot per wave, the
// waves' popcounts through LDS.  *rank = the number of dots of the row at smaller distances, the return value = the number of dots of the row.
static __device__ __forceinline__ int scan_band_row_dots(const float* __restrict__ e_band, long N, int D, int r, float T, long i, bool* dot, float* v,
                                                         int* rank) {
  __shared__ int s_wave[4];
  const int d = threadIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6, waves = (blockDim.x + 63) >> 6;
  *v = 0.f;
  *dot = d < D && scan_band_is_dot(e_band, N, D, i, d, r, T, v);
  const unsigned long long mask = __ballot(*dot);
  if (lane == 0 && wave < 4) s_wave[wave] = __popcll(mask);
  __syncthreads();
  int before = __popcll(mask & ((1ull << lane) - 1ull)), total = 0;
  for (int k = 0; k < waves && k < 4; ++k) {
    const int c = s_wave[k];
    if (k < wave) before += c;
    total += c;
  }
  *rank = before;
  return total;
}

// row_count[i] = the number of dots of band row i, as int64 (the prefix kernel turns the array into offsets in place)
static __global__ void __launch_bounds__(256) scan_band_dot_count_kernel(const float* __restrict__ e_band, long N, int D, int r, float T,
                                                                         long long* __restrict__ row_count) {
  const long i = blockIdx.x;
  if (i >= N || D < 1 || D > SCAN_LOOP_MAX_DEPTH) return;
  r = r > SCREEN_DOT_MAX_R ? SCREEN_DOT_MAX_R : (r < 1 ? 1 : r);
  bool dot;
  float v;
  int rank;
  const int total = scan_band_row_dots(e_band, N, D, r, T, i, &dot, &v, &rank);
  if (threadIdx.x == 0) row_count[i] = total;
}

// row[0 .. N) holds counts and becomes their exclusive prefix, row[N] the total: ONE workgroup of 256 threads, thread t owns the contiguous chunk
// [t c, (t + 1) c) with c = ceil(N / 256) - it adds its chunk up, the 256 partial sums go through LDS, it adds those of the threads below it and
// rewrites its chunk in place.  Integer sums in a fixed order.
static __global__ void __launch_bounds__(256) scan_row_offsets_kernel(long long* __restrict__ row, long N) {
  __shared__ long long s_part[256];
  const long c = (N + 255) / 256, lo = threadIdx.x * c, hi = lo + c < N ? lo + c : N;
  long long sum = 0;
  for (long k = lo; k < hi; ++k) sum += row[k];
  s_part[threadIdx.x] = sum;
  __syncthreads();
  long long base = 0, total = 0;
  for (int k = 0; k < 256; ++k) {
    const long long q = s_part[k];
    if (k < (int)threadIdx.x) base += q;
    total += q;
  }
  for (long k = lo; k < hi; ++k) {
    const long long q = row[k];
    row[k] = base;
    base += q;
  }
  if (threadIdx.x == 0) row[N] = total;
}

// The list: dot k of row i goes to slot row_start[i] + (its rank within the row), as ij = (i, i + d) and enrich = its e - ascending (i, d) order.  The
// predicate is the counting kernel's, evaluated again.  Only slots in [0, cap) are written, cap being the length the host allocated from its copy of
// row_start[N]: whatever the device table holds, no store leaves the lists.
static __global__ void __launch_bounds__(256) scan_band_dot_list_kernel(const float* __restrict__ e_band, long N, int D, int r, float T,
                                                                        const long long* __restrict__ row_start, long cap, long long* __restrict__ ij,
                                                                        float* __restrict__ enrich) {
  const long i = blockIdx.x;
  if (i >= N || D < 1 || D > SCAN_LOOP_MAX_DEPTH) return;
  r = r > SCREEN_DOT_MAX_R ? SCREEN_DOT_MAX_R : (r < 1 ? 1 : r);
  bool dot;
  float v;
  int rank;
  scan_band_row_dots(e_band, N, D, r, T, i, &dot, &v, &rank);
  if (!dot) return;
  const long at = (long)row_start[i] + rank;
  if (at < 0 || at >= cap) return;
  ij[2 * at] = i;
  ij[2 * at + 1] = i + (long)threadIdx.x;
  enrich[at] = v;
}
