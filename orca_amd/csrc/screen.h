// screen.h - the small kernels of the 1 Mb in-silico mutagenesis screen (orca_amd/screen.py): edited snippets straight from the window's
// codes, the per-edit stage-5 row images, the [B][n][128] -> [B][128][n] hand-over of batched stages 5-7, and the map scores (bin with bin, and on aligned bins).
// All of them are HBM-bound and tiny next to the Decoder_1m they feed; each is ONE launch for a whole batch of edits.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// ---- the edited bases: three table formats over one snippet table (include/orca_hip.h: orca_screen_edit_codes, _edit_codes_multi, _assemble_codes) -------
// snippet table (int64 per snippet, SCREEN_EDIT_FIELDS fields): [0] out_off  first output base of this snippet in the packed output  [1] b0  its first
// base in the source's coordinates  [2] nb  its bases; snippets are packed back to back in table order (out_off ascending, no gaps).  The other fields:
//   single span (screen.Edit):     [3] kind  [4] pos  [5] len  [6] pay_off - the one span of the snippet, fields as in the span table
//   spans (screen.EditSet):        [3] span_lo  first span of this snippet in the span table  [4] span_cnt
//   pieces ("del" / "ins" edits):  [3] piece_lo  first piece of this snippet in the piece table  [4] piece_cnt; b0 is an ALT base
// span table (int64 per span, SCREEN_SPAN_FIELDS fields): [0] kind  0 substitution (payload), 1 N-mask, 2 in-place reverse complement  [1] pos  first
// window base of the span  [2] len  [3] pay_off  first payload code of a substitution - a snippet's spans are sorted by pos and pairwise disjoint, so a
// binary search finds the one span that can hold a base.  An inversion reads its source from the unedited window.
// piece table (int64 per piece, SCREEN_PIECE_FIELDS fields): [0] dst  first alt base  [1] kind  [2] src  [3] len - the alt window of an item is a list of
// pieces in alt coordinates over the CONTEXT (the window followed by its right flank); a snippet's pieces are sorted by dst and pairwise disjoint.
// kind 0: context bases [src, src + len) forward; 1: their reverse complement (alt base dst + t is the complement of context[src + len - 1 - t]);
// 2: payload codes [src, src + len); 3: N.  A base no piece covers is N.
// Every kernel is one thread per output base: binary search of its snippet, of the snippet's spans / pieces, then the base.  A sub-table range is clipped
// to its table and every read is bounds-checked (an out-of-range index reads as N), so a malformed table cannot make a kernel leave its buffers.
#define SCREEN_EDIT_FIELDS 8
#define SCREEN_SPAN_FIELDS 4
#define SCREEN_PIECE_FIELDS 4

// the last snippet with out_off <= t (the first one when none is)
static __device__ __forceinline__ const long long* screen_snippet_of(const long long* __restrict__ tab, int ns, long t) {
  int lo = 0, hi = ns - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (tab[(long)mid * SCREEN_EDIT_FIELDS] <= t) lo = mid; else hi = mid - 1;
  }
  return tab + (long)lo * SCREEN_EDIT_FIELDS;
}

// of rows [lo, hi) (clipped to the n rows) of an int64 table with FIELDS columns, the last one whose column K is <= x (the first one when none is);
// NULL for an empty range
template <int FIELDS, int K>
static __device__ __forceinline__ const long long* screen_row_of(const long long* __restrict__ tab, long n, long lo, long hi, long x) {
  lo = lo < 0 ? 0 : lo;
  hi = hi > n ? n : hi;
  if (lo >= hi) return nullptr;
  long a = lo, z = hi - 1;
  while (a < z) {
    const long mid = (a + z + 1) >> 1;
    if ((long)tab[mid * FIELDS + K] <= x) a = mid; else z = mid - 1;
  }
  return tab + a * FIELDS;
}

static __device__ __forceinline__ unsigned screen_code(const unsigned char* __restrict__ buf, long n, long i) { return (i >= 0 && i < n) ? buf[i] : 4u; }
static __device__ __forceinline__ unsigned screen_complement(unsigned s) { return s < 4u ? 3u - s : 4u; }      // A<->T, C<->G; N stays N

// window base w (unedited: c) under the span (kind, pos, len, pay_off)
static __device__ __forceinline__ unsigned screen_span_code(unsigned c, long w, long long kind, long pos, long len, long pay_off, const unsigned char* __restrict__ win,
                                                            long L, const unsigned char* __restrict__ pay, long npay) {
  const long k = w - pos;
  if (w < pos || k >= len) return c;
  if (kind == 0) return screen_code(pay, npay, pay_off + k);
  if (kind == 1) return 4u;
  return screen_complement(screen_code(win, L, pos + len - 1 - k));
}

static __global__ void screen_edit_codes_kernel(const unsigned char* __restrict__ win, long L, const long long* __restrict__ tab, int ns,
                                                const unsigned char* __restrict__ pay, long npay, unsigned char* __restrict__ out, long total) {
  const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= total) return;
  const long long* e = screen_snippet_of(tab, ns, t);
  const long w = (long)e[1] + (t - (long)e[0]);
  const unsigned c = screen_span_code(screen_code(win, L, w), w, e[3], (long)e[4], (long)e[5], (long)e[6], win, L, pay, npay);
  out[t] = (unsigned char)(c > 4u ? 4u : c);
}

static __global__ void screen_edit_codes_multi_kernel(const unsigned char* __restrict__ win, long L, const long long* __restrict__ tab, int ns,
                                                      const long long* __restrict__ spans, long nspans, const unsigned char* __restrict__ pay, long npay,
                                                      unsigned char* __restrict__ out, long total) {
  const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= total) return;
  const long long* e = screen_snippet_of(tab, ns, t);
  const long w = (long)e[1] + (t - (long)e[0]);
  unsigned c = screen_code(win, L, w);
  if (const long long* sp = screen_row_of<SCREEN_SPAN_FIELDS, 1>(spans, nspans, (long)e[3], (long)e[3] + (long)e[4], w))
    c = screen_span_code(c, w, sp[0], (long)sp[1], (long)sp[2], (long)sp[3], win, L, pay, npay);
  out[t] = (unsigned char)(c > 4u ? 4u : c);
}

static __global__ void screen_assemble_codes_kernel(const unsigned char* __restrict__ cx, long C, const long long* __restrict__ tab, int ns,
                                                    const long long* __restrict__ pieces, long npieces, const unsigned char* __restrict__ pay, long npay,
                                                    unsigned char* __restrict__ out, long total) {
  const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= total) return;
  const long long* e = screen_snippet_of(tab, ns, t);
  const long w = (long)e[1] + (t - (long)e[0]);
  unsigned c = 4u;
  if (const long long* pc = screen_row_of<SCREEN_PIECE_FIELDS, 0>(pieces, npieces, (long)e[3], (long)e[3] + (long)e[4], w)) {
    const long dst = (long)pc[0], src = (long)pc[2], len = (long)pc[3], k = w - dst;
    if (w >= dst && k < len) {
      if (pc[1] == 0) c = screen_code(cx, C, src + k);
      else if (pc[1] == 1) c = screen_complement(screen_code(cx, C, src + len - 1 - k));
      else if (pc[1] == 2) c = screen_code(pay, npay, src + k);
    }
  }
  out[t] = (unsigned char)(c > 4u ? 4u : c);
}

// ---- the row images: three segment formats (orca_screen_splice_rows, _splice_rows_multi, _gather_rows) -----------------------------------------------------
// A segment says that rows [row_lo, row_lo + row_cnt) of an image come from elsewhere; a row in no segment is `ref` at its own index.
//   splice table (int64 per image, 3 fields): [row_lo, row_cnt, src_row] - image b has the one segment b, from rows [src_row, ..) of `fresh`
//   segment table (3 fields, the same) with offsets: image b owns segments [seg_off[b], seg_off[b + 1]), sorted by row_lo and disjoint
//   gather table (SCREEN_GATHER_FIELDS fields) with offsets: [row_lo, row_cnt, source, src_row] - source -1: rows [src_row, ..) of `fresh`; -2: rows
//   [src_row, ..) of `ref`; p >= 0: row row_lo + t is the MaxPool1d(5) of rows src_row + 5 t .. + 4 of phase entry p (`entries[p]`, `entry_rows[p]` rows
//   of 128 floats).  The pooling expression is rows_pool5_into_kernel's (p16_planes.h): the same bits.
// One thread per 16-byte unit of the output [B][n5][128]: binary search of the image's segments for the last one with row_lo <= r.  The segment range
// is clipped to the table, every source row to its buffer (a row that would leave it is `ref` at its own index).
#define SCREEN_GATHER_FIELDS 4

// FIELDS columns per segment, src_row the last; RANGED: image b's segments by seg_off, else segment b; SOURCES: the source column, else all from `fresh`
template <int FIELDS, bool RANGED, bool SOURCES>
static __device__ __forceinline__ void screen_row_images(const f32x4* __restrict__ ref, long n5, const f32x4* __restrict__ fresh, long nfresh,
                                                         const f32x4* const* __restrict__ entries, const long long* __restrict__ entry_rows, int P,
                                                         const long long* __restrict__ seg, long nseg, const long long* __restrict__ seg_off, int B,
                                                         f32x4* __restrict__ out) {
  const long u = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const long per = n5 * 32;
  if (u >= (long)B * per) return;
  const int b = (int)(u / per);
  const long r = (u - (long)b * per) >> 5, q = u & 31;
  const long long* g = seg + (long)FIELDS * b;
  if constexpr (RANGED) g = screen_row_of<FIELDS, 0>(seg, nseg, (long)seg_off[b], (long)seg_off[b + 1], r);
  const f32x4* from = ref + r * 32 + q;
  bool pool = false;
  if (g) {
    const long r0 = (long)g[0], cnt = (long)g[1], k = r - r0;
    long source = -1;
    if constexpr (SOURCES) source = (long)g[2];
    const long s = (long)g[FIELDS - 1] + (source >= 0 ? 5 : 1) * k;
    if (r >= r0 && k < cnt) {
      if (source == -1) {
        if (s >= 0 && s < nfresh) from = fresh + s * 32 + q;
      } else if constexpr (SOURCES) {
        if (source == -2) {
          if (s >= 0 && s < n5) from = ref + s * 32 + q;
        } else if (source >= 0 && source < P && s >= 0 && s + 5 <= (long)entry_rows[source]) {
          from = entries[source] + s * 32 + q;
          pool = true;
        }
      }
    }
  }
  f32x4 v = from[0];
  if (pool) {
#pragma unroll
    for (int j = 1; j < 5; ++j) {
      const f32x4 x = from[j * 32];
      v.x = fmaxf(v.x, x.x); v.y = fmaxf(v.y, x.y); v.z = fmaxf(v.z, x.z); v.w = fmaxf(v.w, x.w);
    }
  }
  out[u] = v;
}

static __global__ void screen_splice_rows_kernel(const f32x4* __restrict__ ref, long n5, const f32x4* __restrict__ fresh, long nfresh,
                                                 const long long* __restrict__ tab, int B, f32x4* __restrict__ out) {
  screen_row_images<3, false, false>(ref, n5, fresh, nfresh, nullptr, nullptr, 0, tab, B, nullptr, B, out);
}

static __global__ void screen_splice_rows_multi_kernel(const f32x4* __restrict__ ref, long n5, const f32x4* __restrict__ fresh, long nfresh,
                                                       const long long* __restrict__ seg, long nseg, const long long* __restrict__ seg_off, int B,
                                                       f32x4* __restrict__ out) {
  screen_row_images<3, true, false>(ref, n5, fresh, nfresh, nullptr, nullptr, 0, seg, nseg, seg_off, B, out);
}

static __global__ void screen_gather_rows_kernel(const f32x4* __restrict__ ref, long n5, const f32x4* __restrict__ fresh, long nfresh,
                                                 const f32x4* const* __restrict__ entries, const long long* __restrict__ entry_rows, int P,
                                                 const long long* __restrict__ seg, long nseg, const long long* __restrict__ seg_off, int B,
                                                 f32x4* __restrict__ out) {
  screen_row_images<SCREEN_GATHER_FIELDS, true, true>(ref, n5, fresh, nfresh, entries, entry_rows, P, seg, nseg, seg_off, B, out);
}

// channel-last rows [B][n][128] -> out[b * so_b + c * so_c + j]
static __global__ void screen_rows_to_bins_kernel(const float* __restrict__ src, long n, int B, float* __restrict__ out, long so_b, long so_c) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (long)B * n * 128) return;
  const long c = i % 128, j = (i / 128) % n, b = i / (128 * n);
  out[b * so_b + c * so_c + j] = src[i];
}

// scores of B alt maps [B][n][n] (batch stride map_bs) against ref [n][n]: profile[b][i] = mean_j |alt - ref|, mean[b] = mean of the
// profile (= mean over the map), amax[b] = max |alt - ref|.  One workgroup per map, one wave per row at a time; every map element is
// read once.  A NaN difference propagates into all three (as numpy's mean / max do).
static __global__ void __launch_bounds__(512) screen_scores_kernel(const float* __restrict__ alt, long map_bs, const float* __restrict__ ref, int n,
                                                                   float* __restrict__ profile, float* __restrict__ mean, float* __restrict__ amax) {
  __shared__ double s_sum[8];
  __shared__ float s_max[8];
  const int b = blockIdx.x, lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const float* a = alt + (long)b * map_bs;
  double wsum = 0.0;            // sums in fp64: the scores match a host fp64 restatement to ~1e-12 relative, whatever the order
  float wmax = 0.f;
  bool wnan = false;
  for (int i = wv; i < n; i += 8) {
    double rs = 0.0;
    for (int j = lane; j < n; j += 64) {
      const float d = fabsf(a[(long)i * n + j] - ref[(long)i * n + j]);
      rs += (double)d;
      wnan |= d != d;
      wmax = fmaxf(wmax, d);
    }
    for (int o = 32; o > 0; o >>= 1) rs += __shfl_xor(rs, o, 64);
    if (lane == 0) profile[(long)b * n + i] = (float)(rs / (double)n);
    wsum += rs;
  }
  for (int o = 32; o > 0; o >>= 1) {
    wmax = fmaxf(wmax, __shfl_xor(wmax, o, 64));
    wnan |= __shfl_xor((int)wnan, o, 64) != 0;
  }
  if (lane == 0) {
    s_sum[wv] = wsum;
    s_max[wv] = wnan ? __int_as_float(0x7fc00000) : wmax;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    double t = 0.0;
    float m = 0.f;
    bool nan = false;
    for (int k = 0; k < 8; ++k) {
      t += s_sum[k];
      nan |= s_max[k] != s_max[k];
      m = fmaxf(m, s_max[k]);
    }
    mean[b] = nan ? __int_as_float(0x7fc00000) : (float)(t / ((double)n * (double)n));
    amax[b] = nan ? __int_as_float(0x7fc00000) : m;
  }
}

// region scores of B alt maps [B][n][n] (batch stride map_bs) against ref [n][n]: for rectangle k = (i0, i1, j0, j1) (int32, half open, inside
// [0, n) - the host entry point checks it; clipped here all the same) signed[b][k] = mean of alt - ref, absm[b][k] = mean of |alt - ref|.
// One workgroup per (map, rectangle).  The differences and both sums are fp64 (an fp32 difference is exact in fp64, so the signed mean keeps
// its accuracy under cancellation); a NaN difference propagates through both sums.
static __global__ void __launch_bounds__(256) screen_region_scores_kernel(const float* __restrict__ alt, long map_bs, const float* __restrict__ ref, int n,
                                                                          const int* __restrict__ rects, int K, float* __restrict__ signed_out,
                                                                          float* __restrict__ abs_out) {
  __shared__ double s_sum[4], s_abs[4];
  const int b = blockIdx.x, k = blockIdx.y, lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  int i0 = rects[4 * k], i1 = rects[4 * k + 1], j0 = rects[4 * k + 2], j1 = rects[4 * k + 3];
  i0 = i0 < 0 ? 0 : i0; j0 = j0 < 0 ? 0 : j0;
  i1 = i1 > n ? n : i1; j1 = j1 > n ? n : j1;
  const int h = i1 > i0 ? i1 - i0 : 0, w = j1 > j0 ? j1 - j0 : 0;
  const float* a = alt + (long)b * map_bs;
  double sum = 0.0, asum = 0.0;
  for (int e = threadIdx.x; e < h * w; e += 256) {
    const long at = (long)(i0 + e / w) * n + (j0 + e % w);
    const double d = (double)a[at] - (double)ref[at];
    sum += d;
    asum += fabs(d);
  }
  for (int o = 32; o > 0; o >>= 1) {
    sum += __shfl_xor(sum, o, 64);
    asum += __shfl_xor(asum, o, 64);
  }
  if (lane == 0) { s_sum[wv] = sum; s_abs[wv] = asum; }
  __syncthreads();
  if (threadIdx.x == 0) {
    const double cnt = (double)h * (double)w;
    const double t = (s_sum[0] + s_sum[1]) + (s_sum[2] + s_sum[3]), ta = (s_abs[0] + s_abs[1]) + (s_abs[2] + s_abs[3]);
    signed_out[(long)b * K + k] = (float)(t / cnt);
    abs_out[(long)b * K + k] = (float)(ta / cnt);
  }
}

// ---- aligned scores (screen.bin_map): alt bin i stands for reference bin map[i], or for none (-1) -------------------------------------------------------
// bin map (int32 per alt bin, [B][n]; include/orca_hip.h: orca_screen_aligned_scores): values -1 .. n - 1 - the host entry point checks it; any other value
// reads as -1 here.  Every result is indexed by ALT bin (two alt bins may stand for one reference bin).  At most SCREEN_ALIGNED_MAX_BINS bins: the map of a
// workgroup's alt map lives in LDS.
#define SCREEN_ALIGNED_MAX_BINS 256

// map b's entries into LDS, clipped to -1 .. n - 1 (entries past n are -1); the caller synchronises
static __device__ __forceinline__ int screen_load_bin_map(const int* __restrict__ map, int n, int* s_map) {
  int m = -1;
  if ((int)threadIdx.x < n) {
    m = map[threadIdx.x];
    m = (m >= 0 && m < n) ? m : -1;
  }
  if (threadIdx.x < SCREEN_ALIGNED_MAX_BINS) s_map[threadIdx.x] = m;
  return m;
}

// screen_scores_kernel over the mapped bins M = {i : map[i] >= 0}, c = |M|: d(i, j) = |alt[i][j] - ref[map i][map j]| for i, j in M (difference in fp64);
// profile[b][i] = sum_j d / c (NaN for i outside M), mean[b] = sum_ij d / c^2, amax[b] = max d; all NaN when c = 0.  One workgroup per map, one wave
// per alt row at a time: the alt row is read along its columns, the reference row `map i` at columns `map j` (near-contiguous runs, the map ascends).
// Only mapped pairs are read, so a NaN elsewhere does not show; one at a mapped pair propagates as in screen_scores_kernel.  The order of every sum is
// fixed by (n, the map) alone: a map's results do not depend on B or on its place in the batch.
static __global__ void __launch_bounds__(512) screen_aligned_scores_kernel(const float* __restrict__ alt, long map_bs, const float* __restrict__ ref, int n,
                                                                           const int* __restrict__ bin_map, float* __restrict__ profile,
                                                                           float* __restrict__ mean, float* __restrict__ amax) {
  __shared__ int s_map[SCREEN_ALIGNED_MAX_BINS];
  __shared__ double s_sum[8], s_max[8];
  __shared__ int s_nan[8];
  const int b = blockIdx.x, lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  n = n > SCREEN_ALIGNED_MAX_BINS ? SCREEN_ALIGNED_MAX_BINS : n;
  const int mine = screen_load_bin_map(bin_map + (long)b * n, n, s_map);
  const int c = __syncthreads_count(mine >= 0);
  const float* a = alt + (long)b * map_bs;
  const float qnan = __int_as_float(0x7fc00000);
  double wsum = 0.0, wmax = 0.0;
  bool wnan = false;
  for (int i = wv; i < n; i += 8) {
    const int mi = s_map[i];                         // wave-uniform
    if (mi < 0) {
      if (lane == 0) profile[(long)b * n + i] = qnan;
      continue;
    }
    double rs = 0.0;
    for (int j = lane; j < n; j += 64) {
      const int mj = s_map[j];
      if (mj < 0) continue;
      const double d = fabs((double)a[(long)i * n + j] - (double)ref[(long)mi * n + mj]);
      rs += d;
      wnan |= d != d;
      wmax = fmax(wmax, d);
    }
    for (int o = 32; o > 0; o >>= 1) rs += __shfl_xor(rs, o, 64);
    if (lane == 0) profile[(long)b * n + i] = (float)(rs / (double)c);
    wsum += rs;
  }
  for (int o = 32; o > 0; o >>= 1) {
    wmax = fmax(wmax, __shfl_xor(wmax, o, 64));
    wnan |= __shfl_xor((int)wnan, o, 64) != 0;
  }
  if (lane == 0) {
    s_sum[wv] = wsum;
    s_max[wv] = wmax;
    s_nan[wv] = wnan ? 1 : 0;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    double t = 0.0, m = 0.0;
    bool nan = c == 0;
    for (int k = 0; k < 8; ++k) {
      t += s_sum[k];
      nan |= s_nan[k] != 0;
      m = fmax(m, s_max[k]);
    }
    mean[b] = nan ? qnan : (float)(t / ((double)c * (double)c));
    amax[b] = nan ? qnan : (float)m;
  }
}

// the bins i (ascending) with lo <= s_map[i] < hi into list[]; one wave, returns their number (the same in every lane)
static __device__ __forceinline__ int screen_bins_in(const int* s_map, int n, int lo, int hi, int* list, int lane) {
  int cnt = 0;
  for (int i0 = 0; i0 < n; i0 += 64) {
    const int i = i0 + lane;
    const bool in = i < n && s_map[i] >= lo && s_map[i] < hi;
    const unsigned long long mask = __ballot(in);
    if (in) list[cnt + __popcll(mask & ((1ull << lane) - 1ull))] = i;
    cnt += __popcll(mask);
  }
  return cnt;
}

// screen_region_scores_kernel with the rectangles in REFERENCE bins: rectangle k = (i0, i1, j0, j1) takes the alt pairs (i, j) with map i in [i0, i1) and
// map j in [j0, j1); signed[b][k] = mean of alt[i][j] - ref[map i][map j] over them, absm[b][k] = mean of its absolute value, both NaN when no pair
// qualifies (the region was deleted).  One workgroup per (map, rectangle): wave 0 lists the qualifying alt rows, wave 1 the columns (ascending, in LDS),
// then all four waves walk the pairs.  fp64 differences and sums in a fixed order, as there.
static __global__ void __launch_bounds__(256) screen_aligned_region_scores_kernel(const float* __restrict__ alt, long map_bs, const float* __restrict__ ref, int n,
                                                                                  const int* __restrict__ bin_map, const int* __restrict__ rects, int K,
                                                                                  float* __restrict__ signed_out, float* __restrict__ abs_out) {
  __shared__ int s_map[SCREEN_ALIGNED_MAX_BINS], s_rows[SCREEN_ALIGNED_MAX_BINS], s_cols[SCREEN_ALIGNED_MAX_BINS];
  __shared__ int s_cnt[2];
  __shared__ double s_sum[4], s_abs[4];
  const int b = blockIdx.x, k = blockIdx.y, lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  n = n > SCREEN_ALIGNED_MAX_BINS ? SCREEN_ALIGNED_MAX_BINS : n;
  int i0 = rects[4 * k], i1 = rects[4 * k + 1], j0 = rects[4 * k + 2], j1 = rects[4 * k + 3];
  i0 = i0 < 0 ? 0 : i0; j0 = j0 < 0 ? 0 : j0;
  i1 = i1 > n ? n : i1; j1 = j1 > n ? n : j1;
  screen_load_bin_map(bin_map + (long)b * n, n, s_map);
  __syncthreads();
  if (wv == 0) {
    const int h = screen_bins_in(s_map, n, i0, i1, s_rows, lane);
    if (lane == 0) s_cnt[0] = h;
  } else if (wv == 1) {
    const int w = screen_bins_in(s_map, n, j0, j1, s_cols, lane);
    if (lane == 0) s_cnt[1] = w;
  }
  __syncthreads();
  const int h = s_cnt[0], w = s_cnt[1];
  const float* a = alt + (long)b * map_bs;
  double sum = 0.0, asum = 0.0;
  for (int e = threadIdx.x; e < h * w; e += 256) {
    const int i = s_rows[e / w], j = s_cols[e % w];
    const double d = (double)a[(long)i * n + j] - (double)ref[(long)s_map[i] * n + s_map[j]];
    sum += d;
    asum += fabs(d);
  }
  for (int o = 32; o > 0; o >>= 1) {
    sum += __shfl_xor(sum, o, 64);
    asum += __shfl_xor(asum, o, 64);
  }
  if (lane == 0) { s_sum[wv] = sum; s_abs[wv] = asum; }
  __syncthreads();
  if (threadIdx.x == 0) {
    const double cnt = (double)h * (double)w;
    const double t = (s_sum[0] + s_sum[1]) + (s_sum[2] + s_sum[3]), ta = (s_abs[0] + s_abs[1]) + (s_abs[2] + s_abs[3]);
    const float qnan = __int_as_float(0x7fc00000);
    signed_out[(long)b * K + k] = h * w > 0 ? (float)(t / cnt) : qnan;
    abs_out[(long)b * K + k] = h * w > 0 ? (float)(ta / cnt) : qnan;
  }
}

// ---- tracks (screen.screen_1m(..., insulation=, viewpoints=)): 1-D readouts per map, bin with bin and on aligned bins -----------------------------------
// The diamond of bin i at width w is rows [i - w, i) x columns (i, i + w] of a map: it fits when w <= i < n - w, and ins_w(m)[i] is the mean of m over it
// (lower = more insulated), NaN where it does not fit.  Every diamond is summed on its own - no running update from bin to bin - so a NaN pixel shows in
// the bins whose diamond holds it and in no other, and the order of every sum is fixed by (n, w) alone.
#define SCREEN_INSULATION_MAX_WIDTHS 8
#define SCREEN_INSULATION_MAX_WIDTH 128
#define SCREEN_INSULATION_BINS 32          // bins per workgroup: 4 waves, 8 bins each
#define SCREEN_VIEWPOINTS_MAX 64

// the sum of the diamond of bin i (which fits) over map m, in every lane of the wave: element e = row * w + column goes to lane e % 64, so consecutive
// lanes read consecutive columns; fp64 per lane in ascending e, then the shuffles
static __device__ __forceinline__ double screen_diamond_sum(const float* __restrict__ m, int n, int i, int w, int lane) {
  const float* d = m + (long)(i - w) * n + (i + 1);
  double s = 0.0;
  int r = lane / w, c = lane - r * w;
  const int dr = 64 / w, dc = 64 - dr * w;             // e += 64 moves (r, c) by (dr, dc), carrying once
  for (int e = lane; e < w * w; e += 64) {
    s += (double)d[(long)r * n + c];
    r += dr;
    c += dc;
    if (c >= w) { c -= w; ++r; }
  }
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
  return s;
}

// insulation tracks of B alt maps [B][n][n] (batch stride map_bs) at W widths (int32, 1 .. SCREEN_INSULATION_MAX_WIDTH - the host entry point checks
// them; any other width reads as one that fits nowhere): track[b][k][i] = ins_wk(alt b)[i]; with ref [n][n], delta[b][k][i] = ins(alt b)[i] - ins(ref)[i]
// (the difference of the two fp64 means, rounded once); with the bin map, aligned[b][k][i] = ins(alt b)[i] - ins(ref)[map i] where map i >= 0 and the
// reference diamond fits at map i, else NaN - only the centre bin has to be mapped.  ref, delta, aligned and bin_map may each be NULL (the host entry
// point says which combinations).  One workgroup per (map, width, SCREEN_INSULATION_BINS bins), one wave per bin at a time; the pixels come from global
// memory (a map does not fit LDS; neighbouring diamonds overlap, so the re-reads hit L2).  Where map i == i the aligned value is the delta's expression.
// PAIRED (orca_screen_paired_insulation): map b has a reference of its own, ref + b * ref_bs, and the `delta` slot takes ref_track[b][k][i] = ins_wk(ref b)[i]
// at the reference's own bin i instead of the difference; track and aligned are the expressions above, so the same bits for the same (alt, ref, map).
template <bool PAIRED>
static __device__ __forceinline__ void screen_insulation_body(const float* __restrict__ alt, long map_bs, const float* __restrict__ ref, long ref_bs, int n,
                                                              const int* __restrict__ widths, int W, const int* __restrict__ bin_map,
                                                              float* __restrict__ track, float* __restrict__ delta, float* __restrict__ aligned) {
  __shared__ int s_map[SCREEN_ALIGNED_MAX_BINS];
  const int b = blockIdx.x, k = blockIdx.y, lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  n = n > SCREEN_ALIGNED_MAX_BINS ? SCREEN_ALIGNED_MAX_BINS : n;
  if (bin_map) screen_load_bin_map(bin_map + (long)b * n, n, s_map);
  __syncthreads();
  if (PAIRED) ref += (long)b * ref_bs;
  int w = widths[k];
  w = (w >= 1 && w <= SCREEN_INSULATION_MAX_WIDTH) ? w : n;          // n fits nowhere
  const double ww = (double)w * (double)w;
  const float* a = alt + (long)b * map_bs;
  const float qnan = __int_as_float(0x7fc00000);
  const int i0 = blockIdx.z * SCREEN_INSULATION_BINS;
  for (int i = i0 + wv; i < i0 + SCREEN_INSULATION_BINS && i < n; i += 4) {         // wave-uniform
    const long at = ((long)b * W + k) * n + i;
    const bool fits = i >= w && i < n - w;
    const double ia = fits ? screen_diamond_sum(a, n, i, w, lane) / ww : 0.0;
    const double ir = (fits && ref && (delta || aligned)) ? screen_diamond_sum(ref, n, i, w, lane) / ww : 0.0;
    float al = qnan;
    if (aligned && fits) {
      const int r = bin_map ? s_map[i] : -1;
      if (r == i) al = (float)(ia - ir);
      else if (r >= w && r < n - w && ref) al = (float)(ia - screen_diamond_sum(ref, n, r, w, lane) / ww);
    }
    if (lane == 0) {
      track[at] = fits ? (float)ia : qnan;
      if (delta) delta[at] = (fits && ref) ? (PAIRED ? (float)ir : (float)(ia - ir)) : qnan;
      if (aligned) aligned[at] = al;
    }
  }
}

static __global__ void __launch_bounds__(256) screen_insulation_kernel(const float* __restrict__ alt, long map_bs, const float* __restrict__ ref, int n,
                                                                       const int* __restrict__ widths, int W, const int* __restrict__ bin_map,
                                                                       float* __restrict__ track, float* __restrict__ delta, float* __restrict__ aligned) {
  screen_insulation_body<false>(alt, map_bs, ref, 0, n, widths, W, bin_map, track, delta, aligned);
}

static __global__ void __launch_bounds__(256) screen_paired_insulation_kernel(const float* __restrict__ alt, long alt_bs, const float* __restrict__ ref, long ref_bs,
                                                                              int n, const int* __restrict__ widths, int W, const int* __restrict__ bin_map,
                                                                              float* __restrict__ track, float* __restrict__ ref_track,
                                                                              float* __restrict__ aligned) {
  screen_insulation_body<true>(alt, alt_bs, ref, ref_bs, n, widths, W, bin_map, track, ref_track, aligned);
}

// viewpoint profiles (virtual 4C) of B alt maps [B][n][n] (batch stride map_bs) against ref [n][n] at V viewpoint bins (int32, 0 .. n - 1 - the host
// entry point checks them; clipped here all the same): delta[b][v][j] = alt[b][view][j] - ref[view][j], an fp32 subtraction.  With the bin map the
// viewpoint is a REFERENCE bin: R = the alt bins i with map i == view, ascending, c = |R|; aligned[b][v][j] = (sum_{i in R} alt[b][i][j]) / c -
// ref[view][map j] in fp64 where c >= 1 and map j >= 0 (for c = 1 the fp32 subtraction itself), else NaN - the viewpoint was deleted, or column j stands
// for nothing.  One workgroup per (map, viewpoint), one thread per column: wave 0 lists R in LDS, then every thread walks R down its own column
// (coalesced along the row) and gathers the reference row through the LDS bin map.  bin_map and aligned are NULL together.
// PAIRED (orca_screen_paired_viewpoints): map b has a reference of its own, ref + b * ref_bs, and a view list of its own, views + b * V, whose entries may
// be -1 ("not in this pair's window": c = 0, nothing is read); count[b][v] = c goes out, delta is not written (a pair's two maps share no bin grid).
template <bool PAIRED>
static __device__ __forceinline__ void screen_viewpoints_body(const float* __restrict__ alt, long map_bs, const float* __restrict__ ref, long ref_bs, int n,
                                                              const int* __restrict__ views, int V, const int* __restrict__ bin_map,
                                                              float* __restrict__ delta, float* __restrict__ aligned, int* __restrict__ count) {
  __shared__ int s_map[SCREEN_ALIGNED_MAX_BINS], s_rows[SCREEN_ALIGNED_MAX_BINS];
  __shared__ int s_cnt;
  const int b = blockIdx.x, v = blockIdx.y, lane = threadIdx.x & 63, wv = threadIdx.x >> 6, j = threadIdx.x;
  n = n > SCREEN_ALIGNED_MAX_BINS ? SCREEN_ALIGNED_MAX_BINS : n;
  int view = views[PAIRED ? b * V + v : v];
  const bool absent = PAIRED && (view < 0 || view > n - 1);
  view = view < 0 ? 0 : (view > n - 1 ? n - 1 : view);
  const bool al = bin_map && aligned;
  if (al) screen_load_bin_map(bin_map + (long)b * n, n, s_map);
  __syncthreads();
  if (al && wv == 0) {
    const int c = absent ? 0 : screen_bins_in(s_map, n, view, view + 1, s_rows, lane);
    if (lane == 0) {
      s_cnt = c;
      if (PAIRED) count[(long)b * V + v] = c;
    }
  }
  __syncthreads();
  if (j >= n) return;
  const float* a = alt + (long)b * map_bs;
  const long at = ((long)b * V + v) * n + j;
  if (PAIRED) ref += (long)b * ref_bs;
  else delta[at] = a[(long)view * n + j] - ref[(long)view * n + j];
  if (!al) return;
  const int c = s_cnt, mj = s_map[j];
  float out = __int_as_float(0x7fc00000);
  if (c == 1 && mj >= 0) {
    out = a[(long)s_rows[0] * n + j] - ref[(long)view * n + mj];
  } else if (c > 1 && mj >= 0) {
    double s = 0.0;
    for (int t = 0; t < c; ++t) s += (double)a[(long)s_rows[t] * n + j];
    out = (float)(s / (double)c - (double)ref[(long)view * n + mj]);
  }
  aligned[at] = out;
}

static __global__ void __launch_bounds__(256) screen_viewpoints_kernel(const float* __restrict__ alt, long map_bs, const float* __restrict__ ref, int n,
                                                                       const int* __restrict__ views, int V, const int* __restrict__ bin_map,
                                                                       float* __restrict__ delta, float* __restrict__ aligned) {
  screen_viewpoints_body<false>(alt, map_bs, ref, 0, n, views, V, bin_map, delta, aligned, nullptr);
}

static __global__ void __launch_bounds__(256) screen_paired_viewpoints_kernel(const float* __restrict__ alt, long alt_bs, const float* __restrict__ ref, long ref_bs,
                                                                              int n, const int* __restrict__ views, int V, const int* __restrict__ bin_map,
                                                                              float* __restrict__ aligned, int* __restrict__ count) {
  screen_viewpoints_body<true>(alt, alt_bs, ref, ref_bs, n, views, V, bin_map, nullptr, aligned, count);
}

// ---- distance strata (screen.screen_1m(..., strata=)): similarity of an alt map to the reference, stratified by genomic distance ------------------------
// Stratum d of an [n, n] map is the pairs (i, i + d), 0 <= i < n - d: the upper triangle, diagonal included, is all that is read.  For a pair x = the
// alt pixel and y = ref[i][i + d] or, with the bin map, ref[map i][map (i + d)] for the pairs whose two bins are mapped (the stratum is the ALT
// distance); both converted to fp64 first, c_d = the number of pairs.  Two passes per stratum, each for i ascending from 0.0: the means mx_d, my_d (one
// division by c_d), then the centred sums X_d = sum (x - mx_d)^2, Y_d = sum (y - my_d)^2, C_d = sum (x - mx_d)(y - my_d) and, with dl = x - y, sum dl,
// sum |dl|, sum dl^2.  include/orca_hip.h (orca_screen_strata_scores) says what is made of them.  One workgroup of 256 threads per map, thread t owns
// stratum d = t and walks its own diagonal (address stride n + 1): at a fixed i the lanes of a wave read consecutive addresses a[i n + i + d], so the
// loads stay coalesced while every stratum is summed by one thread, sequentially, in an order fixed by (n, the bin map) alone - no shuffles, no
// atomics, and a map's bits depend neither on B nor on its place in the batch.  The per-stratum sums go to LDS and thread 0 combines the strata
// [d_lo, d_hi) serially for d ascending (empty strata skipped).  The aligned branch differs in the indices of y alone, so where the bin map is the
// identity it evaluates the bin-with-bin expressions: the same bits.  A NaN pixel at a pair of stratum d enters that stratum's sums and, through
// them, the per-map scores if d_lo <= d < d_hi; unmapped pairs and the lower triangle are never read.
// PAIRED (orca_screen_paired_strata_scores): map b has a reference of its own, ref + b * ref_bs, and y = ref_b[min(mi, mj)][max(mi, mj)] with mi = map i,
// mj = map (i + d): inside an inversion the bin map descends and (mi, mj) would lie below the reference's diagonal, which holds the same contact but is
// outside this kernel's contract - the mirrored pixel is read instead, so the lower side of neither map is ever touched.  Where the bin map does not
// descend nothing is swapped: the unpaired expressions, the same bits.
template <bool PAIRED>
static __device__ __forceinline__ void screen_strata_scores_body(const float* __restrict__ alt, long map_bs, const float* __restrict__ ref, long ref_bs, int n,
                                                                 const int* __restrict__ bin_map, int d_lo, int d_hi,
                                                                 float* __restrict__ dist_delta, float* __restrict__ dist_abs,
                                                                 float* __restrict__ dist_rms, double* __restrict__ dist_corr,
                                                                 int* __restrict__ dist_count, float* __restrict__ mse,
                                                                 double* __restrict__ corr, double* __restrict__ scc) {
  __shared__ int s_map[SCREEN_ALIGNED_MAX_BINS], s_c[SCREEN_ALIGNED_MAX_BINS];
  __shared__ double s_mx[SCREEN_ALIGNED_MAX_BINS], s_my[SCREEN_ALIGNED_MAX_BINS], s_X[SCREEN_ALIGNED_MAX_BINS], s_Y[SCREEN_ALIGNED_MAX_BINS],
      s_C[SCREEN_ALIGNED_MAX_BINS], s_Q[SCREEN_ALIGNED_MAX_BINS];
  const int b = blockIdx.x, d = threadIdx.x;
  n = n > SCREEN_ALIGNED_MAX_BINS ? SCREEN_ALIGNED_MAX_BINS : n;
  d_lo = d_lo < 0 ? 0 : d_lo;
  d_hi = d_hi > n ? n : d_hi;
  const bool al = bin_map != nullptr;
  if (al) screen_load_bin_map(bin_map + (long)b * n, n, s_map);
  __syncthreads();
  const float* a = alt + (long)b * map_bs;
  if (PAIRED) ref += (long)b * ref_bs;
  const float qnan = __int_as_float(0x7fc00000);
  const double dnan = (double)qnan;
  if (d < n) {
    int c = 0;
    double sx = 0.0, sy = 0.0;
    for (int i = 0; i + d < n; ++i) {
      int ri = i, rj = i + d;
      if (al) {
        ri = s_map[i];
        rj = s_map[i + d];
        if (ri < 0 || rj < 0) continue;
        if (PAIRED && ri > rj) { const int t = ri; ri = rj; rj = t; }
      }
      sx += (double)a[(long)i * n + i + d];
      sy += (double)ref[(long)ri * n + rj];
      ++c;
    }
    const double cd = (double)c;
    const double mx = sx / cd, my = sy / cd;             // c = 0: never used
    double X = 0.0, Y = 0.0, C = 0.0, sd = 0.0, sa = 0.0, sq = 0.0;
    for (int i = 0; i + d < n; ++i) {
      int ri = i, rj = i + d;
      if (al) {
        ri = s_map[i];
        rj = s_map[i + d];
        if (ri < 0 || rj < 0) continue;
        if (PAIRED && ri > rj) { const int t = ri; ri = rj; rj = t; }
      }
      const double x = (double)a[(long)i * n + i + d], y = (double)ref[(long)ri * n + rj];
      const double ex = x - mx, ey = y - my, dl = x - y;
      X += ex * ex;
      Y += ey * ey;
      C += ex * ey;
      sd += dl;
      sa += fabs(dl);
      sq += dl * dl;
    }
    s_c[d] = c;
    s_mx[d] = mx; s_my[d] = my;
    s_X[d] = X; s_Y[d] = Y; s_C[d] = C; s_Q[d] = sq;
    const long at = (long)b * n + d;
    dist_delta[at] = c > 0 ? (float)(sd / cd) : qnan;
    dist_abs[at] = c > 0 ? (float)(sa / cd) : qnan;
    dist_rms[at] = c > 0 ? (float)sqrt(sq / cd) : qnan;
    dist_corr[at] = (c < 2 || X == 0.0 || Y == 0.0) ? dnan : C / sqrt(X * Y);
    if (dist_count) dist_count[at] = c;
  }
  __syncthreads();
  if (threadIdx.x != 0) return;
  long c = 0;
  double q = 0.0, num = 0.0, den = 0.0, wx = 0.0, wy = 0.0;
  for (int k = d_lo; k < d_hi; ++k) {
    if (s_c[k] == 0) continue;
    const double ck = (double)s_c[k];
    c += s_c[k];
    q += s_Q[k];
    num += s_C[k];
    den += sqrt(s_X[k] * s_Y[k]);
    wx += ck * s_mx[k];
    wy += ck * s_my[k];
  }
  if (c == 0) {
    mse[b] = qnan;
    corr[b] = dnan;
    scc[b] = dnan;
    return;
  }
  const double cc = (double)c, mx = wx / cc, my = wy / cc;
  double X = 0.0, Y = 0.0, C = 0.0;
  for (int k = d_lo; k < d_hi; ++k) {
    if (s_c[k] == 0) continue;
    const double ck = (double)s_c[k], ex = s_mx[k] - mx, ey = s_my[k] - my;
    X += s_X[k] + ck * (ex * ex);
    Y += s_Y[k] + ck * (ey * ey);
    C += s_C[k] + ck * (ex * ey);
  }
  mse[b] = (float)(q / cc);
  scc[b] = den == 0.0 ? dnan : num / den;
  corr[b] = (c < 2 || X == 0.0 || Y == 0.0) ? dnan : C / sqrt(X * Y);
}

static __global__ void __launch_bounds__(256) screen_strata_scores_kernel(const float* __restrict__ alt, long map_bs, const float* __restrict__ ref, int n,
                                                                          const int* __restrict__ bin_map, int d_lo, int d_hi,
                                                                          float* __restrict__ dist_delta, float* __restrict__ dist_abs,
                                                                          float* __restrict__ dist_rms, double* __restrict__ dist_corr,
                                                                          int* __restrict__ dist_count, float* __restrict__ mse,
                                                                          double* __restrict__ corr, double* __restrict__ scc) {
  screen_strata_scores_body<false>(alt, map_bs, ref, 0, n, bin_map, d_lo, d_hi, dist_delta, dist_abs, dist_rms, dist_corr, dist_count, mse, corr, scc);
}

static __global__ void __launch_bounds__(256) screen_paired_strata_scores_kernel(const float* __restrict__ alt, long alt_bs, const float* __restrict__ ref,
                                                                                 long ref_bs, int n, const int* __restrict__ bin_map, int d_lo, int d_hi,
                                                                                 float* __restrict__ dist_delta, float* __restrict__ dist_abs,
                                                                                 float* __restrict__ dist_rms, double* __restrict__ dist_corr,
                                                                                 int* __restrict__ dist_count, float* __restrict__ mse,
                                                                                 double* __restrict__ corr, double* __restrict__ scc) {
  screen_strata_scores_body<true>(alt, alt_bs, ref, ref_bs, n, bin_map, d_lo, d_hi, dist_delta, dist_abs, dist_rms, dist_corr, dist_count, mse, corr, scc);
}

// ---- paired aligned scores (sv.sv_screen(..., scores=)): B alt maps, each against a reference map OF ITS OWN through its bin map --------------------------
// include/orca_hip.h (orca_screen_paired_aligned_scores) has the definitions.  Pair b is alt + b * alt_bs against ref + b * ref_bs; M = {i : map i >= 0},
// c = |M|, and over the c^2 pairs (i, j) of M x M: x = alt[i][j], y = ref[map i][map j], dl = x - y, all fp64.  One workgroup of 8 waves per pair with the
// bin map in LDS, in the mould of screen_aligned_scores_kernel: wave w takes the alt rows w, w + 8, .., lane l the columns l, l + 64, .. - the alt row is
// read along its columns, the reference row `map i` at columns `map j` (runs of consecutive addresses, ascending or, inside an inversion, descending).
// Two passes over the maps: (1) sum x, sum y, sum dl, sum |dl| (also per row: the profile), sum dl^2, max |dl|; thread 0 makes the means mx, my of them;
// (2) the centred sums X, Y, C.  The second pass re-reads what the first just touched (2 x 250 KB: it sits in L2); nothing is staged.  Every thread adds
// its terms in the order it meets them, a sum crosses the lanes by xor shuffles (every lane ends with the same bits) and the 8 waves' sums are combined
// serially by thread 0, wave 0 first: no atomics, and the order of every sum is fixed by (n, the bin map) alone - a pair's bits depend neither on B nor on
// its place in the batch nor on the strides.  Only mapped pairs are read.  A NaN at one makes sum |dl| NaN, and with it every scalar (the maximum by an
// explicit test: fmax drops a NaN) and the row's profile.
static __device__ __forceinline__ double screen_wave_sum(double v) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

static __global__ void __launch_bounds__(512) screen_paired_aligned_scores_kernel(const float* __restrict__ alt, long alt_bs, const float* __restrict__ ref,
                                                                                  long ref_bs, int n, const int* __restrict__ bin_map,
                                                                                  float* __restrict__ profile, float* __restrict__ abs_mean,
                                                                                  float* __restrict__ abs_max, float* __restrict__ delta_mean,
                                                                                  float* __restrict__ rms, double* __restrict__ corr, int* __restrict__ count) {
  __shared__ int s_map[SCREEN_ALIGNED_MAX_BINS];
  __shared__ double s_red[8][6], s_mean[2];
  const int b = blockIdx.x, lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  n = n > SCREEN_ALIGNED_MAX_BINS ? SCREEN_ALIGNED_MAX_BINS : n;
  const int mine = screen_load_bin_map(bin_map + (long)b * n, n, s_map);
  const int c = __syncthreads_count(mine >= 0);
  const float* a = alt + (long)b * alt_bs;
  const float* r = ref + (long)b * ref_bs;
  const float qnan = __int_as_float(0x7fc00000);
  const double dnan = (double)qnan, cc = (double)c * (double)c;
  double sx = 0.0, sy = 0.0, sd = 0.0, sq = 0.0, sa = 0.0, mx_abs = 0.0;
  for (int i = wv; i < n; i += 8) {
    const int mi = s_map[i];                         // wave-uniform
    if (mi < 0) {
      if (lane == 0) profile[(long)b * n + i] = qnan;
      continue;
    }
    double rs = 0.0;
    for (int j = lane; j < n; j += 64) {
      const int mj = s_map[j];
      if (mj < 0) continue;
      const double x = (double)a[(long)i * n + j], y = (double)r[(long)mi * n + mj];
      const double dl = x - y, ad = fabs(dl);
      sx += x;
      sy += y;
      sd += dl;
      sq += dl * dl;
      rs += ad;
      mx_abs = fmax(mx_abs, ad);
    }
    rs = screen_wave_sum(rs);
    if (lane == 0) profile[(long)b * n + i] = (float)(rs / (double)c);
    sa += rs;                                        // the same in every lane
  }
  sx = screen_wave_sum(sx);
  sy = screen_wave_sum(sy);
  sd = screen_wave_sum(sd);
  sq = screen_wave_sum(sq);
  for (int o = 32; o > 0; o >>= 1) mx_abs = fmax(mx_abs, __shfl_xor(mx_abs, o, 64));
  if (lane == 0) {
    s_red[wv][0] = sx; s_red[wv][1] = sy; s_red[wv][2] = sd; s_red[wv][3] = sq; s_red[wv][4] = sa; s_red[wv][5] = mx_abs;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    double tx = 0.0, ty = 0.0, td = 0.0, tq = 0.0, ta = 0.0, tm = 0.0;
    for (int k = 0; k < 8; ++k) {
      tx += s_red[k][0]; ty += s_red[k][1]; td += s_red[k][2]; tq += s_red[k][3]; ta += s_red[k][4];
      tm = fmax(tm, s_red[k][5]);
    }
    s_mean[0] = tx / cc;                             // c = 0: never used
    s_mean[1] = ty / cc;
    const bool none = c == 0;
    abs_mean[b] = none ? qnan : (float)(ta / cc);
    abs_max[b] = (none || ta != ta) ? qnan : (float)tm;
    delta_mean[b] = none ? qnan : (float)(td / cc);
    rms[b] = none ? qnan : (float)sqrt(tq / cc);
    count[b] = c;
  }
  __syncthreads();                                   // the means are there, and s_red has been read
  const double mx = s_mean[0], my = s_mean[1];
  double X = 0.0, Y = 0.0, C = 0.0;
  for (int i = wv; i < n; i += 8) {
    const int mi = s_map[i];
    if (mi < 0) continue;
    for (int j = lane; j < n; j += 64) {
      const int mj = s_map[j];
      if (mj < 0) continue;
      const double ex = (double)a[(long)i * n + j] - mx, ey = (double)r[(long)mi * n + mj] - my;
      X = fma(ex, ex, X);                            // spelled out: where alt and ref hold the same bits, X, Y and C do too
      Y = fma(ey, ey, Y);
      C = fma(ex, ey, C);
    }
  }
  X = screen_wave_sum(X);
  Y = screen_wave_sum(Y);
  C = screen_wave_sum(C);
  if (lane == 0) {
    s_red[wv][0] = X; s_red[wv][1] = Y; s_red[wv][2] = C;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    double tX = 0.0, tY = 0.0, tC = 0.0;
    for (int k = 0; k < 8; ++k) {
      tX += s_red[k][0]; tY += s_red[k][1]; tC += s_red[k][2];
    }
    corr[b] = (c < 2 || tX == 0.0 || tY == 0.0) ? dnan : tC / sqrt(tX * tY);
  }
}

// ---- loops (screen.screen_1m(..., loops=)): dot calls per map, HiCCUPS' neighbourhoods on the model's log observed / expected ---------------------------
// include/orca_hip.h (orca_screen_dot_calls) has the definitions: the eligible pixels, the five sets P, D, LL, H, V of offsets (a, b) with |a|, |b| <= w,
// the enrichment e = mean P - max(mean D, mean LL, mean H, mean V) and what makes a pixel a dot.  screen_dot_enrich is the one place e is computed: `m`
// points at the pixel, `ld` is the row stride of the image it sits in (the map itself, or a row band of it in LDS).  Each set has its own fp64 sum, taken
// over the window row by row (a ascending, then b ascending), then one division by the set's count; no product anywhere, so nothing for the compiler to
// contract, and the bits do not depend on where the image lies.  The five sets cover the whole window, so a NaN anywhere in it makes e NaN.
#define SCREEN_DOT_MAX_W 16
#define SCREEN_DOT_MAX_R 16
#define SCREEN_DOT_MAX_CALLS 4096

static __device__ __forceinline__ bool screen_dot_eligible(int i, int j, int n, int w, int d_min) { return i >= w && j <= n - 1 - w && j - i >= d_min; }

static __device__ __forceinline__ float screen_dot_enrich(const float* m, int ld, int p, int w) {
  double sP = 0.0, sD = 0.0, sL = 0.0, sH = 0.0, sV = 0.0;
  int cP = 0, cD = 0, cL = 0, cH = 0, cV = 0;
  for (int a = -w; a <= w; ++a) {
    const int aa = a < 0 ? -a : a;
    const float* row = m + a * ld;
    for (int b = -w; b <= w; ++b) {
      const int ab = b < 0 ? -b : b;
      const double x = (double)row[b];
      if (aa <= p && ab <= p) {
        sP += x; ++cP;
      } else {
        if (a != 0 && b != 0) { sD += x; ++cD; }
        if (a >= 1 && b <= -1) { sL += x; ++cL; }
      }
      if (aa <= 1 && ab > p) { sH += x; ++cH; }
      if (ab <= 1 && aa > p) { sV += x; ++cV; }
    }
  }
  const double mP = sP / (double)cP, mD = sD / (double)cD, mL = sL / (double)cL, mH = sH / (double)cH, mV = sV / (double)cV;
  double bg = mD;
  if (mL > bg) bg = mL;
  if (mH > bg) bg = mH;
  if (mV > bg) bg = mV;
  const double e = mP - bg;
  return (mP != mP || mD != mD || mL != mL || mH != mH || mV != mV) ? __int_as_float(0x7fc00000) : (float)e;
}

// The enrichment map e[b][i][j] of B maps: NaN at every ineligible pixel.  One workgroup of 256 threads per (map, row i), thread t owns column j = t.
// The eligible pixels of row i are columns i + d_min .. n - 1 - w and their windows lie in rows i - w .. i + w, columns c0 = i + d_min - w .. n - 1:
// strictly above the diagonal (d_min >= 2 w + 1) and all that is read.  That band goes to LDS once - (2 w + 1) rows of 256 floats, row r, column c at
// s_band[r][c - c0], filled with consecutive lanes on consecutive addresses - and every window is summed from there: at a fixed (a, b) the lanes read
// consecutive LDS words, no bank conflict.  A row without an eligible pixel stages nothing.
static __global__ void __launch_bounds__(256) screen_dot_enrich_map_kernel(const float* __restrict__ maps, long map_bs, int n, int p, int w, int d_min,
                                                                           float* __restrict__ e_map) {
  __shared__ float s_band[2 * SCREEN_DOT_MAX_W + 1][SCREEN_ALIGNED_MAX_BINS];
  const int b = blockIdx.x, i = blockIdx.y, j = threadIdx.x;
  n = n > SCREEN_ALIGNED_MAX_BINS ? SCREEN_ALIGNED_MAX_BINS : n;
  w = w > SCREEN_DOT_MAX_W ? SCREEN_DOT_MAX_W : (w < 1 ? 1 : w);
  p = p >= w ? w - 1 : (p < 0 ? 0 : p);
  d_min = d_min < 2 * w + 1 ? 2 * w + 1 : d_min;
  if (i >= n) return;
  const float qnan = __int_as_float(0x7fc00000);
  float* out = e_map + ((long)b * n + i) * n;
  const bool row_ok = i >= w && i <= n - 1 - w - d_min;          // wave-uniform: some column of row i is eligible
  if (!row_ok) {
    if (j < n) out[j] = qnan;
    return;
  }
  const int c0 = i + d_min - w, nc = n - c0, rows = 2 * w + 1;   // c0 >= w + 1 + i > i + w; 2 w + 1 <= nc <= 256
  const float* src = maps + (long)b * map_bs + (long)(i - w) * n + c0;
  for (int r = 0; r < rows; ++r)
    for (int c = j; c < nc; c += 256) s_band[r][c] = src[(long)r * n + c];
  __syncthreads();
  if (j >= n) return;
  out[j] = screen_dot_eligible(i, j, n, w, d_min) ? screen_dot_enrich(&s_band[w][j - c0], SCREEN_ALIGNED_MAX_BINS, p, w) : qnan;
}

// e at Q listed pixels (i, j) of each map, NaN for (-1, -1) and every other ineligible pixel: one thread per pixel, the windows read from the map itself
// with the device function of the kernel above - the same sums in the same order, the same bits.
static __global__ void __launch_bounds__(256) screen_dot_enrichment_kernel(const float* __restrict__ maps, long map_bs, int n, int p, int w, int d_min,
                                                                           const int* __restrict__ pixels, int Q, float* __restrict__ out) {
  const int b = blockIdx.x, q = blockIdx.y * 256 + threadIdx.x;
  n = n > SCREEN_ALIGNED_MAX_BINS ? SCREEN_ALIGNED_MAX_BINS : n;
  w = w > SCREEN_DOT_MAX_W ? SCREEN_DOT_MAX_W : (w < 1 ? 1 : w);
  p = p >= w ? w - 1 : (p < 0 ? 0 : p);
  d_min = d_min < 2 * w + 1 ? 2 * w + 1 : d_min;
  if (q >= Q) return;
  const long at = (long)b * Q + q;
  const int i = pixels[2 * at], j = pixels[2 * at + 1];
  const bool ok = i >= 0 && j >= 0 && j < n && screen_dot_eligible(i, j, n, w, d_min);
  out[at] = ok ? screen_dot_enrich(maps + (long)b * map_bs + (long)i * n + j, n, p, w) : __int_as_float(0x7fc00000);
}

// The dots of each map from its enrichment map (written by screen_dot_enrich_map_kernel, an earlier launch on the same stream), listed in row-major
// order.  One workgroup of 256 threads per map walks the rows that hold eligible pixels, thread t at column j = t.  Pixel (i, j) is a dot when e is not
// NaN, e >= T and, for every pixel within Chebyshev distance r whose e is not NaN (ineligible pixels hold NaN), e > e' where (i', j') precedes (i, j)
// in row-major order and e >= e' where it follows: comparisons of fp32 values, so of two equal neighbours exactly the first is a dot.  The order comes
// from a ballot per wave, the four waves' counts through LDS (two buffers, one barrier per row) and a running base that every thread keeps: no atomics,
// and a map's list depends on the map alone.  count = the number of dots; the first K are written, the rest of the K slots get -1 / NaN.
static __global__ void __launch_bounds__(256) screen_dot_calls_kernel(const float* __restrict__ e_map, int n, int w, int d_min, int r, float T, int K,
                                                                      int* __restrict__ count, int* __restrict__ ij, float* __restrict__ enrich) {
  __shared__ int s_wave[2][4];
  const int b = blockIdx.x, j = threadIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  n = n > SCREEN_ALIGNED_MAX_BINS ? SCREEN_ALIGNED_MAX_BINS : n;
  w = w > SCREEN_DOT_MAX_W ? SCREEN_DOT_MAX_W : (w < 1 ? 1 : w);
  d_min = d_min < 2 * w + 1 ? 2 * w + 1 : d_min;
  r = r > SCREEN_DOT_MAX_R ? SCREEN_DOT_MAX_R : (r < 1 ? 1 : r);
  K = K < 0 ? 0 : K;
  const float* e = e_map + (long)b * n * n;
  int* my_ij = ij + (long)b * K * 2;
  float* my_en = enrich + (long)b * K;
  int base = 0;
  for (int i = w; i <= n - 1 - w - d_min; ++i) {
    bool dot = false;
    float v = 0.f;
    if (j < n && screen_dot_eligible(i, j, n, w, d_min)) {
      v = e[(long)i * n + j];
      dot = v == v && v >= T;
      const int i0 = i - r < 0 ? 0 : i - r, i1 = i + r > n - 1 ? n - 1 : i + r, j0 = j - r < 0 ? 0 : j - r, j1 = j + r > n - 1 ? n - 1 : j + r;
      for (int ii = i0; dot && ii <= i1; ++ii)
        for (int jj = j0; jj <= j1; ++jj) {
          if (ii == i && jj == j) continue;
          const float f = e[(long)ii * n + jj];
          if (f != f) continue;
          const bool before = ii < i || (ii == i && jj < j);
          if (before ? !(v > f) : !(v >= f)) dot = false;
        }
    }
    const unsigned long long mask = __ballot(dot);
    if (lane == 0) s_wave[i & 1][wave] = __popcll(mask);
    __syncthreads();
    int at = base + __popcll(mask & ((1ull << lane) - 1ull));
    for (int k = 0; k < 4; ++k) {
      const int c = s_wave[i & 1][k];
      if (k < wave) at += c;
      base += c;
    }
    if (dot && at < K) {
      my_ij[2 * at] = i;
      my_ij[2 * at + 1] = j;
      my_en[at] = v;
    }
  }
  if (threadIdx.x == 0) count[b] = base;
  for (int k = (base < K ? base : K) + threadIdx.x; k < K; k += 256) {
    my_ij[2 * k] = -1;
    my_ij[2 * k + 1] = -1;
    my_en[k] = __int_as_float(0x7fc00000);
  }
}

// ---- boundaries: domain boundary calls from insulation tracks (screen_1m(..., insulation=, boundaries=), sv.sv_screen(..., insulation=, boundaries=)) ----
// include/orca_hip.h (orca_screen_boundary_calls) has the definitions.  One workgroup of 256 threads per track, grid (B, W); the track goes to LDS once
// and thread i owns bin i.  Bin i is a minimum when 1 <= i <= n - 2, t[i - 1], t[i], t[i + 1] are not NaN, t[i] < t[i - 1] and t[i] <= t[i + 1] (the first
// bin of a plateau).  Its strength is the prominence of the dip: the thread walks left from i - 1 while the bin exists, is not NaN and is >= t[i], L = the
// largest value met (t[i] if none), R the same to the right, strength = min(L, R) - t[i] - comparisons and ONE fp32 subtraction, so the host restatement
// agrees bit for bit.  A NaN ends a walk: nothing is bridged across it.  The walks diverge by design, at most n LDS reads each way.  A minimum is a
// boundary when strength > 0 and strength >= min_strength.  The list is ascending in the bin: a ballot per wave, the four waves' counts through LDS and a
// prefix, as in screen_dot_calls_kernel - no atomics, and a track's outputs depend on the track alone.  count = all boundaries; the first K are written,
// the rest of the K slots get -1 / NaN.  strength_track (may be NULL): the strength at every minimum with strength > 0, NaN elsewhere.
static __global__ void __launch_bounds__(256) screen_boundary_calls_kernel(const float* __restrict__ tracks, int n, float min_strength, int K,
                                                                           int* __restrict__ count, int* __restrict__ bins, float* __restrict__ strength,
                                                                           float* __restrict__ strength_track) {
  __shared__ float s_t[SCREEN_ALIGNED_MAX_BINS];
  __shared__ int s_wave[4];
  const int i = threadIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long tr = (long)blockIdx.x * gridDim.y + blockIdx.y;
  const float nan = __int_as_float(0x7fc00000);
  n = n > SCREEN_ALIGNED_MAX_BINS ? SCREEN_ALIGNED_MAX_BINS : (n < 0 ? 0 : n);
  K = K < 0 ? 0 : K;
  s_t[i] = i < n ? tracks[tr * n + i] : nan;
  __syncthreads();
  float s = nan;
  if (i >= 1 && i <= n - 2) {
    const float v = s_t[i], a = s_t[i - 1], b = s_t[i + 1];
    if (v == v && a == a && b == b && v < a && v <= b) {
      float L = v, R = v;
      for (int j = i - 1; j >= 0; --j) {
        const float f = s_t[j];
        if (!(f >= v)) break;                            // lower, or NaN
        L = f > L ? f : L;
      }
      for (int j = i + 1; j < n; ++j) {
        const float f = s_t[j];
        if (!(f >= v)) break;
        R = f > R ? f : R;
      }
      s = (L < R ? L : R) - v;
    }
  }
  const bool dip = s > 0.f;                              // false for NaN: no minimum here, or a shelf
  if (strength_track && i < n) strength_track[tr * n + i] = dip ? s : nan;
  const bool call = dip && s >= min_strength;
  const unsigned long long mask = __ballot(call);
  if (lane == 0) s_wave[wave] = __popcll(mask);
  __syncthreads();
  int at = __popcll(mask & ((1ull << lane) - 1ull)), total = 0;
  for (int k = 0; k < 4; ++k) {
    const int c = s_wave[k];
    if (k < wave) at += c;
    total += c;
  }
  int* my_bins = bins + tr * K;
  float* my_st = strength + tr * K;
  if (call && at < K) {
    my_bins[at] = i;
    my_st[at] = s;
  }
  if (i == 0) count[tr] = total;
  for (int k = (total < K ? total : K) + i; k < K; k += 256) {
    my_bins[k] = -1;
    my_st[k] = nan;
  }
}

// ---- loops per level of the SV screen (sv.sv_screen(..., scores=True, loops=)): a reference dot followed through the pair's bin map ---------------------
// include/orca_hip.h (orca_screen_paired_dot_follow) has the rule.  Reference dot k = (ri, rj) of pair b, A = the alt bins a with map a = ri, C = those
// with map c = rj: the candidates are the pixels (min(a, c), max(a, c)) over A x C that are eligible in the alt map - the min/max mirrors a pixel of a
// descending bin map into the upper triangle - and the best of them goes out under ONE total order: a non-NaN e beats a NaN e, a larger e a smaller one
// (fp32 comparison), and of two equals the earlier pixel in row-major order.  A x C holds distinct pixels (ri != rj: A and C are disjoint), so the order
// is total and the result does not depend on which lane met which candidate.  e is gathered from the alt maps' enrichment map, written by an earlier
// launch on the same stream (screen_dot_enrich_map_kernel): nothing is computed here but comparisons and one fp32 subtraction.
// One workgroup of 4 waves per (pair, 4 list slots), one wave per slot: the bin map goes to LDS once, the wave lists A and C there (ascending), walks
// the |A| |C| pairs with a stride of 64 (a degenerate map has up to (n / 2)^2 of them) and reduces by shuffles.  A slot that holds no dot - anything but
// 0 <= ri < rj <= n - 1; the lists are on the device only - has no candidate and is never used as an index.  No candidate: 0, (-1, -1), NaN, NaN.
#define SCREEN_FOLLOW_DOTS 4               // list slots per workgroup: one wave each

// is candidate (e, at) better than (f, other)?  at, other: row-major pixel indices, -1 = none yet
static __device__ __forceinline__ bool screen_follow_better(float e, int at, float f, int other) {
  if (at < 0) return false;
  if (other < 0) return true;
  const bool en = e != e, fn = f != f;
  if (en != fn) return fn;
  if (!en && e != f) return e > f;
  return at < other;
}

static __global__ void __launch_bounds__(64 * SCREEN_FOLLOW_DOTS) screen_paired_dot_follow_kernel(const float* __restrict__ alt_e, long e_bs, int n, int w,
                                                                                                  int d_min, const int* __restrict__ ref_ij,
                                                                                                  const float* __restrict__ ref_enrich, int R,
                                                                                                  const int* __restrict__ bin_map, int* __restrict__ candidates,
                                                                                                  int* __restrict__ at_out, float* __restrict__ enrich,
                                                                                                  float* __restrict__ delta) {
  __shared__ int s_map[SCREEN_ALIGNED_MAX_BINS];
  __shared__ int s_a[SCREEN_FOLLOW_DOTS][SCREEN_ALIGNED_MAX_BINS], s_c[SCREEN_FOLLOW_DOTS][SCREEN_ALIGNED_MAX_BINS];
  const int b = blockIdx.x, lane = threadIdx.x & 63, wv = threadIdx.x >> 6, k = blockIdx.y * SCREEN_FOLLOW_DOTS + wv;
  n = n > SCREEN_ALIGNED_MAX_BINS ? SCREEN_ALIGNED_MAX_BINS : n;
  w = w > SCREEN_DOT_MAX_W ? SCREEN_DOT_MAX_W : (w < 1 ? 1 : w);
  d_min = d_min < 2 * w + 1 ? 2 * w + 1 : d_min;
  screen_load_bin_map(bin_map + (long)b * n, n, s_map);
  __syncthreads();
  int ri = -1, rj = -1;
  if (k < R) {
    ri = ref_ij[2 * ((long)b * R + k)];
    rj = ref_ij[2 * ((long)b * R + k) + 1];
  }
  const bool dot = ri >= 0 && ri < rj && rj <= n - 1;              // wave-uniform
  const int na = dot ? screen_bins_in(s_map, n, ri, ri + 1, s_a[wv], lane) : 0;
  const int nc = dot ? screen_bins_in(s_map, n, rj, rj + 1, s_c[wv], lane) : 0;
  __syncthreads();                                                 // the lists are read by other lanes than wrote them
  if (k >= R) return;
  const float* e = alt_e + (long)b * e_bs;
  const float qnan = __int_as_float(0x7fc00000);
  int cnt = 0, best = -1;
  float best_e = qnan;
  for (int t = lane; t < na * nc; t += 64) {
    const int a = s_a[wv][t / nc], c = s_c[wv][t % nc];
    const int i = a < c ? a : c, j = a < c ? c : a;
    if (!screen_dot_eligible(i, j, n, w, d_min)) continue;
    const int at = i * n + j;
    const float v = e[at];
    ++cnt;
    if (screen_follow_better(v, at, best_e, best)) {
      best = at;
      best_e = v;
    }
  }
  for (int o = 32; o > 0; o >>= 1) {
    cnt += __shfl_xor(cnt, o, 64);
    const int other = __shfl_xor(best, o, 64);
    const float f = __shfl_xor(best_e, o, 64);
    if (screen_follow_better(f, other, best_e, best)) {
      best = other;
      best_e = f;
    }
  }
  if (lane != 0) return;
  const long out = (long)b * R + k;
  candidates[out] = cnt;
  at_out[2 * out] = best < 0 ? -1 : best / n;
  at_out[2 * out + 1] = best < 0 ? -1 : best % n;
  enrich[out] = best < 0 ? qnan : best_e;
  delta[out] = best < 0 ? qnan : best_e - ref_enrich[out];
}

// ---- compartments per level of the SV screen (sv.sv_screen(..., scores=True, compartments=)): the K leading eigenpairs of a map ----------------------------
// include/orca_hip.h (orca_screen_eigenvectors) has the definition: the symmetrised upper triangle S, the valid bins, the kept pixels, A = S - mu on them,
// the eigenpairs of A in descending |lambda|, E_k = v_k sqrt(|lambda_k|), the sign by a phase track or by the largest component.
// One workgroup of 16 waves per map.  A IS KEPT AS THE PACKED UPPER TRIANGLE OF S IN LDS, fp32 as it came (131 584 bytes at n = 256, 125 500 at n = 250; the
// CU has 160 KiB): S[i][j], i <= j, at i n - i (i - 1) / 2 + (j - i), and A[i][j] = (double)S - mu is formed on the fly where the pixel is kept.  Every
// iteration reads all of A once; from LDS a row and a column cost the same, so nothing is symmetrised or copied and no workspace is needed.
// Deflated power iteration in fp64, per vector k: v <- start_k (screen_eig_start, on the valid bins), then per iteration: v -= u (u . v) for the earlier
// vectors u in turn, v /= |v|, w = A v, w -= u (u . w) in turn, lambda = v . w, r = |w - lambda v| / |lambda|; stop when r <= tol or after max_iter
// iterations, else v <- w.  (lambda, r) belong to the v that is kept.  r = 0 where w - lambda v is exactly 0 (also with lambda = 0: A = 0 has no kept pixel
// apart from its mean), +inf where lambda = 0 otherwise.
// The order of every sum is fixed by (n, K, d_lo, the valid bins) alone: in w = A v four threads share a row - thread q takes the columns q, q + 4, ..
// ascending - and their sums meet as (q0 + q1) + (q2 + q3) by xor shuffles; a dot product is formed by EVERY wave from the same LDS vectors - lane l takes
// the bins l, l + 64, .., then xor shuffles - so all waves hold the same bits and the loop's exit is uniform.  mu: the rows' sums (the same four-thread
// order) added serially for i ascending.  No atomics, nothing scattered: a map's bits depend neither on B nor on its place in the batch nor on the stride.
#define SCREEN_EIG_MAX_K 3
#define SCREEN_EIG_THREADS 1024
#define SCREEN_EIG_TRI (SCREEN_ALIGNED_MAX_BINS * (SCREEN_ALIGNED_MAX_BINS + 1) / 2)

// the start vector of eigenvector k at bin i: a fixed integer hash of (i, k) mapped to [-0.5, 0.5) - no bin is special, no two vectors start alike
static __device__ __forceinline__ double screen_eig_start(int i, int k) {
  unsigned h = (unsigned)(i + 1) * 2654435761u + (unsigned)(k + 1) * 40503u;
  h ^= h >> 15;
  h *= 2246822519u;
  h ^= h >> 13;
  return (double)(h >> 8) * (1.0 / 16777216.0) - 0.5;
}

// S[i][j] from the packed upper triangle
static __device__ __forceinline__ float screen_eig_s(const float* s_tri, int i, int j, int n) {
  const int lo = i < j ? i : j, hi = i < j ? j : i;
  return s_tri[lo * n - lo * (lo - 1) / 2 + (hi - lo)];
}

// a . b over the SCREEN_ALIGNED_MAX_BINS entries of two LDS vectors (0 outside the valid bins), by one wave: the same bits in every lane of every wave
static __device__ __forceinline__ double screen_eig_dot(const double* a, const double* b, int lane) {
  double s = 0.0;
  for (int j = lane; j < SCREEN_ALIGNED_MAX_BINS; j += 64) s = fma(a[j], b[j], s);
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
  return s;
}

// x -= u (u . x) on LDS vectors, by the whole workgroup
static __device__ __forceinline__ void screen_eig_deflate(double* x, const double* u, int lane) {
  const double d = screen_eig_dot(u, x, lane);
  __syncthreads();                                                 // every wave has read x
  if (threadIdx.x < SCREEN_ALIGNED_MAX_BINS) x[threadIdx.x] = fma(-d, u[threadIdx.x], x[threadIdx.x]);
  __syncthreads();
}

static __global__ void __launch_bounds__(SCREEN_EIG_THREADS) screen_eigenvectors_kernel(const float* __restrict__ maps, long map_bs, int n, int K, int d_lo,
                                                                                        int center, double tol, int max_iter,
                                                                                        const float* __restrict__ phase, float* __restrict__ E,
                                                                                        double* __restrict__ eigenvalue, double* __restrict__ residual,
                                                                                        int* __restrict__ iterations, int* __restrict__ n_valid) {
  __shared__ float s_tri[SCREEN_EIG_TRI];
  __shared__ double s_v[SCREEN_ALIGNED_MAX_BINS], s_w[SCREEN_ALIGNED_MAX_BINS], s_row[SCREEN_ALIGNED_MAX_BINS];
  __shared__ double s_u[SCREEN_EIG_MAX_K][SCREEN_ALIGNED_MAX_BINS];
  __shared__ int s_ok[SCREEN_ALIGNED_MAX_BINS], s_cnt[SCREEN_ALIGNED_MAX_BINS];
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, row = tid >> 2, q = tid & 3;
  n = n > SCREEN_ALIGNED_MAX_BINS ? SCREEN_ALIGNED_MAX_BINS : n;
  K = K > SCREEN_EIG_MAX_K ? SCREEN_EIG_MAX_K : K;
  d_lo = d_lo < 0 ? 0 : d_lo;
  const float* m = maps + (long)b * map_bs;
  const float qnan = __int_as_float(0x7fc00000);
  const double dnan = (double)qnan;
  for (int i = wave; i < n; i += SCREEN_EIG_THREADS / 64)
    for (int j = i + lane; j < n; j += 64) s_tri[i * n - i * (i - 1) / 2 + (j - i)] = m[(long)i * n + j];
  __syncthreads();
  // the valid bins: no NaN in the row of S at |i - j| >= d_lo
  int bad = 0;
  if (row < n)
    for (int j = q; j < n; j += 4) {
      const float s = screen_eig_s(s_tri, row, j, n);
      bad |= (abs(row - j) >= d_lo && s != s) ? 1 : 0;
    }
  bad |= __shfl_xor(bad, 1, 64);
  bad |= __shfl_xor(bad, 2, 64);
  if (q == 0) s_ok[row] = (row < n && !bad) ? 1 : 0;
  __syncthreads();
  int nv = 0;
  for (int j = lane; j < SCREEN_ALIGNED_MAX_BINS; j += 64) nv += s_ok[j];
  for (int o = 32; o > 0; o >>= 1) nv += __shfl_xor(nv, o, 64);
  if (tid == 0) n_valid[b] = nv;
  if (nv <= K) {                                                   // (uniform)
    for (int t = tid; t < K * n; t += SCREEN_EIG_THREADS) E[(long)b * K * n + t] = qnan;
    if (tid < K) {
      eigenvalue[(long)b * K + tid] = dnan;
      residual[(long)b * K + tid] = dnan;
      iterations[(long)b * K + tid] = 0;
    }
    return;
  }
  const bool mine = row < n && s_ok[row] != 0;
  // mu: the mean of the kept pixels
  double rs = 0.0;
  int rc = 0;
  if (mine)
    for (int j = q; j < n; j += 4)
      if (s_ok[j] && abs(row - j) >= d_lo) {
        rs += (double)screen_eig_s(s_tri, row, j, n);
        ++rc;
      }
  rs += __shfl_xor(rs, 1, 64);
  rc += __shfl_xor(rc, 1, 64);
  rs += __shfl_xor(rs, 2, 64);
  rc += __shfl_xor(rc, 2, 64);
  if (q == 0) {
    s_row[row] = rs;
    s_cnt[row] = rc;
  }
  __syncthreads();
  double mu = 0.0;
  if (center) {
    double tot = 0.0;
    long cnt = 0;
    for (int i = 0; i < n; ++i) {
      tot += s_row[i];
      cnt += s_cnt[i];
    }
    mu = cnt > 0 ? tot / (double)cnt : 0.0;
  }
  for (int k = 0; k < K; ++k) {
    if (tid < SCREEN_ALIGNED_MAX_BINS) s_v[tid] = (tid < n && s_ok[tid]) ? screen_eig_start(tid, k) : 0.0;
    __syncthreads();
    double lam = 0.0, rel = 0.0;
    int it = 1;
    for (;; ++it) {
      for (int p = 0; p < k; ++p) screen_eig_deflate(s_v, s_u[p], lane);
      const double vv = screen_eig_dot(s_v, s_v, lane);
      const double inv = vv > 0.0 ? 1.0 / sqrt(vv) : 0.0;
      __syncthreads();
      if (tid < SCREEN_ALIGNED_MAX_BINS) s_v[tid] *= inv;
      __syncthreads();
      double acc = 0.0;
      if (mine)
        for (int j = q; j < n; j += 4) {
          const double a = (s_ok[j] && abs(row - j) >= d_lo) ? (double)screen_eig_s(s_tri, row, j, n) - mu : 0.0;
          acc = fma(a, s_v[j], acc);
        }
      acc += __shfl_xor(acc, 1, 64);
      acc += __shfl_xor(acc, 2, 64);
      if (q == 0) s_w[row] = acc;
      __syncthreads();
      for (int p = 0; p < k; ++p) screen_eig_deflate(s_w, s_u[p], lane);
      lam = screen_eig_dot(s_v, s_w, lane);
      double r2 = 0.0;
      for (int j = lane; j < SCREEN_ALIGNED_MAX_BINS; j += 64) {
        const double t = fma(-lam, s_v[j], s_w[j]);
        r2 = fma(t, t, r2);
      }
      for (int o = 32; o > 0; o >>= 1) r2 += __shfl_xor(r2, o, 64);
      const double rn = sqrt(r2), al = fabs(lam);
      rel = rn == 0.0 ? 0.0 : (al > 0.0 ? rn / al : (double)__int_as_float(0x7f800000));
      if (rel <= tol || it >= max_iter) break;                     // (uniform: every wave holds the same bits)
      __syncthreads();                                             // every wave has read v
      if (tid < SCREEN_ALIGNED_MAX_BINS) s_v[tid] = s_w[tid];
      __syncthreads();
    }
    // the sign: the Pearson correlation with the phase track over the valid bins whose phase is finite, two passes (the means, then the centred sums)
    const double sc = sqrt(fabs(lam));
    double sgn = 0.0;
    if (phase != nullptr) {
      const float* ph = phase + (long)b * n;
      double sp = 0.0, sv = 0.0;
      int c = 0;
      for (int j = lane; j < n; j += 64) {
        const float p = ph[j];
        if (s_ok[j] && p - p == 0.f) {
          sp += (double)p;
          sv += s_v[j];
          ++c;
        }
      }
      for (int o = 32; o > 0; o >>= 1) {
        sp += __shfl_xor(sp, o, 64);
        sv += __shfl_xor(sv, o, 64);
        c += __shfl_xor(c, o, 64);
      }
      if (c >= 2) {
        const double mp = sp / (double)c, mv = sv / (double)c;
        double X = 0.0, Y = 0.0, C = 0.0;
        for (int j = lane; j < n; j += 64) {
          const float p = ph[j];
          if (s_ok[j] && p - p == 0.f) {
            const double ex = s_v[j] - mv, ey = (double)p - mp;
            X = fma(ex, ex, X);
            Y = fma(ey, ey, Y);
            C = fma(ex, ey, C);
          }
        }
        for (int o = 32; o > 0; o >>= 1) {
          X += __shfl_xor(X, o, 64);
          Y += __shfl_xor(Y, o, 64);
          C += __shfl_xor(C, o, 64);
        }
        if (X > 0.0 && Y > 0.0 && C != 0.0 && C == C) sgn = C < 0.0 ? -1.0 : 1.0;
      }
    }
    if (sgn == 0.0) {                                              // the fallback: the component of largest |E_k| (as fp32) positive, the lowest index of equals
      float best = -1.f, bv = 0.f;
      int bi = SCREEN_ALIGNED_MAX_BINS;
      for (int j = lane; j < n; j += 64) {
        const float e = (float)(s_v[j] * sc);
        if (s_ok[j] && fabsf(e) > best) {
          best = fabsf(e);
          bv = e;
          bi = j;
        }
      }
      for (int o = 32; o > 0; o >>= 1) {
        const float ob = __shfl_xor(best, o, 64), ov = __shfl_xor(bv, o, 64);
        const int oi = __shfl_xor(bi, o, 64);
        if (ob > best || (ob == best && oi < bi)) {
          best = ob;
          bv = ov;
          bi = oi;
        }
      }
      sgn = bv < 0.f ? -1.0 : 1.0;
    }
    if (tid < n) E[((long)b * K + k) * n + tid] = s_ok[tid] ? (float)(sgn * s_v[tid] * sc) : qnan;
    if (tid == 0) {
      eigenvalue[(long)b * K + k] = lam;
      residual[(long)b * K + k] = rel;
      iterations[(long)b * K + k] = it;
    }
    if (tid < SCREEN_ALIGNED_MAX_BINS) s_u[k][tid] = s_v[tid];
    __syncthreads();
  }
}

// ---- GC content per bin (orca_screen_gc_tracks): the phase track of the compartments, from the codes the screen already holds ----------------------------
// out[w][i] = #{C, G} / #{A, C, G, T} over the bases [off_w + i bs_w, off_w + (i + 1) bs_w) of codes [L] (0..3 = A, C, G, T; anything else counts as N),
// NaN where the bin holds no A/C/G/T.  One workgroup per (bin, window); up to SCREEN_GC_WINDOWS windows per launch, their offsets and bin sizes by value.
// The bases between the first and the last 16-byte boundary of the bin are read 16 at a time.  Integer counts (any order gives the same), one fp64 division,
// rounded to fp32 once.  The host checks that every window lies in [0, L); the kernel clips all the same.
#define SCREEN_GC_WINDOWS 16
struct screen_gc_windows {
  long long off[SCREEN_GC_WINDOWS], bs[SCREEN_GC_WINDOWS];
};

static __device__ __forceinline__ void screen_gc_count(unsigned c, unsigned& cg, unsigned& all) {
  all += c < 4u ? 1u : 0u;
  cg += (c == 1u || c == 2u) ? 1u : 0u;
}

static __global__ void __launch_bounds__(256) screen_gc_tracks_kernel(const unsigned char* __restrict__ codes, long L, screen_gc_windows win, int W, int n,
                                                                      float* __restrict__ out) {
  __shared__ unsigned long long s_cg[4], s_all[4];
  const int i = blockIdx.x, w = blockIdx.y, tid = threadIdx.x;
  if (w >= W || w >= SCREEN_GC_WINDOWS || i >= n) return;          // (uniform)
  long long off = 0, bs = 0;
  for (int t = 0; t < SCREEN_GC_WINDOWS; ++t)                      // (a select chain: the table stays in registers)
    if (t == w) {
      off = win.off[t];
      bs = win.bs[t];
    }
  long lo = (long)(off + (long long)i * bs), hi = (long)(off + (long long)(i + 1) * bs);
  lo = lo < 0 ? 0 : lo;
  hi = hi > L ? L : hi;
  unsigned long long cg = 0, all = 0;
  if (lo < hi) {
    long a0 = lo + (long)((16 - (reinterpret_cast<unsigned long long>(codes + lo) & 15u)) & 15u);
    a0 = a0 > hi ? hi : a0;
    const long a1 = a0 + ((hi - a0) & ~15L);
    unsigned c1 = 0, c2 = 0;
    for (long p = lo + tid; p < a0; p += 256) screen_gc_count(codes[p], c1, c2);
    for (long p = a1 + tid; p < hi; p += 256) screen_gc_count(codes[p], c1, c2);
    cg += c1;
    all += c2;
    for (long p = a0 + 16L * tid; p < a1; p += 16L * 256) {
      const uint4 v = *reinterpret_cast<const uint4*>(codes + p);
      const unsigned word[4] = {v.x, v.y, v.z, v.w};
      c1 = c2 = 0;
#pragma unroll
      for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int s = 0; s < 32; s += 8) screen_gc_count((word[t] >> s) & 255u, c1, c2);
      cg += c1;
      all += c2;
    }
  }
  for (int o = 32; o > 0; o >>= 1) {
    cg += __shfl_xor(cg, o, 64);
    all += __shfl_xor(all, o, 64);
  }
  if ((tid & 63) == 0) {
    s_cg[tid >> 6] = cg;
    s_all[tid >> 6] = all;
  }
  __syncthreads();
  if (tid != 0) return;
  cg = s_cg[0] + s_cg[1] + s_cg[2] + s_cg[3];
  all = s_all[0] + s_all[1] + s_all[2] + s_all[3];
  out[(long)w * n + i] = all > 0 ? (float)((double)cg / (double)all) : __int_as_float(0x7fc00000);
}

// ---- both strands (screen.screen_1m(..., strands="both")): the '-' strand's map is merged into the '+' strand's as genomepredict merges them ------------
// out[b][i][j] = 0.5 fwd[b][i][j] + 0.5 rev[b][n-1-i][n-1-j] (the expression of strand_merge_kernel: the same bits), and with the two strands' reference maps
// gap[b] = mean_ij |(fwd - ref_fwd)[i][j] - (rev - ref_rev)[n-1-i][n-1-j]| - how far the strands disagree about the item's effect.  One workgroup per map, one
// wave per row at a time, 128 columns per step: lane l holds columns j0 + 2l and j0 + 2l + 1.  The mirrored row n-1-i of `rev` is read FORWARDS - lane m reads
// columns c, c + 1 with c = n - j0 - 128 + 2m - and lane l takes the pair of lane 63 - l, swapped.  `vec` (wave-uniform; n even, every base and batch stride
// 8-byte aligned - rows of 250 floats are no more than that): the pairs are float2 accesses, else two scalar ones; the assignment of columns to lanes, and
// with it the order of the sum, is the same.  Differences and sums in fp64: per lane along its columns, shuffles across the wave, the waves' sums serially -
// fixed by n alone, so a map's gap does not depend on B or on its place in the batch.  A NaN propagates into out and, through the sums, into gap.
// `out` may be `fwd` (an element is read and written by the same thread); `rev` may not overlap `out`.  gap == NULL: no references are read.
static __device__ __forceinline__ float2 screen_load2(const float* row, int c, int n, bool vec) {
  if (vec) return (c >= 0 && c + 1 < n) ? *reinterpret_cast<const float2*>(row + c) : make_float2(0.f, 0.f);
  return make_float2((c >= 0 && c < n) ? row[c] : 0.f, (c + 1 >= 0 && c + 1 < n) ? row[c + 1] : 0.f);
}

static __global__ void __launch_bounds__(512) screen_merge_strands_kernel(const float* fwd, long fwd_bs, const float* __restrict__ rev, long rev_bs,
                                                                          const float* __restrict__ ref_fwd, const float* __restrict__ ref_rev, int n,
                                                                          float* out, long out_bs, float* __restrict__ gap, int vec) {
  __shared__ double s_sum[8];
  const int b = blockIdx.x, lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const float* f = fwd + (long)b * fwd_bs;
  const float* r = rev + (long)b * rev_bs;
  float* o = out + (long)b * out_bs;
  const bool v2 = vec != 0;
  double wsum = 0.0;
  for (int i = wv; i < n; i += 8) {
    const long at = (long)i * n, mat = (long)(n - 1 - i) * n;
    double rs = 0.0;
    for (int j0 = 0; j0 < n; j0 += 128) {
      const int j = j0 + 2 * lane, c = n - j0 - 128 + 2 * lane;
      const float2 mine = screen_load2(r + mat, c, n, v2);        // columns c, c + 1 of the mirrored row: output columns n-1-c, n-2-c
      double e0 = 0.0, e1 = 0.0;
      if (gap) {
        const float2 rr = screen_load2(ref_rev + mat, c, n, v2);
        e0 = (double)mine.x - (double)rr.x;
        e1 = (double)mine.y - (double)rr.y;
      }
      const float m0 = __shfl(mine.y, 63 - lane, 64), m1 = __shfl(mine.x, 63 - lane, 64);      // rev[n-1-i][n-1-j], rev[n-1-i][n-2-j]
      const double g0 = __shfl(e1, 63 - lane, 64), g1 = __shfl(e0, 63 - lane, 64);
      const float2 a = screen_load2(f + at, j, n, v2);
      const float2 res = make_float2(a.x * 0.5f + m0 * 0.5f, a.y * 0.5f + m1 * 0.5f);
      if (gap) {
        const float2 rf = screen_load2(ref_fwd + at, j, n, v2);
        if (j < n) rs += fabs(((double)a.x - (double)rf.x) - g0);
        if (j + 1 < n) rs += fabs(((double)a.y - (double)rf.y) - g1);
      }
      if (v2) {
        if (j + 1 < n) *reinterpret_cast<float2*>(o + at + j) = res;
      } else {
        if (j < n) o[at + j] = res.x;
        if (j + 1 < n) o[at + j + 1] = res.y;
      }
    }
    for (int k = 32; k > 0; k >>= 1) rs += __shfl_xor(rs, k, 64);
    wsum += rs;
  }
  if (!gap) return;
  if (lane == 0) s_sum[wv] = wsum;
  __syncthreads();
  if (threadIdx.x == 0) {
    double t = 0.0;
    for (int k = 0; k < 8; ++k) t += s_sum[k];
    gap[b] = (float)(t / ((double)n * (double)n));
  }
}

// ---- non-additivity (screen.epistasis_1m): a set's map against the sum of its members' effects ----------------------------------------------------------
// Set b has members members[member_off[b] .. member_off[b + 1]) (int64 offsets, int32 indices into the bank; include/orca_hip.h:
// orca_screen_epistasis_scores), S = alt[b] its own map, A_m = bank[members[m]] the map of member m applied alone.  Per pixel, every operand converted to
// fp64 first and no multiplication anywhere: t = sum_m (A_m - ref), added sequentially for m ascending from 0.0 - the additive expectation - and
// r = (S - ref) - t, the residual.  For a one-member set whose map holds its bank entry's bits r is exactly +0.0.  The member list is read from global
// memory (no cap on its length) and is the same for a whole workgroup.  The host entry point checks the table; here the range is clipped to the table
// all the same, and a member outside the bank reads as NaN.
struct screen_epi { double r, t; };

static __device__ __forceinline__ screen_epi screen_epistasis_at(const float* __restrict__ a, const float* __restrict__ bank, long bank_bs, int U,
                                                                 const float* __restrict__ ref, const int* __restrict__ members, long m0, long m1, long at) {
  const double rf = (double)ref[at];
  double t = 0.0;
  for (long m = m0; m < m1; ++m) {
    const int u = members[m];
    t += (u >= 0 && u < U) ? (double)bank[(long)u * bank_bs + at] - rf : (double)__int_as_float(0x7fc00000);
  }
  screen_epi e;
  e.r = ((double)a[at] - rf) - t;
  e.t = t;
  return e;
}

// set b's member range, clipped to the P entries of the table
static __device__ __forceinline__ void screen_member_range(const long long* __restrict__ member_off, long P, int b, long& m0, long& m1) {
  m0 = (long)member_off[b];
  m1 = (long)member_off[b + 1];
  m0 = m0 < 0 ? 0 : m0;
  m1 = m1 > P ? P : m1;
}

// screen_scores_kernel on the residual: profile[b][i] = mean_j |r[i][j]|, mean[b] = mean_ij |r|, amax[b] = max_ij |r| (the largest fp64 |r|, rounded
// once), add_mean[b] = mean_ij |t|.  One workgroup per set, one wave per row at a time: fp64 per lane along its columns, shuffles across the wave, the
// eight waves' sums serially - an order fixed by n alone, no atomics, so a set's bits depend neither on B nor on its place in the batch.  A NaN in a
// map propagates through the sums it enters (a NaN r into profile, mean and amax; a NaN t also into add_mean).
static __global__ void __launch_bounds__(512) screen_epistasis_scores_kernel(const float* __restrict__ alt, long map_bs, const float* __restrict__ bank,
                                                                             long bank_bs, int U, const float* __restrict__ ref, int n,
                                                                             const long long* __restrict__ member_off, const int* __restrict__ members,
                                                                             long P, float* __restrict__ profile, float* __restrict__ mean,
                                                                             float* __restrict__ amax, float* __restrict__ add_mean) {
  __shared__ double s_sum[8], s_add[8], s_max[8];
  __shared__ int s_nan[8];
  const int b = blockIdx.x, lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const float* a = alt + (long)b * map_bs;
  long m0, m1;
  screen_member_range(member_off, P, b, m0, m1);
  double wsum = 0.0, wadd = 0.0, wmax = 0.0;
  bool wnan = false;
  for (int i = wv; i < n; i += 8) {
    double rs = 0.0, ts = 0.0;
    for (int j = lane; j < n; j += 64) {
      const screen_epi e = screen_epistasis_at(a, bank, bank_bs, U, ref, members, m0, m1, (long)i * n + j);
      const double d = fabs(e.r);
      rs += d;
      ts += fabs(e.t);
      wnan |= d != d;
      wmax = fmax(wmax, d);
    }
    for (int o = 32; o > 0; o >>= 1) {
      rs += __shfl_xor(rs, o, 64);
      ts += __shfl_xor(ts, o, 64);
    }
    if (lane == 0) profile[(long)b * n + i] = (float)(rs / (double)n);
    wsum += rs;
    wadd += ts;
  }
  for (int o = 32; o > 0; o >>= 1) {
    wmax = fmax(wmax, __shfl_xor(wmax, o, 64));
    wnan |= __shfl_xor((int)wnan, o, 64) != 0;
  }
  if (lane == 0) {
    s_sum[wv] = wsum;
    s_add[wv] = wadd;
    s_max[wv] = wmax;
    s_nan[wv] = wnan ? 1 : 0;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    double t = 0.0, ta = 0.0, m = 0.0;
    bool nan = false;
    for (int k = 0; k < 8; ++k) {
      t += s_sum[k];
      ta += s_add[k];
      nan |= s_nan[k] != 0;
      m = fmax(m, s_max[k]);
    }
    const double nn = (double)n * (double)n;
    const float qnan = __int_as_float(0x7fc00000);
    mean[b] = (float)(t / nn);
    amax[b] = nan ? qnan : (float)m;
    add_mean[b] = (float)(ta / nn);
  }
}

// screen_region_scores_kernel on the residual: signed[b][k] = mean of r, absm[b][k] = mean of |r| over rectangle k (int32 (i0, i1, j0, j1), half open,
// inside [0, n) - the host entry point checks it; clipped here all the same).  One workgroup per (set, rectangle); fp64 sums in a fixed order.
static __global__ void __launch_bounds__(256) screen_epistasis_region_scores_kernel(const float* __restrict__ alt, long map_bs, const float* __restrict__ bank,
                                                                                    long bank_bs, int U, const float* __restrict__ ref, int n,
                                                                                    const long long* __restrict__ member_off,
                                                                                    const int* __restrict__ members, long P, const int* __restrict__ rects,
                                                                                    int K, float* __restrict__ signed_out, float* __restrict__ abs_out) {
  __shared__ double s_sum[4], s_abs[4];
  const int b = blockIdx.x, k = blockIdx.y, lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  int i0 = rects[4 * k], i1 = rects[4 * k + 1], j0 = rects[4 * k + 2], j1 = rects[4 * k + 3];
  i0 = i0 < 0 ? 0 : i0; j0 = j0 < 0 ? 0 : j0;
  i1 = i1 > n ? n : i1; j1 = j1 > n ? n : j1;
  const int h = i1 > i0 ? i1 - i0 : 0, w = j1 > j0 ? j1 - j0 : 0;
  const float* a = alt + (long)b * map_bs;
  long m0, m1;
  screen_member_range(member_off, P, b, m0, m1);
  double sum = 0.0, asum = 0.0;
  for (int e = threadIdx.x; e < h * w; e += 256) {
    const screen_epi d = screen_epistasis_at(a, bank, bank_bs, U, ref, members, m0, m1, (long)(i0 + e / w) * n + (j0 + e % w));
    sum += d.r;
    asum += fabs(d.r);
  }
  for (int o = 32; o > 0; o >>= 1) {
    sum += __shfl_xor(sum, o, 64);
    asum += __shfl_xor(asum, o, 64);
  }
  if (lane == 0) { s_sum[wv] = sum; s_abs[wv] = asum; }
  __syncthreads();
  if (threadIdx.x == 0) {
    const double cnt = (double)h * (double)w;
    const double t = (s_sum[0] + s_sum[1]) + (s_sum[2] + s_sum[3]), ta = (s_abs[0] + s_abs[1]) + (s_abs[2] + s_abs[3]);
    signed_out[(long)b * K + k] = (float)(t / cnt);
    abs_out[(long)b * K + k] = (float)(ta / cnt);
  }
}
