// screen.h - the small kernels of the 1 Mb in-silico mutagenesis screen (orca_amd/screen.py): edited snippets straight from the window's
// codes, the per-edit stage-5 row images, the [B][n][128] -> [B][128][n] hand-over of batched stages 5-7, and the map scores (bin with bin, and on aligned bins).
// All of them are HBM-bound and tiny next to the Decoder_1m they feed; each is ONE launch for a whole batch of edits.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// ---- edit table (int64 per snippet, SCREEN_EDIT_FIELDS fields; include/orca_hip.h: orca_screen_edit_codes) ---------------------------------------------
//   [0] out_off  first output base of this snippet in the packed output
//   [1] b0       first window base of the snippet
//   [2] nb       bases in the snippet
//   [3] kind     0 substitution (payload), 1 N-mask, 2 in-place reverse complement
//   [4] pos      first window base of the edited span
//   [5] len      bases in the edited span
//   [6] pay_off  first payload code of a substitution
//   [7] (unused)
// Snippets are packed back to back in table order (out_off ascending, no gaps).
#define SCREEN_EDIT_FIELDS 8

// one thread per output base: binary search of its snippet, then the window base with the edit applied.  Every read is bounds-checked
// against L / npay (an out-of-range index reads as N), so a malformed table cannot make the kernel leave its buffers.
static __global__ void screen_edit_codes_kernel(const unsigned char* __restrict__ win, long L, const long long* __restrict__ tab, int ns,
                                                const unsigned char* __restrict__ pay, long npay, unsigned char* __restrict__ out, long total) {
  const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= total) return;
  int lo = 0, hi = ns - 1;
  while (lo < hi) {                                  // last snippet with out_off <= t
    const int mid = (lo + hi + 1) >> 1;
    if (tab[(long)mid * SCREEN_EDIT_FIELDS] <= t) lo = mid; else hi = mid - 1;
  }
  const long long* e = tab + (long)lo * SCREEN_EDIT_FIELDS;
  const long w = (long)e[1] + (t - (long)e[0]);
  unsigned c = (w >= 0 && w < L) ? win[w] : 4u;
  const long pos = (long)e[4], len = (long)e[5];
  if (w >= pos && w < pos + len) {
    const long k = w - pos;
    if (e[3] == 0) {
      const long p = (long)e[6] + k;
      c = (p >= 0 && p < npay) ? pay[p] : 4u;
    } else if (e[3] == 1) {
      c = 4u;
    } else {
      const long src = pos + len - 1 - k;
      const unsigned s = (src >= 0 && src < L) ? win[src] : 4u;
      c = s < 4u ? 3u - s : 4u;                        // A<->T, C<->G; N stays N
    }
  }
  out[t] = (unsigned char)(c > 4u ? 4u : c);
}

// splice table (int64 per edit, 3 fields): [row_lo, row_cnt, src_row] - rows [row_lo, row_lo + row_cnt) of edit b's image come from rows
// [src_row, ..) of `fresh`, every other row from `ref`.  One thread per 16-byte unit of the output [B][n5][128].
static __global__ void screen_splice_rows_kernel(const f32x4* __restrict__ ref, long n5, const f32x4* __restrict__ fresh, long nfresh,
                                                 const long long* __restrict__ tab, int B, f32x4* __restrict__ out) {
  const long u = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const long per = n5 * 32;
  if (u >= (long)B * per) return;
  const int b = (int)(u / per);
  const long r = (u - (long)b * per) >> 5, q = u & 31;
  const long r0 = (long)tab[3 * b], cnt = (long)tab[3 * b + 1], s0 = (long)tab[3 * b + 2];
  const long s = s0 + (r - r0);
  out[u] = (r >= r0 && r < r0 + cnt && s >= 0 && s < nfresh) ? fresh[s * 32 + q] : ref[r * 32 + q];
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

// ---- compound edits (screen.EditSet): several disjoint spans applied to one snippet, several (snippet, row range) segments per image -------------------
// snippet table (int64 per snippet, SCREEN_EDIT_FIELDS fields; include/orca_hip.h: orca_screen_edit_codes_multi)
//   [0] out_off  [1] b0  [2] nb  as above     [3] span_lo  first span of this snippet in the span table     [4] span_cnt  spans of this snippet
// span table (int64 per span, SCREEN_SPAN_FIELDS fields): [0] kind  [1] pos  [2] len  [3] pay_off - a snippet's spans are sorted by pos and
// pairwise disjoint, so a binary search finds the one span that can hold a base.  An inversion reads its source from the unedited window.
#define SCREEN_SPAN_FIELDS 4

// one thread per output base: binary search of its snippet, binary search of the snippet's spans, then the window base with that span's
// edit applied.  The span range is clipped to the table and every read is bounds-checked against L / npay (an out-of-range index reads as N).
static __global__ void screen_edit_codes_multi_kernel(const unsigned char* __restrict__ win, long L, const long long* __restrict__ tab, int ns,
                                                      const long long* __restrict__ spans, long nspans, const unsigned char* __restrict__ pay, long npay,
                                                      unsigned char* __restrict__ out, long total) {
  const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= total) return;
  int lo = 0, hi = ns - 1;
  while (lo < hi) {                                  // last snippet with out_off <= t
    const int mid = (lo + hi + 1) >> 1;
    if (tab[(long)mid * SCREEN_EDIT_FIELDS] <= t) lo = mid; else hi = mid - 1;
  }
  const long long* e = tab + (long)lo * SCREEN_EDIT_FIELDS;
  const long w = (long)e[1] + (t - (long)e[0]);
  unsigned c = (w >= 0 && w < L) ? win[w] : 4u;
  long s0 = (long)e[3], s1 = (long)e[3] + (long)e[4];
  s0 = s0 < 0 ? 0 : s0;
  s1 = s1 > nspans ? nspans : s1;
  if (s0 < s1) {
    long a = s0, b = s1 - 1;
    while (a < b) {                                  // last span with pos <= w (the first one when none is)
      const long mid = (a + b + 1) >> 1;
      if ((long)spans[mid * SCREEN_SPAN_FIELDS + 1] <= w) a = mid; else b = mid - 1;
    }
    const long long* sp = spans + a * SCREEN_SPAN_FIELDS;
    const long pos = (long)sp[1], len = (long)sp[2];
    if (w >= pos && w - pos < len) {
      const long k = w - pos;
      if (sp[0] == 0) {
        const long p = (long)sp[3] + k;
        c = (p >= 0 && p < npay) ? pay[p] : 4u;
      } else if (sp[0] == 1) {
        c = 4u;
      } else {
        const long src = pos + len - 1 - k;
        const unsigned s = (src >= 0 && src < L) ? win[src] : 4u;
        c = s < 4u ? 3u - s : 4u;                        // A<->T, C<->G; N stays N
      }
    }
  }
  out[t] = (unsigned char)(c > 4u ? 4u : c);
}

// segment table (int64 per segment, 3 fields): [row_lo, row_cnt, src_row] as the splice table above; image b owns segments
// [seg_off[b], seg_off[b + 1]), sorted by row_lo and disjoint.  One thread per 16-byte unit of the output [B][n5][128]: binary search of the
// image's segments for the last one with row_lo <= r.  The segment range is clipped to the table, the source row to `fresh`.
static __global__ void screen_splice_rows_multi_kernel(const f32x4* __restrict__ ref, long n5, const f32x4* __restrict__ fresh, long nfresh,
                                                       const long long* __restrict__ seg, long nseg, const long long* __restrict__ seg_off, int B,
                                                       f32x4* __restrict__ out) {
  const long u = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const long per = n5 * 32;
  if (u >= (long)B * per) return;
  const int b = (int)(u / per);
  const long r = (u - (long)b * per) >> 5, q = u & 31;
  long s0 = (long)seg_off[b], s1 = (long)seg_off[b + 1];
  s0 = s0 < 0 ? 0 : s0;
  s1 = s1 > nseg ? nseg : s1;
  f32x4 v = ref[r * 32 + q];
  if (s0 < s1) {
    long a = s0, z = s1 - 1;
    while (a < z) {
      const long mid = (a + z + 1) >> 1;
      if ((long)seg[3 * mid] <= r) a = mid; else z = mid - 1;
    }
    const long r0 = (long)seg[3 * a], cnt = (long)seg[3 * a + 1], s = (long)seg[3 * a + 2] + (r - r0);
    if (r >= r0 && r - r0 < cnt && s >= 0 && s < nfresh) v = fresh[s * 32 + q];
  }
  out[u] = v;
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

// ---- insertions and deletions (screen.Edit "del" / "ins"): the edited bases from a piece list, the row images from several sources ---------------------
// The alt window of an item is a list of PIECES in alt coordinates; the context is the window followed by its right flank.
// snippet table (int64 per snippet, SCREEN_EDIT_FIELDS fields; include/orca_hip.h: orca_screen_assemble_codes)
//   [0] out_off  [1] a0  first ALT base of the snippet  [2] nb  [3] piece_lo  first piece of this snippet in the piece table  [4] piece_cnt
// piece table (int64 per piece, SCREEN_PIECE_FIELDS fields): [0] dst  first alt base  [1] kind  [2] src  [3] len - a snippet's pieces are sorted by
// dst and pairwise disjoint.  kind 0: context bases [src, src + len) forward; 1: their reverse complement (alt base dst + t is the complement of
// context[src + len - 1 - t], N stays N); 2: payload codes [src, src + len); 3: N.
#define SCREEN_PIECE_FIELDS 4

// one thread per output base: binary search of its snippet, binary search of the snippet's pieces.  The piece range is clipped to the table; a base no
// piece covers and a read outside the context / the payload give N.
static __global__ void screen_assemble_codes_kernel(const unsigned char* __restrict__ cx, long C, const long long* __restrict__ tab, int ns,
                                                    const long long* __restrict__ pieces, long npieces, const unsigned char* __restrict__ pay, long npay,
                                                    unsigned char* __restrict__ out, long total) {
  const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= total) return;
  int lo = 0, hi = ns - 1;
  while (lo < hi) {                                  // last snippet with out_off <= t
    const int mid = (lo + hi + 1) >> 1;
    if (tab[(long)mid * SCREEN_EDIT_FIELDS] <= t) lo = mid; else hi = mid - 1;
  }
  const long long* e = tab + (long)lo * SCREEN_EDIT_FIELDS;
  const long w = (long)e[1] + (t - (long)e[0]);
  unsigned c = 4u;
  long s0 = (long)e[3], s1 = (long)e[3] + (long)e[4];
  s0 = s0 < 0 ? 0 : s0;
  s1 = s1 > npieces ? npieces : s1;
  if (s0 < s1) {
    long a = s0, b = s1 - 1;
    while (a < b) {                                  // last piece with dst <= w (the first one when none is)
      const long mid = (a + b + 1) >> 1;
      if ((long)pieces[mid * SCREEN_PIECE_FIELDS] <= w) a = mid; else b = mid - 1;
    }
    const long long* pc = pieces + a * SCREEN_PIECE_FIELDS;
    const long dst = (long)pc[0], src = (long)pc[2], len = (long)pc[3];
    if (w >= dst && w - dst < len) {
      const long k = w - dst;
      if (pc[1] == 0) {
        const long p = src + k;
        c = (p >= 0 && p < C) ? cx[p] : 4u;
      } else if (pc[1] == 1) {
        const long p = src + len - 1 - k;
        const unsigned s = (p >= 0 && p < C) ? cx[p] : 4u;
        c = s < 4u ? 3u - s : 4u;                        // A<->T, C<->G; N stays N
      } else if (pc[1] == 2) {
        const long p = src + k;
        c = (p >= 0 && p < npay) ? pay[p] : 4u;
      }
    }
  }
  out[t] = (unsigned char)(c > 4u ? 4u : c);
}

// segment table (int64 per segment, SCREEN_GATHER_FIELDS fields): [row_lo, row_cnt, source, src_row]; image b owns segments [seg_off[b], seg_off[b + 1]),
// sorted by row_lo and disjoint.  source -1: rows [src_row, ..) of `fresh`; -2: rows [src_row, ..) of `ref`; p >= 0: row row_lo + t is the MaxPool1d(5) of
// rows src_row + 5 t .. + 4 of phase entry p (`entries[p]`, `entry_rows[p]` rows of 128 floats).  A row in no segment is `ref` at its own index.
// One thread per 16-byte unit of the output [B][n5][128].  The segment range is clipped to the table, every source row to its buffer (a row that
// would leave it is `ref` at its own index).  The pooling expression is rows_pool5_into_kernel's (p16_planes.h): the same bits.
#define SCREEN_GATHER_FIELDS 4

static __global__ void screen_gather_rows_kernel(const f32x4* __restrict__ ref, long n5, const f32x4* __restrict__ fresh, long nfresh,
                                                 const f32x4* const* __restrict__ entries, const long long* __restrict__ entry_rows, int P,
                                                 const long long* __restrict__ seg, long nseg, const long long* __restrict__ seg_off, int B,
                                                 f32x4* __restrict__ out) {
  const long u = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const long per = n5 * 32;
  if (u >= (long)B * per) return;
  const int b = (int)(u / per);
  const long r = (u - (long)b * per) >> 5, q = u & 31;
  long s0 = (long)seg_off[b], s1 = (long)seg_off[b + 1];
  s0 = s0 < 0 ? 0 : s0;
  s1 = s1 > nseg ? nseg : s1;
  const f32x4* from = ref + r * 32 + q;
  bool pool = false;
  if (s0 < s1) {
    long a = s0, z = s1 - 1;
    while (a < z) {
      const long mid = (a + z + 1) >> 1;
      if ((long)seg[SCREEN_GATHER_FIELDS * mid] <= r) a = mid; else z = mid - 1;
    }
    const long long* g = seg + SCREEN_GATHER_FIELDS * a;
    const long r0 = (long)g[0], cnt = (long)g[1], source = (long)g[2], k = r - r0;
    if (r >= r0 && k < cnt) {
      if (source == -1) {
        const long s = (long)g[3] + k;
        if (s >= 0 && s < nfresh) from = fresh + s * 32 + q;
      } else if (source == -2) {
        const long s = (long)g[3] + k;
        if (s >= 0 && s < n5) from = ref + s * 32 + q;
      } else if (source >= 0 && source < P) {
        const long s = (long)g[3] + 5 * k;
        if (s >= 0 && s + 5 <= (long)entry_rows[source]) {
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
