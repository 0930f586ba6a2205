// orca_screen.hip - entry points of the 1 Mb mutagenesis screen (orca_amd/screen.py; kernels in screen.h) and of the chromosome scan (orca_amd/scan.py;
// kernels in scan.h and scan_loops.h): table validation on the host, one launch each
// Part of liborca_hip.so (include/orca_hip.h is the ABI; orca_internal.h what the units share).
#include "orca_internal.h"

#include "scan.h"
#include "screen.h"
#include "scan_loops.h"

static inline const f32x4* f4(const float* p) { return reinterpret_cast<const f32x4*>(p); }
static inline const long long* i64(const int64_t* p) { return reinterpret_cast<const long long*>(p); }
static inline dim3 grid256(long threads) { return dim3((unsigned)((threads + 255) / 256)); }

// the end of every entry point: one launch on the context's stream
template <class... P, class... A>
static int launch(orca_ctx* ctx, const char* name, void (*kernel)(P...), dim3 grid, int threads, A... args) {
  HIPCHECK(hipSetDevice(ctx->device));
  hipLaunchKernelGGL(kernel, grid, dim3(threads), 0, ctx->stream, args...);
  LAUNCHCHECK(name);
  return ORCA_OK;
}

// ---- the checks of the small tables.  A table comes twice, on the device for the kernel and on the host for the checks made here before any launch (the
// kernels clip every table-derived index all the same, so the two copies differing cannot make them leave their buffers).  `what` names the entry point
// in the shared messages; wording that differs between the formats is in the entry point's own `snip` / `row` / `seg` check.

// a packed snippet table over a sub-table of 4-field `rows` ("spans" / "pieces"; `key` names column K, LEN is the length's column): out_off ascending
// without gaps, snip(k, e), the sub-table range inside its table, then per row row(s, r) and sorted / disjoint against the row before
template <class Snip, class Row>
static int walk_snippets(const char* what, const char* rows, const char* key, int K, int LEN, const int64_t* table_host, int n_snippets, const int64_t* sub_host,
                         int64_t n_sub, int64_t total, Snip snip, Row row) {
  int64_t off = 0;
  for (int k = 0; k < n_snippets; ++k) {
    const int64_t* e = table_host + (size_t)k * SCREEN_EDIT_FIELDS;
    if (e[0] != off || e[2] <= 0)
      return fail(ORCA_EINVAL, "%s: snippet %d starts at output base %ld with %ld bases, expected %ld (out_off ascending, no gaps)", what, k, (long)e[0], (long)e[2], (long)off);
    ORCA_TRY(snip(k, e));
    if (e[3] < 0 || e[4] < 0 || e[4] > n_sub - e[3]) return fail(ORCA_EINVAL, "%s: snippet %d has %s [%ld, +%ld) of %ld", what, k, rows, (long)e[3], (long)e[4], (long)n_sub);
    for (int64_t s = e[3]; s < e[3] + e[4]; ++s) {
      const int64_t* r = sub_host + (size_t)s * 4;
      ORCA_TRY(row(s, r));
      if (s > e[3] && r[K] < r[K - 4] + r[LEN - 4])
        return fail(ORCA_EINVAL, "%s: %s %ld and %ld of snippet %d overlap or are not sorted by %s", what, rows, (long)s - 1, (long)s, k, key);
    }
    off += e[2];
  }
  return off == total ? ORCA_OK : fail(ORCA_EINVAL, "%s: the snippets hold %ld bases, out holds %ld", what, (long)off, (long)total);
}

// a segment table of FIELDS columns [row_lo, row_cnt, ..] with offsets: monotone from 0 to n_segments (every offset is inside the table before a segment
// is read), then per segment seg(s, g) and sorted / disjoint against the segment before
template <class Seg>
static int walk_segments(const char* what, int FIELDS, const int64_t* segments_host, int64_t n_segments, const int64_t* seg_off_host, int B, Seg seg) {
  if (seg_off_host[0] != 0 || seg_off_host[B] != n_segments)
    return fail(ORCA_EINVAL, "%s: segment offsets run from %ld to %ld, the table holds %ld segments", what, (long)seg_off_host[0], (long)seg_off_host[B], (long)n_segments);
  for (int b = 0; b < B; ++b)
    if (seg_off_host[b + 1] < seg_off_host[b]) return fail(ORCA_EINVAL, "%s: segment offsets decrease at image %d", what, b);
  for (int b = 0; b < B; ++b)
    for (int64_t s = seg_off_host[b]; s < seg_off_host[b + 1]; ++s) {
      const int64_t* g = segments_host + FIELDS * (size_t)s;
      ORCA_TRY(seg(s, g));
      if (s > seg_off_host[b] && g[0] < g[-FIELDS] + g[1 - FIELDS])
        return fail(ORCA_EINVAL, "%s: segments %ld and %ld of image %d overlap or are not sorted by row_lo", what, (long)s - 1, (long)s, b);
    }
  return ORCA_OK;
}

static int check_rects(const char* what, const int32_t* rects_host, int K, int n) {
  for (int k = 0; k < K; ++k) {
    const int32_t* r = rects_host + 4 * k;
    if (r[0] < 0 || r[0] >= r[1] || r[1] > n || r[2] < 0 || r[2] >= r[3] || r[3] > n)
      return fail(ORCA_EINVAL, "%s: rectangle %d = rows [%d, %d) x columns [%d, %d) outside [0, %d) or empty", what, k, r[0], r[1], r[2], r[3], n);
  }
  return ORCA_OK;
}

// the bin map of the aligned scores: B x n int32, -1 .. n - 1
static int check_bin_map(const char* what, const int32_t* bin_map_host, int B, int n) {
  for (int b = 0; b < B; ++b)
    for (int i = 0; i < n; ++i) {
      const int32_t m = bin_map_host[(size_t)b * n + i];
      if (m < -1 || m >= n) return fail(ORCA_EINVAL, "%s: map %d sends alt bin %d to reference bin %d, outside -1 .. %d", what, b, i, m, n - 1);
    }
  return ORCA_OK;
}

// ---- bare edits: one span per snippet, one segment per image; the tables are on the device only (the kernels clip) ------------------------------------------
extern "C" int orca_screen_edit_codes(orca_ctx* ctx, const uint8_t* window, int64_t L, const int64_t* table, int n_snippets, const uint8_t* payload,
                                      int64_t n_payload, uint8_t* out, int64_t total) {
  if (!ctx || !window || !table || !out || n_snippets <= 0) return fail(ORCA_EINVAL, "orca_screen_edit_codes: NULL / empty argument");
  if (n_payload > 0 && !payload) return fail(ORCA_EINVAL, "orca_screen_edit_codes: NULL payload");
  if (total <= 0) return ORCA_OK;
  return launch(ctx, "screen_edit_codes_kernel", screen_edit_codes_kernel, grid256(total), 256, window, (long)L, i64(table), n_snippets, payload, (long)n_payload, out,
                (long)total);
}

extern "C" int orca_screen_splice_rows(orca_ctx* ctx, const float* ref, int64_t n5, const float* fresh, int64_t n_fresh, const int64_t* table, int B, float* out) {
  if (!ctx || !ref || !table || !out || (n_fresh > 0 && !fresh)) return fail(ORCA_EINVAL, "orca_screen_splice_rows: NULL argument");
  if (B <= 0 || n5 <= 0) return ORCA_OK;
  if (!al16(ref) || !al16(out) || (fresh && !al16(fresh))) return fail(ORCA_EINVAL, "orca_screen_splice_rows: rows must be 16-byte aligned");
  return launch(ctx, "screen_splice_rows_kernel", screen_splice_rows_kernel, grid256((long)B * n5 * 32), 256, f4(ref), (long)n5, f4(fresh), (long)n_fresh, i64(table), B,
                reinterpret_cast<f32x4*>(out));
}

// ---- compound edits: spans per snippet, segments per image ---------------------------------------------------------------------------------------------------
extern "C" int orca_screen_edit_codes_multi(orca_ctx* ctx, const uint8_t* window, int64_t L, const int64_t* table, const int64_t* table_host, int n_snippets,
                                            const int64_t* spans, const int64_t* spans_host, int64_t n_spans, const uint8_t* payload, int64_t n_payload,
                                            uint8_t* out, int64_t total) {
  if (!ctx || !window || !table || !table_host || !out) return fail(ORCA_EINVAL, "orca_screen_edit_codes_multi: NULL argument");
  if (n_snippets <= 0 || n_spans < 0 || n_payload < 0 || total < 0 || L <= 0)
    return fail(ORCA_EINVAL, "orca_screen_edit_codes_multi: %d snippets, %ld spans, %ld payload codes, %ld output bases, window of %ld", n_snippets, (long)n_spans,
                (long)n_payload, (long)total, (long)L);
  if (n_spans > 0 && (!spans || !spans_host)) return fail(ORCA_EINVAL, "orca_screen_edit_codes_multi: NULL span table");
  if (n_payload > 0 && !payload) return fail(ORCA_EINVAL, "orca_screen_edit_codes_multi: NULL payload");
  ORCA_TRY(walk_snippets("orca_screen_edit_codes_multi", "spans", "pos", 1, 2, table_host, n_snippets, spans_host, n_spans, total,
    [&](int k, const int64_t* e) -> int {
      if (e[1] >= 0 && e[2] <= L - e[1]) return ORCA_OK;
      return fail(ORCA_EINVAL, "orca_screen_edit_codes_multi: snippet %d = window bases [%ld, +%ld) outside the window of %ld", k, (long)e[1], (long)e[2], (long)L);
    },
    [&](int64_t s, const int64_t* sp) -> int {
      if (sp[0] < 0 || sp[0] > 2 || sp[1] < 0 || sp[2] <= 0 || sp[2] > L - sp[1])
        return fail(ORCA_EINVAL, "orca_screen_edit_codes_multi: span %ld: kind %ld, bases [%ld, +%ld) of %ld", (long)s, (long)sp[0], (long)sp[1], (long)sp[2], (long)L);
      if (sp[0] != 0 || (sp[3] >= 0 && sp[2] <= n_payload - sp[3])) return ORCA_OK;
      return fail(ORCA_EINVAL, "orca_screen_edit_codes_multi: span %ld: payload [%ld, +%ld) of %ld", (long)s, (long)sp[3], (long)sp[2], (long)n_payload);
    }));
  return launch(ctx, "screen_edit_codes_multi_kernel", screen_edit_codes_multi_kernel, grid256(total), 256, window, (long)L, i64(table), n_snippets, i64(spans),
                (long)n_spans, payload, (long)n_payload, out, (long)total);
}

extern "C" int orca_screen_splice_rows_multi(orca_ctx* ctx, const float* ref, int64_t n5, const float* fresh, int64_t n_fresh, const int64_t* segments,
                                             const int64_t* segments_host, int64_t n_segments, const int64_t* seg_off, const int64_t* seg_off_host, int B,
                                             float* out) {
  if (!ctx || !ref || !seg_off || !seg_off_host || !out) return fail(ORCA_EINVAL, "orca_screen_splice_rows_multi: NULL argument");
  if (B < 0 || n5 < 0 || n_fresh < 0 || n_segments < 0)
    return fail(ORCA_EINVAL, "orca_screen_splice_rows_multi: %d images of %ld rows, %ld fresh rows, %ld segments", B, (long)n5, (long)n_fresh, (long)n_segments);
  if (n_fresh > 0 && !fresh) return fail(ORCA_EINVAL, "orca_screen_splice_rows_multi: NULL fresh rows");
  if (n_segments > 0 && (!segments || !segments_host)) return fail(ORCA_EINVAL, "orca_screen_splice_rows_multi: NULL segment table");
  ORCA_TRY(walk_segments("orca_screen_splice_rows_multi", 3, segments_host, n_segments, seg_off_host, B, [&](int64_t s, const int64_t* g) -> int {
    if (g[0] >= 0 && g[1] > 0 && g[1] <= n5 - g[0] && g[2] >= 0 && g[1] <= n_fresh - g[2]) return ORCA_OK;
    return fail(ORCA_EINVAL, "orca_screen_splice_rows_multi: segment %ld = rows [%ld, +%ld) of %ld from fresh row %ld of %ld", (long)s, (long)g[0], (long)g[1], (long)n5, (long)g[2], (long)n_fresh);
  }));
  if (B == 0 || n5 == 0) return ORCA_OK;
  if (!al16(ref) || !al16(out) || (fresh && !al16(fresh))) return fail(ORCA_EINVAL, "orca_screen_splice_rows_multi: rows must be 16-byte aligned");
  return launch(ctx, "screen_splice_rows_multi_kernel", screen_splice_rows_multi_kernel, grid256((long)B * n5 * 32), 256, f4(ref), (long)n5, f4(fresh), (long)n_fresh,
                i64(segments), (long)n_segments, i64(seg_off), B, reinterpret_cast<f32x4*>(out));
}

// ---- insertions and deletions: the edited bases of a batch from piece lists over the context (window + right flank), and the row images from the
// reference rows, the recomputed rows and the stage-4 phase entries
extern "C" int orca_screen_assemble_codes(orca_ctx* ctx, const uint8_t* context, int64_t C, const int64_t* table, const int64_t* table_host, int n_snippets,
                                          const int64_t* pieces, const int64_t* pieces_host, int64_t n_pieces, const uint8_t* payload, int64_t n_payload,
                                          uint8_t* out, int64_t total) {
  if (!ctx || !context || !table || !table_host || !out) return fail(ORCA_EINVAL, "orca_screen_assemble_codes: NULL argument");
  if (n_snippets <= 0 || n_pieces < 0 || n_payload < 0 || total < 0 || C <= 0)
    return fail(ORCA_EINVAL, "orca_screen_assemble_codes: %d snippets, %ld pieces, %ld payload codes, %ld output bases, context of %ld", n_snippets, (long)n_pieces,
                (long)n_payload, (long)total, (long)C);
  if (n_pieces > 0 && (!pieces || !pieces_host)) return fail(ORCA_EINVAL, "orca_screen_assemble_codes: NULL piece table");
  if (n_payload > 0 && !payload) return fail(ORCA_EINVAL, "orca_screen_assemble_codes: NULL payload");
  const int64_t kmax = INT64_MAX / 4;               // every coordinate stays far below the sums the kernel forms
  ORCA_TRY(walk_snippets("orca_screen_assemble_codes", "pieces", "dst", 0, 3, table_host, n_snippets, pieces_host, n_pieces, total,
    [&](int k, const int64_t* e) -> int {
      return (e[1] < 0 || e[1] > kmax || e[2] > kmax) ? fail(ORCA_EINVAL, "orca_screen_assemble_codes: snippet %d = alt bases [%ld, +%ld)", k, (long)e[1], (long)e[2]) : ORCA_OK;
    },
    [&](int64_t s, const int64_t* pc) -> int {
      if (pc[1] < 0 || pc[1] > 3 || pc[0] < 0 || pc[0] > kmax || pc[3] <= 0 || pc[3] > kmax || pc[2] < 0 || pc[2] > kmax)
        return fail(ORCA_EINVAL, "orca_screen_assemble_codes: piece %ld: alt base %ld, kind %ld, source %ld, %ld bases", (long)s, (long)pc[0], (long)pc[1], (long)pc[2], (long)pc[3]);
      if (pc[1] != 2 || pc[3] <= n_payload - pc[2]) return ORCA_OK;
      return fail(ORCA_EINVAL, "orca_screen_assemble_codes: piece %ld: payload [%ld, +%ld) of %ld", (long)s, (long)pc[2], (long)pc[3], (long)n_payload);
    }));
  if (total == 0) return ORCA_OK;
  return launch(ctx, "screen_assemble_codes_kernel", screen_assemble_codes_kernel, grid256(total), 256, context, (long)C, i64(table), n_snippets, i64(pieces),
                (long)n_pieces, payload, (long)n_payload, out, (long)total);
}

extern "C" int orca_screen_gather_rows(orca_ctx* ctx, const float* ref, int64_t n5, const float* fresh, int64_t n_fresh, const float* const* entries,
                                       const int64_t* entry_rows, const int64_t* entry_rows_host, int P, const int64_t* segments, const int64_t* segments_host,
                                       int64_t n_segments, const int64_t* seg_off, const int64_t* seg_off_host, int B, float* out) {
  if (!ctx || !ref || !seg_off || !seg_off_host || !out) return fail(ORCA_EINVAL, "orca_screen_gather_rows: NULL argument");
  if (B < 0 || n5 < 0 || n_fresh < 0 || n_segments < 0 || P < 0)
    return fail(ORCA_EINVAL, "orca_screen_gather_rows: %d images of %ld rows, %ld fresh rows, %d phase entries, %ld segments", B, (long)n5, (long)n_fresh, P, (long)n_segments);
  if (n_fresh > 0 && !fresh) return fail(ORCA_EINVAL, "orca_screen_gather_rows: NULL fresh rows");
  if (P > 0 && (!entries || !entry_rows || !entry_rows_host)) return fail(ORCA_EINVAL, "orca_screen_gather_rows: NULL phase entries");
  if (n_segments > 0 && (!segments || !segments_host)) return fail(ORCA_EINVAL, "orca_screen_gather_rows: NULL segment table");
  for (int p = 0; p < P; ++p)
    if (entry_rows_host[p] < 0) return fail(ORCA_EINVAL, "orca_screen_gather_rows: phase entry %d has %ld rows", p, (long)entry_rows_host[p]);
  ORCA_TRY(walk_segments("orca_screen_gather_rows", SCREEN_GATHER_FIELDS, segments_host, n_segments, seg_off_host, B, [&](int64_t s, const int64_t* g) -> int {
    if (g[0] < 0 || g[1] <= 0 || g[1] > n5 - g[0]) return fail(ORCA_EINVAL, "orca_screen_gather_rows: segment %ld = rows [%ld, +%ld) of %ld", (long)s, (long)g[0], (long)g[1], (long)n5);
    if (g[2] < -2 || g[2] >= P) return fail(ORCA_EINVAL, "orca_screen_gather_rows: segment %ld has source %ld (-1 fresh, -2 ref, or a phase entry below %d)", (long)s, (long)g[2], P);
    const int64_t have = g[2] == -1 ? n_fresh : g[2] == -2 ? n5 : entry_rows_host[g[2]], step = g[2] >= 0 ? 5 : 1;      // a pooled row reads 5 of its entry's
    if (g[3] >= 0 && g[3] <= have && g[1] <= (have - g[3]) / step) return ORCA_OK;
    return fail(ORCA_EINVAL, "orca_screen_gather_rows: segment %ld reads %ld rows from row %ld of source %ld, which cannot give them", (long)s, (long)g[1], (long)g[3], (long)g[2]);
  }));
  if (B == 0 || n5 == 0) return ORCA_OK;
  if (!al16(ref) || !al16(out) || (fresh && !al16(fresh))) return fail(ORCA_EINVAL, "orca_screen_gather_rows: rows must be 16-byte aligned");
  return launch(ctx, "screen_gather_rows_kernel", screen_gather_rows_kernel, grid256((long)B * n5 * 32), 256, f4(ref), (long)n5, f4(fresh), (long)n_fresh,
                reinterpret_cast<const f32x4* const*>(entries), i64(entry_rows), P, i64(segments), (long)n_segments, i64(seg_off), B, reinterpret_cast<f32x4*>(out));
}

// ---- scores ----------------------------------------------------------------------------------------------------------------------------------------------------
extern "C" int orca_screen_scores(orca_ctx* ctx, const float* alt, int64_t map_bs, const float* ref, int B, int n, float* profile, float* mean, float* amax) {
  if (!ctx || !alt || !ref || !profile || !mean || !amax) return fail(ORCA_EINVAL, "orca_screen_scores: NULL argument");
  if (B <= 0 || n <= 0) return ORCA_OK;
  return launch(ctx, "screen_scores_kernel", screen_scores_kernel, dim3((unsigned)B), 512, alt, (long)map_bs, ref, n, profile, mean, amax);
}

extern "C" int orca_screen_region_scores(orca_ctx* ctx, const float* alt, int64_t map_bs, const float* ref, int B, int n, const int32_t* rects,
                                         const int32_t* rects_host, int K, float* mean_signed, float* mean_abs) {
  if (!ctx || !alt || !ref || !rects || !rects_host || !mean_signed || !mean_abs) return fail(ORCA_EINVAL, "orca_screen_region_scores: NULL argument");
  if (B < 0 || n <= 0 || K <= 0 || K > 64 || map_bs < 0) return fail(ORCA_EINVAL, "orca_screen_region_scores: %d maps of %d bins, %d rectangles (1..64)", B, n, K);
  ORCA_TRY(check_rects("orca_screen_region_scores", rects_host, K, n));
  if (B == 0) return ORCA_OK;
  return launch(ctx, "screen_region_scores_kernel", screen_region_scores_kernel, dim3((unsigned)B, (unsigned)K), 256, alt, (long)map_bs, ref, n, rects, K, mean_signed,
                mean_abs);
}

extern "C" int orca_screen_aligned_scores(orca_ctx* ctx, const float* alt, int64_t map_bs, const float* ref, int B, int n, const int32_t* bin_map,
                                          const int32_t* bin_map_host, float* profile, float* mean, float* amax) {
  if (!ctx || !alt || !ref || !bin_map || !bin_map_host || !profile || !mean || !amax) return fail(ORCA_EINVAL, "orca_screen_aligned_scores: NULL argument");
  if (B < 0 || n <= 0 || n > SCREEN_ALIGNED_MAX_BINS || map_bs < 0)
    return fail(ORCA_EINVAL, "orca_screen_aligned_scores: %d maps of %d bins (1..%d), batch stride %ld", B, n, SCREEN_ALIGNED_MAX_BINS, (long)map_bs);
  ORCA_TRY(check_bin_map("orca_screen_aligned_scores", bin_map_host, B, n));
  if (B == 0) return ORCA_OK;
  return launch(ctx, "screen_aligned_scores_kernel", screen_aligned_scores_kernel, dim3((unsigned)B), 512, alt, (long)map_bs, ref, n, bin_map, profile, mean, amax);
}

extern "C" int orca_screen_aligned_region_scores(orca_ctx* ctx, const float* alt, int64_t map_bs, const float* ref, int B, int n, const int32_t* bin_map,
                                                 const int32_t* bin_map_host, const int32_t* rects, const int32_t* rects_host, int K, float* mean_signed,
                                                 float* mean_abs) {
  if (!ctx || !alt || !ref || !bin_map || !bin_map_host || !rects || !rects_host || !mean_signed || !mean_abs)
    return fail(ORCA_EINVAL, "orca_screen_aligned_region_scores: NULL argument");
  if (B < 0 || n <= 0 || n > SCREEN_ALIGNED_MAX_BINS || K <= 0 || K > 64 || map_bs < 0)
    return fail(ORCA_EINVAL, "orca_screen_aligned_region_scores: %d maps of %d bins (1..%d), %d rectangles (1..64)", B, n, SCREEN_ALIGNED_MAX_BINS, K);
  ORCA_TRY(check_rects("orca_screen_aligned_region_scores", rects_host, K, n));
  ORCA_TRY(check_bin_map("orca_screen_aligned_region_scores", bin_map_host, B, n));
  if (B == 0) return ORCA_OK;
  return launch(ctx, "screen_aligned_region_scores_kernel", screen_aligned_region_scores_kernel, dim3((unsigned)B, (unsigned)K), 256, alt, (long)map_bs, ref, n, bin_map,
                rects, K, mean_signed, mean_abs);
}

// ---- non-additivity --------------------------------------------------------------------------------------------------------------------------------------------
// what the two epistasis entry points share: the maps, the bank and the member table (offsets from 0 to P, strictly increasing - no empty set - and every
// index inside the bank)
static int check_epistasis(const char* what, int64_t map_bs, int64_t bank_bs, int B, int n, int U, const int64_t* member_off_host, const int32_t* members_host, int64_t P) {
  if (B < 1 || n < 1 || U < 1 || P < 1) return fail(ORCA_EINVAL, "%s: %d sets (>= 1) of %d bins (>= 1), a bank of %d maps (>= 1), %ld members (>= 1)", what, B, n, U, (long)P);
  const int64_t nn = (int64_t)n * n;
  if (map_bs < nn || bank_bs < nn) return fail(ORCA_EINVAL, "%s: batch strides %ld (alt), %ld (bank) below the map's %ld floats", what, (long)map_bs, (long)bank_bs, (long)nn);
  if (member_off_host[0] != 0) return fail(ORCA_EINVAL, "%s: member offsets start at %ld, expected 0", what, (long)member_off_host[0]);
  for (int b = 0; b < B; ++b) {
    if (member_off_host[b + 1] < member_off_host[b]) return fail(ORCA_EINVAL, "%s: member offsets decrease at set %d", what, b);
    if (member_off_host[b + 1] > P) return fail(ORCA_EINVAL, "%s: member offsets reach %ld at set %d, the table holds %ld members", what, (long)member_off_host[b + 1], b, (long)P);
    if (member_off_host[b + 1] == member_off_host[b]) return fail(ORCA_EINVAL, "%s: set %d is empty (a set has at least one member)", what, b);
  }
  if (member_off_host[B] != P) return fail(ORCA_EINVAL, "%s: member offsets end at %ld, the table holds %ld members", what, (long)member_off_host[B], (long)P);
  for (int64_t m = 0; m < P; ++m)
    if (members_host[m] < 0 || members_host[m] >= U) return fail(ORCA_EINVAL, "%s: member %ld is bank map %d, outside 0 .. %d", what, (long)m, members_host[m], U - 1);
  return ORCA_OK;
}

extern "C" int orca_screen_epistasis_scores(orca_ctx* ctx, const float* alt, int64_t map_bs, const float* bank, int64_t bank_bs, int U, const float* ref, int B, int n,
                                            const int64_t* member_off, const int64_t* member_off_host, const int32_t* members, const int32_t* members_host, int64_t P,
                                            float* profile, float* mean, float* amax, float* add_mean) {
  if (!ctx || !alt || !bank || !ref || !member_off || !member_off_host || !members || !members_host || !profile || !mean || !amax || !add_mean)
    return fail(ORCA_EINVAL, "orca_screen_epistasis_scores: NULL argument");
  ORCA_TRY(check_epistasis("orca_screen_epistasis_scores", map_bs, bank_bs, B, n, U, member_off_host, members_host, P));
  return launch(ctx, "screen_epistasis_scores_kernel", screen_epistasis_scores_kernel, dim3((unsigned)B), 512, alt, (long)map_bs, bank, (long)bank_bs, U, ref, n,
                i64(member_off), members, (long)P, profile, mean, amax, add_mean);
}

extern "C" int orca_screen_epistasis_region_scores(orca_ctx* ctx, const float* alt, int64_t map_bs, const float* bank, int64_t bank_bs, int U, const float* ref, int B,
                                                   int n, const int64_t* member_off, const int64_t* member_off_host, const int32_t* members,
                                                   const int32_t* members_host, int64_t P, const int32_t* rects, const int32_t* rects_host, int K, float* mean_signed,
                                                   float* mean_abs) {
  if (!ctx || !alt || !bank || !ref || !member_off || !member_off_host || !members || !members_host || !rects || !rects_host || !mean_signed || !mean_abs)
    return fail(ORCA_EINVAL, "orca_screen_epistasis_region_scores: NULL argument");
  ORCA_TRY(check_epistasis("orca_screen_epistasis_region_scores", map_bs, bank_bs, B, n, U, member_off_host, members_host, P));
  if (K < 1 || K > 64) return fail(ORCA_EINVAL, "orca_screen_epistasis_region_scores: %d rectangles (1..64)", K);
  ORCA_TRY(check_rects("orca_screen_epistasis_region_scores", rects_host, K, n));
  return launch(ctx, "screen_epistasis_region_scores_kernel", screen_epistasis_region_scores_kernel, dim3((unsigned)B, (unsigned)K), 256, alt, (long)map_bs, bank,
                (long)bank_bs, U, ref, n, i64(member_off), members, (long)P, rects, K, mean_signed, mean_abs);
}

// ---- tracks ----------------------------------------------------------------------------------------------------------------------------------------------------
// what the two track entry points share: the maps, and the bin map that comes exactly with the aligned output
static int check_track_maps(const char* what, int64_t map_bs, int B, int n, const int32_t* bin_map, const int32_t* bin_map_host, const float* aligned) {
  if (B < 1 || n < 1 || n > SCREEN_ALIGNED_MAX_BINS || map_bs < (int64_t)n * n)
    return fail(ORCA_EINVAL, "%s: %d maps (>= 1) of %d bins (1..%d), batch stride %ld (>= n * n)", what, B, n, SCREEN_ALIGNED_MAX_BINS, (long)map_bs);
  if ((aligned != nullptr) != (bin_map != nullptr)) return fail(ORCA_EINVAL, "%s: the aligned output and the bin map come together or not at all", what);
  if (bin_map && !bin_map_host) return fail(ORCA_EINVAL, "%s: NULL host copy of the bin map", what);
  return bin_map ? check_bin_map(what, bin_map_host, B, n) : ORCA_OK;
}

extern "C" int orca_screen_insulation(orca_ctx* ctx, const float* alt, int64_t map_bs, const float* ref, int B, int n, const int32_t* widths,
                                      const int32_t* widths_host, int W, const int32_t* bin_map, const int32_t* bin_map_host, float* track, float* delta,
                                      float* aligned) {
  if (!ctx || !alt || !widths || !widths_host || !track) return fail(ORCA_EINVAL, "orca_screen_insulation: NULL argument");
  if (!ref && (delta || aligned || bin_map)) return fail(ORCA_EINVAL, "orca_screen_insulation: without ref only the track is written (delta, aligned and bin_map must be NULL)");
  ORCA_TRY(check_track_maps("orca_screen_insulation", map_bs, B, n, bin_map, bin_map_host, aligned));
  if (W < 1 || W > SCREEN_INSULATION_MAX_WIDTHS) return fail(ORCA_EINVAL, "orca_screen_insulation: %d widths (1..%d)", W, SCREEN_INSULATION_MAX_WIDTHS);
  for (int k = 0; k < W; ++k)
    if (widths_host[k] < 1 || widths_host[k] > SCREEN_INSULATION_MAX_WIDTH)
      return fail(ORCA_EINVAL, "orca_screen_insulation: width %d is %d bins, outside 1 .. %d", k, widths_host[k], SCREEN_INSULATION_MAX_WIDTH);
  const unsigned chunks = (unsigned)((n + SCREEN_INSULATION_BINS - 1) / SCREEN_INSULATION_BINS);
  return launch(ctx, "screen_insulation_kernel", screen_insulation_kernel, dim3((unsigned)B, (unsigned)W, chunks), 256, alt, (long)map_bs, ref, n, widths, W, bin_map, track,
                delta, aligned);
}

extern "C" int orca_screen_viewpoints(orca_ctx* ctx, const float* alt, int64_t map_bs, const float* ref, int B, int n, const int32_t* views,
                                      const int32_t* views_host, int V, const int32_t* bin_map, const int32_t* bin_map_host, float* delta, float* aligned) {
  if (!ctx || !alt || !ref || !views || !views_host || !delta) return fail(ORCA_EINVAL, "orca_screen_viewpoints: NULL argument");
  ORCA_TRY(check_track_maps("orca_screen_viewpoints", map_bs, B, n, bin_map, bin_map_host, aligned));
  if (V < 1 || V > SCREEN_VIEWPOINTS_MAX) return fail(ORCA_EINVAL, "orca_screen_viewpoints: %d viewpoints (1..%d)", V, SCREEN_VIEWPOINTS_MAX);
  for (int v = 0; v < V; ++v)
    if (views_host[v] < 0 || views_host[v] >= n) return fail(ORCA_EINVAL, "orca_screen_viewpoints: viewpoint %d is bin %d, outside 0 .. %d", v, views_host[v], n - 1);
  return launch(ctx, "screen_viewpoints_kernel", screen_viewpoints_kernel, dim3((unsigned)B, (unsigned)V), 256, alt, (long)map_bs, ref, n, views, V, bin_map, delta, aligned);
}

// ---- distance strata --------------------------------------------------------------------------------------------------------------------------------------------
extern "C" int orca_screen_strata_scores(orca_ctx* ctx, const float* alt, int64_t map_bs, const float* ref, int B, int n, const int32_t* bin_map,
                                         const int32_t* bin_map_host, int d_lo, int d_hi, float* dist_delta, float* dist_abs, float* dist_rms, double* dist_corr,
                                         int32_t* dist_count, float* mse, double* corr, double* scc) {
  if (!ctx || !alt || !ref || !dist_delta || !dist_abs || !dist_rms || !dist_corr || !mse || !corr || !scc)
    return fail(ORCA_EINVAL, "orca_screen_strata_scores: NULL argument");
  if (B < 1 || n < 1 || n > SCREEN_ALIGNED_MAX_BINS || map_bs < (int64_t)n * n)
    return fail(ORCA_EINVAL, "orca_screen_strata_scores: %d maps (>= 1) of %d bins (1..%d), batch stride %ld (>= n * n)", B, n, SCREEN_ALIGNED_MAX_BINS, (long)map_bs);
  if (d_lo < 0 || d_lo >= d_hi || d_hi > n) return fail(ORCA_EINVAL, "orca_screen_strata_scores: strata [%d, %d) of a map of %d bins (0 <= d_lo < d_hi <= n)", d_lo, d_hi, n);
  if ((bin_map != nullptr) != (bin_map_host != nullptr)) return fail(ORCA_EINVAL, "orca_screen_strata_scores: the bin map and its host copy come together or not at all");
  if ((dist_count != nullptr) != (bin_map != nullptr)) return fail(ORCA_EINVAL, "orca_screen_strata_scores: dist_count and the bin map come together or not at all");
  if (bin_map) ORCA_TRY(check_bin_map("orca_screen_strata_scores", bin_map_host, B, n));
  return launch(ctx, "screen_strata_scores_kernel", screen_strata_scores_kernel, dim3((unsigned)B), 256, alt, (long)map_bs, ref, n, bin_map, d_lo, d_hi, dist_delta,
                dist_abs, dist_rms, dist_corr, dist_count, mse, corr, scc);
}

// ---- paired aligned scores: every alt map against a reference map of its own (the SV screen) ------------------------------------------------------------------
extern "C" int orca_screen_paired_aligned_scores(orca_ctx* ctx, const float* alt, int64_t alt_bs, const float* ref, int64_t ref_bs, int B, int n,
                                                 const int32_t* bin_map, const int32_t* bin_map_host, float* profile, float* abs_mean, float* abs_max,
                                                 float* delta_mean, float* rms, double* corr, int32_t* count) {
  if (!ctx || !alt || !ref || !bin_map || !bin_map_host || !profile || !abs_mean || !abs_max || !delta_mean || !rms || !corr || !count)
    return fail(ORCA_EINVAL, "orca_screen_paired_aligned_scores: NULL argument");
  if (B < 1 || n < 1 || n > SCREEN_ALIGNED_MAX_BINS || alt_bs < (int64_t)n * n || ref_bs < (int64_t)n * n)
    return fail(ORCA_EINVAL, "orca_screen_paired_aligned_scores: %d pairs (>= 1) of maps of %d bins (1..%d), batch strides %ld (alt), %ld (ref) (>= n * n)", B, n,
                SCREEN_ALIGNED_MAX_BINS, (long)alt_bs, (long)ref_bs);
  ORCA_TRY(check_bin_map("orca_screen_paired_aligned_scores", bin_map_host, B, n));
  return launch(ctx, "screen_paired_aligned_scores_kernel", screen_paired_aligned_scores_kernel, dim3((unsigned)B), 512, alt, (long)alt_bs, ref, (long)ref_bs, n,
                bin_map, profile, abs_mean, abs_max, delta_mean, rms, corr, count);
}

// ---- paired tracks and strata: the readouts above, every alt map against a reference map of its own (sv.sv_screen(..., insulation=, viewpoints=, strata=)) ---
// what the three share: the pairs, their strides and the bin map, which is required
static int check_pairs(const char* what, int64_t alt_bs, int64_t ref_bs, int B, int n, const int32_t* bin_map_host) {
  if (B < 1 || n < 1 || n > SCREEN_ALIGNED_MAX_BINS || alt_bs < (int64_t)n * n || ref_bs < (int64_t)n * n)
    return fail(ORCA_EINVAL, "%s: %d pairs (>= 1) of maps of %d bins (1..%d), batch strides %ld (alt), %ld (ref) (>= n * n)", what, B, n, SCREEN_ALIGNED_MAX_BINS,
                (long)alt_bs, (long)ref_bs);
  return check_bin_map(what, bin_map_host, B, n);
}

extern "C" int orca_screen_paired_insulation(orca_ctx* ctx, const float* alt, int64_t alt_bs, const float* ref, int64_t ref_bs, int B, int n, const int32_t* widths,
                                             const int32_t* widths_host, int W, const int32_t* bin_map, const int32_t* bin_map_host, float* track,
                                             float* ref_track, float* aligned) {
  if (!ctx || !alt || !ref || !widths || !widths_host || !bin_map || !bin_map_host || !track || !ref_track || !aligned)
    return fail(ORCA_EINVAL, "orca_screen_paired_insulation: NULL argument");
  ORCA_TRY(check_pairs("orca_screen_paired_insulation", alt_bs, ref_bs, B, n, bin_map_host));
  if (W < 1 || W > SCREEN_INSULATION_MAX_WIDTHS) return fail(ORCA_EINVAL, "orca_screen_paired_insulation: %d widths (1..%d)", W, SCREEN_INSULATION_MAX_WIDTHS);
  for (int k = 0; k < W; ++k)
    if (widths_host[k] < 1 || widths_host[k] > SCREEN_INSULATION_MAX_WIDTH)
      return fail(ORCA_EINVAL, "orca_screen_paired_insulation: width %d is %d bins, outside 1 .. %d", k, widths_host[k], SCREEN_INSULATION_MAX_WIDTH);
  const unsigned chunks = (unsigned)((n + SCREEN_INSULATION_BINS - 1) / SCREEN_INSULATION_BINS);
  return launch(ctx, "screen_paired_insulation_kernel", screen_paired_insulation_kernel, dim3((unsigned)B, (unsigned)W, chunks), 256, alt, (long)alt_bs, ref,
                (long)ref_bs, n, widths, W, bin_map, track, ref_track, aligned);
}

extern "C" int orca_screen_paired_viewpoints(orca_ctx* ctx, const float* alt, int64_t alt_bs, const float* ref, int64_t ref_bs, int B, int n, const int32_t* views,
                                             const int32_t* views_host, int V, const int32_t* bin_map, const int32_t* bin_map_host, float* aligned, int32_t* count) {
  if (!ctx || !alt || !ref || !views || !views_host || !bin_map || !bin_map_host || !aligned || !count)
    return fail(ORCA_EINVAL, "orca_screen_paired_viewpoints: NULL argument");
  ORCA_TRY(check_pairs("orca_screen_paired_viewpoints", alt_bs, ref_bs, B, n, bin_map_host));
  if (V < 1 || V > SCREEN_VIEWPOINTS_MAX) return fail(ORCA_EINVAL, "orca_screen_paired_viewpoints: %d viewpoints (1..%d)", V, SCREEN_VIEWPOINTS_MAX);
  for (int b = 0; b < B; ++b)
    for (int v = 0; v < V; ++v) {
      const int32_t x = views_host[(size_t)b * V + v];
      if (x < -1 || x >= n) return fail(ORCA_EINVAL, "orca_screen_paired_viewpoints: viewpoint %d of pair %d is reference bin %d, outside -1 .. %d", v, b, x, n - 1);
    }
  return launch(ctx, "screen_paired_viewpoints_kernel", screen_paired_viewpoints_kernel, dim3((unsigned)B, (unsigned)V), 256, alt, (long)alt_bs, ref, (long)ref_bs, n,
                views, V, bin_map, aligned, count);
}

extern "C" int orca_screen_paired_strata_scores(orca_ctx* ctx, const float* alt, int64_t alt_bs, const float* ref, int64_t ref_bs, int B, int n,
                                                const int32_t* bin_map, const int32_t* bin_map_host, int d_lo, int d_hi, float* dist_delta, float* dist_abs,
                                                float* dist_rms, double* dist_corr, int32_t* dist_count, float* mse, double* corr, double* scc) {
  if (!ctx || !alt || !ref || !bin_map || !bin_map_host || !dist_delta || !dist_abs || !dist_rms || !dist_corr || !dist_count || !mse || !corr || !scc)
    return fail(ORCA_EINVAL, "orca_screen_paired_strata_scores: NULL argument");
  ORCA_TRY(check_pairs("orca_screen_paired_strata_scores", alt_bs, ref_bs, B, n, bin_map_host));
  if (d_lo < 0 || d_lo >= d_hi || d_hi > n)
    return fail(ORCA_EINVAL, "orca_screen_paired_strata_scores: strata [%d, %d) of a map of %d bins (0 <= d_lo < d_hi <= n)", d_lo, d_hi, n);
  return launch(ctx, "screen_paired_strata_scores_kernel", screen_paired_strata_scores_kernel, dim3((unsigned)B), 256, alt, (long)alt_bs, ref, (long)ref_bs, n,
                bin_map, d_lo, d_hi, dist_delta, dist_abs, dist_rms, dist_corr, dist_count, mse, corr, scc);
}

// ---- loops: dot calls and the enrichment at listed pixels ---------------------------------------------------------------------------------------------------------
static int check_dot_params(const char* what, int B, int n, int64_t map_bs, int p, int w, int d_min) {
  if (B < 1 || n < 1 || n > SCREEN_ALIGNED_MAX_BINS || map_bs < (int64_t)n * n)
    return fail(ORCA_EINVAL, "%s: %d maps (>= 1) of %d bins (1..%d), batch stride %ld (>= n * n)", what, B, n, SCREEN_ALIGNED_MAX_BINS, (long)map_bs);
  if (p < 0 || p >= w || w > SCREEN_DOT_MAX_W) return fail(ORCA_EINVAL, "%s: peak half-width p = %d, window half-width w = %d (0 <= p < w <= %d)", what, p, w, SCREEN_DOT_MAX_W);
  if (d_min < 2 * w + 1) return fail(ORCA_EINVAL, "%s: d_min = %d (>= 2 w + 1 = %d: the windows stay above the diagonal)", what, d_min, 2 * w + 1);
  return ORCA_OK;
}

extern "C" int orca_screen_dot_calls(orca_ctx* ctx, const float* maps, int64_t map_bs, int B, int n, int p, int w, int d_min, int r, float T, int K, float* e_map,
                                     int32_t* count, int32_t* ij, float* enrich) {
  if (!ctx || !maps || !e_map || !count || !ij || !enrich) return fail(ORCA_EINVAL, "orca_screen_dot_calls: NULL argument");
  ORCA_TRY(check_dot_params("orca_screen_dot_calls", B, n, map_bs, p, w, d_min));
  if (r < 1 || r > SCREEN_DOT_MAX_R) return fail(ORCA_EINVAL, "orca_screen_dot_calls: local-maximum radius r = %d (1..%d)", r, SCREEN_DOT_MAX_R);
  if (K < 1 || K > SCREEN_DOT_MAX_CALLS) return fail(ORCA_EINVAL, "orca_screen_dot_calls: K = %d listed calls per map (1..%d)", K, SCREEN_DOT_MAX_CALLS);
  if (T != T) return fail(ORCA_EINVAL, "orca_screen_dot_calls: the threshold T is NaN");
  ORCA_TRY(launch(ctx, "screen_dot_enrich_map_kernel", screen_dot_enrich_map_kernel, dim3((unsigned)B, (unsigned)n), 256, maps, (long)map_bs, n, p, w, d_min, e_map));
  return launch(ctx, "screen_dot_calls_kernel", screen_dot_calls_kernel, dim3((unsigned)B), 256, (const float*)e_map, n, w, d_min, r, T, K, count, ij, enrich);
}

extern "C" int orca_screen_dot_enrichment(orca_ctx* ctx, const float* maps, int64_t map_bs, int B, int n, int p, int w, int d_min, const int32_t* pixels,
                                          const int32_t* pixels_host, int Q, float* out) {
  if (!ctx || !maps || !pixels || !pixels_host || !out) return fail(ORCA_EINVAL, "orca_screen_dot_enrichment: NULL argument");
  ORCA_TRY(check_dot_params("orca_screen_dot_enrichment", B, n, map_bs, p, w, d_min));
  if (Q < 1 || Q > SCREEN_DOT_MAX_CALLS) return fail(ORCA_EINVAL, "orca_screen_dot_enrichment: Q = %d pixels per map (1..%d)", Q, SCREEN_DOT_MAX_CALLS);
  for (size_t k = 0; k < (size_t)B * Q * 2; ++k)
    if (pixels_host[k] < -1 || pixels_host[k] >= n)
      return fail(ORCA_EINVAL, "orca_screen_dot_enrichment: pixel %ld of map %ld has coordinate %d, outside -1 .. %d", (long)(k / 2 % Q), (long)(k / 2 / Q), pixels_host[k], n - 1);
  return launch(ctx, "screen_dot_enrichment_kernel", screen_dot_enrichment_kernel, dim3((unsigned)B, (unsigned)((Q + 255) / 256)), 256, maps, (long)map_bs, n, p, w, d_min,
                pixels, Q, out);
}

// the reference dots of B pairs followed into the alt maps' enrichment map; the lists are on the device only (the kernel treats every slot that holds no
// dot as empty), the bin map comes twice
extern "C" int orca_screen_paired_dot_follow(orca_ctx* ctx, const float* alt_e, int64_t e_bs, int B, int n, int w, int d_min, const int32_t* ref_ij,
                                             const float* ref_enrich, int R, const int32_t* bin_map, const int32_t* bin_map_host, int32_t* candidates,
                                             int32_t* at, float* enrich, float* delta) {
  if (!ctx || !alt_e || !ref_ij || !ref_enrich || !bin_map || !bin_map_host || !candidates || !at || !enrich || !delta)
    return fail(ORCA_EINVAL, "orca_screen_paired_dot_follow: NULL argument");
  if (B < 1 || n < 1 || n > SCREEN_ALIGNED_MAX_BINS || e_bs < (int64_t)n * n)
    return fail(ORCA_EINVAL, "orca_screen_paired_dot_follow: %d pairs (>= 1) of enrichment maps of %d bins (1..%d), batch stride %ld (>= n * n)", B, n,
                SCREEN_ALIGNED_MAX_BINS, (long)e_bs);
  if (w < 1 || w > SCREEN_DOT_MAX_W) return fail(ORCA_EINVAL, "orca_screen_paired_dot_follow: window half-width w = %d (1..%d)", w, SCREEN_DOT_MAX_W);
  if (d_min < 2 * w + 1) return fail(ORCA_EINVAL, "orca_screen_paired_dot_follow: d_min = %d (>= 2 w + 1 = %d)", d_min, 2 * w + 1);
  if (R < 1 || R > SCREEN_DOT_MAX_CALLS) return fail(ORCA_EINVAL, "orca_screen_paired_dot_follow: R = %d listed reference dots per pair (1..%d)", R, SCREEN_DOT_MAX_CALLS);
  ORCA_TRY(check_bin_map("orca_screen_paired_dot_follow", bin_map_host, B, n));
  return launch(ctx, "screen_paired_dot_follow_kernel", screen_paired_dot_follow_kernel,
                dim3((unsigned)B, (unsigned)((R + SCREEN_FOLLOW_DOTS - 1) / SCREEN_FOLLOW_DOTS)), 64 * SCREEN_FOLLOW_DOTS, alt_e, (long)e_bs, n, w, d_min, ref_ij,
                ref_enrich, R, bin_map, candidates, at, enrich, delta);
}

// ---- compartments: the leading eigenpairs of B maps, and the GC track that phases them -----------------------------------------------------------------------
extern "C" int orca_screen_eigenvectors(orca_ctx* ctx, const float* maps, int64_t map_bs, int B, int n, int K, int d_lo, int center, double tol, int max_iter,
                                        const float* phase, float* E, double* eigenvalue, double* residual, int32_t* iterations, int32_t* n_valid) {
  if (!ctx || !maps || !E || !eigenvalue || !residual || !iterations || !n_valid) return fail(ORCA_EINVAL, "orca_screen_eigenvectors: NULL argument");
  if (B < 1 || n < 1 || n > SCREEN_ALIGNED_MAX_BINS || map_bs < (int64_t)n * n)
    return fail(ORCA_EINVAL, "orca_screen_eigenvectors: %d maps (>= 1) of %d bins (1..%d), batch stride %ld (>= n * n)", B, n, SCREEN_ALIGNED_MAX_BINS, (long)map_bs);
  if (K < 1 || K > SCREEN_EIG_MAX_K) return fail(ORCA_EINVAL, "orca_screen_eigenvectors: K = %d eigenpairs per map (1..%d)", K, SCREEN_EIG_MAX_K);
  if (d_lo < 0 || d_lo > n - 1) return fail(ORCA_EINVAL, "orca_screen_eigenvectors: d_lo = %d (0..n - 1 = %d)", d_lo, n - 1);
  if (center != 0 && center != 1) return fail(ORCA_EINVAL, "orca_screen_eigenvectors: center = %d (0 or 1)", center);
  if (!(tol > 0.0)) return fail(ORCA_EINVAL, "orca_screen_eigenvectors: tol = %g (> 0)", tol);
  if (max_iter < 1) return fail(ORCA_EINVAL, "orca_screen_eigenvectors: max_iter = %d (>= 1)", max_iter);
  return launch(ctx, "screen_eigenvectors_kernel", screen_eigenvectors_kernel, dim3((unsigned)B), SCREEN_EIG_THREADS, maps, (long)map_bs, n, K, d_lo, center, tol,
                max_iter, phase, E, eigenvalue, residual, iterations, n_valid);
}

// the windows' offsets and bin sizes are host arrays: checked here, handed to the kernel by value, SCREEN_GC_WINDOWS windows per launch
extern "C" int orca_screen_gc_tracks(orca_ctx* ctx, const uint8_t* codes, int64_t L, const int64_t* offsets, const int64_t* binsizes, int W, int n, float* out) {
  if (!ctx || !codes || !offsets || !binsizes || !out) return fail(ORCA_EINVAL, "orca_screen_gc_tracks: NULL argument");
  if (L < 1 || W < 1 || n < 1 || n > 65535) return fail(ORCA_EINVAL, "orca_screen_gc_tracks: %d windows (>= 1) of %d bins (1..65535) of %ld codes (>= 1)", W, n, (long)L);
  for (int w = 0; w < W; ++w)
    if (offsets[w] < 0 || offsets[w] >= L || binsizes[w] < 1 || binsizes[w] > (L - offsets[w]) / n)
      return fail(ORCA_EINVAL, "orca_screen_gc_tracks: window %d = %d bins of %ld bases from base %ld leaves the %ld codes", w, n, (long)binsizes[w], (long)offsets[w], (long)L);
  for (int w0 = 0; w0 < W; w0 += SCREEN_GC_WINDOWS) {
    const int cnt = W - w0 < SCREEN_GC_WINDOWS ? W - w0 : SCREEN_GC_WINDOWS;
    screen_gc_windows win = {};
    for (int w = 0; w < cnt; ++w) {
      win.off[w] = offsets[w0 + w];
      win.bs[w] = binsizes[w0 + w];
    }
    ORCA_TRY(launch(ctx, "screen_gc_tracks_kernel", screen_gc_tracks_kernel, dim3((unsigned)n, (unsigned)cnt), 256, codes, (long)L, win, cnt, n,
                    out + (size_t)w0 * n));
  }
  return ORCA_OK;
}

// ---- boundaries: domain boundary calls from B x W insulation tracks that are on the device already ------------------------------------------------------------
extern "C" int orca_screen_boundary_calls(orca_ctx* ctx, const float* tracks, int B, int W, int n, float min_strength, int K, int32_t* count, int32_t* bins,
                                          float* strength, float* strength_track) {
  if (!ctx || !tracks || !count || !bins || !strength) return fail(ORCA_EINVAL, "orca_screen_boundary_calls: NULL argument");
  if (B < 1 || W < 1 || W > SCREEN_INSULATION_MAX_WIDTHS || n < 3 || n > SCREEN_ALIGNED_MAX_BINS)
    return fail(ORCA_EINVAL, "orca_screen_boundary_calls: %d x %d tracks (B >= 1, W 1..%d) of %d bins (3..%d)", B, W, SCREEN_INSULATION_MAX_WIDTHS, n, SCREEN_ALIGNED_MAX_BINS);
  if (K < 0 || K > n) return fail(ORCA_EINVAL, "orca_screen_boundary_calls: K = %d listed boundaries per track (0..n = %d)", K, n);
  if (!(min_strength >= 0.f)) return fail(ORCA_EINVAL, "orca_screen_boundary_calls: min_strength = %g (>= 0, not NaN)", (double)min_strength);
  return launch(ctx, "screen_boundary_calls_kernel", screen_boundary_calls_kernel, dim3((unsigned)B, (unsigned)W), 256, tracks, n, min_strength, K, count, bins, strength,
                strength_track);
}

// ---- both strands --------------------------------------------------------------------------------------------------------------------------------------------
extern "C" int orca_screen_merge_strands(orca_ctx* ctx, const float* fwd, int64_t fwd_bs, const float* rev, int64_t rev_bs, const float* ref_fwd, const float* ref_rev,
                                         int B, int n, float* out, int64_t out_bs, float* gap) {
  if (!ctx || !fwd || !rev || !out) return fail(ORCA_EINVAL, "orca_screen_merge_strands: NULL argument");
  if (n < 1 || n > 256 || B < 1) return fail(ORCA_EINVAL, "orca_screen_merge_strands: %d maps (>= 1) of %d bins (1..256)", B, n);
  const int64_t nn = (int64_t)n * n;
  if (fwd_bs < nn || rev_bs < nn || out_bs < nn)
    return fail(ORCA_EINVAL, "orca_screen_merge_strands: batch strides %ld (fwd), %ld (rev), %ld (out) below the map's %ld floats", (long)fwd_bs, (long)rev_bs, (long)out_bs, (long)nn);
  if (!ref_fwd) gap = nullptr;                       // the form that merges the reference itself
  if (gap && !ref_rev) return fail(ORCA_EINVAL, "orca_screen_merge_strands: the gap needs both strands' reference maps (ref_rev is NULL)");
  const float* rev_end = rev + (size_t)(B - 1) * rev_bs + nn;
  const float* out_end = out + (size_t)(B - 1) * out_bs + nn;
  if (rev < out_end && out < rev_end) return fail(ORCA_EINVAL, "orca_screen_merge_strands: rev overlaps out (out may be fwd, an element's thread reads and writes it; rev is read mirrored)");
  auto al8 = [](const void* p) { return (reinterpret_cast<uintptr_t>(p) & 7u) == 0; };
  const int vec = n % 2 == 0 && fwd_bs % 2 == 0 && rev_bs % 2 == 0 && out_bs % 2 == 0 && al8(fwd) && al8(rev) && al8(out) && (!gap || (al8(ref_fwd) && al8(ref_rev)));
  return launch(ctx, "screen_merge_strands_kernel", screen_merge_strands_kernel, dim3((unsigned)B), 512, fwd, (long)fwd_bs, rev, (long)rev_bs, ref_fwd, ref_rev, n, out,
                (long)out_bs, gap, vec);
}

// ---- the chromosome scan (orca_amd/scan.py; kernels in scan.h): window maps stitched into a band, the band's insulation, boundary strengths of any length ----
#define SCAN_MAX_TOTAL_BINS (1L << 24)               // N: 67 Gb of 4 kb bins; keeps N * D and every grid far inside their types

extern "C" int orca_scan_stitch_band(orca_ctx* ctx, const float* maps, int64_t map_bs, int B, int n, const int64_t* off, const int64_t* off_host, int trim, int64_t N,
                                     int D, double* sum, int32_t* count, float* lo, float* hi) {
  if (!ctx || !maps || !off || !off_host || !sum || !count || !lo || !hi) return fail(ORCA_EINVAL, "orca_scan_stitch_band: NULL argument");
  if (B < 1 || n < 1 || n > SCAN_MAX_BINS || map_bs < (int64_t)n * n)
    return fail(ORCA_EINVAL, "orca_scan_stitch_band: %d maps (>= 1) of %d bins (1..%d), batch stride %ld (>= n * n)", B, n, SCAN_MAX_BINS, (long)map_bs);
  if (N < n || N > SCAN_MAX_TOTAL_BINS) return fail(ORCA_EINVAL, "orca_scan_stitch_band: a stretch of %ld bins (n = %d .. %ld)", (long)N, n, SCAN_MAX_TOTAL_BINS);
  if (trim < 0 || n - 2 * (int64_t)trim < 1) return fail(ORCA_EINVAL, "orca_scan_stitch_band: trim = %d on maps of %d bins (trim >= 0, n - 2 trim >= 1)", trim, n);
  if (D < 1 || D > n - 2 * trim) return fail(ORCA_EINVAL, "orca_scan_stitch_band: D = %d distances (1 .. n - 2 trim = %d)", D, n - 2 * trim);
  for (int b = 0; b < B; ++b) {
    if (off_host[b] < 0 || off_host[b] > N - n)
      return fail(ORCA_EINVAL, "orca_scan_stitch_band: window %d starts at bin %ld, outside 0 .. N - n = %ld", b, (long)off_host[b], (long)(N - n));
    if (b && off_host[b] <= off_host[b - 1])
      return fail(ORCA_EINVAL, "orca_scan_stitch_band: windows %d and %d start at bins %ld and %ld (strictly ascending)", b - 1, b, (long)off_host[b - 1], (long)off_host[b]);
  }
  const long i0 = (long)off_host[0], rows = (long)off_host[B - 1] + n - i0;
  return launch(ctx, "scan_stitch_band_kernel", scan_stitch_band_kernel, grid256(rows * D), 256, maps, (long)map_bs, B, n, i64(off), trim, (long)N, D, i0, rows, sum, count,
                lo, hi);
}

extern "C" int orca_scan_band_finish(orca_ctx* ctx, const double* sum, const int32_t* count, const float* lo, const float* hi, int64_t N, int D, float* band,
                                     float* range) {
  if (!ctx || !sum || !count || !lo || !hi || !band) return fail(ORCA_EINVAL, "orca_scan_band_finish: NULL argument");
  if (N < 1 || N > SCAN_MAX_TOTAL_BINS || D < 1 || D > SCAN_MAX_BINS)
    return fail(ORCA_EINVAL, "orca_scan_band_finish: a band of %ld bins (1..%ld) x %d distances (1..%d)", (long)N, SCAN_MAX_TOTAL_BINS, D, SCAN_MAX_BINS);
  return launch(ctx, "scan_band_finish_kernel", scan_band_finish_kernel, grid256((long)N * D), 256, sum, count, lo, hi, (long)N, D, band, range);
}

extern "C" int orca_scan_band_insulation(orca_ctx* ctx, const float* band, int64_t N, int D, const int32_t* widths, const int32_t* widths_host, int W, float* track) {
  if (!ctx || !band || !widths || !widths_host || !track) return fail(ORCA_EINVAL, "orca_scan_band_insulation: NULL argument");
  if (N < 1 || N > SCAN_MAX_TOTAL_BINS || D < 1 || D > SCAN_MAX_BINS)
    return fail(ORCA_EINVAL, "orca_scan_band_insulation: a band of %ld bins (1..%ld) x %d distances (1..%d)", (long)N, SCAN_MAX_TOTAL_BINS, D, SCAN_MAX_BINS);
  if (W < 1 || W > SCAN_MAX_WIDTHS) return fail(ORCA_EINVAL, "orca_scan_band_insulation: %d widths (1..%d)", W, SCAN_MAX_WIDTHS);
  for (int k = 0; k < W; ++k) {
    if (widths_host[k] < 1 || 2 * (int64_t)widths_host[k] + 1 > D)
      return fail(ORCA_EINVAL, "orca_scan_band_insulation: width %d is %d bins; 1 <= w and 2 w + 1 <= D = %d (the diamond reaches distance 2 w)", k, widths_host[k], D);
    for (int j = 0; j < k; ++j)
      if (widths_host[j] == widths_host[k]) return fail(ORCA_EINVAL, "orca_scan_band_insulation: widths %d and %d are both %d bins (distinct)", j, k, widths_host[k]);
  }
  return launch(ctx, "scan_band_insulation_kernel", scan_band_insulation_kernel, dim3((unsigned)((N + SCAN_INSULATION_BINS - 1) / SCAN_INSULATION_BINS), (unsigned)W), 256,
                band, (long)N, D, widths, W, track);
}

extern "C" int orca_scan_boundary_strength(orca_ctx* ctx, const float* tracks, int W, int64_t N, float* strength) {
  if (!ctx || !tracks || !strength) return fail(ORCA_EINVAL, "orca_scan_boundary_strength: NULL argument");
  if (W < 1 || W > 65535 || N < 1 || N > SCAN_MAX_TOTAL_BINS)
    return fail(ORCA_EINVAL, "orca_scan_boundary_strength: %d tracks (1..65535) of %ld bins (1..%ld)", W, (long)N, SCAN_MAX_TOTAL_BINS);
  return launch(ctx, "scan_boundary_strength_kernel", scan_boundary_strength_kernel, dim3((unsigned)((N + 255) / 256), (unsigned)W), 256, tracks, (long)N, strength);
}

// ---- loops along the band (scan_1m(..., loops=); kernels in scan_loops.h): the enrichment band, the rows' offsets into the list, the list -----------------------
static int check_band(const char* what, int64_t N, int D) {
  if (N < 1 || N > SCAN_MAX_TOTAL_BINS || D < 2 || D > SCAN_LOOP_MAX_DEPTH)
    return fail(ORCA_EINVAL, "%s: a band of %ld bins (1..%ld) x %d distances (2..%d)", what, (long)N, SCAN_MAX_TOTAL_BINS, D, SCAN_LOOP_MAX_DEPTH);
  return ORCA_OK;
}

static int check_band_calls(const char* what, int64_t N, int D, int r, float T) {
  ORCA_TRY(check_band(what, N, D));
  if (r < 1 || r > SCREEN_DOT_MAX_R) return fail(ORCA_EINVAL, "%s: local-maximum radius r = %d (1..%d)", what, r, SCREEN_DOT_MAX_R);
  if (T != T) return fail(ORCA_EINVAL, "%s: the threshold T is NaN", what);
  return ORCA_OK;
}

static inline int row_threads(int D) { return (D + 63) / 64 * 64; }           // thread d of a row's workgroup stands at distance d: the waves D needs

extern "C" int orca_scan_band_dot_enrichment(orca_ctx* ctx, const float* band, int64_t N, int D, int p, int w, int d_min, float* e_band) {
  if (!ctx || !band || !e_band) return fail(ORCA_EINVAL, "orca_scan_band_dot_enrichment: NULL argument");
  ORCA_TRY(check_band("orca_scan_band_dot_enrichment", N, D));
  if (p < 0 || p >= w || w > SCREEN_DOT_MAX_W)
    return fail(ORCA_EINVAL, "orca_scan_band_dot_enrichment: peak half-width p = %d, window half-width w = %d (0 <= p < w <= %d)", p, w, SCREEN_DOT_MAX_W);
  if (d_min < 2 * w + 1) return fail(ORCA_EINVAL, "orca_scan_band_dot_enrichment: d_min = %d (>= 2 w + 1 = %d: the windows stay above the diagonal)", d_min, 2 * w + 1);
  return launch(ctx, "scan_band_dot_enrich_kernel", scan_band_dot_enrich_kernel, dim3((unsigned)((N + SCAN_LOOP_ROWS - 1) / SCAN_LOOP_ROWS)), 256, band, (long)N, D, p, w,
                d_min, e_band);
}

// two launches: the rows' dot counts into row_start[0 .. N), then their exclusive prefix in place and the total in row_start[N]
extern "C" int orca_scan_band_dot_offsets(orca_ctx* ctx, const float* e_band, int64_t N, int D, int r, float T, int64_t* row_start) {
  if (!ctx || !e_band || !row_start) return fail(ORCA_EINVAL, "orca_scan_band_dot_offsets: NULL argument");
  ORCA_TRY(check_band_calls("orca_scan_band_dot_offsets", N, D, r, T));
  long long* rows = reinterpret_cast<long long*>(row_start);
  ORCA_TRY(launch(ctx, "scan_band_dot_count_kernel", scan_band_dot_count_kernel, dim3((unsigned)N), row_threads(D), e_band, (long)N, D, r, T, rows));
  return launch(ctx, "scan_row_offsets_kernel", scan_row_offsets_kernel, dim3(1), 256, rows, (long)N);
}

extern "C" int orca_scan_band_dot_list(orca_ctx* ctx, const float* e_band, int64_t N, int D, int r, float T, const int64_t* row_start, int64_t cap, int64_t* ij,
                                       float* enrich) {
  if (!ctx || !e_band || !row_start || !ij || !enrich) return fail(ORCA_EINVAL, "orca_scan_band_dot_list: NULL argument");
  ORCA_TRY(check_band_calls("orca_scan_band_dot_list", N, D, r, T));
  if (cap < 0) return fail(ORCA_EINVAL, "orca_scan_band_dot_list: cap = %ld slots (>= 0)", (long)cap);
  if (cap == 0) return ORCA_OK;                                              // an empty list: nothing to write
  return launch(ctx, "scan_band_dot_list_kernel", scan_band_dot_list_kernel, dim3((unsigned)N), row_threads(D), e_band, (long)N, D, r, T, i64(row_start), (long)cap,
                reinterpret_cast<long long*>(ij), enrich);
}
