// orca_encoder.hip - Conv1d launchers, the Encoder (orca_modules.py:929-980) and the U-net encoders Encoder2 / Encoder3 / Encoder2b (:1151-1169, :1388-1406, :1262-1276)
// Part of liborca_hip.so (include/orca_hip.h is the ABI; orca_internal.h what the units share).
#include "orca_internal.h"

#include "conv_kernels.h"
#include "conv_bf16s.h"
#include "conv_stage1.h"
#include "conv_p16.h"
#include "conv_ws.h"
#include "conv_p16w1.h"
#include "conv_p16p5.h"
#include "conv_p16x.h"
#include "conv_small.h"
#include "misc_kernels.h"
#include "p16_planes.h"
#include "screen.h"   // screen_rows_to_bins_kernel (orca_encoder_back5_batch)

// ---------------------------------------------------------------------------
// kernel launch helpers
// ---------------------------------------------------------------------------
template <int COUT, int MW, int NW, int WM, int WN, int KC>
static void launch_conv1d_t(hipStream_t s, const Conv1dArgs& a, int B) {
  constexpr int MT = WM * MW * 32;
  dim3 grid((unsigned)((a.n + MT - 1) / MT), (unsigned)B);
  hipLaunchKernelGGL((conv1d_k9_kernel<COUT, MW, NW, WM, WN, KC>), grid, dim3(WM * WN * 64), 0, s, a);
}

int launch_conv1d(orca_ctx* ctx, const ConvLayer& L, const float* x, long x_bs, long ldx, float* y, long y_bs,
                         long ldy, const float* r1, const float* r2, int B, long n, int relu, int tile, int y_nlc) {
  if (L.ksize != 9) return fail(ORCA_EINVAL, "launch_conv1d on a non-1d layer");
  if (n <= 0 || B <= 0) return ORCA_OK;
  Conv1dArgs a;
  a.x = x; a.w = L.d_w; a.bias = L.d_bias; a.y = y; a.r1 = r1; a.r2 = r2;
  a.x_bs = x_bs; a.y_bs = y_bs; a.ldx = ldx; a.ldy = ldy; a.n = n; a.nchunks = L.nchunks; a.relu = relu; a.y_nlc = y_nlc;
  a.x_vec_ok = al16(x) && (ldx % 4 == 0) && (x_bs % 4 == 0);
  a.y_vec_ok = al16(y) && (ldy % 4 == 0) && (y_bs % 4 == 0) && (!r1 || al16(r1)) && (!r2 || al16(r2));
  hipStream_t s = ctx->stream;
  LaunchTimer timer(ctx, n);
  ORCA_TRY(timer.open());
  int used_tile = 256;
  if (L.cout == 64) {
    if (L.kc == 4) launch_conv1d_t<64, 2, 2, 4, 1, 4>(s, a, B);
    else launch_conv1d_t<64, 2, 2, 4, 1, 8>(s, a, B);
  } else if (L.cout == 96) {
    launch_conv1d_t<96, 2, 3, 4, 1, 8>(s, a, B);
  } else {
    // position tile of the long 128-channel convs: 128 (2 waves/SIMD, 4 accumulators/wave); 256 (1 wave/SIMD, 8 accumulators/wave) on request (`tile`)
    if (tile == 0) tile = (n >= 65536) ? 128 : (n >= 8192 ? 64 : 32);
    if (tile == 256) launch_conv1d_t<128, 4, 2, 2, 2, 8>(s, a, B);
    else if (tile == 128) launch_conv1d_t<128, 2, 2, 2, 2, 8>(s, a, B);
    else if (tile == 64) launch_conv1d_t<128, 1, 2, 2, 2, 8>(s, a, B);
    else if (tile == 32) launch_conv1d_t<128, 1, 1, 1, 4, 8>(s, a, B);
    else return fail(ORCA_EINVAL, "conv1d tile %d unsupported", tile);
    used_tile = tile;
  }
  LAUNCHCHECK("conv1d_k9_kernel");
  return timer.close(L.cout, L.cin, used_tile, B, n, 9);
}

int launch_pool(orca_ctx* ctx, const float* x, long ldx, float* y, long ldy, long rows, long n_out, int k) {
  if (n_out <= 0 || rows <= 0) return ORCA_OK;
  dim3 grid((unsigned)((n_out + 255) / 256), (unsigned)rows);
  switch (k) {
    case 2: hipLaunchKernelGGL((maxpool1d_kernel<2>), grid, dim3(256), 0, ctx->stream, x, ldx, y, ldy, n_out); break;
    case 4: hipLaunchKernelGGL((maxpool1d_kernel<4>), grid, dim3(256), 0, ctx->stream, x, ldx, y, ldy, n_out); break;
    case 5: hipLaunchKernelGGL((maxpool1d_kernel<5>), grid, dim3(256), 0, ctx->stream, x, ldx, y, ldy, n_out); break;
    default: return fail(ORCA_EINVAL, "maxpool k=%d unsupported", k);
  }
  LAUNCHCHECK("maxpool1d_kernel");
  return ORCA_OK;
}

// ---- bf16 split-operand conv1d (channel-last activations) --------------------------------
template <int COUT, int MW, int NW, int WM, int WN, int NS, int DT>
static void launch_b16_t(hipStream_t s, ConvB16Args a, int B) {
  constexpr int MT = WM * MW * 32;
  const int resident = resident_workgroups<conv1d_k9_bf16s_kernel<COUT, MW, NW, WM, WN, NS, DT>, WM * WN * 64>();
  a.tiles_per_row = (a.n + MT - 1) / MT;
  a.batch = B;
  const long ntiles = a.tiles_per_row * B;
  dim3 grid((unsigned)(ntiles < resident ? ntiles : resident));
  hipLaunchKernelGGL((conv1d_k9_bf16s_kernel<COUT, MW, NW, WM, WN, NS, DT>), grid, dim3(WM * WN * 64), 0, s, a);
}

template <int NS, int DT>
static int launch_conv1d_b16_ns(orca_ctx* ctx, const ConvLayer& L, const ConvB16Args& a, int B, int fixed_tile = 0) {
  hipStream_t s = ctx->stream;
  if (L.cout == 64) launch_b16_t<64, 2, 2, 4, 1, NS, DT>(s, a, B);
  else if (L.cout == 96) launch_b16_t<96, 1, 3, 8, 1, NS, DT>(s, a, B);
  else if (L.cout == 128) {
    // stages 6-7 of the Encoder (16 000 / 8 000 positions) make 63 / 32 tiles of 256 positions for 256 CUs: 64-position tiles there
    // (fixed_tile 1: the 256-position tiles whatever the batch - a batch of edits is many rows; 2: what one row of the batch would take alone)
    if constexpr (NS <= 2) {
      if (fixed_tile != 1 && ((a.n + 255) / 256) * (fixed_tile == 2 ? 1 : B) < 200) { launch_b16_t<128, 1, 2, 2, 2, NS, DT>(s, a, B); return ORCA_OK; }
    }
    launch_b16_t<128, 2, 2, 4, 2, NS, DT>(s, a, B);
  }
  else return fail(ORCA_EINVAL, "bf16s conv1d cout %d unsupported", L.cout);
  return ORCA_OK;
}

// x [B][n][cin], y/r1 [B][n][cout] channel-last.  precision: ORCA_PRECISION_BF16 / _BF16X2 / _BF16X3
int launch_conv1d_b16(orca_ctx* ctx, const ConvLayer& L, int precision, const float* x, long x_bs, float* y, long y_bs,
                             const float* r1, int B, long n, int relu, int pool4, const float* r2, int fixed_tile) {
  if (!L.d_wb16) return fail(ORCA_EINVAL, "layer has no bf16 split pack (cin %d)", L.cin);
  if (n <= 0 || B <= 0) return ORCA_OK;
  ConvB16Args a;
  a.x = x; a.w = L.d_wb16; a.bias = L.d_bias; a.y = y; a.r1 = r1; a.r2 = r2; a.x_bs = x_bs; a.y_bs = y_bs; a.n = n;
  a.pool4 = pool4; a.r_bs = (long)n * L.cout;
  a.cin = L.cin; a.nchunks = L.cin / 16; a.relu = relu; a.stagger = 2;
  a.flag = ctx->d_flag;
  if (precision == ORCA_PRECISION_F16X2) {
    if (!L.f16_ok) return fail(ORCA_EINVAL, "layer weights exceed the fp16 range: use ORCA_PRECISION_BF16X3");
    a.w = L.d_wf16;
  }
  LaunchTimer timer(ctx, n);
  ORCA_TRY(timer.open());
  int rc;
  a.cout = L.cout;
  // short rows (the Encoder's stages 5-7 of a local re-encode, one- to three-bin inputs): the K-chunks of a tile side by side, one global
  // round trip and one barrier per launch instead of a chain of eight (conv_small.h: ~6 against 23-27 us).  A function of n alone, so that
  // a row's result never depends on the batch it is computed in
  if (n <= 2048 && !pool4 && L.cout % 32 == 0 && L.cin % 16 == 0) {
    const dim3 grid((unsigned)(((n + 31) / 32) * (L.cout / 32)), (unsigned)B);
    if (precision == ORCA_PRECISION_BF16X3) hipLaunchKernelGGL((conv1d_k9_small_kernel<3, 0>), grid, dim3(512), 0, ctx->stream, a);
    else if (precision == ORCA_PRECISION_BF16X2) hipLaunchKernelGGL((conv1d_k9_small_kernel<2, 0>), grid, dim3(512), 0, ctx->stream, a);
    else if (precision == ORCA_PRECISION_F16X2) hipLaunchKernelGGL((conv1d_k9_small_kernel<2, 1>), grid, dim3(512), 0, ctx->stream, a);
    else hipLaunchKernelGGL((conv1d_k9_small_kernel<1, 0>), grid, dim3(512), 0, ctx->stream, a);
    LAUNCHCHECK("conv1d_k9_small_kernel");
    ctx->counts[0]++;
    return ORCA_OK;
  }
  if (precision == ORCA_PRECISION_BF16X3) rc = launch_conv1d_b16_ns<3, 0>(ctx, L, a, B);
  else if (precision == ORCA_PRECISION_BF16X2) rc = launch_conv1d_b16_ns<2, 0>(ctx, L, a, B, fixed_tile == 2 ? 2 : 0);
  else if (precision == ORCA_PRECISION_F16X2) rc = launch_conv1d_b16_ns<2, 1>(ctx, L, a, B, fixed_tile);
  else rc = launch_conv1d_b16_ns<1, 0>(ctx, L, a, B, fixed_tile == 2 ? 2 : 0);
  if (rc != ORCA_OK) return rc;
  LAUNCHCHECK("conv1d_k9_bf16s_kernel");
  ctx->counts[1]++;
  return timer.close(L.cout, L.cin, -precision, B, n, 9);
}

// ---- where a chunk's input comes from, and the kernel argument structs that carry the bases ----------------------------
struct SeqSource {            // a float [.,4] view or packed base codes
  const float* x = nullptr;   // already offset to the chunk start
  long sx_c = 0, sx_l = 0;
  const unsigned char* codes = nullptr;   // whole sequence of this batch row: 1 byte per base, or (nmask set) a 2-bit genome plane + N mask, the
  const unsigned char* nmask = nullptr;   // sequence starting at genome index `origin` (conv_p16.h: p16_base_at)
  long origin = 0;
  long codes_L = 0, codes_off = 0;
  int reverse = 0;
};

static void set_bases(ConvP16Args& a, const SeqSource& s) {
  a.f1_codes = s.codes; a.f1_nmask = s.nmask; a.f1_origin = s.origin; a.f1_codes_L = s.codes_L; a.f1_codes_off = s.codes_off; a.f1_reverse = s.reverse;
}
static void set_bases(FirstMfmaArgs& a, const SeqSource& s) {
  a.codes = s.codes; a.nmask = s.nmask; a.origin = s.origin; a.codes_L = s.codes_L; a.codes_off = s.codes_off; a.reverse = s.reverse;
}
static EdgeFixArgs edge_source(const SeqSource& s) {   // in_mode 1 (bases) or 0 (float rows); also FirstF32Args::in
  EdgeFixArgs a{};
  if (s.codes) { a.in_mode = 1; a.codes = s.codes; a.nmask = s.nmask; a.origin = s.origin; a.codes_L = s.codes_L; a.codes_off = s.codes_off; a.reverse = s.reverse; }
  else { a.in_mode = 0; a.x = s.x; a.sc = s.sx_c; a.sl = s.sx_l; }
  return a;
}

// ---- P16 (planar split fp16) conv1d with LDS-DMA staging (conv_p16.h) -------------------------------------
// (plane lengths: p16_plen in orca_internal.h)
int launch_p16_zero_pads(orca_ctx* ctx, float* base, int C, long n_valid, int fmt, long plen, long gap0, long gap1) {
  if (gap0 < 0 || gap1 < gap0 || gap1 > n_valid || (plen && plen < P16_GUARD + n_valid)) return fail(ORCA_EINVAL, "internal: zero pads outside the planes");
  hipLaunchKernelGGL(p16_zero_pads_kernel, dim3((unsigned)(fmt == 1 ? C / 8 : C / 8 * 2)), dim3(256), 0, ctx->stream, reinterpret_cast<f32x4*>(base),
                     plen ? plen : p16_plen(n_valid), n_valid, gap0, gap1);
  LAUNCHCHECK("p16_zero_pads_kernel");
  return ORCA_OK;
}

static dim3 cu_grid(long ntiles) { const int ncu = device_cus(); return dim3((unsigned)(ntiles < ncu ? ntiles : ncu)); }   // persistent, one workgroup per CU
// one persistent launch of a planar conv kernel on MT-position tiles x cout blocks of CT: CUs x resident workgroups at most
template <auto KERNEL, int MT, int THREADS, int CT>
static void launch_p16_persistent(hipStream_t s, ConvP16Args a) {
  const int resident = resident_workgroups<KERNEL, THREADS>();
  a.tiles_per_row = (a.n + MT - 1) / MT;
  const long ntiles = a.tiles_per_row * (a.cout / CT);
  dim3 grid((unsigned)(ntiles < resident ? ntiles : resident));
  hipLaunchKernelGGL(KERNEL, grid, dim3(THREADS), 0, s, a);
}

// out_mode and the residual are compile-time in the kernel (its epilogue is branch-free)
template <int CT, int MW, int NW, int WM, int OM, bool R1, int FMT = 0>
static void launch_p16_k(hipStream_t s, const ConvP16Args& a) {
  launch_p16_persistent<conv1d_k9_p16_kernel<CT, MW, NW, WM, OM, R1, 0, false, FMT>, WM * MW * 32, WM * 64, CT>(s, a);
}
// the conv that follows the first layer, with the first layer fused into its input-tile producer (conv_p16.h, F1)
static void launch_p16_fused_first(hipStream_t s, const ConvP16Args& a) {
  launch_p16_persistent<conv1d_k9_p16_kernel<64, 2, 2, 8, 0, false, 0, true>, 512, 512, 64>(s, a);
}
// stage 1's pooled conv on P16 planes with the residual computed from the bases in its epilogue (conv_p16.h, RL)
static void launch_p16_res_bases(hipStream_t s, const ConvP16Args& a) {
  launch_p16_persistent<conv1d_k9_p16_kernel<64, 2, 2, 8, 1, false, 0, false, 0, true>, 512, 512, 64>(s, a);
}

// the 96-cout layers of B16 planes on 512-position tiles with ONE half-by-half refilled weight buffer (conv_p16w1.h)
template <int OM, bool R1>
static void launch_p16w1_k(hipStream_t s, ConvP16Args a) {
  a.tiles_per_row = (a.n + 511) / 512;
  hipLaunchKernelGGL((conv1d_k9_p16w1_kernel<OM, R1, 1>), cu_grid(a.tiles_per_row), dim3(512), 0, s, a);
}
// the same layers of P16 planes on the 16 x 16 x 32 matrix instruction (conv_p16x.h)
template <int OM, bool R1, int CT>
static void launch_p16x_k(hipStream_t s, ConvP16Args a) {
  a.tiles_per_row = (a.n + 511) / 512;
  hipLaunchKernelGGL((conv1d_k9_p16x_kernel<OM, R1, CT / 32, CT>), cu_grid(a.tiles_per_row * (a.cout / CT)), dim3(1024), 0, s, a);
}
static bool launch_p16x(hipStream_t s, const ConvP16Args& a) {      // false: this (cout, out_mode, residual) combination stays on the 32 x 32 x 16 kernels
  const bool r1 = a.r1 != nullptr;
  if (a.cout != 96) return false;
  if (a.out_mode == 0 && !r1) launch_p16x_k<0, false, 96>(s, a);
  else if (a.out_mode == 1 && r1) launch_p16x_k<1, true, 96>(s, a);
  else return false;
  return true;
}
static bool launch_p16w1(hipStream_t s, const ConvP16Args& a) {     // false: this (out_mode, residual) pair stays on the 256-position kernel
  const bool r1 = a.r1 != nullptr;
  if (a.out_mode == 0 && !r1) launch_p16w1_k<0, false>(s, a);
  else if (a.out_mode == 1 && r1) launch_p16w1_k<1, true>(s, a);
  else return false;
  return true;
}

// a 128-cout layer with ReLU, residual and MaxPool1d(5) fused (conv_p16p5.h): out_mode 3
template <int FMT>
static void launch_p16p5(hipStream_t s, ConvP16Args a) {
  a.tiles_per_row = (a.n + 319) / 320;
  const dim3 grid = cu_grid(a.tiles_per_row);
  if (a.r1) hipLaunchKernelGGL((conv1d_k9_p16p5_kernel<true, FMT>), grid, dim3(512), 0, s, a);
  else hipLaunchKernelGGL((conv1d_k9_p16p5_kernel<false, FMT>), grid, dim3(512), 0, s, a);
}

// W-stationary barrier-free form (conv_ws.h): persistent, one workgroup per CU; the grid is a multiple of the number
// of cout blocks (of 8 x that where possible: the blocks of one position range then share an XCD)
template <int FMT, int CIN, int CT, int MW, int NW, int OM, bool R1>
static void launch_ws_k(hipStream_t s, const ConvP16Args& a) {
  const int ncu = device_cus();
  const int ncb = a.cout / CT;
  int grid = (ncu / (8 * ncb)) * (8 * ncb);
  if (grid < ncu - 8) grid = (ncu / ncb) * ncb;
  const long ntw = (a.n + MW * 32 - 1) / (MW * 32);
  const long need = ((ntw + 7) / 8) * ncb;            // workgroups that get at least one wave tile
  if (need < grid) grid = (int)(((need + 8 * ncb - 1) / (8 * ncb)) * (8 * ncb));
  hipLaunchKernelGGL((conv1d_k9_ws_kernel<FMT, CIN, CT, MW, NW, OM, R1>), dim3((unsigned)grid), dim3(512), 0, s, a);
}
template <int FMT, int CIN, int CT, int MW, int NW>
static void launch_ws_t(hipStream_t s, const ConvP16Args& a) {
  const bool r1 = a.r1 != nullptr;
  switch (a.out_mode * 2 + (r1 ? 1 : 0)) {
    case 0: launch_ws_k<FMT, CIN, CT, MW, NW, 0, false>(s, a); break;
    case 1: launch_ws_k<FMT, CIN, CT, MW, NW, 0, true>(s, a); break;
    case 2: launch_ws_k<FMT, CIN, CT, MW, NW, 1, false>(s, a); break;
    case 3: launch_ws_k<FMT, CIN, CT, MW, NW, 1, true>(s, a); break;
    case 4: launch_ws_k<FMT, CIN, CT, MW, NW, 2, false>(s, a); break;
    default: launch_ws_k<FMT, CIN, CT, MW, NW, 2, true>(s, a); break;
  }
}

template <int CT, int MW, int NW, int WM, int FMT = 0>
static void launch_p16_t(hipStream_t s, const ConvP16Args& a) {
  const bool r1 = a.r1 != nullptr;
  switch (a.out_mode * 2 + (r1 ? 1 : 0)) {
    case 0: launch_p16_k<CT, MW, NW, WM, 0, false, FMT>(s, a); break;
    case 1: launch_p16_k<CT, MW, NW, WM, 0, true, FMT>(s, a); break;
    case 2: launch_p16_k<CT, MW, NW, WM, 1, false, FMT>(s, a); break;
    case 3: launch_p16_k<CT, MW, NW, WM, 1, true, FMT>(s, a); break;
    case 4: launch_p16_k<CT, MW, NW, WM, 2, false, FMT>(s, a); break;
    default: launch_p16_k<CT, MW, NW, WM, 2, true, FMT>(s, a); break;
  }
}

// x: P16 [cin] of n positions; y: P16 (out_mode 0: n positions, 1: n/4 pooled) or fp32 [n][cout] (2); r1: P16 [cout], n
struct FusedFirst {   // packed bases + first-layer table: the conv's input is produced instead of read (x may be NULL)
  const SeqSource* src = nullptr;
  const float* table = nullptr;
  const float* bias = nullptr;
  bool residual = false;   // RL form instead: x IS read; the bases + the 17-tap pack (in `table`) give the residual in the epilogue
};

// fmt 0: P16 activations (fp32-class f16x2 arithmetic); fmt 1: B16 activations (plain bf16, BASELINE config 3)
int launch_conv1d_p16(orca_ctx* ctx, const ConvLayer& L, const float* x, void* y, const float* r1, long n, int relu,
                             int out_mode, const FusedFirst* f1, int fmt, const P16Layout* lay) {
  const bool k17 = L.ksize == 17;
  if ((L.ksize != 9 && !k17) || (fmt == 0 ? !L.d_wf16 : !L.d_wb16p)) return fail(ORCA_EINVAL, "layer has no %s pack", fmt == 0 ? "fp16 split" : "bf16");
  if (fmt == 0 && !L.f16_ok) return fail(ORCA_EINVAL, "layer weights exceed the fp16 range: use ORCA_PRECISION_BF16X3");
  if (n <= 0) return ORCA_OK;
  ctx->counts[2]++;
  ConvP16Args a;
  a.x = reinterpret_cast<const f32x4*>(x); a.w = reinterpret_cast<const f32x4*>(fmt == 0 ? L.d_wf16 : L.d_wb16p); a.bias = L.d_bias; a.y = y;
  a.r1 = reinterpret_cast<const f32x4*>(r1); a.x_plen = p16_plen(n); a.y_plen = p16_plen(out_mode == 1 ? n / 4 : out_mode == 3 ? n / 5 : n); a.n = n;
  long n_rec = n;
  if (lay) {
    if (f1 || (lay->y_off && out_mode == 2)) return fail(ORCA_EINVAL, "internal: an explicit plane layout on a conv from the bases / an offset into fp32 rows");
    if (lay->x_plen) a.x_plen = lay->x_plen;
    if (lay->y_plen) a.y_plen = lay->y_plen;
    a.y = static_cast<f32x4*>(y) + lay->y_off;
    if (lay->n_valid) n_rec = lay->n_valid;
  }
  a.nchunks = (fmt == 0 ? L.cin / 16 : L.cin / 32) * (k17 ? 2 : 1); a.cout = L.cout; a.relu = relu; a.out_mode = out_mode; a.flag = ctx->d_flag;
  a.k17 = k17 ? 1 : 0;
  LaunchTimer timer(ctx, n);
  ORCA_TRY(timer.open());
  set_bases(a, f1 ? *f1->src : SeqSource());
  a.f1_table = a.f1_bias = nullptr; a.stamps = nullptr; a.rl_w = nullptr;
  int tile_tag = fmt == 1 ? -6 : -5;
  if (f1 && f1->residual) {
    if (L.cout != 64 || L.cin != 64 || out_mode != 1 || r1 || k17) return fail(ORCA_EINVAL, "residual from the bases: only stage 1's pooled 64 -> 64 planar conv");
    a.rl_w = reinterpret_cast<const f32x4*>(f1->table); a.f1_bias = f1->bias;
    if (fmt == 1) return fail(ORCA_EINVAL, "residual from the bases on B16 planes: the stage runs as ONE kernel (conv_stage1.h)");
    launch_p16_res_bases(ctx->stream, a);
  } else if (f1) {
    if (L.cout != 64 || L.cin != 64 || out_mode != 0 || r1 || fmt != 0 || k17) return fail(ORCA_EINVAL, "fused first layer: only the 64 -> 64 P16 conv that follows it");
    a.f1_table = f1->table; a.f1_bias = f1->bias;
    launch_p16_fused_first(ctx->stream, a);
  } else if (fmt == 1 && !k17 && L.cin == 64 && L.cout == 64) {
    // W-stationary barrier-free kernel (conv_ws.h; P16: measured 3 % slower than the tiled kernel - profiles/HISTORY.md)
    launch_ws_t<1, 64, 64, 2, 2>(ctx->stream, a);
    tile_tag = -8;
  } else if (out_mode == 3) {
    if (k17 || L.cout != 128) return fail(ORCA_EINVAL, "fused MaxPool1d(5): only the 128-cout k9 conv (conv_p16p5.h)");
    if (fmt == 1) launch_p16p5<1>(ctx->stream, a); else launch_p16p5<0>(ctx->stream, a);
    tile_tag = fmt == 1 ? -13 : -12;
  } else if (L.cout == 96 && n >= 65536 && fmt == 0 && launch_p16x(ctx->stream, a)) {
    tile_tag = -14;                      // stage 2 of the Encoder on P16 planes: 16 x 16 x 32 matrix instruction (conv_p16x.h)
  } else if (L.cout == 96 && n >= 65536 && fmt == 1 && launch_p16w1(ctx->stream, a)) {
    tile_tag = -10;                      // ... on B16 planes: 512-position tiles, one half-by-half refilled weight buffer (conv_p16w1.h)
  } else if (L.cout == 96) {
    if (fmt == 1) launch_p16_t<96, 1, 3, 8, 1>(ctx->stream, a); else launch_p16_t<96, 1, 3, 8>(ctx->stream, a);
  } else if (L.cout % 64 == 0) {
    if (fmt == 1) launch_p16_t<64, 2, 2, 8, 1>(ctx->stream, a); else launch_p16_t<64, 2, 2, 8>(ctx->stream, a);
  } else {
    return fail(ORCA_EINVAL, "%s conv1d cout %d unsupported", fmt == 1 ? "b16" : "p16", L.cout);
  }
  LAUNCHCHECK("conv1d_k9_p16_kernel");
  return timer.close(L.cout, L.cin, tile_tag, 1, n_rec, k17 ? 17 : 9);
}

// one first-layer GEMM launch from the bases / flat [n][4] float rows onto planes (fmt 0 P16, 1 B16): ntap 9 (lconv1.a alone), 17 (lconv1 composed),
// 25 (conv1.a o lconv1, + ReLU)
static int launch_first_mfma(orca_ctx* ctx, const SeqSource& src, const float* rows, long n, int ntap, const void* w16, const float* bias, int relu,
                             float* out, int fmt) {
  hipStream_t s = ctx->stream;
  FirstMfmaArgs fm;
  set_bases(fm, src);
  fm.x = src.codes ? nullptr : rows; fm.n = n;
  fm.w = reinterpret_cast<const f32x4*>(w16); fm.bias = bias; fm.relu = relu;
  fm.y = reinterpret_cast<f32x4*>(out); fm.y_plen = p16_plen(n); fm.flag = ctx->d_flag;
  const long nt = (n + 255) / 256;
  const dim3 grid((unsigned)(nt < 2048 ? nt : 2048));
  LaunchTimer timer(ctx, n, ntap > 9);
  ORCA_TRY(timer.open());
  switch (ntap * 2 + fmt) {
    case 18: hipLaunchKernelGGL((conv1d_first_mfma_p16_kernel<0, 0, 9>), grid, dim3(256), 0, s, fm); break;
    case 19: hipLaunchKernelGGL((conv1d_first_mfma_p16_kernel<0, 1, 9>), grid, dim3(256), 0, s, fm); break;
    case 34: hipLaunchKernelGGL((conv1d_first_mfma_p16_kernel<0, 0, 17>), grid, dim3(256), 0, s, fm); break;
    case 35: hipLaunchKernelGGL((conv1d_first_mfma_p16_kernel<0, 1, 17>), grid, dim3(256), 0, s, fm); break;
    case 50: hipLaunchKernelGGL((conv1d_first_mfma_p16_kernel<0, 0, 25>), grid, dim3(256), 0, s, fm); break;
    default: hipLaunchKernelGGL((conv1d_first_mfma_p16_kernel<0, 1, 25>), grid, dim3(256), 0, s, fm); break;
  }
  LAUNCHCHECK("conv1d_first_mfma_p16_kernel");
  return timer.close(64, 4, fmt == 1 ? -6 : -5, 1, n, ntap);
}

// stage 1 of the throughput mode (B16 planes) as ONE kernel from the bases (conv_stage1.h): conv1.b's input tiles are produced in LDS by the matrix
// cores, a1 is neither written nor re-read; `a1_edge` holds the edge-fixed a1 at its first / last 8 positions, y receives the pooled stage output
static int launch_stage1_b16(orca_ctx* ctx, const orca_net* net, const ConvLayer& Lb, const SeqSource& src, const float* a1_edge, float* y, long n) {
  Stage1Args sa;
  ConvP16Args& a1 = sa.c;
  a1.x = nullptr; a1.w = reinterpret_cast<const f32x4*>(Lb.d_wb16p); a1.bias = Lb.d_bias; a1.y = y; a1.r1 = nullptr;
  a1.x_plen = p16_plen(n); a1.y_plen = p16_plen(n / 4); a1.n = n; a1.tiles_per_row = (n + 63) / 64; a1.nchunks = 2; a1.cout = 64;
  a1.relu = 1; a1.out_mode = 1; a1.k17 = 0; a1.flag = ctx->d_flag; a1.stamps = nullptr;
  set_bases(a1, src);
  a1.rl_w = reinterpret_cast<const f32x4*>(net->d_l1_w16); a1.f1_table = nullptr; a1.f1_bias = net->d_l1_bias;
  sa.w25 = reinterpret_cast<const f32x4*>(net->d_c1a_w16); sa.b25 = net->d_c1a_bias;
  sa.a1_edge = reinterpret_cast<const f32x4*>(a1_edge); sa.a1_plen = p16_plen(n);
  LaunchTimer timer(ctx, n);
  ORCA_TRY(timer.open());
  hipLaunchKernelGGL((conv1d_stage1_b16_kernel<1>), cu_grid(((n + 63) / 64 + 7) / 8), dim3(512), 0, ctx->stream, sa);
  LAUNCHCHECK("conv1d_stage1_b16_kernel");
  ctx->counts[2]++;
  // (both 64 -> 64 convs of the stage in one launch: recorded as cin = 128 so that 2 * 9 * cin * cout is the pair's algorithmic work)
  return timer.close(64, 128, -15, 1, n, 9);
}

// the end positions of a stage's composed linear group, recomputed conv by conv (conv_p16.h: lconv_edge_layer_kernel): its first `depth` (2-4) layers
// Ls[0 ..], ReLU behind the third and the fourth.  The last layer covers `half_last` positions per end, layer l four more per layer behind it; the
// outermost 4 per end of lout (layer 2) go to `lo`, the outermost 8 of layer 3 to `t`, where given.  fmt 0 / 1: planes, 2: fp32 channel-major with row
// stride ld_f32, 3: fp32 channel-last.  Scratch: one 40 x 128 float slab per layer in the context.  y_plen: plane length of lo / t where it is not
// p16_plen(n) (a sequence inside longer planes: src.xp, lo, t point at ITS first unit)
static int launch_edge_chain(orca_ctx* ctx, const ConvLayer* Ls, int depth, int half_last, EdgeFixArgs src, long n, float* lo, float* t, int fmt,
                             long ld_f32 = 0, long y_plen = 0) {
  src.n = n;
  if (depth > 4 || 2 * (half_last + 4 * (depth - 1)) > 40) return fail(ORCA_EINVAL, "edge fix: chain too deep");
  for (int l = 0; l < depth; ++l) {
    const ConvLayer& L = Ls[l];
    if (!L.d_w) return fail(ORCA_EINVAL, "edge fix: layer without an fp32 pack");
    EdgeLayerArgs a{};
    a.in = src;
    if (l > 0) a.in.in_mode = -1;
    a.half = half_last + 4 * (depth - 1 - l); a.half_in = a.half + 4;
    a.relu = l >= 2; a.cin = L.cin; a.cout = L.cout; a.kc = L.kc; a.w = L.d_w; a.b = L.d_bias;
    a.sin = l > 0 ? ctx->d_edge + (l - 1) * ORCA_EDGE_SLAB : nullptr;
    a.sout = ctx->d_edge + l * ORCA_EDGE_SLAB;
    float* const y = l == 1 ? lo : l == 2 ? t : nullptr;
    a.y = reinterpret_cast<f32x4*>(y); a.y_plen = fmt == 2 ? ld_f32 : y_plen ? y_plen : p16_plen(n); a.out_fmt = fmt; a.flag = ctx->d_flag;
    a.store_half = !y ? 0 : l == 1 ? 4 : 8;
    hipLaunchKernelGGL(lconv_edge_layer_kernel, dim3((unsigned)(2 * a.half)), dim3(512), 0, ctx->stream, a);
  }
  LAUNCHCHECK("lconv_edge_layer_kernel");
  return ORCA_OK;
}

static int launch_pool_nlc(orca_ctx* ctx, const float* x, float* y, long n_out, int C, int k) {
  if (n_out <= 0) return ORCA_OK;
  if (C % 4 || C / 4 > 256) return fail(ORCA_EINVAL, "maxpool (channel-last): %d channels unsupported", C);
  const long per_block = 2 * (256 / (C / 4));
  dim3 grid((unsigned)((n_out + per_block - 1) / per_block));
  switch (k) {
    case 2: hipLaunchKernelGGL((maxpool1d_nlc_kernel<2>), grid, dim3(256), 0, ctx->stream, x, y, n_out, C); break;
    case 4: hipLaunchKernelGGL((maxpool1d_nlc_kernel<4>), grid, dim3(256), 0, ctx->stream, x, y, n_out, C); break;
    case 5: hipLaunchKernelGGL((maxpool1d_nlc_kernel<5>), grid, dim3(256), 0, ctx->stream, x, y, n_out, C); break;
    default: return fail(ORCA_EINVAL, "maxpool k=%d unsupported", k);
  }
  LAUNCHCHECK("maxpool1d_nlc_kernel");
  return ORCA_OK;
}

static int launch_copy2d(orca_ctx* ctx, const float* src, long lds_, long scol, float* dst, long ldd, long rows, long cols) {
  if (rows <= 0 || cols <= 0) return ORCA_OK;
  dim3 grid((unsigned)((cols + 255) / 256), (unsigned)rows);
  hipLaunchKernelGGL(copy2d_kernel, grid, dim3(256), 0, ctx->stream, src, lds_, scol, dst, ldd, cols);
  LAUNCHCHECK("copy2d_kernel");
  return ORCA_OK;
}

// the same with the rows out of gridDim.y (<= 65 535): a position-strided input of any length
static int launch_copy2d_flat(orca_ctx* ctx, const float* src, long lds_, long scol, float* dst, long ldd, long rows, long cols) {
  if (rows <= 0 || cols <= 0) return ORCA_OK;
  hipLaunchKernelGGL(copy2d_flat_kernel, dim3((unsigned)((rows * cols + 255) / 256)), dim3(256), 0, ctx->stream, src, lds_, scol, dst, ldd, rows, cols);
  LAUNCHCHECK("copy2d_flat_kernel");
  return ORCA_OK;
}

// ---------------------------------------------------------------------------
// Encoder (orca_modules.py:929-980)
// ---------------------------------------------------------------------------
static const int kEncPools[7] = {1, 4, 4, 5, 5, 5, 2};
static const long kHaloBp = 112000;  // x_padding, orca_modules.py:932
static const long kBinBp = 4000;

extern "C" int64_t orca_encoder_num_bins(int64_t L) {
  long n = L;
  for (int i = 1; i < 7; ++i) n /= kEncPools[i];
  return n;
}

// `part` (P16 planes only, SV screens off the 4 kb grid - orca_encoder_stage3_planes and friends below): the FRONT of the Encoder is stages 1-3
// (99 % of its FLOPs; translation-covariant on a 16-base grid with a reach of 351 bases), the BACK stages 4-7 from the MaxPool1d(5)'d stage-3 output
// (stage 4 - 1.2 of the back's 2.0 ms per window - moves into the cache too: ENC_STAGE4 runs it alone on a stage-4 input and hands its fp32 rows over,
// ENC_FRONT4 = the front + stage 4 for the snippets, ENC_BACK5 = stages 5-7 from the MaxPool1d(5)'d rows: covariant on an 80-base grid, reach 1 631 bases)
enum { ENC_FULL = 0, ENC_FRONT_POOLED = 1, ENC_FRONT_UNPOOLED = 2, ENC_BACK = 3, ENC_STAGE4 = 4, ENC_FRONT4 = 5, ENC_BACK5 = 6 };

// The route of one chunk, decided once (enc_route): the pipeline of its arithmetic mode, the form of stage 1, and its part as data.
//   PIPE_P16 (f16x2) / PIPE_B16 (bf16): stages 1-4 on planar 16-bit activations with LDS-DMA staging (conv_p16.h; 2-way split fp16, fp32-class / one
//     bf16 plane, the throughput mode of BASELINE config 3), stages 5-7 channel-last;  PIPE_NLC (bf16x2 / bf16x3): every stage on the channel-last
//     split-operand kernels (conv_bf16s.h);  PIPE_F32: the exact fp32 kernels on channel-major rows
enum { PIPE_P16, PIPE_B16, PIPE_NLC, PIPE_F32 };
enum { OUT_BINS, OUT_PLANES, OUT_PLANES_POOLED, OUT_ROWS };   // the last stage's output: bins [n][128] | planes, every position | planes, MaxPool1d(5)'d | fp32 rows [n][128] before the pool
struct EncRoute {
  int pipe = PIPE_F32;
  int fmt = 0;                 // planar pipelines: 0 P16, 1 B16
  int first = 0, last = 6;     // stages run (0-based); a first stage > 0 reads its already pooled input from buf[0]
  int out = OUT_BINS;
  // planar pipelines.  Composed linear pairs (default; ORCA_ENCODER_FORM_TWO_CONV = the reference's layer sequence - also what a group whose composed
  // weights leave the fp16 range falls back to): lconv1 is ONE 17-tap first layer (K = 68 MFMA GEMM from the bases / float rows), lconv2 / lconv3 are
  // 17-tap planar convs.  The end positions of each group are redone exactly by the edge-fix chain (lconv_edge_layer_kernel).
  bool compose = false;
  bool compose25 = false;      // conv1.a, linear up to its ReLU, joins the group (25 taps from the bases + ReLU, K = 112); _FORM_LCONV1_ONLY keeps it a 64 -> 64 launch
  bool res_from_bases = false; // ... and with packed bases the residual lout1 is computed inside conv1.b's epilogue (conv_p16.h, RL) instead of being stored
                               // by a 17-tap first-layer launch and re-read (float rows, _FORM_STORED_RESIDUAL: the stored form)
  bool stage1_fused = false;   // ... and on B16 planes the whole stage is then ONE kernel from the bases (conv_stage1.h)
  bool fuse1 = false;          // two-conv form from packed input: the first layer is fused into the input-tile producer of the conv that follows it (conv_p16.h, F1)
  // channel-last pipeline: stage 1 composed - from PACKED bases only: the first-layer GEMM splits its X operand into fp16 parts, exact for
  // 0 / 0.25 / 1, while these modes promise fp32 range for arbitrary float rows
  bool compose_nlc = false;
  // two strands of one sequence (encoder_two_strands).  Their stages 1-2 run per strand and hand over to ONE set of planes: the last stage's pooled
  // output goes to units [pooled_off, ..) of the planes `pooled_to` of pooled_plen units instead of buf[kS], whose pads are then the caller's.
  // Stages 3-7 run once on both: `seam` > 0 = the input holds two sequences of *n positions each, the second `seam` positions behind the first
  // (zeros in between; a multiple of 250, so that every later pool keeps the second on a window boundary)
  float* pooled_to = nullptr;
  long pooled_plen = 0, pooled_off = 0;
  long seam = 0;
  bool compose32 = false;      // exact-fp32 mode: stage 1's linear groups composed as in the 16-bit modes (conv_p16.h: first_taps_f32_kernel reads the source directly)
  bool planar() const { return pipe == PIPE_P16 || pipe == PIPE_B16; }
};

static int enc_route(const orca_net* net, const SeqSource& src, int part, EncRoute* route) {
  static const struct { int first, last, out; } kParts[7] = {
      {0, 6, OUT_BINS}, {0, 2, OUT_PLANES_POOLED}, {0, 2, OUT_PLANES}, {3, 6, OUT_BINS}, {3, 3, OUT_ROWS}, {0, 3, OUT_ROWS}, {4, 6, OUT_BINS}};
  EncRoute r;
  const int prec = net->precision, form = net->enc_form;
  r.pipe = prec == ORCA_PRECISION_F16X2 ? PIPE_P16 : prec == ORCA_PRECISION_BF16 ? PIPE_B16 : prec == ORCA_PRECISION_F32 ? PIPE_F32 : PIPE_NLC;
  if (part != ENC_FULL && r.pipe != PIPE_P16) return fail(ORCA_EINVAL, "the Encoder's front / back parts exist in the f16x2 arithmetic (P16 planes) only");
  r.first = kParts[part].first; r.last = kParts[part].last; r.out = kParts[part].out;
  if (r.planar()) {
    r.fmt = r.pipe == PIPE_B16 ? 1 : 0;
    r.compose = form < ORCA_ENCODER_FORM_TWO_CONV && net->d_l1_w16 != nullptr;
    r.compose25 = r.compose && form < ORCA_ENCODER_FORM_LCONV1_ONLY && net->d_c1a_w16 != nullptr;
    r.res_from_bases = r.compose25 && src.codes && form < ORCA_ENCODER_FORM_STORED_RESIDUAL;
    r.stage1_fused = r.res_from_bases && r.fmt == 1;
    r.fuse1 = src.codes && r.fmt == 0 && !r.compose;
  }
  r.compose_nlc = r.pipe == PIPE_NLC && net->d_c1a_w16 && form < ORCA_ENCODER_FORM_LCONV1_ONLY && src.codes;
  r.compose32 = r.pipe == PIPE_F32 && net->d_l1_f32 && form < ORCA_ENCODER_FORM_LCONV1_ONLY;
  *route = r;
  return ORCA_OK;
}

// buffer roles of the planar stages: S holds a stage's (pooled) input and receives its output, T the current conv's input, LO the stage's lout.
// (guards and tails of every planar tensor are zeroed by p16_zero_pads_kernel AFTER its producer: the conv kernels write the units of a ragged
// last tile unmasked.)  The channel-last and fp32 stages rotate: the input in buf[P], T = P + 1, LO = P + 2 (mod 3), the output back in buf[P]
enum { kS = 0, kT = 1, kLO = 2 };
static const int kPlanarStages = 4;   // stages on the planar kernels (pools 4, 4, 5 fused into the conv in front of them)

// stage 1 on planes, the first-layer launches: lout1 into buf[kLO] (composed; not with res_from_bases, which never stores it) and / or the input of
// the stage's next conv into buf[kT] (the first layer's output, or conv1.a's from the 25-tap group; not with stage1_fused)
static int enc_stage1_first_layers(orca_ctx* ctx, const orca_net* net, const SeqSource& src, const EncRoute& r, long n, float* const buf[3]) {
  hipStream_t s = ctx->stream;
  const ConvLayer* L = net->convs.data();
  const bool flat = src.codes || (src.sx_c == 1 && src.sx_l == 4 && al16(src.x));
  if (r.compose || flat || r.fmt == 1) {
    const float* rows = src.x;     // flat [n][4] float rows for the MFMA first-layer kernels (unused with packed input)
    if (!flat) {
      // strided float rows: gather them into a flat [n][4] copy (buf[kS] is free until the stage's last conv), then the MFMA kernel
      hipLaunchKernelGGL(seq_to_rows_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, src.x, src.sx_c, src.sx_l, n, buf[kS]);
      LAUNCHCHECK("seq_to_rows_kernel");
      rows = buf[kS];
    }
    if (r.res_from_bases) { /* no lout1 tensor */ }
    else if (r.compose) ORCA_TRY(launch_first_mfma(ctx, src, rows, n, 17, net->d_l1_w16, net->d_l1_bias, 0, buf[kLO], r.fmt));
    else ORCA_TRY(launch_first_mfma(ctx, src, rows, n, 9, net->d_first_w16, L[0].d_bias, 0, buf[kT], r.fmt));
    if (r.compose25 && !r.stage1_fused) {
      ORCA_TRY(launch_first_mfma(ctx, src, rows, n, 25, net->d_c1a_w16, net->d_c1a_bias, 1, buf[kT], r.fmt));
      ORCA_TRY(launch_p16_zero_pads(ctx, buf[kT], 64, n, r.fmt));
    }
  } else {      // strided float rows, two-conv form on P16 planes: the fp32 first layer
    FirstP16Args fa;
    fa.x = src.x; fa.sc = src.sx_c; fa.sl = src.sx_l; fa.n = n; fa.w = net->d_first_w; fa.bias = L[0].d_bias; fa.y = reinterpret_cast<f32x4*>(buf[kT]);
    fa.y_plen = p16_plen(n); fa.flag = ctx->d_flag;
    hipLaunchKernelGGL(conv1d_first_p16_kernel, dim3((unsigned)((n + 255) / 256), 8), dim3(256), 0, s, fa);
    LAUNCHCHECK("conv1d_first_p16_kernel");
  }
  if (!r.res_from_bases) ORCA_TRY(launch_p16_zero_pads(ctx, r.compose ? buf[kLO] : buf[kT], 64, n, r.fmt));
  return ORCA_OK;
}

// stage 1's last conv with the residual from the bases: relu(conv1.b) + lout1 computed in the epilogue, MaxPool1d(4); the pooled windows at the
// ends from the edge chain's exact conv1.b (slab 3) and lout1 (slab 1)
static int enc_stage1_last_from_bases(orca_ctx* ctx, const orca_net* net, const SeqSource& src, const EncRoute& r, long n, float* const buf[3]) {
  const ConvLayer& Lb = net->convs[3];
  if (r.stage1_fused) {
    ORCA_TRY(launch_stage1_b16(ctx, net, Lb, src, buf[kT], buf[kS], n));
  } else {
    FusedFirst rl;
    rl.src = &src; rl.table = reinterpret_cast<const float*>(net->d_l1_w16); rl.bias = net->d_l1_bias; rl.residual = true;
    ORCA_TRY(launch_conv1d_p16(ctx, Lb, buf[kT], buf[kS], nullptr, n, 1, 1, &rl, r.fmt));
  }
  ORCA_TRY(launch_p16_zero_pads(ctx, buf[kS], Lb.cout, n / 4, r.fmt));
  EdgePoolArgs ep{};
  ep.sc = ctx->d_edge + 3 * ORCA_EDGE_SLAB; ep.half_c = 8; ep.sl = ctx->d_edge + 1 * ORCA_EDGE_SLAB; ep.half_l = 16; ep.n = n; ep.cout = Lb.cout;
  ep.y = reinterpret_cast<f32x4*>(buf[kS]); ep.y_plen = p16_plen(n / 4); ep.out_fmt = r.fmt; ep.flag = ctx->d_flag;
  if (n / 4 > 0) hipLaunchKernelGGL(lconv_edge_pool_kernel, dim3(3), dim3(128), 0, ctx->stream, ep);
  LAUNCHCHECK("lconv_edge_pool_kernel");
  return ORCA_OK;
}

// stage 1 on planes: the source -> its MaxPool1d(4)'d output in buf[kS] (*n positions in, *n / 4 out).  Five variants (EncRoute): two convs with the
// first layer fused into the second (fuse1) or stored; lconv1 composed; conv1.a composed too, the residual stored; the residual from the bases, as
// one kernel on B16 planes
static int enc_stage1_planes(orca_ctx* ctx, const orca_net* net, const SeqSource& src, const EncRoute& r, float* const buf[3], long* n_io) {
  const ConvLayer* L = net->convs.data();
  const long n = *n_io;
  const int fmt = r.fmt, C = L[3].cout;
  if (!r.fuse1) ORCA_TRY(enc_stage1_first_layers(ctx, net, src, r, n, buf));    // (fuse1: the first layer's output is never materialised)
  if (r.compose) {
    const EdgeFixArgs ef = edge_source(src);
    // (res_from_bases: lout1 is never stored; conv1.b's own end positions are needed for the pooled windows)
    if (r.res_from_bases) ORCA_TRY(launch_edge_chain(ctx, L, 4, 8, ef, n, nullptr, buf[kT], fmt));
    else if (r.compose25) ORCA_TRY(launch_edge_chain(ctx, L, 3, 8, ef, n, buf[kLO], buf[kT], fmt));
    else ORCA_TRY(launch_edge_chain(ctx, L, 2, 4, ef, n, buf[kLO], nullptr, fmt));
  } else {
    FusedFirst f1;
    f1.src = &src; f1.table = net->d_first_tab; f1.bias = L[0].d_bias;
    ORCA_TRY(launch_conv1d_p16(ctx, L[1], buf[kT], buf[kLO], nullptr, n, 0, 0, r.fuse1 ? &f1 : nullptr, fmt));   // lout
    ORCA_TRY(launch_p16_zero_pads(ctx, buf[kLO], C, n, fmt));
  }
  if (!r.compose25) {     // (composed: conv1.a's output is already in buf[kT], straight from the bases)
    ORCA_TRY(launch_conv1d_p16(ctx, L[2], buf[kLO], buf[kT], nullptr, n, 1, 0, nullptr, fmt));
    ORCA_TRY(launch_p16_zero_pads(ctx, buf[kT], C, n, fmt));
  }
  if (r.res_from_bases) {
    ORCA_TRY(enc_stage1_last_from_bases(ctx, net, src, r, n, buf));
  } else {
    ORCA_TRY(launch_conv1d_p16(ctx, L[3], buf[kT], buf[kS], buf[kLO], n, 1, 1, nullptr, fmt));          // relu(.)+lout, MaxPool1d(4)
    ORCA_TRY(launch_p16_zero_pads(ctx, buf[kS], C, n / 4, fmt));
  }
  *n_io = n / 4;
  return ORCA_OK;
}

// the planar stages behind stage 1 (2 .. 4, from r.first, up to r.last): buf[kS] with *n positions -> buf[kS].  The pool behind a stage is fused into
// its last conv (conv_p16.h: MaxPool1d(4), conv_p16p5.h: MaxPool1d(5)) unless the route hands the planes over unpooled; stage 4 hands over fp32 rows
static int enc_planar_stages(orca_ctx* ctx, const orca_net* net, const EncRoute& r, float* const buf[3], long* n_io) {
  const int fmt = r.fmt;
  float *S = buf[kS], *T = buf[kT], *LO = buf[kLO];
  long n = *n_io, off = r.seam;      // positions of one sequence; joint tensors: the second sequence's first position
  for (int st = r.first > 1 ? r.first : 1; st < kPlanarStages && st <= r.last; ++st) {
    const ConvLayer* Ls = &net->convs[4 * st];
    const int C = Ls[3].cout;
    // joint tensors: nt positions, the gap [n, off) among them, in planes with room for a pooled producer's ragged last tile behind ANY position
    const long nt = off + n;
    const auto plen = [&](long pos) { return r.seam ? p16_plen(pos + 128) : p16_plen(pos); };
    const auto conv = [&](const ConvLayer& L, const float* x, void* y, const float* r1, int relu, int out_mode, long n_out) {
      const P16Layout lay{plen(nt), plen(n_out), 0, 2 * n};
      return launch_conv1d_p16(ctx, L, x, y, r1, nt, relu, out_mode, nullptr, fmt, r.seam ? &lay : nullptr);
    };
    const auto pads = [&](float* base, long n1, long off1) {      // guards, tail and the gap of a tensor of n1 positions per sequence
      return r.seam ? launch_p16_zero_pads(ctx, base, C, off1 + n1, fmt, plen(off1 + n1), n1, off1) : launch_p16_zero_pads(ctx, base, C, n1, fmt);
    };
    // the stage's linear pair: (pooled) previous output S -> lout in LO
    if (r.compose && st <= 2 && net->comp[st].d_wf16) {
      ORCA_TRY(conv(net->comp[st], S, LO, nullptr, 0, 0, nt));
      ORCA_TRY(pads(LO, n, off));
      for (int seg = 0; seg < (r.seam ? 2 : 1); ++seg) {          // exact ends of every sequence
        EdgeFixArgs ef{};
        ef.in_mode = fmt == 1 ? 3 : 2; ef.xp = reinterpret_cast<const f32x4*>(S) + seg * off; ef.x_plen = plen(nt);
        ORCA_TRY(launch_edge_chain(ctx, Ls, 2, 4, ef, n, LO + 4 * seg * off, nullptr, fmt, 0, plen(nt)));
      }
    } else {
      ORCA_TRY(conv(Ls[0], S, T, nullptr, 0, 0, nt));
      ORCA_TRY(pads(T, n, off));
      ORCA_TRY(conv(Ls[1], T, LO, nullptr, 0, 0, nt));   // lout
      ORCA_TRY(pads(LO, n, off));
    }
    ORCA_TRY(conv(Ls[2], LO, T, nullptr, 1, 0, nt));
    ORCA_TRY(pads(T, n, off));
    // the last conv: relu(.) + lout
    if (st + 1 == kPlanarStages) {
      ORCA_TRY(conv(Ls[3], T, S, LO, 1, 2, nt));          // fp32 channel-last hand-over
      break;
    }
    const int pool = kEncPools[st + 1];
    if (pool != 4 && (pool != 5 || C != 128)) return fail(ORCA_EINVAL, "internal: planar stage %d followed by an unexpected pool", st + 1);
    if (r.seam && (n % pool || off % pool)) return fail(ORCA_EINVAL, "internal: joint stage %d: %ld positions, seam %ld, pool %d", st + 1, n, off, pool);
    if (st == r.last && r.out == OUT_PLANES) {   // stage 3's output as it is, every position: what a stage-3 cache keeps (the pool is the reader's)
      ORCA_TRY(conv(Ls[3], T, S, LO, 1, 0, nt));
      ORCA_TRY(pads(S, n, off));
      break;
    }
    if (st == r.last && r.pooled_to) {           // into the joint planes of the two-strand route (their pads: encoder_two_strands)
      const P16Layout lay{0, r.pooled_plen, r.pooled_off, 0};
      ORCA_TRY(launch_conv1d_p16(ctx, Ls[3], T, r.pooled_to, LO, n, 1, pool == 4 ? 1 : 3, nullptr, fmt, &lay));
      n /= pool;
      break;
    }
    ORCA_TRY(conv(Ls[3], T, S, LO, 1, pool == 4 ? 1 : 3, nt / pool));   // MaxPool1d(4) / MaxPool1d(5) (conv_p16p5.h)
    ORCA_TRY(pads(S, n / pool, off / pool));
    n /= pool; off /= pool;
  }
  *n_io = n;
  return ORCA_OK;
}

// the pipelines that start from float rows: the source as channel-major [4][ld1] in buf[0] (packed bases are expanded into buf[2] as [n][4] first)
static int enc_rows_channel_major(orca_ctx* ctx, const SeqSource& src, long n1, float* const buf[3], long ld1) {
  const float* x = src.x;
  long sx_c = src.sx_c, sx_l = src.sx_l;
  if (src.codes) {
    hipLaunchKernelGGL(expand_codes_kernel, dim3((unsigned)((n1 + 255) / 256)), dim3(256), 0, ctx->stream, src.codes, src.nmask, src.origin, src.codes_L,
                       src.codes_off, src.reverse, n1, buf[2]);
    LAUNCHCHECK("expand_codes_kernel");
    x = buf[2]; sx_c = 1; sx_l = 4;
  }
  hipLaunchKernelGGL(seq_to_channel_major_kernel, dim3((unsigned)((n1 + 255) / 256)), dim3(256), 0, ctx->stream, x, sx_c, sx_l, n1, buf[0], ld1);
  LAUNCHCHECK("seq_to_channel_major_kernel");
  return ORCA_OK;
}

// stage 1's linear groups of the channel-last pipeline composed (the fallback of the fp16-range guard runs this in bf16x3): lconv1 and
// conv1.a o lconv1 as 17- / 25-tap first-layer GEMMs writing fp32 channel-last, exact ends by the edge chain
static int enc_stage1_groups_nlc(orca_ctx* ctx, const orca_net* net, const SeqSource& src, long n, float* lo, float* t) {
  hipStream_t s = ctx->stream;
  FirstMfmaArgs fm;
  set_bases(fm, src);
  fm.x = src.codes ? nullptr : src.x; fm.n = n; fm.y_plen = 0; fm.flag = nullptr;
  const long nt = (n + 255) / 256;
  const dim3 grid((unsigned)(nt < 2048 ? nt : 2048));
  fm.w = reinterpret_cast<const f32x4*>(net->d_l1_w16); fm.bias = net->d_l1_bias; fm.relu = 0; fm.y = reinterpret_cast<f32x4*>(lo);
  hipLaunchKernelGGL((conv1d_first_mfma_p16_kernel<0, 2, 17>), grid, dim3(256), 0, s, fm);
  fm.w = reinterpret_cast<const f32x4*>(net->d_c1a_w16); fm.bias = net->d_c1a_bias; fm.relu = 1; fm.y = reinterpret_cast<f32x4*>(t);
  hipLaunchKernelGGL((conv1d_first_mfma_p16_kernel<0, 2, 25>), grid, dim3(256), 0, s, fm);
  LAUNCHCHECK("conv1d_first_mfma_p16_kernel");
  return launch_edge_chain(ctx, net->convs.data(), 3, 8, edge_source(src), n, lo, t, 3);
}

// stages `st_from` .. 7 on the channel-last kernels (conv_bf16s.h / conv_small.h): every stage of the channel-last pipeline, stages 5-7 of the planar
// ones (buf[0] holds stage 4's fp32 rows, or - first stage 5 - the already pooled rows of the caller).  Two strands (r.seam, stages 5-7): buf[0]
// holds both, the second r.seam / 5 rows behind the first; stage 5's pool packs them into a batch of two rows that every conv then runs in ONE
// launch, each row zero-padded by the kernel and computed as it would be alone (tile shape from n: fixed_tile 2).  The result is [2][n][128]
static int enc_stages_nlc(orca_ctx* ctx, const orca_net* net, const SeqSource& src, const EncRoute& r, int st_from, long n, float* const buf[3], long ld1,
                          float** out, long* out_ld, long* out_n) {
  const int prec = net->precision;
  const int B = r.seam ? 2 : 1, own_tile = r.seam ? 2 : 0;
  if (r.seam && st_from != kPlanarStages) return fail(ORCA_EINVAL, "internal: two strands enter the channel-last stages behind stage 4");
  int P = 0;
  // stage 1 uncomposed: the 4-channel first layer stays on the fp32 kernel (K = 36, 1 % of the FLOPs) and writes channel-last
  if (r.pipe == PIPE_NLC && !r.compose_nlc) ORCA_TRY(enc_rows_channel_major(ctx, src, n, buf, ld1));
  for (int st = st_from; st < 7 && st <= r.last; ++st) {
    const ConvLayer* L = &net->convs[4 * st];
    if (kEncPools[st] == 4) {
      n = n / 4;  // MaxPool1d(4) was fused into the epilogue of the previous stage's last conv
    } else if (kEncPools[st] > 1 && st != r.first) {
      const long n2 = n / kEncPools[st];
      const int Q = (P + 1) % 3;
      if (B > 1 && n % kEncPools[st]) return fail(ORCA_EINVAL, "internal: stage %d: a batch row of %ld positions under MaxPool1d(%d)", st + 1, n, kEncPools[st]);
      if (B > 1 && st == st_from) {      // from the joint rows: each strand's own windows
        ORCA_TRY(launch_pool_nlc(ctx, buf[P], buf[Q], n2, L[0].cin, kEncPools[st]));
        ORCA_TRY(launch_pool_nlc(ctx, buf[P] + (r.seam / 5) * L[0].cin, buf[Q] + n2 * L[0].cin, n2, L[0].cin, kEncPools[st]));
      } else {
        ORCA_TRY(launch_pool_nlc(ctx, buf[P], buf[Q], B * n2, L[0].cin, kEncPools[st]));
      }
      P = Q; n = n2;
    }
    const int T = (P + 1) % 3, LO = (P + 2) % 3;
    const long bs = B > 1 ? n * 128 : 0;
    if (st == 0 && r.compose_nlc) {
      ORCA_TRY(enc_stage1_groups_nlc(ctx, net, src, n, buf[LO], buf[T]));
    } else {
      if (st == 0) ORCA_TRY(launch_conv1d(ctx, L[0], buf[P], 0, ld1, buf[T], 0, 0, nullptr, nullptr, 1, n, 0, 0, 1));
      else ORCA_TRY(launch_conv1d_b16(ctx, L[0], prec, buf[P], bs, buf[T], bs, nullptr, B, n, 0, 0, nullptr, own_tile));
      ORCA_TRY(launch_conv1d_b16(ctx, L[1], prec, buf[T], bs, buf[LO], bs, nullptr, B, n, 0, 0, nullptr, own_tile));
      ORCA_TRY(launch_conv1d_b16(ctx, L[2], prec, buf[LO], bs, buf[T], bs, nullptr, B, n, 1, 0, nullptr, own_tile));
    }
    ORCA_TRY(launch_conv1d_b16(ctx, L[3], prec, buf[T], bs, buf[P], bs, st < 6 ? buf[LO] : nullptr, B, n, 1,
                               (st < 6 && kEncPools[st + 1] == 4) ? 1 : 0, nullptr, own_tile));
  }
  if (r.last < 6 && kEncPools[r.last + 1] == 4) n = n / 4;   // stopped behind stage 1 / 2 (orca_encoder_probe): their last conv pooled
  *out = buf[P]; *out_ld = -128; *out_n = n;   // negative ld: result is channel-last [n][C]
  return ORCA_OK;
}

// the exact-fp32 pipeline: channel-major rows [C][ld], every pool a launch
static int enc_stages_f32(orca_ctx* ctx, const orca_net* net, const SeqSource& src, const EncRoute& r, long n, float* const buf[3], long ld,
                          float** out, long* out_ld, long* out_n) {
  hipStream_t s = ctx->stream;
  int P = 0, cprev = 4;
  if (!r.compose32) ORCA_TRY(enc_rows_channel_major(ctx, src, n, buf, ld));
  for (int st = 0; st < 7 && st <= r.last; ++st) {
    const ConvLayer* L = &net->convs[4 * st];
    if (kEncPools[st] > 1) {
      const long n2 = n / kEncPools[st], ld2 = ru4(n2);
      const int Q = (P + 1) % 3;
      ORCA_TRY(launch_pool(ctx, buf[P], ld, buf[Q], ld2, cprev, n2, kEncPools[st]));
      P = Q; n = n2; ld = ld2;
    }
    const int T = (P + 1) % 3, LO = (P + 2) % 3;
    if (st == 0 && r.compose32) {
      // lconv1 (17 taps) and conv1.a o lconv1 (25 taps + ReLU) straight from the source, fp32 FMAs; exact ends by the edge chain
      FirstF32Args fa{};
      fa.in = edge_source(src);
      fa.in.n = n; fa.ldy = ld;
      const long nt = (n + 127) / 128;
      const dim3 grid((unsigned)(nt < 4096 ? nt : 4096));
      fa.w = net->d_l1_f32; fa.bias = net->d_l1_bias32; fa.relu = 0; fa.y = buf[LO];
      hipLaunchKernelGGL((first_taps_f32_kernel<17>), grid, dim3(256), 0, s, fa);
      fa.w = net->d_c1a_f32; fa.bias = net->d_c1a_bias32; fa.relu = 1; fa.y = buf[T];
      hipLaunchKernelGGL((first_taps_f32_kernel<25>), grid, dim3(256), 0, s, fa);
      LAUNCHCHECK("first_taps_f32_kernel");
      ORCA_TRY(launch_edge_chain(ctx, L, 3, 8, fa.in, n, buf[LO], buf[T], 2, ld));
    } else {
      ORCA_TRY(launch_conv1d(ctx, L[0], buf[P], 0, ld, buf[T], 0, ld, nullptr, nullptr, 1, n, 0, 0));
      ORCA_TRY(launch_conv1d(ctx, L[1], buf[T], 0, ld, buf[LO], 0, ld, nullptr, nullptr, 1, n, 0, 0));
      ORCA_TRY(launch_conv1d(ctx, L[2], buf[LO], 0, ld, buf[T], 0, ld, nullptr, nullptr, 1, n, 1, 0));
    }
    ORCA_TRY(launch_conv1d(ctx, L[3], buf[T], 0, ld, buf[P], 0, ld, st < 6 ? buf[LO] : nullptr, nullptr, 1, n, 1, 0));
    cprev = L[3].cout;
  }
  *out = buf[P]; *out_ld = ld; *out_n = n;
  return ORCA_OK;
}

// One chunk: src (n1 positions; a part that starts behind stage 1: its input in buf[0]) -> the route's output in one of the three buffers.
// *out_ld: row stride of a channel-major result [128][ld]; negative: fp32 channel-last [n][128]; 0: planes
static int enc_run_route(orca_ctx* ctx, orca_net* net, const SeqSource& src, const EncRoute& r, long n1, float* const buf[3],
                         long ld1, float** out, long* out_ld, long* out_n) {
  if (r.pipe == PIPE_F32) return enc_stages_f32(ctx, net, src, r, n1, buf, ld1, out, out_ld, out_n);
  long n = n1;
  int st = r.first;
  if (r.planar() && st < kPlanarStages) {
    if (st == 0) ORCA_TRY(enc_stage1_planes(ctx, net, src, r, buf, &n));
    ORCA_TRY(enc_planar_stages(ctx, net, r, buf, &n));
    if (r.last < kPlanarStages) { *out = buf[kS]; *out_ld = r.out == OUT_ROWS ? -128 : 0; *out_n = n; return ORCA_OK; }
    st = kPlanarStages;
  }
  return enc_stages_nlc(ctx, net, src, r, st, n, buf, ld1, out, out_ld, out_n);
}

static int encoder_chunk(orca_ctx* ctx, orca_net* net, const SeqSource& src, long n1, float* const buf[3],
                         long ld1, float** out, long* out_ld, long* out_n, int part = ENC_FULL) {
  EncRoute r;
  ORCA_TRY(enc_route(net, src, part, &r));
  return enc_run_route(ctx, net, src, r, n1, buf, ld1, out, out_ld, out_n);
}

static int encoder_forward_impl(orca_ctx* ctx, orca_net* net, const float* x, int64_t sx_b, int64_t sx_c, int64_t sx_l,
                                const unsigned char* codes, int64_t sc_b, int reverse,
                                int B, int64_t L, int64_t bin_lo, int64_t bin_hi, float* out, int64_t so_b,
                                int64_t so_c, int64_t chunk_bp, int64_t win_origin = 0, int64_t win_len = -1,
                                const unsigned char* nmask = nullptr, int64_t two_origin = 0) {
  if (!ctx || !net || (!x && !codes) || !out) return fail(ORCA_EINVAL, "orca_encoder_forward: NULL argument");
  if (net->kind != ORCA_NET_ENCODER) return fail(ORCA_EINVAL, "orca_encoder_forward: net is not an Encoder");
  HIPCHECK(hipSetDevice(ctx->device));
  const long total = orca_encoder_num_bins(L);
  if (bin_hi <= 0) bin_hi = total;
  if (bin_lo < 0 || bin_lo > bin_hi || bin_hi > total) return fail(ORCA_EINVAL, "bin range [%ld,%ld) outside [0,%ld)", (long)bin_lo, (long)bin_hi, total);
  if (bin_lo == bin_hi || B <= 0) return ORCA_OK;
  bool chunk_auto = false;
  if (chunk_bp <= 0) {
    // a 32 Mb window is one chunk; longer inputs (the 256 Mb models) run in 128 Mb chunks: 98 GB of workspace (3 x 64 channels x 4 B per base) of
    // the 288 GB, a quarter of the chunk seams (each costs a 224 kb halo and one latency-bound pass through stages 5-7): 418 -> 406 ms per
    // genomepredict_256Mb call against 32 Mb chunks, 412 with 64 Mb (same box).  $ORCA_ENCODER_CHUNK_BP overrides.
    // The chunk size does not change a result beyond fp32 round-off of the last stages (tests/test_gpu_e2e.py::test_encoder_256mb_chunk_sizes).
    // The choice is DETERMINISTIC (free memory varies per rank and per run and does not count what torch's allocator holds): the
    // largest of 128 / 64 / 32 Mb whose workspace (768 B per base) stays under 40 % of the device's TOTAL memory divided by
    // $ORCA_RANKS_PER_DEVICE (default 1; bench.py and the tests set it when several ranks share one GPU).
    const char* e = getenv("ORCA_ENCODER_CHUNK_BP");
    chunk_bp = e ? atol(e) : 32000000L;
    chunk_auto = !e;
    if (!e && L > 32000000L) {
      size_t fr = 0, tot = 0;
      const char* r = getenv("ORCA_RANKS_PER_DEVICE");
      const long rpd = r && atol(r) > 0 ? atol(r) : 1;
      if (hipMemGetInfo(&fr, &tot) == hipSuccess)
        for (long c : {128000000L, 64000000L})
          if ((double)(c + 2 * kHaloBp + 4096) * 768.0 <= 0.40 * (double)tot / (double)rpd) { chunk_bp = c; break; }
    }
  }
  if (chunk_bp % kBinBp) return fail(ORCA_EINVAL, "chunk_bp must be a multiple of 4000");
  long chunk_bins = 0, ld1 = 0;
  float* buf[3];
  for (;;) {
    chunk_bins = chunk_bp / kBinBp;
    long max_n1 = 0;
    for (long cb0 = bin_lo; cb0 < bin_hi; cb0 += chunk_bins) {
      const long cb1 = cb0 + chunk_bins < bin_hi ? cb0 + chunk_bins : bin_hi;
      const long lo = cb0 * kBinBp - kHaloBp > 0 ? cb0 * kBinBp - kHaloBp : 0;
      const long hi = (cb1 == total) ? L : (cb1 * kBinBp + kHaloBp < L ? cb1 * kBinBp + kHaloBp : L);
      if (hi - lo > max_n1) max_n1 = hi - lo;
    }
    ld1 = ru4(max_n1) + 1024;   // slack: P16 planes are padded to 512 positions + guards
    const int rc = ws_three(ctx, (size_t)64 * ld1, buf);
    if (rc == ORCA_OK) break;
    // the deterministic choice above looks at TOTAL memory; if the device cannot give that much right now (another process, ranks
    // sharing it without $ORCA_RANKS_PER_DEVICE, torch's allocator holding most of it) fall back chunk size by chunk size - same result
    if (rc != ORCA_ENOMEM || !chunk_auto || chunk_bp <= 32000000L) return rc;
    (void)hipGetLastError();
    chunk_bp /= 2;
  }
  for (int b = 0; b < B; ++b) {
    for (long cb0 = bin_lo; cb0 < bin_hi; cb0 += chunk_bins) {
      const long cb1 = cb0 + chunk_bins < bin_hi ? cb0 + chunk_bins : bin_hi;
      const long lo = cb0 * kBinBp - kHaloBp > 0 ? cb0 * kBinBp - kHaloBp : 0;
      const long hi = (cb1 == total) ? L : (cb1 * kBinBp + kHaloBp < L ? cb1 * kBinBp + kHaloBp : L);
      float* res; long rld, rn;
      SeqSource src;
      if (codes && win_len >= 0) {
        // the caller holds only bases [win_origin, win_origin + win_len) of the L-base sequence: this chunk reads strand positions
        // [lo, hi) = bases [lo, hi) (forward) or [L - hi, L - lo) (reverse complement)
        const long b0 = reverse ? L - hi : lo, b1 = reverse ? L - lo : hi;
        if (b0 < win_origin || b1 > win_origin + win_len)
          return fail(ORCA_EINVAL, "code window [%ld,%ld) does not cover bases [%ld,%ld) needed for bins [%ld,%ld) (112 kb halo included)",
                      (long)win_origin, (long)(win_origin + win_len), b0, b1, (long)cb0, (long)cb1);
      }
      if (codes) { src.codes = codes + (nmask ? 0 : (long)b * sc_b - win_origin); src.nmask = nmask; src.origin = two_origin; src.codes_L = L; src.codes_off = lo; src.reverse = reverse; }
      else { src.x = x + (long)b * sx_b + lo * sx_l; src.sx_c = sx_c; src.sx_l = sx_l; }
      ORCA_TRY(encoder_chunk(ctx, net, src, hi - lo, buf, ru4(hi - lo), &res, &rld, &rn));
      const long keep = cb0 - lo / kBinBp;
      if (keep + (cb1 - cb0) > rn) return fail(ORCA_EINVAL, "internal: chunk produced %ld bins, need %ld", rn, keep + (cb1 - cb0));
      if (rld < 0)  // channel-last result [bins][128] -> out[c][bin]
        ORCA_TRY(launch_copy2d(ctx, res + keep * 128, 1, 128, out + (long)b * so_b + (cb0 - bin_lo), so_c, 128, cb1 - cb0));
      else
        ORCA_TRY(launch_copy2d(ctx, res + keep, rld, 1, out + (long)b * so_b + (cb0 - bin_lo), so_c, 128, cb1 - cb0));
    }
  }
  return ORCA_OK;
}

extern "C" int orca_encoder_forward(orca_ctx* ctx, orca_net* net, const float* x, int64_t sx_b, int64_t sx_c, int64_t sx_l,
                                    int B, int64_t L, int64_t bin_lo, int64_t bin_hi, float* out, int64_t so_b,
                                    int64_t so_c, int64_t chunk_bp) {
  return encoder_forward_impl(ctx, net, x, sx_b, sx_c, sx_l, nullptr, 0, 0, B, L, bin_lo, bin_hi, out, so_b, so_c, chunk_bp);
}

extern "C" int orca_encoder_forward_codes(orca_ctx* ctx, orca_net* net, const uint8_t* codes, int64_t sc_b, int reverse, int B,
                                          int64_t L, int64_t bin_lo, int64_t bin_hi, float* out, int64_t so_b, int64_t so_c,
                                          int64_t chunk_bp) {
  return encoder_forward_impl(ctx, net, nullptr, 0, 0, 0, codes, sc_b, reverse, B, L, bin_lo, bin_hi, out, so_b, so_c, chunk_bp);
}

extern "C" int orca_encoder_forward_codes_window(orca_ctx* ctx, orca_net* net, const uint8_t* codes, int64_t sc_b, int64_t win_origin, int64_t win_len,
                                                 int reverse, int B, int64_t L, int64_t bin_lo, int64_t bin_hi, float* out, int64_t so_b,
                                                 int64_t so_c, int64_t chunk_bp) {
  if (win_origin < 0 || win_len < 0 || win_origin + win_len > L) return fail(ORCA_EINVAL, "code window [%ld,+%ld) outside the %ld-base sequence", (long)win_origin, (long)win_len, (long)L);
  return encoder_forward_impl(ctx, net, nullptr, 0, 0, 0, codes, sc_b, reverse, B, L, bin_lo, bin_hi, out, so_b, so_c, chunk_bp, win_origin, win_len);
}

// Encoder straight from a 2-bit genome resident in HBM (orca_amd/genome.py TwoBitGenome: 2 bits per base + 1 N bit = 3/8 byte per base):
// the sequence is bases [start, start + L) of the chromosome whose planes are `two` / `nmask`; the one-hot expansion of a base happens
// where the 1-byte codes are expanded - in LDS inside the first-layer kernels / the residual-from-the-bases epilogue (conv_p16.h:
// p16_base_at) - so neither the unpack pass (orca_genome_unpack_2bit) nor the 1 byte/base window ever exists.
extern "C" int orca_encoder_forward_2bit(orca_ctx* ctx, orca_net* net, const uint8_t* two, const uint8_t* nmask, int64_t start, int reverse,
                                         int64_t L, int64_t bin_lo, int64_t bin_hi, float* out, int64_t so_c, int64_t chunk_bp) {
  if (!two || !nmask || start < 0) return fail(ORCA_EINVAL, "orca_encoder_forward_2bit: NULL plane or negative start");
  return encoder_forward_impl(ctx, net, nullptr, 0, 0, 0, two, 0, reverse, 1, L, bin_lo, bin_hi, out, 0, so_c, chunk_bp, 0, -1, nmask, start);
}

// Both strands of one packed sequence.  Stages 1-2 (n = L and L / 4: hundreds of tile rounds per launch) run per strand; each strand's last
// stage-2 conv writes its MaxPool1d(4)'d output into ONE set of planes - the forward strand at position 0, the reverse complement at off3 =
// roundup(n3 + 40, 250), zeros in between - and stages 3-7 (n <= L / 16: launches of a few rounds and latency chains) run ONCE on both.  The
// kernels see one longer sequence (stages 3-4) or a batch of two rows (stages 5-7); every position reads the inputs and does the arithmetic it
// would in a call of its own, so the result is bit-identical to two orca_encoder_forward_codes calls.  The joint input is a fourth workspace
// buffer (96 channels x ~2 L / 16 positions x 4 B: 1.5 GB for 32 Mb), because the second strand's stages 1-2 need all three others.
static int encoder_two_strands_joint(orca_ctx* ctx, orca_net* net, const unsigned char* codes, long L, float* const out[2], long so_c) {
  const long n3 = L / 16, off3 = (n3 + 40 + 249) / 250 * 250;
  const long plen3 = p16_plen(off3 + n3 + 128);                       // enc_planar_stages: plen() of the joint tensors
  const long ld1 = ru4(L) + 1024;
  // (a plane unit is 4 floats, a C-channel P16 tensor C / 4 units per position)
  size_t per = (size_t)64 * ld1;
  if (per < (size_t)128 * plen3) per = (size_t)128 * plen3;           // stage 3's 128-channel joint tensors
  size_t perj = (size_t)net->convs[7].cout * plen3;                   // the joint input, then stage 3's pooled output and stage 4's fp32 rows
  const size_t nt4 = (size_t)(off3 + n3) / 5;
  if (perj < 128 * (size_t)p16_plen((long)nt4 + 128)) perj = 128 * (size_t)p16_plen((long)nt4 + 128);
  ORCA_TRY(ws_ensure(ctx, 3 * ru256(per * sizeof(float)) + ru256(perj * sizeof(float))));
  float* buf[3];
  for (int i = 0; i < 3; ++i) buf[i] = ws_take(ctx, per);
  float* const joint = ws_take(ctx, perj);
  if (!joint) return fail(ORCA_ENOMEM, "internal: workspace arena exhausted");
  SeqSource src;
  src.codes = codes; src.codes_L = L; src.codes_off = 0;
  EncRoute r;
  ORCA_TRY(enc_route(net, src, ENC_FULL, &r));
  if (!r.planar()) return fail(ORCA_EINVAL, "internal: the two-strand route needs a planar pipeline");
  const int C3 = net->convs[7].cout;
  for (int strand = 0; strand < 2; ++strand) {
    EncRoute f = r;
    f.last = 1; f.out = OUT_PLANES_POOLED; f.pooled_to = joint; f.pooled_plen = plen3; f.pooled_off = strand * off3;
    src.reverse = strand;
    long n = L;
    ORCA_TRY(enc_stage1_planes(ctx, net, src, f, buf, &n));
    ORCA_TRY(enc_planar_stages(ctx, net, f, buf, &n));
    if (n != n3) return fail(ORCA_EINVAL, "internal: stages 1-2 produced %ld positions for %ld bases", n, L);
  }
  ORCA_TRY(launch_p16_zero_pads(ctx, joint, C3, off3 + n3, r.fmt, plen3, n3, off3));
  r.first = 2; r.seam = off3;
  float* const jb[3] = {joint, buf[1], buf[2]};
  long n = n3;
  ORCA_TRY(enc_planar_stages(ctx, net, r, jb, &n));
  float* res; long rld, rn;
  ORCA_TRY(enc_stages_nlc(ctx, net, src, r, kPlanarStages, n, jb, ru4(L), &res, &rld, &rn));
  if (rn != orca_encoder_num_bins(L)) return fail(ORCA_EINVAL, "internal: the joint stages produced %ld bins, need %ld", rn, (long)orca_encoder_num_bins(L));
  for (int strand = 0; strand < 2; ++strand) ORCA_TRY(launch_copy2d(ctx, res + strand * rn * 128, 1, 128, out[strand], so_c, 128, rn));
  return ORCA_OK;
}

extern "C" int orca_encoder_forward_two_strands(orca_ctx* ctx, orca_net* net, const uint8_t* codes, int64_t L, float* out_fwd, float* out_rev, int64_t so_c) {
  if (!ctx || !net || !codes || !out_fwd || !out_rev) return fail(ORCA_EINVAL, "orca_encoder_forward_two_strands: NULL argument");
  if (net->kind != ORCA_NET_ENCODER) return fail(ORCA_EINVAL, "orca_encoder_forward_two_strands: net is not an Encoder");
  const char* e = getenv("ORCA_ENCODER_CHUNK_BP");
  const bool planar = net->precision == ORCA_PRECISION_F16X2 || net->precision == ORCA_PRECISION_BF16;
  // the joint pass: one chunk of whole bins on the default planar route; everything else is the two calls it has always been
  if (!net->enc_two_strands || !planar || net->enc_form != ORCA_ENCODER_FORM_DEFAULT || L <= 0 || L % kBinBp || L > (e ? atol(e) : 32000000L)) {
    ORCA_TRY(orca_encoder_forward_codes(ctx, net, codes, 0, 0, 1, L, 0, 0, out_fwd, 0, so_c, 0));
    return orca_encoder_forward_codes(ctx, net, codes, 0, 1, 1, L, 0, 0, out_rev, 0, so_c, 0);
  }
  HIPCHECK(hipSetDevice(ctx->device));
  float* const out[2] = {out_fwd, out_rev};
  return encoder_two_strands_joint(ctx, net, codes, L, out, so_c);
}

extern "C" int orca_net_set_encoder_two_strands(orca_net* net, int on) {
  if (!net || net->kind != ORCA_NET_ENCODER) return fail(ORCA_EINVAL, "orca_net_set_encoder_two_strands: not an Encoder net");
  net->enc_two_strands = on ? 1 : 0;
  return ORCA_OK;
}

extern "C" int orca_net_get_encoder_two_strands(orca_net* net, int* on) {
  if (!net || !on || net->kind != ORCA_NET_ENCODER) return fail(ORCA_EINVAL, "orca_net_get_encoder_two_strands: not an Encoder net");
  *on = net->enc_two_strands;
  return ORCA_OK;
}

// orca_encoder_probe: the ENC_FULL route of the net's own arithmetic and form, stopped behind stage `stage` (EncRoute::last), and what that route
// leaves there copied out as fp32 channel-last rows.  The route comes from enc_route like every other; only `last` and the hand-over format of a
// planar stage are the probe's, so that the part exports keep their refusals
extern "C" int orca_encoder_probe(orca_ctx* ctx, orca_net* net, const uint8_t* codes, int reverse, const float* x, int64_t sx_c, int64_t sx_l, int64_t L,
                                  int stage, float* out, int64_t out_floats, int64_t* n_out, int* channels, int* pool) {
  if (!ctx || !net || !out || !n_out || !channels || !pool) return fail(ORCA_EINVAL, "orca_encoder_probe: NULL argument");
  if ((codes == nullptr) == (x == nullptr)) return fail(ORCA_EINVAL, "orca_encoder_probe: exactly one of codes and x");
  if (net->kind != ORCA_NET_ENCODER) return fail(ORCA_EINVAL, "orca_encoder_probe: net is not an Encoder");
  if (stage < 1 || stage > 7 || L <= 0) return fail(ORCA_EINVAL, "orca_encoder_probe: stage %d (1..7) of %ld bases", stage, (long)L);
  SeqSource src;
  if (codes) { src.codes = codes; src.codes_L = L; src.codes_off = 0; src.reverse = reverse ? 1 : 0; }
  else { src.x = x; src.sx_c = sx_c; src.sx_l = sx_l; }
  EncRoute r;
  ORCA_TRY(enc_route(net, src, ENC_FULL, &r));
  r.last = stage - 1;
  long n = L;                                              // positions the stage reads
  for (int st = 1; st < stage; ++st) n /= kEncPools[st];
  int pl = 1;                                              // the pool the route has already applied to what it leaves behind the stage
  if (r.pipe == PIPE_NLC && stage <= 2) pl = 4;            // fused into the last conv's epilogue (conv_bf16s.h)
  if (r.planar() && stage < kPlanarStages) { pl = kEncPools[stage]; r.out = OUT_PLANES_POOLED; }
  if (r.planar() && stage == kPlanarStages) r.out = OUT_ROWS;
  const int C = net->convs[4 * (stage - 1) + 3].cout;
  const long nout = n / pl;
  if (n <= 0 || nout <= 0) return fail(ORCA_EINVAL, "orca_encoder_probe: %ld bases leave stage %d no position", (long)L, stage);
  if (nout * C > out_floats) return fail(ORCA_EINVAL, "orca_encoder_probe: out holds %ld floats, stage %d needs %ld x %d", (long)out_floats, stage, nout, C);
  HIPCHECK(hipSetDevice(ctx->device));
  const long ld1 = ru4(L) + 1024;
  float* buf[3];
  ORCA_TRY(ws_three(ctx, (size_t)64 * ld1, buf));
  float* res; long rld, rn;
  ORCA_TRY(enc_run_route(ctx, net, src, r, L, buf, ru4(L), &res, &rld, &rn));
  if (rn != nout) return fail(ORCA_EINVAL, "internal: the probe of stage %d produced %ld positions, expected %ld", stage, rn, nout);
  if (rld > 0) {                                           // channel-major [C][ld]
    ORCA_TRY(launch_copy2d_flat(ctx, res, 1, rld, out, C, nout, C));
  } else if (rld < 0) {                                    // fp32 rows [n][C]
    HIPCHECK(hipMemcpyAsync(out, res, (size_t)nout * C * sizeof(float), hipMemcpyDeviceToDevice, ctx->stream));
  } else {
    const dim3 grid((unsigned)((nout * (C / 4) + 255) / 256));
    if (r.fmt == 1) hipLaunchKernelGGL(b16_to_nlc_kernel, grid, dim3(256), 0, ctx->stream, reinterpret_cast<const f32x4*>(res), out, nout, C, p16_plen(nout));
    else hipLaunchKernelGGL(p16_to_nlc_kernel, grid, dim3(256), 0, ctx->stream, reinterpret_cast<const f32x4*>(res), out, nout, C, p16_plen(nout));
    LAUNCHCHECK("p16_to_nlc_kernel");
  }
  *n_out = nout; *channels = C; *pool = pl;
  return ORCA_OK;
}

// ---------------------------------------------------------------------------
// The Encoder in two parts (f16x2 / P16 planes): stage-3 cache of a chromosome -> stage-4 input of a window -> bins.
// Stages 1-3 hold 99 % of the Encoder's FLOPs and are translation-covariant on a 16-base grid (pools 4 x 4) with a reach of 351 bases
// (orca_modules.py:811-852): their output on a chromosome, kept once per strand and per phase mod 16 (512 bytes per base and strand), serves
// EVERY window of every allele built from pieces of that chromosome, whatever its phase on the 4 kb grid - the reference's structural-variant
// drivers place their windows at the variant's own phase (orca_predict.py:1613).  A window then costs a MaxPool1d(5) gather from the cache, the
// front on a few kb around its ends and junctions, and stages 4-7.
// ---------------------------------------------------------------------------
extern "C" int64_t orca_p16_plane_units(int64_t n) { return p16_plen(n); }

static int front_run(orca_ctx* ctx, orca_net* net, const uint8_t* codes, int64_t L, int reverse, int64_t base0, int64_t nbases, int part, float** res, long* rn) {
  if (!ctx || !net || !codes) return fail(ORCA_EINVAL, "encoder front: NULL argument");
  if (net->kind != ORCA_NET_ENCODER) return fail(ORCA_EINVAL, "encoder front: net is not an Encoder");
  if (net->precision != ORCA_PRECISION_F16X2) return fail(ORCA_EINVAL, "encoder front: f16x2 arithmetic only (P16 planes)");
  if (nbases <= 0 || nbases % 80 || base0 < 0 || base0 + nbases > L) return fail(ORCA_EINVAL, "encoder front: bases [%ld,+%ld) of %ld: a positive multiple of 80 inside the sequence", (long)base0, (long)nbases, (long)L);
  HIPCHECK(hipSetDevice(ctx->device));
  const long ld1 = ru4(nbases) + 1024;
  float* buf[3];
  ORCA_TRY(ws_three(ctx, (size_t)64 * ld1, buf));
  SeqSource src;
  src.codes = codes; src.codes_L = L; src.codes_off = base0; src.reverse = reverse;
  long rld;
  return encoder_chunk(ctx, net, src, nbases, buf, ru4(nbases), res, &rld, rn, part);
}

extern "C" int orca_encoder_stage3_planes(orca_ctx* ctx, orca_net* net, const uint8_t* codes, int64_t L, int reverse, float* planes, int64_t plane_units) {
  if (!planes) return fail(ORCA_EINVAL, "orca_encoder_stage3_planes: NULL argument");
  float* res; long rn;
  ORCA_TRY(front_run(ctx, net, codes, L, reverse, 0, L, ENC_FRONT_UNPOOLED, &res, &rn));
  if (plane_units != p16_plen(rn)) return fail(ORCA_EINVAL, "orca_encoder_stage3_planes: planes of %ld units, %ld positions need %ld", (long)plane_units, rn, p16_plen(rn));
  HIPCHECK(hipMemcpyAsync(planes, res, (size_t)32 * plane_units * 16, hipMemcpyDeviceToDevice, ctx->stream));
  return ORCA_OK;
}

extern "C" int orca_p16_pool5_into(orca_ctx* ctx, const float* src, int64_t src_units, int64_t src_pos0, float* dst, int64_t dst_units, int64_t dst_pos0, int64_t count) {
  if (!ctx || !src || !dst) return fail(ORCA_EINVAL, "orca_p16_pool5_into: NULL argument");
  if (count <= 0) return ORCA_OK;
  if (src_pos0 < 0 || dst_pos0 < 0 || P16_GUARD + src_pos0 + 5 * count > src_units || P16_GUARD + dst_pos0 + count > dst_units)
    return fail(ORCA_EINVAL, "orca_p16_pool5_into: positions [%ld,+5 x %ld) / [%ld,+%ld) outside planes of %ld / %ld units", (long)src_pos0, (long)count, (long)dst_pos0, (long)count, (long)src_units, (long)dst_units);
  HIPCHECK(hipSetDevice(ctx->device));
  hipLaunchKernelGGL(p16_pool5_into_kernel, dim3((unsigned)((count + 255) / 256), 16), dim3(256), 0, ctx->stream, reinterpret_cast<const f32x4*>(src), (long)src_units, (long)src_pos0,
                     reinterpret_cast<f32x4*>(dst), (long)dst_units, (long)dst_pos0, (long)count);
  LAUNCHCHECK("p16_pool5_into_kernel");
  return ORCA_OK;
}

extern "C" int orca_encoder_front_snippet(orca_ctx* ctx, orca_net* net, const uint8_t* codes, int64_t L, int reverse, int64_t base0, int64_t nbases, int64_t skip,
                                          int64_t count, float* dst, int64_t dst_units, int64_t dst_pos0) {
  if (!dst) return fail(ORCA_EINVAL, "orca_encoder_front_snippet: NULL argument");
  float* res; long rn;
  ORCA_TRY(front_run(ctx, net, codes, L, reverse, base0, nbases, ENC_FRONT_POOLED, &res, &rn));
  if (skip < 0 || count <= 0 || skip + count > rn || dst_pos0 < 0 || P16_GUARD + dst_pos0 + count > dst_units)
    return fail(ORCA_EINVAL, "orca_encoder_front_snippet: pooled positions [%ld,+%ld) of %ld -> [%ld,..) of planes of %ld units", (long)skip, (long)count, rn, (long)dst_pos0, (long)dst_units);
  hipLaunchKernelGGL(p16_copy_units_kernel, dim3((unsigned)((count + 255) / 256), 32), dim3(256), 0, ctx->stream, reinterpret_cast<const f32x4*>(res), p16_plen(rn), (long)skip,
                     reinterpret_cast<f32x4*>(dst), (long)dst_units, (long)dst_pos0, (long)count);
  LAUNCHCHECK("p16_copy_units_kernel");
  return ORCA_OK;
}

// stage 4 onwards (ENC_BACK / ENC_STAGE4) from a copy of the caller's stage-4 input planes
static int back_run(orca_ctx* ctx, orca_net* net, const float* s4, int64_t s4_units, int64_t n4, int part, float** res, long* rld, long* rn) {
  HIPCHECK(hipSetDevice(ctx->device));
  const long ld = ru4(n4) + 1024;                         // per buffer: 128 channels x ld floats (P16 planes of 128 channels; fp32 [n][128] behind stage 4)
  float* buf[3];
  ORCA_TRY(ws_three(ctx, (size_t)128 * ld, buf));
  HIPCHECK(hipMemcpyAsync(buf[0], s4, (size_t)32 * s4_units * 16, hipMemcpyDeviceToDevice, ctx->stream));
  ORCA_TRY(launch_p16_zero_pads(ctx, buf[0], 128, n4, 0));
  return encoder_chunk(ctx, net, SeqSource(), n4, buf, ru4(n4), res, rld, rn, part);
}

extern "C" int orca_encoder_back(orca_ctx* ctx, orca_net* net, const float* s4, int64_t s4_units, int64_t n4, float* out, int64_t so_c) {
  if (!ctx || !net || !s4 || !out) return fail(ORCA_EINVAL, "orca_encoder_back: NULL argument");
  if (net->kind != ORCA_NET_ENCODER || net->precision != ORCA_PRECISION_F16X2) return fail(ORCA_EINVAL, "orca_encoder_back: an Encoder net in the f16x2 arithmetic");
  if (n4 <= 0 || n4 % 50 || s4_units != p16_plen(n4)) return fail(ORCA_EINVAL, "orca_encoder_back: %ld stage-4 positions (a multiple of 50) in planes of %ld units (need %ld)", (long)n4, (long)s4_units, p16_plen(n4));
  float* res; long rld, rn;
  ORCA_TRY(back_run(ctx, net, s4, s4_units, n4, ENC_BACK, &res, &rld, &rn));
  if (rld >= 0 || rn != n4 / 50) return fail(ORCA_EINVAL, "internal: the Encoder's back part produced %ld bins for %ld positions", rn, (long)n4);
  return launch_copy2d(ctx, res, 1, 128, out, so_c, 128, rn);
}

// ---- one level further: stage 4 in the cache (fp32 rows [n][128] on the 80-base grid, phases mod 80; same 512 bytes per base and strand) ----
extern "C" int orca_encoder_stage4_rows(orca_ctx* ctx, orca_net* net, const float* s4, int64_t s4_units, int64_t n4, float* rows) {
  if (!ctx || !net || !s4 || !rows) return fail(ORCA_EINVAL, "orca_encoder_stage4_rows: NULL argument");
  if (net->kind != ORCA_NET_ENCODER || net->precision != ORCA_PRECISION_F16X2) return fail(ORCA_EINVAL, "orca_encoder_stage4_rows: an Encoder net in the f16x2 arithmetic");
  if (n4 <= 0 || s4_units != p16_plen(n4)) return fail(ORCA_EINVAL, "orca_encoder_stage4_rows: %ld positions in planes of %ld units (need %ld)", (long)n4, (long)s4_units, p16_plen(n4));
  float* res; long rld, rn;
  ORCA_TRY(back_run(ctx, net, s4, s4_units, n4, ENC_STAGE4, &res, &rld, &rn));
  if (rld >= 0 || rn != n4) return fail(ORCA_EINVAL, "internal: stage 4 produced %ld rows for %ld positions", rn, (long)n4);
  HIPCHECK(hipMemcpyAsync(rows, res, (size_t)n4 * 128 * sizeof(float), hipMemcpyDeviceToDevice, ctx->stream));
  return ORCA_OK;
}

static int launch_rows_pool5(orca_ctx* ctx, const float* src, long src_pos0, float* dst, long dst_pos0, long count) {
  if (count <= 0) return ORCA_OK;
  hipLaunchKernelGGL(rows_pool5_into_kernel, dim3((unsigned)((count * 32 + 255) / 256)), dim3(256), 0, ctx->stream, reinterpret_cast<const f32x4*>(src), src_pos0,
                     reinterpret_cast<f32x4*>(dst), dst_pos0, count);
  LAUNCHCHECK("rows_pool5_into_kernel");
  return ORCA_OK;
}

extern "C" int orca_rows_pool5_into(orca_ctx* ctx, const float* src, int64_t src_rows, int64_t src_pos0, float* dst, int64_t dst_rows, int64_t dst_pos0, int64_t count) {
  if (!ctx || !src || !dst) return fail(ORCA_EINVAL, "orca_rows_pool5_into: NULL argument");
  if (count < 0 || src_pos0 < 0 || dst_pos0 < 0 || src_pos0 + 5 * count > src_rows || dst_pos0 + count > dst_rows)
    return fail(ORCA_EINVAL, "orca_rows_pool5_into: rows [%ld,+5 x %ld) of %ld -> [%ld,+%ld) of %ld", (long)src_pos0, (long)count, (long)src_rows, (long)dst_pos0, (long)count, (long)dst_rows);
  HIPCHECK(hipSetDevice(ctx->device));
  return launch_rows_pool5(ctx, src, (long)src_pos0, dst, (long)dst_pos0, (long)count);
}

extern "C" int orca_encoder_front4_snippet(orca_ctx* ctx, orca_net* net, const uint8_t* codes, int64_t L, int reverse, int64_t base0, int64_t nbases, int64_t skip,
                                           int64_t count, float* dst, int64_t dst_rows, int64_t dst_pos0) {
  if (!dst) return fail(ORCA_EINVAL, "orca_encoder_front4_snippet: NULL argument");
  if (base0 % 400 || nbases % 400) return fail(ORCA_EINVAL, "orca_encoder_front4_snippet: bases [%ld,+%ld): multiples of 400 (the pooled rows must line up with the window's)", (long)base0, (long)nbases);
  float* res; long rn;
  ORCA_TRY(front_run(ctx, net, codes, L, reverse, base0, nbases, ENC_FRONT4, &res, &rn));
  if (skip < 0 || count <= 0 || 5 * (skip + count) > rn || dst_pos0 < 0 || dst_pos0 + count > dst_rows)
    return fail(ORCA_EINVAL, "orca_encoder_front4_snippet: pooled rows [%ld,+%ld) of %ld -> [%ld,..) of %ld", (long)skip, (long)count, rn / 5, (long)dst_pos0, (long)dst_rows);
  return launch_rows_pool5(ctx, res, 5 * (long)skip, dst, (long)dst_pos0, (long)count);
}

// the same for SEVERAL ranges of one front run: the snippets of a window strand concatenated (the window's ends first and last, so that the run's own ends
// are the window's; the seams between snippets lie inside the margins nobody reads) - one chain of ~44 small launches per strand instead of one per snippet
extern "C" int orca_encoder_front4_ranges(orca_ctx* ctx, orca_net* net, const uint8_t* codes, int64_t L, int reverse, int n_ranges, const int64_t* ranges_host,
                                          float* dst, int64_t dst_rows) {
  if (!dst || !ranges_host || n_ranges <= 0) return fail(ORCA_EINVAL, "orca_encoder_front4_ranges: NULL / empty argument");
  if (L % 400) return fail(ORCA_EINVAL, "orca_encoder_front4_ranges: %ld bases: a multiple of 400", (long)L);
  float* res; long rn;
  ORCA_TRY(front_run(ctx, net, codes, L, reverse, 0, L, ENC_FRONT4, &res, &rn));
  for (int k = 0; k < n_ranges; ++k) {
    const long skip = (long)ranges_host[3 * k], count = (long)ranges_host[3 * k + 1], pos0 = (long)ranges_host[3 * k + 2];
    if (skip < 0 || count <= 0 || 5 * (skip + count) > rn || pos0 < 0 || pos0 + count > dst_rows)
      return fail(ORCA_EINVAL, "orca_encoder_front4_ranges: range %d: pooled rows [%ld,+%ld) of %ld -> [%ld,..) of %ld", k, skip, count, rn / 5, pos0, (long)dst_rows);
    ORCA_TRY(launch_rows_pool5(ctx, res, 5 * skip, dst, pos0, count));
  }
  return ORCA_OK;
}

extern "C" int orca_encoder_back5(orca_ctx* ctx, orca_net* net, const float* rows, int64_t n5, float* out, int64_t so_c) {
  if (!ctx || !net || !rows || !out) return fail(ORCA_EINVAL, "orca_encoder_back5: NULL argument");
  if (net->kind != ORCA_NET_ENCODER || net->precision != ORCA_PRECISION_F16X2) return fail(ORCA_EINVAL, "orca_encoder_back5: an Encoder net in the f16x2 arithmetic");
  if (n5 <= 0 || n5 % 10) return fail(ORCA_EINVAL, "orca_encoder_back5: %ld stage-5 positions (a multiple of 10)", (long)n5);
  HIPCHECK(hipSetDevice(ctx->device));
  const long ld = ru4(n5) + 1024;
  float* buf[3];
  ORCA_TRY(ws_three(ctx, (size_t)128 * ld, buf));
  HIPCHECK(hipMemcpyAsync(buf[0], rows, (size_t)n5 * 128 * sizeof(float), hipMemcpyDeviceToDevice, ctx->stream));
  SeqSource src;
  float* res; long rld, rn;
  ORCA_TRY(encoder_chunk(ctx, net, src, n5, buf, ru4(n5), &res, &rld, &rn, ENC_BACK5));
  if (rld >= 0 || rn != n5 / 10) return fail(ORCA_EINVAL, "internal: stages 5-7 produced %ld bins for %ld positions", rn, (long)n5);
  return launch_copy2d(ctx, res, 1, 128, out, so_c, 128, rn);
}


// stages 5-7 of B windows at once: rows [B][n5][128] -> out[b * so_b + c * so_c + bin].  Every conv is ONE launch for the batch with a batch stride, so
// each window keeps its own zero padding (stacking the windows end to end would leak activations across the seams from the first conv on).  The
// rows are read in place (stage 5's first conv reads them; nothing writes them).
extern "C" int orca_encoder_back5_batch(orca_ctx* ctx, orca_net* net, const float* rows, int B, int64_t n5, float* out, int64_t so_b, int64_t so_c) {
  if (!ctx || !net || !rows || !out) return fail(ORCA_EINVAL, "orca_encoder_back5_batch: NULL argument");
  if (net->kind != ORCA_NET_ENCODER || net->precision != ORCA_PRECISION_F16X2) return fail(ORCA_EINVAL, "orca_encoder_back5_batch: an Encoder net in the f16x2 arithmetic");
  if (n5 <= 0 || n5 % 10) return fail(ORCA_EINVAL, "orca_encoder_back5_batch: %ld stage-5 positions (a multiple of 10)", (long)n5);
  if (B <= 0) return ORCA_OK;
  HIPCHECK(hipSetDevice(ctx->device));
  const size_t per = (size_t)B * n5 * 128;
  float* w[3];
  ORCA_TRY(ws_three(ctx, per, w));
  const int prec = ORCA_PRECISION_F16X2;
  long n = n5;
  const float* x = rows;
  float* res = nullptr;
  // stage 5 (st 4): rows -> w[2] (T = w[0], LO = w[1]); stage 6: pool5 w[2] -> w[0], out -> w[0] (T = w[1], LO = w[2]);
  // stage 7: pool2 w[0] -> w[1], out -> w[1] (T = w[2], LO = w[0]; no residual)
  for (int st = 4; st < 7; ++st) {
    const ConvLayer* Ls = &net->convs[4 * st];
    float *P, *T, *LO;
    if (st == 4) { T = w[0]; LO = w[1]; P = w[2]; }
    else {
      const int q = st == 5 ? 0 : 1;
      const long n2 = n / kEncPools[st];
      ORCA_TRY(launch_pool_nlc(ctx, res, w[q], (long)B * n2, Ls[0].cin, kEncPools[st]));
      n = n2; x = w[q]; P = w[q]; T = w[(q + 1) % 3]; LO = w[(q + 2) % 3];
    }
    const long bs = n * 128;
    ORCA_TRY(launch_conv1d_b16(ctx, Ls[0], prec, x, bs, T, bs, nullptr, B, n, 0, 0, nullptr, 1));
    ORCA_TRY(launch_conv1d_b16(ctx, Ls[1], prec, T, bs, LO, bs, nullptr, B, n, 0, 0, nullptr, 1));
    ORCA_TRY(launch_conv1d_b16(ctx, Ls[2], prec, LO, bs, T, bs, nullptr, B, n, 1, 0, nullptr, 1));
    ORCA_TRY(launch_conv1d_b16(ctx, Ls[3], prec, T, bs, P, bs, st < 6 ? LO : nullptr, B, n, 1, 0, nullptr, 1));
    res = P;
  }
  if (n != n5 / 10) return fail(ORCA_EINVAL, "internal: stages 5-7 produced %ld bins for %ld positions", n, (long)n5);
  const long total = (long)B * n * 128;
  hipLaunchKernelGGL(screen_rows_to_bins_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, ctx->stream, res, n, B, out, (long)so_b, (long)so_c);
  LAUNCHCHECK("screen_rows_to_bins_kernel");
  return ORCA_OK;
}


extern "C" int orca_pack_sequence(orca_ctx* ctx, const float* x, int64_t sx_c, int64_t sx_l, int64_t L, uint8_t* codes, int* packable) {
  if (!ctx || !x || !codes || !packable) return fail(ORCA_EINVAL, "orca_pack_sequence: NULL argument");
  HIPCHECK(hipSetDevice(ctx->device));
  HIPCHECK(hipMemsetAsync(ctx->d_flag + 1, 0, sizeof(unsigned), ctx->stream));
  hipLaunchKernelGGL(pack_sequence_kernel, dim3((unsigned)((L + 255) / 256)), dim3(256), 0, ctx->stream, x, sx_c, sx_l, L, codes, ctx->d_flag + 1);
  LAUNCHCHECK("pack_sequence_kernel");
  unsigned h = 0;
  HIPCHECK(hipMemcpyAsync(&h, ctx->d_flag + 1, sizeof h, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHECK(hipStreamSynchronize(ctx->stream));
  *packable = h ? 0 : 1;
  return ORCA_OK;
}

// ---------------------------------------------------------------------------
// Encoder2 / Encoder3 (orca_modules.py:1151-1169, :1388-1406)
// ---------------------------------------------------------------------------
static int launch_transpose(orca_ctx* ctx, const float* src, long lds_, long src_bs, float* dst, long ldd, long dst_bs, long rows, long cols, int B) {
  if (rows <= 0 || cols <= 0 || B <= 0) return ORCA_OK;
  dim3 grid((unsigned)((cols + 31) / 32), (unsigned)((rows + 31) / 32), (unsigned)B);
  hipLaunchKernelGGL(transpose2d_kernel, grid, dim3(32, 8), 0, ctx->stream, src, lds_, src_bs, dst, ldd, dst_bs, rows, cols);
  LAUNCHCHECK("transpose2d_kernel");
  return ORCA_OK;
}

// The U-net encoders on the 16-bit matrix cores (conv_bf16s.h: channel-last fp32 activations [B][n][128], split operands).  Same graph as
// the fp32 path below; the skip connection of the expanding path is the kernel's second residual and the result of a level overwrites the
// contracting-path encoding it consumed.  The outputs are handed over channel-major ([B][128][n], the C ABI's layout) by tiled transposes.
static int unet_forward_nlc(orca_ctx* ctx, orca_net* net, const float* x, int64_t sx_b, int64_t sx_c, int64_t sx_l, int B, int n,
                            float* const* outs, int nlev, bool up_only) {
  const int prec = net->precision;
  const size_t full = (size_t)B * 128 * n;
  size_t need = 3 * ru256(full * sizeof(float));
  for (int i = 0; i <= nlev; ++i) need += ru256((full >> i) * sizeof(float));
  ORCA_TRY(ws_ensure(ctx, need));
  std::vector<float*> encs(nlev + 1);
  for (int i = 0; i <= nlev; ++i) encs[i] = ws_take(ctx, full >> i);
  float* t0 = ws_take(ctx, full);
  float* t1 = ws_take(ctx, full);
  float* t2 = ws_take(ctx, full);
  hipStream_t s = ctx->stream;
  // the (possibly strided) channel-major input -> [B][n][128]
  if (sx_l == 1) ORCA_TRY(launch_transpose(ctx, x, sx_c, sx_b, encs[0], 128, (long)n * 128, 128, n, B));
  else
    for (int b = 0; b < B; ++b) ORCA_TRY(launch_copy2d_flat(ctx, x + (long)b * sx_b, sx_l, sx_c, encs[0] + (size_t)b * n * 128, 128, n, 128));
  const ConvLayer* L = net->convs.data();
  for (int i = 0; i < nlev; ++i) {      // contracting path
    const long no = n >> (i + 1), bs = 128 * no;
    ORCA_TRY(launch_pool_nlc(ctx, encs[i], t0, (long)B * no, 128, 2));          // rows of all batch entries in one pass (n >> i is even)
    ORCA_TRY(launch_conv1d_b16(ctx, L[4 * i + 0], prec, t0, bs, t1, bs, nullptr, B, no, 0));
    ORCA_TRY(launch_conv1d_b16(ctx, L[4 * i + 1], prec, t1, bs, t2, bs, nullptr, B, no, 0));   // lout
    ORCA_TRY(launch_conv1d_b16(ctx, L[4 * i + 2], prec, t2, bs, t1, bs, nullptr, B, no, 1));
    ORCA_TRY(launch_conv1d_b16(ctx, L[4 * i + 3], prec, t1, bs, encs[i + 1], bs, t2, B, no, 1));
  }
  auto hand_over = [&](int lev) { const long nl = n >> lev; return launch_transpose(ctx, encs[lev], 128, nl * 128, outs[lev], nl, 128 * nl, nl, 128, B); };
  ORCA_TRY(hand_over(nlev));
  if (up_only) {
    for (int lev = 0; lev < nlev; ++lev) ORCA_TRY(hand_over(lev));
    return ORCA_OK;
  }
  const float* cur = encs[nlev];
  for (int i = 0; i < nlev; ++i) {      // expanding path
    const int lev = nlev - 1 - i;
    const long no = n >> lev, bs = 128 * no;
    const long total = (long)B * no * 32;
    hipLaunchKernelGGL(upsample1d_x2_nlc_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, cur, t0, (long)B * no, 128);
    LAUNCHCHECK("upsample1d_x2_nlc_kernel");
    const ConvLayer* D = L + 4 * nlev + 4 * i;
    ORCA_TRY(launch_conv1d_b16(ctx, D[0], prec, t0, bs, t1, bs, nullptr, B, no, 0));
    ORCA_TRY(launch_conv1d_b16(ctx, D[1], prec, t1, bs, t2, bs, nullptr, B, no, 0));           // lout
    ORCA_TRY(launch_conv1d_b16(ctx, D[2], prec, t2, bs, t1, bs, nullptr, B, no, 1));
    ORCA_TRY(launch_conv1d_b16(ctx, D[3], prec, t1, bs, encs[lev], bs, t2, B, no, 1, 0, encs[lev]));   // + lout + skip, in place of the skip
    ORCA_TRY(hand_over(lev));
    cur = encs[lev];
  }
  return ORCA_OK;
}

extern "C" int orca_unet_forward(orca_ctx* ctx, orca_net* net, const float* x, int64_t sx_b, int64_t sx_c, int64_t sx_l, int B,
                                 int n, float* const* outs, int n_outs) {
  if (!ctx || !net || !x || !outs) return fail(ORCA_EINVAL, "orca_unet_forward: NULL argument");
  if (net->kind != ORCA_NET_ENCODER2 && net->kind != ORCA_NET_ENCODER3 && net->kind != ORCA_NET_ENCODER2B)
    return fail(ORCA_EINVAL, "orca_unet_forward: wrong net kind");
  HIPCHECK(hipSetDevice(ctx->device));
  const bool up_only = net->kind == ORCA_NET_ENCODER2B;   // Encoder2b: the contracting path IS the output
  const int nlev = net->kind == ORCA_NET_ENCODER3 ? 3 : 5;
  if (n_outs != nlev + 1) return fail(ORCA_EINVAL, "expected %d output pointers, got %d", nlev + 1, n_outs);
  if (n <= 0 || (n % (1 << nlev))) return fail(ORCA_EINVAL, "length %d not divisible by %d", n, 1 << nlev);
  if (B <= 0) return ORCA_OK;
  // Every precision but "f32" runs the channel-last split-operand path: levels of <= 2048 positions on conv_small.h (the K-chunks of a tile
  // side by side: ~7 us per launch where the exact fp32 kernel's latency chain took 31 - 28 of an Encoder2's 40 convs at 8 000 bins), the
  // longer ones on conv_bf16s.h.  65.6 against 66.4 ms per bench step (same box, alternating); until round 4 the exact fp32 kernels
  // served every precision below 32 000 positions per launch - which also made a row's bits depend on the batch it was computed in.
  if (net->precision != ORCA_PRECISION_F32) return unet_forward_nlc(ctx, net, x, sx_b, sx_c, sx_l, B, n, outs, nlev, up_only);
  const size_t full = (size_t)B * 128 * n;
  size_t need = 0;
  for (int i = 0; i < nlev; ++i) need += ru256((full >> i) * sizeof(float));  // encs[0..nlev-1]
  need += 3 * ru256(full * sizeof(float));
  ORCA_TRY(ws_ensure(ctx, need));
  std::vector<float*> encs(nlev + 1);
  for (int i = 0; i < nlev; ++i) encs[i] = up_only ? outs[i] : ws_take(ctx, full >> i);
  encs[nlev] = outs[nlev];
  float* t0 = ws_take(ctx, full);
  float* t1 = ws_take(ctx, full);
  float* t2 = ws_take(ctx, full);
  hipStream_t s = ctx->stream;
  // stage the (possibly strided) input as contiguous [B][128][n]
  for (int b = 0; b < B; ++b)
    ORCA_TRY(launch_copy2d(ctx, x + (long)b * sx_b, sx_c, sx_l, encs[0] + (size_t)b * 128 * n, n, 128, n));
  const ConvLayer* L = net->convs.data();
  // contracting path
  for (int i = 0; i < nlev; ++i) {
    const long ni = n >> i, no = n >> (i + 1);
    ORCA_TRY(launch_pool(ctx, encs[i], ni, t0, no, (long)B * 128, no, 2));
    const long bs = 128 * no;
    ORCA_TRY(launch_conv1d(ctx, L[4 * i + 0], t0, bs, no, t1, bs, no, nullptr, nullptr, B, no, 0, 0));
    ORCA_TRY(launch_conv1d(ctx, L[4 * i + 1], t1, bs, no, t2, bs, no, nullptr, nullptr, B, no, 0, 0));  // lout
    ORCA_TRY(launch_conv1d(ctx, L[4 * i + 2], t2, bs, no, t1, bs, no, nullptr, nullptr, B, no, 1, 0));
    ORCA_TRY(launch_conv1d(ctx, L[4 * i + 3], t1, bs, no, encs[i + 1], bs, no, t2, nullptr, B, no, 1, 0));
  }
  if (up_only) return ORCA_OK;
  // expanding path
  const float* cur = encs[nlev];
  for (int i = 0; i < nlev; ++i) {
    const int lev = nlev - 1 - i;
    const long ni = n >> (lev + 1), no = n >> lev;
    dim3 grid((unsigned)((no + 255) / 256), (unsigned)(B * 128));
    hipLaunchKernelGGL(upsample1d_x2_kernel, grid, dim3(256), 0, s, cur, ni, t0, no, no);
    LAUNCHCHECK("upsample1d_x2_kernel");
    const long bs = 128 * no;
    const ConvLayer* D = L + 4 * nlev + 4 * i;
    ORCA_TRY(launch_conv1d(ctx, D[0], t0, bs, no, t1, bs, no, nullptr, nullptr, B, no, 0, 0));
    ORCA_TRY(launch_conv1d(ctx, D[1], t1, bs, no, t2, bs, no, nullptr, nullptr, B, no, 0, 0));  // lout
    ORCA_TRY(launch_conv1d(ctx, D[2], t2, bs, no, t1, bs, no, nullptr, nullptr, B, no, 1, 0));
    ORCA_TRY(launch_conv1d(ctx, D[3], t1, bs, no, outs[lev], bs, no, t2, encs[lev], B, no, 1, 0));
    cur = outs[lev];
  }
  return ORCA_OK;
}

