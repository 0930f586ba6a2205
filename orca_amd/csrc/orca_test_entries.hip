// orca_test_entries.hip - single-layer entry points (one conv / pool of the library on caller-owned tensors): what tests/test_gpu_kernels.py and the tools drive
// Part of liborca_hip.so (include/orca_hip.h is the ABI; orca_internal.h what the units share).
#include "orca_internal.h"

#include "conv_p16.h"        // nlc <-> P16 / B16 conversions
#include "conv2d_m16.h"      // nchw <-> M16 conversions
#include "misc_kernels.h"

// ---------------------------------------------------------------------------
// the arena's contents as a test input: no call may read arena or edge-scratch bytes it has not written itself (tests/test_gpu_arena.py)
// ---------------------------------------------------------------------------
extern "C" int orca_ctx_fill_workspace(orca_ctx* ctx, int byte, size_t* filled) {
  if (!ctx || !filled) return fail(ORCA_EINVAL, "orca_ctx_fill_workspace: NULL argument");
  HIPCHECK(hipSetDevice(ctx->device));
  if (ctx->ws_used && ctx->ws_stream != ctx->stream) HIPCHECK(hipStreamSynchronize(ctx->ws_stream));
  HIPCHECK(hipStreamSynchronize(ctx->stream));
  const size_t edge = 4 * (size_t)ORCA_EDGE_SLAB * sizeof(float);
  if (ctx->ws && ctx->ws_bytes) HIPCHECK(hipMemsetAsync(ctx->ws, byte, ctx->ws_bytes, ctx->stream));
  HIPCHECK(hipMemsetAsync(ctx->d_edge, byte, edge, ctx->stream));
  HIPCHECK(hipStreamSynchronize(ctx->stream));
  *filled = ctx->ws_bytes + edge;
  return ORCA_OK;
}

// ---------------------------------------------------------------------------
// single-layer entry points
// ---------------------------------------------------------------------------
extern "C" int orca_conv1d_forward(orca_ctx* ctx, const orca_conv_desc* conv, const float* x, int64_t x_bs, int64_t ldx, float* y,
                                   int64_t y_bs, int64_t ldy, const float* r1, const float* r2, int B, int64_t n, int relu,
                                   int tile) {
  if (!ctx || !conv || !x || !y) return fail(ORCA_EINVAL, "orca_conv1d_forward: NULL argument");
  HIPCHECK(hipSetDevice(ctx->device));
  ConvLayer L;
  ORCA_TRY(make_layer(*conv, &L));
  int rc = launch_conv1d(ctx, L, x, x_bs, ldx, y, y_bs, ldy, r1, r2, B, n, relu, tile);
  (void)hipStreamSynchronize(ctx->stream);
  free_layer(L);
  return rc;
}

extern "C" int orca_conv1d_nlc_forward(orca_ctx* ctx, const orca_conv_desc* conv, int precision, const float* x, float* y,
                                       const float* r1, int B, int64_t n, int relu) {
  if (!ctx || !conv || !x || !y) return fail(ORCA_EINVAL, "orca_conv1d_nlc_forward: NULL argument");
  if (precision < ORCA_PRECISION_BF16 || precision > ORCA_PRECISION_F16X2) return fail(ORCA_EINVAL, "precision %d unsupported here", precision);
  HIPCHECK(hipSetDevice(ctx->device));
  ConvLayer L;
  ORCA_TRY(make_layer(*conv, &L));
  int rc = launch_conv1d_b16(ctx, L, precision, x, (long)n * conv->cin, y, (long)n * conv->cout, r1, B, n, relu);
  (void)hipStreamSynchronize(ctx->stream);
  free_layer(L);
  return rc;
}

// the launcher as the nets call it: second residual (may be y), fused MaxPool1d(4), the tile rule of the long 128-cout layers
extern "C" int orca_conv1d_nlc_forward_full(orca_ctx* ctx, const orca_conv_desc* conv, int precision, const float* x, float* y,
                                            const float* r1, const float* r2, int B, int64_t n, int relu, int pool4, int fixed_tile) {
  if (!ctx || !conv || !x || !y) return fail(ORCA_EINVAL, "orca_conv1d_nlc_forward_full: NULL argument");
  if (precision < ORCA_PRECISION_BF16 || precision > ORCA_PRECISION_F16X2) return fail(ORCA_EINVAL, "precision %d unsupported here", precision);
  if (B <= 0 || B > 65535 || n < 0) return fail(ORCA_EINVAL, "orca_conv1d_nlc_forward_full: batch %d / length %ld unsupported", B, (long)n);
  if (pool4 < 0 || pool4 > 1 || fixed_tile < 0 || fixed_tile > 2) return fail(ORCA_EINVAL, "orca_conv1d_nlc_forward_full: pool4 %d (0, 1) / fixed_tile %d (0..2)", pool4, fixed_tile);
  if (pool4 && r2) return fail(ORCA_EINVAL, "orca_conv1d_nlc_forward_full: the pooled epilogue takes no second residual");
  if (conv->ksize != 9 || conv->cin % 16 || (conv->cout != 64 && conv->cout != 96 && conv->cout != 128))
    return fail(ORCA_EINVAL, "orca_conv1d_nlc_forward_full: %d taps, %d -> %d channels unsupported", conv->ksize, conv->cin, conv->cout);
  HIPCHECK(hipSetDevice(ctx->device));
  ConvLayer L;
  ORCA_TRY(make_layer(*conv, &L));
  const long nout = pool4 ? n / 4 : n;
  int rc = launch_conv1d_b16(ctx, L, precision, x, (long)n * conv->cin, y, nout * conv->cout, r1, B, n, relu, pool4, r2, fixed_tile);
  (void)hipStreamSynchronize(ctx->stream);
  free_layer(L);
  return rc;
}

static int conv1d_planar_test(orca_ctx* ctx, const orca_conv_desc* conv, const float* x, float* y, const float* r1, int64_t n, int relu,
                              int out_mode, int fmt) {
  if (!ctx || !conv || !x || !y) return fail(ORCA_EINVAL, "orca_conv1d_p16/b16_forward: NULL argument");
  HIPCHECK(hipSetDevice(ctx->device));
  ConvLayer L;
  if (conv->ksize == 17) {     // a 17-tap layer as the Encoder's composed pairs run it: weight_host [cout][cin][17]
    std::vector<double> w17((size_t)conv->cout * conv->cin * 17), b17(conv->cout);
    for (size_t i = 0; i < w17.size(); ++i) w17[i] = conv->weight_host[i];
    for (int i = 0; i < conv->cout; ++i) b17[i] = conv->bias_host[i];
    ORCA_TRY(make_layer17(conv->cin, conv->cout, w17, b17, &L));
  } else
  ORCA_TRY(make_layer(*conv, &L));
  const long nout = out_mode == 1 ? n / 4 : out_mode == 3 ? n / 5 : n;
  // the pooled-by-5 kernel's ragged last 320-position tile ends up to 303 units behind a plane (conv_p16p5.h), and its guard sees those lanes:
  // behind the LAST input (and residual) plane they get 512 zero units of the entry's own instead of whatever the arena holds there
  const size_t kSlack = 4 * 512;
  const size_t sx = (size_t)conv->cin * p16_plen(n), sy = (size_t)conv->cout * p16_plen(nout), sr = (size_t)conv->cout * p16_plen(n);
  int rc = ws_ensure(ctx, ru256((sx + kSlack) * 4) + ru256(sy * 4) + ru256((sr + kSlack) * 4));
  if (rc == ORCA_OK) {
    float* xp = ws_take(ctx, sx + kSlack);
    (void)hipMemsetAsync(xp + sx, 0, kSlack * sizeof(float), ctx->stream);
    float* yp = ws_take(ctx, sy);
    float* rp = ws_take(ctx, sr + kSlack);
    (void)hipMemsetAsync(rp + sr, 0, kSlack * sizeof(float), ctx->stream);
    hipStream_t s = ctx->stream;
    auto blocks = [](long n_, int C) { return dim3((unsigned)((n_ * (C / 4) + 255) / 256)); };
    auto to_planar = [&](const float* src, float* dst, int C) {
      if (fmt == 1) hipLaunchKernelGGL(nlc_to_b16_kernel, blocks(n, C), dim3(256), 0, s, src, reinterpret_cast<f32x4*>(dst), (long)n, C, p16_plen(n));
      else hipLaunchKernelGGL(nlc_to_p16_kernel, blocks(n, C), dim3(256), 0, s, src, reinterpret_cast<f32x4*>(dst), (long)n, C, p16_plen(n));
    };
    (void)launch_p16_zero_pads(ctx, xp, conv->cin, n, fmt);
    to_planar(x, xp, conv->cin);
    if (r1) {
      (void)launch_p16_zero_pads(ctx, rp, conv->cout, n, fmt);
      to_planar(r1, rp, conv->cout);
    }
    rc = launch_conv1d_p16(ctx, L, xp, out_mode == 2 ? (void*)y : (void*)yp, r1 ? rp : nullptr, n, relu, out_mode, nullptr, fmt);
    if (rc == ORCA_OK && out_mode != 2 && nout > 0) (void)launch_p16_zero_pads(ctx, yp, conv->cout, nout, fmt);   // as in the Encoder: pads after the producer
    if (rc == ORCA_OK && out_mode != 2 && nout > 0) {
      if (fmt == 1) hipLaunchKernelGGL(b16_to_nlc_kernel, blocks(nout, conv->cout), dim3(256), 0, s, reinterpret_cast<const f32x4*>(yp), y, nout, conv->cout, p16_plen(nout));
      else hipLaunchKernelGGL(p16_to_nlc_kernel, blocks(nout, conv->cout), dim3(256), 0, s, reinterpret_cast<const f32x4*>(yp), y, nout, conv->cout, p16_plen(nout));
    }
    hipError_t e = hipGetLastError();
    if (rc == ORCA_OK && e != hipSuccess) rc = fail(ORCA_EHIP, "planar conv test path: %s", hipGetErrorString(e));
  }
  (void)hipStreamSynchronize(ctx->stream);
  free_layer(L);
  return rc;
}

extern "C" int orca_conv1d_p16_forward(orca_ctx* ctx, const orca_conv_desc* conv, const float* x, float* y, const float* r1, int64_t n,
                                       int relu, int out_mode) {
  return conv1d_planar_test(ctx, conv, x, y, r1, n, relu, out_mode, 0);
}

extern "C" int orca_conv1d_b16_forward(orca_ctx* ctx, const orca_conv_desc* conv, const float* x, float* y, const float* r1, int64_t n,
                                       int relu, int out_mode) {
  if (conv && conv->cin % 32) return fail(ORCA_EINVAL, "orca_conv1d_b16_forward: cin %d is not a multiple of 32", conv->cin);
  return conv1d_planar_test(ctx, conv, x, y, r1, n, relu, out_mode, 1);
}

extern "C" int orca_conv2d_forward(orca_ctx* ctx, const orca_conv_desc* conv, const float* x, float* y, const float* r, int B,
                                   int n, int relu) {
  if (!ctx || !conv || !x || !y) return fail(ORCA_EINVAL, "orca_conv2d_forward: NULL argument");
  if (n <= 0 || n > ORCA_LDW) return fail(ORCA_EINVAL, "map size %d unsupported", n);
  HIPCHECK(hipSetDevice(ctx->device));
  ConvLayer L;
  ORCA_TRY(make_layer(*conv, &L));
  const int cpad = L.nchunks * 8;
  const size_t plane = (size_t)n * ORCA_LDW;
  int rc = ws_ensure(ctx, ru256(B * plane * cpad * 4) + 2 * ru256(B * plane * L.cout * 4));
  if (rc == ORCA_OK) {
    float* xp = ws_take(ctx, B * plane * cpad);
    float* yp = ws_take(ctx, B * plane * L.cout);
    float* rp = ws_take(ctx, B * plane * L.cout);
    hipStream_t s = ctx->stream;
    (void)hipMemsetAsync(xp, 0, B * plane * cpad * 4, s);
    for (int b = 0; b < B; ++b)
      hipLaunchKernelGGL(pad_rows_kernel, dim3((unsigned)(conv->cin * n)), dim3(ORCA_LDW), 0, s, x + (size_t)b * conv->cin * n * n,
                         xp + b * plane * cpad, n, 1);
    if (r) hipLaunchKernelGGL(pad_rows_kernel, dim3((unsigned)(B * L.cout * n)), dim3(ORCA_LDW), 0, s, r, rp, n, 1);
    rc = launch_conv2d(ctx, L, xp, plane * cpad, yp, plane * L.cout, r ? rp : nullptr, plane * L.cout, B, n, relu);
    if (rc == ORCA_OK) {
      hipLaunchKernelGGL(pad_rows_kernel, dim3((unsigned)(B * L.cout * n)), dim3(ORCA_LDW), 0, s, yp, y, n, 0);
      hipError_t e = hipGetLastError();
      if (e != hipSuccess) rc = fail(ORCA_EHIP, "pad_rows_kernel: %s", hipGetErrorString(e));
    }
  }
  (void)hipStreamSynchronize(ctx->stream);
  free_layer(L);
  return rc;
}

// single dilated 3x3 layer on M16 maps (conv2d_m16.h; dilations 1-8: launch_conv2d_m16 refuses larger ones, which only run as whole residual
// blocks - conv2d_dblock_test below)
template <int NS, int DT>
static int conv2d_m16_test(orca_ctx* ctx, const ConvLayer& L, int mode, const float* x, float* y, const float* r, int B, int n, int relu) {
  const int xo = 2 * ((L.cin + 15) / 16), yo = L.cout / 8;
  const size_t upo = (size_t)NS * n * ORCA_LDW;
  ORCA_TRY(ws_ensure(ctx, ru256(B * upo * xo * 16) + 2 * ru256(B * upo * yo * 16)));
  f32x4* xp = reinterpret_cast<f32x4*>(ws_take(ctx, B * upo * xo * 4));
  f32x4* yp = reinterpret_cast<f32x4*>(ws_take(ctx, B * upo * yo * 4));
  f32x4* rp = reinterpret_cast<f32x4*>(ws_take(ctx, B * upo * yo * 4));
  hipStream_t s = ctx->stream;
  for (int b = 0; b < B; ++b) {
    hipLaunchKernelGGL((nchw_to_m16_kernel<NS, DT>), dim3((unsigned)n), dim3(ORCA_LDW), 0, s, x + (size_t)b * L.cin * n * n, L.cin, n, xp + b * upo * xo, xo);
    if (r) hipLaunchKernelGGL((nchw_to_m16_kernel<NS, DT>), dim3((unsigned)n), dim3(ORCA_LDW), 0, s, r + (size_t)b * L.cout * n * n, L.cout, n, rp + b * upo * yo, yo);
  }
  ORCA_TRY(launch_conv2d_m16(ctx, L, xp, upo * xo, xo, yp, upo * yo, yo, r ? rp : nullptr, upo * yo, B, n, relu, mode));
  for (int b = 0; b < B; ++b)
    hipLaunchKernelGGL((m16_to_nchw_kernel<NS, DT>), dim3((unsigned)n), dim3(ORCA_LDW), 0, s, yp + b * upo * yo, L.cout, n, y + (size_t)b * L.cout * n * n);
  LAUNCHCHECK("conv2d_m16 test path");
  return ORCA_OK;
}

extern "C" int orca_conv2d_m16_forward(orca_ctx* ctx, const orca_conv_desc* conv, int precision, const float* x, float* y, const float* r,
                                       int B, int n, int relu) {
  if (!ctx || !conv || !x || !y) return fail(ORCA_EINVAL, "orca_conv2d_m16_forward: NULL argument");
  if (n <= 0 || n > ORCA_LDW) return fail(ORCA_EINVAL, "map size %d unsupported", n);
  HIPCHECK(hipSetDevice(ctx->device));
  ConvLayer L;
  ORCA_TRY(make_layer(*conv, &L));
  int rc;
  if (precision == ORCA_PRECISION_F16X2) rc = conv2d_m16_test<2, 1>(ctx, L, 0, x, y, r, B, n, relu);
  else if (precision == ORCA_PRECISION_BF16) rc = conv2d_m16_test<1, 0>(ctx, L, 1, x, y, r, B, n, relu);
  else if (precision == ORCA_PRECISION_F16) rc = conv2d_m16_test<1, 1>(ctx, L, 2, x, y, r, B, n, relu);
  else rc = fail(ORCA_EINVAL, "orca_conv2d_m16_forward: precision %d has no M16 kernel", precision);
  (void)hipStreamSynchronize(ctx->stream);
  free_layer(L);
  return rc;
}

// one whole residual block of dilation 16 / 32 / 64 (conv2d_dblock.h) on caller-owned maps: the launch of decoder_m16, grid included
template <int NS, int DT>
static int conv2d_dblock_test(orca_ctx* ctx, const ConvLayer* L, const float* x, float* y, int B, int n) {
  const size_t sz64 = (size_t)NS * n * ORCA_LDW * 8;
  ORCA_TRY(ws_ensure(ctx, ru256(B * sz64 * 16)));
  f32x4* cur = reinterpret_cast<f32x4*>(ws_take(ctx, B * sz64 * 4));
  hipStream_t s = ctx->stream;
  for (int b = 0; b < B; ++b)
    hipLaunchKernelGGL((nchw_to_m16_kernel<NS, DT>), dim3((unsigned)n), dim3(ORCA_LDW), 0, s, x + (size_t)b * 64 * n * n, 64, n, cur + b * sz64, 8);
  ORCA_TRY((launch_dblocks<NS, DT>(ctx, cur, (long)sz64, B, n, L, 1)));
  for (int b = 0; b < B; ++b)
    hipLaunchKernelGGL((m16_to_nchw_kernel<NS, DT>), dim3((unsigned)n), dim3(ORCA_LDW), 0, s, cur + b * sz64, 64, n, y + (size_t)b * 64 * n * n);
  LAUNCHCHECK("conv2d_dblock test path");
  return ORCA_OK;
}

extern "C" int orca_conv2d_dblock_forward(orca_ctx* ctx, const orca_conv_desc* convs, int precision, const float* x, float* y, int B, int n) {
  if (!ctx || !convs || !x || !y) return fail(ORCA_EINVAL, "orca_conv2d_dblock_forward: NULL argument");
  if (n <= 0 || n > ORCA_LDW || B <= 0 || B > 65535) return fail(ORCA_EINVAL, "orca_conv2d_dblock_forward: map size %d / batch %d unsupported", n, B);
  if (precision != ORCA_PRECISION_F16X2 && precision != ORCA_PRECISION_BF16 && precision != ORCA_PRECISION_F16)
    return fail(ORCA_EINVAL, "orca_conv2d_dblock_forward: precision %d has no block kernel", precision);
  const int d = convs[0].dilation;
  if (!(d == 16 || d == 32 || d == 64)) return fail(ORCA_EINVAL, "orca_conv2d_dblock_forward: dilation %d (16, 32 or 64)", d);
  for (int k = 0; k < 4; ++k) {
    const int cin = k & 1 ? 32 : 64, cout = k & 1 ? 64 : 32;
    if (convs[k].ksize != 3 || convs[k].cin != cin || convs[k].cout != cout || convs[k].dilation != d)
      return fail(ORCA_EINVAL, "orca_conv2d_dblock_forward: conv %d must be 3x3, %d -> %d, dilation %d", k, cin, cout, d);
  }
  HIPCHECK(hipSetDevice(ctx->device));
  ConvLayer L[4];
  int rc = ORCA_OK;
  for (int k = 0; k < 4 && rc == ORCA_OK; ++k) {
    rc = make_layer(convs[k], &L[k]);
    if (rc == ORCA_OK && precision != ORCA_PRECISION_BF16 && !L[k].f16_ok) rc = fail(ORCA_EINVAL, "layer weights exceed the fp16 range");
  }
  if (rc == ORCA_OK) {
    if (precision == ORCA_PRECISION_F16X2) rc = conv2d_dblock_test<2, 1>(ctx, L, x, y, B, n);
    else if (precision == ORCA_PRECISION_BF16) rc = conv2d_dblock_test<1, 0>(ctx, L, x, y, B, n);
    else rc = conv2d_dblock_test<1, 1>(ctx, L, x, y, B, n);
  }
  (void)hipStreamSynchronize(ctx->stream);
  for (int k = 0; k < 4; ++k) free_layer(L[k]);
  return rc;
}

// a run of nblk blocks (conv2d_dblock_run_kernel) against the chain of per-block launches, BOTH on one M16 buffer between one conversion in and one
// out: chained orca_conv2d_dblock_forward calls would re-split hi + lo through fp32 between the blocks, which can differ from the stored units by a
// rounding tie
extern "C" int orca_conv2d_dblock_run_forward(orca_ctx* ctx, const orca_conv_desc* convs, int nblk, int precision, const float* x, float* y, int B,
                                              int n, int fused) {
  if (!ctx || !convs || !x || !y) return fail(ORCA_EINVAL, "orca_conv2d_dblock_run_forward: NULL argument");
  if (n <= 0 || n > ORCA_LDW || B <= 0 || B > 65535) return fail(ORCA_EINVAL, "orca_conv2d_dblock_run_forward: map size %d / batch %d unsupported", n, B);
  if (precision != ORCA_PRECISION_F16X2) return fail(ORCA_EINVAL, "orca_conv2d_dblock_run_forward: precision %d has no run kernel (f16x2 only)", precision);
  if (nblk != 2 && nblk != 3) return fail(ORCA_EINVAL, "orca_conv2d_dblock_run_forward: %d blocks (2 or 3)", nblk);
  const int d0 = convs[0].dilation;
  if (!(d0 == 16 || d0 == 32) || (d0 << (nblk - 1)) > 64) return fail(ORCA_EINVAL, "orca_conv2d_dblock_run_forward: %d blocks from dilation %d (16, 32 (, 64) or 32, 64)", nblk, d0);
  for (int k = 0; k < 4 * nblk; ++k) {
    const int cin = k & 1 ? 32 : 64, cout = k & 1 ? 64 : 32, d = d0 << (k >> 2);
    if (convs[k].ksize != 3 || convs[k].cin != cin || convs[k].cout != cout || convs[k].dilation != d)
      return fail(ORCA_EINVAL, "orca_conv2d_dblock_run_forward: conv %d must be 3x3, %d -> %d, dilation %d", k, cin, cout, d);
  }
  HIPCHECK(hipSetDevice(ctx->device));
  ConvLayer L[12];
  int rc = ORCA_OK, made = 0;
  for (; made < 4 * nblk && rc == ORCA_OK; ++made) {
    rc = make_layer(convs[made], &L[made]);
    if (rc == ORCA_OK && !L[made].f16_ok) rc = fail(ORCA_EINVAL, "layer weights exceed the fp16 range");
  }
  const size_t sz64 = (size_t)2 * n * ORCA_LDW * 8;
  if (rc == ORCA_OK) rc = ws_ensure(ctx, ru256(B * sz64 * 16));
  if (rc == ORCA_OK) {
    f32x4* cur = reinterpret_cast<f32x4*>(ws_take(ctx, B * sz64 * 4));
    hipStream_t s = ctx->stream;
    for (int b = 0; b < B; ++b)
      hipLaunchKernelGGL((nchw_to_m16_kernel<2, 1>), dim3((unsigned)n), dim3(ORCA_LDW), 0, s, x + (size_t)b * 64 * n * n, 64, n, cur + b * sz64, 8);
    if (fused) rc = launch_dblocks<2, 1>(ctx, cur, (long)sz64, B, n, L, nblk);
    else
      for (int blk = 0; blk < nblk && rc == ORCA_OK; ++blk) rc = launch_dblocks<2, 1>(ctx, cur, (long)sz64, B, n, L + 4 * blk, 1);
    for (int b = 0; b < B; ++b)
      hipLaunchKernelGGL((m16_to_nchw_kernel<2, 1>), dim3((unsigned)n), dim3(ORCA_LDW), 0, s, cur + b * sz64, 64, n, y + (size_t)b * 64 * n * n);
    if (rc == ORCA_OK && hipGetLastError() != hipSuccess) rc = fail(ORCA_EHIP, "conv2d_dblock_run test path: launch failed");
  }
  (void)hipStreamSynchronize(ctx->stream);
  for (int k = 0; k < made; ++k) free_layer(L[k]);
  return rc;
}

extern "C" int orca_pointwise1d_forward(orca_ctx* ctx, const float* w_dev, const float* bias_dev, int cout, int cin, const float* x,
                                        int64_t x_bs, int64_t ldx, float* y, int64_t y_bs, int64_t ldy, int B, int64_t n, int act) {
  if (!ctx || !w_dev || !bias_dev || !x || !y) return fail(ORCA_EINVAL, "orca_pointwise1d_forward: NULL argument");
  if (cout <= 0 || cin <= 0 || B <= 0 || n < 0 || act < 0 || act > 2) return fail(ORCA_EINVAL, "orca_pointwise1d_forward: bad shape / activation");
  if (n == 0) return ORCA_OK;
  HIPCHECK(hipSetDevice(ctx->device));
  dim3 grid((unsigned)((n + 255) / 256), (unsigned)cout, (unsigned)B);
  hipLaunchKernelGGL(pointwise1d_kernel, grid, dim3(256), 0, ctx->stream, w_dev, bias_dev, cin, x, (long)x_bs, (long)ldx, y, (long)y_bs,
                     (long)ldy, (long)n, act);
  LAUNCHCHECK("pointwise1d_kernel");
  return ORCA_OK;
}

extern "C" int orca_maxpool1d_forward(orca_ctx* ctx, const float* x, int64_t ldx, float* y, int64_t ldy, int64_t rows,
                                      int64_t n_out, int k) {
  if (!ctx || !x || !y) return fail(ORCA_EINVAL, "orca_maxpool1d_forward: NULL argument");
  HIPCHECK(hipSetDevice(ctx->device));
  return launch_pool(ctx, x, ldx, y, ldy, rows, n_out, k);
}

