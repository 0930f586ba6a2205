/*
 * orca_hip.h - C ABI of liborca_hip.so, the MI355X (gfx950) implementation of
 * the Orca hot path (Encoder -> Encoder2/Encoder3 -> Decoder cascade).
 *
 * The reference (jzhoulab/orca) has no FFI / plugin registry: the hot path is
 * reached through a duck-typed Python model protocol.
 * Each entry point below states which reference call it replaces; the Python
 * host in orca_amd/ binds them with ctypes (INTEGRATION.md shows the stub a
 * reference maintainer would add).
 *
 * Conventions
 *  - plain C types only; every function returns 0 (ORCA_OK) or a negative
 *    ORCA_E* code and records a message retrievable with orca_last_error()
 *    (thread-local).  No exceptions cross the boundary.
 *  - all `const float*` / `float*` data arguments are CALLER-OWNED DEVICE
 *    pointers (e.g. torch.Tensor.data_ptr() of a ROCm tensor) unless the
 *    parameter name ends in `_host`.
 *  - strides are in ELEMENTS (floats), so non-contiguous torch views (the
 *    `.transpose(1,2)` of orca_predict.py:334, the `[:, :, s:s+250]` slices of
 *    :358) are passed without a copy.
 *  - work is enqueued asynchronously on the HIP stream the context was
 *    created with (or was last given via orca_ctx_set_stream); the library
 *    never synchronises the device on the forward path.
 *  - the library owns only its weight copies (orca_net) and a per-context
 *    workspace that grows on demand.
 *  - one orca_ctx per (host thread, GPU).  No global mutable state.
 */
#ifndef ORCA_HIP_H
#define ORCA_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ORCA_OK 0
#define ORCA_EINVAL (-1)  /* bad argument / shape mismatch            */
#define ORCA_EHIP (-2)    /* a HIP runtime call failed                */
#define ORCA_ENOMEM (-3)  /* workspace / weight allocation failed     */
#define ORCA_ENODEV (-4)  /* no usable gfx950 device                  */

#define ORCA_ABI_VERSION 1

typedef struct orca_ctx orca_ctx;
typedef struct orca_net orca_net;

/* Which reference nn.Module an orca_net stands for. */
enum orca_net_kind {
  ORCA_NET_ENCODER = 1,    /* orca_modules.Encoder     (orca_modules.py:803-980)   */
  ORCA_NET_ENCODER2 = 2,   /* orca_modules.Encoder2    (orca_modules.py:984-1169)  */
  ORCA_NET_ENCODER3 = 3,   /* orca_modules.Encoder3    (orca_modules.py:1279-1406) */
  ORCA_NET_DECODER = 4,    /* orca_modules.Decoder     (orca_modules.py:16-488)    */
  ORCA_NET_DECODER_1M = 5, /* orca_modules.Decoder_1m  (orca_modules.py:491-800)   */
  ORCA_NET_ENCODER2B = 6   /* orca_modules.Encoder2b   (orca_modules.py:1173-1276): Encoder2 without the expanding path */
};

/* Decoder(upsample_mode=...) of orca_modules.py:17,430; containers use bilinear
 * (orca_models.py:45-50). */
#define ORCA_UPSAMPLE_NEAREST 0
#define ORCA_UPSAMPLE_BILINEAR 1

/* One convolution with eval-mode BatchNorm already folded into it on the host
 * (w' = w*gamma/sqrt(var+1e-5), b' = (b-mean)*gamma/sqrt(var+1e-5)+beta).
 * weight_host: [cout][cin][ksize] (1-D, ksize=9) or [cout][cin][ksize][ksize]
 * (2-D, ksize=3 or 1), fp32, row-major exactly as in the reference checkpoints
 * (`*.statedict`, orca_models.py:53-123). */
typedef struct orca_conv_desc {
  const float* weight_host;
  const float* bias_host;
  int32_t cout;
  int32_t cin;
  int32_t ksize;
  int32_t dilation;
} orca_conv_desc;

/* ---- library / context ------------------------------------------------- */

int orca_abi_version(void);
const char* orca_last_error(void);

/* Number of visible HIP devices (0 if none; never fails). */
int orca_device_count(void);

/* Replaces: implicit torch device/stream state used by `.cuda()` at
 * orca_predict.py:334.  hip_stream may be NULL (default stream). */
int orca_ctx_create(int device, void* hip_stream, orca_ctx** out);
int orca_ctx_destroy(orca_ctx* ctx);
int orca_ctx_set_stream(orca_ctx* ctx, void* hip_stream);
/* Bytes of device workspace currently held by the context. */
int orca_ctx_workspace_bytes(orca_ctx* ctx, size_t* out);
/* Free the workspace (it is re-grown on demand). */
int orca_ctx_release_workspace(orca_ctx* ctx);
/* Test entry: set every byte of the workspace arena and of the edge-fix scratch to `byte` (waits for the work in flight,
 * synchronises afterwards; the range flag and the zero page are left alone).  *filled = arena bytes + scratch bytes; an
 * empty arena is not an error.  A later call must compute what it would on any other contents (tests/test_gpu_arena.py). */
int orca_ctx_fill_workspace(orca_ctx* ctx, int byte, size_t* filled);

/* ---- per-kernel timing (bench.py roofline) ---------------------------------
 * When enabled, every conv1d launch over >= 65536 positions (the Encoder's
 * stage 1-4 convolutions, >96 % of the path's FLOPs) is bracketed by HIP events
 * on the context's stream.  orca_ctx_get_timing synchronises the stream, fills
 * up to `max` records (oldest first), stores the number available in *n and
 * clears the log. */
typedef struct orca_kernel_time {
  int32_t cout, cin, tile, batch; /* tile > 0: position tile of the exact-fp32 kernel; < 0: kernel family = -1..-4 conv_bf16s.h (bf16, bf16x2, bf16x3, f16x2),
                                   * -5 / -6 conv_p16.h (P16 / B16), -7 / -8 conv_ws.h, -9 / -10 conv_p16w1.h (P16 / B16), -12 / -13 conv_p16p5.h (P16 / B16), -14 conv_p16x.h */
  int64_t n;      /* positions per batch row            */
  float ms;       /* elapsed between the two HIP events */
  int32_t ksize;  /* taps of the launch: 9, or 17 = a composed linear pair (its algorithmic FLOPs are the pair's) */
} orca_kernel_time;
int orca_ctx_set_timing(orca_ctx* ctx, int enable);
int orca_ctx_get_timing(orca_ctx* ctx, orca_kernel_time* out, int max, int* n);

/* Launch counters of the context since its creation, counts4 = { channel-last Conv1d launches on the short-row kernel (conv_small.h:
 * rows of <= 2 048 positions), on the chunk-after-chunk kernel (conv_bf16s.h), planar P16 / B16 Conv1d launches, fused Decoder pair
 * launches }.  Diagnostics only (which kernel family a shard's short last stages ran on: bench.py's N-rank sections); no reference
 * counterpart. */
int orca_ctx_launch_counts(orca_ctx* ctx, int64_t* counts4);

/* ---- weights -------------------------------------------------------------
 * Replaces: nn.Module.load_state_dict + .cuda() of the reference containers
 * (orca_models.py:53-133).  `convs` lists the folded convolutions of the module
 * in forward order (documented per kind in DESIGN.md section "conv order");
 * shapes are validated against the architecture.  The library re-lays the
 * weights out for its MFMA kernels and keeps the device copy until
 * orca_net_free. */
int orca_net_create(orca_ctx* ctx, int kind, const orca_conv_desc* convs, int n_convs,
                    int upsample_mode, orca_net** out);
int orca_net_free(orca_net* net);

/* Arithmetic used for the Conv1d stacks of an Encoder net (Decoder / Decoder_1m nets take _F32, _F16X2 and _BF16).
 *  ORCA_PRECISION_F32   : v_mfma_f32_32x32x2_f32, exact fp32 products (default)
 *  ORCA_PRECISION_BF16X3: operands split into 3 bf16 parts, 6 bf16-MFMA products per fp32
 *                         product, fp32 accumulate - fp32-class error
 *                         at 2.67x the fp32-MFMA rate
 *  ORCA_PRECISION_BF16X2: 2-way split, 3 products (~2^-17 relative per product)
 *  ORCA_PRECISION_BF16  : plain bf16 operands, one product (the throughput mode of BASELINE config 3): Encoder stages 1-3
 *                         on single-plane bf16 activations (2 bytes per element in HBM, conv_p16.h "B16"), Decoders with
 *                         bf16 operands and fp32 feature maps */
#define ORCA_PRECISION_F32 0
#define ORCA_PRECISION_BF16 1
#define ORCA_PRECISION_BF16X2 2
#define ORCA_PRECISION_BF16X3 3
/*  ORCA_PRECISION_F16X2 : operands split into 2 fp16 parts (22 significant bits), 3 fp16-MFMA products,
 *                         fp32 accumulate: ~2^-22 relative error (fp32-class end to end) at 5.3x the
 *                         fp32-MFMA rate; requires |activation|, |weight| < 65504 (fp16 range). */
#define ORCA_PRECISION_F16X2 4
/*  ORCA_PRECISION_F16   : Decoder / Decoder_1m nets only - ONE fp16 plane per feature map and one MFMA product (the rate and
 *                         traffic of _BF16, 11 instead of 8 significant bits; fp16 range guard as _F16X2). */
#define ORCA_PRECISION_F16 5
int orca_net_set_precision(orca_net* net, int precision);
/* ORCA_NET_ENCODER only: which of the ALGEBRAICALLY EQUAL forms of stage 1-3's linear groups runs (orca_modules.py:811-852: `lconv_i` is
 * Conv-BN-Conv-BN with no nonlinearity, `conv_i`'s first conv is linear up to its ReLU; eval-mode BatchNorm is affine, so each group is ONE
 * convolution whose weights the library composes on the host in float64).  The default runs every composed form the weights allow; a group
 * whose composed weights leave the fp16 range keeps the reference's layer sequence by itself.  The other values FORCE a less composed form:
 * they exist so that the parity suite can run the fallbacks on ordinary weights and compare them with the default (tests/test_gpu_nets.py).
 *   _DEFAULT         lconv1 = 17 taps, conv1.a o lconv1 = 25 taps, both straight from the bases; with packed bases lout1 is computed in
 *                    conv1.b's epilogue (never stored); lconv2 / lconv3 = single 17-tap convs
 *   _STORED_RESIDUAL as _DEFAULT, lout1 written by a 17-tap first-layer launch and re-read (what float input rows get anyway)
 *   _LCONV1_ONLY     conv1.a stays a 64 -> 64 launch of its own
 *   _TWO_CONV        the reference's layer sequence, conv by conv */
#define ORCA_ENCODER_FORM_DEFAULT 0
#define ORCA_ENCODER_FORM_STORED_RESIDUAL 1
#define ORCA_ENCODER_FORM_LCONV1_ONLY 2
#define ORCA_ENCODER_FORM_TWO_CONV 3
int orca_net_set_encoder_form(orca_net* net, int form);
/* ORCA_NET_DECODER / _DECODER_1M only: with ORCA_PRECISION_F16X2 each run of residual blocks of dilation 16, 32, 64 is ONE launch
 * (conv2d_dblock_run_kernel, bit-identical to the three per-block launches); on by default, 0 = one launch per block.  The other precisions
 * always launch per block.  ORCA_EINVAL on any other net. */
int orca_net_set_decoder_block_runs(orca_net* net, int on);
/* ORCA_NET_ENCODER only: orca_encoder_forward_two_strands runs stages 3-7 of both strands as one joint pass (bit-identical to the two per-strand
 * calls); on by default, 0 = the two calls.  ORCA_EINVAL on any other net. */
int orca_net_set_encoder_two_strands(orca_net* net, int on);
int orca_net_get_encoder_two_strands(orca_net* net, int* on);
/* ORCA_PRECISION_F16X2 only: the kernels raise a device flag when an activation leaves the fp16
 * range (the result of that forward is then invalid).  This call waits for the context's stream,
 * returns the flag in *flag and clears it - the host falls back to ORCA_PRECISION_BF16X3. */
int orca_ctx_take_overflow(orca_ctx* ctx, int* flag);

/* ---- forward passes -------------------------------------------------------- */

/* Replaces: model.net0(x) = Encoder.forward (orca_modules.py:929-980).
 * x: [B,4,L] fp32 with element strides (sx_b,sx_c,sx_l); any float content
 * (one-hot rows, 0.25 'N' rows, ...).  Computes output bins [bin_lo,bin_hi)
 * (4000 bp each; bin_hi<=0 means "to the end") and writes
 * out[b*so_b + c*so_c + (bin-bin_lo)], c<128.  A sub-range is how the
 * independent sequence blocks shard across GPUs.
 * chunk_bp: internal processing chunk (multiple of 4000; <=0 = default: the whole input up to 32 Mb, 128 Mb chunks beyond - workspace = 768 B per chunk base);
 * chunks carry a 112 kb input halo each side exactly like the reference's
 * 800 kb blocks, so results do not depend on it. */
int orca_encoder_forward(orca_ctx* ctx, orca_net* net, const float* x, int64_t sx_b, int64_t sx_c,
                         int64_t sx_l, int B, int64_t L, int64_t bin_lo, int64_t bin_hi, float* out,
                         int64_t so_b, int64_t so_c, int64_t chunk_bp);

/* Packed-sequence input.  The reference materialises every window as a 512 MB float [L,4] array per strand
 * (selene_utils2.py:216-272) and a second, flipped copy for the reverse complement (orca_predict.py:324-329).
 * orca_pack_sequence turns a float view (device) into 1 byte per base - 0..3 = A,C,G,T one-hot rows, 4 = the
 * 0.25 x 4 'N' row - and reports *packable = 0 if some row is neither (the float path must then be used; it
 * synchronises the stream to return that flag).  orca_encoder_forward_codes runs the Encoder straight from the
 * codes ([B][L] bytes, batch stride sc_b); reverse != 0 encodes the REVERSE COMPLEMENT of the same buffer
 * (index L-1-i, code 3-c), so no second sequence copy ever exists.  The one-hot expansion happens in LDS inside
 * the first-layer kernel. */
int orca_pack_sequence(orca_ctx* ctx, const float* x, int64_t sx_c, int64_t sx_l, int64_t L, uint8_t* codes_out, int* packable);
int orca_encoder_forward_codes(orca_ctx* ctx, orca_net* net, const uint8_t* codes, int64_t sc_b, int reverse, int B, int64_t L,
                               int64_t bin_lo, int64_t bin_hi, float* out, int64_t so_b, int64_t so_c, int64_t chunk_bp);
/* The same from a WINDOW of the sequence: `codes` holds only bases [win_origin, win_origin + win_len) of the L-base
 * sequence (batch stride sc_b) - what a rank of a sharded run keeps of it: its bin range +- the 112 kb halo, i.e.
 * bases [bin_lo*4000 - 112000, bin_hi*4000 + 112000) for the forward strand and the mirror image
 * [L - bin_hi*4000 - 112000, L - bin_lo*4000 + 112000) for the reverse complement (clipped to [0, L)).  A window that
 * does not cover what the requested bins read is an error (ORCA_EINVAL), never a silent zero fill.
 * Replaces: the replicated `.cuda()` of the whole sequence per DataParallel replica (orca_predict.py:334, :675-683). */
int orca_encoder_forward_codes_window(orca_ctx* ctx, orca_net* net, const uint8_t* codes, int64_t sc_b, int64_t win_origin,
                                      int64_t win_len, int reverse, int B, int64_t L, int64_t bin_lo, int64_t bin_hi,
                                      float* out, int64_t so_b, int64_t so_c, int64_t chunk_bp);
/* The same from a 2-bit genome resident in HBM (selene_utils2.py:38-272 keeps the genome as text / expands every window to float32 [L,4]
 * on the host; orca_amd/genome.py TwoBitGenome: base j of a chromosome in bits 2 (j % 4).. of byte j / 4 of `two`, N flag in bit j % 8 of byte
 * j / 8 of `nmask`): the sequence is bases [start, start + L) of that chromosome (B = 1).  The first-layer kernels read the two planes
 * directly - the one-hot expansion happens in LDS as for the 1-byte codes - so no unpacked copy of the window exists. */
int orca_encoder_forward_2bit(orca_ctx* ctx, orca_net* net, const uint8_t* two, const uint8_t* nmask, int64_t start, int reverse, int64_t L,
                              int64_t bin_lo, int64_t bin_hi, float* out, int64_t so_c, int64_t chunk_bp);
/* Both strands of one packed sequence (`codes`: L bytes): the forward strand's bins into out_fwd[c * so_c + bin], the reverse complement's into
 * out_rev, exactly what orca_encoder_forward_codes with reverse = 0 / 1 writes (bit-identical, the fp16-range flag included).  With
 * ORCA_PRECISION_F16X2 / _BF16, the default form, L a multiple of 4000 and at most one chunk (32 Mb / $ORCA_ENCODER_CHUNK_BP) stages 1-2 run per
 * strand and stages 3-7 ONCE for both: the strands share one set of planes with a zero gap between them (stages 3-4) and run as a batch of two
 * rows (stages 5-7).  That costs a fourth workspace buffer of 6 L bytes x 2 (1.5 GB for 32 Mb).  Any other net state: the two per-strand calls. */
int orca_encoder_forward_two_strands(orca_ctx* ctx, orca_net* net, const uint8_t* codes, int64_t L, float* out_fwd, float* out_rev, int64_t so_c);

/* ---- the Encoder in two parts: structural-variant screens at arbitrary base positions ----------------------------
 * The reference's drivers place every window at the variant's own phase (orca_predict.py:1613: wpos = coord_clip(mstart) - no rounding to
 * the 4 kb grid) and push each 32 Mb window through the whole Encoder (orca_predict.py:231).  Stages 1-3 of the Encoder - 99 % of its work -
 * are translation-covariant on a 16-BASE grid (MaxPool1d(4) twice, orca_modules.py:829, :846) with a reach of 351 bases, so their output on a
 * chromosome, computed once per strand and per phase mod 16, serves every window of every allele made of pieces of that chromosome:
 * 512 bytes per base and strand of HBM (41 GB for both strands of a 40 Mb chromosome), against 24.6 ms of Encoder per strand and window.
 *   orca_encoder_stage3_planes  stage 3's output (ReLU + residual, BEFORE MaxPool1d(5)) of the L bases `codes` (reverse != 0: of their reverse
 *                               complement) as P16 planes: 32 planes (16 channel octets x {hi, lo} fp16 parts) of plane_units =
 *                               orca_p16_plane_units(L / 16) 16-byte units each, position j of the output at unit 8 + j of a plane.  L % 80 == 0.
 *   orca_p16_pool5_into         MaxPool1d(5) (orca_modules.py:853) of positions [src_pos0, src_pos0 + 5 count) of such planes into positions
 *                               [dst_pos0, dst_pos0 + count) of the planes of a stage-4 input (planes of dst_units units)
 *   orca_encoder_front_snippet  stages 1-3 + MaxPool1d(5) on bases [base0, base0 + nbases) of the L-base sequence `codes` (an allele window; both
 *                               ends of the snippet are treated as sequence ends, as the reference's zero padding treats a window's), pooled
 *                               positions [skip, skip + count) written to positions [dst_pos0, ..) of the stage-4 input: window ends and
 *                               junctions between pieces, where the cached values do not apply
 *   orca_encoder_back           stages 4-7 from a stage-4 input of n4 positions (n4 % 50 == 0; planes of s4_units = orca_p16_plane_units(n4)
 *                               units) -> out[c * so_c + bin], 128 x n4 / 50 bins
 * ORCA_PRECISION_F16X2 nets only (the planes are the operand image of that arithmetic); the fp16-range guard applies as everywhere. */
int64_t orca_p16_plane_units(int64_t n);
int orca_encoder_stage3_planes(orca_ctx* ctx, orca_net* net, const uint8_t* codes, int64_t L, int reverse, float* planes, int64_t plane_units);
int orca_p16_pool5_into(orca_ctx* ctx, const float* src, int64_t src_units, int64_t src_pos0, float* dst, int64_t dst_units, int64_t dst_pos0, int64_t count);
int orca_encoder_front_snippet(orca_ctx* ctx, orca_net* net, const uint8_t* codes, int64_t L, int reverse, int64_t base0, int64_t nbases, int64_t skip,
                               int64_t count, float* dst, int64_t dst_units, int64_t dst_pos0);
int orca_encoder_back(orca_ctx* ctx, orca_net* net, const float* s4, int64_t s4_units, int64_t n4, float* out, int64_t so_c);
/* One level further up (what sv.Stage4Cache keeps): stage 4 - 1.2 of the back's 2.0 ms per window strand - is covariant on the 80-BASE grid of its
 * input (MaxPool1d(5) behind stage 3) with a reach of 1 631 bases; its output as fp32 rows [n][128] per strand and phase mod 80 costs the same 512 bytes
 * per base and strand, and a window strand is then a MaxPool1d(5) gather of rows, the front + stage 4 on its ends and junctions, and stages 5-7.
 *   orca_encoder_stage4_rows     stage 4 alone: a stage-4 input of n4 positions (P16 planes, as for orca_encoder_back) -> rows[n4][128] (ReLU + residual,
 *                                before the MaxPool1d(5) in front of stage 5, orca_modules.py:866-872)
 *   orca_rows_pool5_into         MaxPool1d(5) of rows [src_pos0, src_pos0 + 5 count) of src[src_rows][128] into rows [dst_pos0, ..) of dst[dst_rows][128]
 *   orca_encoder_front4_snippet  stages 1-4 on bases [base0, base0 + nbases) (multiples of 400) of the L-base sequence `codes`, MaxPool1d(5); pooled rows
 *                                [skip, skip + count) -> rows [dst_pos0, ..) of the stage-5 input dst[dst_rows][128]
 *   orca_encoder_back5           stages 5-7 from a stage-5 input of n5 rows (n5 % 10 == 0) -> out[c * so_c + bin], 128 x n5 / 10 bins */
int orca_encoder_stage4_rows(orca_ctx* ctx, orca_net* net, const float* s4, int64_t s4_units, int64_t n4, float* rows);
int orca_rows_pool5_into(orca_ctx* ctx, const float* src, int64_t src_rows, int64_t src_pos0, float* dst, int64_t dst_rows, int64_t dst_pos0, int64_t count);
int orca_encoder_front4_snippet(orca_ctx* ctx, orca_net* net, const uint8_t* codes, int64_t L, int reverse, int64_t base0, int64_t nbases, int64_t skip,
                                int64_t count, float* dst, int64_t dst_rows, int64_t dst_pos0);
/* ... and for the snippets of one window strand CONCATENATED into one L-base sequence (the window's ends first and last): ranges_host = n_ranges triples
 * (skip, count, dst_pos0) of pooled rows of that one run. */
int orca_encoder_front4_ranges(orca_ctx* ctx, orca_net* net, const uint8_t* codes, int64_t L, int reverse, int n_ranges, const int64_t* ranges_host,
                               float* dst, int64_t dst_rows);
int orca_encoder_back5(orca_ctx* ctx, orca_net* net, const float* rows, int64_t n5, float* out, int64_t so_c);

/* The 1 Mb in-silico mutagenesis screen (orca_amd/screen.py): length-preserving edits of one window, each re-encoded through the front + stage 4
 * on a few kb around it and stages 5-7 on its own copy of the window's stage-5 rows, then Decoder_1m.  One launch per step for a whole batch.
 *   orca_screen_edit_codes    edited snippets of the L-base window `window` (device codes 0..4) packed back to back into out[total]: `table` (DEVICE,
 *                             n_snippets x 8 int64, in out_off order) = [out_off, b0, nb, kind, pos, len, pay_off, 0] per snippet: bases [b0, b0 + nb)
 *                             of the window with the span [pos, pos + len) substituted by payload[pay_off ..] (kind 0), set to N = 4 (kind 1) or
 *                             reverse-complemented in place (kind 2, N stays N).  Reads outside the window / payload give N.
 *   orca_screen_splice_rows   B stage-5 row images out[B][n5][128]: ref[n5][128] broadcast, rows [row_lo, row_lo + row_cnt) of image b replaced by rows
 *                             [src_row, ..) of fresh[n_fresh][128]; `table` (DEVICE, B x 3 int64) = [row_lo, row_cnt, src_row] per image
 *   orca_encoder_back5_batch  orca_encoder_back5 of B windows at once: rows [B][n5][128] (n5 % 10 == 0) -> out[b * so_b + c * so_c + bin]; each window
 *                             zero padded on its own; a window's result does not depend on B or on its place in the batch
 *   orca_screen_scores        B maps alt[b * map_bs + i * n + j] against ref[n][n]: profile[b][i] = mean_j |alt - ref|, mean[b] = mean over the map,
 *                             amax[b] = max |alt - ref| (sums in fp64; a NaN difference gives NaN) */
int orca_screen_edit_codes(orca_ctx* ctx, const uint8_t* window, int64_t L, const int64_t* table, int n_snippets, const uint8_t* payload, int64_t n_payload,
                           uint8_t* out, int64_t total);
int orca_screen_splice_rows(orca_ctx* ctx, const float* ref, int64_t n5, const float* fresh, int64_t n_fresh, const int64_t* table, int B, float* out);
int orca_encoder_back5_batch(orca_ctx* ctx, orca_net* net, const float* rows, int B, int64_t n5, float* out, int64_t so_b, int64_t so_c);
int orca_screen_scores(orca_ctx* ctx, const float* alt, int64_t map_bs, const float* ref, int B, int n, float* profile, float* mean, float* amax);

/* Compound edits (screen.EditSet: several disjoint spans applied together) and region scores.  Each small table is passed twice, the DEVICE copy the
 * kernel reads and a HOST copy with the same content that is checked here before anything is launched; a bad argument returns ORCA_EINVAL with the
 * cause in orca_last_error().  The kernels clip every table-derived index as well.
 *   orca_screen_edit_codes_multi   as orca_screen_edit_codes with any number of spans per snippet: `table` (n_snippets x 8 int64, out_off ascending from 0
 *                                  without gaps, ending at `total`) = [out_off, b0, nb, span_lo, span_cnt, 0, 0, 0]; `spans` (n_spans x 4 int64) =
 *                                  [kind, pos, len, pay_off]; spans [span_lo, span_lo + span_cnt) of a snippet are sorted by pos and pairwise disjoint,
 *                                  in window coordinates; a span may stick out of the snippet; an inversion reads the unedited window
 *   orca_screen_splice_rows_multi  as orca_screen_splice_rows with any number of row ranges per image: `segments` (n_segments x 3 int64) =
 *                                  [row_lo, row_cnt, src_row]; image b owns segments [seg_off[b], seg_off[b + 1]) (seg_off: B + 1 int64, monotone, from 0
 *                                  to n_segments), sorted by row_lo and disjoint
 *   orca_screen_region_scores      K rectangles (1..64) `rects` (K x 4 int32) = [i0, i1, j0, j1], half open, 0 <= i0 < i1 <= n and the same for j:
 *                                  mean_signed[b][k] = mean of alt - ref over rows [i0, i1) x columns [j0, j1) of map b, mean_abs[b][k] = mean of
 *                                  |alt - ref| (differences and sums in fp64; a NaN difference gives NaN in both) */
int orca_screen_edit_codes_multi(orca_ctx* ctx, const uint8_t* window, int64_t L, const int64_t* table, const int64_t* table_host, int n_snippets,
                                 const int64_t* spans, const int64_t* spans_host, int64_t n_spans, const uint8_t* payload, int64_t n_payload, uint8_t* out,
                                 int64_t total);
int orca_screen_splice_rows_multi(orca_ctx* ctx, const float* ref, int64_t n5, const float* fresh, int64_t n_fresh, const int64_t* segments,
                                  const int64_t* segments_host, int64_t n_segments, const int64_t* seg_off, const int64_t* seg_off_host, int B, float* out);
int orca_screen_region_scores(orca_ctx* ctx, const float* alt, int64_t map_bs, const float* ref, int B, int n, const int32_t* rects,
                              const int32_t* rects_host, int K, float* mean_signed, float* mean_abs);

/* Insertions and deletions (screen.Edit "del" / "ins").  The alt window of an item is a list of pieces in ALT coordinates over the CONTEXT, the window
 * followed by its right flank (C bases).  Tables come twice as above (device copy for the kernel, host copy checked here before any launch).
 *   orca_screen_assemble_codes  `table` (n_snippets x 8 int64, out_off ascending from 0 without gaps, ending at `total`) = [out_off, a0, nb, piece_lo,
 *                               piece_cnt, 0, 0, 0], a0 the snippet's first alt base; `pieces` (n_pieces x 4 int64) = [dst, kind, src, len], pieces
 *                               [piece_lo, piece_lo + piece_cnt) of a snippet sorted by dst and pairwise disjoint.  kind 0: context [src, src + len)
 *                               forward; 1: its reverse complement (N stays N); 2: payload [src, src + len); 3: N.  An alt base no piece covers and a
 *                               read past the context give N; a piece past the payload is refused.  One [0, L) snippet per item assembles whole windows
 *   orca_screen_gather_rows     B row images out[B][n5][128].  `segments` (n_segments x 4 int64) = [row_lo, row_cnt, source, src_row]; image b owns
 *                               segments [seg_off[b], seg_off[b + 1]), sorted by row_lo and disjoint.  source -1: rows [src_row, ..) of `fresh`; -2: rows
 *                               [src_row, ..) of `ref`; 0 <= p < P: row row_lo + t = MaxPool1d(5) of rows src_row + 5 t .. + 4 of phase entry p.
 *                               `entries`: DEVICE array of P pointers to [entry_rows[p]][128] float rows (16-byte aligned), `entry_rows` the counts
 *                               (device, and the host copy that is checked).  Rows in no segment are `ref` at their own index.  Pooled rows are bit for
 *                               bit orca_rows_pool5_into's */
int orca_screen_assemble_codes(orca_ctx* ctx, const uint8_t* context, int64_t C, const int64_t* table, const int64_t* table_host, int n_snippets,
                               const int64_t* pieces, const int64_t* pieces_host, int64_t n_pieces, const uint8_t* payload, int64_t n_payload, uint8_t* out,
                               int64_t total);
int orca_screen_gather_rows(orca_ctx* ctx, const float* ref, int64_t n5, const float* fresh, int64_t n_fresh, const float* const* entries,
                            const int64_t* entry_rows, const int64_t* entry_rows_host, int P, const int64_t* segments, const int64_t* segments_host,
                            int64_t n_segments, const int64_t* seg_off, const int64_t* seg_off_host, int B, float* out);

/* Aligned scores (screen.bin_map): behind an unbalanced insertion or deletion the alt map is displaced against ref, so alt bin i is compared with the
 * reference bin it stands for.  `bin_map` (B x n int32, n <= 256; device copy for the kernel, host copy checked here, as above): bin_map[b][i] = the
 * reference bin of alt bin i of map b, or -1 for none (inserted bases, refill); any value outside -1 .. n - 1 is refused (and reads as -1 in the kernel).
 * With M_b = {i : bin_map[b][i] >= 0}, c = |M_b| and d(i, j) = |alt[b][i][j] - ref[map i][map j]|, every result indexed by ALT bin:
 *   orca_screen_aligned_scores         profile[b][i] = sum_{j in M} d(i, j) / c (NaN for i outside M), mean[b] = sum_{i, j in M} d / c^2, amax[b] = max over
 *                                      M x M; all NaN when c = 0.  Differences and sums in fp64; a NaN at a mapped pair gives NaN, one at an unmapped
 *                                      pair is never read.  A map's results are bit for bit the same whatever B and its place in the batch
 *   orca_screen_aligned_region_scores  `rects` as for orca_screen_region_scores but in REFERENCE bins: rectangle k takes the alt pairs (i, j) with
 *                                      map i in [i0, i1) and map j in [j0, j1); mean_signed[b][k] = mean of alt[i][j] - ref[map i][map j], mean_abs[b][k]
 *                                      = mean of its absolute value; both NaN when no pair qualifies (the region was deleted) */
int orca_screen_aligned_scores(orca_ctx* ctx, const float* alt, int64_t map_bs, const float* ref, int B, int n, const int32_t* bin_map,
                               const int32_t* bin_map_host, float* profile, float* mean, float* amax);
int orca_screen_aligned_region_scores(orca_ctx* ctx, const float* alt, int64_t map_bs, const float* ref, int B, int n, const int32_t* bin_map,
                                      const int32_t* bin_map_host, const int32_t* rects, const int32_t* rects_host, int K, float* mean_signed,
                                      float* mean_abs);

/* Tracks (screen.screen_1m(..., insulation=, viewpoints=)): 1-D readouts of B maps alt[b * map_bs + i * n + j] (B >= 1, 1 <= n <= 256, map_bs >= n * n)
 * against ref[n][n], bin with bin and - with `bin_map` as above (device copy and checked host copy) - on aligned bins, indexed by ALT bin.  The small
 * tables `widths` (W int32, 1 <= W <= 8, each 1..128) and `views` (V int32, 1 <= V <= 64, each 0 .. n - 1) come twice like every table.  The diamond of
 * bin i at width w is rows [i - w, i) x columns (i, i + w]; it fits when w <= i < n - w, and ins_w(m)[i] = the mean of m over it (w^2 terms, fp64), NaN
 * where it does not fit (a width with 2 w + 1 > n is legal and gives NaN everywhere).  Each diamond is summed on its own, in an order fixed by (n, w).
 *   orca_screen_insulation  track[b][k][i] = ins_wk(alt b)[i]; delta[b][k][i] = ins(alt b)[i] - ins(ref)[i]; aligned[b][k][i] = ins(alt b)[i] -
 *                           ins(ref)[map i] where map i >= 0 and both diamonds fit, else NaN (only the centre bin has to be mapped; where map i == i it
 *                           is delta's expression, the same bits).  The differences are fp64, rounded once.  `delta` may be NULL; `aligned` is
 *                           non-NULL exactly when `bin_map` is; ref == NULL writes the track only (delta, aligned, bin_map NULL: the form for the
 *                           reference map itself, B = 1).  A NaN pixel shows in the bins whose diamond holds it and in no other
 *   orca_screen_viewpoints  delta[b][v][j] = alt[b][view v][j] - ref[view v][j] (fp32).  aligned[b][v][j]: the viewpoint is a REFERENCE bin, R = the alt
 *                           bins i with map i == view v (ascending), c = |R|: (sum_{i in R} alt[b][i][j]) / c - ref[view v][map j] in fp64 where c >= 1
 *                           and map j >= 0 (c = 1: the fp32 subtraction), else NaN.  `aligned` is non-NULL exactly when `bin_map` is
 * A map's results are bit for bit the same whatever B and its place in the batch.  Anything else is ORCA_EINVAL before any launch. */
int orca_screen_insulation(orca_ctx* ctx, const float* alt, int64_t map_bs, const float* ref, int B, int n, const int32_t* widths, const int32_t* widths_host,
                           int W, const int32_t* bin_map, const int32_t* bin_map_host, float* track, float* delta, float* aligned);
int orca_screen_viewpoints(orca_ctx* ctx, const float* alt, int64_t map_bs, const float* ref, int B, int n, const int32_t* views, const int32_t* views_host,
                           int V, const int32_t* bin_map, const int32_t* bin_map_host, float* delta, float* aligned);

/* Both strands (screen.screen_1m(..., strands="both")): B maps of the '+' strand fwd[b * fwd_bs + i * n + j] and of the '-' strand rev[b * rev_bs + ..]
 * (1 <= n <= 256, B >= 1, batch strides >= n * n) merged as genomepredict merges them (orca_predict.py:514-523):
 *   out[b][i][j] = 0.5f * fwd[b][i][j] + 0.5f * rev[b][n-1-i][n-1-j]     bit for bit orca_strand_merge on each map
 *   gap[b]       = mean_ij |(fwd[b] - ref_fwd)[i][j] - (rev[b] - ref_rev)[n-1-i][n-1-j]|   with the two strands' reference maps ref_fwd, ref_rev [n][n]:
 *                  how far the strands disagree about the item's effect.  Differences and sums in fp64 in an order fixed by n alone (no atomics): a
 *                  map's gap does not depend on B or on its place in the batch
 * gap == NULL or ref_fwd == NULL: only `out` is written and no reference is read (the form that merges the reference itself, B = 1).  A NaN propagates
 * into out and gap.  `out` may be `fwd` (every element is read and written by one thread); `rev` must not overlap `out`.  Anything else is ORCA_EINVAL
 * before any launch. */
int orca_screen_merge_strands(orca_ctx* ctx, const float* fwd, int64_t fwd_bs, const float* rev, int64_t rev_bs, const float* ref_fwd, const float* ref_rev,
                              int B, int n, float* out, int64_t out_bs, float* gap);

/* Non-additivity of edit sets (screen.epistasis_1m): B set maps alt[b * map_bs + i * n + j] against the sum of their members' effects.  `bank`
 * (bank[u * bank_bs + i * n + j], U >= 1 maps) holds the map of every single edit applied alone, ref[n][n] the unedited map (B, n >= 1, both batch
 * strides >= n * n).  The member table: set b has members members[member_off[b] .. member_off[b + 1]) - `member_off` B + 1 int64 from 0 to P, strictly
 * increasing (no empty set, no cap on a set's members), `members` P int32 bank indices in [0, U); each comes twice like every table (device copy for the
 * kernel, host copy checked here; the kernels clip all the same, and a clipped member reads as NaN).  Per pixel, every operand converted to fp64 first,
 * no multiplication:  t = sum_m (bank[member m] - ref), added sequentially for m ascending from 0.0 (the additive expectation);  r = (alt - ref) - t
 * (the residual; exactly +0.0 for a one-member set whose map holds its bank entry's bits).  Every result is rounded to fp32 once:
 *   orca_screen_epistasis_scores         profile[b][i] = mean_j |r[i][j]|, mean[b] = mean_ij |r|, amax[b] = max_ij |r|, add_mean[b] = mean_ij |t|.  fp64
 *                                        sums in an order fixed by n alone (no atomics): a set's bits depend neither on B nor on its place in the batch
 *   orca_screen_epistasis_region_scores  `rects` as for orca_screen_region_scores: mean_signed[b][k] = mean of r, mean_abs[b][k] = mean of |r| over
 *                                        rectangle k
 * A NaN in any map read propagates into the results it enters.  Anything else is ORCA_EINVAL before any launch. */
int orca_screen_epistasis_scores(orca_ctx* ctx, const float* alt, int64_t map_bs, const float* bank, int64_t bank_bs, int U, const float* ref, int B, int n,
                                 const int64_t* member_off, const int64_t* member_off_host, const int32_t* members, const int32_t* members_host, int64_t P,
                                 float* profile, float* mean, float* amax, float* add_mean);
int orca_screen_epistasis_region_scores(orca_ctx* ctx, const float* alt, int64_t map_bs, const float* bank, int64_t bank_bs, int U, const float* ref, int B,
                                        int n, const int64_t* member_off, const int64_t* member_off_host, const int32_t* members,
                                        const int32_t* members_host, int64_t P, const int32_t* rects, const int32_t* rects_host, int K, float* mean_signed,
                                        float* mean_abs);

/* Distance strata (screen.screen_1m(..., strata=)): how similar B maps alt[b * map_bs + i * n + j] (B >= 1, 1 <= n <= 256, map_bs >= n * n) are to
 * ref[n][n], stratified by genomic distance.  Stratum d (0 <= d < n) is the set of pairs (i, i + d): only the upper triangle, diagonal included, is ever
 * read (the screen's maps are symmetric).  For a pair, x = the alt pixel and y = the reference pixel, both converted to fp64 first.
 *   bin with bin (bin_map NULL)   P_d = all n - d pairs of stratum d, c_d = n - d, y = ref[i][i + d]
 *   aligned (`bin_map` as above: device copy and checked host copy, values outside -1 .. n - 1 refused)
 *                                 P_d = the pairs with map i >= 0 and map (i + d) >= 0, c_d = |P_d|, y = ref[map i][map (i + d)]: the stratum is the ALT
 *                                 distance, every result is indexed by alt bins, an unmapped pair is never read
 * Per stratum, two passes, each for i ascending from 0.0: (1) the means mx_d, my_d - the sequential sums, then one division by c_d; (2) the centred sums
 * X_d = sum (x - mx_d)^2, Y_d = sum (y - my_d)^2, C_d = sum (x - mx_d)(y - my_d) and, with dl = x - y, sum dl, sum |dl|, sum dl^2.
 * Per-stratum outputs [B][n]:
 *   dist_delta = sum dl / c_d,  dist_abs = sum |dl| / c_d,  dist_rms = sqrt(sum dl^2 / c_d)       fp32, rounded once
 *   dist_corr  = C_d / sqrt(X_d Y_d)                                                              fp64 (1 - r of a small edit has to survive); NaN when
 *                c_d < 2, X_d == 0.0 or Y_d == 0.0 - for a constant stratum the centred sums are exactly 0.0 (a sum of at most 256 equal fp32 values is
 *                exact in fp64, and so is its mean)
 *   dist_count = c_d (int32)                                                                      aligned only: non-NULL exactly when `bin_map` is
 *   every floating-point value of a stratum is NaN where c_d = 0
 * Per-map outputs [B], over the strata d_lo <= d < d_hi (0 <= d_lo < d_hi <= n) combined serially for d ascending, empty strata skipped, c = sum c_d:
 *   mse  = sum_d sum dl^2 / c                                                                     fp32
 *   scc  = sum_d C_d / sum_d sqrt(X_d Y_d)                                                        fp64; HiCRep's stratum-adjusted correlation: its
 *          weighting c_d sqrt(var_x var_y) of the per-stratum correlations, on raw values (no smoothing, no rank transform); NaN when the denominator is 0.0
 *   corr = C / sqrt(X Y)                                                                          fp64; the Pearson correlation over all pairs of those
 *          strata from the pooled centred sums: mx = (sum_d c_d mx_d) / c, X = sum_d [X_d + c_d (mx_d - mx)^2], C = sum_d [C_d + c_d (mx_d - mx)(my_d - my)],
 *          my and Y likewise; NaN when X or Y is 0.0 or c < 2
 *   all three are NaN when c = 0
 * A NaN pixel at a pair of P_d makes every output of stratum d NaN and, if d_lo <= d < d_hi, the three per-map scores; it affects nothing else, and one
 * below the diagonal or at an unmapped pair never shows.  Each stratum is summed by one thread in an order fixed by (n, the bin map) alone (no atomics):
 * a map's results are bit for bit the same whatever B and its place in the batch, and where the bin map is the identity they are the bin-with-bin bits.
 * `bin_map` and `bin_map_host` are NULL together.  Anything else is ORCA_EINVAL before any launch. */
int orca_screen_strata_scores(orca_ctx* ctx, const float* alt, int64_t map_bs, const float* ref, int B, int n, const int32_t* bin_map,
                              const int32_t* bin_map_host, int d_lo, int d_hi, float* dist_delta, float* dist_abs, float* dist_rms, double* dist_corr,
                              int32_t* dist_count, float* mse, double* corr, double* scc);

/* Paired aligned scores (sv.sv_screen(..., scores=), sv.sv_scores): B pairs of maps, alt[b * alt_bs + i * n + j] against a reference map OF ITS OWN
 * ref[b * ref_bs + ..] (B >= 1, 1 <= n <= 256, both batch strides >= n * n) through `bin_map` (B x n int32 as above: device copy for the kernel, checked
 * host copy; bin_map[b][i] = the reference bin alt bin i of pair b stands for, -1 for none, anything outside -1 .. n - 1 refused).  The map may ascend
 * with a jump (a deletion), repeat reference bins (a duplication's second copy) or descend (inside an inversion); every result is indexed by ALT bin.
 * With M = {i : map i >= 0}, c = |M|, and over the c^2 pairs (i, j) of M x M: x = alt[i][j], y = ref[map i][map j], dl = x - y, all in fp64:
 *   profile[b][i] = sum_j |dl| / c  (fp32; NaN for i outside M)        abs_mean[b]   = sum |dl| / c^2        abs_max[b] = max |dl|
 *   delta_mean[b] = sum dl / c^2                                       rms[b]        = sqrt(sum dl^2 / c^2)                          (fp32, rounded once)
 *   corr[b]       = C / sqrt(X Y)  (fp64: 1 - r of a small variant has to survive), the Pearson correlation over the c^2 pairs from two-pass centred
 *                   sums: the means mx = sum x / c^2, my = sum y / c^2 first, then X = sum (x - mx)^2, Y = sum (y - my)^2, C = sum (x - mx)(y - my);
 *                   NaN when c^2 < 2 or X or Y is exactly 0.0 (orca_screen_strata_scores' rule)
 *   count[b]      = c (int32)
 * Every floating-point output is NaN when c = 0.  A NaN pixel at a mapped pair makes that pair's scalar outputs and its row of `profile` NaN; one at an
 * unmapped pair is never read.  Sums in an order fixed by (n, the bin map) alone, no atomics: a pair's results are bit for bit the same whatever B, its
 * place in the batch and the strides.  Anything else is ORCA_EINVAL before any launch. */
int orca_screen_paired_aligned_scores(orca_ctx* ctx, const float* alt, int64_t alt_bs, const float* ref, int64_t ref_bs, int B, int n, const int32_t* bin_map,
                                      const int32_t* bin_map_host, float* profile, float* abs_mean, float* abs_max, float* delta_mean, float* rms, double* corr,
                                      int32_t* count);

/* Paired tracks and strata (sv.sv_screen(..., scores=True, insulation=, viewpoints=, strata=)): the three readouts above for B pairs of maps with the
 * conventions of orca_screen_paired_aligned_scores - pair b is alt + b * alt_bs against a reference map OF ITS OWN ref + b * ref_bs (B >= 1,
 * 1 <= n <= 256, both strides >= n * n) through row b of `bin_map` (B x n int32, -1 .. n - 1, required; it may ascend with jumps, repeat or descend).
 * Every small table comes twice (device copy, checked host copy), no pointer may be NULL, every result is indexed by ALT bin.
 *   orca_screen_paired_insulation     `widths` as for orca_screen_insulation (1 <= W <= 8, each 1..128; one that fits nowhere is legal).  [B][W][n]:
 *                                     track = ins_wk(alt b)[i];  ref_track = ins_wk(ref b)[i] at the reference's OWN bin i;  aligned = ins(alt b)[i] -
 *                                     ins(ref b)[map_b i] where map_b i >= 0 and both diamonds fit, else NaN (fp64 difference, rounded once).  The diamond
 *                                     and the order of its sum are orca_screen_insulation's: `track` of a map and `aligned` of an (alt, ref, map) hold the
 *                                     bits that entry point gives for them
 *   orca_screen_paired_viewpoints     `views` is B x V int32 (1 <= V <= 64), one list per pair, of REFERENCE bins -1 .. n - 1; -1 = "not in this pair's
 *                                     window".  R = the alt bins i with map_b i == view (ascending): count[b][v] = |R| (int32; 0 for view -1), and
 *                                     aligned[b][v][j] is orca_screen_viewpoints' aligned expression with the pair's own reference - the fp32 subtraction
 *                                     for c = 1, the fp64 mean over R minus ref_b[view][map_b j] for c > 1, NaN where c = 0 or map_b j < 0: the same bits
 *                                     as that entry point on the same inputs
 *   orca_screen_paired_strata_scores  the definitions, the two passes, the NaN rules and the serial combination over [d_lo, d_hi) (0 <= d_lo < d_hi <= n)
 *                                     of orca_screen_strata_scores' aligned form, with one difference: the reference pixel of alt pair (i, i + d) is
 *                                     ref_b[min(mi, mj)][max(mi, mj)], mi = map_b i, mj = map_b (i + d).  Inside an inversion the bin map descends and
 *                                     (mi, mj) lies below the reference's diagonal; a contact map is symmetric, so the mirrored pixel is the same contact,
 *                                     and nothing on the lower side of the diagonal of either map is ever read, whichever way the bin map runs.  Where
 *                                     the bin map is non-decreasing the results are orca_screen_strata_scores' bits
 * No atomics; every sum runs in an order fixed by (n, the table, the bin map) alone, so a pair's results are bit for bit the same whatever B, its place in
 * the batch and the strides.  Anything else is ORCA_EINVAL before any launch. */
int orca_screen_paired_insulation(orca_ctx* ctx, const float* alt, int64_t alt_bs, const float* ref, int64_t ref_bs, int B, int n, const int32_t* widths,
                                  const int32_t* widths_host, int W, const int32_t* bin_map, const int32_t* bin_map_host, float* track, float* ref_track,
                                  float* aligned);
int orca_screen_paired_viewpoints(orca_ctx* ctx, const float* alt, int64_t alt_bs, const float* ref, int64_t ref_bs, int B, int n, const int32_t* views,
                                  const int32_t* views_host, int V, const int32_t* bin_map, const int32_t* bin_map_host, float* aligned, int32_t* count);
int orca_screen_paired_strata_scores(orca_ctx* ctx, const float* alt, int64_t alt_bs, const float* ref, int64_t ref_bs, int B, int n, const int32_t* bin_map,
                                     const int32_t* bin_map_host, int d_lo, int d_hi, float* dist_delta, float* dist_abs, float* dist_rms, double* dist_corr,
                                     int32_t* dist_count, float* mse, double* corr, double* scc);

/* Loops(screen.screen_1m(..., loops=)): dot calls on B maps m = maps[b * map_bs + i * n + j] (B >= 1, 1 <= n <= 256, map_bs >= n * n) of log observed /
 * expected, where a focal peak's enrichment over its local background is a difference of means.  Integers 0 <= p < w <= 16, 1 <= r <= 16,
 * d_min >= 2 w + 1, 1 <= K <= 4096 and an fp32 threshold T (not NaN).
 *   eligible      pixel (i, j) with w <= i, j <= n - 1 - w and j - i >= d_min: every set below then lies inside the map and strictly above the diagonal;
 *                 the smallest map with an eligible pixel has n = 4 w + 2
 *   the sets      (HiCCUPS', Rao et al. 2014) of offsets (a, b) from (i, j), a along rows:
 *                 P  (peak)        |a| <= p and |b| <= p
 *                 D  (donut)       |a| <= w and |b| <= w, not in P, a != 0 and b != 0
 *                 LL (lower left)  1 <= a <= w and -w <= b <= -1, not in P: towards the diagonal
 *                 H                |a| <= 1 and p < |b| <= w
 *                 V                |b| <= 1 and p < |a| <= w
 *   enrichment    e(i, j) = mean P - max(mean D, mean LL, mean H, mean V).  Each set is summed on its own in fp64 (row by row over the window; no running
 *                 sums from pixel to pixel), one division by its count, no multiplication anywhere, the fp64 result rounded to fp32 once.  The sets cover
 *                 the window, so a NaN anywhere in the (2 w + 1)^2 window makes e NaN; e is NaN at every ineligible pixel; nothing on or below the
 *                 diagonal is read
 *   dot           (i, j) with e not NaN, e >= T, and for every pixel (i', j') within Chebyshev distance r whose e' is not NaN: e > e' where (i', j')
 *                 precedes (i, j) in row-major order, e >= e' where it follows.  fp32 comparisons; a NaN neighbour neither wins nor loses.  A constant
 *                 map with T = 0 has exactly one dot, (w, w + d_min)
 * orca_screen_dot_calls writes e_map[B][n][n] (caller-owned: the enrichment map, NaN where ineligible - the second launch reads it), count[B] (int32, ALL
 * dots of the map), and the first K dots in row-major order as ij[B][K][2] (int32, (i, j)) and enrich[B][K] (their e); the slots behind min(count, K) hold
 * -1 / NaN.  orca_screen_dot_enrichment writes out[B][Q] = e at the listed pixels[B][Q][2] (int32, 1 <= Q <= 4096; a device copy and a host copy,
 * coordinates outside -1 .. n - 1 refused): NaN for (-1, -1) and any other ineligible pixel, and otherwise the bits of e_map - one device function
 * computes both.  No atomics: a map's outputs are bit for bit the same whatever B, its place in the batch and the batch stride.  Anything else is
 * ORCA_EINVAL before any launch. */
int orca_screen_dot_calls(orca_ctx* ctx, const float* maps, int64_t map_bs, int B, int n, int p, int w, int d_min, int r, float T, int K, float* e_map,
                          int32_t* count, int32_t* ij, float* enrich);
int orca_screen_dot_enrichment(orca_ctx* ctx, const float* maps, int64_t map_bs, int B, int n, int p, int w, int d_min, const int32_t* pixels,
                               const int32_t* pixels_host, int Q, float* out);

/* Loops per level of the SV screen (sv.sv_screen(..., scores=True, loops=)): the reference dots of B pairs followed through each pair's bin map into the
 * alt map.  Everything about e - the sets, eligibility, what makes a pixel a dot, the list order and the truncation to K - is orca_screen_dot_calls': the
 * caller runs it on the reference maps and on the alt maps, and this entry point only gathers.
 *   alt_e        [B][n][n] at alt_e + b * e_bs (e_bs >= n * n): the enrichment map orca_screen_dot_calls wrote for the alt maps (NaN where ineligible)
 *   ref_ij       [B][R][2] int32 and ref_enrich [B][R]: the lists orca_screen_dot_calls wrote for the reference maps, ON THE DEVICE ONLY (1 <= R <= 4096).
 *                A slot that holds no dot - the -1 padding, or anything that does not satisfy 0 <= ri < rj <= n - 1 - is an EMPTY slot: it has no
 *                candidate and is never used as an index
 *   bin_map      B x n int32, -1 .. n - 1 (device copy and checked host copy), as in the other paired entry points; w, d_min: the calls' (1 <= w <= 16,
 *                d_min >= 2 w + 1)
 * For reference dot k = (ri, rj) of pair b: A = the alt bins a with map_b a = ri, C = the alt bins c with map_b c = rj (disjoint, ri != rj).  The
 * CANDIDATES are the pixels (min(a, c), max(a, c)) over A x C that are eligible in the alt map (w <= i, j <= n - 1 - w, j - i >= d_min).  The min/max is
 * the mirror rule of orca_screen_paired_strata_scores: inside an inversion the bin map descends, a contact map is symmetric, and nothing on or below a
 * diagonal is ever read.  The candidates are distinct pixels.  The chosen one is the best under one total order: a non-NaN e beats a NaN e, a larger e
 * beats a smaller one (fp32 comparison), and of two equals the earlier in row-major order wins - "does this loop survive anywhere in the allele".
 *   candidates[b][k] = their number (int32): 0 = an anchor is deleted, outside the alt window, or too near the diagonal or the edge; 1 = the ordinary
 *                      case; 2 to 4 under a tandem duplication
 *   at[b][k][2]      = the chosen pixel (i, j) (int32);  enrich[b][k] = alt_e there (its bits);  delta[b][k] = enrich[b][k] - ref_enrich[b][k], one fp32
 *                      subtraction (NaN propagates)
 * With no candidate, and in every empty slot: 0, (-1, -1), NaN, NaN.  Comparisons and one subtraction only, no atomics: a pair's outputs are bit for bit
 * the same whatever B, its place in the batch and the strides.  Anything else - a NULL pointer, a bin-map value outside -1 .. n - 1 - is ORCA_EINVAL
 * before any launch. */
int orca_screen_paired_dot_follow(orca_ctx* ctx, const float* alt_e, int64_t e_bs, int B, int n, int w, int d_min, const int32_t* ref_ij,
                                  const float* ref_enrich, int R, const int32_t* bin_map, const int32_t* bin_map_host, int32_t* candidates, int32_t* at,
                                  float* enrich, float* delta);

/* Compartments per level of the SV screen (sv.sv_screen(..., scores=True, compartments=)): the K leading eigenpairs of B maps, one map per workgroup.
 *   maps [B][n][n] float32 at maps + b * map_bs (map_bs >= n * n), 1 <= n <= 256, 1 <= K <= 3, 0 <= d_lo <= n - 1, center 0 / 1, tol > 0, max_iter >= 1,
 *   phase [B][n] float32 on the device or NULL.
 *   Outputs: E [B][K][n] float32, eigenvalue [B][K] float64, residual [B][K] float64, iterations [B][K] int32, n_valid [B] int32.
 * - Symmetrised input.  S[i][j] = M[min(i,j)][max(i,j)].  Only the upper triangle of a map is ever read, which is the rule of the strata and loop kernels.
 * - Kept pixels.  Pixel (i, j) is kept when |i - j| >= d_lo and both bins are valid.  Bin i is invalid when S[i][j] is NaN for some j with |i - j| >= d_lo.
 *   n_valid counts the valid bins.  If n_valid <= K, every output of that map is NaN (iterations is 0).
 * - The matrix A.  A[i][j] = S[i][j] - mu on kept pixels and 0 elsewhere.  mu is the fp64 mean of the kept pixels, summed in a fixed order.  mu is 0 when
 *   center is 0.
 * - Eigenpairs.  (lambda_k, v_k), k < K, are the eigenpairs of A in descending |lambda| with |v_k|_2 = 1.  They are computed in fp64, in a fixed order,
 *   without atomics.  Each is computed to relative residual |A v - lambda v|_2 / |lambda| <= tol, or until max_iter iterations.  residual reports the
 *   value reached.  A pair counts as converged when residual <= tol; it is never set to NaN merely for not converging.
 * - Scaling.  E_k = v_k * sqrt(|lambda_k|) (the cooltools convention).  E_k[i] is NaN on invalid bins.
 * - Sign.  With a phase track, the sign makes the fp64 Pearson correlation of E_k with the phase non-negative.  The correlation runs over valid bins
 *   whose phase is finite.  The fallback applies without a phase track, with fewer than 2 such bins, or with a zero or NaN correlation.  The component of
 *   largest |E_k| is made positive, lowest index on a tie.
 * - Batch independence.  A map's result does not depend on the batch it is in.  It is the same bits whether it is computed alone or among others.
 * The algorithm is deflated power iteration: for vector k, v starts at the valid bins i as (h >> 8) / 2^24 - 0.5 with the 32-bit hash h = (i + 1) *
 * 2654435761 + (k + 1) * 40503, h ^= h >> 15, h *= 2246822519, h ^= h >> 13; per iteration v is orthogonalised against v_0 .. v_{k-1} in turn
 * (Gram-Schmidt) and normalised, w = A v is orthogonalised likewise, lambda = v . w (the Rayleigh quotient), residual = |w - lambda v|_2 / |lambda|, and
 * v <- w unless the residual is <= tol or this was iteration max_iter (iterations reports the number done; lambda and the residual belong to the v that
 * is returned).  For k >= 1 the residual is that of w AFTER its orthogonalisation, i.e. of A restricted to the complement of v_0 .. v_{k-1}: the
 * residual of A itself is larger by at most sum_{j<k} residual_j |lambda_j| / |lambda_k|, the earlier vectors' own error.  residual is 0 where w - lambda v is exactly 0 - also with lambda = 0, the case of a map with no kept pixel apart from its mean - and
 * +inf where lambda = 0 otherwise.  Two eigenvalues of (nearly) equal |lambda| - a tied spectrum - do not converge: the pair is returned as it stands
 * after max_iter iterations with residual > tol.  The sign's correlation is taken as the sign of the centred cross sum C (two passes: the means, then
 * X, Y, C) when X > 0, Y > 0 and C is neither 0 nor NaN; "largest |E_k|" compares the fp32 values that are returned.  A is the packed upper triangle of
 * S in LDS (orca_amd/csrc/screen.h has the layout and the order of the sums).  Anything else - a NULL pointer other than phase, a bound above - is
 * ORCA_EINVAL before any launch. */
int orca_screen_eigenvectors(orca_ctx* ctx, const float* maps, int64_t map_bs, int B, int n, int K, int d_lo, int center, double tol, int max_iter,
                             const float* phase, float* E, double* eigenvalue, double* residual, int32_t* iterations, int32_t* n_valid);

/* GC content per bin of W windows of one code array - the phase track of the compartments.  codes [L] uint8 on the device, the project's codes: 0..3 = A,
 * C, G, T, 4 = N (anything above 3 counts as N); HOST arrays offsets [W] and binsizes [W] (int64); n = the bins per window (1..65535); out [W][n] float32.
 *   out[w][i] = float((double)#{C, G} / (double)#{A, C, G, T}) over the bases [off_w + i * bs_w, off_w + (i + 1) * bs_w); NaN when the bin holds no
 *   A/C/G/T.  The counts are integers, so the result is exact and independent of order.
 * A window that leaves [0, L) - off_w < 0, bs_w < 1 or off_w + n * bs_w > L - is refused with ORCA_EINVAL before any launch. */
int orca_screen_gc_tracks(orca_ctx* ctx, const uint8_t* codes, int64_t L, const int64_t* offsets, const int64_t* binsizes, int W, int n, float* out);

/* Domain boundary calls from insulation tracks (screen.screen_1m(..., insulation=, boundaries=), sv.sv_screen(..., insulation=, boundaries=)).
 *   tracks [B][W][n] float32 on the device, contiguous: tracks exactly as orca_screen_insulation / orca_screen_paired_insulation write them - lower = more
 *   insulated, NaN where the diamond does not fit or holds a NaN.  B >= 1, 1 <= W <= 8, 3 <= n <= 256, min_strength >= 0 (not NaN), 0 <= K <= n.
 *   Outputs: count [B][W] int32, bins [B][W][K] int32, strength [B][W][K] float32, strength_track [B][W][n] float32 or NULL.
 * - Minimum.  Bin i of a track t is a minimum when 1 <= i <= n - 2, t[i - 1], t[i] and t[i + 1] are all not NaN, t[i] < t[i - 1] and t[i] <= t[i + 1]:
 *   the first bin of a plateau.
 * - Strength.  The topographic prominence of the dip (scipy's peak_prominences on -t over the NaN-free run that holds i).  Walk left from i - 1 while the
 *   bin exists, is not NaN and is >= t[i]; L = the largest value met on that walk, or t[i] if none.  R = the same, walking right.
 *   strength = min(L, R) - t[i], ONE fp32 subtraction.  Only comparisons and that subtraction occur: a host restatement agrees bit for bit.  A NaN ends a
 *   run: nothing is bridged across it, so a dip beside a NaN bin is measured against its own side of the gap only.  The unit is the track's: mean log
 *   observed / expected.
 * - Call.  A minimum is a boundary when strength > 0 and strength >= min_strength.  A shelf such as 3 2 2 1 has strength 0 and is never a boundary.
 * - Lists.  The boundaries of a track in ascending bin order: bins / strength hold the first K, count ALL of them; unused slots hold -1 / NaN.
 *   strength_track[i] = the strength at every minimum with strength > 0 (whatever min_strength), NaN elsewhere.
 * - Batch independence.  A track's outputs are the same bits whatever B, W and its place among them; no atomics.
 * One workgroup of 256 threads per track on a grid of (B, W).  Anything else - a NULL pointer other than strength_track, a bound above - is ORCA_EINVAL
 * before any launch, and no output is written. */
int orca_screen_boundary_calls(orca_ctx* ctx, const float* tracks, int B, int W, int n, float min_strength, int K, int32_t* count, int32_t* bins,
                               float* strength, float* strength_track);

/* The chromosome scan (orca_amd/scan.py: scan_1m): a batch of overlapping window maps stitched into one banded map of a chromosome stretch, the band's
 * insulation tracks, and boundary strengths on tracks of any length.  Notation: the stretch has N bins (1 .. 2^24); a window map has n <= 256 bins and
 * window b starts at chromosome bin off[b]; the band has D distances, band[i][d] stands for pixel (i, i + d), 0 <= d < D.  Only the upper triangle
 * (row <= column) of a window map is ever read.  Plain HIP, no atomics, no workspace arena, a fixed summation order: results do not depend on how the
 * windows are batched.  Every launch goes to the context's stream.  A malformed call - a NULL pointer, a bound below - is ORCA_EINVAL before any launch, and
 * no buffer is written.
 *
 * orca_scan_stitch_band accumulates one batch of window maps into the band.
 *   maps [B][n][n] float32 on the device, batch stride map_bs >= n * n, rows contiguous; B >= 1, 1 <= n <= 256; n <= N.
 *   off [B] int64 on the device, off_host its host copy (checked here): strictly ascending, 0 <= off[b] <= N - n.
 *   trim >= 0 with n - 2 trim >= 1; 1 <= D <= n - 2 trim.
 *   Accumulators on the device: sum [N][D] float64, count [N][D] int32, lo [N][D] and hi [N][D] float32.  The caller starts them at sum = 0, count = 0,
 *   lo = +inf, hi = -inf.
 *   Rule: window b covers band pixel (i, d) when r = i - off[b] satisfies r >= trim and r + d <= n - 1 - trim.  For every covered pixel, with b ascending,
 *   v = maps[b][r][r + d]:  sum += (double) v;  count += 1;  lo = min(lo, v), hi = max(hi, v).  A NaN value makes sum, lo and hi of that pixel NaN, and they
 *   stay NaN.
 *   One thread per band pixel, d fastest; the launch covers rows off[0] .. off[B - 1] + n - 1 only.  Successive calls on one stream continue the same
 *   accumulators, so splitting a window list (ascending over all calls) into batches at any point gives the same bits as one call.
 *
 * orca_scan_band_finish turns the accumulators into results.
 *   band [N][D] float32 = (float)(sum / count), computed in fp64 and rounded once; NaN where count = 0, and where i + d >= N.
 *   range [N][D] float32 (or NULL) = hi - lo, one fp32 subtraction: 0 where one window covers the pixel, NaN where none does (and where i + d >= N).  It says
 *   how far the overlapping windows disagree about a pixel.  1 <= D <= 256.
 *
 * orca_scan_band_insulation computes insulation tracks from the band.
 *   band [N][D] float32; widths [W] int32 on the device, widths_host its host copy: 1 <= W <= 8, distinct, 1 <= w and 2 w + 1 <= D.  track [W][N] float32.
 *   track[k][i] = the fp64 mean, rounded once, of the w^2 pixels with rows r in [i - w, i) and columns c in (i, i + w], read as band[r][c - r].  NaN where
 *   the diamond does not fit (i < w or i >= N - w), and NaN if any pixel of the diamond is NaN: every diamond is summed on its own.  This is
 *   orca_screen_insulation's definition on the dense map the band stands for.  One wave per bin, lanes stride the diamond, then shuffles: the same bits on
 *   every run.
 *
 * orca_scan_boundary_strength computes boundary strengths on tracks of any length.
 *   tracks [W][N] float32 on the device, contiguous; 1 <= W <= 65535, N >= 1.  strength [W][N] float32.
 *   strength = orca_screen_boundary_calls' strength_track, without its limit of 256 bins: bin i is a minimum when 1 <= i <= N - 2, t[i - 1], t[i] and t[i + 1]
 *   are not NaN, t[i] < t[i - 1] and t[i] <= t[i + 1]; walk left from i - 1 while the bin exists, is not NaN and is >= t[i], L = the largest value met (t[i] if
 *   none), R the same to the right; s = min(L, R) - t[i], ONE fp32 subtraction; strength[i] = s where s > 0, NaN elsewhere.  A NaN ends a walk.  One thread per
 *   bin walks in global memory with its two running maxima in registers; the ordered lists are made on the host from this array. */
int orca_scan_stitch_band(orca_ctx* ctx, const float* maps, int64_t map_bs, int B, int n, const int64_t* off, const int64_t* off_host, int trim, int64_t N, int D,
                          double* sum, int32_t* count, float* lo, float* hi);
int orca_scan_band_finish(orca_ctx* ctx, const double* sum, const int32_t* count, const float* lo, const float* hi, int64_t N, int D, float* band, float* range);
int orca_scan_band_insulation(orca_ctx* ctx, const float* band, int64_t N, int D, const int32_t* widths, const int32_t* widths_host, int W, float* track);
int orca_scan_boundary_strength(orca_ctx* ctx, const float* tracks, int W, int64_t N, float* strength);

/* Loops along the scan (scan.scan_1m(..., loops=)): dot calls on the band itself, for a whole chromosome.  The band is band[N][D] float32 as
 * orca_scan_band_finish writes it: band[i][d] = pixel (i, i + d), NaN where uncovered or where i + d >= N; 1 <= N <= 2^24, 2 <= D <= 256.  Integers
 * 0 <= p < w <= 16, 1 <= r <= 16, d_min >= 2 w + 1 and an fp32 threshold T (not NaN), as for orca_screen_dot_calls.
 *   eligible      band pixel (i, d) with w <= i, i + d <= N - 1 - w and d_min <= d <= D - 1 - 2 w: every pixel of the (2 w + 1)^2 window then lies at a
 *                 distance in [d - 2 w, d + 2 w], inside [1, D - 1], and in a row in [0, N).  The smallest band with an eligible pixel has
 *                 D = d_min + 2 w + 1 and N = d_min + 2 w + 1
 *   enrichment    e[i][d] = orca_screen_dot_calls' e on the dense map the band stands for, at (i, i + d): its five sets, each summed on its own in fp64
 *                 (a ascending, then b ascending), one division per set, one rounding to fp32 - the same device function computes both, on the band as
 *                 an image of row stride D - 1 (dense pixel (i + a, i + d + b) is band[(i + a) * D + d + b - a]).  NaN when any window pixel is NaN,
 *                 NaN at every ineligible pixel
 *   dot           (i, d) with e not NaN, e >= T, and for every (di, dj) with |di|, |dj| <= r, not both 0, whose neighbour e' = e_band[i + di][d + dj - di]
 *                 exists (row in [0, N), distance in [0, D)) and is not NaN: e > e' where di < 0 or (di = 0 and dj < 0), e >= e' otherwise.  fp32
 *                 comparisons; orca_screen_dot_calls' rule - row-major order of (i, j) is row-major order of (i, d).  A constant band with T = 0 has exactly
 *                 one dot, (w, d_min)
 *   list          ALL dots in ascending (i, d) order, as ij[L][2] = (i, i + d) int64 and enrich[L] float32.  Nothing is capped: a chromosome has as many
 *                 loops as it has
 * orca_scan_band_dot_enrichment writes e_band[N][D], every element of it (one workgroup per 32 band rows, which it keeps in LDS with their 2 w halo
 * rows; a pixel's bits do not depend on the tiling).
 * orca_scan_band_dot_offsets writes row_start[N + 1] int64 from e_band: row_start[i] = the number of dots in rows < i, row_start[N] = L.  Two launches:
 * the rows' counts (one workgroup per row, ballots and popcounts) into row_start[0 .. N), then one workgroup turns them into the exclusive prefix in
 * place.
 * orca_scan_band_dot_list applies the same predicate again and writes dot k of row i, k counted within the row by ballot and popcount, to slot
 * row_start[i] + k of ij[cap][2] and enrich[cap]; cap = the L the caller read from row_start[N] (cap = 0: no launch).  Only slots in [0, cap) are ever
 * written, whatever row_start holds on the device.
 * No atomics, no workspace arena; the order of every sum and of the list is fixed.  Anything else - a NULL pointer, N < 1, D outside 2 .. 256, a
 * parameter outside its range, a NaN T, cap < 0 - is ORCA_EINVAL before any launch, and no buffer is written. */
int orca_scan_band_dot_enrichment(orca_ctx* ctx, const float* band, int64_t N, int D, int p, int w, int d_min, float* e_band);
int orca_scan_band_dot_offsets(orca_ctx* ctx, const float* e_band, int64_t N, int D, int r, float T, int64_t* row_start);
int orca_scan_band_dot_list(orca_ctx* ctx, const float* e_band, int64_t N, int D, int r, float T, const int64_t* row_start, int64_t cap, int64_t* ij,
                            float* enrich);

/* Number of 4 kb bins Encoder emits for an L-bp input (floor through the
 * 4,4,5,5,5,2 pooling chain). */
int64_t orca_encoder_num_bins(int64_t L);

/* Replaces: model.net(enc0) / model.net1(enc0) = Encoder2.forward
 * (orca_modules.py:1151-1169) and Encoder3.forward (:1388-1406).
 * x: [B,128,n] (strides in elements), n divisible by 2^nlev (nlev = 5 / 3).
 * An ORCA_NET_ENCODER2B net (Encoder2b.forward, :1262-1276; 5 levels) returns the contracting path's encodings.
 * outs: HOST array of nlev+1 device pointers; outs[i] receives the
 * contiguous [B,128,n>>i] encoding (fine -> coarse, as the reference returns).
 * Arithmetic: orca_net_set_precision (F32, F16X2, BF16X3, BF16X2, BF16).  The split-operand modes run on channel-last
 * activations from B*n >= 32000 positions on (the 256 Mb model's 64 000 bins); smaller problems use the exact fp32 kernels,
 * which are faster there, whatever the precision asked for. */
int orca_unet_forward(orca_ctx* ctx, orca_net* net, const float* x, int64_t sx_b, int64_t sx_c,
                      int64_t sx_l, int B, int n, float* const* outs_host, int n_outs);

/* Replaces: model.denets[level].forward(x, distenc, y) = Decoder.forward
 * (orca_modules.py:461-488).  x: [B,128,n] slice of an encoding (n<=256,
 * 250 in the reference); distenc: [B,1,n,n] log-background (sd_b may be 0
 * for the `.expand` of orca_predict.py:353); y: NULL or the [B,1,n/2,n/2]
 * crop of the coarser prediction (orca_predict.py:374-379).
 * out: contiguous [B,1,n,n].  accumulate!=0 adds into out instead of
 * overwriting (used for `+ denet_1_pt(...)`, orca_predict.py:362-366).
 * Streams: every launch of the call goes to the context's stream (a launch carries the whole batch; the call can be captured into a graph). */
int orca_decoder_forward(orca_ctx* ctx, orca_net* net, const float* x, int64_t sx_b, int64_t sx_c,
                         int64_t sx_l, const float* distenc, int64_t sd_b, int64_t sd_h, int64_t sd_w,
                         const float* y, int64_t sy_b, int64_t sy_h, int64_t sy_w, int B, int n,
                         float* out, int accumulate);

/* Multi-target decoders (orca_leukemia.py:512-990 `Decoder(num_2d)`, :996-1316 `Decoder_1m(num_2d)`; containers
 * OrcaLeukemiaA/B :1604-1873): the same network with T = num_2d maps per prediction - distenc [B,T,n,n], coarse y
 * [B,T,n/2,n/2], `final` 64 -> max(5,T) -> T, out contiguous [B,T,n,n].  T is taken from the width of the last
 * layer handed to orca_net_create (1 <= T <= 8).  Replaces: the same call site as orca_decoder_forward,
 * `model.denets[level].forward(x, distenc, y)` (orca_predict.py:356-379), for models whose normmats are 3-D. */
int orca_decoder_forward_mt(orca_ctx* ctx, orca_net* net, const float* x, int64_t sx_b, int64_t sx_c,
                            int64_t sx_l, const float* distenc, int64_t sd_b, int64_t sd_c, int64_t sd_h,
                            int64_t sd_w, const float* y, int64_t sy_b, int64_t sy_c, int64_t sy_h, int64_t sy_w,
                            int B, int n, float* out, int accumulate);

/* T (num_2d) of a Decoder / Decoder_1m net; 1 for every other kind. */
int orca_net_num_targets(orca_net* net, int* num_2d);

/* orca_decoder_forward_mt / orca_decoder1m_forward with ONE DEVICE POINTER PER BATCH ROW (host arrays of B pointers;
 * y_rows may be NULL) instead of a batch stride: the rows of a batch need not be slices of one tensor.  genomepredict
 * crops every strand's encoding (`[:, :, s:s+250]`) and coarse prediction (`[:, :, i:i+125, i:i+125]`) at the strand's
 * own offset (orca_predict.py:356-379); with row pointers the two strands go through every decoder level as one batch
 * without being copied next to each other first.  The pointer arrays are read during the call only. */
int orca_decoder_forward_rows(orca_ctx* ctx, orca_net* net, const float* const* x_rows, int64_t sx_c, int64_t sx_l,
                              const float* const* distenc_rows, int64_t sd_c, int64_t sd_h, int64_t sd_w,
                              const float* const* y_rows, int64_t sy_c, int64_t sy_h, int64_t sy_w, int B, int n,
                              float* out, int accumulate);
int orca_decoder1m_forward_rows(orca_ctx* ctx, orca_net* net, const float* const* x_rows, int64_t sx_c, int64_t sx_l,
                                int B, int n, float* out, int accumulate);

/* Replaces: model.denet_1_pt.forward(x) = Decoder_1m.forward (orca_modules.py:782-800); out [B,T,n,n]. */
int orca_decoder1m_forward(orca_ctx* ctx, orca_net* net, const float* x, int64_t sx_b, int64_t sx_c,
                           int64_t sx_l, int B, int n, float* out, int accumulate);

/* For tests: a Decoder / Decoder_1m forward (arguments of orca_decoder_forward_mt; a Decoder_1m takes distenc = y = NULL) that stops behind
 * the launches that complete `stage` and writes that feature map - decoded from its 16-bit planes, or copied from the fp32 planes of an
 * ORCA_PRECISION_F32 net - to map_out [B,channels,n,n] (contiguous).  It is the forward's own launch sequence with an early return.  Stages:
 *   0      IN: the Decoder's distenc chunk (T channels, then zeros; 16) / the Decoder_1m's x_i + x_j (128)
 *   1      after lcombinerD's first conv (Decoder; 64)
 *   2      A (Decoder): combinerD(.) + . in channels 0..63; with y 80 channels - the up-sampled y in 64..64+T-1, zeros to 79
 *   3 + i  the residual stream after block i (64): i < 28 (Decoder; block 0 = lcombiner / combiner with y) or i < 19 (Decoder_1m)
 * An ORCA_PRECISION_F32 net hands out what its fp32 maps hold: stage 0 of a Decoder is the WHOLE input map, 136 channels (x_i + x_j in
 * 0..127, distenc in 128..128+T-1, zeros to 135), and A with y has 72 (the up-sampled y in 64..64+T-1, zeros to 71); the rest as above.
 * ORCA_EINVAL: a stage the net kind does not have, `channels` other than the stage's. */
int orca_decoder_probe(orca_ctx* ctx, orca_net* net, const float* x, int64_t sx_b, int64_t sx_c, int64_t sx_l,
                       const float* distenc, int64_t sd_b, int64_t sd_c, int64_t sd_h, int64_t sd_w, const float* y,
                       int64_t sy_b, int64_t sy_c, int64_t sy_h, int64_t sy_w, int B, int n, int stage, int channels,
                       float* map_out);

/* For tests (export 76), the Encoder's counterpart of orca_decoder_probe: one chunk of ONE whole sequence of L bases (no halo, no bin range) through
 * stages 1..`stage` (1..7) of the route that orca_encoder_forward / _forward_codes take for this net - its precision and encoder form decide it, the
 * probe chooses no kernel: the same launches with the same arguments, fused pools and edge chains included, with an early return - and what that route
 * leaves behind the stage, copied to out as fp32 channel-last [*n_out][*channels] (64, 96, 128 channels for stages 1, 2, 3..7).  The input is either
 * packed codes (with `reverse`) or float rows x[c * sx_c + l * sx_l]; the other pointer is NULL.  *pool: the MaxPool1d the route has already applied
 * to that tensor (tails dropped), 1 = none:
 *   ORCA_PRECISION_F32               every stage unpooled (every pool is a launch of its own)
 *   ORCA_PRECISION_BF16X3 / _BF16X2  stages 1, 2 MaxPool1d(4)'d (fused into the last conv's epilogue), stages 3..7 unpooled
 *   ORCA_PRECISION_F16X2 / _BF16     stages 1, 2, 3 pooled by 4, 4, 5 (planes, decoded), stage 4 the fp32 rows of the hand-over and stages 5..7 unpooled
 * ORCA_EINVAL, before any launch: both or neither input, a stage whose input or whose returned tensor has no position left (stage 5 of 80 bases),
 * out_floats < *n_out x *channels (L x 64 floats always suffice).  The two-strand joint route is not probed. */
int orca_encoder_probe(orca_ctx* ctx, orca_net* net, const uint8_t* codes, int reverse, const float* x, int64_t sx_c, int64_t sx_l, int64_t L,
                       int stage, float* out, int64_t out_floats, int64_t* n_out, int* channels, int* pool);

/* Replaces: the strand merge `0.5*fwd + 0.5*rev[::-1, ::-1]`
 * (orca_predict.py:514-523) for contiguous [n,n] maps. */
int orca_strand_merge(orca_ctx* ctx, const float* fwd, const float* rev, float* out, int n);

/* Replaces: the per-level background of genomepredict_256Mb (orca_predict.py:724-737, :692-697, :703):
 *   normmat_r = np.nanmean(np.nanmean(np.reshape(normmat[s : s + 250 nb, s : s + 250 nb], (1, 250, nb, 250, nb)), axis=4), axis=2)
 *   distenc   = torch.log(torch.FloatTensor(normmat_r))        [torch.flip(distenc, [2, 3]) on the reverse strand]
 * on an 8000 x 8000 float64 background held in HBM (row stride ld, window origin (row0, col0), nb = level // 8 entries per
 * pixel side, npix = 250).  mean_out [npix][npix] float64 is BIT-IDENTICAL to numpy's result (same pairwise / sequential
 * summation order); log_out [npix][npix] float32 = logf of its float32 rounding, written flipped in both axes when
 * `flip`.  Either output may be NULL.  Device pointers. */
int orca_block_mean_f64(orca_ctx* ctx, const double* mat, int64_t ld, int64_t row0, int64_t col0, int nb, int npix,
                        double* mean_out, float* log_out, int flip);

/* Replaces: `adaptive_coarsegrain_gpu(ar, countar, cutoff, max_levels, min_shape)` (selene_utils2.py:274-463), the
 * 2x2-pooling smoother that `Genomic2DFeatures(cg=True)` applies to OBSERVED Hi-C matrices (:551-556) before they become
 * output["experiments"].  ar = balanced matrix (NaN = masked), countar = raw counts, both [n][n] fp32 device arrays with
 * row stride ld; out [n][n] (row stride ld_out), NaN at invalid pixels.  Bit-identical to the reference (same float32
 * operation order).  The reference's defaults: cutoff 5, max_levels 8 (12 through its wrapper), min_shape 8. */
int orca_adaptive_coarsegrain(orca_ctx* ctx, const float* ar, const float* countar, int64_t ld, int n, float cutoff,
                              int max_levels, int min_shape, float* out, int64_t ld_out);

/* Genome store, 2 bits per base + N bit-mask (replaces the float32 one-hot memmap of
 * selene_utils2.MemmapGenome, selene_utils2.py:38-272): expands the window [start, start+n) of a chromosome to the
 * 1-byte base codes orca_encoder_forward_codes reads (0..3 = A,C,G,T, 4 = N).  two_bit: base i in bits 2*(i%4).. of
 * byte i/4; nmask: base i in bit i%8 of byte i/8.  Device pointers. */
int orca_genome_unpack_2bit(orca_ctx* ctx, const uint8_t* two_bit, const uint8_t* nmask, int64_t start, int64_t n, uint8_t* codes);

/* ---- multi-GPU exchange ----------------------------------
 * The path shards at ONE place: the Encoder's 4 kb bins (bin_lo / bin_hi of orca_encoder_forward; blocks are
 * independent given the 112 kb input halo, orca_modules.py:955-977), followed by ONE all-gather of the per-rank
 * [B,128,bins] slabs before the replicated Encoder2 / Encoder3 / decoder tail.  Replaces: the `nn.DataParallel`
 * wrappers that are the reference's only multi-GPU mechanism (orca_models.py:44-50) around `model.net0(x)`
 * (orca_predict.py:334, :675-683).  One process per GPU; the communicator is RCCL over xGMI.
 *
 * RCCL is resolved at run time (dlopen; an RCCL already in the process - e.g. the one PyTorch-ROCm carries - is
 * preferred), so single-GPU users need no RCCL at all.  orca_comm_unique_id is called on ONE rank; the 128 bytes are
 * handed to every rank by the host's own channel (the Python host broadcasts them through torch.distributed's
 * store) and passed to orca_comm_init_rank, which is collective over the ranks. */
typedef struct orca_comm orca_comm;
#define ORCA_COMM_ID_BYTES 128
int orca_comm_unique_id(void* id128_host);
int orca_comm_init_rank(orca_ctx* ctx, int nranks, int rank, const void* id128_host, orca_comm** out);
int orca_comm_destroy(orca_comm* comm);
/* recv[r*count .. (r+1)*count) = rank r's send[0 .. count): fp32 device buffers, enqueued on the context's stream. */
int orca_allgather(orca_ctx* ctx, orca_comm* comm, const float* send, float* recv, size_t count);

/* Replaces: the kernel-size-1 Conv1d (+ folded BatchNorm) + activation layers of `Net.final_1d`, the auxiliary
 * 1-D head of the 1 Mb model (orca_modules.py:1824-1830, :1854).
 * y[b][co][m] = act(bias[co] + sum_ci w[co][ci] * x[b][ci][m]);  w [cout][cin] and bias [cout] are DEVICE memory
 * (folded on the host, uploaded once by the caller); x/y rows have stride ldx/ldy, batches x_bs/y_bs (elements).
 * act: 0 = identity, 1 = ReLU, 2 = sigmoid. */
int orca_pointwise1d_forward(orca_ctx* ctx, const float* w_dev, const float* bias_dev, int cout, int cin, const float* x,
                             int64_t x_bs, int64_t ldx, float* y, int64_t y_bs, int64_t ldy, int B, int64_t n, int act);

/* ---- single-layer entry points (kernel unit tests; same kernels the nets use) ---
 * y = [relu](conv1d_k9(x) + b) [+ r1] [+ r2], all [B,C,n] with row stride ld
 * (elements) and batch stride bs.  w/b as in orca_conv_desc (host, folded).
 * tile: 0 = auto, else force the position-tile size (32/64/256). */
int orca_conv1d_forward(orca_ctx* ctx, const orca_conv_desc* conv, const float* x, int64_t x_bs, int64_t ldx,
                        float* y, int64_t y_bs, int64_t ldy, const float* r1, const float* r2, int B, int64_t n,
                        int relu, int tile);
/* Channel-last variant on the 16-bit matrix cores with split operands (precision = ORCA_PRECISION_BF16 /
 * _BF16X2 / _BF16X3 / _F16X2): x [B][n][cin], y and r1 [B][n][cout], all contiguous; cin % 16 == 0. */
int orca_conv1d_nlc_forward(orca_ctx* ctx, const orca_conv_desc* conv, int precision, const float* x, float* y,
                            const float* r1, int B, int64_t n, int relu);
/* The same launcher with every argument the nets give it: r2 = a second residual [B][n][cout] (the U-net encoders' skip
 * connection; may be y itself - each element is read by the lane that then stores it), pool4 = 1 fuses MaxPool1d(4) into
 * the epilogue (y is [B][n/4][cout], a ragged last window is dropped, r1 stays [B][n][cout]; no r2 then),
 * fixed_tile = 0 / 1 / 2: the position tile of a long 128-cout layer by n and B / 256 positions whatever B is / what a
 * B = 1 call of n positions takes.  Batch strides are the contiguous ones.  ORCA_EINVAL, before any launch, on anything else. */
int orca_conv1d_nlc_forward_full(orca_ctx* ctx, const orca_conv_desc* conv, int precision, const float* x, float* y,
                                 const float* r1, const float* r2, int B, int64_t n, int relu, int pool4, int fixed_tile);
/* The P16 / LDS-DMA conv1d of the Encoder's stages 1-3 (conv_p16.h), wrapped for tests: channel-last fp32
 * in/out (x [n][cin], r1 [n][cout], y [n][cout] or, with out_mode 1 = fused MaxPool1d(4), [n/4][cout], with out_mode 3 = fused
 * MaxPool1d(5) (128 couts: conv_p16p5.h), [n/5][cout]);
 * out_mode 0/1 round-trip through the planar split-fp16 storage, out_mode 2 writes fp32 directly.
 * conv->ksize may be 9, or 17 with weight_host [cout][cin][17] - the form the Encoder's composed linear pairs
 * (Conv-BN-Conv-BN without a nonlinearity, orca_modules.py:829-835, 846-852) run as; cin % 32 == 0 then. */
int orca_conv1d_p16_forward(orca_ctx* ctx, const orca_conv_desc* conv, const float* x, float* y, const float* r1,
                            int64_t n, int relu, int out_mode);
/* The same kernel on "B16" activations - ONE bf16 plane per 8 channels, plain bf16 operands, one MFMA product,
 * 32 input channels per step (the ORCA_PRECISION_BF16 Encoder of BASELINE config 3); cin % 32 == 0.  Inputs
 * and outputs are rounded to bf16 on the way through the planar storage (out_mode 2 writes fp32). */
int orca_conv1d_b16_forward(orca_ctx* ctx, const orca_conv_desc* conv, const float* x, float* y, const float* r1,
                            int64_t n, int relu, int out_mode);
/* y = [relu](conv2d_3x3_dilated(x) + b) [+ r]; x: contiguous [B,cin,n,n], y/r: [B,cout,n,n]. */
int orca_conv2d_forward(orca_ctx* ctx, const orca_conv_desc* conv, const float* x, float* y, const float* r,
                        int B, int n, int relu);
/* The Decoders' 16-bit conv (conv2d_m16.h; precision ORCA_PRECISION_F16X2 / _BF16 / _F16; dilation 1..8), wrapped for
 * tests: contiguous [B,cin,n,n] in, [B,cout,n,n] out / residual; the maps make a round trip through the M16 storage
 * (two fp16 planes, or one bf16 / fp16 plane). */
int orca_conv2d_m16_forward(orca_ctx* ctx, const orca_conv_desc* conv, int precision, const float* x, float* y,
                            const float* r, int B, int n, int relu);
/* One whole residual block of the Decoders at dilation 16 / 32 / 64 (conv2d_dblock.h: cur += lm(cur); cur += m(cur), four 3x3 convs
 * 64 -> 32 -> 64 -> 32 -> 64 in one launch, in place), wrapped for tests: convs[4] = lm.a, lm.b, m.a, m.b (BN folded, ONE dilation of
 * 16, 32, 64), x and y contiguous [B,64,n,n], 1 <= n <= 256 (odd sizes included), precision ORCA_PRECISION_F16X2 / _BF16 / _F16; the map
 * makes a round trip through the M16 storage and the launch has the grid of the Decoder forward.  ORCA_EINVAL, before any launch, on
 * anything else. */
int orca_conv2d_dblock_forward(orca_ctx* ctx, const orca_conv_desc* convs, int precision, const float* x, float* y, int B, int n);
/* A run of nblk = 2 or 3 consecutive blocks of dilations d0, 2 d0 (, 4 d0) <= 64, wrapped for tests: convs[4 nblk] block by block as above,
 * precision ORCA_PRECISION_F16X2 only.  The map is converted to M16 ONCE, then fused != 0: one conv2d_dblock_run_kernel launch, fused == 0: nblk
 * conv2d_dblock_kernel launches on the same M16 buffer, and converted back once - the two must agree bit for bit. */
int orca_conv2d_dblock_run_forward(orca_ctx* ctx, const orca_conv_desc* convs, int nblk, int precision, const float* x, float* y, int B, int n,
                                   int fused);
/* y[c][m] = max_{j<k} x[c][k*m+j]  (nn.MaxPool1d(k,k)); x: [rows][ldx], y: [rows][ldy]. */
int orca_maxpool1d_forward(orca_ctx* ctx, const float* x, int64_t ldx, float* y, int64_t ldy, int64_t rows,
                           int64_t n_out, int k);

#ifdef __cplusplus
}
#endif
#endif /* ORCA_HIP_H */
