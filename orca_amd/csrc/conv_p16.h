// conv_p16.h - the Encoder's hot convolutions (stages 1-3, 96 % of its FLOPs) on "P16" activations.
//
// P16 = planar 2-way-split fp16 storage of an fp32 activation tensor [n][C]:
//     value(pos, ch) = hi + lo,   hi = fp16(v), lo = fp16(v - hi)            (22 significant bits)
//     plane (p = ch/8, s in {hi,lo}) is a contiguous array of 16-byte units, one unit per position holding the
//     8 channels 8p..8p+7;  unit(p, s, pos) at  base + ((2p + s) * PLEN + P16_GUARD + pos) * 16 bytes.
//   Same 4 bytes per element as fp32, but it IS the MFMA operand image: a conv's input tile is a set of
//   contiguous 16-byte runs that `global_load_lds` (LDS-DMA) drops straight into the LDS operand image - no
//   staging registers, no VALU conversion, no ds_write pass.  Each plane carries P16_GUARD (8) guard units on the left and
//   >= 24 on the right that are kept ZERO (p16_zero_pads_kernel + producers), so the conv's zero padding and the
//   ragged last tile need no predication at all.
//
// Kernel: persistent workgroups, 8 waves, (tile, chunk) stream as in conv_bf16s.h, but with TWO LDS buffers:
// the DMA of step s+1 is issued inside the MFMA block of step s and lands underneath it; one barrier per step.
// Arithmetic: 3 fp16 MFMA products per fp32 product (hi*hi + hi*lo + lo*hi), fp32 accumulate.
// Measured dead ends of this kernel (de-phased wave groups, parked-accumulator epilogue, one wave per SIMD, dedicated DMA
// waves, residual prefetch, segmented planes, ...) and the power-limit measurements are logged in DESIGN.md section 7.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "conv_bf16s.h"

#define P16_GUARD 8   // zero guard units on the left of every plane (>= 8 + 16 on the right): covers the 17-tap composed convs
#define P16_HALO 4    // half width of a k9 conv: image column i of a tile at m0 is position m0 + i - P16_HALO

// Base code (0..3 = A,C,G,T, 4 = N) of forward-strand base i of a sequence that is given either as 1 byte per base (`nmask` NULL) or as a
// window of a 2-bit genome (selene_utils2.py:216-222 expands such a store to float32 [L,4] on the host): `codes` is then the 2-bit plane -
// base j in bits 2 (j % 4) .. of byte j / 4 -, `nmask` the N bit mask - bit j % 8 of byte j / 8 -, j = origin + i (orca_amd/genome.py).
__device__ __forceinline__ int p16_base_at(const unsigned char* __restrict__ codes, const unsigned char* __restrict__ nmask, long origin, long i) {
  if (!nmask) return codes[i];
  const long j = origin + i;
  const unsigned c = (codes[j >> 2] >> ((j & 3) * 2)) & 3u;
  return ((nmask[j >> 3] >> (j & 7)) & 1u) ? 4 : (int)c;
}

struct ConvP16Args {
  const f32x4* x;      // P16 input, cin channels
  const f32x4* w;      // fp16 pack [cin/16][2][9][2][cout][8]  (units of 16 B)
  const float* bias;
  void* y;             // output: P16 (out_mode 0/1) or fp32 channel-last [n][cout] (out_mode 2)
  const f32x4* r1;     // optional residual, P16 with cout channels and the INPUT's plane length
  long x_plen, y_plen; // plane lengths (16-byte units) of x (and r1) / y
  long n;              // valid positions of x
  long tiles_per_row;  // ceil(n / MT)
  int nchunks;         // cin / 16
  int cout;            // total output channels (multiple of CT)
  int relu;
  int out_mode;        // 0: P16 same length; 1: P16 with MaxPool1d(4) fused (length n/4); 2: fp32 [n][cout]
  int k17;             // 17-tap conv (a composed linear pair, see orca_hip.hip: compose_pair) run as 2 * cin/16 k9 steps: step 2c + h
                       // covers taps 9h .. 9h+8 (tap 17 has zero weights) on the input shifted by 9h - 4 positions
  unsigned* flag;      // raised when a value written to P16 leaves the fp16 range
  unsigned long long* stamps;   // micro-benchmark only (ABL & 128): s_memtime stamps of workgroup 0 / wave 0
  // fused first layer (template flag F1): x is not read; the input tiles are PRODUCED from the packed bases
  const unsigned char* f1_codes;   // 1 byte per base of the whole sequence (see FirstMfmaArgs), or a 2-bit genome plane with
  const unsigned char* f1_nmask;   // ... its N mask (NULL: 1-byte codes) and the genome index of the sequence's base 0 (p16_base_at)
  long f1_origin;
  long f1_codes_L, f1_codes_off;   // chunk position p is strand position codes_off + p
  int f1_reverse;
  const f32x4* rl_w;               // RL: fp16 split pack [2 splits][5 k-steps][2 g][64 couts][8] of the composed 17-tap lconv1 (K = tap*4 + ci);
                                   //     its bias comes in f1_bias, the bases in f1_codes / f1_codes_L / f1_codes_off / f1_reverse
  const float* f1_table;           // [9 taps][4 K-chunks][6 codes][4 quads][4] fp32: folded first-layer weights per base code
                                   // (4 = N, 5 = padding); (code, quad) adjacent so the 16 lanes of a ds_read_b128 group -
                                   // 4 positions x 4 channel quads - hit 16 different 16-byte bank slots
  const float* f1_bias;            // [64] folded first-layer bias
};

__device__ __forceinline__ void p16_split_store(char* plane_hi, long plen_bytes, f32x4 v, bool valid, bool& ovf) {
  // 4 consecutive channels of one position -> 8 bytes in the hi plane and 8 bytes in the lo plane
  u32x2 sp[2];
  if (!valid) v = (f32x4)(0.f);
  split4<2, 1>(v, sp, ovf);
  *reinterpret_cast<u32x2*>(plane_hi) = sp[0];
  *reinterpret_cast<u32x2*>(plane_hi + plen_bytes) = sp[1];
}

typedef _Float16 f16x4 __attribute__((ext_vector_type(4)));
typedef unsigned int u32x4_t __attribute__((ext_vector_type(4)));
__device__ __forceinline__ f32x4 p16_load4(const char* plane_hi, long plen_bytes) {
  const f16x4 h = *reinterpret_cast<const f16x4*>(plane_hi), l = *reinterpret_cast<const f16x4*>(plane_hi + plen_bytes);
  f32x4 v;
  v.x = (float)h[0] + (float)l[0];
  v.y = (float)h[1] + (float)l[1];
  v.z = (float)h[2] + (float)l[2];
  v.w = (float)h[3] + (float)l[3];
  return v;
}

// 16-byte LDS-DMA: each lane supplies its own global address, the LDS destination is wave-uniform base +
// lane*16.  (The builtin only exists in the device pass; the host pass just needs the kernel to parse.)
__device__ __forceinline__ void p16_glds16(const f32x4* gsrc, f32x4* lds_wave_base) {
#if defined(__HIP_DEVICE_COMPILE__)
  __builtin_amdgcn_global_load_lds(gsrc, lds_wave_base, 16, 0, 0);
#else
  (void)gsrc; (void)lds_wave_base;
#endif
}

// 4 fp32 (one position, 4 consecutive couts) -> packed fp16 hi pair-of-pairs and lo = fp16(v - hi):
// 2 x v_cvt_pk_f16_f32 + 4 x v_fma_mix{lo,hi}_f16 (the f16 operand is widened inside the FMA; v - hi is exact in fp32)
__device__ __forceinline__ void p16_split_hl(const f32x4 v, unsigned& h0, unsigned& h1, unsigned& l0, unsigned& l1) {
#if defined(__HIP_DEVICE_COMPILE__)
  const float vx = v.x, vy = v.y, vz = v.z, vw = v.w;
  asm("v_cvt_pk_f16_f32 %0, %1, %2" : "=v"(h0) : "v"(vx), "v"(vy));
  asm("v_cvt_pk_f16_f32 %0, %1, %2" : "=v"(h1) : "v"(vz), "v"(vw));
  asm("v_fma_mixlo_f16 %0, %1, -1.0, %2 op_sel_hi:[1,0,0]" : "=v"(l0) : "v"(h0), "v"(vx));
  asm("v_fma_mixhi_f16 %0, %1, -1.0, %2 op_sel:[1,0,0] op_sel_hi:[1,0,0]" : "+v"(l0) : "v"(h0), "v"(vy));
  asm("v_fma_mixlo_f16 %0, %1, -1.0, %2 op_sel_hi:[1,0,0]" : "=v"(l1) : "v"(h1), "v"(vz));
  asm("v_fma_mixhi_f16 %0, %1, -1.0, %2 op_sel:[1,0,0] op_sel_hi:[1,0,0]" : "+v"(l1) : "v"(h1), "v"(vw));
#else
  (void)v; h0 = h1 = l0 = l1 = 0u;
#endif
}

// v_permlane32_swap: lanes 32..63 of `a` <-> lanes 0..31 of `b`
__device__ __forceinline__ void p16_swap32(unsigned& a, unsigned& b) {
#if defined(__HIP_DEVICE_COMPILE__)
  const u32x2 r = __builtin_amdgcn_permlane32_swap(a, b, false, false);
  a = r.x; b = r.y;
#endif
}

__device__ __forceinline__ float p16_dpp_quad_max(float v) {
#if defined(__HIP_DEVICE_COMPILE__)
  float t = __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, v), 0xB1, 0xf, 0xf, true));   // quad_perm [1,0,3,2]
  v = fmaxf(v, t);
  t = __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, v), 0x4E, 0xf, 0xf, true));         // quad_perm [2,3,0,1]
  v = fmaxf(v, t);
#endif
  return v;
}

// plain v_max_f32 / v_max3_f32: fmaxf() compiles to TWO instructions per value (a canonicalising v_max x,x in front of the
// real one - 128 instead of 64 VALU per tile epilogue), which the epilogue cannot afford: it runs with the matrix pipe idle
__device__ __forceinline__ float p16_vmax(float a, float b) {
  float r;
  asm("v_max_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
  return r;
}
__device__ __forceinline__ float p16_vmax3_abs(float m, float a, float b) {   // max(m, |a|, |b|)
  float r;
  asm("v_max3_f32 %0, |%1|, |%2|, %3" : "=v"(r) : "v"(a), "v"(b), "v"(m));
  return r;
}

// LDS operand reads the compiler cannot see.  While an LDS-DMA (`global_load_lds`) is in flight the compiler
// treats it as a pending FLAT access and turns EVERY lgkmcnt wait into lgkmcnt(0) - which also waits for the
// fragment prefetch issued a moment earlier and exposes the LDS latency once per two taps (~2 000 of a step's
// 9 800 cycles).  These reads are therefore issued from inline asm and retired by explicit counted waits
// (LDS returns in order): p16_lds_wait<N>() lets the N youngest reads stay in flight; the fragments it guards are
// in/out operands so that the MFMAs consuming them cannot be scheduled above the wait.
__device__ __forceinline__ unsigned p16_lds_addr(const void* p) {
  return (unsigned)(unsigned long)((__attribute__((address_space(3))) const char*)p);
}
__device__ __forceinline__ f16x8 p16_lds_read16(unsigned addr, const int off) {   // off: constant after unrolling
  f16x8 r;
  asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(r) : "v"(addr), "i"(off));
  return r;
}
__device__ __forceinline__ f32x4 p16_lds_read16f(unsigned addr, const int off) {   // off: constant after unrolling
  f32x4 r;
  asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(r) : "v"(addr), "i"(off));
  return r;
}
// LDS traffic of the fused-first-layer producer, all hidden from the compiler: with an LDS-DMA in flight it guards
// every LDS access it can see with s_waitcnt vmcnt(0) (possible alias with the DMA's destination) and the producer
// would wait out the W-chunk DMA in the middle of the MFMA block.  The regions are disjoint by construction.
__device__ __forceinline__ void p16_lds_read3(unsigned addr, unsigned& d0, unsigned& d1, unsigned& d2) {
  asm volatile("ds_read_b32 %0, %3\n\tds_read_b32 %1, %3 offset:4\n\tds_read_b32 %2, %3 offset:8\n\ts_waitcnt lgkmcnt(0)"
               : "=&v"(d0), "=&v"(d1), "=&v"(d2) : "v"(addr));
}
__device__ __forceinline__ void p16_lds_write8(unsigned addr, u32x2 v, const int off) {
  asm volatile("ds_write_b64 %0, %1 offset:%2" : : "v"(addr), "v"(v), "i"(off) : "memory");
}
__device__ __forceinline__ void p16_lds_wait0(f32x4& a, f32x4& b, f32x4& c) {
  asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(a), "+v"(b), "+v"(c));
}
template <int MW, int NW>
__device__ __forceinline__ void p16_f1_wait0(f16x8 (&a)[2][MW], f16x8 (&b)[2][NW], f32x4 (&r)[5]) {
  static_assert(MW == 2 && NW == 2, "fused first layer: 64 x 64 wave tile");
  asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(a[0][0]), "+v"(a[0][1]), "+v"(a[1][0]), "+v"(a[1][1]), "+v"(b[0][0]), "+v"(b[0][1]), "+v"(b[1][0]),
               "+v"(b[1][1]), "+v"(r[0]), "+v"(r[1]), "+v"(r[2]), "+v"(r[3]), "+v"(r[4]));
}
template <int N, int MW, int NW>
__device__ __forceinline__ void p16_lds_wait(f16x8 (&a)[2][MW], f16x8 (&b)[2][NW]) {
  static_assert(MW <= 2 && NW <= 3, "operand list below");
  if constexpr (MW == 2 && NW == 2)
    asm volatile("s_waitcnt lgkmcnt(%8)" : "+v"(a[0][0]), "+v"(a[0][1]), "+v"(a[1][0]), "+v"(a[1][1]), "+v"(b[0][0]), "+v"(b[0][1]), "+v"(b[1][0]), "+v"(b[1][1]) : "n"(N));
  else if constexpr (MW == 1 && NW == 3)
    asm volatile("s_waitcnt lgkmcnt(%8)" : "+v"(a[0][0]), "+v"(a[1][0]), "+v"(b[0][0]), "+v"(b[0][1]), "+v"(b[0][2]), "+v"(b[1][0]), "+v"(b[1][1]), "+v"(b[1][2]) : "n"(N));
  else if constexpr (MW == 1 && NW == 2)
    asm volatile("s_waitcnt lgkmcnt(%6)" : "+v"(a[0][0]), "+v"(a[1][0]), "+v"(b[0][0]), "+v"(b[0][1]), "+v"(b[1][0]), "+v"(b[1][1]) : "n"(N));
  else if constexpr (MW == 2 && NW == 1)
    asm volatile("s_waitcnt lgkmcnt(%6)" : "+v"(a[0][0]), "+v"(a[0][1]), "+v"(a[1][0]), "+v"(a[1][1]), "+v"(b[0][0]), "+v"(b[1][0]) : "n"(N));
  else
    static_assert(MW == 2 && NW == 2, "add the operand list for this wave tile");
}

// CT = couts per workgroup tile (cout blocks of CT are separate tiles), wave tile = MW x NW subtiles of 32x32.
// OM = out_mode, R1 = residual present: compile-time, the epilogue is branch-free.
// ABL (micro-benchmark only, 0 in the library): 1 = no DMA after the first step (64 / 256: only the W / X pieces are
// dropped), 2 = stores in a position-blocked plane order, 8 = LDS operands read once, 16 = no epilogue stores,
// 32 = stores folded into an L2-resident window, 128 = per-wave s_memtime stamps into a.stamps, 512 = epilogues of
// the upper half of the waves half a tile late (timing of a de-phased variant).
// Cost split of the 64 -> 64 conv at 32 M positions (5.89 ms): X DMA 11 %, W DMA 4 %, stores 7 % (half of it issue,
// half HBM), LDS operand reads ~7 %; with all DMA and stores off 4.65 ms (507 TFLOP/s-eq) at the higher clock that buys.
// K depth matters: 128 input channels (8 steps per tile) run at 440-460 TFLOP/s-eq against 380-400 for 64 (4 steps):
// the step that carries the epilogue costs ~1.8 plain steps more.
// s_memtime stamps (ABL & 128, tools/microbench_p16.hip) of the first version of this kernel, per step of
// ~12 000 cycles at the 1.8 GHz the part sustains here: MFMA block 6 700 (the pipe needs 6 912), epilogue 2 150
// (8 300 per tile - VALU- and store-issue-bound), DMA issue burst 1 440, vmcnt + barrier tail 3 000.  Hence:
//   * the accumulators start from the bias (16 ds_read_b128 per tile) instead of 0;
//   * hi/lo split in 6 instructions per 4 values (p16_split_hl), the range guard is a running v_max3;
//   * v_permlane32_swap pairs lanes l / l+32 (couts 4g..4g+3 of the same position) so that every lane stores - and
//     loads, for the residual - whole 16-byte units: half the VMEM instructions, uniform base + lane offset;
//   * MaxPool1d(4) on DPP quad permutes, the 4 lanes of a quad store one dword each of the pooled unit;
//   * the LDS-DMA of the next buffer is issued inside taps 0..4 of the MFMA block, two pieces per tap, instead of
//     as a burst in front of it (8 waves x 9 x 1 KB against the CU's 64 B/clk path).
//
// F1 (fused first layer; the conv right after it, 64 -> 64): the 16-channel input image of the next step is not
// DMA'd from a stored first-layer output but PRODUCED in place from the packed bases.  With one-hot input the 4 -> 64
// k9 convolution is a table sum, out[p][ch] = b[ch] + sum_t T[t][code(p + t - 4)][ch]  (T = the folded weights per base
// code: 13.8 KB of LDS), i.e. per step and thread 4 x (9 ds_read_b128 + 36 adds + hi/lo split + 2 ds_write_b64) - cheaper
// than the DMA of the same 33 KB (timing emulation: 5.07 vs 5.96 ms for 32 M positions) and the first-layer kernel with
// its 8 GB store / re-load of the 64-channel tensor disappears (2.4 ms per strand).
// FMT = 0: P16 (2-way split fp16, 3 products, 16 input channels per step).
// FMT = 1: "B16" - ONE bf16 plane per 8 channels (2 bytes per element, the throughput mode of BASELINE config 3), one
//   product, 32 input channels per step.  The LDS image of a step has the same shape in both formats - the split index
//   s of P16 becomes the k-pair index of B16 (channels 16 s + 8 g + e of the step's 32) - so the DMA geometry, the
//   fragment reads and the counted waits are shared; only the product list and the epilogue differ.
//   B16 planes: unit(p = ch/8, pos) at base + (p * PLEN + P16_GUARD + pos) * 16 bytes, guards as in P16.
//   B16 weight pack: [cin/32][2 k-pairs][9][2][cout][8] bf16.
// RL (conv1.b of stage 1, packed input): the residual `lout1` is not LOADED from a stored tensor but COMPUTED in the epilogue - lout1 is
//   the 17-tap composed conv of the bases (see conv1d_first_mfma_p16_kernel, NTAP = 17), i.e. per 32 x 32 accumulator tile a K = 80 GEMM of
//   the W17 pack (20 KB of LDS) with one-hot operand units built from the tile's base codes (544 bytes of LDS): 10 MFMAs per tile that
//   accumulate straight into the ReLU'd accumulators, in the part of the step where the matrix pipe used to idle.  The 17-tap first-layer
//   launch with its 8 GB store, and this kernel's 8 GB residual read, disappear.
template <int CT, int MW, int NW, int WM, int OM, bool R1, int ABL = 0, bool F1 = false, int FMT = 0, bool RL = false>
__global__ __launch_bounds__(WM * 64, WM / 4) void conv1d_k9_p16_kernel(ConvP16Args a) {
  static_assert(!RL || (CT == 64 && WM == 8 && MW == 2 && NW == 2 && !R1 && !F1), "residual from the bases: the 64 -> 64 planar conv of stage 1");
  static_assert(!F1 || (CT == 64 && WM == 8 && MW == 2), "fused first layer: 64-cout tiles of 512 positions");
  static_assert(!F1 || FMT == 0, "fused first layer: P16 only");
  static_assert(NW * 32 == CT, "one wave covers all couts of the tile");
  constexpr int NT = WM * 64;
  constexpr int MT = WM * MW * 32;
  constexpr int XROW = MT + 8;
  constexpr int XU = 2 * 2 * XROW;      // X image units  [s][g][XROW]
  constexpr int WU = 2 * 9 * 2 * CT;    // W image units  [s][tap][g][CT]
  constexpr int BU = XU + WU;           // one buffer
  constexpr int NIT = (BU + NT - 1) / NT;
  constexpr int DPT = (NIT + 4) / 5;    // DMA pieces per tap, taps 0..4
  constexpr int NG = MW * NW * 4;       // epilogue groups per wave: 1 position x 4 couts per lane
  __shared__ f32x4 smem[2 * BU + 32];   // + bias of all couts (<= 128 floats)

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int l31 = lane & 31, g = lane >> 5;
  const int ncb = a.cout / CT;                       // cout blocks
  const long ntiles = a.tiles_per_row * ncb;
  long tile = blockIdx.x;
  if (tile >= ntiles) return;
  // (cout block, position tile) of a tile index, carried incrementally: a 64-bit division per use is ~130 scalar instructions
  int tile_cb = 0;
  long tile_pos = tile;
  while (tile_pos >= a.tiles_per_row) { tile_pos -= a.tiles_per_row; ++tile_cb; }

  float* bias_s = reinterpret_cast<float*>(smem + 2 * BU);
  if (tid < a.cout) bias_s[tid] = a.bias[tid];   // visible after the first barrier
  constexpr int F1_WIN = 544;                          // bases a tile's producer looks at: positions m0-8 .. m0+MT+12 (528 used)
  __shared__ float f1_tab[F1 ? 9 * 6 * 64 : 4];
  __shared__ float f1_b[F1 ? 64 : 4];
  __shared__ unsigned char f1_win[F1 ? 2 * F1_WIN : 4];   // two tiles' windows
  if (F1) {
    for (int i = tid; i < 9 * 6 * 64; i += NT) f1_tab[i] = a.f1_table[i];
    if (tid < 64) f1_b[tid] = a.f1_bias[tid];
  }
  constexpr int RL_WIN = 544;                          // bases a tile's residual looks at: positions m0-8 .. m0+MT+11 (532 used)
  __shared__ f32x4 rl_ws[RL ? 2 * 5 * 2 * 64 : 1];
  __shared__ float rl_b[RL ? 64 : 4];
  __shared__ unsigned char rl_win[RL ? 2 * RL_WIN : 4];
  __shared__ u32x2 rl_oh[RL ? 8 : 1];                  // fp16 one-hot row per base code (4 = N = 0.25 x 4, 5 = zero row)
  if (RL) {
    for (int i = tid; i < 2 * 5 * 2 * 64; i += NT) rl_ws[i] = a.rl_w[i];
    if (tid < 64) rl_b[tid] = a.f1_bias[tid];
    if (tid < 8) {
      u32x2 v;
      v.x = tid == 0 ? 0x3C00u : tid == 1 ? 0x3C000000u : tid == 4 ? 0x34003400u : 0u;
      v.y = tid == 2 ? 0x3C00u : tid == 3 ? 0x3C000000u : tid == 4 ? 0x34003400u : 0u;
      rl_oh[tid] = v;
    }
  }
  // base code at chunk position p (5 = outside the chunk: the first layer's zero padding).  Split in two so that the
  // global load (f1_fetch) and the use of its result (f1_fix) can sit a whole step apart.
  auto f1_fetch = [&](long p) -> unsigned char {
    if (p < 0 || p >= a.n) return (unsigned char)5;
    const long P = a.f1_codes_off + p;
    return (unsigned char)p16_base_at(a.f1_codes, a.f1_nmask, a.f1_origin, a.f1_reverse ? a.f1_codes_L - 1 - P : P);
  };
  auto f1_fix = [&](unsigned char raw) -> unsigned char {
    int cc = raw;
    if (a.f1_reverse && cc < 4) cc = 3 - cc;
    return (unsigned char)(cc > 4 ? 5 : cc);
  };
  // Producer of one input position col i (0 .. XROW-1) of K-chunk `kc` of the tile at m0 -> buffer `buf`, in two parts
  // so that the work can be spread over the taps of the MFMA block: WINDOW decodes the 9 bases the position looks at
  // (3 aligned dwords of the window), QUAD computes 4 of the chunk's 16 channels.
#define P16_F1_WINDOW(i_, m0_, slot_, kc_)                                                                             \
  {                                                                                                                \
    const int ii_ = (i_) < XROW ? (i_) : 0;                                                                        \
    unsigned d0_, d1_, d2_;                                                                                        \
    p16_lds_read3(f1_win_lds + (slot_) * F1_WIN + (ii_ & ~3), d0_, d1_, d2_);                                      \
    const int sh_ = (ii_ & 3) * 8;                                                                                 \
    const unsigned long long lo_ = (((unsigned long long)d1_ << 32) | d0_) >> sh_;        /* bases i .. */          \
    const unsigned long long hi_ = (((unsigned long long)d2_ << 32) | d1_) >> sh_;        /* bases i+4 .. */        \
    _Pragma("unroll") for (int t_ = 0; t_ < 9; ++t_) {   /* byte offset of T[t][kc][code][0][0] */                 \
      const unsigned code_ = (unsigned)((t_ < 4 ? lo_ >> (8 * t_) : hi_ >> (8 * (t_ - 4))) & 0xff);                \
      f1_off[t_] = f1_tab_lds + (unsigned)(((t_ * 4 + (kc_)) * 6) * 64) + code_ * 64;                              \
    }                                                                                                              \
    const long p_ = (m0_) + ii_ - P16_HALO;                                                                       \
    f1_in = p_ >= 0 && p_ < a.n;                     /* else: this conv's own zero padding / ragged tail */         \
  }
#define P16_F1_QUAD(i_, quad_, kc_, buf_)                                                                          \
  if ((i_) < XROW) {                                                                                               \
    f32x4 v_ = p16_lds_read16f(f1_b_lds + 64 * (kc_), (quad_) * 16);          /* retired by the first wait below */ \
    /* the 9 table rows in 3 batches of 3 asm reads: left to the compiler, each read is followed by a full       \
       lgkmcnt(0) wait (it recycles one register quad) and a quad costs 9 LDS round trips */                     \
    _Pragma("unroll") for (int t_ = 0; t_ < 9; t_ += 3) {                                                          \
      f32x4 r0_ = p16_lds_read16f(f1_off[t_], (quad_) * 16), r1_ = p16_lds_read16f(f1_off[t_ + 1], (quad_) * 16),  \
            r2_ = p16_lds_read16f(f1_off[t_ + 2], (quad_) * 16);                                                   \
      p16_lds_wait0(r0_, r1_, r2_);                                                                                \
      v_ += r0_; v_ += r1_; v_ += r2_;                                                                             \
    }                                                                                                              \
    if (!f1_in) v_ = (f32x4)(0.f);                                                                                 \
    vmax = p16_vmax3_abs(p16_vmax3_abs(vmax, v_.x, v_.y), v_.z, v_.w);                                                     \
    unsigned h0_, h1_, l0_, l1_;                                                                                   \
    p16_split_hl(v_, h0_, h1_, l0_, l1_);                                                                          \
    const unsigned xd_ = smem_lds + (unsigned)((buf_) * BU * 16) + (unsigned)((i_) * 16);                          \
    u32x2 hh_, ll_;                                                                                                \
    hh_.x = h0_; hh_.y = h1_; ll_.x = l0_; ll_.y = l1_;                                                            \
    p16_lds_write8(xd_, hh_, ((quad_) >> 1) * XROW * 16 + ((quad_) & 1) * 8);                                      \
    p16_lds_write8(xd_, ll_, (2 + ((quad_) >> 1)) * XROW * 16 + ((quad_) & 1) * 8);                                \
  }
  // Software-pipelined form used inside the MFMA block: tap t ISSUES half a quad's table reads (5 LDS reads), tap t+1
  // CONSUMES them - by then they have landed behind the 12 MFMAs in between, so the producer never waits on LDS
  // (a 250-cycle round trip under load; done naively a quad is 4 of them and stalls the wave's MFMAs for a microsecond).
  // Half h of quad q: h = 0 -> bias + rows 0..3, h = 1 -> rows 4..8.  At most 8 + 5 + 2 LDS operations are in flight.
#define P16_F1_ISSUE(quad_, half_, kc_)                                                                            \
  if (!(ABL & 4096)) {                                                                                             \
    if ((half_) == 0) {                                                                                            \
      f1_r[0] = p16_lds_read16f(f1_b_lds + 64 * (kc_), (quad_) * 16);                                              \
      _Pragma("unroll") for (int t_ = 0; t_ < 4; ++t_) f1_r[1 + t_] = p16_lds_read16f(f1_off[t_], (quad_) * 16);   \
    } else {                                                                                                       \
      _Pragma("unroll") for (int t_ = 0; t_ < 5; ++t_) f1_r[t_] = p16_lds_read16f(f1_off[4 + t_], (quad_) * 16);   \
    }                                                                                                              \
  }
#define P16_F1_CONSUME(i_, quad_, half_, buf_)                                                                     \
  {                                                                                                                \
    if ((half_) == 0) f1_v = ((f1_r[0] + f1_r[1]) + (f1_r[2] + f1_r[3])) + f1_r[4];                                \
    else {                                                                                                         \
      f32x4 v_ = f1_v + (((f1_r[0] + f1_r[1]) + (f1_r[2] + f1_r[3])) + f1_r[4]);                                   \
      if (!f1_in) v_ = (f32x4)(0.f);                                                                               \
      vmax = p16_vmax3_abs(p16_vmax3_abs(vmax, v_.x, v_.y), v_.z, v_.w);                                                   \
      unsigned h0_, h1_, l0_, l1_;                                                                                 \
      p16_split_hl(v_, h0_, h1_, l0_, l1_);                                                                        \
      const unsigned xd_ = smem_lds + (unsigned)((buf_) * BU * 16) + (unsigned)((i_) * 16);                        \
      u32x2 hh_, ll_;                                                                                              \
      hh_.x = h0_; hh_.y = h1_; ll_.x = l0_; ll_.y = l1_;                                                          \
      if (ABL & 2048) { asm volatile("" ::"v"(hh_), "v"(ll_), "v"(xd_)); } else {                                  \
      p16_lds_write8(xd_, hh_, ((quad_) >> 1) * XROW * 16 + ((quad_) & 1) * 8);                                    \
      p16_lds_write8(xd_, ll_, (2 + ((quad_) >> 1)) * XROW * 16 + ((quad_) & 1) * 8);                              \
      }                                                                                                            \
    }                                                                                                              \
  }
  f32x4 f1_r[5], f1_v = (f32x4)(0.f);
#pragma unroll
  for (int k = 0; k < 5; ++k) f1_r[k] = (f32x4)(0.f);
  unsigned f1_off[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};      // LDS byte addresses of T[t][kc][code][0][0]
  const unsigned f1_tab_lds = p16_lds_addr(f1_tab), f1_b_lds = p16_lds_addr(f1_b), f1_win_lds = p16_lds_addr(f1_win), smem_lds = p16_lds_addr(smem);
  bool f1_in = false;

  // thread-constant DMA geometry (16-byte units): unit i = tid + it*NT of the buffer image
  int xrel[NIT];    // X: (g*2 + s) * x_plen + col        W: grp * cout + cc
  bool isx[NIT], act[NIT];
#pragma unroll
  for (int it = 0; it < NIT; ++it) {
    const int i = tid + it * NT;
    act[it] = i < BU;
    isx[it] = i < XU;
    if (isx[it]) {
      const int row = i / XROW, col = i - row * XROW;      // row = s*2 + g
      const int s = row >> 1, gg = row & 1;
      xrel[it] = (int)((FMT == 1 ? (s * 2 + gg) : (gg * 2 + s)) * a.x_plen) + col;
    } else {
      const int u = (i < BU ? i : BU - 1) - XU;
      const int grp = u / CT, cc = u - grp * CT;           // grp = (s*9 + tap)*2 + g
      xrel[it] = grp * a.cout + cc;
    }
  }
  const long wchunk = (long)2 * 9 * 2 * a.cout;            // units per K-chunk in the weight pack
  const f32x4 *xsrc = nullptr, *wsrc = nullptr;            // uniform sources of the (tile, chunk) being fetched
#define P16_SRC(cb, pos, c)                                                            \
  {                                                                                    \
    const int cx_ = a.k17 ? ((c) >> 1) : (c);                                          \
    const int xo_ = a.k17 ? (((c) & 1) ? 9 : 0) : (P16_GUARD - P16_HALO);              \
    xsrc = a.x + (long)cx_ * 4 * a.x_plen + (pos) * MT + xo_;                          \
    wsrc = a.w + (long)(c) * wchunk + (cb) * CT;                                       \
  }
#define P16_DMA_ONE(it, buf) \
  if (act[it] && !(F1 && isx[it])) p16_glds16((isx[it] ? xsrc : wsrc) + xrel[it], smem + (buf) * BU + (it) * NT + wave * 64);

  // accumulators start from the bias of the tile's cout block
  f32x16 acc[MW][NW];
#define P16_ACC_INIT(cb)                                                                                      \
  {                                                                                                           \
    const int co0_ = (cb) * CT + 4 * g;                                                                       \
    _Pragma("unroll") for (int j = 0; j < NW; ++j) _Pragma("unroll") for (int q = 0; q < 4; ++q) {            \
      const f32x4 b_ = *reinterpret_cast<const f32x4*>(bias_s + co0_ + j * 32 + 8 * q);                       \
      _Pragma("unroll") for (int i = 0; i < MW; ++i) {                                                        \
        acc[i][j][4 * q + 0] = b_.x; acc[i][j][4 * q + 1] = b_.y; acc[i][j][4 * q + 2] = b_.z; acc[i][j][4 * q + 3] = b_.w; \
      }                                                                                                       \
    }                                                                                                         \
  }

  // ---- epilogue (uniform bases, thread-constant lane offsets) ----
  // (P16_EPILOGUE / P16_ACC_INIT stay defined for conv_ws.h, which supplies its own P16_EPI_CB / P16_EPI_M0)
#define P16_EPI_CB epi_cb
#define P16_EPI_M0 (epi_pos * MT + wave * (MW * 32))
  const int quad_r = l31 & 3;
  const long xpl16 = a.x_plen * 16, ypl16 = a.y_plen * 16;
  const unsigned lane_unit = (unsigned)(l31 * 16) + (g ? (unsigned)ypl16 : 0u);        // OM 0: g=0 stores the hi unit, g=1 the lo unit
  const unsigned lane_res = (unsigned)(l31 * 16) + (g ? (unsigned)xpl16 : 0u);         // residual: g=0 loads the hi unit, g=1 the lo unit
  const unsigned lane_pool = (unsigned)((l31 >> 2) * 16 + quad_r * 4) + (g ? (unsigned)ypl16 : 0u);
  const unsigned lane_f32 = (unsigned)(l31 * a.cout * 4 + g * 16);                     // OM 2
  float vmax = 0.f;    // running max |value| written to P16 (fp16 range guard)
  long epi_tile = -1;  // finished tile whose accumulators still await their epilogue (-1: none)
  int epi_cb = 0;
  long epi_pos = 0;
  int epi_slot = 0;    // RL: window slot of that tile

  // Runs at the START of the next step (after the barrier that drained this step's DMA): its stores drain
  // underneath that step's MFMA block and are retired by the step's closing barrier.
#define P16_EPILOGUE_B16()                                                                                       \
  {                                                                                                              \
    const long tcb = P16_EPI_CB;                                                                                 \
    const long m0 = P16_EPI_M0;                                                                                  \
    u32x4_t rr[R1 ? NG / 2 : 1];                                                                                 \
    if (R1) {                                                                                                    \
      _Pragma("unroll") for (int i = 0; i < MW; ++i) _Pragma("unroll") for (int j = 0; j < NW; ++j) _Pragma("unroll") for (int qp = 0; qp < 2; ++qp) { \
        const char* rb_ = reinterpret_cast<const char*>(a.r1) + (long)(((int)tcb * CT + j * 32) / 8 + 2 * qp) * xpl16 + (P16_GUARD + m0 + i * 32) * 16; \
        rr[(i * NW + j) * 2 + qp] = *reinterpret_cast<const u32x4_t*>(rb_ + lane_res);                           \
      }                                                                                                          \
    }                                                                                                            \
    _Pragma("unroll") for (int i = 0; i < MW; ++i) _Pragma("unroll") for (int j = 0; j < NW; ++j) _Pragma("unroll") for (int qp = 0; qp < 2; ++qp) { \
      const int co = (int)tcb * CT + j * 32 + 16 * qp;   /* q0 = 2 qp: couts co + 4g .. +3, q1: co + 8 + 4g .. */ \
      const long p0 = m0 + i * 32;                       /* + l31 per lane */                                    \
      f32x4 v0, v1;                                                                                              \
      v0.x = acc[i][j][8 * qp + 0]; v0.y = acc[i][j][8 * qp + 1]; v0.z = acc[i][j][8 * qp + 2]; v0.w = acc[i][j][8 * qp + 3]; \
      v1.x = acc[i][j][8 * qp + 4]; v1.y = acc[i][j][8 * qp + 5]; v1.z = acc[i][j][8 * qp + 6]; v1.w = acc[i][j][8 * qp + 7]; \
      if (R1) {   /* the lane loaded the whole unit of plane 2 qp + g: trade halves with lane l +- 32 */          \
        const u32x4_t u_ = rr[(i * NW + j) * 2 + qp];                                                            \
        unsigned ux_ = u_.x, uy_ = u_.y, uz_ = u_.z, uw_ = u_.w;                                                 \
        p16_swap32(ux_, uz_);   /* ux, uy = couts 4g..4g+3 of q0;  uz, uw = the same of q1 */                    \
        p16_swap32(uy_, uw_);                                                                                    \
        v0.x += bf16lo_f32(ux_); v0.y += bf16hi_f32(ux_); v0.z += bf16lo_f32(uy_); v0.w += bf16hi_f32(uy_);      \
        v1.x += bf16lo_f32(uz_); v1.y += bf16hi_f32(uz_); v1.z += bf16lo_f32(uw_); v1.w += bf16hi_f32(uw_);      \
      }                                                                                                          \
      if (OM == 2) {                                                                                             \
        if (p0 + l31 < a.n) {                                                                                    \
          char* o_ = reinterpret_cast<char*>(a.y) + (p0 * a.cout + co) * 4 + lane_f32;                           \
          *reinterpret_cast<f32x4*>(o_) = v0;                                                                    \
          *reinterpret_cast<f32x4*>(o_ + 32) = v1;                                                               \
        }                                                                                                        \
      } else {                                                                                                   \
        if (OM == 1) {                                                                                           \
          v0.x = p16_dpp_quad_max(v0.x); v0.y = p16_dpp_quad_max(v0.y); v0.z = p16_dpp_quad_max(v0.z); v0.w = p16_dpp_quad_max(v0.w); \
          v1.x = p16_dpp_quad_max(v1.x); v1.y = p16_dpp_quad_max(v1.y); v1.z = p16_dpp_quad_max(v1.z); v1.w = p16_dpp_quad_max(v1.w); \
        }                                                                                                        \
        unsigned a0_ = cvt_pk_bf16(v0.x, v0.y), a1_ = cvt_pk_bf16(v0.z, v0.w);                                   \
        unsigned b0_ = cvt_pk_bf16(v1.x, v1.y), b1_ = cvt_pk_bf16(v1.z, v1.w);                                   \
        p16_swap32(a0_, b0_);   /* g=0: {a, b} = couts 0-3 | 4-7 of plane 2 qp;  g=1: of plane 2 qp + 1 */       \
        p16_swap32(a1_, b1_);                                                                                    \
        u32x4_t unit_;                                                                                           \
        unit_.x = a0_; unit_.y = a1_; unit_.z = b0_; unit_.w = b1_;                                              \
        char* yb_ = reinterpret_cast<char*>(a.y) + (long)(co >> 3) * ypl16;                                      \
        if (ABL & 16) {                                                                                          \
          asm volatile("" ::"v"(unit_));                                                                         \
        } else if (OM == 0 && (ABL & 32)) {   /* micro-benchmark (timing only): tile-major order [512-block][plane][512] */ \
          *reinterpret_cast<u32x4_t*>(reinterpret_cast<char*>(a.y) + ((((p0 >> 9) * (a.cout >> 3) + (co >> 3) + g) << 9) + (p0 & 511) + l31) * 16) = unit_; \
        } else if (OM == 0) {                                                                                    \
          *reinterpret_cast<u32x4_t*>(yb_ + (P16_GUARD + p0) * 16 + lane_unit) = unit_;                          \
        } else {                                                                                                 \
          const unsigned d01_ = (quad_r & 1) ? unit_.y : unit_.x, d23_ = (quad_r & 1) ? unit_.w : unit_.z;       \
          *reinterpret_cast<unsigned*>(yb_ + (P16_GUARD + (p0 >> 2)) * 16 + lane_pool) = (quad_r & 2) ? d23_ : d01_; \
        }                                                                                                        \
      }                                                                                                          \
    }                                                                                                            \
  }
#define P16_EPILOGUE_P16()                                                                                       \
  {                                                                                                              \
    const long tcb = P16_EPI_CB;                                                                                 \
    const long m0 = P16_EPI_M0;                                                                                  \
    u32x4_t rr[R1 ? NG : 1];                                                                                     \
    if (R1) {                                                                                                    \
      _Pragma("unroll") for (int i = 0; i < MW; ++i) _Pragma("unroll") for (int j = 0; j < NW; ++j) _Pragma("unroll") for (int q = 0; q < 4; ++q) { \
        const char* rb_ = reinterpret_cast<const char*>(a.r1) + (long)(((int)tcb * CT + j * 32) / 8 + q) * 2 * xpl16 + (P16_GUARD + m0 + i * 32) * 16; \
        rr[(i * NW + j) * 4 + q] = *reinterpret_cast<const u32x4_t*>(rb_ + lane_res);                            \
      }                                                                                                          \
    }                                                                                                            \
    _Pragma("unroll") for (int i = 0; i < MW; ++i) _Pragma("unroll") for (int j = 0; j < NW; ++j) _Pragma("unroll") for (int q = 0; q < 4; ++q) { \
      const int co = (int)tcb * CT + j * 32 + 8 * q;   /* + 4*g per lane */                                      \
      const long p0 = m0 + i * 32;                     /* + l31 per lane */                                      \
      f32x4 v;                                                                                                   \
      v.x = acc[i][j][4 * q + 0]; v.y = acc[i][j][4 * q + 1]; v.z = acc[i][j][4 * q + 2]; v.w = acc[i][j][4 * q + 3]; \
      if (R1) {                                                                                                  \
        const u32x4_t u_ = rr[(i * NW + j) * 4 + q];                                                             \
        unsigned ux_ = u_.x, uy_ = u_.y, uz_ = u_.z, uw_ = u_.w;                                                 \
        p16_swap32(ux_, uz_);   /* both halves: ux = hi pair 0, uz = lo pair 0 of the lane's 4 couts */          \
        p16_swap32(uy_, uw_);                                                                                    \
        const f16x2 h0_ = __builtin_bit_cast(f16x2, ux_), h1_ = __builtin_bit_cast(f16x2, uy_);                  \
        const f16x2 l0_ = __builtin_bit_cast(f16x2, uz_), l1_ = __builtin_bit_cast(f16x2, uw_);                  \
        v.x += (float)h0_.x + (float)l0_.x; v.y += (float)h0_.y + (float)l0_.y;                                  \
        v.z += (float)h1_.x + (float)l1_.x; v.w += (float)h1_.y + (float)l1_.y;                                  \
      }                                                                                                          \
      if (OM == 2) {                                                                                             \
        if (p0 + l31 < a.n) *reinterpret_cast<f32x4*>(reinterpret_cast<char*>(a.y) + (p0 * a.cout + co) * 4 + lane_f32) = v; \
      } else {                                                                                                   \
        if (OM == 1) {                                                                                           \
          v.x = p16_dpp_quad_max(v.x); v.y = p16_dpp_quad_max(v.y);                                              \
          v.z = p16_dpp_quad_max(v.z); v.w = p16_dpp_quad_max(v.w);                                              \
        }                                                                                                        \
        vmax = p16_vmax3_abs(p16_vmax3_abs(vmax, v.x, v.y), v.z, v.w);                                                   \
        unsigned h0_, h1_, l0_, l1_;                                                                             \
        p16_split_hl(v, h0_, h1_, l0_, l1_);                                                                     \
        p16_swap32(h0_, l0_);   /* g=0: {h, l} = hi halves of couts 0-3 | 4-7;  g=1: the lo halves */            \
        p16_swap32(h1_, l1_);                                                                                    \
        u32x4_t unit_;                                                                                           \
        unit_.x = h0_; unit_.y = h1_; unit_.z = l0_; unit_.w = l1_;                                              \
        char* yb_ = reinterpret_cast<char*>(a.y) + (long)(co >> 3) * 2 * ypl16;                                  \
        if (ABL & 16) {                                                                                          \
          asm volatile("" ::"v"(unit_));                                                                         \
        } else if (OM == 0 && (ABL & 32)) {   /* micro-benchmark: same stores, folded into a 2 MB (L2-resident) window */ \
          *reinterpret_cast<u32x4_t*>(reinterpret_cast<char*>(a.y) + ((((long)(co >> 3) * 2 * ypl16 + (P16_GUARD + p0) * 16 + lane_unit)) & 0x1FFFF0L)) = unit_; \
        } else if (OM == 0) {                                                                                    \
          *reinterpret_cast<u32x4_t*>(yb_ + (P16_GUARD + p0) * 16 + lane_unit) = unit_;                          \
        } else {                                                                                                 \
          const unsigned d01_ = (quad_r & 1) ? unit_.y : unit_.x, d23_ = (quad_r & 1) ? unit_.w : unit_.z;       \
          *reinterpret_cast<unsigned*>(yb_ + (P16_GUARD + (p0 >> 2)) * 16 + lane_pool) = (quad_r & 2) ? d23_ : d01_; \
        }                                                                                                        \
      }                                                                                                          \
    }                                                                                                            \
  }
  // (conv_ws.h defines its own, empty, P16_EPI_HOOK)
#define P16_EPI_HOOK()                                                                                           \
    if constexpr (RL) {   /* + lout1 of the tile's positions, straight from the bases (see the RL note above) */  \
      const unsigned char* win_ = rl_win + epi_slot * RL_WIN + wave * (MW * 32) + l31 + 2 * g;                   \
      _Pragma("unroll") for (int i = 0; i < MW; ++i) {                                                           \
        f16x8 xf_[5];                                                                                            \
        _Pragma("unroll") for (int kk = 0; kk < 5; ++kk) {                                                       \
          const u32x2 o0_ = rl_oh[win_[i * 32 + 4 * kk]], o1_ = rl_oh[win_[i * 32 + 4 * kk + 1]];                \
          u32x4_t u_;                                                                                            \
          u_.x = o0_.x; u_.y = o0_.y; u_.z = o1_.x; u_.w = o1_.y;                                                \
          xf_[kk] = __builtin_bit_cast(f16x8, u_);                                                               \
        }                                                                                                        \
        _Pragma("unroll") for (int j = 0; j < NW; ++j) _Pragma("unroll") for (int q = 0; q < 4; ++q) {           \
          const f32x4 b_ = *reinterpret_cast<const f32x4*>(rl_b + j * 32 + 8 * q + 4 * g);                       \
          acc[i][j][4 * q + 0] += b_.x; acc[i][j][4 * q + 1] += b_.y; acc[i][j][4 * q + 2] += b_.z; acc[i][j][4 * q + 3] += b_.w; \
        }                                                                                                        \
        _Pragma("unroll") for (int kk = 0; kk < 5; ++kk) _Pragma("unroll") for (int sp = 1; sp >= 0; --sp) _Pragma("unroll") for (int j = 0; j < NW; ++j) \
          acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, rl_ws[((sp * 5 + kk) * 2 + g) * 64 + j * 32 + l31]), xf_[kk], acc[i][j], 0, 0, 0); \
      }                                                                                                          \
    }
  // ReLU in place on the accumulators, skipped as a whole (scalar branch) by the linear layers.  The units of a ragged last
  // tile beyond n are written unmasked: the caller runs p16_zero_pads_kernel AFTER the conv (tail and guards must read zero).
#define P16_EPILOGUE()                                                                                           \
  {                                                                                                              \
    if (a.relu) {                                                                                                \
      _Pragma("unroll") for (int i = 0; i < MW; ++i) _Pragma("unroll") for (int j = 0; j < NW; ++j) _Pragma("unroll") for (int r = 0; r < 16; ++r) \
        acc[i][j][r] = p16_vmax(acc[i][j][r], 0.f);                                                              \
    }                                                                                                            \
    P16_EPI_HOOK()                                                                                               \
    if constexpr (FMT == 1) P16_EPILOGUE_B16() else P16_EPILOGUE_P16()                                           \
  }

  P16_SRC(tile_cb, tile_pos, 0);
#pragma unroll
  for (int it = 0; it < NIT; ++it) P16_DMA_ONE(it, 0);
  int f1_slot = 0;                      // window slot of the CURRENT tile
  unsigned char f1_next[2] = {5, 5};    // bases of the next tile's window, in flight between step 0 and step 1 of a tile
  if (RL) {                             // the first tile's window; the table, bias and pack become visible with it
    const long m0_ = tile_pos * MT;
    for (int k = tid; k < RL_WIN; k += NT) rl_win[k] = f1_fix(f1_fetch(m0_ - 8 + k));
  }
  if (F1) {
    const long m0_ = tile_pos * MT;
    for (int k = tid; k < F1_WIN; k += NT) f1_win[k] = f1_fix(f1_fetch(m0_ - 8 + k));
    __syncthreads();                    // window + table + bias visible
    for (int r = 0; r < 2; ++r) {
      P16_F1_WINDOW(tid + r * NT, m0_, 0, 0);
#pragma unroll
      for (int q = 0; q < 4; ++q) P16_F1_QUAD(tid + r * NT, q, 0, 0);
    }
  }
  __syncthreads();   // drains vmcnt (the DMA) and joins the waves; the bias is visible
  P16_ACC_INIT(tile_cb);

  int c = 0, cur = 0;
  int nstamp = 0;
  unsigned long long clk0 = 0, rt0 = 0;
  if (ABL & 128) { clk0 = __builtin_readcyclecounter(); rt0 = __builtin_amdgcn_s_memrealtime(); }
  // stamps[(step * 8 + wave) * 5 + k]: k = 0 step start, 1 epilogue done, 3 MFMA block done, 4 own DMA + stores retired
#define P16_STAMP(k) if ((ABL & 128) && blockIdx.x == 0 && lane == 0 && nstamp >= 200 && nstamp < 400) a.stamps[((nstamp - 200) * 8 + wave) * 5 + (k)] = __builtin_readcyclecounter();
  while (true) {
    const bool last_chunk = (c + 1 == a.nchunks);
    const long ntile = last_chunk ? tile + gridDim.x : tile;
    const int nc = last_chunk ? 0 : c + 1;
    const bool more = ntile < ntiles;
    int nx_cb = tile_cb;            // the tile after this one (tile + gridDim.x)
    long nx_pos = tile_pos + gridDim.x;
    while (nx_pos >= a.tiles_per_row) { nx_pos -= a.tiles_per_row; ++nx_cb; }
    const int ntile_cb = last_chunk ? nx_cb : tile_cb;
    const long ntile_pos = last_chunk ? nx_pos : tile_pos;
    P16_STAMP(0);
    if (epi_tile >= 0) {
      // raised priority: the SIMD's older wave reaches its MFMA block first and would otherwise starve the
      // younger wave's epilogue VALU work until its own block is over
      __builtin_amdgcn_s_setprio(3);
      P16_EPILOGUE();
      P16_ACC_INIT(tile_cb);
      __builtin_amdgcn_s_setprio(0);
      epi_tile = -1;
    }
    P16_STAMP(1);
    if (more) P16_SRC(ntile_cb, ntile_pos, nc);
    if (F1) {   // the next tile's bases: fetched during the tile's first step, parked in LDS during its second
      const long nxt_ = tile + gridDim.x;
      const long m0n_ = nx_pos * MT - 8;
      if (c == 0 && nxt_ < ntiles) {
        f1_next[0] = f1_fetch(m0n_ + tid);                      // raw: nothing may touch the loaded byte during this step
        if (tid < F1_WIN - NT) f1_next[1] = f1_fetch(m0n_ + NT + tid);
      }
      if (c == 1 && nxt_ < ntiles) {
        f1_win[(f1_slot ^ 1) * F1_WIN + tid] = f1_fix(f1_next[0]);
        if (tid < F1_WIN - NT) f1_win[(f1_slot ^ 1) * F1_WIN + NT + tid] = f1_fix(f1_next[1]);
      }
    }
    if (RL) {   // the next tile's bases, as above, for its epilogue
      const long nxt_ = tile + gridDim.x;
      const long m0n_ = nx_pos * MT - 8;
      if (c == 0 && nxt_ < ntiles) {
        f1_next[0] = f1_fetch(m0n_ + tid);
        if (tid < RL_WIN - NT) f1_next[1] = f1_fetch(m0n_ + NT + tid);
      }
      if (c == 1 && nxt_ < ntiles) {
        rl_win[(f1_slot ^ 1) * RL_WIN + tid] = f1_fix(f1_next[0]);
        if (tid < RL_WIN - NT) rl_win[(f1_slot ^ 1) * RL_WIN + NT + tid] = f1_fix(f1_next[1]);
      }
    }
    const long f1_m0 = F1 ? ntile_pos * MT : 0;      // tile whose input the producer builds during this step
    const int f1_ws = (F1 && last_chunk) ? (f1_slot ^ 1) : f1_slot;

    const bool skip_tap8 = a.k17 && (c & 1);      // uniform
    const unsigned xa0 = p16_lds_addr(smem + cur * BU + g * XROW + wave * (MW * 32) + l31);   // + (s*2*XROW + i*32 + tap)*16
    const unsigned wb0 = p16_lds_addr(smem + cur * BU + XU + g * CT + l31);                    // + (((s*9+tap)*2)*CT + j*32)*16
    // operand fragments are double-buffered across taps: tap t+1 is read from LDS while tap t feeds the MFMAs
    f16x8 av[2][2][MW], bv[2][2][NW];
#define P16_READ_FRAGS(buf_, tap_)                                                                                 \
  _Pragma("unroll") for (int s = 0; s < 2; ++s) {                                                                  \
    _Pragma("unroll") for (int i = 0; i < MW; ++i) av[buf_][s][i] = p16_lds_read16(xa0, (s * 2 * XROW + i * 32 + (tap_)) * 16); \
    _Pragma("unroll") for (int j = 0; j < NW; ++j) bv[buf_][s][j] = p16_lds_read16(wb0, (((s * 9 + (tap_)) * 2) * CT + j * 32) * 16); \
  }
    P16_READ_FRAGS(0, 0);
#pragma unroll
    for (int tap = 0; tap < 9; ++tap) {
      const int fb = (ABL & 8) ? 0 : (tap & 1);
      if constexpr (F1) {
        // all LDS reads issued so far (this tap's fragments, the producer's half quad of the previous tap) have had a whole
        // tap to land: retire them together; the fragment wait further down then only orders the MFMAs
        p16_f1_wait0<MW, NW>(av[fb], bv[fb], f1_r);
        if (more && !(ABL & 8192)) {   // the next step's input image, position `tid`: tap t consumes half-quad t-1 and issues half-quad t
          if (tap >= 1) P16_F1_CONSUME(tid, (tap - 1) >> 1, (tap - 1) & 1, cur ^ 1);
          if (tap == 0) P16_F1_WINDOW(tid, f1_m0, f1_ws, nc);
          if (tap < 8) P16_F1_ISSUE(tap >> 1, tap & 1, nc);
          // the XROW - NT = 8 halo positions beyond the threads: lanes 0..7 of waves 0..3 (one per SIMD), wave q computes
          // channel quad q of all eight - un-pipelined (4 LDS round trips), after this wave's own last half quad
          if (tap == 8 && wave < 4 && lane < XROW - NT && !(ABL & 1024)) {
            P16_F1_WINDOW(NT + lane, f1_m0, f1_ws, nc);
            if (wave == 0) { P16_F1_QUAD(NT + lane, 0, nc, cur ^ 1) }
            else if (wave == 1) { P16_F1_QUAD(NT + lane, 1, nc, cur ^ 1) }
            else if (wave == 2) { P16_F1_QUAD(NT + lane, 2, nc, cur ^ 1) }
            else { P16_F1_QUAD(NT + lane, 3, nc, cur ^ 1) }
          }
        }
      }
      if (tap + 1 < 9 && !(ABL & 8)) P16_READ_FRAGS(fb ^ 1, tap + 1);
      if (more && tap < 5 && !(ABL & 1)) {   // the next buffer's DMA, spread over the first taps
#pragma unroll
        for (int d = 0; d < DPT; ++d)
          if (tap * DPT + d < NIT && !((ABL & 64) && !isx[tap * DPT + d]) && !((ABL & 256) && isx[tap * DPT + d])) P16_DMA_ONE(tap * DPT + d, cur ^ 1);   // ABL 64 / 256: no W / no X pieces
      }
      if (F1) p16_lds_wait<15, MW, NW>(av[fb], bv[fb]);                      // already retired above: ordering only
      else if (tap + 1 < 9) p16_lds_wait<2 * (MW + NW), MW, NW>(av[fb], bv[fb]);   // this tap's fragments are in, the next tap's stay in flight
      else p16_lds_wait<0, MW, NW>(av[fb], bv[fb]);
      if ((ABL & 16384) && tap >= 6) { /* micro-benchmark: 2/3 of the MFMA work (timing only) */ }
      else if (tap == 8 && skip_tap8) { /* 17-tap conv, second tap half: its ninth tap does not exist (zero weights) */ }
      else if constexpr (FMT == 1) {
#pragma unroll
        for (int p = 0; p < 2; ++p)   // the two k-pairs of the step's 32 input channels
#pragma unroll
          for (int i = 0; i < MW; ++i)
#pragma unroll
            for (int j = 0; j < NW; ++j)
              acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, bv[fb][p][j]), __builtin_bit_cast(bf16x8, av[fb][p][i]), acc[i][j], 0, 0, 0);
      } else {
#pragma unroll
      for (int p = 0; p < 3; ++p) {
        constexpr int PA[3] = {1, 0, 0}, PB[3] = {0, 1, 0};   // lo*hi, hi*lo, hi*hi (largest last)
#pragma unroll
        for (int i = 0; i < MW; ++i)
#pragma unroll
          for (int j = 0; j < NW; ++j)
            acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(bv[fb][PB[p]][j], av[fb][PA[p]][i], acc[i][j], 0, 0, 0);  // D[cout][pos]
      }
      }
      if ((ABL & 128) && blockIdx.x == 0 && lane == 0 && nstamp == 250 && (wave & 3) == 0) a.stamps[8100 + (wave >> 2) * 16 + tap] = __builtin_readcyclecounter();   // per-tap stamps of waves 0 and 4, one step
      __builtin_amdgcn_sched_barrier(0);
    }
#undef P16_READ_FRAGS

    P16_STAMP(3);
    if (ABL & 512) {   // micro-benchmark: TIMING of a de-phased variant - waves WM/2.. take their epilogue half a tile later
      if (wave < WM / 2 ? last_chunk : (c + 1 == a.nchunks / 2)) { epi_tile = tile; epi_cb = tile_cb; epi_pos = tile_pos; }   // (the late group's results are meaningless)
    } else
    if (last_chunk) { epi_tile = tile; epi_cb = tile_cb; epi_pos = tile_pos; epi_slot = f1_slot; }

    if (!more) break;
    if (ABL & 128) { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); P16_STAMP(4); ++nstamp; }
    __syncthreads();   // next buffer has landed (vmcnt drained), everyone is done reading the current one
    if ((F1 || RL) && last_chunk) f1_slot ^= 1;
    tile = ntile;
    tile_cb = ntile_cb;
    tile_pos = ntile_pos;
    c = nc;
    cur ^= 1;
  }
  if (epi_tile >= 0) P16_EPILOGUE();   // the last tile
  if ((ABL & 128) && blockIdx.x == 0 && tid == 0) {
    a.stamps[8190] = __builtin_readcyclecounter() - clk0;
    a.stamps[8191] = __builtin_amdgcn_s_memrealtime() - rt0;
  }
#undef P16_EPI_CB
#undef P16_EPI_M0
#undef P16_EPI_HOOK
#undef P16_STAMP
#undef P16_DMA_ONE
#undef P16_SRC
#undef P16_F1_CONSUME
#undef P16_F1_ISSUE
#undef P16_F1_QUAD
#undef P16_F1_WINDOW
  if (FMT == 0 && OM != 2 && vmax > 65504.f && a.flag) *a.flag = 1u;
}

// zero the guard / tail units of every plane: [0, P16_GUARD) and [P16_GUARD + n_valid, plen); and the units of positions [gap0, gap1) between two
// sequences that share the planes (the two strands of orca_encoder_forward_two_strands; gap0 = gap1: one sequence)
static __global__ void p16_zero_pads_kernel(f32x4* __restrict__ base, long plen, long n_valid, long gap0, long gap1) {
  f32x4* pl = base + (long)blockIdx.x * plen;
  const long tail0 = P16_GUARD + n_valid, ngap = gap1 - gap0;
  for (long i = threadIdx.x; i < P16_GUARD + ngap + (plen - tail0); i += blockDim.x) {
    const long u = i < P16_GUARD ? i : i < P16_GUARD + ngap ? gap0 + i : tail0 + (i - P16_GUARD - ngap);
    pl[u] = (f32x4)(0.f);
  }
}

// ---- first layer: Conv1d(4,64,k9,p4)+BN straight from the [L][4] float sequence to P16 ------------------
// K = 36 only (1 % of the Encoder FLOPs): plain fp32 FMAs.  One thread = one position x one cout octet.
struct FirstP16Args {
  const float* x;   // element strides sc (channel), sl (position)
  long sc, sl, n;
  const float* w;   // [64][4][9] folded
  const float* bias;
  f32x4* y;         // P16, 64 channels
  long y_plen;
  unsigned* flag;
};

static __global__ __launch_bounds__(256) void conv1d_first_p16_kernel(FirstP16Args a) {
  __shared__ float ws[36 * 8];   // [tap*4+ci][8 couts of this octet]
  __shared__ float bs[8];
  const int oct = blockIdx.y;
  for (int t = threadIdx.x; t < 288; t += 256) {
    const int k = t >> 3, e = t & 7;               // k = tap*4 + ci
    ws[t] = a.w[((oct * 8 + e) * 4 + (k & 3)) * 9 + (k >> 2)];
  }
  if (threadIdx.x < 8) bs[threadIdx.x] = a.bias[oct * 8 + threadIdx.x];
  __syncthreads();
  const long pos = (long)blockIdx.x * 256 + threadIdx.x;
  if (pos >= a.n) return;
  float xin[36];
  const bool fast = (a.sc == 1 && a.sl == 4);
#pragma unroll
  for (int t = 0; t < 9; ++t) {
    const long p = pos + t - 4;
    const bool ok = (p >= 0 && p < a.n);
    if (fast) {
      f32x4 v = (f32x4)(0.f);
      if (ok) v = *reinterpret_cast<const f32x4*>(a.x + p * 4);
      xin[4 * t + 0] = v.x; xin[4 * t + 1] = v.y; xin[4 * t + 2] = v.z; xin[4 * t + 3] = v.w;
    } else {
#pragma unroll
      for (int ci = 0; ci < 4; ++ci) xin[4 * t + ci] = ok ? a.x[p * a.sl + ci * a.sc] : 0.f;
    }
  }
  float o[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) o[e] = bs[e];
#pragma unroll
  for (int k = 0; k < 36; ++k) {
    const f32x4 w0 = *reinterpret_cast<const f32x4*>(ws + k * 8), w1 = *reinterpret_cast<const f32x4*>(ws + k * 8 + 4);
    o[0] = fmaf(w0.x, xin[k], o[0]); o[1] = fmaf(w0.y, xin[k], o[1]); o[2] = fmaf(w0.z, xin[k], o[2]); o[3] = fmaf(w0.w, xin[k], o[3]);
    o[4] = fmaf(w1.x, xin[k], o[4]); o[5] = fmaf(w1.y, xin[k], o[5]); o[6] = fmaf(w1.z, xin[k], o[6]); o[7] = fmaf(w1.w, xin[k], o[7]);
  }
  char* pl = reinterpret_cast<char*>(a.y) + (long)oct * 2 * a.y_plen * 16 + (P16_GUARD + pos) * 16;
  f32x4 lo4, hi4;
  lo4.x = o[0]; lo4.y = o[1]; lo4.z = o[2]; lo4.w = o[3];
  hi4.x = o[4]; hi4.y = o[5]; hi4.z = o[6]; hi4.w = o[7];
  bool ovf = false;
  p16_split_store(pl, a.y_plen * 16, lo4, true, ovf);
  p16_split_store(pl + 8, a.y_plen * 16, hi4, true, ovf);
  if (ovf && a.flag) *a.flag = 1u;
}

// ---- first layer on the matrix cores ----------------------------------------------------------------------
// With the sequence stored [L][4] the 9-tap x 4-channel window of a position is 36 CONTIGUOUS floats, so
// Conv1d(4,64,k9) is a GEMM with K = tap*4+ci = 36 (padded to 48 = three k16 steps; the pad weights are zero).
// X operand of lane (pos, g) for k-step kk = the 8 halves at flat index 4*(pos-4) + 16*kk + 8*g of the split
// window image (8-byte aligned: two ds_read_b64).  Persistent; W stays in LDS; the next tile's window is
// prefetched to registers under the current tile's MFMAs + epilogue.  HBM-write bound (8 GB P16 output).
struct FirstMfmaArgs {
  const float* x;     // [n][4] contiguous fp32, or NULL when `codes` is given
  // packed input: 1 byte per base (0..3 = A,C,G,T one-hot rows, 4 = N = 0.25 x 4, other = zero row).  The chunk's
  // position p is strand position off+p; on the reverse strand that is base L-1-(off+p), complemented (3-code).
  const unsigned char* codes;
  const unsigned char* nmask;   // non-NULL: `codes` is a 2-bit genome plane, this its N mask, `origin` the genome index of base 0 (p16_base_at)
  long origin;
  long codes_L, codes_off;
  int reverse;
  long n;
  const f32x4* w;     // fp16 pack [2 splits][3 ksteps][2 g][64 couts][8]  (units of 16 B), k >= 36 zero
  const float* bias;
  f32x4* y;           // P16, 64 channels
  long y_plen;
  unsigned* flag;
  int relu;           // ReLU on the result (the 25-tap composition ends in conv1.a's BN + ReLU)
};

// ABL (tools/microbench_first.hip only): 1 = no MFMA, 16 = no stores, 32 = input not re-fetched per tile
// FMT = 1: the output is B16 (one bf16 plane per 8 channels) instead of P16, FMT = 2: fp32 channel-last [n][64]; the arithmetic is unchanged.
// NTAP = 9: the first layer alone (lconv1.a).  NTAP = 17: the COMPOSED linear pair lconv1 = Conv(4,64,k9)-BN-Conv(64,64,k9)-BN
//   (orca_modules.py:811-816 has no nonlinearity between the two) as ONE 17-tap conv from the bases, K = 68 -> 80: the
//   64 -> 64 launch at full resolution that used to follow the first layer is gone.  The 4 positions next to each end of
//   the chunk are redone by lconv_edge_fix_kernel (the intermediate is zero-padded there, which a single conv cannot express).
//   With packed input the X operand is exactly representable in fp16 (0, 0.25, 1): its lo plane is zero and the lo*hi product is skipped.
// NTAP = 25: conv1.a's pre-activation is linear in the bases too - Conv(64,64,k9)-BN applied to lconv1's output (orca_modules.py:819-821
//   on :811-816) = ONE 25-tap conv from the bases, K = 100 -> 112, followed by the ReLU (a.relu): the second 64 -> 64 launch at full
//   resolution is gone as well.  Its 8 positions next to each end are redone by the edge-fix chain.
template <int ABL = 0, int FMT = 0, int NTAP = 9>
__global__ __launch_bounds__(256, 2) void conv1d_first_mfma_p16_kernel(FirstMfmaArgs a) {
  constexpr int H = (NTAP - 1) / 2;               // conv half width
  constexpr int KS = (4 * NTAP + 15) / 16;        // k16 steps (K = 4 NTAP padded; the pad weights are zero)
  constexpr int MT = 256, WIN = MT + 4 * KS;      // positions m0-H .. (9-tap window + k padding overrun)
  constexpr int WU = 2 * KS * 2 * 64;             // weight units
  __shared__ f32x4 wsm[WU];
  __shared__ u32x2 xsm[2][WIN];                   // [split][position] -> 4 halves (the 4 channels)
  __shared__ float bias_s[64];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int l31 = lane & 31, g = lane >> 5;
  const long ntiles = (a.n + MT - 1) / MT;
  for (int i = tid; i < WU; i += 256) wsm[i] = a.w[i];
  if (tid < 64) bias_s[tid] = a.bias[tid];
  bool overflow = false;
  float vmax = 0.f;
  const bool exact_x = a.codes != nullptr;        // uniform

  f32x4 xr[2];
  auto fetch = [&](long p) -> f32x4 {
    if (p < 0 || p >= a.n) return (f32x4)(0.f);
    if (!a.codes) return *reinterpret_cast<const f32x4*>(a.x + p * 4);
    const long P = a.codes_off + p;
    int c = p16_base_at(a.codes, a.nmask, a.origin, a.reverse ? a.codes_L - 1 - P : P);
    if (a.reverse && c < 4) c = 3 - c;
    f32x4 v = (f32x4)(c == 4 ? 0.25f : 0.f);   // LDS-staged one-hot expansion of the packed base
    if (c < 4) v[c] = 1.f;
    return v;
  };
  auto load_win = [&](long t, f32x4& r0, f32x4& r1) {
    const long p0 = t * MT - H + tid;
    r0 = fetch(p0);
    r1 = (tid < WIN - 256) ? fetch(p0 + 256) : (f32x4)(0.f);
  };
  long tile = blockIdx.x;
  if (tile >= ntiles) return;
  load_win(tile, xr[0], xr[1]);
  for (; tile < ntiles; tile += gridDim.x) {
    __syncthreads();   // previous tile's LDS reads are done
    {
      u32x2 sp[2];
      split4<2, 1>(xr[0], sp, overflow);
      xsm[0][tid] = sp[0]; xsm[1][tid] = sp[1];
      if (tid < WIN - 256) {
        split4<2, 1>(xr[1], sp, overflow);
        xsm[0][256 + tid] = sp[0]; xsm[1][256 + tid] = sp[1];
      }
    }
    __syncthreads();
    if (tile + gridDim.x < ntiles && !(ABL & 32)) load_win(tile + gridDim.x, xr[0], xr[1]);

    f32x16 acc[2][2];   // start from the bias (lane: couts j*32 + 8q + 4g .. +3 in registers 4q..4q+3)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const f32x4 b_ = *reinterpret_cast<const f32x4*>(bias_s + j * 32 + 8 * q + 4 * g);
#pragma unroll
        for (int i = 0; i < 2; ++i) { acc[i][j][4 * q + 0] = b_.x; acc[i][j][4 * q + 1] = b_.y; acc[i][j][4 * q + 2] = b_.z; acc[i][j][4 * q + 3] = b_.w; }
      }
#pragma unroll
    for (int kk = 0; kk < KS; ++kk) {
      f16x8 xv[2][2], wv[2][2];
#pragma unroll
      for (int s = 0; s < 2; ++s) {
#pragma unroll
        for (int i = 0; i < 2; ++i) {
          const int pr = wave * 64 + i * 32 + l31 + 4 * kk + 2 * g;   // window position holding k = 16kk + 8g
          const u32x2 lo = xsm[s][pr], hi = xsm[s][pr + 1];
          u32x4_t q = {lo.x, lo.y, hi.x, hi.y};
          xv[s][i] = __builtin_bit_cast(f16x8, q);
        }
#pragma unroll
        for (int j = 0; j < 2; ++j) wv[s][j] = __builtin_bit_cast(f16x8, wsm[((s * KS + kk) * 2 + g) * 64 + j * 32 + l31]);
      }
#pragma unroll
      for (int p = 0; p < 3; ++p) {
        constexpr int PA[3] = {1, 0, 0}, PB[3] = {0, 1, 0};
        if (p == 0 && exact_x) continue;   // x lo plane is all zero
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
          for (int j = 0; j < 2; ++j)
            if (!(ABL & 1)) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(wv[PB[p]][j], xv[PA[p]][i], acc[i][j], 0, 0, 0);
      }
    }
    // epilogue as in conv1d_k9_p16_kernel: lanes l / l+32 exchange halves so that each stores one 16-byte unit
    // (g = 0: the hi unit, g = 1: the lo unit); positions >= n get zeros (they are tail guard units of the plane)
    const long ypl = a.y_plen * 16;
    const unsigned lane_unit = (unsigned)(l31 * 16) + (g ? (unsigned)ypl : 0u);
    if (a.relu) {
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
          for (int r = 0; r < 16; ++r) acc[i][j][r] = p16_vmax(acc[i][j][r], 0.f);
    }
    if constexpr (FMT == 2) {   // fp32 channel-last [n][64]: the hand-over to the register-staged kernels (conv_bf16s.h) of the bf16x3 / bf16x2 modes
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const long p = tile * MT + wave * 64 + i * 32 + l31;
        if (p < a.n) {
          float* o_ = reinterpret_cast<float*>(a.y) + p * 64 + 4 * g;
#pragma unroll
          for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
              f32x4 v;
              v.x = acc[i][j][4 * q + 0]; v.y = acc[i][j][4 * q + 1]; v.z = acc[i][j][4 * q + 2]; v.w = acc[i][j][4 * q + 3];
              *reinterpret_cast<f32x4*>(o_ + j * 32 + 8 * q) = v;
            }
        }
      }
      continue;
    }
    if constexpr (FMT == 1) {
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const long p0 = tile * MT + wave * 64 + i * 32;
        const bool ok = p0 + l31 < a.n;
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
          for (int qp = 0; qp < 2; ++qp) {
            f32x4 v0, v1;
            v0.x = acc[i][j][8 * qp + 0]; v0.y = acc[i][j][8 * qp + 1]; v0.z = acc[i][j][8 * qp + 2]; v0.w = acc[i][j][8 * qp + 3];
            v1.x = acc[i][j][8 * qp + 4]; v1.y = acc[i][j][8 * qp + 5]; v1.z = acc[i][j][8 * qp + 6]; v1.w = acc[i][j][8 * qp + 7];
            if (!ok) { v0 = (f32x4)(0.f); v1 = (f32x4)(0.f); }
            unsigned a0 = cvt_pk_bf16(v0.x, v0.y), a1 = cvt_pk_bf16(v0.z, v0.w), b0 = cvt_pk_bf16(v1.x, v1.y), b1 = cvt_pk_bf16(v1.z, v1.w);
            p16_swap32(a0, b0);
            p16_swap32(a1, b1);
            u32x4_t unit;
            unit.x = a0; unit.y = a1; unit.z = b0; unit.w = b1;
            *reinterpret_cast<u32x4_t*>(reinterpret_cast<char*>(a.y) + (long)(j * 4 + 2 * qp) * ypl + (P16_GUARD + p0) * 16 + lane_unit) = unit;
          }
      }
      continue;
    }
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const long p0 = tile * MT + wave * 64 + i * 32;
      const bool ok = p0 + l31 < a.n;
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          f32x4 v;
          v.x = acc[i][j][4 * q + 0]; v.y = acc[i][j][4 * q + 1]; v.z = acc[i][j][4 * q + 2]; v.w = acc[i][j][4 * q + 3];
          if (!ok) v = (f32x4)(0.f);
          vmax = p16_vmax3_abs(p16_vmax3_abs(vmax, v.x, v.y), v.z, v.w);                                  
          unsigned h0, h1, l0, l1;
          p16_split_hl(v, h0, h1, l0, l1);
          p16_swap32(h0, l0);
          p16_swap32(h1, l1);
          u32x4_t unit;
          unit.x = h0; unit.y = h1; unit.z = l0; unit.w = l1;
          if (ABL & 16) asm volatile("" ::"v"(unit));
          else if (ABL & 64) { constexpr long G = (ABL >> 8) ? (ABL >> 8) : 1; *reinterpret_cast<u32x4_t*>(reinterpret_cast<char*>(a.y) + ((((tile / G) * 16 + (j * 4 + q) * 2 + g) * G + tile % G) * 256 + wave * 64 + i * 32 + l31) * 16) = unit; }   // blocked-planar test pattern: G tiles per block
          else *reinterpret_cast<u32x4_t*>(reinterpret_cast<char*>(a.y) + (long)(j * 4 + q) * 2 * ypl + (P16_GUARD + p0) * 16 + lane_unit) = unit;
        }
    }
  }
  if (vmax > 65504.f) overflow = true;
  if (FMT == 0 && overflow && a.flag) *a.flag = 1u;
}

// ---- packed sequence helpers --------------------------------------------------------------------------------
// [L][4] float rows (element strides sc, sl) -> 1-byte codes; *bad is raised for rows that are neither one-hot nor N
static __global__ void pack_sequence_kernel(const float* __restrict__ x, long sc, long sl, long L, unsigned char* __restrict__ codes,
                                     unsigned* __restrict__ bad) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= L) return;
  float v[4];
#pragma unroll
  for (int c = 0; c < 4; ++c) v[c] = x[i * sl + c * sc];
  int code = 5;
  if (v[0] == 0.25f && v[1] == 0.25f && v[2] == 0.25f && v[3] == 0.25f) code = 4;
  else {
    int ones = 0, zeros = 0, which = 0;
#pragma unroll
    for (int c = 0; c < 4; ++c) { if (v[c] == 1.f) { ++ones; which = c; } else if (v[c] == 0.f) ++zeros; }
    if (ones == 1 && zeros == 3) code = which;
  }
  if (code == 5) *bad = 1u;
  codes[i] = (unsigned char)code;
}
// codes -> [n][4] fp32 rows of strand positions off .. off+n-1 (used by the non-P16 arithmetic modes)
static __global__ void expand_codes_kernel(const unsigned char* __restrict__ codes, const unsigned char* __restrict__ nmask, long origin, long L, long off, int reverse,
                                    long n, float* __restrict__ y) {
  const long p = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= n) return;
  const long P = off + p;
  int c = p16_base_at(codes, nmask, origin, reverse ? L - 1 - P : P);
  if (reverse && c < 4) c = 3 - c;
  f32x4 v = (f32x4)(c == 4 ? 0.25f : 0.f);
  if (c < 4) v[c] = 1.f;
  reinterpret_cast<f32x4*>(y)[p] = v;
}

// ---- converters (tests, and the stage 3 -> 4 hand-over) -------------------------------------------------
// fp32 channel-last [n][C] -> P16
static __global__ void nlc_to_p16_kernel(const float* __restrict__ x, f32x4* __restrict__ y, long n, int C, long plen) {
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const int c4n = C / 4;
  if (idx >= n * c4n) return;
  const long pos = idx / c4n;
  const int c4 = (int)(idx - pos * c4n);
  const f32x4 v = *reinterpret_cast<const f32x4*>(x + pos * C + 4 * c4);
  bool ovf = false;
  p16_split_store(reinterpret_cast<char*>(y) + (long)(c4 >> 1) * 2 * plen * 16 + (P16_GUARD + pos) * 16 + (c4 & 1) * 8, plen * 16, v, true, ovf);
}
// fp32 channel-last [n][C] -> B16 (one bf16 plane per 8 channels), and back
static __global__ void nlc_to_b16_kernel(const float* __restrict__ x, f32x4* __restrict__ y, long n, int C, long plen) {
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const int c4n = C / 4;
  if (idx >= n * c4n) return;
  const long pos = idx / c4n;
  const int c4 = (int)(idx - pos * c4n);
  const f32x4 v = *reinterpret_cast<const f32x4*>(x + pos * C + 4 * c4);
  u32x2 pk;
  pk.x = cvt_pk_bf16(v.x, v.y); pk.y = cvt_pk_bf16(v.z, v.w);
  *reinterpret_cast<u32x2*>(reinterpret_cast<char*>(y) + (long)(c4 >> 1) * plen * 16 + (P16_GUARD + pos) * 16 + (c4 & 1) * 8) = pk;
}
static __global__ void b16_to_nlc_kernel(const f32x4* __restrict__ x, float* __restrict__ y, long n, int C, long plen) {
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const int c4n = C / 4;
  if (idx >= n * c4n) return;
  const long pos = idx / c4n;
  const int c4 = (int)(idx - pos * c4n);
  const u32x2 pk = *reinterpret_cast<const u32x2*>(reinterpret_cast<const char*>(x) + (long)(c4 >> 1) * plen * 16 + (P16_GUARD + pos) * 16 + (c4 & 1) * 8);
  f32x4 v;
  v.x = bf16lo_f32(pk.x); v.y = bf16hi_f32(pk.x); v.z = bf16lo_f32(pk.y); v.w = bf16hi_f32(pk.y);
  *reinterpret_cast<f32x4*>(y + pos * C + 4 * c4) = v;
}
// P16 -> fp32 channel-last [n][C]
static __global__ void p16_to_nlc_kernel(const f32x4* __restrict__ x, float* __restrict__ y, long n, int C, long plen) {
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const int c4n = C / 4;
  if (idx >= n * c4n) return;
  const long pos = idx / c4n;
  const int c4 = (int)(idx - pos * c4n);
  *reinterpret_cast<f32x4*>(y + pos * C + 4 * c4) =
      p16_load4(reinterpret_cast<const char*>(x) + (long)(c4 >> 1) * 2 * plen * 16 + (P16_GUARD + pos) * 16 + (c4 & 1) * 8, plen * 16);
}

// ---- composed linear groups: exact ends -------------------------------------------------------------------------------
// lconv_i = [MaxPool] Conv k9 - BN - Conv k9 - BN has no nonlinearity (orca_modules.py:811-816, 829-835, 846-852), so the
// library runs it as ONE 17-tap conv with weights composed on the host in fp64 (orca_hip.hip: compose_pair); in stage 1 the
// first conv of conv1 (linear up to its ReLU) joins the group: 25 taps from the bases.  A single conv differs from the chain
// in the 4 (8) outputs next to each end of the chunk: PyTorch zero-pads every INTERMEDIATE there, while the composed conv sees
// the intermediates' virtual values b + (partial window).  Those positions are recomputed with the reference's own step-by-step
// formula in fp32 and overwritten.  (Ends that are halo seams of a longer sequence are discarded by the caller anyway; ends of the
// true sequence are what this is for.)
struct EdgeFixArgs {           // where a chunk's input comes from
  int in_mode;                 // 0: float rows (x, sc, sl; 4 channels)  1: base codes (4 channels)  2: P16 planes  3: B16 planes  (-1: scratch)
  const float* x; long sc, sl;
  const unsigned char* codes; const unsigned char* nmask; long origin; long codes_L, codes_off; int reverse;   // (nmask: p16_base_at)
  const f32x4* xp; long x_plen;
  long n;
};

// A chain of tiny launches, one per conv of the composed group: layer l turns the values at the first / last `half + 4` positions
// (from the chunk's input, or from the previous layer's scratch) into the values at the first / last `half` positions - exactly the
// reference's arithmetic, zero padding of every intermediate included - keeps them in a scratch for the next layer and stores the
// outermost `store_half` of them into the planar tensor the composed conv wrote.  One workgroup per position, threads = (tap half,
// output channel): weight reads coalesced over the channel, 4 or 8 independent loads in flight per thread; ~10 us per layer (the first version - one
// workgroup per OUTPUT recomputing its 9 intermediates with a division per MAC - took 150-760 us per stage).
__device__ __forceinline__ float edge_fix_load(const EdgeFixArgs& a, long pos, int ci) {
  if (pos < 0 || pos >= a.n) return 0.f;
  if (a.in_mode == 0) return a.x[pos * a.sl + ci * a.sc];
  if (a.in_mode == 1) {
    const long P = a.codes_off + pos;
    int c = p16_base_at(a.codes, a.nmask, a.origin, a.reverse ? a.codes_L - 1 - P : P);
    if (a.reverse && c < 4) c = 3 - c;
    return c == 4 ? 0.25f : (c == ci ? 1.f : 0.f);
  }
  if (a.in_mode == 2) {
    const _Float16* u = reinterpret_cast<const _Float16*>(a.xp + (long)(ci >> 3) * 2 * a.x_plen + P16_GUARD + pos);
    const _Float16* l = reinterpret_cast<const _Float16*>(a.xp + ((long)(ci >> 3) * 2 + 1) * a.x_plen + P16_GUARD + pos);
    return (float)u[ci & 7] + (float)l[ci & 7];
  }
  const unsigned short* u = reinterpret_cast<const unsigned short*>(a.xp + (long)(ci >> 3) * a.x_plen + P16_GUARD + pos);
  return __builtin_bit_cast(float, (unsigned)u[ci & 7] << 16);
}

// position handled by slot b of an end list of `half` positions per end: the first `half`, then the last `half` (each position once)
__device__ __forceinline__ long edge_fix_pos(int b, int half, long n) {
  const long p = b < half ? b : n - 2 * half + b;
  return (p < 0 || p >= n || (b >= half && p < half)) ? -1 : p;
}

struct EdgeLayerArgs {
  EdgeFixArgs in;              // layer 1: where the chunk's input comes from (in.in_mode 0..3, in.n); deeper layers: in.in_mode = -1
  const float* sin;            // deeper layers: previous scratch [2 * half_in][128]
  int half_in;                 // = half + 4
  int half, store_half, relu;
  int cin, cout, kc;
  const float* w; const float* b;   // fp32 pack [cin/kc][9][kc][cout], bias
  float* sout;                 // scratch [2 * half][128] (may be NULL for the last layer)
  f32x4* y; long y_plen; int out_fmt;   // planar tensor receiving the outermost store_half positions per end (NULL: none);
                                        // out_fmt 0: P16, 1: B16, 2: fp32 channel-major [cout][y_plen] (the exact-fp32 mode; y_plen = row stride in floats), 3: fp32 channel-last [n][cout]
  unsigned* flag;              // fp16-range guard of the P16 stores (out_fmt 0): the exact end values are not the composed conv's, whose guard saw only its own
};

template <int KC>
__device__ __forceinline__ float edge_layer_dot(const EdgeLayerArgs& a, const float (*xs)[128], int co, int th) {
  // items (chunk c, tap t) of KC MACs each, dealt round-robin to the 4 thread groups; the KC loads of an item are independent
  float acc = 0.f;
  const int nitems = (a.cin / KC) * 9;
  for (int it = th; it < nitems; it += 4) {
    const int c = it / 9, t = it - c * 9;
    const float* w = a.w + ((long)it * KC) * a.cout + co;
    const float* xv = &xs[t][c * KC];
    float wv[KC];
#pragma unroll
    for (int k = 0; k < KC; ++k) wv[k] = w[(long)k * a.cout];
#pragma unroll
    for (int k = 0; k < KC; ++k) acc = fmaf(wv[k], xv[k], acc);
  }
  return acc;
}

static __global__ __launch_bounds__(512) void lconv_edge_layer_kernel(EdgeLayerArgs a) {
  __shared__ float xs[9][128];
  __shared__ float part[3][128];
  const int tid = threadIdx.x, co = tid & 127, th = tid >> 7;
  const long n = a.in.n;
  const long p = edge_fix_pos(blockIdx.x, a.half, n);
  if (p < 0) return;
  for (int idx = tid; idx < 9 * a.cin; idx += 512) {
    const int j = idx / a.cin, ci = idx - j * a.cin;
    const long q = p - 4 + j;
    float v = 0.f;
    if (a.in.in_mode >= 0) v = edge_fix_load(a.in, q, ci);
    else if (q >= 0 && q < n) {      // slot of q in the previous scratch: left list [0, half_in), right list [n - half_in, n)
      const int slot = q < a.half_in ? (int)q : (int)(a.half_in + q - (n - a.half_in));
      v = a.sin[slot * 128 + ci];
    }
    xs[j][ci] = v;
  }
  __syncthreads();
  float acc = 0.f;
  if (co < a.cout) acc = a.kc == 8 ? edge_layer_dot<8>(a, xs, co, th) : edge_layer_dot<4>(a, xs, co, th);
  if (th) part[th - 1][co] = acc;
  __syncthreads();
  if (!th && co < a.cout) {
    acc = a.b[co] + ((acc + part[0][co]) + (part[1][co] + part[2][co]));
    if (a.relu) acc = fmaxf(acc, 0.f);
    if (a.sout) a.sout[blockIdx.x * 128 + co] = acc;
    if (a.y && (p < a.store_half || p >= n - a.store_half)) {
      if (a.out_fmt == 2) {
        reinterpret_cast<float*>(a.y)[(long)co * a.y_plen + p] = acc;
      } else if (a.out_fmt == 3) {            // fp32 channel-last [n][cout]
        reinterpret_cast<float*>(a.y)[p * a.cout + co] = acc;
      } else if (a.out_fmt == 0) {
        const _Float16 h = (_Float16)acc;
        const _Float16 l = (_Float16)(acc - (float)h);
        if (!(fabsf(acc) <= 65504.f) && a.flag) *a.flag = 1u;      // (a NaN raises it too)
        reinterpret_cast<_Float16*>(a.y + (long)(co >> 3) * 2 * a.y_plen + P16_GUARD + p)[co & 7] = h;
        reinterpret_cast<_Float16*>(a.y + ((long)(co >> 3) * 2 + 1) * a.y_plen + P16_GUARD + p)[co & 7] = l;
      } else {
        reinterpret_cast<unsigned short*>(a.y + (long)(co >> 3) * a.y_plen + P16_GUARD + p)[co & 7] = (unsigned short)(cvt_pk_bf16(acc, 0.f) & 0xffffu);
      }
    }
  }
}

// ---- the composed first-layer groups in EXACT fp32 (precision "f32") ------------------------------------------------------------
// out[co][p] = [relu](b[co] + sum_{t < NTAP} sum_{ci < 4} W[t][ci][co] * x[p + t - (NTAP-1)/2][ci]) with fp32 FMAs in a fixed order:
// NTAP = 17 -> lconv1, NTAP = 25 -> conv1.a o lconv1 + ReLU (weights composed on the host in fp64, see orca_hip.hip).  One thread per
// position and 32-channel half; the workgroup's input window sits in LDS, the weights are read as wave-uniform (broadcast) float4.
// 6 400 FMA per position for the 25-tap group against the 73 728 of the 64 -> 64 conv it replaces in this mode.
struct FirstF32Args {
  EdgeFixArgs in;        // in_mode 0 (float rows: x, sc, sl) or 1 (base codes); in.n = positions
  const float* w;        // [NTAP][4][64]
  const float* bias;     // [64]
  float* y;              // [64][ldy] channel-major
  long ldy;
  int relu;
};
template <int NTAP>
__global__ __launch_bounds__(256) void first_taps_f32_kernel(FirstF32Args a) {
  constexpr int H = (NTAP - 1) / 2, PT = 128, WINP = PT + NTAP - 1;
  __shared__ f32x4 xw[WINP];             // window rows: the 4 channels of positions m0 - H ..
  __shared__ f32x4 ws[NTAP * 4 * 16];    // [t][ci][16 float4 = 64 couts]
  __shared__ f32x4 bs[16];
  const int tid = threadIdx.x, pl = tid & (PT - 1), half = tid >> 7;      // half: couts 32 half .. +31
  for (int i = tid; i < NTAP * 4 * 16; i += 256) ws[i] = reinterpret_cast<const f32x4*>(a.w)[i];
  if (tid < 16) bs[tid] = reinterpret_cast<const f32x4*>(a.bias)[tid];
  const long ntiles = (a.in.n + PT - 1) / PT;
  for (long tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const long m0 = tile * PT;
    __syncthreads();                     // previous tile's window reads are done (and, first time, the weights are in)
    for (int i = tid; i < WINP; i += 256) {
      f32x4 v;
      v.x = edge_fix_load(a.in, m0 - H + i, 0); v.y = edge_fix_load(a.in, m0 - H + i, 1);
      v.z = edge_fix_load(a.in, m0 - H + i, 2); v.w = edge_fix_load(a.in, m0 - H + i, 3);
      xw[i] = v;
    }
    __syncthreads();
    f32x4 acc[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) acc[q] = bs[half * 8 + q];
#pragma unroll 1
    for (int t = 0; t < NTAP; ++t) {
      const f32x4 xv = xw[pl + t];
#pragma unroll
      for (int ci = 0; ci < 4; ++ci) {
        const float xs_ = ci == 0 ? xv.x : ci == 1 ? xv.y : ci == 2 ? xv.z : xv.w;
        const f32x4* wr = ws + (t * 4 + ci) * 16 + half * 8;
#pragma unroll
        for (int q = 0; q < 8; ++q) {
          const f32x4 w4 = wr[q];
          acc[q].x = fmaf(w4.x, xs_, acc[q].x); acc[q].y = fmaf(w4.y, xs_, acc[q].y);
          acc[q].z = fmaf(w4.z, xs_, acc[q].z); acc[q].w = fmaf(w4.w, xs_, acc[q].w);
        }
      }
    }
    const long p = m0 + pl;
    if (p < a.in.n) {
#pragma unroll
      for (int q = 0; q < 8; ++q) {
        f32x4 v = acc[q];
        if (a.relu) { v.x = fmaxf(v.x, 0.f); v.y = fmaxf(v.y, 0.f); v.z = fmaxf(v.z, 0.f); v.w = fmaxf(v.w, 0.f); }
        float* yo = a.y + (long)(half * 32 + 4 * q) * a.ldy + p;
        yo[0] = v.x; yo[a.ldy] = v.y; yo[2 * a.ldy] = v.z; yo[3 * a.ldy] = v.w;
      }
    }
  }
}

// RL form of stage 1 (the residual lout1 is computed in conv1.b's epilogue, never stored): the pooled output's windows that touch
// the first / last 4 positions are redone from the chain's scratches - v[p] = relu(conv1.b)[p] + lout1[p] (true values), MaxPool1d(4).
// Block 0: window 0; blocks 1, 2: the last two windows (the earlier one only if it reaches into the last 4 positions).
struct EdgePoolArgs {
  const float* sc; int half_c;     // relu(conv1.b) at the first / last half_c positions   [2 half_c][128]
  const float* sl; int half_l;     // lout1 at the first / last half_l positions            [2 half_l][128]
  long n; int cout;
  f32x4* y; long y_plen; int out_fmt;
  unsigned* flag;                  // fp16-range guard of the P16 stores (out_fmt 0), as in EdgeLayerArgs
};
static __global__ __launch_bounds__(128) void lconv_edge_pool_kernel(EdgePoolArgs a) {
  const long nw = a.n / 4;
  long w;
  if (blockIdx.x == 0) w = 0;
  else {
    w = nw - (long)blockIdx.x;                 // nw-1, nw-2
    if (w <= 0 || 4 * w + 3 < a.n - 4) return; // window 0 is block 0's; untouched windows stay
  }
  if (w >= nw) return;
  const int co = threadIdx.x;
  if (co >= a.cout) return;
  float m = -3.4e38f;
  for (int r = 0; r < 4; ++r) {
    const long p = 4 * w + r;
    const int s1 = p < a.half_c ? (int)p : (int)(a.half_c + p - (a.n - a.half_c));
    const int s2 = p < a.half_l ? (int)p : (int)(a.half_l + p - (a.n - a.half_l));
    m = fmaxf(m, a.sc[s1 * 128 + co] + a.sl[s2 * 128 + co]);
  }
  if (a.out_fmt == 0) {
    const _Float16 h = (_Float16)m;
    const _Float16 l = (_Float16)(m - (float)h);
    if (!(fabsf(m) <= 65504.f) && a.flag) *a.flag = 1u;
    reinterpret_cast<_Float16*>(a.y + (long)(co >> 3) * 2 * a.y_plen + P16_GUARD + w)[co & 7] = h;
    reinterpret_cast<_Float16*>(a.y + ((long)(co >> 3) * 2 + 1) * a.y_plen + P16_GUARD + w)[co & 7] = l;
  } else {
    reinterpret_cast<unsigned short*>(a.y + (long)(co >> 3) * a.y_plen + P16_GUARD + w)[co & 7] = (unsigned short)(cvt_pk_bf16(m, 0.f) & 0xffffu);
  }
}
