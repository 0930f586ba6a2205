// conv2d_dblock.h - whole dilated residual blocks of the Decoders in ONE launch, for dilations >= 16, on M16 maps (conv2d_m16.h):
// conv2d_dblock_kernel runs one block, conv2d_dblock_run_kernel a run of blocks of dilations 16, 32 (, 64); both are dblock_body.
//
// A Decoder is 28 (Decoder_1m: 19) blocks   oth = lm(cur) + cur;  cur = m(oth) + oth   of four 3x3 convolutions
// 64 -> 32 -> 64 -> 32 -> 64 that all share one dilation d (orca_modules.py:22-422, :477-486; dilations 1..64 cycling).
// A 3x3 conv with dilation d only ever combines pixels whose rows AND columns are congruent mod d: the 250 x 250 map is
// d*d independent sub-images of ceil(250/d)^2 pixels (16x16 at d = 16, 8x8 at 32, 4x4 at 64) on each of which the block
// is four PLAIN 3x3 convs with zero padding at the sub-image border (= the map border).  A workgroup takes 256 pixels'
// worth of sub-images (1 / 4 / 16 of them), gathers their units, and runs the four convs back to back out of LDS: no halo,
// no recompute, no intermediate map in HBM, the result written IN PLACE - 1 launch and 1 read + 1 write of the map
// instead of 4 launches and 4 reads (each 3x) + 4 writes.
//
// LDS: A = 64-channel operand image [split][8 octets][256 px + 16 zero units], B = the 32-channel one, W ring of three pieces
// [split][9 taps][2][32 couts]; 157 KB in f16x2, 79 KB in bf16.  The gather is LDS-DMA straight from the M16 planes (the
// units ARE the operand image; a pixel outside the map is fetched from a zero pad pixel).  A lane's operand for tap (dy, dx)
// is the unit of pixel p + dy*S + dx of its sub-image (S = side) or the zero unit when that leaves the sub-image: the padding
// costs one address select per read.  The residuals (cur for lm, oth for m) are read back from the A image in the MFMA
// layout (hi + lo), the result goes out as whole 16-byte units per lane (P16 recipe).  Weights stream as 18 KB pieces
// through the ring, issued two pieces ahead, counted waits, one barrier per piece.
//
// A RUN of consecutive blocks of dilations dil, 2 dil (, 4 dil) <= 64 in one launch: in both Decoders the blocks of dilation >= 16 only
// occur as runs 16, 32, 64.  Rows and columns congruent mod 32 are congruent mod 16: the sub-image of dilation dil a workgroup has
// gathered holds every pixel the blocks of dilation 2 dil and 4 dil combine for its pixels, only the neighbour stride in the S x S grid
// changes - block b reads p + (dy S + dx) << b, or the zero unit when pr + (dy << b) or pc + (dx << b) leaves [0, S) (grid pixels outside
// the map hold zero: the gather fetched them from the pad pixel, `put` writes 0 for !pvalid - the zero padding of the larger dilations).
// The geometry (pix, XCD placement, gather, final scatter) is the one of dilation dil for the whole run; between the blocks the residual
// stream stays in the A image: the second and third gather, the first and second scatter and two launches are gone.
//   * the weight ring runs through the block boundaries (pieces 16 nblk, numbered globally; 16 % 3 = 1: the ring slots rotate by one per
//     block); the counted waits of pieces 0-2 that cover the gather apply in the first block only, vmcnt(0) at the very last piece only;
//   * the biases of all blocks are loaded up front (48 units per block);
//   * an intermediate block's last epilogue splits with p16_split_hl - the very instructions whose result a per-block launch stores and the
//     next gather reads back - and raises the overflow flag as that launch does: the run is bit-identical to the chain of per-block launches;
//   * the blocks are a RUNTIME loop around the sixteen unrolled pieces: three unrolled copies would fill the 64 KB instruction cache two
//     CUs share.
// Figures of the gfx950 build (symbol size in the code object, VGPRs, scratch bytes per lane, LDS bytes, workgroups per CU):
//   conv2d_dblock_run_kernel<2, 1>  23 152 bytes, 228 VGPRs, no scratch, 162 048 bytes of LDS (160 512 + 96 more bias units), 1
//   conv2d_dblock_kernel<2, 1>      21 872 bytes, 182 VGPRs, no scratch, 160 512, 1
//   conv2d_dblock_kernel<1, 0>      13 076 bytes, 120 VGPRs, no scratch,  80 640, 2
//   conv2d_dblock_kernel<1, 1>      14 304 bytes, 128 VGPRs, 100 (held to 128 VGPRs for the second workgroup; tests/test_build_cpu.py tolerates 128), 80 640, 2
#pragma once
#include "conv2d_m16.h"

struct DBlockArgs {
  f32x4* cur;              // 64-channel M16 map, updated in place
  const void* w[12];       // per block lm.a (64->32), lm.b (32->64), m.a (64->32), m.b (32->64): packs [cin/16][NS][9][2][cout][8]
  const float* bias[12];
  long bs;                 // batch stride (units)
  int H, W, dil, nblk;     // block b has dilation dil << b <= 64; nblk = 2 or 3 (conv2d_dblock_kernel: one block, nblk is not read)
  unsigned* flag;
};

// The block's result goes out with PLAIN (write-back) stores, unlike the per-layer kernels' write-through ones (m16_store_unit): a workgroup's units are
// scattered - dilation 16: 16 bytes of every 128-byte line, 32: 64 bytes - and the 8 workgroups that share a line sit on one XCD, so its L2 merges them
// into whole lines before they leave; written through, every unit went out as its own partial line.  tools/microbench_dblock.hip, us per launch at
// B = 2, write-through -> write-back: d = 16 66.8 -> 55.5, d = 32 74.5 -> 61.7, d = 64 52.8 -> 48.0; single fp16 plane, B = 8: 106 -> 86, 108 -> 85,
// 84 -> 77 (round 5; DBLOCK_STORE_WT=1 at compile time: the write-through form).
#ifndef DBLOCK_STORE_WT
#define DBLOCK_STORE_WT 0
#endif
__device__ __forceinline__ void db_store_unit(u32x4_t* p, const u32x4_t& v) {
#if DBLOCK_STORE_WT
  m16_store_unit(p, v);
#else
  *p = v;
#endif
}

template <int N>
__device__ __forceinline__ void db_vmwait() { asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory"); }

// MAXBLK = 1: one block (nblk, first, last, the ring slots, the bias offset and the neighbour stride are constants: no block loop is left);
// MAXBLK = 3: a run of a.nblk blocks.
// ABL (tools/microbench_dblock.hip only, 0 in the library): 1 = no MFMAs, 2 = no weight DMA behind the first three pieces, 4 = no gather,
// 8 = no operand reads, 16 = one barrier per layer instead of per piece (timing only: races), 64 = no XCD grouping of the sub-images
template <int NS, int DT, int MAXBLK, int ABL>
__device__ __forceinline__ void dblock_body(const DBlockArgs& a) {
  // Runs are f16x2 only: the single-plane modes run two workgroups per CU on 2 x 80 640 bytes of LDS, which has no room for the 96 more
  // bias units, and keep their per-block launches.
  static_assert(MAXBLK == 1 || (NS == 2 && DT == 1), "block runs: f16x2 only");
  constexpr int WNS = DT == 1 ? 2 : 1;               // splits in the weight pack (the fp16 pack always carries hi and lo)
  constexpr int NT = 512, PXW = 256 + 16;            // 256 pixels + 16 zero units (one per bank slot of a 16-lane read group, see nb16)
  constexpr int AU = NS * 8 * PXW, BU = NS * 4 * PXW; // operand images (16-byte units)
  constexpr int WP = NS * 9 * 2 * 32;                // one weight piece: 16 input channels x 32 couts
  constexpr int WIT = (WP + NT - 1) / NT;
  static_assert(NS * 8 * 256 / NT == 4 * NS, "gather: NS DMA instructions per thread and K-chunk of the first layer (the same for every wave)");
  constexpr int EXTRA = (WP - (WIT - 1) * NT + 63) / 64;     // waves that issue WIT (the others WIT - 1) DMA instructions per piece
  __shared__ f32x4 smem[AU + BU + 3 * WP + 48 * MAXBLK];
  f32x4* const As = smem;
  f32x4* const Bs = smem + AU;
  f32x4* const Ws = smem + AU + BU;
  float* const bias_s = reinterpret_cast<float*>(smem + AU + BU + 3 * WP);   // per block [32 | 64 | 32 | 64]

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int l31 = lane & 31, g = lane >> 5;
  const int d = a.dil, H = a.H, W = a.W;                // d = 16 / 32 / 64
  const int nblk = MAXBLK == 1 ? 1 : a.nblk;
  const int ld = 31 - __builtin_clz(d);                 // log2(d)
  const int lS = 8 - ld, S = 1 << lS;                   // sub-image side 16 / 8 / 4
  const int lG = 2 * ld - 8, G = 1 << lG;               // sub-images per workgroup 1 / 4 / 16 (all in one row of sub-images)
  f32x4* const cur = a.cur + (long)blockIdx.y * a.bs;

  // Workgroups go to the XCDs round-robin (b % 8); 8 consecutive pixels of a map row (one 128-byte line of a plane) belong to
  // 8 consecutive sub-image columns j0: the workgroups holding them are placed on ONE XCD (32 per XCD = 4 runs of 8 columns at
  // d = 16, 2 workgroups x 4 columns at d = 32), so that a line is fetched into one L2 only.
  int bx = (int)blockIdx.x;
  if (!(ABL & 64)) {
    const int xcd = bx & 7, t = bx >> 3;                // t = 0..31 on this XCD
    if (G == 1) { const int run = xcd * 4 + (t >> 3); bx = (run >> 1) * 16 + (run & 1) * 8 + (t & 7); }       // sid = i0*16 + j0
    else if (G == 4) { const int pair = xcd * 16 + (t >> 1); bx = pair * 2 + (t & 1); }                        // workgroup = 4 columns: pairs
  }
  auto pix = [&](int p, int& row, int& col, int& r, int& c) {
    const int sid = (bx << lG) + (p >> (2 * lS)), q = p & ((1 << (2 * lS)) - 1);
    r = q >> lS; c = q & (S - 1);
    row = (sid >> ld) + (r << ld);
    col = (sid & (d - 1)) + (c << ld);
  };
  {   // workgroup-uniform early exit (small maps): its sub-images start at row i0, columns j0 .. j0 + G - 1
    const int sid0 = bx << lG;
    if ((sid0 >> ld) >= H || (sid0 & (d - 1)) >= W) return;
  }

  // ---- zero units: BEFORE the first DMA (a visible LDS store behind a pending DMA makes the compiler wait for it) ----
  if (tid < NS * 8 * 16) As[(tid >> 4) * PXW + 256 + (tid & 15)] = (f32x4)(0.f);
  if (tid >= 256 && tid < 256 + NS * 4 * 16) Bs[((tid - 256) >> 4) * PXW + 256 + (tid & 15)] = (f32x4)(0.f);
  __syncthreads();
  // ---- a block's four biases [32 | 64 | 32 | 64] by ONE DMA instruction of wave 0 (48 lanes x 16 bytes, per-lane sources): a register-staged
  // copy put a global-load round trip in front of the gather.  They are the wave's oldest transfers: every counted wait below covers them ----
  if (wave == 0 && lane < 48) {
#pragma unroll
    for (int b = 0; b < MAXBLK; ++b)
      if (b < nblk) {
        const float *b0 = a.bias[4 * b], *b1 = a.bias[4 * b + 1], *b2 = a.bias[4 * b + 2], *b3 = a.bias[4 * b + 3];
        const float* src = lane < 8 ? b0 + 4 * lane : (lane < 24 ? b1 + 4 * (lane - 8) : (lane < 32 ? b2 + 4 * (lane - 24) : b3 + 4 * (lane - 32)));
        p16_glds16(reinterpret_cast<const f32x4*>(src), smem + AU + BU + 3 * WP + 48 * b);
      }
  }

  // ---- weight pieces: piece i = 0..15 of a block = (layer i / 4, K-chunk k, cout half h); `wl` = the pack of its layer, `slot` = its ring
  // slot (units).  Layers 0 / 2 (64 -> 32): pieces k = 0..3;  layers 1 / 3 (32 -> 64): h = 0: k = 0, 1;  h = 1: k = 0, 1 ----
  auto issue_piece = [&](const void* wl, int i, int slot) {
    const int L = i >> 2, j = i & 3;
    const bool wide = L & 1;                         // 32 -> 64
    const int k = wide ? (j & 1) : j, h = wide ? (j >> 1) : 0, cout = wide ? 64 : 32;
    f32x4* dst = Ws + slot;
#pragma unroll
    for (int it = 0; it < WIT; ++it) {
      const int u = tid + it * NT;
      const int grp = u >> 5, co = u & 31;           // grp = (s*9 + tap)*2 + g
      if (u < WP) p16_glds16(reinterpret_cast<const f32x4*>(wl) + ((long)k * (WNS * 9 * 2) + grp) * cout + h * 32 + co, dst + it * NT + wave * 64);
    }
  };
  // ring slots of pieces i % 3 = 0, 1, 2 of the CURRENT block (global piece 16 b + i sits in slot (b + i) % 3)
  int ro0 = 0, ro1 = WP, ro2 = 2 * WP;
  // ---- gather: the units of the workgroup's 256 pixels, all 8 octets x NS planes, by LDS-DMA; a pixel outside the map is
  // fetched from pad pixel 255 of row 0 (zero; maps with W = 256 have no outside pixels).  Issued K-CHUNK BY K-CHUNK of the first layer
  // (octets 2k, 2k + 1 of every split), the first block's first three weight pieces in between: piece k of layer 0 waits for chunk k alone
  // (counted waits in DB_LAYER), so three quarters of the cold gather run under the first pieces' MFMAs ----
  {
    int row, col, r_, c_;
    pix(tid & 255, row, col, r_, c_);
    const bool ok = row < H && col < W;
    const long off = ok ? (long)row * M16_PX + col : 255;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
#pragma unroll
      for (int s_ = 0; s_ < NS; ++s_) {
        const int plane = s_ * 8 + 2 * k + (wave >> 2);            // = s*8 + o
        if (!(ABL & 4)) p16_glds16(cur + m16_plane(plane & 7, s_, NS, H) + off, As + plane * PXW + (wave & 3) * 64);
      }
      if (k < 3) issue_piece(a.w[0], k, k * WP);
    }
  }

  // ---- this lane's pixel in the MFMA layout ------------------------------------------------------------------------
  const int p = wave * 32 + l31;
  int prow, pcol, pr, pc;
  pix(p, prow, pcol, pr, pc);
  const bool pvalid = prow < H && pcol < W;
  const long poff = (long)prow * M16_PX + pcol;

  f32x16 acc[2];
  const unsigned as_lds = p16_lds_addr(As), bs_lds = p16_lds_addr(Bs), ws_lds = p16_lds_addr(Ws + g * 32 + l31);
  bool overflow = false;
  // 4 consecutive couts of the lane's pixel -> the 8-byte half g of the units of octet `oct` in image X (XG octets per split)
  auto put = [&](f32x4* Xs, int XG, int oct, f32x4 v) {
    if (!pvalid) v = (f32x4)(0.f);
    u32x2 sp[NS];
    split4<NS, DT>(v, sp, overflow);
#pragma unroll
    for (int s = 0; s < NS; ++s) *reinterpret_cast<u32x2*>(reinterpret_cast<char*>(Xs + (s * XG + oct) * PXW + p) + 8 * g) = sp[s];
  };
  // the same 4 channels of the 64-channel image A as fp32 (hi + lo): the block's residual stream
  auto get_A = [&](int oct) -> f32x4 {
    float f[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int s = 0; s < NS; ++s) {
      const u32x2 u = *reinterpret_cast<const u32x2*>(reinterpret_cast<const char*>(As + (s * 8 + oct) * PXW + p) + 8 * g);
      float a0, a1, a2, a3;
      m16_pair<DT>(u.x, a0, a1);
      m16_pair<DT>(u.y, a2, a3);
      f[0] += a0; f[1] += a1; f[2] += a2; f[3] += a3;
    }
    f32x4 r;
    r.x = f[0]; r.y = f[1]; r.z = f[2]; r.w = f[3];
    return r;
  };
  auto acc4 = [&](int h, int q, const float* bl, bool relu) -> f32x4 {
    const f32x4 b = *reinterpret_cast<const f32x4*>(bl + 8 * q + 4 * g);
    f32x4 v;
    v.x = acc[h][4 * q + 0] + b.x; v.y = acc[h][4 * q + 1] + b.y; v.z = acc[h][4 * q + 2] + b.z; v.w = acc[h][4 * q + 3] + b.w;
    if (relu) { v.x = p16_vmax(v.x, 0.f); v.y = p16_vmax(v.y, 0.f); v.z = p16_vmax(v.z, 0.f); v.w = p16_vmax(v.w, 0.f); }
    return v;
  };
  auto zero_acc = [&]() {
#pragma unroll
    for (int h = 0; h < 2; ++h)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[h][r] = 0.f;
  };
  // The operand reads are inline asm with counted waits, as in conv_p16.h: with an LDS-DMA in flight the compiler would
  // put s_waitcnt vmcnt(0) in front of every LDS read it can see.
#define DB_READ(buf_, t_)                                                                                         \
  _Pragma("unroll") for (int s = 0; s < NS; ++s) {                                                                \
    xv[buf_][s] = p16_lds_read16(xrow + nb16[t_], s * XG * PXW * 16);                                             \
    wv[buf_][s] = p16_lds_read16(wrow, ((s * 9 + (t_)) * 2) * 32 * 16);                                           \
  }
  // Layer LY (0..3) of a block = weight pieces 4 LY .. 4 LY + 3.  WIDE: 32 -> 64 (pieces (h, k) = (0,0) (0,1) (1,0) (1,1)), else 64 -> 32
  // (k = 0..3).  At a piece's wait its weights (and, pieces 0-2 of the first block, its K-chunk of the gather) must have landed; what was
  // issued behind them may stay in flight, per wave (waves < EXTRA issue WIT, the others WIT - 1 instructions per weight piece; every wave NS
  // per gather chunk): first block, piece 0: G1 W1 G2 W2 G3, piece 1: G2 W2 G3, piece 2: G3 W3; EVERY other piece of the launch, block
  // boundaries included: exactly the next piece's weights (piece i + 2 goes out behind piece i's barrier, so at piece i + 1's wait pieces
  // i + 1 and i + 2 are the youngest and i + 2 may stay in flight); the launch's last piece: nothing.  Pieces 14 and 15 of a block that is not
  // the last issue pieces 0 and 1 of the next block; piece 0 of a later block issues its piece 2 (the first block's went out with the gather).
  // The barrier - this piece has landed for every wave, and everyone is done with the buffer piece + 2 goes into - is a BARE one behind the
  // wave's own LDS traffic (the `put`s of the previous layer): __syncthreads() compiles to s_waitcnt vmcnt(0) lgkmcnt(0) + s_barrier and
  // retired the weight piece in flight at every piece (conv2d_m16.h).
#define DB_WAIT(NG, NW) /* NG gather chunks and NW weight pieces may stay in flight */                           \
  if (wave < EXTRA) db_vmwait<(NG) * NS + (NW) * WIT>(); else db_vmwait<(NG) * NS + (NW) * (WIT - 1)>()
#define DB_LAYER(LY, XLDS, XG_, WIDE)                                                                             \
  {                                                                                                               \
    constexpr int XG = XG_;                                                                                       \
    _Pragma("unroll") for (int j = 0; j < 4; ++j) {                                                               \
      constexpr bool wide_ = WIDE;                                                                                \
      const int piece = 4 * (LY) + j;                                                                             \
      const int k = wide_ ? (j & 1) : j;                                                                          \
      const int h = wide_ ? (j >> 1) : 0;                                                                         \
      if (piece <= 2 && first) {                                                                                  \
        if (piece == 0) { DB_WAIT(3, 2); } else if (piece == 1) { DB_WAIT(2, 1); } else { DB_WAIT(1, 1); }        \
      } else if (piece == 15 && last) db_vmwait<0>();                                                             \
      else { DB_WAIT(0, 1); }                                                                                     \
      if (!(ABL & 16) || j == 0) asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");                  \
      if (!(ABL & 2)) {                                                                                           \
        const int slot2 = (piece + 2) % 3 == 0 ? ro0 : ((piece + 2) % 3 == 1 ? ro1 : ro2);                        \
        if (piece == 0) { if (!first) issue_piece(wb[0], 2, slot2); }                                             \
        else if (piece >= 14) { if (!last) issue_piece(wb[4], piece - 14, slot2); }                               \
        else issue_piece(wb[(piece + 2) >> 2], piece + 2, slot2);                                                 \
      }                                                                                                           \
      const unsigned wrow = ws_lds + (unsigned)((piece % 3 == 0 ? ro0 : (piece % 3 == 1 ? ro1 : ro2)) * 16);     \
      const unsigned xrow = (XLDS) + (unsigned)((2 * k + g) * PXW * 16);                                          \
      f16x8 xv[2][NS], wv[2][NS];                                                                                 \
      DB_READ(0, 0);                                                                                              \
      _Pragma("unroll") for (int t = 0; t < 9; ++t) {                                                             \
        const int fb = t & 1;                                                                                     \
        if (t + 1 < 9) { if (!(ABL & 8)) { DB_READ(fb ^ 1, t + 1); m16_wait<2 * NS, NS>(xv[fb], wv[fb]); } }      \
        else m16_wait<0, NS>(xv[fb], wv[fb]);                                                                     \
        typedef typename Op16<DT>::vec V_;                                                                        \
        if constexpr ((ABL & 1) != 0) { asm volatile("" ::"v"(xv[fb][0]), "v"(wv[fb][0])); } else                \
        if constexpr (NS == 2) {                                                                                  \
          acc[h] = Op16<DT>::mfma(__builtin_bit_cast(V_, wv[fb][0]), __builtin_bit_cast(V_, xv[fb][NS - 1]), acc[h]); \
          acc[h] = Op16<DT>::mfma(__builtin_bit_cast(V_, wv[fb][NS - 1]), __builtin_bit_cast(V_, xv[fb][0]), acc[h]); \
        }                                                                                                         \
        if constexpr ((ABL & 1) == 0) acc[h] = Op16<DT>::mfma(__builtin_bit_cast(V_, wv[fb][0]), __builtin_bit_cast(V_, xv[fb][0]), acc[h]); \
        __builtin_amdgcn_sched_barrier(0);                                                                        \
      }                                                                                                           \
    }                                                                                                             \
  }

  float vmax = 0.f;
#pragma unroll 1
  for (int bi = 0; bi < nblk; ++bi) {
    const int b = MAXBLK == 1 ? 0 : bi;
    const bool first = b == 0, last = MAXBLK == 1 || b + 1 == nblk;
    // this block's four weight packs and the next block's first
    const void* wb[5];
#pragma unroll
    for (int q = 0; q < 5; ++q) wb[q] = a.w[4 * b + (q < 4 || !last ? q : 0)];
    const float* const bl = bias_s + 192 * b;
    // byte offset of the tap's source unit within a plane: the neighbour at stride 1 << b of the S x S grid.  Outside the sub-image: a zero
    // unit - the one in the SAME bank slot as the unit the lane would have read (256 + (q & 15)): the 16 lanes of a ds_read_b128 group read
    // 16 consecutive units = all 64 banks, so a single zero unit collided with one of them whenever a group mixed inside and outside lanes
    // (SQ_LDS_BANK_CONFLICT 18.7 % of SQ_LDS_IDX_ACTIVE, round 4)
    unsigned nb16[9];
#pragma unroll
    for (int t = 0; t < 9; ++t) {
      const int dy = (t / 3 - 1) * (1 << b), dx = (t % 3 - 1) * (1 << b);
      const bool in = (unsigned)(pr + dy) < (unsigned)S && (unsigned)(pc + dx) < (unsigned)S;
      nb16[t] = (in ? (unsigned)(p + dy * S + dx) : 256u + ((unsigned)(p + dy * S + dx) & 15u)) * 16u;
    }
    // ---- lm.a: 64 -> 32, linear ----
    zero_acc();
    DB_LAYER(0, as_lds, 8, false);
#pragma unroll
    for (int q = 0; q < 4; ++q) put(Bs, 4, q, acc4(0, q, bl, false));
    // ---- lm.b: 32 -> 64, linear, + cur (read back from A) -> oth -> A (a lane rewrites exactly the bytes it has read) ----
    zero_acc();
    DB_LAYER(1, bs_lds, 4, true);
#pragma unroll
    for (int h = 0; h < 2; ++h)
#pragma unroll
      for (int q = 0; q < 4; ++q) put(As, 8, h * 4 + q, acc4(h, q, bl + 32 + h * 32, false) + get_A(h * 4 + q));
    // ---- m.a: 64 -> 32, ReLU ----
    zero_acc();
    DB_LAYER(2, as_lds, 8, false);
#pragma unroll
    for (int q = 0; q < 4; ++q) put(Bs, 4, q, acc4(0, q, bl + 96, true));
    // ---- m.b: 32 -> 64, ReLU, + oth (from A) -> cur: the last block stores it (HBM, in place, whole 16-byte units per lane), the others
    // leave it in A as the very units that store would have written and the next block's gather read back (p16_split_hl; 0 outside the map) ----
    zero_acc();
    DB_LAYER(3, bs_lds, 4, true);
    if constexpr (NS == 2) {
#pragma unroll
      for (int h = 0; h < 2; ++h)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          f32x4 v = acc4(h, q, bl + 128 + h * 32, true) + get_A(h * 4 + q);
          vmax = p16_vmax3_abs(p16_vmax3_abs(vmax, v.x, v.y), v.z, v.w);
          if (!last && !pvalid) v = (f32x4)(0.f);
          unsigned h0_, h1_, l0_, l1_;
          p16_split_hl(v, h0_, h1_, l0_, l1_);
          if (last) {
            p16_swap32(h0_, l0_);          // g = 0: the hi unit of octet h*4 + q, g = 1: its lo unit
            p16_swap32(h1_, l1_);
            u32x4_t unit_;
            unit_.x = h0_; unit_.y = h1_; unit_.z = l0_; unit_.w = l1_;
            if (pvalid) db_store_unit(reinterpret_cast<u32x4_t*>(cur) + m16_plane(h * 4 + q, g, NS, H) + poff, unit_);
          } else {
            u32x2 hi_, lo_;
            hi_.x = h0_; hi_.y = h1_; lo_.x = l0_; lo_.y = l1_;
            *reinterpret_cast<u32x2*>(reinterpret_cast<char*>(As + (h * 4 + q) * PXW + p) + 8 * g) = hi_;
            *reinterpret_cast<u32x2*>(reinterpret_cast<char*>(As + (8 + h * 4 + q) * PXW + p) + 8 * g) = lo_;
          }
        }
    } else {   // single plane: one unit per octet pair
#pragma unroll
      for (int h = 0; h < 2; ++h)
#pragma unroll
        for (int qp = 0; qp < 2; ++qp) {
          const f32x4 v0 = acc4(h, 2 * qp, bl + 128 + h * 32, true) + get_A(h * 4 + 2 * qp);
          const f32x4 v1 = acc4(h, 2 * qp + 1, bl + 128 + h * 32, true) + get_A(h * 4 + 2 * qp + 1);
          if (DT == 1) vmax = p16_vmax3_abs(p16_vmax3_abs(p16_vmax3_abs(p16_vmax3_abs(vmax, v0.x, v0.y), v0.z, v0.w), v1.x, v1.y), v1.z, v1.w);
          unsigned a0_ = m16_pk2<DT>(v0.x, v0.y), a1_ = m16_pk2<DT>(v0.z, v0.w), b0_ = m16_pk2<DT>(v1.x, v1.y), b1_ = m16_pk2<DT>(v1.z, v1.w);
          p16_swap32(a0_, b0_);          // g = 0: the unit of octet h*4 + 2 qp, g = 1: of the next octet
          p16_swap32(a1_, b1_);
          u32x4_t unit_;
          unit_.x = a0_; unit_.y = a1_; unit_.z = b0_; unit_.w = b1_;
          if (pvalid) db_store_unit(reinterpret_cast<u32x4_t*>(cur) + m16_plane(h * 4 + 2 * qp + g, 0, NS, H) + poff, unit_);
        }
    }
    if constexpr (MAXBLK > 1) { const int t_ = ro0; ro0 = ro1; ro1 = ro2; ro2 = t_; }
  }
#undef DB_LAYER
#undef DB_WAIT
#undef DB_READ
  if (DT == 1 && pvalid && vmax > 65504.f) overflow = true;
  if (DT == 1 && overflow && a.flag) *a.flag = 1u;
}

template <int NS, int DT, int ABL = 0>
__global__ __launch_bounds__(512, NS == 1 ? 4 : 2) void conv2d_dblock_kernel(DBlockArgs a) {   // bf16: 79 KB of LDS, two workgroups per CU if <= 128 VGPRs
  dblock_body<NS, DT, 1, ABL>(a);
}

template <int NS, int DT, int ABL = 0>
__global__ __launch_bounds__(512, 2) void conv2d_dblock_run_kernel(DBlockArgs a) {
  dblock_body<NS, DT, 3, ABL>(a);
}
