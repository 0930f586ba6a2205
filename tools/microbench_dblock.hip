// Ablation micro-benchmark of conv2d_dblock_kernel (one Decoder residual block per launch) and, with DBLOCK_RUN=1, of conv2d_dblock_run_kernel (a run of
// blocks 16, 32, 64 per launch) against the chain of per-block launches.  DBLOCK_BLOCKS=1: only the per-block launches of the three 16-bit modes;
// DBLOCK_V1_ABL=1 / DBLOCK_V2_ABL=1: the ablation ladders of the block kernel / of tools/parked/conv2d_dblock2.h.
// hipcc --offload-arch=gfx950 -O3 -std=c++17 -w -I orca_amd/csrc -I include -I tools tools/microbench_dblock.hip -o tools/microbench_dblock
#include <hip/hip_runtime.h>
#include <cstdio>
#include <vector>
#include "parked/conv2d_dblock2.h"
template <int NS, int DT, int ABL>
static void run(DBlockArgs a, int B, const char* what) {
  hipEvent_t e0, e1; hipEventCreate(&e0); hipEventCreate(&e1);
  float best = 1e9;
  for (int r = 0; r < 6; ++r) {
    hipEventRecord(e0, 0);
    for (int k = 0; k < 10; ++k) hipLaunchKernelGGL((conv2d_dblock_kernel<NS, DT, ABL>), dim3(256, B), dim3(512), 0, 0, a);
    hipEventRecord(e1, 0); hipEventSynchronize(e1);
    float ms; hipEventElapsedTime(&ms, e0, e1); if (r > 0 && ms < best) best = ms;
  }
  printf("NS=%d d=%2d B=%d ABL=%2d (%s): %.1f us per launch  [%s]\n", NS, a.dil, B, ABL, what, best * 100.f, hipGetErrorString(hipGetLastError()));
}
template <int NS, int DT, int PX, int ABL>
static void run2(DBlockArgs a, int B, const char* what) {
  hipEvent_t e0, e1; hipEventCreate(&e0); hipEventCreate(&e1);
  float best = 1e9;
  for (int r = 0; r < 6; ++r) {
    hipEventRecord(e0, 0);
    for (int k = 0; k < 10; ++k) hipLaunchKernelGGL((conv2d_dblock2_kernel<NS, DT, PX, ABL>), dim3(65536 / PX, B), dim3(2 * PX), 0, 0, a);
    hipEventRecord(e1, 0); hipEventSynchronize(e1);
    float ms; hipEventElapsedTime(&ms, e0, e1); if (r > 0 && ms < best) best = ms;
  }
  printf("v2 PX=%d NS=%d d=%2d B=%d ABL=%2d (%s): %.1f us per launch  [%s]\n", PX, NS, a.dil, B, ABL, what, best * 100.f, hipGetErrorString(hipGetLastError()));
}
// one launch of each kernel from the same input: the maps must be bit-identical
template <int NS, int DT, int PX>
static void same(DBlockArgs a, int B, const std::vector<unsigned short>& h, size_t map_units) {
  const size_t bytes = map_units * 16 * B;
  std::vector<unsigned short> o1(bytes / 2), o2(bytes / 2);
  hipMemcpy(a.cur, h.data(), bytes, hipMemcpyHostToDevice);
  hipLaunchKernelGGL((conv2d_dblock_kernel<NS, DT, 0>), dim3(256, B), dim3(512), 0, 0, a);
  hipMemcpy(o1.data(), a.cur, bytes, hipMemcpyDeviceToHost);
  hipMemcpy(a.cur, h.data(), bytes, hipMemcpyHostToDevice);
  hipLaunchKernelGGL((conv2d_dblock2_kernel<NS, DT, PX, 0>), dim3(65536 / PX, B), dim3(2 * PX), 0, 0, a);
  hipMemcpy(o2.data(), a.cur, bytes, hipMemcpyDeviceToHost);
  size_t diff = 0, nz = 0;
  for (size_t i = 0; i < o1.size(); ++i) { diff += o1[i] != o2[i]; nz += o1[i] != 0; }
  printf("same? PX=%d NS=%d DT=%d d=%2d B=%d: %zu of %zu halfwords differ (%zu nonzero)  [%s]\n", PX, NS, DT, a.dil, B, diff, o1.size(), nz, hipGetErrorString(hipGetLastError()));
  hipMemcpy(a.cur, h.data(), bytes, hipMemcpyHostToDevice);
}
// ---- a run of blocks 16, 32, 64 in one launch (conv2d_dblock_run_kernel) against the chain of three per-block launches (DBLOCK_RUN=1) ----
template <int ABL>
static float run_fused(DBlockArgs ra, int B, const char* what) {
  hipEvent_t e0, e1; hipEventCreate(&e0); hipEventCreate(&e1);
  float best = 1e9;
  for (int r = 0; r < 6; ++r) {
    hipEventRecord(e0, 0);
    for (int k = 0; k < 10; ++k) hipLaunchKernelGGL((conv2d_dblock_run_kernel<2, 1, ABL>), dim3(256, B), dim3(512), 0, 0, ra);
    hipEventRecord(e1, 0); hipEventSynchronize(e1);
    float ms; hipEventElapsedTime(&ms, e0, e1); if (r > 0 && ms < best) best = ms;
  }
  printf("run d0=%d nblk=%d B=%d ABL=%d (%s): %.1f us per run  [%s]\n", ra.dil, ra.nblk, B, ABL, what, best * 100.f, hipGetErrorString(hipGetLastError()));
  return best * 100.f;
}
static void launch_chain(DBlockArgs a, int nblk, int B) {
  const int d0 = a.dil;
  for (int b = 0; b < nblk; ++b) { a.dil = d0 << b; hipLaunchKernelGGL((conv2d_dblock_kernel<2, 1, 0>), dim3(256, B), dim3(512), 0, 0, a); }
}
static float run_chain(DBlockArgs a, int nblk, int B) {
  hipEvent_t e0, e1; hipEventCreate(&e0); hipEventCreate(&e1);
  float best = 1e9;
  for (int r = 0; r < 6; ++r) {
    hipEventRecord(e0, 0);
    for (int k = 0; k < 10; ++k) launch_chain(a, nblk, B);
    hipEventRecord(e1, 0); hipEventSynchronize(e1);
    float ms; hipEventElapsedTime(&ms, e0, e1); if (r > 0 && ms < best) best = ms;
  }
  printf("chain d0=%d nblk=%d B=%d (%d per-block launches): %.1f us per chain  [%s]\n", a.dil, nblk, B, nblk, best * 100.f, hipGetErrorString(hipGetLastError()));
  return best * 100.f;
}
// the chain and the run from the same input: the maps must be bit-identical
static void same_run(DBlockArgs a, DBlockArgs ra, int B, const std::vector<unsigned short>& h, size_t map_units) {
  const size_t bytes = map_units * 16 * B;
  std::vector<unsigned short> o1(bytes / 2), o2(bytes / 2);
  hipMemcpy(a.cur, h.data(), bytes, hipMemcpyHostToDevice);
  launch_chain(a, ra.nblk, B);
  hipMemcpy(o1.data(), a.cur, bytes, hipMemcpyDeviceToHost);
  hipMemcpy(a.cur, h.data(), bytes, hipMemcpyHostToDevice);
  hipLaunchKernelGGL((conv2d_dblock_run_kernel<2, 1, 0>), dim3(256, B), dim3(512), 0, 0, ra);
  hipMemcpy(o2.data(), a.cur, bytes, hipMemcpyDeviceToHost);
  size_t diff = 0, nz = 0;
  for (size_t i = 0; i < o1.size(); ++i) { diff += o1[i] != o2[i]; nz += o1[i] != 0; }
  printf("same? run d0=%d nblk=%d B=%d: %zu of %zu halfwords differ (%zu nonzero)  [%s]\n", ra.dil, ra.nblk, B, diff, o1.size(), nz, hipGetErrorString(hipGetLastError()));
  hipMemcpy(a.cur, h.data(), bytes, hipMemcpyHostToDevice);
}
int main() {
  const int n = 250;
  const size_t map = (size_t)8 * 2 * n * 256;           // units of a 64-channel M16 map (NS = 2; the bf16 runs use half of it)
  f32x4* cur; hipMalloc(&cur, map * 16 * 8);
  std::vector<unsigned short> h(map * 8 * 8); unsigned s = 12345u;
  for (auto& v : h) { s = s * 1664525u + 1013904223u; v = (unsigned short)(((s >> 9) & 0x83ff) | 0x3000); }
  hipMemcpy(cur, h.data(), h.size() * 2, hipMemcpyHostToDevice);
  void* w[4]; float* b[4];
  for (int k = 0; k < 4; ++k) {
    const size_t units = (size_t)4 * 2 * 9 * 2 * 64;
    hipMalloc(&w[k], units * 16); hipMalloc(&b[k], 256);
    std::vector<unsigned short> hw(units * 8);
    for (auto& v : hw) { s = s * 1664525u + 1013904223u; v = (unsigned short)(((s >> 9) & 0x83ff) | 0x2000); }
    hipMemcpy(w[k], hw.data(), hw.size() * 2, hipMemcpyHostToDevice); hipMemset(b[k], 0, 256);
  }
  DBlockArgs a{}; a.cur = cur; a.bs = map; a.H = n; a.W = n; a.flag = nullptr;
  for (int k = 0; k < 4; ++k) { a.w[k] = w[k]; a.bias[k] = b[k]; }
  a.bs = map;
  if (getenv("DBLOCK_BLOCKS")) {   // the per-block launches of the three 16-bit modes: f16x2 at B = 2, f16 and bf16 at B = 8
    for (int rep = 0; rep < 6; ++rep)   // the first repetition warms up (clocks, L2): the figures settle from the second on
      for (int d : {16, 32, 64}) { a.dil = d; run<2, 1, 0>(a, 2, "f16x2"); run<1, 1, 0>(a, 8, "f16"); run<1, 0, 0>(a, 8, "bf16"); }
    return 0;
  }
  if (getenv("DBLOCK_RUN")) {
    DBlockArgs ra{}; ra.cur = cur; ra.bs = map; ra.H = n; ra.W = n; ra.flag = nullptr;
    for (int k = 0; k < 12; ++k) { ra.w[k] = w[k & 3]; ra.bias[k] = b[k & 3]; }
    // the pad pixels (columns n .. 255) must hold zero as every Decoder kernel leaves them: the run kernel keeps 0 for the grid pixels outside the
    // map where the per-block launches gather pad pixel 255 of row 0 again
    std::vector<unsigned short> hz(h);
    for (size_t u = 0; u < hz.size() / 8; ++u)
      if ((int)(u & 255) >= n) for (int e = 0; e < 8; ++e) hz[u * 8 + e] = 0;
    for (int d0 : {16, 32}) {
      a.dil = d0; ra.dil = d0; ra.nblk = d0 == 16 ? 3 : 2;
      same_run(a, ra, 2, hz, map);
    }
    hipMemcpy(cur, h.data(), h.size() * 2, hipMemcpyHostToDevice);
    a.dil = 16; ra.dil = 16; ra.nblk = 3;
    for (int rep = 0; rep < 3; ++rep)
      for (int B : {1, 2, 4, 8}) {
        const float tc = run_chain(a, 3, B), tf = run_fused<0>(ra, B, "full");
        printf("  B=%d: run / chain = %.3f (saves %.1f us)\n", B, tf / tc, tc - tf);
      }
    for (int B : {1, 2})
      for (int rep = 0; rep < 2; ++rep) {
        run_fused<0>(ra, B, "full");
        run_fused<1>(ra, B, "no MFMA");
        run_fused<2>(ra, B, "no W DMA behind the first three pieces");
        run_fused<4>(ra, B, "no gather");
        run_fused<1 + 2>(ra, B, "no MFMA, no W DMA");
        run_fused<1 + 2 + 4>(ra, B, "barriers, operand reads, epilogues, scatter");
      }
    return 0;
  }
  for (int d : {32, 64}) { a.dil = d; same<2, 1, 128>(a, 2, h, map); same<1, 1, 128>(a, 2, h, map); same<1, 0, 128>(a, 2, h, map); }
  for (int d : {16, 32, 64}) { a.dil = d; same<2, 1, 256>(a, 2, h, map); same<1, 0, 256>(a, 2, h, map); }
  for (int d : {32, 64}) {
    a.dil = d;
    for (int B : {1, 2, 4, 8}) { run<2, 1, 0>(a, B, "v1"); run2<2, 1, 128, 0>(a, B, "v2"); run2<2, 1, 256, 0>(a, B, "v2"); }
    for (int B : {2, 8}) { run<1, 1, 0>(a, B, "v1 f16"); run2<1, 1, 128, 0>(a, B, "v2 f16"); run2<1, 1, 256, 0>(a, B, "v2 f16"); }
  }
  a.dil = 16;
  for (int B : {1, 2, 4, 8}) { run<2, 1, 0>(a, B, "v1"); run2<2, 1, 256, 0>(a, B, "v2"); }
  for (int B : {2, 8}) { run<1, 1, 0>(a, B, "v1 f16"); run2<1, 1, 256, 0>(a, B, "v2 f16"); }
  if (getenv("DBLOCK_V1_ABL")) {
    for (int d : {16, 32, 64}) {
      a.dil = d;
      for (int rep = 0; rep < 2; ++rep) {
        run<2, 1, 0>(a, 2, "v1 full");
        run<2, 1, 1>(a, 2, "no MFMA");
        run<2, 1, 2>(a, 2, "no W DMA in the loop");
        run<2, 1, 4>(a, 2, "no gather");
        run<2, 1, 8>(a, 2, "no operand reads");
        run<2, 1, 16>(a, 2, "one barrier per layer");
        run<2, 1, 1 + 8>(a, 2, "no MFMA, no operand reads");
        run<2, 1, 1 + 2 + 8>(a, 2, "no MFMA, no reads, no DMA");
        run<2, 1, 1 + 2 + 4 + 8>(a, 2, "only barriers + epilogues");
        run<2, 1, 1 + 2 + 4 + 8 + 16>(a, 2, "only epilogues");
      }
    }
    return 0;
  }
  if (getenv("DBLOCK_V2_ABL")) {
    for (int d : {32, 64}) {
      a.dil = d;
      for (int rep = 0; rep < 2; ++rep) {
      run<2, 1, 0>(a, 2, "v1 full");
      run2<2, 1, 128, 0>(a, 2, "full");
      run2<2, 1, 128, 1>(a, 2, "no MFMA");
      run2<2, 1, 128, 2>(a, 2, "no W DMA in the loop");
      run2<2, 1, 128, 4>(a, 2, "no gather");
      run2<2, 1, 128, 8>(a, 2, "no operand reads");
      run2<2, 1, 128, 16>(a, 2, "one barrier per layer");
      run2<2, 1, 128, 2 + 16>(a, 2, "no W DMA, one barrier per layer");
      run2<2, 1, 128, 1 + 8>(a, 2, "no MFMA, no operand reads");
      run2<2, 1, 128, 1 + 2 + 8>(a, 2, "no MFMA, no reads, no DMA");
      run2<2, 1, 128, 1 + 2 + 4 + 8>(a, 2, "only barriers + epilogues");
      run2<2, 1, 128, 1 + 2 + 4 + 8 + 16>(a, 2, "only epilogues");
      }
    }
    return 0;
  }
  if (getenv("DBLOCK_V2_ONLY")) return 0;
  for (int d : {16, 32, 64}) {
    a.dil = d;
    run<2, 1, 0>(a, 1, "full");
    run<2, 1, 0>(a, 2, "full");
    run<2, 1, 0>(a, 8, "full");
  }
  a.dil = 16;
  run<2, 1, 1>(a, 1, "no MFMA");
  run<2, 1, 2>(a, 1, "no W DMA in the loop");
  run<2, 1, 4>(a, 1, "no gather");
  run<2, 1, 64>(a, 1, "no XCD grouping of the sub-images");
  run<2, 1, 8>(a, 1, "no operand reads");
  run<2, 1, 16>(a, 1, "one barrier per layer");
  run<2, 1, 1 + 8>(a, 1, "no MFMA, no operand reads");
  run<2, 1, 1 + 2 + 8>(a, 1, "no MFMA, no reads, no DMA");
  run<2, 1, 1 + 2 + 4 + 8>(a, 1, "only barriers + epilogues");
  run<1, 0, 0>(a, 1, "bf16 full");
  run<1, 0, 0>(a, 8, "bf16 full");
  return 0;
}
