// Round 6 lab: what does a kernel's FIRST touch of memory it has not seen for a while cost beyond the cache miss - i.e. do address translations matter for
// the decode chain, whose 229 launches per step each stream a different 3-13 MB weight matrix out of a 1.6 GB set?
//   tools/bin/tlb_lab [launches]
// A chain of dependent launches (same stream), each a skinny-GEMM-like read of REG bytes (240 workgroups x 4 waves x 10 one-KiB wave requests, all requested up
// front, summed, one store per workgroup) from region (i * STRIDE) mod SPAN of one big allocation:
//   SPAN = REG           the same bytes every launch (caches and translations warm)
//   SPAN = 512 MB        beyond L2 (32 MB) and the Infinity Cache (256 MB): data cold, 256 two-MB pages
//   SPAN = 2 / 8 / 24 GB data cold, 1 000 - 12 000 two-MB pages
// and the same with a RIDER: one wave of every launch also touches one cache line in each 2 MB page of the NEXT launch's region (translations warmed one launch ahead,
// 5 loads).  Output: us per launch.
//   tools/bin/tlb_lab ffn2 [launches]
// The one-utterance FFN2's bytes (13.1 MB per launch, cold: regions rotate through 2 GB) as 80 workgroups x 160 one-KiB wave requests (40 per wave: today's sixteen-column
// tiles) and as 160 workgroups x 80 (20 per wave: eight-column tiles), every request issued up front, alternating in one process; also the cross-attention out-projection's
// 3.3 MB as 80 x 40 and 160 x 20.  Output: us per launch of each form, pair by pair.
//   tools/bin/tlb_lab ffn5 [launches]
// The bare request pattern of the one-utterance FFN2 and FFN1 launches, activation rows included, before and after the five-column slabs: per workgroup of four
// waves, first the rows' requests (L2-hot: the same 50 / 25 KiB for every workgroup and launch - 13 per wave for FFN2's 5 x 5120 f16, 10 + 5 + 5 + 5 for FFN1's
// 5 x 1280 fp32), then the wave's weight requests (cold, non-temporal, regions rotating through 2 GB): FFN2 160 workgroups x (4 x 20 + 51) against 256 x (4 x 14 + 51),
// FFN1 160 x (4 x 20 + 25) against 256 x (4 x 14 + 25).  Dependent chains, alternating in one process, eight pairs.  Output: us per launch of each form.
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); exit(1); } } while (0)
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
constexpr size_t REG = 240ull * 4 * 10 * 1024;      // 9.83 MB per launch (the QKV matrix's bytes)

__global__ __launch_bounds__(256) void stream_read(const u32x4* __restrict__ base, const char* __restrict__ next, int rider, unsigned* out) {
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const u32x4* p = base + ((size_t)(blockIdx.x * 4 + wave) * 10) * 64 + lane;
  u32x4 v[10];
#pragma unroll
  for (int u = 0; u < 10; ++u) v[u] = __builtin_nontemporal_load(p + (size_t)u * 64);
  unsigned r = 0;
  if (rider && blockIdx.x == 0 && wave == 0 && lane < 6) r = *reinterpret_cast<const unsigned*>(next + (size_t)lane * (2u << 20));      // one line per 2 MB page of the next region
  unsigned s = r;
#pragma unroll
  for (int u = 0; u < 10; ++u) s += v[u][0] ^ v[u][1] ^ v[u][2] ^ v[u][3];
  if (s == 0x12345678u) out[blockIdx.x] = s;      // (never true on zero-filled memory: keeps the loads alive without a store on the path)
  if (tid == 0 && blockIdx.x == 0) out[0] = 1;
}

// `R` one-KiB requests per wave, all up front; the grid decides how many workgroups share the region's bytes
template <int R>
__global__ __launch_bounds__(256) void stream_read_r(const u32x4* __restrict__ base, unsigned* out) {
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const u32x4* p = base + ((size_t)(blockIdx.x * 4 + wave) * R) * 64 + lane;
  u32x4 v[R];
#pragma unroll
  for (int u = 0; u < R; ++u) v[u] = __builtin_nontemporal_load(p + (size_t)u * 64);
  unsigned s = 0;
#pragma unroll
  for (int u = 0; u < R; ++u) s += v[u][0] ^ v[u][1] ^ v[u][2] ^ v[u][3];
  if (s == 0x12345678u) out[blockIdx.x] = s;
  if (tid == 0 && blockIdx.x == 0) out[0] = 1;
}
template <int R>
static float chain_r(hipStream_t st, hipEvent_t e0, hipEvent_t e1, const char* buf, size_t stride, size_t nreg, int wgs, int n, unsigned* out) {
  CK(hipEventRecord(e0, st));
  for (int i = 0; i < n; ++i) hipLaunchKernelGGL(stream_read_r<R>, dim3(wgs), dim3(256), 0, st, reinterpret_cast<const u32x4*>(buf + (size_t)(i % nreg) * stride), out);
  CK(hipEventRecord(e1, st)); CK(hipEventSynchronize(e1));
  float ms; CK(hipEventElapsedTime(&ms, e0, e1));
  return 1e3f * ms / n;
}
static int ffn2_mode(int n) {
  const size_t STRIDE = 14ull << 20, SPAN = 2ull << 30, nreg = SPAN / STRIDE;      // 13.1 MB regions, 2 MB aligned; 80 x 4 x 40 KiB = 160 x 4 x 20 KiB fit
  char* buf; CK(hipMalloc(&buf, SPAN)); CK(hipMemset(buf, 0, SPAN));
  unsigned* out; CK(hipMalloc(&out, 4096));
  hipStream_t st; CK(hipStreamCreate(&st));
  hipEvent_t e0, e1; CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
  printf("chains of %d dependent launches over 2 GB of cold regions, every request up front, non-temporal; us per launch\n", n);
  printf("pair   FFN2 13.1 MB: 80 wg x 4 x 40   160 wg x 4 x 20   |   cross-out 3.3 MB: 80 wg x 4 x 10   160 wg x 4 x 5\n");
  for (int pair = -1; pair < 8; ++pair) {      // (pair -1 warms the code objects and clocks; not printed)
    const float a = chain_r<40>(st, e0, e1, buf, STRIDE, nreg, 80, n, out), b = chain_r<20>(st, e0, e1, buf, STRIDE, nreg, 160, n, out);
    const float c = chain_r<10>(st, e0, e1, buf, STRIDE, nreg, 80, n, out), d = chain_r<5>(st, e0, e1, buf, STRIDE, nreg, 160, n, out);
    if (pair >= 0) printf("%4d   %30.3f   %15.3f   |   %33.3f   %14.3f\n", pair, a, b, c, d);
  }
  return 0;
}

// RW weight requests per wave behind RX0 (wave 0) / RX1 (waves 1-3) row requests, all up front
template <int RW, int RX0, int RX1>
__global__ __launch_bounds__(256) void stream_read_rx(const u32x4* __restrict__ base, const u32x4* __restrict__ rows, unsigned* out) {
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const u32x4* q = rows + (size_t)(wave * RX0) * 64 + lane;
  const u32x4* p = base + ((size_t)(blockIdx.x * 4 + wave) * RW) * 64 + lane;
  const int rx = wave == 0 ? RX0 : RX1;
  u32x4 x[RX0], v[RW];
#pragma unroll
  for (int i = 0; i < RX0; ++i) { x[i] = u32x4{0u, 0u, 0u, 0u}; if (i < rx) x[i] = q[(size_t)i * 64]; }
#pragma unroll
  for (int u = 0; u < RW; ++u) v[u] = __builtin_nontemporal_load(p + (size_t)u * 64);
  unsigned s = 0;
#pragma unroll
  for (int i = 0; i < RX0; ++i) s += x[i][0] ^ x[i][1] ^ x[i][2] ^ x[i][3];
#pragma unroll
  for (int u = 0; u < RW; ++u) s += v[u][0] ^ v[u][1] ^ v[u][2] ^ v[u][3];
  if (s == 0x12345678u) out[blockIdx.x] = s;
  if (tid == 0 && blockIdx.x == 0) out[0] = 1;
}
template <int RW, int RX0, int RX1>
static float chain_rx(hipStream_t st, hipEvent_t e0, hipEvent_t e1, const char* buf, const char* rows, size_t stride, size_t nreg, int wgs, int n, unsigned* out) {
  CK(hipEventRecord(e0, st));
  for (int i = 0; i < n; ++i)
    hipLaunchKernelGGL((stream_read_rx<RW, RX0, RX1>), dim3(wgs), dim3(256), 0, st, reinterpret_cast<const u32x4*>(buf + (size_t)(i % nreg) * stride), reinterpret_cast<const u32x4*>(rows), out);
  CK(hipEventRecord(e1, st)); CK(hipEventSynchronize(e1));
  float ms; CK(hipEventElapsedTime(&ms, e0, e1));
  return 1e3f * ms / n;
}
static int ffn5_mode(int n) {
  const size_t STRIDE = 16ull << 20, SPAN = 2ull << 30, nreg = SPAN / STRIDE;      // 256 x 4 x 14 KiB = 14.7 MB and 160 x 4 x 20 KiB = 13.1 MB fit a 16 MB region
  char* buf; CK(hipMalloc(&buf, SPAN)); CK(hipMemset(buf, 0, SPAN));
  char* rows; CK(hipMalloc(&rows, 64 << 10)); CK(hipMemset(rows, 0, 64 << 10));      // 4 waves x 13 KiB
  unsigned* out; CK(hipMalloc(&out, 4096));
  hipStream_t st; CK(hipStreamCreate(&st));
  hipEvent_t e0, e1; CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
  printf("chains of %d dependent launches over 2 GB of cold regions, rows' requests (L2-hot) then weight requests (non-temporal), all up front; us per launch\n", n);
  printf("pair   FFN2: 160 wg x (4 x 20 + 52)   256 wg x (4 x 14 + 52)   |   FFN1: 160 wg x (4 x 20 + 25)   256 wg x (4 x 14 + 25)\n");
  for (int pair = -1; pair < 8; ++pair) {      // (pair -1 warms the code objects and clocks; not printed)
    const float a = chain_rx<20, 13, 13>(st, e0, e1, buf, rows, STRIDE, nreg, 160, n, out), b = chain_rx<14, 13, 13>(st, e0, e1, buf, rows, STRIDE, nreg, 256, n, out);
    const float c = chain_rx<20, 10, 5>(st, e0, e1, buf, rows, STRIDE, nreg, 160, n, out), d = chain_rx<14, 10, 5>(st, e0, e1, buf, rows, STRIDE, nreg, 256, n, out);
    if (pair >= 0) printf("%4d   %30.3f   %22.3f   |   %30.3f   %22.3f\n", pair, a, b, c, d);
  }
  return 0;
}

int main(int argc, char** argv) {
  if (argc > 1 && !strcmp(argv[1], "ffn2")) return ffn2_mode(argc > 2 ? atoi(argv[2]) : 3000);
  if (argc > 1 && !strcmp(argv[1], "ffn5")) return ffn5_mode(argc > 2 ? atoi(argv[2]) : 3000);
  const int n = argc > 1 ? atoi(argv[1]) : 3000;
  size_t freeb = 0, total = 0; CK(hipMemGetInfo(&freeb, &total));
  const size_t cap = 26ull << 30;
  char* buf; CK(hipMalloc(&buf, cap)); CK(hipMemset(buf, 0, cap));
  unsigned* out; CK(hipMalloc(&out, 4096));
  hipStream_t st; CK(hipStreamCreate(&st));
  hipEvent_t e0, e1; CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
  const size_t STRIDE = 12ull << 20;      // regions 12 MB apart (2 MB aligned)
  const size_t spans[] = {STRIDE, 512ull << 20, 2ull << 30, 8ull << 30, 24ull << 30};
  printf("chain of %d dependent launches, each reading %.2f MB (240 workgroups x 40 one-KiB wave requests, non-temporal), region stride 12 MB\n", n, REG / 1e6);
  for (int round = 0; round < 3; ++round)
   for (size_t span : spans)
    for (int rider = 0; rider < 2; ++rider) {
      const size_t nreg = span / STRIDE;
      for (int rep = 0; rep < 2; ++rep) {      // (first repetition warms what can be warmed)
        CK(hipEventRecord(e0, st));
        for (int i = 0; i < n; ++i) {
          const size_t off = (size_t)(i % nreg) * STRIDE, nxt = (size_t)((i + 1) % nreg) * STRIDE;
          hipLaunchKernelGGL(stream_read, dim3(240), dim3(256), 0, st, reinterpret_cast<const u32x4*>(buf + off), buf + nxt, rider, out);
        }
        CK(hipEventRecord(e1, st)); CK(hipEventSynchronize(e1));
        float ms; CK(hipEventElapsedTime(&ms, e0, e1));
        if (rep) printf("  span %8.0f MB (%5zu regions) %s: %.3f us per launch\n", span / 1048576.0, nreg, rider ? "with the next region's pages touched one launch ahead" : "plain", 1e3 * ms / n);
      }
    }
  return 0;
}
