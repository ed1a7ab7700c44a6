// dec_kernels.hip — Whisper decoder step, logits processors and beam search on gfx950
// (the reference runs these inside ctranslate2 Whisper.generate,
// call site reference main.py:687-693, semantics SURVEY §3.4 + Appendix C).
//
// A decode step has M = B*beam <= 96 rows: every projection is a weight-streaming, HBM-bound
// skinny GEMM.  MI355X mapping:
//  * weights are re-packed once at load into MFMA A-fragment order ([N/16][K/32][64 lanes][8 f16])
//    so every wave-level load is ONE fully coalesced 1 KiB global_load_dwordx4 that feeds
//    v_mfma_f32_16x16x32_f16 directly (rows of the M<=16 activation block are the B operand, read
//    from LDS); 4 waves split K, partial accumulators meet in LDS, the epilogue (bias, GELU,
//    fp32 residual, KV-cache scatter) is fused.  The pre-LN LayerNorm is FOLDED into the
//    projection's weights (fold_ln_kernel): the kernel multiplies the raw rows and applies mean / rstd in its epilogue.
//  * self-attention KV cache: after every beam step the rows of each live beam are rewritten in place from its parent's
//    (kv_reorder_kernel), so the attention kernel's K/V addresses depend on nothing it has to load.
//  * cross-attention K is stored [H][dh/8][T][8] and V transposed [H][64][Tpad] so that both are MFMA A fragments read with
//    16-byte loads; the `beam` query rows of an utterance are folded into one pass over the utterance's K/V (shared per
//    utterance, never tiled per beam); the T axis is split into 256-key chunks across workgroups with an in-launch,
//    placement-independent last-arriver combine.
//  * suppress masks, log-softmax statistics and the top-2*beam candidates are computed in one
//    pass over the logits (16 chunks per row), the beam bookkeeping runs on device (one wave per
//    utterance) so the host never sees logits and a whole step replays as one HIP graph.
#include <string.h>
#include "common.hpp"
#include "kernels.hpp"

namespace wis {

// =======================================================================================
// packed image: [Npad/rows][K/32][4 k-quarters][rows][8 f16]; rows = 16 is the full MFMA A fragment ([64 lanes][8]),
// rows = 8 / 4 keep only the first rows of each fragment so that small-N matrices still spread over every CU.
__global__ void pack_gemv_kernel(const f16* __restrict__ W, f16* __restrict__ Wp, int N, int Npad, int K, int n_scale, float scale, int rows) {
  const int ksteps = K / 32;
  const size_t total = (size_t)Npad * ksteps * 4;
  for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (size_t)gridDim.x * blockDim.x) {
    const int row = (int)(idx % rows);
    size_t t = idx / rows;
    const int kq = (int)(t & 3); t >>= 2;
    const int ks = (int)(t % ksteps), nt = (int)(t / ksteps);
    const int n = rows * nt + row, k = 32 * ks + 8 * kq;
    f16x8 v;
    if (n < N) {
      v = *reinterpret_cast<const f16x8*>(W + (size_t)n * K + k);
      if (n < n_scale) {
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = (f16)((float)v[j] * scale);
      }
    } else {
#pragma unroll
      for (int j = 0; j < 8; ++j) v[j] = (f16)0.f;
    }
    *reinterpret_cast<f16x8*>(Wp + idx * 8) = v;
  }
}
// ---- 8-bit weights (compute type int8_float16; SURVEY §8(f)4, reference main.py:242): the same fragment order with one BYTE
// per weight, [Npad/16][K/32][64 lanes][8 B], stored offset-binary (q + 128) with one fp32 dequantisation scale per output row
// (CTranslate2's per-row scheme: scale = absmax / 127, q = rint(w / scale)).  The kernel widens a lane's 8 bytes to 8 exact
// f16 values with two byte permutes and two packed subtractions per dword ((0x6400 | u) is the f16 number 1024 + u), feeds
// the SAME f16 MFMA (activations stay f16, accumulation fp32) and multiplies the row scale into the epilogue.
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
template <bool W8> struct WFrag;
template <> struct WFrag<false> {
  typedef u32x4 T;
  static __device__ __forceinline__ T zero() { return T{0u, 0u, 0u, 0u}; }
  static __device__ __forceinline__ f16x8 cvt(const T& w) { return *reinterpret_cast<const f16x8*>(&w); }
};
template <> struct WFrag<true> {
  typedef u32x2 T;
  static __device__ __forceinline__ T zero() { return T{0x80808080u, 0x80808080u}; }     // q = 0
  static __device__ __forceinline__ f16x8 cvt(const T& w) {
    typedef _Float16 h2 __attribute__((ext_vector_type(2)));
    const unsigned K64 = 0x64646464u;
    unsigned a[4] = {__builtin_amdgcn_perm(K64, w.x, 0x04010400u), __builtin_amdgcn_perm(K64, w.x, 0x04030402u),
                     __builtin_amdgcn_perm(K64, w.y, 0x04010400u), __builtin_amdgcn_perm(K64, w.y, 0x04030402u)};
    const h2 off = {(f16)1152.0f, (f16)1152.0f};
    f16x8 r;
#pragma unroll
    for (int i = 0; i < 4; ++i) { const h2 v = *reinterpret_cast<const h2*>(&a[i]) - off; r[2 * i] = v[0]; r[2 * i + 1] = v[1]; }
    return r;
  }
};
// per-row dequantisation scale (absmax / 127, times the folded query scaling) of W [N][K]; rows >= N get 0
__global__ void row_scale_kernel(const f16* __restrict__ W, float* __restrict__ scale, int N, int Npad, int K, int n_scale, float qscale) {
  const int n = blockIdx.x, lane = threadIdx.x;
  if (n >= Npad) return;
  float mx = 0.f;
  if (n < N) for (int k = lane; k < K; k += 64) mx = fmaxf(mx, fabsf((float)W[(size_t)n * K + k]));
  mx = wave_max(mx);
  if (lane == 0) scale[n] = (n < N) ? (mx > 0.f ? mx / 127.0f : 1.0f) * (n < n_scale ? qscale : 1.0f) : 0.f;
}
__global__ void pack_gemv8_kernel(const f16* __restrict__ W, const float* __restrict__ scale, unsigned char* __restrict__ Wp, int N, int Npad, int K,
                                  int n_scale, float qscale) {
  const int ksteps = K / 32;
  const size_t total = (size_t)Npad * ksteps * 4;
  for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (size_t)gridDim.x * blockDim.x) {
    const int row = (int)(idx & 15);
    size_t t = idx >> 4;
    const int kq = (int)(t & 3); t >>= 2;
    const int ks = (int)(t % ksteps), nt = (int)(t / ksteps);
    const int n = 16 * nt + row, k = 32 * ks + 8 * kq;
    unsigned char out[8];
    if (n < N) {
      const float inv = 1.0f / (scale[n] / (n < n_scale ? qscale : 1.0f));     // quantise the UNSCALED row; the folded factor lives in scale[]
      const f16x8 v = *reinterpret_cast<const f16x8*>(W + (size_t)n * K + k);
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        float q = rintf((float)v[j] * inv);
        q = fminf(fmaxf(q, -127.f), 127.f);
        out[j] = (unsigned char)((int)q + 128);
      }
    } else {
#pragma unroll
      for (int j = 0; j < 8; ++j) out[j] = 128;
    }
    *reinterpret_cast<u32x2*>(Wp + idx * 8) = *reinterpret_cast<const u32x2*>(out);
  }
}
int launch_pack_gemv8(hipStream_t st, const f16* W, unsigned char* Wp, float* scale, int N, int Npad, int K, int n_scale, float qscale) {
  if (K % 32 || Npad % 16 || Npad < N) { set_error("pack_gemv8: bad shape N=%d Npad=%d K=%d", N, Npad, K); return WIS_E_ARG; }
  hipLaunchKernelGGL(row_scale_kernel, dim3(Npad), dim3(64), 0, st, W, scale, N, Npad, K, n_scale, qscale);
  const size_t total = (size_t)Npad * (K / 32) * 4;
  int blocks = (int)((total + 255) / 256); if (blocks > 4096) blocks = 4096;
  hipLaunchKernelGGL(pack_gemv8_kernel, dim3(blocks), dim3(256), 0, st, W, scale, Wp, N, Npad, K, n_scale, qscale);
  return WIS_OK;
}

// ---- LayerNorm folded into the following projection (pre-LN blocks: y = W . LN(x) + b).  With W' = W o gamma (columns scaled),
//   y_n = rs * ( sum_k W'_nk x_k  -  mu * c_n ) + b'_n,     c_n = sum_k W'_nk,     b'_n = b_n + sum_k W_nk beta_k,
// so the skinny GEMM runs on the RAW activation row (cast to f16) and the row statistics (mu, rs) are only needed in its
// epilogue - the normalise-and-restage pass, its barrier and the gamma / beta loads leave the kernel's critical path.
// One wave per matrix row: rewrites W in place as f16(W * gamma), accumulates c from the ROUNDED products (what the MFMA
// will see) and adds W . beta to the bias.  Rows < n_scale carry the folded query scaling (applied to W by the packer).
__global__ void fold_ln_kernel(f16* __restrict__ W, const float* __restrict__ gamma, const float* __restrict__ beta, float* __restrict__ bias,
                               float* __restrict__ csum, int N, int K, int n_scale, float qscale) {
  const int n = blockIdx.x, lane = threadIdx.x;
  if (n >= N) return;
  float c = 0.f, wb = 0.f;
  for (int k = lane; k < K; k += 64) {
    const float w = (float)W[(size_t)n * K + k];
    const f16 wg = (f16)(w * gamma[k]);
    W[(size_t)n * K + k] = wg;
    c += (float)wg; wb += w * beta[k];
  }
  c = wave_sum(c); wb = wave_sum(wb);
  const float f = n < n_scale ? qscale : 1.0f;
  if (lane == 0) { csum[n] = c * f; bias[n] += wb * f; }
}
// 8-bit variant of c: from the de-quantised values the MFMA will see (scale_n * sum_k q_nk; scale[] already carries qscale)
__global__ void csum8_kernel(const f16* __restrict__ W, const float* __restrict__ scale, float* __restrict__ csum, int N, int K, int n_scale, float qscale) {
  const int n = blockIdx.x, lane = threadIdx.x;
  if (n >= N) return;
  const float inv = 1.0f / (scale[n] / (n < n_scale ? qscale : 1.0f));
  float c = 0.f;
  for (int k = lane; k < K; k += 64) { float q = rintf((float)W[(size_t)n * K + k] * inv); c += fminf(fmaxf(q, -127.f), 127.f); }
  c = wave_sum(c);
  if (lane == 0) csum[n] = c * scale[n];
}
int launch_fold_ln(hipStream_t st, f16* W, const float* gamma, const float* beta, float* bias, float* csum, int N, int K, int n_scale, float qscale) {
  hipLaunchKernelGGL(fold_ln_kernel, dim3(N), dim3(64), 0, st, W, gamma, beta, bias, csum, N, K, n_scale, qscale);
  return WIS_OK;
}
int launch_csum8(hipStream_t st, const f16* W, const float* scale, float* csum, int N, int K, int n_scale, float qscale) {
  hipLaunchKernelGGL(csum8_kernel, dim3(N), dim3(64), 0, st, W, scale, csum, N, K, n_scale, qscale);
  return WIS_OK;
}

// tile height of an [N][K] decoder matrix: the full 16-row MFMA fragment unless the matrix is both narrow (fewer than
// ~200 tiles) and deep (K >= 2048: FFN2), where 4-row tiles spread the long per-tile stream over every CU.  For the
// narrow d x d matrices the kernel is latency-bound and extra workgroups only add prologue work.
int gemv_rows_for(int N, int K) {
  (void)N; (void)K;
  return 16;   // measured on MI355X (round 1): the K = 5120 stream is already HBM-bound with 80 workgroups (13 MB in ~6k
               // cycles = 4.5 TB/s); 4-row tiles and a 40-deep prefetch cost ~1.5k cycles of issue per launch and gained nothing
}
int launch_pack_gemv(hipStream_t st, const f16* W, f16* Wp, int N, int Npad, int K, int n_scale, float scale, int rows) {
  if (K % 32 || Npad % rows || Npad < N || (rows != 16 && rows != 8 && rows != 4)) { set_error("pack_gemv: bad shape N=%d Npad=%d K=%d rows=%d", N, Npad, K, rows); return WIS_E_ARG; }
  const size_t total = (size_t)Npad * (K / 32) * 4;
  int blocks = (int)((total + 255) / 256); if (blocks > 4096) blocks = 4096;
  hipLaunchKernelGGL(pack_gemv_kernel, dim3(blocks), dim3(256), 0, st, W, Wp, N, Npad, K, n_scale, scale, rows);
  return WIS_OK;
}

// The eight-column image (gemv_body NC = 8): [Npad/8][K/64][64 lanes][8 f16].  Lane l of a wave request carries column 8 nt + (l & 7), k-step
// 2 kp + ((l >> 3) & 1) of the pair, k-quarter l >> 4 - i.e. A-fragment rows 0-7 hold the even k-step, rows 8-15 the odd one.  Same bytes as the sixteen-column image.
__global__ void pack_gemv_nc8_kernel(const f16* __restrict__ W, f16* __restrict__ Wp, int N, int Npad, int K) {
  const int kpairs = K / 64;
  const size_t total = (size_t)(Npad / 8) * kpairs * 64;
  for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (size_t)gridDim.x * blockDim.x) {
    const int l = (int)(idx & 63);
    const size_t t = idx >> 6;
    const int kp = (int)(t % kpairs), nt = (int)(t / kpairs);
    const int n = 8 * nt + (l & 7), k = 64 * kp + 32 * ((l >> 3) & 1) + 8 * (l >> 4);
    f16x8 v;
    if (n < N) v = *reinterpret_cast<const f16x8*>(W + (size_t)n * K + k);
    else {
#pragma unroll
      for (int j = 0; j < 8; ++j) v[j] = (f16)0.f;
    }
    *reinterpret_cast<f16x8*>(Wp + idx * 8) = v;
  }
}
int launch_pack_gemv_nc8(hipStream_t st, const f16* W, f16* Wp, int N, int Npad, int K) {
  if (K % 64 || Npad % 8 || Npad < N) { set_error("pack_gemv_nc8: bad shape N=%d Npad=%d K=%d", N, Npad, K); return WIS_E_ARG; }
  const size_t total = (size_t)(Npad / 8) * (K / 64) * 64;
  int blocks = (int)((total + 255) / 256); if (blocks > 4096) blocks = 4096;
  hipLaunchKernelGGL(pack_gemv_nc8_kernel, dim3(blocks), dim3(256), 0, st, W, Wp, N, Npad, K);
  return WIS_OK;
}
// the shapes launch_gemv runs on eight-column tiles (GemvP::rows = 8, Wp that image): the single-chunk f16-activation form at
// K = 1280 and 5120 (SC 10 and 40), as many rows as its register staging holds
bool gemv_nc8_shape(int M, int N, int K) { return (K == 1280 || K == 5120) && N % 8 == 0 && M >= 1 && M <= 16 && M * (K / 8) <= 13 * 256; }

// The five-column image (gemv_nc5_kernel): [N/5 slabs][K/32/kw wave K-ranges][ceil(kw/3) requests][64 lanes][8 f16].  A wave request is one
// full KiB, five columns x THREE k-steps: lane l carries A-fragment row l & 15 and k-quarter l >> 4; rows 0-4 hold the slab's columns for k-step 3u of the
// K-range, rows 5-9 for 3u + 1, rows 10-14 for 3u + 2, row 15 is zero.  The last request of a K-range carries the one or two k-steps left over (kw = 40: one,
// kw = 20: two), the unused rows zero.  16/15 of the sixteen-column image's bytes, plus the ragged last requests: 12 % more at kw = 40.
__global__ void pack_gemv_nc5_kernel(const f16* __restrict__ W, f16* __restrict__ Wp, int N, int K, int kw) {
  const int rq = (kw + 2) / 3, nr = K / 32 / kw;
  const size_t total = (size_t)(N / 5) * nr * rq * 64;
  for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (size_t)gridDim.x * blockDim.x) {
    const int l = (int)(idx & 63);
    size_t t = idx >> 6;
    const int u = (int)(t % rq); t /= rq;
    const int rg = (int)(t % nr), slab = (int)(t / nr);
    const int row = l & 15, j = row / 5, ksl = 3 * u + j;
    const int n = 5 * slab + (row - 5 * j), k = 32 * (rg * kw + ksl) + 8 * (l >> 4);
    f16x8 v;
    if (row < 15 && ksl < kw) v = *reinterpret_cast<const f16x8*>(W + (size_t)n * K + k);
    else {
#pragma unroll
      for (int e = 0; e < 8; ++e) v[e] = (f16)0.f;
    }
    *reinterpret_cast<f16x8*>(Wp + idx * 8) = v;
  }
}
size_t gemv_nc5_elems(int N, int K, int kw) { return (size_t)(N / 5) * (K / 32 / kw) * ((kw + 2) / 3) * 512; }
int launch_pack_gemv_nc5(hipStream_t st, const f16* W, f16* Wp, int N, int K, int kw) {
  if (N < 5 || N % 5 || K % 32 || kw < 1 || (K / 32) % kw) { set_error("pack_gemv_nc5: bad shape N=%d K=%d kw=%d", N, K, kw); return WIS_E_ARG; }
  const size_t total = gemv_nc5_elems(N, K, kw) / 8;
  int blocks = (int)((total + 255) / 256); if (blocks > 4096) blocks = 4096;
  hipLaunchKernelGGL(pack_gemv_nc5_kernel, dim3(blocks), dim3(256), 0, st, W, Wp, N, K, kw);
  return WIS_OK;
}
// the launches launch_gemv runs on five-column slabs (GemvP::rows = 5, Wp that image with kw = 40): K = 5120, f16 rows (FFN2; four waves split K), plain /
// residual epilogues, as many rows as the register staging holds, N / 5 workgroups in ONE dispatch round on this device - a part with fewer CUs than workgroups
// keeps the other forms (a second round costs more than the requests saved)
static int device_cu_count() {
  static int cus[64];
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return 0;
  if (!cus[dev]) { int v = 0; if (hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) v = 0; cus[dev] = v > 0 ? v : -1; }
  return cus[dev] > 0 ? cus[dev] : 0;
}
bool gemv_nc5_shape(int M, int N, int K, int flags) {
  return K == 5120 && M >= 1 && M * (K / 8) <= 13 * 256 && N >= 5 && N % 5 == 0 && !(flags & ~(GV_RESID | GV_OUT_F32 | GV_GELU)) && N / 5 <= device_cu_count();
}

// 8-byte {tag, value} granules: one relaxed agent-scope (write-through) store each, "the data is the flag" (guide G16 form R2) - the hand-off of the
// decoder cross-attention's chunk partials (dec_cross_attn_kernel SPIN).  Lesson of the three in-launch hand-offs that were tried for the step's other
// stages and lost (retired experiments): an in-launch hand-off is two fabric round trips (granule store -> L2 -> poll), like a kernel boundary.
typedef unsigned long long gran_t;
__device__ __forceinline__ void st_gran(gran_t* p, unsigned tag, float v) {
  __hip_atomic_store(p, ((gran_t)tag << 32) | (gran_t)__float_as_uint(v), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ gran_t ld_gran(const gran_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
constexpr unsigned CA_SPIN_LIMIT = 1u << 17;      // sweeps before the combiner gives up (~0.1 s)

// =======================================================================================
// Skinny GEMM.  grid = Npad/16 workgroups of 4 waves; wave w streams the k-steps of its quarter of
// every staged K-chunk.  Dynamic LDS: xs f16 [M][KC+8] | red f32 [4][64][4] | stats f32 [MAX_ROWS][2] (unused) | sred f32 [4][8]
//
// Memory-latency structure (one dependent round trip): the activation loads (L2-hot, written by the
// previous kernel) are issued FIRST, then a 16-deep prefetch of this wave's weight fragments (HBM);
// vmcnt retires in order, so LayerNorm statistics and the f16 staging of x run from registers while
// the weight stream is in flight, and the MFMAs consume the fragments as they land, refilling the ring.
// SC (template): compile-time k-steps per wave (K / 128) for the common single-chunk shapes {3,4,6,8,10} so the prefetch and
// the MFMA loop are straight-line code (every runtime `u < S` guard would be a scalar branch around one load); SC = 0 is the
// generic ring of 16 fragments with refill.
// Two A/B builds of this body found no gain and are gone: requesting the epilogue operands right behind the weight prefetch instead of after the last
// MFMA (33.12 vs 32.82 ms per utterance: the round trip is already hidden behind the cross-wave reduction, and 15-18 more live VGPRs cost what it saves),
// and fetching the rows' LayerNorm shifts with one vector load per row instead of through the scalar cache (the round-2..4 form: five of a wave's 25 requests).
// MB (16-row blocks) is 1 at every call site - more than 16 rows take launch_gemv_frag.  The `MB > 1` arms below (30-piece register staging, multi-chunk
// `more`, per-block accumulators) are dead at compile time; they and the parameter stay because without them hipcc allocates the registers of the MODE 1
// kernels differently, and this body is kept instruction for instruction.
// MODE 0: generic staging from global; 1: fast LayerNorm prologue from registers; 2: fast f16 activations from registers
// NT (r5; MB = 1, single chunk, compile-time SC only): n-tiles per workgroup.  2: waves 0-1 own tile 2 nt, waves 2-3 tile 2 nt + 1, half of
// K each (SC = K / 64 fragments per wave, all requested up front) - half as many workgroups stage the activation rows, each with twice
// the weight bytes in flight: N = 4d of the one-utterance step is 160 workgroups (one per CU) instead of 320 on 256 CUs.
// NC (MODE 2, MB = 1, NT = 1, even compile-time SC, f16 weights): output columns per workgroup.  8: the eight-column image (pack_gemv_nc8_kernel) - a wave
// request is still one full KiB, eight columns x TWO k-steps (lanes with bit 3 clear carry the even k-step of the pair in A-fragment rows 0-7, lanes with
// bit 3 set the odd one in rows 8-15), so a workgroup issues HALF the requests of a sixteen-column tile and N / 8 workgroups share the matrix: the
// one-utterance FFN2 and cross-attention out-projection run on 160 workgroups instead of 80.  Per request two MFMAs: the registers as they landed against
// the even k-step's activations, then the same registers rotated by eight lanes within each row of 16 (DPP row_ror:8: the odd k-step's weights arrive in
// rows 0-7) against the odd k-step's.  Rows 0-7 of the accumulator thus see the wave's k-steps in today's order, each through the same MFMA, and the
// cross-wave reduction is unchanged: bit-identical outputs.  Rows 8-15 of the accumulator are by-products nobody reads.  Today the cross-attention
// out-projection (K = d) runs this form; FFN2 (K = 4d) moved on to FIVE-column slabs, three k-steps per request, N / 5 = 256 workgroups at large's width -
// a kernel of its own below (gemv_nc5_kernel), so that this body keeps its instructions.  FFN1 on such slabs (four per workgroup in NT = 2's place) measured
// slower and stays on NT = 2.
template <int MB, int MODE, int SC, int RM, bool W8, int NT = 1, int NC = 16>
__device__ __forceinline__ void gemv_body(const GemvP& p, const int KC, const int nt, char* smem) {
  static_assert(NT == 1 || (NT == 2 && MB == 1 && SC > 0), "two-tile workgroups: <= 16 rows, every fragment prefetched");
  static_assert(NC == 16 || (NC == 8 && MB == 1 && NT == 1 && MODE == 2 && SC > 0 && SC % 2 == 0 && !W8), "eight-column tiles: f16 activations and weights, k-steps in pairs, all prefetched");
  typedef typename WFrag<W8>::T WT;
  constexpr int GV_PF = SC > 0 ? (NC == 8 ? SC / 2 : SC) : 16;
  // full MFMA A fragments.  4- / 8-row tiles were measured twice: packed that way (round 1) and as HALF tiles of the ordinary image (round 6: 160 workgroups
  // addressing rows 8 h .. 8 h + 7 of every fragment for the one-utterance FFN2, 1.2152 / 1.2137 vs 1.2152 / 1.2159 ms per step, session r6L) - no gain: a
  // wave's request costs the CU's address path the same ~50 cycles whether 64 or 32 of its lanes are active, and the stream is those requests
  // (NC = 8 is not that form: its requests stay FULL - eight columns x two k-steps -, so a workgroup issues half as many)
  constexpr int rows = NC;
  const int M = p.M, K = p.K;
  const int xstr = KC + 8;
  f16* xs = reinterpret_cast<f16*>(smem);
  float* red = reinterpret_cast<float*>(smem + (((size_t)M * xstr * 2 + 15) & ~(size_t)15));
  float* stats = red + 4 * MB * 64 * 4;
  float* sred = stats + 2 * MAX_ROWS;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int ksteps = K / 32;
  const int S = SC > 0 ? SC : KC / 128;          // k-steps per wave per chunk
  const int wt = NT == 2 ? wave >> 1 : 0;        // the wave's n-tile within the workgroup
  const int ksl0 = (NT == 2 ? (wave & 1) : wave) * S;      // first chunk-local k-step of this wave
  // fragment (tile, k-step) = 4*rows 16-byte pieces: piece (kq, row) at kq*rows + row; lanes with row >= rows stay zero
  const bool wact = (lane & 15) < rows;
  const int wstep = 4 * rows;                     // pieces per k-step
  // (NC == 8: request `u` of the wave = k-steps ksl0 + 2u, + 1 of tile nt, 64 pieces)
  const WT* wp4 = NC == 8 ? reinterpret_cast<const WT*>(p.Wp) + ((size_t)nt * (ksteps >> 1) + (ksl0 >> 1)) * 64 + lane
                          : reinterpret_cast<const WT*>(p.Wp) + (size_t)(nt * NT + wt) * ksteps * wstep + (lane >> 4) * rows + (lane & 15);
  const WT wzero = WFrag<W8>::zero();
  const int k4n = K >> 2;                        // float4 per row
  // LayerNorm-folded path (MODE 1; host-selected, M <= 8, K <= 2048): the raw fp32 rows live in registers, thread owns float4
  // columns k4 = tid, tid + 256 of every row; they are cast to f16 and staged at once, the statistics (single shifted pass,
  // c = x[r][0]: var = E[(x-c)^2] - E[x-c]^2) are reduced AFTER the MFMA loop and meet the accumulators in the epilogue.
  // MODE 3 (r5, GV_LN16): the same on the F16 copy of the rows that whoever produces residual rows leaves next to them (12.8 KB per
  // workgroup instead of 25.6 KB): thread t < K / 8 owns the 16-byte chunk t of every row - five requests per thread in 2.5 waves where
  // the fp32 form issues ten in four -, stages it as it is, and takes the statistics from those same values (the ones the MFMAs consume).
  constexpr bool fast = MODE == 1 || MODE == 3;
  constexpr bool x16 = MODE == 3;
  constexpr int RMAX = fast ? RM : 1;        // RM in {3, 5, 8}: smallest that holds M (rows >= M are clamped duplicates)
  f32x4 xv[RMAX][2];      // (vector type, not HIP's float4 struct: hipcc split each struct load into an overlapping dwordx2 + dwordx3 pair)
  u32x4 xv16[RMAX];
  unsigned c16raw[RMAX];      // (whichever set the instantiation does not use is never materialised)
  float cshift[RMAX];
  unsigned long long* pf = (nt == 0 && tid == 0) ? p.prof : nullptr;
  if (tid == 0) tl_begin(p.prof);
  stamp(pf, 0);
  if (x16) {
    const u32x4* x8 = reinterpret_cast<const u32x4*>(p.x);
    const int k8n16 = K >> 3, t8 = tid < k8n16 ? tid : k8n16 - 1;      // (clamped address: threads >= K / 8 load a valid chunk and drop it)
#pragma unroll
    for (int r = 0; r < RMAX; ++r) { const int rr = r < M ? r : M - 1; xv16[r] = x8[(size_t)rr * k8n16 + t8]; }
#pragma unroll
    for (int r = 0; r < RMAX; ++r) { const int rr = r < M ? r : M - 1; c16raw[r] = uniform_load_issue_u32(reinterpret_cast<const f16*>(p.x) + (size_t)rr * K); }
  }
  if (fast && !x16) {
    const f32x4* x4 = reinterpret_cast<const f32x4*>(p.x);
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int k4 = tid + 256 * j;
      if (k4 < k4n) {
#pragma unroll
        for (int r = 0; r < RMAX; ++r) { const int rr = r < M ? r : M - 1; xv[r][j] = x4[(size_t)rr * k4n + k4]; }   // rows >= M: clamped duplicates
      }
    }
#pragma unroll
    // (the shifts are uniform over the workgroup: fetched through the SCALAR cache - as vector loads they were five of a wave's 25 requests
    // on the CU's address path, the unit the start of these kernels is bound by)
    for (int r = 0; r < RMAX; ++r) { const int rr = r < M ? r : M - 1; cshift[r] = uniform_load_issue_f32(reinterpret_cast<const float*>(p.x) + (size_t)rr * K); }
  }
  // f16 activations (attention / FFN hidden output of the previous kernel): same idea, up to 13 x 16 B per thread
  // (single chunk: the launcher selects this mode only when KC == K)
  constexpr bool fastx = MODE == 2;
  constexpr int NXH = fastx ? (MB == 1 ? 13 : 30) : 1;
  u32x4 xh[NXH];
  const int c8 = KC >> 3, k8n = K >> 3, nx = M * c8;     // 16-byte pieces per chunk row / per full row / per chunk
  // piece index -> row without an integer division (hipcc expands `idx / c8` by a run-time divisor into ~30 instructions, thirteen
  // times per thread, in front of the weight prefetch): (idx + 0.5) * (1 / c8) truncates to the exact quotient for idx < 2^20
  const float inv_c8 = 1.0f / (float)c8;
#define WIS_ROW_OF(idx) ((int)(((float)(idx) + 0.5f) * inv_c8))
  if (fastx) {
    const u32x4* x8 = reinterpret_cast<const u32x4*>(p.x);
    if (p.x2) {                 // columns >= xsplit come from a second row-major matrix (the fused out-proj + cross-Q stage)
      const u32x4* y8 = reinterpret_cast<const u32x4*>(p.x2);
      const int s8 = p.xsplit >> 3, r8 = c8 - s8;
#pragma unroll
      for (int i = 0; i < NXH; ++i) {
        const int idx = tid + 256 * i;
        if (idx < nx) { const int row = WIS_ROW_OF(idx), col = idx - row * c8; xh[i] = col < s8 ? x8[(size_t)row * s8 + col] : y8[(size_t)row * r8 + (col - s8)]; }
      }
    } else if (MB == 1 || KC == K) {   // MB == 1: the launcher only selects this mode for a single chunk
#pragma unroll
      for (int i = 0; i < NXH; ++i) { const int idx = tid + 256 * i; if (idx < nx) xh[i] = x8[idx]; }
    } else {
#pragma unroll
      for (int i = 0; i < NXH; ++i) { const int idx = tid + 256 * i; if (idx < nx) { const int row = WIS_ROW_OF(idx); xh[i] = x8[(size_t)row * k8n + (idx - row * c8)]; } }
    }
  }
  // weight prefetch for chunk 0 (independent of x)
  WT wf[GV_PF];
  if constexpr (NC == 8) {
#pragma unroll
    for (int u = 0; u < GV_PF; ++u) wf[u] = __builtin_nontemporal_load(wp4 + (size_t)u * 64);
  } else {
    const WT* wq = wp4 + (size_t)ksl0 * wstep;
#pragma unroll
    for (int u = 0; u < GV_PF; ++u) { wf[u] = wzero; if ((SC > 0 || u < S) && wact) wf[u] = __builtin_nontemporal_load(wq + (size_t)u * wstep); }
  }

  // epilogue operands (bias, folded column sums, row scales, residual, KV-cache row)
  const bool ep_act = tid < MB * NT * 64;        // (NT == 2: wave 0 finishes tile 2 nt, wave 1 tile 2 nt + 1)
  const int ep_m = NT == 2 ? (lane & 15) : (tid >> 6) * 16 + (lane & 15), ep_n = rows * (nt * NT + (NT == 2 ? (tid >> 6) & 1 : 0)) + 4 * (lane >> 4);
  const bool ep_ok = ep_act && ep_m < M && ep_n < p.N && 4 * (lane >> 4) < rows;
  float4 ep_bias = make_float4(0.f, 0.f, 0.f, 0.f), ep_cs = ep_bias, ep_res = ep_bias, ep_sc = make_float4(1.f, 1.f, 1.f, 1.f);
  // (MODE 1 leaves slot and position unset where the K / V arm that reads them does not run: zeroing their registers on the other paths made hipcc wait
  // there for the requests it believes may be in flight into them - s_waitcnt vmcnt(0) in front of the reductions, for bias and column sums as well)
  int ep_slot, ep_pos;
  if constexpr (MODE != 1) { ep_slot = 0; ep_pos = 0; }
#define WIS_FL (MODE == 1 ? fl : p.flags)      /* (the other modes read the struct where they always did: their instructions stay) */
#define WIS_EP_LOADS()                                                                                              \
  if (ep_ok) {                                                                                                      \
    if (p.bias) ep_bias = *reinterpret_cast<const float4*>(p.bias + ep_n);                                          \
    if (fast) ep_cs = *reinterpret_cast<const float4*>(p.csum + ep_n);                                              \
    if (W8) ep_sc = *reinterpret_cast<const float4*>(p.wscale + ep_n);                                              \
    if (WIS_FL & GV_QKV) { if (ep_n >= p.d) { ep_slot = p.slot[ep_m]; ep_pos = p.pos[ep_m]; } }                    \
    else if (WIS_FL & GV_RESID) ep_res = *reinterpret_cast<const float4*>(reinterpret_cast<const float*>(p.y) + (size_t)ep_m * p.N + ep_n); \
  }
  stamp(pf, 1);
  float sa[RMAX], sb[RMAX];
  if (x16) {
    uniform_load_wait();
#pragma unroll
    for (int r = 0; r < RMAX; ++r) uniform_load_landed(c16raw[r]);
#pragma unroll
    for (int r = 0; r < RMAX; ++r) {
      const int rr = r < M ? r : M - 1;
      cshift[r] = (float)__builtin_bit_cast(f16, (unsigned short)(c16raw[r] & 0xFFFFu));
      sa[r] = 0.f; sb[r] = 0.f;
      if (tid < (K >> 3)) {
        *reinterpret_cast<u32x4*>(xs + (size_t)rr * xstr + tid * 8) = xv16[r];
        const f16x8 h = *reinterpret_cast<const f16x8*>(&xv16[r]);
#pragma unroll
        for (int e = 0; e < 8; ++e) { const float v = (float)h[e] - cshift[r]; sa[r] += v; sb[r] += v * v; }
      }
    }
    stamp(pf, 2);
  } else
  if (fast) {
    uniform_load_wait();      // the rows' shifts (requested with the activation rows, long landed)
#pragma unroll
    for (int r = 0; r < RMAX; ++r) uniform_load_landed(cshift[r]);
#pragma unroll
    for (int r = 0; r < RMAX; ++r) {
      const int rr = r < M ? r : M - 1;       // clamped rows rewrite row M-1 with identical values (benign)
      sa[r] = 0.f; sb[r] = 0.f;
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const int k4 = tid + 256 * j;
        if (k4 < k4n) {
          const f16x4 o = {(f16)xv[r][j][0], (f16)xv[r][j][1], (f16)xv[r][j][2], (f16)xv[r][j][3]};
          *reinterpret_cast<f16x4*>(xs + (size_t)rr * xstr + k4 * 4) = o;
          const float a = xv[r][j][0] - cshift[r], b = xv[r][j][1] - cshift[r], c = xv[r][j][2] - cshift[r], e = xv[r][j][3] - cshift[r];
          sa[r] += (a + b) + (c + e); sb[r] += (a * a + b * b) + (c * c + e * e);
        }
      }
    }
    stamp(pf, 2);
  } else if (fastx) {
#pragma unroll
    for (int i = 0; i < NXH; ++i) {
      const int idx = tid + 256 * i;
      if (idx < nx) { const int row = WIS_ROW_OF(idx), k8 = idx - row * c8; *reinterpret_cast<u32x4*>(xs + (size_t)row * xstr + k8 * 8) = xh[i]; }
    }
  }

  f32x4 acc[MB];
#pragma unroll
  for (int mb = 0; mb < MB; ++mb) acc[mb] = f32x4{0.f, 0.f, 0.f, 0.f};
  int xrow[MB];
#pragma unroll
  for (int mb = 0; mb < MB; ++mb) { int r = mb * 16 + (lane & 15); xrow[mb] = (r < M ? r : M - 1) * xstr + 8 * (lane >> 4); }

  const int c8n = KC / 8;
  // p.flags sits in the by-value struct, which is not preloaded, and hipcc sank its scalar load BEHIND the MFMA loop, with the wait in front of the first
  // epilogue operand request.  MODE 1: held in an SGPR from here on, so it is fetched with the operand pointers in front of the loop and waited for at its head.
  int fl = 0;
  if constexpr (MODE == 1) { fl = p.flags; asm volatile("" : "+s"(fl)); }
  if constexpr (MODE == 1) __builtin_assume(K >= 128);      // (the loop runs: without this hipcc guards registers of the weight ring behind it with vmcnt waits for a path that skips it)
  for (int kc0 = 0; kc0 < K; kc0 += KC) {
    const WT* wq = wp4 + (size_t)(kc0 / 32 + ksl0) * wstep;
    const bool more = MB > 1 && kc0 + KC < K;     // (dead: MB == 1)
    if (kc0 > 0 && SC == 0) {
#pragma unroll
      for (int u = 0; u < GV_PF; ++u) if (u < S && wact) wf[u] = __builtin_nontemporal_load(wq + (size_t)u * wstep);
    }
    if (fastx && more) {   // next chunk's activations: in flight during this chunk's MFMAs
      const u32x4* x8 = reinterpret_cast<const u32x4*>(p.x) + ((kc0 + KC) >> 3);
#pragma unroll
      for (int i = 0; i < NXH; ++i) { const int idx = tid + 256 * i; if (idx < nx) { const int row = WIS_ROW_OF(idx); xh[i] = x8[(size_t)row * k8n + (idx - row * c8)]; } }
    }
    if (!fast && !fastx) {
      // stage x[:, kc0:kc0+KC] (f16 activations)
      {
        for (int idx = tid; idx < M * c8n; idx += 256) {
          const int r = idx / c8n, c8 = idx - r * c8n, k = kc0 + c8 * 8;
          *reinterpret_cast<f16x8*>(xs + (size_t)r * xstr + c8 * 8) =
              *reinterpret_cast<const f16x8*>(reinterpret_cast<const f16*>(p.x) + (size_t)r * K + k);
        }
      }
    }
    __syncthreads();
    stamp(pf, 3);
    if constexpr (NC == 8) {
#pragma unroll
      for (int u = 0; u < GV_PF; ++u) {
        const f16x8 a0 = WFrag<W8>::cvt(wf[u]);
        const f16x8 x0 = *reinterpret_cast<const f16x8*>(xs + xrow[0] + (ksl0 + 2 * u) * 32);
        acc[0] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a0, x0, acc[0], 0, 0, 0);
        u32x4 wr;      // row_ror:8 - lane l takes lane l ^ 8's registers
#pragma unroll
        for (int e = 0; e < 4; ++e) wr[e] = (unsigned)__builtin_amdgcn_update_dpp(0, (int)wf[u][e], 0x128, 0xf, 0xf, false);
        const f16x8 a1 = *reinterpret_cast<const f16x8*>(&wr);
        const f16x8 x1 = *reinterpret_cast<const f16x8*>(xs + xrow[0] + (ksl0 + 2 * u + 1) * 32);
        acc[0] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a1, x1, acc[0], 0, 0, 0);
      }
    } else if (SC > 0) {
#pragma unroll
      for (int u = 0; u < GV_PF; ++u) {
        const f16x8 a = WFrag<W8>::cvt(wf[u]);
#pragma unroll
        for (int mb = 0; mb < MB; ++mb) {
          const f16x8 xb = *reinterpret_cast<const f16x8*>(xs + xrow[mb] + (ksl0 + u) * 32);
          acc[mb] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a, xb, acc[mb], 0, 0, 0);
        }
        if (more && wact) wf[u] = __builtin_nontemporal_load(wq + (size_t)(KC / 32 + u) * wstep);   // same slot, next chunk
      }
    } else {
      for (int base = 0; base < S; base += GV_PF) {
#pragma unroll
        for (int u = 0; u < GV_PF; ++u) {
          if (base + u < S) {
            const f16x8 a = WFrag<W8>::cvt(wf[u]);
#pragma unroll
            for (int mb = 0; mb < MB; ++mb) {
              const f16x8 xb = *reinterpret_cast<const f16x8*>(xs + xrow[mb] + (ksl0 + base + u) * 32);
              acc[mb] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a, xb, acc[mb], 0, 0, 0);
            }
            if (base + u + GV_PF < S && wact) wf[u] = __builtin_nontemporal_load(wq + (size_t)(base + u + GV_PF) * wstep);
          }
        }
      }
    }
    __syncthreads();
    if (fastx && more) {
#pragma unroll
      for (int i = 0; i < NXH; ++i) {
        const int idx = tid + 256 * i;
        if (idx < nx) { const int row = WIS_ROW_OF(idx), k8 = idx - row * c8; *reinterpret_cast<u32x4*>(xs + (size_t)row * xstr + k8 * 8) = xh[i]; }
      }
    }
  }
  stamp(pf, 4);
  // (requested NOW - every weight fragment has been consumed, so they cannot hold up the in-order vmcnt queue - and
  // covered by the reductions and the barrier below; requested BEFORE the activations they delayed them and cost more than they saved)
  WIS_EP_LOADS()
#undef WIS_EP_LOADS
  if constexpr (MODE == 1) {   // LayerNorm statistics of the folded form: reduced here, behind the MFMAs, published with the accumulators
    // (the wave's 2 RM sums through one interleaved tree - wave_sum's own, word for word - and lane 0 publishes them behind ONE branch with wide LDS
    // stores; one wave_sum per value was ~190 dependent instructions, five exec-masked branches and five ds_write_b64 in front of the barrier, with
    // the MFMA loop over and nothing to run beside them)
    float t[2 * RMAX];
#pragma unroll
    for (int r = 0; r < RMAX; ++r) { t[2 * r] = sa[r]; t[2 * r + 1] = sb[r]; }
    wave_sums(t);
    if (lane == 0) {
      float* o = sred + wave * 16;
#pragma unroll
      for (int i = 0; i + 4 <= 2 * RMAX; i += 4) *reinterpret_cast<float4*>(o + i) = make_float4(t[i], t[i + 1], t[i + 2], t[i + 3]);
      if constexpr ((2 * RMAX) % 4 != 0) *reinterpret_cast<float2*>(o + 2 * RMAX - 2) = make_float2(t[2 * RMAX - 2], t[2 * RMAX - 1]);
    }
  } else if (fast) {
#pragma unroll
    for (int r = 0; r < RMAX; ++r) {
      const float ta = wave_sum(sa[r]), tb = wave_sum(sb[r]);
      if (lane == 0) { sred[wave * 16 + 2 * r] = ta; sred[wave * 16 + 2 * r + 1] = tb; }
    }
  }
  // cross-wave reduction; D[i = n][j = m]: lane holds m = lane&15, n = 4*(lane>>4) + r
#pragma unroll
  for (int mb = 0; mb < MB; ++mb)
    *reinterpret_cast<float4*>(red + ((size_t)(wave * MB + mb) * 64 + lane) * 4) = make_float4(acc[mb][0], acc[mb][1], acc[mb][2], acc[mb][3]);
  __syncthreads();
  stamp(pf, 5);
  if (tid < MB * NT * 64) {
    const int mb = NT == 2 ? 0 : tid >> 6, ln = tid & 63;
    float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
    if (NT == 2) {      // the two K halves of this wave's tile
      const int w0 = 2 * (tid >> 6);
      const float4 t0 = *reinterpret_cast<const float4*>(red + ((size_t)w0 * 64 + ln) * 4), t1 = *reinterpret_cast<const float4*>(red + ((size_t)(w0 + 1) * 64 + ln) * 4);
      s.x = t0.x + t1.x; s.y = t0.y + t1.y; s.z = t0.z + t1.z; s.w = t0.w + t1.w;
    } else {
#pragma unroll
    for (int w = 0; w < 4; ++w) {
      const float4 t = *reinterpret_cast<const float4*>(red + ((size_t)(w * MB + mb) * 64 + ln) * 4);
      s.x += t.x; s.y += t.y; s.z += t.z; s.w += t.w;
    }
    }
    const int m = ep_m, n = ep_n;
    float4 rsum = make_float4(0.f, 0.f, 0.f, 0.f);      // the residual row values this lane stored (statistics partials below)
    if (ep_ok) {
      if (W8) { s.x *= ep_sc.x; s.y *= ep_sc.y; s.z *= ep_sc.z; s.w *= ep_sc.w; }
      if (fast) {   // y = rs * (W' x - mu * c) [+ b' below]
        const int r = m < RMAX ? m : RMAX - 1;
        const float invK = 1.0f / (float)K;
        const float A = ((sred[2 * r] + sred[16 + 2 * r]) + (sred[32 + 2 * r] + sred[48 + 2 * r])) * invK;
        const float Bq = ((sred[2 * r + 1] + sred[17 + 2 * r]) + (sred[33 + 2 * r] + sred[49 + 2 * r])) * invK;
        float shift = cshift[0];                          // the row's shift x[m][0], still in registers
#pragma unroll
        for (int q = 1; q < RMAX; ++q) shift = (r == q) ? cshift[q] : shift;
        const float mu = shift + A;
        const float rs = 1.0f / sqrtf(fmaxf(Bq - A * A, 0.f) + 1e-5f);
        s.x = rs * (s.x - mu * ep_cs.x); s.y = rs * (s.y - mu * ep_cs.y); s.z = rs * (s.z - mu * ep_cs.z); s.w = rs * (s.w - mu * ep_cs.w);
      }
      s.x += ep_bias.x; s.y += ep_bias.y; s.z += ep_bias.z; s.w += ep_bias.w;
      if (WIS_FL & GV_QKV) {
        const int d = p.d;
        if (n < d) {
          *reinterpret_cast<float4*>(p.q + (size_t)m * d + n) = s;
        } else {
          const bool isk = n < 2 * d;
          // (MODE 1: slot and position widen by ZERO - both are non-negative -, which is no instruction; widened by sign, hipcc shifted each at its load,
          // behind an s_waitcnt vmcnt, so wave 0 of a K / V tile sat out the operands' round trip in front of the statistics reduction.  64-bit as before:
          // slot * ctx * d passes 2^31 elements at large's cache sizes.)
          f16* dst;
          if constexpr (MODE == 1) {
            asm volatile("" : "+v"(ep_slot), "+v"(ep_pos));      // (the 32-bit words as they landed, opaque up to here: nothing of the widening moves up to the requests)
            dst = (isk ? p.kc : p.vc) + ((size_t)(unsigned)ep_slot * (size_t)p.ctx + (size_t)(unsigned)ep_pos) * d + (n - (isk ? d : 2 * d));
          } else
          dst = (isk ? p.kc : p.vc) + ((size_t)ep_slot * p.ctx + ep_pos) * d + (n - (isk ? d : 2 * d));
          const f16x4 o = {(f16)s.x, (f16)s.y, (f16)s.z, (f16)s.w};
          *reinterpret_cast<f16x4*>(dst) = o;
        }
      } else {
        if (WIS_FL & GV_GELU) { s.x = gelu_erf(s.x); s.y = gelu_erf(s.y); s.z = gelu_erf(s.z); s.w = gelu_erf(s.w); }
        const size_t o = (size_t)m * p.N + n;
        if (WIS_FL & GV_RESID) {
          const float4 r = make_float4(ep_res.x + s.x, ep_res.y + s.y, ep_res.z + s.z, ep_res.w + s.w);
          rsum = r;
          *reinterpret_cast<float4*>(reinterpret_cast<float*>(p.y) + o) = r;
          if (p.y16) { const f16x4 h = {(f16)r.x, (f16)r.y, (f16)r.z, (f16)r.w}; *reinterpret_cast<f16x4*>(p.y16 + o) = h; }   // f16 copy: next layer's folded cross-Q input
        } else if (WIS_FL & GV_OUT_F32) {
          *reinterpret_cast<float4*>(reinterpret_cast<float*>(p.y) + o) = s;
        } else {
          const f16x4 h = {(f16)s.x, (f16)s.y, (f16)s.z, (f16)s.w};
          *reinterpret_cast<f16x4*>(reinterpret_cast<f16*>(p.y) + o) = h;
        }
      }
    }
    // LayerNorm partials of the rows this launch produces (GV_RESID with stat_out: the out-projection in front of the folded cross-attention
    // query): per (row, 16-column tile) the pair (sum, M2 about the tile mean), as gemv_frag_kernel's residual epilogue leaves them - the
    // four lanes of a row (kq = 0..3) hold four columns each; whole waves take part in the shuffles.  The consumer merges d / 16 pairs per
    // row instead of re-reading and re-summing the whole rows in every one of its workgroups.
    if ((WIS_FL & GV_RESID) && p.stat_out) {
      float t1 = ep_ok ? (rsum.x + rsum.y) + (rsum.z + rsum.w) : 0.f;
      t1 += __shfl_xor(t1, 16); t1 += __shfl_xor(t1, 32);
      float t2 = 0.f;
      if (ep_ok) { const float ml = t1 * 0.0625f, a_ = rsum.x - ml, b_ = rsum.y - ml, c_ = rsum.z - ml, e_ = rsum.w - ml; t2 = (a_ * a_ + b_ * b_) + (c_ * c_ + e_ * e_); }
      t2 += __shfl_xor(t2, 16); t2 += __shfl_xor(t2, 32);
      const int tile = nt * NT + (NT == 2 ? (tid >> 6) & 1 : 0);
      if ((lane >> 4) == 0 && m < M && rows * tile < p.N) *reinterpret_cast<float2*>(p.stat_out + ((size_t)m * (p.N >> 4) + tile) * 2) = make_float2(t1, t2);
    }
  }
  stamp(pf, 6);
  if (tid == 0) tl_end(p.prof);
#undef WIS_ROW_OF
#undef WIS_FL
}
// Kernel arguments: what the kernel needs BEFORE its first vector load (activation / weight base addresses, the shape) leads the
// argument list as plain scalars, the rest follows as the struct.  With -amdgpu-kernarg-preload-count (build.py) the command
// processor delivers the leading 16 dwords in SGPRs at wave launch, so the activation and weight requests go out without waiting
// for a scalar load of the kernarg segment (an HBM round trip: the step's 1.6 GB weight stream leaves nothing of it in the
// caches between replays); hipcc preloads only scalar / pointer arguments, never a by-value struct (kernarg_preload_length 0).
#define WIS_GV_LEAD(q) (q).x, (q).x2, (q).Wp, (q).M, (q).N, (q).K, (q).xsplit
#define WIS_GV_LEAD_DECL(s) const void* s##x, const void* s##x2, const f16* s##Wp, int s##M, int s##N, int s##K, int s##xsplit
#define WIS_GV_LEAD_APPLY(q, s) (q).x = s##x; (q).x2 = s##x2; (q).Wp = s##Wp; (q).M = s##M; (q).N = s##N; (q).K = s##K; (q).xsplit = s##xsplit
template <int MB, int MODE, int SC, int RM, bool W8, int NT = 1, int NC = 16>
__global__ __launch_bounds__(256) void gemv_kernel(WIS_GV_LEAD_DECL(l_), int KC, GemvP p) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  WIS_GV_LEAD_APPLY(p, l_);
  gemv_body<MB, MODE, SC, RM, W8, NT, NC>(p, KC, blockIdx.x, smem);
}
// Two skinny GEMMs in ONE launch (workgroups [0, nA) run problem A, the rest problem B; both f16-activation, single-chunk,
// <= 16 rows): the decoder's attention output projection together with the cross-attention query projection folded THROUGH it
// (model.hip out_cq_dual): one dependent stage instead of two.  At d = 384 and 1280 and <= 8 rows the stage runs a kernel of its own
// (gemv_out_cq_kernel below, out_cq_shape); this one serves the other widths and 9 .. 16 rows.
template <int SCA, int SCB>
__global__ __launch_bounds__(256) void gemv_dual_kernel(int nA, int M, const void* ax, const f16* aWp, const void* bx, const void* bx2, const f16* bWp, int bxsplit,
                                                        GemvP pa, GemvP pb) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  // (K of either problem is the instantiation's: SC k-steps of 32 per wave, four waves)
  if ((int)blockIdx.x < nA) { pa.x = ax; pa.x2 = nullptr; pa.Wp = aWp; pa.M = M; pa.K = SCA * 128; gemv_body<1, 2, SCA, 1, false>(pa, SCA * 128, blockIdx.x, smem); }
  else { pb.x = bx; pb.x2 = bx2; pb.Wp = bWp; pb.M = M; pb.K = SCB * 128; pb.xsplit = bxsplit; gemv_body<1, 2, SCB, 1, false>(pb, SCB * 128, (int)blockIdx.x - nA, smem); }
}
static bool out_cq_shape(const GemvP& pa, const GemvP& pb);      // the stage's own kernel (gemv_out_cq_kernel, below) and the pairs it serves
static void launch_out_cq(hipStream_t st, dim3 grid, dim3 block, size_t lds, int nA, const GemvP& a, const GemvP& b);
int launch_gemv_dual(hipStream_t st, const GemvP& pa, const GemvP& pb) {
  if (pa.M != pb.M || pa.M < 1 || pa.M > 16 || pa.x2 || pa.wscale || pb.wscale || (pa.flags & (GV_LN | GV_QKV)) || (pb.flags & (GV_LN | GV_QKV))) { set_error("gemv_dual: unsupported pair"); return WIS_E_UNSUPPORTED; }
  if (pa.M * (pa.K / 8) > 13 * 256 || pb.M * (pb.K / 8) > 13 * 256 || pa.K % 128 || pb.K % 128) { set_error("gemv_dual: rows do not fit the register staging (M=%d K=%d/%d)", pa.M, pa.K, pb.K); return WIS_E_UNSUPPORTED; }
  const int sa = pa.K / 128, sb = pb.K / 128;
  const size_t aux = (size_t)4 * 64 * 16 + MAX_ROWS * 8 + 4 * 16 * 4 + 16;
  const int Kmax = pa.K > pb.K ? pa.K : pb.K;
  const size_t lds = (((size_t)pa.M * (Kmax + 8) * 2 + 15) & ~(size_t)15) + aux;
  if (lds > 65536) { set_error("gemv_dual: LDS"); return WIS_E_UNSUPPORTED; }
  // pb.rows = 8: problem B's Wp is the eight-column image (out_cq_dual, where out_cq_nc8_shape holds) - twice the workgroups on B's side
  const bool b8 = pb.rows == 8;
  if (b8 && !(out_cq_shape(pa, pb) && out_cq_nc8_shape(pa.M, pa.K))) { set_error("gemv_dual: the eight-column image serves the out-projection + cross-Q pair of large's width, <= 8 rows (M=%d K=%d/%d)", pa.M, pa.K, pb.K); return WIS_E_UNSUPPORTED; }
  const int nA = cdiv(pa.N, 16), nB = b8 ? pb.N / 8 : cdiv(pb.N, 16);
  dim3 grid(nA + nB), block(256);
  GemvP a = pa, b = pb; a.rows = 16; b.rows = b8 ? 8 : 16;
  if (out_cq_shape(pa, pb)) launch_out_cq(st, grid, block, lds, nA, a, b);
  else if (sa == 10 && sb == 20) hipLaunchKernelGGL((gemv_dual_kernel<10, 20>), grid, block, lds, st, nA, a.M, a.x, a.Wp, b.x, b.x2, b.Wp, b.xsplit, a, b);
  else if (sa == 8 && sb == 16) hipLaunchKernelGGL((gemv_dual_kernel<8, 16>), grid, block, lds, st, nA, a.M, a.x, a.Wp, b.x, b.x2, b.Wp, b.xsplit, a, b);
  else if (sa == 6 && sb == 12) hipLaunchKernelGGL((gemv_dual_kernel<6, 12>), grid, block, lds, st, nA, a.M, a.x, a.Wp, b.x, b.x2, b.Wp, b.xsplit, a, b);
  else if (sa == 4 && sb == 8) hipLaunchKernelGGL((gemv_dual_kernel<4, 8>), grid, block, lds, st, nA, a.M, a.x, a.Wp, b.x, b.x2, b.Wp, b.xsplit, a, b);
  else if (sa == 3 && sb == 6) hipLaunchKernelGGL((gemv_dual_kernel<3, 6>), grid, block, lds, st, nA, a.M, a.x, a.Wp, b.x, b.x2, b.Wp, b.xsplit, a, b);
  else { set_error("gemv_dual: K=%d/%d not instantiated", pa.K, pb.K); return WIS_E_UNSUPPORTED; }
  return WIS_OK;
}

// ---- five-column slabs (the one-utterance FFN2 on 256 workgroups; image: pack_gemv_nc5_kernel) -------------------------------------------------------
// The NC = 8 idea with three k-steps per request.  Per request three MFMAs: the registers as they landed against the activations of k-step 3u, the same
// registers rotated left by five lanes within each row of 16 (rows 5-9 arrive in rows 0-4) against 3u + 1, rotated left by ten against 3u + 2.  Rows 0-4 of
// an accumulator see their k-steps in the sixteen-column order, each through the same MFMA; rows 5-15 are by-products nobody reads.
// DPP row_ror:n hands lane l the registers of lane (l - n) & 15 of its row: left by five is row_ror:11, left by ten row_ror:6.
// The requests go out in index order and request u's rotations stay behind request u - 1's MFMAs (only LDS reads and scalar work may cross): vmcnt retires
// in order, so the wave waits for ONE more request at a time and its MFMAs run while the rest of the stream is in flight.  Left alone, hipcc issued the loads
// out of order and hoisted the rotations - the wave then waited for the whole stream in front of its fifth request, and read each B operand from LDS one MFMA ahead.  (The same schedule on the eight-column
// kernel gained at K = 4d and lost 0.5 us per launch at K = d in the eager trace: that body is left as it was.)
#define GV_IN_ORDER() __builtin_amdgcn_sched_barrier(0x104)
template <int CTRL>
__device__ __forceinline__ f16x8 nc5_rot(const u32x4& w) {
  u32x4 r;
#pragma unroll
  for (int e = 0; e < 4; ++e) r[e] = (unsigned)__builtin_amdgcn_update_dpp(0, (int)w[e], CTRL, 0xf, 0xf, false);
  return *reinterpret_cast<const f16x8*>(&r);
}
// Five columns are 20 / 10 bytes of a row: the epilogue's lanes address them at element, not vector, alignment (gfx950 takes global accesses at any alignment).
// Lanes with k-quarter 0 hold local columns 0-3 of the accumulator, lanes with k-quarter 1 local column 4 in element 0: the latter move it to element 3 and
// address the four columns that END at the slab's last one (`5 slab + kq`), so one request per operand serves both groups and nothing past the row is read.
__device__ __forceinline__ f32x4 ld4_f32(const float* p) { f32x4 v; __builtin_memcpy(&v, p, 16); return v; }
// (component by component: a sum of ext-vector values lowers to packed-f32 instructions, which no kernel with MFMAs may contain - tools/isa_lint.py)
__device__ __forceinline__ f32x4 add4_f32(const f32x4& a, const f32x4& b) { return f32x4{a[0] + b[0], a[1] + b[1], a[2] + b[2], a[3] + b[3]}; }
__device__ __forceinline__ void st_nc5_f32(float* p, const f32x4& v, int kq) { if (kq) p[3] = v[3]; else __builtin_memcpy(p, &v, 16); }
__device__ __forceinline__ void st_nc5_f16(f16* p, const f32x4& v, int kq) {
  const f16x4 h = {(f16)v[0], (f16)v[1], (f16)v[2], (f16)v[3]};
  if (kq) p[3] = h[3]; else __builtin_memcpy(p, &h, 8);
}
// FFN2's form: gemv_body MODE 2 (f16 rows, staged from registers) on slab blockIdx.x; the four waves take a K quarter of SC k-steps each - ceil(SC / 3)
// requests, all up front -, meet in LDS and wave 0 finishes the five columns as gemv_body finishes sixteen: per element the same sums in the same order.
template <int SC>
__global__ __launch_bounds__(256) void gemv_nc5_kernel(WIS_GV_LEAD_DECL(l_), int KC, GemvP p) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  WIS_GV_LEAD_APPLY(p, l_);
  (void)KC;
  constexpr int K = SC * 128, RQ = (SC + 2) / 3, xstr = K + 8, c8 = K / 8, NXH = 13;
  const int M = p.M;
  f16* xs = reinterpret_cast<f16*>(smem);
  float* red = reinterpret_cast<float*>(smem + (((size_t)M * xstr * 2 + 15) & ~(size_t)15));
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, slab = blockIdx.x;
  unsigned long long* pf = (slab == 0 && tid == 0) ? p.prof : nullptr;
  if (tid == 0) tl_begin(p.prof);
  stamp(pf, 0);
  u32x4 xh[NXH];
  const int nx = M * c8;
  const u32x4* x8 = reinterpret_cast<const u32x4*>(p.x);
#pragma unroll
  for (int i = 0; i < NXH; ++i) { const int idx = tid + 256 * i; if (idx < nx) xh[i] = x8[idx]; }
  const u32x4* wp4 = reinterpret_cast<const u32x4*>(p.Wp) + ((size_t)slab * 4 + wave) * RQ * 64 + lane;
  u32x4 wf[RQ];
#pragma unroll
  for (int u = 0; u < RQ; ++u) { wf[u] = __builtin_nontemporal_load(wp4 + (size_t)u * 64); GV_IN_ORDER(); }
  stamp(pf, 1);
#pragma unroll
  for (int i = 0; i < NXH; ++i) {
    const int idx = tid + 256 * i;
    if (idx < nx) { const int row = idx / c8, k8 = idx - row * c8; *reinterpret_cast<u32x4*>(xs + (size_t)row * xstr + k8 * 8) = xh[i]; }
  }
  __syncthreads();
  stamp(pf, 3);
  f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
  const int m = lane & 15, kq = lane >> 4;
  const f16* xw = xs + (m < M ? m : M - 1) * xstr + 8 * kq + wave * SC * 32;
  // the wave's B operands, all SC k-steps, into registers while its weights are in flight (one workgroup per CU: the register file is this wave's): read
  // one MFMA ahead, each LDS round trip sat between two MFMAs of a wave whose weights had all landed
  f16x8 xb[SC];
#pragma unroll
  for (int k = 0; k < SC; ++k) xb[k] = *reinterpret_cast<const f16x8*>(xw + k * 32);
  __builtin_amdgcn_sched_barrier(0);
#pragma unroll
  for (int u = 0; u < RQ; ++u) {
    acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(*reinterpret_cast<const f16x8*>(&wf[u]), xb[3 * u], acc, 0, 0, 0);
    if (3 * u + 1 < SC) acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(nc5_rot<0x12B>(wf[u]), xb[3 * u + 1 < SC ? 3 * u + 1 : 0], acc, 0, 0, 0);
    if (3 * u + 2 < SC) acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(nc5_rot<0x126>(wf[u]), xb[3 * u + 2 < SC ? 3 * u + 2 : 0], acc, 0, 0, 0);
    GV_IN_ORDER();
  }
  stamp(pf, 4);
  // epilogue operands, requested behind the stream and covered by the reduction barrier, as in gemv_body
  const bool ep_ok = wave == 0 && m < M && kq < 2;
  const size_t o = (size_t)m * p.N + 5 * slab + kq;
  f32x4 ep_bias = f32x4{0.f, 0.f, 0.f, 0.f}, ep_res = ep_bias;
  if (ep_ok) {
    if (p.bias) ep_bias = ld4_f32(p.bias + 5 * slab + kq);
    if (p.flags & GV_RESID) ep_res = ld4_f32(reinterpret_cast<const float*>(p.y) + o);
  }
  *reinterpret_cast<f32x4*>(red + ((size_t)wave * 64 + lane) * 4) = acc;
  __syncthreads();
  stamp(pf, 5);
  if (wave == 0) {
    f32x4 s = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int w = 0; w < 4; ++w) s = add4_f32(s, *reinterpret_cast<const f32x4*>(red + ((size_t)w * 64 + lane) * 4));
    if (ep_ok) {
      if (kq) s[3] = s[0];
      s = add4_f32(s, ep_bias);
      if (p.flags & GV_GELU) { s[0] = gelu_erf(s[0]); s[1] = gelu_erf(s[1]); s[2] = gelu_erf(s[2]); s[3] = gelu_erf(s[3]); }
      if (p.flags & GV_RESID) {
        const f32x4 r = add4_f32(ep_res, s);
        st_nc5_f32(reinterpret_cast<float*>(p.y) + o, r, kq);
        if (p.y16) st_nc5_f16(p.y16 + o, r, kq);
      } else if (p.flags & GV_OUT_F32) st_nc5_f32(reinterpret_cast<float*>(p.y) + o, s, kq);
      else st_nc5_f16(reinterpret_cast<f16*>(p.y) + o, s, kq);
    }
  }
  stamp(pf, 6);
  if (tid == 0) tl_end(p.prof);
}

// ---- the fused out-projection + folded cross-Q stage of <= 8 rows: a kernel of its own (launch_gemv_dual selects it) ------------------------------------
// gemv_dual_kernel's two arms on the same sixteen-column images, the same k order per wave, the same cross-wave sum and epilogue arithmetic: the same bits.
// What differs is when a wave asks for what.  In gemv_dual_kernel<10, 20> the guarded activation requests (`if (idx < nx) xh[i] = ...`, thirteen slots for
// rows that fill five) compiled to thirteen branches with a wait for everything outstanding behind each load: three dependent memory round trips, four in
// wave 0, before the first weight byte was requested.  Here a thread's pieces number what eight rows need (NXH), every one is requested unconditionally at a
// clamped index - a thread beyond the rows asks for the last piece and drops it - and the arm's weight requests follow in index order with no branch and no
// wait in between.  Arm B (K = 2d, the longer stream) takes gemv_nc5_kernel's schedule: the wave's B operands go from LDS into registers once behind the
// staging barrier, and the MFMAs consume the requests in index order while the rest of the stream is in flight (left alone, hipcc waited for 19 of the 20
// requests behind the fourth MFMA and read each B operand from LDS in front of its MFMA).  Arm A keeps gemv_body's loop.
// SC = d / 128: k-steps per wave of arm A; arm B's waves take 2 SC.
// NC (arm B): output columns per workgroup.  8: Wp is the eight-column image (pack_gemv_nc8_kernel) - a request is eight columns x two k-steps, two MFMAs
// through row_ror:8 as in gemv_body NC = 8, SW / 2 requests per wave, d / 8 workgroups.
template <int SC, bool ARM_B, int NC = 16>
__device__ __forceinline__ void out_cq_arm(const GemvP& p, const int nt, char* smem) {
  static_assert(NC == 16 || (NC == 8 && ARM_B), "eight-column tiles: arm B");
  constexpr int SW = ARM_B ? 2 * SC : SC, K = SW * 128, xstr = K + 8, c8 = K / 8, s8 = c8 / 2;
  constexpr int RQ = NC == 8 ? SW / 2 : SW;      // weight requests per wave
  constexpr int NXH = (8 * c8 + 255) / 256;      // 16-byte pieces per thread at eight rows
  const int M = p.M;
  f16* xs = reinterpret_cast<f16*>(smem);
  float* red = reinterpret_cast<float*>(smem + (((size_t)M * xstr * 2 + 15) & ~(size_t)15));
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  unsigned long long* pf = (nt == 0 && tid == 0) ? p.prof : nullptr;
  if (tid == 0) tl_begin(p.prof);
  stamp(pf, 0);
  // activation rows (written by the previous launch): arm A's are the attention output, arm B's the row-wise concatenation [x | x2] at column d
  const int nx = M * c8;
  const u32x4* x8 = reinterpret_cast<const u32x4*>(p.x);
  const u32x4* y8 = reinterpret_cast<const u32x4*>(p.x2);
  u32x4 xh[NXH];
#pragma unroll
  for (int i = 0; i < NXH; ++i) {
    const int idx = min(tid + 256 * i, nx - 1);
    if (ARM_B) {
      const int row = idx / c8, col = idx - row * c8;
      const u32x4* src = col < s8 ? x8 + (row * s8 + col) : y8 + (row * s8 + (col - s8));
      xh[i] = *src;
    } else xh[i] = x8[idx];
  }
  GV_IN_ORDER();
  // the wave's weight fragments: k-steps wave SW .. wave SW + SW - 1 of tile nt, all requested up front (either image: RQ KiB-requests per tile and wave)
  const u32x4* wq = reinterpret_cast<const u32x4*>(p.Wp) + ((size_t)nt * 4 + wave) * RQ * 64 + lane;
  u32x4 wf[RQ];
#pragma unroll
  for (int u = 0; u < RQ; ++u) { wf[u] = __builtin_nontemporal_load(wq + (size_t)u * 64); GV_IN_ORDER(); }
  stamp(pf, 1);
#pragma unroll
  for (int i = 0; i < NXH; ++i) {
    const int idx = tid + 256 * i;
    if (idx < nx) { const int row = idx / c8, k8 = idx - row * c8; *reinterpret_cast<u32x4*>(xs + (size_t)row * xstr + k8 * 8) = xh[i]; }
  }
  __syncthreads();
  stamp(pf, 3);
  f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
  const f16* xw = xs + ((lane & 15) < M ? (lane & 15) : M - 1) * xstr + 8 * (lane >> 4) + wave * SW * 32;
  if (ARM_B) {
    f16x8 xb[SW];
#pragma unroll
    for (int k = 0; k < SW; ++k) xb[k] = *reinterpret_cast<const f16x8*>(xw + k * 32);
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int u = 0; u < RQ; ++u) {
      if (NC == 8) {      // rows 0-7 of the accumulator see k-steps 2 u, 2 u + 1 in order; rows 8-15 are by-products nobody reads
        acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(*reinterpret_cast<const f16x8*>(&wf[u]), xb[2 * u], acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(nc5_rot<0x128>(wf[u]), xb[NC == 8 ? 2 * u + 1 : 0], acc, 0, 0, 0);
      } else acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(*reinterpret_cast<const f16x8*>(&wf[u]), xb[u], acc, 0, 0, 0);
      GV_IN_ORDER();
    }
  } else {
#pragma unroll
    for (int u = 0; u < SW; ++u)
      acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(*reinterpret_cast<const f16x8*>(&wf[u]), *reinterpret_cast<const f16x8*>(xw + u * 32), acc, 0, 0, 0);
  }
  stamp(pf, 4);
  // epilogue operands, requested behind the stream and covered by the reduction barrier, as in gemv_body; wave 0 finishes the tile
  const int ep_m = lane & 15, ep_n = NC * nt + 4 * (lane >> 4);
  const bool ep_ok = tid < 64 && ep_m < M && ep_n < p.N && 4 * (lane >> 4) < NC;
  float4 ep_bias = make_float4(0.f, 0.f, 0.f, 0.f), ep_res = ep_bias;
  if (ep_ok) {
    if (p.bias) ep_bias = *reinterpret_cast<const float4*>(p.bias + ep_n);
    if (!ARM_B) ep_res = *reinterpret_cast<const float4*>(reinterpret_cast<const float*>(p.y) + (size_t)ep_m * p.N + ep_n);
  }
  *reinterpret_cast<float4*>(red + ((size_t)wave * 64 + lane) * 4) = make_float4(acc[0], acc[1], acc[2], acc[3]);
  __syncthreads();
  stamp(pf, 5);
  if (tid < 64) {
    float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
    for (int w = 0; w < 4; ++w) {
      const float4 t = *reinterpret_cast<const float4*>(red + ((size_t)w * 64 + lane) * 4);
      s.x += t.x; s.y += t.y; s.z += t.z; s.w += t.w;
    }
    float4 rsum = make_float4(0.f, 0.f, 0.f, 0.f);
    if (ep_ok) {
      s.x += ep_bias.x; s.y += ep_bias.y; s.z += ep_bias.z; s.w += ep_bias.w;
      const size_t o = (size_t)ep_m * p.N + ep_n;
      if (ARM_B) {      // GV_OUT_F32: the raw folded query
        *reinterpret_cast<float4*>(reinterpret_cast<float*>(p.y) + o) = s;
      } else {          // GV_RESID: x1 in place
        const float4 r = make_float4(ep_res.x + s.x, ep_res.y + s.y, ep_res.z + s.z, ep_res.w + s.w);
        rsum = r;
        *reinterpret_cast<float4*>(reinterpret_cast<float*>(p.y) + o) = r;
      }
    }
    // LayerNorm partials of x1 per (row, 16-column tile): (sum, M2 about the tile mean), gemv_body's arithmetic - the cross-attention merges d / 16 pairs per row
    if (!ARM_B && p.stat_out) {
      float t1 = ep_ok ? (rsum.x + rsum.y) + (rsum.z + rsum.w) : 0.f;
      t1 += __shfl_xor(t1, 16); t1 += __shfl_xor(t1, 32);
      float t2 = 0.f;
      if (ep_ok) { const float ml = t1 * 0.0625f, a_ = rsum.x - ml, b_ = rsum.y - ml, c_ = rsum.z - ml, e_ = rsum.w - ml; t2 = (a_ * a_ + b_ * b_) + (c_ * c_ + e_ * e_); }
      t2 += __shfl_xor(t2, 16); t2 += __shfl_xor(t2, 32);
      if ((lane >> 4) == 0 && ep_m < M && 16 * nt < p.N) *reinterpret_cast<float2*>(p.stat_out + ((size_t)ep_m * (p.N >> 4) + nt) * 2) = make_float2(t1, t2);
    }
  }
  stamp(pf, 6);
  if (tid == 0) tl_end(p.prof);
}
// (the argument list of gemv_dual_kernel: what the first loads need leads as scalars)
template <int SC, int NCB>
__global__ __launch_bounds__(256) void gemv_out_cq_kernel(int nA, int M, const void* ax, const f16* aWp, const void* bx, const void* bx2, const f16* bWp, int bxsplit,
                                                          GemvP pa, GemvP pb) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  (void)bxsplit;      // (= d: the launcher checked it)
  if ((int)blockIdx.x < nA) { pa.x = ax; pa.x2 = nullptr; pa.Wp = aWp; pa.M = M; out_cq_arm<SC, false>(pa, blockIdx.x, smem); }
  else { pb.x = bx; pb.x2 = bx2; pb.Wp = bWp; pb.M = M; out_cq_arm<SC, true, NCB>(pb, (int)blockIdx.x - nA, smem); }
}
// arm B on eight-column tiles: large's width, a CU for each of the d / 16 + d / 8 workgroups (one dispatch round, as gemv_nc5_shape)
bool out_cq_nc8_shape(int M, int d) { return d == 1280 && M >= 1 && M <= 8 && d / 16 + d / 8 <= device_cu_count(); }
// the pairs the kernel above serves (launch_gemv_dual has checked the rest): the stage as out_cq_dual assembles it - residual out-projection d x d beside the
// raw cross-Q d x 2d on [x | x2] split at d, f16 weights, whole sixteen-column tiles, <= 8 rows - at the widths it is instantiated for
static bool out_cq_shape(const GemvP& pa, const GemvP& pb) {
  return pa.M <= 8 && pa.flags == GV_RESID && pb.flags == GV_OUT_F32 && pb.K == 2 * pa.K && pb.x2 && pb.xsplit == pa.K && !pa.y16 && !pb.y16 && !pb.stat_out &&
         pa.N % 16 == 0 && pb.N % 16 == 0 && (pa.K == 1280 || pa.K == 384);
}
static void launch_out_cq(hipStream_t st, dim3 grid, dim3 block, size_t lds, int nA, const GemvP& a, const GemvP& b) {
  if (b.rows == 8) hipLaunchKernelGGL((gemv_out_cq_kernel<10, 8>), grid, block, lds, st, nA, a.M, a.x, a.Wp, b.x, b.x2, b.Wp, b.xsplit, a, b);
  else if (a.K == 1280) hipLaunchKernelGGL((gemv_out_cq_kernel<10, 16>), grid, block, lds, st, nA, a.M, a.x, a.Wp, b.x, b.x2, b.Wp, b.xsplit, a, b);
  else hipLaunchKernelGGL((gemv_out_cq_kernel<3, 16>), grid, block, lds, st, nA, a.M, a.x, a.Wp, b.x, b.x2, b.Wp, b.xsplit, a, b);
}
int launch_gemv(hipStream_t st, const GemvP& p) {
  if (p.M < 1 || p.M > 16 || p.K < 128 || p.K % 128 || (p.N % 4 && p.rows != 5)) { set_error("gemv: M=%d N=%d K=%d unsupported (the LDS-staged form holds one 16-row block; more rows take launch_gemv_frag)", p.M, p.N, p.K); return WIS_E_UNSUPPORTED; }
  // largest K-chunk (multiple of 128 dividing K) whose f16 image of M rows fits 64 KiB of LDS (several workgroups per CU)
  int KC = p.K;
  const size_t aux = (size_t)4 * 64 * 16 + MAX_ROWS * 8 + 4 * 16 * 4 + 16;   // red + stats + sred (+ alignment)
  while ((size_t)p.M * (KC + 8) * 2 + aux > 65536) {
    int next = 0;
    for (int c = KC - 128; c >= 128; c -= 128) if (p.K % c == 0) { next = c; break; }
    if (!next) { set_error("gemv: cannot chunk K=%d for M=%d", p.K, p.M); return WIS_E_UNSUPPORTED; }
    KC = next;
  }
  const size_t lds = (((size_t)p.M * (KC + 8) * 2 + 15) & ~(size_t)15) + aux;
  const int rows = p.rows ? p.rows : 16;
  GemvP pp = p; pp.rows = rows;
  const int npad = cdiv(p.N, rows) * rows;
  dim3 grid(npad / rows), block(256);
  int mode = 0;
  if (p.flags & GV_LN) {
    // folded LayerNorm: raw fp32 rows in registers - at most 8 rows of at most 2048 columns (more rows take launch_gemv_frag)
    if (p.M > 8 || p.K > 2048 || KC != p.K || !p.csum) { set_error("gemv: fused LayerNorm needs M <= 8, K <= 2048 and the folded column sums (M=%d K=%d)", p.M, p.K); return WIS_E_UNSUPPORTED; }
  }
  if (p.flags & GV_LN16) {
    if ((p.flags & GV_LN) || p.M > 8 || p.K > 2048 || p.K % 8 || KC != p.K || !p.csum) {
      set_error("gemv: the LayerNorm fold on f16 rows needs column sums, M <= 8, K <= 2048 (M=%d K=%d)", p.M, p.K); return WIS_E_UNSUPPORTED; }
  }
  if (KC == p.K) {
    if (p.flags & GV_LN) mode = 1;
    else if (p.flags & GV_LN16) mode = 3;
    else if (p.M * (p.K / 8) <= 13 * 256) mode = 2;
  }
  const int sck = KC / 128;
  const int sc = (KC == p.K && (sck == 3 || sck == 4 || sck == 6 || sck == 8 || sck == 10)) ? sck : 0;
  // rows = 5: Wp is the five-column image (gemv_nc5_kernel), one slab per workgroup
  if (rows == 5) {
    if (mode != 2 || p.wscale || p.stat_out || p.x2 || !gemv_nc5_shape(p.M, p.N, p.K, p.flags)) {
      set_error("gemv: the five-column image serves f16 rows and weights at K = 5120 without row partials, one dispatch round (M=%d N=%d K=%d flags=%d)", p.M, p.N, p.K, p.flags); return WIS_E_UNSUPPORTED; }
    hipLaunchKernelGGL((gemv_nc5_kernel<40>), dim3(p.N / 5), block, lds, st, WIS_GV_LEAD(pp), KC, pp);
    return WIS_OK;
  }
#define WIS_GV1(MODEv, SCv, RMv, W8v) hipLaunchKernelGGL((gemv_kernel<1, MODEv, SCv, RMv, W8v>), grid, block, lds, st, WIS_GV_LEAD(pp), KC, pp)
#define WIS_GV(MODEv, SCv, RMv) do { if (p.wscale) WIS_GV1(MODEv, SCv, RMv, true); else WIS_GV1(MODEv, SCv, RMv, false); } while (0)
#define WIS_GV_SC(MODEv, RMv) do { switch (sc) { case 3: WIS_GV(MODEv, 3, RMv); break; case 4: WIS_GV(MODEv, 4, RMv); break; case 6: WIS_GV(MODEv, 6, RMv); break; \
                                                 case 8: WIS_GV(MODEv, 8, RMv); break; case 10: WIS_GV(MODEv, 10, RMv); break; default: WIS_GV(MODEv, 0, RMv); } } while (0)
  // two n-tiles per workgroup (gemv_body NT = 2): FFN1 of the one-utterance step (K = 1280, N >= 4096, 4-5 rows, f16 weights) - 320 tiles on 256 CUs left a
  // quarter of the CUs with two workgroups; 160 two-tile workgroups: decode step 1.268 -> 1.250 ms.  Not the QKV projection: its 240 tiles had a CU each
  // already, and 120 fat workgroups measured SLOWER (1.292 ms) - fatter workgroups pay only where they remove a second round.
  if (mode == 1 && sc == 10 && p.M > 3 && p.M <= 5 && !p.wscale && rows == 16 && p.N % 32 == 0 && !(p.flags & (GV_RESID | GV_QKV)) && p.N >= 4096) {
    hipLaunchKernelGGL((gemv_kernel<1, 1, 20, 5, false, 2>), dim3(p.N / 32), block, lds, st, WIS_GV_LEAD(pp), KC, pp);
    return WIS_OK;
  }
  // rows = 8: Wp is the eight-column image (gemv_body NC = 8) - twice the workgroups, half the weight requests each.  Plain and residual
  // epilogues only: the LayerNorm partials of stat_out are per sixteen columns
  if (rows != 16 && rows != 8) { set_error("gemv: %d-row weight tiles have no kernel", rows); return WIS_E_UNSUPPORTED; }
  if (rows == 8) {
    if (mode != 2 || p.wscale || p.stat_out || (p.flags & GV_QKV) || !gemv_nc8_shape(p.M, p.N, p.K)) {
      set_error("gemv: the eight-column image serves f16 rows and weights at K = 1280 / 5120 without row partials (M=%d N=%d K=%d flags=%d)", p.M, p.N, p.K, p.flags); return WIS_E_UNSUPPORTED; }
    if (sck == 40) hipLaunchKernelGGL((gemv_kernel<1, 2, 40, 1, false, 1, 8>), dim3(p.N / 8), block, lds, st, WIS_GV_LEAD(pp), KC, pp);
    else hipLaunchKernelGGL((gemv_kernel<1, 2, 10, 1, false, 1, 8>), dim3(p.N / 8), block, lds, st, WIS_GV_LEAD(pp), KC, pp);
    return WIS_OK;
  }
  if (mode == 1) { if (p.M <= 3) WIS_GV_SC(1, 3); else if (p.M <= 5) WIS_GV_SC(1, 5); else WIS_GV_SC(1, 8); }
  else if (mode == 3) { if (p.M <= 3) WIS_GV_SC(3, 3); else if (p.M <= 5) WIS_GV_SC(3, 5); else WIS_GV_SC(3, 8); }
  else if (mode == 2) {
    // K = 4d of the one-utterance step (FFN2: 80 workgroups x 160 KiB of weights): EVERY fragment requested up front (40 per wave:
    // 160 VGPRs, one workgroup per CU anyway) instead of a ring of 16 - the ring held 64 KiB in flight per CU, and 80 CUs x 64 KiB
    // over the memory latency is what the stream ran at
    if (sck == 40 && !p.wscale) WIS_GV1(2, 40, 1, false);
    else WIS_GV_SC(2, 1);
  } else WIS_GV_SC(0, 1);
#undef WIS_GV_SC
#undef WIS_GV
#undef WIS_GV1
  return WIS_OK;
}

// =======================================================================================
// Batched decode rows (8 < M <= 96): skinny GEMM on activation FRAGMENT images.  grid = Npad/16 workgroups of 4 waves; wave w owns
// the k-steps [w*S, (w+1)*S), S = K/128.  Per k-step a wave issues ONE 1 KiB weight fragment load (HBM, non-temporal) and MB
// 1 KiB activation fragment loads (L2: the image is 40-120 KiB and every workgroup reads it), PF k-steps ahead of the MFMAs -
// no LDS staging of the activations, no staging barrier, 12 KiB of LDS (the cross-wave reduction) so several workgroups share a CU
// (the LDS-staged form held 103 KiB per workgroup: one workgroup per CU, two dispatch rounds for the 320-tile FFN1).
// LayerNorm (GV_LN): the projection is stored folded (W o gamma, b + W.beta, column sums c); mean / rstd of a row come from the
// per-16-column partial sums the producing residual epilogue left in stat_in (summed in a fixed order: deterministic):
//   y = rs * (W'x - mu * c) + b'.
// Residual epilogues (GV_RESID) write the fp32 rows in place, their f16 fragment image for the next projection and the partials.
// A lane's quarter of a row's LayerNorm partials at K = 1280: 20 (sum, M2) pairs = 160 contiguous bytes, taken as TEN 16-byte loads requested together (they were 20
// eight-byte loads - in the two-tile kernel issued four at a time, five dependent rounds in the kernel's tail; a wave request costs the CU's address path the same
// whatever it carries); merged in pair order: the sums come out bit for bit as before.
__device__ __forceinline__ void ln_partials20(const float2* sp, float c, float& s1, float& s2) {
  const float4* sp4 = reinterpret_cast<const float4*>(sp);
  float4 v[10];
#pragma unroll
  for (int i = 0; i < 10; ++i) v[i] = sp4[i];
#pragma unroll
  for (int i = 0; i < 10; ++i) {
    const float dm0 = v[i].x * 0.0625f - c; s1 += dm0; s2 += v[i].y + 16.0f * dm0 * dm0;
    const float dm1 = v[i].z * 0.0625f - c; s1 += dm1; s2 += v[i].w + 16.0f * dm1 * dm1;
  }
}
// MS (r6): M split - the workgroup computes MB row blocks (from p.mb0) of an image of p.mbi: a projection with few n-tiles (d x d: 80) is run by
// (n-tile, row-block group) workgroups, each pulling ITS rows' activation fragments through its CU instead of the whole image (the phase stamps put 40-50 %
// of such a wave's life into getting the image's requests accepted: profiles/r06_phase_cycles.md); no cross-workgroup reduction - rows are independent.
// The row-block groups of an n-tile read the same weight fragments (ids a multiple of 8 apart: dispatched to the same XCD, whose L2 serves the repeats), so
// the weights are requested with ordinary loads there, not non-temporal ones.
template <int MB, int PF, bool W8, bool MS = false>
__device__ __forceinline__ void gemv_frag_body(const GemvP& p, const int nt, const int KS, const int ksi) {
  typedef typename WFrag<W8>::T WT;
  constexpr int EPN = (MB + 3) / 4;      // row blocks a wave finishes in the epilogue: wave w owns blocks w, w + 4 (up to 96 rows = 6 blocks)
  __shared__ __attribute__((aligned(16))) float red[4 * MB * 64 * 4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  // K slices (KS > 1: the K = 4d projection - 80 workgroups would each pull the whole activation image and a 160 KiB weight
  // panel through one CU's ~55 GB/s; see GemvP::ksplit): slice ksi covers the k-steps [ksi, ksi + 1) * ksteps / KS, a quarter per wave
  const int M = p.M, K = p.K, ksteps = K >> 5, S = ksteps / (4 * KS);
  // (wks / wk0: the matrix is a k-step window of a wider packed image - the two halves of the folded cross-Q matrix [W'q | W'q Wo])
  const int wks = p.wks ? p.wks : ksteps;
  // phase stamps of ONE wave (tap builds only; stamp() is empty otherwise): workgroup 0 / slice 0 / thread 0 -
  // 0 start, 1 first PF k-steps requested, 2 stream consumed (MFMA loop), 3 epilogue operands requested + partial sums in LDS + barrier,
  // 4 K-split merge passed (ticket), 5 epilogue done
  unsigned long long* pf = (nt == 0 && ksi == 0 && tid == 0 && (!MS || p.mb0 == 0)) ? p.prof : nullptr;
  stamp(pf, 0);
  const WT* wq = reinterpret_cast<const WT*>(p.Wp) + ((size_t)nt * wks + p.wk0 + (size_t)(ksi * 4 + wave) * S) * 64 + lane;
  const int MBI = MS ? p.mbi : MB, mb0 = MS ? p.mb0 : 0;      // row blocks of the image, this workgroup's first
  const u32x4* xq = reinterpret_cast<const u32x4*>(p.x) + ((size_t)(ksi * 4 + wave) * S * MBI + mb0) * 64 + lane;
  WT a[PF]; u32x4 b[PF][MB];
#pragma unroll
  for (int u = 0; u < PF; ++u) {
    if (u < S) {
      a[u] = MS ? wq[(size_t)u * 64] : __builtin_nontemporal_load(wq + (size_t)u * 64);
#pragma unroll
      for (int mb = 0; mb < MB; ++mb) b[u][mb] = xq[(size_t)(u * MBI + (MS && mb0 + mb >= MBI ? 0 : mb)) * 64];      // (a ragged last group: a valid block, its sums discarded)
    }
  }
  stamp(pf, 1);
  f32x4 acc[MB];
#pragma unroll
  for (int mb = 0; mb < MB; ++mb) acc[mb] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int base = 0; base < S; base += PF) {
#pragma unroll
    for (int u = 0; u < PF; ++u) {
      if (base + u < S) {
        const f16x8 av = WFrag<W8>::cvt(a[u]);
#pragma unroll
        for (int mb = 0; mb < MB; ++mb) acc[mb] = __builtin_amdgcn_mfma_f32_16x16x32_f16(av, *reinterpret_cast<const f16x8*>(&b[u][mb]), acc[mb], 0, 0, 0);
        const int nx = base + u + PF;
        if (nx < S) {
          a[u] = MS ? wq[(size_t)nx * 64] : __builtin_nontemporal_load(wq + (size_t)nx * 64);
#pragma unroll
          for (int mb = 0; mb < MB; ++mb) b[u][mb] = xq[(size_t)(nx * MBI + (MS && mb0 + mb >= MBI ? 0 : mb)) * 64];
        }
      }
    }
  }
  stamp(pf, 2);
  // epilogue operands: requested behind the whole stream, covered by the reduction barrier
  const int l15 = lane & 15, kq = lane >> 4;
  const int ep_n = 16 * nt + 4 * kq;
  const bool ln = p.flags & GV_LN;
  const int nq = K >> 6;                                      // (K/16) partial pairs per row, a quarter per lane
  // LayerNorm statistics from the row's per-16-column partials (sum, M2 about the tile's own mean - see the residual epilogue
  // below): pairs merge like Welford / Chan states, in ONE pass about a shift c = the mean of the row's first tile:
  //   mu = c + mean_t(m_t - c),   M2 = sum_t (M2_t + 16 (m_t - c)^2) - K (mu - c)^2
  // so a row whose mean is large against its spread loses nothing to the E[x^2] - mu^2 cancellation (|mu - c| is of the order of
  // the row's own spread; the <= 8-row kernel shifts by x[r][0] for the same reason), and both sums are ready before the reduction
  // barrier (a second pass about the exact mean put a dependent lane exchange + 20 more reads behind it).
  bool ep_act[EPN], ep_ok[EPN]; int ep_m[EPN];
  float4 ep_bias = make_float4(0.f, 0.f, 0.f, 0.f), ep_cs = ep_bias, ep_sc = make_float4(1.f, 1.f, 1.f, 1.f);
  float4 ep_res[EPN]; int ep_slot[EPN], ep_pos[EPN]; float s1[EPN], s2[EPN], sc0[EPN];
  if (ep_n < p.N) {
    if (p.bias) ep_bias = *reinterpret_cast<const float4*>(p.bias + ep_n);
    if (ln) ep_cs = *reinterpret_cast<const float4*>(p.csum + ep_n);
    if (W8) ep_sc = *reinterpret_cast<const float4*>(p.wscale + ep_n);
  }
#pragma unroll
  for (int e = 0; e < EPN; ++e) {
    const int mb = wave + 4 * e;
    ep_act[e] = mb < MB && (!MS || mb0 + mb < MBI); ep_m[e] = (mb0 + mb) * 16 + l15; ep_ok[e] = ep_act[e] && ep_m[e] < M && ep_n < p.N;
    ep_res[e] = make_float4(0.f, 0.f, 0.f, 0.f); ep_slot[e] = 0; ep_pos[e] = 0; s1[e] = 0.f; s2[e] = 0.f; sc0[e] = 0.f;
    if (ep_act[e]) {
      const int mm = ep_m[e] < M ? ep_m[e] : M - 1;
      if (ln) {       // this lane sums a quarter of the row's partials (rows >= M: a clamped duplicate, discarded)
        const float2* row = reinterpret_cast<const float2*>(p.stat_in) + (size_t)mm * (K >> 4);
        const float2* sp = row + (size_t)kq * nq;
        const float c = row[0].x * 0.0625f;
        sc0[e] = c;
        if (PF == 10) {      // K = 1280: the lane's 20 pairs, all requested at once
          ln_partials20(sp, c, s1[e], s2[e]);
        } else {
#pragma unroll 4
          for (int i = 0; i < nq; ++i) { const float2 v = sp[i]; const float dm = v.x * 0.0625f - c; s1[e] += dm; s2[e] += v.y + 16.0f * dm * dm; }
        }
      }
      if (ep_ok[e]) {
        if (p.flags & GV_QKV) { if (ep_n >= p.d) { ep_slot[e] = p.slot[ep_m[e]]; ep_pos[e] = p.pos[ep_m[e]]; } }
        else if (p.flags & GV_RESID) ep_res[e] = *reinterpret_cast<const float4*>(reinterpret_cast<const float*>(p.y) + (size_t)ep_m[e] * p.N + ep_n);
      }
    }
  }
#pragma unroll
  for (int mb = 0; mb < MB; ++mb)
    *reinterpret_cast<float4*>(red + ((size_t)(wave * MB + mb) * 64 + lane) * 4) = make_float4(acc[mb][0], acc[mb][1], acc[mb][2], acc[mb][3]);
  __syncthreads();
  stamp(pf, 3);
  if (KS > 1) {
    // publish this slice's sums (write-through, agent scope: the other slices of the n-tile run on other XCDs), take a ticket; the
    // last arriver re-arms the ticket, drops its stale L1 lines and goes on to add the slices in index order (the order never
    // depends on who arrived last: bit-reproducible) - the hand-off of the cross-attention's ticket form
#pragma unroll
    for (int e = 0; e < EPN; ++e) {
      if (!ep_act[e]) continue;
      const int ep_mb = wave + 4 * e;
      f32x4 s = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int w = 0; w < 4; ++w) {
        const float4 t = *reinterpret_cast<const float4*>(red + ((size_t)(w * MB + ep_mb) * 64 + lane) * 4);
        s[0] += t.x; s[1] += t.y; s[2] += t.z; s[3] += t.w;
      }
      float* dst = p.kpart + ((((size_t)nt * KS + ksi) * MB + ep_mb) * 64 + lane) * 4;
      asm volatile("global_store_dwordx4 %0, %1, off sc1" :: "v"(dst), "v"(s) : "memory");
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __shared__ int s_last;
    __syncthreads();
    if (tid == 0) {
      const unsigned prev = __hip_atomic_fetch_add(p.kcnt + nt, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      const int last = prev == (unsigned)(KS - 1);
      if (last) {
        __hip_atomic_store(p.kcnt + nt, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
      }
      s_last = last;
    }
    __syncthreads();
    stamp(pf, 4);
    if (!s_last) return;
  }
#pragma unroll
  for (int e = 0; e < EPN; ++e) {
    if (!ep_act[e]) { if (e == EPN - 1) stamp(pf, 5); continue; }                                   // whole waves: a row block belongs to one wave
    const int ep_mb = wave + 4 * e;
    float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
    if (KS > 1) {
      for (int k = 0; k < KS; ++k) {
        const float4 t = *reinterpret_cast<const float4*>(p.kpart + ((((size_t)nt * KS + k) * MB + ep_mb) * 64 + lane) * 4);
        s.x += t.x; s.y += t.y; s.z += t.z; s.w += t.w;
      }
    } else {
#pragma unroll
      for (int w = 0; w < 4; ++w) {
        const float4 t = *reinterpret_cast<const float4*>(red + ((size_t)(w * MB + ep_mb) * 64 + lane) * 4);
        s.x += t.x; s.y += t.y; s.z += t.z; s.w += t.w;
      }
    }
    if (W8) { s.x *= ep_sc.x; s.y *= ep_sc.y; s.z *= ep_sc.z; s.w *= ep_sc.w; }
    if (ln) {     // the four lanes of a row (kq = 0..3) hold a quarter of its sums each: ((q0 + q1) + (q2 + q3)) on every lane
      float t1 = s1[e], t2 = s2[e];
      t1 += __shfl_xor(t1, 16); t2 += __shfl_xor(t2, 16);
      t1 += __shfl_xor(t1, 32); t2 += __shfl_xor(t2, 32);
      const float invK = 1.0f / (float)K;
      const float dmu = t1 * 16.0f * invK, mu = sc0[e] + dmu;      // K / 16 tiles
      const float rs = 1.0f / sqrtf(fmaxf(t2 * invK - dmu * dmu, 0.f) + 1e-5f);
      s.x = rs * (s.x - mu * ep_cs.x); s.y = rs * (s.y - mu * ep_cs.y); s.z = rs * (s.z - mu * ep_cs.z); s.w = rs * (s.w - mu * ep_cs.w);
    }
    s.x += ep_bias.x; s.y += ep_bias.y; s.z += ep_bias.z; s.w += ep_bias.w;
    const int m = ep_m[e], n = ep_n;
    if (p.flags & GV_QKV) {
      if (ep_ok[e]) {
        const int d = p.d;
        if (n < d) {
          *reinterpret_cast<float4*>(p.q + (size_t)m * d + n) = s;
        } else {
          const bool isk = n < 2 * d;
          f16* dst = (isk ? p.kc : p.vc) + ((size_t)ep_slot[e] * p.ctx + ep_pos[e]) * d + (n - (isk ? d : 2 * d));
          const f16x4 o = {(f16)s.x, (f16)s.y, (f16)s.z, (f16)s.w};
          *reinterpret_cast<f16x4*>(dst) = o;
        }
      }
      continue;
    }
    if (p.flags & GV_GELU) { s.x = gelu_erf(s.x); s.y = gelu_erf(s.y); s.z = gelu_erf(s.z); s.w = gelu_erf(s.w); }
    if (p.flags & GV_RESID) {
      const float4 r = make_float4(ep_res[e].x + s.x, ep_res[e].y + s.y, ep_res[e].z + s.z, ep_res[e].w + s.w);
      float t1 = 0.f, t2 = 0.f;
      if (ep_ok[e]) {
        *reinterpret_cast<float4*>(reinterpret_cast<float*>(p.y) + (size_t)m * p.N + n) = r;
        if (p.y_xf) { const f16x4 h = {(f16)r.x, (f16)r.y, (f16)r.z, (f16)r.w}; *reinterpret_cast<f16x4*>(p.y_xf + xf_index(m, n, p.ymb)) = h; }
        t1 = (r.x + r.y) + (r.z + r.w);
      }
      if (p.stat_out) {      // partials of this workgroup's 16 columns of row m: (sum, M2 about the tile mean); all four kq lanes take part in the shuffles
        t1 += __shfl_xor(t1, 16);
        t1 += __shfl_xor(t1, 32);
        if (ep_ok[e]) { const float ml = t1 * 0.0625f, a_ = r.x - ml, b_ = r.y - ml, c_ = r.z - ml, e_ = r.w - ml; t2 = (a_ * a_ + b_ * b_) + (c_ * c_ + e_ * e_); }
        t2 += __shfl_xor(t2, 16);
        t2 += __shfl_xor(t2, 32);
        if (kq == 0 && m < M && 16 * nt < p.N) *reinterpret_cast<float2*>(p.stat_out + ((size_t)m * (p.N >> 4) + nt) * 2) = make_float2(t1, t2);
      }
      continue;
    }
    if (!ep_ok[e]) continue;
    if (p.flags & GV_OUT_F32) {
      *reinterpret_cast<float4*>(reinterpret_cast<float*>(p.y) + (size_t)m * p.N + n) = s;
    } else {
      const f16x4 h = {(f16)s.x, (f16)s.y, (f16)s.z, (f16)s.w};
      f16* yo = reinterpret_cast<f16*>(p.y);
      *reinterpret_cast<f16x4*>(yo + (p.ymb ? xf_index(m, n, p.ymb) : (size_t)m * p.N + n)) = h;
    }
  }
  stamp(pf, 6);
}

template <int MB, int PF, bool W8>
__global__ __launch_bounds__(256) void gemv_frag_kernel(const void* l_x, const f16* l_Wp, int l_M, int l_N, int l_K, int l_wks, int l_wk0, int KS, GemvP p) {
  p.x = l_x; p.Wp = l_Wp; p.M = l_M; p.N = l_N; p.K = l_K; p.wks = l_wks; p.wk0 = l_wk0;      // (KS = gridDim.y, passed: the hidden grid-size arguments are a kernarg load too)
  gemv_frag_body<MB, PF, W8>(p, blockIdx.x, KS, blockIdx.y);
}
template <int MB, int PF, bool W8>      // the M-split form: grid (n-tiles, 1, row-block groups), MB row blocks per workgroup of an image of mbi
__global__ __launch_bounds__(256) void gemv_frag_ms_kernel(const void* l_x, const f16* l_Wp, int l_M, int l_N, int l_K, int l_wks, int l_wk0, int mbi, GemvP p) {
  p.x = l_x; p.Wp = l_Wp; p.M = l_M; p.N = l_N; p.K = l_K; p.wks = l_wks; p.wk0 = l_wk0; p.mbi = mbi; p.mb0 = blockIdx.z * MB;
  gemv_frag_body<MB, PF, W8, true>(p, blockIdx.x, 1, 0);
}
// Up to three skinny GEMMs of one row count in ONE launch (f16 weights, no K split): workgroups [0, n0) run problem 0, the next n1
// problem 1, the rest problem 2 - a dependent stage less per decoder layer at 9-96 rows (model.hip dec_forward_frag): the self-attention
// output projection together with the two halves of the cross-attention query folded THROUGH it (q_raw = W'q x0 + (W'q Wo) a + W'q bo:
// one half reads the layer input's fragment image, the other the attention output's; the cross-attention kernel adds the halves and
// applies the LayerNorm statistics of the rows the out-projection produces in this same launch).
struct GemvP3 { GemvP p[3]; int n0, n1; };
// (r6: what a workgroup's first requests need - which problem it is, that problem's activation and weight bases, the common shape and the k-step window -
// leads the argument list as 14 dwords of scalars, so the command processor preloads it into SGPRs (build.py: -amdgpu-kernarg-preload-count); the by-value
// struct alone had a preload length of 0: every workgroup began with a kernarg fetch)
template <int MB, int PF>
__global__ __launch_bounds__(256) void gemv_frag3_kernel(int n0, int n1, const void* x0, const void* x1, const void* x2, const f16* w0, const f16* w1, const f16* w2, GemvP3 ps) {
  const int b = blockIdx.x;
  const int sel = b < n0 ? 0 : (b < n0 + n1 ? 1 : 2);
  const int nt = sel == 0 ? b : (sel == 1 ? b - n0 : b - n0 - n1);
  GemvP p = ps.p[sel];
  p.x = sel == 0 ? x0 : (sel == 1 ? x1 : x2);
  p.Wp = sel == 0 ? w0 : (sel == 1 ? w1 : w2);
  gemv_frag_body<MB, PF, false>(p, nt, 1, 0);
}

// The same skinny GEMM with TWO n-tiles (32 output columns) per workgroup, for the LayerNorm-folded projections that have more
// n-tiles than the chip has CUs (FFN1: 320, vocabulary: 3242): a workgroup's ingest is its weight panel PLUS the whole activation
// image (41 + 123 KB at 8 utterances), a CU takes in ~55 GB/s, and with 320 one-tile workgroups 64 CUs get two of them - the
// kernel's time is those CUs' 328 KB.  Two tiles per workgroup: 160 workgroups x (82 + 123) KB, one round.  Every activation
// fragment feeds two MFMAs.  No residual form, no K split (those projections have 80 n-tiles).
template <int MB, int PF, bool W8>
__global__ __launch_bounds__(256) void gemv_frag2_kernel(WIS_GV_LEAD_DECL(l_), GemvP p) {
  WIS_GV_LEAD_APPLY(p, l_);
  typedef typename WFrag<W8>::T WT;
  constexpr int EPN = (MB + 3) / 4;
  __shared__ __attribute__((aligned(16))) float red[4 * MB * 2 * 64 * 4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nt0 = 2 * blockIdx.x;
  const int M = p.M, K = p.K, ksteps = K >> 5, S = ksteps >> 2;
  const WT* wq0 = reinterpret_cast<const WT*>(p.Wp) + ((size_t)nt0 * ksteps + (size_t)wave * S) * 64 + lane;
  const WT* wq1 = wq0 + (size_t)ksteps * 64;
  const u32x4* xq = reinterpret_cast<const u32x4*>(p.x) + (size_t)wave * S * MB * 64 + lane;
  unsigned long long* pf = (blockIdx.x == 0 && tid == 0) ? p.prof : nullptr;      // (phase stamps as in gemv_frag_body; tap builds only)
  stamp(pf, 0);
  WT a0[PF], a1[PF]; u32x4 b[PF][MB];
#pragma unroll
  for (int u = 0; u < PF; ++u) {
    if (u < S) {
      a0[u] = __builtin_nontemporal_load(wq0 + (size_t)u * 64);
      a1[u] = __builtin_nontemporal_load(wq1 + (size_t)u * 64);
#pragma unroll
      for (int mb = 0; mb < MB; ++mb) b[u][mb] = xq[(size_t)(u * MB + mb) * 64];
    }
  }
  stamp(pf, 1);
  f32x4 acc[MB][2];
#pragma unroll
  for (int mb = 0; mb < MB; ++mb) { acc[mb][0] = f32x4{0.f, 0.f, 0.f, 0.f}; acc[mb][1] = f32x4{0.f, 0.f, 0.f, 0.f}; }
  for (int base = 0; base < S; base += PF) {
#pragma unroll
    for (int u = 0; u < PF; ++u) {
      if (base + u < S) {
        const f16x8 av0 = WFrag<W8>::cvt(a0[u]), av1 = WFrag<W8>::cvt(a1[u]);
#pragma unroll
        for (int mb = 0; mb < MB; ++mb) {
          const f16x8 xb = *reinterpret_cast<const f16x8*>(&b[u][mb]);
          acc[mb][0] = __builtin_amdgcn_mfma_f32_16x16x32_f16(av0, xb, acc[mb][0], 0, 0, 0);
          acc[mb][1] = __builtin_amdgcn_mfma_f32_16x16x32_f16(av1, xb, acc[mb][1], 0, 0, 0);
        }
        const int nx = base + u + PF;
        if (nx < S) {
          a0[u] = __builtin_nontemporal_load(wq0 + (size_t)nx * 64);
          a1[u] = __builtin_nontemporal_load(wq1 + (size_t)nx * 64);
#pragma unroll
          for (int mb = 0; mb < MB; ++mb) b[u][mb] = xq[(size_t)(nx * MB + mb) * 64];
        }
      }
    }
  }
  stamp(pf, 2);
  // epilogue operands (requested behind the whole stream, covered by the reduction barrier): per n-tile the bias / column sums /
  // row scales, per owned row block the LayerNorm statistics (one pass about the first tile's mean, as in gemv_frag_kernel)
  const int l15 = lane & 15, kq = lane >> 4;
  const int nq = K >> 6;
  float4 ep_bias[2], ep_cs[2], ep_sc[2];
  int ep_n[2];
#pragma unroll
  for (int nb = 0; nb < 2; ++nb) {
    ep_n[nb] = 16 * (nt0 + nb) + 4 * kq;
    ep_bias[nb] = make_float4(0.f, 0.f, 0.f, 0.f); ep_cs[nb] = ep_bias[nb]; ep_sc[nb] = make_float4(1.f, 1.f, 1.f, 1.f);
    if (ep_n[nb] < p.N) {
      if (p.bias) ep_bias[nb] = *reinterpret_cast<const float4*>(p.bias + ep_n[nb]);
      ep_cs[nb] = *reinterpret_cast<const float4*>(p.csum + ep_n[nb]);
      if (W8) ep_sc[nb] = *reinterpret_cast<const float4*>(p.wscale + ep_n[nb]);
    }
  }
  bool ep_act[EPN]; int ep_m[EPN], ep_slot[EPN], ep_pos[EPN]; float s1[EPN], s2[EPN], sc0[EPN];
#pragma unroll
  for (int e = 0; e < EPN; ++e) {
    const int mb = wave + 4 * e;
    ep_act[e] = mb < MB; ep_m[e] = mb * 16 + l15; ep_slot[e] = 0; ep_pos[e] = 0; s1[e] = 0.f; s2[e] = 0.f; sc0[e] = 0.f;
    if (ep_act[e]) {
      const int mm = ep_m[e] < M ? ep_m[e] : M - 1;
      const float2* row = reinterpret_cast<const float2*>(p.stat_in) + (size_t)mm * (K >> 4);
      const float2* sp = row + (size_t)kq * nq;
      const float c = row[0].x * 0.0625f;
      sc0[e] = c;
      if (nq == 20) ln_partials20(sp, c, s1[e], s2[e]);      // (uniform: K = 1280)
      else {
#pragma unroll 4
        for (int i = 0; i < nq; ++i) { const float2 v = sp[i]; const float dm = v.x * 0.0625f - c; s1[e] += dm; s2[e] += v.y + 16.0f * dm * dm; }
      }
      if ((p.flags & GV_QKV) && ep_m[e] < M) { ep_slot[e] = p.slot[ep_m[e]]; ep_pos[e] = p.pos[ep_m[e]]; }
    }
  }
#pragma unroll
  for (int mb = 0; mb < MB; ++mb)
#pragma unroll
    for (int nb = 0; nb < 2; ++nb)
      *reinterpret_cast<float4*>(red + ((size_t)((wave * MB + mb) * 2 + nb) * 64 + lane) * 4) = make_float4(acc[mb][nb][0], acc[mb][nb][1], acc[mb][nb][2], acc[mb][nb][3]);
  __syncthreads();
  stamp(pf, 3);
  stamp(pf, 4);
#pragma unroll
  for (int e = 0; e < EPN; ++e) {
    if (!ep_act[e]) continue;                                   // whole waves: a row block belongs to one wave
    const int ep_mb = wave + 4 * e, m = ep_m[e];
    float t1 = s1[e], t2 = s2[e];
    t1 += __shfl_xor(t1, 16); t2 += __shfl_xor(t2, 16);
    t1 += __shfl_xor(t1, 32); t2 += __shfl_xor(t2, 32);
    const float invK = 1.0f / (float)K;
    const float dmu = t1 * 16.0f * invK, mu = sc0[e] + dmu;
    const float rs = 1.0f / sqrtf(fmaxf(t2 * invK - dmu * dmu, 0.f) + 1e-5f);
#pragma unroll
    for (int nb = 0; nb < 2; ++nb) {
      float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
      for (int w = 0; w < 4; ++w) {
        const float4 t = *reinterpret_cast<const float4*>(red + ((size_t)((w * MB + ep_mb) * 2 + nb) * 64 + lane) * 4);
        s.x += t.x; s.y += t.y; s.z += t.z; s.w += t.w;
      }
      if (W8) { s.x *= ep_sc[nb].x; s.y *= ep_sc[nb].y; s.z *= ep_sc[nb].z; s.w *= ep_sc[nb].w; }
      s.x = rs * (s.x - mu * ep_cs[nb].x) + ep_bias[nb].x; s.y = rs * (s.y - mu * ep_cs[nb].y) + ep_bias[nb].y;
      s.z = rs * (s.z - mu * ep_cs[nb].z) + ep_bias[nb].z; s.w = rs * (s.w - mu * ep_cs[nb].w) + ep_bias[nb].w;
      const int n = ep_n[nb];
      if (m >= M || n >= p.N) continue;
      if (p.flags & GV_QKV) {
        const int d = p.d;
        if (n < d) {
          *reinterpret_cast<float4*>(p.q + (size_t)m * d + n) = s;
        } else {
          const bool isk = n < 2 * d;
          f16* dst = (isk ? p.kc : p.vc) + ((size_t)ep_slot[e] * p.ctx + ep_pos[e]) * d + (n - (isk ? d : 2 * d));
          const f16x4 o = {(f16)s.x, (f16)s.y, (f16)s.z, (f16)s.w};
          *reinterpret_cast<f16x4*>(dst) = o;
        }
        continue;
      }
      if (p.flags & GV_GELU) { s.x = gelu_erf(s.x); s.y = gelu_erf(s.y); s.z = gelu_erf(s.z); s.w = gelu_erf(s.w); }
      if (p.flags & GV_OUT_F32) {
        *reinterpret_cast<float4*>(reinterpret_cast<float*>(p.y) + (size_t)m * p.N + n) = s;
      } else {
        const f16x4 h = {(f16)s.x, (f16)s.y, (f16)s.z, (f16)s.w};
        f16* yo = reinterpret_cast<f16*>(p.y);
        *reinterpret_cast<f16x4*>(yo + (p.ymb ? xf_index(m, n, p.ymb) : (size_t)m * p.N + n)) = h;
      }
    }
  }
  stamp(pf, 5);
  stamp(pf, 6);
}

int launch_gemv_frag3(hipStream_t st, const GemvP* p, int n) {
  if (n < 2 || n > 3) { set_error("gemv_frag3: %d problems", n); return WIS_E_ARG; }
  GemvP3 ps; memset(&ps, 0, sizeof(ps));
  int nts[3] = {0, 0, 0};
  for (int i = 0; i < n; ++i) {
    const GemvP& g = p[i];
    if (g.M != p[0].M || g.xmb != p[0].xmb || g.K != p[0].K || g.M < 1 || g.M > MAX_ROWS || g.K % 128 || g.N % 16 || g.xmb != cdiv(g.M, 16) || g.wscale || g.ksplit > 1 ||
        (g.flags & (GV_LN | GV_QKV))) { set_error("gemv_frag3: problem %d unsupported (M=%d N=%d K=%d flags=%d)", i, g.M, g.N, g.K, g.flags); return WIS_E_UNSUPPORTED; }
    ps.p[i] = g; nts[i] = g.N / 16;
  }
  if (n == 2) ps.p[2] = ps.p[1];
  ps.n0 = nts[0]; ps.n1 = nts[1];
  dim3 grid(nts[0] + nts[1] + nts[2]), block(256);
  const bool s10 = p[0].K == 1280;
#define WIS_GF3_ARGS ps.n0, ps.n1, ps.p[0].x, ps.p[1].x, ps.p[2].x, ps.p[0].Wp, ps.p[1].Wp, ps.p[2].Wp, ps
#define WIS_GF3(MBv, PFA, PFB) do { if (s10) hipLaunchKernelGGL((gemv_frag3_kernel<MBv, PFA>), grid, block, 0, st, WIS_GF3_ARGS); else hipLaunchKernelGGL((gemv_frag3_kernel<MBv, PFB>), grid, block, 0, st, WIS_GF3_ARGS); } while (0)
  switch (p[0].xmb) {
    case 1: WIS_GF3(1, 10, 8); break;
    case 2: WIS_GF3(2, 10, 8); break;
    case 3: WIS_GF3(3, 10, 8); break;
    case 4: WIS_GF3(4, 6, 6); break;
    case 5: WIS_GF3(5, 6, 6); break;
    case 6: WIS_GF3(6, 6, 6); break;
    default: set_error("gemv_frag3: %d row blocks unsupported", p[0].xmb); return WIS_E_UNSUPPORTED;
  }
#undef WIS_GF3
#undef WIS_GF3_ARGS
  return WIS_OK;
}

int launch_gemv_frag(hipStream_t st, const GemvP& p) {
  if (p.M < 1 || p.M > MAX_ROWS || p.K % 128 || p.N % 4 || p.xmb != cdiv(p.M, 16)) { set_error("gemv_frag: M=%d N=%d K=%d xmb=%d unsupported", p.M, p.N, p.K, p.xmb); return WIS_E_UNSUPPORTED; }
  if ((p.flags & GV_LN) && (!p.csum || !p.stat_in)) { set_error("gemv_frag: the folded LayerNorm needs column sums and row partials"); return WIS_E_ARG; }
  if ((p.flags & GV_RESID) && (p.N % 16)) { set_error("gemv_frag: residual rows need N %% 16 == 0"); return WIS_E_UNSUPPORTED; }
  const int npad = cdiv(p.N, 16) * 16;
  const int ks = p.ksplit > 1 ? p.ksplit : 1;
  if (ks > 1 && (!p.kpart || !p.kcnt || (p.K / 32) % (4 * ks) || (p.flags & GV_LN))) { set_error("gemv_frag: K split %d unsupported (K=%d)", ks, p.K); return WIS_E_UNSUPPORTED; }
  // two n-tiles per workgroup where there are more n-tiles than CUs (LayerNorm-folded projections: FFN1, vocabulary): -1.7 ... -3.5 % of
  // the decode time at 8 / 16 utterances.  ON since round 4 (WIS_FRAG_NB=1 keeps one tile per workgroup: A/B switch).  Round 3 kept it
  // off for a sporadic corruption of its five-row-block instantiation (168 VGPRs: three waves per SIMD) - features 12 and 14 of a tile
  // wrong for a whole row block.  Cause, narrowed down in round 4 (tools/frag2_lab.hip, tools/frag_stress.hip): hipcc's SLP pass had
  // turned the epilogue's f32 arithmetic into packed-f32 VALU instructions (v_pk_add_f32 / v_pk_mul_f32); the
  // LOW halves of those packed results (float4 components x and z = features 12 and 14 of the 4-feature group a lane owns) come
  // out wrong in lanes 48-63 when three such waves share a SIMD - 14-22 of every 40 launches, 10 808 of 96 000 with four launches
  // in flight, on EVERY box the SLP build was run on (round 4 wrote "some chips": its clean runs were of other builds; corrected in
  // round 5); the same source built with -fno-slp-vectorize (scalar v_add / v_fma: same 168 registers, same
  // occupancy) is clean (0 of 240 000 launches), as is any form with two waves per SIMD.  The whole library is therefore compiled
  // without SLP vectorisation (build.py HIP_FLAGS), tools/isa_lint.py fails the build on any MFMA kernel that contains packed-f32
  // arithmetic, and tests/test_gpu_stress.py bit-compares 10^4 launches of every shipped instantiation on four streams with the
  // idle-GPU launch.
  static const int env_nb = getenv("WIS_FRAG_NB") ? atoi(getenv("WIS_FRAG_NB")) : 2;
  if (env_nb == 2 && (p.flags & GV_LN) && !(p.flags & GV_RESID) && ks == 1 && (npad / 16) % 2 == 0 && npad / 16 > 256) {
    dim3 g2(npad / 32), blk(256);
#define WIS_GF2(MBv, PFv) do { if (p.wscale) hipLaunchKernelGGL((gemv_frag2_kernel<MBv, PFv, true>), g2, blk, 0, st, WIS_GV_LEAD(p), p); \
                               else hipLaunchKernelGGL((gemv_frag2_kernel<MBv, PFv, false>), g2, blk, 0, st, WIS_GV_LEAD(p), p); } while (0)
    switch (p.xmb) {
      case 1: WIS_GF2(1, 6); break;
      case 2: WIS_GF2(2, 6); break;
      case 3: WIS_GF2(3, 6); break;
      case 4: WIS_GF2(4, 4); break;
      case 5: WIS_GF2(5, 4); break;
      case 6: WIS_GF2(6, 4); break;
      default: set_error("gemv_frag: %d row blocks unsupported", p.xmb); return WIS_E_UNSUPPORTED;
    }
#undef WIS_GF2
    return WIS_OK;
  }
  // M split (r6): few n-tiles (<= 85: the d x d projections), no K split, 2-6 row blocks in equal groups: (n-tile, group) workgroups of 1 or 2 row blocks
  // (WIS_FRAG_MSPLIT=0: one workgroup per n-tile, A/B switch)
  static const bool env_ms = !(getenv("WIS_FRAG_MSPLIT") && atoi(getenv("WIS_FRAG_MSPLIT")) == 0);
  // ... INSTEAD of a K split where one was asked for (the K = 4d projection, 80 n-tiles: two K slices were 160 workgroups of 80 KB of weights + HALF the
  // image each and a ticket merge; three row-block groups are 240 workgroups of 160 KB + a THIRD of the image, no merge: 1.996 -> 1.936 ms per step at 8 utterances)
  const int ms_groups = p.xmb <= 1 ? 0 : (p.xmb <= 3 ? p.xmb : (p.xmb + 1) / 2);      // groups of one row block up to 48 rows, of two beyond (the last may be ragged)
  if (env_ms && ms_groups && npad / 16 <= 85) {
    dim3 gm(npad / 16, 1, ms_groups), blk(256);
    // (a 20- / 12-deep ring for the K = 5120 streams - 160 KB requested per CU instead of 64 - measured 1.930 / 1.937 vs 1.937 / 1.938 ms per step at 8 utterances
    // and no better at 12 / 16, session r6K: what a CU takes in is capped near 64 GB/s whatever is asked for; the eight-deep ring stays)
    const bool s10m = p.K == 1280;
#define WIS_GFM(MBv) do { \
    if (p.wscale) { if (s10m) hipLaunchKernelGGL((gemv_frag_ms_kernel<MBv, 10, true>), gm, blk, 0, st, p.x, p.Wp, p.M, p.N, p.K, p.wks, p.wk0, p.xmb, p); else hipLaunchKernelGGL((gemv_frag_ms_kernel<MBv, 8, true>), gm, blk, 0, st, p.x, p.Wp, p.M, p.N, p.K, p.wks, p.wk0, p.xmb, p); } \
    else { if (s10m) hipLaunchKernelGGL((gemv_frag_ms_kernel<MBv, 10, false>), gm, blk, 0, st, p.x, p.Wp, p.M, p.N, p.K, p.wks, p.wk0, p.xmb, p); else hipLaunchKernelGGL((gemv_frag_ms_kernel<MBv, 8, false>), gm, blk, 0, st, p.x, p.Wp, p.M, p.N, p.K, p.wks, p.wk0, p.xmb, p); } } while (0)
    if (p.xmb <= 3) WIS_GFM(1); else WIS_GFM(2);
#undef WIS_GFM
    return WIS_OK;
  }
  dim3 grid(npad / 16, ks), block(256);
  const bool s10 = p.K / ks == 1280;     // ten k-steps per wave: the whole stream of a wave is requested up front
  // up to three row blocks: the whole wave stream (ten k-steps) or eight k-steps in flight; four to six row blocks (49-96 rows):
  // a six-deep ring, so that weight + activation fragments stay inside the register file ((MB + 1) x 4 VGPRs per k-step)
#define WIS_GF(MBv, PFA, PFB) do { \
    if (p.wscale) { if (s10) hipLaunchKernelGGL((gemv_frag_kernel<MBv, PFA, true>), grid, block, 0, st, p.x, p.Wp, p.M, p.N, p.K, p.wks, p.wk0, (int)grid.y, p); else hipLaunchKernelGGL((gemv_frag_kernel<MBv, PFB, true>), grid, block, 0, st, p.x, p.Wp, p.M, p.N, p.K, p.wks, p.wk0, (int)grid.y, p); } \
    else { if (s10) hipLaunchKernelGGL((gemv_frag_kernel<MBv, PFA, false>), grid, block, 0, st, p.x, p.Wp, p.M, p.N, p.K, p.wks, p.wk0, (int)grid.y, p); else hipLaunchKernelGGL((gemv_frag_kernel<MBv, PFB, false>), grid, block, 0, st, p.x, p.Wp, p.M, p.N, p.K, p.wks, p.wk0, (int)grid.y, p); } } while (0)
  // (a twelve-deep ring for the K = 4d slices at 33-48 rows, 218 VGPRs: 2.138 vs 2.134 ms per step at 8 utterances - that kernel is bound by
  // its activation fragments from L2, not by bytes in flight; the one-utterance FFN2, bound by exactly that, takes launch_gemv's SC = 40 form)
  switch (p.xmb) {
    case 1: WIS_GF(1, 10, 8); break;
    case 2: WIS_GF(2, 10, 8); break;
    case 3: WIS_GF(3, 10, 8); break;
    case 4: WIS_GF(4, 6, 6); break;
    case 5: WIS_GF(5, 6, 6); break;
    case 6: WIS_GF(6, 6, 6); break;
    default: set_error("gemv_frag: %d row blocks unsupported", p.xmb); return WIS_E_UNSUPPORTED;
  }
#undef WIS_GF
  return WIS_OK;
}

// rows (fp32 or f16, row-major) -> fragment image + per-16-column partial sums.  grid M, block 256: a thread owns 4 consecutive
// columns; the partials of a 16-column tile are the sums over 4 adjacent threads, in the same (a+b)+(c+d) order everywhere.
__device__ __forceinline__ void xf_emit4(float4 v, int m, int col, f16* xf, float* stat, int K, int MB) {
  if (xf) { const f16x4 h = {(f16)v.x, (f16)v.y, (f16)v.z, (f16)v.w}; *reinterpret_cast<f16x4*>(xf + xf_index(m, col, MB)) = h; }
  if (stat) {      // (sum, M2 about the tile mean) of the 16-column tile: the pair format gemv_frag_kernel merges
    float t1 = (v.x + v.y) + (v.z + v.w);
    t1 += dpp_f<0xB1>(t1);       // quad: lanes 4j .. 4j+3 = the four column quads of one 16-column tile
    t1 += dpp_f<0x4E>(t1);
    const float ml = t1 * 0.0625f, a = v.x - ml, b = v.y - ml, c = v.z - ml, e = v.w - ml;
    float t2 = (a * a + b * b) + (c * c + e * e);
    t2 += dpp_f<0xB1>(t2);
    t2 += dpp_f<0x4E>(t2);
    if ((threadIdx.x & 3) == 0) *reinterpret_cast<float2*>(stat + ((size_t)m * (K >> 4) + (col >> 4)) * 2) = make_float2(t1, t2);
  }
}
__global__ __launch_bounds__(256) void xf_pack_kernel(const void* __restrict__ x, int x_f16, f16* __restrict__ xf, float* __restrict__ stat, int K, int MB) {
  const int m = blockIdx.x;
  for (int c4 = threadIdx.x; c4 < (K >> 2); c4 += 256) {     // K % 16 == 0: whole quads of threads stay together
    float4 v;
    if (x_f16) { const f16x4 h = *reinterpret_cast<const f16x4*>(reinterpret_cast<const f16*>(x) + (size_t)m * K + 4 * c4); v = make_float4((float)h[0], (float)h[1], (float)h[2], (float)h[3]); }
    else v = *reinterpret_cast<const float4*>(reinterpret_cast<const float*>(x) + (size_t)m * K + 4 * c4);
    xf_emit4(v, m, 4 * c4, xf, stat, K, MB);
  }
}
int launch_xf_pack(hipStream_t st, const void* x, int x_f16, f16* xf, float* stat, int M, int K, int MB) {
  if (K % 16 || MB < cdiv(M, 16)) { set_error("xf_pack: K=%d MB=%d unsupported", K, MB); return WIS_E_UNSUPPORTED; }
  hipLaunchKernelGGL(xf_pack_kernel, dim3(M), dim3(256), 0, st, x, x_f16, xf, stat, K, MB);
  return WIS_OK;
}
__global__ __launch_bounds__(256) void dec_embed_xf_kernel(const f16* __restrict__ emb, const f16* __restrict__ pos_emb, const int* __restrict__ tok,
                                                           const int* __restrict__ pos, float* __restrict__ x, f16* __restrict__ xf, float* __restrict__ stat, int d, int MB) {
  const int m = blockIdx.x;
  const f16* e = emb + (size_t)tok[m] * d;
  const f16* pe = pos_emb + (size_t)pos[m] * d;
  for (int c4 = threadIdx.x; c4 < (d >> 2); c4 += 256) {
    const f16x4 a = *reinterpret_cast<const f16x4*>(e + 4 * c4), b = *reinterpret_cast<const f16x4*>(pe + 4 * c4);
    const float4 v = make_float4((float)a[0] + (float)b[0], (float)a[1] + (float)b[1], (float)a[2] + (float)b[2], (float)a[3] + (float)b[3]);
    *reinterpret_cast<float4*>(x + (size_t)m * d + 4 * c4) = v;
    xf_emit4(v, m, 4 * c4, xf, stat, d, MB);
  }
}
int launch_dec_embed_xf(hipStream_t st, const f16* emb, const f16* pos_emb, const int* tok, const int* pos, float* x, f16* xf, float* stat, int M, int d, int MB) {
  hipLaunchKernelGGL(dec_embed_xf_kernel, dim3(M), dim3(256), 0, st, emb, pos_emb, tok, pos, x, xf, stat, d, MB);
  return WIS_OK;
}

// =======================================================================================
// x[m] = E[tok[m]] + pos_emb[pos[m]]   (no embedding scale; learned positions) -> fp32
__global__ void dec_embed_kernel(const f16* __restrict__ emb, const f16* __restrict__ pos_emb, const int* __restrict__ tok,
                                 const int* __restrict__ pos, float* __restrict__ x, f16* __restrict__ xh, int d) {
  const int m = blockIdx.x;
  const f16* e = emb + (size_t)tok[m] * d;
  const f16* pe = pos_emb + (size_t)pos[m] * d;
  for (int i = threadIdx.x; i < d; i += blockDim.x) {
    const float v = (float)e[i] + (float)pe[i];
    x[(size_t)m * d + i] = v;
    if (xh) xh[(size_t)m * d + i] = (f16)v;          // f16 copy of the layer input (fused out-proj + cross-Q stage)
  }
}
int launch_dec_embed(hipStream_t st, const f16* emb, const f16* pos_emb, const int* tok, const int* pos, float* x, int M, int d, f16* xh) {
  hipLaunchKernelGGL(dec_embed_kernel, dim3(M), dim3(256), 0, st, emb, pos_emb, tok, pos, x, xh, d);
  return WIS_OK;
}

// =======================================================================================
// causal self-attention of one new token per row over its cached history.  grid (M, H), block 64.
// lane = (pl = position slot 0..7, c = 16-byte chunk 0..7 of the 64-wide head): one wave instruction moves 8 cache
// rows x 128 B; K and V of the first 64 positions are all issued up front (one round trip), the 8-lane dot
// products and the position reductions are DPP ops, longer histories continue with an online softmax.
// Logical slot of row m = (m / rpu) * sstride + (m % rpu) * rmul (decode rows own their slot, prefill rows share
// the utterance's first slot).
// (argument order: everything the first round of loads needs - q, the caches, the row table, the shape - sits in the first 14
// dwords, which -amdgpu-kernarg-preload-count delivers in SGPRs at wave launch; `out` and the taps are only read at the end)
// TREE (draft verification of a beam search, model.hip verify_beam_draft): the rows of the pass are nodes of a beam tree - row m's history is not
// one slot but a path: positions < w0 in slot anc[m * aw], position w0 + t in slot anc[m * aw + t] (each node's K / V sits in the slot of the beam
// that produced it).  One dependent load more than the plain form, on a path that runs once per 16 steps.
// NB (r6): 8-position blocks requested up front and per pass of the loop: 8 (64 positions), or 2 / 4 when the caller KNOWS the histories are short (model.hip picks the
// step graph by the step index: every row of a decode pass has the same length) - the kernel always asks for 8 NB positions of K and V per (row, head), whatever the
// length (the addresses must not wait for it), so at 8 utterances its 800 waves put 13 600 wave requests through the CUs' address paths for histories of ~20 positions;
// any NB is correct for any length (the loop goes on in steps of 8 NB positions)
template <bool TREE, int NB>
__global__ __launch_bounds__(64) void dec_self_attn_kernel(const float* __restrict__ q, const f16* __restrict__ kc, const f16* __restrict__ vc,
                                                           const int* __restrict__ pos, int d, int ctx, int rpu, int sstride, int rmul,
                                                           f16* __restrict__ out, unsigned long long* prof, int out_mb,
                                                           const int* __restrict__ anc, int w0, int aw, const int* __restrict__ base) {
  __shared__ float red[4][64];
  const int m = blockIdx.x, h = blockIdx.y, lane = threadIdx.x, pl = lane >> 3, c = lane & 7;
  unsigned long long* pf = (m == 0 && h == 0 && lane == 0) ? prof : nullptr;
  if (lane == 0) tl_begin(prof);
  stamp(pf, 0);
  // the row's history lives in ITS OWN slot (kv_reorder_kernel made it so after the last beam step): the K / V addresses of the
  // first 64 positions depend on nothing that has to be loaded, so q, the row's length and all of K and V travel in ONE round
  // trip (positions >= len are fetched from valid memory and masked below)
  // (TREE: positions before the window live in slot base[m] - or, without a base table, in the slot of the row's window-step-0 ancestor)
  const int ls = TREE ? (base ? base[m] : anc[(size_t)m * aw]) : (m / rpu) * sstride + (m % rpu) * rmul;
  const int len = pos[m] + 1;
  // slot that holds position p of this row's history
  auto slot_of = [&](int p) -> int {
    if (!TREE) return ls;
    int t = p - w0; t = t < aw - 1 ? t : aw - 1;
    return t < 0 ? ls : anc[(size_t)m * aw + t];
  };
  const float4 q0 = *reinterpret_cast<const float4*>(q + (size_t)m * d + h * 64 + 8 * c);
  const float4 q1 = *reinterpret_cast<const float4*>(q + (size_t)m * d + h * 64 + 8 * c + 4);
  const float qv[8] = {q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, q1.z, q1.w};
  const int hoff = h * 64 + 8 * c;
  const f16* krow = kc + (size_t)ls * ctx * d + hoff;
  const f16* vrow = vc + (size_t)ls * ctx * d + hoff;
  u32x4 kr[NB], vr[NB];
  if (!TREE) {
#pragma unroll
    for (int i = 0; i < NB; ++i) kr[i] = *reinterpret_cast<const u32x4*>(krow + (size_t)(8 * i + pl) * d);      // ctx >= 64: in bounds
#pragma unroll
    for (int i = 0; i < NB; ++i) vr[i] = *reinterpret_cast<const u32x4*>(vrow + (size_t)(8 * i + pl) * d);
  } else {
    int sl[NB];
#pragma unroll
    for (int i = 0; i < NB; ++i) sl[i] = slot_of(8 * i + pl);
#pragma unroll
    for (int i = 0; i < NB; ++i) kr[i] = *reinterpret_cast<const u32x4*>(kc + ((size_t)sl[i] * ctx + 8 * i + pl) * d + hoff);
#pragma unroll
    for (int i = 0; i < NB; ++i) vr[i] = *reinterpret_cast<const u32x4*>(vc + ((size_t)sl[i] * ctx + 8 * i + pl) * d + hoff);
  }
  stamp(pf, 1);
  float m_run = -INFINITY, l_run = 0.f;
  float acc[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) acc[j] = 0.f;
  // (do-while: a `for (p0 = 0; p0 < len; ...)` head makes hipcc wait for the row length - a scalar load, one full round trip -
  // BEFORE it issues the q / K / V loads above; the first block is unconditional, len >= 1)
  int p0 = 0;
  do {
    if (p0 > 0) {   // histories beyond 8 NB positions: next block (not prefetched).  Unconditional loads from a clamped position (masked
                    // below): guarded per position, hipcc serialised the sixteen loads into eight wait-for-the-last-pair round trips
#pragma unroll
      for (int i = 0; i < NB; ++i) {
        const int p = p0 + 8 * i + pl, pc = p < len ? p : len - 1;
        if (!TREE) {
          kr[i] = *reinterpret_cast<const u32x4*>(krow + (size_t)pc * d);
          vr[i] = *reinterpret_cast<const u32x4*>(vrow + (size_t)pc * d);
        } else {
          const int sl = slot_of(pc);
          kr[i] = *reinterpret_cast<const u32x4*>(kc + ((size_t)sl * ctx + pc) * d + hoff);
          vr[i] = *reinterpret_cast<const u32x4*>(vc + ((size_t)sl * ctx + pc) * d + hoff);
        }
      }
    }
    float sc[NB]; float mx = -INFINITY;
#pragma unroll
    for (int i = 0; i < NB; ++i) {
      const int p = p0 + 8 * i + pl;
      float dot = 0.f;
      if (p < len) {
        const f16x8 kv = *reinterpret_cast<const f16x8*>(&kr[i]);
#pragma unroll
        for (int j = 0; j < 8; ++j) dot = fmaf((float)kv[j], qv[j], dot);
      }
      dot += dpp_f<0xB1>(dot); dot += dpp_f<0x4E>(dot); dot += dpp_f<0x141>(dot);   // sum over the 8 chunk lanes
      sc[i] = (p < len) ? dot : -INFINITY;
      mx = fmaxf(mx, sc[i]);
    }
    mx = wave_max(mx);
    const float m_new = fmaxf(m_run, mx);
    const float alpha = __expf(m_run - m_new);
    float lsum = 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[j] *= alpha;
#pragma unroll
    for (int i = 0; i < NB; ++i) {
      const float pw = __expf(sc[i] - m_new);     // 0 for masked positions
      lsum += pw;
      if (p0 + 8 * i + pl < len) {
        const f16x8 vv = *reinterpret_cast<const f16x8*>(&vr[i]);
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[j] = fmaf(pw, (float)vv[j], acc[j]);
      }
    }
    l_run = l_run * alpha + wave_sum(lsum) * 0.125f;   // every position is replicated on its 8 chunk lanes
    m_run = m_new;
    p0 += 8 * NB;
  } while (p0 < len);
  stamp(pf, 2);
  // reduce acc over the 8 position slots: xor 8 inside the 16-lane row by DPP, the four rows through LDS
#pragma unroll
  for (int j = 0; j < 8; ++j) acc[j] += dpp_f<0x128>(acc[j]);     // row_ror:8
  if ((lane & 8) == 0) {
#pragma unroll
    for (int j = 0; j < 8; ++j) red[lane >> 4][8 * c + j] = acc[j];
  }
  __syncthreads();
  stamp(pf, 3);
  const float o = (red[0][lane] + red[1][lane]) + (red[2][lane] + red[3][lane]);
  out[out_mb ? xf_index(m, h * 64 + lane, out_mb) : (size_t)m * d + h * 64 + lane] = (f16)(o / l_run);
  stamp(pf, 4);
  if (lane == 0) tl_end(prof);
}
int launch_dec_self_attn(hipStream_t st, const SelfAttnP& p) {
  if (p.ctx > 512 || p.ctx < 64) { set_error("dec_self_attn: ctx=%d outside [64, 512]", p.ctx); return WIS_E_UNSUPPORTED; }
  if (p.plen) {      // the long-prompt route's decode step: rpu rows per utterance, each in a slot of its own behind the shared prefix
    if (p.anc || p.rmul != 1 || p.rpu < 1 || p.M % p.rpu != 0) { set_error("dec_self_attn: a shared prompt prefix takes whole utterances of decode rows (M %d, rpu %d, rmul %d)", p.M, p.rpu, p.rmul); return WIS_E_ARG; }
    return launch_dec_self_attn_long(st, p.q, p.kc, p.vc, p.pos, p.plen, p.M / p.rpu, p.rpu, p.H, p.d, p.ctx, p.sstride, p.out, p.out_mb);
  }
#define WIS_SA(TREEv, NBv) hipLaunchKernelGGL((dec_self_attn_kernel<TREEv, NBv>), dim3(p.M, p.H), dim3(64), 0, st, p.q, p.kc, p.vc, p.pos, p.d, p.ctx, p.rpu, p.sstride, p.rmul, p.out, \
                                              p.prof, p.out_mb, p.anc, p.w0, p.aw, p.base)
  if (p.anc) {
    if (p.aw < 1) { set_error("dec_self_attn: ancestor table of width %d", p.aw); return WIS_E_ARG; }
    WIS_SA(true, 8);
  } else if (p.nb == 2) WIS_SA(false, 2);
  else if (p.nb == 4) WIS_SA(false, 4);
  else WIS_SA(false, 8);
#undef WIS_SA
  return WIS_OK;
}

// =======================================================================================
// The decode step's self-attention behind a LONG prompt (generate.hip, the long-prompt route).  grid (B, H), block 256 = 4 waves: ONE workgroup serves the
// k <= MAX_R live rows (m = b k + j) of utterance b at head h.  The prompt's positions [0, plen[b]) lie in the utterance's first slot b * sstride and nowhere
// else - every K / V chunk of them is loaded ONCE and used against all k queries - and row j's own positions plen[b] .. pos[m] lie in slot b * sstride + j.
// Lane = (pl = position slot 0..7, c = 16-byte chunk 0..7 of the head), as in dec_self_attn_kernel; the history is split over the waves in blocks of 8
// positions: prefix block i of wave w holds positions 32 i + 8 w + pl (8 blocks: plen <= SA_LONG_MAX_PLEN = 256), suffix chunk s holds plen + 32 s + 8 w + pl
// of every row.  A wave issues its 8 + 8 prefix requests - addresses clamped by ctx alone, so they wait for nothing - and the first suffix chunk of all k rows
// (which needs plen: one scalar round trip) before it consumes anything; only rows with more than 32 generated positions go round a loop, one chunk of
// all k rows per pass.  Rows j >= k are skipped (k is a kernel argument: uniform branches).  Every (wave, row) keeps a partial (max, sum, acc[8] per lane = 64 columns over the 8 chunk lanes); the four waves' partials meet in LDS.
// Arithmetic as the plain kernel's: f16 K / V, f32 q, f32 dots and accumulation, __expf, the output rounded to f16 - in another summation order.
// Reads beyond a row's length come from clamped addresses inside the cache (position <= min(ctx - 1, ...) of a slot the row may read) and are masked.
__global__ __launch_bounds__(256) void dec_self_attn_long_kernel(const float* __restrict__ q, const f16* __restrict__ kc, const f16* __restrict__ vc,
                                                                 const int* __restrict__ pos, const int* __restrict__ plen, int d, int ctx, int k, int sstride,
                                                                 f16* __restrict__ out, int out_mb) {
  constexpr int PB = SA_LONG_MAX_PLEN / 32;      // prefix blocks per wave
  __shared__ float red[4][MAX_R][4][64];      // [wave][row][16-lane row of the wave][column]
  __shared__ float red_m[4][MAX_R], red_l[4][MAX_R];
  const int b = blockIdx.x, h = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, pl = lane >> 3, c = lane & 7;
  const int hoff = h * 64 + 8 * c, s0 = b * sstride, m0 = b * k;
  const int wp = 8 * wave + pl;                  // this lane's position inside a 32-position block row
  // ---- requests: prefix K / V (no dependence), the control words, q of every row, the first suffix chunk of every row
  const f16* kbase = kc + (size_t)s0 * ctx * d + hoff;
  const f16* vbase = vc + (size_t)s0 * ctx * d + hoff;
  u32x4 kr[PB], vr[PB];
#pragma unroll
  for (int i = 0; i < PB; ++i) { const int p = 32 * i + wp, pc = p < ctx ? p : ctx - 1; kr[i] = *reinterpret_cast<const u32x4*>(kbase + (size_t)pc * d); }
#pragma unroll
  for (int i = 0; i < PB; ++i) { const int p = 32 * i + wp, pc = p < ctx ? p : ctx - 1; vr[i] = *reinterpret_cast<const u32x4*>(vbase + (size_t)pc * d); }
  const int pn = plen[b];
  int last[MAX_R];                               // last position of row j (pos[m]); rows >= k repeat row k - 1 and are never written
#pragma unroll
  for (int j = 0; j < MAX_R; ++j) last[j] = pos[m0 + (j < k ? j : k - 1)];
  float qv[MAX_R][8];
#pragma unroll
  for (int j = 0; j < MAX_R; ++j) {
    if (j >= k) continue;                        // (uniform: rows beyond the utterance's k cost neither requests nor arithmetic)
    const float* qp = q + (size_t)(m0 + j) * d + hoff;
    const float4 q0 = *reinterpret_cast<const float4*>(qp), q1 = *reinterpret_cast<const float4*>(qp + 4);
    qv[j][0] = q0.x; qv[j][1] = q0.y; qv[j][2] = q0.z; qv[j][3] = q0.w; qv[j][4] = q1.x; qv[j][5] = q1.y; qv[j][6] = q1.z; qv[j][7] = q1.w;
  }
  u32x4 ks[MAX_R], vs[MAX_R];
  int maxlast = 0;
#pragma unroll
  for (int j = 0; j < MAX_R; ++j) {
    if (j >= k) continue;
    const int p = pn + wp, pc = p < last[j] ? (p > 0 ? p : 0) : last[j];      // (a row without a suffix reads its position pos[m] = plen - 1 of its own slot: inside the cache, masked)
    const size_t off = ((size_t)(s0 + j) * ctx + pc) * d + hoff;
    ks[j] = *reinterpret_cast<const u32x4*>(kc + off);
    vs[j] = *reinterpret_cast<const u32x4*>(vc + off);
    maxlast = last[j] > maxlast ? last[j] : maxlast;
  }
  // ---- prefix: every block's scores of row j, one softmax partial per (wave, row)
  float m_run[MAX_R], l_run[MAX_R], acc[MAX_R][8];
#pragma unroll
  for (int j = 0; j < MAX_R; ++j) {
    if (j >= k) continue;
    float sc[PB]; float mx = -INFINITY;
#pragma unroll
    for (int i = 0; i < PB; ++i) {
      const int p = 32 * i + wp;
      const bool ok = p < pn && p <= last[j];
      float dot = 0.f;
      if (ok) {
        const f16x8 kv = *reinterpret_cast<const f16x8*>(&kr[i]);
#pragma unroll
        for (int e = 0; e < 8; ++e) dot = fmaf((float)kv[e], qv[j][e], dot);
      }
      dot += dpp_f<0xB1>(dot); dot += dpp_f<0x4E>(dot); dot += dpp_f<0x141>(dot);   // sum over the 8 chunk lanes
      sc[i] = ok ? dot : -INFINITY;
      mx = fmaxf(mx, sc[i]);
    }
    mx = wave_max(mx);
    const float ms = mx == -INFINITY ? 0.f : mx;      // (a wave whose share of the prompt is empty: every weight 0, no NaN)
    float lsum = 0.f;
#pragma unroll
    for (int e = 0; e < 8; ++e) acc[j][e] = 0.f;
#pragma unroll
    for (int i = 0; i < PB; ++i) {
      const float pw = __expf(sc[i] - ms);            // 0 for masked positions
      lsum += pw;
      if (32 * i + wp < pn && 32 * i + wp <= last[j]) {
        const f16x8 vv = *reinterpret_cast<const f16x8*>(&vr[i]);
#pragma unroll
        for (int e = 0; e < 8; ++e) acc[j][e] = fmaf(pw, (float)vv[e], acc[j][e]);
      }
    }
    m_run[j] = mx; l_run[j] = wave_sum(lsum) * 0.125f;   // every position is replicated on its 8 chunk lanes
  }
  // ---- suffix: one chunk of 32 positions of every row per pass (the first one is already on its way; later ones are requested and consumed in the same
  // pass, not prefetched: requesting chunk c + 1 ahead of consuming chunk c was built - together with the skipped rows it spills to scratch (1160 bytes
  // per lane), without them it keeps 168 AGPRs of spill moves in the loop; measured instead: profiles/prompt_ab.md, the 128-token rows)
  int p0 = pn;
  do {
    if (p0 > pn) {
#pragma unroll
      for (int j = 0; j < MAX_R; ++j) {
        if (j >= k) continue;
        const int p = p0 + wp, pc = p < last[j] ? p : last[j];
        const size_t off = ((size_t)(s0 + j) * ctx + pc) * d + hoff;
        ks[j] = *reinterpret_cast<const u32x4*>(kc + off);
        vs[j] = *reinterpret_cast<const u32x4*>(vc + off);
      }
    }
#pragma unroll
    for (int j = 0; j < MAX_R; ++j) {
      if (j >= k) continue;
      const bool ok = p0 + wp <= last[j];
      float dot = 0.f;
      if (ok) {
        const f16x8 kv = *reinterpret_cast<const f16x8*>(&ks[j]);
#pragma unroll
        for (int e = 0; e < 8; ++e) dot = fmaf((float)kv[e], qv[j][e], dot);
      }
      dot += dpp_f<0xB1>(dot); dot += dpp_f<0x4E>(dot); dot += dpp_f<0x141>(dot);
      const float sc = ok ? dot : -INFINITY;
      const float m_new = fmaxf(m_run[j], wave_max(sc));
      const float ms = m_new == -INFINITY ? 0.f : m_new;
      const float alpha = __expf(m_run[j] - ms), pw = __expf(sc - ms);
#pragma unroll
      for (int e = 0; e < 8; ++e) acc[j][e] *= alpha;
      if (ok) {
        const f16x8 vv = *reinterpret_cast<const f16x8*>(&vs[j]);
#pragma unroll
        for (int e = 0; e < 8; ++e) acc[j][e] = fmaf(pw, (float)vv[e], acc[j][e]);
      }
      l_run[j] = l_run[j] * alpha + wave_sum(pw) * 0.125f;
      m_run[j] = m_new;
    }
    p0 += 32;
  } while (p0 <= maxlast);
  // ---- merge: acc over the wave's 8 position slots (xor 8 inside the 16-lane row by DPP, the four rows through LDS), then the four waves' partials
#pragma unroll
  for (int j = 0; j < MAX_R; ++j) {
    if (j >= k) continue;
#pragma unroll
    for (int e = 0; e < 8; ++e) acc[j][e] += dpp_f<0x128>(acc[j][e]);     // row_ror:8
    if (j < k && (lane & 8) == 0) {
#pragma unroll
      for (int e = 0; e < 8; ++e) red[wave][j][lane >> 4][8 * c + e] = acc[j][e];
    }
    if (j < k && lane == 0) { red_m[wave][j] = m_run[j]; red_l[wave][j] = l_run[j]; }
  }
  __syncthreads();
#pragma unroll
  for (int j2 = 0; j2 < MAX_R / 4; ++j2) {
    const int j = wave + 4 * j2;
    if (j >= k) continue;                // (uniform; no barrier behind this point)
    const float m0_ = red_m[0][j], m1_ = red_m[1][j], m2_ = red_m[2][j], m3_ = red_m[3][j];
    const float M_ = fmaxf(fmaxf(m0_, m1_), fmaxf(m2_, m3_));      // finite: position 0 belongs to every row
    const float w0_ = __expf(m0_ - M_), w1_ = __expf(m1_ - M_), w2_ = __expf(m2_ - M_), w3_ = __expf(m3_ - M_);
    const float L_ = (red_l[0][j] * w0_ + red_l[1][j] * w1_) + (red_l[2][j] * w2_ + red_l[3][j] * w3_);
    float ow[4];
#pragma unroll
    for (int w = 0; w < 4; ++w) ow[w] = (red[w][j][0][lane] + red[w][j][1][lane]) + (red[w][j][2][lane] + red[w][j][3][lane]);
    const float o = (ow[0] * w0_ + ow[1] * w1_) + (ow[2] * w2_ + ow[3] * w3_);
    const int m = m0 + j;
    out[out_mb ? xf_index(m, h * 64 + lane, out_mb) : (size_t)m * d + h * 64 + lane] = (f16)(o / L_);
  }
}
int launch_dec_self_attn_long(hipStream_t st, const float* q, const f16* kc, const f16* vc, const int* pos, const int* plen, int B, int k, int H, int d, int ctx, int sstride,
                              f16* out, int out_mb) {
  if (ctx > 512 || ctx < 64) { set_error("dec_self_attn_long: ctx=%d outside [64, 512]", ctx); return WIS_E_UNSUPPORTED; }
  if (k < 1 || k > MAX_R || sstride < k || d != H * 64 || !plen) { set_error("dec_self_attn_long: %d rows per utterance (1..%d) in %d slots, d = %d at %d heads", k, MAX_R, sstride, d, H); return WIS_E_ARG; }
  hipLaunchKernelGGL(dec_self_attn_long_kernel, dim3(B, H), dim3(256), 0, st, q, kc, vc, pos, plen, d, ctx, k, sstride, out, out_mb);
  return WIS_OK;
}

// =======================================================================================
// cross-attention of the R (<= 16) query rows of one utterance over a chunk of <= 256 encoder keys, on the
// matrix cores.  grid (chunks, H, B), block 256 = 4 waves.
//   scores  S^T[key][r] = K[key][:] . Q[r][:]      v_mfma_f32_16x16x32_f16, A = K (16 keys x 32 dh, 16-byte loads from
//                                                   the [H][dh/8][T][8] image), B = Q^T (registers); wave w owns key tiles w, w+4, ..
//   output  O^T[dh][r]  = V^T[dh][:] . P[r][:]      A = V^T (16 dh x 32 keys, 16-byte loads from the [H][64][Tpad] image),
//                                                   B = P^T (f16 in LDS); wave w owns dh 16w..16w+15
// Q, then every K and V fragment, are issued up front (one memory round trip; vmcnt retires in order, so the tiny Q load
// is first).  No cross-lane shuffles: the MFMA output layout puts a query row on a lane column.  Chunk partials
// (o[64], max, sum) are published with write-through (sc1) relaxed agent-scope stores and combined by the last-arriving
// workgroup with sc1 loads: placement independent, no fences (guide §6 G16).
__device__ __forceinline__ void st_sc1(float* p, float v) {
  __hip_atomic_store(reinterpret_cast<unsigned*>(p), __float_as_uint(v), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ float ld_sc1(const float* p) {
  return __uint_as_float(__hip_atomic_load(reinterpret_cast<const unsigned*>(p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
}
constexpr int CA_PSTR = 264;   // f16 row pitch of the P image (256 keys + 8: 16-byte aligned, bank-skewed)

// TPW = key tiles per wave (CL / 64): 2 for 128-key chunks, 4 for 256-key chunks; loads are unconditional with clamped
// addresses (masked by `kl < n` below), so the issue phase is straight-line code.
// CM = the most chunks the combine handles (its partial buffers are register arrays of that size): 6 for the default 256-key
// chunking, 16 otherwise.  With [16] arrays at every chunking the kernel needed 218 VGPRs - two workgroups per CU, so the 960
// workgroups of an 8-utterance batch ran in two rounds; with CM = 6 it needs 88 (five per CU).
// FOLD: the folded-query prologue (B = 1-sized row counts only; its own instantiation so that the batched kernel keeps its
// register budget).
// SPIN (small grids: B * H <= 192, <= 6 chunks, <= 8 rows): the chunk partials travel as 8-byte {tag, value} GRANULES, one write-through
// store each (guide G16 form R2: "the data is the flag") - a producing workgroup stores and leaves: no drain, no barrier, no ticket.
// The workgroup of the LAST chunk of every (utterance, head) is its combiner: it keeps its own partial in LDS and re-reads the other
// chunks' granules (relaxed agent-scope loads) until every tag equals this launch's epoch, then combines in the fixed chunk order
// (the same arithmetic, in the same order, as the ticket form: bit-identical results).  The epoch of an (utterance, head) is a word
// in device memory that its combiner advances at the end of the launch (launches on a stream are ordered, so the next launch
// reads the new value; tags only grow, so a slot's old contents can never match) - nothing is reset between launches, and graph
// replays stay valid.  Progress: producers never wait; at most B * H <= 192 workgroups spin, fewer than the chip's 256 CUs, so a
// producer always finds a slot.  The spin is bounded: on exhaustion the combiner raises a flag (checked by wis_generate) instead of
// hanging.  What it removes from the hand-off: the store drain, the returning ticket atomic and the agent-scope acquire (1.7 us).

// FOLD: 0 = q is the finished query; 1 = folded query, statistics reduced from the rows themselves (xres = x1 fp32 [B*R][d]: the one-utterance
// step); 2 = folded query of the BATCHED step: q_raw arrives as two halves (q + q2: W'q x0 + W'q bo and (W'q Wo) a, model.hip
// dec_forward_frag) and the statistics come from the per-16-column (sum, M2) partials the out-projection's residual epilogue left
// (xres = [B*R][d/16][2]; merged like gemv_frag_kernel merges them) - 80 pairs per row instead of 1280 floats; 3 = the same with V requested
// up front (small grids: the one-utterance step); 4 (r5) = 2 with the query's operands handed out through LDS AND V up front (see STG below).
template <int TPW, int CM, int FOLD, bool SPIN>
// (argument order as in dec_self_attn_kernel: the first 14 dwords - q, K, V^T, the folded query's rows / second half, the epoch block and
// the packed shape - are preloaded into SGPRs, so the kernel's first round of requests (q, the statistics' rows, the K fragments) does
// not wait for a kernarg fetch; what needs the later arguments - column sums / bias of the folded query, V^T's pitch - is requested behind them)
__global__ __launch_bounds__(256) void dec_cross_attn_kernel(const float* __restrict__ q, const f16* __restrict__ kx, const f16* __restrict__ vt,
                                                             const float* __restrict__ xres, const float* __restrict__ q2, unsigned* epoch, int RHCC, int dT,
                                                             int TpadF, f16* __restrict__ out, float* part, unsigned* counters,
                                                             unsigned long long* prof, int out_mb,
                                                             const float* __restrict__ qcs, const float* __restrict__ qb, gran_t* gran) {
  // rows | heads << 8 | chunk length << 14 | chunks << 24, d | T << 16: six pointers + two words = the 14 preloaded dwords
  const int R = RHCC & 0xFF, H = (RHCC >> 8) & 0x3F, CL = (RHCC >> 14) & 0x3FF, C = (RHCC >> 24) & 0xFF, d = dT & 0xFFFF, T = (dT >> 16) & 0xFFFF;
  __shared__ float ssc[16][257];
  __shared__ __attribute__((aligned(16))) f16 sp16[16 * CA_PSTR];
  __shared__ float smax[16][16];
  __shared__ float ssumw[4][16];
  __shared__ float smx[16], ssum[16];
  __shared__ int s_last;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l15 = lane & 15, kq = lane >> 4;
  const int c = blockIdx.x, h = blockIdx.y, b = blockIdx.z;
  // bit 30 of the V^T pitch argument: the row groups b = 0 .. B-1 are rows of ONE utterance (draft verification: up to 96 tree rows
  // against utterance 0's K / V); queries, outputs, partials and tickets stay per group
  const int Tpad = TpadF & 0x3FFFFFFF, bkv = (TpadF >> 30) ? 0 : b;
  const int klo = c * CL, n = (klo + CL <= T) ? CL : T - klo;   // 1 <= n <= 256, klo % 32 == 0
  // (tap builds: workgroup (0, 0, 0) stamps entries 0-5 of its row, the LAST chunk's workgroup - the combiner of the granule form - entries 7-13)
  unsigned long long* pf = (h == 0 && b == 0 && tid == 0 && prof) ? (c == 0 ? prof : (c == C - 1 ? prof + 7 : nullptr)) : nullptr;
  if (tid == 0) tl_begin(prof);
  stamp(pf, 0);

  // ---- loads: Q (B operand, lane = (row r, k-quarter)), K fragments, V^T fragments
  const int rq = l15 < R ? l15 : R - 1;
  const float* qp = q + (size_t)(b * R + rq) * d + h * 64 + 8 * kq;
  // STG (FOLD 4, the batched fold with everything requested up front): the query rows (both halves), the folded query's column sums and
  // its bias - (2 R + 2) x 64 floats that every wave would fetch for itself into 64 VGPRs, sixteen requests per wave - are fetched once
  // per wave as one 16-byte piece per lane and array (clamped, unconditional) and handed out through LDS behind the prologue's barrier.
  // What that buys is REGISTERS: the operands no longer sit in VGPRs beside the K fragments while the requests are in flight, so the V
  // fragments can be requested up front as well and the kernel still fits four workgroups per CU.
  constexpr bool STG = FOLD == 4;
  float4 qa0_, qa1_, qb0_, qb1_, stq, stq2, stc;
  qa0_ = qa1_ = qb0_ = qb1_ = stq = stq2 = stc = make_float4(0.f, 0.f, 0.f, 0.f);
  if (!STG) {
    qa0_ = *reinterpret_cast<const float4*>(qp); qa1_ = *reinterpret_cast<const float4*>(qp + 4);
    qb0_ = *reinterpret_cast<const float4*>(qp + 32); qb1_ = *reinterpret_cast<const float4*>(qp + 36);
  } else {
    const int sr = (tid >> 4) < R ? (tid >> 4) : R - 1;      // thread t < 16 R owns piece (t & 15) of row t >> 4
    const size_t so = (size_t)(b * R + sr) * d + h * 64 + 4 * (tid & 15);
    stq = *reinterpret_cast<const float4*>(q + so);
    if (q2) stq2 = *reinterpret_cast<const float4*>(q2 + so);      // (uniform)
  }
  unsigned ep_now = 0;
  if (SPIN) ep_now = __hip_atomic_load(epoch + 1 + b * H + h, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);      // requested with everything else (word 0 is the flag)
  // Folded query (model.hip fused_out_cq): `q` holds q_raw = W'x0 + (W'Wo) a + W'bo of the LayerNorm-folded cross-attention query
  // projection, computed one stage early from the layer input and the self-attention output; the LayerNorm statistics belong
  // to the rows the out-projection has produced SINCE (xres = x1, fp32 [B*R][d]).  Every workgroup reduces its utterance's R
  // rows itself (R x d floats from L2, requested together with K and V) and finishes q = rs (q_raw - mu c) + b'.
  // wave w reduces rows w and w + 4 of the utterance (R <= 8): 5 float4 per lane and row cover d <= 1280
  constexpr bool PSTAT = FOLD >= 2;
  constexpr int NXS = FOLD == 1 ? 5 : 1;
  float4 xs4[2][NXS]; float4 cs0, cs1, cs2, cs3, bq0, bq1, bq2, bq3;
  float4 qc0, qc1, qc2, qc3; float2 pt[2][2];
  const int d4 = d >> 2, ntile = d >> 4;
  if (PSTAT) {
    qc0 = qc1 = qc2 = qc3 = make_float4(0.f, 0.f, 0.f, 0.f);
    if (!STG && q2) {      // (uniform: the batched step's second half of q_raw; the one-utterance step's dual launch leaves the whole of it in q)
      const float* qp2 = q2 + (size_t)(b * R + rq) * d + h * 64 + 8 * kq;
      qc0 = *reinterpret_cast<const float4*>(qp2); qc1 = *reinterpret_cast<const float4*>(qp2 + 4); qc2 = *reinterpret_cast<const float4*>(qp2 + 32); qc3 = *reinterpret_cast<const float4*>(qp2 + 36);
    }
#pragma unroll
    for (int j = 0; j < 2; ++j) {      // wave w merges the partials of rows w and w + 4: lane = tile (and tile + 64; d <= 2048)
      const int r = wave + 4 * j;
      const float2* sp = reinterpret_cast<const float2*>(xres) + (size_t)(b * R + (r < R ? r : R - 1)) * ntile;
      pt[j][0] = sp[lane < ntile ? lane : ntile - 1];
      pt[j][1] = sp[lane + 64 < ntile ? lane + 64 : ntile - 1];
    }
  }
  if (FOLD == 1) {
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int r = wave + 4 * j;
      const float4* xr = reinterpret_cast<const float4*>(xres) + (size_t)(b * R + (r < R ? r : R - 1)) * d4;
#pragma unroll
      for (int i = 0; i < NXS; ++i) { const int c4 = lane + 64 * i; xs4[j][i] = xr[c4 < d4 ? c4 : d4 - 1]; }      // unconditional (clamped; masked in the sums): no exec-masked branch between the loads
    }
  }
  // (K fragments: addressed from preloaded arguments only, so they go out before the first wait for a scalar kernarg load)
  const f16* kb = kx + (size_t)(bkv * H + h) * 8 * T * 8;
  u32x4 kf[TPW][2];
#pragma unroll
  for (int i = 0; i < TPW; ++i) {
    int key = klo + 16 * (wave + 4 * i) + l15; if (key > T - 1) key = T - 1;      // clamped; masked below
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) kf[i][ks] = *reinterpret_cast<const u32x4*>(kb + ((size_t)(kq + 4 * ks) * T + key) * 8);
  }
  if (STG) {      // threads 0-15 of every wave: the head's 64 column sums, 16-31: its bias
    stc = *reinterpret_cast<const float4*>(((tid & 16) ? qb : qcs) + h * 64 + 4 * (tid & 15));
  }
  if (FOLD && !STG) {
    const float* cp = qcs + h * 64 + 8 * kq; const float* bp = qb + h * 64 + 8 * kq;
    cs0 = *reinterpret_cast<const float4*>(cp); cs1 = *reinterpret_cast<const float4*>(cp + 4); cs2 = *reinterpret_cast<const float4*>(cp + 32); cs3 = *reinterpret_cast<const float4*>(cp + 36);
    bq0 = *reinterpret_cast<const float4*>(bp); bq1 = *reinterpret_cast<const float4*>(bp + 4); bq2 = *reinterpret_cast<const float4*>(bp + 32); bq3 = *reinterpret_cast<const float4*>(bp + 36);
  }
  constexpr int NSTEP = 2 * TPW;                      // 32-key P.V steps per chunk; V^T is zero padded up to Tpad >= chunks * CL
  const f16* vb = vt + ((size_t)(bkv * H + h) * 64 + 16 * wave + l15) * Tpad + klo + 8 * kq;
  u32x4 vf[NSTEP];
  // (batched fold: the V fragments are requested BEHIND the query prologue - its column sums, biases, second q half and partials
  // are dead by then, so the kernel stays near the 88 registers of the plain form (five workgroups per CU: the 960 workgroups of an
  // 8-utterance batch in one round) instead of 153 (three per CU); V is not needed before the softmax)
  // FOLD 2 / 3: statistics from row partials; 2 requests V BEHIND the prologue (large grids: registers decide how many workgroups a CU
  // holds), 3 with everything else (the one-utterance step's 120 workgroups have CUs to spare)
  constexpr bool VLATE = FOLD == 2;
  if (!VLATE) {
#pragma unroll
    for (int sidx = 0; sidx < NSTEP; ++sidx) vf[sidx] = *reinterpret_cast<const u32x4*>(vb + 32 * sidx);
  }
  stamp(pf, 1);

  float4 qa0 = qa0_, qa1 = qa1_, qb0 = qb0_, qb1 = qb1_;
  if (FOLD) {
    // mean / rstd of the rows: a DPP wave reduction per row (fixed order: bit-reproducible), published through LDS behind a RAW
    // barrier - `__syncthreads()` would first wait for every outstanding load, i.e. for the K / V fragments this prologue is
    // supposed to run in the shadow of (measured with three `__syncthreads()` here: cross-attention 9.0 -> 12.1 us)
    __shared__ float srow[16][2];
    __builtin_amdgcn_sched_barrier(0);      // every load of the kernel is requested above this line: the statistics wait for their rows only
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int r = wave + 4 * j;
      float a1 = 0.f, a2 = 0.f;
      if (PSTAT) {
        // Chan merge of the (sum, M2 about the tile mean) pairs about c0 = the first tile's mean (gemv_frag_kernel's one-pass form):
        //   mu = c0 + mean_t (m_t - c0),   var = (sum_t (M2_t + 16 (m_t - c0)^2)) / d - (mu - c0)^2
        const float c0 = readlane_f(pt[j][0].x, 0) * 0.0625f;
#pragma unroll
        for (int i = 0; i < 2; ++i) {
          const bool in = lane + 64 * i < ntile;
          const float dm = in ? pt[j][i].x * 0.0625f - c0 : 0.f;
          a1 += dm; a2 += in ? pt[j][i].y + 16.0f * dm * dm : 0.f;
        }
        a1 = wave_sum(a1); a2 = wave_sum(a2);
        if (lane == 0 && r < R) { const float invd = 1.0f / (float)d, dmu = a1 * 16.0f * invd; srow[r][0] = c0 + dmu; srow[r][1] = 1.0f / sqrtf(fmaxf(a2 * invd - dmu * dmu, 0.f) + 1e-5f); }
      } else {
      // ONE pass, shifted by the row's first element: no E[x^2] - mu^2 cancellation for rows with a large common offset, and both
      // wave reductions issue together (a second pass over the registers about the exact mean measured +2.3 us per launch)
      const float c0 = readlane_f(xs4[j][0].x, 0);
#pragma unroll
      for (int i = 0; i < NXS; ++i) {
        const float4 v = xs4[j][i];
        const bool in = lane + 64 * i < d4;
        const float a = in ? v.x - c0 : 0.f, b = in ? v.y - c0 : 0.f, c = in ? v.z - c0 : 0.f, e = in ? v.w - c0 : 0.f;
        a1 += (a + b) + (c + e); a2 += (a * a + b * b) + (c * c + e * e);
      }
      a1 = wave_sum(a1); a2 = wave_sum(a2);
      if (lane == 0 && r < R) { const float ms = a1 / (float)d; srow[r][0] = c0 + ms; srow[r][1] = 1.0f / sqrtf(fmaxf(a2 / (float)d - ms * ms, 0.f) + 1e-5f); }
      }
    }
    constexpr int SQP = 68;      // row pitch of the staged operands (floats): 16-byte aligned, rows four banks apart
    __shared__ __attribute__((aligned(16))) float sq[STG ? 10 * SQP : 4];      // rows 0..7: q_raw (both halves added), 8: column sums, 9: bias
    if (STG) {
      if (tid < 16 * R) *reinterpret_cast<float4*>(&sq[(tid >> 4) * SQP + 4 * (tid & 15)]) = make_float4(stq.x + stq2.x, stq.y + stq2.y, stq.z + stq2.z, stq.w + stq2.w);
      if (tid < 32) *reinterpret_cast<float4*>(&sq[(8 + (tid >> 4)) * SQP + 4 * (tid & 15)]) = stc;
    }
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
    const float mu = srow[rq][0], rs = srow[rq][1];
    if (STG) {
      const float* sqr = &sq[rq * SQP + 8 * kq]; const float* scs = &sq[8 * SQP + 8 * kq]; const float* sbq = &sq[9 * SQP + 8 * kq];
      qa0 = *reinterpret_cast<const float4*>(sqr); qa1 = *reinterpret_cast<const float4*>(sqr + 4); qb0 = *reinterpret_cast<const float4*>(sqr + 32); qb1 = *reinterpret_cast<const float4*>(sqr + 36);
      cs0 = *reinterpret_cast<const float4*>(scs); cs1 = *reinterpret_cast<const float4*>(scs + 4); cs2 = *reinterpret_cast<const float4*>(scs + 32); cs3 = *reinterpret_cast<const float4*>(scs + 36);
      bq0 = *reinterpret_cast<const float4*>(sbq); bq1 = *reinterpret_cast<const float4*>(sbq + 4); bq2 = *reinterpret_cast<const float4*>(sbq + 32); bq3 = *reinterpret_cast<const float4*>(sbq + 36);
    }
    if (PSTAT && !STG) {      // the two halves of q_raw (when there are two; the staged form added them on the way into LDS)
      qa0 = make_float4(qa0.x + qc0.x, qa0.y + qc0.y, qa0.z + qc0.z, qa0.w + qc0.w); qa1 = make_float4(qa1.x + qc1.x, qa1.y + qc1.y, qa1.z + qc1.z, qa1.w + qc1.w);
      qb0 = make_float4(qb0.x + qc2.x, qb0.y + qc2.y, qb0.z + qc2.z, qb0.w + qc2.w); qb1 = make_float4(qb1.x + qc3.x, qb1.y + qc3.y, qb1.z + qc3.z, qb1.w + qc3.w);
    }
    qa0 = make_float4(rs * (qa0.x - mu * cs0.x) + bq0.x, rs * (qa0.y - mu * cs0.y) + bq0.y, rs * (qa0.z - mu * cs0.z) + bq0.z, rs * (qa0.w - mu * cs0.w) + bq0.w);
    qa1 = make_float4(rs * (qa1.x - mu * cs1.x) + bq1.x, rs * (qa1.y - mu * cs1.y) + bq1.y, rs * (qa1.z - mu * cs1.z) + bq1.z, rs * (qa1.w - mu * cs1.w) + bq1.w);
    qb0 = make_float4(rs * (qb0.x - mu * cs2.x) + bq2.x, rs * (qb0.y - mu * cs2.y) + bq2.y, rs * (qb0.z - mu * cs2.z) + bq2.z, rs * (qb0.w - mu * cs2.w) + bq2.w);
    qb1 = make_float4(rs * (qb1.x - mu * cs3.x) + bq3.x, rs * (qb1.y - mu * cs3.y) + bq3.y, rs * (qb1.z - mu * cs3.z) + bq3.z, rs * (qb1.w - mu * cs3.w) + bq3.w);
  }
  if (VLATE) {
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int sidx = 0; sidx < NSTEP; ++sidx) vf[sidx] = *reinterpret_cast<const u32x4*>(vb + 32 * sidx);
  }
  f16x8 qf0, qf1;
  qf0[0] = (f16)qa0.x; qf0[1] = (f16)qa0.y; qf0[2] = (f16)qa0.z; qf0[3] = (f16)qa0.w; qf0[4] = (f16)qa1.x; qf0[5] = (f16)qa1.y; qf0[6] = (f16)qa1.z; qf0[7] = (f16)qa1.w;
  qf1[0] = (f16)qb0.x; qf1[1] = (f16)qb0.y; qf1[2] = (f16)qb0.z; qf1[3] = (f16)qb0.w; qf1[4] = (f16)qb1.x; qf1[5] = (f16)qb1.y; qf1[6] = (f16)qb1.z; qf1[7] = (f16)qb1.w;

  // ---- scores: D[i = key][j = r]: lane holds r = l15, keys 16t + 4kq + reg
  float lmax = -INFINITY;
#pragma unroll
  for (int i = 0; i < TPW; ++i) {
    const int t = wave + 4 * i;
    {
      f32x4 acc = {0.f, 0.f, 0.f, 0.f};
      acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(*reinterpret_cast<const f16x8*>(&kf[i][0]), qf0, acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(*reinterpret_cast<const f16x8*>(&kf[i][1]), qf1, acc, 0, 0, 0);
#pragma unroll
      for (int r4 = 0; r4 < 4; ++r4) {
        const int kl = 16 * t + 4 * kq + r4;
        const float v = (kl < n) ? acc[r4] : -INFINITY;
        ssc[l15][kl] = v;
        lmax = fmaxf(lmax, v);
      }
    }
  }
  smax[wave * 4 + kq][l15] = lmax;
  __syncthreads();
  stamp(pf, 2);
  if (tid < 16) {
    float mxv = -INFINITY;
#pragma unroll
    for (int i = 0; i < 16; ++i) mxv = fmaxf(mxv, smax[i][tid]);
    smx[tid] = mxv;
  }
  __syncthreads();
  // ---- P = exp(S - max) as f16 (thread = key), row sums
  {
    const int kl = tid;
    const bool valid = kl < 64 * TPW;
    float e[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      e[r] = 0.f;
      if (r < R) {
        if (valid) e[r] = __expf(ssc[r][kl] - smx[r]);
        sp16[r * CA_PSTR + kl] = (f16)e[r];
      }
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) if (r < R) { const float v = wave_sum(e[r]); if (lane == 0) ssumw[wave][r] = v; }
  }
  __syncthreads();
  stamp(pf, 3);
  if (tid < 16) ssum[tid] = (ssumw[0][tid] + ssumw[1][tid]) + (ssumw[2][tid] + ssumw[3][tid]);

  // ---- O^T[dh][r]: wave w owns dh 16w .. 16w+15; D[i = dh][j = r]: lane holds r = l15, dh = 16w + 4kq + reg
  f32x4 oacc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int sidx = 0; sidx < NSTEP; ++sidx) {
    {
      const f16x8 pb = *reinterpret_cast<const f16x8*>(&sp16[rq * CA_PSTR + 32 * sidx + 8 * kq]);
      oacc = __builtin_amdgcn_mfma_f32_16x16x32_f16(*reinterpret_cast<const f16x8*>(&vf[sidx]), pb, oacc, 0, 0, 0);
    }
  }
  __syncthreads();   // ssum visible
  stamp(pf, 4);
  const int dh0 = 16 * wave + 4 * kq;
  if (C == 1) {
    if (l15 < R) {
      const float inv = 1.0f / ssum[l15];
      const f16x4 o = {(f16)(oacc[0] * inv), (f16)(oacc[1] * inv), (f16)(oacc[2] * inv), (f16)(oacc[3] * inv)};
      *reinterpret_cast<f16x4*>(out + (out_mb ? xf_index(b * R + l15, h * 64 + dh0, out_mb) : (size_t)(b * R + l15) * d + h * 64 + dh0)) = o;
    }
    return;
  }
  if (SPIN) {
    const unsigned tag = ep_now + 1u;
    // slot of (utterance-head, chunk c, row r): fixed strides (6 chunks x 8 rows) - the same words for every R / C / batch size, so a tag
    // in a slot was always written under THIS (utterance, head)'s epoch and can never alias another one's (advisor, round 3)
    gran_t* gbase = gran + (size_t)(b * H + h) * 6 * 8 * 66;
    if (c != C - 1) {      // producer: one granule per value, no drain, no ticket
      if (l15 < R) {
        gran_t* gp = gbase + ((size_t)c * 8 + l15) * 66;
#pragma unroll
        for (int r4 = 0; r4 < 4; ++r4) st_gran(gp + dh0 + r4, tag, oacc[r4]);
        if (wave == 0 && kq == 0) { st_gran(gp + 64, tag, smx[l15]); st_gran(gp + 65, tag, ssum[l15]); }
      }
      stamp(pf, 5);
      if (tid == 0) tl_end(prof);
      return;
    }
    // combiner: own partial through LDS (the score buffer is free), the other chunks' from their granules
    if (l15 < R) {
#pragma unroll
      for (int r4 = 0; r4 < 4; ++r4) ssc[l15][dh0 + r4] = oacc[r4];
      if (wave == 0 && kq == 0) { ssc[l15][64] = smx[l15]; ssc[l15][65] = ssum[l15]; }
    }
    __syncthreads();
    stamp(pf, 5);
    for (int item = tid; item < R * 32; item += 256) {
      const int r = item >> 5, dp = item & 31;
      float2 ml[CM], ov[CM];
      unsigned spins = 0;
      for (;;) {
        bool ok = true;
#pragma unroll
        for (int cc = 0; cc < CM - 1; ++cc) {
          if (cc < C - 1) {
            const gran_t* gp = gbase + ((size_t)cc * 8 + r) * 66;
            const gran_t g0 = ld_gran(gp + 64), g1 = ld_gran(gp + 65), g2 = ld_gran(gp + 2 * dp), g3 = ld_gran(gp + 2 * dp + 1);
            ok = ok & ((unsigned)(g0 >> 32) == tag) & ((unsigned)(g1 >> 32) == tag) & ((unsigned)(g2 >> 32) == tag) & ((unsigned)(g3 >> 32) == tag);
            ml[cc] = make_float2(__uint_as_float((unsigned)g0), __uint_as_float((unsigned)g1));
            ov[cc] = make_float2(__uint_as_float((unsigned)g2), __uint_as_float((unsigned)g3));
          }
        }
        if (ok) break;
        if (++spins > CA_SPIN_LIMIT) { atomicOr(epoch, 1u); break; }      // word 0: the give-up flag
        __builtin_amdgcn_s_sleep(1);
      }
      float M_ = ssc[r][64];
#pragma unroll
      for (int cc = 0; cc < CM - 1; ++cc) if (cc < C - 1) M_ = fmaxf(M_, ml[cc].x);
      float L = 0.f, O0 = 0.f, O1 = 0.f;
#pragma unroll
      for (int cc = 0; cc < CM - 1; ++cc) {
        if (cc < C - 1) {
          const float w = __expf(ml[cc].x - M_);
          L = fmaf(ml[cc].y, w, L); O0 = fmaf(ov[cc].x, w, O0); O1 = fmaf(ov[cc].y, w, O1);
        }
      }
      {      // own chunk last: the fixed chunk order 0 .. C-1 of the ticket form
        const float w = __expf(ssc[r][64] - M_);
        L = fmaf(ssc[r][65], w, L); O0 = fmaf(ssc[r][2 * dp], w, O0); O1 = fmaf(ssc[r][2 * dp + 1], w, O1);
      }
      const float inv = 1.0f / L;
      typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));
      const f16x2 o2 = {(f16)(O0 * inv), (f16)(O1 * inv)};
      *reinterpret_cast<f16x2*>(out + (out_mb ? xf_index(b * R + r, h * 64 + 2 * dp, out_mb) : (size_t)(b * R + r) * d + h * 64 + 2 * dp)) = o2;
    }
    if (tid == 0) __hip_atomic_store(epoch + 1 + b * H + h, tag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);      // next launch's epoch
    stamp(pf, 6);
    if (tid == 0) tl_end(prof);
    return;
  }
  // ---- split-T: publish the partial with write-through stores; the last-arriving workgroup combines
  float* pbase = part + ((size_t)(b * H + h) * C) * R * 66;
  if (l15 < R) {
    float* pp = pbase + ((size_t)c * R + l15) * 66;
#pragma unroll
    for (int r4 = 0; r4 < 4; ++r4) st_sc1(pp + dh0 + r4, oacc[r4]);
    if (wave == 0 && kq == 0) { st_sc1(pp + 64, smx[l15]); st_sc1(pp + 65, ssum[l15]); }
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");     // every storing wave drains its write-through stores
  __syncthreads();
  stamp(pf, 5);
  if (tid == 0) {
    const unsigned prev = __hip_atomic_fetch_add(counters + b * H + h, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const int last = (prev == (unsigned)(C - 1));
    if (last) {
      __hip_atomic_store(counters + b * H + h, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // re-arm for the next launch
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");                                          // drop this CU's stale L1 lines
    }
    s_last = last;
  }
  __syncthreads();
  stamp(pf, 6);
  if (tid == 0) tl_end(prof);
  if (!s_last) return;
  // one round: thread = (row r, dh pair); plain (pipelined) loads, made safe by the agent-scope acquire that lane 0
  // executed after winning the ticket (guide §6 G16 consumer form: relaxed ticket -> ONE acquire -> barrier -> plain loads;
  // 8-byte sc1 buffer loads were measured 4x slower than this on MI355X)
  // (R <= 16 rows x 32 dh pairs = up to 512 items over the 256 threads: the merged prefill pass of a long prompt has more than 8
  // rows per utterance - the op-level test at R = 16 found rows 8..15 uncombined when this was a single `if (tid < R * 32)`)
  for (int item = tid; item < R * 32; item += 256) {
    const int r = item >> 5, dp = item & 31;
    float2 ml[CM], ov[CM];
#pragma unroll
    for (int cc = 0; cc < CM; ++cc) {
      if (cc < C) {
        const float* pp = pbase + ((size_t)cc * R + r) * 66;
        ml[cc] = *reinterpret_cast<const float2*>(pp + 64);
        ov[cc] = *reinterpret_cast<const float2*>(pp + 2 * dp);
      }
    }
    float M_ = -INFINITY;
#pragma unroll
    for (int cc = 0; cc < CM; ++cc) if (cc < C) M_ = fmaxf(M_, ml[cc].x);
    float L = 0.f, O0 = 0.f, O1 = 0.f;
#pragma unroll
    for (int cc = 0; cc < CM; ++cc) {
      if (cc < C) {
        const float w = __expf(ml[cc].x - M_);
        L = fmaf(ml[cc].y, w, L); O0 = fmaf(ov[cc].x, w, O0); O1 = fmaf(ov[cc].y, w, O1);
      }
    }
    const float inv = 1.0f / L;
    typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));
    const f16x2 o2 = {(f16)(O0 * inv), (f16)(O1 * inv)};
    *reinterpret_cast<f16x2*>(out + (out_mb ? xf_index(b * R + r, h * 64 + 2 * dp, out_mb) : (size_t)(b * R + r) * d + h * 64 + 2 * dp)) = o2;
  }
  stamp(pf, 7);
  if (tid == 0) tl_end(prof);
}

// =======================================================================================
// Cross-attention of the batched step with ROLES (round 6; the folded query from row partials, 256-key chunks, <= 8 rows, d <= 1280).
// What the phase stamps of dec_cross_attn_kernel<4, 6, 4> showed at 8 utterances (profiles/r06_phase_cycles.md): a wave spends half of its
// life getting its 17 requests ACCEPTED (960 workgroups ask for 61 MB at once; the CU's address path takes them at the rate HBM
// answers), and scores, softmax and P.V - 6 us - start only behind that: a wave that is waiting for the memory pipeline to take its V
// requests cannot multiply the K fragments that have landed.  Here the waves of a workgroup have roles:
//   waves 0-1 (K waves)  request the query's operands, the row partials and the K fragments of THEIR 128 keys, finish the folded query,
//                        take scores, maximum, exponentials and row sums of their half chunk in registers (the MFMA output layout keeps a
//                        query row in a lane column: two cross-row shuffles, no score buffer), exchange the two row maxima through LDS flag
//                        words (K wave with K wave: no workgroup barrier) and leave P (f16) + (max, sum) in LDS behind a flag word;
//   waves 2-3 (V waves)  request V^T (32 head dimensions each) once the K waves' requests are in (one raw barrier), so K leads V through
//                        the memory pipeline, then accumulate O = V P half chunk by half chunk as the flags come up and publish the chunk
//                        partial as before (two granules per 16-byte store).
// The K waves never wait for a V wave (no workgroup barrier between the first one and the tail), so scores and softmax run while V is
// still streaming in.  Arithmetic: P and O are dec_cross_attn_kernel's bit for bit (exponentials about the chunk's maximum, P.V steps in key
// order); the row sum is added in another order (last-bit differences); partial format, combine and its order are the same.
// NT: K / V fragments by non-temporal loads - small grids only (every fragment is read once by one workgroup; measured -0.4 % of the one-utterance
// step, +1.6 % of the step at 8 utterances: session r6D)
#define WIS_CA_LD(p) (NT ? __builtin_nontemporal_load(p) : *(p))
// two granules in one 16-byte write-through store (the lane's neighbouring values): each half is a naturally aligned 8-byte unit of one 16-byte
// aligned store of one lane, which the memory pipeline carries in one piece (the reader still takes 8-byte granules); a quarter of the write
// transactions of the one-granule form
__device__ __forceinline__ void st_gran2(gran_t* p, unsigned tag, float v0, float v1) {
  const u32x4 g = {__float_as_uint(v0), tag, __float_as_uint(v1), tag};
  asm volatile("global_store_dwordx4 %0, %1, off sc1" :: "v"(p), "v"(g) : "memory");
}
// (Measured and not kept, round 6: the folded query finished ONCE per workgroup by the first V wave - which has nothing to ask for before the barrier - instead of by
// every K wave for itself, 81 instead of 96 wave requests per workgroup: 1.222 / 1.219 vs 1.204 / 1.205 ms per step at one utterance - the K waves then wait for a
// wave that started later - and 1.863 / 1.874 / 1.881 / 1.888 vs 1.880 / 1.885 / 1.883 / 1.886 at eight: nothing; sessions r6R / r6S.)
// NKW = K waves = V waves per workgroup: 2 at every call site (256 threads, four workgroups per CU: the batched step's 960 workgroups in one round).  4 + 4 waves
// for the one-utterance step's 120 workgroups measured 0.8 % slower per step: the CU's address path takes the same requests no faster from eight waves.
// all-reduce over the four 16-lane rows of a lane column (lanes l, l + 16, l + 32, l + 48) with gfx950's row-swap moves: v_permlane32_swap exchanges the upper
// half of its first operand with the lower half of its second (both = v: one register then holds the lower half's values twice, the other the upper half's),
// v_permlane16_swap the odd rows of the first with the even rows of the second - two VALU moves instead of two ds_bpermute round trips through the LDS pipe
__device__ __forceinline__ float xrow_max(float v) {
  const auto a = __builtin_amdgcn_permlane32_swap(__float_as_uint(v), __float_as_uint(v), false, false);
  const float m = fmaxf(__uint_as_float(a[0]), __uint_as_float(a[1]));
  const auto b = __builtin_amdgcn_permlane16_swap(__float_as_uint(m), __float_as_uint(m), false, false);
  return fmaxf(__uint_as_float(b[0]), __uint_as_float(b[1]));
}
__device__ __forceinline__ float xrow_sum(float v) {      // (both lanes of a pair add the same two operands in the same order: every lane of the column holds the same bits)
  const auto a = __builtin_amdgcn_permlane32_swap(__float_as_uint(v), __float_as_uint(v), false, false);
  const float m = __uint_as_float(a[0]) + __uint_as_float(a[1]);
  const auto b = __builtin_amdgcn_permlane16_swap(__float_as_uint(m), __float_as_uint(m), false, false);
  return __uint_as_float(b[0]) + __uint_as_float(b[1]);
}
template <bool SPIN, bool NT, int NKW>
__global__ __launch_bounds__(128 * NKW) void dec_cross_attn_rs_kernel(const float* __restrict__ q, const f16* __restrict__ kx, const f16* __restrict__ vt,
                                                                const float* __restrict__ xres, const float* __restrict__ q2, unsigned* epoch, int RHCC, int dT,
                                                                int TpadF, f16* __restrict__ out, float* part, unsigned* counters,
                                                                unsigned long long* prof, int out_mb,
                                                                const float* __restrict__ qcs, const float* __restrict__ qb, gran_t* gran) {
  constexpr int CM = 6, SQP = 68, NPT = 10, KT = 16 / NKW, KEYS = 256 / NKW, NB = 4 / NKW, VS = 8 / NKW, NTHR = 128 * NKW;      // key tiles / keys per K wave, 16-dh blocks / 32-key steps per flag per V wave
  // (CM: <= 6 chunks; SQP: staged operand pitch; NPT: row partials per lane, 8 lanes per row, d <= 1280)
  const int R = RHCC & 0xFF, H = (RHCC >> 8) & 0x3F, C = (RHCC >> 24) & 0xFF, d = dT & 0xFFFF, T = (dT >> 16) & 0xFFFF;
  __shared__ __attribute__((aligned(16))) f16 sp16[16 * CA_PSTR];
  __shared__ __attribute__((aligned(16))) float sq[NKW][10 * SQP];      // per K wave: rows 0..7 q_raw (both halves added), 8 column sums, 9 bias
  __shared__ float srow[NKW][8][2];
  __shared__ float sml[NKW][16][2];                                    // (chunk max, sum) of the K waves' parts
  __shared__ float own[16][66];                                        // the combiner's own partial
  __shared__ float smaxw[NKW][16];                                       // the K waves' row maxima (exchanged behind flagm)
  __shared__ int flag[NKW], flagm[NKW];
  __shared__ int s_last;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l15 = lane & 15, kq = lane >> 4;
  const int c = blockIdx.x, h = blockIdx.y, b = blockIdx.z;
  const int Tpad = TpadF & 0x3FFFFFFF, bkv = (TpadF >> 30) ? 0 : b;
  const int klo = c * 256, n = (klo + 256 <= T) ? 256 : T - klo;
  const bool kwave = wave < NKW; const int kw = wave & (NKW - 1);
  const int rq = l15 < R ? l15 : R - 1;
  // (tap builds: workgroup (0, 0, 0): its first K wave stamps entries 0-5 of the row, its first V wave entries 7-13)
  unsigned long long* pf = (c == 0 && h == 0 && b == 0 && lane == 0 && prof) ? (wave == 0 ? prof : (wave == NKW ? prof + 7 : nullptr)) : nullptr;
  if (tid == 0) tl_begin(prof);
  stamp(pf, 0);
  unsigned ep_now = 0;
  if (SPIN) ep_now = __hip_atomic_load(epoch + 1 + b * H + h, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  float o_[NB][4]; float Mc = 0.f, Lc = 0.f;      // V waves: the chunk's partial (NB 16-dh blocks of lane column r = l15)
#pragma unroll
  for (int i = 0; i < NB; ++i)
#pragma unroll
    for (int r4 = 0; r4 < 4; ++r4) o_[i][r4] = 0.f;

  if (kwave) {
    // ---- requests: the query's operands (one 16-byte piece per lane and array), the row partials (lane = (row, eighth)), the K fragments
    float4 stq[2], stq2[2];
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int sr0 = (lane >> 4) + 4 * u, sr = sr0 < R ? sr0 : R - 1;
      const size_t so = (size_t)(b * R + sr) * d + h * 64 + 4 * (lane & 15);
      stq[u] = *reinterpret_cast<const float4*>(q + so);
      stq2[u] = make_float4(0.f, 0.f, 0.f, 0.f);
      if (q2) stq2[u] = *reinterpret_cast<const float4*>(q2 + so);      // (uniform)
    }
    const float4 stc = *reinterpret_cast<const float4*>(((lane & 16) ? qb : qcs) + h * 64 + 4 * (lane & 15));
    const int ntile = d >> 4, l8 = lane & 7, prow = (lane >> 3) < R ? (lane >> 3) : R - 1;
    const float2* sp = reinterpret_cast<const float2*>(xres) + (size_t)(b * R + prow) * ntile;
    float2 pt[NPT];
#pragma unroll
    for (int i = 0; i < NPT; ++i) { const int t = l8 + 8 * i; pt[i] = sp[t < ntile ? t : ntile - 1]; }
    const f16* kb = kx + (size_t)(bkv * H + h) * 8 * T * 8;
    u32x4 kf[KT][2];
#pragma unroll
    for (int i = 0; i < KT; ++i) {
      int key = klo + KEYS * kw + 16 * i + l15; if (key > T - 1) key = T - 1;      // clamped; masked below
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) kf[i][ks] = WIS_CA_LD(reinterpret_cast<const u32x4*>(kb + ((size_t)(kq + 4 * ks) * T + key) * 8));
    }
    __builtin_amdgcn_sched_barrier(0);
    asm volatile("s_barrier" ::: "memory");      // the K requests are in: the V waves may ask for theirs (raw: no wait for any load)
    __builtin_amdgcn_sched_barrier(0);           // (and nothing that waits for a load moves above it: hipcc had hoisted the first statistics' wait)
    stamp(pf, 1);
    // ---- LayerNorm statistics of the R rows (Chan merge of the per-16-column (sum, M2) pairs about the first tile's mean), in every K wave
    const float c0 = __shfl(pt[0].x, lane & ~7) * 0.0625f;
    float a1 = 0.f, a2 = 0.f;
#pragma unroll
    for (int i = 0; i < NPT; ++i) {
      const bool in = l8 + 8 * i < ntile;
      const float dm = in ? pt[i].x * 0.0625f - c0 : 0.f;
      a1 += dm; a2 += in ? pt[i].y + 16.0f * dm * dm : 0.f;
    }
    a1 += dpp_f<0xB1>(a1); a2 += dpp_f<0xB1>(a2);
    a1 += dpp_f<0x4E>(a1); a2 += dpp_f<0x4E>(a2);
    a1 += dpp_f<0x141>(a1); a2 += dpp_f<0x141>(a2);      // the 8 lanes of a row hold its sums
    float* sqw = sq[kw];
    if (l8 == 0) {
      const float invd = 1.0f / (float)d, dmu = a1 * 16.0f * invd;
      srow[kw][lane >> 3][0] = c0 + dmu; srow[kw][lane >> 3][1] = 1.0f / sqrtf(fmaxf(a2 * invd - dmu * dmu, 0.f) + 1e-5f);
    }
#pragma unroll
    for (int u = 0; u < 2; ++u)
      *reinterpret_cast<float4*>(&sqw[((lane >> 4) + 4 * u) * SQP + 4 * (lane & 15)]) = make_float4(stq[u].x + stq2[u].x, stq[u].y + stq2[u].y, stq[u].z + stq2[u].z, stq[u].w + stq2[u].w);
    if (lane < 32) *reinterpret_cast<float4*>(&sqw[(8 + (lane >> 4)) * SQP + 4 * (lane & 15)]) = stc;
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");      // wave-private staging: the wave's own LDS writes have landed
    const float mu = srow[kw][rq][0], rs = srow[kw][rq][1];
    const float* sqr = &sqw[rq * SQP + 8 * kq]; const float* scs = &sqw[8 * SQP + 8 * kq]; const float* sbq = &sqw[9 * SQP + 8 * kq];
    f16x8 qf0, qf1;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      qf0[e] = (f16)(rs * (sqr[e] - mu * scs[e]) + sbq[e]);
      qf1[e] = (f16)(rs * (sqr[32 + e] - mu * scs[32 + e]) + sbq[32 + e]);
    }
    stamp(pf, 2);
    // ---- scores of this wave's KEYS keys: D[key][r], lane holds r = l15 and keys 16 i + 4 kq + reg; maximum and sums across the four lane rows
    f32x4 acc[KT];
    float lmax = -INFINITY;
#pragma unroll
    for (int i = 0; i < KT; ++i) {
      f32x4 a = {0.f, 0.f, 0.f, 0.f};
      a = __builtin_amdgcn_mfma_f32_16x16x32_f16(*reinterpret_cast<const f16x8*>(&kf[i][0]), qf0, a, 0, 0, 0);
      a = __builtin_amdgcn_mfma_f32_16x16x32_f16(*reinterpret_cast<const f16x8*>(&kf[i][1]), qf1, a, 0, 0, 0);
#pragma unroll
      for (int r4 = 0; r4 < 4; ++r4) {
        const int kl = KEYS * kw + 16 * i + 4 * kq + r4;
        a[r4] = (kl < n) ? a[r4] : -INFINITY;
        lmax = fmaxf(lmax, a[r4]);
      }
      acc[i] = a;
    }
    stamp(pf, 3);
    lmax = xrow_max(lmax);
    // the chunk's maximum = the larger of the two K waves' (the exponentials are taken about the CHUNK's maximum, as dec_cross_attn_kernel takes them:
    // P and O come out bit for bit as there, only the row sum is added in another order): the one exchange between the two K waves, through LDS
    // behind a flag word each - no workgroup barrier, the V waves are not involved
    if (kq == 0) smaxw[kw][l15] = lmax;
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    if (lane == 0) __hip_atomic_store(&flagm[kw], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
#pragma unroll
    for (int w = 0; w < NKW; ++w)
      while (__hip_atomic_load(&flagm[w], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) == 0) __builtin_amdgcn_s_sleep(1);
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    float mref = smaxw[0][l15];                               // finite: the chunk holds a key
#pragma unroll
    for (int w = 1; w < NKW; ++w) mref = fmaxf(mref, smaxw[w][l15]);
    float lsum = 0.f;
#pragma unroll
    for (int i = 0; i < KT; ++i) {
      f16x4 ph;
#pragma unroll
      for (int r4 = 0; r4 < 4; ++r4) { const float e = __expf(acc[i][r4] - mref); lsum += e; ph[r4] = (f16)e; }
      *reinterpret_cast<f16x4*>(&sp16[l15 * CA_PSTR + KEYS * kw + 16 * i + 4 * kq]) = ph;
    }
    lsum = xrow_sum(lsum);
    if (kq == 0) { sml[kw][l15][0] = mref; sml[kw][l15][1] = lsum; }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    if (lane == 0) __hip_atomic_store(&flag[kw], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    stamp(pf, 4);
  } else {
    if (lane < 2 * NKW && wave == NKW) __hip_atomic_store(lane < NKW ? &flag[lane] : &flagm[lane - NKW], 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
    __builtin_amdgcn_sched_barrier(0);
    stamp(pf, 0);
    // ---- V^T fragments of this wave's 16 NB head dimensions, in key order (the first K wave's keys first)
    const f16* vb = vt + ((size_t)(bkv * H + h) * 64 + 16 * NB * kw + l15) * Tpad + klo + 8 * kq;
    u32x4 vf[NB][8];
#pragma unroll
    for (int j = 0; j < NKW; ++j)
#pragma unroll
      for (int blk = 0; blk < NB; ++blk)
#pragma unroll
        for (int s4 = 0; s4 < VS; ++s4) vf[blk][VS * j + s4] = WIS_CA_LD(reinterpret_cast<const u32x4*>(vb + (size_t)blk * 16 * Tpad + 32 * (VS * j + s4)));
    __builtin_amdgcn_sched_barrier(0);
    stamp(pf, 1);
    f32x4 oacc[NB];
#pragma unroll
    for (int blk = 0; blk < NB; ++blk) oacc[blk] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int j = 0; j < NKW; ++j) {      // the 32-key steps in key order, as dec_cross_attn_kernel accumulates them; K wave j's keys as soon as its P is there
      while (__hip_atomic_load(&flag[j], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) == 0) __builtin_amdgcn_s_sleep(1);
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
      for (int s4 = 0; s4 < VS; ++s4) {
        const f16x8 pb = *reinterpret_cast<const f16x8*>(&sp16[rq * CA_PSTR + 32 * (VS * j + s4) + 8 * kq]);
#pragma unroll
        for (int blk = 0; blk < NB; ++blk) oacc[blk] = __builtin_amdgcn_mfma_f32_16x16x32_f16(*reinterpret_cast<const f16x8*>(&vf[blk][VS * j + s4]), pb, oacc[blk], 0, 0, 0);
      }
      if (j == 0 || j == NKW - 1) stamp(pf, j == 0 ? 2 : 3);
    }
    Mc = sml[0][rq][0];
    if (NKW == 2) Lc = sml[0][rq][1] + sml[1][rq][1];
    else Lc = (sml[0][rq][1] + sml[1][rq][1]) + (sml[2 % NKW][rq][1] + sml[3 % NKW][rq][1]);
#pragma unroll
    for (int blk = 0; blk < NB; ++blk)
#pragma unroll
      for (int r4 = 0; r4 < 4; ++r4) o_[blk][r4] = oacc[blk][r4];
    stamp(pf, 4);
  }

  // ---- the chunk's partial: (O[64], M, L) per row, published / combined as in dec_cross_attn_kernel (V wave kw owns dh 16 NB kw .. 16 NB (kw + 1) - 1)
  const int dhb = 16 * NB * kw + 4 * kq;      // + 16 blk
  const bool pub = !kwave && l15 < R;
  if (C == 1) {
    if (pub) {
      const float inv = 1.0f / Lc;
#pragma unroll
      for (int blk = 0; blk < NB; ++blk) {
        const f16x4 o = {(f16)(o_[blk][0] * inv), (f16)(o_[blk][1] * inv), (f16)(o_[blk][2] * inv), (f16)(o_[blk][3] * inv)};
        *reinterpret_cast<f16x4*>(out + (out_mb ? xf_index(b * R + l15, h * 64 + dhb + 16 * blk, out_mb) : (size_t)(b * R + l15) * d + h * 64 + dhb + 16 * blk)) = o;
      }
    }
    return;
  }
  if (SPIN) {
    const unsigned tag = ep_now + 1u;
    gran_t* gbase = gran + (size_t)(b * H + h) * 6 * 8 * 66;
    if (c != C - 1) {
      if (pub) {
        gran_t* gp = gbase + ((size_t)c * 8 + l15) * 66;
#pragma unroll
        for (int blk = 0; blk < NB; ++blk) { st_gran2(gp + dhb + 16 * blk, tag, o_[blk][0], o_[blk][1]); st_gran2(gp + dhb + 16 * blk + 2, tag, o_[blk][2], o_[blk][3]); }
        if (wave == NKW && kq == 0) st_gran2(gp + 64, tag, Mc, Lc);
      }
      stamp(pf, 5);
      if (tid == 0) tl_end(prof);
      return;
    }
    if (pub) {
#pragma unroll
      for (int blk = 0; blk < NB; ++blk)
#pragma unroll
        for (int r4 = 0; r4 < 4; ++r4) own[l15][dhb + 16 * blk + r4] = o_[blk][r4];
      if (wave == NKW && kq == 0) { own[l15][64] = Mc; own[l15][65] = Lc; }
    }
    __syncthreads();
    stamp(pf, 5);
    for (int item = tid; item < R * 32; item += NTHR) {
      const int r = item >> 5, dp = item & 31;
      float2 ml[CM], ov[CM];
      unsigned spins = 0;
      for (;;) {
        bool ok = true;
#pragma unroll
        for (int cc = 0; cc < CM - 1; ++cc) {
          if (cc < C - 1) {
            const gran_t* gp = gbase + ((size_t)cc * 8 + r) * 66;
            const gran_t g0 = ld_gran(gp + 64), g1 = ld_gran(gp + 65), g2 = ld_gran(gp + 2 * dp), g3 = ld_gran(gp + 2 * dp + 1);
            ok = ok & ((unsigned)(g0 >> 32) == tag) & ((unsigned)(g1 >> 32) == tag) & ((unsigned)(g2 >> 32) == tag) & ((unsigned)(g3 >> 32) == tag);
            ml[cc] = make_float2(__uint_as_float((unsigned)g0), __uint_as_float((unsigned)g1));
            ov[cc] = make_float2(__uint_as_float((unsigned)g2), __uint_as_float((unsigned)g3));
          }
        }
        if (ok) break;
        if (++spins > CA_SPIN_LIMIT) { atomicOr(epoch, 1u); break; }
        __builtin_amdgcn_s_sleep(1);
      }
      float M_ = own[r][64];
#pragma unroll
      for (int cc = 0; cc < CM - 1; ++cc) if (cc < C - 1) M_ = fmaxf(M_, ml[cc].x);
      float L = 0.f, O0 = 0.f, O1 = 0.f;
#pragma unroll
      for (int cc = 0; cc < CM - 1; ++cc) {
        if (cc < C - 1) {
          const float w = __expf(ml[cc].x - M_);
          L = fmaf(ml[cc].y, w, L); O0 = fmaf(ov[cc].x, w, O0); O1 = fmaf(ov[cc].y, w, O1);
        }
      }
      {
        const float w = __expf(own[r][64] - M_);
        L = fmaf(own[r][65], w, L); O0 = fmaf(own[r][2 * dp], w, O0); O1 = fmaf(own[r][2 * dp + 1], w, O1);
      }
      const float inv = 1.0f / L;
      typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));
      const f16x2 o2 = {(f16)(O0 * inv), (f16)(O1 * inv)};
      *reinterpret_cast<f16x2*>(out + (out_mb ? xf_index(b * R + r, h * 64 + 2 * dp, out_mb) : (size_t)(b * R + r) * d + h * 64 + 2 * dp)) = o2;
    }
    if (tid == 0) __hip_atomic_store(epoch + 1 + b * H + h, tag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    stamp(pf, 6);
    if (tid == 0) tl_end(prof);
    return;
  }
  // ---- ticket form (large grids)
  float* pbase = part + ((size_t)(b * H + h) * C) * R * 66;
  if (pub) {
    float* pp = pbase + ((size_t)c * R + l15) * 66;
#pragma unroll
    for (int blk = 0; blk < NB; ++blk)
#pragma unroll
      for (int r4 = 0; r4 < 4; ++r4) st_sc1(pp + dhb + 16 * blk + r4, o_[blk][r4]);
    if (wave == NKW && kq == 0) { st_sc1(pp + 64, Mc); st_sc1(pp + 65, Lc); }
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  stamp(pf, 5);
  if (tid == 0) {
    const unsigned prev = __hip_atomic_fetch_add(counters + b * H + h, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const int last = (prev == (unsigned)(C - 1));
    if (last) {
      __hip_atomic_store(counters + b * H + h, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    }
    s_last = last;
  }
  __syncthreads();
  if (tid == 0) tl_end(prof);
  if (!s_last) return;
  for (int item = tid; item < R * 32; item += NTHR) {
    const int r = item >> 5, dp = item & 31;
    float2 ml[CM], ov[CM];
#pragma unroll
    for (int cc = 0; cc < CM; ++cc) {
      if (cc < C) {
        const float* pp = pbase + ((size_t)cc * R + r) * 66;
        ml[cc] = *reinterpret_cast<const float2*>(pp + 64);
        ov[cc] = *reinterpret_cast<const float2*>(pp + 2 * dp);
      }
    }
    float M_ = -INFINITY;
#pragma unroll
    for (int cc = 0; cc < CM; ++cc) if (cc < C) M_ = fmaxf(M_, ml[cc].x);
    float L = 0.f, O0 = 0.f, O1 = 0.f;
#pragma unroll
    for (int cc = 0; cc < CM; ++cc) {
      if (cc < C) {
        const float w = __expf(ml[cc].x - M_);
        L = fmaf(ml[cc].y, w, L); O0 = fmaf(ov[cc].x, w, O0); O1 = fmaf(ov[cc].y, w, O1);
      }
    }
    const float inv = 1.0f / L;
    typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));
    const f16x2 o2 = {(f16)(O0 * inv), (f16)(O1 * inv)};
    *reinterpret_cast<f16x2*>(out + (out_mb ? xf_index(b * R + r, h * 64 + 2 * dp, out_mb) : (size_t)(b * R + r) * d + h * 64 + 2 * dp)) = o2;
  }
  stamp(pf, 6);
}

int launch_dec_cross_attn(hipStream_t st, const CrossAttnP& p) {
  const int B = p.B, R = p.R, H = p.H, d = p.d, T = p.T, Tpad = p.Tpad, chunks = p.chunks, xres_is_stat = p.xres_is_stat;
  const float* const xres = p.xres;
  if (xres && (!p.qcs || !p.qb || R > 8 || d > (xres_is_stat ? 2048 : 1280))) { set_error("dec_cross_attn: folded query needs column sums, bias, R <= 8 and d <= 1280 (2048 from partials)"); return WIS_E_ARG; }
  if (xres_is_stat && !xres) { set_error("dec_cross_attn: the fold from partials needs the row partials"); return WIS_E_ARG; }
  if (R < 1 || R > 16 || chunks < 1 || chunks > 16) { set_error("dec_cross_attn: R=%d chunks=%d unsupported", R, chunks); return WIS_E_UNSUPPORTED; }
  if (H > 63 || d > 65535 || T > 65535) { set_error("dec_cross_attn: H=%d d=%d T=%d beyond the packed shape arguments", H, d, T); return WIS_E_UNSUPPORTED; }
  const int CL = cdiv(cdiv(T, chunks), 32) * 32;     // chunk length: multiple of 32 keys (16-byte aligned V^T fragments)
  if ((CL != 128 && CL != 256) || CL * chunks > Tpad) { set_error("dec_cross_attn: %d chunks of %d keys unsupported (Tpad %d)", chunks, CL, Tpad); return WIS_E_UNSUPPORTED; }
  const int used = cdiv(T, CL);                      // chunks that actually hold keys
  static const int env_spin = getenv("WIS_CA_SPIN") ? atoi(getenv("WIS_CA_SPIN")) : 1;      // 0: always the ticket form (A/B switch)
  // granule hand-off: small grids only (fewer spinning combiners than CUs), the default 256-key chunking, <= 8 rows per utterance
  const bool spin = env_spin && p.gran && p.epoch && B * H <= CA_SPIN_MAX_BH && CL == 256 && used >= 2 && used <= 6 && R <= 8;
#define WIS_CA(TPWv, CMv, FOLDv, SPINv) hipLaunchKernelGGL((dec_cross_attn_kernel<TPWv, CMv, FOLDv, SPINv>), dim3(used, H, B), dim3(256), 0, st, p.q, p.kx, p.vt, xres, p.q2, p.epoch, \
                                                  (R | (H << 8) | (CL << 14) | (used << 24)), (d | (T << 16)), (Tpad | (p.kv_shared ? (1 << 30) : 0)), p.out, p.part, p.counters, p.prof, p.out_mb, p.qcs, p.qb, p.gran)
  if (xres_is_stat) {
    const bool small = (long)B * H * used <= 256;      // at most one workgroup per CU: V is requested up front (FOLD 3)
    // the role-split kernel (K waves / V waves): WIS_CA_RS=0 off (A/B switch), 1 the batched step's grids only, 2 (default) the one-utterance step's too
    static const int ca_rs = getenv("WIS_CA_RS") ? atoi(getenv("WIS_CA_RS")) : 2;
    if (ca_rs && (!small || ca_rs >= 2) && CL == 256 && used <= 6 && R <= 8 && d <= 1280) {
#define WIS_CA_RS(SPINv, NTv) hipLaunchKernelGGL((dec_cross_attn_rs_kernel<SPINv, NTv, 2>), dim3(used, H, B), dim3(256), 0, st, p.q, p.kx, p.vt, xres, p.q2, p.epoch, \
                                                        (R | (H << 8) | (CL << 14) | (used << 24)), (d | (T << 16)), (Tpad | (p.kv_shared ? (1 << 30) : 0)), p.out, p.part, p.counters, p.prof, p.out_mb, p.qcs, p.qb, p.gran)
      if (spin) { if (small) WIS_CA_RS(true, true); else WIS_CA_RS(true, false); }
      else { if (small) WIS_CA_RS(false, true); else WIS_CA_RS(false, false); }
#undef WIS_CA_RS
      return WIS_OK;
    }
    // FOLD 4 (large grids, <= 8 rows): the folded query's operands through LDS, V requested up front (WIS_CA_FOLD4=0: FOLD 2, V behind the prologue)
    static const bool fold4 = !(getenv("WIS_CA_FOLD4") && atoi(getenv("WIS_CA_FOLD4")) == 0);
    const bool f4 = fold4 && !small && R <= 8;
    if (spin) { if (small) WIS_CA(4, 6, 3, true); else if (f4) WIS_CA(4, 6, 4, true); else WIS_CA(4, 6, 2, true); }
    else if (CL <= 128) WIS_CA(2, 16, 2, false);
    else if (used <= 6) { if (small) WIS_CA(4, 6, 3, false); else if (f4) WIS_CA(4, 6, 4, false); else WIS_CA(4, 6, 2, false); } else WIS_CA(4, 16, 2, false);
  }
  else if (spin) { if (xres) WIS_CA(4, 6, 1, true); else WIS_CA(4, 6, 0, true); }
  else if (xres) { if (CL <= 128) WIS_CA(2, 16, 1, false); else if (used <= 6) WIS_CA(4, 6, 1, false); else WIS_CA(4, 16, 1, false); }
  else { if (CL <= 128) WIS_CA(2, 16, 0, false); else if (used <= 6) WIS_CA(4, 6, 0, false); else WIS_CA(4, 16, 0, false); }
#undef WIS_CA
  return WIS_OK;
}

// =======================================================================================
// logits processors + log-softmax statistics + per-sub-chunk top-n_cand.  grid (STAT_SUB / 4, M), block 256: every WAVE owns one
// of the STAT_SUB = 64 sub-chunks of a logits row (811 values for the multilingual vocabulary, 13 per lane) and works alone - the
// maximum, the sum of exponentials and the n_cand selection rounds are DPP wave reductions, no workgroup barrier anywhere
// (round 1 ran ten block-wide arg-best rounds with a barrier each: 21 us per step).
__device__ __forceinline__ bool better(float av, int ai, float bv, int bi) { return av > bv || (av == bv && ai < bi); }
// the same order without short-circuit control flow (hipcc turns `||` / `&&` on lane-varying operands into exec-mask branches;
// inside unrolled selection loops that is one branch per element)
__device__ __forceinline__ bool better_b(float av, int ai, float bv, int bi) { return (av > bv) | ((av == bv) & (ai < bi)); }
__device__ __forceinline__ void take_better(float& v, int& i, float ov, int oi) { const bool t = better_b(ov, oi, v, i); v = t ? ov : v; i = t ? oi : i; }

// ---- the noise of a sampled decode (include/wis_hip.h states it bit for bit; tests/sample_ref.py restates it in numpy)
// word 0 of Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3") over counter (c0, c1, c2, c3), key (k0, k1)
__device__ __forceinline__ unsigned philox4x32_10_w0(unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned k0, unsigned k1) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const unsigned h0 = __umulhi(0xD2511F53u, c0), l0 = 0xD2511F53u * c0;
    const unsigned h1 = __umulhi(0xCD9E8D57u, c2), l1 = 0xCD9E8D57u * c2;
    c0 = h1 ^ c1 ^ k0; c1 = l1; c2 = h0 ^ c3 ^ k1; c3 = l0;
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
  return c0;
}
// u = ((w >> 9) + 0.5) 2^-23 (exact in fp32, strictly inside (0, 1)), g = -log(-log(u)) with the accurate logf: the winners of a Gumbel-max are
// the u closest to 1, where log(u) is tiny and the fast __logf loses its relative accuracy
__device__ __forceinline__ float gumbel_of_word(unsigned w) {
  const float u = ((float)(w >> 9) + 0.5f) * 1.1920928955078125e-07f;
  return -logf(-logf(u));
}
// the perturbed value of token id `tk` with processed logit x: x / T + g, fp32, a true division (-inf stays -inf)
__device__ __forceinline__ float gumbel_perturb(float x, unsigned w, float T) { return __fadd_rn(__fdiv_rn(x, T), gumbel_of_word(w)); }

// TS: the timestamp form - three more [lo, hi) ranges of the row are masked, as ts_rules_kernel left them for the row in ts_desc
// (the plain form takes ts_desc = nullptr and compiles to what it was before the template parameter existed)
// SAMP: whole-vocabulary sampling - maximum and sum of exponentials of the UNPERTURBED row as ever (the score needs them), then every value is
// perturbed (x / T + Gumbel noise) and the wave reports its single best perturbed entry: st_val[.][0] = the perturbed value, [1] = that entry's
// unperturbed logit, st_idx[.][0] = its id (cfg.n_cand = 2 is the layout; the other instantiations never read sp)
template <bool TS, bool SAMP = false>
__global__ __launch_bounds__(256) void logit_stats_kernel(const float* __restrict__ logits, const float* __restrict__ bias_all,
                                                          const float* __restrict__ bias_begin, const int* __restrict__ step_u,
                                                          float* __restrict__ st_max, float* __restrict__ st_sum,
                                                          float* __restrict__ st_val, int* __restrict__ st_idx, SampleCfg cfg,
                                                          int lr_b, int lr_j, int lr_off, unsigned long long* prof, const int* __restrict__ rowmap,
                                                          const int* __restrict__ ts_desc, SampleP sp) {
  constexpr int PT = 16;   // values per lane: supports n_vocab <= 64 * 64 * 16
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int sc = blockIdx.x * 4 + wave, m = blockIdx.y, b = m / cfg.beam;
  unsigned long long* pf = (blockIdx.x == 0 && blockIdx.y == 0 && tid == 0) ? prof : nullptr;
  stamp(pf, 0);
  const int step = step_u[b];
  const int SL = cdiv(cfg.n_vocab, STAT_SUB);
  const int lo = sc * SL, hi = (lo + SL < cfg.n_vocab) ? lo + SL : cfg.n_vocab;
  // logits row of (utterance b, beam j): decode steps b*beam + j; the merged prefill+first step samples every beam from the
  // utterance's last prompt row (beams > 0 carry cum = -inf there)
  // (rowmap: draft verification of a beam search - live beam j's logits sit in the row of the draft node it was matched to)
  const int jb = m - b * cfg.beam;
  const float* row = logits + (size_t)(b * lr_b + (rowmap ? rowmap[jb] : jb) * lr_j + lr_off) * cfg.n_vocab_pad;
  const bool first = (step == 0) && cfg.suppress_blank;
  const bool mask_eot = cfg.fixed_new > 0 && step < cfg.fixed_new;
  const bool force_eot = cfg.fixed_new > 0 && step >= cfg.fixed_new;

  // straight-line loads: every stream of every value is requested before anything is waited for (clamped addresses, masks applied
  // by select - a guarded `if (nidx < hi) { load }` per value compiled into sixteen branches with a wait each: 15k cycles)
  float vals[PT]; u64 keys[PT];
  float lv[PT], la[PT], lb[PT];
  int r0l = 0, r0h = 0, r1l = 0, r1h = 0, r2l = 0, r2h = 0;
  if constexpr (TS) {
    const int* dsc = ts_desc + m * TS_DESC_INTS;
    r0l = dsc[0]; r0h = dsc[1]; r1l = dsc[2]; r1h = dsc[3]; r2l = dsc[4]; r2h = dsc[5];
  }
#pragma unroll
  for (int i = 0; i < PT; ++i) {
    const int nidx = lo + lane + 64 * i;
    const int cidx = nidx < hi ? nidx : hi - 1;
    lv[i] = row[cidx]; lb[i] = bias_begin[cidx]; la[i] = bias_all ? bias_all[cidx] : 0.f;
  }
  float mx = -INFINITY;
#pragma unroll
  for (int i = 0; i < PT; ++i) {
    const int nidx = lo + lane + 64 * i;
    float v = lv[i] + la[i];
    v = first ? v + lb[i] : v;
    bool dead = (nidx >= hi) | (mask_eot & (nidx == cfg.eot)) | (force_eot & (nidx != cfg.eot));
    if constexpr (TS) dead = dead | ((nidx >= r0l) & (nidx < r0h)) | ((nidx >= r1l) & (nidx < r1h)) | ((nidx >= r2l) & (nidx < r2h));
    v = dead ? -INFINITY : v;
    vals[i] = v; keys[i] = nidx < hi ? sel_key(v, nidx) : 0ull; mx = fmaxf(mx, v);
  }
  stamp(pf, 1);
  mx = wave_max(mx);
  float sum = 0.f;
  if (mx > -INFINITY) {
#pragma unroll
    for (int i = 0; i < PT; ++i) sum += __expf(vals[i] - mx);   // exp(-inf) = 0 for masked / out of range
  }
  sum = wave_sum(sum);
  if (lane == 0) { st_max[m * STAT_SUB + sc] = mx; st_sum[m * STAT_SUB + sc] = sum; }
  stamp(pf, 2);
  if constexpr (SAMP) {
    // one Philox block per value, all independent; the noise words of a test table are requested straight-line like the row itself
    const unsigned long long seed = sp.seeds[b];
    const unsigned k0 = (unsigned)seed, k1 = (unsigned)(seed >> 32);
    unsigned nw[PT];
    if (sp.noise) {
#pragma unroll
      for (int i = 0; i < PT; ++i) { const int nidx = lo + lane + 64 * i; nw[i] = sp.noise[(size_t)m * cfg.n_vocab + (nidx < hi ? nidx : hi - 1)]; }
    } else {
#pragma unroll
      for (int i = 0; i < PT; ++i) nw[i] = philox4x32_10_w0((unsigned)(lo + lane + 64 * i), (unsigned)step, (unsigned)jb, 0u, k0, k1);
    }
    u64 t[PT];
#pragma unroll
    for (int i = 0; i < PT; ++i) { const int nidx = lo + lane + 64 * i; t[i] = nidx < hi ? sel_key(gumbel_perturb(vals[i], nw[i], sp.T), nidx) : 0ull; keys[i] = t[i]; }
#pragma unroll
    for (int w = PT / 2; w >= 1; w >>= 1)
#pragma unroll
      for (int i = 0; i < w; ++i) t[i] = key_max(t[i], t[i + w]);
    const u64 best = wave_max_key(t[0]);
    float xw = -INFINITY;      // the winner's unperturbed logit: one lane holds the key (ids are distinct)
#pragma unroll
    for (int i = 0; i < PT; ++i) xw = ((keys[i] == best) & (best != 0ull)) ? vals[i] : xw;
    xw = wave_max(xw);
    if (lane == 0) {
      st_val[((size_t)m * STAT_SUB + sc) * 2] = best ? key_value(best) : -INFINITY;
      st_val[((size_t)m * STAT_SUB + sc) * 2 + 1] = xw;
      st_idx[((size_t)m * STAT_SUB + sc) * 2] = best ? key_index(best) : 0x7fffffff;
    }
    return;
  }
  // top-n_cand of the sub-chunk in (value desc, index asc) order: n_cand rounds of a wave arg-best over the lanes' best
  // not-yet-picked value
  // n_cand rounds: lane-local best key strictly below the previous pick (independent tests, a 4-level max tree - a scan that
  // threads one running best through all 16 values is a 16-deep dependent chain, and a lone wave per SIMD has nothing to hide a
  // dependent VALU latency behind), then a wave maximum of the keys
  u64 prev = ~0ull;
  for (int rnd = 0; rnd < cfg.n_cand; ++rnd) {
    u64 t[PT];
#pragma unroll
    for (int i = 0; i < PT; ++i) t[i] = keys[i] < prev ? keys[i] : 0ull;
#pragma unroll
    for (int w = PT / 2; w >= 1; w >>= 1)
#pragma unroll
      for (int i = 0; i < w; ++i) t[i] = key_max(t[i], t[i + w]);
    const u64 best = wave_max_key(t[0]);
    if (lane == 0) {     // an exhausted sub-chunk (every value picked or out of range) reports (-inf, INT_MAX)
      st_val[((size_t)m * STAT_SUB + sc) * cfg.n_cand + rnd] = best ? key_value(best) : -INFINITY;
      st_idx[((size_t)m * STAT_SUB + sc) * cfg.n_cand + rnd] = best ? key_index(best) : 0x7fffffff;
    }
    prev = best;
  }
  stamp(pf, 3);
}
int launch_logit_stats(hipStream_t st, const float* logits, const float* bias_all, const float* bias_begin, const int* step_u,
                       float* st_max, float* st_sum, float* st_val, int* st_idx, int B, const SampleCfg& cfg, int lr_b, int lr_j, int lr_off,
                       unsigned long long* prof, const int* rowmap, const int* ts_desc, const SampleP* sp) {
  if (cdiv(cfg.n_vocab, STAT_SUB) > 16 * 64) { set_error("logit_stats: vocab too large"); return WIS_E_UNSUPPORTED; }
  const SampleP none;
  if (sp && sp->topk < 0) {
    if (rowmap || cfg.n_cand != 2 || !sp->seeds || !(sp->T > 0.f)) { set_error("logit_stats: sampling form misconfigured"); return WIS_E_ARG; }
    if (ts_desc) hipLaunchKernelGGL((logit_stats_kernel<true, true>), dim3(STAT_SUB / 4, B * cfg.beam), dim3(256), 0, st, logits, bias_all, bias_begin, step_u,
                                    st_max, st_sum, st_val, st_idx, cfg, lr_b, lr_j, lr_off, prof, rowmap, ts_desc, *sp);
    else hipLaunchKernelGGL((logit_stats_kernel<false, true>), dim3(STAT_SUB / 4, B * cfg.beam), dim3(256), 0, st, logits, bias_all, bias_begin, step_u,
                            st_max, st_sum, st_val, st_idx, cfg, lr_b, lr_j, lr_off, prof, rowmap, nullptr, *sp);
    return WIS_OK;
  }
  if (ts_desc) hipLaunchKernelGGL((logit_stats_kernel<true, false>), dim3(STAT_SUB / 4, B * cfg.beam), dim3(256), 0, st, logits, bias_all, bias_begin, step_u,
                                  st_max, st_sum, st_val, st_idx, cfg, lr_b, lr_j, lr_off, prof, rowmap, ts_desc, none);
  else hipLaunchKernelGGL((logit_stats_kernel<false, false>), dim3(STAT_SUB / 4, B * cfg.beam), dim3(256), 0, st, logits, bias_all, bias_begin, step_u,
                          st_max, st_sum, st_val, st_idx, cfg, lr_b, lr_j, lr_off, prof, rowmap, nullptr, none);
  return WIS_OK;
}

// =======================================================================================
// Whisper's timestamp rules (openai-whisper ApplyTimestampRules, restated by CTranslate2 4.1.0 for prompts without <|notimestamps|>),
// the pre-pass of the timestamp form of the sampling tail.  grid B*beam (one workgroup per live row), block 256.  The row's generated
// history is bs.alive[m][0 .. step_u[b]); every rule masks a RANGE of ids, so what the pass leaves for logit_stats_kernel<true> is three
// [lo, hi) ranges per row (ts_desc, TS_DESC_INTS ints: ranges, then the decision flag and the step it was taken at):
//   range 0: <|notimestamps|> - or [0, tb) once the decision below masks the text, or at the first step
//   range 1: last token a timestamp: [tb, V) after a pair (or as the only token), else [0, eot) (text, EOT stays allowed);
//            first step: (tb + max_initial_timestamp_index, V)
//   range 2: timestamps may not decrease: [tb, t_last), t_last = the last timestamp when it opened a segment, else the last + 1
// Decision: over the row after bias_all / bias_begin / mask_eot and ranges 0-2, logsumexp(allowed timestamp logits) > max(allowed text
// logits) masks the text (the log-softmax normaliser is common to both sides; an all-masked side is -inf; strict).  force_eot (the
// measurement convention's last step) overrides every rule: nothing is masked here and logit_stats_kernel keeps EOT alone.
__device__ __forceinline__ float block_max_256(float v, float* red) {
  v = wave_max(v);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  __syncthreads();
  if (lane == 0) red[wave] = v;
  __syncthreads();
  return fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
}
__device__ __forceinline__ float block_sum_256(float v, float* red) {
  v = wave_sum(v);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  __syncthreads();
  if (lane == 0) red[wave] = v;
  __syncthreads();
  return (red[0] + red[1]) + (red[2] + red[3]);
}
__global__ __launch_bounds__(256) void ts_rules_kernel(const float* __restrict__ logits, const float* __restrict__ bias_all,
                                                       const float* __restrict__ bias_begin, const int* __restrict__ step_u,
                                                       const int* __restrict__ alive, SampleCfg cfg, int no_ts, int max_init,
                                                       int lr_b, int lr_j, int lr_off, int* __restrict__ ts_desc) {
  __shared__ float red[4];
  const int tid = threadIdx.x, m = blockIdx.x, b = m / cfg.beam, jb = m - b * cfg.beam;
  const int V = cfg.n_vocab, tb = no_ts + 1;
  int step = step_u[b];
  step = step < cfg.max_new ? step : cfg.max_new;
  const bool force_eot = cfg.fixed_new > 0 && step >= cfg.fixed_new;
  int* dsc = ts_desc + m * TS_DESC_INTS;
  if (force_eot) {
    if (tid < TS_DESC_INTS) dsc[tid] = (tid == 7) ? step : 0;
    return;
  }
  const bool first = (step == 0) && cfg.suppress_blank;
  const bool mask_eot = cfg.fixed_new > 0 && step < cfg.fixed_new;
  int r0l = no_ts, r0h = no_ts + 1, r1l = 0, r1h = 0, r2l = 0, r2h = 0;
  if (step == 0) {
    r0l = 0; r0h = tb;
    if (max_init >= 0 && tb + max_init + 1 < V) { r1l = tb + max_init + 1; r1h = V; }
  } else {
    // history: the position of the last timestamp (block maximum of the positions that hold one; max_new <= 256 = one token per thread)
    const int* hist = alive + (size_t)m * cfg.max_new;
    const int tk = tid < step ? hist[tid] : -1;
    const float lastpos = block_max_256(tk >= tb ? (float)tid : -1.f, red);
    const int last = hist[step - 1];
    const bool last_ts = last >= tb;
    const bool pen_ts = step < 2 || hist[step - 2] >= tb;
    if (last_ts) { if (pen_ts) { r1l = tb; r1h = V; } else { r1l = 0; r1h = cfg.eot; } }
    if (lastpos >= 0.f) {
      const int t_ts = hist[(int)lastpos];
      const int t_last = (last_ts && !pen_ts) ? t_ts : t_ts + 1;
      r2l = tb; r2h = t_last;
    }
  }
  // the decision, over the row as every earlier processor left it
  const float* row = logits + (size_t)(b * lr_b + jb * lr_j + lr_off) * cfg.n_vocab_pad;
  auto value = [&](int i) -> float {
    float v = row[i] + (bias_all ? bias_all[i] : 0.f);
    v = first ? v + bias_begin[i] : v;
    const bool dead = (mask_eot & (i == cfg.eot)) | ((i >= r0l) & (i < r0h)) | ((i >= r1l) & (i < r1h)) | ((i >= r2l) & (i < r2h));
    return dead ? -INFINITY : v;
  };
  float tmx = -INFINITY;
  for (int i = tid; i < tb; i += 256) tmx = fmaxf(tmx, value(i));
  float smx = -INFINITY;
  for (int i = tb + tid; i < V; i += 256) smx = fmaxf(smx, value(i));
  tmx = block_max_256(tmx, red);
  smx = block_max_256(smx, red);
  float ssum = 0.f;
  if (smx > -INFINITY)
    for (int i = tb + tid; i < V; i += 256) ssum += expf(value(i) - smx);
  ssum = block_sum_256(ssum, red);
  const float lse = smx > -INFINITY ? smx + logf(ssum) : -INFINITY;
  const bool ts_wins = lse > tmx;
  if (ts_wins) { r0l = 0; r0h = tb; }
  if (tid == 0) {
    dsc[0] = r0l; dsc[1] = r0h; dsc[2] = r1l; dsc[3] = r1h; dsc[4] = r2l; dsc[5] = r2h; dsc[6] = ts_wins ? 1 : 0; dsc[7] = step;
  }
}
int launch_ts_rules(hipStream_t st, const float* logits, const float* bias_all, const float* bias_begin, const BeamState& bs, int B,
                    const SampleCfg& cfg, int no_ts, int max_init, int lr_b, int lr_j, int lr_off, int* ts_desc) {
  if (cfg.max_new > 256 || no_ts + 1 >= cfg.n_vocab) { set_error("ts_rules: config out of range"); return WIS_E_UNSUPPORTED; }
  hipLaunchKernelGGL(ts_rules_kernel, dim3(B * cfg.beam), dim3(256), 0, st, logits, bias_all, bias_begin, bs.step_u, bs.alive, cfg, no_ts, max_init,
                     lr_b, lr_j, lr_off, ts_desc);
  return WIS_OK;
}

// =======================================================================================
// repetition_penalty / no_repeat_ngram_size (CTranslate2 4.1.0 RepetitionPenalty / NoRepeatNgram, restated), the pre-pass at the head of the
// sampling tail when either option is on.  grid B*beam (one workgroup per live row), block 256.  The row's generated history is
// bs.alive[m][0 .. min(step_u[b], max_new)) - max_new <= 256 = one token per thread, as in ts_rules_kernel - and the row of m->logits the
// step samples from is PATCHED IN PLACE, so every kernel behind this one reads a row that already carries both rules:
//   penalty p: every DISTINCT history token t gets one read-modify-write, x < 0 ? x * p : x / p (fp32, a true division) - the thread that
//              holds the first occurrence of t does it, so a token that occurs three times is penalised once;
//   n-gram n:  thread i <= L - n compares h[i .. i+n-2] with the last n - 1 tokens and stores -inf at h[i+n-1] on a match (n = 1: every
//              history token; L < n: nothing).  The bans are stored behind a barrier: a token both penalised and banned ends as -inf.
// Nothing happens at step 0 (every beam samples from ONE shared prompt row there, and no history exists), for a finished (or parked)
// utterance, or on the measurement convention's forced-EOT step (only EOT survives that step, and EOT is in no history that continues).
__global__ __launch_bounds__(256) void rep_rules_kernel(float* __restrict__ logits, const int* __restrict__ step_u, const int* __restrict__ done,
                                                        const int* __restrict__ alive, SampleCfg cfg, float penalty, int ngram,
                                                        int lr_b, int lr_j, int lr_off) {
  __shared__ int4 sh4[64];
  int* sh = reinterpret_cast<int*>(sh4);
  const int tid = threadIdx.x, m = blockIdx.x, b = m / cfg.beam, jb = m - b * cfg.beam;
  if (done[b]) return;
  int L = step_u[b];
  L = L < cfg.max_new ? L : cfg.max_new;
  if (L <= 0 || (cfg.fixed_new > 0 && L >= cfg.fixed_new)) return;
  const int V = cfg.n_vocab;
  int tk = tid < L ? alive[(size_t)m * cfg.max_new + tid] : -1;
  tk = (tk >= 0 && tk < V) ? tk : -1;      // (nothing outside the row is ever addressed)
  sh[tid] = tk;
  __syncthreads();
  float* row = logits + (size_t)(b * lr_b + jb * lr_j + lr_off) * cfg.n_vocab_pad;
  if (penalty != 1.f) {
    bool dup = false;      // an earlier position holds the same token (broadcast LDS reads, four positions each)
    for (int i = 0; i < L; i += 4) {
      const int4 h = sh4[i >> 2];
      dup = dup | ((h.x == tk) & (i < tid)) | ((h.y == tk) & (i + 1 < tid)) | ((h.z == tk) & (i + 2 < tid)) | ((h.w == tk) & (i + 3 < tid));
    }
    if (tk >= 0 && !dup) { const float x = row[tk]; row[tk] = x < 0.f ? x * penalty : __fdiv_rn(x, penalty); }
  }
  if (ngram >= 1 && L >= ngram) {
    __syncthreads();       // the penalty's stores are ahead of the bans (workgroup-scope release / acquire)
    bool hit = tid <= L - ngram;
    const int i0 = hit ? tid : 0, tail = L - ngram + 1;
    for (int q = 0; q < ngram - 1; ++q) hit = hit & (sh[i0 + q] == sh[tail + q]);
    const int t = sh[i0 + ngram - 1];
    if (hit && t >= 0) row[t] = -INFINITY;
  }
}
int launch_rep_rules(hipStream_t st, float* logits, const BeamState& bs, int B, const SampleCfg& cfg, float penalty, int ngram, int lr_b, int lr_j, int lr_off) {
  if (cfg.max_new > 256 || !(penalty > 0.f) || ngram < 0) { set_error("rep_rules: config out of range"); return WIS_E_UNSUPPORTED; }
  hipLaunchKernelGGL(rep_rules_kernel, dim3(B * cfg.beam), dim3(256), 0, st, logits, bs.step_u, bs.done, bs.alive, cfg, penalty, ngram, lr_b, lr_j, lr_off);
  return WIS_OK;
}

// no_speech_prob (openai-whisper probs_at_sot, CTranslate2 return_no_speech_prob): softmax over the full vocabulary of the raw logits of
// the decoder row that read <|startoftranscript|>, at <|nospeech|>.  grid B, block 256; row of utterance b = logits + (b * rs + r0) * ld
__global__ __launch_bounds__(256) void no_speech_kernel(const float* __restrict__ logits, int ld, int rs, int r0, int V, int ns, float* __restrict__ out) {
  __shared__ float red[4];
  const int b = blockIdx.x, tid = threadIdx.x;
  const float* row = logits + (size_t)(b * rs + r0) * ld;
  float mx = -INFINITY;
  for (int i = tid; i < V; i += 256) mx = fmaxf(mx, row[i]);
  mx = block_max_256(mx, red);
  float s = 0.f;
  for (int i = tid; i < V; i += 256) s += expf(row[i] - mx);
  s = block_sum_256(s, red);
  if (tid == 0) out[b] = expf(row[ns] - mx) / s;
}
int launch_no_speech(hipStream_t st, const float* logits, int ld, int B, int rs, int r0, int V, int ns, float* out) {
  if (ns < 0 || ns >= V) { set_error("no_speech: token %d outside the vocabulary", ns); return WIS_E_ARG; }
  hipLaunchKernelGGL(no_speech_kernel, dim3(B), dim3(256), 0, st, logits, ld, rs, r0, V, ns, out);
  return WIS_OK;
}
// ... of a batch whose prompts differ in length (wis_generate_ragged): the <|startoftranscript|> row is another one in every utterance, and not every
// utterance has it in this pass.  rows: device word per utterance - its row of the pass's rs (row of utterance b = logits + (b * rs + rows[b]) * ld), or a
// value outside [0, rs): out[b] is left alone (the workgroup returns as a whole).  The arithmetic, reduction order included, is no_speech_kernel's.
__global__ __launch_bounds__(256) void no_speech_rows_kernel(const float* __restrict__ logits, int ld, int rs, const int* __restrict__ rows, int V, int ns, float* __restrict__ out) {
  __shared__ float red[4];
  const int b = blockIdx.x, tid = threadIdx.x;
  const int r0 = rows[b];
  if (r0 < 0 || r0 >= rs) return;
  const float* row = logits + (size_t)(b * rs + r0) * ld;
  float mx = -INFINITY;
  for (int i = tid; i < V; i += 256) mx = fmaxf(mx, row[i]);
  mx = block_max_256(mx, red);
  float s = 0.f;
  for (int i = tid; i < V; i += 256) s += expf(row[i] - mx);
  s = block_sum_256(s, red);
  if (tid == 0) out[b] = expf(row[ns] - mx) / s;
}
int launch_no_speech_rows(hipStream_t st, const float* logits, int ld, int B, int rs, const int* rows, int V, int ns, float* out) {
  if (ns < 0 || ns >= V || !rows || rs < 1) { set_error("no_speech_rows: token %d outside the vocabulary, or no row table", ns); return WIS_E_ARG; }
  hipLaunchKernelGGL(no_speech_rows_kernel, dim3(B), dim3(256), 0, st, logits, ld, rs, rows, V, ns, out);
  return WIS_OK;
}

// Greedy pick of teacher-forced rows (wis_generate_draft: the final decode of a streamed recording verifies the last interim hypothesis
// in a few multi-row passes instead of one pass per token).  One wave per logits row over what logit_stats_kernel left for it: the
// log-softmax normaliser from the 64 sub-chunk (max, sum-exp) pairs and the best candidate of the 64 sub-chunk winners, in
// beam_step_kernel's arithmetic and order (score = logit - lse, ties to the lower token id) - the token beam_step would take at k = 1.
__global__ __launch_bounds__(64) void greedy_pick_kernel(const float* __restrict__ st_max, const float* __restrict__ st_sum, const float* __restrict__ st_val,
                                                         const int* __restrict__ st_idx, int n_cand, int V, int* __restrict__ tok_out, float* __restrict__ lp_out) {
  const int m = blockIdx.x, lane = threadIdx.x;
  const float smx = st_max[m * STAT_SUB + lane], ssm = st_sum[m * STAT_SUB + lane];
  const float v = st_val[((size_t)m * STAT_SUB + lane) * n_cand];
  const int ix = st_idx[((size_t)m * STAT_SUB + lane) * n_cand];
  const float M_ = wave_max(smx);
  const float S = wave_sum(smx > -INFINITY ? ssm * __expf(smx - M_) : 0.f);
  const float lse = M_ + logf(S);
  const int tk = ix > V - 1 ? V - 1 : ix;
  const u64 best = wave_max_key(sel_key(v > -INFINITY ? v - lse : -INFINITY, tk));
  if (lane == 0) { tok_out[m] = key_index(best); lp_out[m] = key_value(best); }
}
int launch_greedy_pick(hipStream_t st, const float* st_max, const float* st_sum, const float* st_val, const int* st_idx, int rows, const SampleCfg& cfg, int* tok_out, float* lp_out) {
  hipLaunchKernelGGL(greedy_pick_kernel, dim3(rows), dim3(64), 0, st, st_max, st_sum, st_val, st_idx, cfg.n_cand, cfg.n_vocab, tok_out, lp_out);
  return WIS_OK;
}

// =======================================================================================
// beam search bookkeeping (CTranslate2 4.1.0 BeamSearch::search semantics).  grid B, block 256 (four waves per
// utterance).  Everything the step needs from memory - the candidate pool (k rows x 64 sub-chunks x n_cand), the row statistics,
// the cumulative scores, the step / done / hypothesis counters and the token histories - is requested up front in one round
// trip; the pool lives in registers (<= 32 entries per thread), the n_cand selection rounds are wave arg-bests joined through a
// double-buffered 4-entry LDS exchange (one barrier per round).
// PSL = pool entries per thread: 16 covers beam <= 5 (5 x 64 x 10 = 3200 entries), 32 the largest beam (8 x 64 x 16)
// End of a beam step for one workgroup (thread 0, after the workgroup's global writes are fenced): count it; the workgroup that
// ends the step as the LAST of the grid publishes the step to the host-mapped progress block - one 8-byte system-scope release
// store that the host polls between graph launches (generate.hip run_paced), so a search that ends on EOT is noticed without a
// stream round trip.  Results of finished utterances were written to the same block (and fenced at system scope) before their
// workgroup's count, so whoever reads "done = B" in the record finds them there.
__device__ __forceinline__ void publish_step(const BeamState& bs) {
  __threadfence();
  const unsigned B = gridDim.x;
  const unsigned n = atomicAdd(bs.tick, 1u) + 1u;
  if (n % B != 0u) return;
  __threadfence();
  const unsigned steps = n / B;
  const unsigned done = (unsigned)__hip_atomic_load(bs.all_done, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  const unsigned gen = __hip_atomic_load(bs.tick + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  const unsigned gu = bs.giveup ? (__hip_atomic_load(bs.giveup, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0u ? 1u : 0u) : 0u;
  const unsigned long long now = (unsigned long long)__builtin_amdgcn_s_memrealtime();
  if (steps == 1u) __hip_atomic_store(bs.host + HP_STAMP0, now, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  __hip_atomic_store(bs.host + HP_STAMP, now, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  if (done >= B && atomicCAS(bs.tick + 2, 0u, steps) == 0u) {
    __hip_atomic_store(bs.host + HP_DONE_STEP, (unsigned long long)steps, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    __hip_atomic_store(bs.host + HP_DONE_STAMP, now, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  }
  const unsigned long long rec = ((unsigned long long)(gen & 0xFFFFu) << 48) | ((unsigned long long)(steps & 0xFFFFu) << 32) | ((unsigned long long)gu << 16) | (done & 0xFFFFu);
  __hip_atomic_store(bs.host + HP_REC, rec, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}

// The prompt length of a step kernel: a kernel argument (PT = int: the shipped instantiations), or one device word per utterance (PT = const int*: the
// long-prompt route - one captured step serves every prompt length, as the Philox seeds are read)
__device__ __forceinline__ int prompt_len(int P, int) { return P; }
__device__ __forceinline__ int prompt_len(const int* plen, int b) { return plen[b]; }

template <int PSL, class PT>
__global__ __launch_bounds__(256) void beam_step_kernel(const float* __restrict__ st_max, const float* __restrict__ st_sum,
                                                        const float* __restrict__ st_val, const int* __restrict__ st_idx,
                                                        BeamState bs, RowMeta rm, PT P, int ctx, SampleCfg cfg, unsigned long long* prof, int n_best) {
  constexpr int HPT = (MAX_R * 256 + 255) / 256;                    // history tokens per thread (8)
  __shared__ float lse[MAX_R], s_cum[MAX_R];
  __shared__ float cand_v[MAX_CAND]; __shared__ int cand_word[MAX_CAND]; __shared__ int cand_org[MAX_CAND];
  __shared__ int nb_src[MAX_R]; __shared__ int nb_tok[MAX_R]; __shared__ float nb_cum[MAX_R];
  __shared__ int hyp_src[MAX_R]; __shared__ int hyp_slot[MAX_R]; __shared__ int hyp_n[MAX_R]; __shared__ int n_newhyp;
  __shared__ int s_finished;
  __shared__ int sh_alive[MAX_R * 256];
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  unsigned long long* pf = (b == 0 && tid == 0) ? prof : nullptr;
  stamp(pf, 0);
  const int k = cfg.beam, NC = cfg.n_cand, V = cfg.n_vocab;
  const int r0 = b * k, per_row = STAT_SUB * NC, total = k * per_row;
  // ---- one round trip: pool, statistics, scores, counters, histories
  float pv_[PSL]; int pi_[PSL];
#pragma unroll
  for (int u = 0; u < PSL; ++u) {
    const int e = tid + 256 * u, ce = e < total ? e : total - 1;       // clamped address, masked by select: straight-line loads
    const float v = st_val[(size_t)r0 * per_row + ce]; const int ix = st_idx[(size_t)r0 * per_row + ce];     // rows r0 .. r0+k-1 are contiguous
    pv_[u] = e < total ? v : -INFINITY; pi_[u] = e < total ? ix : 0x7fffffff;
  }
  float smx[2], ssm[2];                      // wave w reduces rows w and w + 4; lane = sub-chunk
#pragma unroll
  for (int j2 = 0; j2 < 2; ++j2) {
    const int j = wave + 4 * j2, mrow = r0 + (j < k ? j : 0);
    smx[j2] = st_max[mrow * STAT_SUB + lane]; ssm[j2] = st_sum[mrow * STAT_SUB + lane];
  }
  const float my_cum = tid < k ? bs.cum[r0 + tid] : 0.f;
  int hist_tok[HPT];
#pragma unroll
  for (int u = 0; u < HPT; ++u) {            // token histories of the k beams, whole rows (nothing here waits for the step counter)
    const int i = tid + 256 * u, j = i >> 8, t = i & 255;
    const int cj = j < k ? j : k - 1, ct = t < cfg.max_new ? t : cfg.max_new - 1;
    hist_tok[u] = bs.alive[(size_t)(r0 + cj) * cfg.max_new + ct];
  }
  const int done_b = bs.done[b];
  const int step = bs.step_u[b];
  const int nh0 = bs.n_hyp[b];
  if (done_b) { if (tid == 0) publish_step(bs); return; }

  stamp(pf, 1);
#pragma unroll
  for (int u = 0; u < HPT; ++u) { const int i = tid + 256 * u; if (i < MAX_R * 256) sh_alive[i] = hist_tok[u]; }
  if (tid < k) s_cum[tid] = my_cum;
  // log-softmax normaliser per live row
#pragma unroll
  for (int j2 = 0; j2 < 2; ++j2) {
    const int j = wave + 4 * j2;
    const float M_ = wave_max(smx[j2]);
    const float S = wave_sum(smx[j2] > -INFINITY ? ssm[j2] * __expf(smx[j2] - M_) : 0.f);
    if (lane == 0 && j < k) lse[j] = M_ + logf(S);
  }
  __syncthreads();
  stamp(pf, 2);
  // score = logit - lse + cum ; id = (beam << 20) | token (orders like the flat id beam * V + token, V < 2^20); every pool entry
  // becomes one selection key (common.hpp sel_key: score descending, then id ascending)
  u64 pk[PSL];
  u64 lbest = 0ull;
  const float inv_per_row = 1.0f / (float)per_row;
#pragma unroll
  for (int u = 0; u < PSL; ++u) {
    const int e = tid + 256 * u;
    int j = (int)(((float)e + 0.5f) * inv_per_row);          // e / per_row (e < 8192: exact in fp32), no integer division
    j = j < k ? j : k - 1;                                   // entries beyond the pool: clamped row, masked below
    const float v = pv_[u];
    const float sc_ = (v - lse[j]) + s_cum[j];               // (-inf stays -inf: lse and cum of a live row are finite or -inf, never +inf)
    int tk = pi_[u]; tk = tk > V - 1 ? V - 1 : tk;           // exhausted sub-chunks report INT_MAX with -inf
    pk[u] = e < total ? sel_key(v > -INFINITY ? sc_ : -INFINITY, (j << 20) | tk) : 0ull;
    lbest = key_max(lbest, pk[u]);
  }
  stamp(pf, 3);
  // top-NC of the pool, hierarchically (a block-wide selection round costs a wave reduction, an LDS exchange and a barrier - 2400
  // cycles measured; ten of them were half the kernel): every wave selects the top NC of ITS quarter of the pool on its own (wave
  // maximum of the lane-local bests, retire, 4-level max tree; no barrier), then the 4 NC wave candidates are ranked in one pass -
  // a candidate's rank is the number of candidates with a larger key (keys are distinct: the id is part of the key).
  __shared__ u64 wcand[4 * MAX_CAND];
  for (int rnd = 0; rnd < NC; ++rnd) {
    const u64 wb = wave_max_key(lbest);
    if (lane == 0) wcand[wave * NC + rnd] = wb;
#pragma unroll
    for (int u = 0; u < PSL; ++u) pk[u] = pk[u] == wb ? 0ull : pk[u];
    u64 t[PSL];
#pragma unroll
    for (int u = 0; u < PSL; ++u) t[u] = pk[u];
#pragma unroll
    for (int w = PSL / 2; w >= 1; w >>= 1)
#pragma unroll
      for (int u = 0; u < w; ++u) t[u] = key_max(t[u], t[u + w]);
    lbest = t[0];
  }
  if (tid < MAX_CAND) { cand_v[tid] = -INFINITY; cand_word[tid] = V - 1; cand_org[tid] = 0; }     // fewer real entries than candidates: -inf on a valid row / token
  __syncthreads();
  if (tid < 4 * NC) {
    const u64 mine = wcand[tid];
    int rank = 0;
#pragma unroll
    for (int m2 = 0; m2 < 4 * MAX_CAND; ++m2) rank += (m2 < 4 * NC && wcand[m2] > mine) ? 1 : 0;      // broadcast LDS reads, independent compares
    if (mine != 0ull && rank < NC) {
      const int bi = key_index(mine);
      cand_v[rank] = key_value(mine); cand_word[rank] = bi & 0xFFFFF; cand_org[rank] = (bi >> 20) & 0x7FF;
    }
  }
  __syncthreads();

  stamp(pf, 4);
  // serial bookkeeping
  if (tid == 0) {
    const bool is_last = (step + 1 >= cfg.max_new);
    int nh = nh0, second = k, newh = 0; bool top_finished = false;
    for (int kk = 0; kk < k; ++kk) {
      int next = kk;
      const bool eos = cand_word[kk] == cfg.eot;
      if (eos || is_last) {
        if (kk == 0) top_finished = true;
        if (nh < cfg.max_hyp) {
          hyp_src[newh] = kk; hyp_slot[newh] = nh; hyp_n[newh] = eos ? step : step + 1;   // EOS is not part of the hypothesis
          bs.hyp_score[b * cfg.max_hyp + nh] = cand_v[kk];
          bs.hyp_len[b * cfg.max_hyp + nh] = hyp_n[newh];
          ++newh; ++nh;
        }
        for (int j = second; j < NC; ++j)
          if (cand_word[j] != cfg.eot) { next = j; second = j + 1; break; }
      }
      nb_src[kk] = next; nb_tok[kk] = cand_word[next]; nb_cum[kk] = cand_v[next];
    }
    n_newhyp = newh;
    bs.n_hyp[b] = nh;
    bool fin = is_last;
    if (!fin) fin = cfg.allow_early_exit ? (top_finished && nh >= cfg.early_exit_hyps) : (nh >= cfg.max_candidates);
    s_finished = fin ? 1 : 0;
  }
  __syncthreads();

  stamp(pf, 5);
  const int hist = step;                 // tokens already in alive[] (sh_alive holds the whole rows)
  const int npos = prompt_len(P, b) - 1 + step + 1;     // cache positions valid after this step
  // finished hypotheses of this step
  for (int hh = 0; hh < n_newhyp; ++hh) {
    const int kk = hyp_src[hh], org = cand_org[kk], n = hyp_n[hh];
    int* dst = bs.hyp_tok + ((size_t)b * cfg.max_hyp + hyp_slot[hh]) * cfg.max_new;
    for (int t = tid; t < n; t += 256) dst[t] = (t < hist) ? sh_alive[org * 256 + t] : cand_word[kk];
  }
  if (s_finished) {
    __syncthreads();
    __threadfence_block();
    if (tid == 0) {
      // finalize_result: score / len^length_penalty, best first: the n_best best, the first registered among equal scores (result i of the
      // utterance at b n_best + i; n_best = 1 is the one result at b)
      const int nh = bs.n_hyp[b];
      unsigned taken = 0u;
      for (int r = 0; r < n_best; ++r) {
        int best = -1; float bsc = -INFINITY;
        for (int i = 0; i < nh; ++i) {
          if ((taken >> i) & 1u) continue;
          if (best < 0) best = i;
          float s = bs.hyp_score[b * cfg.max_hyp + i];
          const int n = bs.hyp_len[b * cfg.max_hyp + i];
          if (cfg.length_penalty != 0.f) s /= powf((float)n, cfg.length_penalty);
          if (s > bsc) { bsc = s; best = i; }
        }
        cand_org[r] = best;
        const int len = best >= 0 ? bs.hyp_len[b * cfg.max_hyp + best] : 0;
        if (best >= 0) taken |= 1u << best;
        bs.out_len[b * n_best + r] = len;
        bs.out_score[b * n_best + r] = bsc;
        hp_out_len(bs.host)[b * n_best + r] = len;      // the host's copy of the result (fenced below, before the step is published)
        hp_out_score(bs.host)[b * n_best + r] = bsc;
      }
      bs.done[b] = 1;
    }
    __syncthreads();
    for (int r = 0; r < n_best; ++r) {
      const int best = cand_org[r];
      if (best < 0) continue;
      const int n = bs.hyp_len[b * cfg.max_hyp + best];
      const int* src = bs.hyp_tok + ((size_t)b * cfg.max_hyp + best) * cfg.max_new;
      int* hids = hp_out_ids(bs.host) + (size_t)(b * n_best + r) * cfg.max_new;
      for (int t = tid; t < n; t += 256) { const int v = src[t]; bs.out_ids[(size_t)(b * n_best + r) * cfg.max_new + t] = v; hids[t] = v; }
    }
    __threadfence_system();
    __syncthreads();
    if (tid == 0) { atomicAdd(bs.all_done, 1); publish_step(bs); }
    return;
  }
  stamp(pf, 7);
  // next live beams
  for (int j = 0; j < k; ++j) {
    const int org = cand_org[nb_src[j]];
    int* al = bs.alive + (size_t)(r0 + j) * cfg.max_new;
    for (int t = tid; t < hist; t += 256) al[t] = sh_alive[org * 256 + t];
    if (tid == 0) {
      al[hist] = nb_tok[j];
      // KV slot this beam continues from: the merged prefill + first step left the prompt's K/V in the utterance's first slot
      bs.parent[r0 + j] = (step == 0) ? r0 : r0 + org;
      { int* tr = bs.traj + ((size_t)(b * 256 + step) * MAX_R + j) * 2; tr[0] = nb_tok[j]; tr[1] = org; }      // the search's trajectory (a later call's draft)
      bs.cum[r0 + j] = nb_cum[j];
      rm.tok[r0 + j] = nb_tok[j];
      rm.pos[r0 + j] = npos;
      rm.slot[r0 + j] = r0 + j;                    // decode rows own their KV slot (the merged first step ran on prompt rows)
    }
  }
  if (tid == 0) bs.step_u[b] = step + 1;
  __syncthreads();
  if (tid == 0) publish_step(bs);
  stamp(pf, 8);
}
int launch_beam_step(hipStream_t st, const float* st_max, const float* st_sum, const float* st_val, const int* st_idx,
                     const BeamState& bs, const RowMeta& rm, int B, int P, int ctx, const SampleCfg& cfg, unsigned long long* prof, int n_best, const int* plen) {
  if (cfg.beam > MAX_R || cfg.n_cand > MAX_CAND || cfg.max_new > 256 || ctx > 512 || cfg.n_vocab > (1 << 20)) { set_error("beam_step: config out of range"); return WIS_E_UNSUPPORTED; }
  if (n_best < 1 || n_best > cfg.beam || B * n_best > HP_MAXB) { set_error("beam_step: %d results per utterance at beam %d", n_best, cfg.beam); return WIS_E_ARG; }
  const bool small = cfg.beam * STAT_SUB * cfg.n_cand <= 16 * 256;
  if (plen) {
    if (small) hipLaunchKernelGGL((beam_step_kernel<16, const int*>), dim3(B), dim3(256), 0, st, st_max, st_sum, st_val, st_idx, bs, rm, plen, ctx, cfg, prof, n_best);
    else hipLaunchKernelGGL((beam_step_kernel<32, const int*>), dim3(B), dim3(256), 0, st, st_max, st_sum, st_val, st_idx, bs, rm, plen, ctx, cfg, prof, n_best);
  }
  else if (small) hipLaunchKernelGGL((beam_step_kernel<16, int>), dim3(B), dim3(256), 0, st, st_max, st_sum, st_val, st_idx, bs, rm, P, ctx, cfg, prof, n_best);
  else hipLaunchKernelGGL((beam_step_kernel<32, int>), dim3(B), dim3(256), 0, st, st_max, st_sum, st_val, st_idx, bs, rm, P, ctx, cfg, prof, n_best);
  return WIS_OK;
}

// =======================================================================================
// The step of a SAMPLED decode, in beam_step_kernel's place (include/wis_hip.h states the rule).  grid B, block 256: an utterance's cfg.beam = n
// rows are its n independent samples; wave w draws rows w and w + 4, no barrier inside a wave's work.
//   whole vocabulary (TOPK false): logit_stats_kernel<., true> left each sub-chunk's best PERTURBED entry; the draw is the arg-best of the 64.
//   top-k (TOPK true): the pool is unperturbed, k candidates per sub-chunk (16 entries per lane at most); k selection rounds (wave maximum of the
//     lane-local bests, retire) give the row's top-k in sel_key order, each is perturbed as it is selected (every lane computes the same Philox
//     block: the round's winner is wave-uniform), the best perturbed one is the draw.
// Then one thread per row: score += (x[t] - lse) / T, the token joins bs.alive, a row that drew EOT (or the last step) freezes its result
// (bs.out_len / out_score; its tokens are alive[row][0 .. len)) and raises its own done flag - from then on the row is fed EOT, and EOT is what
// its history collects (the processors of a later step read valid ids there).  All n rows done: the results go to the host block (result j at
// row b n + j), bs.done[b] = 1.  Every path ends in publish_step, as beam_step_kernel's do.
template <bool TOPK, class PT>
__global__ __launch_bounds__(256) void sample_step_kernel(const float* __restrict__ st_max, const float* __restrict__ st_sum,
                                                          const float* __restrict__ st_val, const int* __restrict__ st_idx,
                                                          BeamState bs, RowMeta rm, PT P, SampleCfg cfg, SampleP sp) {
  __shared__ int s_tok[MAX_R]; __shared__ float s_sc[MAX_R]; __shared__ int s_len[MAX_R]; __shared__ int s_ndone;
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int n = cfg.beam, NC = cfg.n_cand, V = cfg.n_vocab, r0 = b * n;
  const int done_b = bs.done[b];
  const int step = bs.step_u[b];
  if (done_b) { if (tid == 0) publish_step(bs); return; }
  const unsigned long long seed = sp.seeds[b];
  const unsigned k0 = (unsigned)seed, k1 = (unsigned)(seed >> 32);
  if (tid == 0) s_ndone = 0;
#pragma unroll
  for (int j2 = 0; j2 < 2; ++j2) {
    const int j = wave + 4 * j2;
    if (j >= n) continue;                      // (wave-uniform)
    const int mrow = r0 + j;
    const float smx = st_max[mrow * STAT_SUB + lane], ssm = st_sum[mrow * STAT_SUB + lane];
    int tok; float xw;
    if constexpr (!TOPK) {
      const size_t e = ((size_t)mrow * STAT_SUB + lane) * 2;
      const float pv = st_val[e], xv = st_val[e + 1];
      int ix = st_idx[e]; ix = ix > V - 1 ? V - 1 : ix;
      const u64 mine = sel_key(pv, ix);
      const u64 best = wave_max_key(mine);
      tok = key_index(best);
      xw = wave_max(mine == best ? xv : -INFINITY);
    } else {
      constexpr int PSL = MAX_CAND;            // 64 sub-chunks x NC <= 16 candidates = 16 entries per lane
      const int total = STAT_SUB * NC;
      u64 pk[PSL]; u64 lbest = 0ull;
#pragma unroll
      for (int u = 0; u < PSL; ++u) {
        const int e = lane + 64 * u, ce = e < total ? e : total - 1;       // clamped address, masked by select
        const float v = st_val[(size_t)mrow * total + ce]; int ix = st_idx[(size_t)mrow * total + ce];
        ix = ix > V - 1 ? V - 1 : ix;
        pk[u] = e < total ? sel_key(v, ix) : 0ull;
        lbest = key_max(lbest, pk[u]);
      }
      u64 pbest = 0ull; xw = -INFINITY;
      for (int rnd = 0; rnd < NC; ++rnd) {
        const u64 wb = wave_max_key(lbest);
        const float x = key_value(wb); int t = wb ? key_index(wb) : 0; t = t < 0 ? 0 : (t > V - 1 ? V - 1 : t);      // (nothing outside the row's noise is ever addressed)
        const unsigned w = sp.noise ? sp.noise[(size_t)mrow * V + t] : philox4x32_10_w0((unsigned)t, (unsigned)step, (unsigned)j, 0u, k0, k1);
        const u64 cand = wb ? sel_key(gumbel_perturb(x, w, sp.T), t) : 0ull;
        xw = cand > pbest ? x : xw; pbest = key_max(pbest, cand);
#pragma unroll
        for (int u = 0; u < PSL; ++u) pk[u] = pk[u] == wb ? 0ull : pk[u];
        u64 tt[PSL];
#pragma unroll
        for (int u = 0; u < PSL; ++u) tt[u] = pk[u];
#pragma unroll
        for (int w2 = PSL / 2; w2 >= 1; w2 >>= 1)
#pragma unroll
          for (int u = 0; u < w2; ++u) tt[u] = key_max(tt[u], tt[u + w2]);
        lbest = tt[0];
      }
      tok = pbest ? key_index(pbest) : V - 1;
    }
    const float M_ = wave_max(smx);
    const float S = wave_sum(smx > -INFINITY ? ssm * __expf(smx - M_) : 0.f);
    const float lse = M_ + logf(S);
    if (lane == 0) { s_tok[j] = tok; s_sc[j] = __fdiv_rn(xw - lse, sp.T); }
  }
  __syncthreads();
  const bool is_last = step + 1 >= cfg.max_new;
  const int npos = prompt_len(P, b) - 1 + step + 1;           // cache positions valid after this step
  if (tid < n) {
    const int row = r0 + tid;
    int rd = bs.row_done[row];
    int tok = cfg.eot;
    if (!rd) {
      tok = s_tok[tid];
      const float cum = bs.cum[row] + s_sc[tid];
      bs.cum[row] = cum;
      const bool eos = tok == cfg.eot;
      if (eos || is_last) {
        const int len = eos ? step : step + 1;   // EOS is not part of the hypothesis
        float s = cum;
        if (cfg.length_penalty != 0.f) s /= powf((float)len, cfg.length_penalty);
        bs.out_len[row] = len; bs.out_score[row] = s; bs.row_done[row] = 1; rd = 1;
      }
    }
    bs.alive[(size_t)row * cfg.max_new + step] = tok;      // (step < max_new: the max_new-th step ends every row)
    bs.parent[row] = (step == 0) ? r0 : row;             // the merged prefill + first step left the prompt's K/V in the utterance's first slot
    { int* tr = bs.traj + ((size_t)(b * 256 + step) * MAX_R + tid) * 2; tr[0] = tok; tr[1] = tid; }
    rm.tok[row] = rd ? cfg.eot : tok;
    rm.pos[row] = npos;
    rm.slot[row] = row;
    s_len[tid] = bs.out_len[row];
    if (rd) atomicAdd(&s_ndone, 1);
  }
  __syncthreads();
  if (s_ndone >= n) {
    for (int j = 0; j < n; ++j) {
      const int row = r0 + j, len = s_len[j];
      const int* src = bs.alive + (size_t)row * cfg.max_new;
      int* hids = hp_out_ids(bs.host) + (size_t)row * cfg.max_new;
      for (int t = tid; t < len; t += 256) { const int v = src[t]; bs.out_ids[(size_t)row * cfg.max_new + t] = v; hids[t] = v; }
      if (tid == 0) { hp_out_len(bs.host)[row] = len; hp_out_score(bs.host)[row] = bs.out_score[row]; }
    }
    if (tid == 0) bs.done[b] = 1;
    __threadfence_system();
    __syncthreads();
    if (tid == 0) { atomicAdd(bs.all_done, 1); publish_step(bs); }
    return;
  }
  if (tid == 0) bs.step_u[b] = step + 1;
  __syncthreads();
  if (tid == 0) publish_step(bs);
}
int launch_sample_step(hipStream_t st, const float* st_max, const float* st_sum, const float* st_val, const int* st_idx,
                       const BeamState& bs, const RowMeta& rm, int B, int P, const SampleCfg& cfg, const SampleP& sp, const int* plen) {
  const bool whole = sp.topk < 0;
  if (cfg.beam < 1 || cfg.beam > MAX_R || B * cfg.beam > HP_MAXB || cfg.max_new > 256 || cfg.n_vocab > (1 << 20) || !sp.seeds || !(sp.T > 0.f) ||
      (whole ? cfg.n_cand != 2 : (sp.topk < 2 || sp.topk > MAX_CAND || cfg.n_cand != sp.topk))) { set_error("sample_step: config out of range"); return WIS_E_UNSUPPORTED; }
  if (plen) {
    if (whole) hipLaunchKernelGGL((sample_step_kernel<false, const int*>), dim3(B), dim3(256), 0, st, st_max, st_sum, st_val, st_idx, bs, rm, plen, cfg, sp);
    else hipLaunchKernelGGL((sample_step_kernel<true, const int*>), dim3(B), dim3(256), 0, st, st_max, st_sum, st_val, st_idx, bs, rm, plen, cfg, sp);
  }
  else if (whole) hipLaunchKernelGGL((sample_step_kernel<false, int>), dim3(B), dim3(256), 0, st, st_max, st_sum, st_val, st_idx, bs, rm, P, cfg, sp);
  else hipLaunchKernelGGL((sample_step_kernel<true, int>), dim3(B), dim3(256), 0, st, st_max, st_sum, st_val, st_idx, bs, rm, P, cfg, sp);
  return WIS_OK;
}

// =======================================================================================
// Draft verification at beam > 1 (generate.hip seed_beam_draft; one utterance): a window of replayed beam steps is queued WITHOUT host round trips; this
// one-workgroup kernel behind every replayed step matches the live set the step produced (tokens + the beams they continued from, as beam_step_kernel
// recorded them in bs.traj) with the draft's entry for that step - as SETS: two candidates whose scores tie to within the summation order of a pass may
// swap beam slots between the draft's search and this one, which changes nothing about the search itself, so live beam j may sit in ANY slot of the draft
// as long as every live beam is found exactly once: (token, origin) of real beam j == (token, origin) of draft node i with the origin translated
// through the previous step's matching.  vs[8 + j] = the draft node live beam j is matched to: the replay reads beam j's logits from that node's row
// (logit_stats_kernel rowmap).  All matched: vs[0] = steps verified so far.  A live beam the draft does not have - or no draft entry left - : the step
// itself stands (its inputs were verified), but nothing behind it does - done = 2 parks the search (beam_step_kernel and the kernels below return at
// their `done` test) until the host resumes it.
// Cache bookkeeping (book = 1: the steps of a window): the window's pass left node (s, i)'s K / V in slot i (draft index), so a live beam's history is a
// path through slots; per live beam the kernel maintains that path - vs[32 + 32 j + t] = the slot that holds beam j's row of window step t, vs[16 + j] =
// the slot that holds everything before the window - by pulling the parent's path and appending the parent's node; kv_gather_kernel below turns the
// paths into the layout ordinary steps expect (slot j = beam j's whole history) once per window.
// vs layout (ints): 0 steps verified | 2 window steps applied | 8.. matching | 16.. pre-window slot | 32.. paths [8][32]
constexpr int VS_PERM = 8, VS_BASE = 16, VS_PATH = 32, VS_PATH_W = 32, VS_INTS = VS_PATH + MAX_R * VS_PATH_W;
__global__ __launch_bounds__(64) void draft_match_kernel(BeamState bs, const int* __restrict__ draft, int n_draft, int k, int* __restrict__ vs, int book) {
  __shared__ int org_r[MAX_R], tok_r[MAX_R], perm_prev[MAX_R], old_base[MAX_R], old_path[MAX_R][VS_PATH_W];
  const int tid = threadIdx.x;
  if (bs.done[0]) return;                    // (uniform: finished, or parked by an earlier step)
  const int s = bs.step_u[0] - 1;            // the step that just completed
  const int t = vs[2];
  if (tid < k) {
    const int* tr = bs.traj + ((size_t)s * MAX_R + tid) * 2;
    tok_r[tid] = tr[0]; org_r[tid] = tr[1]; perm_prev[tid] = vs[VS_PERM + tid]; old_base[tid] = vs[VS_BASE + tid];
  }
  for (int e = tid; e < k * VS_PATH_W; e += 64) old_path[e / VS_PATH_W][e % VS_PATH_W] = vs[VS_PATH + e];
  __syncthreads();
  if (book) {
    for (int e = tid; e < k * VS_PATH_W; e += 64) {
      const int j = e / VS_PATH_W, u = e % VS_PATH_W, pj = org_r[j];
      if (u < t) vs[VS_PATH + e] = old_path[pj][u];
      else if (u == t) vs[VS_PATH + e] = perm_prev[pj];      // the parent's own row of this step sits in the slot of the draft node it was matched to
    }
    if (tid < k) vs[VS_BASE + tid] = old_base[org_r[tid]];
  }
  if (tid == 0) {
    bool ok = s >= 0 && s < n_draft;
    int pn[MAX_R]; unsigned used = 0;
    if (ok) {
      const int* dr = draft + (size_t)s * MAX_R * 2;
      for (int j = 0; j < k && ok; ++j) {
        const int want_org = perm_prev[org_r[j]];
        int hit = -1;
        for (int i = 0; i < k; ++i) if (!((used >> i) & 1u) && dr[2 * i] == tok_r[j] && dr[2 * i + 1] == want_org) { hit = i; break; }
        if (hit < 0) ok = false; else { pn[j] = hit; used |= 1u << hit; }
      }
    }
    if (ok) { for (int j = 0; j < k; ++j) vs[VS_PERM + j] = pn[j]; vs[0] = s + 1; }
    else bs.done[0] = 2;
    if (book) vs[2] = t + 1;
  }
}
int launch_draft_match(hipStream_t st, const BeamState& bs, const int* draft, int n_draft, int beam, int* vstate, int book) {
  hipLaunchKernelGGL(draft_match_kernel, dim3(1), dim3(64), 0, st, bs, draft, n_draft, beam, vstate, book);
  return WIS_OK;
}
// The paths of draft_match_kernel applied to the cache, once per window: slot j becomes beam j's history - positions before the window from slot
// vs[16 + j], window step u (position w0 + u) from slot vs[32 + 32 j + u], for the vs[2] steps the window's replay completed (a parked search included:
// the step that parked it stands).  grid (8 position slices, 2 L), one thread = one 16-byte column chunk of ALL k slots at a position: loads, waits,
// stores - the in-place gather of kv_reorder_kernel with a parent table per position.
__global__ __launch_bounds__(256) void kv_gather_kernel(f16* __restrict__ kc, f16* __restrict__ vc, size_t lstride, const int* __restrict__ vs, const int* __restrict__ done,
                                                        int k, int w0, int ctx, int d) {
  const int lk = blockIdx.y, tid = threadIdx.x;
  const int nwin = vs[2];
  if (done[0] == 1 || nwin <= 0) return;         // finished inside the window (the cache is not read again) / nothing replayed
  f16* cache = ((lk & 1) ? vc : kc) + (size_t)(lk >> 1) * lstride;
  const int c8 = d >> 3, npos = w0 + nwin;
  for (int p = blockIdx.x; p < npos; p += gridDim.x) {
    int par[MAX_R];
#pragma unroll
    for (int j = 0; j < MAX_R; ++j) par[j] = j < k ? (p < w0 ? vs[VS_BASE + j] : vs[VS_PATH + j * VS_PATH_W + (p - w0)]) : j;
    for (int ch = tid; ch < c8; ch += 256) {
      u32x4 v[MAX_R];
#pragma unroll
      for (int j = 0; j < MAX_R; ++j) if (j < k && par[j] != j) v[j] = *reinterpret_cast<const u32x4*>(cache + ((size_t)par[j] * ctx + p) * d + ch * 8);
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#pragma unroll
      for (int j = 0; j < MAX_R; ++j) if (j < k && par[j] != j) *reinterpret_cast<u32x4*>(cache + ((size_t)j * ctx + p) * d + ch * 8) = v[j];
    }
  }
}
int launch_kv_gather(hipStream_t st, f16* kc, f16* vc, size_t layer_stride, int L, const int* vstate, const int* done, int beam, int w0, int ctx, int d) {
  hipLaunchKernelGGL(kv_gather_kernel, dim3(8, 2 * L), dim3(256), 0, st, kc, vc, layer_stride, vstate, done, beam, w0, ctx, d);
  return WIS_OK;
}

// =======================================================================================
// Beam reorder of the self-attention KV cache (CTranslate2 gathers its cache tensors by beam_origin after every step): slot j of
// an utterance becomes a copy of slot parent[j] for every layer and every valid position.  grid (8 position slices, 2 L, B);
// thread = one 16-byte column chunk of ALL the utterance's rows at a position: it loads the k parents' chunks, waits, then
// stores - reads and writes of an address meet only inside one thread, so the permutation is safe in place.  Moving
// beam x positions x d bytes per step (16 MB at position 20, large-v2) buys the self-attention kernel a K/V address that
// depends on nothing it has to load: one fabric round trip per layer instead of two.
// FROM (the long-prompt route, launch_kv_reorder_from): P is a device word per utterance, and only positions [P, P - 1 + step) move - the prompt's positions
// stay in the utterance's first slot (dec_self_attn_long_kernel reads them there), never copied, never reordered
template <bool FROM, class PT>
__global__ __launch_bounds__(256) void kv_reorder_kernel(f16* __restrict__ kc, f16* __restrict__ vc, size_t lstride, const int* __restrict__ parent,
                                                         const int* __restrict__ step_u, const int* __restrict__ done, int k, PT P, int ctx, int d) {
  const int b = blockIdx.z, lk = blockIdx.y, tid = threadIdx.x;
  if (k < 2) return;
  const int r0 = b * k;
  // the three control words are requested together (a `done` test in front of the `parent` loads in front of the `step` load is
  // three dependent round trips before the first cache row moves)
  const int dn = done[b], st = step_u[b];
  const int Pb = prompt_len(P, b);
  int par[MAX_R];
#pragma unroll
  for (int j = 0; j < MAX_R; ++j) par[j] = parent[r0 + (j < k ? j : 0)];
  bool ident = true;
#pragma unroll
  for (int j = 0; j < MAX_R; ++j) { if (j < k) ident = ident & (par[j] == r0 + j); else par[j] = r0 + j; }
  if (dn | (int)ident) return;
  const int npos = Pb - 1 + st;                 // beam_step already counted this step: positions 0 .. npos-1 hold history
  f16* cache = ((lk & 1) ? vc : kc) + (size_t)(lk >> 1) * lstride;
  const int c8 = d >> 3;
  for (int p = (FROM ? Pb : 0) + blockIdx.x; p < npos; p += gridDim.x) {
    for (int ch = tid; ch < c8; ch += 256) {
      u32x4 v[MAX_R];
#pragma unroll
      for (int j = 0; j < MAX_R; ++j) if (j < k && par[j] != r0 + j) v[j] = *reinterpret_cast<const u32x4*>(cache + ((size_t)par[j] * ctx + p) * d + ch * 8);      // (a slot that continues itself moves nothing: neither read nor written)
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");      // every parent chunk is in registers before any row is overwritten
#pragma unroll
      for (int j = 0; j < MAX_R; ++j) if (j < k && par[j] != r0 + j) *reinterpret_cast<u32x4*>(cache + ((size_t)(r0 + j) * ctx + p) * d + ch * 8) = v[j];
    }
  }
}
int launch_kv_reorder(hipStream_t st, f16* kc, f16* vc, size_t layer_stride, int L, const BeamState& bs, int B, int beam, int P, int ctx, int d) {
  if (beam < 2) return WIS_OK;        // greedy: a row always continues itself
  if (beam > MAX_R) { set_error("kv_reorder: beam %d > %d", beam, MAX_R); return WIS_E_UNSUPPORTED; }
  hipLaunchKernelGGL((kv_reorder_kernel<false, int>), dim3(8, 2 * L, B), dim3(256), 0, st, kc, vc, layer_stride, bs.parent, bs.step_u, bs.done, beam, P, ctx, d);
  return WIS_OK;
}
int launch_kv_reorder_from(hipStream_t st, f16* kc, f16* vc, size_t layer_stride, int L, const BeamState& bs, int B, int beam, const int* plen, int ctx, int d) {
  if (beam < 2) return WIS_OK;
  if (beam > MAX_R || !plen) { set_error("kv_reorder_from: beam %d > %d, or no prompt lengths", beam, MAX_R); return WIS_E_UNSUPPORTED; }
  hipLaunchKernelGGL((kv_reorder_kernel<true, const int*>), dim3(8, 2 * L, B), dim3(256), 0, st, kc, vc, layer_stride, bs.parent, bs.step_u, bs.done, beam, plen, ctx, d);
  return WIS_OK;
}

// =======================================================================================
__global__ void lang_probs_kernel(const float* __restrict__ logits, int ld, const int* __restrict__ lang_ids, int n_lang, float* __restrict__ probs) {
  const int b = blockIdx.x, lane = threadIdx.x;
  const float* row = logits + (size_t)b * ld;
  float mx = -INFINITY;
  for (int i = lane; i < n_lang; i += 64) mx = fmaxf(mx, row[lang_ids[i]]);
  mx = wave_max(mx);
  float s = 0.f;
  for (int i = lane; i < n_lang; i += 64) s += __expf(row[lang_ids[i]] - mx);
  s = wave_sum(s);
  for (int i = lane; i < n_lang; i += 64) probs[(size_t)b * n_lang + i] = __expf(row[lang_ids[i]] - mx) / s;
}
int launch_lang_probs(hipStream_t st, const float* logits, int ld, const int* lang_ids, int n_lang, float* probs, int B) {
  hipLaunchKernelGGL(lang_probs_kernel, dim3(B), dim3(64), 0, st, logits, ld, lang_ids, n_lang, probs);
  return WIS_OK;
}

// =======================================================================================
// Phrase-constrained decoding (include/wis_hip.h states the rule), the pre-pass behind rep_rules_kernel when wis_gen_opts_t::phrases is on.
// (The last kernel of the file: every other kernel of the code object lies where it lay before this one existed.)
// grid B*beam (one workgroup per live row), block 256.  WALK: the row's generated history bs.alive[m][0 .. min(step_u[b], max_new)) is followed
// from the root of the flat trie (one int4 record per edge: {token, first child record, children, child ends a phrase}; record 0 = the root's
// pseudo-edge; a node's children are contiguous and ascending by token) - per history token the workgroup scans the node's children 256 per
// round, the thread that finds the token publishes the child's record in LDS (two slots, alternating: two barriers per token).  A history that
// leaves the trie (or is longer than PHRASE_MAX_DEPTH) leaves the row as it is.  MASK: every thread reads its share of the node's children's
// values (and <|endoftext|>'s when the node ends a phrase) into LDS, barrier, ids [0, n_vocab) are filled with -inf (float4 stores between a
// scalar head and tail: the row's alignment is whatever ld makes it), barrier, the kept values go back bit for bit.  Ids >= n_vocab are never
// written.  Rows that share ONE logits row (lr_j == 0: the pass that carries the prompt, every history empty) are masked by the utterance's
// first workgroup alone.  The host validates a set before it reaches the device (model.hip wis_model_set_phrases); the kernel checks every
// child range and token against n_rec / n_vocab again, so no table - a tap caller's included - can make it address outside its buffers.
__global__ __launch_bounds__(256) void phrase_rules_kernel(float* __restrict__ logits, const int* __restrict__ step_u, const int* __restrict__ done,
                                                           const int* __restrict__ alive, const int4* __restrict__ trie, int n_rec, SampleCfg cfg,
                                                           int lr_b, int lr_j, int lr_off) {
  __shared__ int4 s_rec[2];
  __shared__ int s_tok[PHRASE_MAX_CHILDREN];
  __shared__ float s_val[PHRASE_MAX_CHILDREN];
  __shared__ float s_eot;
  const int tid = threadIdx.x, m = blockIdx.x, b = m / cfg.beam, jb = m - b * cfg.beam;
  if (done[b] || n_rec < 1) return;
  if (lr_j == 0 && jb != 0) return;
  int L = step_u[b];
  L = L < cfg.max_new ? L : cfg.max_new;
  if (L < 0 || L > PHRASE_MAX_DEPTH) return;
  const int V = cfg.n_vocab;
  int4 node = trie[0];
  for (int i = 0; i < L; ++i) {
    const int first = node.y, n = node.z;
    if (first < 1 || n < 1 || n > PHRASE_MAX_CHILDREN || first > n_rec - n) return;      // a leaf, or no record range of this table
    const int tk = alive[(size_t)m * cfg.max_new + i];
    if (tid == 0) s_rec[i & 1] = make_int4(-1, 0, 0, 0);
    __syncthreads();
    for (int c = tid; c < n; c += 256) {
      const int4 r = trie[first + c];
      if (r.x == tk && tk >= 0) s_rec[i & 1] = r;      // (ascending tokens: at most one child matches)
    }
    __syncthreads();
    node = s_rec[i & 1];
    if (node.x < 0) return;      // the history is no path of the trie: the row stays as it is
  }
  const int first = node.y, n = node.z, ends = node.w;
  const bool kids = n >= 1;
  if (kids && (first < 1 || n > PHRASE_MAX_CHILDREN || first > n_rec - n)) return;
  if (!kids && !ends) return;      // (a validated set has no such node)
  float* row = logits + (size_t)(b * lr_b + jb * lr_j + lr_off) * cfg.n_vocab_pad;
  if (kids)
    for (int c = tid; c < n; c += 256) {
      int t = trie[first + c].x;
      t = (t >= 0 && t < V) ? t : -1;
      s_tok[c] = t;
      s_val[c] = t >= 0 ? row[t] : 0.f;
    }
  const bool keep_eot = ends != 0 && cfg.eot >= 0 && cfg.eot < V;
  if (keep_eot && tid == 0) s_eot = row[cfg.eot];
  __syncthreads();      // every kept value is read - it lies in LDS - before the fill
  int head = (int)((4u - (unsigned)((reinterpret_cast<uintptr_t>(row) >> 2) & 3u)) & 3u);
  head = head < V ? head : V;
  const int n4 = (V - head) >> 2, tail0 = head + 4 * n4;
  if (tid < head) row[tid] = -INFINITY;
  float4* row4 = reinterpret_cast<float4*>(row + head);
  const float4 ninf4 = make_float4(-INFINITY, -INFINITY, -INFINITY, -INFINITY);
  for (int i = tid; i < n4; i += 256) row4[i] = ninf4;
  if (tid < V - tail0) row[tail0 + tid] = -INFINITY;
  __syncthreads();      // the fill is ahead of the values that go back (workgroup-scope release / acquire, as in rep_rules_kernel)
  if (kids)
    for (int c = tid; c < n; c += 256) { const int t = s_tok[c]; if (t >= 0) row[t] = s_val[c]; }
  if (keep_eot && tid == 0) row[cfg.eot] = s_eot;
}
int launch_phrase_rules(hipStream_t st, float* logits, const BeamState& bs, int B, const SampleCfg& cfg, const int4* trie, int n_rec, int lr_b, int lr_j, int lr_off) {
  if (!trie || n_rec < 1 || n_rec > PHRASE_MAX_RECORDS || cfg.max_new < 1 || cfg.n_vocab < 1 || cfg.n_vocab_pad < cfg.n_vocab) { set_error("phrase_rules: config out of range"); return WIS_E_UNSUPPORTED; }
  hipLaunchKernelGGL(phrase_rules_kernel, dim3(B * cfg.beam), dim3(256), 0, st, logits, bs.step_u, bs.done, bs.alive, trie, n_rec, cfg, lr_b, lr_j, lr_off);
  return WIS_OK;
}

// =======================================================================================
// The phrase mask WITH the in-grammar mass (include/wis_hip.h, THE PHRASE MASS RULE): phrase_rules_kernel's place in the tail when
// wis_gen_opts_t::phrase_mass is on.  (Behind phrase_rules_kernel, the walk duplicated, not shared: that kernel's code stays what it was.)
// Same grid, same walk, same early-outs, same lr_j == 0 rule, the same mask stored the same way - the row it leaves is phrase_rules_kernel's bit
// for bit.  The walk also publishes the INDEX of the record it arrived at (s_at, beside s_rec); the root is record 0.  Between the gather of the
// kept values and the fill, ONE pass over u[t] = row[t] + (bias_all ? bias_all[t] : 0) (+ bias_begin[t] at step 0 with suppress_blank: the form
// logit_stats_kernel gives a row of a call without timestamps) yields M = max u and den = sum exp(u - M) over [0, n_vocab), and MA, num: the same two
// over the allowed ids alone (an LDS bitmap of the node's children and <|endoftext|> at a phrase end, set while the kept values are gathered); the
// mass is (MA - M) + log(num) - log(den) - the rule's log(sum over A of exp(u - M)) - log(den) with the allowed sum taken about its OWN maximum, so
// a share far below fp32's exp range (allowed logits 100 under the row's best) is still a number, not an underflow.
// THE REDUCTION ORDER (tests/phrase_mass_ref.py derives its fp32 bound from it):
//   thread tid owns the ids t = tid (mod 256), ascending, in chunks of 8 (ids base + 256 j + tid, base = 0, 2048, ..; ids >= n_vocab count as -inf).
//   Online, per chunk, for (m, sd) over all ids: cm = max(m, the chunk's 8 values); mm = cm, or 0 when cm is -inf; sd = sd E(m, mm); then for
//   j = 0 .. 7 in order sd += E(v[j], mm); m = cm.   E(a, b) = 1 when a == b, else __expf(a - b) (so exp(-inf) = 0, never -inf - -inf; a +inf
//   maximum counts its own entries as 1 each).  (ma, sn) likewise over the allowed ids (a value that is not allowed counts as -inf and adds 0).
//   Then M = the maximum of the 256 m (exact), every thread scales its sd by E(m, M or 0 when -inf); the 256 values are summed by wave_sum (a
//   balanced pairwise tree over the 64 lanes) and the four waves' sums as (w0 + w1) + (w2 + w3); MA and num likewise.  The two reductions take the
//   same operations in the same order, so a row whose finite entries are all allowed gives MA == M, num == den and a mass of exactly 0.
//   logmass = -inf when M or MA is -inf, else min(0, (MA == M ? 0 : MA - M) + (logf(num) - logf(den))).
// Thread 0 stores the one float at logmass[b lm_ld + record index] (a vector store), only for a row whose cumulative score is finite (cum null: a tap
// caller's rows all count): a dead slot (cum -inf) can repeat a live beam's history, and its row is not the model's row for that history.  A row that
// returns early stores nothing.  n_vocab <= PHRASE_MASS_MAX_VOCAB (the bitmap; launch_logit_stats has the same limit).
constexpr int PHRASE_MASS_MAX_VOCAB = 65536;
__device__ __forceinline__ float mass_term(float a, float b) { return a == b ? 1.f : __expf(a - b); }
__global__ __launch_bounds__(256) void phrase_rules_mass_kernel(float* __restrict__ logits, const int* __restrict__ step_u, const int* __restrict__ done,
                                                                const int* __restrict__ alive, const int4* __restrict__ trie, int n_rec, SampleCfg cfg,
                                                                int lr_b, int lr_j, int lr_off, const float* __restrict__ bias_all,
                                                                const float* __restrict__ bias_begin, const float* __restrict__ cum,
                                                                float* __restrict__ logmass, int lm_ld) {
  __shared__ int4 s_rec[2];
  __shared__ int s_at[2];
  __shared__ int s_tok[PHRASE_MAX_CHILDREN];
  __shared__ float s_val[PHRASE_MAX_CHILDREN];
  __shared__ float s_eot;
  __shared__ unsigned s_bits[PHRASE_MASS_MAX_VOCAB / 32];
  __shared__ float s_red[4][4];
  const int tid = threadIdx.x, m = blockIdx.x, b = m / cfg.beam, jb = m - b * cfg.beam;
  if (done[b] || n_rec < 1) return;
  if (lr_j == 0 && jb != 0) return;
  const int step = step_u[b];
  int L = step;
  L = L < cfg.max_new ? L : cfg.max_new;
  if (L < 0 || L > PHRASE_MAX_DEPTH) return;
  const int V = cfg.n_vocab;
  if (V > PHRASE_MASS_MAX_VOCAB || lm_ld < n_rec) return;      // (the launcher refuses both)
  int4 node = trie[0];
  int at = 0;
  for (int i = 0; i < L; ++i) {
    const int first = node.y, n = node.z;
    if (first < 1 || n < 1 || n > PHRASE_MAX_CHILDREN || first > n_rec - n) return;      // a leaf, or no record range of this table
    const int tk = alive[(size_t)m * cfg.max_new + i];
    if (tid == 0) s_rec[i & 1] = make_int4(-1, 0, 0, 0);
    __syncthreads();
    for (int c = tid; c < n; c += 256) {
      const int4 r = trie[first + c];
      if (r.x == tk && tk >= 0) { s_rec[i & 1] = r; s_at[i & 1] = first + c; }      // (ascending tokens: at most one child matches)
    }
    __syncthreads();
    node = s_rec[i & 1];
    if (node.x < 0) return;      // the history is no path of the trie: the row stays as it is, no slot is written
    at = s_at[i & 1];      // in [1, n_rec): first + c < first + n <= n_rec
  }
  const int first = node.y, n = node.z, ends = node.w;
  const bool kids = n >= 1;
  if (kids && (first < 1 || n > PHRASE_MAX_CHILDREN || first > n_rec - n)) return;
  if (!kids && !ends) return;      // (a validated set has no such node)
  float* row = logits + (size_t)(b * lr_b + jb * lr_j + lr_off) * cfg.n_vocab_pad;
  const bool want = !cum || cum[m] > -INFINITY;      // (workgroup-uniform)
  if (want) {
    for (int w = tid; w < ((V + 31) >> 5); w += 256) s_bits[w] = 0u;
    __syncthreads();
  }
  if (kids)
    for (int c = tid; c < n; c += 256) {
      int t = trie[first + c].x;
      t = (t >= 0 && t < V) ? t : -1;
      s_tok[c] = t;
      s_val[c] = t >= 0 ? row[t] : 0.f;
      if (want && t >= 0) atomicOr(&s_bits[t >> 5], 1u << (t & 31));
    }
  const bool keep_eot = ends != 0 && cfg.eot >= 0 && cfg.eot < V;
  if (keep_eot && tid == 0) { s_eot = row[cfg.eot]; if (want) atomicOr(&s_bits[cfg.eot >> 5], 1u << (cfg.eot & 31)); }
  __syncthreads();      // every kept value is read - it lies in LDS -, the bitmap is whole
  if (want) {
    const bool begin = (step == 0) && cfg.suppress_blank;
    float mx = -INFINITY, sd = 0.f, ma = -INFINITY, sn = 0.f;
    for (int base = 0; base < V; base += 8 * 256) {
      float v[8]; bool ok[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) {      // clamped addresses, masks by select: the eight requests of a stream leave before anything is waited for
        const int idx = base + 256 * j + tid, c = idx < V ? idx : V - 1;
        float x = row[c] + (bias_all ? bias_all[c] : 0.f);
        x = begin ? x + bias_begin[c] : x;
        v[j] = idx < V ? x : -INFINITY;
        ok[j] = (idx < V) & (((s_bits[c >> 5] >> (c & 31)) & 1u) != 0u);
      }
      float cm = mx, ca = ma;
#pragma unroll
      for (int j = 0; j < 8; ++j) { cm = fmaxf(cm, v[j]); ca = fmaxf(ca, ok[j] ? v[j] : -INFINITY); }
      const float mm = cm == -INFINITY ? 0.f : cm, am = ca == -INFINITY ? 0.f : ca;
      sd *= mass_term(mx, mm); sn *= mass_term(ma, am);
#pragma unroll
      for (int j = 0; j < 8; ++j) { sd += mass_term(v[j], mm); sn += ok[j] ? mass_term(v[j], am) : 0.f; }
      mx = cm; ma = ca;
    }
    const int lane = tid & 63, wave = tid >> 6;
    const float wm = wave_max(mx), wa = wave_max(ma);
    if (lane == 0) { s_red[0][wave] = wm; s_red[1][wave] = wa; }
    __syncthreads();
    const float M = fmaxf(fmaxf(s_red[0][0], s_red[0][1]), fmaxf(s_red[0][2], s_red[0][3]));
    const float MA = fmaxf(fmaxf(s_red[1][0], s_red[1][1]), fmaxf(s_red[1][2], s_red[1][3]));
    sd = wave_sum(sd * mass_term(mx, M == -INFINITY ? 0.f : M)); sn = wave_sum(sn * mass_term(ma, MA == -INFINITY ? 0.f : MA));
    if (lane == 0) { s_red[2][wave] = sd; s_red[3][wave] = sn; }
    __syncthreads();
    if (tid == 0) {
      const float den = (s_red[2][0] + s_red[2][1]) + (s_red[2][2] + s_red[2][3]);
      const float num = (s_red[3][0] + s_red[3][1]) + (s_red[3][2] + s_red[3][3]);
      float lm = -INFINITY;      // (M or MA -inf: nothing, or nothing allowed, is finite; otherwise the sums are >= 1: their maximum's own term)
      if (M > -INFINITY && MA > -INFINITY) lm = fminf(0.f, (MA == M ? 0.f : MA - M) + (logf(num) - logf(den)));
      logmass[(size_t)b * lm_ld + at] = lm;
    }
  }
  __syncthreads();      // every read of the row is done before the fill
  int head = (int)((4u - (unsigned)((reinterpret_cast<uintptr_t>(row) >> 2) & 3u)) & 3u);
  head = head < V ? head : V;
  const int n4 = (V - head) >> 2, tail0 = head + 4 * n4;
  if (tid < head) row[tid] = -INFINITY;
  float4* row4 = reinterpret_cast<float4*>(row + head);
  const float4 ninf4 = make_float4(-INFINITY, -INFINITY, -INFINITY, -INFINITY);
  for (int i = tid; i < n4; i += 256) row4[i] = ninf4;
  if (tid < V - tail0) row[tail0 + tid] = -INFINITY;
  __syncthreads();      // the fill is ahead of the values that go back
  if (kids)
    for (int c = tid; c < n; c += 256) { const int t = s_tok[c]; if (t >= 0) row[t] = s_val[c]; }
  if (keep_eot && tid == 0) row[cfg.eot] = s_eot;
}
int launch_phrase_rules_mass(hipStream_t st, float* logits, const BeamState& bs, int B, const SampleCfg& cfg, const int4* trie, int n_rec, int lr_b, int lr_j, int lr_off,
                             const float* bias_all, const float* bias_begin, float* logmass, int lm_ld) {
  if (!trie || n_rec < 1 || n_rec > PHRASE_MAX_RECORDS || cfg.max_new < 1 || cfg.n_vocab < 1 || cfg.n_vocab_pad < cfg.n_vocab || cfg.n_vocab > PHRASE_MASS_MAX_VOCAB ||
      !bias_begin || !logmass || lm_ld < n_rec) { set_error("phrase_rules_mass: config out of range"); return WIS_E_UNSUPPORTED; }
  hipLaunchKernelGGL(phrase_rules_mass_kernel, dim3(B * cfg.beam), dim3(256), 0, st, logits, bs.step_u, bs.done, bs.alive, trie, n_rec, cfg, lr_b, lr_j, lr_off,
                     bias_all, bias_begin, bs.cum, logmass, lm_ld);
  return WIS_OK;
}

// The in-grammar mass of finished results (THE PHRASE MASS RULE): one wave per (utterance, result), launched once behind the search.  Result r = b n + i:
// ids[r id_ld .. + len[r]) is walked from the root - 64 children per round, the matching lane found by ballot - and the slots
// logmass[b lm_ld + record] of the len + 1 nodes of the path, the root first, are added in path order in fp32 (a NaN slot - one the search never
// wrote - propagates).  -inf: a filler (score not above -inf), a length outside [0, PHRASE_MAX_DEPTH], a token that is no child, a record range
// outside the table, a path that does not end a phrase.  score may be null.  Lane 0 stores out[r].
__global__ __launch_bounds__(64) void phrase_mass_gather_kernel(const int* __restrict__ ids, const int* __restrict__ len, const float* __restrict__ score,
                                                                const int4* __restrict__ trie, int n_rec, const float* __restrict__ logmass, int lm_ld,
                                                                int n, int id_ld, float* __restrict__ out) {
  const int r = blockIdx.x, b = r / n, lane = threadIdx.x;
  const int L = len[r];
  bool path = n_rec >= 1 && lm_ld >= n_rec && L >= 0 && L <= PHRASE_MAX_DEPTH && L <= id_ld && !(score && !(score[r] > -INFINITY));
  float acc = 0.f;
  if (path) {
    int4 node = trie[0];
    acc = logmass[(size_t)b * lm_ld];
    for (int i = 0; i < L && path; ++i) {
      const int first = node.y, nn = node.z, tk = ids[(size_t)r * id_ld + i];
      int found = -1;
      if (first >= 1 && nn >= 1 && nn <= PHRASE_MAX_CHILDREN && first <= n_rec - nn && tk >= 0)
        for (int c0 = 0; c0 < nn && found < 0; c0 += 64) {
          const int c = c0 + lane;
          const unsigned long long hit = __ballot(c < nn && trie[first + (c < nn ? c : 0)].x == tk);
          if (hit) found = first + c0 + (__ffsll((long long)hit) - 1);
        }
      path = found >= 0;
      if (path) { node = trie[found]; acc += logmass[(size_t)b * lm_ld + found]; }
    }
    path = path && node.w != 0;
  }
  if (lane == 0) out[r] = path ? acc : -INFINITY;
}
int launch_phrase_mass_gather(hipStream_t st, const int* ids, const int* len, const float* score, const int4* trie, int n_rec, const float* logmass, int lm_ld,
                              int B, int n, int id_ld, float* out) {
  if (!ids || !len || !trie || !logmass || !out || n_rec < 1 || n_rec > PHRASE_MAX_RECORDS || lm_ld < n_rec || B < 1 || n < 1 || id_ld < 1) { set_error("phrase_mass_gather: config out of range"); return WIS_E_UNSUPPORTED; }
  hipLaunchKernelGGL(phrase_mass_gather_kernel, dim3(B * n), dim3(64), 0, st, ids, len, score, trie, n_rec, logmass, lm_ld, n, id_ld, out);
  return WIS_OK;
}

// =======================================================================================
// Hotword boosting (include/wis_hip.h, THE HOTWORD RULE), the pre-pass behind rep_rules_kernel when wis_gen_opts_t::hotwords is on.
// (The last kernel of the file: every other kernel of the code object lies where it lay before this one existed.)
// grid B*beam (one workgroup per live row), block 256.  The set is a flat trie in phrase_rules_kernel's record format.
// HISTORY: the last K = min(L, 31) generated tokens of the row go to LDS (an id outside [0, n_vocab) as -1: it breaks every suffix that holds it).
// WALK: thread k <= K follows suffix S_k = the last k tokens from the root on its own - the 32 walks are independent; a node's children ascend by
//   token, so each token is a binary search over the node's child range (<= 12 dependent loads) - and leaves the child range of the node it ends
//   at in LDS ({0, 0}: the suffix is no path, or ends at a leaf).  S_0 is the root.  Most suffixes die at their first token.
// BOOST: the workgroup goes through the <= 32 end nodes, 256 children per round; per child token t the thread sets t's bit in an LDS bitmap
//   (65536 bits = 8 KB, the first n_vocab cleared and used) with atomicOr, and the thread that found the bit clear does row[t] = row[t] + boost - ONE fp32 addition per token of the boost
//   set however many suffixes name it, and no two threads ever touch the same element.  <|endoftext|> is never boosted; "ends an entry" flags
//   are not read.  Ids >= n_vocab are never written.
// ctl = {boost's bits, n_rec} in device memory (the handle's control words: the boost is written ahead of every call's steps, the record count
// with the set - a captured step carries the address, never either value, so one step graph serves every boost and every set).
// Rows that share ONE logits row (lr_j == 0: the pass that carries the prompt, every history empty) are boosted by the utterance's first
// workgroup alone.  Nothing happens for a finished utterance or on the measurement convention's forced-EOT step (as in rep_rules_kernel).
// The host validates a set before it reaches the device; the kernel checks every child range and token against n_rec / n_vocab again.
// The SampleCfg fields it reads lead the argument list as scalars behind the pointers (kernarg preload, build.py).
constexpr int HOTWORD_MAX_VOCAB = 65536, HOTWORD_SUFFIXES = 32;
__global__ __launch_bounds__(256) void hotword_rules_kernel(float* __restrict__ logits, const int* __restrict__ step_u, const int* __restrict__ done,
                                                            const int* __restrict__ alive, const int4* __restrict__ trie, const int* __restrict__ ctl,
                                                            int beam, int max_new, int fixed_new, int n_vocab, int n_vocab_pad, int eot,
                                                            int lr_b, int lr_j, int lr_off) {
  __shared__ int s_h[HOTWORD_SUFFIXES];
  __shared__ int2 s_end[HOTWORD_SUFFIXES];
  __shared__ unsigned s_bits[HOTWORD_MAX_VOCAB / 32];
  const int tid = threadIdx.x, m = blockIdx.x, b = m / beam, jb = m - b * beam;
  const float boost = __int_as_float(ctl[0]);
  const int n_rec = ctl[1];
  if (done[b] || n_rec < 1 || n_rec > PHRASE_MAX_RECORDS) return;
  if (lr_j == 0 && jb != 0) return;
  int L = step_u[b];
  L = L < max_new ? L : max_new;
  if (L < 0 || (fixed_new > 0 && L >= fixed_new)) return;
  const int V = n_vocab;
  if (V > HOTWORD_MAX_VOCAB) return;      // (the launcher refuses it)
  const int K = L < HOTWORD_SUFFIXES - 1 ? L : HOTWORD_SUFFIXES - 1;
  if (tid < K) {
    const int tk = alive[(size_t)m * max_new + (L - K + tid)];
    s_h[tid] = (tk >= 0 && tk < V) ? tk : -1;
  }
  for (int i = tid; i < (V + 31) >> 5; i += 256) s_bits[i] = 0u;
  __syncthreads();
  if (tid <= K) {
    int4 node = trie[0];
    bool live = true;
    for (int i = K - tid; i < K && live; ++i) {
      const int first = node.y, n = node.z, tk = s_h[i];
      live = tk >= 0 && first >= 1 && n >= 1 && n <= PHRASE_MAX_CHILDREN && first <= n_rec - n;
      if (!live) break;
      int lo = 0, hi = n;      // the first child whose token is >= tk
      while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (trie[first + mid].x < tk) lo = mid + 1; else hi = mid;
      }
      live = lo < n;
      if (live) { node = trie[first + lo]; live = node.x == tk; }
    }
    const int first = node.y, n = node.z;
    live = live && first >= 1 && n >= 1 && n <= PHRASE_MAX_CHILDREN && first <= n_rec - n;
    s_end[tid] = live ? make_int2(first, n) : make_int2(0, 0);
  }
  __syncthreads();
  float* row = logits + (size_t)(b * lr_b + jb * lr_j + lr_off) * n_vocab_pad;
  for (int k = 0; k <= K; ++k) {
    const int2 e = s_end[k];
    for (int c = tid; c < e.y; c += 256) {
      const int t = trie[e.x + c].x;
      if (t < 0 || t >= V || t == eot) continue;
      const unsigned bit = 1u << (t & 31);
      if (!(atomicOr(&s_bits[t >> 5], bit) & bit)) row[t] = __fadd_rn(row[t], boost);
    }
  }
}
int launch_hotword_rules(hipStream_t st, float* logits, const BeamState& bs, int B, const SampleCfg& cfg, const int4* trie, const int* ctl,
                         int lr_b, int lr_j, int lr_off) {
  if (!trie || !ctl || cfg.max_new < 1 || cfg.max_new > 256 || cfg.n_vocab < 1 || cfg.n_vocab_pad < cfg.n_vocab ||
      cfg.n_vocab > HOTWORD_MAX_VOCAB) { set_error("hotword_rules: config out of range"); return WIS_E_UNSUPPORTED; }
  hipLaunchKernelGGL(hotword_rules_kernel, dim3(B * cfg.beam), dim3(256), 0, st, logits, bs.step_u, bs.done, bs.alive, trie, ctl, cfg.beam, cfg.max_new,
                     cfg.fixed_new, cfg.n_vocab, cfg.n_vocab_pad, cfg.eot, lr_b, lr_j, lr_off);
  return WIS_OK;
}

}  // namespace wis
