// prefill.hip — the one-pass prefix route of a long prompt (generate.hip seed_prefill_onepass): the prompt positions 0 .. Np - 1 of every utterance as
// M = B Np <= PF_MAX_ROWS rows through every decoder layer in ONE pass, GEMM-shaped.  Row m = b Np + i is position i of utterance b; every activation is
// row-major ([M][d] fp32 residual stream, f16 operands), nothing here reads or writes the step's fragment images.
//
//   prefill_embed_kernel       token + position rows -> x (fp32)
//   prefill_rowstat_kernel     one wave per row: LayerNorm mean / rstd of the fp32 row and its f16 copy (the operand of the LayerNorm-folded projections)
//   prefill_proj_kernel        Y = epi(A W^T): A f16 [M][K] through LDS in K chunks of 128, W read IN PLACE from the decoder's fragment image
//                              ([N/16][K/32][64 lanes][8 f16], dec_kernels.hip pack_gemv_kernel) - one 1 KiB request per k-step, straight into the MFMA's A operand
//   prefill_self_attn_kernel   causal attention of 16 queries over keys 0 .. i of the same pass (read where the QKV epilogue put them: the cache slot)
//   prefill_cross_attn_kernel  16 queries over the utterance's T encoder keys, the keys split over the four waves of the workgroup, flash-style
//
// THE SPLIT of the projection.  A workgroup owns ONE 16-column tile and a run of row blocks; its four waves share the tile's weight fragment of a k-step and take
// every fourth row block of the run each (at most PF_WAVE_RB accumulators per wave).  grid = (N / 16, row runs): the runs are what spreads a narrow N - at
// N = 1280 (80 tiles) three runs make 240 workgroups, at N = 3840 / 5120 one run covers every row block.  It is a ROW-BLOCK split, not a K split: no partial
// sums leave a workgroup, so there is no ticket, no scratch and one summation order per element whatever the grid.  A run streams its tile's fragments from
// memory once; the second and third run of a tile find them in L2.
// LDS: one chunk of the run's rows, [rows][128 + 8] f16 (the pad spreads the sixteen rows of a B-fragment read over all 64 banks): at most fifteen row blocks (63.75 KiB), two
// workgroups per CU; 256 rows go as two runs of eight.  The next chunk's rows and weight fragments are requested into registers before the MFMAs of the current one.
//
// v_mfma_f32_16x16x32_f16 everywhere: A = 16 weight rows (or keys, or V^T rows) x 32 k, B = 16 activation rows (queries) x 32 k, D[4 g + j][lane & 15] on
// lane 16 g + (lane & 15).  In the attention kernels the scores of two 16-key tiles ARE the B operand of the P.V product: lane group g holds keys 4 g .. 4 g + 3
// of each tile, and the V^T operand is gathered in that key order - no transpose of P through LDS.
#include <algorithm>
#include "common.hpp"
#include "kernels.hpp"

namespace wis {

constexpr int PF_KC = 128, PF_PITCH = PF_KC + 8, PF_WAVE_RB = 4, PF_RUN_MAX = 15;

__global__ __launch_bounds__(256) void prefill_embed_kernel(const f16* __restrict__ emb, const f16* __restrict__ pos_emb, const int* __restrict__ tok, int M, int Np, int d,
                                                            float* __restrict__ x) {
  const int m = blockIdx.x;
  if (m >= M) return;
  const f16* e = emb + (size_t)tok[m] * d; const f16* pe = pos_emb + (size_t)(m % Np) * d;
  for (int k = threadIdx.x; k < d; k += 256) x[(size_t)m * d + k] = (float)e[k] + (float)pe[k];
}

// mean and 1 / sqrt(var + 1e-5) of row m (two passes over the row in registers' reach: the variance about the mean), and the row as f16
__global__ __launch_bounds__(64) void prefill_rowstat_kernel(const float* __restrict__ x, int M, int d, float* __restrict__ stat, f16* __restrict__ xh) {
  const int m = blockIdx.x, lane = threadIdx.x;
  if (m >= M) return;
  const float* r = x + (size_t)m * d;
  float s = 0.f;
  for (int k = lane; k < d; k += 64) { const float v = r[k]; s += v; xh[(size_t)m * d + k] = (f16)v; }
  const float mu = wave_sum(s) / (float)d;
  float q = 0.f;
  for (int k = lane; k < d; k += 64) { const float v = r[k] - mu; q += v * v; }
  const float var = wave_sum(q) / (float)d;
  if (lane == 0) { stat[2 * m] = mu; stat[2 * m + 1] = 1.0f / sqrtf(var + 1e-5f); }
}

// ---- the projection -------------------------------------------------------------------------------------------------------------------------------------------
template <int EPI>
__global__ __launch_bounds__(256) void prefill_proj_kernel(PrefillProjP p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char pf_lds[];
  f16* sa = reinterpret_cast<f16*>(pf_lds);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, g = lane >> 4, c = lane & 15;
  const int nt = blockIdx.x, M = p.M, K = p.K;
  const int MB = cdiv(M, 16), run = cdiv(MB, (int)gridDim.y);
  const int mb0 = blockIdx.y * run, nrb = min(run, MB - mb0);      // this workgroup's row blocks [mb0, mb0 + nrb)
  if (nrb <= 0) return;                                            // (uniform: a last run that is empty)
  const int rows = nrb * 16, row0 = mb0 * 16;
  const int nmine = wave < nrb ? (nrb - wave + 3) / 4 : 0;         // row blocks wave, wave + 4, ... of the run
  const int nch = K / PF_KC, ksteps = K / 32;
  const u32x4* wp = reinterpret_cast<const u32x4*>(p.Wp) + (size_t)nt * ksteps * 64 + lane;
  // staging: piece i of the chunk = row i / 16, 16-byte column i % 16; thread tid takes pieces tid, tid + 256, ... (PF_WAVE_RB * 4 at most)
  u32x4 areg[PF_WAVE_RB * 4]; u32x4 wcur[4], wnext[4];
  auto request = [&](int ch) {
#pragma unroll
    for (int i = 0; i < PF_WAVE_RB * 4; ++i) {
      const int piece = tid + 256 * i, r = piece >> 4, col = piece & 15;
      areg[i] = u32x4{0u, 0u, 0u, 0u};
      if (r < rows && row0 + r < M) areg[i] = *reinterpret_cast<const u32x4*>(p.A + (size_t)(row0 + r) * K + ch * PF_KC + col * 8);
    }
#pragma unroll
    for (int s = 0; s < 4; ++s) wnext[s] = wp[(size_t)(ch * 4 + s) * 64];
  };
  f32x4 acc[PF_WAVE_RB];
#pragma unroll
  for (int e = 0; e < PF_WAVE_RB; ++e) acc[e] = f32x4{0.f, 0.f, 0.f, 0.f};
  request(0);
  for (int ch = 0; ch < nch; ++ch) {
#pragma unroll
    for (int i = 0; i < PF_WAVE_RB * 4; ++i) {
      const int piece = tid + 256 * i, r = piece >> 4, col = piece & 15;
      if (r < rows) *reinterpret_cast<u32x4*>(sa + r * PF_PITCH + col * 8) = areg[i];
    }
#pragma unroll
    for (int s = 0; s < 4; ++s) wcur[s] = wnext[s];
    __syncthreads();
    if (ch + 1 < nch) request(ch + 1);
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      const f16x8 wa = *reinterpret_cast<const f16x8*>(&wcur[s]);
#pragma unroll
      for (int e = 0; e < PF_WAVE_RB; ++e) {
        if (e < nmine) {
          const f16x8 xb = *reinterpret_cast<const f16x8*>(sa + ((wave + 4 * e) * 16 + c) * PF_PITCH + s * 32 + g * 8);
          acc[e] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wa, xb, acc[e], 0, 0, 0);
        }
      }
    }
    __syncthreads();
  }
  // epilogue: lane holds columns n .. n + 3 of row m
  const int n = 16 * nt + 4 * g;
  const float4 bias = *reinterpret_cast<const float4*>(p.bias + n);
  float4 cs = make_float4(0.f, 0.f, 0.f, 0.f);
  if (EPI != PF_EPI_RESID) cs = *reinterpret_cast<const float4*>(p.csum + n);
#pragma unroll
  for (int e = 0; e < PF_WAVE_RB; ++e) {
    if (e >= nmine) continue;
    const int m = row0 + (wave + 4 * e) * 16 + c;
    if (m >= M) continue;
    float4 s = make_float4(acc[e][0], acc[e][1], acc[e][2], acc[e][3]);
    if (EPI != PF_EPI_RESID) {      // the LayerNorm fold: rs (W' x - mu c) + b'
      const float mu = p.stat[2 * m], rs = p.stat[2 * m + 1];
      s.x = rs * (s.x - mu * cs.x); s.y = rs * (s.y - mu * cs.y); s.z = rs * (s.z - mu * cs.z); s.w = rs * (s.w - mu * cs.w);
    }
    s.x += bias.x; s.y += bias.y; s.z += bias.z; s.w += bias.w;
    if (EPI == PF_EPI_RESID) {
      float4* y = reinterpret_cast<float4*>(p.y32 + (size_t)m * p.N + n);
      const float4 r = *y;
      *y = make_float4(r.x + s.x, r.y + s.y, r.z + s.z, r.w + s.w);
      continue;
    }
    if (EPI == PF_EPI_LN_GELU) { s.x = gelu_erf(s.x); s.y = gelu_erf(s.y); s.z = gelu_erf(s.z); s.w = gelu_erf(s.w); }
    const f16x4 h = {(f16)s.x, (f16)s.y, (f16)s.z, (f16)s.w};
    if (EPI == PF_EPI_QKV) {      // q rows; K / V into slot (m / Np) sstride at position m % Np
      const int d = p.d;
      if (n < d) { *reinterpret_cast<f16x4*>(p.y16 + (size_t)m * d + n) = h; continue; }
      const bool isk = n < 2 * d;
      f16* dst = (isk ? p.kc : p.vc) + ((size_t)(m / p.Np) * p.sstride * p.ctx + (m % p.Np)) * d + (n - (isk ? d : 2 * d));
      *reinterpret_cast<f16x4*>(dst) = h;
      continue;
    }
    *reinterpret_cast<f16x4*>(p.y16 + (size_t)m * p.N + n) = h;
  }
}

int launch_prefill_proj(hipStream_t st, const PrefillProjP& p) {
  if (p.M < 1 || p.M > PF_MAX_ROWS || p.N < 16 || p.N % 16 || p.K < PF_KC || p.K % PF_KC) { set_error("prefill_proj: bad shape M=%d N=%d K=%d (M <= %d, N %% 16 == 0, K %% %d == 0)", p.M, p.N, p.K, PF_MAX_ROWS, PF_KC); return WIS_E_ARG; }
  if (!p.A || !p.Wp || !p.bias || (p.epi != PF_EPI_RESID && (!p.csum || !p.stat)) || (p.epi == PF_EPI_RESID ? !p.y32 : !p.y16)) { set_error("prefill_proj: missing operand"); return WIS_E_ARG; }
  if (p.epi == PF_EPI_QKV && (!p.kc || !p.vc || p.N != 3 * p.d || p.Np < 1 || p.M % p.Np || p.Np > p.ctx || p.sstride < 1)) { set_error("prefill_proj: bad QKV epilogue (N = 3 d, M = B Np, Np <= ctx)"); return WIS_E_ARG; }
  const int MB = cdiv(p.M, 16), tiles = p.N / 16;
  // row runs: enough of them to put a workgroup on (nearly) every CU where the tiles alone do not, never more than the row blocks; a run holds at most PF_RUN_MAX (its chunk stays inside 64 KiB of LDS)
  int runs = std::min(MB, std::max(1, 256 / tiles));
  runs = std::max(runs, cdiv(MB, PF_RUN_MAX));
  const int run = cdiv(MB, runs);
  const size_t lds = (size_t)run * 16 * PF_PITCH * 2;
  const dim3 grid(tiles, runs), block(256);
  switch (p.epi) {
    case PF_EPI_QKV: hipLaunchKernelGGL(prefill_proj_kernel<PF_EPI_QKV>, grid, block, lds, st, p); break;
    case PF_EPI_RESID: hipLaunchKernelGGL(prefill_proj_kernel<PF_EPI_RESID>, grid, block, lds, st, p); break;
    case PF_EPI_LN_F16: hipLaunchKernelGGL(prefill_proj_kernel<PF_EPI_LN_F16>, grid, block, lds, st, p); break;
    case PF_EPI_LN_GELU: hipLaunchKernelGGL(prefill_proj_kernel<PF_EPI_LN_GELU>, grid, block, lds, st, p); break;
    default: set_error("prefill_proj: epilogue %d (0 QKV, 1 residual, 2 LayerNorm-folded f16, 3 LayerNorm-folded GELU)", p.epi); return WIS_E_ARG;
  }
  return WIS_OK;
}

int launch_prefill_embed(hipStream_t st, const f16* emb, const f16* pos_emb, const int* tok, int M, int Np, int d, float* x) {
  hipLaunchKernelGGL(prefill_embed_kernel, dim3(M), dim3(256), 0, st, emb, pos_emb, tok, M, Np, d, x);
  return WIS_OK;
}
int launch_prefill_rowstat(hipStream_t st, const float* x, int M, int d, float* stat, f16* xh) {
  hipLaunchKernelGGL(prefill_rowstat_kernel, dim3(M), dim3(64), 0, st, x, M, d, stat, xh);
  return WIS_OK;
}

// ---- causal self-attention of the prefix ------------------------------------------------------------------------------------------------------------------------
// grid (query blocks, H, B), one wave: queries i = 16 qb + (lane & 15) of utterance b against keys 0 .. 16 qb + 15 (a key above the query's own position is
// masked).  q f16 [B Np][d] (scaled by the projection); K / V in cache slot b sstride, [ctx][d].  All scores of the block live in registers (Np <= 256: sixteen
// tiles of four), so the softmax is two-pass and exact about the row maximum; V goes through LDS 32 keys at a time for the gather in P's key order.
__global__ __launch_bounds__(64) void prefill_self_attn_kernel(const f16* __restrict__ q, const f16* __restrict__ kc, const f16* __restrict__ vc, f16* __restrict__ out,
                                                               int Np, int H, int ctx, int sstride) {
  constexpr int VP = 72;      // V tile pitch (f16): rows 4 g apart land 16 banks apart
  __shared__ __attribute__((aligned(16))) f16 sv[32 * VP];
  const int lane = threadIdx.x, g = lane >> 4, c = lane & 15;
  const int qb = blockIdx.x, h = blockIdx.y, b = blockIdx.z, d = 64 * H;
  const int i = 16 * qb + c, iq = min(i, Np - 1);
  const f16* kb = kc + (size_t)b * sstride * ctx * d + h * 64;
  const f16* vb = vc + (size_t)b * sstride * ctx * d + h * 64;
  const f16* qr = q + ((size_t)b * Np + iq) * d + h * 64;
  const f16x8 q0 = *reinterpret_cast<const f16x8*>(qr + 8 * g), q1 = *reinterpret_cast<const f16x8*>(qr + 32 + 8 * g);
  float s[16][4];
  float mx = -INFINITY;
#pragma unroll
  for (int kt = 0; kt < 16; ++kt) {
#pragma unroll
    for (int j = 0; j < 4; ++j) s[kt][j] = -INFINITY;
    if (kt <= qb) {
      const f16* kr = kb + (size_t)min(16 * kt + c, Np - 1) * d;
      const f16x8 k0 = *reinterpret_cast<const f16x8*>(kr + 8 * g), k1 = *reinterpret_cast<const f16x8*>(kr + 32 + 8 * g);
      f32x4 a = {0.f, 0.f, 0.f, 0.f};
      a = __builtin_amdgcn_mfma_f32_16x16x32_f16(k0, q0, a, 0, 0, 0);
      a = __builtin_amdgcn_mfma_f32_16x16x32_f16(k1, q1, a, 0, 0, 0);
#pragma unroll
      for (int j = 0; j < 4; ++j) { s[kt][j] = (16 * kt + 4 * g + j <= i) ? a[j] : -INFINITY; mx = fmaxf(mx, s[kt][j]); }
    }
  }
  mx = fmaxf(mx, __shfl_xor(mx, 16)); mx = fmaxf(mx, __shfl_xor(mx, 32));      // (key 0 is never masked: mx is finite)
  float sum = 0.f;
  f32x4 o[4];
#pragma unroll
  for (int dt = 0; dt < 4; ++dt) o[dt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int kp = 0; kp < 8; ++kp) {
    if (2 * kp > qb) continue;
    f16x8 pb;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float p0 = __expf(s[2 * kp][j] - mx), p1 = __expf(s[2 * kp + 1][j] - mx);
      sum += p0 + p1; pb[j] = (f16)p0; pb[4 + j] = (f16)p1;
    }
    __syncthreads();      // (one wave: the previous tile's gathers are done)
#pragma unroll
    for (int t = 0; t < 4; ++t) {      // 32 keys x 64 values: piece = key (lane / 8) + 8 t, 16-byte column lane % 8
      const int key = (lane >> 3) + 8 * t, col = lane & 7;
      *reinterpret_cast<u32x4*>(sv + key * VP + col * 8) = *reinterpret_cast<const u32x4*>(vb + (size_t)min(32 * kp + key, Np - 1) * d + col * 8);
    }
    __syncthreads();
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) {
      f16x8 va;
#pragma unroll
      for (int j = 0; j < 4; ++j) { va[j] = sv[(4 * g + j) * VP + 16 * dt + c]; va[4 + j] = sv[(16 + 4 * g + j) * VP + 16 * dt + c]; }
      o[dt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(va, pb, o[dt], 0, 0, 0);
    }
  }
  sum += __shfl_xor(sum, 16); sum += __shfl_xor(sum, 32);
  if (i >= Np) return;
  const float inv = 1.0f / sum;
  f16* orow = out + ((size_t)b * Np + i) * d + h * 64;
#pragma unroll
  for (int dt = 0; dt < 4; ++dt) {
    const f16x4 hv = {(f16)(o[dt][0] * inv), (f16)(o[dt][1] * inv), (f16)(o[dt][2] * inv), (f16)(o[dt][3] * inv)};
    *reinterpret_cast<f16x4*>(orow + 16 * dt + 4 * g) = hv;
  }
}

int launch_prefill_self_attn(hipStream_t st, const f16* q, const f16* kc, const f16* vc, f16* out, int B, int Np, int H, int ctx, int sstride) {
  if (!q || !kc || !vc || !out || B < 1 || H < 1 || Np < 1 || Np > PF_MAX_ROWS || Np > ctx || sstride < 1) { set_error("prefill_self_attn: bad argument (1 <= Np <= min(%d, ctx))", PF_MAX_ROWS); return WIS_E_ARG; }
  hipLaunchKernelGGL(prefill_self_attn_kernel, dim3(cdiv(Np, 16), H, B), dim3(64), 0, st, q, kc, vc, out, Np, H, ctx, sstride);
  return WIS_OK;
}

// ---- cross-attention of the prefix ------------------------------------------------------------------------------------------------------------------------------
// grid (query blocks, H, B), four waves: wave w takes the 32-key steps w, w + 4, ... of the utterance's T keys for the block's 16 queries, with running
// maximum / sum / output (the next step's K and V^T fragments requested ahead of the current step's MFMAs); the four partial results meet in LDS and wave 0
// writes the rows.  kx [B][H][8][T][8] holds exactly T keys (the index is clamped, the score masked); vt [B][H][64][Tpad] is read up to the end of the last step.
__global__ __launch_bounds__(256) void prefill_cross_attn_kernel(const f16* __restrict__ q, const f16* __restrict__ kx, const f16* __restrict__ vt, f16* __restrict__ out,
                                                                 int Np, int H, int T, int Tpad) {
  __shared__ float so[4][16][68];      // per wave: 64 output columns, maximum, sum of every query
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, g = lane >> 4, c = lane & 15;
  const int qb = blockIdx.x, h = blockIdx.y, b = blockIdx.z, d = 64 * H;
  const int i = 16 * qb + c, iq = min(i, Np - 1);
  const f16* qr = q + ((size_t)b * Np + iq) * d + h * 64;
  const f16x8 q0 = *reinterpret_cast<const f16x8*>(qr + 8 * g), q1 = *reinterpret_cast<const f16x8*>(qr + 32 + 8 * g);
  const f16* kh = kx + ((size_t)b * H + h) * 64 * T;
  const f16* vh = vt + ((size_t)b * H + h) * 64 * Tpad;
  const int nsteps = cdiv(T, 32);
  u32x4 kf[4], kn[4]; u32x4 vf[4], vn[4];
  auto request = [&](int st_) {
    const int key0 = 32 * st_;
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      const int key = min(key0 + 16 * t + c, T - 1);
      kn[2 * t] = *reinterpret_cast<const u32x4*>(kh + ((size_t)g * T + key) * 8);
      kn[2 * t + 1] = *reinterpret_cast<const u32x4*>(kh + ((size_t)(4 + g) * T + key) * 8);
    }
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) {
      const f16* vr = vh + (size_t)(16 * dt + c) * Tpad + key0 + 4 * g;
      const uint2 lo = *reinterpret_cast<const uint2*>(vr), hi = *reinterpret_cast<const uint2*>(vr + 16);
      vn[dt] = u32x4{lo.x, lo.y, hi.x, hi.y};
    }
  };
  float mx = -INFINITY, sum = 0.f;
  f32x4 o[4];
#pragma unroll
  for (int dt = 0; dt < 4; ++dt) o[dt] = f32x4{0.f, 0.f, 0.f, 0.f};
  if (wave < nsteps) request(wave);
  for (int st_ = wave; st_ < nsteps; st_ += 4) {
#pragma unroll
    for (int t = 0; t < 4; ++t) { kf[t] = kn[t]; vf[t] = vn[t]; }
    if (st_ + 4 < nsteps) request(st_ + 4);
    float sc[2][4]; float tm = -INFINITY;
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      f32x4 a = {0.f, 0.f, 0.f, 0.f};
      a = __builtin_amdgcn_mfma_f32_16x16x32_f16(*reinterpret_cast<const f16x8*>(&kf[2 * t]), q0, a, 0, 0, 0);
      a = __builtin_amdgcn_mfma_f32_16x16x32_f16(*reinterpret_cast<const f16x8*>(&kf[2 * t + 1]), q1, a, 0, 0, 0);
#pragma unroll
      for (int j = 0; j < 4; ++j) { sc[t][j] = (32 * st_ + 16 * t + 4 * g + j < T) ? a[j] : -INFINITY; tm = fmaxf(tm, sc[t][j]); }
    }
    tm = fmaxf(tm, __shfl_xor(tm, 16)); tm = fmaxf(tm, __shfl_xor(tm, 32));      // (a step's first key is below T: tm is finite)
    const float nm = fmaxf(mx, tm), f = __expf(mx - nm);      // (first step: exp(-inf) = 0 on zeros)
    mx = nm; sum *= f;
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) { o[dt][0] *= f; o[dt][1] *= f; o[dt][2] *= f; o[dt][3] *= f; }
    f16x8 pb;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float p0 = __expf(sc[0][j] - mx), p1 = __expf(sc[1][j] - mx);
      sum += p0 + p1; pb[j] = (f16)p0; pb[4 + j] = (f16)p1;
    }
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) o[dt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(*reinterpret_cast<const f16x8*>(&vf[dt]), pb, o[dt], 0, 0, 0);
  }
  sum += __shfl_xor(sum, 16); sum += __shfl_xor(sum, 32);
#pragma unroll
  for (int dt = 0; dt < 4; ++dt)
#pragma unroll
    for (int j = 0; j < 4; ++j) so[wave][c][16 * dt + 4 * g + j] = o[dt][j];
  if (g == 0) { so[wave][c][64] = mx; so[wave][c][65] = sum; }
  __syncthreads();
  if (wave != 0 || i >= Np) return;
  float m4 = -INFINITY;
#pragma unroll
  for (int w = 0; w < 4; ++w) m4 = fmaxf(m4, so[w][c][64]);      // (a wave without a step left -inf and zeros)
  float fw[4], tot = 0.f;
#pragma unroll
  for (int w = 0; w < 4; ++w) { fw[w] = __expf(so[w][c][64] - m4); tot += fw[w] * so[w][c][65]; }
  const float inv = 1.0f / tot;
  f16* orow = out + ((size_t)b * Np + i) * d + h * 64;
#pragma unroll
  for (int dt = 0; dt < 4; ++dt) {
    float r[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int col = 16 * dt + 4 * g + j;
      r[j] = ((fw[0] * so[0][c][col] + fw[1] * so[1][c][col]) + (fw[2] * so[2][c][col] + fw[3] * so[3][c][col])) * inv;
    }
    const f16x4 hv = {(f16)r[0], (f16)r[1], (f16)r[2], (f16)r[3]};
    *reinterpret_cast<f16x4*>(orow + 16 * dt + 4 * g) = hv;
  }
}

int launch_prefill_cross_attn(hipStream_t st, const f16* q, const f16* kx, const f16* vt, f16* out, int B, int Np, int H, int T, int Tpad) {
  if (!q || !kx || !vt || !out || B < 1 || H < 1 || Np < 1 || Np > PF_MAX_ROWS || T < 1 || Tpad < cdiv(T, 32) * 32 || Tpad % 4) { set_error("prefill_cross_attn: bad argument (Np <= %d, Tpad >= T rounded up to 32)", PF_MAX_ROWS); return WIS_E_ARG; }
  hipLaunchKernelGGL(prefill_cross_attn_kernel, dim3(cdiv(Np, 16), H, B), dim3(256), 0, st, q, kx, vt, out, Np, H, T, Tpad);
  return WIS_OK;
}

}  // namespace wis
