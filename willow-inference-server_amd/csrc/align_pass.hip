// align_pass.hip — the one-pass teacher-forced decoder of wis_align (align.hip align_one_pass, wis_model_set_align_pass(m, 1)): every position of every utterance's
// known text as ONE ragged batch of rows through all decoder layers, GEMM-shaped.  Utterance b contributes L_b rows at positions 0 .. L_b - 1, back to back:
// row off[b] + i is position i of utterance b, M = off[B]; the device table off [B + 1] is all that describes the batch.  Activations are row-major
// ([M][d] fp32 residual stream, f16 operands); the decoder's weight fragment images and the f16 cross K / V images are read in place, the self K / V of the pass
// live in its own [M][3 d] q | k | v buffer - nothing here touches the generate caches.
//
//   ap_embed_kernel        token + position rows -> x (fp32), the position from the offset table
//   ap_proj_kernel         Y = epi(A W^T) for ANY M.  A workgroup owns 64 COLUMNS (its four waves one 16-column tile each, every wave its own weight fragments:
//                          a fragment is requested once per workgroup) and a run of up to 8 row blocks whose K chunk of 128 lies in LDS, shared by the four
//                          waves as the MFMA's B operand.  grid = (N / 64, row runs): the run length shrinks until the grid has about 256 workgroups, and
//                          M > 128 is simply more runs.  It is a row split, not a K split: one summation order per element whatever the grid.
//                          The LayerNorm-folded epilogues read the fp32 residual rows THEMSELVES: the staging threads round them to f16 for the operand
//                          and sum x and x^2 on the way, so the row statistics need no launch of their own (8 launches per layer, not 11).
//   ap_self_attn_kernel    ragged causal attention, grid (64-query groups, H, B): the four waves take one 16-query block each of the SAME utterance and head
//                          and share every 32-key V tile through LDS (staged once per workgroup); online softmax, so any length fits the registers.
//                          No block straddles two utterances: the grid is per utterance and a group past L_b leaves at once.
//   ap_cross_attn_kernel   grid (32-query groups, H, B): TWO query blocks per workgroup against the utterance's T encoder keys split over the four waves -
//                          every K / V^T fragment a wave requests serves both blocks.  The heads wis_align selected copy their (f16) queries to
//                          AlignState::qsel on the way, in align_capture_kernel's layout: no capture launch.
//
// v_mfma_f32_16x16x32_f16 everywhere, operand conventions as in prefill.hip: A = 16 weight rows (keys, V^T rows) x 32 k, B = 16 activation rows (queries) x
// 32 k, D[4 g + j][lane & 15] on lane 16 g + (lane & 15); the scores of two 16-key tiles are the B operand of the P.V product.
#include <string.h>

#include <algorithm>
#include <vector>

#include "common.hpp"
#include "kernels.hpp"
#include "model.hpp"
#include "tap.hpp"

namespace wis {

constexpr int AP_KC = 128, AP_PITCH = AP_KC + 8, AP_RUN = 8;      // K chunk, its LDS pitch (f16), row blocks per workgroup at most

// utterance of row m (off [B + 1], ascending; B is small: a linear walk)
__device__ __forceinline__ int ap_utt(const int* __restrict__ off, int B, int m) {
  int b = 0;
  while (b + 1 < B && off[b + 1] <= m) ++b;
  return b;
}

__global__ __launch_bounds__(256) void ap_embed_kernel(const f16* __restrict__ emb, const f16* __restrict__ pos_emb, const int* __restrict__ tok, const int* __restrict__ off,
                                                       int B, int d, float* __restrict__ x) {
  const int m = blockIdx.x, b = ap_utt(off, B, m);
  const f16* e = emb + (size_t)tok[m] * d; const f16* pe = pos_emb + (size_t)(m - off[b]) * d;
  for (int k = threadIdx.x; k < d; k += 256) x[(size_t)m * d + k] = (float)e[k] + (float)pe[k];
}

// ---- the projection -------------------------------------------------------------------------------------------------------------------------------------------
template <int EPI>
__global__ __launch_bounds__(256) void ap_proj_kernel(AlignProjP p, int run) {
  constexpr bool LN = EPI != AP_EPI_RESID;
  constexpr int NREG = LN ? 2 : 1;      // 16-byte registers per staged piece of 8 elements (fp32 source: two)
  __shared__ __attribute__((aligned(16))) f16 sa[AP_RUN * 16 * AP_PITCH];
  __shared__ float sstat[AP_RUN * 16][2];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, g = lane >> 4, c = lane & 15;
  const int M = p.M, K = p.K, tiles = p.N / 16;
  const int MB = cdiv(M, 16), mb0 = blockIdx.y * run, nrb = min(run, MB - mb0);      // this workgroup's row blocks [mb0, mb0 + nrb)
  if (nrb <= 0) return;                                                              // (uniform)
  const int row0 = mb0 * 16;
  const int nt = 4 * blockIdx.x + wave;
  const bool has = nt < tiles;                                                       // (a last column group of fewer than four tiles: the wave only stages)
  const int nch = K / AP_KC, ksteps = K / 32;
  const u32x4* wp = reinterpret_cast<const u32x4*>(p.Wp) + (size_t)(has ? nt : tiles - 1) * ksteps * 64 + lane;
  // staging: piece i of the thread = row pr + 16 i of the run, elements 8 pc .. 8 pc + 7 of the chunk
  const int pr = tid >> 4, pc = tid & 15;
  u32x4 areg[AP_RUN * NREG]; u32x4 wcur[4], wnext[4];
  float s1[AP_RUN], s2[AP_RUN];
#pragma unroll
  for (int i = 0; i < AP_RUN; ++i) { s1[i] = 0.f; s2[i] = 0.f; }
  auto request = [&](int ch) {
#pragma unroll
    for (int i = 0; i < AP_RUN; ++i) {
#pragma unroll
      for (int r = 0; r < NREG; ++r) areg[NREG * i + r] = u32x4{0u, 0u, 0u, 0u};
      const int m = row0 + pr + 16 * i;
      if (i < nrb && m < M) {
        if (LN) {
          const float* src = reinterpret_cast<const float*>(p.A) + (size_t)m * K + ch * AP_KC + pc * 8;
          areg[NREG * i] = *reinterpret_cast<const u32x4*>(src); areg[NREG * i + NREG - 1] = *reinterpret_cast<const u32x4*>(src + 4);
        } else {
          areg[i] = *reinterpret_cast<const u32x4*>(reinterpret_cast<const f16*>(p.A) + (size_t)m * K + ch * AP_KC + pc * 8);
        }
      }
    }
#pragma unroll
    for (int s = 0; s < 4; ++s) wnext[s] = wp[(size_t)(ch * 4 + s) * 64];
  };
  f32x4 acc[AP_RUN];
#pragma unroll
  for (int e = 0; e < AP_RUN; ++e) acc[e] = f32x4{0.f, 0.f, 0.f, 0.f};
  request(0);
  for (int ch = 0; ch < nch; ++ch) {
#pragma unroll
    for (int i = 0; i < AP_RUN; ++i) {
      if (i >= nrb) continue;
      f16* dst = sa + (pr + 16 * i) * AP_PITCH + pc * 8;
      if (LN) {
        f16x8 hv;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const float v = __uint_as_float(areg[NREG * i + (j >> 2) * (NREG - 1)][j & 3]);
          s1[i] += v; s2[i] += v * v; hv[j] = (f16)v;
        }
        *reinterpret_cast<f16x8*>(dst) = hv;
      } else {
        *reinterpret_cast<u32x4*>(dst) = areg[i];
      }
    }
#pragma unroll
    for (int s = 0; s < 4; ++s) wcur[s] = wnext[s];
    __syncthreads();
    if (ch + 1 < nch) request(ch + 1);
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      const f16x8 wa = *reinterpret_cast<const f16x8*>(&wcur[s]);
#pragma unroll
      for (int e = 0; e < AP_RUN; ++e) {
        if (e < nrb) {
          const f16x8 xb = *reinterpret_cast<const f16x8*>(sa + (e * 16 + c) * AP_PITCH + s * 32 + g * 8);
          acc[e] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wa, xb, acc[e], 0, 0, 0);
        }
      }
    }
    __syncthreads();
  }
  if (LN) {      // the sixteen threads of a row (lanes 16 q .. 16 q + 15 of one wave) close its sums: mean and 1 / sqrt(var + 1e-5), var = E[x^2] - mean^2
#pragma unroll
    for (int i = 0; i < AP_RUN; ++i) {
      if (i >= nrb) continue;
      float a = s1[i], b = s2[i];
#pragma unroll
      for (int x = 1; x < 16; x <<= 1) { a += __shfl_xor(a, x); b += __shfl_xor(b, x); }
      if (pc == 0) {
        const float mu = a / (float)K, var = fmaxf(b / (float)K - mu * mu, 0.f);
        sstat[pr + 16 * i][0] = mu; sstat[pr + 16 * i][1] = 1.0f / sqrtf(var + 1e-5f);
      }
    }
    __syncthreads();
  }
  if (!has) return;
  // epilogue: lane holds columns n .. n + 3 of row m
  const int n = 16 * nt + 4 * g;
  const float4 bias = *reinterpret_cast<const float4*>(p.bias + n);
  float4 cs = make_float4(0.f, 0.f, 0.f, 0.f);
  if (LN) cs = *reinterpret_cast<const float4*>(p.csum + n);
#pragma unroll
  for (int e = 0; e < AP_RUN; ++e) {
    if (e >= nrb) continue;
    const int m = row0 + e * 16 + c;
    if (m >= M) continue;
    float4 s = make_float4(acc[e][0], acc[e][1], acc[e][2], acc[e][3]);
    if (LN) {      // the LayerNorm fold: rs (W' x - mu c) + b'
      const float mu = sstat[e * 16 + c][0], rs = sstat[e * 16 + c][1];
      s.x = rs * (s.x - mu * cs.x); s.y = rs * (s.y - mu * cs.y); s.z = rs * (s.z - mu * cs.z); s.w = rs * (s.w - mu * cs.w);
    }
    s.x += bias.x; s.y += bias.y; s.z += bias.z; s.w += bias.w;
    if (EPI == AP_EPI_RESID) {
      float4* y = reinterpret_cast<float4*>(p.y32 + (size_t)m * p.ldy + n);
      const float4 r = *y;
      *y = make_float4(r.x + s.x, r.y + s.y, r.z + s.z, r.w + s.w);
      continue;
    }
    if (EPI == AP_EPI_LN_F32) { *reinterpret_cast<float4*>(p.y32 + (size_t)m * p.ldy + n) = s; continue; }
    if (EPI == AP_EPI_LN_GELU) { s.x = gelu_erf(s.x); s.y = gelu_erf(s.y); s.z = gelu_erf(s.z); s.w = gelu_erf(s.w); }
    const f16x4 h = {(f16)s.x, (f16)s.y, (f16)s.z, (f16)s.w};
    *reinterpret_cast<f16x4*>(p.y16 + (size_t)m * p.ldy + n) = h;
  }
}

int launch_align_proj(hipStream_t st, const AlignProjP& p) {
  if (p.M < 1 || p.N < 16 || p.N % 16 || p.K < AP_KC || p.K % AP_KC || p.ldy < p.N || p.ldy % 4) { set_error("align_proj: bad shape M=%d N=%d K=%d ld=%d (N %% 16 == 0, K %% %d == 0, ld >= N)", p.M, p.N, p.K, p.ldy, AP_KC); return WIS_E_ARG; }
  const bool ln = p.epi != AP_EPI_RESID, f32 = p.epi == AP_EPI_RESID || p.epi == AP_EPI_LN_F32;
  if (!p.A || !p.Wp || !p.bias || (ln && !p.csum) || (f32 ? !p.y32 : !p.y16)) { set_error("align_proj: missing operand"); return WIS_E_ARG; }
  // row runs: as short as it takes to put about 256 workgroups on the grid, never longer than AP_RUN (the chunk's LDS)
  const int MB = cdiv(p.M, 16), groups = cdiv(p.N / 16, 4);
  const int runs = std::min(MB, std::max(cdiv(MB, AP_RUN), cdiv(256, groups))), run = cdiv(MB, runs);
  const dim3 grid(groups, cdiv(MB, run)), block(256);
  switch (p.epi) {
    case AP_EPI_LN_F16: hipLaunchKernelGGL(ap_proj_kernel<AP_EPI_LN_F16>, grid, block, 0, st, p, run); break;
    case AP_EPI_RESID: hipLaunchKernelGGL(ap_proj_kernel<AP_EPI_RESID>, grid, block, 0, st, p, run); break;
    case AP_EPI_LN_GELU: hipLaunchKernelGGL(ap_proj_kernel<AP_EPI_LN_GELU>, grid, block, 0, st, p, run); break;
    case AP_EPI_LN_F32: hipLaunchKernelGGL(ap_proj_kernel<AP_EPI_LN_F32>, grid, block, 0, st, p, run); break;
    default: set_error("align_proj: epilogue %d (0 LayerNorm-folded f16, 1 residual, 2 LayerNorm-folded GELU, 3 LayerNorm-folded f32)", p.epi); return WIS_E_ARG;
  }
  return WIS_OK;
}

int launch_align_embed(hipStream_t st, const f16* emb, const f16* pos_emb, const int* tok, const int* off, int B, int M, int d, float* x) {
  hipLaunchKernelGGL(ap_embed_kernel, dim3(M), dim3(256), 0, st, emb, pos_emb, tok, off, B, d, x);
  return WIS_OK;
}

// ---- ragged causal self-attention -----------------------------------------------------------------------------------------------------------------------------
// qkv f16 [M][3 d]: q (scaled by the projection) | k | v of row m.  Wave w of group blockIdx.x owns queries 16 (4 blockIdx.x + w) + (lane & 15) of utterance
// b = blockIdx.z; the workgroup walks the keys 32 at a time up to its last block's diagonal, a wave joins a step's arithmetic while the step starts at or
// below its own diagonal (the barriers it always joins).  A step a wave computes holds an unmasked key for each of its queries, so its maximum is finite.
__global__ __launch_bounds__(256) void ap_self_attn_kernel(const f16* __restrict__ qkv, const int* __restrict__ off, f16* __restrict__ out, int H) {
  constexpr int VP = 72;      // V tile pitch (f16): rows 4 g apart land 16 banks apart
  __shared__ __attribute__((aligned(16))) f16 sv[32 * VP];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, g = lane >> 4, c = lane & 15;
  const int h = blockIdx.y, b = blockIdx.z, d = 64 * H, ld = 3 * d;
  const int r0 = off[b], L = off[b + 1] - r0;
  if (64 * (int)blockIdx.x >= L) return;      // (uniform)
  const int qb = 4 * blockIdx.x + wave, i = 16 * qb + c, iq = min(i, L - 1);
  const bool active = 16 * qb < L;            // (wave-uniform)
  const f16* base = qkv + (size_t)r0 * ld + h * 64;
  const f16* qr = base + (size_t)iq * ld;
  const f16x8 q0 = *reinterpret_cast<const f16x8*>(qr + 8 * g), q1 = *reinterpret_cast<const f16x8*>(qr + 32 + 8 * g);
  const int qbl = min(4 * (int)blockIdx.x + 3, (L - 1) / 16), nsteps = qbl / 2 + 1;
  float mx = -INFINITY, sum = 0.f;
  f32x4 o[4];
#pragma unroll
  for (int dt = 0; dt < 4; ++dt) o[dt] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int kp = 0; kp < nsteps; ++kp) {
    const bool mine = active && 2 * kp <= qb;
    __syncthreads();      // the previous step's gathers are done
    {                     // 32 keys x 64 values: thread = key tid / 8, 16-byte column tid % 8
      const int key = tid >> 3, col = tid & 7;
      *reinterpret_cast<u32x4*>(sv + key * VP + col * 8) = *reinterpret_cast<const u32x4*>(base + (size_t)min(32 * kp + key, L - 1) * ld + 2 * d + col * 8);
    }
    f16x8 pb;
    if (mine) {
      float sc[2][4]; float tm = -INFINITY;
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        const f16* kr = base + (size_t)min(32 * kp + 16 * t + c, L - 1) * ld + d;
        const f16x8 k0 = *reinterpret_cast<const f16x8*>(kr + 8 * g), k1 = *reinterpret_cast<const f16x8*>(kr + 32 + 8 * g);
        f32x4 a = {0.f, 0.f, 0.f, 0.f};
        a = __builtin_amdgcn_mfma_f32_16x16x32_f16(k0, q0, a, 0, 0, 0);
        a = __builtin_amdgcn_mfma_f32_16x16x32_f16(k1, q1, a, 0, 0, 0);
#pragma unroll
        for (int j = 0; j < 4; ++j) { sc[t][j] = (32 * kp + 16 * t + 4 * g + j <= i) ? a[j] : -INFINITY; tm = fmaxf(tm, sc[t][j]); }
      }
      tm = fmaxf(tm, __shfl_xor(tm, 16)); tm = fmaxf(tm, __shfl_xor(tm, 32));
      const float nm = fmaxf(mx, tm), f = __expf(mx - nm);      // (first step: exp(-inf) = 0 on zeros)
      mx = nm; sum *= f;
#pragma unroll
      for (int dt = 0; dt < 4; ++dt) { o[dt][0] *= f; o[dt][1] *= f; o[dt][2] *= f; o[dt][3] *= f; }
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float p0 = __expf(sc[0][j] - mx), p1 = __expf(sc[1][j] - mx);
        sum += p0 + p1; pb[j] = (f16)p0; pb[4 + j] = (f16)p1;
      }
    }
    __syncthreads();
    if (mine) {
#pragma unroll
      for (int dt = 0; dt < 4; ++dt) {
        f16x8 va;
#pragma unroll
        for (int j = 0; j < 4; ++j) { va[j] = sv[(4 * g + j) * VP + 16 * dt + c]; va[4 + j] = sv[(16 + 4 * g + j) * VP + 16 * dt + c]; }
        o[dt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(va, pb, o[dt], 0, 0, 0);
      }
    }
  }
  sum += __shfl_xor(sum, 16); sum += __shfl_xor(sum, 32);
  if (i >= L) return;
  const float inv = 1.0f / sum;
  f16* orow = out + (size_t)(r0 + i) * d + h * 64;
#pragma unroll
  for (int dt = 0; dt < 4; ++dt) {
    const f16x4 hv = {(f16)(o[dt][0] * inv), (f16)(o[dt][1] * inv), (f16)(o[dt][2] * inv), (f16)(o[dt][3] * inv)};
    *reinterpret_cast<f16x4*>(orow + 16 * dt + 4 * g) = hv;
  }
}

int launch_align_self_attn(hipStream_t st, const f16* qkv, const int* off, f16* out, int B, int H, int Lmax) {
  if (!qkv || !off || !out || B < 1 || B > 65535 || H < 1 || Lmax < 1) { set_error("align_self_attn: bad argument"); return WIS_E_ARG; }
  hipLaunchKernelGGL(ap_self_attn_kernel, dim3(cdiv(Lmax, 64), H, B), dim3(256), 0, st, qkv, off, out, H);
  return WIS_OK;
}

// ---- ragged cross-attention, with the alignment heads' capture ------------------------------------------------------------------------------------------------
// q f16 [M][d] (scaled).  Workgroup = queries 32 blockIdx.x .. + 31 of utterance b as two 16-query blocks; wave w takes the 32-key steps w, w + 4, ... of the
// utterance's T keys for BOTH blocks with running maximum / sum / output per block (the next step's fragments requested ahead of the current step's MFMAs);
// the partial results meet in LDS, waves 0 and 1 write one block each.  kx [B][H][8][T][8] holds exactly T keys (the index is clamped, the score masked);
// vt [B][H][64][Tpad] is read up to the end of the last step.  head_sel [H] (or null): index s of head h in the handle's selection or -1; a selected head's
// queries at positions P .. P + ncap - 1 go to qsel [B][nsel][ncap][64] at matrix row position - P.
__global__ __launch_bounds__(256) void ap_cross_attn_kernel(const f16* __restrict__ q, const int* __restrict__ off, const f16* __restrict__ kx, const f16* __restrict__ vt,
                                                            f16* __restrict__ out, int H, int T, int Tpad, const int* __restrict__ head_sel, f16* __restrict__ qsel,
                                                            int nsel, int ncap, int P) {
  __shared__ float so[4][32][68];      // per wave: 64 output columns, maximum, sum of every query
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, g = lane >> 4, c = lane & 15;
  const int h = blockIdx.y, b = blockIdx.z, d = 64 * H;
  const int r0 = off[b], L = off[b + 1] - r0;
  if (32 * (int)blockIdx.x >= L) return;      // (uniform)
  f16x8 q0[2], q1[2];
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    const f16* qr = q + (size_t)(r0 + min(32 * (int)blockIdx.x + 16 * u + c, L - 1)) * d + h * 64;
    q0[u] = *reinterpret_cast<const f16x8*>(qr + 8 * g); q1[u] = *reinterpret_cast<const f16x8*>(qr + 32 + 8 * g);
  }
  const int s = head_sel ? head_sel[h] : -1;
  if (wave == 0 && s >= 0) {
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int i = 32 * blockIdx.x + 16 * u + c, row = i - P;
      if (i < L && row >= 0 && row < ncap) {
        f16* dst = qsel + (((size_t)b * nsel + s) * ncap + row) * 64;
        *reinterpret_cast<f16x8*>(dst + 8 * g) = q0[u]; *reinterpret_cast<f16x8*>(dst + 32 + 8 * g) = q1[u];
      }
    }
  }
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
  float mx[2] = {-INFINITY, -INFINITY}, sum[2] = {0.f, 0.f};
  f32x4 o[2][4];
#pragma unroll
  for (int u = 0; u < 2; ++u)
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) o[u][dt] = f32x4{0.f, 0.f, 0.f, 0.f};
  if (wave < nsteps) request(wave);
  for (int st_ = wave; st_ < nsteps; st_ += 4) {
#pragma unroll
    for (int t = 0; t < 4; ++t) { kf[t] = kn[t]; vf[t] = vn[t]; }
    if (st_ + 4 < nsteps) request(st_ + 4);
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      float sc[2][4]; float tm = -INFINITY;
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        f32x4 a = {0.f, 0.f, 0.f, 0.f};
        a = __builtin_amdgcn_mfma_f32_16x16x32_f16(*reinterpret_cast<const f16x8*>(&kf[2 * t]), q0[u], a, 0, 0, 0);
        a = __builtin_amdgcn_mfma_f32_16x16x32_f16(*reinterpret_cast<const f16x8*>(&kf[2 * t + 1]), q1[u], a, 0, 0, 0);
#pragma unroll
        for (int j = 0; j < 4; ++j) { sc[t][j] = (32 * st_ + 16 * t + 4 * g + j < T) ? a[j] : -INFINITY; tm = fmaxf(tm, sc[t][j]); }
      }
      tm = fmaxf(tm, __shfl_xor(tm, 16)); tm = fmaxf(tm, __shfl_xor(tm, 32));      // (a step's first key is below T: tm is finite)
      const float nm = fmaxf(mx[u], tm), f = __expf(mx[u] - nm);                     // (first step: exp(-inf) = 0 on zeros)
      mx[u] = nm; sum[u] *= f;
#pragma unroll
      for (int dt = 0; dt < 4; ++dt) { o[u][dt][0] *= f; o[u][dt][1] *= f; o[u][dt][2] *= f; o[u][dt][3] *= f; }
      f16x8 pb;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float p0 = __expf(sc[0][j] - nm), p1 = __expf(sc[1][j] - nm);
        sum[u] += p0 + p1; pb[j] = (f16)p0; pb[4 + j] = (f16)p1;
      }
#pragma unroll
      for (int dt = 0; dt < 4; ++dt) o[u][dt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(*reinterpret_cast<const f16x8*>(&vf[dt]), pb, o[u][dt], 0, 0, 0);
    }
  }
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    float su = sum[u];
    su += __shfl_xor(su, 16); su += __shfl_xor(su, 32);
#pragma unroll
    for (int dt = 0; dt < 4; ++dt)
#pragma unroll
      for (int j = 0; j < 4; ++j) so[wave][16 * u + c][16 * dt + 4 * g + j] = o[u][dt][j];
    if (g == 0) { so[wave][16 * u + c][64] = mx[u]; so[wave][16 * u + c][65] = su; }
  }
  __syncthreads();
  const int i = 32 * blockIdx.x + 16 * wave + c, qi = 16 * wave + c;      // waves 0 and 1: the block they close
  if (wave >= 2 || i >= L) return;
  float m4 = -INFINITY;
#pragma unroll
  for (int w = 0; w < 4; ++w) m4 = fmaxf(m4, so[w][qi][64]);      // (a wave without a step left -inf and zeros)
  float fw[4], tot = 0.f;
#pragma unroll
  for (int w = 0; w < 4; ++w) { fw[w] = __expf(so[w][qi][64] - m4); tot += fw[w] * so[w][qi][65]; }
  const float inv = 1.0f / tot;
  f16* orow = out + (size_t)(r0 + i) * d + h * 64;
#pragma unroll
  for (int dt = 0; dt < 4; ++dt) {
    float r[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int col = 16 * dt + 4 * g + j;
      r[j] = ((fw[0] * so[0][qi][col] + fw[1] * so[1][qi][col]) + (fw[2] * so[2][qi][col] + fw[3] * so[3][qi][col])) * inv;
    }
    const f16x4 hv = {(f16)r[0], (f16)r[1], (f16)r[2], (f16)r[3]};
    *reinterpret_cast<f16x4*>(orow + 16 * dt + 4 * g) = hv;
  }
}

int launch_align_cross_attn(hipStream_t st, const f16* q, const int* off, const f16* kx, const f16* vt, f16* out, int B, int H, int Lmax, int T, int Tpad,
                            const int* head_sel, f16* qsel, int nsel, int ncap, int P) {
  if (!q || !off || !kx || !vt || !out || B < 1 || B > 65535 || H < 1 || Lmax < 1 || T < 1 || Tpad < cdiv(T, 32) * 32 || Tpad % 4 || (head_sel && (!qsel || nsel < 1 || ncap < 1 || P < 0))) {
    set_error("align_cross_attn: bad argument (Tpad >= T rounded up to 32; a head table needs qsel)"); return WIS_E_ARG;
  }
  hipLaunchKernelGGL(ap_cross_attn_kernel, dim3(cdiv(Lmax, 32), H, B), dim3(256), 0, st, q, off, kx, vt, out, H, T, Tpad, head_sel, qsel, nsel, ncap, P);
  return WIS_OK;
}

// ---- the taps (tests/test_gpu_align_pass_ops.py) ----------------------------------------------------------------------------------------------------------------
// a host row table off [B + 1] -> device; *Lmax the longest utterance, M = off[B]
static int tap_offsets(Tap& t, const int32_t* off, int B, int** d_off, int* Lmax) {
  if (!off || B < 1 || B > 65535 || off[0] != 0) { set_error("%s: bad row table", t.name); return WIS_E_ARG; }
  *Lmax = 0;
  for (int b = 0; b < B; ++b) {
    if (off[b + 1] <= off[b]) { set_error("%s: utterance %d has no rows", t.name, b); return WIS_E_ARG; }
    *Lmax = std::max(*Lmax, off[b + 1] - off[b]);
  }
  WIS_RET(t.get(d_off, (size_t)B + 1));
  WIS_HIP_CHECK(hipMemcpyAsync(*d_off, off, ((size_t)B + 1) * 4, hipMemcpyHostToDevice, t.st));
  return WIS_OK;
}

}  // namespace wis

using namespace wis;

extern "C" {

// ap_proj_kernel on a raw weight matrix: x fp32 [M][K] (LayerNorm-folded epilogues 0 / 2 / 3, gamma and beta given) or f16 [M][K] (epilogue 1), W f16 [N][K], y f16
// [M][N] (0, 2) or fp32 [M][N] (1: in place on the residual; 3).  All device memory.
int wis_op_align_pass_proj(int device, int epi, const void* x, const float* gamma, const float* beta, const void* W_f16, const float* bias, void* y, int M, int N, int K) {
  Tap t(device, "wis_op_align_pass_proj"); WIS_RET(t.rc);
  const bool ln = epi != AP_EPI_RESID;
  if (!x || !W_f16 || !bias || !y || epi < AP_EPI_LN_F16 || epi > AP_EPI_LN_F32 || ln != (gamma != nullptr) || ln != (beta != nullptr) || M < 1 || N < 16 || N % 16 || K < AP_KC || K % AP_KC) {
    set_error("wis_op_align_pass_proj: bad argument"); return WIS_E_ARG;
  }
  hipStream_t st = t.st;
  f16 *w = nullptr, *wp = nullptr; float *b = nullptr, *csum = nullptr;
  WIS_RET(t.get(&w, (size_t)N * K)); WIS_RET(t.get(&wp, (size_t)N * K)); WIS_RET(t.get(&b, (size_t)N)); WIS_RET(t.get(&csum, (size_t)N, true));
  WIS_HIP_CHECK(hipMemcpyAsync(w, W_f16, (size_t)N * K * 2, hipMemcpyDeviceToDevice, st));
  WIS_HIP_CHECK(hipMemcpyAsync(b, bias, (size_t)N * 4, hipMemcpyDeviceToDevice, st));
  WIS_RET(prep_projection(st, w, N, N, K, 0, 1.f, gamma, beta, b, csum, wp, nullptr, 16));      // the loader's preparation, without the query scaling
  AlignProjP p; memset(&p, 0, sizeof(p));
  p.A = x; p.Wp = wp; p.bias = b; p.csum = ln ? csum : nullptr; p.M = M; p.N = N; p.K = K; p.ldy = N; p.epi = epi;
  if (epi == AP_EPI_RESID || epi == AP_EPI_LN_F32) p.y32 = reinterpret_cast<float*>(y); else p.y16 = reinterpret_cast<f16*>(y);
  return t.finish(launch_align_proj(st, p));
}

// ap_self_attn_kernel: qkv f16 [M][192 H], out f16 [M][64 H] (device); off [B + 1] (host), off[0] = 0, M = off[B]
int wis_op_align_pass_self_attn(int device, const void* qkv_f16, const int32_t* off, void* out_f16, int B, int H) {
  Tap t(device, "wis_op_align_pass_self_attn"); WIS_RET(t.rc);
  int* d_off = nullptr; int Lmax = 0;
  WIS_RET(tap_offsets(t, off, B, &d_off, &Lmax));
  return t.finish(launch_align_self_attn(t.st, reinterpret_cast<const f16*>(qkv_f16), d_off, reinterpret_cast<f16*>(out_f16), B, H, Lmax));
}

// ap_cross_attn_kernel: q / out f16 [M][64 H], kx f16 [B][H][8][T][8], vt f16 [B][H][64][Tpad] (device); off [B + 1] and head_sel [H] (host; null: no capture);
// qsel f16 [B][nsel][ncap][64] of qsel_elems elements (device)
int wis_op_align_pass_cross_attn(int device, const void* q_f16, const int32_t* off, const void* kx_f16, const void* vt_f16, void* out_f16, int B, int H, int T, int Tpad,
                                 const int32_t* head_sel, void* qsel_f16, long long qsel_elems, int nsel, int ncap, int P) {
  Tap t(device, "wis_op_align_pass_cross_attn"); WIS_RET(t.rc);
  int *d_off = nullptr, *d_sel = nullptr; int Lmax = 0;
  WIS_RET(tap_offsets(t, off, B, &d_off, &Lmax));
  if (head_sel) {
    if (H < 1 || !qsel_f16 || nsel < 1 || ncap < 1 || P < 0 || (long long)B * nsel * ncap * 64 > qsel_elems) { set_error("wis_op_align_pass_cross_attn: qsel of %lld elements for [%d][%d][%d][64]", qsel_elems, B, nsel, ncap); return WIS_E_ARG; }
    for (int h = 0; h < H; ++h) if (head_sel[h] < -1 || head_sel[h] >= nsel) { set_error("wis_op_align_pass_cross_attn: head %d: selection index %d outside %d", h, head_sel[h], nsel); return WIS_E_ARG; }
    WIS_RET(t.get(&d_sel, (size_t)H));
    WIS_HIP_CHECK(hipMemcpyAsync(d_sel, head_sel, (size_t)H * 4, hipMemcpyHostToDevice, t.st));
  }
  return t.finish(launch_align_cross_attn(t.st, reinterpret_cast<const f16*>(q_f16), d_off, reinterpret_cast<const f16*>(kx_f16), reinterpret_cast<const f16*>(vt_f16),
                                          reinterpret_cast<f16*>(out_f16), B, H, Lmax, T, Tpad, d_sel, reinterpret_cast<f16*>(qsel_f16), nsel, ncap, P));
}

}  // extern "C"
