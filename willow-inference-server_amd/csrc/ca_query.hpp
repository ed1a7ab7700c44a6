// ca_query.hpp — the cross-attention query folded from ROW PARTIALS, finished by a whole workgroup of 256 threads (device code, header only).
//
// `q` (+ `q2`, optional) hold q_raw = W'q x0 + (W'q Wo) a + W'q bo of the LayerNorm-folded query projection (model.hip out_cq_dual / out_cq_frag3), `stat` the
// (sum x, sum (x - tile mean)^2) pairs per 16 columns of the R <= 8 un-normalised rows [B*R][d/16][2] (d <= 2048), qcs / qb the folded projection's
// column sums and bias.  The workgroup merges mean / rstd of its utterance's rows and finishes q = rstd (q_raw - mean qcs) + qb for head h.
// This is dec_cross_attn_kernel's FOLD 4 prologue (dec_kernels.hip: the operands fetched once per workgroup as one 16-byte piece per thread and array and
// handed out through LDS, the Chan merge about the first tile's mean, the same expression for every element), in two steps so that a kernel can put its
// own requests between them:
//   ca_fold_request   every load of the prologue, unconditional and clamped (no exec-masked branch between the loads)
//   ca_fold_finish    statistics, staging, ONE raw workgroup barrier (it waits for LDS only, never for the caller's outstanding loads), then the lane's
//                     B fragments of the finished query, rounded to f16: lane (r = rq, k-quarter kq) gets q[r][8 kq ..] and q[r][32 + 8 kq ..]
#pragma once
#include "common.hpp"

namespace wis {

constexpr int CA_SQP = 68;      // row pitch of the staged operands (floats): 16-byte aligned, rows four banks apart
struct CaFoldLds {
  __attribute__((aligned(16))) float sq[10 * CA_SQP];      // rows 0..7: q_raw (both halves added), 8: column sums, 9: bias
  float srow[8][2];                                        // (mean, rstd) per row
};
struct CaFoldReq { float4 q, q2, c; float2 pt[2][2]; };

__device__ __forceinline__ void ca_fold_request(CaFoldReq& f, const float* __restrict__ q, const float* __restrict__ q2, const float* __restrict__ stat,
                                                const float* __restrict__ qcs, const float* __restrict__ qb, int b, int h, int R, int d) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, ntile = d >> 4;
  const int sr = (tid >> 4) < R ? (tid >> 4) : R - 1;      // thread t < 16 R owns piece (t & 15) of row t >> 4
  const size_t so = (size_t)(b * R + sr) * d + h * 64 + 4 * (tid & 15);
  f.q = *reinterpret_cast<const float4*>(q + so);
  f.q2 = make_float4(0.f, 0.f, 0.f, 0.f);
  if (q2) f.q2 = *reinterpret_cast<const float4*>(q2 + so);      // (uniform)
#pragma unroll
  for (int j = 0; j < 2; ++j) {      // wave w merges the partials of rows w and w + 4: lane = tile (and tile + 64)
    const int r = wave + 4 * j;
    const float2* sp = reinterpret_cast<const float2*>(stat) + (size_t)(b * R + (r < R ? r : R - 1)) * ntile;
    f.pt[j][0] = sp[lane < ntile ? lane : ntile - 1];
    f.pt[j][1] = sp[lane + 64 < ntile ? lane + 64 : ntile - 1];
  }
  f.c = *reinterpret_cast<const float4*>(((tid & 16) ? qb : qcs) + h * 64 + 4 * (tid & 15));      // threads 0-15 of every wave: the head's column sums, 16-31: its bias
}

__device__ __forceinline__ void ca_fold_finish(const CaFoldReq& f, CaFoldLds& s, int R, int d, int rq, int kq, f16x8& qf0, f16x8& qf1) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, ntile = d >> 4;
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    // Chan merge of the (sum, M2 about the tile mean) pairs about c0 = the first tile's mean:
    //   mu = c0 + mean_t (m_t - c0),   var = (sum_t (M2_t + 16 (m_t - c0)^2)) / d - (mu - c0)^2
    const int r = wave + 4 * j;
    const float c0 = readlane_f(f.pt[j][0].x, 0) * 0.0625f;
    float a1 = 0.f, a2 = 0.f;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const bool in = lane + 64 * i < ntile;
      const float dm = in ? f.pt[j][i].x * 0.0625f - c0 : 0.f;
      a1 += dm; a2 += in ? f.pt[j][i].y + 16.0f * dm * dm : 0.f;
    }
    a1 = wave_sum(a1); a2 = wave_sum(a2);
    if (lane == 0 && r < R) { const float invd = 1.0f / (float)d, dmu = a1 * 16.0f * invd; s.srow[r][0] = c0 + dmu; s.srow[r][1] = 1.0f / sqrtf(fmaxf(a2 * invd - dmu * dmu, 0.f) + 1e-5f); }
  }
  if (tid < 16 * R) *reinterpret_cast<float4*>(&s.sq[(tid >> 4) * CA_SQP + 4 * (tid & 15)]) = make_float4(f.q.x + f.q2.x, f.q.y + f.q2.y, f.q.z + f.q2.z, f.q.w + f.q2.w);
  if (tid < 32) *reinterpret_cast<float4*>(&s.sq[(8 + (tid >> 4)) * CA_SQP + 4 * (tid & 15)]) = f.c;
  asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
  const float mu = s.srow[rq][0], rs = s.srow[rq][1];
  const float* sqr = &s.sq[rq * CA_SQP + 8 * kq]; const float* scs = &s.sq[8 * CA_SQP + 8 * kq]; const float* sbq = &s.sq[9 * CA_SQP + 8 * kq];
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    qf0[e] = (f16)(rs * (sqr[e] - mu * scs[e]) + sbq[e]);
    qf1[e] = (f16)(rs * (sqr[32 + e] - mu * scs[32 + e]) + sbq[32 + e]);
  }
}

}  // namespace wis
