// align.hip — word-level timestamps: cross-attention alignment and dynamic time warping (wis_align).
// An object of its own on model.hpp's interface (the decoder pass, the handle) and tap.hpp's scaffold (the wis_op_* taps at the end).
//
// What openai-whisper's find_alignment / CTranslate2's Whisper.align compute, on the GPU:
//   1. the text is teacher-forced through the batched-row decoder route in passes of 16 positions (dec_forward_frag, un-folded
//      branch: the finished cross-attention query of every row lies in fp32 in m->dq behind the cross-Q projection).  After each
//      layer that holds alignment heads, align_capture_kernel copies those heads' 64-wide query slices, rounded to f16 exactly as the
//      cross-attention kernel rounds its MFMA operand, to [utterance][selected head][row][64]: 128 bytes per (head, token), nothing
//      that grows with the frame count.
//   2. per chunk of G selected heads (G from a fixed scratch budget, so 320 heads cost what 6 cost):
//        align_scores_kernel   P = softmax(q . K^T) over ALL n_audio_ctx keys from the cross-attention's own K image ([H][8][T][8], f16;
//                              the query scaling is folded into the projections, so there is no further factor), cropped to
//                              num_frames / 2 on the way out
//        align_norm_kernel     (P - mean) / std over the TOKEN axis per frame (population std, two passes)
//        align_median_kernel   median of odd width along frames with reflect padding (rank selection in LDS; NaN sorts last like
//                              torch.sort), summed over the chunk's heads in head order into ONE [tokens][frames] matrix;
//                              the last chunk divides by the head count and negates
//   3. align_dtw_kernel        anti-diagonal wavefront of dtw_cpu's recurrence (every cell is one f32 add of values fixed by its three
//                              predecessors, so the bits are the serial loop's), 2-bit trace, backtrace and forward-order path on the GPU
//   4. align_prob_kernel       softmax(logits[: eot])[text token] at the row that predicts it
#include <math.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "common.hpp"
#include "kernels.hpp"
#include "model.hpp"
#include "tap.hpp"

using namespace wis;

namespace {

constexpr int AL_RW = 8;                 // query rows per wave of align_scores_kernel
constexpr int AL_MAXW = 63;              // widest median filter
constexpr int AL_DTW_THREADS = 512;      // one thread per cost-table row (N + 1 <= 512: n_text_ctx is 448)
constexpr size_t AL_W_BUDGET = (size_t)96 << 20;      // bytes of per-chunk probability scratch

// ---- 1. capture -------------------------------------------------------------------------------------------------------------
// grid (M rows, heads of this layer), block 64.  Row r of the pass = utterance ub0 + r / 16 at position t0 + r % 16; matrix row = position - P.
__global__ __launch_bounds__(64) void align_capture_kernel(const float* __restrict__ dq, f16* __restrict__ qsel, const int* __restrict__ sel_head,
                                                           int s0, int nsel, int d, int ub0, int t0, int P, int ncap) {
  const int r = blockIdx.x, s = s0 + blockIdx.y, b = ub0 + (r >> 4), i = t0 + (r & 15) - P;
  if (i < 0 || i >= ncap) return;
  qsel[(((size_t)b * nsel + s) * ncap + i) * 64 + threadIdx.x] = (f16)dq[(size_t)r * d + sel_head[s] * 64 + threadIdx.x];
}
// the op's form of the same copy: q fp32 [nsel][n][64] -> f16 [nsel][ncap][64]
__global__ __launch_bounds__(64) void align_q16_kernel(const float* __restrict__ q, f16* __restrict__ qsel, int n, int ncap) {
  const int i = blockIdx.x, s = blockIdx.y;
  qsel[((size_t)s * ncap + i) * 64 + threadIdx.x] = (f16)q[((size_t)s * n + i) * 64 + threadIdx.x];
}

// ---- 2a. attention weights ----------------------------------------------------------------------------------------------------
// grid (ceil(nmax / 8), G, B), block 64 = one wave that owns 8 query rows of one (utterance, selected head): lane = key within a strip of 64.
// q (f16 pairs) is read from LDS as broadcast 16-byte reads, K straight from the [8][T][8] image (16 contiguous bytes per lane and dh octet:
// a strip's 64 lanes read 1 KB runs), products on v_dot2_f32_f16 with fp32 accumulation.  Pass 1 leaves the raw scores in W and finds
// the row maxima, pass 2 the sums, pass 3 writes exp(s - max) / sum for the first `F` keys (the softmax runs over all T keys; the
// crop comes after it).  Every lane re-reads only what it wrote itself.
typedef _Float16 al_h2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ float al_dot2(unsigned a, unsigned b, float c) {
  return __builtin_amdgcn_fdot2(__builtin_bit_cast(al_h2, a), __builtin_bit_cast(al_h2, b), c, false);
}
__global__ __launch_bounds__(64) void align_scores_kernel(const f16* __restrict__ qsel, const f16* __restrict__ kbase, const long long* __restrict__ koff,
                                                          long long kbstride, const int* __restrict__ dN, const int* __restrict__ dF,
                                                          float* __restrict__ W, int g0, int G, int nsel, int ncap, int nmax, int T) {
  __shared__ __attribute__((aligned(16))) unsigned sq[AL_RW][32];
  const int lane = threadIdx.x, g = blockIdx.y, b = blockIdx.z, s = g0 + g, r0 = blockIdx.x * AL_RW;
  const int N = dN[b], F = dF[b];
  if (r0 >= N) return;
  const unsigned* qp = reinterpret_cast<const unsigned*>(qsel + ((size_t)b * nsel + s) * ncap * 64);
  for (int e = lane; e < AL_RW * 32; e += 64) { int r = r0 + (e >> 5); if (r > N - 1) r = N - 1; sq[e >> 5][e & 31] = qp[(size_t)r * 32 + (e & 31)]; }
  __syncthreads();
  const f16* kb = kbase + koff[s] + (size_t)b * kbstride;
  float* Wr = W + ((size_t)(b * G + g) * nmax + r0) * T;
  float mx[AL_RW];
#pragma unroll
  for (int r = 0; r < AL_RW; ++r) mx[r] = -INFINITY;
  for (int k0 = 0; k0 < T; k0 += 64) {
    const int key = k0 + lane, kc = key < T ? key : T - 1;
    float acc[AL_RW];
#pragma unroll
    for (int r = 0; r < AL_RW; ++r) acc[r] = 0.f;
#pragma unroll
    for (int c = 0; c < 8; ++c) {
      const u32x4 kv = *reinterpret_cast<const u32x4*>(kb + ((size_t)c * T + kc) * 8);
#pragma unroll
      for (int r = 0; r < AL_RW; ++r) {
        const u32x4 qv = *reinterpret_cast<const u32x4*>(&sq[r][4 * c]);
        acc[r] = al_dot2(kv[0], qv[0], acc[r]); acc[r] = al_dot2(kv[1], qv[1], acc[r]);
        acc[r] = al_dot2(kv[2], qv[2], acc[r]); acc[r] = al_dot2(kv[3], qv[3], acc[r]);
      }
    }
    if (key < T) {
#pragma unroll
      for (int r = 0; r < AL_RW; ++r) if (r0 + r < N) { Wr[(size_t)r * T + key] = acc[r]; mx[r] = fmaxf(mx[r], acc[r]); }
    }
  }
#pragma unroll
  for (int r = 0; r < AL_RW; ++r) {
    if (r0 + r >= N) break;      // (uniform)
    const float m_ = wave_max(mx[r]);
    float su = 0.f;
    for (int key = lane; key < T; key += 64) su += expf(Wr[(size_t)r * T + key] - m_);
    su = wave_sum(su);
    for (int key = lane; key < F; key += 64) Wr[(size_t)r * T + key] = expf(Wr[(size_t)r * T + key] - m_) / su;
  }
}

// ---- 2b. (w - mean) / std over tokens -------------------------------------------------------------------------------------------
// grid (ceil(fmax / 64), G, B), block 256 = 64 frames x 4 row partitions (partials combined in a fixed order through LDS)
__global__ __launch_bounds__(256) void align_norm_kernel(float* __restrict__ W, const int* __restrict__ dN, const int* __restrict__ dF, int G, int nmax, int T) {
  __shared__ float sp[4][64];
  const int fl = threadIdx.x & 63, rp = threadIdx.x >> 6, g = blockIdx.y, b = blockIdx.z, f = blockIdx.x * 64 + fl;
  const int N = dN[b], F = dF[b];
  if (blockIdx.x * 64 >= F) return;
  const bool in = f < F;
  float* Wc = W + (size_t)(b * G + g) * nmax * T + (in ? f : 0);
  float a = 0.f;
  for (int r = rp; r < N; r += 4) a += Wc[(size_t)r * T];
  sp[rp][fl] = a;
  __syncthreads();
  const float mean = (((sp[0][fl] + sp[1][fl]) + sp[2][fl]) + sp[3][fl]) / (float)N;
  __syncthreads();
  a = 0.f;
  for (int r = rp; r < N; r += 4) { const float dlt = Wc[(size_t)r * T] - mean; a += dlt * dlt; }
  sp[rp][fl] = a;
  __syncthreads();
  const float sd = sqrtf((((sp[0][fl] + sp[1][fl]) + sp[2][fl]) + sp[3][fl]) / (float)N);
  if (in) for (int r = rp; r < N; r += 4) Wc[(size_t)r * T] = (Wc[(size_t)r * T] - mean) / sd;
}

// ---- 2c. median along frames, sum over the chunk's heads -----------------------------------------------------------------------
// torch.sort's order: NaN behind everything
__device__ __forceinline__ bool al_less(float a, float b) { return a < b || (a == a && b != b); }
// grid (ceil(fmax / 256), nmax, B), block 256.  acc [B][nmax][T]: first chunk stores, later chunks add, the last one writes -(sum / nsel).
__global__ __launch_bounds__(256) void align_median_kernel(const float* __restrict__ W, float* __restrict__ acc, const int* __restrict__ dN, const int* __restrict__ dF,
                                                           int G, int nmax, int T, int width, int first, int last, int nsel) {
  __shared__ float sw[256 + AL_MAXW];
  const int t = threadIdx.x, row = blockIdx.y, b = blockIdx.z, f0 = blockIdx.x * 256, f = f0 + t;
  const int N = dN[b], F = dF[b];
  if (row >= N || f0 >= F) return;
  const int pad = width / 2;
  const bool filt = pad > 0 && F > pad;
  float a = 0.f;
  for (int g = 0; g < G; ++g) {
    const float* Wr = W + ((size_t)(b * G + g) * nmax + row) * T;
    if (!filt) { if (f < F) a += Wr[f]; continue; }
    for (int e = t; e < 256 + 2 * pad; e += 256) {
      int x = f0 + e - pad;
      if (x < 0) x = -x;
      if (x > F - 1) x = 2 * (F - 1) - x;
      if (x < 0) x = 0;                       // (only positions no in-range output reads)
      if (x > F - 1) x = F - 1;
      sw[e] = Wr[x];
    }
    __syncthreads();
    if (f < F) {
      float res = sw[t + pad];
      for (int i = 0; i < width; ++i) {
        const float vi = sw[t + i];
        int cnt = 0;
        for (int j = 0; j < width; ++j) { const float vj = sw[t + j]; cnt += (al_less(vj, vi) || (!al_less(vi, vj) && j < i)) ? 1 : 0; }
        if (cnt == pad) res = vi;
      }
      a += res;
    }
    __syncthreads();
  }
  if (f < F) {
    float* o = acc + ((size_t)b * nmax + row) * T + f;
    if (!first) a += *o;
    *o = last ? -(a / (float)nsel) : a;
  }
}

// ---- 3. dynamic time warping ----------------------------------------------------------------------------------------------------
// grid (B), block 512: thread i owns row i of the (N + 1) x (M + 1) cost table and walks it left to right, one anti-diagonal d = i + j per
// step; cost[i - 1][j] and cost[i - 1][j - 1] come from the neighbour thread through three rotating LDS rows (one barrier per step),
// cost[i][j - 1] stays in a register, x is prefetched three steps ahead.  trace (0 diagonal / 1 up / 2 left, borders 2 along row 0 and 1
// along column 0) is packed 16 cells to a word per row, so the backtrace's one thread re-loads only when it changes row or word.
// It writes the path backwards into `rev`; the block then copies it out in forward order.
__global__ __launch_bounds__(AL_DTW_THREADS) void align_dtw_kernel(const float* __restrict__ x, long long xbstride, int pitch, const int* __restrict__ dN, const int* __restrict__ dF,
                                                                 int N1, int M1, unsigned* __restrict__ trace, long long tbstride, int wpr,
                                                                 int* __restrict__ rev, int* __restrict__ out_text, int* __restrict__ out_time, int* __restrict__ out_len, int cap) {
  __shared__ float sc[3][AL_DTW_THREADS];
  __shared__ int s_len;
  const int i = threadIdx.x, b = blockIdx.x;
  const int N = dN ? dN[b] : N1, M = dF ? dF[b] : M1;
  const float* xr = x + (size_t)b * xbstride + (size_t)(i > 0 ? i - 1 : 0) * pitch;
  unsigned* tr = trace + (size_t)b * tbstride;
  const bool row_in = i >= 1 && i <= N;
  float left = INFINITY;                 // cost[i][0]
  unsigned word = row_in ? 1u : 2u;      // cell j = 0: up (column 0) / left (row 0)
  float xa = 0.f, xb = 0.f, xc = 0.f;
  if (row_in) { xa = xr[0]; xb = M > 1 ? xr[1] : 0.f; xc = M > 2 ? xr[2] : 0.f; }
  for (int d = 0; d <= N + M; ++d) {
    const int j = d - i;
    float* cur = sc[d % 3];
    if (i <= N && j >= 0 && j <= M) {
      if (i == 0) {
        cur[0] = d == 0 ? 0.f : INFINITY;
        if (j > 0) { word |= 2u << (2 * (j & 15)); }
        if ((j & 15) == 15 || j == M) { tr[j >> 4] = word; word = 0; }
      } else if (j == 0) {
        cur[i] = INFINITY;
      } else {
        const float c1 = sc[(d + 2) % 3][i - 1], c0 = sc[(d + 1) % 3][i - 1], c2 = left;      // up (diagonal d - 1), diagonal (d - 2), left
        int tc; float c;
        if (c0 < c1 && c0 < c2) { c = c0; tc = 0; }
        else if (c1 < c0 && c1 < c2) { c = c1; tc = 1; }
        else { c = c2; tc = 2; }
        const float v = xa + c;
        xa = xb; xb = xc; xc = (j + 3 <= M) ? xr[j + 2] : 0.f;
        left = v; cur[i] = v;
        word |= (unsigned)tc << (2 * (j & 15));
        if ((j & 15) == 15 || j == M) { tr[(size_t)i * wpr + (j >> 4)] = word; word = 0; }
      }
    }
    __syncthreads();
  }
  __threadfence_block();
  __syncthreads();
  int* rv = rev + (size_t)b * 2 * cap;
  if (i == 0) {
    int ci = N, cj = M, n = 0, wi = -1, wj = -1; unsigned w = 0;
    while (ci > 0 || cj > 0) {
      if (wi != ci || wj != (cj >> 4)) { wi = ci; wj = cj >> 4; w = __hip_atomic_load(tr + (size_t)ci * wpr + wj, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
      const unsigned tc = (w >> (2 * (cj & 15))) & 3u;
      if (n < cap) { rv[2 * n] = ci - 1; rv[2 * n + 1] = cj - 1; }
      ++n;
      if (tc == 0) { --ci; --cj; } else if (tc == 1) --ci; else --cj;
    }
    s_len = n < cap ? n : cap;
    out_len[b] = s_len;
  }
  __syncthreads();
  const int L = s_len;
  for (int k = i; k < L; k += AL_DTW_THREADS) {
    out_text[(size_t)b * cap + k] = __hip_atomic_load(rv + 2 * (L - 1 - k), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    out_time[(size_t)b * cap + k] = __hip_atomic_load(rv + 2 * (L - 1 - k) + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
  }
}

// ---- 4. text token probabilities ------------------------------------------------------------------------------------------------
// grid (rows of the pass), block 256: softmax over ids < eot of the row's logits at target[row] (< 0: no output) -> probs[dst[row]]
__global__ __launch_bounds__(256) void align_prob_kernel(const float* __restrict__ logits, int vpad, int eot, const int* __restrict__ target, const int* __restrict__ dst,
                                                         float* __restrict__ probs) {
  __shared__ float sr[4];
  const int r = blockIdx.x, t = threadIdx.x, tg = target[r];
  if (tg < 0) return;
  const float* lr = logits + (size_t)r * vpad;
  float mx = -INFINITY;
  for (int v = t; v < eot; v += 256) mx = fmaxf(mx, lr[v]);
  mx = wave_max(mx);
  if ((t & 63) == 0) sr[t >> 6] = mx;
  __syncthreads();
  mx = fmaxf(fmaxf(sr[0], sr[1]), fmaxf(sr[2], sr[3]));
  __syncthreads();
  float su = 0.f;
  for (int v = t; v < eot; v += 256) su += expf(lr[v] - mx);
  su = wave_sum(su);
  if ((t & 63) == 0) sr[t >> 6] = su;
  __syncthreads();
  if (t == 0) probs[dst[r]] = expf(lr[tg] - mx) / (((sr[0] + sr[1]) + sr[2]) + sr[3]);
}

// ---- launch helpers (wis_align and the wis_op_* taps share them) ----------------------------------------------------------------
// heads per chunk under the scratch budget
int align_chunk_heads(int nsel, int B, int nmax, int T) {
  const size_t per = (size_t)B * nmax * T * 4;
  size_t g = AL_W_BUDGET / (per ? per : 1);
  if (g < 1) g = 1;
  return (int)std::min<size_t>(g, (size_t)nsel);
}
// heads_per_chunk = 0: the budget rule; > 0 (the stage tap): that many, so that small shapes run more than one chunk
int align_heads_per_chunk(int nsel, int B, int nmax, int T, int heads_per_chunk) {
  return heads_per_chunk > 0 ? std::min(heads_per_chunk, nsel) : align_chunk_heads(nsel, B, nmax, T);
}
// the alignment matrix -mean_h median((P_h - mean) / std) of B utterances into acc [B][nmax][T]
int launch_align_matrix(hipStream_t st, const f16* qsel, const f16* kbase, const long long* koff, long long kbstride, const int* dN, const int* dF,
                        float* W, float* acc, int B, int nsel, int ncap, int nmax, int fmax, int T, int width, hipEvent_t* ev = nullptr, int nev = 0, int* used_ev = nullptr,
                        int heads_per_chunk = 0) {
  if (width < 1 || width > AL_MAXW || !(width & 1)) { set_error("align: median_filter_width %d must be odd and within [1, %d]", width, AL_MAXW); return WIS_E_ARG; }
  if (nsel < 1 || nmax < 1 || fmax < 1 || fmax > T) { set_error("align: bad shape (heads %d, tokens %d, frames %d of %d)", nsel, nmax, fmax, T); return WIS_E_ARG; }
  const int G = align_heads_per_chunk(nsel, B, nmax, T, heads_per_chunk);
  int e = 0;
  for (int g0 = 0; g0 < nsel; g0 += G) {
    const int Gc = std::min(G, nsel - g0);
    hipLaunchKernelGGL(align_scores_kernel, dim3(cdiv(nmax, AL_RW), Gc, B), dim3(64), 0, st, qsel, kbase, koff, kbstride, dN, dF, W, g0, Gc, nsel, ncap, nmax, T);
    if (ev && e + 2 <= nev) hipEventRecord(ev[e++], st);
    hipLaunchKernelGGL(align_norm_kernel, dim3(cdiv(fmax, 64), Gc, B), dim3(256), 0, st, W, dN, dF, Gc, nmax, T);
    hipLaunchKernelGGL(align_median_kernel, dim3(cdiv(fmax, 256), nmax, B), dim3(256), 0, st, W, acc, dN, dF, Gc, nmax, T, width, g0 == 0 ? 1 : 0, g0 + Gc >= nsel ? 1 : 0, nsel);
    if (ev && e + 1 <= nev) hipEventRecord(ev[e++], st);
  }
  if (used_ev) *used_ev = e;
  WIS_HIP_CHECK(hipGetLastError());
  return WIS_OK;
}
inline int dtw_wpr(int M) { return (M + 1 + 15) / 16; }
int launch_align_dtw(hipStream_t st, const float* x, long long xbstride, int pitch, const int* dN, const int* dF, int N, int M, int B,
                     unsigned* trace, int* rev, int* out_text, int* out_time, int* out_len, int cap) {
  if (N < 1 || M < 1 || N + 1 > AL_DTW_THREADS) { set_error("align: DTW of %d x %d unsupported (1 <= rows <= %d)", N, M, AL_DTW_THREADS - 1); return WIS_E_UNSUPPORTED; }
  const int wpr = dtw_wpr(M);
  hipLaunchKernelGGL(align_dtw_kernel, dim3(B), dim3(AL_DTW_THREADS), 0, st, x, xbstride, pitch, dN, dF, N, M, trace, (long long)(N + 1) * wpr, wpr, rev, out_text, out_time, out_len, cap);
  WIS_HIP_CHECK(hipGetLastError());
  return WIS_OK;
}

// ---- per-handle state -------------------------------------------------------------------------------------------------------------
// the selected heads, sorted by (layer, head); empty list = every head of the upper half of the decoder layers
std::vector<std::pair<int, int>> align_selected(const wis_model* m) {
  std::vector<std::pair<int, int>> v;
  const int L = m->cfg.n_dec_layers, H = m->cfg.n_heads;
  if (m->al.heads.empty()) { for (int l = L / 2; l < L; ++l) for (int h = 0; h < H; ++h) v.emplace_back(l, h); }
  else { for (size_t i = 0; i + 1 < m->al.heads.size(); i += 2) v.emplace_back(m->al.heads[i], m->al.heads[i + 1]); }
  std::sort(v.begin(), v.end());
  v.erase(std::unique(v.begin(), v.end()), v.end());
  return v;
}
template <class T>
int al_malloc(wis_model* m, T** p, size_t n) {
  void* q = nullptr;
  const size_t b = std::max<size_t>(n * sizeof(T), 256);
  hipError_t e = hipMalloc(&q, b);
  if (e != hipSuccess) { set_error("align: hipMalloc(%zu bytes) failed: %s", b, hipGetErrorString(e)); return WIS_E_NOMEM; }
  m->allocs.push_back(q); m->bytes += b; *p = static_cast<T*>(q);
  return WIS_OK;
}
// first align call of a handle (or the first one after the heads changed): scratch sized by max_batch, n_text_ctx and n_audio_ctx
int align_prepare(wis_model* m) {
  AlignState& a = m->al;
  if (a.ready) return WIS_OK;
  const wis_config_t& c = m->cfg;
  const auto sel = align_selected(m);
  const int nsel = (int)sel.size(), Bm = c.max_batch, T = c.n_audio_ctx, ncap = c.n_text_ctx;
  a.layer_s0.assign(c.n_dec_layers + 1, 0);
  std::vector<int> heads(nsel); std::vector<long long> koff(nsel);
  for (int s = 0; s < nsel; ++s) {
    heads[s] = sel[s].second; a.layer_s0[sel[s].first + 1]++;
    koff[s] = (long long)((const char*)m->kx[sel[s].first] - (const char*)m->kx_all) / 2 + (long long)sel[s].second * T * 64;
  }
  for (int l = 0; l < c.n_dec_layers; ++l) a.layer_s0[l + 1] += a.layer_s0[l];
  if (nsel > a.sel_cap) {
    for (void* old : {(void*)a.d_sel_head, (void*)a.d_koff, (void*)a.qsel}) if (old) {      // a larger head set: the smaller buffers go
      auto it = std::find(m->allocs.begin(), m->allocs.end(), old);
      if (it != m->allocs.end()) m->allocs.erase(it);
      hipFree(old);
    }
    m->bytes -= a.sel_bytes; a.sel_bytes = 0;
    const size_t b0 = m->bytes;
    a.d_sel_head = nullptr; a.d_koff = nullptr; a.qsel = nullptr;
    WIS_RET(al_malloc(m, &a.d_sel_head, nsel)); WIS_RET(al_malloc(m, &a.d_koff, nsel));
    WIS_RET(al_malloc(m, &a.qsel, (size_t)Bm * nsel * ncap * 64));
    a.sel_cap = nsel; a.sel_bytes = m->bytes - b0;
  }
  if (!a.W) {
    WIS_RET(al_malloc(m, &a.W, std::max(AL_W_BUDGET / 4, (size_t)Bm * ncap * T)));
    WIS_RET(al_malloc(m, &a.acc, (size_t)Bm * ncap * T));
    WIS_RET(al_malloc(m, &a.trace, (size_t)Bm * (ncap + 1) * dtw_wpr(T)));
    WIS_RET(al_malloc(m, &a.rev, (size_t)Bm * 2 * (ncap + T)));
    WIS_RET(al_malloc(m, &a.path, (size_t)Bm * 2 * (ncap + T)));
    WIS_RET(al_malloc(m, &a.d_meta, (size_t)Bm * 3 + 2 * MAX_ROWS));
    WIS_RET(al_malloc(m, &a.probs, (size_t)Bm * ncap));
    for (auto& e : a.ev) if (hipEventCreate(&e) != hipSuccess) { set_error("align: event create failed"); return WIS_E_HIP; }
  }
  WIS_HIP_CHECK(hipMemcpyAsync(a.d_sel_head, heads.data(), (size_t)nsel * 4, hipMemcpyHostToDevice, m->st));
  WIS_HIP_CHECK(hipMemcpyAsync(a.d_koff, koff.data(), (size_t)nsel * 8, hipMemcpyHostToDevice, m->st));
  WIS_HIP_CHECK(hipStreamSynchronize(m->st));
  a.nsel = nsel; a.ready = true;
  return WIS_OK;
}
}  // namespace
// dec_forward_frag's hook (model.hpp): the finished cross-Q of layer l's rows lies in m->dq
int wis::align_capture_q(wis_model* m, int l, int M) {
  const AlignState& a = m->al;
  const int s0 = a.layer_s0[l], n = a.layer_s0[l + 1] - s0;
  if (n > 0) hipLaunchKernelGGL(align_capture_kernel, dim3(M, n), dim3(64), 0, m->st, m->dq, a.qsel, a.d_sel_head, s0, a.nsel, m->cfg.d_model, a.cap_ub0, a.cap_t0, a.cap_P, m->cfg.n_text_ctx);
  return WIS_OK;
}
namespace {

// the whole alignment up to the matrix (want_dtw: and the paths / probabilities).  Results stay in m->al (acc, path, probs).
int align_run(wis_model* m, const float* input, int input_kind, int B, const int32_t* start_seq, int P, const int32_t* text, const int32_t* text_len,
              const int32_t* num_frames, int width, bool want_dtw, const char* who) {
  const wis_config_t& c = m->cfg;
  const int T = c.n_audio_ctx, ncap = c.n_text_ctx, V = c.n_vocab;
  WIS_RET(check_batch(m, B, 1));
  if (P < 1 || width < 1 || width > AL_MAXW || !(width & 1)) { set_error("%s: bad argument (start sequence of %d tokens, median_filter_width %d: odd, within [1, %d])", who, P, width, AL_MAXW); return WIS_E_ARG; }
  if (ncap % 16) { set_error("%s: n_text_ctx = %d is not a multiple of the 16-row pass", who, ncap); return WIS_E_UNSUPPORTED; }      // (padded rows must stay below n_text_ctx)
  const int eot = c.eot, nots = c.no_timestamps;
  int Lmax = 0, nmax = 0, fmax = 0;
  std::vector<int> off(B + 1, 0), hN(B), hF(B);
  for (int b = 0; b < B; ++b) {
    if (text_len[b] < 0 || P + 1 + text_len[b] > ncap) { set_error("%s: utterance %d: %d start + 1 + %d text tokens exceed n_text_ctx = %d", who, b, P, text_len[b], ncap); return WIS_E_ARG; }
    if (num_frames[b] < 2 || num_frames[b] / 2 > T) { set_error("%s: utterance %d: num_frames %d outside [2, %d]", who, b, num_frames[b], 2 * T); return WIS_E_ARG; }
    off[b + 1] = off[b] + text_len[b];
    hN[b] = text_len[b] + 1; hF[b] = num_frames[b] / 2;
    Lmax = std::max(Lmax, P + 1 + text_len[b]); nmax = std::max(nmax, hN[b]); fmax = std::max(fmax, hF[b]);
  }
  for (int k = 0; k < P; ++k) if (start_seq[k] < 0 || start_seq[k] >= V) { set_error("%s: start token %d out of range", who, start_seq[k]); return WIS_E_ARG; }
  for (int k = 0; k < off[B]; ++k) if (text[k] < 0 || text[k] >= V) { set_error("%s: text token %d out of range", who, text[k]); return WIS_E_ARG; }
  WIS_RET(align_prepare(m));
  AlignState& a = m->al;
  hipStream_t st = m->st;
  a.n_ev = 0;
  hipEventRecord(a.ev[0], st);
  WIS_RET(run_front(m, input, input_kind, B));
  hipEventRecord(a.ev[1], st);
  int* dN = a.d_meta; int* dF = a.d_meta + B; int* d_tgt = a.d_meta + 3 * c.max_batch; int* d_dst = d_tgt + MAX_ROWS;
  {
    int* h = m->h_pin->al_frames;
    memcpy(h, hN.data(), (size_t)B * 4); memcpy(h + B, hF.data(), (size_t)B * 4);
    WIS_HIP_CHECK(hipMemcpyAsync(a.d_meta, h, (size_t)2 * B * 4, hipMemcpyHostToDevice, st));
  }
  // teacher-forced passes of 16 positions over groups of <= MAX_ROWS / 16 utterances: always 16 rows per utterance (a shorter tail is
  // padded with eot inputs at the following positions, which later rows never attend to), so every pass takes the un-folded batched-row
  // route whose finished cross-Q the capture reads
  const int Lpad = cdiv(Lmax, 16) * 16, UG = MAX_ROWS / 16;
  auto tok_at = [&](int b, int p) { return p < P ? start_seq[p] : (p == P ? nots : (p - P - 1 < text_len[b] ? text[off[b] + p - P - 1] : eot)); };
  for (int ub0 = 0; ub0 < B; ub0 += UG) {
    const int nb = std::min(UG, B - ub0), M = nb * 16;
    int glen = 0;
    for (int u = 0; u < nb; ++u) glen = std::max(glen, P + 1 + text_len[ub0 + u]);
    for (int t0 = 0; t0 < glen && t0 < Lpad; t0 += 16) {
      std::vector<int> tok(M), pos(M), slot(M), ls(M), tgt(M, -1), dst(M, 0);
      for (int u = 0; u < nb; ++u) for (int i = 0; i < 16; ++i) {
        const int r = u * 16 + i, b = ub0 + u, p = t0 + i;
        tok[r] = tok_at(b, p); pos[r] = p; slot[r] = u; ls[r] = u;
        const int row = p - P;      // matrix row: predicts text token `row`
        if (row >= 0 && row < text_len[b]) { tgt[r] = text[off[b] + row]; dst[r] = b * ncap + row; }
      }
      a.cap_ub0 = ub0; a.cap_t0 = t0; a.cap_P = P;
      for (int attempt = 0; attempt < 2; ++attempt) {      // (a pass whose granule hand-off gave up is repeated in the ticket form)
        SpinClaim claim(m, nb);
        WIS_RET(upload_rows(m, tok, pos, slot, ls));
        PinnedScratch* h = m->h_pin;
        memcpy(h->al_tgt, tgt.data(), (size_t)M * 4); memcpy(h->al_dst, dst.data(), (size_t)M * 4);
        WIS_HIP_CHECK(hipMemcpyAsync(d_tgt, h->al_tgt, (size_t)M * 4, hipMemcpyHostToDevice, st));
        WIS_HIP_CHECK(hipMemcpyAsync(d_dst, h->al_dst, (size_t)M * 4, hipMemcpyHostToDevice, st));
        a.capture = true; a.kv_ub0 = ub0;      // the group's rows read the cross K / V of utterances ub0 .. ub0 + nb - 1
        const int rc = dec_forward(m, M, 16, nb, want_dtw, 1, 0);
        a.capture = false; a.kv_ub0 = 0;
        WIS_RET(rc);
        if (want_dtw) hipLaunchKernelGGL(align_prob_kernel, dim3(M), dim3(256), 0, st, m->logits, m->n_vocab_pad, eot, d_tgt, d_dst, a.probs);
        bool gave_up = false;
        WIS_RET(spin_gave_up(m, &gave_up));      // (synchronises: the pinned staging areas are free again)
        if (!gave_up) break;
      }
    }
  }
  hipEventRecord(a.ev[2], st);
  WIS_RET(launch_align_matrix(st, a.qsel, m->kx_all, a.d_koff, (long long)c.n_heads * T * 64, dN, dF, a.W, a.acc, B, a.nsel, ncap, nmax, fmax, T, width,
                              a.ev + 5, (int)(sizeof(a.ev) / sizeof(a.ev[0])) - 5, &a.n_ev));
  a.ev_partial = a.n_ev < 2 * cdiv(a.nsel, align_chunk_heads(a.nsel, B, nmax, T));
  hipEventRecord(a.ev[3], st);
  if (want_dtw) WIS_RET(launch_align_dtw(st, a.acc, (long long)nmax * T, T, dN, dF, nmax, fmax, B, a.trace, a.rev, a.path, a.path + (size_t)B * (ncap + T), a.d_meta + 2 * c.max_batch, ncap + T));
  hipEventRecord(a.ev[4], st);
  a.last_nmax = nmax;
  return WIS_OK;
}

}  // namespace

extern "C" {

int wis_model_set_alignment_heads(wis_model_t* m, const int32_t* layer_head_pairs, int n) {
  if (!m || n < 0 || (n > 0 && !layer_head_pairs)) { set_error("wis_model_set_alignment_heads: bad argument"); return WIS_E_ARG; }
  for (int i = 0; i < n; ++i) {
    const int l = layer_head_pairs[2 * i], h = layer_head_pairs[2 * i + 1];
    if (l < 0 || l >= m->cfg.n_dec_layers || h < 0 || h >= m->cfg.n_heads) { set_error("wis_model_set_alignment_heads: (layer %d, head %d) outside %d x %d", l, h, m->cfg.n_dec_layers, m->cfg.n_heads); return WIS_E_ARG; }
  }
  WIS_ENTER(m, "wis_model_set_alignment_heads")
  m->al.heads.assign(layer_head_pairs, layer_head_pairs + 2 * (size_t)n);
  m->al.ready = false;
  return WIS_OK;
}

int wis_align(wis_model_t* m, const float* input, int input_kind, int B, const int32_t* start_seq, int P, const int32_t* text, const int32_t* text_len,
              const int32_t* num_frames, int median_filter_width, int32_t* path_text, int32_t* path_time, int32_t* path_len, float* token_probs) {
  if (!m || !input || !start_seq || !text_len || !num_frames || !path_text || !path_time || !path_len || !token_probs || B < 1) { set_error("wis_align: bad argument"); return WIS_E_ARG; }
  WIS_ENTER(m, "wis_align")
  WIS_HIP_CHECK(hipSetDevice(m->device));
  WIS_RET(align_run(m, input, input_kind, B, start_seq, P, text, text_len, num_frames, median_filter_width, true, "wis_align"));
  const AlignState& a = m->al;
  const int ncap = m->cfg.n_text_ctx, cap = ncap + m->cfg.n_audio_ctx;
  // outputs: path_text / path_time [B][n_text_ctx + n_audio_ctx], path_len [B], token_probs [B][n_text_ctx]
  WIS_HIP_CHECK(hipMemcpyAsync(path_text, a.path, (size_t)B * cap * 4, hipMemcpyDeviceToHost, m->st));
  WIS_HIP_CHECK(hipMemcpyAsync(path_time, a.path + (size_t)B * cap, (size_t)B * cap * 4, hipMemcpyDeviceToHost, m->st));
  WIS_HIP_CHECK(hipMemcpyAsync(path_len, a.d_meta + 2 * m->cfg.max_batch, (size_t)B * 4, hipMemcpyDeviceToHost, m->st));
  WIS_HIP_CHECK(hipMemcpyAsync(token_probs, a.probs, (size_t)B * ncap * 4, hipMemcpyDeviceToHost, m->st));
  WIS_HIP_CHECK(hipStreamSynchronize(m->st));
  return WIS_OK;
}

int wis_debug_align_matrix(wis_model_t* m, const float* input, int input_kind, int B, const int32_t* start_seq, int P, const int32_t* text, const int32_t* text_len,
                           const int32_t* num_frames, int median_filter_width, float* out) {
  if (!m || !input || !start_seq || !text_len || !num_frames || !out || B < 1) { set_error("wis_debug_align_matrix: bad argument"); return WIS_E_ARG; }
  WIS_ENTER(m, "wis_debug_align_matrix")
  WIS_HIP_CHECK(hipSetDevice(m->device));
  WIS_RET(align_run(m, input, input_kind, B, start_seq, P, text, text_len, num_frames, median_filter_width, false, "wis_debug_align_matrix"));
  // out: the utterances' dense [text_len + 1][num_frames / 2] matrices back to back
  const int T = m->cfg.n_audio_ctx; size_t o = 0;
  for (int b = 0; b < B; ++b) {
    const int N = text_len[b] + 1, F = num_frames[b] / 2;
    WIS_HIP_CHECK(hipMemcpy2DAsync(out + o, (size_t)F * 4, m->al.acc + (size_t)b * m->al.last_nmax * T, (size_t)T * 4, (size_t)F * 4, N, hipMemcpyDeviceToHost, m->st));
    o += (size_t)N * F;
  }
  WIS_HIP_CHECK(hipStreamSynchronize(m->st));
  return WIS_OK;
}

int wis_align_last_timing(wis_model_t* m, float* ms) {
  if (!m || !ms || !m->al.W) { set_error("wis_align_last_timing: no align call on this handle yet"); return WIS_E_STATE; }
  const AlignState& a = m->al;
  // ms[0..5]: encoder + cross K/V, decoder passes, matrix (all of it), DTW, attention weights alone, normalise + filter alone
  for (int i = 0; i < 4; ++i) { ms[i] = 0.f; if (hipEventElapsedTime(&ms[i], a.ev[i], a.ev[i + 1]) != hipSuccess) ms[i] = -1.f; }
  ms[4] = ms[5] = a.ev_partial ? -1.f : 0.f;      // (more head chunks than event pairs: no split)
  for (int e = 0; e + 1 < a.n_ev && !a.ev_partial; e += 2) {
    float t = 0.f;
    if (hipEventElapsedTime(&t, e == 0 ? a.ev[2] : a.ev[5 + e - 1], a.ev[5 + e]) == hipSuccess) ms[4] += t;
    if (hipEventElapsedTime(&t, a.ev[5 + e], a.ev[5 + e + 1]) == hipSuccess) ms[5] += t;
  }
  return WIS_OK;
}

int wis_op_dtw(int device, const float* x, int N, int M, int32_t* text_idx, int32_t* time_idx, int32_t* len) {
  Tap t(device, "wis_op_dtw"); WIS_RET(t.rc);
  if (!x || !text_idx || !time_idx || !len || N < 1 || M < 1) { set_error("wis_op_dtw: bad argument"); return WIS_E_ARG; }
  unsigned* trace = nullptr; int* rev = nullptr;
  WIS_RET(t.get(&trace, (size_t)(N + 1) * dtw_wpr(M))); WIS_RET(t.get(&rev, (size_t)2 * (N + M)));
  // text_idx / time_idx hold up to N + M - 1 entries
  return t.finish(launch_align_dtw(t.st, x, 0, M, nullptr, nullptr, N, M, 1, trace, rev, text_idx, time_idx, len, N + M - 1));
}

int wis_op_align_matrix(int device, const float* q, const void* kx_f16, int T_tokens, int n_heads_sel, int T, int frames, int width, float* out) {
  Tap t(device, "wis_op_align_matrix"); WIS_RET(t.rc);
  if (!q || !kx_f16 || !out || T_tokens < 1 || n_heads_sel < 1 || T < 1 || frames < 1 || frames > T) { set_error("wis_op_align_matrix: bad argument"); return WIS_E_ARG; }
  hipStream_t st = t.st;
  // q fp32 [n_heads_sel][T_tokens][64] (finished queries), kx_f16 [n_heads_sel][8][T][8] (the cross-attention K image), out fp32 [T_tokens][frames]
  const int n = T_tokens, G = align_chunk_heads(n_heads_sel, 1, n, T);
  f16* qsel = nullptr; long long* koff = nullptr; int* meta = nullptr; float *W = nullptr, *acc = nullptr;
  std::vector<long long> hk(n_heads_sel);
  for (int s = 0; s < n_heads_sel; ++s) hk[s] = (long long)s * T * 64;
  const int hm[2] = {n, frames};
  WIS_RET(t.get(&qsel, (size_t)n_heads_sel * n * 64)); WIS_RET(t.get(&koff, (size_t)n_heads_sel)); WIS_RET(t.get(&meta, 2));
  WIS_RET(t.get(&W, (size_t)G * n * T)); WIS_RET(t.get(&acc, (size_t)n * T));
  hipMemcpyAsync(koff, hk.data(), (size_t)n_heads_sel * 8, hipMemcpyHostToDevice, st);
  hipMemcpyAsync(meta, hm, 8, hipMemcpyHostToDevice, st);
  hipLaunchKernelGGL(align_q16_kernel, dim3(n, n_heads_sel), dim3(64), 0, st, q, qsel, n, n);
  WIS_RET(launch_align_matrix(st, qsel, reinterpret_cast<const f16*>(kx_f16), koff, 0, meta, meta + 1, W, acc, 1, n_heads_sel, n, n, frames, T, width));
  if (hipMemcpy2DAsync(out, (size_t)frames * 4, acc, (size_t)T * 4, (size_t)frames * 4, n, hipMemcpyDeviceToDevice, st) != hipSuccess) { set_error("wis_op_align_matrix: copy failed"); return WIS_E_HIP; }
  return t.finish(WIS_OK);
}

// One stage of the matrix (or the chain) on B ragged utterances, with the shipped call's index arithmetic in the caller's hands: stage 0 scores +
// softmax, 1 norm, 2 median + head sum, 3 the chain (launch_align_matrix itself).  N / F / koff are host arrays; q fp32 [B][nsel][ncap][64] (rows
// >= N[b] are never read), K f16 of k_elems elements, W of w_elems and acc of acc_elems floats are device buffers the caller fills beforehand and reads
// back whole.  Stages 0 - 2 keep chunk c (heads c G .. c G + Gc - 1, laid out [B][Gc][nmax][T]) at W + c B G nmax T; the chain reuses W + 0 as wis_align does.
int wis_op_align_stage(int device, int stage, const float* q, const void* kx_f16, long long k_elems, const long long* koff, long long kbstride,
                       const int32_t* N, const int32_t* F, int B, int nsel, int ncap, int nmax, int fmax, int T, int width, int heads_per_chunk,
                       float* W, long long w_elems, float* acc, long long acc_elems) {
  Tap t(device, "wis_op_align_stage"); WIS_RET(t.rc);
  const bool need_q = stage == 0 || stage == 3, need_acc = stage == 2 || stage == 3;
  if (stage < 0 || stage > 3 || !N || !F || !W || (need_q && (!q || !kx_f16 || !koff)) || (need_acc && !acc)) { set_error("wis_op_align_stage: bad argument"); return WIS_E_ARG; }
  if (B < 1 || B > 65535 || nsel < 1 || nsel > 65535 || nmax < 1 || nmax > 65535 || ncap < nmax || T < 1 || fmax < 1 || fmax > T || heads_per_chunk < 0 || kbstride < 0) {
    set_error("wis_op_align_stage: bad shape (B %d, heads %d, tokens %d of %d, frames %d of %d, heads_per_chunk %d)", B, nsel, nmax, ncap, fmax, T, heads_per_chunk); return WIS_E_ARG;
  }
  if (width < 1 || width > AL_MAXW || !(width & 1)) { set_error("wis_op_align_stage: median_filter_width %d must be odd and within [1, %d]", width, AL_MAXW); return WIS_E_ARG; }
  for (int b = 0; b < B; ++b) if (N[b] < 1 || N[b] > nmax || F[b] < 1 || F[b] > fmax) {
    set_error("wis_op_align_stage: utterance %d: %d tokens of %d, %d frames of %d", b, N[b], nmax, F[b], fmax); return WIS_E_ARG;
  }
  const int G = align_heads_per_chunk(nsel, B, nmax, T, heads_per_chunk), nchunks = cdiv(nsel, G);
  const long long region = (long long)B * G * nmax * T;
  if (w_elems < (stage == 3 ? 1 : nchunks) * region || (need_acc && acc_elems < (long long)B * nmax * T)) {
    set_error("wis_op_align_stage: W of %lld floats (needs %lld) or acc of %lld (needs %lld) too small", w_elems, (stage == 3 ? 1 : nchunks) * region, acc_elems, (long long)B * nmax * T); return WIS_E_ARG;
  }
  if (need_q) for (int s = 0; s < nsel; ++s) {      // every (utterance, head) image lies inside K, 16-byte aligned
    const long long last = koff[s] + (long long)(B - 1) * kbstride;
    if (koff[s] < 0 || (koff[s] & 7) || (kbstride & 7) || last + (long long)T * 64 > k_elems) { set_error("wis_op_align_stage: head %d: K image at %lld (+ %lld per utterance) outside %lld elements or unaligned", s, koff[s], kbstride, k_elems); return WIS_E_ARG; }
  }
  hipStream_t st = t.st;
  f16* qsel = nullptr; long long* d_koff = nullptr; int* meta = nullptr;
  WIS_RET(t.get(&meta, (size_t)2 * B));
  hipMemcpyAsync(meta, N, (size_t)B * 4, hipMemcpyHostToDevice, st);
  hipMemcpyAsync(meta + B, F, (size_t)B * 4, hipMemcpyHostToDevice, st);
  const int *dN = meta, *dF = meta + B;
  const f16* kb = reinterpret_cast<const f16*>(kx_f16);
  if (need_q) {
    WIS_RET(t.get(&qsel, (size_t)B * nsel * ncap * 64)); WIS_RET(t.get(&d_koff, (size_t)nsel));
    hipMemcpyAsync(d_koff, koff, (size_t)nsel * 8, hipMemcpyHostToDevice, st);
    hipLaunchKernelGGL(align_q16_kernel, dim3(ncap, B * nsel), dim3(64), 0, st, q, qsel, ncap, ncap);
  }
  if (stage == 3) return t.finish(launch_align_matrix(st, qsel, kb, d_koff, kbstride, dN, dF, W, acc, B, nsel, ncap, nmax, fmax, T, width, nullptr, 0, nullptr, heads_per_chunk));
  for (int g0 = 0, c = 0; g0 < nsel; g0 += G, ++c) {      // launch_align_matrix's loop, one kernel of it
    const int Gc = std::min(G, nsel - g0);
    float* Wc = W + (size_t)c * region;
    if (stage == 0) hipLaunchKernelGGL(align_scores_kernel, dim3(cdiv(nmax, AL_RW), Gc, B), dim3(64), 0, st, qsel, kb, d_koff, kbstride, dN, dF, Wc, g0, Gc, nsel, ncap, nmax, T);
    if (stage == 1) hipLaunchKernelGGL(align_norm_kernel, dim3(cdiv(fmax, 64), Gc, B), dim3(256), 0, st, Wc, dN, dF, Gc, nmax, T);
    if (stage == 2) hipLaunchKernelGGL(align_median_kernel, dim3(cdiv(fmax, 256), nmax, B), dim3(256), 0, st, Wc, acc, dN, dF, Gc, nmax, T, width, g0 == 0 ? 1 : 0, g0 + Gc >= nsel ? 1 : 0, nsel);
  }
  return t.finish(WIS_OK);
}

// B cost tables in one buffer as wis_align lays them out: table b at x + b xbstride, rows `pitch` apart, N[b] x M[b] (host arrays) under common
// nmax / fmax -> text_idx / time_idx [B][cap], len [B] (device; cap >= nmax + fmax: a path takes N + M - 1 entries, and N + M when non-finite costs send it
// along the borders, as dtw_cpu's does)
int wis_op_dtw_batch(int device, const float* x, long long x_elems, long long xbstride, int pitch, const int32_t* N, const int32_t* M, int B, int nmax, int fmax, int cap,
                     int32_t* text_idx, int32_t* time_idx, int32_t* len) {
  Tap t(device, "wis_op_dtw_batch"); WIS_RET(t.rc);
  if (!x || !N || !M || !text_idx || !time_idx || !len || B < 1 || B > 65535 || nmax < 1 || fmax < 1 || pitch < fmax || xbstride < 0 || cap < 1 || (long long)cap < (long long)nmax + fmax) {
    set_error("wis_op_dtw_batch: bad argument"); return WIS_E_ARG;
  }
  for (int b = 0; b < B; ++b) if (N[b] < 1 || N[b] > nmax || M[b] < 1 || M[b] > fmax || (long long)b * xbstride + (long long)(N[b] - 1) * pitch + M[b] > x_elems) {
    set_error("wis_op_dtw_batch: table %d (%d x %d of %d x %d) outside its buffer of %lld floats", b, N[b], M[b], nmax, fmax, x_elems); return WIS_E_ARG;
  }
  if (nmax + 1 > AL_DTW_THREADS) return launch_align_dtw(t.st, x, xbstride, pitch, nullptr, nullptr, nmax, fmax, B, nullptr, nullptr, text_idx, time_idx, len, cap);      // (refuses before it launches)
  unsigned* trace = nullptr; int* rev = nullptr; int* meta = nullptr;
  WIS_RET(t.get(&trace, (size_t)B * (nmax + 1) * dtw_wpr(fmax))); WIS_RET(t.get(&rev, (size_t)B * 2 * cap)); WIS_RET(t.get(&meta, (size_t)2 * B));
  hipMemcpyAsync(meta, N, (size_t)B * 4, hipMemcpyHostToDevice, t.st);
  hipMemcpyAsync(meta + B, M, (size_t)B * 4, hipMemcpyHostToDevice, t.st);
  return t.finish(launch_align_dtw(t.st, x, xbstride, pitch, meta, meta + B, nmax, fmax, B, trace, rev, text_idx, time_idx, len, cap));
}

// align_prob_kernel on caller-supplied logits [rows][vpad] (device): target / dst are host arrays, probs a device buffer of probs_len floats
int wis_op_align_probs(int device, const float* logits, int rows, int vpad, int eot, const int32_t* target, const int32_t* dst, float* probs, int probs_len) {
  Tap t(device, "wis_op_align_probs"); WIS_RET(t.rc);
  if (!logits || !target || !dst || !probs || rows < 1 || vpad < 1 || eot < 1 || eot > vpad || probs_len < 1) { set_error("wis_op_align_probs: bad argument"); return WIS_E_ARG; }
  for (int r = 0; r < rows; ++r) if (target[r] >= 0 && (target[r] >= vpad || dst[r] < 0 || dst[r] >= probs_len)) {
    set_error("wis_op_align_probs: row %d: target %d of %d ids or slot %d of %d out of range", r, target[r], vpad, dst[r], probs_len); return WIS_E_ARG;
  }
  int* meta = nullptr;
  WIS_RET(t.get(&meta, (size_t)2 * rows));
  hipMemcpyAsync(meta, target, (size_t)rows * 4, hipMemcpyHostToDevice, t.st);
  hipMemcpyAsync(meta + rows, dst, (size_t)rows * 4, hipMemcpyHostToDevice, t.st);
  hipLaunchKernelGGL(align_prob_kernel, dim3(rows), dim3(256), 0, t.st, logits, vpad, eot, meta, meta + rows, probs);
  return t.finish(WIS_OK);
}

// align_capture_kernel on a caller-supplied pass: dq fp32 [M][d] (device), sel_head [nsel] (host), the layer's heads s0 .. s0 + n_layer_heads - 1,
// qsel f16 [>= ub0 + ceil(M / 16)][nsel][ncap][64] of qsel_elems elements (device)
int wis_op_align_capture(int device, const float* dq, int M, int d, const int32_t* sel_head, int s0, int n_layer_heads, int nsel, int ub0, int t0, int P, int ncap,
                         void* qsel_f16, long long qsel_elems) {
  Tap t(device, "wis_op_align_capture"); WIS_RET(t.rc);
  if (!dq || !sel_head || !qsel_f16 || M < 1 || M > 65535 || d < 64 || d % 64 || s0 < 0 || n_layer_heads < 1 || nsel < 1 || s0 + n_layer_heads > nsel || ub0 < 0 || t0 < 0 || P < 0 || ncap < 1) {
    set_error("wis_op_align_capture: bad argument"); return WIS_E_ARG;
  }
  for (int s = s0; s < s0 + n_layer_heads; ++s) if (sel_head[s] < 0 || sel_head[s] >= d / 64) { set_error("wis_op_align_capture: head %d outside %d", sel_head[s], d / 64); return WIS_E_ARG; }
  if ((long long)(ub0 + (M - 1) / 16 + 1) * nsel * ncap * 64 > qsel_elems) { set_error("wis_op_align_capture: utterances up to %d outside qsel of %lld elements", ub0 + (M - 1) / 16, qsel_elems); return WIS_E_ARG; }
  int* d_sel = nullptr;
  WIS_RET(t.get(&d_sel, (size_t)nsel));
  hipMemcpyAsync(d_sel, sel_head, (size_t)nsel * 4, hipMemcpyHostToDevice, t.st);
  hipLaunchKernelGGL(align_capture_kernel, dim3(M, n_layer_heads), dim3(64), 0, t.st, dq, reinterpret_cast<f16*>(qsel_f16), d_sel, s0, nsel, d, ub0, t0, P, ncap);
  return t.finish(WIS_OK);
}

}  // extern "C"
