// sv.hip — speaker verification: the WavLM-base-plus-sv x-vector embedder (HF WavLMForXVector, post-LN encoder, weighted layer sum).
// An object of its own: it shares no state with the Whisper handle (model.hpp), only the encoder's launch_* functions and tap.hpp's scaffold.
//
// PCM (host, already trimmed / gain-normalised / feature-extractor-normalised by wis_hip/sv.py) -> 512-float embedding (host).  Every
// step from the first convolution to the statistics pooling runs on the GPU:
//   conv 0 (1 -> 512, k10 s5) + GroupNorm(512 groups) + GELU   sv_conv0_stats_kernel / sv_conv0_apply_kernel (direct conv, recomputed
//                                                               in the apply pass instead of storing 31999 x 512 fp32 pre-norm values)
//   conv 1-6 (512 -> 512, stride 2) + GELU                      the encoder GEMM over channels-last rows: im2col row t is the contiguous
//                                                               span x + 2 t 512 of length k 512 (lda = 1024, no copy; W [out][k][in])
//   feature projection: LayerNorm(512), Linear 512 -> 768       sv_ln_kernel + GEMM
//   positional conv (k128, groups 16, weight norm folded) + GELU + residual, encoder LayerNorm     sv_posconv_kernel (MFMA) + sv_ln_kernel
//   12 post-LN layers: QKV GEMM, gated relative-position attention (sv_attn_kernel: bias from a per-(head, distance) table, gate
//   from the layer input inside the kernel; no [H][T][T] tensor), out-proj + residual, LayerNorm, FFN (GELU), + residual, LayerNorm
//   weighted layer sum                                          accumulated in fp32 by the LayerNorm that produces each hidden state
//   projector, TDNN x5 (ReLU), mean / unbiased std, Linear 3000 -> 512     GEMMs + sv_relu_gather_kernel (ReLU and the dilated taps'
//                                                               im2col), sv_stats_kernel, sv_linear_kernel (M = 1, fp32)
#include <math.h>
#include <string.h>

#include <mutex>
#include <string>
#include <vector>

#include "common.hpp"
#include "kernels.hpp"
#include "tap.hpp"

using namespace wis;

namespace {

// ---- the one architecture served (HF WavLMConfig defaults with the -sv head) --------------------------------------------------
constexpr int C0 = 512;          // feature-encoder channels
constexpr int D = 768, H = 12, DH = 64, FF = 3072, NL = 12;
constexpr int PK = 128, PG = 16, PCG = D / PG;   // positional conv: kernel, groups, channels per group (48)
constexpr int NTD = 5, XV = 512;
constexpr int TD_DIM[NTD] = {512, 512, 512, 512, 1500};
constexpr int TD_K[NTD] = {5, 3, 3, 1, 1};
constexpr int TD_DIL[NTD] = {1, 2, 3, 1, 1};
constexpr int TD_LAST_PAD = 1536;                // tdnn.4's N padded to the GEMM's 128 columns (zero weights and bias)
constexpr int CONV_K[7] = {10, 3, 3, 3, 3, 2, 2}, CONV_S[7] = {5, 2, 2, 2, 2, 2, 2};
constexpr int CHUNK0 = 64;                       // conv 0 frames per workgroup (GroupNorm partial statistics per chunk)

__device__ __forceinline__ float gelu_f(float x) { return gelu_erf(x); }
// element-wise scaling of an accumulator quad that stays scalar f32 arithmetic (the asm barriers keep the backend from pairing the
// products into v_pk_mul_f32, which tools/isa_lint.py forbids in MFMA kernels)
__device__ __forceinline__ f32x4 scale4(f32x4 v, float a) {
  float x = v[0] * a, y = v[1] * a, z = v[2] * a, w = v[3] * a;
  asm("" : "+v"(x)); asm("" : "+v"(z));
  return f32x4{x, y, z, w};
}

// ---- conv 0 ----------------------------------------------------------------------------------------------------------------------
// y[t][c] = sum_j w[c][j] x[5 t + j]; pass 1 leaves (mean, M2) of every (chunk, channel), pass 2 recomputes y in the same order
__device__ __forceinline__ float conv0_at(const float* s, const float* w, int tl) {
  float a = 0.f;
#pragma unroll
  for (int j = 0; j < 10; ++j) a += w[j] * s[tl * 5 + j];
  return a;
}
__global__ __launch_bounds__(256) void sv_conv0_stats_kernel(const float* __restrict__ x, const float* __restrict__ w0, float* __restrict__ part, int T0) {
  __shared__ float s[CHUNK0 * 5 + 5];
  const int t0 = blockIdx.x * CHUNK0, nt = min(CHUNK0, T0 - t0);
  const int ns = (nt - 1) * 5 + 10;
  for (int i = threadIdx.x; i < ns; i += 256) s[i] = x[(int64_t)t0 * 5 + i];
  __syncthreads();
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const int c = threadIdx.x + 256 * h;
    float w[10];
#pragma unroll
    for (int j = 0; j < 10; ++j) w[j] = w0[c * 10 + j];
    float mean = 0.f, m2 = 0.f;
    for (int t = 0; t < nt; ++t) {
      const float y = conv0_at(s, w, t);
      const float dl = y - mean;
      mean += dl / (float)(t + 1);
      m2 += dl * (y - mean);
    }
    float2* p = reinterpret_cast<float2*>(part) + (size_t)blockIdx.x * C0 + c;
    *p = make_float2(mean, m2);
  }
}
// per channel: merge the chunks' (mean, M2) in chunk order (Chan et al.), GroupNorm eps 1e-5 -> (scale, shift) with the affine folded
__global__ void sv_conv0_norm_kernel(const float* __restrict__ part, const float* __restrict__ gamma, const float* __restrict__ beta,
                                     float* __restrict__ ss, int T0, int n_chunks) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= C0) return;
  float n = 0.f, mean = 0.f, m2 = 0.f;
  for (int k = 0; k < n_chunks; ++k) {
    const float2 p = reinterpret_cast<const float2*>(part)[(size_t)k * C0 + c];
    const float nb = (float)min(CHUNK0, T0 - k * CHUNK0), nn = n + nb;
    const float dl = p.x - mean;
    mean += dl * (nb / nn);
    m2 += p.y + dl * dl * (n * nb / nn);
    n = nn;
  }
  const float rstd = 1.0f / sqrtf(m2 / n + 1e-5f);
  const float sc = rstd * gamma[c];
  ss[c] = sc;
  ss[C0 + c] = beta[c] - mean * sc;
}
__global__ __launch_bounds__(256) void sv_conv0_apply_kernel(const float* __restrict__ x, const float* __restrict__ w0, const float* __restrict__ ss,
                                                             f16* __restrict__ y, int T0) {
  __shared__ float s[CHUNK0 * 5 + 5];
  const int t0 = blockIdx.x * CHUNK0, nt = min(CHUNK0, T0 - t0);
  const int ns = (nt - 1) * 5 + 10;
  for (int i = threadIdx.x; i < ns; i += 256) s[i] = x[(int64_t)t0 * 5 + i];
  __syncthreads();
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const int c = threadIdx.x + 256 * h;
    float w[10];
#pragma unroll
    for (int j = 0; j < 10; ++j) w[j] = w0[c * 10 + j];
    const float sc = ss[c], sh = ss[C0 + c];
    for (int t = 0; t < nt; ++t) y[(size_t)(t0 + t) * C0 + c] = (f16)gelu_f(conv0_at(s, w, t) * sc + sh);
  }
}

// ---- LayerNorm over rows (one wave per row, d = 64 NV) ----------------------------------------------------------------------------
// x (f16 or f32) -> y16 (f16) and optionally y32 (f32); wmode 1: ws = wl * y32-value, 2: ws += wl * value (the weighted layer sum,
// fp32), ws16 (optional): f16 copy of the updated ws
template <int NV, bool IN16>
__global__ __launch_bounds__(256) void sv_ln_kernel(const void* __restrict__ xv, const float* __restrict__ g, const float* __restrict__ b,
                                                    f16* __restrict__ y16, float* __restrict__ y32, float* __restrict__ ws, f16* __restrict__ ws16,
                                                    float wl, int wmode, int M, float eps) {
  const int lane = threadIdx.x & 63, row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= M) return;
  constexpr int d = 64 * NV;
  float v[NV];
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    const size_t o = (size_t)row * d + lane + 64 * i;
    v[i] = IN16 ? (float)reinterpret_cast<const f16*>(xv)[o] : reinterpret_cast<const float*>(xv)[o];
    s += v[i];
  }
  const float mean = wave_sum(s) / (float)d;
  float q = 0.f;
#pragma unroll
  for (int i = 0; i < NV; ++i) { const float a = v[i] - mean; q += a * a; }
  const float rstd = 1.0f / sqrtf(wave_sum(q) / (float)d + eps);
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    const int c = lane + 64 * i;
    const size_t o = (size_t)row * d + c;
    const float r = (v[i] - mean) * rstd * g[c] + b[c];
    y16[o] = (f16)r;
    if (y32) y32[o] = r;
    if (wmode) {
      const float a = wmode == 1 ? wl * r : ws[o] + wl * r;
      ws[o] = a;
      if (ws16) ws16[o] = (f16)a;
    }
  }
}

// ---- positional convolution (MFMA 16x16x16 f16) -----------------------------------------------------------------------------------
// out[t][o] = x[t][o] + GELU(bias[o] + sum_{k, c} W[o][k][c] x[t + k - 64][g 48 + c]),  o = g 48 + oo.  One wave: 16 frames x the 48
// outputs of one group; A = x rows (f32 -> f16 on load, zero outside [0, T)), B = W [768][128][48] f16 (weight norm folded at load).
// MFMA 16x16x16 layouts: A lane l holds A[l % 16][4 (l / 16) + i], B lane l holds B[4 (l / 16) + i][l % 16], D lane l holds
// D[4 (l / 16) + i][l % 16].
__global__ __launch_bounds__(64) void sv_posconv_kernel(const float* __restrict__ x, const f16* __restrict__ W, const float* __restrict__ bias,
                                                        float* __restrict__ out, int T) {
  const int lane = threadIdx.x, g = blockIdx.y, t0 = blockIdx.x * 16;
  const int r = lane & 15, kq = (lane >> 4) * 4;
  f32x4 acc[3];
#pragma unroll
  for (int j = 0; j < 3; ++j) acc[j] = f32x4{0.f, 0.f, 0.f, 0.f};
  const int trow = t0 + r;
  for (int k = 0; k < PK; ++k) {
    const int ts = trow + k - PK / 2;
    const bool ok = ts >= 0 && ts < T;
    const float* xr = x + (size_t)(ok ? ts : 0) * D + g * PCG + kq;
#pragma unroll
    for (int cb = 0; cb < 3; ++cb) {
      const float4 a4 = *reinterpret_cast<const float4*>(xr + cb * 16);
      f16x4 a = {(f16)(ok ? a4.x : 0.f), (f16)(ok ? a4.y : 0.f), (f16)(ok ? a4.z : 0.f), (f16)(ok ? a4.w : 0.f)};
#pragma unroll
      for (int ob = 0; ob < 3; ++ob) {
        const int o = g * PCG + ob * 16 + r;
        const f16x4 bw = *reinterpret_cast<const f16x4*>(W + ((size_t)o * PK + k) * PCG + cb * 16 + kq);
        acc[ob] = __builtin_amdgcn_mfma_f32_16x16x16f16(a, bw, acc[ob], 0, 0, 0);
      }
    }
  }
#pragma unroll
  for (int ob = 0; ob < 3; ++ob) {
    const int o = g * PCG + ob * 16 + r;
    const float bo = bias[o];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int t = t0 + kq + i;
      if (t < T) out[(size_t)t * D + o] = x[(size_t)t * D + o] + gelu_f(acc[ob][i] + bo);
    }
  }
}

// ---- attention with the gated relative position bias ------------------------------------------------------------------------------
// score(q, key) = Q[q] . K[key] (Q pre-scaled by 1/8 in the projection) + gate[h][q] * tab[h][key - q + L - 1], softmax over keys.
// One wave = 16 queries of one head; keys in blocks of 16, online softmax.  S^T = K Q^T puts the 4 keys of a lane beside ONE query
// (l % 16), so the row statistics are a 4-register + 2-shuffle reduction and P^T is already the B operand of O^T += V^T P^T.
// gate[h][q] = a (b c_h - 1) + 2,  (a, b) = sigmoid of the pair sums of gru_rel_pos_linear(x[q][64 h .. 64 h + 63]) (the layer input).
__global__ __launch_bounds__(64) void sv_attn_kernel(const f16* __restrict__ qkv, const float* __restrict__ xin, const float* __restrict__ gw,
                                                     const float* __restrict__ gb, const float* __restrict__ gconst, const float* __restrict__ tab,
                                                     int L, f16* __restrict__ out, int T) {
  const int lane = threadIdx.x, h = blockIdx.y, q0 = blockIdx.x * 16;
  const int r = lane & 15, kq = (lane >> 4) * 4, grp = lane >> 4;
  const int q = q0 + r, qc = q < T ? q : T - 1;
  constexpr int LD = 3 * D;
  // gate of query q (every lane of column r ends with it)
  float gate;
  {
    const float* xr = xin + (size_t)qc * D + h * DH;
    float o0 = gb[2 * grp], o1 = gb[2 * grp + 1];
    const float* w0 = gw + (2 * grp) * DH;
    const float* w1 = w0 + DH;
    for (int k = 0; k < DH; ++k) { const float xv = xr[k]; o0 += w0[k] * xv; o1 += w1[k] * xv; }
    float s = o0 + o1;
    s += __shfl_xor(s, 16);               // groups (0, 1): outputs 0..3, groups (2, 3): outputs 4..7
    const float sg = 1.0f / (1.0f + expf(-s));
    const float other = __shfl_xor(sg, 32);
    const float ga = grp < 2 ? sg : other, gbv = grp < 2 ? other : sg;
    gate = ga * (gbv * gconst[h] - 1.0f) + 2.0f;
  }
  f16x4 qf[4];
#pragma unroll
  for (int kk = 0; kk < 4; ++kk) qf[kk] = *reinterpret_cast<const f16x4*>(qkv + (size_t)qc * LD + h * DH + kk * 16 + kq);
  const float* th = tab + (size_t)h * (2 * L - 1) + (L - 1);
  f32x4 o[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) o[j] = f32x4{0.f, 0.f, 0.f, 0.f};
  float m = -INFINITY, l = 0.f;
  for (int k0 = 0; k0 < T; k0 += 16) {
    const int kr = min(k0 + r, T - 1);
    f32x4 s = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) {
      const f16x4 kf = *reinterpret_cast<const f16x4*>(qkv + (size_t)kr * LD + D + h * DH + kk * 16 + kq);
      s = __builtin_amdgcn_mfma_f32_16x16x16f16(kf, qf[kk], s, 0, 0, 0);
    }
    float sv[4], bm = -INFINITY;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int key = k0 + kq + i;
      sv[i] = key < T ? s[i] + gate * th[min(key, T - 1) - qc] : -INFINITY;
      bm = fmaxf(bm, sv[i]);
    }
    bm = fmaxf(bm, __shfl_xor(bm, 16));
    bm = fmaxf(bm, __shfl_xor(bm, 32));
    const float mn = fmaxf(m, bm);
    const float alpha = expf(m - mn);
    m = mn;
    f16x4 pf;
    float ps = 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i) { const float p = expf(sv[i] - mn); ps += p; pf[i] = (f16)p; }
    ps += __shfl_xor(ps, 16);
    ps += __shfl_xor(ps, 32);
    l = l * alpha + ps;
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) {
      f16x4 vf;
#pragma unroll
      for (int i = 0; i < 4; ++i) vf[i] = qkv[(size_t)min(k0 + kq + i, T - 1) * LD + 2 * D + h * DH + dt * 16 + r];
      o[dt] = scale4(o[dt], alpha);
      o[dt] = __builtin_amdgcn_mfma_f32_16x16x16f16(vf, pf, o[dt], 0, 0, 0);
    }
  }
  if (q >= T) return;
  const float inv = 1.0f / l;
#pragma unroll
  for (int dt = 0; dt < 4; ++dt) {
    // O^T lane layout: d = dt 16 + 4 (l / 16) + i for query l % 16 -> four consecutive features of row q
    f16x4 v = {(f16)(o[dt][0] * inv), (f16)(o[dt][1] * inv), (f16)(o[dt][2] * inv), (f16)(o[dt][3] * inv)};
    *reinterpret_cast<f16x4*>(out + (size_t)q * D + h * DH + dt * 16 + kq) = v;
  }
}
// tab[h][r] = E[bucket[r]][h], r = key - query + L - 1
__global__ void sv_bias_table_kernel(const float* __restrict__ E, const int* __restrict__ bucket, float* __restrict__ tab, int L) {
  const int n = 2 * L - 1;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < H * n; i += gridDim.x * blockDim.x) {
    const int h = i / n, r = i - h * n;
    tab[i] = E[bucket[r] * H + h];
  }
}

// ---- x-vector head --------------------------------------------------------------------------------------------------------------
// g[t][j C + c] = ReLU(z[t + j dil][c])  (z f32 [..][ldz]); k = 1 is the plain ReLU + f16 conversion
__global__ void sv_relu_gather_kernel(const float* __restrict__ z, int ldz, f16* __restrict__ g, int Tout, int C, int k, int dil) {
  const int64_t total = (int64_t)Tout * k * C;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t t = i / (k * C);
    const int rem = (int)(i - t * k * C), j = rem / C, c = rem - j * C;
    g[i] = (f16)fmaxf(z[(t + (int64_t)j * dil) * ldz + c], 0.f);
  }
}
// statistics pooling of ReLU(z) over T rows: s[c] = mean, s[n + c] = unbiased std (two passes per channel)
__global__ void sv_stats_kernel(const float* __restrict__ z, int ldz, float* __restrict__ s, int T, int n) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= n) return;
  float a = 0.f;
  for (int t = 0; t < T; ++t) a += fmaxf(z[(size_t)t * ldz + c], 0.f);
  const float mean = a / (float)T;
  float q = 0.f;
  for (int t = 0; t < T; ++t) { const float e = fmaxf(z[(size_t)t * ldz + c], 0.f) - mean; q += e * e; }
  s[c] = mean;
  s[n + c] = sqrtf(q / (float)(T - 1));
}
// y[o] = b[o] + W[o] . x   (fp32, one wave per output)
__global__ __launch_bounds__(256) void sv_linear_kernel(const float* __restrict__ x, const float* __restrict__ W, const float* __restrict__ b,
                                                        float* __restrict__ y, int N, int K) {
  const int lane = threadIdx.x & 63, o = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (o >= N) return;
  float a = 0.f;
  for (int k = lane; k < K; k += 64) a += W[(size_t)o * K + k] * x[k];
  a = wave_sum(a);
  if (lane == 0) y[o] = a + b[o];
}
// weight conversion: src (f16 | f32) n elements -> dst (f16 | f32), times `scale`
__global__ void sv_convert_kernel(const void* __restrict__ src, int src_f16, void* __restrict__ dst, int dst_f16, int64_t n, float scale) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const float v = (src_f16 ? (float)reinterpret_cast<const f16*>(src)[i] : reinterpret_cast<const float*>(src)[i]) * scale;
    if (dst_f16) reinterpret_cast<f16*>(dst)[i] = (f16)v; else reinterpret_cast<float*>(dst)[i] = v;
  }
}

}  // namespace

// ---- host side ----------------------------------------------------------------------------------------------------------------------
struct SvLayer {
  f16 *w_qkv, *w_out, *w_f1, *w_f2;
  float *b_qkv, *b_out, *b_f1, *b_f2, *ln1_g, *ln1_b, *ln2_g, *ln2_b, *gw, *gb, *gconst;
};
struct wis_sv {
  wis_sv_config_t cfg;
  int device = 0;
  hipStream_t st = nullptr;
  std::vector<void*> allocs;
  size_t bytes = 0;
  int64_t max_samples = 0;
  int T0max = 0, Tmax = 0;
  // weights
  float *w_conv0, *gn_g, *gn_b;
  f16* w_conv[6];
  float *fp_ln_g, *fp_ln_b, *b_fp; f16* w_fp;
  f16* w_pos; float *b_pos, *enc_ln_g, *enc_ln_b;
  float* tab;                      // [H][2 Tmax - 1] relative position bias (layer 0's embedding, shared by all layers)
  SvLayer L[NL];
  float lw[NL + 1];                // softmax(layer_weights)
  f16* w_proj; float* b_proj;
  f16* w_td[NTD]; float* b_td[NTD];
  float *w_fe, *b_fe;
  // activations
  float* pcm; float* c0part; float* c0ss;
  f16 *fa, *fb;                    // feature-encoder ping-pong [T0max][512]
  f16* xn512; float* x32; float* x32b; float* h; f16* hn; float* h1; f16* hn1;
  f16* qkv; f16* ao; f16* ff; float* ws; f16* ws16;
  f16* pj; float* z; f16* gbuf; float* stats; float* emb;
  float* zero;                     // [512] zeros: the bias of the bias-free conv GEMMs
  f16* feat_out;                   // conv features of the last run (= fa or fb)
  int T = 0, T_td = 0;
};

namespace {

template <class T>
int sv_alloc(wis_sv* s, T** p, size_t n) {
  size_t b = n * sizeof(T); if (!b) b = 16;
  void* q = nullptr;
  if (hipMalloc(&q, b) != hipSuccess) { set_error("wis_sv: hipMalloc(%zu) failed", b); return WIS_E_NOMEM; }
  s->allocs.push_back(q); s->bytes += b; *p = static_cast<T*>(q);
  return WIS_OK;
}

struct SvLoader {
  const wis_tensor_t* t; int n; const char* base; size_t arena_bytes; int on_device;
  int get(const std::string& name, int64_t ne, const void** p, int* f16) const {
    for (int i = 0; i < n; ++i) {
      if (name != t[i].name) continue;
      int64_t k = 1; for (int r = 0; r < t[i].rank; ++r) k *= t[i].shape[r];
      if (k != ne) { set_error("wis_sv: weight '%s': %lld elements, expected %lld", name.c_str(), (long long)k, (long long)ne); return WIS_E_FORMAT; }
      if (t[i].dtype != WIS_DT_F16 && t[i].dtype != WIS_DT_F32) { set_error("wis_sv: weight '%s': dtype %d unsupported", name.c_str(), t[i].dtype); return WIS_E_FORMAT; }
      const size_t es = t[i].dtype == WIS_DT_F16 ? 2 : 4;
      if (t[i].offset + (size_t)ne * es > arena_bytes) { set_error("wis_sv: weight '%s' exceeds the arena", name.c_str()); return WIS_E_FORMAT; }
      *p = base + t[i].offset; *f16 = t[i].dtype == WIS_DT_F16;
      return WIS_OK;
    }
    set_error("wis_sv: weight '%s' missing from the index", name.c_str());
    return WIS_E_FORMAT;
  }
};

// tensor -> device buffer (dst preset: write into it, e.g. a slice of a concatenated matrix)
template <class T>
int sv_load(wis_sv* s, const SvLoader& Ld, const std::string& name, int64_t ne, T** dst, float scale = 1.f, int64_t alloc_ne = 0) {
  const void* p; int f16; WIS_RET(Ld.get(name, ne, &p, &f16));
  if (!*dst) {
    WIS_RET(sv_alloc(s, dst, (size_t)(alloc_ne > ne ? alloc_ne : ne)));
    if (alloc_ne > ne) WIS_HIP_CHECK(hipMemsetAsync(*dst, 0, (size_t)alloc_ne * sizeof(T), s->st));
  }
  hipLaunchKernelGGL(sv_convert_kernel, dim3(blocks_for(ne)), dim3(256), 0, s->st, p, f16, static_cast<void*>(*dst), (int)(sizeof(T) == 2), ne, scale);
  return WIS_OK;
}

int sv_check_config(const wis_sv_config_t* c) {
  bool ok = c->conv_dim == C0 && c->n_conv_layers == 7 && c->hidden_size == D && c->n_heads == H && c->n_layers == NL &&
            c->intermediate_size == FF && c->num_conv_pos_embeddings == PK && c->num_conv_pos_embedding_groups == PG &&
            c->num_buckets == 320 && c->max_bucket_distance == 800 && c->n_tdnn == NTD && c->xvector_output_dim == XV &&
            c->max_samples >= 0 && c->max_samples <= (int64_t)16000 * 60;
  for (int i = 0; ok && i < 7; ++i) ok = c->conv_kernel[i] == CONV_K[i] && c->conv_stride[i] == CONV_S[i];
  for (int i = 0; ok && i < NTD; ++i) ok = c->tdnn_dim[i] == TD_DIM[i] && c->tdnn_kernel[i] == TD_K[i] && c->tdnn_dilation[i] == TD_DIL[i];
  return ok;
}

// frames after the feature encoder for n samples (0: too short for a stage)
int sv_frames(int64_t n, int* t0_out = nullptr) {
  int64_t t = n;
  for (int i = 0; i < 7; ++i) {
    if (t < CONV_K[i]) return 0;
    t = (t - CONV_K[i]) / CONV_S[i] + 1;
    if (i == 0 && t0_out) *t0_out = (int)t;
  }
  return (int)t;
}
int td_reduction() { int r = 0; for (int i = 0; i < NTD; ++i) r += (TD_K[i] - 1) * TD_DIL[i]; return r; }

int sv_load_weights(wis_sv* s, const SvLoader& Ld) {
  const std::string fe = "wavlm.feature_extractor.conv_layers.";
  WIS_RET(sv_load(s, Ld, fe + "0.conv.weight", (int64_t)C0 * 10, &s->w_conv0));
  WIS_RET(sv_load(s, Ld, fe + "0.layer_norm.weight", C0, &s->gn_g));
  WIS_RET(sv_load(s, Ld, fe + "0.layer_norm.bias", C0, &s->gn_b));
  for (int i = 1; i < 7; ++i) { s->w_conv[i - 1] = nullptr; WIS_RET(sv_load(s, Ld, fe + std::to_string(i) + ".conv.weight", (int64_t)C0 * C0 * CONV_K[i], &s->w_conv[i - 1])); }
  WIS_RET(sv_load(s, Ld, "wavlm.feature_projection.layer_norm.weight", C0, &s->fp_ln_g));
  WIS_RET(sv_load(s, Ld, "wavlm.feature_projection.layer_norm.bias", C0, &s->fp_ln_b));
  WIS_RET(sv_load(s, Ld, "wavlm.feature_projection.projection.weight", (int64_t)D * C0, &s->w_fp));
  WIS_RET(sv_load(s, Ld, "wavlm.feature_projection.projection.bias", D, &s->b_fp));
  WIS_RET(sv_load(s, Ld, "wavlm.encoder.pos_conv_embed.conv.weight", (int64_t)D * PCG * PK, &s->w_pos));
  WIS_RET(sv_load(s, Ld, "wavlm.encoder.pos_conv_embed.conv.bias", D, &s->b_pos));
  WIS_RET(sv_load(s, Ld, "wavlm.encoder.layer_norm.weight", D, &s->enc_ln_g));
  WIS_RET(sv_load(s, Ld, "wavlm.encoder.layer_norm.bias", D, &s->enc_ln_b));
  for (int l = 0; l < NL; ++l) {
    SvLayer& w = s->L[l];
    memset(&w, 0, sizeof(w));
    const std::string p = "wavlm.encoder.layers." + std::to_string(l) + ".";
    WIS_RET(sv_alloc(s, &w.w_qkv, (size_t)3 * D * D));
    WIS_RET(sv_alloc(s, &w.b_qkv, (size_t)3 * D));
    f16* wq = w.w_qkv; f16* wk = w.w_qkv + (size_t)D * D; f16* wv = w.w_qkv + (size_t)2 * D * D;
    float* bq = w.b_qkv; float* bk = w.b_qkv + D; float* bv = w.b_qkv + 2 * D;
    const float qs = 0.125f;      // head_dim ** -0.5, applied to q = x Wq^T + bq (exact in f16)
    WIS_RET(sv_load(s, Ld, p + "attention.q_proj.weight", (int64_t)D * D, &wq, qs));
    WIS_RET(sv_load(s, Ld, p + "attention.k_proj.weight", (int64_t)D * D, &wk));
    WIS_RET(sv_load(s, Ld, p + "attention.v_proj.weight", (int64_t)D * D, &wv));
    WIS_RET(sv_load(s, Ld, p + "attention.q_proj.bias", D, &bq, qs));
    WIS_RET(sv_load(s, Ld, p + "attention.k_proj.bias", D, &bk));
    WIS_RET(sv_load(s, Ld, p + "attention.v_proj.bias", D, &bv));
    WIS_RET(sv_load(s, Ld, p + "attention.out_proj.weight", (int64_t)D * D, &w.w_out));
    WIS_RET(sv_load(s, Ld, p + "attention.out_proj.bias", D, &w.b_out));
    WIS_RET(sv_load(s, Ld, p + "attention.gru_rel_pos_linear.weight", 8 * DH, &w.gw));
    WIS_RET(sv_load(s, Ld, p + "attention.gru_rel_pos_linear.bias", 8, &w.gb));
    WIS_RET(sv_load(s, Ld, p + "attention.gru_rel_pos_const", H, &w.gconst));
    WIS_RET(sv_load(s, Ld, p + "layer_norm.weight", D, &w.ln1_g));
    WIS_RET(sv_load(s, Ld, p + "layer_norm.bias", D, &w.ln1_b));
    WIS_RET(sv_load(s, Ld, p + "feed_forward.intermediate_dense.weight", (int64_t)FF * D, &w.w_f1));
    WIS_RET(sv_load(s, Ld, p + "feed_forward.intermediate_dense.bias", FF, &w.b_f1));
    WIS_RET(sv_load(s, Ld, p + "feed_forward.output_dense.weight", (int64_t)D * FF, &w.w_f2));
    WIS_RET(sv_load(s, Ld, p + "feed_forward.output_dense.bias", D, &w.b_f2));
    WIS_RET(sv_load(s, Ld, p + "final_layer_norm.weight", D, &w.ln2_g));
    WIS_RET(sv_load(s, Ld, p + "final_layer_norm.bias", D, &w.ln2_b));
  }
  // relative position bias table of the largest T: depends on key - query only
  {
    const int L = s->Tmax, n = 2 * L - 1;
    std::vector<int32_t> bk(n);
    WIS_RET(wis_sv_rel_buckets(s->cfg.num_buckets, s->cfg.max_bucket_distance, -(L - 1), n, bk.data()));
    float* E = nullptr; int* dbk = nullptr;
    WIS_RET(sv_load(s, Ld, "wavlm.encoder.layers.0.attention.rel_attn_embed.weight", (int64_t)320 * H, &E));
    WIS_RET(sv_alloc(s, &dbk, (size_t)n));
    WIS_RET(sv_alloc(s, &s->tab, (size_t)H * n));
    WIS_HIP_CHECK(hipMemcpyAsync(dbk, bk.data(), (size_t)n * 4, hipMemcpyHostToDevice, s->st));
    hipLaunchKernelGGL(sv_bias_table_kernel, dim3(blocks_for((int64_t)H * n)), dim3(256), 0, s->st, E, dbk, s->tab, L);
    WIS_HIP_CHECK(hipStreamSynchronize(s->st));       // (bk leaves scope)
  }
  // softmax(layer_weights) on the host: the per-layer LayerNorm launches take it as an argument
  {
    const void* p; int f16;
    WIS_RET(Ld.get("layer_weights", NL + 1, &p, &f16));
    std::vector<char> raw((size_t)(NL + 1) * (f16 ? 2 : 4));
    if (Ld.on_device) WIS_HIP_CHECK(hipMemcpy(raw.data(), p, raw.size(), hipMemcpyDeviceToHost));
    else memcpy(raw.data(), p, raw.size());
    double v[NL + 1], mx = -1e300, sum = 0.0;
    for (int i = 0; i <= NL; ++i) {
      v[i] = f16 ? (double)(float)reinterpret_cast<const _Float16*>(raw.data())[i] : (double)reinterpret_cast<const float*>(raw.data())[i];
      if (v[i] > mx) mx = v[i];
    }
    for (int i = 0; i <= NL; ++i) { v[i] = exp(v[i] - mx); sum += v[i]; }
    for (int i = 0; i <= NL; ++i) s->lw[i] = (float)(v[i] / sum);
  }
  WIS_RET(sv_load(s, Ld, "projector.weight", (int64_t)TD_DIM[0] * D, &s->w_proj));
  WIS_RET(sv_load(s, Ld, "projector.bias", TD_DIM[0], &s->b_proj));
  for (int i = 0; i < NTD; ++i) {
    const int in = i ? TD_DIM[i - 1] : TD_DIM[0], out = TD_DIM[i], outp = i == NTD - 1 ? TD_LAST_PAD : out;
    s->w_td[i] = nullptr; s->b_td[i] = nullptr;
    WIS_RET(sv_load(s, Ld, "tdnn." + std::to_string(i) + ".kernel.weight", (int64_t)out * in * TD_K[i], &s->w_td[i], 1.f, (int64_t)outp * in * TD_K[i]));
    WIS_RET(sv_load(s, Ld, "tdnn." + std::to_string(i) + ".kernel.bias", out, &s->b_td[i], 1.f, outp));
  }
  WIS_RET(sv_load(s, Ld, "feature_extractor.weight", (int64_t)XV * 2 * TD_DIM[NTD - 1], &s->w_fe));
  WIS_RET(sv_load(s, Ld, "feature_extractor.bias", XV, &s->b_fe));
  return WIS_OK;
}

int sv_alloc_buffers(wis_sv* s) {
  const int T0 = s->T0max, T = s->Tmax;
  WIS_RET(sv_alloc(s, &s->pcm, (size_t)s->max_samples));
  WIS_RET(sv_alloc(s, &s->c0part, (size_t)cdiv(T0, CHUNK0) * C0 * 2));
  WIS_RET(sv_alloc(s, &s->c0ss, (size_t)2 * C0));
  WIS_RET(sv_alloc(s, &s->fa, (size_t)T0 * C0));
  WIS_RET(sv_alloc(s, &s->fb, (size_t)((T0 - 3) / 2 + 1) * C0));
  WIS_RET(sv_alloc(s, &s->xn512, (size_t)T * C0));
  WIS_RET(sv_alloc(s, &s->x32, (size_t)T * D));
  WIS_RET(sv_alloc(s, &s->x32b, (size_t)T * D));
  WIS_RET(sv_alloc(s, &s->h, (size_t)T * D));
  WIS_RET(sv_alloc(s, &s->hn, (size_t)T * D));
  WIS_RET(sv_alloc(s, &s->h1, (size_t)T * D));
  WIS_RET(sv_alloc(s, &s->hn1, (size_t)T * D));
  WIS_RET(sv_alloc(s, &s->qkv, (size_t)T * 3 * D));
  WIS_RET(sv_alloc(s, &s->ao, (size_t)T * D));
  WIS_RET(sv_alloc(s, &s->ff, (size_t)T * FF));
  WIS_RET(sv_alloc(s, &s->ws, (size_t)T * D));
  WIS_RET(sv_alloc(s, &s->ws16, (size_t)T * D));
  WIS_RET(sv_alloc(s, &s->pj, (size_t)T * TD_DIM[0]));
  WIS_RET(sv_alloc(s, &s->z, (size_t)T * TD_LAST_PAD));
  WIS_RET(sv_alloc(s, &s->gbuf, (size_t)T * 3 * 512));
  WIS_RET(sv_alloc(s, &s->stats, (size_t)2 * TD_DIM[NTD - 1]));
  WIS_RET(sv_alloc(s, &s->emb, (size_t)XV));
  WIS_RET(sv_alloc(s, &s->zero, (size_t)C0));
  WIS_HIP_CHECK(hipMemsetAsync(s->zero, 0, (size_t)C0 * 4, s->st));
  return WIS_OK;
}

template <bool IN16>
int sv_ln(hipStream_t st, const void* x, const float* g, const float* b, f16* y16, float* y32, float* ws, f16* ws16, float wl, int wmode, int M, int d) {
  const dim3 grid(cdiv(M, 4)), blk(256);
  if (d == 512) hipLaunchKernelGGL((sv_ln_kernel<8, IN16>), grid, blk, 0, st, x, g, b, y16, y32, ws, ws16, wl, wmode, M, 1e-5f);
  else if (d == 768) hipLaunchKernelGGL((sv_ln_kernel<12, IN16>), grid, blk, 0, st, x, g, b, y16, y32, ws, ws16, wl, wmode, M, 1e-5f);
  else { set_error("wis_sv: LayerNorm width %d", d); return WIS_E_UNSUPPORTED; }
  return WIS_OK;
}

// the launches sv_forward shares with the wis_op_sv_* entries (tests call each kernel through these, with the production grids)
void sv_launch_conv0(hipStream_t st, const float* pcm, const float* w0, const float* gamma, const float* beta, float* part, float* ss, f16* y, int T0) {
  const int nch = cdiv(T0, CHUNK0);
  hipLaunchKernelGGL(sv_conv0_stats_kernel, dim3(nch), dim3(256), 0, st, pcm, w0, part, T0);
  hipLaunchKernelGGL(sv_conv0_norm_kernel, dim3(C0 / 256), dim3(256), 0, st, part, gamma, beta, ss, T0, nch);
  hipLaunchKernelGGL(sv_conv0_apply_kernel, dim3(nch), dim3(256), 0, st, pcm, w0, ss, y, T0);
}
void sv_launch_posconv(hipStream_t st, const float* x, const f16* W, const float* bias, float* out, int T) {
  hipLaunchKernelGGL(sv_posconv_kernel, dim3(cdiv(T, 16), PG), dim3(64), 0, st, x, W, bias, out, T);
}
void sv_launch_attn(hipStream_t st, const f16* qkv, const float* xin, const float* gw, const float* gb, const float* gconst, const float* tab,
                    int L, f16* out, int T) {
  hipLaunchKernelGGL(sv_attn_kernel, dim3(cdiv(T, 16), H), dim3(64), 0, st, qkv, xin, gw, gb, gconst, tab, L, out, T);
}
// statistics pooling of ReLU(z[T][ldz]) over the first n columns -> stats [2n], then emb [XV] = W_fe stats + b_fe
void sv_launch_xvector_tail(hipStream_t st, const float* z, int ldz, int T, int n, const float* w_fe, const float* b_fe, float* stats, float* emb) {
  hipLaunchKernelGGL(sv_stats_kernel, dim3(cdiv(n, 256)), dim3(256), 0, st, z, ldz, stats, T, n);
  hipLaunchKernelGGL(sv_linear_kernel, dim3(cdiv(XV, 4)), dim3(256), 0, st, stats, w_fe, b_fe, emb, XV, 2 * n);
}

// the forward pass; stop_hidden >= 0: return after hidden state `stop_hidden` (0 = encoder input after the positional conv + LayerNorm,
// l = output of layer l) is in s->h
int sv_forward(wis_sv* s, int64_t n, int stop_hidden) {
  hipStream_t st = s->st;
  int T0 = 0;
  const int T = sv_frames(n, &T0);
  if (T - td_reduction() < 2) { set_error("wis_sv_embed: %lld samples leave %d frames, the x-vector head needs >= %d", (long long)n, T, td_reduction() + 2); return WIS_E_ARG; }
  s->T = T; s->T_td = T - td_reduction();
  // feature encoder
  sv_launch_conv0(st, s->pcm, s->w_conv0, s->gn_g, s->gn_b, s->c0part, s->c0ss, s->fa, T0);
  f16* src = s->fa; f16* dst = s->fb;
  int t = T0;
  for (int i = 1; i < 7; ++i) {
    const int to = (t - CONV_K[i]) / CONV_S[i] + 1;
    GemmP p = gemm_plain(src, CONV_S[i] * C0, s->w_conv[i - 1], to, C0, CONV_K[i] * C0);
    WIS_RET(launch_gemm_generic(st, p, s->zero, nullptr, dst, 1));      // GELU, no bias (conv_bias = False)
    f16* tmp = src; src = dst; dst = tmp; t = to;
  }
  s->feat_out = src;
  // feature projection, positional conv, encoder LayerNorm -> hidden state 0
  WIS_RET(sv_ln<true>(st, src, s->fp_ln_g, s->fp_ln_b, s->xn512, nullptr, nullptr, nullptr, 0.f, 0, T, C0));
  WIS_RET(launch_gemm_generic(st, gemm_plain(s->xn512, C0, s->w_fp, T, D, C0), s->b_fp, nullptr, s->x32, 4));
  sv_launch_posconv(st, s->x32, s->w_pos, s->b_pos, s->x32b, T);
  WIS_RET(sv_ln<false>(st, s->x32b, s->enc_ln_g, s->enc_ln_b, s->hn, s->h, s->ws, nullptr, s->lw[0], 1, T, D));
  if (stop_hidden == 0) return WIS_OK;
  for (int l = 0; l < NL; ++l) {
    const SvLayer& w = s->L[l];
    WIS_RET(launch_gemm_generic(st, gemm_plain(s->hn, D, w.w_qkv, T, 3 * D, D), w.b_qkv, nullptr, s->qkv, 0));
    sv_launch_attn(st, s->qkv, s->h, w.gw, w.gb, w.gconst, s->tab, s->Tmax, s->ao, T);
    WIS_RET(launch_gemm_generic(st, gemm_plain(s->ao, D, w.w_out, T, D, D), w.b_out, s->h, s->x32, 2 | 4));
    WIS_RET(sv_ln<false>(st, s->x32, w.ln1_g, w.ln1_b, s->hn1, s->h1, nullptr, nullptr, 0.f, 0, T, D));
    WIS_RET(launch_gemm_generic(st, gemm_plain(s->hn1, D, w.w_f1, T, FF, D), w.b_f1, nullptr, s->ff, 1));
    WIS_RET(launch_gemm_generic(st, gemm_plain(s->ff, FF, w.w_f2, T, D, FF), w.b_f2, s->h1, s->x32, 2 | 4));
    const bool last = l + 1 == NL;
    WIS_RET(sv_ln<false>(st, s->x32, w.ln2_g, w.ln2_b, s->hn, s->h, s->ws, last ? s->ws16 : nullptr, s->lw[l + 1], 2, T, D));
    if (stop_hidden == l + 1) return WIS_OK;
  }
  // x-vector head
  WIS_RET(launch_gemm_generic(st, gemm_plain(s->ws16, D, s->w_proj, T, TD_DIM[0], D), s->b_proj, nullptr, s->pj, 0));
  const f16* a = s->pj; int lda = TD_DIM[0];
  t = T;
  for (int i = 0; i < NTD; ++i) {
    const int in = i ? TD_DIM[i - 1] : TD_DIM[0], K = TD_K[i] * in, N = i == NTD - 1 ? TD_LAST_PAD : TD_DIM[i];
    const int to = t - (TD_K[i] - 1) * TD_DIL[i];
    // dilation 1: im2col row u is the span a + u lda of length K (lda = in); else the gather below built [to][K] rows
    WIS_RET(launch_gemm_generic(st, gemm_plain(a, lda, s->w_td[i], to, N, K), s->b_td[i], nullptr, s->z, 4));
    t = to;
    if (i + 1 < NTD) {
      const int kn = TD_K[i + 1], dn = TD_DIL[i + 1], tn = t - (kn - 1) * dn;
      if (dn == 1) {       // plain ReLU image; the next GEMM reads it with lda = C (k taps overlap)
        hipLaunchKernelGGL(sv_relu_gather_kernel, dim3(blocks_for((int64_t)t * TD_DIM[i])), dim3(256), 0, st, s->z, N, s->gbuf, t, TD_DIM[i], 1, 1);
        lda = TD_DIM[i];
      } else {
        hipLaunchKernelGGL(sv_relu_gather_kernel, dim3(blocks_for((int64_t)tn * kn * TD_DIM[i])), dim3(256), 0, st, s->z, N, s->gbuf, tn, TD_DIM[i], kn, dn);
        lda = kn * TD_DIM[i];
      }
      a = s->gbuf;
    }
  }
  sv_launch_xvector_tail(st, s->z, TD_LAST_PAD, t, TD_DIM[NTD - 1], s->w_fe, s->b_fe, s->stats, s->emb);
  return WIS_OK;
}

int sv_upload(wis_sv* s, const float* pcm, int64_t n) {
  if (!pcm || n <= 0) { set_error("wis_sv_embed: bad argument"); return WIS_E_ARG; }
  if (n > s->max_samples) { set_error("wis_sv_embed: %lld samples exceed the handle's %lld", (long long)n, (long long)s->max_samples); return WIS_E_STATE; }
  WIS_HIP_CHECK(hipSetDevice(s->device));
  WIS_HIP_CHECK(hipMemcpyAsync(s->pcm, pcm, (size_t)n * 4, hipMemcpyHostToDevice, s->st));
  return WIS_OK;
}

}  // namespace

extern "C" {

int wis_sv_rel_buckets(int num_buckets, int max_distance, int first, int n, int32_t* out) {
  if (!out || n < 0 || num_buckets < 4 || max_distance <= num_buckets / 4) { set_error("wis_sv_rel_buckets: bad argument"); return WIS_E_ARG; }
  // HF WavLMAttention._relative_positions_bucket in float32 arithmetic, as torch evaluates it
  const int nb = num_buckets / 2, max_exact = nb / 2;
  const float denom = (float)log((double)max_distance / (double)max_exact);
  for (int i = 0; i < n; ++i) {
    const int r = first + i, a = r < 0 ? -r : r;
    int b = r > 0 ? nb : 0;
    if (a < max_exact) b += a;
    else {
      float v = logf((float)a / (float)max_exact);
      v = v / denom;
      v = v * (float)(nb - max_exact);
      v = (float)max_exact + v;
      const int big = (int)v;
      b += big < nb - 1 ? big : nb - 1;
    }
    out[i] = b;
  }
  return WIS_OK;
}

int wis_sv_create(const wis_sv_config_t* cfg, const void* arena, size_t arena_bytes, int arena_on_device, const wis_tensor_t* tensors,
                  int n_tensors, int device, wis_sv_t** out) {
  if (!cfg || !arena || !tensors || !out || n_tensors <= 0) { set_error("wis_sv_create: bad argument"); return WIS_E_ARG; }
  if (!sv_check_config(cfg)) {
    set_error("wis_sv_create: unsupported architecture (WavLM-base-plus-sv only: 7 conv layers of 512, hidden 768 x 12 layers x 12 heads, "
              "positional conv k128 g16, 320 buckets / 800, TDNN 512,512,512,512,1500 k5,3,3,1,1 d1,2,3,1,1, x-vector 512)");
    return WIS_E_UNSUPPORTED;
  }
  wis_sv* s = new wis_sv();
  s->cfg = *cfg; s->device = device;
  s->max_samples = cfg->max_samples ? cfg->max_samples : 160000;
  s->Tmax = sv_frames(s->max_samples, &s->T0max);
  int rc = WIS_OK;
  void* d_arena = nullptr;
  do {
    if (s->Tmax - td_reduction() < 2) { set_error("wis_sv_create: max_samples %lld too small", (long long)s->max_samples); rc = WIS_E_ARG; break; }
    if (hipSetDevice(device) != hipSuccess) { set_error("wis_sv_create: no HIP device %d", device); rc = WIS_E_HIP; break; }
    if (hipStreamCreateWithFlags(&s->st, hipStreamNonBlocking) != hipSuccess) { set_error("wis_sv_create: stream create failed"); rc = WIS_E_HIP; break; }
    const char* base = static_cast<const char*>(arena);
    if (!arena_on_device) {
      if (hipMalloc(&d_arena, arena_bytes) != hipSuccess) { set_error("wis_sv_create: hipMalloc(arena %zu) failed", arena_bytes); rc = WIS_E_NOMEM; break; }
      if (hipMemcpy(d_arena, arena, arena_bytes, hipMemcpyHostToDevice) != hipSuccess) { set_error("wis_sv_create: arena upload failed"); rc = WIS_E_HIP; break; }
      base = static_cast<const char*>(d_arena);
    }
    SvLoader Ld{tensors, n_tensors, base, arena_bytes, 1};
    if ((rc = sv_load_weights(s, Ld))) break;
    if ((rc = sv_alloc_buffers(s))) break;
    if (hipStreamSynchronize(s->st) != hipSuccess) { set_error("wis_sv_create: init failed"); rc = WIS_E_HIP; break; }
  } while (0);
  if (d_arena) hipFree(d_arena);
  if (rc) { wis_sv_destroy(s); return rc; }
  *out = s;
  return WIS_OK;
}

void wis_sv_destroy(wis_sv_t* s) {
  if (!s) return;
  hipSetDevice(s->device);
  if (s->st) hipStreamSynchronize(s->st);
  for (void* p : s->allocs) hipFree(p);
  if (s->st) hipStreamDestroy(s->st);
  delete s;
}

size_t wis_sv_device_bytes(const wis_sv_t* s) { return s ? s->bytes : 0; }

int wis_sv_embed(wis_sv_t* s, const float* pcm, int64_t n, float* emb) {
  if (!s || !emb) { set_error("wis_sv_embed: bad argument"); return WIS_E_ARG; }
  WIS_RET(sv_upload(s, pcm, n));
  WIS_RET(sv_forward(s, n, -1));
  WIS_HIP_CHECK(hipMemcpyAsync(emb, s->emb, (size_t)XV * 4, hipMemcpyDeviceToHost, s->st));
  WIS_HIP_CHECK(hipStreamSynchronize(s->st));
  return WIS_OK;
}

int wis_debug_sv_taps(wis_sv_t* s, const float* pcm, int64_t n, int tap, int layer, float* out, int64_t cap, int32_t* rows, int32_t* cols) {
  if (!s || !out || !rows || !cols || tap < 0 || tap > 2 || (tap == 1 && (layer < 0 || layer > NL))) { set_error("wis_debug_sv_taps: bad argument"); return WIS_E_ARG; }
  WIS_RET(sv_upload(s, pcm, n));
  WIS_RET(sv_forward(s, n, tap == 1 ? layer : -1));
  std::vector<f16> tmp;
  int r = 0, c = 0;
  if (tap == 0) { r = s->T; c = C0; }
  else if (tap == 1) { r = s->T; c = D; }
  else { r = s->T_td; c = TD_DIM[NTD - 1]; }
  if ((int64_t)r * c > cap) { set_error("wis_debug_sv_taps: %d x %d floats exceed the output's %lld", r, c, (long long)cap); return WIS_E_ARG; }
  if (tap == 0) {
    tmp.resize((size_t)r * c);
    WIS_HIP_CHECK(hipMemcpyAsync(tmp.data(), s->feat_out, tmp.size() * 2, hipMemcpyDeviceToHost, s->st));
    WIS_HIP_CHECK(hipStreamSynchronize(s->st));
    for (size_t i = 0; i < tmp.size(); ++i) out[i] = (float)tmp[i];
  } else if (tap == 1) {
    WIS_HIP_CHECK(hipMemcpyAsync(out, s->h, (size_t)r * c * 4, hipMemcpyDeviceToHost, s->st));
    WIS_HIP_CHECK(hipStreamSynchronize(s->st));
  } else {     // TDNN output after its ReLU (z holds the pre-activation of the last layer, [T_td][1536])
    std::vector<float> z((size_t)r * TD_LAST_PAD);
    WIS_HIP_CHECK(hipMemcpyAsync(z.data(), s->z, z.size() * 4, hipMemcpyDeviceToHost, s->st));
    WIS_HIP_CHECK(hipStreamSynchronize(s->st));
    for (int i = 0; i < r; ++i) for (int j = 0; j < c; ++j) out[(size_t)i * c + j] = z[(size_t)i * TD_LAST_PAD + j] > 0.f ? z[(size_t)i * TD_LAST_PAD + j] : 0.f;
  }
  *rows = r; *cols = c;
  return WIS_OK;
}

// ---- single-kernel taps (tests): device pointers in, the production launch helper on the device's op stream, synchronised --------
int wis_op_sv_conv0(int device, const float* pcm, int64_t n, const float* w0, const float* gamma, const float* beta, void* y) {
  if (!pcm || !w0 || !gamma || !beta || !y || n < CONV_K[0] || n > (int64_t)16000 * 60) { set_error("wis_op_sv_conv0: bad argument"); return WIS_E_ARG; }
  Tap t(device, "wis_op_sv_conv0"); WIS_RET(t.rc);
  const int T0 = (int)((n - CONV_K[0]) / CONV_S[0] + 1);
  float *part = nullptr, *ss = nullptr;
  WIS_RET(t.get(&part, (size_t)cdiv(T0, CHUNK0) * C0 * 2)); WIS_RET(t.get(&ss, (size_t)2 * C0));
  sv_launch_conv0(t.st, pcm, w0, gamma, beta, part, ss, reinterpret_cast<f16*>(y), T0);
  return t.finish(WIS_OK);
}
int wis_op_sv_posconv(int device, const float* x, const void* W, const float* bias, float* out, int T) {
  if (!x || !W || !bias || !out || T < 1) { set_error("wis_op_sv_posconv: bad argument"); return WIS_E_ARG; }
  Tap t(device, "wis_op_sv_posconv"); WIS_RET(t.rc);
  sv_launch_posconv(t.st, x, reinterpret_cast<const f16*>(W), bias, out, T);
  return t.finish(WIS_OK);
}
int wis_op_sv_attention(int device, const void* qkv, const float* xin, const float* gw, const float* gb, const float* gconst, const float* tab,
                        int L, void* out, int T) {
  if (!qkv || !xin || !gw || !gb || !gconst || !tab || !out || T < 1 || L < T) { set_error("wis_op_sv_attention: bad argument"); return WIS_E_ARG; }
  Tap t(device, "wis_op_sv_attention"); WIS_RET(t.rc);
  sv_launch_attn(t.st, reinterpret_cast<const f16*>(qkv), xin, gw, gb, gconst, tab, L, reinterpret_cast<f16*>(out), T);
  return t.finish(WIS_OK);
}
int wis_op_sv_layernorm(int device, const void* x, int in_f16, const float* gamma, const float* beta, void* y16, float* y32, float* ws, void* ws16,
                        float wl, int wmode, int M, int d) {
  if (!x || !gamma || !beta || !y16 || wmode < 0 || wmode > 2 || (wmode && !ws) || M < 1) { set_error("wis_op_sv_layernorm: bad argument"); return WIS_E_ARG; }
  Tap t(device, "wis_op_sv_layernorm"); WIS_RET(t.rc);
  return t.finish(in_f16 ? sv_ln<true>(t.st, x, gamma, beta, reinterpret_cast<f16*>(y16), y32, ws, reinterpret_cast<f16*>(ws16), wl, wmode, M, d)
                         : sv_ln<false>(t.st, x, gamma, beta, reinterpret_cast<f16*>(y16), y32, ws, reinterpret_cast<f16*>(ws16), wl, wmode, M, d));
}
int wis_op_sv_xvector_tail(int device, const float* z, int ldz, int T, int n, const float* w_fe, const float* b_fe, float* stats, float* emb) {
  if (!z || !w_fe || !b_fe || !stats || !emb || T < 2 || n < 1 || n > ldz) { set_error("wis_op_sv_xvector_tail: bad argument"); return WIS_E_ARG; }
  Tap t(device, "wis_op_sv_xvector_tail"); WIS_RET(t.rc);
  sv_launch_xvector_tail(t.st, z, ldz, T, n, w_fe, b_fe, stats, emb);
  return t.finish(WIS_OK);
}

}  // extern "C"
