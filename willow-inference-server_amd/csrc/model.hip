// model.hip — model lifecycle, weight re-packing, the encoder and decoder passes, the search-state helpers and wis_detect_language:
// the definitions behind model.hpp.  The other drivers are objects of their own on that interface: generate.hip (wis_generate*, the
// sampling tail), taps.hip (debug / measurement taps, wis_op_*), align.hip (wis_align).
//
// Replaces the ctranslate2.models.Whisper object the reference builds at main.py:341-444 and
// drives at main.py:535-537, 638-639, 685-693.  One handle = one replica on one GPU: weights are
// converted ONCE into the layouts the kernels stream (row-major f16 [N][K] for the encoder MFMA
// GEMM, MFMA-fragment-packed for the decoder's skinny GEMMs), all activations / KV caches live in
// HBM for the handle's lifetime, and a decode step (~260 kernels) is captured once into a HIP
// graph and replayed: every step-dependent value (positions, tokens, beam parents, scores)
// lives in device memory, so the host only launches graphs and polls a done counter.
#include <math.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <atomic>
#include <mutex>
#include <memory>
#include <string>
#include <vector>

#include "common.hpp"
#include "kernels.hpp"
#include "model.hpp"

using namespace wis;

namespace wis {

// ---- small utility kernels -------------------------------------------------------------
// generic convert: src (f16|f32) [rows][cols] -> dst (f16|f32) [rows][dst_ld]; rows < n_scale scaled
__global__ void convert_kernel(const void* __restrict__ src, int src_f16, void* __restrict__ dst, int dst_f16,
                               int64_t rows, int64_t cols, int64_t dst_ld, int64_t n_scale, float scale) {
  const int64_t total = rows * cols;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t r = i / cols, c = i - r * cols;
    float v = src_f16 ? (float)reinterpret_cast<const f16*>(src)[i] : reinterpret_cast<const float*>(src)[i];
    if (r < n_scale) v *= scale;
    if (dst_f16) reinterpret_cast<f16*>(dst)[r * dst_ld + c] = (f16)v; else reinterpret_cast<float*>(dst)[r * dst_ld + c] = v;
  }
}
// encoder output handed back in through the host (WIS_IN_ENC_HOST): f32 -> f16, eight values per thread and trip (two 16-byte loads, one
// 16-byte store; n8 = B T d / 8, d a multiple of 64).  Values that were f16 before the host saw them convert back exactly.
__global__ __launch_bounds__(256) void enc_f32_to_f16_kernel(const float4* __restrict__ s, f16x8* __restrict__ d, int64_t n8) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n8; i += (int64_t)gridDim.x * 256) {
    const float4 a = s[2 * i], b = s[2 * i + 1];
    f16x8 o;
    o[0] = (f16)a.x; o[1] = (f16)a.y; o[2] = (f16)a.z; o[3] = (f16)a.w;
    o[4] = (f16)b.x; o[5] = (f16)b.y; o[6] = (f16)b.z; o[7] = (f16)b.w;
    d[i] = o;
  }
}
// conv weight [out][in][3] -> f16 [out][row_len], element (o, k*cpad + c) = W[o][c][k]; channel padding and the row tail
// [3*cpad, row_len) are zero (row_len = K rounded up to the GEMM's 64-deep k-tile)
__global__ void conv_pack_kernel(const void* __restrict__ src, int src_f16, f16* __restrict__ dst, int out, int in, int cpad, int row_len) {
  const int64_t total = (int64_t)out * row_len;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int o = (int)(i / row_len), rem = (int)(i - (int64_t)o * row_len), k = rem / cpad, c = rem - k * cpad;
    float v = 0.f;
    if (k < 3 && c < in) {
      const int64_t s = ((int64_t)o * in + c) * 3 + k;
      v = src_f16 ? (float)reinterpret_cast<const f16*>(src)[s] : reinterpret_cast<const float*>(src)[s];
    }
    dst[i] = (f16)v;
  }
}
// mel f32 [B][NM][3000] -> conv1 input image f16 [B][3002][CC]: NM = 80 bins padded to CC = 96 channels, or 128 bins (CC = 128)
template <int NM, int CC>
__global__ void mel_to_image_kernel(const float* __restrict__ mel, f16* __restrict__ img) {
  __shared__ float s_t[NM][65];
  const int tid = threadIdx.x, w = blockIdx.y, f0 = blockIdx.x * 64;
  for (int o = tid; o < NM * 64; o += 256) {
    const int m = o >> 6, f = o & 63;
    if (f0 + f < 3000) s_t[m][f] = mel[((size_t)w * NM + m) * 3000 + f0 + f];
  }
  __syncthreads();
  for (int o = tid; o < 64 * CC; o += 256) {
    const int f = o / CC, c = o - f * CC;
    if (f0 + f < 3000) img[((size_t)w * 3002 + f0 + f + 1) * CC + c] = (c < NM) ? (f16)s_t[c][f] : (f16)0.f;
  }
}
// conv1 over the [3002][C] image (C = conv1_channels(n_mels)) as one implicit-im2col GEMM: K = 3C, rounded up to whole 64-deep
// k-tiles (80 bins: 288 -> 320, the 32 extra columns carry zero weights and read into the next row; 128 bins: 384, no pad)
int conv1_k(int n_mels) { return cdiv(3 * conv1_channels(n_mels), 64) * 64; }
// The convs' GEMM descriptions (run_encoder, and the op taps on shorter images): B utterances of T output rows each; output row t of an
// utterance starts at row t (conv1, stride 1) / 2 t (conv2, stride 2) of its padded time-major image and runs over three image rows
GemmP conv1_gemm(const f16* img, const f16* w, int B, int T, int n_mels, int N) {      // image [B][T + 2][conv1_channels]
  const int cc = conv1_channels(n_mels);
  GemmP p; p.klen = 0; p.A = img; p.a_bs = (int64_t)(T + 2) * cc; p.a_rs = cc; p.a_rpb = T; p.W = w; p.M = B * T; p.N = N; p.K = conv1_k(n_mels);
  return p;
}
GemmP conv2_gemm(const f16* c1, const f16* w, int B, int T, int cin, int N) {      // image [B][2 T + 2][cin]
  GemmP p; p.klen = 0; p.A = c1; p.a_bs = (int64_t)(2 * T + 2) * cin; p.a_rs = 2 * cin; p.a_rpb = T; p.W = w; p.M = B * T; p.N = N; p.K = 3 * cin;
  return p;
}
// dst[c][r] = src[r][c] as f16 (src f16 or f32, [rows][cols])
__global__ void transpose_to_f16_kernel(const void* __restrict__ src, int src_f16, f16* __restrict__ dst, int rows, int cols) {
  __shared__ float t[32][33];
  const int c0 = blockIdx.x * 32, r0 = blockIdx.y * 32, tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  for (int i = ty; i < 32; i += 8) {
    const int r = r0 + i, c = c0 + tx;
    if (r < rows && c < cols) t[i][tx] = src_f16 ? (float)reinterpret_cast<const f16*>(src)[(size_t)r * cols + c] : reinterpret_cast<const float*>(src)[(size_t)r * cols + c];
  }
  __syncthreads();
  for (int i = ty; i < 32; i += 8) {
    const int c = c0 + i, r = r0 + tx;
    if (r < rows && c < cols) dst[(size_t)c * rows + r] = (f16)t[tx][i];
  }
}
// y[n] = sum_k W[n][k] x[k]  (W f16 rows of pitch ld, x fp32); one wave per row
__global__ void matvec_rows_kernel(const f16* __restrict__ W, int ld, const float* __restrict__ x, float* __restrict__ y, int N, int K) {
  const int n = blockIdx.x, lane = threadIdx.x;
  if (n >= N) return;
  float a = 0.f;
  for (int k = lane; k < K; k += 64) a += (float)W[(size_t)n * ld + k] * x[k];
  a = wave_sum(a);
  if (lane == 0) y[n] = a;
}
__global__ void f16_to_f32_kernel(const f16* __restrict__ s, float* __restrict__ d, int64_t n) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) d[i] = (float)s[i];
}

// K-splits of the encoder's FFN2 at M rows (0 = one workgroup per output tile over the whole K): split while the 128x128 tiles
// are too few for 256 CUs; four ways while that still leaves <= 512 workgroups, else two (the split length stays a multiple of
// the 64-deep k-tile for every Whisper width)
int enc_splitk(int d, int M) {
  const int tiles = (d / 128) * cdiv(M, 128);
  if (tiles >= 200) return 0;
  return (tiles <= 128 && (4 * d) % (4 * 64) == 0) ? 4 : 2;
}
// Bump allocator over large slabs: the ~700 tensors and buffers of a replica come from a handful of hipMalloc calls, so the
// small per-layer parameters (biases, LayerNorm vectors: 2.5-10 KB) sit next to their matrices inside the same large-page
// fragments instead of each owning a 4 KB page - every decode kernel touches 3-5 of them on its critical path, and a
// translation miss there costs more than the kernel's whole weight stream.
constexpr size_t SLAB_BYTES = (size_t)1 << 30;
template <class T>
static int dalloc(wis_model* m, T** p, size_t n_elems) {
  size_t b = n_elems * sizeof(T); if (b == 0) b = 16;
  const size_t align = b >= ((size_t)1 << 20) ? ((size_t)1 << 16) : 256;
  size_t pad = (align - (reinterpret_cast<uintptr_t>(m->slab_cur) & (align - 1))) & (align - 1);
  if (!m->slab_cur || pad + b > m->slab_left) {
    const size_t sb = b > SLAB_BYTES ? ((b + ((size_t)2 << 20) - 1) & ~(((size_t)2 << 20) - 1)) : SLAB_BYTES;
    void* q = nullptr;
    hipError_t e = hipMalloc(&q, sb);
    if (e != hipSuccess) { set_error("hipMalloc(%zu bytes) failed: %s", sb, hipGetErrorString(e)); return WIS_E_NOMEM; }
    m->allocs.push_back(q); m->slab_cur = static_cast<char*>(q); m->slab_left = sb; pad = 0;
  }
  m->slab_cur += pad; m->slab_left -= pad;
  *p = reinterpret_cast<T*>(m->slab_cur);
  m->slab_cur += b; m->slab_left -= b; m->bytes += b + pad;
  return WIS_OK;
}
// the two utility kernels as the other objects launch them (model.hpp)
void launch_convert(hipStream_t st, const void* src, int src_f16, void* dst, int dst_f16, int64_t rows, int64_t cols, int64_t dst_ld, int64_t n_scale, float scale) {
  hipLaunchKernelGGL(convert_kernel, dim3(blocks_for(rows * cols)), dim3(256), 0, st, src, src_f16, dst, dst_f16, rows, cols, dst_ld, n_scale, scale);
}
void launch_f16_to_f32(hipStream_t st, const f16* s, float* d, int64_t n) {
  hipLaunchKernelGGL(f16_to_f32_kernel, dim3(blocks_for(n)), dim3(256), 0, st, s, d, n);
}
// the convs' weights [N][cin][3] (f32 or f16) -> the GEMMs' W operand (conv_pack_kernel)
void pack_conv1_w(hipStream_t st, const void* src, int src_f16, f16* dst, int N, int n_mels) {
  const int k1 = conv1_k(n_mels);      // 80 bins: K = 3*96 = 288 padded to 320 = 5 x 64; 128: 384
  hipLaunchKernelGGL(conv_pack_kernel, dim3(blocks_for((int64_t)N * k1)), dim3(256), 0, st, src, src_f16, dst, N, n_mels, conv1_channels(n_mels), k1);
}
void pack_conv2_w(hipStream_t st, const void* src, int src_f16, f16* dst, int N, int cin) {
  hipLaunchKernelGGL(conv_pack_kernel, dim3(blocks_for((int64_t)N * 3 * cin)), dim3(256), 0, st, src, src_f16, dst, N, cin, cin, 3 * cin);
}
int launch_mel_to_image(hipStream_t st, const float* mel, f16* img, int B, int n_mels) {
  if (n_mels == 128) hipLaunchKernelGGL((mel_to_image_kernel<128, 128>), dim3(cdiv(3000, 64), B), dim3(256), 0, st, mel, img);
  else if (n_mels == 80) hipLaunchKernelGGL((mel_to_image_kernel<80, 96>), dim3(cdiv(3000, 64), B), dim3(256), 0, st, mel, img);
  else { set_error("mel_to_image: %d mel bins (80 or 128)", n_mels); return WIS_E_UNSUPPORTED; }
  return WIS_OK;
}

namespace {
struct TensorSrc { const void* p; int f16; int64_t rows, cols; };

struct Loader {
  const wis_tensor_t* t; int n; const char* arena;   // arena: DEVICE base pointer
  size_t arena_bytes;
  const wis_tensor_t* find(const std::string& name) const {
    for (int i = 0; i < n; ++i) if (name == t[i].name) return &t[i];
    return nullptr;
  }
  int get(const std::string& name, int64_t rows, int64_t cols, TensorSrc* out) const {
    const wis_tensor_t* x = find(name);
    if (!x) { set_error("weight '%s' missing from the index", name.c_str()); return WIS_E_FORMAT; }
    int64_t ne = 1; for (int i = 0; i < x->rank; ++i) ne *= x->shape[i];
    if (ne != rows * cols) { set_error("weight '%s': %lld elements, expected %lld", name.c_str(), (long long)ne, (long long)(rows * cols)); return WIS_E_FORMAT; }
    const size_t es = x->dtype == WIS_DT_F16 ? 2 : 4;
    if (x->dtype != WIS_DT_F16 && x->dtype != WIS_DT_F32) { set_error("weight '%s': dtype %d unsupported", name.c_str(), x->dtype); return WIS_E_FORMAT; }
    if (x->offset + (size_t)ne * es > arena_bytes) { set_error("weight '%s' exceeds the arena", name.c_str()); return WIS_E_FORMAT; }
    out->p = arena + x->offset; out->f16 = x->dtype == WIS_DT_F16; out->rows = rows; out->cols = cols;
    return WIS_OK;
  }
};
}  // namespace

static int to_f32(wis_model* m, const Loader& L, const std::string& name, int64_t n, float** out, int64_t n_scale = 0, float scale = 1.f) {
  TensorSrc s; WIS_RET(L.get(name, n, 1, &s));
  if (!*out) WIS_RET(dalloc(m, out, (size_t)n));          // *out preset: a view into a block the caller allocated
  hipLaunchKernelGGL(convert_kernel, dim3(blocks_for(n)), dim3(256), 0, m->st, s.p, s.f16, *out, 0, n, (int64_t)1, (int64_t)1, n_scale, scale);
  return WIS_OK;
}
static int to_f16_mat(wis_model* m, const Loader& L, const std::string& name, int64_t rows, int64_t cols, f16** out, int64_t n_scale = 0, float scale = 1.f) {
  TensorSrc s; WIS_RET(L.get(name, rows, cols, &s));
  if (!*out) WIS_RET(dalloc(m, out, (size_t)rows * cols));
  hipLaunchKernelGGL(convert_kernel, dim3(blocks_for(rows * cols)), dim3(256), 0, m->st, s.p, s.f16, *out, 1, rows, cols, cols, n_scale, scale);
  return WIS_OK;
}
// W (f16 [N][K] row-major staging) -> what the skinny GEMMs stream, on the caller's buffers (loader and op taps).  gamma given: fold that LayerNorm
// (fold_ln_kernel rewrites W; `bias`, loaded, receives W . beta; `csum`, zeroed, the column sums).  out: the f16 fragment image - or, with scale_out, the
// 8-bit image + row scales, the column sums retaken from what the MFMA will see; null: fold only.  Rows [0, n_scale) (the query part) are scaled by `scale`.
int prep_projection(hipStream_t st, f16* W, int N, int Npad, int K, int n_scale, float scale, const float* gamma, const float* beta, float* bias, float* csum,
                    void* out, float* scale_out, int rows) {
  if (gamma) {
    if (!bias || !csum) { set_error("prep_projection: LayerNorm folding needs a bias vector and a column-sum output"); return WIS_E_ARG; }
    WIS_RET(launch_fold_ln(st, W, gamma, beta, bias, csum, N, K, n_scale, scale));
  }
  if (!out) return WIS_OK;
  if (!scale_out) return launch_pack_gemv(st, W, static_cast<f16*>(out), N, Npad, K, n_scale, scale, rows);
  WIS_RET(launch_pack_gemv8(st, W, static_cast<unsigned char*>(out), scale_out, N, Npad, K, n_scale, scale));
  if (gamma) WIS_RET(launch_csum8(st, W, scale_out, csum, N, K, n_scale, scale));
  return WIS_OK;
}
// checkpoint matrix -> packed projection through the f16 image `tmp` (build_cq_fold reads the folded weights there); allocations in slab order: column
// sums, then the 8-bit image and its scales or the f16 image.  out->N is the logical N; *npad_out the packed image's rows
static int to_packed(wis_model* m, const Loader& L, const std::string& name, int N, int K, f16* tmp, int n_scale, float scale, const float* ln_gamma, const float* ln_beta,
              float* bias, DecProj* out, int* npad_out = nullptr) {
  TensorSrc s; WIS_RET(L.get(name, N, K, &s));
  const int rows = gemv_rows_for(N, K);
  const int Npad = cdiv(N, rows) * rows;
  hipLaunchKernelGGL(convert_kernel, dim3(blocks_for((int64_t)N * K)), dim3(256), 0, m->st, s.p, s.f16, tmp, 1, (int64_t)N, (int64_t)K, (int64_t)K, (int64_t)0, 1.f);
  float *csum = nullptr, *wscale = nullptr; f16* wp = nullptr;
  if (ln_gamma) { WIS_RET(dalloc(m, &csum, (size_t)Npad)); WIS_HIP_CHECK(hipMemsetAsync(csum, 0, (size_t)Npad * 4, m->st)); }
  if (m->w8) { unsigned char* q8 = nullptr; WIS_RET(dalloc(m, &q8, (size_t)Npad * K)); WIS_RET(dalloc(m, &wscale, (size_t)Npad)); wp = reinterpret_cast<f16*>(q8); }
  else WIS_RET(dalloc(m, &wp, (size_t)Npad * K));
  WIS_RET(prep_projection(m->st, tmp, N, Npad, K, n_scale, scale, ln_gamma, ln_beta, bias, csum, wp, wscale, rows));
  *out = DecProj{wp, wscale, bias, csum, N, K, rows};
  if (npad_out) *npad_out = Npad;
  return WIS_OK;
}
// `name`/weight + `name`/bias of the checkpoint as a DecProj.  A LayerNorm-folded projection converts its bias first (the fold adds W . beta to it), the
// others the matrix first: that is the order of the allocations, i.e. the slab layout (SLAB_BYTES) - keep it.
static int load_proj(wis_model* m, const Loader& L, const std::string& name, int N, int K, f16* tmp, int n_scale, float scale, const float* ln_gamma, const float* ln_beta, DecProj* out) {
  float* bias = nullptr;
  if (ln_gamma) WIS_RET(to_f32(m, L, name + "/bias", N, &bias, n_scale, scale));
  WIS_RET(to_packed(m, L, name + "/weight", N, K, tmp, n_scale, scale, ln_gamma, ln_beta, bias, out));
  if (!ln_gamma) { WIS_RET(to_f32(m, L, name + "/bias", N, &bias, n_scale, scale)); out->bias = bias; }
  return WIS_OK;
}

// A second, eight-column image of a projection whose f16 row-major matrix is still in `tmp` (right behind its load_proj): the step of <= 8 rows runs it on
// N / 8 workgroups (dec_kernels.hip gemv_body NC = 8).  The batched route keeps reading the sixteen-column image, so both exist: N * K * 2 bytes more.
// Nothing is added where the kernel form does not apply (8-bit weights, other widths than large's).
static int add_nc8_image(wis_model* m, const f16* tmp, DecProj* p) {
  if (m->w8 || !gemv_nc8_shape(1, p->N, p->K)) return WIS_OK;
  f16* wp8 = nullptr;
  WIS_RET(dalloc(m, &wp8, (size_t)p->N * p->K));
  WIS_RET(launch_pack_gemv_nc8(m->st, tmp, wp8, p->N, p->N, p->K));
  p->Wp8 = wp8;
  return WIS_OK;
}
// ... or a five-column image (dec_kernels.hip gemv_nc5_kernel: FFN2 on N / 5 workgroups, one per CU at large's width), where the pass of <= 8 rows would run it
// on this device: gemv_nc5_elems * 2 bytes (the matrix's bytes plus about 12 %: a zero row in sixteen and a ragged last request per wave).  *added: it exists.
static int add_nc5_image(wis_model* m, const f16* tmp, DecProj* p, bool* added) {
  *added = false;
  if (m->w8 || !gemv_nc5_shape(1, p->N, p->K, GV_RESID)) return WIS_OK;
  f16* wp5 = nullptr;
  WIS_RET(dalloc(m, &wp5, gemv_nc5_elems(p->N, p->K, 40)));
  WIS_RET(launch_pack_gemv_nc5(m->st, tmp, wp5, p->N, p->K, 40));
  p->Wp5 = wp5; *added = true;
  return WIS_OK;
}

// The cross-Q fold's matrix and bias (load_weights below; the wis_op_gemv_out_cq tap builds its operands with the same code): wq_gamma = f16(Wq o gamma)
// [d][d] as fold_ln_kernel left it, wo / bo = the self-attention output projection (f16 or f32 [d][d]; fp32 [d]) ->
//   p_cqo = packed [W'q | W'q Wo] ([d][2d], W'q = wq_gamma * qs, the product rounded to f16 like every other stored weight),  b_cqo = W'q bo.
// fcat [d][2d], fwot [d][d], fwqo [d][d]: f16 staging of the caller.
int build_cq_fold(hipStream_t st, const f16* wq_gamma, const void* wo, int wo_f16, const float* bo, int d, float qs, f16* fcat, f16* fwot, f16* fwqo, f16* p_cqo, float* b_cqo) {
  hipLaunchKernelGGL(convert_kernel, dim3(blocks_for((int64_t)d * d)), dim3(256), 0, st, wq_gamma, 1, fcat, 1, (int64_t)d, (int64_t)d, (int64_t)2 * d, (int64_t)d, qs);   // left half: W'q
  hipLaunchKernelGGL(transpose_to_f16_kernel, dim3(cdiv(d, 32), cdiv(d, 32)), dim3(256), 0, st, wo, wo_f16, fwot, d, d);
  GemmP gp = gemm_plain(fcat, 2 * d, fwot, d, d, d);
  WIS_RET(launch_gemm_generic(st, gp, nullptr, nullptr, fwqo, 0));                                     // W'q . Wo  (f16 inputs, fp32 accumulate)
  hipLaunchKernelGGL(convert_kernel, dim3(blocks_for((int64_t)d * d)), dim3(256), 0, st, fwqo, 1, fcat + d, 1, (int64_t)d, (int64_t)d, (int64_t)2 * d, (int64_t)0, 1.f);   // right half
  WIS_RET(launch_pack_gemv(st, fcat, p_cqo, d, d, 2 * d, 0, 1.f, 16));
  hipLaunchKernelGGL(matvec_rows_kernel, dim3(d), dim3(64), 0, st, fcat, 2 * d, bo, b_cqo, d, d);
  return WIS_OK;
}

static int load_weights(wis_model* m, const Loader& L) {
  const wis_config_t& c = m->cfg;
  const int d = c.d_model, V = c.n_vocab;
  const float qs = 0.125f;   // 1/sqrt(64), folded into the query projections (exact: power of two)
  f16* tmp = nullptr;        // staging for packed conversions: largest matrix = embeddings [V][d]
  f16 *fcat = nullptr, *fwot = nullptr, *fwqo = nullptr;      // cross-Q fold staging: [W'q | W'q Wo] [d][2d], Wo^T, W'q Wo
  {
    size_t big = (size_t)V * d; if ((size_t)4 * d * d > big) big = (size_t)4 * d * d;
    WIS_HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&tmp), big * 2));
    if (m->cq_fold) {
      WIS_HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&fcat), (size_t)2 * d * d * 2));
      WIS_HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&fwot), (size_t)d * d * 2));
      WIS_HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&fwqo), (size_t)d * d * 2));
    }
  }
  int rc = WIS_OK;
  do {
    // ---- encoder
    {
      TensorSrc s;
      if ((rc = L.get("encoder/conv1/weight", d, (int64_t)c.n_mels * 3, &s))) break;
      if ((rc = dalloc(m, &m->w_conv1, (size_t)d * conv1_k(c.n_mels)))) break;
      pack_conv1_w(m->st, s.p, s.f16, m->w_conv1, d, c.n_mels);
      if ((rc = L.get("encoder/conv2/weight", d, (int64_t)d * 3, &s))) break;
      if ((rc = dalloc(m, &m->w_conv2, (size_t)d * 3 * d))) break;
      pack_conv2_w(m->st, s.p, s.f16, m->w_conv2, d, d);
    }
    if ((rc = to_f32(m, L, "encoder/conv1/bias", d, &m->b_conv1))) break;
    if ((rc = to_f32(m, L, "encoder/conv2/bias", d, &m->b_conv2))) break;
    if (L.find("encoder/position_encodings/encodings")) {
      if ((rc = to_f32(m, L, "encoder/position_encodings/encodings", (int64_t)c.n_audio_ctx * d, &m->enc_pos))) break;
    } else {
      // Whisper sinusoids: inc = ln(10000)/(d/2-1); pos[t] = [sin(t inv) | cos(t inv)]
      std::vector<float> pe((size_t)c.n_audio_ctx * d);
      const int half = d / 2; const double inc = log(10000.0) / (half - 1);
      for (int t = 0; t < c.n_audio_ctx; ++t)
        for (int i = 0; i < half; ++i) {
          const float inv = (float)exp(-inc * i);           // fp32 table like torch.exp(float32)
          const float a = (float)t * inv;
          pe[(size_t)t * d + i] = sinf(a); pe[(size_t)t * d + half + i] = cosf(a);
        }
      if ((rc = dalloc(m, &m->enc_pos, pe.size()))) break;
      WIS_HIP_CHECK(hipMemcpyAsync(m->enc_pos, pe.data(), pe.size() * 4, hipMemcpyHostToDevice, m->st));
      WIS_HIP_CHECK(hipStreamSynchronize(m->st));
    }
    if ((rc = to_f32(m, L, "encoder/layer_norm/gamma", d, &m->enc_ln_g))) break;
    if ((rc = to_f32(m, L, "encoder/layer_norm/beta", d, &m->enc_ln_b))) break;
    m->enc.resize(c.n_enc_layers);
    for (int l = 0; l < c.n_enc_layers && !rc; ++l) {
      const std::string p = "encoder/layer_" + std::to_string(l) + "/";
      EncLayerW& w = m->enc[l];
      if ((rc = to_f32(m, L, p + "self_attention/layer_norm/gamma", d, &w.ln1_g))) break;
      if ((rc = to_f32(m, L, p + "self_attention/layer_norm/beta", d, &w.ln1_b))) break;
      // (the lazy-reference attention loop takes exp2 of the MFMA result directly: log2(e) rides on the query projection too)
      const float qs_enc = enc_attn_lazy() ? qs * 1.4426950408889634f : qs;
      if ((rc = to_f16_mat(m, L, p + "self_attention/linear_0/weight", 3 * d, d, &w.w_qkv, d, qs_enc))) break;
      if ((rc = to_f32(m, L, p + "self_attention/linear_0/bias", 3 * d, &w.b_qkv, d, qs_enc))) break;
      if ((rc = to_f16_mat(m, L, p + "self_attention/linear_1/weight", d, d, &w.w_out))) break;
      if ((rc = to_f32(m, L, p + "self_attention/linear_1/bias", d, &w.b_out))) break;
      if ((rc = to_f32(m, L, p + "ffn/layer_norm/gamma", d, &w.ln2_g))) break;
      if ((rc = to_f32(m, L, p + "ffn/layer_norm/beta", d, &w.ln2_b))) break;
      if ((rc = to_f16_mat(m, L, p + "ffn/linear_0/weight", 4 * d, d, &w.w_f1))) break;
      if ((rc = to_f32(m, L, p + "ffn/linear_0/bias", 4 * d, &w.b_f1))) break;
      if ((rc = to_f16_mat(m, L, p + "ffn/linear_1/weight", d, 4 * d, &w.w_f2))) break;
      if ((rc = to_f32(m, L, p + "ffn/linear_1/bias", d, &w.b_f2))) break;
    }
    if (rc) break;
    // ---- decoder
    if ((rc = to_f16_mat(m, L, "decoder/embeddings/weight", V, d, &m->emb))) break;
    if ((rc = to_f16_mat(m, L, "decoder/position_encodings/encodings", c.n_text_ctx, d, &m->dec_pos))) break;
    if ((rc = to_f32(m, L, "decoder/layer_norm/gamma", d, &m->dec_ln_g))) break;
    if ((rc = to_f32(m, L, "decoder/layer_norm/beta", d, &m->dec_ln_b))) break;
    // every projection that follows a LayerNorm is stored LayerNorm-folded (W o gamma, bias + W . beta, column sums): the final
    // LayerNorm into the tied vocabulary projection (which has no bias of its own) ...
    float* b_proj = nullptr;
    if ((rc = dalloc(m, &b_proj, (size_t)V + 64))) break;
    if (hipMemsetAsync(b_proj, 0, ((size_t)V + 64) * 4, m->st) != hipSuccess) { set_error("memset failed"); rc = WIS_E_HIP; break; }
    if ((rc = to_packed(m, L, "decoder/embeddings/weight", V, d, tmp, 0, 1.f, m->dec_ln_g, m->dec_ln_b, b_proj, &m->proj, &m->n_vocab_pad))) break;
    m->proj.N = m->n_vocab_pad;      // launched over the padded vocabulary
    m->dec.resize(c.n_dec_layers);
    if ((rc = dalloc(m, &m->w_ckv_all, (size_t)c.n_dec_layers * 2 * d * d))) break;      // one [L * 2d][d] matrix: a single GEMM projects every layer
    if ((rc = dalloc(m, &m->b_ckv_all, (size_t)c.n_dec_layers * 2 * d))) break;
    for (int l = 0; l < c.n_dec_layers && !rc; ++l) {
      const std::string p = "decoder/layer_" + std::to_string(l) + "/";
      DecLayerW& w = m->dec[l];
      if ((rc = to_f32(m, L, p + "self_attention/layer_norm/gamma", d, &w.ln1_g))) break;
      if ((rc = to_f32(m, L, p + "self_attention/layer_norm/beta", d, &w.ln1_b))) break;
      // ... and ln1 -> QKV, ln2 -> cross-Q, ln3 -> FFN1 of every layer
      if ((rc = load_proj(m, L, p + "self_attention/linear_0", 3 * d, d, tmp, d, qs, w.ln1_g, w.ln1_b, &w.qkv))) break;
      if ((rc = load_proj(m, L, p + "self_attention/linear_1", d, d, tmp, 0, 1.f, nullptr, nullptr, &w.out))) break;
      if ((rc = to_f32(m, L, p + "attention/layer_norm/gamma", d, &w.ln2_g))) break;
      if ((rc = to_f32(m, L, p + "attention/layer_norm/beta", d, &w.ln2_b))) break;
      if ((rc = load_proj(m, L, p + "attention/linear_0", d, d, tmp, d, qs, w.ln2_g, w.ln2_b, &w.cq))) break;
      if (m->cq_fold) {
        // Cross-attention query folded through the self-attention output projection (one dependent stage less per layer):
        //   x1 = x0 + Wo a + bo,   q = rs(x1) (W'q x1 - mu(x1) c) + b'      (LayerNorm-folded form, W'q = (Wq o gamma) / 8)
        //   W'q x1 = W'q x0 + (W'q Wo) a + W'q bo  =: q_raw  - computable from the LAYER INPUT x0 and the attention output a, i.e.
        // in the same launch as the out-projection; mu / rs of x1 are applied by the cross-attention kernel (dec_kernels.hip).
        // tmp holds f16(Wq o gamma) (load_proj above); W'q Wo is rounded to f16 like every other stored weight.
        TensorSrc so; if ((rc = L.get(p + "self_attention/linear_1/weight", d, d, &so))) break;
        f16* p_cqo = nullptr; float* b_cqo = nullptr;
        if ((rc = dalloc(m, &p_cqo, (size_t)d * 2 * d))) break;
        if ((rc = dalloc(m, &b_cqo, (size_t)d))) break;
        if ((rc = build_cq_fold(m->st, tmp, so.p, so.f16, w.out.bias, d, qs, fcat, fwot, fwqo, p_cqo, b_cqo))) break;
        w.cqo = DecProj{p_cqo, nullptr, b_cqo, nullptr, d, 2 * d, 16};
        // ... and its eight-column image for the pass of <= 8 rows (fcat still holds the row-major [d][2d]); the batched route keeps reading the other
        if (!m->w8 && out_cq_nc8_shape(1, d)) {
          f16* p8 = nullptr;
          if ((rc = dalloc(m, &p8, (size_t)d * 2 * d))) break;
          if ((rc = launch_pack_gemv_nc8(m->st, fcat, p8, d, d, 2 * d))) break;
          w.cqo.Wp8 = p8;
        }
      }
      w.w_ckv = m->w_ckv_all + (size_t)l * 2 * d * d; w.b_ckv = m->b_ckv_all + (size_t)l * 2 * d;
      if ((rc = to_f16_mat(m, L, p + "attention/linear_1/weight", 2 * d, d, &w.w_ckv))) break;
      if ((rc = to_f32(m, L, p + "attention/linear_1/bias", 2 * d, &w.b_ckv))) break;
      if ((rc = load_proj(m, L, p + "attention/linear_2", d, d, tmp, 0, 1.f, nullptr, nullptr, &w.cout))) break;
      if ((rc = add_nc8_image(m, tmp, &w.cout))) break;
      if ((rc = to_f32(m, L, p + "ffn/layer_norm/gamma", d, &w.ln3_g))) break;
      if ((rc = to_f32(m, L, p + "ffn/layer_norm/beta", d, &w.ln3_b))) break;
      bool nc5 = false;
      if ((rc = load_proj(m, L, p + "ffn/linear_0", 4 * d, d, tmp, 0, 1.f, w.ln3_g, w.ln3_b, &w.f1))) break;
      if ((rc = load_proj(m, L, p + "ffn/linear_1", d, 4 * d, tmp, 0, 1.f, nullptr, nullptr, &w.f2))) break;
      if ((rc = add_nc5_image(m, tmp, &w.f2, &nc5))) break;
      // (the five-column image serves every pass FFN2's eight-column image would: at K = 4d both end at the rows the register staging holds)
      if (!nc5 && (rc = add_nc8_image(m, tmp, &w.f2))) break;
    }
  } while (0);
  hipError_t e = hipStreamSynchronize(m->st);
  hipFree(tmp); hipFree(fcat); hipFree(fwot); hipFree(fwqo);
  if (rc) return rc;
  if (e != hipSuccess) { set_error("weight conversion failed: %s", hipGetErrorString(e)); return WIS_E_HIP; }
  return WIS_OK;
}

// K slices of the batched FFN2 (GemvP::ksplit).  Measured (decode ms per utterance batch, 17 steps): 8 utterances 40.7 unsplit / 38.6 two slices / 38.9 four;
// 12: 46.7 two / 46.9 four; 16: 60.9 unsplit / 58.7 two / 59.5 four.  WIS_FRAG_KSPLIT=1: no split (A/B switch).  ffn2_ksplit: the slices a K-deep FFN2 takes -
// the setting where the k-steps divide into slices of whole wave quarters, else 1 (launch_gemv_frag still prefers its M split from two row blocks on)
static int frag_ksplit_setting() {
  static const int env_ks = getenv("WIS_FRAG_KSPLIT") ? atoi(getenv("WIS_FRAG_KSPLIT")) : 2;
  return env_ks >= 1 && env_ks <= 8 ? env_ks : 2;
}
int ffn2_ksplit(int K) {
  const int ks = frag_ksplit_setting();
  return ks > 1 && (K / 32) % (4 * ks) == 0 ? ks : 1;
}
// part: [N/16][ks][xmb][64] float4 slice sums; cnt: [N/16] tickets, zeroed once
void frag_set_ksplit(GemvP& g, int ks, float* part, unsigned* cnt) {
  if (ks > 1) { g.ksplit = ks; g.kpart = part; g.kcnt = cnt; }
}

static int alloc_buffers(wis_model* m) {
  const wis_config_t& c = m->cfg;
  const int d = c.d_model, H = c.n_heads, Bm = c.max_batch, T = c.n_audio_ctx, L = c.n_dec_layers;
  const int slots = Bm * c.max_beam, ctx = c.n_text_ctx;
  m->Tpad = cdiv(T, 64) * 64;
  const size_t img_elems = (size_t)Bm * 3002 * conv1_channels(c.n_mels) + 64;     // +64: the last window's zero-weighted over-read (80 bins)
  WIS_RET(dalloc(m, &m->img, img_elems));
  WIS_RET(dalloc(m, &m->c1, (size_t)Bm * 3002 * d));
  WIS_RET(dalloc(m, &m->x, (size_t)Bm * T * d));
  WIS_RET(dalloc(m, &m->xn, (size_t)Bm * T * d));
  WIS_RET(dalloc(m, &m->qk, (size_t)Bm * T * 2 * d));
  WIS_RET(dalloc(m, &m->vt, (size_t)Bm * H * 64 * m->Tpad));
  WIS_RET(dalloc(m, &m->ao, (size_t)Bm * T * d));
  WIS_RET(dalloc(m, &m->hbuf, (size_t)Bm * T * 4 * d));
  WIS_RET(dalloc(m, &m->mem, (size_t)Bm * T * d));
  {  // split-key encoder attention (small batches): per-workgroup softmax states and the pair tickets
    int bs = 600 / (H * cdiv(T, 128)); if (bs > Bm) bs = Bm;
    if (bs >= 1) {
      WIS_RET(dalloc(m, &m->enc_part, enc_attention_part_floats(bs, T, H)));
      WIS_RET(dalloc(m, &m->enc_cnt, (size_t)bs * H * cdiv(T, 128)));
      WIS_HIP_CHECK(hipMemsetAsync(m->enc_cnt, 0, (size_t)bs * H * cdiv(T, 128) * 4, m->st));
      m->enc_part_cap = (size_t)bs * H * cdiv(T, 128);
    }
  }
  {  // fp32 partial tiles of the K-split FFN2 (small row counts only)
    size_t sk = 0;
    for (int b = 1; b <= Bm; ++b) { const size_t need = (size_t)enc_splitk(d, b * T) * b * T * d; if (need > sk) sk = need; }      // not monotonic in b: 4 splits, then 2, then none
    m->skbuf = nullptr;
    if (sk) WIS_RET(dalloc(m, &m->skbuf, sk));
  }
  WIS_HIP_CHECK(hipMemsetAsync(m->img, 0, img_elems * 2, m->st));
  WIS_HIP_CHECK(hipMemsetAsync(m->c1, 0, (size_t)Bm * 3002 * d * 2, m->st));
  WIS_HIP_CHECK(hipMemsetAsync(m->vt, 0, (size_t)Bm * H * 64 * m->Tpad * 2, m->st));
  m->kx.resize(L); m->vx.resize(L); m->kc.resize(L); m->vc.resize(L);
  m->kv_layer_stride = (size_t)slots * ctx * d;
  WIS_RET(dalloc(m, &m->kc_all, m->kv_layer_stride * L));
  WIS_RET(dalloc(m, &m->vc_all, m->kv_layer_stride * L));
  m->kx_lstride = (size_t)Bm * H * 8 * T * 8; m->vx_lstride = (size_t)Bm * H * 64 * m->Tpad;
  WIS_RET(dalloc(m, &m->kx_all, m->kx_lstride * L));
  WIS_RET(dalloc(m, &m->vx_all, m->vx_lstride * L));
  WIS_HIP_CHECK(hipMemsetAsync(m->vx_all, 0, m->vx_lstride * L * 2, m->st));
  for (int l = 0; l < L; ++l) {
    m->kx[l] = m->kx_all + (size_t)l * m->kx_lstride;
    m->vx[l] = m->vx_all + (size_t)l * m->vx_lstride;
    m->kc[l] = m->kc_all + (size_t)l * slots * ctx * d;     // one block per cache: kv_reorder_kernel walks the layers by stride
    m->vc[l] = m->vc_all + (size_t)l * slots * ctx * d;
  }
  WIS_RET(dalloc(m, &m->dx, (size_t)MAX_ROWS * d));
  WIS_RET(dalloc(m, &m->dq, (size_t)MAX_ROWS * d));
  WIS_RET(dalloc(m, &m->dq2, (size_t)MAX_ROWS * d));
  WIS_RET(dalloc(m, &m->dao, (size_t)MAX_ROWS * d));
  WIS_RET(dalloc(m, &m->dh, (size_t)MAX_ROWS * 4 * d));
  WIS_RET(dalloc(m, &m->dln, (size_t)MAX_ROWS * d));
  WIS_RET(dalloc(m, &m->dxh, (size_t)MAX_ROWS * d));
  {  // fragment images (kernels.hpp xf_index): [K/32][3 row blocks][64][8] f16; zeroed once (rows >= M are never written)
    const size_t img = xf_elems(d, MAX_ROWS / 16), img4 = xf_elems(4 * d, MAX_ROWS / 16);
    WIS_RET(dalloc(m, &m->dxf, img)); WIS_RET(dalloc(m, &m->daoxf, img)); WIS_RET(dalloc(m, &m->dhxf, img4));
    WIS_RET(dalloc(m, &m->dstat, (size_t)MAX_ROWS * (d / 16) * 2));
    WIS_HIP_CHECK(hipMemsetAsync(m->dxf, 0, img * 2, m->st)); WIS_HIP_CHECK(hipMemsetAsync(m->daoxf, 0, img * 2, m->st));
    WIS_HIP_CHECK(hipMemsetAsync(m->dhxf, 0, img4 * 2, m->st));
  }
  WIS_RET(dalloc(m, &m->logits, (size_t)MAX_ROWS * m->n_vocab_pad));
  // (row groups of the cross-attention: utterances - or, verifying a beam-search draft, up to MAX_ROWS / 16 groups of 16 tree rows of ONE utterance)
  const int Bg = Bm > MAX_ROWS / 16 ? Bm : MAX_ROWS / 16;
  WIS_RET(dalloc(m, &m->part, (size_t)Bg * H * 16 * 16 * 66));
  WIS_RET(dalloc(m, &m->counters, (size_t)Bg * H));
  WIS_HIP_CHECK(hipMemsetAsync(m->counters, 0, (size_t)Bg * H * 4, m->st));
  {
    // (K split of the batched FFN2: frag_ksplit_setting / ffn2_ksplit above)
    m->gf_ksplit = frag_ksplit_setting();
    const size_t nt = (size_t)cdiv(d, 16);
    WIS_RET(dalloc(m, &m->gf_part, nt * m->gf_ksplit * (MAX_ROWS / 16) * 64 * 4));
    WIS_RET(dalloc(m, &m->gf_cnt, nt));
    WIS_HIP_CHECK(hipMemsetAsync(m->gf_cnt, 0, nt * 4, m->st));
  }
  {
    const int bh = Bm * H < CA_SPIN_MAX_BH ? Bm * H : CA_SPIN_MAX_BH;
    WIS_RET(dalloc(m, &m->ca_gran, (size_t)bh * 6 * 8 * 66));
    WIS_RET(dalloc(m, &m->ca_epoch, (size_t)bh + 1));
    WIS_HIP_CHECK(hipMemsetAsync(m->ca_gran, 0, (size_t)bh * 6 * 8 * 66 * 8, m->st));
    WIS_HIP_CHECK(hipMemsetAsync(m->ca_epoch, 0, ((size_t)bh + 1) * 4, m->st));
  }
  WIS_RET(dalloc(m, &m->rm.tok, MAX_ROWS)); WIS_RET(dalloc(m, &m->rm.pos, MAX_ROWS));
  WIS_RET(dalloc(m, &m->rm.slot, MAX_ROWS)); WIS_RET(dalloc(m, &m->rm.lslot, MAX_ROWS));
  WIS_RET(dalloc(m, &m->rm_win.tok, MAX_ROWS)); WIS_RET(dalloc(m, &m->rm_win.pos, MAX_ROWS)); WIS_RET(dalloc(m, &m->rm_win.slot, MAX_ROWS)); WIS_RET(dalloc(m, &m->rm_win.lslot, MAX_ROWS));
  const int max_new = MAX_STEPS, max_hyp = MAX_HYP;
  WIS_RET(dalloc(m, &m->bs.step_u, Bm)); WIS_RET(dalloc(m, &m->bs.done, Bm)); WIS_RET(dalloc(m, &m->bs.n_hyp, Bm));
  WIS_RET(dalloc(m, &m->bs.cum, slots));
  WIS_RET(dalloc(m, &m->bs.alive, (size_t)slots * max_new));
  WIS_RET(dalloc(m, &m->bs.parent, (size_t)slots));
  WIS_RET(dalloc(m, &m->bs.row_done, (size_t)slots)); WIS_RET(dalloc(m, &m->d_seeds, (size_t)MAX_ROWS)); WIS_RET(dalloc(m, &m->d_plen, (size_t)MAX_ROWS)); WIS_RET(dalloc(m, &m->d_sa_tab, (size_t)2 * MAX_ROWS));
  WIS_RET(dalloc(m, &m->bs.hyp_score, (size_t)Bm * max_hyp)); WIS_RET(dalloc(m, &m->bs.hyp_len, (size_t)Bm * max_hyp));
  WIS_RET(dalloc(m, &m->bs.hyp_tok, (size_t)Bm * max_hyp * max_new));
  WIS_RET(dalloc(m, &m->bs.all_done, 4));
  WIS_RET(dalloc(m, &m->bs.tick, 4));
  WIS_RET(dalloc(m, &m->vstep, MAX_ROWS)); WIS_RET(dalloc(m, &m->pick_tok, MAX_ROWS)); WIS_RET(dalloc(m, &m->pick_lp, MAX_ROWS));
  WIS_RET(dalloc(m, &m->bs.traj, (size_t)Bm * MAX_STEPS * MAX_R * 2));
  WIS_RET(dalloc(m, &m->d_draft, sizeof(PinnedScratch::draft) / sizeof(int))); WIS_RET(dalloc(m, &m->d_anc, sizeof(PinnedScratch::anc) / sizeof(int))); WIS_RET(dalloc(m, &m->d_vstate, DRAFT_VS_INTS)); WIS_RET(dalloc(m, &m->d_base, MAX_ROWS));
  WIS_HIP_CHECK(hipMemsetAsync(m->bs.tick, 0, 16, m->st));
  WIS_RET(dalloc(m, &m->bs.out_ids, (size_t)slots * max_new)); WIS_RET(dalloc(m, &m->bs.out_len, slots)); WIS_RET(dalloc(m, &m->bs.out_score, slots));      // (up to max_beam results per utterance)
  WIS_RET(dalloc(m, &m->st_max, (size_t)MAX_ROWS * STAT_SUB)); WIS_RET(dalloc(m, &m->st_sum, (size_t)MAX_ROWS * STAT_SUB));
  WIS_RET(dalloc(m, &m->st_val, (size_t)MAX_ROWS * STAT_SUB * MAX_CAND)); WIS_RET(dalloc(m, &m->st_idx, (size_t)MAX_ROWS * STAT_SUB * MAX_CAND));
  WIS_RET(dalloc(m, &m->ts_desc, (size_t)MAX_ROWS * TS_DESC_INTS)); WIS_RET(dalloc(m, &m->d_nsp, (size_t)MAX_ROWS)); WIS_RET(dalloc(m, &m->d_nsp_rows, (size_t)MAX_ROWS));
  WIS_RET(dalloc(m, &m->d_in, (size_t)Bm * WIS_N_SAMPLES));
  WIS_RET(dalloc(m, &m->d_nsamp, Bm));
  WIS_RET(dalloc(m, &m->lm_logspec, (size_t)Bm * c.n_mels * WIS_N_FRAMES));
  WIS_RET(dalloc(m, &m->lm_gmax, Bm));
  WIS_RET(dalloc(m, &m->d_probs, (size_t)Bm * (c.n_lang > 0 ? c.n_lang : 1)));
  WIS_RET(dalloc(m, &m->d_prof, ((size_t)c.n_dec_layers * 8 + 2) * 16));   // + sampling kernels (tap builds)
  WIS_RET(dalloc(m, &m->d_trie, (size_t)PHRASE_MAX_RECORDS));      // (carved behind every buffer that existed before the phrase set did: each lies where it lay)
  WIS_RET(dalloc(m, &m->d_hot, (size_t)PHRASE_MAX_RECORDS + 1));      // (the last buffer carved, for the same reason; its last record holds the kernel's two control words)
  m->d_hot_ctl = reinterpret_cast<int*>(m->d_hot + PHRASE_MAX_RECORDS);
  WIS_HIP_CHECK(hipMemsetAsync(m->d_hot_ctl, 0, 16, m->st));
  WIS_HIP_CHECK(hipHostMalloc(reinterpret_cast<void**>(&m->h_pin), sizeof(PinnedScratch), hipHostMallocDefault));
  // fine-grained (coherent) host memory mapped into the device: beam_step_kernel's system-scope stores land here while the
  // stream is still running
  WIS_HIP_CHECK(hipHostMalloc(reinterpret_cast<void**>(&m->h_prog), HP_BYTES, hipHostMallocMapped | hipHostMallocCoherent));
  memset(m->h_prog, 0, HP_BYTES);
  { void* dp = nullptr; WIS_HIP_CHECK(hipHostGetDevicePointer(&dp, m->h_prog, 0)); m->bs.host = static_cast<unsigned long long*>(dp); }
  m->bs.giveup = m->ca_epoch;
  for (int i = 0; i < 8; ++i) WIS_HIP_CHECK(hipEventCreate(&m->ev[i]));
  WIS_HIP_CHECK(hipStreamCreateWithFlags(&m->st_enc, hipStreamNonBlocking));
  WIS_HIP_CHECK(hipEventCreateWithFlags(&m->ev_enc, hipEventDisableTiming));
  WIS_HIP_CHECK(hipEventCreateWithFlags(&m->ev_ckv, hipEventDisableTiming));
  WIS_HIP_CHECK(hipEventRecord(m->ev_ckv, m->st));
  return WIS_OK;
}

// ---- input -> conv1 image --------------------------------------------------------------
int stage_input(wis_model* m, const float* input, int kind, int B, hipStream_t on) {
  hipStream_t st = on ? on : m->st;
  if (kind == WIS_IN_PCM_HOST || kind == WIS_IN_PCM_DEV) {
    const float* dp = input;
    if (kind == WIS_IN_PCM_HOST) {
      WIS_HIP_CHECK(hipMemcpyAsync(m->d_in, input, (size_t)B * WIS_N_SAMPLES * 4, hipMemcpyHostToDevice, st));
      dp = m->d_in;
    }
    int64_t* hn = m->h_pin->nsamp;
    for (int b = 0; b < B; ++b) hn[b] = WIS_N_SAMPLES;
    WIS_HIP_CHECK(hipMemcpyAsync(m->d_nsamp, hn, (size_t)B * 8, hipMemcpyHostToDevice, st));
    WIS_RET(logmel_device(m->ctx, st, m->lm_logspec, m->lm_gmax, dp, WIS_N_SAMPLES, m->d_nsamp, B, nullptr, m->img, m->cfg.n_mels));
  } else if (kind == WIS_IN_MEL_HOST || kind == WIS_IN_MEL_DEV) {
    const float* dm = input;
    if (kind == WIS_IN_MEL_HOST) {
      WIS_HIP_CHECK(hipMemcpyAsync(m->d_in, input, (size_t)B * m->cfg.n_mels * 3000 * 4, hipMemcpyHostToDevice, st));      // d_in: B x 480000 floats
      dm = m->d_in;
    }
    WIS_RET(launch_mel_to_image(st, dm, m->img, B, m->cfg.n_mels));
  } else { set_error("bad input_kind %d", kind); return WIS_E_ARG; }
  return WIS_OK;
}

// ---- encoder + cross K/V ---------------------------------------------------------------
int run_encoder(wis_model* m, int B, hipStream_t on) {
  const wis_config_t& c = m->cfg; hipStream_t st = on ? on : m->st;
  const int d = c.d_model, H = c.n_heads, T = c.n_audio_ctx, M = B * T;
  {  // conv1: implicit im2col over the [3002][C] image; 80 bins: C = 96, K = 288 (+32 zero-weighted columns that read into the next
     // row); 128 bins: C = 128, K = 384
    WIS_RET(launch_gemm_conv1(st, conv1_gemm(m->img, m->w_conv1, B, 3000, c.n_mels, d), m->b_conv1, m->c1, 3000));
  }
  // conv2 (stride 2) + GELU + positions -> fp32 residual stream
  WIS_RET(launch_gemm_conv2(st, conv2_gemm(m->c1, m->w_conv2, B, T, d, d), m->b_conv2, m->enc_pos, m->x, T));
  // Few row tiles (one utterance of the larger models): FFN2 (N = d, K = 4d) has too few 128x128 tiles for 256 CUs, so K is split
  // over workgroups (240-480 of them) and the reduction launch carries the LayerNorm of whatever consumes the rows next - the next
  // layer's ln1, or ln_post after the last layer.  Measured for large-v2 at M = 1500 with the weights streamed from HBM
  // (tools/gemm_lab.hip): 64x128 tiles over the whole K 52 us; 2 splits 42.6 + 6.0 (reduce) + 6.2 (LayerNorm) us; 4 splits + fused
  // reduce-LayerNorm: see profiles/.
  const int splits = enc_splitk(d, M);
  const bool split = splits > 0;
  bool xn_ready = false;
  for (int l = 0; l < c.n_enc_layers; ++l) {
    const EncLayerW& w = m->enc[l];
    if (!xn_ready) WIS_RET(launch_layernorm(st, m->x, w.ln1_g, w.ln1_b, m->xn, M, d));
    WIS_RET(launch_gemm_qkv(st, gemm_plain(m->xn, d, w.w_qkv, M, 3 * d, d), w.b_qkv, m->qk, m->vt, d, T, m->Tpad, H));
    WIS_RET(launch_enc_attention(st, m->qk, m->vt, m->ao, B, T, m->Tpad, H, m->enc_part, m->enc_cnt, m->enc_part_cap));
    WIS_RET(launch_gemm_generic(st, gemm_plain(m->ao, d, w.w_out, M, d, d), w.b_out, m->x, m->x, 2 | 4));
    WIS_RET(launch_layernorm(st, m->x, w.ln2_g, w.ln2_b, m->xn, M, d));
    WIS_RET(launch_gemm_generic(st, gemm_plain(m->xn, d, w.w_f1, M, 4 * d, d), w.b_f1, nullptr, m->hbuf, 1));
    if (split) {
      const bool last = l + 1 == c.n_enc_layers;
      const float* g = last ? m->enc_ln_g : m->enc[l + 1].ln1_g;
      const float* b = last ? m->enc_ln_b : m->enc[l + 1].ln1_b;
      WIS_RET(launch_gemm_splitk_resid(st, gemm_plain(m->hbuf, 4 * d, w.w_f2, M, d, 4 * d), splits, m->skbuf, w.b_f2, m->x, m->x, g, b, last ? m->mem : m->xn));
      xn_ready = true;
    } else {
      WIS_RET(launch_gemm_generic(st, gemm_plain(m->hbuf, 4 * d, w.w_f2, M, d, 4 * d), w.b_f2, m->x, m->x, 2 | 4));
    }
  }
  if (!split) WIS_RET(launch_layernorm(st, m->x, m->enc_ln_g, m->enc_ln_b, m->mem, M, d));
  return WIS_OK;
}
int run_cross_kv(wis_model* m, int B, const f16* mem) {
  const wis_config_t& c = m->cfg;
  const int d = c.d_model, T = c.n_audio_ctx;
  // every decoder layer's K/V projection of the encoder memory in one GEMM (weights, biases and outputs are single blocks)
  return launch_gemm_crosskv(m->st, gemm_plain(mem ? mem : m->mem, d, m->w_ckv_all, B * T, c.n_dec_layers * 2 * d, d), m->b_ckv_all, m->kx_all, m->vx_all, d, T, m->Tpad,
                             c.n_heads, (int64_t)m->kx_lstride, (int64_t)m->vx_lstride);
}
// input -> cross K / V (model.hpp has the contract).  The caller has checked B (check_batch) and that `input` is not null.
int run_front(wis_model* m, const float* input, int kind, int B, hipStream_t enc, bool timed) {
  hipStream_t st = m->st;
  const bool given = input_is_encoded(kind);
  hipStream_t se = (enc && !given) ? enc : st;
  const f16* mem = nullptr;
  m->front_skipped = given;
  if (timed) WIS_HIP_CHECK(hipEventRecord(m->ev[0], se));
  if (!given) WIS_RET(stage_input(m, input, kind, B, se));
  if (timed) WIS_HIP_CHECK(hipEventRecord(m->ev[1], se));
  if (!given) WIS_RET(run_encoder(m, B, se));
  if (timed) WIS_HIP_CHECK(hipEventRecord(m->ev[2], se));
  if (se != st) { WIS_HIP_CHECK(hipEventRecord(m->ev_enc, se)); WIS_HIP_CHECK(hipStreamWaitEvent(st, m->ev_enc, 0)); }
  if (kind == WIS_IN_ENC_DEV) mem = reinterpret_cast<const f16*>(input);
  if (kind == WIS_IN_ENC_HOST) {
    const int64_t n = (int64_t)B * m->cfg.n_audio_ctx * m->cfg.d_model;
    if (n % 8) { set_error("WIS_IN_ENC_HOST: d_model %d is not a multiple of 8", m->cfg.d_model); return WIS_E_UNSUPPORTED; }
    WIS_HIP_CHECK(hipMemcpyAsync(m->x, input, (size_t)n * 4, hipMemcpyHostToDevice, st));      // x [max_batch T][d] f32: the residual stream, free outside the encoder
    hipLaunchKernelGGL(enc_f32_to_f16_kernel, dim3(blocks_for(n / 8)), dim3(256), 0, st, reinterpret_cast<const float4*>(m->x), reinterpret_cast<f16x8*>(m->mem), n / 8);
  }
  WIS_RET(run_cross_kv(m, B, mem));
  if (timed) WIS_HIP_CHECK(hipEventRecord(m->ev[3], st));
  return WIS_OK;
}

// ---- granule hand-off of the cross-attention: when it may be used -------------------------------
// Its progress argument ("at most CA_SPIN_MAX_BH combiners spin, fewer than the chip's CUs, so a producer always finds a slot") is about
// everything that runs on the GPU at the same time, so the budget is kept per DEVICE and claimed per CALL: a call that wants the
// granule form adds its B x heads combiners to the device's count for its duration and takes the ticket form when that would
// exceed the budget.  (Until round 5 the budget was divided by the handles ALIVE on the device - a server holding several model
// sizes at four replicas each never got the granule form although at most a few of its handles decode at any time, while bench.py,
// with one handle, always did: the published decode numbers were for a path the server did not run.)  Whatever happens, a spin
// that runs out never fails a request: the flag travels with every step's progress record / is read after every tap pass, the handle
// switches to the ticket form for good and the call is run again (wis_generate / wis_detect_language / the logits taps).
// The budget is process-wide state: it is defined here and nowhere else, and generate.hip, taps.hip and align.hip claim from it through
// SpinClaim (declared in model.hpp, its members defined below).
std::atomic<int> g_spin_bh[64];
// claims whose call has returned while ONE over-run decode step of it may still be running on the handle's stream (a search that ended on
// EOT does not wait for the step queued behind the one that finished it): the combiners of that step still spin, so its share of the
// budget is released only when the event recorded behind it has completed - checked by whoever claims next on the device (advisor, round 5:
// released at return, the budget could be over-subscribed for the length of one step)
struct DeferredClaim { hipEvent_t ev; int n; };
std::mutex g_spin_mu;
std::vector<DeferredClaim> g_spin_deferred[64];
static void spin_collect(int device) {
  std::lock_guard<std::mutex> lk(g_spin_mu);
  auto& v = g_spin_deferred[device & 63];
  for (size_t i = 0; i < v.size();) {
    if (hipEventQuery(v[i].ev) != hipErrorNotReady) { g_spin_bh[device & 63].fetch_sub(v[i].n, std::memory_order_relaxed); v[i] = v.back(); v.pop_back(); }
    else ++i;
  }
}
SpinClaim::SpinClaim(wis_model* mm, int B) : m(mm) {
  static const bool env_share = getenv("WIS_CA_SPIN_SHARED") != nullptr;      // test switch: ignore the budget (exercises the shared-GPU hazard on purpose)
  m->spin_now = false;
  spin_collect(m->device);
  if (m->spin_off) return;
  if (env_share) { m->spin_now = true; return; }
  const int need = B * m->cfg.n_heads;
  std::atomic<int>& a = g_spin_bh[m->device & 63];
  int cur = a.load(std::memory_order_relaxed);
  while (cur + need <= CA_SPIN_MAX_BH)
    if (a.compare_exchange_weak(cur, cur + need, std::memory_order_relaxed)) { n = need; m->spin_now = true; return; }
}
SpinClaim::~SpinClaim() { if (n) g_spin_bh[m->device & 63].fetch_sub(n, std::memory_order_relaxed); }
// the call returns with work of its own still queued on `st`: hand the claim to the deferred list behind an event on that stream
void SpinClaim::defer(hipStream_t st) {
  if (!n) return;
  if (hipEventRecord(m->ev[6], st) != hipSuccess) return;      // (then the destructor releases as before)
  std::lock_guard<std::mutex> lk(g_spin_mu);
  auto& v = g_spin_deferred[m->device & 63];
  for (auto& d : v) if (d.ev == m->ev[6]) { d.n += n; n = 0; return; }      // (re-recorded: the earlier share now waits for the later record too)
  v.push_back({m->ev[6], n}); n = 0;
}
// reads and clears the give-up flag (word 0 of the epoch block); true = a combiner gave up: results of the pass are garbage
int spin_gave_up(wis_model* m, bool* gave_up) {
  int* h = &m->h_pin->giveup;
  WIS_HIP_CHECK(hipMemcpyAsync(h, m->ca_epoch, 4, hipMemcpyDeviceToHost, m->st));
  WIS_HIP_CHECK(hipStreamSynchronize(m->st));
  *gave_up = *h != 0;
  if (*gave_up) {
    WIS_HIP_CHECK(hipMemsetAsync(m->ca_epoch, 0, 4, m->st));
    m->spin_off = true; ++m->handoff_retries;
    fprintf(stderr, "[wis_hip] device %d: decoder cross-attention granule hand-off timed out; this handle uses the ticket hand-off from now on, the call is repeated\n", m->device);
  }
  return WIS_OK;
}

// ---- one decoder forward over the current row metadata ---------------------------------
// sstride / rmul: logical-slot mapping of the rows (decode rows: beam, 1; prefill rows: beam, 0; single rows: 1, 0)
// Batched rows (8 < M <= 48): every activation a projection reads lives in HBM as an MFMA fragment image, LayerNorm statistics
// travel as per-16-column partial sums from the residual epilogues (kernels.hpp launch_gemv_frag): 8 launches per layer, no
// LayerNorm launch, no per-workgroup LDS staging of the activations.
// tw: a tree window (model.hpp TreeWin)

// ---- the step's projection stages: the ONLY places that assemble a GemvP from a projection (both forwards, the weight-stream tap, the op taps); raw
// operand pointers, so a tap passes its own scratch; every member they do not name stays zero.  launch_gemv (<= 8 rows): x fp32 under GV_LN, else f16
GemvP gemv_small(const DecProj& p, const void* x, void* y, int M, int flags) {
  GemvP g; memset(&g, 0, sizeof(g));
  g.x = x; g.csum = p.csum; g.Wp = p.Wp; g.wscale = p.scale; g.bias = p.bias; g.y = y; g.M = M; g.N = p.N; g.K = p.K; g.flags = flags; g.rows = p.rows;
  // eight-column tiles where the projection has that image (FFN2, cross-attention out-projection of large models): f16 rows, plain or residual epilogue
  if (p.Wp8 && !(flags & ~(GV_RESID | GV_OUT_F32 | GV_GELU)) && gemv_nc8_shape(M, p.N, p.K)) { g.Wp = p.Wp8; g.rows = 8; }
  // five-column slabs where the projection has that image (FFN2 of large models): one workgroup on every CU, f16 rows, plain or residual epilogue
  if (p.Wp5 && !p.scale && !p.csum && gemv_nc5_shape(M, p.N, p.K, flags)) { g.Wp = p.Wp5; g.rows = 5; }
  return g;
}
// launch_gemv_frag (batched rows) on the rows' fragment image; the caller adds the stage's own: output, statistics, QKV cache members, prof, FFN2's K split
GemvP gemv_frag(const DecProj& p, const void* xf, int M, int flags) {
  GemvP g; memset(&g, 0, sizeof(g));
  g.x = xf; g.csum = p.csum; g.Wp = p.Wp; g.wscale = p.scale; g.bias = p.bias; g.M = M; g.N = p.N; g.K = p.K; g.flags = flags; g.xmb = cdiv(M, 16); g.rows = 16;
  return g;
}
// The fused out-projection + cross-Q stage (cq_fold; w.cqo = packed [W'q | W'q Wo], W'q bo), <= 8 rows, ONE launch_gemv_dual (`rows` of gb: 8 = w.cqo's
// eight-column image, where the loader added one and out_cq_nc8_shape holds for these rows - 160 workgroups on the cross-Q's side instead of 80; else 0):
//   ga: x1 = x0 + Wo a + bo in place, x1's LayerNorm partials to `stat` (the cross-attention's prologue merges them: decode step 1.352 -> 1.330 ms)
//   gb: q_raw = W'q x0 + (W'q Wo) a + W'q bo from the f16 layer input xh and the attention output a; the cross-attention kernel applies rs, mu of x1 and b'
void out_cq_dual(const DecLayerW& w, const f16* a, const f16* xh, float* x1, float* stat, float* q, int M, GemvP* ga, GemvP* gb) {
  const int d = w.out.K;
  memset(ga, 0, sizeof(*ga));
  ga->x = a; ga->Wp = w.out.Wp; ga->bias = w.out.bias; ga->y = x1; ga->M = M; ga->N = d; ga->K = d; ga->flags = GV_RESID; ga->stat_out = stat;
  memset(gb, 0, sizeof(*gb));
  gb->x = xh; gb->x2 = a; gb->xsplit = d; gb->Wp = w.cqo.Wp; gb->bias = w.cqo.bias; gb->y = q; gb->M = M; gb->N = d; gb->K = w.cqo.K; gb->flags = GV_OUT_F32;
  if (w.cqo.Wp8 && out_cq_nc8_shape(M, d)) { gb->Wp = w.cqo.Wp8; gb->rows = 8; }
}
// The same stage on batched rows, ONE launch_gemv_frag3 of three d x d problems: x1 = x0 + Wo a + bo (+ partials; x1's fragment image has no reader, so
// x0's image xf stays valid), q = W'q x0 + W'q bo and q2 = (W'q Wo) a - the two k-step halves of w.cqo.  The cross-attention kernel finishes
// q = rs (q + q2 - mu c) + b': the folded cross-Q projection as a launch of its own (6.4 us per layer at 8 utterances) is gone.
void out_cq_frag3(const DecLayerW& w, const f16* af, const f16* xf, float* x1, float* stat, float* q, float* q2, int M, GemvP g3[3]) {
  const int d = w.out.K;
  g3[0] = gemv_frag(w.out, af, M, GV_RESID);
  g3[0].wscale = nullptr; g3[0].y = x1; g3[0].ymb = g3[0].xmb; g3[0].stat_out = stat;
  g3[1] = gemv_frag(w.cqo, xf, M, GV_OUT_F32);
  g3[1].K = d; g3[1].y = q; g3[1].wks = w.cqo.K / 32; g3[1].wk0 = 0;
  g3[2] = gemv_frag(w.cqo, af, M, GV_OUT_F32);
  g3[2].K = d; g3[2].bias = nullptr; g3[2].y = q2; g3[2].wks = w.cqo.K / 32; g3[2].wk0 = d / 32;
}

// The other stages of the batched route, as dec_forward_frag and the wis_op_gemv_frag_stage tap launch them (ymb = the rows' own row blocks):
//   frag_resid        y += W x + b in place (cross-attention out-projection, FFN2; the self-attention out-projection when the fold is off), the rows' f16
//                     fragment image and per-16-column LayerNorm partials for the projection that follows (either may be null)
//   frag_ln_f32       the LayerNorm-folded projection into fp32 rows (cross-Q when the fold is off, the vocabulary): statistics from the producer's partials
//   frag_ln_gelu_xf   FFN1: LayerNorm-folded, GELU, the f16 rows straight into FFN2's fragment image
GemvP frag_resid(const DecProj& p, const f16* xf, float* y, f16* y_xf, float* stat_out, int M) {
  GemvP g = gemv_frag(p, xf, M, GV_RESID);
  g.y = y; g.y_xf = y_xf; g.ymb = g.xmb; g.stat_out = stat_out;
  return g;
}
GemvP frag_ln_f32(const DecProj& p, const f16* xf, const float* stat_in, float* y, int M) {
  GemvP g = gemv_frag(p, xf, M, GV_LN | GV_OUT_F32);
  g.stat_in = stat_in; g.y = y;
  return g;
}
GemvP frag_ln_gelu_xf(const DecProj& p, const f16* xf, const float* stat_in, f16* y_xf, int M) {
  GemvP g = gemv_frag(p, xf, M, GV_LN | GV_GELU);
  g.stat_in = stat_in; g.y = y_xf; g.ymb = g.xmb;
  return g;
}
// WIS_SA_LONG=0: A/B switch and fallback of the long-prompt route's step self-attention
bool sa_long_kernel(const wis_model* m) {
  static const bool sa_long_on = !(getenv("WIS_SA_LONG") && atoi(getenv("WIS_SA_LONG")) == 0);
  return m->sa_long_form >= 0 ? m->sa_long_form != 0 : sa_long_on;
}
// the decode step of the long-prompt route (wis_model::sa_plen set around it): the rows read their utterance's prompt prefix in its first slot - through
// dec_self_attn_long_kernel, or as a TREE of width 1 (base = the utterance's first slot, the one ancestor = the row's own slot, w0 = the prompt length)
static void sa_shared_prefix(const wis_model* m, SelfAttnP* sa) {
  if (!m->sa_plen) return;
  if (sa_long_kernel(m)) { sa->plen = m->sa_plen; return; }
  sa->anc = m->d_sa_tab; sa->base = m->d_sa_tab + MAX_ROWS; sa->w0 = m->sa_w0; sa->aw = 1;
}
static int dec_forward_frag(wis_model* m, int M, int R, int B, bool want_logits, int sstride, int rmul, int chunks, const TreeWin* tw = nullptr) {
  const wis_config_t& c = m->cfg; hipStream_t st = m->st;
  const int d = c.d_model, H = c.n_heads, T = c.n_audio_ctx, ctx = c.n_text_ctx, MB = cdiv(M, 16);
  if (tw && (M % 16 != 0 || R != 16 || B != M / 16)) { set_error("dec_forward_frag: a tree window takes whole groups of 16 rows"); return WIS_E_ARG; }
  WIS_RET(launch_dec_embed_xf(st, m->emb, m->dec_pos, m->rm.tok, m->rm.pos, m->dx, m->dxf, m->dstat, M, d, MB));
  // cross-Q folded through the self-attention out-projection (f16 weights; <= 8 rows per utterance: the cross-attention kernel's
  // statistics prologue); WIS_NO_FRAG_FOLD=1 keeps the two-launch form (A/B switch)
  static const bool no_frag_fold = getenv("WIS_NO_FRAG_FOLD") != nullptr;
  const bool fold = m->cq_fold && !no_frag_fold && R <= 8;
  // what every layer's attention launches share; the layer adds its caches / K, V images (and its stamp row)
  SelfAttnP sa;
  sa.q = m->dq; sa.pos = m->rm.pos; sa.out = m->daoxf; sa.M = M; sa.H = H; sa.d = d; sa.ctx = ctx; sa.rpu = R; sa.sstride = sstride; sa.rmul = rmul; sa.out_mb = MB; sa.nb = m->sa_nb;
  if (!tw) sa_shared_prefix(m, &sa);
  if (tw) { sa.anc = tw->anc; sa.w0 = tw->w0; sa.aw = tw->aw; sa.base = tw->base; }
  CrossAttnP ca;
  ca.q = m->dq; ca.out = m->daoxf; ca.part = m->part; ca.counters = m->counters; ca.B = B; ca.R = R; ca.H = H; ca.d = d; ca.T = T; ca.Tpad = m->Tpad; ca.chunks = chunks; ca.out_mb = MB;
  ca.epoch = m->ca_epoch;
  for (int l = 0; l < c.n_dec_layers; ++l) {
    const DecLayerW& w = m->dec[l];
    // (tap builds: stamp rows of layer 0's kernels, same row numbering as dec_forward: 0 QKV, 1 self-attn, 2 out-proj (+ q halves), 4 cross-attn,
    // 5 cross-out, 6 FFN1, 7 FFN2)
    unsigned long long* pr = (m->prof_on && l == 0) ? m->d_prof : nullptr;
    GemvP g = gemv_frag(w.qkv, m->dxf, M, GV_LN | GV_QKV);
    g.stat_in = m->dstat; g.q = m->dq; g.kc = m->kc[l]; g.vc = m->vc[l]; g.slot = m->rm.slot; g.pos = m->rm.pos; g.d = d; g.ctx = ctx;
    g.prof = pr;
    WIS_RET(launch_gemv_frag(st, g));
    sa.kc = m->kc[l]; sa.vc = m->vc[l];
    WIS_RET(launch_dec_self_attn(st, sa));
    if (fold) {
      if (m->al.capture) { set_error("dec_forward_frag: an alignment pass needs the un-folded route (more than 8 rows per utterance)"); return WIS_E_STATE; }
      GemvP g3[3];
      out_cq_frag3(w, m->daoxf, m->dxf, m->dx, m->dstat, m->dq, m->dq2, M, g3);
      g3[0].prof = pr ? pr + 32 : nullptr;
      WIS_RET(launch_gemv_frag3(st, g3, 3));
      CrossAttnP cf = ca;      // the batched fold: q = q + q2, statistics from x1's row partials
      cf.kx = m->kx[l]; cf.vt = m->vx[l]; cf.prof = pr ? pr + 64 : nullptr; cf.xres = m->dstat; cf.qcs = w.cq.csum; cf.qb = w.cq.bias;
      cf.gran = m->spin_now ? m->ca_gran : nullptr; cf.q2 = m->dq2; cf.xres_is_stat = 1;
      WIS_RET(launch_dec_cross_attn(st, cf));
    } else {
    g = frag_resid(w.out, m->daoxf, m->dx, m->dxf, m->dstat, M);
    WIS_RET(launch_gemv_frag(st, g));
    g = frag_ln_f32(w.cq, m->dxf, m->dstat, m->dq, M);
    WIS_RET(launch_gemv_frag(st, g));
    // (wis_align decodes a batch in groups of utterances: the group's first utterance picks the K / V block the rows' b = 0 reads; 0 otherwise)
    const size_t ku = (size_t)m->al.kv_ub0 * H * T * 64, vu = (size_t)m->al.kv_ub0 * H * 64 * m->Tpad;
    CrossAttnP cp = ca;
    cp.kx = m->kx[l] + ku; cp.vt = m->vx[l] + vu; cp.gran = (m->spin_now && !tw) ? m->ca_gran : nullptr; cp.kv_shared = (tw && !tw->own_kv) ? 1 : 0;
    WIS_RET(launch_dec_cross_attn(st, cp));
    if (m->al.capture) WIS_RET(align_capture_q(m, l, M));      // wis_align: m->dq holds this layer's finished cross-Q until the next layer's QKV projection
    }
    g = frag_resid(w.cout, m->daoxf, m->dx, m->dxf, m->dstat, M);
    g.prof = pr ? pr + 80 : nullptr;
    WIS_RET(launch_gemv_frag(st, g));
    g = frag_ln_gelu_xf(w.f1, m->dxf, m->dstat, m->dhxf, M);
    g.prof = pr ? pr + 96 : nullptr;
    WIS_RET(launch_gemv_frag(st, g));
    g = frag_resid(w.f2, m->dhxf, m->dx, m->dxf, m->dstat, M);
    g.prof = pr ? pr + 112 : nullptr;
    frag_set_ksplit(g, ffn2_ksplit(w.f2.K), m->gf_part, m->gf_cnt);      // K = 4d over `ksplit` workgroups per n-tile
    WIS_RET(launch_gemv_frag(st, g));
  }
  if (want_logits) {
    GemvP g = frag_ln_f32(m->proj, m->dxf, m->dstat, m->logits, M);
    WIS_RET(launch_gemv_frag(st, g));
  }
  return WIS_OK;
}

// The route of a pass of M rows without a tree window (dec_forward; wis_bench_weight_stream streams every matrix alone by the same choice):
//   frag   more than 8 rows: dec_forward_frag.  The other two describe the <= 8-row step:
//   fold   the fused out-projection + cross-Q stage (cq_fold: f16 decoder weights)
//   ln16   WIS_B1_LN=f16 (off by default: statistics of rounded rows cost parity at large-v2): the LayerNorm-folded projections (QKV,
//          FFN1, the vocabulary) read the f16 copy of the rows their producers leave (GV_LN16, 12.8 KB against 25.6 KB at five rows) and take the statistics
//          from it.  (Statistics from the producers' per-16-column partials measured slower, 1.357 against 1.345 ms per step.)
StepRoute small_route(const wis_model* m, int M) {
  static const bool ln_f16 = [] { const char* e = getenv("WIS_B1_LN"); return e && !strcmp(e, "f16"); }();
  const int d = m->cfg.d_model;
  const bool frag = M > 8, ln_ok = !frag && m->cq_fold && d % 64 == 0 && M * (d / 8) <= 13 * 256;
  return {frag, m->cq_fold, ln_ok && ln_f16 && d <= 2048};
}

// The step of <= 8 rows: LDS-staged skinny GEMMs (launch_gemv) with the LayerNorm folded into their prologue; more rows and tree windows take
// dec_forward_frag.  One launch per stage: running the self-attention inside the QKV projection's launch (granule hand-off) was built, bit-identical and
// slower (1.280 against 1.250 ms per step) - an in-launch hand-off is two fabric round trips, like a kernel boundary (retired experiments).
int dec_forward(wis_model* m, int M, int R, int B, bool want_logits, int sstride, int rmul, const TreeWin* tw) {
  const wis_config_t& c = m->cfg; hipStream_t st = m->st;
  const int d = c.d_model, H = c.n_heads, T = c.n_audio_ctx, ctx = c.n_text_ctx;
  static const int env_chunks = getenv("WIS_CROSS_CHUNKS") ? atoi(getenv("WIS_CROSS_CHUNKS")) : 0;
  // 256-key chunks (6 per utterance-head): measured faster than 128-key chunks at every batch size (fewer partials to publish and combine)
  const int chunks = env_chunks ? env_chunks : 6;
  const StepRoute rt = small_route(m, M);
  if (tw || rt.frag) return dec_forward_frag(m, M, R, B, want_logits, sstride, rmul, chunks, tw);
  if (m->al.capture) { set_error("wis_align needs the batched-row decoder route (more than 8 rows per pass)"); return WIS_E_STATE; }
  const bool fold = rt.fold, ln16 = rt.ln16;
  // the LayerNorm-folded projections: the fp32 rows, or their f16 copy `x16`
  const int ln = ln16 ? GV_LN16 : GV_LN;
  auto ln_x = [&](const f16* x16) { return ln16 ? (const void*)x16 : (const void*)m->dx; };
  WIS_RET(launch_dec_embed(st, m->emb, m->dec_pos, m->rm.tok, m->rm.pos, m->dx, M, d, fold ? m->dxh : nullptr));
  SelfAttnP sa;
  sa.q = m->dq; sa.pos = m->rm.pos; sa.out = m->dao; sa.M = M; sa.H = H; sa.d = d; sa.ctx = ctx; sa.rpu = R; sa.sstride = sstride; sa.rmul = rmul; sa.nb = m->sa_nb;
  sa_shared_prefix(m, &sa);
  CrossAttnP ca;
  ca.q = m->dq; ca.out = m->dao; ca.part = m->part; ca.counters = m->counters; ca.B = B; ca.R = R; ca.H = H; ca.d = d; ca.T = T; ca.Tpad = m->Tpad; ca.chunks = chunks;
  ca.gran = m->spin_now ? m->ca_gran : nullptr; ca.epoch = m->ca_epoch;
  for (int l = 0; l < c.n_dec_layers; ++l) {
    const DecLayerW& w = m->dec[l];
    // stamp rows of this layer's 8 kernels: QKV, self-attn, out, cross-Q, cross-attn, cross-out, FFN1, FFN2
    unsigned long long* pr = (m->prof_on && (l == 0 || m->prof_all)) ? m->d_prof + (size_t)l * 8 * 16 : nullptr;
    // self-attention block
    GemvP g = gemv_small(w.qkv, ln_x(m->dxh), nullptr, M, ln | GV_QKV);
    g.q = m->dq; g.kc = m->kc[l]; g.vc = m->vc[l]; g.slot = m->rm.slot; g.pos = m->rm.pos; g.d = d; g.ctx = ctx;
    g.prof = pr;
    WIS_RET(launch_gemv(st, g));
    sa.kc = m->kc[l]; sa.vc = m->vc[l]; sa.prof = pr ? pr + 16 : nullptr;
    WIS_RET(launch_dec_self_attn(st, sa));
    ca.kx = m->kx[l]; ca.vt = m->vx[l]; ca.prof = pr ? pr + 64 : nullptr;
    if (fold) {
      GemvP ga, gb;
      out_cq_dual(w, m->dao, m->dxh, m->dx, m->dstat, m->dq, M, &ga, &gb);
      ga.prof = pr ? pr + 32 : nullptr;
      gb.prof = pr ? pr + 48 : nullptr;      // (arm B stamps the cross-Q row, which the fold leaves free)
      WIS_RET(launch_gemv_dual(st, ga, gb));
      CrossAttnP cf = ca;      // the folded query: statistics of x1 from the out-projection's row partials
      cf.xres = m->dstat; cf.qcs = w.cq.csum; cf.qb = w.cq.bias; cf.xres_is_stat = 1;
      WIS_RET(launch_dec_cross_attn(st, cf));
    } else {
    g = gemv_small(w.out, m->dao, m->dx, M, GV_RESID);
    g.prof = pr ? pr + 32 : nullptr;
    WIS_RET(launch_gemv(st, g));
    // cross-attention block
    g = gemv_small(w.cq, m->dx, m->dq, M, GV_LN | GV_OUT_F32);
    g.prof = pr ? pr + 48 : nullptr;
    WIS_RET(launch_gemv(st, g));
    WIS_RET(launch_dec_cross_attn(st, ca));
    }
    g = gemv_small(w.cout, m->dao, m->dx, M, GV_RESID);
    g.prof = pr ? pr + 80 : nullptr;
    if (ln16) g.y16 = m->dln;      // FFN1's input: f16 rows
    WIS_RET(launch_gemv(st, g));
    // FFN
    g = gemv_small(w.f1, ln_x(m->dln), m->dh, M, ln | GV_GELU);
    g.prof = pr ? pr + 96 : nullptr;
    WIS_RET(launch_gemv(st, g));
    g = gemv_small(w.f2, m->dh, m->dx, M, GV_RESID);
    g.prof = pr ? pr + 112 : nullptr;
    g.y16 = fold ? m->dxh : nullptr;             // the next layer's x0 in f16
    WIS_RET(launch_gemv(st, g));
  }
  if (want_logits) WIS_RET(launch_gemv(st, gemv_small(m->proj, ln_x(m->dxh), m->logits, M, ln | GV_OUT_F32)));
  return WIS_OK;
}

// search state of a device batch: beams tiled up front with scores [0, -inf, ...] (CT2 GPU path), counters cleared
// (samples: the rows of an utterance are independent samples - every one starts live, with its own done flag; n_res results per utterance)
int init_beam_state(wis_model* m, int B, int beam, bool samples, int n_res) {
  hipStream_t st = m->st;
  const int Mrows = B * beam;
  // staged in pinned memory of its own (PinnedScratch::beam_cum / beam_tick): the copies run when the stream gets there, nothing waits for them here
  float* cum = m->h_pin->beam_cum;
  for (int r = 0; r < Mrows; ++r) cum[r] = (r % beam == 0 || samples) ? 0.f : -INFINITY;
  unsigned* tk = m->h_pin->beam_tick;
  m->gen = (m->gen % 0xFFFFu) + 1u;      // 1 .. 65535: never the 0 of a cleared record
  tk[0] = 0; tk[1] = m->gen; tk[2] = 0; tk[3] = 0;
  WIS_HIP_CHECK(hipMemcpyAsync(m->bs.cum, cum, (size_t)Mrows * 4, hipMemcpyHostToDevice, st));
  WIS_HIP_CHECK(hipMemcpyAsync(m->bs.tick, tk, 16, hipMemcpyHostToDevice, st));
  WIS_HIP_CHECK(hipMemsetAsync(m->bs.step_u, 0, (size_t)B * 4, st));
  WIS_HIP_CHECK(hipMemsetAsync(m->bs.done, 0, (size_t)B * 4, st));
  WIS_HIP_CHECK(hipMemsetAsync(m->bs.n_hyp, 0, (size_t)B * 4, st));
  WIS_HIP_CHECK(hipMemsetAsync(m->bs.all_done, 0, 16, st));
  WIS_HIP_CHECK(hipMemsetAsync(m->bs.out_len, 0, (size_t)B * n_res * 4, st));
  if (samples) WIS_HIP_CHECK(hipMemsetAsync(m->bs.row_done, 0, (size_t)Mrows * 4, st));
  return WIS_OK;
}
// the utterances' Philox keys of a sampled decode (seeds NULL: all 0), staged like the search counters
int upload_seeds(wis_model* m, const uint64_t* seeds, int B) {
  unsigned long long* h = m->h_pin->seeds;
  for (int b = 0; b < B; ++b) h[b] = seeds ? (unsigned long long)seeds[b] : 0ull;
  WIS_HIP_CHECK(hipMemcpyAsync(m->d_seeds, h, (size_t)B * 8, hipMemcpyHostToDevice, m->st));
  return WIS_OK;
}
// decoding options -> what the sampling kernels take (CTranslate2 4.1.0 BeamSearch defaults where WIS passes none, main.py:687-693)
SampleCfg make_sample_cfg(const wis_model* m, const wis_gen_opts_t* o, int beam, int max_new, float* patience_out) {
  const wis_config_t& c = m->cfg;
  SampleCfg sc; memset(&sc, 0, sizeof(sc));
  sc.n_vocab = c.n_vocab; sc.n_vocab_pad = m->n_vocab_pad; sc.eot = c.eot; sc.beam = beam; sc.n_cand = 2 * beam; sc.max_new = max_new;
  sc.fixed_new = o->fixed_new_tokens; sc.suppress_blank = o->suppress_blank; sc.greedy = beam == 1;
  sc.length_penalty = o->length_penalty; sc.max_hyp = MAX_HYP;
  const float patience = o->patience > 0.f ? o->patience : 1.f;
  // hypotheses an utterance can hold: the search ends once max_candidates exist and one step adds at most `beam`, so
  // max_candidates + beam - 1 slots never overflow (MAX_HYP = 3 MAX_R: patience <= 2 at any beam; check_patience refuses more)
  sc.max_candidates = (int)lroundf((float)beam * patience); if (sc.max_candidates < 1) sc.max_candidates = 1;
  // CT2: allow_early_exit = patience == 1 && length_penalty == 0 && coverage_penalty == 0
  sc.allow_early_exit = (patience == 1.f && o->length_penalty == 0.f) ? 1 : 0;
  sc.early_exit_hyps = WIS_EARLY_EXIT_NUM_HYPOTHESES ? 1 : sc.max_candidates;      // num_hypotheses = 1; resolve_sample_opts (generate.hip) puts a caller's n here
  *patience_out = patience;
  return sc;
}

// A patience the hypothesis storage cannot honour is an argument error, not a silently shorter search (CTranslate2 would keep
// searching until round(beam x patience) hypotheses exist and return different ids)
int check_patience(int beam, float patience) {
  const float p = patience > 0.f ? patience : 1.f;
  const long want = lroundf((float)beam * p);
  if (want > MAX_HYP - beam + 1) {
    set_error("patience %.3g at beam_size %d needs %ld finished hypotheses; the engine holds %d (patience <= %.3g at this beam)", (double)p, beam, want, MAX_HYP - beam + 1,
              (double)(MAX_HYP - beam + 1) / (double)beam);
    return WIS_E_ARG;
  }
  return WIS_OK;
}

int upload_rows(wis_model* m, const std::vector<int>& tok, const std::vector<int>& pos, const std::vector<int>& slot, const std::vector<int>& lslot, bool wait, RowStage* stage) {
  const size_t n = tok.size();
  RowStage* h = stage ? stage : &m->h_pin->rows;      // (a caller that uploads twice without a wait in between passes a second staging area)
  memcpy(h->tok, tok.data(), n * 4); memcpy(h->pos, pos.data(), n * 4); memcpy(h->slot, slot.data(), n * 4); memcpy(h->lslot, lslot.data(), n * 4);
  WIS_HIP_CHECK(hipMemcpyAsync(m->rm.tok, h->tok, n * 4, hipMemcpyHostToDevice, m->st));
  WIS_HIP_CHECK(hipMemcpyAsync(m->rm.pos, h->pos, n * 4, hipMemcpyHostToDevice, m->st));
  WIS_HIP_CHECK(hipMemcpyAsync(m->rm.slot, h->slot, n * 4, hipMemcpyHostToDevice, m->st));
  WIS_HIP_CHECK(hipMemcpyAsync(m->rm.lslot, h->lslot, n * 4, hipMemcpyHostToDevice, m->st));
  // the pinned staging area is reused by the next upload: make sure the copies are done (wis_generate uploads once per call and
  // drains its stream before it returns or re-enters, so it does not wait here)
  if (wait) WIS_HIP_CHECK(hipStreamSynchronize(m->st));
  return WIS_OK;
}

int check_batch(wis_model* m, int B, int beam) {
  if (B < 1 || B > m->cfg.max_batch) { set_error("batch %d outside [1, max_batch=%d]", B, m->cfg.max_batch); return WIS_E_STATE; }
  if (beam < 1 || beam > m->cfg.max_beam || beam > MAX_R) { set_error("beam_size %d outside [1, %d]", beam, m->cfg.max_beam < MAX_R ? m->cfg.max_beam : MAX_R); return WIS_E_STATE; }
  if (B * beam > MAX_ROWS) { set_error("B*beam = %d exceeds %d decoder rows per device batch", B * beam, MAX_ROWS); return WIS_E_STATE; }
  return WIS_OK;
}

// n rows at one position, row r in KV slot r of its own (R = 1 rows of n utterances; the tuning taps' B * beam rows of token 100)
int single_row_setup(wis_model* m, int n, const std::vector<int>& tok, int pos) {
  std::vector<int> ps(n, pos), slot(n), ls(n);
  for (int r = 0; r < n; ++r) { slot[r] = r; ls[r] = r; }
  return upload_rows(m, tok, ps, slot, ls);
}

std::atomic<int> g_active_calls[64];      // compute calls running per device, every handle and entry point (model.hpp BusyGuard); read by front_half's stream choice (generate.hip)


// The validator of a flat token trie (include/wis_hip.h has the layout and its rules).  EVERYTHING is checked here, on the host, before a byte
// reaches the device: the records are walked in index order with one running cursor - a node's children must start exactly where the previous
// node's ended - so every record but the root is the child of exactly one earlier record, no range leaves the table and no walk can cycle.
int validate_token_trie(const char* who, const int32_t* trie, int n, int n_vocab, int eot, const unsigned char* tok_flags, int* deepest_out) {
  if (n > PHRASE_MAX_RECORDS) { set_error("%s: %d records (at most %d)", who, n, PHRASE_MAX_RECORDS); return WIS_E_UNSUPPORTED; }
  auto bad = [who](const char* what, int i) { set_error("%s: record %d: %s", who, i, what); return WIS_E_ARG; };
  std::vector<int> depth((size_t)n, 0);
  int cursor = 1, deepest = 0;
  for (int i = 0; i < n; ++i) {
    const int32_t tok = trie[4 * i], first = trie[4 * i + 1], nc = trie[4 * i + 2], ends = trie[4 * i + 3];
    if (i >= cursor) return bad("not the child of an earlier record (tree order)", i);
    if (ends != 0 && ends != 1) return bad("the phrase-end flag is 0 or 1", i);
    if (i == 0) {
      if (tok != -1 || ends != 0 || nc < 1) return bad("the root's pseudo-edge is {-1, 1, children >= 1, 0}", i);
    } else {
      if (tok < 0 || tok >= eot || tok >= n_vocab) return bad("the token is no text token (0 <= id < <|endoftext|>)", i);
      if (tok_flags && (tok_flags[tok] & 1)) return bad("the token is in the model's suppress_ids", i);
      if (tok_flags && depth[i] == 1 && (tok_flags[tok] & 2)) return bad("a phrase's first token is in the model's suppress_ids_begin", i);
    }
    if (nc < 0) return bad("a negative number of children", i);
    if (nc > PHRASE_MAX_CHILDREN) { set_error("%s: record %d: %d children (at most %d per node)", who, i, nc, PHRASE_MAX_CHILDREN); return WIS_E_UNSUPPORTED; }
    if (nc == 0) {
      if (first != 0) return bad("a leaf's first-child index is 0", i);
      if (!ends) return bad("a leaf that ends no phrase", i);
      continue;
    }
    if (first != cursor || nc > n - cursor) return bad("the children do not follow the previous node's (tree order), or leave the table", i);
    if (depth[i] + 1 > PHRASE_MAX_DEPTH) { set_error("%s: record %d: a phrase of more than %d tokens", who, i, PHRASE_MAX_DEPTH); return WIS_E_UNSUPPORTED; }
    for (int k = 0; k < nc; ++k) {
      depth[cursor + k] = depth[i] + 1;
      if (k > 0 && trie[4 * (cursor + k)] <= trie[4 * (cursor + k - 1)]) return bad("children not in strictly ascending token order", cursor + k);
    }
    deepest = std::max(deepest, depth[i] + 1);
    cursor += nc;
  }
  if (cursor != n) { set_error("%s: %d records, the tree holds %d", who, n, cursor); return WIS_E_ARG; }
  if (deepest_out) *deepest_out = deepest;
  return WIS_OK;
}
}  // namespace wis

// =======================================================================================
extern "C" {

int wis_version(void) { return WIS_ABI_VERSION; }
const char* wis_last_error(void) { return get_error(); }
int wis_device_count(void) { int n = 0; if (hipGetDeviceCount(&n) != hipSuccess) return 0; return n; }
int wis_supported_compute_types(int device, char* out, size_t cap) {
  (void)device;
  const char* s = "float16,float32,int8_float16";
  if (!out || cap < strlen(s) + 1) { set_error("buffer too small"); return WIS_E_ARG; }
  strcpy(out, s); return WIS_OK;
}

int wis_model_create(const wis_config_t* cfg, const void* arena, size_t arena_bytes, int arena_on_device,
                     const wis_tensor_t* tensors, int n_tensors, int device, wis_model_t** out) {
  if (!cfg || !arena || !tensors || !out || n_tensors <= 0) { set_error("wis_model_create: bad argument"); return WIS_E_ARG; }
  if (cfg->d_model % 128 || cfg->d_model != cfg->n_heads * 64 || cfg->d_model > 2048 || !mel_bins_supported(cfg->n_mels) || cfg->n_enc_layers < 1 || cfg->n_dec_layers < 1 || cfg->n_audio_ctx != 1500 ||
      cfg->n_text_ctx > 512 || cfg->max_batch < 1 || cfg->max_beam < 1 || cfg->max_beam > MAX_R || cfg->n_vocab < 1024) {
    set_error("wis_model_create: unsupported config (d_model %% 128, head_dim 64, n_mels 80 or 128, n_audio_ctx 1500, max_beam <= %d)", MAX_R);
    return WIS_E_UNSUPPORTED;
  }
  DeviceCtx* ctx; WIS_RET(get_ctx(device, &ctx));
  wis_model* m = new wis_model();
  m->cfg = *cfg; m->device = device; m->ctx = ctx;
  m->w8 = cfg->decoder_weight_bits == 8;
  m->cq_fold = !m->w8 && getenv("WIS_NO_CQFOLD") == nullptr;     // (8-bit weights keep the two-stage form: the fold would change what is quantised)
  m->use_graph = getenv("WIS_NO_GRAPH") == nullptr;
  memset(&m->timing, 0, sizeof(m->timing));
  int rc = WIS_OK;
  void* d_arena = nullptr;
  do {
    if (hipStreamCreateWithFlags(&m->st, hipStreamNonBlocking) != hipSuccess) { set_error("stream create failed"); rc = WIS_E_HIP; break; }
    const char* base = reinterpret_cast<const char*>(arena);
    if (!arena_on_device) {
      if (hipMalloc(&d_arena, arena_bytes) != hipSuccess) { set_error("hipMalloc(arena %zu) failed", arena_bytes); rc = WIS_E_NOMEM; break; }
      if (hipMemcpy(d_arena, arena, arena_bytes, hipMemcpyHostToDevice) != hipSuccess) { set_error("arena upload failed"); rc = WIS_E_HIP; break; }
      base = reinterpret_cast<const char*>(d_arena);
    }
    Loader L{tensors, n_tensors, base, arena_bytes};
    if ((rc = load_weights(m, L))) break;
    // logits processors as additive masks (0 / -inf) over the padded vocabulary
    {
      std::vector<float> ba(m->n_vocab_pad, 0.f), bb(m->n_vocab_pad, 0.f);
      for (int i = 0; i < cfg->n_suppress; ++i) if (cfg->suppress_ids[i] >= 0 && cfg->suppress_ids[i] < cfg->n_vocab) ba[cfg->suppress_ids[i]] = -INFINITY;
      for (int i = 0; i < cfg->n_suppress_begin; ++i) if (cfg->suppress_ids_begin[i] >= 0 && cfg->suppress_ids_begin[i] < cfg->n_vocab) bb[cfg->suppress_ids_begin[i]] = -INFINITY;
      if ((rc = dalloc(m, &m->bias_all, ba.size())) || (rc = dalloc(m, &m->bias_begin, bb.size()))) break;
      hipMemcpy(m->bias_all, ba.data(), ba.size() * 4, hipMemcpyHostToDevice);
      hipMemcpy(m->bias_begin, bb.data(), bb.size() * 4, hipMemcpyHostToDevice);
      if ((rc = dalloc(m, &m->d_lang_ids, (size_t)(cfg->n_lang > 0 ? cfg->n_lang : 1)))) break;
      if (cfg->n_lang > 0) hipMemcpy(m->d_lang_ids, cfg->lang_ids, (size_t)cfg->n_lang * 4, hipMemcpyHostToDevice);
    }
    m->tok_flags.assign((size_t)cfg->n_vocab, 0);      // (what wis_model_set_phrases validates a set against)
    for (int i = 0; i < cfg->n_suppress; ++i) if (cfg->suppress_ids[i] >= 0 && cfg->suppress_ids[i] < cfg->n_vocab) m->tok_flags[cfg->suppress_ids[i]] |= 1;
    for (int i = 0; i < cfg->n_suppress_begin; ++i) if (cfg->suppress_ids_begin[i] >= 0 && cfg->suppress_ids_begin[i] < cfg->n_vocab) m->tok_flags[cfg->suppress_ids_begin[i]] |= 2;
    m->cfg.suppress_ids = nullptr; m->cfg.suppress_ids_begin = nullptr; m->cfg.lang_ids = nullptr;   // caller-owned memory is not retained
    // everything carved so far is the (read-only) weight set: it moves into a shareable block; the buffers start on fresh slabs
    m->wslabs = std::make_shared<WeightSlabs>();
    m->wslabs->device = device; m->wslabs->slabs.swap(m->allocs); m->wslabs->bytes = m->bytes;
    m->slab_cur = nullptr; m->slab_left = 0;
    if ((rc = alloc_buffers(m))) break;
    if (hipStreamSynchronize(m->st) != hipSuccess) { set_error("model init failed"); rc = WIS_E_HIP; break; }
  } while (0);
  if (d_arena) hipFree(d_arena);
  if (rc) { wis_model_destroy(m); return rc; }
  *out = m;
  return WIS_OK;
}

void wis_model_destroy(wis_model_t* m) {
  if (!m) return;
  hipSetDevice(m->device);
  if (m->st) hipStreamSynchronize(m->st);
  spin_collect(m->device);      // (a deferred spin claim of this handle waits on one of its events: completed by the synchronise above)
  for (auto& kv : m->graphs) hipGraphExecDestroy(kv.second);
  for (void* p : m->allocs) hipFree(p);
  if (m->h_pin) hipHostFree(m->h_pin);
  if (m->h_prog) hipHostFree(m->h_prog);
  for (int i = 0; i < 8; ++i) if (m->ev[i]) hipEventDestroy(m->ev[i]);
  for (hipEvent_t e : m->al.ev) if (e) hipEventDestroy(e);
  if (m->st_enc) { hipStreamSynchronize(m->st_enc); hipStreamDestroy(m->st_enc); }
  if (m->ev_enc) hipEventDestroy(m->ev_enc);
  if (m->ev_ckv) hipEventDestroy(m->ev_ckv);
  if (m->st) hipStreamDestroy(m->st);
  delete m;
}
size_t wis_model_device_bytes(const wis_model_t* m) { return m ? m->bytes : 0; }

int wis_model_clone(wis_model_t* parent, wis_model_t** out) {
  if (!parent || !out || !parent->wslabs) { set_error("wis_model_clone: bad argument"); return WIS_E_ARG; }
  WIS_HIP_CHECK(hipSetDevice(parent->device));
  wis_model* m = new wis_model();
  m->cfg = parent->cfg; m->device = parent->device; m->ctx = parent->ctx;
  m->wslabs = parent->wslabs;
  // the weight set (device pointers into the shared slabs)
  m->w_conv1 = parent->w_conv1; m->w_conv2 = parent->w_conv2; m->b_conv1 = parent->b_conv1; m->b_conv2 = parent->b_conv2;
  m->enc_pos = parent->enc_pos; m->enc_ln_g = parent->enc_ln_g; m->enc_ln_b = parent->enc_ln_b;
  m->enc = parent->enc; m->dec = parent->dec;
  m->emb = parent->emb; m->dec_pos = parent->dec_pos; m->proj = parent->proj; m->dec_ln_g = parent->dec_ln_g; m->dec_ln_b = parent->dec_ln_b;
  m->bias_all = parent->bias_all; m->bias_begin = parent->bias_begin; m->d_lang_ids = parent->d_lang_ids; m->n_vocab_pad = parent->n_vocab_pad;
  m->w_ckv_all = parent->w_ckv_all; m->b_ckv_all = parent->b_ckv_all;
  m->w8 = parent->w8; m->cq_fold = parent->cq_fold;
  m->use_graph = parent->use_graph;
  m->al.heads = parent->al.heads;      // (the clone allocates its own align scratch on its first wis_align)
  m->tok_flags = parent->tok_flags;      // (a clone has a phrase buffer of its own and starts without a set)
  memset(&m->timing, 0, sizeof(m->timing));
  int rc = WIS_OK;
  do {
    if (hipStreamCreateWithFlags(&m->st, hipStreamNonBlocking) != hipSuccess) { set_error("stream create failed"); rc = WIS_E_HIP; break; }
    if ((rc = alloc_buffers(m))) break;
    if (hipStreamSynchronize(m->st) != hipSuccess) { set_error("clone init failed"); rc = WIS_E_HIP; break; }
  } while (0);
  if (rc) { wis_model_destroy(m); return rc; }
  *out = m;
  return WIS_OK;
}

int wis_last_no_speech_prob(wis_model_t* m, int B, float* out) {
  if (!m || !out || B < 1) { set_error("wis_last_no_speech_prob: bad argument"); return WIS_E_ARG; }
  WIS_ENTER(m, "wis_last_no_speech_prob")
  if (m->nsp_B == 0) { set_error("wis_last_no_speech_prob: the last wis_generate on this handle did not ask for no_speech_prob"); return WIS_E_STATE; }
  if (B > m->nsp_B) { set_error("wis_last_no_speech_prob: %d utterances asked, the last call had %d", B, m->nsp_B); return WIS_E_ARG; }
  WIS_HIP_CHECK(hipSetDevice(m->device));
  WIS_HIP_CHECK(hipMemcpyAsync(out, m->d_nsp, (size_t)B * 4, hipMemcpyDeviceToHost, m->st));
  WIS_HIP_CHECK(hipStreamSynchronize(m->st));
  return WIS_OK;
}

int wis_last_phrase_mass(wis_model_t* m, int B, int n, float* out) {
  if (!m || !out || B < 1 || n < 1) { set_error("wis_last_phrase_mass: bad argument"); return WIS_E_ARG; }
  WIS_ENTER(m, "wis_last_phrase_mass")
  if (m->phr_mass_B == 0) { set_error("wis_last_phrase_mass: the last search on this handle did not set phrase_mass"); return WIS_E_STATE; }
  if (B > m->phr_mass_B || n != m->phr_mass_n) { set_error("wis_last_phrase_mass: %d utterances x %d results asked, the last call had %d x %d", B, n, m->phr_mass_B, m->phr_mass_n); return WIS_E_ARG; }
  WIS_HIP_CHECK(hipSetDevice(m->device));
  WIS_HIP_CHECK(hipMemcpyAsync(out, m->d_phr_mass, (size_t)B * n * 4, hipMemcpyDeviceToHost, m->st));
  WIS_HIP_CHECK(hipStreamSynchronize(m->st));
  return WIS_OK;
}

int wis_last_trajectory(wis_model_t* m, int b, int32_t* tok, int32_t* org, int cap_steps, int32_t* n_steps) {
  if (!m || !tok || !org || !n_steps || cap_steps < 0) { set_error("wis_last_trajectory: bad argument"); return WIS_E_ARG; }
  WIS_ENTER(m, "wis_last_trajectory")
  WIS_HIP_CHECK(hipSetDevice(m->device));
  if (m->last_ragged) { set_error("wis_last_trajectory: the last call's prompts differed in length (wis_generate_ragged): its rows do not line up with a drafted call's"); return WIS_E_STATE; }
  if (b < 0 || b >= m->last_B) { set_error("wis_last_trajectory: utterance %d outside the last call's batch of %d", b, m->last_B); return WIS_E_ARG; }
  const int k = m->last_beam;
  int n = 0;
  WIS_HIP_CHECK(hipMemcpyAsync(&n, m->bs.step_u + b, 4, hipMemcpyDeviceToHost, m->st));
  WIS_HIP_CHECK(hipStreamSynchronize(m->st));
  if (n < 0 || n > MAX_STEPS) { set_error("wis_last_trajectory: step counter %d out of range", n); return WIS_E_STATE; }
  if (n > cap_steps) n = cap_steps;
  std::vector<int> raw((size_t)n * MAX_R * 2);
  if (n) WIS_HIP_CHECK(hipMemcpy(raw.data(), m->bs.traj + (size_t)b * MAX_STEPS * MAX_R * 2, raw.size() * 4, hipMemcpyDeviceToHost));
  for (int s = 0; s < n; ++s) for (int j = 0; j < k; ++j) { tok[s * k + j] = raw[((size_t)s * MAX_R + j) * 2]; org[s * k + j] = raw[((size_t)s * MAX_R + j) * 2 + 1]; }
  *n_steps = n;
  return WIS_OK;
}

// Installs a phrase set: validated on the host (validate_token_trie), then one copy into the handle's buffer.
int wis_model_set_phrases(wis_model_t* m, const int32_t* trie, int n_records) {
  if (!m || n_records < 0 || (n_records > 0 && !trie)) { set_error("wis_model_set_phrases: bad argument"); return WIS_E_ARG; }
  WIS_ENTER(m, "wis_model_set_phrases")
  if (n_records == 0) { m->phr_n = 0; m->phr_depth = 0; return WIS_OK; }
  const int n = n_records;
  int deepest = 0;
  WIS_RET(validate_token_trie("wis_model_set_phrases", trie, n, m->cfg.n_vocab, m->cfg.eot, m->tok_flags.data(), &deepest));
  WIS_HIP_CHECK(hipSetDevice(m->device));
  m->phr_n = 0;      // (a failed copy leaves no set behind)
  WIS_HIP_CHECK(hipMemcpyAsync(m->d_trie, trie, (size_t)n * 16, hipMemcpyHostToDevice, m->st));      // behind whatever step of an earlier call is still queued
  WIS_HIP_CHECK(hipStreamSynchronize(m->st));
  m->phr_n = n; m->phr_depth = deepest;
  return WIS_OK;
}

// ... and a hotword set (THE HOTWORD RULE): the same table, the same validator, a buffer of its own - neither set disturbs the other
int wis_model_set_hotwords(wis_model_t* m, const int32_t* trie, int n_records) {
  if (!m || n_records < 0 || (n_records > 0 && !trie)) { set_error("wis_model_set_hotwords: bad argument"); return WIS_E_ARG; }
  WIS_ENTER(m, "wis_model_set_hotwords")
  if (n_records == 0) { m->hot_n = 0; return WIS_OK; }
  const int n = n_records;
  WIS_RET(validate_token_trie("wis_model_set_hotwords", trie, n, m->cfg.n_vocab, m->cfg.eot, m->tok_flags.data(), nullptr));
  WIS_HIP_CHECK(hipSetDevice(m->device));
  m->hot_n = 0;      // (a failed copy leaves no set behind)
  WIS_HIP_CHECK(hipMemcpyAsync(m->d_hot, trie, (size_t)n * 16, hipMemcpyHostToDevice, m->st));      // behind whatever step of an earlier call is still queued
  WIS_HIP_CHECK(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(m->d_hot_ctl + 1), n, 1, m->st));      // (the record count the kernel checks its ranges against)
  WIS_HIP_CHECK(hipStreamSynchronize(m->st));
  m->hot_n = n;
  return WIS_OK;
}

int wis_debug_sa_long(wis_model_t* m, int form) {
  if (!m || form < -1 || form > 1) { set_error("wis_debug_sa_long: bad argument"); return WIS_E_ARG; }
  WIS_ENTER(m, "wis_debug_sa_long")
  m->sa_long_form = form;
  return WIS_OK;
}
int wis_debug_graph_count(wis_model_t* m, int* count) {
  if (!m || !count) { set_error("wis_debug_graph_count: bad argument"); return WIS_E_ARG; }
  WIS_ENTER(m, "wis_debug_graph_count")
  *count = (int)m->graphs.size();
  return WIS_OK;
}
int wis_debug_handoff(wis_model_t* m, int raise_flag, int* retries, int* spin_disabled) {
  if (!m) { set_error("wis_debug_handoff: bad argument"); return WIS_E_ARG; }
  WIS_ENTER(m, "wis_debug_handoff")
  WIS_HIP_CHECK(hipSetDevice(m->device));
  if (raise_flag) {      // what a combiner does when its bounded spin runs out
    const unsigned one = 1u;
    WIS_HIP_CHECK(hipMemcpyAsync(m->ca_epoch, &one, 4, hipMemcpyHostToDevice, m->st));
    WIS_HIP_CHECK(hipStreamSynchronize(m->st));
  }
  if (retries) *retries = m->handoff_retries;
  if (spin_disabled) *spin_disabled = m->spin_off ? 1 : 0;
  return WIS_OK;
}

int wis_last_timing(const wis_model_t* m, wis_timing_t* t) {
  if (!m || !t) { set_error("wis_last_timing: bad argument"); return WIS_E_ARG; }
  *t = m->timing; return WIS_OK;
}

int wis_detect_language(wis_model_t* m, const float* input, int input_kind, int B, float* lang_probs) {
  if (!m || !input || !lang_probs) { set_error("wis_detect_language: bad argument"); return WIS_E_ARG; }
  if (m->cfg.n_lang <= 0) { set_error("model has no lang_ids"); return WIS_E_UNSUPPORTED; }
  WIS_ENTER(m, "wis_detect_language")
  WIS_HIP_CHECK(hipSetDevice(m->device));
  WIS_RET(check_batch(m, B, 1));
  WIS_RET(run_front(m, input, input_kind, B));
  std::vector<int> tok(B, m->cfg.sot);
  for (int attempt = 0; attempt < 2; ++attempt) {
    SpinClaim claim(m, B);
    WIS_RET(single_row_setup(m, B, tok, 0));
    WIS_RET(dec_forward(m, B, 1, B, true, 1, 0));
    WIS_RET(launch_lang_probs(m->st, m->logits, m->n_vocab_pad, m->d_lang_ids, m->cfg.n_lang, m->d_probs, B));
    WIS_HIP_CHECK(hipMemcpyAsync(lang_probs, m->d_probs, (size_t)B * m->cfg.n_lang * 4, hipMemcpyDeviceToHost, m->st));
    bool gave_up = false;
    WIS_RET(spin_gave_up(m, &gave_up));      // (synchronises the stream)
    if (!gave_up) break;
  }
  return WIS_OK;
}

// the encoder alone, its output left in a block of the caller's (include/wis_hip.h): what the WIS_IN_ENC_* kinds of the other entry points take back
int wis_encode(wis_model_t* m, const float* input, int input_kind, int B, void* enc_out_dev_f16, float* enc_out_host_or_null) {
  if (!m) { set_error("wis_encode: the model handle is null"); return WIS_E_ARG; }
  if (!input) { set_error("wis_encode: input is null"); return WIS_E_ARG; }
  if (!enc_out_dev_f16) { set_error("wis_encode: enc_out_dev_f16 is null (the caller provides the device block)"); return WIS_E_ARG; }
  if (input_is_encoded(input_kind)) { set_error("wis_encode: input_kind %d is encoder output already (WIS_IN_MEL_* / WIS_IN_PCM_* are encoded)", input_kind); return WIS_E_UNSUPPORTED; }
  if (input_kind < WIS_IN_MEL_HOST || input_kind > WIS_IN_PCM_DEV) { set_error("wis_encode: bad input_kind %d", input_kind); return WIS_E_ARG; }
  if (B < 1 || B > m->cfg.max_batch) { set_error("wis_encode: B = %d outside [1, max_batch=%d]", B, m->cfg.max_batch); return WIS_E_ARG; }
  WIS_ENTER(m, "wis_encode")
  WIS_HIP_CHECK(hipSetDevice(m->device));
  WIS_RET(stage_input(m, input, input_kind, B));
  WIS_RET(run_encoder(m, B));
  const int64_t n = (int64_t)B * m->cfg.n_audio_ctx * m->cfg.d_model;
  WIS_HIP_CHECK(hipMemcpyAsync(enc_out_dev_f16, m->mem, (size_t)n * 2, hipMemcpyDeviceToDevice, m->st));
  if (enc_out_host_or_null) {
    launch_f16_to_f32(m->st, m->mem, m->x, n);   // x is free after the encoder
    WIS_HIP_CHECK(hipMemcpyAsync(enc_out_host_or_null, m->x, (size_t)n * 4, hipMemcpyDeviceToHost, m->st));
  }
  WIS_HIP_CHECK(hipStreamSynchronize(m->st));
  return WIS_OK;
}

}  // extern "C"
