// cross_q8.hip — the int8 cross-attention K/V (wis_model_ext_t::cross_kv_bits = 8; include/wis_hip.h states the rule): the kernel that turns the f16
// images the cross K/V projection writes into int8 images + per-key scales, and the decode step's cross-attention kernel that reads them.
//
// Images of one decoder layer (B utterances, H heads, T keys, Tpad = T rounded up to 64; every 16-byte piece is what ONE lane of the consumer asks for):
//   kq  i8  [B][H][4][Tpad][16]   cell (j, t) = K[t][8 j .. 8 j + 7] followed by K[t][32 + 8 j .. 32 + 8 j + 7]: BOTH k-steps of the score MFMA's A
//                                 fragment of lane (key t, k-quarter j) - one request where the f16 image [B][H][8][T][8] takes two
//   vq  i8  [B][H][64][Tpad]      row dh; byte 64 g + 16 j + 8 e + i = V[64 g + 32 e + 8 j + i][dh]: the A fragments of lane (dh, k-quarter j) for the TWO
//                                 32-key P.V steps 2 g + e of a 64-key group - one request where the f16 image [B][H][64][Tpad] takes two
//   sk, sv  f32 [B][H][Tpad]      the scale of key t's 64 K values / of its 64 V values
// Keys [T, Tpad) hold int8 zeros and scale 1 in all four.
#include "common.hpp"
#include "kernels.hpp"
#include "ca_query.hpp"

namespace wis {

// one value by the rule (enc_kernels.hip quant_rows_kernel's expression); inv = 1 / scale
__device__ __forceinline__ unsigned q8_byte(float v, float inv) { return (unsigned)((int)fminf(fmaxf(rintf(v * inv), -127.f), 127.f) & 255); }
__device__ __forceinline__ unsigned q8_pack4(f16 a, f16 b, f16 c, f16 d, float ia, float ib, float ic, float id) {
  return q8_byte((float)a, ia) | (q8_byte((float)b, ib) << 8) | (q8_byte((float)c, ic) << 16) | (q8_byte((float)d, id) << 24);
}
// all-reduce over the four 16-lane rows of a lane column (lanes l, l + 16, l + 32, l + 48) with gfx950's row-swap moves (dec_cross_attn_rs_kernel's form)
__device__ __forceinline__ float q8_xrow_max(float v) {
  const auto a = __builtin_amdgcn_permlane32_swap(__float_as_uint(v), __float_as_uint(v), false, false);
  const float m = fmaxf(__uint_as_float(a[0]), __uint_as_float(a[1]));
  const auto b = __builtin_amdgcn_permlane16_swap(__float_as_uint(m), __float_as_uint(m), false, false);
  return fmaxf(__uint_as_float(b[0]), __uint_as_float(b[1]));
}
__device__ __forceinline__ float q8_xrow_sum(float v) {      // (both lanes of a pair add the same two operands in the same order: every lane of the column holds the same bits)
  const auto a = __builtin_amdgcn_permlane32_swap(__float_as_uint(v), __float_as_uint(v), false, false);
  const float m = __uint_as_float(a[0]) + __uint_as_float(a[1]);
  const auto b = __builtin_amdgcn_permlane16_swap(__float_as_uint(m), __float_as_uint(m), false, false);
  return __uint_as_float(b[0]) + __uint_as_float(b[1]);
}

// =======================================================================================
// f16 images -> int8 images + scales, for G layers in one launch.  grid (Tpad / 64, B H, G), block 256: a workgroup owns 64 keys of one (layer,
// utterance, head), both K and V.  Every request of the workgroup - 2 x 16 bytes of K and 2 x 16 bytes of V^T per thread - goes out first.
//   K   lane (key = 16 wave + l15, quarter j) reads cells j and j + 4 of its key (8 values each; along t the 16 lanes of a row read 256 contiguous bytes),
//       the key's absmax is an all-reduce over the four lane rows, and the lane writes its own 16-byte output cell: no LDS.
//   V   a key's 64 values lie down a COLUMN of V^T [64][Tpad], so the 64 x 64 tile is read along t in 16-byte pieces, kept in LDS, reduced per key
//       by four threads (16 head dimensions each), and written back ALONG t: thread (dh, quarter j) quantises the 16 keys of its output piece, each
//       with its own scale.  Reads and writes of both images are 16 bytes wide.
// Keys >= T are taken as zeros whatever the input holds there: zero values, scale 1.
constexpr int Q8_TP = 72;      // f16 pitch of the V tile's rows: 16-byte aligned, rows four banks apart
__global__ __launch_bounds__(256) void cross_kv_quant_kernel(const f16* __restrict__ kx, const f16* __restrict__ vt, int8_t* __restrict__ kq, int8_t* __restrict__ vq,
                                                             float* __restrict__ sk, float* __restrict__ sv, int H, int T, int Tpad, int64_t kx_ls, int64_t vt_ls,
                                                             int64_t kq_ls, int64_t vq_ls, int64_t s_ls) {
  __shared__ __attribute__((aligned(16))) f16 tile[64 * Q8_TP];
  __shared__ float smx[4][64];
  __shared__ float sinv[64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l15 = lane & 15, j = lane >> 4;
  const int t0 = 64 * blockIdx.x, bh = blockIdx.y, l = blockIdx.z;
  // ---- requests
  const int t = t0 + 16 * wave + l15, tc = t < T ? t : T - 1;
  const f16* kb = kx + l * kx_ls + (size_t)bh * 64 * T;
  f16x8 ka = *reinterpret_cast<const f16x8*>(kb + ((size_t)j * T + tc) * 8), kc = *reinterpret_cast<const f16x8*>(kb + ((size_t)(j + 4) * T + tc) * 8);
  const f16* vb = vt + l * vt_ls + (size_t)bh * 64 * Tpad + t0;
  const int vr = tid >> 3, vp = tid & 7;      // piece vp (8 keys) of rows vr and vr + 32
  f16x8 v0 = *reinterpret_cast<const f16x8*>(vb + (size_t)vr * Tpad + 8 * vp), v1 = *reinterpret_cast<const f16x8*>(vb + (size_t)(vr + 32) * Tpad + 8 * vp);
  const f16x8 zero8 = {0, 0, 0, 0, 0, 0, 0, 0};
  // ---- K
  if (t >= T) { ka = zero8; kc = zero8; }
  float mx = 0.f;
#pragma unroll
  for (int i = 0; i < 8; ++i) mx = fmaxf(mx, fmaxf(fabsf((float)ka[i]), fabsf((float)kc[i])));
  mx = q8_xrow_max(mx);
  {
    const float sc = mx > 0.f ? mx / 127.0f : 1.0f, inv = 1.0f / sc;
    const u32x4 o = {q8_pack4(ka[0], ka[1], ka[2], ka[3], inv, inv, inv, inv), q8_pack4(ka[4], ka[5], ka[6], ka[7], inv, inv, inv, inv),
                     q8_pack4(kc[0], kc[1], kc[2], kc[3], inv, inv, inv, inv), q8_pack4(kc[4], kc[5], kc[6], kc[7], inv, inv, inv, inv)};
    *reinterpret_cast<u32x4*>(kq + l * kq_ls + (((size_t)bh * 4 + j) * Tpad + t) * 16) = o;      // t < Tpad: the grid covers exactly Tpad keys
    if (j == 0) sk[l * s_ls + (size_t)bh * Tpad + t] = sc;
  }
  // ---- V
#pragma unroll
  for (int i = 0; i < 8; ++i) if (t0 + 8 * vp + i >= T) { v0[i] = 0; v1[i] = 0; }
  *reinterpret_cast<f16x8*>(&tile[vr * Q8_TP + 8 * vp]) = v0;
  *reinterpret_cast<f16x8*>(&tile[(vr + 32) * Q8_TP + 8 * vp]) = v1;
  __syncthreads();
  {
    float m = 0.f;
#pragma unroll
    for (int i = 0; i < 16; ++i) m = fmaxf(m, fabsf((float)tile[(16 * wave + i) * Q8_TP + lane]));      // thread (key = lane, dh 16 wave ..)
    smx[wave][lane] = m;
  }
  __syncthreads();
  if (tid < 64) {
    const float m = fmaxf(fmaxf(smx[0][tid], smx[1][tid]), fmaxf(smx[2][tid], smx[3][tid]));
    const float sc = m > 0.f ? m / 127.0f : 1.0f;
    sinv[tid] = 1.0f / sc;
    sv[l * s_ls + (size_t)bh * Tpad + t0 + tid] = sc;
  }
  __syncthreads();
  {
    const int dh = tid >> 2, jj = tid & 3;      // output piece: keys 8 jj .. + 7 and 32 + 8 jj .. + 7 of the group
    const f16x8 a = *reinterpret_cast<const f16x8*>(&tile[dh * Q8_TP + 8 * jj]), c = *reinterpret_cast<const f16x8*>(&tile[dh * Q8_TP + 32 + 8 * jj]);
    const float* ia = &sinv[8 * jj]; const float* ic = &sinv[32 + 8 * jj];
    const u32x4 o = {q8_pack4(a[0], a[1], a[2], a[3], ia[0], ia[1], ia[2], ia[3]), q8_pack4(a[4], a[5], a[6], a[7], ia[4], ia[5], ia[6], ia[7]),
                     q8_pack4(c[0], c[1], c[2], c[3], ic[0], ic[1], ic[2], ic[3]), q8_pack4(c[4], c[5], c[6], c[7], ic[4], ic[5], ic[6], ic[7])};
    *reinterpret_cast<u32x4*>(vq + l * vq_ls + ((size_t)bh * 64 + dh) * Tpad + t0 + 16 * jj) = o;
  }
}

int launch_cross_kv_quant(hipStream_t st, const f16* kx, const f16* vt, int B, int H, int T, int Tpad, int L, int64_t kx_ls, int64_t vt_ls,
                          int8_t* kq, int8_t* vq, float* sk, float* sv, int64_t kq_ls, int64_t vq_ls, int64_t s_ls) {
  if (!kx || !vt || !kq || !vq || !sk || !sv || B < 1 || H < 1 || T < 1 || L < 1 || Tpad < T || Tpad % 64 || (int64_t)B * H > 65535 || L > 65535) {
    set_error("cross_kv_quant: B=%d H=%d T=%d Tpad=%d L=%d unsupported (Tpad %% 64, Tpad >= T)", B, H, T, Tpad, L); return WIS_E_ARG; }
  const int64_t img = (int64_t)B * H * 64 * Tpad;
  if (kx_ls % 8 || vt_ls % 8 || kq_ls % 16 || vq_ls % 16 || kx_ls < (int64_t)B * H * 64 * T || vt_ls < img || kq_ls < img || vq_ls < img || s_ls < (int64_t)B * H * Tpad) {
    set_error("cross_kv_quant: layer strides %lld / %lld / %lld / %lld / %lld too short or not 16-byte multiples", (long long)kx_ls, (long long)vt_ls, (long long)kq_ls,
              (long long)vq_ls, (long long)s_ls); return WIS_E_ARG; }
  hipLaunchKernelGGL(cross_kv_quant_kernel, dim3(Tpad / 64, B * H, L), dim3(256), 0, st, kx, vt, kq, vq, sk, sv, H, T, Tpad, kx_ls, vt_ls, kq_ls, vq_ls, s_ls);
  return WIS_OK;
}

// =======================================================================================
// The cross-K/V projection that writes the int8 images itself: C = mem [B T][d] . W [L 2d][d]^T over ALL decoder layers in one launch, and an epilogue that
// sees whole (key, head) rows.  Block 256 = 4 waves as 2 (key halves) x 2 (heads); a workgroup owns 128 keys of ONE utterance x 128 columns = two heads.
//   Rows go by (utterance, 128-key block), not by flat M: a wave's 64 keys are one 64-key group of the V image; keys >= T read row T - 1 and leave as zeros
//   with scale 1 (the quantiser's rule), a wave whose 64 keys start at Tpad or beyond has nothing to write.
//   Columns go by head: head column hc = n / 64 of the concatenated weight rows is (layer hc / 2H, K head hc % 2H < H, else V head hc % 2H - H), so the tile
//   may straddle K | V or two layers - every wave has ONE head and picks its epilogue by it (wave-uniform).
// k-loop: gemm_f16_kernel's 128 x 128 form (register staging, two LDS buffers, one barrier per k-tile, two workgroups per CU), byte-addressed: a staged row
// is 128 bytes of k - 64 f16 or 128 int8 - at a 144-byte pitch (conflict-free ds_read_b128), so one loader serves both operand widths; a k-tile that ends
// beyond the row (int8, d = 64) is zero filled.  MODE names the accumulator chain:
//   CQ_F16_32  v_mfma_f32_32x32x16_f16, 16 k per link, links in k order   = gemm_f16_kernel / gemm_pp_kernel
//   CQ_F16_16  v_mfma_f32_16x16x32_f16, 32 k per link, links in k order   = gemm_8p_kernel
//   CQ_I8      v_mfma_i32_32x32x32_i8 (exact), then (float)acc * (sa[m] * sw[n])  = gemm_i8_kernel
// launch_cross_kv_fused takes the f16 chain launch_gemm_crosskv's kernel runs at the shape (gemm_crosskv_chain), so an output is the same f32 sum.
// Operand order: K waves D[n][m] (weights as MFMA A: a lane holds one key and 4 consecutive head dimensions), V waves D[m][n] (activations as A: a lane
// holds one head dimension and 4 consecutive keys), so BOTH write 8-byte f16 quads into the orientation their image needs.
// Epilogue, per wave and without a workgroup barrier (the k-tile buffers are free behind the loop's last barrier; a wave has 9.5 KB of them to itself):
//   acc (+ scales) + bias in f32 -> f16 -> wave tile [64][72] f16 (144-byte pitch: rows four banks apart; Q8_TP), keys >= T as zeros
//   K  tile [key][dh]: lane (key 16 i + l15, quarter j) reads its two 8-value cells (2 x ds_read_b128), the key's absmax is an all-reduce over the four lane
//      rows (q8_xrow_max: permlane32 / permlane16 swaps), the lane writes its own 16-byte cell of kq - cross_kv_quant_kernel's K half, from LDS
//   V  tile [dh][key] - the transposition happened in the MFMA: lane (key pair, dh half) takes the absmax of 32 head dimensions of two keys (ds_read_b32),
//      one permlane32 swap joins the halves, the inverse scales go through 64 floats of LDS, and lane (dh, quarter j) quantises the 16 keys of its 16-byte
//      piece of vq, each with its own scale - cross_kv_quant_kernel's V half
enum { CQ_F16_32 = 0, CQ_F16_16 = 1, CQ_I8 = 2 };
typedef int i32x4 __attribute__((ext_vector_type(4)));
typedef int i32x16 __attribute__((ext_vector_type(16)));
typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));
constexpr int CQ_RB = 2 * Q8_TP;               // bytes per staged operand row and per epilogue tile row
constexpr int CQ_BUF = 256 * CQ_RB;            // one k-tile: 128 activation rows, then 128 weight rows
constexpr int CQ_WAVE = 64 * CQ_RB + 512;      // a wave's epilogue block: the tile, 64 inverse scales, 64 activation row scales
__device__ __forceinline__ float q8_x32_max(float v) {      // max over the lane pair (l, l + 32)
  const auto a = __builtin_amdgcn_permlane32_swap(__float_as_uint(v), __float_as_uint(v), false, false);
  return fmaxf(__uint_as_float(a[0]), __uint_as_float(a[1]));
}
__device__ __forceinline__ void cq_put(char* tile, int x, int y, float a, float b, float c, float d) {
  const f16x4 o = {(f16)a, (f16)b, (f16)c, (f16)d};
  *reinterpret_cast<f16x4*>(tile + x * CQ_RB + 2 * y) = o;
}
template <int MODE>
__global__ __launch_bounds__(256) void cross_kv_q8_fused_kernel(const char* __restrict__ A, const char* __restrict__ W, int rowbytes, int T, int Tpad, int H, int nkb, int nmt,
                                                                int nnt, const float* __restrict__ sa, const float* __restrict__ sw, const float* __restrict__ bias,
                                                                int8_t* __restrict__ kq, int8_t* __restrict__ vq, float* __restrict__ sk, float* __restrict__ sv,
                                                                int64_t q_ls, int64_t s_ls) {
  constexpr bool I8 = MODE == CQ_I8;
  __shared__ __attribute__((aligned(16))) char smem[2 * CQ_BUF];
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave >> 1, wn = wave & 1, l31 = lane & 31, hi = lane >> 5, l15 = lane & 15, kq4 = lane >> 4;
  // XCD-aware regrouping of the workgroup id, then m-fastest tile coordinates (gemm_f16_kernel)
  const int nwg = nmt * nnt;
  int wg;
  {
    const int orig = blockIdx.x, xcd = orig & 7, q = nwg >> 3, r = nwg & 7;
    wg = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (orig >> 3);
  }
  const int mt = wg % nmt, nt = wg / nmt;
  const int b = mt / nkb, t0 = (mt - b * nkb) * 128, n0 = nt * 128;
  const int hc = 2 * nt + wn, lyr = hc / (2 * H), hw = hc - lyr * 2 * H;
  const bool isV = hw >= H;
  const int h = isV ? hw - H : hw;

  // loader: 16-byte chunk c -> row c >> 3, byte offset (c & 7) * 16; rows lrow + 32 i.  Keys >= T read key T - 1 (their results leave as zeros)
  const int lrow = tid >> 3, lkc = (tid & 7) * 16;
  auto arow = [&](int i) -> const char* {
    int t = t0 + lrow + 32 * i; if (t > T - 1) t = T - 1;
    return A + ((int64_t)b * T + t) * rowbytes;
  };
  const char* ga0 = arow(0); const char* ga1 = arow(1); const char* ga2 = arow(2); const char* ga3 = arow(3);
  const char* gw0 = W + (int64_t)(n0 + lrow) * rowbytes;
  const int64_t wrp = (int64_t)32 * rowbytes;
  const int soff = lrow * CQ_RB + lkc;
  uint4 ra0, ra1, ra2, ra3, rw0, rw1, rw2, rw3;
  const uint4 z4 = make_uint4(0u, 0u, 0u, 0u);
#define WIS_CQ_GLOAD(kt) {                                                                                                          \
    int ko = (kt) * 128 + lkc; const bool past = ko >= rowbytes; if (past) ko = 0;                                                  \
    ra0 = *reinterpret_cast<const uint4*>(ga0 + ko); ra1 = *reinterpret_cast<const uint4*>(ga1 + ko);                               \
    ra2 = *reinterpret_cast<const uint4*>(ga2 + ko); ra3 = *reinterpret_cast<const uint4*>(ga3 + ko);                               \
    rw0 = *reinterpret_cast<const uint4*>(gw0 + ko); rw1 = *reinterpret_cast<const uint4*>(gw0 + wrp + ko);                         \
    rw2 = *reinterpret_cast<const uint4*>(gw0 + 2 * wrp + ko); rw3 = *reinterpret_cast<const uint4*>(gw0 + 3 * wrp + ko);           \
    if (past) { ra0 = z4; ra1 = z4; ra2 = z4; ra3 = z4; rw0 = z4; rw1 = z4; rw2 = z4; rw3 = z4; } }
#define WIS_CQ_SSTORE(buf) {                                                                                                        \
    char* sa_ = smem + (buf) * CQ_BUF + soff; char* sw_ = sa_ + 128 * CQ_RB;                                                        \
    *reinterpret_cast<uint4*>(sa_) = ra0; *reinterpret_cast<uint4*>(sa_ + 32 * CQ_RB) = ra1;                                        \
    *reinterpret_cast<uint4*>(sa_ + 64 * CQ_RB) = ra2; *reinterpret_cast<uint4*>(sa_ + 96 * CQ_RB) = ra3;                           \
    *reinterpret_cast<uint4*>(sw_) = rw0; *reinterpret_cast<uint4*>(sw_ + 32 * CQ_RB) = rw1;                                        \
    *reinterpret_cast<uint4*>(sw_ + 64 * CQ_RB) = rw2; *reinterpret_cast<uint4*>(sw_ + 96 * CQ_RB) = rw3; }

  f32x16 accf[2][2]; i32x16 acci[2][2]; f32x4 acc4[4][4];      // [block of p rows][block of q rows]; one of the three per MODE
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int c = 0; c < 2; ++c)
#pragma unroll
      for (int r = 0; r < 16; ++r) { accf[a][c][r] = 0.f; acci[a][c][r] = 0; }
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int c = 0; c < 4; ++c) acc4[a][c] = f32x4{0.f, 0.f, 0.f, 0.f};

  const int nk = (rowbytes + 127) / 128;
  WIS_CQ_GLOAD(0) WIS_CQ_SSTORE(0)
  __syncthreads();
  for (int kt = 0; kt < nk; ++kt) {
    const int cur = kt & 1;
    if (kt + 1 < nk) WIS_CQ_GLOAD(kt + 1)
    // first MFMA operand p (its rows become the quads a lane holds), second operand q (its rows become the lane's own index): K waves p = weights,
    // q = activations; V waves the other way round - a choice of two LDS base addresses, the loop is the same
    const char* sAb = smem + cur * CQ_BUF + wm * 64 * CQ_RB;
    const char* sWb = smem + cur * CQ_BUF + (128 + wn * 64) * CQ_RB;
    const char* pB = isV ? sAb : sWb;
    const char* qB = isV ? sWb : sAb;
    if constexpr (MODE == CQ_F16_16) {
#pragma unroll
      for (int kb = 0; kb < 2; ++kb) {      // lane (l15, quarter) feeds k 32 kb + 8 quarter .. + 7 of its row to both operands
        f16x8 pf[4], qf[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          pf[i] = *reinterpret_cast<const f16x8*>(pB + (16 * i + l15) * CQ_RB + kb * 64 + kq4 * 16);
          qf[i] = *reinterpret_cast<const f16x8*>(qB + (16 * i + l15) * CQ_RB + kb * 64 + kq4 * 16);
        }
#pragma unroll
        for (int pi = 0; pi < 4; ++pi)
#pragma unroll
          for (int qi = 0; qi < 4; ++qi) acc4[pi][qi] = __builtin_amdgcn_mfma_f32_16x16x32_f16(pf[pi], qf[qi], acc4[pi][qi], 0, 0, 0);
      }
    } else {
#pragma unroll
      for (int kk = 0; kk < 4; ++kk) {      // lane (l31, hi) feeds bytes 32 kk + 16 hi .. + 15 of its row to both operands
        u32x4 pr[2], qr[2];
#pragma unroll
        for (int i = 0; i < 2; ++i) {
          pr[i] = *reinterpret_cast<const u32x4*>(pB + (32 * i + l31) * CQ_RB + kk * 32 + hi * 16);
          qr[i] = *reinterpret_cast<const u32x4*>(qB + (32 * i + l31) * CQ_RB + kk * 32 + hi * 16);
        }
#pragma unroll
        for (int pi = 0; pi < 2; ++pi)
#pragma unroll
          for (int qi = 0; qi < 2; ++qi) {
            if constexpr (I8) acci[pi][qi] = __builtin_amdgcn_mfma_i32_32x32x32_i8(__builtin_bit_cast(i32x4, pr[pi]), __builtin_bit_cast(i32x4, qr[qi]), acci[pi][qi], 0, 0, 0);
            else accf[pi][qi] = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, pr[pi]), __builtin_bit_cast(f16x8, qr[qi]), accf[pi][qi], 0, 0, 0);
          }
      }
    }
    if (kt + 1 < nk) WIS_CQ_SSTORE(cur ^ 1)
    __syncthreads();
  }
#undef WIS_CQ_GLOAD
#undef WIS_CQ_SSTORE

  // ---- epilogue: wave-private from here on (no barrier below this line)
  const int t0w = t0 + 64 * wm;
  if (t0w >= Tpad) return;
  const int ncol = n0 + 64 * wn;      // the wave's first column: bias / weight-scale index
  char* tile = smem + wave * CQ_WAVE;
  float* sinv = reinterpret_cast<float*>(tile + 64 * CQ_RB);
  float* ssa = sinv + 64;
  if constexpr (I8) {
    int t = t0w + lane; if (t > T - 1) t = T - 1;
    ssa[lane] = sa[(int64_t)b * T + t];
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  }
  // x = the index a lane holds ONE of (K waves: key, V waves: head dimension), y = the index it holds quads of; tile [x][y]
  constexpr int NX = MODE == CQ_F16_16 ? 4 : 2, XB = 64 / NX, NQ = MODE == CQ_F16_16 ? 1 : 4;
  const int xl = MODE == CQ_F16_16 ? l15 : l31, yl = MODE == CQ_F16_16 ? 4 * kq4 : 4 * hi;
  auto accv = [&](int yb, int xb, int r) -> float {      // block (quads, lane index) = (p, q)
    if constexpr (MODE == CQ_F16_16) return acc4[yb][xb][r];
    else if constexpr (I8) return (float)acci[yb][xb][r];
    else return accf[yb][xb][r];
  };
  if (!isV) {
#pragma unroll
    for (int mi = 0; mi < NX; ++mi) {
      const int x = XB * mi + xl;
      const bool dead = t0w + x >= T;
      const float sam = I8 ? ssa[x] : 0.f;
#pragma unroll
      for (int ni = 0; ni < NX; ++ni)
#pragma unroll
        for (int r4 = 0; r4 < NQ; ++r4) {
          const int y = XB * ni + 8 * r4 + yl;
          const float4 bq = *reinterpret_cast<const float4*>(bias + ncol + y);
          float4 sq = make_float4(0.f, 0.f, 0.f, 0.f);
          if constexpr (I8) sq = *reinterpret_cast<const float4*>(sw + ncol + y);
          float v0, v1, v2, v3;
          if constexpr (I8) {
            v0 = accv(ni, mi, 4 * r4) * (sam * sq.x) + bq.x; v1 = accv(ni, mi, 4 * r4 + 1) * (sam * sq.y) + bq.y;
            v2 = accv(ni, mi, 4 * r4 + 2) * (sam * sq.z) + bq.z; v3 = accv(ni, mi, 4 * r4 + 3) * (sam * sq.w) + bq.w;
          } else {
            v0 = accv(ni, mi, 4 * r4) + bq.x; v1 = accv(ni, mi, 4 * r4 + 1) + bq.y; v2 = accv(ni, mi, 4 * r4 + 2) + bq.z; v3 = accv(ni, mi, 4 * r4 + 3) + bq.w;
          }
          if (dead) { v0 = 0.f; v1 = 0.f; v2 = 0.f; v3 = 0.f; }
          cq_put(tile, x, y, v0, v1, v2, v3);
        }
    }
  } else {
#pragma unroll
    for (int ni = 0; ni < NX; ++ni) {
      const int x = XB * ni + xl;
      const float bv = bias[ncol + x];
      const float swv = I8 ? sw[ncol + x] : 0.f;
#pragma unroll
      for (int mi = 0; mi < NX; ++mi)
#pragma unroll
        for (int r4 = 0; r4 < NQ; ++r4) {
          const int y = XB * mi + 8 * r4 + yl;
          float v0, v1, v2, v3;
          if constexpr (I8) {
            const float4 s4 = *reinterpret_cast<const float4*>(ssa + y);
            v0 = accv(mi, ni, 4 * r4) * (s4.x * swv) + bv; v1 = accv(mi, ni, 4 * r4 + 1) * (s4.y * swv) + bv;
            v2 = accv(mi, ni, 4 * r4 + 2) * (s4.z * swv) + bv; v3 = accv(mi, ni, 4 * r4 + 3) * (s4.w * swv) + bv;
          } else {
            v0 = accv(mi, ni, 4 * r4) + bv; v1 = accv(mi, ni, 4 * r4 + 1) + bv; v2 = accv(mi, ni, 4 * r4 + 2) + bv; v3 = accv(mi, ni, 4 * r4 + 3) + bv;
          }
          const int tk = t0w + y;
          if (tk >= T) v0 = 0.f;
          if (tk + 1 >= T) v1 = 0.f;
          if (tk + 2 >= T) v2 = 0.f;
          if (tk + 3 >= T) v3 = 0.f;
          cq_put(tile, x, y, v0, v1, v2, v3);
        }
    }
  }
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");      // wave-private tile: the wave's own LDS writes have landed
  const size_t bh = (size_t)b * H + h;
  if (!isV) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int key = 16 * i + l15, t = t0w + key;
      const f16x8 ka = *reinterpret_cast<const f16x8*>(tile + key * CQ_RB + 16 * kq4), kc = *reinterpret_cast<const f16x8*>(tile + key * CQ_RB + 64 + 16 * kq4);
      float mx = 0.f;
#pragma unroll
      for (int e = 0; e < 8; ++e) mx = fmaxf(mx, fmaxf(fabsf((float)ka[e]), fabsf((float)kc[e])));
      mx = q8_xrow_max(mx);
      const float sc = mx > 0.f ? mx / 127.0f : 1.0f, inv = 1.0f / sc;
      const u32x4 o = {q8_pack4(ka[0], ka[1], ka[2], ka[3], inv, inv, inv, inv), q8_pack4(ka[4], ka[5], ka[6], ka[7], inv, inv, inv, inv),
                       q8_pack4(kc[0], kc[1], kc[2], kc[3], inv, inv, inv, inv), q8_pack4(kc[4], kc[5], kc[6], kc[7], inv, inv, inv, inv)};
      *reinterpret_cast<u32x4*>(kq + lyr * q_ls + ((bh * 4 + kq4) * Tpad + t) * 16) = o;      // t < Tpad: t0w < Tpad, both multiples of 64
      if (kq4 == 0) sk[lyr * s_ls + bh * Tpad + t] = sc;
    }
    return;
  }
  {
    const int kp = lane & 31;      // keys 2 kp, 2 kp + 1; head dimensions 32 hi .. + 31
    float m0 = 0.f, m1 = 0.f;
#pragma unroll
    for (int i = 0; i < 32; ++i) {
      const f16x2 v = *reinterpret_cast<const f16x2*>(tile + (32 * hi + i) * CQ_RB + 4 * kp);
      m0 = fmaxf(m0, fabsf((float)v[0])); m1 = fmaxf(m1, fabsf((float)v[1]));
    }
    m0 = q8_x32_max(m0); m1 = q8_x32_max(m1);
    const float s0 = m0 > 0.f ? m0 / 127.0f : 1.0f, s1 = m1 > 0.f ? m1 / 127.0f : 1.0f;
    if (hi == 0) {
      *reinterpret_cast<float2*>(sinv + 2 * kp) = make_float2(1.0f / s0, 1.0f / s1);
      *reinterpret_cast<float2*>(sv + lyr * s_ls + bh * Tpad + t0w + 2 * kp) = make_float2(s0, s1);
    }
  }
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int pc = lane + 64 * i, dh = pc >> 2, jj = pc & 3;      // output piece: keys 8 jj .. + 7 and 32 + 8 jj .. + 7 of the group
    const f16x8 a = *reinterpret_cast<const f16x8*>(tile + dh * CQ_RB + 16 * jj), c = *reinterpret_cast<const f16x8*>(tile + dh * CQ_RB + 64 + 16 * jj);
    const float4 ia0 = *reinterpret_cast<const float4*>(sinv + 8 * jj), ia1 = *reinterpret_cast<const float4*>(sinv + 8 * jj + 4);
    const float4 ic0 = *reinterpret_cast<const float4*>(sinv + 32 + 8 * jj), ic1 = *reinterpret_cast<const float4*>(sinv + 36 + 8 * jj);
    const u32x4 o = {q8_pack4(a[0], a[1], a[2], a[3], ia0.x, ia0.y, ia0.z, ia0.w), q8_pack4(a[4], a[5], a[6], a[7], ia1.x, ia1.y, ia1.z, ia1.w),
                     q8_pack4(c[0], c[1], c[2], c[3], ic0.x, ic0.y, ic0.z, ic0.w), q8_pack4(c[4], c[5], c[6], c[7], ic1.x, ic1.y, ic1.z, ic1.w)};
    *reinterpret_cast<u32x4*>(vq + lyr * q_ls + (bh * 64 + dh) * Tpad + t0w + 16 * jj) = o;
  }
}

int launch_cross_kv_fused(hipStream_t st, const CrossKvQ8P& p) {
  const bool i8 = p.sa != nullptr;
  if (!p.A || !p.W || !p.bias || !p.kq || !p.vq || !p.sk || !p.sv || (p.sa == nullptr) != (p.sw == nullptr) || p.B < 1 || p.T < 1 || p.H < 1 || p.L < 1 || p.d != 64 * p.H ||
      p.Tpad < p.T || p.Tpad % 64) {
    set_error("cross_kv_fused: B=%d T=%d Tpad=%d H=%d d=%d L=%d unsupported (d = 64 H, Tpad %% 64, Tpad >= T; int8 operands bring both scale vectors)", p.B, p.T, p.Tpad, p.H,
              p.d, p.L); return WIS_E_ARG; }
  const int64_t img = (int64_t)p.B * p.H * 64 * p.Tpad;
  if (p.q_ls % 16 || p.s_ls % 2 || p.q_ls < img || p.s_ls < (int64_t)p.B * p.H * p.Tpad) {
    set_error("cross_kv_fused: layer strides %lld / %lld too short or misaligned", (long long)p.q_ls, (long long)p.s_ls); return WIS_E_ARG; }
  const int nkb = cdiv(p.Tpad, 128), nmt = p.B * nkb, nnt = p.L * p.H;      // (L 2 d / 128 column tiles)
  if ((int64_t)nmt * nnt > 0x7fffffff || (int64_t)p.B * p.T * p.d > 0x7fffffff) { set_error("cross_kv_fused: B=%d T=%d d=%d L=%d too large", p.B, p.T, p.d, p.L); return WIS_E_ARG; }
  const dim3 grid(nmt * nnt);
  const char* A = reinterpret_cast<const char*>(p.A); const char* W = reinterpret_cast<const char*>(p.W);
#define WIS_CQ_LAUNCH(MODE, RB) hipLaunchKernelGGL((cross_kv_q8_fused_kernel<MODE>), grid, dim3(256), 0, st, A, W, RB, p.T, p.Tpad, p.H, nkb, nmt, nnt, p.sa, p.sw, p.bias, \
                                                   p.kq, p.vq, p.sk, p.sv, p.q_ls, p.s_ls)
  if (i8) WIS_CQ_LAUNCH(CQ_I8, p.d);
  else if (p.chain == 16) WIS_CQ_LAUNCH(CQ_F16_16, 2 * p.d);
  else if (p.chain == 32) WIS_CQ_LAUNCH(CQ_F16_32, 2 * p.d);
  else { set_error("cross_kv_fused: f16 operands need the accumulator chain of the shape (16 or 32), got %d", p.chain); return WIS_E_ARG; }
#undef WIS_CQ_LAUNCH
  return WIS_OK;
}

// =======================================================================================
// Cross-attention of the R (<= 16) query rows of one utterance over a chunk of 256 keys of the int8 images.  grid (chunks, H, B), block 256 = 4 waves.
//
// What the f16 kernels showed: a workgroup of this family is bound by how fast the CU's address path takes its wave requests, not by
// arithmetic, so the design counts requests.  A 16-byte request of a lane carries 16 int8 values, and the two images above are laid out so that those
// 16 are two whole MFMA fragments of that lane.  Per wave:
//   K       4 requests   key tiles 4 wave .. 4 wave + 3 of the chunk (64 keys), both k-steps of a tile in one        (f16: 8)
//   V       4 requests   head dimensions 16 wave .. + 15, the chunk's four 64-key groups, two P.V steps in one        (f16: 8)
//   scales  1 request    lanes 0-15 the wave's 64 sk as float4, lanes 16-31 its 64 sv; handed to the lanes that need them through a wave-private LDS
//                        row (a lane's four scores are four consecutive keys: one 16-byte LDS read per tile) - not one request per tile
//   query   4 requests (finished query) / 5 (the fold from partials: ca_query.hpp, operands once per workgroup through LDS)
// 13 or 14 against the f16 kernel's 20 or 21.  Everything is requested up front: with 8 KB less in flight per wave than the f16 form the kernel has the
// registers for it (K 16, V 16, query 16), and V is not needed before the softmax.
// Every wave takes scores, maxima, exponentials and row sums of ITS 64 keys in registers: the MFMA output layout keeps a query row in a lane column and
// a lane's 16 scores are the row's, so the chunk maximum is two cross-row moves and one exchange of 4 x 16 floats through LDS - no score buffer.  Two
// raw workgroup barriers (they wait for LDS, never for the V requests still in flight): behind the maxima, behind P.
// Arithmetic (include/wis_hip.h): int8 -> f16 in registers is exact (v_perm_b32 puts the byte under the exponent of 1024, one packed f16 subtraction removes
// 1152: three VALU operations per pair); score = (f32 MFMA result) * sk[t]; exponentials about the chunk maximum, the row sum over the unrounded
// exponentials; p * sv[t] in f32, then rounded to f16 - the per-key V scale rides on P, which has to be converted anyway.
// Chunk partials (o[64], max, sum) are published with write-through stores and combined by the last-arriving workgroup (the f16 kernels' ticket form:
// same partial format, same combine order).  Nothing here waits for another workgroup.
__device__ __forceinline__ void q8_st_sc1(float* p, float v) {
  __hip_atomic_store(reinterpret_cast<unsigned*>(p), __float_as_uint(v), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// 8 int8 (two dwords) -> f16x8, exact: f16 bits 0x6400 | u = 1024 + u for a byte u; u = b ^ 0x80 = b + 128
__device__ __forceinline__ f16x8 q8_i8x8_f16(unsigned lo, unsigned hi) {
  const u32x4 w = {__builtin_amdgcn_perm(0x64646464u, lo, 0x04010400u) ^ 0x00800080u, __builtin_amdgcn_perm(0x64646464u, lo, 0x04030402u) ^ 0x00800080u,
                   __builtin_amdgcn_perm(0x64646464u, hi, 0x04010400u) ^ 0x00800080u, __builtin_amdgcn_perm(0x64646464u, hi, 0x04030402u) ^ 0x00800080u};
  const f16x8 bias = {1152, 1152, 1152, 1152, 1152, 1152, 1152, 1152};
  return __builtin_bit_cast(f16x8, w) - bias;
}
constexpr int Q8_PSTR = 264;   // f16 row pitch of the P image (256 keys + 8: 16-byte aligned, bank-skewed)
constexpr int Q8_CM = 6;       // chunks the combine handles (register arrays of that size): 1536 keys

// (argument order: the first 15 dwords - what the first round of requests is addressed from - are preloaded into SGPRs)
template <bool FOLD>
__global__ __launch_bounds__(256) void dec_cross_attn_q8_kernel(const float* __restrict__ q, const int8_t* __restrict__ kq8, const float* __restrict__ sk,
                                                                const float* __restrict__ sv, const float* __restrict__ xres, const float* __restrict__ q2,
                                                                int RHC, int dT, int TpadF, const int8_t* __restrict__ vq8, f16* __restrict__ out, float* part,
                                                                unsigned* counters, int out_mb, const float* __restrict__ qcs, const float* __restrict__ qb) {
  // rows | heads << 8 | chunks << 24, d | T << 16, Tpad | kv_shared << 30
  const int R = RHC & 0xFF, H = (RHC >> 8) & 0x3F, C = (RHC >> 24) & 0xFF, d = dT & 0xFFFF, T = (dT >> 16) & 0xFFFF;
  __shared__ __attribute__((aligned(16))) f16 sp16[16 * Q8_PSTR];
  __shared__ __attribute__((aligned(16))) float ssc[2][256];      // the chunk's sk | sv (wave w: its own keys 64 w .. 64 w + 63)
  __shared__ float smax[4][16], ssumw[4][16];
  __shared__ int s_last;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l15 = lane & 15, kq = lane >> 4;
  const int c = blockIdx.x, h = blockIdx.y, b = blockIdx.z;
  const int Tpad = TpadF & 0x3FFFFFFF, bkv = (TpadF >> 30) ? 0 : b;      // kv_shared: the row groups are rows of ONE utterance
  const int klo = c * 256, n = (klo + 256 <= T) ? 256 : T - klo;        // 1 <= n <= 256
  const int rq = l15 < R ? l15 : R - 1;

  // ---- requests: the query's operands, K, the scales, V (all addresses clamped into the images; what a clamp fetches is masked by kl < n below)
  CaFoldReq fr;
  float4 qa0, qa1, qb0, qb1;
  if (FOLD) ca_fold_request(fr, q, q2, xres, qcs, qb, b, h, R, d);
  else {
    const float* qp = q + (size_t)(b * R + rq) * d + h * 64 + 8 * kq;
    qa0 = *reinterpret_cast<const float4*>(qp); qa1 = *reinterpret_cast<const float4*>(qp + 4);
    qb0 = *reinterpret_cast<const float4*>(qp + 32); qb1 = *reinterpret_cast<const float4*>(qp + 36);
  }
  const size_t bh = (size_t)bkv * H + h;
  const int8_t* kb = kq8 + bh * 64 * Tpad;
  u32x4 kf[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    int key = klo + 64 * wave + 16 * i + l15; if (key > Tpad - 1) key = Tpad - 1;
    kf[i] = *reinterpret_cast<const u32x4*>(kb + ((size_t)kq * Tpad + key) * 16);
  }
  int s0 = klo + 64 * wave + 4 * l15; if (s0 > Tpad - 4) s0 = Tpad - 4;
  const float4 sc4 = *reinterpret_cast<const float4*>(((lane & 16) ? sv : sk) + bh * Tpad + s0);
  const int8_t* vb = vq8 + (bh * 64 + 16 * wave + l15) * Tpad + 16 * kq;
  u32x4 vf[4];
#pragma unroll
  for (int g = 0; g < 4; ++g) {
    int g0 = klo + 64 * g; if (g0 > Tpad - 64) g0 = Tpad - 64;
    vf[g] = *reinterpret_cast<const u32x4*>(vb + g0);
  }
  __builtin_amdgcn_sched_barrier(0);      // every load of the kernel is requested above this line

  // ---- the finished query as B fragments (f16), the wave's scales into its LDS row
  f16x8 qf0, qf1;
  if constexpr (FOLD) {      // (the staging block exists in this instantiation only)
    __shared__ CaFoldLds fold_lds;
    ca_fold_finish(fr, fold_lds, R, d, rq, kq, qf0, qf1);
  } else {
    qf0[0] = (f16)qa0.x; qf0[1] = (f16)qa0.y; qf0[2] = (f16)qa0.z; qf0[3] = (f16)qa0.w; qf0[4] = (f16)qa1.x; qf0[5] = (f16)qa1.y; qf0[6] = (f16)qa1.z; qf0[7] = (f16)qa1.w;
    qf1[0] = (f16)qb0.x; qf1[1] = (f16)qb0.y; qf1[2] = (f16)qb0.z; qf1[3] = (f16)qb0.w; qf1[4] = (f16)qb1.x; qf1[5] = (f16)qb1.y; qf1[6] = (f16)qb1.z; qf1[7] = (f16)qb1.w;
  }
  if (lane < 32) *reinterpret_cast<float4*>(&ssc[lane >> 4][64 * wave + 4 * l15]) = sc4;
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");      // wave-private row: the wave's own LDS writes have landed

  // ---- scores of this wave's 64 keys: D[key][r], lane holds r = l15 and keys 64 wave + 16 i + 4 kq + reg
  float s[4][4];
  float lmax = -INFINITY;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(q8_i8x8_f16(kf[i][0], kf[i][1]), qf0, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(q8_i8x8_f16(kf[i][2], kf[i][3]), qf1, acc, 0, 0, 0);
    const int kl0 = 64 * wave + 16 * i + 4 * kq;
    const float4 skv = *reinterpret_cast<const float4*>(&ssc[0][kl0]);
    s[i][0] = (kl0 + 0 < n) ? acc[0] * skv.x : -INFINITY; s[i][1] = (kl0 + 1 < n) ? acc[1] * skv.y : -INFINITY;
    s[i][2] = (kl0 + 2 < n) ? acc[2] * skv.z : -INFINITY; s[i][3] = (kl0 + 3 < n) ? acc[3] * skv.w : -INFINITY;
    lmax = fmaxf(fmaxf(lmax, fmaxf(s[i][0], s[i][1])), fmaxf(s[i][2], s[i][3]));
  }
  lmax = q8_xrow_max(lmax);
  if (kq == 0) smax[wave][l15] = lmax;
  asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
  const float mref = fmaxf(fmaxf(smax[0][l15], smax[1][l15]), fmaxf(smax[2][l15], smax[3][l15]));      // finite: key klo is a key of the chunk
  // ---- P = exp(S - max) sv as f16, row sums of the unrounded exponentials
  float lsum = 0.f;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int kl0 = 64 * wave + 16 * i + 4 * kq;
    const float4 svv = *reinterpret_cast<const float4*>(&ssc[1][kl0]);
    const float e0 = __expf(s[i][0] - mref), e1 = __expf(s[i][1] - mref), e2 = __expf(s[i][2] - mref), e3 = __expf(s[i][3] - mref);
    lsum += e0; lsum += e1; lsum += e2; lsum += e3;
    const f16x4 ph = {(kl0 + 0 < n) ? (f16)(e0 * svv.x) : (f16)0, (kl0 + 1 < n) ? (f16)(e1 * svv.y) : (f16)0,
                      (kl0 + 2 < n) ? (f16)(e2 * svv.z) : (f16)0, (kl0 + 3 < n) ? (f16)(e3 * svv.w) : (f16)0};
    *reinterpret_cast<f16x4*>(&sp16[l15 * Q8_PSTR + kl0]) = ph;
  }
  lsum = q8_xrow_sum(lsum);
  if (kq == 0) ssumw[wave][l15] = lsum;
  asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");

  // ---- O^T[dh][r]: wave w owns dh 16 w .. 16 w + 15; D[dh][r]: lane holds r = l15, dh = 16 w + 4 kq + reg; the 32-key steps in key order
  f32x4 oacc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int g = 0; g < 4; ++g) {
    const f16x8 p0 = *reinterpret_cast<const f16x8*>(&sp16[rq * Q8_PSTR + 64 * g + 8 * kq]);
    const f16x8 p1 = *reinterpret_cast<const f16x8*>(&sp16[rq * Q8_PSTR + 64 * g + 32 + 8 * kq]);
    oacc = __builtin_amdgcn_mfma_f32_16x16x32_f16(q8_i8x8_f16(vf[g][0], vf[g][1]), p0, oacc, 0, 0, 0);
    oacc = __builtin_amdgcn_mfma_f32_16x16x32_f16(q8_i8x8_f16(vf[g][2], vf[g][3]), p1, oacc, 0, 0, 0);
  }
  const float Lc = (ssumw[0][l15] + ssumw[1][l15]) + (ssumw[2][l15] + ssumw[3][l15]);
  const int dh0 = 16 * wave + 4 * kq;
  if (C == 1) {
    if (l15 < R) {
      const float inv = 1.0f / Lc;
      const f16x4 o = {(f16)(oacc[0] * inv), (f16)(oacc[1] * inv), (f16)(oacc[2] * inv), (f16)(oacc[3] * inv)};
      *reinterpret_cast<f16x4*>(out + (out_mb ? xf_index(b * R + l15, h * 64 + dh0, out_mb) : (size_t)(b * R + l15) * d + h * 64 + dh0)) = o;
    }
    return;
  }
  // ---- split-T: publish the partial with write-through stores; the last-arriving workgroup combines (dec_cross_attn_kernel's ticket form)
  float* pbase = part + ((size_t)(b * H + h) * C) * R * 66;
  if (l15 < R) {
    float* pp = pbase + ((size_t)c * R + l15) * 66;
#pragma unroll
    for (int r4 = 0; r4 < 4; ++r4) q8_st_sc1(pp + dh0 + r4, oacc[r4]);
    if (wave == 0 && kq == 0) { q8_st_sc1(pp + 64, mref); q8_st_sc1(pp + 65, Lc); }
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");     // every storing wave drains its write-through stores
  __syncthreads();
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
  if (!s_last) return;
  for (int item = tid; item < R * 32; item += 256) {      // thread = (row r, dh pair)
    const int r = item >> 5, dp = item & 31;
    float2 ml[Q8_CM], ov[Q8_CM];
#pragma unroll
    for (int cc = 0; cc < Q8_CM; ++cc) {
      if (cc < C) {
        const float* pp = pbase + ((size_t)cc * R + r) * 66;
        ml[cc] = *reinterpret_cast<const float2*>(pp + 64);
        ov[cc] = *reinterpret_cast<const float2*>(pp + 2 * dp);
      }
    }
    float M_ = -INFINITY;
#pragma unroll
    for (int cc = 0; cc < Q8_CM; ++cc) if (cc < C) M_ = fmaxf(M_, ml[cc].x);
    float L = 0.f, O0 = 0.f, O1 = 0.f;
#pragma unroll
    for (int cc = 0; cc < Q8_CM; ++cc) {
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
}

// launch_dec_cross_attn's int8 branch (CrossAttnP::kq8 set).  256-key chunks always: p.chunks only has to be positive; T <= 1536
int launch_dec_cross_attn_q8(hipStream_t st, const CrossAttnP& p) {
  const int B = p.B, R = p.R, H = p.H, d = p.d, T = p.T, Tpad = p.Tpad;
  if (!p.q || !p.kq8 || !p.vq8 || !p.sk || !p.sv || !p.out || !p.part || !p.counters || B < 1) { set_error("dec_cross_attn (int8 K/V): bad argument"); return WIS_E_ARG; }
  if (p.xres && (!p.xres_is_stat || !p.qcs || !p.qb || R > 8 || d > 2048)) {
    set_error("dec_cross_attn (int8 K/V): the folded query comes from row partials with column sums and bias, R <= 8 and d <= 2048"); return WIS_E_ARG; }
  if ((p.xres_is_stat || p.q2) && !p.xres) { set_error("dec_cross_attn (int8 K/V): the fold from partials needs the row partials"); return WIS_E_ARG; }
  if (R < 1 || R > 16 || p.chunks < 1) { set_error("dec_cross_attn (int8 K/V): R=%d chunks=%d unsupported", R, p.chunks); return WIS_E_UNSUPPORTED; }
  if (H < 1 || H > 63 || d != 64 * H || T < 1 || T > 256 * Q8_CM || Tpad < T || Tpad % 64) {
    set_error("dec_cross_attn (int8 K/V): H=%d d=%d T=%d Tpad=%d unsupported (d = 64 H, T <= %d, Tpad %% 64)", H, d, T, Tpad, 256 * Q8_CM); return WIS_E_UNSUPPORTED; }
  const int used = cdiv(T, 256);
  const dim3 grid(used, H, B);
  const int rhc = R | (H << 8) | (used << 24), dt = d | (T << 16), tp = Tpad | (p.kv_shared ? (1 << 30) : 0);
  if (p.xres) hipLaunchKernelGGL((dec_cross_attn_q8_kernel<true>), grid, dim3(256), 0, st, p.q, p.kq8, p.sk, p.sv, p.xres, p.q2, rhc, dt, tp, p.vq8, p.out, p.part, p.counters,
                                 p.out_mb, p.qcs, p.qb);
  else hipLaunchKernelGGL((dec_cross_attn_q8_kernel<false>), grid, dim3(256), 0, st, p.q, p.kq8, p.sk, p.sv, p.xres, p.q2, rhc, dt, tp, p.vq8, p.out, p.part, p.counters,
                          p.out_mb, p.qcs, p.qb);
  return WIS_OK;
}

}  // namespace wis
