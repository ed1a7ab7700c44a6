// resample.hip — an object of its own beside logmel.hip (the audio front end's other half; the device context is logmel.hip's, common.hpp).  Sample-rate conversion of an upload to 16 kHz on gfx950: the resampling half of
// `librosa.load(audio_file, sr=16000)` (reference main.py:579, :815; `x-audio-sample-rate` on /api/willow).
//
// The filter and the output are the ones wis_hip/audio.py defines (_resample_filter, resample):
//   up = 16000 / g, down = sr_in / g, g = gcd(sr_in, 16000); q = max(up, down)
//   h[t], t = 0 .. 64 q: Kaiser-windowed sinc, 32 zero crossings each side at the lower rate, beta 14.769656459379492,
//                        cut-off 0.945 of the lower Nyquist, scaled so that the taps sum to `up`; half = 32 q
//   n_out = ceil(n_in up / down);  y[m] = sum over k in [0, n_in) of x[k] h[m down - k up + half]
//
// Layout.  With c = m down + half, k_hi = c / up and t0 = c mod up, output m reads the taps h[t0 + j up] against x[k_hi - j],
// j = 0 .. taps_per_phase - 1 (taps_per_phase = ceil(n_taps / up); tap indices past the prototype's end are zero taps).  The
// device table is phase-major and reversed, tab[t0][i] = h[t0 + (taps_per_phase - 1 - i) up], so one output's taps are
// contiguous and ascend with k: y[m] = sum_i x[k_hi - (taps_per_phase - 1) + i] tab[t0][i].  The table is built once per (up, down)
// and device from the fp64 prototype (rounded to f32 once) and stays in HBM.
//
// Kernel.  256 threads = 256 consecutive outputs; the workgroup's input span (at most ceil(256 down / up) + taps_per_phase + 2
// floats: 1923 at 96 kHz) is staged in LDS with zeros outside the signal.  Plain f32 FMAs, no MFMA.  Every index that scales
// with the position in the signal (m down, k) is 64-bit: an hour of 96 kHz audio passes 2^31.
//
// Invariant: the bits of y[m] depend on the signal, the ratio and m alone - not on the workgroup, launch or segment that
// computed them.  Every output is ALWAYS the same taps_per_phase-term sum: four FMA chains over i = 0, 1, 2, 3 (mod 4),
// ascending, merged as (a0 + a1) + (a2 + a3).  Edges read zeros; the sum is never shortened by position.
//
// Long inputs run in segments over a bounded workspace (own stream, own staging; per-device free list, as wis_logmel's): a
// slice of input with the filter's reach goes up, the outputs whose support lies inside it come back.
#include <math.h>
#include <string.h>
#include <mutex>
#include <vector>

#include "common.hpp"

namespace wis {

namespace {
constexpr int RS_OUT_RATE = WIS_SAMPLE_RATE;
constexpr int RS_ZEROS = 32;                          // zero crossings each side, at the lower rate
constexpr double RS_BETA = 14.769656459379492, RS_ROLLOFF = 0.945;
constexpr int64_t RS_MAX_TAPS = (int64_t)1 << 20;     // prototype taps served on the device (64 max(up, down) + 1)
constexpr int RS_BLOCK = 256;                         // outputs per workgroup
constexpr int RS_SPAN_LDS = 4096;                     // floats of LDS for the input span; a wider span (down / up > 12 or so) reads HBM
constexpr int64_t RS_SEGMENT = (int64_t)1 << 22;      // input samples per segment (wis_resample; wis_resample_ex overrides)
constexpr int64_t RS_SEGMENT_OUT = (int64_t)1 << 24;  // ... and at most this many outputs (extreme up-sampling)
constexpr int64_t RS_MAX_IN = (int64_t)1 << 46;       // samples of a signal: n_in * up (up <= 16000) stays inside int64
constexpr size_t RS_MAX_TABLES = 64;                  // distinct ratios kept per device

struct RsPlan { int up, down, half, tpp; int64_t n_taps; };

int gcd_i(int a, int b) { while (b) { const int t = a % b; a = b; b = t; } return a; }
// up / down and the prototype's size for sr_in -> 16 kHz; WIS_E_UNSUPPORTED above the tap cap (p is filled in either way)
int make_plan(int sr_in, RsPlan* p) {
  const int g = gcd_i(sr_in, RS_OUT_RATE);
  p->up = RS_OUT_RATE / g; p->down = sr_in / g;
  const int64_t q = p->up > p->down ? p->up : p->down;
  p->n_taps = 2 * RS_ZEROS * q + 1;
  p->tpp = (int)((p->n_taps + p->up - 1) / p->up);
  if (p->n_taps > RS_MAX_TAPS) { p->half = 0; return WIS_E_UNSUPPORTED; }
  p->half = (int)(RS_ZEROS * q);
  return WIS_OK;
}
int64_t out_len(int64_t n_in, const RsPlan& p) { return (n_in * p.up + p.down - 1) / p.down; }

// modified Bessel function I0 by its power series sum_k ((x / 2)^k / k!)^2: all terms positive, so no cancellation
double bessel_i0(double x) {
  const double q = 0.25 * x * x;
  double term = 1.0, sum = 1.0;
  for (int k = 1; k < 1000; ++k) {
    term *= q / ((double)k * (double)k);
    sum += term;
    if (term < 1e-18 * sum) break;
  }
  return sum;
}
// the fp64 prototype, as audio._resample_filter: fc sinc(fc t) kaiser(2 n + 1, beta)[t + n], t = -n .. n, times up / sum
void build_filter(int up, int down, double* h) {
  const int64_t q = up > down ? up : down, n = RS_ZEROS * q, L = 2 * n + 1;
  const double PI = 3.14159265358979323846, fc = RS_ROLLOFF / (double)q, i0b = bessel_i0(RS_BETA);
  long double sum = 0.0L;
  for (int64_t i = 0; i < L; ++i) {
    const double t = (double)(i - n), y = PI * (fc * t);
    const double sinc = y == 0.0 ? 1.0 : sin(y) / y;
    const double r = t / (double)n;
    double a = 1.0 - r * r; if (a < 0.0) a = 0.0;
    h[i] = fc * sinc * (bessel_i0(RS_BETA * sqrt(a)) / i0b);
    sum += h[i];
  }
  const double scale = (double)up / (double)sum;
  for (int64_t i = 0; i < L; ++i) h[i] *= scale;
}

struct RsTable { int up, down; float* d_tab; };     // d_tab f32 [up][taps_per_phase]
// everything one wis_resample call touches on the device; owned by exactly one caller between acquire and release
struct RsWs {
  hipStream_t stream = nullptr;
  float* d_x = nullptr; float* d_y = nullptr;
  int64_t cap_x = 0, cap_y = 0;
};
}  // namespace

struct ResampleCtx {
  std::mutex mu;                 // the tables and the free list
  std::vector<RsTable> tabs;
  std::vector<RsWs*> ws_free;
};
ResampleCtx* resample_ctx_new() { return new ResampleCtx(); }

namespace {
// the device's table for the plan's ratio, built at first use under the context's lock
int get_table(DeviceCtx* c, const RsPlan& p, const float** out) {
  ResampleCtx* r = ctx_resample(c);
  std::lock_guard<std::mutex> lk(r->mu);
  for (const RsTable& t : r->tabs) if (t.up == p.up && t.down == p.down) { *out = t.d_tab; return WIS_OK; }
  if (r->tabs.size() >= RS_MAX_TABLES) { set_error("resample: %zu ratios are already resident on this device", r->tabs.size()); return WIS_E_UNSUPPORTED; }
  std::vector<double> h((size_t)p.n_taps);
  build_filter(p.up, p.down, h.data());
  std::vector<float> tab((size_t)p.up * p.tpp, 0.f);
  for (int t0 = 0; t0 < p.up; ++t0)
    for (int j = 0; j < p.tpp; ++j) {
      const int64_t t = t0 + (int64_t)j * p.up;
      if (t < p.n_taps) tab[(size_t)t0 * p.tpp + (p.tpp - 1 - j)] = (float)h[(size_t)t];
    }
  float* d = nullptr;
  if (hipMalloc(&d, tab.size() * 4) != hipSuccess) { (void)hipGetLastError(); set_error("resample: out of device memory for the %d/%d tap table", p.up, p.down); return WIS_E_NOMEM; }
  if (hipMemcpy(d, tab.data(), tab.size() * 4, hipMemcpyHostToDevice) != hipSuccess) { hipFree(d); set_error("resample: tap table upload failed"); return WIS_E_HIP; }
  r->tabs.push_back(RsTable{p.up, p.down, d});
  *out = d;
  return WIS_OK;
}

int rs_acquire(DeviceCtx* c, int64_t need_x, int64_t need_y, RsWs** out) {
  ResampleCtx* r = ctx_resample(c);
  RsWs* w = nullptr;
  {
    std::lock_guard<std::mutex> lk(r->mu);
    if (!r->ws_free.empty()) { w = r->ws_free.back(); r->ws_free.pop_back(); }
  }
  if (!w) {
    w = new RsWs();
    if (hipStreamCreateWithFlags(&w->stream, hipStreamNonBlocking) != hipSuccess) { delete w; set_error("wis_resample: stream create failed"); return WIS_E_HIP; }
  }
  if (need_x > w->cap_x || need_y > w->cap_y) {      // grown only while exclusively owned and idle (every call ends synchronised)
    hipFree(w->d_x); hipFree(w->d_y);
    w->d_x = w->d_y = nullptr; w->cap_x = w->cap_y = 0;
    if (hipMalloc(&w->d_x, (size_t)need_x * 4) != hipSuccess || hipMalloc(&w->d_y, (size_t)need_y * 4) != hipSuccess) {
      (void)hipGetLastError();
      hipFree(w->d_x); hipFree(w->d_y); w->d_x = w->d_y = nullptr;
      set_error("wis_resample: out of device memory for a segment of %lld samples", (long long)need_x);
      std::lock_guard<std::mutex> lk(r->mu); r->ws_free.push_back(w);      // caps 0: the next owner re-allocates
      return WIS_E_NOMEM;
    }
    w->cap_x = need_x; w->cap_y = need_y;
  }
  *out = w; return WIS_OK;
}
void rs_release(DeviceCtx* c, RsWs* w) {
  ResampleCtx* r = ctx_resample(c);
  std::lock_guard<std::mutex> lk(r->mu);
  r->ws_free.push_back(w);
}
}  // namespace

// ---------------------------------------------------------------------------------------
// grid ceil(count / 256), block 256.  x holds samples k_base .. k_base + n_slice - 1 of a signal of n_in samples; out[o] is
// output m0 + o, o < count.  A sample outside the signal is zero; so is one outside the slice (the host refuses a slice that
// does not cover the outputs' support, this guard only keeps every read inside the buffer).
__global__ __launch_bounds__(RS_BLOCK) void resample_kernel(
    const float* __restrict__ x, int64_t n_slice, int64_t k_base, int64_t n_in, int64_t m0, int64_t count,
    int up, int down, int half, int tpp, const float* __restrict__ tab, float* __restrict__ out, int use_lds) {
  __shared__ float s_x[RS_SPAN_LDS];
  const int tid = threadIdx.x;
  const int64_t o0 = (int64_t)blockIdx.x * RS_BLOCK;
  const int64_t left = count - o0;
  const int nb = left < RS_BLOCK ? (int)left : RS_BLOCK;       // outputs of this workgroup
  const int64_t mb = m0 + o0;
  const int64_t kb_lo = (mb * down + half) / up - (tpp - 1);   // first sample the workgroup's first output reads
  if (use_lds) {
    const int64_t kb_hi = ((mb + nb - 1) * down + half) / up;  // last sample its last output reads
    const int span = (int)(kb_hi - kb_lo + 1);                 // <= ceil(255 down / up) + tpp <= RS_SPAN_LDS (launcher's rule)
    for (int t = tid; t < span; t += RS_BLOCK) {
      const int64_t k = kb_lo + t, s = k - k_base;
      s_x[t] = (k >= 0 && k < n_in && s >= 0 && s < n_slice) ? x[s] : 0.f;
    }
    __syncthreads();
  }
  if (tid >= nb) return;
  const int64_t c = (mb + tid) * down + half, k_hi = c / up;
  const int t0 = (int)(c - k_hi * up);
  const int64_t k_lo = k_hi - (tpp - 1);
  const float* __restrict__ tp = tab + (size_t)t0 * tpp;
  float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
  int i = 0;
  if (use_lds) {
    const float* xs = s_x + (int)(k_lo - kb_lo);
    for (; i + 3 < tpp; i += 4) {
      a0 = fmaf(xs[i], tp[i], a0); a1 = fmaf(xs[i + 1], tp[i + 1], a1);
      a2 = fmaf(xs[i + 2], tp[i + 2], a2); a3 = fmaf(xs[i + 3], tp[i + 3], a3);
    }
    if (i < tpp) a0 = fmaf(xs[i], tp[i], a0);
    if (i + 1 < tpp) a1 = fmaf(xs[i + 1], tp[i + 1], a1);
    if (i + 2 < tpp) a2 = fmaf(xs[i + 2], tp[i + 2], a2);
  } else {
    auto rd = [&](int ii) -> float {
      const int64_t k = k_lo + ii, s = k - k_base;
      return (k >= 0 && k < n_in && s >= 0 && s < n_slice) ? x[s] : 0.f;
    };
    for (; i + 3 < tpp; i += 4) {
      a0 = fmaf(rd(i), tp[i], a0); a1 = fmaf(rd(i + 1), tp[i + 1], a1);
      a2 = fmaf(rd(i + 2), tp[i + 2], a2); a3 = fmaf(rd(i + 3), tp[i + 3], a3);
    }
    if (i < tpp) a0 = fmaf(rd(i), tp[i], a0);
    if (i + 1 < tpp) a1 = fmaf(rd(i + 1), tp[i + 1], a1);
    if (i + 2 < tpp) a2 = fmaf(rd(i + 2), tp[i + 2], a2);
  }
  out[o0 + tid] = (a0 + a1) + (a2 + a3);
}

namespace {
// the samples outputs m0 .. m0 + count - 1 read, before clipping to the signal: [*k_lo, *k_hi]
void support(const RsPlan& p, int64_t m0, int64_t count, int64_t* k_lo, int64_t* k_hi) {
  *k_lo = (m0 * p.down + p.half) / p.up - (p.tpp - 1);
  *k_hi = ((m0 + count - 1) * p.down + p.half) / p.up;
}
int launch_resample(hipStream_t st, const RsPlan& p, const float* d_tab, const float* d_x, int64_t n_slice, int64_t k_base, int64_t n_in,
                    int64_t m0, int64_t count, float* d_out) {
  if (count <= 0) return WIS_OK;
  const int64_t span_max = ((int64_t)RS_BLOCK * p.down + p.up - 1) / p.up + p.tpp + 2;      // the ratio's, not the launch's: one form per ratio
  hipLaunchKernelGGL(resample_kernel, dim3((unsigned)((count + RS_BLOCK - 1) / RS_BLOCK)), dim3(RS_BLOCK), 0, st,
                     d_x, n_slice, k_base, n_in, m0, count, p.up, p.down, p.half, p.tpp, d_tab, d_out, span_max <= RS_SPAN_LDS ? 1 : 0);
  WIS_HIP_CHECK(hipGetLastError());
  return WIS_OK;
}
}  // namespace

// the single-kernel tap's body (wis_op_resample_segment, csrc/taps.hip): device pointers, the caller's stream
int resample_segment(DeviceCtx* c, hipStream_t st, const float* d_x, int64_t n_slice, int64_t k_base, int64_t n_in_total, int64_t m0, int64_t count,
                     int up, int down, float* d_out) {
  const char* who = "wis_op_resample_segment";
  if (!d_x || !d_out || n_slice < 1 || k_base < 0 || n_in_total < 1 || n_in_total > RS_MAX_IN || k_base + n_slice > n_in_total || m0 < 0 || count < 1 ||
      count > ((int64_t)1 << 30) || up < 1 || down < 1) { set_error("%s: bad argument", who); return WIS_E_ARG; }
  if (gcd_i(up, down) != 1 || RS_OUT_RATE % up) { set_error("%s: up = %d, down = %d is no reduced ratio to %d Hz", who, up, down, RS_OUT_RATE); return WIS_E_ARG; }
  if ((int64_t)down * (RS_OUT_RATE / up) > 0x7fffffff) { set_error("%s: ratio %d/%d out of range", who, up, down); return WIS_E_ARG; }
  RsPlan p;
  const int rc = make_plan((int)((int64_t)down * (RS_OUT_RATE / up)), &p);
  if (rc != WIS_OK) { set_error("%s: %lld prototype taps for %d/%d (at most %lld)", who, (long long)p.n_taps, up, down, (long long)RS_MAX_TAPS); return rc; }
  if (p.up != up || p.down != down) { set_error("%s: up = %d, down = %d is no reduced ratio to %d Hz", who, up, down, RS_OUT_RATE); return WIS_E_ARG; }
  if (m0 + count > out_len(n_in_total, p)) { set_error("%s: outputs [%lld, %lld) of %lld", who, (long long)m0, (long long)(m0 + count), (long long)out_len(n_in_total, p)); return WIS_E_ARG; }
  int64_t k_lo, k_hi; support(p, m0, count, &k_lo, &k_hi);
  if (k_lo < 0) k_lo = 0;
  if (k_hi > n_in_total - 1) k_hi = n_in_total - 1;
  if (k_lo <= k_hi && (k_lo < k_base || k_hi >= k_base + n_slice)) {
    set_error("%s: the outputs read samples [%lld, %lld], the slice holds [%lld, %lld]", who, (long long)k_lo, (long long)k_hi, (long long)k_base, (long long)(k_base + n_slice - 1));
    return WIS_E_ARG;
  }
  const float* d_tab; WIS_RET(get_table(c, p, &d_tab));
  return launch_resample(st, p, d_tab, d_x, n_slice, k_base, n_in_total, m0, count, d_out);
}

}  // namespace wis

// ---------------------------------------------------------------------------------------
using namespace wis;

extern "C" int wis_resample_plan(int sr_in, int64_t n_in, int* up, int* down, int64_t* n_out, int* taps_per_phase, int64_t* n_taps) {
  if (sr_in <= 0 || n_in < 0 || n_in > RS_MAX_IN) { set_error("wis_resample_plan: sr_in = %d, n_in = %lld", sr_in, (long long)n_in); return WIS_E_ARG; }
  RsPlan p;
  const int rc = make_plan(sr_in, &p);
  if (up) *up = p.up;
  if (down) *down = p.down;
  if (n_out) *n_out = out_len(n_in, p);
  if (taps_per_phase) *taps_per_phase = p.tpp;
  if (n_taps) *n_taps = p.n_taps;
  if (rc != WIS_OK) set_error("wis_resample_plan: %d Hz -> %d Hz takes %lld prototype taps (at most %lld on the device)", sr_in, RS_OUT_RATE, (long long)p.n_taps, (long long)RS_MAX_TAPS);
  return rc;
}

extern "C" int wis_resample_filter(int up, int down, double* h, int64_t cap) {
  if (up < 1 || down < 1 || !h) { set_error("wis_resample_filter: bad argument"); return WIS_E_ARG; }
  const int64_t n_taps = 2 * RS_ZEROS * (int64_t)(up > down ? up : down) + 1;
  if (n_taps > RS_MAX_TAPS) { set_error("wis_resample_filter: %lld prototype taps (at most %lld)", (long long)n_taps, (long long)RS_MAX_TAPS); return WIS_E_UNSUPPORTED; }
  if (cap < n_taps) { set_error("wis_resample_filter: room for %lld taps, the prototype has %lld", (long long)cap, (long long)n_taps); return WIS_E_ARG; }
  build_filter(up, down, h);
  return WIS_OK;
}

// Re-entrant: every call runs on a workspace of its own (stream + staging) taken from the device's free list.
extern "C" int wis_resample_ex(int device, const float* pcm, int64_t n_in, int sr_in, float* out, int64_t out_cap, int64_t* n_out_p, int64_t segment_samples) {
  if (sr_in <= 0 || n_in < 0 || n_in > RS_MAX_IN || (!pcm && n_in > 0) || !n_out_p || out_cap < 0 || segment_samples < 0) { set_error("wis_resample: bad argument"); return WIS_E_ARG; }
  RsPlan p{};
  if (sr_in == RS_OUT_RATE) { p.up = p.down = 1; }
  else if (make_plan(sr_in, &p) != WIS_OK) {
    set_error("wis_resample: %d Hz -> %d Hz takes %lld prototype taps (at most %lld on the device)", sr_in, RS_OUT_RATE, (long long)p.n_taps, (long long)RS_MAX_TAPS);
    return WIS_E_UNSUPPORTED;
  }
  const int64_t n_out = out_len(n_in, p);
  *n_out_p = n_out;
  if (out_cap < n_out || (!out && n_out > 0)) { set_error("wis_resample: room for %lld samples, the result has %lld", (long long)out_cap, (long long)n_out); return WIS_E_ARG; }
  if (n_out == 0) return WIS_OK;
  if (sr_in == RS_OUT_RATE) { memcpy(out, pcm, (size_t)n_in * 4); return WIS_OK; }
  DeviceCtx* c; WIS_RET(get_ctx(device, &c));
  const float* d_tab; WIS_RET(get_table(c, p, &d_tab));
  // outputs per segment: what `segment` input samples produce; the slice is those outputs' support (the filter's reach on both sides)
  const int64_t seg = segment_samples ? segment_samples : RS_SEGMENT;
  int64_t mc = seg * p.up / p.down;
  if (mc < 1) mc = 1;
  if (mc > RS_SEGMENT_OUT) mc = RS_SEGMENT_OUT;
  if (mc > n_out) mc = n_out;
  int64_t need_x = (mc * p.down + p.up - 1) / p.up + p.tpp + 2;
  if (need_x > n_in) need_x = n_in;
  RsWs* ws; WIS_RET(rs_acquire(c, need_x, mc, &ws));
  hipStream_t st = ws->stream;
  auto body = [&]() -> int {
    for (int64_t ma = 0; ma < n_out; ma += mc) {
      const int64_t cnt = n_out - ma < mc ? n_out - ma : mc;
      int64_t k_lo, k_hi; support(p, ma, cnt, &k_lo, &k_hi);
      if (k_lo < 0) k_lo = 0;
      if (k_hi > n_in - 1) k_hi = n_in - 1;
      const int64_t n_slice = k_hi - k_lo + 1;
      if (n_slice < 1 || n_slice > ws->cap_x) { set_error("wis_resample: segment of %lld samples over a workspace of %lld", (long long)n_slice, (long long)ws->cap_x); return WIS_E_STATE; }
      WIS_HIP_CHECK(hipMemcpyAsync(ws->d_x, pcm + k_lo, (size_t)n_slice * 4, hipMemcpyHostToDevice, st));
      WIS_RET(launch_resample(st, p, d_tab, ws->d_x, n_slice, k_lo, n_in, ma, cnt, ws->d_y));
      WIS_HIP_CHECK(hipMemcpyAsync(out + ma, ws->d_y, (size_t)cnt * 4, hipMemcpyDeviceToHost, st));
    }
    WIS_HIP_CHECK(hipStreamSynchronize(st));      // the caller's buffers are free again
    return WIS_OK;
  };
  const int rc = body();
  if (rc != WIS_OK) hipStreamSynchronize(st);     // nothing of this call may still be in flight when the workspace is recycled
  rs_release(c, ws);
  return rc;
}
extern "C" int wis_resample(int device, const float* pcm, int64_t n_in, int sr_in, float* out, int64_t out_cap, int64_t* n_out) {
  return wis_resample_ex(device, pcm, n_in, sr_in, out, out_cap, n_out, 0);
}
