// taps.hip — debug, tuning and measurement taps (wis_debug_*, wis_bench_weight_stream, wis_dev_*, wis_op_*).  An object of its own: the taps run the
// product's own helpers (dec_forward, the stage builders, prep_projection: model.hpp), not copies of them.  tap.hpp says how to write a wis_op_* tap.
#include <string.h>
#include <algorithm>
#include <vector>

#include "common.hpp"
#include "kernels.hpp"
#include "model.hpp"
#include "tap.hpp"

using namespace wis;

// wis_op_wave_sums: one wave, wave_sum per value and wave_sums<N> on the same registers (the only kernel this object has: the helper is inlined
// into gemv_body and has no launch of its own)
template <int N>
__global__ __launch_bounds__(64) void wave_sums_tap_kernel(const float* __restrict__ x, float* __restrict__ out_old, float* __restrict__ out_new) {
  const int lane = threadIdx.x;
  float v[N], w[N];
#pragma unroll
  for (int i = 0; i < N; ++i) v[i] = x[i * 64 + lane];
#pragma unroll
  for (int i = 0; i < N; ++i) w[i] = wave_sum(v[i]);
  wave_sums(v);
#pragma unroll
  for (int i = 0; i < N; ++i) { out_old[i * 64 + lane] = w[i]; out_new[i * 64 + lane] = v[i]; }
}

extern "C" {

int wis_debug_encode(wis_model_t* m, const float* input, int input_kind, int B, float* enc_out) {
  if (!m || !input || !enc_out) { set_error("wis_debug_encode: bad argument"); return WIS_E_ARG; }
  WIS_ENTER(m, "wis_debug_encode")
  WIS_HIP_CHECK(hipSetDevice(m->device));
  WIS_RET(check_batch(m, B, 1));
  WIS_RET(stage_input(m, input, input_kind, B));
  WIS_RET(run_encoder(m, B));
  const int64_t n = (int64_t)B * m->cfg.n_audio_ctx * m->cfg.d_model;
  launch_f16_to_f32(m->st, m->mem, m->x, n);   // x is free after the encoder
  WIS_HIP_CHECK(hipMemcpyAsync(enc_out, m->x, (size_t)n * 4, hipMemcpyDeviceToHost, m->st));
  WIS_HIP_CHECK(hipStreamSynchronize(m->st));
  return WIS_OK;
}

// teacher-forced logits in blocks of R positions (wis_debug_logits: R = 1); `who` is the entry point the caller used
static int debug_logits_rows(const char* who, wis_model_t* m, const float* input, int input_kind, int B, const int32_t* dec_in, int T, int R, float* logits) {
  WIS_ENTER(m, who)
  WIS_HIP_CHECK(hipSetDevice(m->device));
  WIS_RET(check_batch(m, B, 1));
  if (B * R > MAX_ROWS) { set_error("%s: B*R = %d exceeds %d decoder rows per pass", who, B * R, MAX_ROWS); return WIS_E_STATE; }
  WIS_RET(run_front(m, input, input_kind, B));
  const int V = m->cfg.n_vocab;
  // the rows (b, i) of a pass sit at positions t0 + i of utterance b's KV slot (causal by position, like the merged prompt pass of
  // wis_generate), so a pass has B * R rows - with B * R > 8 it takes the batched-row route (dec_forward_frag: fragment images,
  // partial-sum LayerNorm statistics) that one row per utterance never reaches at small B
  for (int t0 = 0; t0 < T; t0 += R) {
    const int rows = std::min(R, T - t0), M = B * rows;
    std::vector<int> tok(M), pos(M), slot(M), ls(M);
    for (int b = 0; b < B; ++b) for (int i = 0; i < rows; ++i) { const int r = b * rows + i; tok[r] = dec_in[b * T + t0 + i]; pos[r] = t0 + i; slot[r] = b; ls[r] = b; }
    for (int r = 0; r < M; ++r) if (tok[r] < 0 || tok[r] >= V) { set_error("%s: token %d out of range", who, tok[r]); return WIS_E_ARG; }
    for (int attempt = 0; attempt < 2; ++attempt) {      // (a pass whose granule hand-off gave up is repeated in the ticket form)
      SpinClaim claim(m, B);
      WIS_RET(upload_rows(m, tok, pos, slot, ls));
      WIS_RET(dec_forward(m, M, rows, B, true, 1, 0));
      for (int b = 0; b < B; ++b) for (int i = 0; i < rows; ++i)
        WIS_HIP_CHECK(hipMemcpyAsync(logits + ((size_t)b * T + t0 + i) * V, m->logits + (size_t)(b * rows + i) * m->n_vocab_pad, (size_t)V * 4, hipMemcpyDeviceToHost, m->st));
      bool gave_up = false;
      WIS_RET(spin_gave_up(m, &gave_up));
      if (!gave_up) break;
    }
  }
  return WIS_OK;
}
int wis_debug_logits(wis_model_t* m, const float* input, int input_kind, int B, const int32_t* dec_in, int T, float* logits) {
  if (!m || !input || !dec_in || !logits || T < 1 || T > m->cfg.n_text_ctx) { set_error("wis_debug_logits: bad argument"); return WIS_E_ARG; }
  return debug_logits_rows("wis_debug_logits", m, input, input_kind, B, dec_in, T, 1, logits);
}
int wis_debug_logits_rows(wis_model_t* m, const float* input, int input_kind, int B, const int32_t* dec_in, int T, int R, float* logits) {
  if (!m || !input || !dec_in || !logits || T < 1 || T > m->cfg.n_text_ctx || R < 1 || R > 16) { set_error("wis_debug_logits_rows: bad argument (1 <= R <= 16)"); return WIS_E_ARG; }
  return debug_logits_rows("wis_debug_logits_rows", m, input, input_kind, B, dec_in, T, R, logits);
}

int wis_debug_phase_cycles(wis_model_t* m, int B, int beam, int pos, uint64_t* out) {
  if (!m || !out) { set_error("wis_debug_phase_cycles: bad argument"); return WIS_E_ARG; }
  if (!WIS_TAPS) { set_error("tuning taps are not compiled in (rebuild with WIS_EXTRA_HIPFLAGS=-DWIS_TAPS=1)"); return WIS_E_UNSUPPORTED; }
  WIS_ENTER(m, "wis_debug_phase_cycles")
  WIS_HIP_CHECK(hipSetDevice(m->device));
  WIS_RET(check_batch(m, B, beam));
  SpinClaim claim(m, B);      // the hand-off form wis_generate would take for this batch now (and not whatever the last call left behind)
  const int Mrows = B * beam, ctx = m->cfg.n_text_ctx;
  if (pos < 0 || pos >= ctx) { set_error("bad pos"); return WIS_E_ARG; }
  WIS_HIP_CHECK(hipStreamSynchronize(m->st));
  WIS_RET(single_row_setup(m, Mrows, std::vector<int>(Mrows, 100), pos));
  WIS_HIP_CHECK(hipMemsetAsync(m->d_prof, 0, 8 * 16 * 8, m->st));
  WIS_RET(dec_forward(m, Mrows, beam, B, false, beam, 1));   // warm
  m->prof_on = true;
  int rc = dec_forward(m, Mrows, beam, B, false, beam, 1);
  m->prof_on = false;
  WIS_RET(rc);
  // API order: QKV gemv, out-proj gemv, cross-attn, self-attn, FFN1 gemv, FFN2 gemv  <-  rows 0, 2, 4, 1, 6, 7
  // (more than 8 rows - the batched-row kernels, round 6: the fourth slot carries the cross-attention output projection (row 5); the attention
  // kernels' stamps are the one-utterance forms' and stay empty there)
  static const int rows_small[6] = {0, 2, 4, 1, 6, 7}, rows_frag[6] = {0, 2, 4, 5, 6, 7};
  const int* rows = Mrows > 8 ? rows_frag : rows_small;
  for (int i = 0; i < 6; ++i)
    WIS_HIP_CHECK(hipMemcpyAsync(out + i * 16, m->d_prof + rows[i] * 16, 16 * 8, hipMemcpyDeviceToHost, m->st));
  bool gave_up = false;
  WIS_RET(spin_gave_up(m, &gave_up));      // (synchronises the stream; a raised flag is consumed here, not by the next wis_generate)
  if (gave_up) { set_error("wis_debug_phase_cycles: the granule hand-off gave up during the tap; stamps are not valid"); return WIS_E_STATE; }
  return WIS_OK;
}

int wis_debug_phase_cycles_cq_arm(wis_model_t* m, uint64_t* out) {
  if (!m || !out) { set_error("wis_debug_phase_cycles_cq_arm: bad argument"); return WIS_E_ARG; }
  if (!WIS_TAPS) { set_error("tuning taps are not compiled in (rebuild with WIS_EXTRA_HIPFLAGS=-DWIS_TAPS=1)"); return WIS_E_UNSUPPORTED; }
  WIS_HIP_CHECK(hipSetDevice(m->device));
  WIS_HIP_CHECK(hipMemcpy(out, m->d_prof + 3 * 16, 16 * 8, hipMemcpyDeviceToHost));      // (row 3, the cross-Q row: dec_forward hands it to the launch's arm B)
  return WIS_OK;
}

int wis_debug_sampling_cycles(wis_model_t* m, uint64_t* out) {
  if (!m || !out) { set_error("wis_debug_sampling_cycles: bad argument"); return WIS_E_ARG; }
  if (!WIS_TAPS) { set_error("tuning taps are not compiled in (rebuild with WIS_EXTRA_HIPFLAGS=-DWIS_TAPS=1)"); return WIS_E_UNSUPPORTED; }
  WIS_HIP_CHECK(hipSetDevice(m->device));
  WIS_HIP_CHECK(hipMemcpy(out, m->d_prof + (size_t)m->cfg.n_dec_layers * 8 * 16, 2 * 16 * 8, hipMemcpyDeviceToHost));
  return WIS_OK;
}

int wis_debug_timeline(wis_model_t* m, int B, int beam, int pos, int use_graph, uint64_t* out, int n_out) {
  if (!m || !out) { set_error("wis_debug_timeline: bad argument"); return WIS_E_ARG; }
  if (!WIS_TAPS) { set_error("tuning taps are not compiled in (rebuild with WIS_EXTRA_HIPFLAGS=-DWIS_TAPS=1)"); return WIS_E_UNSUPPORTED; }
  WIS_ENTER(m, "wis_debug_timeline")
  WIS_HIP_CHECK(hipSetDevice(m->device));
  WIS_RET(check_batch(m, B, beam));
  SpinClaim claim(m, B);
  const int Mrows = B * beam, ctx = m->cfg.n_text_ctx, nk = m->cfg.n_dec_layers * 8;
  if (pos < 0 || pos >= ctx || n_out < nk) { set_error("wis_debug_timeline: bad pos / out size (need %d rows)", nk); return WIS_E_ARG; }
  WIS_HIP_CHECK(hipStreamSynchronize(m->st));
  WIS_RET(single_row_setup(m, Mrows, std::vector<int>(Mrows, 100), pos));
  std::vector<unsigned long long> init((size_t)nk * 16, 0ull);
  for (int k = 0; k < nk; ++k) init[(size_t)k * 16 + 14] = ~0ull;
  m->prof_on = true; m->prof_all = true;
  int rc = WIS_OK;
  hipGraph_t g = nullptr; hipGraphExec_t gx = nullptr;
  do {
    if (use_graph) {
      if (hipStreamBeginCapture(m->st, hipStreamCaptureModeThreadLocal) != hipSuccess) { set_error("capture failed"); rc = WIS_E_HIP; break; }
      rc = dec_forward(m, Mrows, beam, B, true, beam, 1);
      if (hipStreamEndCapture(m->st, &g) != hipSuccess || rc) { if (!rc) { set_error("end capture failed"); rc = WIS_E_HIP; } break; }
      if (hipGraphInstantiate(&gx, g, nullptr, nullptr, 0) != hipSuccess) { set_error("instantiate failed"); rc = WIS_E_HIP; break; }
    }
    for (int it = 0; it < 3 && !rc; ++it) {   // the last iteration is the one reported
      if (hipMemcpyAsync(m->d_prof, init.data(), init.size() * 8, hipMemcpyHostToDevice, m->st) != hipSuccess) { rc = WIS_E_HIP; break; }
      hipStreamSynchronize(m->st);
      if (use_graph) { if (hipGraphLaunch(gx, m->st) != hipSuccess) { set_error("graph launch failed"); rc = WIS_E_HIP; } }
      else rc = dec_forward(m, Mrows, beam, B, true, beam, 1);
      hipStreamSynchronize(m->st);
    }
  } while (0);
  m->prof_on = false; m->prof_all = false;
  if (gx) hipGraphExecDestroy(gx);
  if (g) hipGraphDestroy(g);
  WIS_RET(rc);
  { bool gave_up = false; WIS_RET(spin_gave_up(m, &gave_up)); if (gave_up) { set_error("wis_debug_timeline: the granule hand-off gave up during the tap"); return WIS_E_STATE; } }
  std::vector<unsigned long long> h((size_t)nk * 16);
  WIS_HIP_CHECK(hipMemcpy(h.data(), m->d_prof, h.size() * 8, hipMemcpyDeviceToHost));
  for (int k = 0; k < nk; ++k) { out[2 * k] = h[(size_t)k * 16 + 14]; out[2 * k + 1] = h[(size_t)k * 16 + 15]; }
  return WIS_OK;
}

int wis_bench_weight_stream(wis_model_t* m, int M, int passes, float* total_ms, int* launches_per_pass, double* bytes_per_pass) {
  if (!m || M < 1 || M > MAX_ROWS || passes < 1 || !total_ms) { set_error("wis_bench_weight_stream: bad argument"); return WIS_E_ARG; }
  WIS_ENTER(m, "wis_bench_weight_stream")
  WIS_HIP_CHECK(hipSetDevice(m->device));
  const int d = m->cfg.d_model; hipStream_t st = m->st;
  int launches = 0; double bytes = 0;
  const StepRoute rt = small_route(m, M);      // dec_forward's route at this row count
  const bool frag = rt.frag, ln16 = rt.ln16;
  // one projection alone, by the step's route, on zero rows (K = d: the layer input, K = 4d: the FFN hidden rows), into the logits buffer.  (ln16: every
  // LayerNorm-folded matrix reads the f16 rows here, cross-Q too - the step runs cross-Q inside the fused stage and has no such launch of its own)
  auto stream = [&](const DecProj& p, bool count) -> int {
    if (count) { ++launches; bytes += (double)p.N * p.K * (m->w8 ? 1 : 2); }
    const bool ln = p.csum != nullptr;
    if (frag) {
      GemvP g = gemv_frag(p, p.K == d ? m->dxf : m->dhxf, M, (ln ? GV_LN : 0) | GV_OUT_F32);
      g.y = m->logits; g.stat_in = m->dstat;
      return launch_gemv_frag(st, g);
    }
    if (ln && ln16) return launch_gemv(st, gemv_small(p, m->dxh, m->logits, M, GV_LN16 | GV_OUT_F32));
    return launch_gemv(st, gemv_small(p, ln ? (const void*)m->dx : (const void*)m->dh, m->logits, M, (ln ? GV_LN : 0) | GV_OUT_F32));
  };
  auto pass = [&](bool count) -> int {      // every layer's six matrices in step order, then the vocabulary projection
    for (const DecLayerW& w : m->dec) for (const DecProj* p : w.streamed()) WIS_RET(stream(*p, count));
    return stream(m->proj, count);
  };
  if (frag) {       // zero rows: fragment image of zeros (allocation state), partial sums of zeros
    WIS_HIP_CHECK(hipMemsetAsync(m->dxf, 0, xf_elems(d, MAX_ROWS / 16) * 2, st));
    WIS_HIP_CHECK(hipMemsetAsync(m->dhxf, 0, xf_elems(4 * d, MAX_ROWS / 16) * 2, st));
    WIS_HIP_CHECK(hipMemsetAsync(m->dstat, 0, (size_t)MAX_ROWS * (d / 16) * 2 * 4, st));
  }
  WIS_HIP_CHECK(hipMemsetAsync(m->dx, 0, (size_t)MAX_ROWS * d * 4, st));
  WIS_HIP_CHECK(hipMemsetAsync(m->dh, 0, (size_t)MAX_ROWS * 4 * d * 2, st));
  if (ln16) {
    WIS_HIP_CHECK(hipMemsetAsync(m->dxh, 0, (size_t)MAX_ROWS * d * 2, st));
    WIS_HIP_CHECK(hipMemsetAsync(m->dstat, 0, (size_t)MAX_ROWS * (d / 16) * 2 * 4, st));
  }
  WIS_RET(pass(true));   // warm-up pass (also counts launches / bytes)
  // the timed passes run the way the product runs these kernels: captured once into a HIP graph and replayed (wis_generate replays
  // its decode step as a graph); WIS_NO_GRAPH=1 (profilers that cannot follow a capture) falls back to eager launches
  hipGraph_t graph = nullptr; hipGraphExec_t gexec = nullptr;
  if (m->use_graph) {
    WIS_HIP_CHECK(hipStreamBeginCapture(st, hipStreamCaptureModeThreadLocal));
    const int rc = pass(false);
    const hipError_t e = hipStreamEndCapture(st, &graph);
    if (rc || e != hipSuccess) { if (graph) hipGraphDestroy(graph); if (rc) return rc; set_error("weight-stream tap: graph capture failed: %s", hipGetErrorString(e)); return WIS_E_HIP; }
    if (hipGraphInstantiate(&gexec, graph, nullptr, nullptr, 0) != hipSuccess) { hipGraphDestroy(graph); set_error("weight-stream tap: graph instantiate failed"); return WIS_E_HIP; }
    hipGraphDestroy(graph);
    if (hipGraphLaunch(gexec, st) != hipSuccess) { hipGraphExecDestroy(gexec); set_error("weight-stream tap: graph launch failed"); return WIS_E_HIP; }      // untimed first replay
  }
  int rc2 = WIS_OK;
  hipError_t e2 = hipEventRecord(m->ev[6], st);
  for (int i = 0; i < passes && !rc2 && e2 == hipSuccess; ++i) { if (gexec) e2 = hipGraphLaunch(gexec, st); else rc2 = pass(false); }
  if (e2 == hipSuccess) e2 = hipEventRecord(m->ev[7], st);
  if (e2 == hipSuccess) e2 = hipStreamSynchronize(st);
  if (gexec) hipGraphExecDestroy(gexec);
  WIS_RET(rc2);
  WIS_HIP_CHECK(e2);
  WIS_HIP_CHECK(hipEventElapsedTime(total_ms, m->ev[6], m->ev[7]));
  if (launches_per_pass) *launches_per_pass = launches;
  if (bytes_per_pass) *bytes_per_pass = bytes;
  return WIS_OK;
}

// ---- raw device helpers + single-kernel entry points -----------------------------------
int wis_dev_alloc(int device, size_t bytes, void** out) {
  DeviceCtx* c; WIS_RET(get_ctx(device, &c));
  WIS_HIP_CHECK(hipMalloc(out, bytes ? bytes : 16)); return WIS_OK;
}
int wis_dev_free(int device, void* p) { DeviceCtx* c; WIS_RET(get_ctx(device, &c)); WIS_HIP_CHECK(hipFree(p)); return WIS_OK; }
int wis_dev_h2d(int device, void* dst, const void* src, size_t bytes) { DeviceCtx* c; WIS_RET(get_ctx(device, &c)); WIS_HIP_CHECK(hipMemcpy(dst, src, bytes, hipMemcpyHostToDevice)); return WIS_OK; }
int wis_dev_d2h(int device, void* dst, const void* src, size_t bytes) { DeviceCtx* c; WIS_RET(get_ctx(device, &c)); WIS_HIP_CHECK(hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost)); return WIS_OK; }
int wis_dev_sync(int device) { DeviceCtx* c; WIS_RET(get_ctx(device, &c)); WIS_HIP_CHECK(hipDeviceSynchronize()); return WIS_OK; }
int wis_dev_copy_peer(int dst_device, void* dst, int src_device, const void* src, size_t bytes) {
  if (!dst || !src) { set_error("wis_dev_copy_peer: bad argument"); return WIS_E_ARG; }
  DeviceCtx* c; WIS_RET(get_ctx(src_device, &c)); WIS_RET(get_ctx(dst_device, &c));      // both devices exist; current = dst
  if (src_device != dst_device) {
    int can = 0;
    if (hipDeviceCanAccessPeer(&can, dst_device, src_device) == hipSuccess && can) {
      hipError_t e = hipDeviceEnablePeerAccess(src_device, 0);                            // direct xGMI path; already-enabled is fine
      if (e != hipSuccess && e != hipErrorPeerAccessAlreadyEnabled) (void)hipGetLastError();
    }
  }
  WIS_HIP_CHECK(hipMemcpyPeer(dst, dst_device, src, src_device, bytes));
  return WIS_OK;
}

int wis_op_gemm(int device, const void* A, int lda, const void* W, const float* bias, const float* residual, void* C, int M, int N, int K, int flags) {
  Tap t(device, "wis_op_gemm"); WIS_RET(t.rc);
  const GemmP g = gemm_plain(reinterpret_cast<const f16*>(A), lda, reinterpret_cast<const f16*>(W), M, N, K);
  if (flags & 8) {   // split-K = 2 path of the encoder's FFN2: requires bias, residual and fp32 output
    if (!bias || !residual || (flags & 7) != (2 | 4)) { set_error("wis_op_gemm: split-K needs bias, residual, flags 2|4|8"); return WIS_E_ARG; }
    float* scratch = nullptr;
    WIS_RET(t.get(&scratch, (size_t)2 * M * N));
    return t.finish(launch_gemm_splitk_resid(t.st, g, 2, scratch, bias, residual, reinterpret_cast<float*>(C)));
  }
  return t.finish(launch_gemm_generic(t.st, g, bias, residual, C, flags));
}
int wis_op_layernorm(int device, const float* x, const float* gamma, const float* beta, void* y, int M, int d) {
  Tap t(device, "wis_op_layernorm"); WIS_RET(t.rc);
  return t.finish(launch_layernorm(t.st, x, gamma, beta, reinterpret_cast<f16*>(y), M, d));
}
int wis_op_enc_attention(int device, const void* qk, const void* vt, void* out, int B, int T, int Tpad, int H) {
  Tap t(device, "wis_op_enc_attention"); WIS_RET(t.rc);
  // same rule as the encoder: the split-key form (two workgroups per query tile and head, in-launch merge) at small grids
  float* part = nullptr; unsigned* counters = nullptr;
  const size_t ncnt = (size_t)B * H * cdiv(T, 128);
  WIS_RET(t.get(&part, enc_attention_part_floats(B, T, H))); WIS_RET(t.get(&counters, ncnt, true));
  f16* qk2 = nullptr;      // the lazy-reference loop wants log2(e) on Q as well (the engine folds it into the projection): a scaled private copy
  if (enc_attn_lazy()) {
    const size_t n = (size_t)B * T * 2 * H * 64;
    WIS_RET(t.get(&qk2, n));
    hipMemcpyAsync(qk2, qk, n * 2, hipMemcpyDeviceToDevice, t.st);
    launch_scale_q_log2e(t.st, qk2, (int64_t)B * T, H * 64);
  }
  return t.finish(launch_enc_attention(t.st, qk2 ? qk2 : reinterpret_cast<const f16*>(qk), reinterpret_cast<const f16*>(vt), reinterpret_cast<f16*>(out), B, T, Tpad, H, part, counters, ncnt));
}
int wis_op_enc_attention_ex(int device, const void* qk, const void* vt, void* out, int B, int T, int Tpad, int H, int form) {
  Tap t(device, "wis_op_enc_attention_ex"); WIS_RET(t.rc);
  if (form & ~3) { set_error("wis_op_enc_attention_ex: form=%d (bit 0: lazy loop, bit 1: split-key pair)", form); return WIS_E_ARG; }
  const bool lazy = form & 1, split = form & 2;
  if (B < 1 || T < 1 || H < 1) { set_error("wis_op_enc_attention_ex: B=%d T=%d H=%d", B, T, H); return WIS_E_ARG; }
  if (split && cdiv(T, 64) < 4) { set_error("wis_op_enc_attention_ex: the split-key pair needs at least four key tiles (T=%d)", T); return WIS_E_ARG; }
  // Q is read as given (the lazy loop's log2(e) / 8 is the caller's, as the engine's query projection delivers it): no scaled copy
  float* part = nullptr; unsigned* counters = nullptr;
  if (split) { WIS_RET(t.get(&part, enc_attention_part_floats(B, T, H))); WIS_RET(t.get(&counters, (size_t)B * H * cdiv(T, 128), true)); }
  return t.finish(launch_enc_attention_form(t.st, reinterpret_cast<const f16*>(qk), reinterpret_cast<const f16*>(vt), reinterpret_cast<f16*>(out), B, T, Tpad, H, part, counters, lazy, split));
}
int wis_op_gemv(int device, const void* x, const float* gamma, const float* beta, const void* W, const float* bias, void* y, int M, int N, int K, int flags) {
  Tap t(device, "wis_op_gemv"); WIS_RET(t.rc);
  hipStream_t st = t.st;
  if (flags & GV_QKV) { set_error("wis_op_gemv: flag 16 is internal"); return WIS_E_ARG; }
  const int rows = gemv_rows_for(N, K), Npad = cdiv(N, rows) * rows;
  // (tap flags: 32 = quantise the matrix to 8 bits per weight first; 64 = GV_LN16: x is the F16 copy of the rows, LayerNorm folded)
  const bool w8 = flags & 32, ln16 = (flags & GV_LN16) != 0, ln = (flags & GV_LN) || ln16;
  flags &= ~32;
  if (ln16 && ((flags & GV_LN) || M > 8 || w8)) { set_error("wis_op_gemv: flag 64 (LayerNorm fold on f16 rows): <= 8 rows, f16 weights, without flag 8"); return WIS_E_ARG; }
  if (ln && (!gamma || !beta)) { set_error("wis_op_gemv: flags 8 / 64 need gamma and beta"); return WIS_E_ARG; }
  // the same preparation the model loader does: optional LayerNorm fold into a private copy of W / bias, then packing
  f16 *wp = nullptr, *wtmp = nullptr, *xfr = nullptr; float *wsc = nullptr, *b2 = nullptr, *cs = nullptr, *stt = nullptr;
  WIS_RET(t.get(&wp, (size_t)Npad * K)); WIS_RET(t.get(&wtmp, (size_t)N * K)); WIS_RET(t.get(&b2, (size_t)Npad, true)); WIS_RET(t.get(&cs, (size_t)Npad, true));
  if (w8) WIS_RET(t.get(&wsc, (size_t)Npad));      // (allocated for the 8-bit form only)
  hipMemcpyAsync(wtmp, W, (size_t)N * K * 2, hipMemcpyDeviceToDevice, st);
  if (bias) hipMemcpyAsync(b2, bias, (size_t)N * 4, hipMemcpyDeviceToDevice, st);
  WIS_RET(prep_projection(st, wtmp, N, Npad, K, 0, 1.f, ln ? gamma : nullptr, beta, b2, cs, wp, wsc, rows));
  GemvP g; memset(&g, 0, sizeof(g));
  g.x = x; g.csum = ln ? cs : nullptr; g.Wp = wp; g.wscale = wsc; g.bias = (bias || ln) ? b2 : nullptr; g.y = y; g.M = M; g.N = N; g.K = K; g.flags = flags; g.rows = rows;
  if (M <= 8) return t.finish(launch_gemv(st, g));
  // the product's batched route (dec_forward_frag): activations as a fragment image, LayerNorm statistics as row partials
  const int MBf = cdiv(M, 16);
  WIS_RET(t.get(&xfr, xf_elems(K, MBf), true));
  if (ln) WIS_RET(t.get(&stt, (size_t)M * (K / 16) * 2));
  WIS_RET(launch_xf_pack(st, x, ln ? 0 : 1, xfr, ln ? stt : nullptr, M, K, MBf));
  g.x = xfr; g.xmb = MBf; g.stat_in = stt;
  // a K = 4d projection on f16 rows (FFN2) asks for dec_forward_frag's K split (ffn2_ksplit: two slices unless WIS_FRAG_KSPLIT says otherwise).  As in the
  // step, launch_gemv_frag honours it only at one row block (<= 16 rows: gemv_frag_kernel, grid.y = slices, merged in the launch); from 17 rows on and up to
  // 85 n-tiles it runs gemv_frag_ms_kernel (row-block groups, no K split) instead.  Other slice counts: wis_op_gemv_frag_stage.
  const int ks = (!ln && K >= 4096) ? ffn2_ksplit(K) : 1;
  if (ks > 1) {
    const size_t nt = (size_t)cdiv(N, 16);
    float* part = nullptr; unsigned* cnt = nullptr;
    WIS_RET(t.get(&part, nt * ks * MBf * 64 * 4)); WIS_RET(t.get(&cnt, nt, true));
    frag_set_ksplit(g, ks, part, cnt);
    if (!(flags & GV_RESID)) WIS_RET(launch_gemv_frag(st, g));      // a first launch on the same tickets: they must re-arm themselves
  }
  return t.finish(launch_gemv_frag(st, g));
}

// One projection stage of the batched route, assembled by dec_forward_frag's own builders (model.hip frag_resid / frag_ln_gelu_xf / frag_ln_f32) on a matrix
// prepared as the loader prepares it; launch_gemv_frag picks the kernel.  include/wis_hip.h has the contract.  Nothing but the stage's outputs is written.
int wis_op_gemv_frag_stage(int device, int stage, const void* x, int x_is_image, int xmb, const float* stat_in, const float* gamma, const float* beta,
                           const void* W_f16, const float* bias, int w8, float* y, void* y_xf, float* stat_out, int M, int N, int K, int ksplit) {
  Tap t(device, "wis_op_gemv_frag_stage"); WIS_RET(t.rc);
  hipStream_t st = t.st;
  const bool ln = stage == 1 || stage == 2;
  if (stage < 0 || stage > 2 || !x || !W_f16 || !bias || (ln && (!gamma || !beta)) || (stage != 1 && !y) || (stage == 1 && !y_xf) || (x_is_image && ln && !stat_in) ||
      M < 1 || M > 8 * MAX_ROWS || N < 4 || K < 32 || K % 32 || ksplit < -1 || ksplit == 0 || ksplit > 8 || xmb < 0 || (xmb && !x_is_image)) {
    set_error("wis_op_gemv_frag_stage: bad argument"); return WIS_E_ARG;
  }
  const int Npad = cdiv(N, 16) * 16, MB = xmb ? xmb : cdiv(M, 16);
  f16 *wp = nullptr, *wtmp = nullptr, *xfr = nullptr; float *wsc = nullptr, *b2 = nullptr, *cs = nullptr, *stt = nullptr;
  WIS_RET(t.get(&wp, (size_t)Npad * K)); WIS_RET(t.get(&wtmp, (size_t)N * K)); WIS_RET(t.get(&b2, (size_t)Npad, true)); WIS_RET(t.get(&cs, (size_t)Npad, true));
  if (w8) WIS_RET(t.get(&wsc, (size_t)Npad));
  hipMemcpyAsync(wtmp, W_f16, (size_t)N * K * 2, hipMemcpyDeviceToDevice, st);
  hipMemcpyAsync(b2, bias, (size_t)N * 4, hipMemcpyDeviceToDevice, st);
  WIS_RET(prep_projection(st, wtmp, N, Npad, K, 0, 1.f, ln ? gamma : nullptr, beta, b2, cs, wp, wsc, 16));
  const DecProj proj{wp, wsc, b2, ln ? cs : nullptr, N, K, 16};
  const f16* xf = reinterpret_cast<const f16*>(x);
  if (!x_is_image) {      // row-major rows (fp32 behind a LayerNorm, else f16) -> fragment image (+ partials), as wis_op_gemv does
    WIS_RET(t.get(&xfr, xf_elems(K, MB), true));
    if (ln) WIS_RET(t.get(&stt, (size_t)M * (K / 16) * 2));
    WIS_RET(launch_xf_pack(st, x, ln ? 0 : 1, xfr, stt, M, K, MB));
    xf = xfr; stat_in = stt;
  }
  GemvP g = stage == 0 ? frag_resid(proj, xf, y, reinterpret_cast<f16*>(y_xf), stat_out, M)
          : stage == 1 ? frag_ln_gelu_xf(proj, xf, stat_in, reinterpret_cast<f16*>(y_xf), M) : frag_ln_f32(proj, xf, stat_in, y, M);
  if (xmb) g.xmb = xmb;      // (a ready image of another row-block count: launch_gemv_frag's answer)
  const int ks = ksplit < 0 ? (stage == 0 ? ffn2_ksplit(K) : 1) : ksplit;
  if (ks > 1) {
    // two launches on one set of tickets (they must re-arm themselves); the residual rows are put back in between
    const size_t nt = (size_t)cdiv(N, 16);
    float *part = nullptr, *y0 = nullptr; unsigned* cnt = nullptr;
    WIS_RET(t.get(&part, nt * ks * MB * 64 * 4)); WIS_RET(t.get(&cnt, nt, true));
    frag_set_ksplit(g, ks, part, cnt);
    if (stage == 0) { WIS_RET(t.get(&y0, (size_t)M * N)); hipMemcpyAsync(y0, y, (size_t)M * N * 4, hipMemcpyDeviceToDevice, st); }
    WIS_RET(launch_gemv_frag(st, g));
    if (stage == 0) hipMemcpyAsync(y, y0, (size_t)M * N * 4, hipMemcpyDeviceToDevice, st);
  }
  return t.finish(launch_gemv_frag(st, g));
}

// The two embedding launches of the step on the caller's tables: launch_dec_embed_xf (xf given: x, the rows' fragment image of ceil(M / 16) row blocks and
// their partials - the batched route) or launch_dec_embed (x and, optionally, the f16 copy xh).  tok / pos are HOST arrays, range-checked here.
int wis_op_dec_embed(int device, const void* emb_f16, const void* pos_f16, const int32_t* tok, const int32_t* pos, float* x, void* xh_f16, void* xf_f16, float* stat,
                     int M, int d, int n_vocab, int n_ctx) {
  Tap t(device, "wis_op_dec_embed"); WIS_RET(t.rc);
  if (!emb_f16 || !pos_f16 || !tok || !pos || !x || M < 1 || M > MAX_ROWS || d < 32 || d % 32 || n_vocab < 1 || n_ctx < 1 || (xf_f16 ? (!stat || xh_f16 != nullptr) : stat != nullptr)) {
    set_error("wis_op_dec_embed: bad argument"); return WIS_E_ARG;
  }
  for (int r = 0; r < M; ++r) if (tok[r] < 0 || tok[r] >= n_vocab || pos[r] < 0 || pos[r] >= n_ctx) { set_error("wis_op_dec_embed: row %d: token %d / position %d out of range", r, tok[r], pos[r]); return WIS_E_ARG; }
  int *d_tok = nullptr, *d_pos = nullptr;
  WIS_RET(t.get(&d_tok, (size_t)M)); WIS_RET(t.get(&d_pos, (size_t)M));
  WIS_HIP_CHECK(hipMemcpy(d_tok, tok, (size_t)M * 4, hipMemcpyHostToDevice)); WIS_HIP_CHECK(hipMemcpy(d_pos, pos, (size_t)M * 4, hipMemcpyHostToDevice));
  const f16 *e = reinterpret_cast<const f16*>(emb_f16), *pe = reinterpret_cast<const f16*>(pos_f16);
  if (xf_f16) return t.finish(launch_dec_embed_xf(t.st, e, pe, d_tok, d_pos, x, reinterpret_cast<f16*>(xf_f16), stat, M, d, cdiv(M, 16)));
  return t.finish(launch_dec_embed(t.st, e, pe, d_tok, d_pos, x, M, d, reinterpret_cast<f16*>(xh_f16)));
}

// The single-chunk f16-activation form of launch_gemv (the one-utterance FFN2 and cross-attention out-projection: K = 5120 / 1280) on sixteen-column
// tiles (cols = 16: the fragment image) or eight-column tiles (cols = 8: launch_pack_gemv_nc8's image) of the same row-major W [N][K].  flags: GV_RESID
// (y fp32 [M][N] in place, y16 an optional f16 copy), GV_OUT_F32, GV_GELU or none (y f16).  Nothing but the M x N outputs is written.
// cols = 5: the stage as the step assembles it (gemv_small) for a projection that carries the sixteen-column image (tap flag 32: the matrix quantised to 8 bits
// first, as wis_op_gemv's) and - packed by the loader's launcher, where the loader would add one - the five-column image: gemv_small's predicate picks the
// form, so a shape it refuses (N no multiple of five, more rows than the register staging holds, 8-bit weights) runs the sixteen-column kernel.
static int op_gemv_cols5(Tap& t, const void* x, const void* W, const float* bias, void* y, void* y16, int M, int N, int K, int flags, bool w8) {
  const int Npad = cdiv(N, 16) * 16;
  f16 *wp = nullptr, *wrow = nullptr, *wp5 = nullptr; float *wsc = nullptr, *b2 = nullptr;
  WIS_RET(t.get(&wp, (size_t)Npad * K)); WIS_RET(t.get(&wrow, (size_t)N * K)); WIS_RET(t.get(&b2, (size_t)Npad, true));
  if (w8) WIS_RET(t.get(&wsc, (size_t)Npad));
  hipMemcpyAsync(wrow, W, (size_t)N * K * 2, hipMemcpyDeviceToDevice, t.st);
  if (bias) hipMemcpyAsync(b2, bias, (size_t)N * 4, hipMemcpyDeviceToDevice, t.st);
  WIS_RET(prep_projection(t.st, wrow, N, Npad, K, 0, 1.f, nullptr, nullptr, b2, nullptr, wp, wsc, 16));
  DecProj proj{wp, wsc, bias ? b2 : nullptr, nullptr, N, K, 16};
  if (!w8 && gemv_nc5_shape(1, N, K, flags)) {
    WIS_RET(t.get(&wp5, gemv_nc5_elems(N, K, 40)));
    WIS_RET(launch_pack_gemv_nc5(t.st, wrow, wp5, N, K, 40));
    proj.Wp5 = wp5;
  }
  GemvP g = gemv_small(proj, x, y, M, flags);
  g.y16 = reinterpret_cast<f16*>(y16);
  return t.finish(launch_gemv(t.st, g));
}
int wis_op_gemv_cols(int device, const void* x, const void* W, const float* bias, void* y, void* y16, int M, int N, int K, int flags, int cols) {
  Tap t(device, "wis_op_gemv_cols"); WIS_RET(t.rc);
  const bool w8 = cols == 5 && (flags & 32);      // (tap flag, cols = 5 only)
  if (w8) flags &= ~32;
  if (!x || !W || !y || (cols != 5 && cols != 8 && cols != 16) || N < 1 || (cols != 5 && N % cols) || (flags & ~(GV_RESID | GV_OUT_F32 | GV_GELU)) || (y16 && !(flags & GV_RESID))) { set_error("wis_op_gemv_cols: bad argument"); return WIS_E_ARG; }
  if (cols == 5) {
    if (M < 1 || M > 16 || K < 128 || K % 128) { set_error("wis_op_gemv_cols: M=%d K=%d", M, K); return WIS_E_ARG; }
    return op_gemv_cols5(t, x, W, bias, y, y16, M, N, K, flags, w8);
  }
  if (!gemv_nc8_shape(M, N, K)) { set_error("wis_op_gemv_cols: M=%d N=%d K=%d is not a shape of the eight-column form", M, N, K); return WIS_E_UNSUPPORTED; }
  f16* wp = nullptr;
  WIS_RET(t.get(&wp, (size_t)N * K));
  WIS_RET(cols == 8 ? launch_pack_gemv_nc8(t.st, reinterpret_cast<const f16*>(W), wp, N, N, K) : launch_pack_gemv(t.st, reinterpret_cast<const f16*>(W), wp, N, N, K, 0, 1.f, 16));
  GemvP g; memset(&g, 0, sizeof(g));
  g.x = x; g.Wp = wp; g.bias = bias; g.y = y; g.y16 = reinterpret_cast<f16*>(y16); g.M = M; g.N = N; g.K = K; g.flags = flags; g.rows = cols;
  return t.finish(launch_gemv(t.st, g));
}

// wis_op_dec_self_attn is the nb = 8, row-major, no-tree case of wis_op_dec_self_attn_ex; `who` is the entry point the caller used
static int op_dec_self_attn(const char* who, int device, const float* q, const void* kc, const void* vc, const int32_t* pos, void* out,
                            int M, int H, int ctx, int rpu, int sstride, int rmul, int nb, int out_mb, const int32_t* anc, int w0, int aw, const int32_t* base) {
  Tap t(device, who); WIS_RET(t.rc);
  if (!q || !kc || !vc || !pos || !out || M < 1 || H < 1 || rpu < 1 || (nb != 2 && nb != 4 && nb != 8) || (out_mb && out_mb < cdiv(M, 16)) || (base && !anc)) {
    set_error("%s: bad argument", who); return WIS_E_ARG; }
  const int d = 64 * H;
  if (out_mb) WIS_HIP_CHECK(hipMemsetAsync(out, 0, xf_elems(d, out_mb) * 2, t.st));      // the fragment image's rows beyond M stay zero
  SelfAttnP sa;
  sa.q = q; sa.kc = reinterpret_cast<const f16*>(kc); sa.vc = reinterpret_cast<const f16*>(vc); sa.pos = pos; sa.out = reinterpret_cast<f16*>(out);
  sa.M = M; sa.H = H; sa.d = d; sa.ctx = ctx; sa.rpu = rpu; sa.sstride = sstride; sa.rmul = rmul; sa.out_mb = out_mb; sa.anc = anc; sa.w0 = w0; sa.aw = aw; sa.base = base; sa.nb = nb;
  return t.finish(launch_dec_self_attn(t.st, sa));
}
int wis_op_dec_self_attn(int device, const float* q, const void* kc, const void* vc, const int32_t* pos, void* out,
                         int M, int H, int ctx, int rpu, int sstride, int rmul) {
  return op_dec_self_attn("wis_op_dec_self_attn", device, q, kc, vc, pos, out, M, H, ctx, rpu, sstride, rmul, 8, 0, nullptr, 0, 0, nullptr);
}
int wis_op_dec_self_attn_ex(int device, const float* q, const void* kc, const void* vc, const int32_t* pos, void* out,
                            int M, int H, int ctx, int rpu, int sstride, int rmul, int nb, int out_mb,
                            const int32_t* anc, int w0, int aw, const int32_t* base) {
  return op_dec_self_attn("wis_op_dec_self_attn_ex", device, q, kc, vc, pos, out, M, H, ctx, rpu, sstride, rmul, nb, out_mb, anc, w0, aw, base);
}
// the long-prompt route's step kernel (launch_dec_self_attn_long, through the launch function the decoder forward calls: SelfAttnP::plen)
int wis_op_dec_self_attn_long(int device, const float* q, const void* kc, const void* vc, const int32_t* pos, const int32_t* plen, void* out,
                              int B, int k, int H, int ctx, int out_mb) {
  Tap t(device, "wis_op_dec_self_attn_long"); WIS_RET(t.rc);
  if (!q || !kc || !vc || !pos || !plen || !out || B < 1 || H < 1 || k < 1 || k > MAX_R || (out_mb && out_mb < cdiv(B * k, 16))) { set_error("wis_op_dec_self_attn_long: bad argument"); return WIS_E_ARG; }
  const int d = 64 * H;
  if (out_mb) WIS_HIP_CHECK(hipMemsetAsync(out, 0, xf_elems(d, out_mb) * 2, t.st));      // the fragment image's rows beyond B k stay zero
  SelfAttnP sa;
  sa.q = q; sa.kc = reinterpret_cast<const f16*>(kc); sa.vc = reinterpret_cast<const f16*>(vc); sa.pos = pos; sa.out = reinterpret_cast<f16*>(out);
  sa.M = B * k; sa.H = H; sa.d = d; sa.ctx = ctx; sa.rpu = k; sa.sstride = k; sa.rmul = 1; sa.out_mb = out_mb; sa.plen = plen;
  return t.finish(launch_dec_self_attn(t.st, sa));
}
static int op_dec_cross_attn(int device, const float* q, const float* xres, const float* qcs, const float* qb, const void* kx, const void* vt, void* out,
                             int B, int R, int H, int T, int chunks, const float* q2 = nullptr, int xres_is_stat = 0, int out_mb = 0, int kv_shared = 0, bool no_spin = false) {
  Tap t(device, "wis_op_dec_cross_attn"); WIS_RET(t.rc);
  if (!q || !kx || !vt || !out || B < 1 || H < 1 || T < 1) { set_error("wis_op_dec_cross_attn: bad argument"); return WIS_E_ARG; }
  if (out_mb && out_mb < cdiv(B * R, 16)) { set_error("wis_op_dec_cross_attn: %d row blocks for %d rows", out_mb, B * R); return WIS_E_ARG; }
  hipStream_t st = t.st;
  const bool small = B * H <= CA_SPIN_MAX_BH && !no_spin;      // the product's rule: the granule hand-off on small grids (launch_dec_cross_attn decides by chunking / rows)
  CrossAttnP ca;
  WIS_RET(t.get(&ca.part, (size_t)B * H * 16 * 16 * 66)); WIS_RET(t.get(&ca.counters, (size_t)B * H, true));
  if (small) { WIS_RET(t.get(&ca.gran, (size_t)B * H * 6 * 8 * 66, true)); WIS_RET(t.get(&ca.epoch, (size_t)B * H + 1, true)); }
  if (out_mb) hipMemsetAsync(out, 0, xf_elems(64 * H, out_mb) * 2, st);      // the fragment image's rows beyond B * R stay zero
  ca.q = q; ca.kx = reinterpret_cast<const f16*>(kx); ca.vt = reinterpret_cast<const f16*>(vt); ca.out = reinterpret_cast<f16*>(out);
  ca.B = B; ca.R = R; ca.H = H; ca.d = 64 * H; ca.T = T; ca.Tpad = cdiv(T, 64) * 64; ca.chunks = chunks; ca.out_mb = out_mb; ca.xres = xres; ca.qcs = qcs; ca.qb = qb;
  ca.q2 = q2; ca.xres_is_stat = xres_is_stat; ca.kv_shared = kv_shared;
  int rc = WIS_OK;
  for (int rep = 0; rep < 3 && !rc; ++rep) rc = launch_dec_cross_attn(st, ca);      // three launches: the epochs of the granule form advance from launch to launch
  unsigned flag = 0;
  if (small && !rc) hipMemcpyAsync(&flag, ca.epoch, 4, hipMemcpyDeviceToHost, st);
  const int verdict = t.finish(rc);      // (synchronises: flag has arrived)
  if (!rc && flag) { set_error("wis_op_dec_cross_attn: granule hand-off timed out"); return WIS_E_HIP; }
  return verdict;
}
int wis_op_dec_cross_attn(int device, const float* q, const void* kx, const void* vt, void* out, int B, int R, int H, int T, int chunks) {
  return op_dec_cross_attn(device, q, nullptr, nullptr, nullptr, kx, vt, out, B, R, H, T, chunks);
}
int wis_op_dec_cross_attn_folded(int device, const float* q_raw, const float* xres, const float* qcs, const float* qb, const void* kx, const void* vt, void* out,
                                 int B, int R, int H, int T, int chunks) {
  if (!xres || !qcs || !qb) { set_error("wis_op_dec_cross_attn_folded: bad argument"); return WIS_E_ARG; }
  return op_dec_cross_attn(device, q_raw, xres, qcs, qb, kx, vt, out, B, R, H, T, chunks);
}
int wis_op_dec_cross_attn_stat(int device, const float* q, const float* q2, const float* stat, const float* qcs, const float* qb, const void* kx, const void* vt, void* out,
                               int B, int R, int H, int T, int chunks, int out_mb, int kv_shared, int no_spin) {
  if (stat ? (!qcs || !qb) : (qcs || qb || q2)) { set_error("wis_op_dec_cross_attn_stat: the fold takes partials, column sums and bias together; the plain form none of them"); return WIS_E_ARG; }
  return op_dec_cross_attn(device, q, stat, qcs, qb, kx, vt, out, B, R, H, T, chunks, q2, stat ? 1 : 0, out_mb, kv_shared, no_spin != 0);
}

int wis_op_gemv_qkv(int device, const float* x, const float* gamma, const float* beta, const void* W, const float* bias, const int32_t* slot, const int32_t* pos,
                    float* q, void* kc, void* vc, int M, int d, int ctx) {
  Tap t(device, "wis_op_gemv_qkv"); WIS_RET(t.rc);
  if (!x || !gamma || !beta || !W || !bias || !slot || !pos || !q || !kc || !vc || M < 1 || M > MAX_ROWS || d < 128 || d % 128 || ctx < 1) { set_error("wis_op_gemv_qkv: bad argument"); return WIS_E_ARG; }
  hipStream_t st = t.st;
  const int N = 3 * d, MB = cdiv(M, 16);
  const float qs = 0.125f;
  f16 *wp = nullptr, *wtmp = nullptr, *xf = nullptr; float *b2 = nullptr, *cs = nullptr, *stt = nullptr;
  WIS_RET(t.get(&wp, (size_t)N * d)); WIS_RET(t.get(&wtmp, (size_t)N * d)); WIS_RET(t.get(&b2, (size_t)N)); WIS_RET(t.get(&cs, (size_t)N, true));
  if (M > 8) { WIS_RET(t.get(&xf, xf_elems(d, MB), true)); WIS_RET(t.get(&stt, (size_t)M * (d / 16) * 2)); }
  // what load_weights does for a layer's DecProj `qkv` (w.qkv): the bias's query part scaled, the LayerNorm folded, the query rows scaled by the packer
  hipMemcpyAsync(wtmp, W, (size_t)N * d * 2, hipMemcpyDeviceToDevice, st);
  launch_convert(st, bias, 0, b2, 0, N, 1, 1, d, qs);
  const DecProj qkv{wp, nullptr, b2, cs, N, d, gemv_rows_for(N, d)};
  WIS_RET(prep_projection(st, wtmp, N, N, d, d, qs, gamma, beta, b2, cs, wp, nullptr, qkv.rows));
  GemvP g;
  if (M <= 8) g = gemv_small(qkv, x, nullptr, M, GV_LN | GV_QKV);      // dec_forward
  else {
    // dec_forward_frag: the rows as a fragment image, their LayerNorm statistics as row partials
    WIS_RET(launch_xf_pack(st, x, 0, xf, stt, M, d, MB));
    g = gemv_frag(qkv, xf, M, GV_LN | GV_QKV);
    g.stat_in = stt;
  }
  g.q = q; g.kc = reinterpret_cast<f16*>(kc); g.vc = reinterpret_cast<f16*>(vc); g.slot = slot; g.pos = pos; g.d = d; g.ctx = ctx;
  return t.finish(M <= 8 ? launch_gemv(st, g) : launch_gemv_frag(st, g));
}

int wis_op_wave_sums(int device, const float* x, int N, float* out_old, float* out_new) {
  Tap t(device, "wis_op_wave_sums"); WIS_RET(t.rc);
  if (!x || !out_old || !out_new || (N != 6 && N != 10 && N != 16)) { set_error("wis_op_wave_sums: N=%d (6, 10 or 16 values per lane)", N); return WIS_E_ARG; }
  if (N == 6) hipLaunchKernelGGL((wave_sums_tap_kernel<6>), dim3(1), dim3(64), 0, t.st, x, out_old, out_new);
  else if (N == 10) hipLaunchKernelGGL((wave_sums_tap_kernel<10>), dim3(1), dim3(64), 0, t.st, x, out_old, out_new);
  else hipLaunchKernelGGL((wave_sums_tap_kernel<16>), dim3(1), dim3(64), 0, t.st, x, out_old, out_new);
  return t.finish(WIS_OK);
}

int wis_op_gemv_out_cq(int device, const void* a, const float* x0, const void* Wo, const float* bo, const void* Wq, const float* bq, const float* gamma, const float* beta,
                       float* x1, float* stat, float* q, float* q2, float* qcs, float* qb, int M, int d, int force_frag) {
  Tap t(device, "wis_op_gemv_out_cq"); WIS_RET(t.rc);
  const bool frag = M > 8 || force_frag;
  if (!a || !x0 || !Wo || !bo || !Wq || !bq || !gamma || !beta || !x1 || !stat || !q || !qcs || !qb || (frag && !q2) || M < 1 || M > MAX_ROWS || d < 128 || d % 128) {
    set_error("wis_op_gemv_out_cq: bad argument"); return WIS_E_ARG; }
  hipStream_t st = t.st;
  const int MB = cdiv(M, 16);
  const float qs = 0.125f;
  f16 *wtmp = nullptr, *fcat = nullptr, *fwot = nullptr, *fwqo = nullptr, *p_cqo = nullptr, *p_out = nullptr, *xh = nullptr, *xf = nullptr, *af = nullptr; float* b_cqo = nullptr;
  WIS_RET(t.get(&wtmp, (size_t)d * d)); WIS_RET(t.get(&fcat, (size_t)2 * d * d)); WIS_RET(t.get(&fwot, (size_t)d * d)); WIS_RET(t.get(&fwqo, (size_t)d * d));
  WIS_RET(t.get(&p_cqo, (size_t)2 * d * d)); WIS_RET(t.get(&p_out, (size_t)d * d)); WIS_RET(t.get(&b_cqo, (size_t)d));
  if (frag) { WIS_RET(t.get(&xf, xf_elems(d, MB), true)); WIS_RET(t.get(&af, xf_elems(d, MB), true)); }
  else WIS_RET(t.get(&xh, (size_t)M * d));
  // load_weights, decoder layer: cq (the cross-Q bias scaled, the LayerNorm folded: bias / csum are what the cross-attention kernel takes as qb / qcs), out, then the fold
  hipMemcpyAsync(wtmp, Wq, (size_t)d * d * 2, hipMemcpyDeviceToDevice, st);
  launch_convert(st, bq, 0, qb, 0, d, 1, 1, d, qs);
  hipMemsetAsync(qcs, 0, (size_t)d * 4, st);
  DecLayerW w{};
  w.out = DecProj{p_out, nullptr, bo, nullptr, d, d, gemv_rows_for(d, d)};
  w.cqo = DecProj{p_cqo, nullptr, b_cqo, nullptr, d, 2 * d, 16};
  WIS_RET(prep_projection(st, wtmp, d, d, d, d, qs, gamma, beta, qb, qcs, nullptr, nullptr, 16));      // (the fold alone: the stage streams w.out and w.cqo)
  WIS_RET(launch_pack_gemv(st, reinterpret_cast<const f16*>(Wo), p_out, d, d, d, 0, 1.f, w.out.rows));
  WIS_RET(build_cq_fold(st, wtmp, Wo, 1, bo, d, qs, fcat, fwot, fwqo, p_cqo, b_cqo));
  if (out_cq_nc8_shape(1, d)) {      // ... and the eight-column image where the loader adds one (out_cq_dual picks it)
    f16* p8 = nullptr;
    WIS_RET(t.get(&p8, (size_t)2 * d * d));
    WIS_RET(launch_pack_gemv_nc8(st, fcat, p8, d, d, 2 * d));
    w.cqo.Wp8 = p8;
  }
  hipMemcpyAsync(x1, x0, (size_t)M * d * 4, hipMemcpyDeviceToDevice, st);      // the residual epilogue works in place
  if (!frag) {
    // dec_forward: one dual launch on the f16 rows (the attention output; the f16 copy of the layer input that the embedding / FFN2 epilogues leave)
    launch_convert(st, x0, 0, xh, 1, M, d, d, 0, 1.f);
    GemvP ga, gb;
    out_cq_dual(w, reinterpret_cast<const f16*>(a), xh, x1, stat, q, M, &ga, &gb);
    return t.finish(launch_gemv_dual(st, ga, gb));
  }
  // dec_forward_frag: three d x d problems on the fragment images of the layer input and the attention output
  WIS_RET(launch_xf_pack(st, x0, 0, xf, nullptr, M, d, MB));
  WIS_RET(launch_xf_pack(st, a, 1, af, nullptr, M, d, MB));
  GemvP g3[3];
  out_cq_frag3(w, af, xf, x1, stat, q, q2, M, g3);
  return t.finish(launch_gemv_frag3(st, g3, 3));
}

// ---- taps of what run_encoder / run_cross_kv launch (tests/test_gpu_enc_ops.py): the product's launch_* functions on the product's GemmP helpers
// (conv1_gemm, conv2_gemm, gemm_plain) and weight packers, with free B and T; the tile and kernel form are gemm_pick_tile's / launch_gemm_t's choice
int wis_op_mel_to_image(int device, const float* mel, void* img_f16, int B, int n_mels) {
  Tap t(device, "wis_op_mel_to_image"); WIS_RET(t.rc);
  if (!mel || !img_f16 || B < 1) { set_error("wis_op_mel_to_image: bad argument"); return WIS_E_ARG; }
  return t.finish(launch_mel_to_image(t.st, mel, reinterpret_cast<f16*>(img_f16), B, n_mels));
}
int wis_op_enc_conv(int device, int which, const void* img_f16, const void* W, int w_is_f16, const float* bias, const float* pos, void* out,
                    int B, int T, int Cin, int N) {
  Tap t(device, "wis_op_enc_conv"); WIS_RET(t.rc);
  if (!img_f16 || !W || !bias || !out || B < 1 || T < 1 || N < 128 || (which != 1 && which != 2) || (which == 2 && !pos) || (int64_t)B * (2 * (int64_t)T + 2) > 0x7fffffff) {
    set_error("wis_op_enc_conv: bad argument"); return WIS_E_ARG; }
  if (which == 1 ? !mel_bins_supported(Cin) : (Cin < 64 || Cin % 64)) { set_error("wis_op_enc_conv: conv%d with %d input channels", which, Cin); return WIS_E_UNSUPPORTED; }
  f16* wp = nullptr;
  WIS_RET(t.get(&wp, (size_t)N * (which == 1 ? conv1_k(Cin) : 3 * Cin)));
  if (which == 1) {
    pack_conv1_w(t.st, W, w_is_f16, wp, N, Cin);
    return t.finish(launch_gemm_conv1(t.st, conv1_gemm(reinterpret_cast<const f16*>(img_f16), wp, B, T, Cin, N), bias, reinterpret_cast<f16*>(out), T));
  }
  pack_conv2_w(t.st, W, w_is_f16, wp, N, Cin);
  return t.finish(launch_gemm_conv2(t.st, conv2_gemm(reinterpret_cast<const f16*>(img_f16), wp, B, T, Cin, N), bias, pos, reinterpret_cast<float*>(out), T));
}
int wis_op_enc_qkv(int device, const void* xn_f16, const void* W_f16, const float* bias, void* qk_f16, void* vt_f16, int B, int T, int H) {
  Tap t(device, "wis_op_enc_qkv"); WIS_RET(t.rc);
  if (!xn_f16 || !W_f16 || !bias || !qk_f16 || !vt_f16 || B < 1 || T < 1 || H < 1 || (int64_t)B * T > 0x7fffffff / (3 * 64 * (int64_t)H)) { set_error("wis_op_enc_qkv: bad argument"); return WIS_E_ARG; }
  if (T % 4) { set_error("wis_op_enc_qkv: T = %d (the transposed V tiles store 4 consecutive keys of one utterance: T %% 4 == 0)", T); return WIS_E_ARG; }
  const int d = 64 * H;
  return t.finish(launch_gemm_qkv(t.st, gemm_plain(reinterpret_cast<const f16*>(xn_f16), d, reinterpret_cast<const f16*>(W_f16), B * T, 3 * d, d), bias,
                                  reinterpret_cast<f16*>(qk_f16), reinterpret_cast<f16*>(vt_f16), d, T, cdiv(T, 64) * 64, H));
}
int wis_op_enc_crosskv(int device, const void* mem_f16, const void* W_f16, const float* bias, void* kx_f16, void* vt_f16, int B, int T, int H, int L,
                       int64_t kx_lstride, int64_t vt_lstride) {
  Tap t(device, "wis_op_enc_crosskv"); WIS_RET(t.rc);
  if (!mem_f16 || !W_f16 || !bias || !kx_f16 || !vt_f16 || B < 1 || T < 1 || H < 1 || L < 1 || (int64_t)L * 2 * 64 * H > 0x7fffffff || (int64_t)B * T > 0x7fffffff / (64 * (int64_t)H)) {
    set_error("wis_op_enc_crosskv: bad argument"); return WIS_E_ARG; }
  if (T % 4) { set_error("wis_op_enc_crosskv: T = %d (the transposed V tiles store 4 consecutive keys of one utterance: T %% 4 == 0)", T); return WIS_E_ARG; }
  const int d = 64 * H, Tpad = cdiv(T, 64) * 64;
  if (kx_lstride < (int64_t)B * T * d || vt_lstride < (int64_t)B * d * Tpad || kx_lstride % 8 || vt_lstride % 8) {      // (16-byte stores into every layer's image)
    set_error("wis_op_enc_crosskv: layer strides must be multiples of 8 elements and at least the layer's image"); return WIS_E_ARG; }
  return t.finish(launch_gemm_crosskv(t.st, gemm_plain(reinterpret_cast<const f16*>(mem_f16), d, reinterpret_cast<const f16*>(W_f16), B * T, L * 2 * d, d), bias,
                                      reinterpret_cast<f16*>(kx_f16), reinterpret_cast<f16*>(vt_f16), d, T, Tpad, H, kx_lstride, vt_lstride));
}
int wis_op_gemm_splitk_ln(int device, const void* A_f16, const void* W_f16, const float* bias, float* X, const float* gamma, const float* beta, void* Y_f16,
                          int M, int N, int K, int splits) {
  Tap t(device, "wis_op_gemm_splitk_ln"); WIS_RET(t.rc);
  if (!A_f16 || !W_f16 || !bias || !X || !gamma || !beta || !Y_f16 || M < 1 || N < 128 || K < 64 || splits < 0 || splits > 16 || (int64_t)M * N > 0x7fffffff) {
    set_error("wis_op_gemm_splitk_ln: bad argument"); return WIS_E_ARG; }
  if (!splits) splits = enc_splitk(N, M);      // run_encoder's choice for FFN2 at these rows
  if (!splits) { set_error("wis_op_gemm_splitk_ln: the encoder does not split K at M = %d, N = %d", M, N); return WIS_E_UNSUPPORTED; }
  float* scratch = nullptr;
  WIS_RET(t.get(&scratch, (size_t)splits * M * N));
  return t.finish(launch_gemm_splitk_resid(t.st, gemm_plain(reinterpret_cast<const f16*>(A_f16), K, reinterpret_cast<const f16*>(W_f16), M, N, K), splits, scratch, bias, X, X,
                                           gamma, beta, reinterpret_cast<f16*>(Y_f16)));
}

// ---- taps of what runs behind the logits (tests/test_gpu_sample_ops.py): the cache movers of a beam step and of a verified draft window, and the three
// softmax readers, through the product's launch_* functions on caller-supplied device memory
int wis_op_kv_reorder(int device, void* kc_f16, void* vc_f16, int64_t layer_stride_elems, int L, const int32_t* parent, const int32_t* step_u, const int32_t* done,
                      int B, int beam, int P, int ctx, int d) {
  Tap t(device, "wis_op_kv_reorder"); WIS_RET(t.rc);
  if (!kc_f16 || !vc_f16 || !parent || !step_u || !done || L < 1 || B < 1 || beam < 1 || P < 1 || ctx < 1 || d < 8 || d % 8 || layer_stride_elems < (int64_t)B * beam * ctx * d || layer_stride_elems % 8) {
    set_error("wis_op_kv_reorder: bad argument"); return WIS_E_ARG; }
  BeamState bs; memset(&bs, 0, sizeof(bs));
  bs.parent = const_cast<int*>(parent); bs.step_u = const_cast<int*>(step_u); bs.done = const_cast<int*>(done);
  return t.finish(launch_kv_reorder(t.st, reinterpret_cast<f16*>(kc_f16), reinterpret_cast<f16*>(vc_f16), (size_t)layer_stride_elems, L, bs, B, beam, P, ctx, d));
}
int wis_op_kv_reorder_from(int device, void* kc_f16, void* vc_f16, int64_t layer_stride_elems, int L, const int32_t* parent, const int32_t* step_u, const int32_t* done,
                           const int32_t* plen, int B, int beam, int ctx, int d) {
  Tap t(device, "wis_op_kv_reorder_from"); WIS_RET(t.rc);
  if (!kc_f16 || !vc_f16 || !parent || !step_u || !done || !plen || L < 1 || B < 1 || beam < 1 || ctx < 1 || d < 8 || d % 8 || layer_stride_elems < (int64_t)B * beam * ctx * d || layer_stride_elems % 8) {
    set_error("wis_op_kv_reorder_from: bad argument"); return WIS_E_ARG; }
  BeamState bs; memset(&bs, 0, sizeof(bs));
  bs.parent = const_cast<int*>(parent); bs.step_u = const_cast<int*>(step_u); bs.done = const_cast<int*>(done);
  return t.finish(launch_kv_reorder_from(t.st, reinterpret_cast<f16*>(kc_f16), reinterpret_cast<f16*>(vc_f16), (size_t)layer_stride_elems, L, bs, B, beam, plen, ctx, d));
}
int wis_op_kv_gather(int device, void* kc_f16, void* vc_f16, int64_t layer_stride_elems, int L, const int32_t* vstate, const int32_t* done, int beam, int w0, int ctx, int d) {
  Tap t(device, "wis_op_kv_gather"); WIS_RET(t.rc);
  if (!kc_f16 || !vc_f16 || !vstate || !done || L < 1 || beam < 1 || beam > MAX_R || w0 < 0 || w0 >= ctx || d < 8 || d % 8 || layer_stride_elems < (int64_t)beam * ctx * d || layer_stride_elems % 8) {
    set_error("wis_op_kv_gather: bad argument"); return WIS_E_ARG; }
  return t.finish(launch_kv_gather(t.st, reinterpret_cast<f16*>(kc_f16), reinterpret_cast<f16*>(vc_f16), (size_t)layer_stride_elems, L, vstate, done, beam, w0, ctx, d));
}
int wis_op_no_speech(int device, const float* logits, int ld, int B, int rs, int r0, int V, int ns, float* out) {
  Tap t(device, "wis_op_no_speech"); WIS_RET(t.rc);
  if (!logits || !out || B < 1 || rs < 1 || r0 < 0 || r0 >= rs || V < 1 || ld < V) { set_error("wis_op_no_speech: bad argument"); return WIS_E_ARG; }
  return t.finish(launch_no_speech(t.st, logits, ld, B, rs, r0, V, ns, out));
}
int wis_op_no_speech_rows(int device, const float* logits, int ld, int B, int rs, const int32_t* rows, int V, int ns, float* out) {
  Tap t(device, "wis_op_no_speech_rows"); WIS_RET(t.rc);
  if (!logits || !rows || !out || B < 1 || rs < 1 || V < 1 || ld < V) { set_error("wis_op_no_speech_rows: bad argument"); return WIS_E_ARG; }
  return t.finish(launch_no_speech_rows(t.st, logits, ld, B, rs, rows, V, ns, out));
}
int wis_op_lang_probs(int device, const float* logits, int ld, const int32_t* lang_ids, int n_lang, float* probs, int B) {
  Tap t(device, "wis_op_lang_probs"); WIS_RET(t.rc);
  if (!logits || !lang_ids || !probs || B < 1 || n_lang < 1 || ld < 1) { set_error("wis_op_lang_probs: bad argument"); return WIS_E_ARG; }
  return t.finish(launch_lang_probs(t.st, logits, ld, lang_ids, n_lang, probs, B));
}
int wis_op_greedy_rows(int device, const float* logits, int n_vocab, int n_vocab_pad, int eot, const float* bias_all, const float* bias_begin, const int32_t* step_u,
                       int B, int beam, int lr_b, int lr_j, int lr_off, const int32_t* rowmap, int32_t* tok_out, float* lp_out) {
  Tap t(device, "wis_op_greedy_rows"); WIS_RET(t.rc);
  if (!logits || !bias_begin || !step_u || !tok_out || !lp_out || B < 1 || beam < 1 || beam > MAX_R || n_vocab < STAT_SUB || n_vocab_pad < n_vocab || eot < 0 || eot >= n_vocab ||
      lr_b < 0 || lr_j < 0 || lr_off < 0) { set_error("wis_op_greedy_rows: bad argument"); return WIS_E_ARG; }
  const int rows = B * beam;
  SampleCfg sc; memset(&sc, 0, sizeof(sc));
  sc.n_vocab = n_vocab; sc.n_vocab_pad = n_vocab_pad; sc.eot = eot; sc.beam = beam; sc.n_cand = 2; sc.suppress_blank = 1; sc.greedy = 1;
  float *smax = nullptr, *ssum = nullptr, *sval = nullptr; int* sidx = nullptr;
  WIS_RET(t.get(&smax, (size_t)rows * STAT_SUB)); WIS_RET(t.get(&ssum, (size_t)rows * STAT_SUB));
  WIS_RET(t.get(&sval, (size_t)rows * STAT_SUB * sc.n_cand)); WIS_RET(t.get(&sidx, (size_t)rows * STAT_SUB * sc.n_cand));
  WIS_RET(launch_logit_stats(t.st, logits, bias_all, bias_begin, step_u, smax, ssum, sval, sidx, B, sc, lr_b, lr_j, lr_off, nullptr, rowmap));
  return t.finish(launch_greedy_pick(t.st, smax, ssum, sval, sidx, rows, sc, tok_out, lp_out));
}

// the phrase mask of one step on caller-supplied rows, histories and trie (tests/test_gpu_phrase_ops.py)
int wis_op_phrase_rules(int device, float* logits, int n_vocab, int n_vocab_pad, int eot, const int32_t* trie, int n_rec, const int32_t* alive,
                        const int32_t* step_u, const int32_t* done, int B, int beam, int max_new, int lr_b, int lr_j, int lr_off) {
  Tap t(device, "wis_op_phrase_rules"); WIS_RET(t.rc);
  if (!logits || !trie || !alive || !step_u || !done || n_rec < 1 || n_rec > PHRASE_MAX_RECORDS || n_vocab < 1 || n_vocab_pad < n_vocab || eot < 0 || eot >= n_vocab ||
      B < 1 || beam < 1 || beam > MAX_R || B * beam > MAX_ROWS || max_new < 1 || max_new > MAX_STEPS || lr_b < 0 || lr_j < 0 || lr_off < 0) {
    set_error("wis_op_phrase_rules: bad argument"); return WIS_E_ARG; }
  SampleCfg sc; memset(&sc, 0, sizeof(sc));
  sc.n_vocab = n_vocab; sc.n_vocab_pad = n_vocab_pad; sc.eot = eot; sc.beam = beam; sc.max_new = max_new;
  BeamState bs; memset(&bs, 0, sizeof(bs));
  bs.alive = const_cast<int*>(alive); bs.step_u = const_cast<int*>(step_u); bs.done = const_cast<int*>(done);
  return t.finish(launch_phrase_rules(t.st, logits, bs, B, sc, reinterpret_cast<const int4*>(trie), n_rec, lr_b, lr_j, lr_off));
}

// ... with the in-grammar mass, and the gather of finished results' sums (tests/test_gpu_phrase_mass_ops.py); every row counts as live (no cum)
int wis_op_phrase_mass(int device, float* logits, int n_vocab, int n_vocab_pad, int eot, const int32_t* trie, int n_rec, const int32_t* alive,
                       const int32_t* step_u, const int32_t* done, int B, int beam, int max_new, int lr_b, int lr_j, int lr_off,
                       const float* bias_all, const float* bias_begin, int suppress_blank, float* logmass) {
  Tap t(device, "wis_op_phrase_mass"); WIS_RET(t.rc);
  if (!logits || !trie || !alive || !step_u || !done || !bias_begin || !logmass || n_rec < 1 || n_rec > PHRASE_MAX_RECORDS || n_vocab < 1 || n_vocab > 65536 ||
      n_vocab_pad < n_vocab || eot < 0 || eot >= n_vocab || B < 1 || beam < 1 || beam > MAX_R || B * beam > MAX_ROWS || max_new < 1 || max_new > MAX_STEPS ||
      lr_b < 0 || lr_j < 0 || lr_off < 0) {
    set_error("wis_op_phrase_mass: bad argument"); return WIS_E_ARG; }
  SampleCfg sc; memset(&sc, 0, sizeof(sc));
  sc.n_vocab = n_vocab; sc.n_vocab_pad = n_vocab_pad; sc.eot = eot; sc.beam = beam; sc.max_new = max_new; sc.suppress_blank = suppress_blank ? 1 : 0;
  BeamState bs; memset(&bs, 0, sizeof(bs));
  bs.alive = const_cast<int*>(alive); bs.step_u = const_cast<int*>(step_u); bs.done = const_cast<int*>(done);
  return t.finish(launch_phrase_rules_mass(t.st, logits, bs, B, sc, reinterpret_cast<const int4*>(trie), n_rec, lr_b, lr_j, lr_off, bias_all, bias_begin, logmass, n_rec));
}
int wis_op_phrase_mass_gather(int device, const int32_t* ids, const int32_t* len, const float* score, const int32_t* trie, int n_rec,
                              const float* logmass, int B, int n, int id_ld, float* out) {
  Tap t(device, "wis_op_phrase_mass_gather"); WIS_RET(t.rc);
  if (!ids || !len || !trie || !logmass || !out || n_rec < 1 || n_rec > PHRASE_MAX_RECORDS || B < 1 || n < 1 || B * n > MAX_ROWS || id_ld < 1 || id_ld > MAX_STEPS) {
    set_error("wis_op_phrase_mass_gather: bad argument"); return WIS_E_ARG; }
  return t.finish(launch_phrase_mass_gather(t.st, ids, len, score, reinterpret_cast<const int4*>(trie), n_rec, logmass, n_rec, B, n, id_ld, out));
}

// the hotword boost of one step on caller-supplied rows, histories and trie (tests/test_gpu_hotword_ops.py); the table is read back and validated
// on the host before anything is launched
int wis_op_hotword_rules(int device, float* logits, int n_vocab, int n_vocab_pad, int eot, const int32_t* trie, int n_rec, const int32_t* alive,
                         const int32_t* step_u, const int32_t* done, int B, int beam, int max_new, int fixed_new, float boost,
                         int lr_b, int lr_j, int lr_off) {
  Tap t(device, "wis_op_hotword_rules"); WIS_RET(t.rc);
  if (!logits || !trie || !alive || !step_u || !done || n_rec < 1 || n_rec > PHRASE_MAX_RECORDS || n_vocab < 1 || n_vocab > 65536 || n_vocab_pad < n_vocab ||
      eot < 0 || eot >= n_vocab || B < 1 || beam < 1 || beam > MAX_R || B * beam > MAX_ROWS || max_new < 1 || max_new > MAX_STEPS || fixed_new < 0 ||
      !std::isfinite(boost) || !(boost > 0.f) || lr_b < 0 || lr_j < 0 || lr_off < 0) {
    set_error("wis_op_hotword_rules: bad argument"); return WIS_E_ARG; }
  std::vector<int32_t> host((size_t)n_rec * 4);
  WIS_HIP_CHECK(hipMemcpy(host.data(), trie, host.size() * 4, hipMemcpyDeviceToHost));
  const int vrc = validate_token_trie("wis_op_hotword_rules", host.data(), n_rec, n_vocab, eot, nullptr, nullptr);
  if (vrc != WIS_OK) return WIS_E_ARG;      // (a table beyond the limits too: this entry point answers every malformed table alike)
  int ctl_h[4] = {0, n_rec, 0, 0}; memcpy(&ctl_h[0], &boost, 4);
  int* ctl = nullptr;
  WIS_RET(t.get(&ctl, 4));
  WIS_HIP_CHECK(hipMemcpy(ctl, ctl_h, sizeof(ctl_h), hipMemcpyHostToDevice));
  SampleCfg sc; memset(&sc, 0, sizeof(sc));
  sc.n_vocab = n_vocab; sc.n_vocab_pad = n_vocab_pad; sc.eot = eot; sc.beam = beam; sc.max_new = max_new; sc.fixed_new = fixed_new;
  BeamState bs; memset(&bs, 0, sizeof(bs));
  bs.alive = const_cast<int*>(alive); bs.step_u = const_cast<int*>(step_u); bs.done = const_cast<int*>(done);
  return t.finish(launch_hotword_rules(t.st, logits, bs, B, sc, reinterpret_cast<const int4*>(trie), ctl, lr_b, lr_j, lr_off));
}

// ---- the resampler's kernel alone (tests/test_gpu_resample_ops.py): one launch of csrc/resample.hip on a caller-supplied slice of a longer signal
int wis_op_resample_segment(int device, const float* x_slice, int64_t n_slice, int64_t k_base, int64_t n_in_total, int64_t m0, int64_t count,
                            int up, int down, float* out) {
  Tap t(device, "wis_op_resample_segment"); WIS_RET(t.rc);
  DeviceCtx* c = nullptr; WIS_RET(get_ctx(device, &c));
  return t.finish(resample_segment(c, t.st, x_slice, n_slice, k_base, n_in_total, m0, count, up, down, out));
}

// ---- the log-mel front end on caller-supplied device memory, its scratch exposed (tests/test_gpu_logmel_ops.py): the whole window as stage_input runs it
// (logmel_device), or a range of 16-frame tiles alone as a streaming session runs it (logmel_frames, no finalize).  n_samples goes to the device as given:
// the clamp to the window is the kernel's
int wis_op_logmel(int device, int n_mels, const float* d_pcm, int64_t stride, const int64_t* n_samples, int n_win, int tile0, int n_tiles,
                  float* d_logspec, unsigned* d_gmax, float* d_mel, void* d_img_f16) {
  Tap t(device, "wis_op_logmel"); WIS_RET(t.rc);
  if (!d_pcm || !n_samples || !d_logspec || !d_gmax || n_win < 1 || stride < 0) { set_error("wis_op_logmel: bad argument"); return WIS_E_ARG; }
  DeviceCtx* c = nullptr; WIS_RET(get_ctx(device, &c));
  const bool whole = tile0 == 0 && n_tiles == cdiv(WIS_N_FRAMES, 16);
  if (!whole && (d_mel || d_img_f16)) { set_error("wis_op_logmel: a tile range has no finalize pass: d_mel and d_img_f16 must be null"); return WIS_E_ARG; }
  int64_t* d_ns = nullptr;
  WIS_RET(t.get(&d_ns, (size_t)n_win));
  WIS_HIP_CHECK(hipMemcpy(d_ns, n_samples, (size_t)n_win * 8, hipMemcpyHostToDevice));
  if (whole) return t.finish(logmel_device(c, t.st, d_logspec, d_gmax, d_pcm, stride, d_ns, n_win, d_mel, reinterpret_cast<f16*>(d_img_f16), n_mels));
  WIS_HIP_CHECK(hipMemsetAsync(d_gmax, 0, (size_t)n_win * 4, t.st));
  return t.finish(logmel_frames(c, t.st, d_logspec, d_gmax, d_pcm, stride, d_ns, n_win, tile0, n_tiles, n_mels));
}

}  // extern "C"
