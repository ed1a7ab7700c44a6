// kernels.hpp — launch wrappers shared between the kernel files and the model driver.
#pragma once
#include "common.hpp"

namespace wis {

// ---- encoder ---------------------------------------------------------------------------
struct GemmP {
  const f16* A; int64_t a_bs; int a_rs; int a_rpb;   // A row m -> A + (m / a_rpb)*a_bs + (m % a_rpb)*a_rs
  const f16* W;                                      // [N][K] row-major
  int M, N, K;
  int klen;                                          // split-K: K range per blockIdx.z slice (0 = whole K, gridDim.z = 1)
  // column sub-ranges (the 8-phase kernel's separate launches for plain and transposed tiles): the launch covers N columns, column c of it
  // is output feature (c / n_span) * n_period + n_phase + c % n_span (n_span = 0: the identity)
  int n_span = 0, n_period = 0, n_phase = 0;
};
static inline GemmP gemm_plain(const f16* A, int lda, const f16* W, int M, int N, int K) {
  GemmP p; p.A = A; p.a_bs = 0; p.a_rs = lda; p.a_rpb = 0x7fffffff; p.W = W; p.M = M; p.N = N; p.K = K; p.klen = 0; return p;
}
int launch_layernorm(hipStream_t st, const float* x, const float* gamma, const float* beta, f16* y, int M, int d);
int launch_gemm_generic(hipStream_t st, const GemmP& p, const float* bias, const float* resid, void* C, int flags);
// split-K GEMM for deep-K / narrow-N shapes: `splits` K-slices write fp32 partial tiles to `scratch` ([splits][M][N]), then
// one elementwise pass adds the slices + bias + residual into X (fp32, may alias resid).  Keeps dense 128x128 tiles and still
// launches >= 1 workgroup per CU.
int launch_gemm_splitk_resid(hipStream_t st, const GemmP& p, int splits, float* scratch, const float* bias, const float* resid, float* X,
                             const float* ln_gamma = nullptr, const float* ln_beta = nullptr, f16* Y = nullptr);
int launch_gemm_conv1(hipStream_t st, const GemmP& p, const float* bias, f16* C, int T);
int launch_gemm_conv2(hipStream_t st, const GemmP& p, const float* bias, const float* pos, float* X, int T);
int launch_gemm_qkv(hipStream_t st, const GemmP& p, const float* bias, f16* qk, f16* vt, int d, int T, int Tpad, int H);
int launch_gemm_crosskv(hipStream_t st, const GemmP& p, const float* bias, f16* kx, f16* vt, int d, int T, int Tpad, int H, int64_t kx_lstride, int64_t vt_lstride);
// part / counters: split-key scratch sized for `part_cap` (utterance, head, 128-query tile) triples (enc_attention_part_floats); the
// split-key form is only taken when the launch fits that capacity
int launch_enc_attention(hipStream_t st, const f16* qk, const f16* vt, f16* out, int B, int T, int Tpad, int H, float* part = nullptr, unsigned* counters = nullptr,
                         size_t part_cap = 0);
// the same launch with the loop (lazy: enc_attn_lazy_kernel, Q pre-multiplied by log2(e) / sqrt(64); else enc_attn_kernel, Q by 1 / sqrt(64)) and
// the form (split: two workgroups per query tile and head; needs part / counters for every pair and cdiv(T, 64) >= 4) named by the caller
int launch_enc_attention_form(hipStream_t st, const f16* qk, const f16* vt, f16* out, int B, int T, int Tpad, int H, float* part, unsigned* counters,
                              bool lazy, bool split);
size_t enc_attention_part_floats(int B, int T, int H);
// true: the lazy-reference loop (enc_attn_lazy_kernel), which expects Q pre-multiplied by log2(e) / sqrt(64); fixed per process
bool enc_attn_lazy();
void launch_scale_q_log2e(hipStream_t st, f16* qk, int64_t rows, int d);      // (op-level entry: Q half of a [rows][2d] image times log2(e))

// ---- decoder ---------------------------------------------------------------------------
constexpr int MAX_ROWS = 96;      // decoder rows per pass: B*beam (decode) or B*P (merged prefill + first step): 16 utterances x beam 5 + slack; wis_hip/ctranslate2.py MAX_DECODER_ROWS
constexpr int MAX_R = 8;          // rows per utterance (beam or prompt prefix length)
constexpr int MAX_CAND = 2 * MAX_R;
constexpr int MAX_HYP = 3 * MAX_R;      // finished hypotheses an utterance can hold (model.hip make_sample_cfg)

// per-row decode metadata (device arrays, length MAX_ROWS)
struct RowMeta {
  int* tok;     // input token of the row
  int* pos;     // text position of the row (KV-cache index it writes)
  int* slot;    // physical KV slot the row writes
  int* lslot;   // logical KV slot of the row (prefill rows of an utterance share one)
};

// skinny GEMM (decoder): y = epi(LN?(x) . Wp^T + b), Wp packed in MFMA 16x16x32 A-fragment order
enum { GV_GELU = 1, GV_RESID = 2, GV_OUT_F32 = 4, GV_LN = 8, GV_QKV = 16,      // (32 is free: wis_op_gemv's tap uses it for "quantise to 8 bits first")
       GV_LN16 = 64 };     // LayerNorm-folded projection on f16 rows, statistics taken from those rows in the kernel (<= 8 rows)
struct GemvP {
  const void* x;                 // f32 [M][K] (raw, un-normalised) when GV_LN else f16 [M][K]
  const float* gamma; const float* beta;   // unused (the affine part lives in the folded weights / bias); kept: removing them moves every later member, and the gemv kernels are kept instruction for instruction
  const float* csum;             // GV_LN: column sums of the gamma-folded weights (see fold_ln_kernel); bias then is b + W.beta
  const f16* Wp; const float* bias;
  const float* wscale;           // non-null: Wp is the 8-bit packed image, one dequantisation scale per output row
  void* y;                       // [M][N] f32 (GV_OUT_F32 / GV_RESID in place) or f16
  int M, N, K, flags;
  // GV_QKV epilogue: n < d -> q (f32 [M][d]); d <= n < 2d -> K cache; n >= 2d -> V cache
  float* q; f16* kc; f16* vc; const int* slot; const int* pos; int d; int ctx;   // cache [slots][ctx][d]
  unsigned long long* prof;      // optional phase stamps (workgroup 0)
  int rows;                      // output columns per workgroup (0 => 16): 16 = Wp in A-fragment order, 8 (launch_gemv, gemv_nc8_shape only) = Wp the eight-column image of launch_pack_gemv_nc8, 5 (launch_gemv, gemv_nc5_shape only) = Wp the five-column image of launch_pack_gemv_nc5; launch_gemv_dual: problem B's 8 under out_cq_nc8_shape, else ignored
  const void* x2; int xsplit;    // f16 activations only: columns >= xsplit are read from x2 (row-major [M][K - xsplit]); x then is [M][xsplit]
  f16* y16;                      // GV_RESID: optional f16 row-major copy of the produced rows
  // ---- batched rows (launch_gemv_frag, M > 8): activations live in HBM in MFMA B-fragment order ("xf", xf_index below)
  int xmb;                       // 16-row blocks of the x fragment image (= ceil(M / 16))
  const float* stat_in;          // GV_LN: per-row partials of the raw fp32 rows, [M][K/16][2] = (sum x, sum (x - tile mean)^2) per 16 columns (merged Welford-style)
  float* stat_out;               // GV_RESID: the same partials of the rows this launch produces, [M][N/16][2]
  f16* y_xf;                     // GV_RESID: f16 fragment image of the produced rows (next projection's input); f16 output: the output itself
  int ymb;                       // 16-row blocks of y_xf (0: f16 output stays row-major [M][N])
  // K split over workgroups (launch_gemv_frag, ksplit > 1): workgroup (n-tile, k-slice) streams its slice, publishes the 16-column sums
  // to kpart [N/16][ksplit][xmb][64] float4 and the last-arriving slice of an n-tile (ticket kcnt[N/16], zero-initialised once,
  // re-armed by the winner) adds the slices in index order and runs the epilogue
  int ksplit; float* kpart; unsigned* kcnt;
  // M split over workgroups (launch_gemv_frag decides; set by the kernel): this workgroup's first row block and the image's row blocks
  int mb0, mbi;
  // the weight matrix as a k-step window of a wider packed image (launch_gemv_frag / launch_gemv_frag3): wks = k-steps per n-tile of
  // the image (0: K / 32, the matrix is the whole image), wk0 = first k-step of the window
  int wks, wk0;
};
int launch_gemv(hipStream_t st, const GemvP& p);
// two f16-activation skinny GEMMs in one launch
int launch_gemv_dual(hipStream_t st, const GemvP& pa, const GemvP& pb);
// launch_gemv_dual serves pb.rows = 8 (problem B's Wp the eight-column image of launch_pack_gemv_nc8) for the out-projection + cross-Q pair at these shapes:
// large's width, <= 8 rows, d / 16 + d / 8 workgroups in one dispatch round on this device
bool out_cq_nc8_shape(int M, int d);
// Batched decode rows (8 < M <= 96).  The skinny GEMM reads its activations as ready-made MFMA B fragments straight from L2
// (written in that order by the producing kernel: no per-workgroup LDS staging, no staging barrier, many workgroups per CU), and
// the pre-LN LayerNorm needs no launch of its own: every residual epilogue leaves per-16-column partial sums of the rows it
// produced, the folded projection that follows (W o gamma, b + W.beta, column sums) turns them into mean / rstd in its epilogue.
int launch_gemv_frag(hipStream_t st, const GemvP& p);
// n (2 or 3) such GEMMs of one row count in one launch (f16 weights, no K split, same K / 128 for all): see gemv_frag3_kernel
int launch_gemv_frag3(hipStream_t st, const GemvP* p, int n);
// activation fragment image: element (row m, column k) of an [M][K] matrix, MB = ceil(M / 16) row blocks:
//   [k / 32][m / 16][lane = (m % 16) + 16 * ((k / 8) % 4)][k % 8]      (one 1 KiB wave load per (k-step, row block))
__host__ __device__ static inline size_t xf_index(int m, int k, int MB) {
  return ((size_t)((k >> 5) * MB + (m >> 4)) * 64 + (m & 15) + 16 * ((k >> 3) & 3)) * 8 + (k & 7);
}
// f16 elements of a fragment image of K columns and MB row blocks (host code: allocation and memset sizes)
constexpr size_t xf_elems(int K, int MB) { return (size_t)(K / 32) * MB * 64 * 8; }
// x (fp32 or f16, row-major [M][K]) -> fragment image (+ optional per-16-column partial sums): test taps and the weight-stream tap
int launch_xf_pack(hipStream_t st, const void* x, int x_f16, f16* xf, float* stat, int M, int K, int MB);
int launch_dec_embed_xf(hipStream_t st, const f16* emb, const f16* pos_emb, const int* tok, const int* pos, float* x, f16* xf, float* stat, int M, int d, int MB);
int launch_fold_ln(hipStream_t st, f16* W, const float* gamma, const float* beta, float* bias, float* csum, int N, int K, int n_scale, float qscale);
int launch_csum8(hipStream_t st, const f16* W, const float* scale, float* csum, int N, int K, int n_scale, float qscale);
int launch_pack_gemv8(hipStream_t st, const f16* W, unsigned char* Wp, float* scale, int N, int Npad, int K, int n_scale, float qscale);
// pack W [N][K] f16 row-major -> Wp [Npad/rows][K/32][4][rows][8]; matrix rows >= N are zero; scale matrix rows
// [0, n_scale) by `scale` (folds the 1/sqrt(dh) query scaling into the projection)
int launch_pack_gemv(hipStream_t st, const f16* W, f16* Wp, int N, int Npad, int K, int n_scale, float scale, int rows = 16);
// pack W [N][K] f16 row-major -> the eight-column image [Npad/8][K/64][64][8] (dec_kernels.hip pack_gemv_nc8_kernel); Npad % 8 == 0, K % 64 == 0
int launch_pack_gemv_nc8(hipStream_t st, const f16* W, f16* Wp, int N, int Npad, int K);
bool gemv_nc8_shape(int M, int N, int K);      // launch_gemv serves GemvP::rows = 8 at these shapes
// pack W [N][K] f16 row-major -> the five-column image [N/5][K/32/kw][ceil(kw/3)][64][8] (dec_kernels.hip pack_gemv_nc5_kernel) of gemv_nc5_elems f16 elements;
// kw = k-steps per wave K-range (a divisor of K / 32): 40 for the form launch_gemv runs (FFN2, K = 5120: a K quarter per wave); N % 5 == 0
size_t gemv_nc5_elems(int N, int K, int kw);
int launch_pack_gemv_nc5(hipStream_t st, const f16* W, f16* Wp, int N, int K, int kw);
// launch_gemv serves GemvP::rows = 5 at these shapes and stage flags: one dispatch round of five-column slabs on the current device
bool gemv_nc5_shape(int M, int N, int K, int flags);
int gemv_rows_for(int N, int K);     // tile height used for an [N][K] decoder matrix

int launch_dec_embed(hipStream_t st, const f16* emb, const f16* pos_emb, const int* tok, const int* pos, float* x, int M, int d, f16* xh = nullptr);
// logical slot of row m = (m / rpu) * sstride + (m % rpu) * rmul
// out_mb: 0 = out is row-major f16 [M][d]; > 0 = fragment image with that many 16-row blocks (batched decode)
// anc (optional; draft verification at beam > 1, model.hip verify_beam_draft): the rows of a pass are the nodes of a beam TREE - row m reads
// the cache rows of positions < w0 from slot anc[m * aw] and position w0 + t from slot anc[m * aw + t] (its ancestor at window step t)
struct SelfAttnP {
  const float* q = nullptr; const f16* kc = nullptr; const f16* vc = nullptr; const int* pos = nullptr; f16* out = nullptr;
  int M = 0, H = 0, d = 0, ctx = 0, rpu = 0, sstride = 0, rmul = 0;
  unsigned long long* prof = nullptr; int out_mb = 0; const int* anc = nullptr; int w0 = 0, aw = 0;
  const int* base = nullptr;      // (optional): slot of the positions before w0, per row
  int nb = 8;                     // 8-position blocks per pass (2 / 4 / 8; plain form only)
  const int* plen = nullptr;      // (optional; the long-prompt route's decode step): device word per utterance - the length of the prompt prefix its rpu rows share in slot
                                  // (m / rpu) * sstride; the pass runs dec_self_attn_long_kernel (one workgroup per (utterance, head)) in the plain kernel's place
};
int launch_dec_self_attn(hipStream_t st, const SelfAttnP& p);
// The decode step's self-attention behind a long prompt (dec_kernels.hip dec_self_attn_long_kernel): utterance b's k <= MAX_R rows (m = b k + j) read positions
// < plen[b] from slot b * sstride - once for all k rows - and positions plen[b] .. pos[m] from their own slot b * sstride + j.  plen[b] in [1, SA_LONG_MAX_PLEN]
constexpr int SA_LONG_MAX_PLEN = 256;
int launch_dec_self_attn_long(hipStream_t st, const float* q, const f16* kc, const f16* vc, const int* pos, const int* plen, int B, int k, int H, int d, int ctx, int sstride,
                              f16* out, int out_mb);
// cross attention of R rows per utterance over the utterance's T encoder keys.
//   q f32 [B*R][d] (pre-scaled), kx f16 [B][H][8][T][8], vt f16 [B][H][64][Tpad] (zero padded) -> out f16 [B*R][d]
// gran / epoch (optional): the granule hand-off of small grids (dec_kernels.hip, SPIN): gran = 8-byte slots [B*H][6][8][66], epoch =
// ONE flag word (non-zero: a combiner's bounded spin ran out) followed by [B*H] monotonic epoch words, all zero-initialised once
constexpr int CA_SPIN_MAX_BH = 192;      // spinning combiners per launch: fewer than the chip's 256 CUs, so a producer always finds a slot (8 utterances x 20 heads = 160)
struct CrossAttnP {
  const float* q = nullptr; const f16* kx = nullptr; const f16* vt = nullptr; f16* out = nullptr; float* part = nullptr; unsigned* counters = nullptr;
  int B = 0, R = 0, H = 0, d = 0, T = 0, Tpad = 0, chunks = 0;
  unsigned long long* prof = nullptr; int out_mb = 0;
  const float* xres = nullptr; const float* qcs = nullptr; const float* qb = nullptr;   // folded query: see the kernel
  unsigned long long* gran = nullptr; unsigned* epoch = nullptr;
  const float* q2 = nullptr; int xres_is_stat = 0;    // batched fold: q = q + q2; xres = row partials [B*R][d/16][2] instead of the rows
  int kv_shared = 0;      // 1: every row group b reads utterance 0's K / V (the B groups are rows of ONE utterance: draft verification)
};
int launch_dec_cross_attn(hipStream_t st, const CrossAttnP& p);

// sampling: per-(row, chunk) masked max / sum-exp / top-2k of the logits
struct SampleCfg {
  int n_vocab, n_vocab_pad, eot, beam, n_cand, max_new, fixed_new, suppress_blank, greedy;
  float length_penalty; int max_hyp; int allow_early_exit; int max_candidates;
  int early_exit_hyps;      // finished hypotheses an early exit needs besides a finished top candidate (WIS_EARLY_EXIT_NUM_HYPOTHESES)
};
// CTranslate2's early exit (patience 1, length_penalty 0): `top_beam_finished && hypotheses.size() >= num_hypotheses` (1: the product
// returns one hypothesis) - or, with 0 here, `>= max_candidates` as rounds 1-5 had it.  Unpinned either way (no CTranslate2 offline);
// the oracle's switch is oracle/whisper_ref.py EARLY_EXIT_NEEDS, the deciding cases are in tests/golden/make_ct2_golden.py.
#ifndef WIS_EARLY_EXIT_NUM_HYPOTHESES
#define WIS_EARLY_EXIT_NUM_HYPOTHESES 1
#endif
constexpr int STAT_SUB = 64;      // sub-chunks per logits row (one wave each): statistics and top-n_cand candidates per sub-chunk
// Random sampling (include/wis_hip.h states the rule): what the sampling kernels take besides SampleCfg.  An utterance's cfg.beam rows are its
// samples.  topk < 0: the whole vocabulary - the statistics kernel perturbs every value and leaves per sub-chunk {best perturbed value, that entry's
// unperturbed logit} in st_val and its id in st_idx (cfg.n_cand = 2 is the layout); topk >= 2: the pool stays unperturbed (cfg.n_cand = topk per
// sub-chunk), the sample step selects and perturbs.  topk = 0: off.
struct SampleP {
  int topk = 0; float T = 1.f;
  const unsigned long long* seeds = nullptr;      // device [B]: Philox key per utterance (written at the start of the call: never a captured value)
  const unsigned* noise = nullptr;                // device [rows][n_vocab] (wis_debug_search_n's table) in place of the Philox words, or null
};
int launch_logit_stats(hipStream_t st, const float* logits, const float* bias_all, const float* bias_begin, const int* step_u,
                       float* st_max, float* st_sum, float* st_val, int* st_idx, int B, const SampleCfg& cfg,
                       int lr_b, int lr_j, int lr_off, unsigned long long* prof = nullptr,    // logits row of (b, j) = b*lr_b + j*lr_j + lr_off
                       const int* rowmap = nullptr,       // ... or b*lr_b + rowmap[j]*lr_j + lr_off (device table: draft verification of a beam search)
                       const int* ts_desc = nullptr,      // timestamp form: the ranges launch_ts_rules left per row are masked too
                       const SampleP* sp = nullptr);      // whole-vocabulary sampling (sp->topk < 0): the perturbed form
// Whisper's timestamp rules for prompts without <|notimestamps|> (dec_kernels.hip ts_rules_kernel): per live row, the masked ranges
// of the step (+ the decision flag, the step) -> ts_desc [B*beam][TS_DESC_INTS]; rows as launch_logit_stats reads them.
// max_init < 0: no cap on the first timestamp
constexpr int TS_DESC_INTS = 8;
struct BeamState;
int launch_ts_rules(hipStream_t st, const float* logits, const float* bias_all, const float* bias_begin, const BeamState& bs, int B,
                    const SampleCfg& cfg, int no_ts, int max_init, int lr_b, int lr_j, int lr_off, int* ts_desc);
// repetition_penalty / no_repeat_ngram_size (dec_kernels.hip rep_rules_kernel): per live row, the row of `logits` the step samples from is
// patched in place from the row's generated history - one penalty per distinct history token, -inf per banned n-gram completion - ahead of
// every other kernel of the tail; rows as launch_logit_stats reads them.  penalty 1 / ngram 0: that rule is off (the caller launches
// nothing when both are)
int launch_rep_rules(hipStream_t st, float* logits, const BeamState& bs, int B, const SampleCfg& cfg, float penalty, int ngram, int lr_b, int lr_j, int lr_off);
// phrase-constrained decoding (dec_kernels.hip phrase_rules_kernel): per live row whose generated history is a path of the flat trie, every id
// of [0, n_vocab) but the node's children (and <|endoftext|> at a phrase end) is stored as -inf in the row of `logits` the step samples from;
// behind launch_rep_rules, ahead of everything else of the tail; rows as launch_logit_stats reads them.  trie: device, n_rec int4 records
// {token, first child record, children, child ends a phrase}, record 0 the root's pseudo-edge (include/wis_hip.h has the layout's rules)
constexpr int PHRASE_MAX_RECORDS = 65535, PHRASE_MAX_CHILDREN = 4096, PHRASE_MAX_DEPTH = 32;
int launch_phrase_rules(hipStream_t st, float* logits, const BeamState& bs, int B, const SampleCfg& cfg, const int4* trie, int n_rec, int lr_b, int lr_j, int lr_off);
// ... with the in-grammar mass (dec_kernels.hip phrase_rules_mass_kernel, in launch_phrase_rules' place when wis_gen_opts_t::phrase_mass is on): the
// same mask, and per live row with a finite cumulative score (bs.cum; null: every row) one float at logmass[b lm_ld + the node's record index] - the
// log of the share of the row's softmax, under the bias lists launch_logit_stats applies, that the node allows.  lm_ld >= n_rec floats per utterance
int launch_phrase_rules_mass(hipStream_t st, float* logits, const BeamState& bs, int B, const SampleCfg& cfg, const int4* trie, int n_rec, int lr_b, int lr_j, int lr_off,
                             const float* bias_all, const float* bias_begin, float* logmass, int lm_ld);
// ... and, behind the search, per result r = b n + i (ids [B n][id_ld], len / score [B n]; score may be null) the sum of the slots along its path -> out [B n]
int launch_phrase_mass_gather(hipStream_t st, const int* ids, const int* len, const float* score, const int4* trie, int n_rec, const float* logmass, int lm_ld,
                              int B, int n, int id_ld, float* out);
constexpr int PHRASE_MASS_LD = 65536;      // floats per utterance of a handle's logmass buffer (>= PHRASE_MAX_RECORDS)
// hotword boosting (dec_kernels.hip hotword_rules_kernel; include/wis_hip.h, THE HOTWORD RULE): per live row, every token that continues a suffix
// of the row's generated history along the flat trie (the root's children always) gets ONE fp32 addition of *boost in the row of `logits` the
// step samples from; behind launch_rep_rules, ahead of everything else of the tail; rows as launch_logit_stats reads them.  trie: device, records
// in launch_phrase_rules' format; ctl: device, {the boost's fp32 bits, the record count}, read by the kernel (a captured launch carries the
// address, neither value)
int launch_hotword_rules(hipStream_t st, float* logits, const BeamState& bs, int B, const SampleCfg& cfg, const int4* trie, const int* ctl,
                         int lr_b, int lr_j, int lr_off);
// probability of <|nospeech|> under the full-vocabulary softmax of each utterance's <|startoftranscript|> row (b * rs + r0)
int launch_no_speech(hipStream_t st, const float* logits, int ld, int B, int rs, int r0, int V, int ns, float* out);
// ... with the row of every utterance in device memory (rows [B]; a value outside [0, rs): utterance b is not in this pass, out[b] stays as it is)
int launch_no_speech_rows(hipStream_t st, const float* logits, int ld, int B, int rs, const int* rows, int V, int ns, float* out);
struct BeamState {
  int* step_u;      // [B] generated-token count so far
  int* done;        // [B]
  int* n_hyp;       // [B]
  float* cum;       // [B*beam] cumulative log-prob of live beams
  int* alive;       // [B*beam][max_new] token history of live beams
  int* parent;      // [B*beam] KV slot each live beam descends from after the last beam step (kv_reorder_kernel applies it)
  float* hyp_score; // [B][max_hyp] raw cumulative score
  int* hyp_len;     // [B][max_hyp]
  int* hyp_tok;     // [B][max_hyp][max_new]
  int* all_done;    // [1] utterances finished so far
  int* out_ids; int* out_len; float* out_score;   // final result [B][max_new], [B], [B]
  // progress of the search, published to the host without a stream round trip (generate.hip run_paced):
  unsigned* tick;                 // device [4]: {workgroups of beam_step_kernel that ended since init, call generation, step at which all_done reached B, -}
  const unsigned* giveup;         // word 0 of the cross-attention hand-off's epoch block (a combiner's bounded spin ran out)
  unsigned long long* host;       // device address of the HOST-mapped (fine-grained) progress block, layout HP_* below
  int* row_done;                  // [B*beam] sampled decodes: the sample of this row has finished (its result stands, the row is fed EOT)
  int* traj;                      // [B][256 steps][MAX_R][2]: (token, beam slot it continued from) of every live beam after each step - the search's
                                  // trajectory, what a later call verifies as its DRAFT (wis_last_trajectory / wis_generate_draft_beam)
};
// host-mapped progress block (uint64 words).  The workgroup of a beam step that ends LAST writes HP_REC with one system-scope
// release store after everything else of the step - finished utterances' results included - has been made visible to the host.
enum { HP_REC = 0,          // (generation << 48) | (steps completed << 32) | (give-up flag << 16) | utterances done
       HP_STAMP0 = 1,       // 100 MHz constant clock at the end of the first beam step of the call (merged prefill + first step)
       HP_STAMP = 2,        // ... at the end of the latest beam step
       HP_DONE_STEP = 3,    // steps completed when the last utterance finished (0 until then)
       HP_DONE_STAMP = 4,   // constant clock at that moment
       HP_WORDS = 8,        // results follow: int out_len[HP_MAXB], float out_score[HP_MAXB], int out_ids[HP_MAXB][256]; result i of utterance b at b n + i (n results per utterance)
       HP_MAXB = MAX_ROWS };
constexpr size_t HP_BYTES = HP_WORDS * 8 + (size_t)HP_MAXB * 8 + (size_t)HP_MAXB * 256 * 4;
__host__ __device__ inline int* hp_out_len(unsigned long long* hp) { return reinterpret_cast<int*>(hp + HP_WORDS); }
__host__ __device__ inline float* hp_out_score(unsigned long long* hp) { return reinterpret_cast<float*>(hp + HP_WORDS) + HP_MAXB; }
__host__ __device__ inline int* hp_out_ids(unsigned long long* hp) { return reinterpret_cast<int*>(hp + HP_WORDS) + 2 * HP_MAXB; }
// after a beam step: every live beam's KV rows (all layers, positions < P - 1 + step) become a copy of its parent's
int launch_kv_reorder(hipStream_t st, f16* kc, f16* vc, size_t layer_stride, int L, const BeamState& bs, int B, int beam, int P, int ctx, int d);
// ... behind a long prompt: the prompt's positions [0, plen[b]) stay in the utterance's first slot for the whole search and are never moved - only positions
// [plen[b], plen[b] - 1 + step) of every live beam become a copy of its parent's.  plen: device word per utterance
int launch_kv_reorder_from(hipStream_t st, f16* kc, f16* vc, size_t layer_stride, int L, const BeamState& bs, int B, int beam, const int* plen, int ctx, int d);
// plen (launch_beam_step, launch_sample_step; the long-prompt route): the prompt length comes from this device word per utterance, P is ignored - a second
// instantiation of the kernel, so that one captured step serves every prompt length
int launch_beam_step(hipStream_t st, const float* st_max, const float* st_sum, const float* st_val, const int* st_idx,
                     const BeamState& bs, const RowMeta& rm, int B, int P, int ctx, const SampleCfg& cfg, unsigned long long* prof = nullptr,
                     int n_best = 1,       // results per utterance: the n_best best finished hypotheses at b n_best + i (bs.out_*, the host block)
                     const int* plen = nullptr);
// the sampled decode's step (dec_kernels.hip sample_step_kernel), in beam_step's place: per sample row the Gumbel-max draw from what
// launch_logit_stats left, score, history, per-row done flag; the utterance ends when all its rows have (or at max_new)
int launch_sample_step(hipStream_t st, const float* st_max, const float* st_sum, const float* st_val, const int* st_idx,
                       const BeamState& bs, const RowMeta& rm, int B, int P, const SampleCfg& cfg, const SampleP& sp, const int* plen = nullptr);
// draft verification at beam > 1 (one utterance; dec_kernels.hip draft_match_kernel / kv_gather_kernel): behind a replayed beam step, match the live set
// it produced with the draft's entry for the step AS A SET (draft = [n_draft][MAX_R][2] in BeamState::traj's layout); vstate ints: 0 steps verified,
// 2 window steps applied, 8.. the draft node each live beam is matched to (logit_stats rowmap), 16.. / 32.. the slots holding each beam's history
// (book = 1: maintained per window step, applied to the cache by launch_kv_gather once per window).  No match: done[0] = 2 parks the search
constexpr int DRAFT_VS_INTS = 32 + MAX_R * 32, DRAFT_VS_PERM = 8, DRAFT_VS_BASE = 16;
int launch_draft_match(hipStream_t st, const BeamState& bs, const int* draft, int n_draft, int beam, int* vstate, int book);
int launch_kv_gather(hipStream_t st, f16* kc, f16* vc, size_t layer_stride, int L, const int* vstate, const int* done, int beam, int w0, int ctx, int d);
// teacher-forced rows: the token a k = 1 beam step would take from each row's statistics, and its log-probability
int launch_greedy_pick(hipStream_t st, const float* st_max, const float* st_sum, const float* st_val, const int* st_idx, int rows, const SampleCfg& cfg, int* tok_out, float* lp_out);
// language detection: softmax over lang_ids of the row's logits
int launch_lang_probs(hipStream_t st, const float* logits, int ld, const int* lang_ids, int n_lang, float* probs, int B);

}  // namespace wis
