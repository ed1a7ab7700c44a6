// model.hpp — the model handle (wis_model) and the driver's internal interface: what model.hip defines and generate.hip, taps.hip and
// align.hip use.  Declarations only: every function here, and every piece of process-wide state behind them (the spin budget, the count of
// running calls, the read-once WIS_* switches), is defined in exactly one object - a `static` copied into this header would become one
// copy per object, and three spin budgets are how a shared GPU is made to hang.
#pragma once
#include <string.h>
#include <array>
#include <atomic>
#include <map>
#include <memory>
#include <vector>

#include "common.hpp"
#include "kernels.hpp"

namespace wis {

struct EncLayerW {
  float *ln1_g, *ln1_b, *ln2_g, *ln2_b;
  f16 *w_qkv, *w_out, *w_f1, *w_f2;
  float *b_qkv, *b_out, *b_f1, *b_f2;
};
// One decoder projection as the step streams it (load_weights: load_proj; the taps fill one from their own scratch)
struct DecProj {
  const f16* Wp;          // MFMA-fragment packed matrix; the 8-bit image when `scale` is given
  const float* scale;     // int8_float16: dequantisation scale per output row, else null
  const float* bias;      // LayerNorm-folded projections: b + W . beta
  const float* csum;      // column sums of the LayerNorm-folded weights (dec_kernels.hip fold_ln_kernel): non-null exactly when the projection follows a LayerNorm
  int N, K;               // launch shape (the vocabulary projection: N = n_vocab_pad)
  int rows;               // weight rows per workgroup tile the matrix was packed for (gemv_rows_for)
  const f16* Wp8 = nullptr;      // the same f16 matrix as an eight-column image (add_nc8_image), or null: the route of <= 8 rows streams this one where gemv_nc8_shape holds
  const f16* Wp5 = nullptr;      // the same f16 matrix as a five-column image (add_nc5_image: FFN2, in place of Wp8), or null: streamed where gemv_nc5_shape holds
};
struct DecLayerW {
  float *ln1_g, *ln1_b, *ln2_g, *ln2_b, *ln3_g, *ln3_b;
  DecProj qkv, out, cq, cout, f1, f2;
  DecProj cqo;                                       // cross-Q folded THROUGH the out-projection: packed [W'q | W'q Wo] ([d][2d]) and W'q bo (out_cq_dual / out_cq_frag3)
  f16* w_ckv; float* b_ckv;                          // row-major [2d][d] (encoder-side GEMM)
  // the six matrices a decode step streams per layer, in step order
  std::array<const DecProj*, 6> streamed() const { return {&qkv, &out, &cq, &cout, &f1, &f2}; }
};

struct GraphKey {
  int B, beam, P, max_new, fixed_new, suppress_blank, suppress_default, early_exit, spin, sa_nb; float lp, patience;
  int timestamps, max_init;      // the timestamp form of the step (ts_rules_kernel ahead of logit_stats_kernel<true>) and its first-timestamp cap
  float rep_pen; int rep_ngram;  // rep_rules_kernel at the head of the tail (both 0: off, no such launch)
  int samp_topk; float samp_T; int n_hyp;      // sampled decode (sample_step_kernel in beam_step_kernel's place) / results per utterance; all 0: off, one result
  int phrases;                   // phrase_rules_kernel behind rep_rules_kernel (0: off, no such launch; 2: phrase_rules_mass_kernel in its place; the set itself is device memory: no part of the key)
  int hotwords;                  // hotword_rules_kernel behind rep_rules_kernel (0: off, no such launch; the set AND the boost are device memory: no part of the key)
  bool operator<(const GraphKey& o) const { return memcmp(this, &o, sizeof(GraphKey)) < 0; }
};

// the device slabs that hold a model's converted weights: shared by every replica cloned from it on the same GPU (wis_model_clone),
// freed when the last of them is destroyed
struct WeightSlabs {
  int device; std::vector<void*> slabs; size_t bytes = 0;
  ~WeightSlabs() { hipSetDevice(device); for (void* p : slabs) hipFree(p); }
};

// word-level alignment (csrc/align.hip): the handle's alignment heads and the scratch its first wis_align allocates
struct AlignState {
  std::vector<int> heads;                 // (layer, head) pairs of wis_model_set_alignment_heads; empty: every head of the upper half of the decoder
  bool ready = false;                     // the selection below matches `heads`
  bool capture = false;                   // a wis_align decoder pass is running: dec_forward_frag hands every layer's finished cross-Q to align_capture_q
  int nsel = 0, sel_cap = 0; size_t sel_bytes = 0;
  std::vector<int> layer_s0;              // selected heads of layer l: [layer_s0[l], layer_s0[l + 1]) of the (layer, head)-sorted selection
  int* d_sel_head = nullptr; long long* d_koff = nullptr;      // per selected head: its head index, the element offset of its K image in kx_all (utterance 0)
  f16* qsel = nullptr;                    // captured queries [max_batch][nsel][n_text_ctx][64]
  float *W = nullptr, *acc = nullptr;     // one chunk of heads' probabilities; the matrix [max_batch][tokens][n_audio_ctx]
  unsigned* trace = nullptr; int *rev = nullptr, *path = nullptr, *d_meta = nullptr; float* probs = nullptr;
  int cap_ub0 = 0, cap_t0 = 0, cap_P = 0, last_nmax = 0;
  int kv_ub0 = 0;                         // first utterance of the group a wis_align decoder pass (or a long prompt's prefill window) runs (dec_forward_frag offsets the cross K / V by it); 0 outside
  hipEvent_t ev[5 + 128] = {}; int n_ev = 0;      // phase boundaries of the last call (wis_align_last_timing); ev[5..]: (weights, filter) pairs of the first 64 head chunks
  bool ev_partial = false;                // the last call had more head chunks than event pairs: the weights / filter split is not reported
};

constexpr int ANC_W = 32;      // ancestor-table entries per row = the most steps a window holds (beam 2 / 3: 32 steps = 64 / 96 rows)
constexpr int MAX_STEPS = 256;      // decode steps a search can take (the cap on max_new; BeamState::traj and the draft hold this many entries)

// The handle's pinned host staging block.  Every area is a member of its own: a copy out of one may still be pending on the stream when
// the host fills the next (the prompt rows against a window's rows, init_beam_state's staging against the rows'), and nothing here is
// large enough to be worth sharing.  Extents follow the device buffers they stage (alloc_buffers).
struct RowStage { int tok[MAX_ROWS], pos[MAX_ROWS], slot[MAX_ROWS], lslot[MAX_ROWS]; };      // upload_rows -> RowMeta
struct PinnedScratch {
  int64_t nsamp[MAX_ROWS];                     // stage_input: samples per utterance
  int giveup;                                  // spin_gave_up: the give-up flag read back
  RowStage rows, win_rows;                     // the search's rows (every caller's default); the rows of a draft-verification window
  float beam_cum[MAX_ROWS]; unsigned beam_tick[4];      // init_beam_state
  unsigned long long seeds[MAX_ROWS];          // upload_seeds: the Philox key of every utterance of a sampled decode
  int sa_tab[2 * MAX_ROWS];                    // stage_search, WIS_SA_LONG=0: wis_model::d_sa_tab
  int plen[MAX_ROWS];                          // stage_search: the prompt length of every utterance (wis_model::d_plen)
  int nsp_rows[MAX_ROWS];                      // wis_generate_ragged: the <|startoftranscript|> row of every utterance of a prefill pass (wis_model::d_nsp_rows)
  unsigned reseed_tick[4];                     // reseed_tick: bs.tick behind a draft verification
  // wis_generate_draft: step index of the verified rows, their picks read back; then the search state `steps` ordinary steps would have left
  int vstep[MAX_ROWS], pick_tok[MAX_ROWS]; float pick_lp[MAX_ROWS];
  int hist[MAX_STEPS];
  struct { int step, tok, pos, slot; float cum; } seed;
  // wis_generate_draft_beam: the draft in BeamState::traj's layout, the host image of the verification state, done / step_u read back per
  // window, the window rows' ancestor table and base slots, the per-window reset of the path bookkeeping (vs[2], then vs[DRAFT_VS_BASE + j])
  int draft[MAX_STEPS * MAX_R * 2];
  int vstate[DRAFT_VS_INTS]; int win_done, win_step;
  int anc[MAX_ROWS * ANC_W], base[MAX_ROWS];
  int path_reset[1 + MAX_R];
  struct { int parent[MAX_R], step, done; } tree_seed;      // wis_debug_tree_logits: the search state behind the prompt pass
  int al_frames[2 * MAX_ROWS], al_tgt[MAX_ROWS], al_dst[MAX_ROWS];      // wis_align: {tokens, frames} per utterance; target token / matrix row per pass row
};
static_assert(MAX_ROWS % 16 == 0, "a verification window is padded to whole groups of 16 rows: min(ANC_W, MAX_ROWS / beam) steps x beam rows must still fit MAX_ROWS");
static_assert(sizeof(PinnedScratch::draft) == sizeof(int) * MAX_STEPS * MAX_R * 2, "the draft area holds one {token, origin} pair per step and beam slot");
static_assert(sizeof(PinnedScratch::anc) == sizeof(int) * MAX_ROWS * ANC_W, "ANC_W ancestor slots per window row");
// (the device buffers these two are copied to - d_draft, d_anc - are allocated by the staging areas' own extents: alloc_buffers)
static_assert(DRAFT_VS_PERM + MAX_R <= 16 && DRAFT_VS_BASE + MAX_R <= 32 && DRAFT_VS_INTS >= 32, "the verification state's head (32 ints up, 16 back) holds the matching and the base slots");

}  // namespace wis

// (the tag include/wis_hip.h declares for wis_model_t: the one type of this header outside namespace wis)
struct wis_model {
  wis_config_t cfg;
  int device;
  wis::DeviceCtx* ctx;
  hipStream_t st;
  std::shared_ptr<wis::WeightSlabs> wslabs;      // weights (read-only after load): possibly shared with clones
  std::vector<void*> allocs;    // this replica's own slabs (activations, caches, state), carved by dalloc()
  char* slab_cur = nullptr; size_t slab_left = 0;
  size_t bytes = 0;
  // weights
  wis::f16 *w_conv1, *w_conv2; float *b_conv1, *b_conv2, *enc_pos, *enc_ln_g, *enc_ln_b;
  std::vector<wis::EncLayerW> enc;
  std::vector<wis::DecLayerW> dec;
  wis::f16 *emb, *dec_pos; float *dec_ln_g, *dec_ln_b;
  wis::DecProj proj;            // the tied vocabulary projection behind the final LayerNorm (N = n_vocab_pad; it has no bias of its own: bias = W . beta)
  float *bias_all, *bias_begin; int* d_lang_ids;
  int n_vocab_pad;
  // activations
  int Tpad;
  wis::f16 *img, *c1, *xn, *qk, *vt, *ao, *hbuf, *mem;
  float* x; float* skbuf; float* enc_part = nullptr; unsigned* enc_cnt = nullptr;
  std::vector<wis::f16*> kx, vx;        // per decoder layer cross K / V
  std::vector<wis::f16*> kc, vc;        // per decoder layer self KV cache [slots][ctx][d] (views into kc_all / vc_all)
  wis::f16 *kc_all = nullptr, *vc_all = nullptr; size_t kv_layer_stride = 0;
  wis::f16 *kx_all = nullptr, *vx_all = nullptr, *w_ckv_all = nullptr; float* b_ckv_all = nullptr;   // cross K/V: one block each, all layers
  size_t kx_lstride = 0, vx_lstride = 0;
  // decode state
  float *dx, *dq, *logits, *part; wis::f16 *dao, *dh, *dln; unsigned* counters;
  float* dq2 = nullptr;         // batched fold: second half of the cross-attention q_raw (dec_forward_frag)
  const int* sa_plen = nullptr;      // set around the decode step of the long-prompt route (generate.hip StepGraph): the pass's self-attention reads the prompt prefix shared in the utterance's first slot (SelfAttnP::plen)
  int sa_long_form = -1;      // wis_debug_sa_long: 1 / 0 pick the step's self-attention form on this handle whatever WIS_SA_LONG says (-1: the switch decides)
  int sa_w0 = 0; int* d_sa_tab = nullptr;      // WIS_SA_LONG=0 (A/B form, fallback): the same read pattern through dec_self_attn_kernel<TREE> - w0 = the prompt length (a kernel
                                               // argument: this form keeps one step graph per prompt length), [0, MAX_ROWS) the rows' own slots, [MAX_ROWS, 2 MAX_ROWS) their utterance's first slot
  int* d_plen = nullptr;             // prompt length per utterance [MAX_ROWS], written at the start of every call (stage_search): what the long-prompt route's step kernels read in P's place
  int sa_nb = 8;      // 8-position blocks the step's self-attention asks for per pass (generate.hip StepGraph: by the step index; 8 outside the step loops)
  float* gf_part = nullptr; unsigned* gf_cnt = nullptr; int gf_ksplit = 1;      // K split of the batched FFN2 skinny GEMM: slice sums, tickets (GemvP::ksplit)
  unsigned long long* ca_gran = nullptr; unsigned* ca_epoch = nullptr;      // granule hand-off of the decoder cross-attention (small grids): slots, flag + epochs
  bool spin_off = false;        // sticky: a combiner's bounded spin ran out once on this handle - it keeps to the ticket hand-off from then on
  int handoff_retries = 0;      // calls repeated because a combiner's spin ran out (wis_debug_handoff: expected to stay 0)
  bool spin_now = true;         // this call's decision (SpinClaim): dec_forward passes the granule buffers only when set
  wis::f16 *dxf = nullptr, *daoxf = nullptr, *dhxf = nullptr; float* dstat = nullptr;   // batched rows: fragment images of x / attention out / FFN hidden, row partial sums
  wis::RowMeta rm; wis::BeamState bs;
  wis::RowMeta rm_win;          // row metadata of a draft-verification window (wis_generate_draft_beam): the search's own rows (rm, written by beam_step_kernel) stay untouched
  float *st_max, *st_sum, *st_val; int* st_idx;
  unsigned long long* d_seeds = nullptr;      // sampled decodes: Philox key per utterance [MAX_ROWS], written at the start of every call (SampleP::seeds)
  int* ts_desc = nullptr;       // timestamp rules: masked ranges per live row [MAX_ROWS][TS_DESC_INTS] (ts_rules_kernel -> logit_stats_kernel<true>)
  float* d_nsp = nullptr;       // no_speech_prob per utterance of the last wis_generate that asked for it
  int nsp_B = 0;                // ... its batch size; 0: the last call did not ask (wis_last_no_speech_prob answers WIS_E_STATE)
  int* d_nsp_rows = nullptr;    // wis_generate_ragged: per utterance of a prefill pass, the pass row that read <|startoftranscript|> or -1 [MAX_ROWS] (launch_no_speech_rows)
  float* d_in; int64_t* d_nsamp; float* d_probs;
  int* vstep = nullptr; int* pick_tok = nullptr; float* pick_lp = nullptr;      // wis_generate_draft: per-row step index, picked token / log-probability of the teacher-forced rows
  int* d_draft = nullptr; int* d_anc = nullptr; int* d_vstate = nullptr; int* d_base = nullptr;        // wis_generate_draft_beam: the draft trajectory [MAX_STEPS][MAX_R][2], the window rows' ancestor slots [MAX_ROWS][ANC_W], the verification state, the rows' base slots
  float* lm_logspec = nullptr; unsigned* lm_gmax = nullptr;   // log-mel scratch of THIS replica (never shared with other callers)
  wis::PinnedScratch* h_pin = nullptr;      // pinned host staging (one block, named areas)
  unsigned long long* h_prog = nullptr;      // host-mapped progress block of the beam search (kernels.hpp HP_*): the decode loop polls it
  unsigned gen = 0;                          // generation of the current search (records of an earlier call's over-run step are ignored)
  int last_B = 0, last_beam = 0;             // shape of the last generate call (wis_last_trajectory)
  bool last_ragged = false;                  // ... its prompts differed in length (wis_generate_ragged): wis_last_trajectory answers WIS_E_STATE
  bool overrun_left = false;                 // the last call returned with an over-run decode step still queued (its give-up flag, if any, is not the next call's)
  hipEvent_t ev[8];
  hipStream_t st_enc = nullptr;             // wis_generate's front half (log-mel, encoder) runs here: it overlaps the previous call's over-run decode step on `st`
  hipEvent_t ev_enc = nullptr, ev_ckv = nullptr;      // encoder output ready (st_enc -> st); cross-K/V projection done reading it (st -> the next call's st_enc)
  wis_timing_t timing;
  bool front_skipped = false;               // the last run_front was handed encoder output: no log-mel, no encoder ran (wis_last_timing: 0 ms for both)
  std::map<wis::GraphKey, hipGraphExec_t> graphs;
  bool use_graph;
  bool w8 = false;              // decoder weights stored as 8-bit packed fragments
  bool cq_fold = false;         // f16 decoder weights: the fused out-projection + cross-Q stage is available (p_cqo)
  wis::f16* dxh = nullptr;      // f16 row-major copy of the layer input rows (written by the embedding / FFN2 epilogues)
  unsigned long long* d_prof;   // [L*8][16] stamp rows, one per layer kernel (wis_debug_phase_cycles / wis_debug_timeline)
  bool prof_on; bool prof_all;
  size_t enc_part_cap = 0;      // (utterance, head, query tile) triples the split-key encoder attention buffers were sized for
  std::atomic_flag busy = ATOMIC_FLAG_INIT;   // one compute call at a time per handle (BusyGuard)
  wis::AlignState al;
  // phrase-constrained decoding (wis_model_set_phrases): the handle's set as a flat trie in a buffer of FIXED capacity (PHRASE_MAX_RECORDS records,
  // allocated with the other buffers: the pointer a captured step carries never changes, installing a set is a copy), its record count (0: no set)
  // and its longest phrase; tok_flags: per token id, bit 0 = in the model's suppress_ids, bit 1 = in suppress_ids_begin (what a set is validated against)
  int4* d_trie = nullptr; int phr_n = 0, phr_depth = 0;
  // wis_gen_opts_t::phrase_mass: per (utterance, trie record) the log in-grammar mass of the step that visited the node, [max_batch][PHRASE_MASS_LD] f32,
  // then [MAX_ROWS] f32 for the gathered sums per result; allocated on the handle's first call with the option on (generate.hip phrase_mass_begin) and
  // never moved - captured steps hold the address; a clone has its own.  phr_mass_B / _n: batch and results per utterance of the last call when that
  // call computed the mass, else 0 (wis_last_phrase_mass answers WIS_E_STATE)
  float* d_logmass = nullptr; float* d_phr_mass = nullptr; int phr_mass_B = 0, phr_mass_n = 0;
  std::vector<unsigned char> tok_flags;
  // hotword boosting (wis_model_set_hotwords): a second set, apart from the phrase set, in a buffer of its own of the same fixed capacity - the
  // LAST buffer carved - and its record count (0: no set); d_hot_ctl: the two words {boost bits, record count} behind the table that hotword_rules_kernel
  // reads - the boost written ahead of every call's steps (as the sampling seeds are), the count with the set: one captured step serves every value
  int4* d_hot = nullptr; int hot_n = 0; int* d_hot_ctl = nullptr;
};

namespace wis {

// ---- one compute call at a time per handle ---------------------------------------------------------------------------------------------
// A handle runs ONE compute call at a time (its activations, KV caches and stream are single-instance; the Python shim feeds every
// replica from one worker thread).  A second thread entering the same handle is refused with WIS_E_STATE instead of silently
// corrupting the first call's state - SURVEY 8(b) asks for thread safety at the boundary: concurrency comes from replicas and the
// micro-batcher, never from two calls inside one replica.
extern std::atomic<int> g_active_calls[64];      // compute calls running per device (all handles): front_half's stream choice (generate.hip); defined in model.hip
struct BusyGuard {
  wis_model* m; bool ok;
  explicit BusyGuard(wis_model* mm) : m(mm), ok(!mm->busy.test_and_set(std::memory_order_acquire)) { if (ok) g_active_calls[m->device & 63].fetch_add(1, std::memory_order_relaxed); }
  ~BusyGuard() { if (ok) { g_active_calls[m->device & 63].fetch_sub(1, std::memory_order_relaxed); m->busy.clear(std::memory_order_release); } }
};
#define WIS_ENTER(m, what)                                                                                      \
  ::wis::BusyGuard _busy(m);                                                                                    \
  if (!_busy.ok) { ::wis::set_error("%s: another call is running on this handle (one call at a time per replica)", what); return WIS_E_STATE; }

// ---- input, encoder, cross K/V ---------------------------------------------------------------------------------------------------------
int check_batch(wis_model* m, int B, int beam);
int stage_input(wis_model* m, const float* input, int kind, int B, hipStream_t on = nullptr);
int run_encoder(wis_model* m, int B, hipStream_t on = nullptr);
int run_cross_kv(wis_model* m, int B, const f16* mem = nullptr);      // mem: the GEMM's A operand [B T][d] (null: the handle's own m->mem)
// The front half of every entry point that reads audio: input -> cross K / V of B utterances on m->st.
//   WIS_IN_MEL_* / WIS_IN_PCM_*: stage_input + run_encoder on `enc` (null: m->st), then run_cross_kv on m->st behind them (enc != m->st:
//   through ev_enc) - what every call site enqueued before the helper existed, launch for launch.
//   WIS_IN_ENC_DEV: no log-mel, no encoder; the cross-K/V GEMM reads the caller's block in place (include/wis_hip.h wis_encode says why it may).
//   WIS_IN_ENC_HOST: the f32 values go up into m->x (free outside the encoder), enc_f32_to_f16_kernel writes m->mem, then the same GEMM.
//   Both run on m->st whatever `enc` says: there is no encoder to run beside the previous call's over-run step.
// timed (wis_generate): ev[0] .. ev[3] around log-mel / encoder / cross-K/V for wis_last_timing; m->front_skipped says the first two did not run.
inline bool input_is_encoded(int kind) { return kind == WIS_IN_ENC_DEV || kind == WIS_IN_ENC_HOST; }
int run_front(wis_model* m, const float* input, int kind, int B, hipStream_t enc = nullptr, bool timed = false);
// what run_encoder launches, for the op taps on shorter images: conv1's K (3 C rounded up to whole 64-deep k-tiles), the convs' GEMM
// descriptions and weight packers, the mel -> image transpose, the FFN2 K split at M rows
int conv1_k(int n_mels);
GemmP conv1_gemm(const f16* img, const f16* w, int B, int T, int n_mels, int N);      // image [B][T + 2][conv1_channels]
GemmP conv2_gemm(const f16* c1, const f16* w, int B, int T, int cin, int N);          // image [B][2 T + 2][cin]
void pack_conv1_w(hipStream_t st, const void* src, int src_f16, f16* dst, int N, int n_mels);
void pack_conv2_w(hipStream_t st, const void* src, int src_f16, f16* dst, int N, int cin);
int launch_mel_to_image(hipStream_t st, const float* mel, f16* img, int B, int n_mels);
int enc_splitk(int d, int M);
// model.hip's two utility kernels for the other objects (a kernel is launched from the object that holds it): convert_kernel over
// blocks_for(rows * cols) workgroups, f16_to_f32_kernel over blocks_for(n)
void launch_convert(hipStream_t st, const void* src, int src_f16, void* dst, int dst_f16, int64_t rows, int64_t cols, int64_t dst_ld, int64_t n_scale, float scale);
void launch_f16_to_f32(hipStream_t st, const f16* s, float* d, int64_t n);

// ---- weight preparation shared with the op taps ----------------------------------------------------------------------------------------
int prep_projection(hipStream_t st, f16* W, int N, int Npad, int K, int n_scale, float scale, const float* gamma, const float* beta, float* bias, float* csum,
                    void* out, float* scale_out, int rows);
int build_cq_fold(hipStream_t st, const f16* wq_gamma, const void* wo, int wo_f16, const float* bo, int d, float qs, f16* fcat, f16* fwot, f16* fwqo, f16* p_cqo, float* b_cqo);

// ---- granule hand-off of the cross-attention: the per-device budget, claimed per call (model.hip) ---------------------------------------
struct SpinClaim {
  wis_model* m; int n = 0;
  SpinClaim(wis_model* mm, int B);
  ~SpinClaim();
  void defer(hipStream_t st);      // the call returns with work of its own still queued on `st`: the claim is released when that work has run
  SpinClaim(const SpinClaim&) = delete;
  SpinClaim& operator=(const SpinClaim&) = delete;
};
int spin_gave_up(wis_model* m, bool* gave_up);

// ---- the decoder pass ------------------------------------------------------------------------------------------------------------------
// tw (draft verification at beam > 1): the M rows are nodes of ONE utterance's beam tree - self-attention by ancestor table (anc [M][aw], first
// window position w0), cross-attention as B = M / 16 groups of R = 16 rows that all read utterance 0's K / V
// own_kv: the B groups are B utterances (the windowed prefill of a long prompt) - group b reads the cross K / V of utterance AlignState::kv_ub0 + b
struct TreeWin { const int* anc; int w0, aw; const int* base = nullptr; bool own_kv = false; };
struct StepRoute { bool frag, fold, ln16; };      // (small_route, model.hip)
StepRoute small_route(const wis_model* m, int M);
bool sa_long_kernel(const wis_model* m);      // false under WIS_SA_LONG=0 (or wis_debug_sa_long(m, 0)): the long-prompt route's step runs the TREE form of dec_self_attn_kernel instead of dec_self_attn_long_kernel
int dec_forward(wis_model* m, int M, int R, int B, bool want_logits, int sstride, int rmul, const TreeWin* tw = nullptr);
int upload_rows(wis_model* m, const std::vector<int>& tok, const std::vector<int>& pos, const std::vector<int>& slot, const std::vector<int>& lslot, bool wait = true, RowStage* stage = nullptr);
int single_row_setup(wis_model* m, int n, const std::vector<int>& tok, int pos);
int align_capture_q(wis_model* m, int l, int M);      // dec_forward_frag's hook into a wis_align pass (align.hip)
// the step's projection stages (model.hip has their contracts)
GemvP gemv_small(const DecProj& p, const void* x, void* y, int M, int flags);
GemvP gemv_frag(const DecProj& p, const void* xf, int M, int flags);
void out_cq_dual(const DecLayerW& w, const f16* a, const f16* xh, float* x1, float* stat, float* q, int M, GemvP* ga, GemvP* gb);
void out_cq_frag3(const DecLayerW& w, const f16* af, const f16* xf, float* x1, float* stat, float* q, float* q2, int M, GemvP g3[3]);
GemvP frag_resid(const DecProj& p, const f16* xf, float* y, f16* y_xf, float* stat_out, int M);
GemvP frag_ln_f32(const DecProj& p, const f16* xf, const float* stat_in, float* y, int M);
GemvP frag_ln_gelu_xf(const DecProj& p, const f16* xf, const float* stat_in, f16* y_xf, int M);
int ffn2_ksplit(int K);
void frag_set_ksplit(GemvP& g, int ks, float* part, unsigned* cnt);

// ---- search state ----------------------------------------------------------------------------------------------------------------------
int init_beam_state(wis_model* m, int B, int beam, bool samples = false, int n_res = 1);
int upload_seeds(wis_model* m, const uint64_t* seeds, int B);
// the ONE validator of a flat token trie (wis_model_set_phrases, wis_model_set_hotwords, wis_op_hotword_rules): n >= 1 records of four int32 on the
// host; tok_flags: the model's suppress bits per token id (null: none known); *deepest: the longest entry.  `who` leads the messages
int validate_token_trie(const char* who, const int32_t* trie, int n, int n_vocab, int eot, const unsigned char* tok_flags, int* deepest);
SampleCfg make_sample_cfg(const wis_model* m, const wis_gen_opts_t* o, int beam, int max_new, float* patience_out);
int check_patience(int beam, float patience);

}  // namespace wis
