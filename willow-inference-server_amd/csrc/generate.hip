// generate.hip — the generate driver (wis_generate, wis_generate_n, wis_generate_ragged, wis_generate_draft, wis_generate_draft_beam) as a sequence of stages, and the
// two taps that are made of its file-local helpers (wis_debug_search*: the sampling tail alone; wis_debug_tree_logits: a draft window alone).
// An object of its own on model.hpp's interface; everything below but the entry points is file-local.
//
//   make_gen_ctx      every argument check, the resolved shape and sampling options of the call
//   stage_search      search counters, prompt rows, progress block: staged before anything the encoder produces
//   front_half        log-mel, encoder, cross-K/V (on a stream of its own while the handle is alone on the GPU)
//   seed_*            five ways to "the search stands after `steps` passes": merged prefill, windowed prefill of a long prompt (one length, or one per utterance), greedy draft, beam-draft windows
//   StepGraph         the decode step as a cached HIP graph (three self-attention lengths)
//   run_burst / run_paced      the two step loops
//   results_*         three forms of result read-back, then the timing record
#include <math.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>
#include <algorithm>
#include <chrono>
#include <cmath>
#include <vector>

#include "common.hpp"
#include "kernels.hpp"
#include "model.hpp"

using namespace wis;

namespace {

// what the sampling tail reads of a call (wis_debug_search builds one for a search over given logits)
struct SampleCtx {
  wis_model* m; hipStream_t st;
  int B, P, beam;
  SampleCfg sc; const float* bias_all;
  bool ts; int ts_max_init;      // Whisper's timestamp rules (prompts without <|notimestamps|>): a pre-pass ahead of the sampling statistics of every step
  float rep_pen = 1.f; int rep_ngram = 0;      // repetition_penalty / no_repeat_ngram_size (1 / 0: off): a pre-pass that patches the logits rows, ahead of everything else
  bool rep() const { return rep_pen != 1.f || rep_ngram != 0; }
  bool phrases = false;          // wis_gen_opts_t::phrases: the handle's phrase set masks every live row behind the repetition rules (phrase_rules_kernel)
  bool phr_mass = false;         // wis_gen_opts_t::phrase_mass: phrase_rules_mass_kernel in that kernel's place - the same mask, and the node's in-grammar mass
  bool hotwords = false;         // wis_gen_opts_t::hotwords: the handle's hotword set boosts every live row behind the repetition rules (hotword_rules_kernel)
  float hot_boost = 0.f;         // ... by this much: written to the handle's device word ahead of the call's steps (hotword_begin), never a kernel argument
  SampleP sp;                    // random sampling (topk 0: off): sample_step_kernel stands in beam_step_kernel's place, `beam` counts the utterance's samples
  int n_res = 1;                 // results per utterance (num_hypotheses)
  bool sampling() const { return sp.topk != 0; }
  const int* plen = nullptr;     // the long-prompt route (P > SHORT_PROMPT): the step kernels read the prompt length from this device word per utterance, P stays out of the step graph
};
// prompts up to here take the merged prefill + first step in one pass and keep P as a kernel argument of the step; longer ones the long-prompt route (seed_prefill_long)
constexpr int SHORT_PROMPT = 16;
// sampling_topk / sampling_temperature / num_hypotheses of a call, resolved (0 in the C struct: off / 1 / 1) - or refused.  *rows = decoder rows per
// utterance: the beams of a search, the samples of a sampled decode.  single: an entry point whose outputs hold one hypothesis per utterance
static int resolve_sample_opts(const wis_gen_opts_t* o, bool single, bool drafted, SampleCtx* g, int* rows) {
  const int k = o->sampling_topk, beam = o->beam_size < 1 ? 1 : o->beam_size;
  const float T = o->sampling_temperature;
  const int n = o->num_hypotheses == 0 ? 1 : o->num_hypotheses;
  const bool on = !(k == 0 || k == 1);
  if (drafted && (on || (T != 0.f && T != 1.f) || n != 1)) { set_error("sampling_topk / sampling_temperature / num_hypotheses: not available for drafted decodes"); return WIS_E_UNSUPPORTED; }
  if (k < -1) { set_error("sampling_topk %d: -1 (whole vocabulary), 0 or 1 (off), 2 .. %d", k, MAX_CAND); return WIS_E_ARG; }
  if (k > MAX_CAND) { set_error("sampling_topk %d: the engine samples from the whole vocabulary (-1) or from at most %d candidates", k, MAX_CAND); return WIS_E_UNSUPPORTED; }
  if (!std::isfinite(T) || T < 0.f) { set_error("sampling_temperature %g: a finite value > 0 (0: 1)", (double)T); return WIS_E_ARG; }
  if (n < 1 || n > MAX_R) { set_error("num_hypotheses %d outside [1, %d]", n, MAX_R); return WIS_E_ARG; }
  if (on && beam > 1) { set_error("sampling applies at beam_size 1 (got beam_size %d)", beam); return WIS_E_ARG; }
  if (!on && n > beam) { set_error("num_hypotheses %d: a search at beam_size %d returns at most %d (more at beam_size 1 needs sampling)", n, beam, beam); return WIS_E_ARG; }
  if (single && n > 1) { set_error("num_hypotheses %d: this entry point returns one hypothesis per utterance (wis_generate_n / wis_debug_search_n)", n); return WIS_E_ARG; }
  g->sp = SampleP();
  g->sp.topk = on ? k : 0; g->sp.T = T == 0.f ? 1.f : T;
  g->n_res = n;
  *rows = on ? n : beam;
  return WIS_OK;
}
// ... and what they change in the sampling kernels' configuration (make_sample_cfg ran for `rows` rows per utterance)
static void apply_sample_opts(wis_model* m, SampleCtx* g) {
  if (g->sampling()) { g->sc.n_cand = g->sp.topk < 0 ? 2 : g->sp.topk; g->sp.seeds = m->d_seeds; }
  else if (g->n_res > 1 && WIS_EARLY_EXIT_NUM_HYPOTHESES) g->sc.early_exit_hyps = g->n_res;      // CTranslate2: hypotheses.size() >= num_hypotheses
}
// repetition_penalty / no_repeat_ngram_size of a call, resolved (0 in the C struct means "off" for both) - or refused
static int resolve_rep_opts(const wis_gen_opts_t* o, SampleCtx* g) {
  const float p = o->repetition_penalty; const int n = o->no_repeat_ngram_size;
  if (!std::isfinite(p) || p < 0.f) { set_error("repetition_penalty %g: a finite value > 0 (1 or 0: off)", (double)p); return WIS_E_ARG; }
  if (n < 0) { set_error("no_repeat_ngram_size %d: >= 0 (0: off)", n); return WIS_E_ARG; }
  g->rep_pen = p == 0.f ? 1.f : p; g->rep_ngram = n;
  return WIS_OK;
}
// wis_gen_opts_t::phrases of a call, resolved - or refused; *max_new: the call's usual value in, what the constrained search takes out
// (max_new_tokens = 0: at most the longest phrase + 1, the step that can only take <|endoftext|>; an explicit value below that is refused)
static int resolve_phrase_opts(const wis_model* m, const wis_gen_opts_t* o, bool drafted, SampleCtx* g, int* max_new) {
  g->phrases = false; g->phr_mass = false;
  if (o->phrase_mass != 0 && o->phrase_mass != 1) { set_error("phrase_mass %d: 0 (off) or 1 (the in-grammar mass of every result)", o->phrase_mass); return WIS_E_ARG; }
  if (o->phrase_mass && o->phrases == 0) { set_error("phrase_mass: needs phrases = 1 (the mass is that of the handle's phrase set)"); return WIS_E_ARG; }
  if (o->phrases == 0) return WIS_OK;
  if (o->phrases != 1) { set_error("phrases %d: 0 (off) or 1 (the handle's phrase set)", o->phrases); return WIS_E_ARG; }
  if (drafted) { set_error("phrases: not available for drafted decodes (wis_generate_draft / wis_generate_draft_beam)"); return WIS_E_UNSUPPORTED; }
  if (o->timestamps) { set_error("phrases: not available with timestamps (a phrase holds text tokens only)"); return WIS_E_UNSUPPORTED; }
  if (o->fixed_new_tokens > 0) { set_error("phrases: not available with fixed_new_tokens (a phrase ends where the set says)"); return WIS_E_UNSUPPORTED; }
  if (g->sampling()) { set_error("phrases: not available for sampled decodes (sampling_topk 0 or 1)"); return WIS_E_UNSUPPORTED; }
  if (m->phr_n < 1) { set_error("phrases: the handle has no phrase set (wis_model_set_phrases)"); return WIS_E_STATE; }
  const int need = m->phr_depth + 1;
  if (o->max_new_tokens > 0 && o->max_new_tokens < need) { set_error("max_new_tokens %d: the phrase set's longest phrase needs %d (its %d tokens and <|endoftext|>)", o->max_new_tokens, need, m->phr_depth); return WIS_E_ARG; }
  if (*max_new < need) { set_error("phrases: the longest phrase (%d tokens) does not fit the %d steps this call can take", m->phr_depth, *max_new); return WIS_E_ARG; }
  if (o->max_new_tokens == 0 && *max_new > need) *max_new = need;
  g->phrases = true; g->phr_mass = o->phrase_mass == 1;
  return WIS_OK;
}
// wis_gen_opts_t::hotwords / hotword_boost of a call, resolved - or refused (THE HOTWORD RULE has the table; both callers have capped max_new at
// MAX_STEPS = 256 before this, the most hotword_rules_kernel's history holds)
static int resolve_hotword_opts(const wis_model* m, const wis_gen_opts_t* o, bool drafted, SampleCtx* g) {
  g->hotwords = false; g->hot_boost = 0.f;
  if (o->hotwords == 0) return WIS_OK;
  if (o->hotwords != 1) { set_error("hotwords %d: 0 (off) or 1 (the handle's hotword set)", o->hotwords); return WIS_E_ARG; }
  if (!std::isfinite(o->hotword_boost) || !(o->hotword_boost > 0.f)) { set_error("hotword_boost %g: a finite value > 0 with hotwords = 1", (double)o->hotword_boost); return WIS_E_ARG; }
  if (o->phrases) { set_error("hotwords: not available together with phrases (a constrained search has nothing left to bias)"); return WIS_E_ARG; }
  if (drafted) { set_error("hotwords: not available for drafted decodes (wis_generate_draft / wis_generate_draft_beam)"); return WIS_E_UNSUPPORTED; }
  if (m->hot_n < 1) { set_error("hotwords: the handle has no hotword set (wis_model_set_hotwords)"); return WIS_E_STATE; }
  g->hotwords = true; g->hot_boost = o->hotword_boost;
  return WIS_OK;
}
// A call with hotwords on, before its first step is enqueued: the boost goes to the handle's device word in stream order - behind an earlier
// call's over-run step, ahead of every step of this one.  The captured steps read the word, so one graph serves every value.
static int hotword_begin(wis_model* m, float boost, hipStream_t st) {
  unsigned bits; memcpy(&bits, &boost, 4);
  WIS_HIP_CHECK(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(m->d_hot_ctl), (int)bits, 1, st));
  return WIS_OK;
}
// A call with phrase_mass on, before anything of it is enqueued: the handle's logmass buffer (allocated here once, as the align scratch is on the first
// wis_align; it never moves), and NaN in the slots of the installed set for each of the call's utterances - a slot the search does not write
// reads as NaN afterwards, never as an earlier call's value (bytes 0xFF: a NaN in every float)
static int phrase_mass_begin(wis_model* m, int B, hipStream_t st) {
  if (!m->d_logmass) {
    void* q = nullptr;
    const size_t bytes = ((size_t)m->cfg.max_batch * PHRASE_MASS_LD + MAX_ROWS) * 4;
    if (hipMalloc(&q, bytes) != hipSuccess) { (void)hipGetLastError(); set_error("phrase_mass: out of device memory (%zu bytes)", bytes); return WIS_E_NOMEM; }
    m->allocs.push_back(q); m->bytes += bytes;
    m->d_logmass = static_cast<float*>(q); m->d_phr_mass = m->d_logmass + (size_t)m->cfg.max_batch * PHRASE_MASS_LD;
  }
  WIS_HIP_CHECK(hipMemset2DAsync(m->d_logmass, (size_t)PHRASE_MASS_LD * 4, 0xFF, (size_t)m->phr_n * 4, (size_t)B, st));
  return WIS_OK;
}
// ... and behind its search: the sums along the results' paths (n results per utterance, where the beam step left them), left in device memory for
// wis_last_phrase_mass
static int phrase_mass_end(wis_model* m, int B, int n, int max_new, hipStream_t st) {
  WIS_RET(launch_phrase_mass_gather(st, m->bs.out_ids, m->bs.out_len, m->bs.out_score, m->d_trie, m->phr_n, m->d_logmass, PHRASE_MASS_LD, B, n, max_new, m->d_phr_mass));
  m->phr_mass_B = B; m->phr_mass_n = n;
  return WIS_OK;
}
// everything a stage needs to know about the call: built once (make_gen_ctx), read-only afterwards
struct GenCtx : SampleCtx {
  const float* input; const int32_t* prompt; const wis_gen_opts_t* o;
  const int32_t *draft, *draft_org; int n_draft;
  const uint64_t* seeds;         // sampled decode: one Philox key per utterance, or null (all 0)
  int max_new; float patience;
  std::chrono::steady_clock::time_point t0;      // total_ms counts from here: the shape is resolved, nothing is enqueued yet
  int sot_row;                   // no_speech_prob: the prompt row that reads <|startoftranscript|> (the same in every utterance of the batch); -1: not asked
  bool drafting, beam_draft;
  bool long_p;                   // the long-prompt route
  int Pl;                        // ... its last window: the prompt rows P - Pl .. P - 1 run as the merged prefill + first step
  bool ragged = false;           // wis_generate_ragged with lengths that differ: every utterance on the long-prompt route, P = the LONGEST prompt (what max_new and the context check take)
  std::vector<int> plens, poff;  // ... the utterances' own lengths (what d_plen holds), where each one's ids start in `prompt`
  std::vector<int> sot_rows;     // ... no_speech_prob: the <|startoftranscript|> position of every utterance (empty: not asked; sot_row stays -1)
  bool nsp() const { return sot_row >= 0 || !sot_rows.empty(); }
};

// draft / n_draft: wis_generate_draft (one utterance, beam 1): the tokens of an earlier hypothesis to verify first
// draft_org (beam > 1, wis_generate_draft_beam): draft = [n_draft][beam] tokens, draft_org = [n_draft][beam] the beam slot each continued from -
// the trajectory of an earlier SEARCH (wis_last_trajectory)
// plen_v (wis_generate_ragged, lengths that differ): the length of every utterance's prompt, `prompt` holds them back to back; P is not read
// None of the checks depends on device state: a refused call has enqueued nothing.
static int make_gen_ctx(wis_model* m, const float* input, int B, const int32_t* prompt, int P, const wis_gen_opts_t* o,
                        const int32_t* draft, int n_draft, const int32_t* draft_org, const uint64_t* seeds, bool single, const int32_t* plen_v, GenCtx* out) {
  const wis_config_t& c = m->cfg;
  GenCtx& g = *out;
  g.m = m; g.st = m->st; g.input = input; g.prompt = prompt; g.o = o; g.draft = draft; g.draft_org = draft_org; g.n_draft = n_draft; g.B = B; g.P = P;
  g.seeds = seeds;
  int rows = 1;
  WIS_RET(resolve_sample_opts(o, single, draft != nullptr, &g, &rows));
  const int beam = g.beam = rows;
  WIS_RET(check_batch(m, B, beam));
  if (!g.sampling()) WIS_RET(check_patience(beam, o->patience));
  const int max_prompt = std::min(c.n_text_ctx / 2 + 4, SA_LONG_MAX_PLEN);      // openai-whisper's n_ctx / 2 - 1 prompt tokens behind <|startofprev|>, the start sequence; the step's self-attention covers a prefix of SA_LONG_MAX_PLEN positions
  int n_prompt = B * P;
  if (plen_v) {
    g.ragged = true; g.plens.assign(plen_v, plen_v + B); g.poff.resize(B);
    n_prompt = P = 0;
    for (int b = 0; b < B; ++b) {
      if (plen_v[b] < 1 || plen_v[b] > max_prompt) { set_error("prompt length %d of utterance %d unsupported (1..%d)", plen_v[b], b, max_prompt); return WIS_E_UNSUPPORTED; }
      g.poff[b] = n_prompt; n_prompt += plen_v[b]; P = std::max(P, (int)plen_v[b]);
    }
    g.P = P;
    if (!sa_long_kernel(m)) { set_error("prompts of different lengths need dec_self_attn_long_kernel (the TREE form of the step's self-attention, WIS_SA_LONG=0, keeps the prompt length as a kernel argument)"); return WIS_E_UNSUPPORTED; }
    if (draft != nullptr) { set_error("prompts of different lengths: not available for drafted decodes"); return WIS_E_UNSUPPORTED; }
    if (o->max_new_tokens > 0 && P + o->max_new_tokens > c.n_text_ctx) { set_error("max_new_tokens %d behind a prompt of %d tokens exceeds the decoder's %d positions", o->max_new_tokens, P, c.n_text_ctx); return WIS_E_ARG; }
  }
  if (P < 1 || P > max_prompt) { set_error("prompt length %d unsupported (1..%d)", P, max_prompt); return WIS_E_UNSUPPORTED; }
  if (!g.ragged && P <= SHORT_PROMPT && B * P > MAX_ROWS) { set_error("prompt length %d unsupported (1..16, B*P <= %d)", P, MAX_ROWS); return WIS_E_UNSUPPORTED; }
  if (P > SHORT_PROMPT && draft != nullptr) { set_error("prompts of more than %d tokens: not available for drafted decodes (wis_generate_draft / wis_generate_draft_beam)", SHORT_PROMPT); return WIS_E_UNSUPPORTED; }
  g.long_p = P > SHORT_PROMPT || g.ragged; g.Pl = std::min(16, MAX_ROWS / B);
  g.plen = g.long_p ? m->d_plen : nullptr;
  int max_new = o->max_new_tokens > 0 ? o->max_new_tokens : std::min(c.n_text_ctx / 2, c.n_text_ctx - P);
  if (max_new > MAX_STEPS) max_new = MAX_STEPS;
  if (P - 1 + max_new > c.n_text_ctx) max_new = c.n_text_ctx - (P - 1);
  WIS_RET(resolve_hotword_opts(m, o, draft != nullptr, &g));      // (ahead of the phrase options: hotwords with phrases is refused as such, whatever the phrase set's state)
  WIS_RET(resolve_phrase_opts(m, o, draft != nullptr, &g, &max_new));
  g.max_new = max_new;
  for (int i = 0; i < n_prompt; ++i) if (prompt[i] < 0 || prompt[i] >= c.n_vocab) { set_error("prompt token %d out of range", prompt[i]); return WIS_E_ARG; }
  WIS_RET(resolve_rep_opts(o, &g));
  g.t0 = std::chrono::steady_clock::now();
  g.sc = make_sample_cfg(m, o, beam, max_new, &g.patience);
  apply_sample_opts(m, &g);
  g.bias_all = o->suppress_default ? m->bias_all : nullptr;
  const bool drafting = g.drafting = draft != nullptr && n_draft > 0;
  const bool beam_draft = g.beam_draft = drafting && draft_org != nullptr;
  if (drafting && B != 1) { set_error("wis_generate_draft: one utterance per call (got B = %d)", B); return WIS_E_UNSUPPORTED; }
  if (drafting && !beam_draft && beam != 1) { set_error("wis_generate_draft: beam_size 1 (a beam search is drafted by its trajectory: wis_generate_draft_beam)"); return WIS_E_UNSUPPORTED; }
  g.ts = o->timestamps != 0;
  g.ts_max_init = o->max_initial_timestamp_index < 0 ? -1 : o->max_initial_timestamp_index;
  if (g.ts && draft != nullptr) { set_error("timestamps: not available for drafted decodes (wis_generate_draft / wis_generate_draft_beam)"); return WIS_E_UNSUPPORTED; }
  if (g.rep() && draft != nullptr) { set_error("repetition_penalty / no_repeat_ngram_size: not available for drafted decodes (wis_generate_draft / wis_generate_draft_beam)"); return WIS_E_UNSUPPORTED; }
  int sot_row = -1;
  if (o->no_speech_prob && g.ragged) {
    g.sot_rows.assign(B, -1);
    for (int b = 0; b < B; ++b) {
      for (int i = 0; i < g.plens[b]; ++i) if (prompt[g.poff[b] + i] == c.sot) { g.sot_rows[b] = i; break; }
      if (g.sot_rows[b] < 0) { set_error("no_speech_prob: the prompt of utterance %d holds no <|startoftranscript|>", b); return WIS_E_ARG; }
    }
  } else
  if (o->no_speech_prob && !drafting) {
    for (int i = 0; i < P; ++i) if (prompt[i] == c.sot) { sot_row = i; break; }
    for (int b = 1; b < B && sot_row >= 0; ++b) if (prompt[b * P + sot_row] != c.sot) sot_row = -1;
    if (sot_row < 0) { set_error("no_speech_prob: the prompts hold no common <|startoftranscript|> position"); return WIS_E_ARG; }
  }
  g.sot_row = sot_row;
  if (beam_draft && (beam < 2 || n_draft > MAX_STEPS)) { set_error("wis_generate_draft_beam: beam_size >= 2 and at most 256 draft steps (got %d, %d)", beam, n_draft); return WIS_E_ARG; }
  if (drafting) for (int i = 0; i < n_draft * (beam_draft ? beam : 1); ++i) if (draft[i] < 0 || draft[i] >= c.n_vocab) { set_error("draft token %d out of range", draft[i]); return WIS_E_ARG; }
  if (beam_draft) for (int i = 0; i < n_draft * beam; ++i) if (draft_org[i] < 0 || draft_org[i] >= beam) { set_error("draft origin %d outside [0, beam_size)", draft_org[i]); return WIS_E_ARG; }
  return WIS_OK;
}

// ---- decode state first: search counters and the prompt rows depend on nothing the encoder produces, and staged from pinned
// memory they cost the host no wait - the whole chain log-mel -> encoder -> cross-K/V -> prefill is enqueued behind them in one go
// (the prefill's ~230 launches are issued while the encoder runs instead of after two stream drains)
static int stage_search(const GenCtx& g) {
  wis_model* m = g.m; const int B = g.B, P = g.P, beam = g.beam;
  WIS_RET(init_beam_state(m, B, beam, g.sampling(), g.sampling() ? beam : g.n_res));
  if (g.sampling()) WIS_RET(upload_seeds(m, g.seeds, B));
  m->last_B = B; m->last_beam = beam; m->last_ragged = g.ragged;
  if (g.long_p) {      // (its prompt rows go up window by window: seed_prefill_long)
    int* hp = m->h_pin->plen;
    for (int b = 0; b < B; ++b) hp[b] = g.ragged ? g.plens[b] : P;
    WIS_HIP_CHECK(hipMemcpyAsync(m->d_plen, hp, (size_t)B * 4, hipMemcpyHostToDevice, g.st));
    if (!sa_long_kernel(m)) {      // the TREE form's tables: row r = b beam + j owns slot r, its utterance's prefix lies in slot b beam
      int* ht = m->h_pin->sa_tab;
      for (int r = 0; r < B * beam; ++r) { ht[r] = r; ht[MAX_ROWS + r] = r / beam * beam; }
      WIS_HIP_CHECK(hipMemcpyAsync(m->d_sa_tab, ht, sizeof(m->h_pin->sa_tab), hipMemcpyHostToDevice, g.st));
    }
  } else
  if (!g.drafting || g.beam_draft) {
    std::vector<int> tok(B * P), pos(B * P), slot(B * P), ls(B * P);
    for (int b = 0; b < B; ++b) for (int i = 0; i < P; ++i) { tok[b * P + i] = g.prompt[b * P + i]; pos[b * P + i] = i; slot[b * P + i] = b * beam; ls[b * P + i] = b * beam; }
    WIS_RET(upload_rows(m, tok, pos, slot, ls, false));
  }
  // a give-up flag raised by the PREVIOUS call's over-run step (it ran after that call had returned) says nothing about this call: cleared
  // behind that step, in stream order, before this call's first decoder pass can raise it again
  if (m->overrun_left) { WIS_HIP_CHECK(hipMemsetAsync(m->ca_epoch, 0, 4, g.st)); m->overrun_left = false; }
  __atomic_store_n(&m->h_prog[HP_REC], 0ull, __ATOMIC_RELAXED);      // (a record of an earlier call's over-run step may still land here: it carries that call's generation)
  m->h_prog[HP_DONE_STEP] = 0; m->h_prog[HP_DONE_STAMP] = 0; m->h_prog[HP_STAMP0] = 0;
  return WIS_OK;
}

// Front half on a stream of its own.  A search that ended on EOT may have left ONE over-run decode step running on `st` (run_paced): the
// log-mel and the encoder of this call touch none of the decoder's buffers, so they start at once beside it instead of behind it;
// the cross-K/V projection (which overwrites what that step still reads) and everything after it stay on `st`.  st_enc waits for the
// previous call's cross-K/V projection - the last reader of the encoder's output buffer.
// ... but only while this is the ONLY call running on the GPU.  HIP streams share a handful of hardware queues (four by default): with
// several replicas decoding at once a second stream per handle puts one replica's encoder and another's decode chain into the same
// queue, and the chain waits behind 100 us GEMMs - measured, 8 utterances per batch, 2 / 3 / 4 batches in flight: 130 / 151 / 145
// utterances/s with the second stream against 165 / 178 / 165 without.  Under that load the over-run step costs next to nothing anyway
// (the GPU is shared; the step is a thin chain).
static int front_half(const GenCtx& g) {
  wis_model* m = g.m; hipStream_t st = g.st; const int B = g.B;
  static const bool one_stream = getenv("WIS_ONE_STREAM") != nullptr;      // A/B switch
  static const bool two_streams = getenv("WIS_TWO_STREAMS") != nullptr;    // A/B switch: the second stream whatever else runs
  const bool alone = g_active_calls[m->device & 63].load(std::memory_order_relaxed) <= 1;
  hipStream_t se = (one_stream || !(alone || two_streams)) ? st : m->st_enc;
  if (input_is_encoded(g.o->input_kind)) se = st;      // encoder output handed in (wis_encode): nothing to run beside the over-run step
  if (se != st) WIS_HIP_CHECK(hipStreamWaitEvent(se, m->ev_ckv, 0));
  WIS_RET(run_front(m, g.input, g.o->input_kind, B, se, true));
  WIS_HIP_CHECK(hipEventRecord(m->ev_ckv, st));
  return WIS_OK;
}

// The sampling tail of a decoder pass: [repetition rules ->] [phrase mask | hotword boost ->] [timestamp rules ->] candidate statistics -> beam step -> cache reorder.  The logits row of (b, j) is
// b*rows.b + j*rows.j + rows.off: a step samples beam j from row b*beam + j {beam, 1, 0}, the pass that carries the prompt samples every beam from the
// last prompt row {P, 0, P - 1}.  TAIL_TAPS: the tap build's stamp rows of the two sampling kernels (the product build carries none).
// TAIL_NO_CACHE: a search over given logits has no cache to reorder (wis_debug_search).
struct LogitRows { int b, j, off; };
enum { TAIL_TAPS = 1, TAIL_NO_CACHE = 2 };
static int sampling_tail(const SampleCtx& g, LogitRows rows, int flags) {
  wis_model* m = g.m; hipStream_t st = g.st; const wis_config_t& c = m->cfg;
  const int lr_b = rows.b, lr_j = rows.j, lr_off = rows.off;
  unsigned long long* prof = (WIS_TAPS && (flags & TAIL_TAPS)) ? m->d_prof + (size_t)c.n_dec_layers * 8 * 16 : nullptr;
  if (g.rep()) WIS_RET(launch_rep_rules(st, m->logits, m->bs, g.B, g.sc, g.rep_pen, g.rep_ngram, lr_b, lr_j, lr_off));
  if (g.phrases && !g.phr_mass) WIS_RET(launch_phrase_rules(st, m->logits, m->bs, g.B, g.sc, m->d_trie, m->phr_n, lr_b, lr_j, lr_off));
  if (g.phrases && g.phr_mass) WIS_RET(launch_phrase_rules_mass(st, m->logits, m->bs, g.B, g.sc, m->d_trie, m->phr_n, lr_b, lr_j, lr_off, g.bias_all, m->bias_begin, m->d_logmass, PHRASE_MASS_LD));
  if (g.hotwords) WIS_RET(launch_hotword_rules(st, m->logits, m->bs, g.B, g.sc, m->d_hot, m->d_hot_ctl, lr_b, lr_j, lr_off));
  if (g.ts) WIS_RET(launch_ts_rules(st, m->logits, g.bias_all, m->bias_begin, m->bs, g.B, g.sc, c.no_timestamps, g.ts_max_init, lr_b, lr_j, lr_off, m->ts_desc));
  if (g.sampling()) {      // statistics (whole vocabulary: perturbed) -> sample step; every row continues itself: the cache moves only behind the prompt pass
    WIS_RET(launch_logit_stats(st, m->logits, g.bias_all, m->bias_begin, m->bs.step_u, m->st_max, m->st_sum, m->st_val, m->st_idx, g.B, g.sc, lr_b, lr_j, lr_off, nullptr,
                               nullptr, g.ts ? m->ts_desc : nullptr, &g.sp));
    WIS_RET(launch_sample_step(st, m->st_max, m->st_sum, m->st_val, m->st_idx, m->bs, m->rm, g.B, g.P, g.sc, g.sp, g.plen));
  } else {
  WIS_RET(launch_logit_stats(st, m->logits, g.bias_all, m->bias_begin, m->bs.step_u, m->st_max, m->st_sum, m->st_val, m->st_idx, g.B, g.sc, lr_b, lr_j, lr_off, prof ? prof + 16 : nullptr,
                             nullptr, g.ts ? m->ts_desc : nullptr));
  WIS_RET(launch_beam_step(st, m->st_max, m->st_sum, m->st_val, m->st_idx, m->bs, m->rm, g.B, g.P, c.n_text_ctx, g.sc, prof, g.n_res, g.plen));
  }
  if (!(flags & TAIL_NO_CACHE) && g.plen) return launch_kv_reorder_from(st, m->kc_all, m->vc_all, m->kv_layer_stride, c.n_dec_layers, m->bs, g.B, g.beam, g.plen, c.n_text_ctx, c.d_model);
  if (!(flags & TAIL_NO_CACHE)) WIS_RET(launch_kv_reorder(st, m->kc_all, m->vc_all, m->kv_layer_stride, c.n_dec_layers, m->bs, g.B, g.beam, g.P, c.n_text_ctx, c.d_model));
  return WIS_OK;
}

// where the search stands when the step loops take over
struct Seed {
  int steps = 1;              // decoder passes done: the first step runs with the prefill pass
  bool spec_done = false;     // the draft verification already met the end of the utterance
  bool beam_fin = false;      // ... of a beam search: the replayed beam steps finished it, results are where beam_step_kernel puts them
  std::vector<int> spec_gen; float spec_cum = 0.f; int spec_len = 0;      // greedy draft: tokens generated by the verification, their score, the result's length
  int accepted = 0;           // draft tokens (beam draft: steps) verified
};

// Verification passes keep to the ticket hand-off of the cross-attention: their picks are accepted on the host pass by pass, outside the
// progress record that carries the granule form's give-up flag (advisor, round 5) - the ordinary steps behind them take the call's form again
struct TicketScope {
  wis_model* m; bool spin_call;
  explicit TicketScope(wis_model* mm) : m(mm), spin_call(mm->spin_now) { m->spin_now = false; }
  ~TicketScope() { m->spin_now = spin_call; }
};

// the progress record counts passes: `steps` of them are done when the ordinary steps resume behind a verification
static int reseed_tick(wis_model* m, int steps) {
  unsigned* tk = m->h_pin->reseed_tick;
  tk[0] = (unsigned)steps; tk[1] = m->gen; tk[2] = 0; tk[3] = 0;
  WIS_HIP_CHECK(hipMemcpyAsync(m->bs.tick, tk, 16, hipMemcpyHostToDevice, m->st));
  return WIS_OK;
}

// a (token, origin) trajectory of n steps x k beams in BeamState::traj's layout ([step][MAX_R][2]); entries of slots >= k are left alone
static void pack_traj(int* hd, const int32_t* tok, const int32_t* org, int n, int k) {
  for (int s_ = 0; s_ < n; ++s_) for (int j = 0; j < k; ++j) { hd[(s_ * MAX_R + j) * 2] = tok[s_ * k + j]; hd[(s_ * MAX_R + j) * 2 + 1] = org[s_ * k + j]; }
}

// ---- prefill + FIRST decode step in one pass: all P prompt tokens of an utterance are rows (b, i) at positions i in the
// utterance's first KV slot (causal by position); the logits of the last prompt row seed the beams (CT2 forwards
// prompt[:-1] and then feeds prompt[-1] as the first decoder input — the same arithmetic, one weight pass instead of two)
static int seed_prefill(const GenCtx& g) {
  wis_model* m = g.m; const wis_config_t& c = m->cfg; const int B = g.B, P = g.P;
  WIS_RET(dec_forward(m, B * P, P, B, true, g.beam, 0));
  // every prompt row has its logits after this pass: the <|startoftranscript|> row's are what no_speech_prob reads (raw, no processors)
  if (g.sot_row >= 0) WIS_RET(launch_no_speech(g.st, m->logits, m->n_vocab_pad, B, P, g.sot_row, c.n_vocab, c.no_speech, m->d_nsp));
  return sampling_tail(g, {P, 0, P - 1}, TAIL_TAPS);
}

// ---- the long-prompt route (P > SHORT_PROMPT): WINDOWED prefill.  Prompt positions 0 .. P - Pl - 1 are teacher-forced without logits in passes of 16
// consecutive positions per utterance over groups of at most MAX_ROWS / 16 utterances - the un-folded batched-row route wis_align forces its text through,
// with the self-attention in the TREE row-group form (every row's history in ONE slot: an ancestor table of width 1 that names the utterance's first slot
// b * beam, where the rows' K / V go) - and the last Pl = min(16, MAX_ROWS / B) prompt rows run as the merged prefill + first step of seed_prefill, at
// positions P - Pl .. P - 1: that pass has logits, the sampling tail reads its last row.  no_speech_prob reads the <|startoftranscript|> row: the window
// that holds it runs with logits too.  The prompt's K / V stays in slot b * beam for the whole search: the step's self-attention reads it there for all of
// the utterance's rows (dec_self_attn_long_kernel), a decode row keeps only the positions from P on in its own slot, and the cache reorder moves only those -
// behind this pass there is nothing to move.
static int seed_prefill_ragged(const GenCtx& g);
static int seed_prefill_long(const GenCtx& g) {
  if (g.ragged) return seed_prefill_ragged(g);
  wis_model* m = g.m; hipStream_t st = g.st; const wis_config_t& c = m->cfg; PinnedScratch* hp = m->h_pin;
  const int B = g.B, P = g.P, beam = g.beam, Pl = g.Pl, Np = P - Pl, G = MAX_ROWS / 16;
  for (int ub0 = 0; ub0 < B; ub0 += G) {
    const int nb = std::min(G, B - ub0), M = nb * 16;
    for (int r = 0; r < M; ++r) hp->base[r] = hp->anc[r] = (ub0 + r / 16) * beam;
    WIS_HIP_CHECK(hipMemcpyAsync(m->d_anc, hp->anc, (size_t)M * 4, hipMemcpyHostToDevice, st));
    WIS_HIP_CHECK(hipMemcpyAsync(m->d_base, hp->base, (size_t)M * 4, hipMemcpyHostToDevice, st));
    for (int t0 = 0; t0 < Np; t0 += 16) {
      const int n = std::min(16, Np - t0);      // (a short last window is padded with copies of its last row: the same K / V to the same place)
      std::vector<int> tok(M), pos(M), slot(M), ls(M);
      for (int r = 0; r < M; ++r) {
        const int u = ub0 + r / 16, i = std::min(r % 16, n - 1);
        tok[r] = g.prompt[u * P + t0 + i]; pos[r] = t0 + i; slot[r] = ls[r] = u * beam;
      }
      WIS_RET(upload_rows(m, tok, pos, slot, ls));      // (waits: the staging areas are free for the next window)
      const bool nsp = g.sot_row >= t0 && g.sot_row < t0 + n;
      TreeWin tw{m->d_anc, t0, 1}; tw.base = m->d_base; tw.own_kv = true;
      m->al.kv_ub0 = ub0;
      const int rc = dec_forward(m, M, 16, nb, nsp, 1, 0, &tw);
      m->al.kv_ub0 = 0;
      WIS_RET(rc);
      if (nsp) WIS_RET(launch_no_speech(st, m->logits, m->n_vocab_pad, nb, 16, g.sot_row - t0, c.n_vocab, c.no_speech, m->d_nsp + ub0));
    }
  }
  std::vector<int> tok(B * Pl), pos(B * Pl), slot(B * Pl), ls(B * Pl);
  for (int b = 0; b < B; ++b) for (int i = 0; i < Pl; ++i) { tok[b * Pl + i] = g.prompt[b * P + Np + i]; pos[b * Pl + i] = Np + i; slot[b * Pl + i] = ls[b * Pl + i] = b * beam; }
  WIS_RET(upload_rows(m, tok, pos, slot, ls, false));
  WIS_RET(dec_forward(m, B * Pl, Pl, B, true, beam, 0));
  if (g.sot_row >= Np) WIS_RET(launch_no_speech(st, m->logits, m->n_vocab_pad, B, Pl, g.sot_row - Np, c.n_vocab, c.no_speech, m->d_nsp));
  return sampling_tail(g, {Pl, 0, Pl - 1}, TAIL_TAPS | TAIL_NO_CACHE);
}

// ---- the same for prompts of DIFFERENT lengths (wis_generate_ragged): every utterance u on the long-prompt route, whatever its length P_u.  Its prefix
// positions are 0 .. Np_u - 1, Np_u = max(0, P_u - Pl); the pass of window t0 carries only the utterances with Np_u > t0 (a short last window of an
// utterance padded with copies of its last row, as above).  The row-group cross-attention finds a group's K / V by kv_ub0 + group, so a pass covers a
// RUN of consecutive utterances, in groups of at most MAX_ROWS / 16: one pass per maximal run - any order of lengths is right, the longest first needs the
// fewest passes (every run is then a head of the batch).  The last pass is right-aligned: row i of utterance u is position P_u - Pl + i, and where
// P_u < Pl the rows in front are copies of its first row (the same K / V to the same place); the sampling tail reads row Pl - 1 as ever.
// no_speech_prob: the <|startoftranscript|> row differs per utterance, and so does the pass that holds it - a pass runs with logits when any of its
// utterances has its row there, and no_speech_rows_kernel takes the rows from device memory (-1: not in this pass).
static int seed_prefill_ragged(const GenCtx& g) {
  wis_model* m = g.m; hipStream_t st = g.st; const wis_config_t& c = m->cfg; PinnedScratch* hp = m->h_pin;
  const int B = g.B, beam = g.beam, Pl = g.Pl, G = MAX_ROWS / 16;
  const bool want_nsp = !g.sot_rows.empty();
  auto prefix = [&](int u) { return std::max(0, g.plens[u] - Pl); };
  int np_max = 0;
  for (int u = 0; u < B; ++u) np_max = std::max(np_max, prefix(u));
  for (int t0 = 0; t0 < np_max; t0 += 16) {
    for (int u0 = 0; u0 < B;) {
      if (prefix(u0) <= t0) { ++u0; continue; }
      int u1 = u0;
      while (u1 < B && u1 - u0 < G && prefix(u1) > t0) ++u1;
      const int nb = u1 - u0, M = nb * 16;
      for (int r = 0; r < M; ++r) hp->base[r] = hp->anc[r] = (u0 + r / 16) * beam;
      WIS_HIP_CHECK(hipMemcpyAsync(m->d_anc, hp->anc, (size_t)M * 4, hipMemcpyHostToDevice, st));
      WIS_HIP_CHECK(hipMemcpyAsync(m->d_base, hp->base, (size_t)M * 4, hipMemcpyHostToDevice, st));
      std::vector<int> tok(M), pos(M), slot(M), ls(M);
      for (int r = 0; r < M; ++r) {
        const int u = u0 + r / 16, n = std::min(16, prefix(u) - t0), i = std::min(r % 16, n - 1);
        tok[r] = g.prompt[g.poff[u] + t0 + i]; pos[r] = t0 + i; slot[r] = ls[r] = u * beam;
      }
      bool nsp = false;
      if (want_nsp) {
        for (int b = 0; b < nb; ++b) {
          const int u = u0 + b, s_ = g.sot_rows[u] - t0;
          hp->nsp_rows[b] = (s_ >= 0 && s_ < std::min(16, prefix(u) - t0)) ? s_ : -1;
          nsp = nsp || hp->nsp_rows[b] >= 0;
        }
        if (nsp) WIS_HIP_CHECK(hipMemcpyAsync(m->d_nsp_rows, hp->nsp_rows, (size_t)nb * 4, hipMemcpyHostToDevice, st));
      }
      WIS_RET(upload_rows(m, tok, pos, slot, ls));      // (waits: the staging areas - the rows', the tables', the no-speech rows' - are free for the next pass)
      TreeWin tw{m->d_anc, t0, 1}; tw.base = m->d_base; tw.own_kv = true;
      m->al.kv_ub0 = u0;
      const int rc = dec_forward(m, M, 16, nb, nsp, 1, 0, &tw);
      m->al.kv_ub0 = 0;
      WIS_RET(rc);
      if (nsp) WIS_RET(launch_no_speech_rows(st, m->logits, m->n_vocab_pad, nb, 16, m->d_nsp_rows, c.n_vocab, c.no_speech, m->d_nsp + u0));
      u0 = u1;
    }
  }
  std::vector<int> tok(B * Pl), pos(B * Pl), slot(B * Pl), ls(B * Pl);
  for (int b = 0; b < B; ++b) for (int i = 0; i < Pl; ++i) {
    const int p = std::max(g.plens[b] - Pl + i, 0);
    tok[b * Pl + i] = g.prompt[g.poff[b] + p]; pos[b * Pl + i] = p; slot[b * Pl + i] = ls[b * Pl + i] = b * beam;
  }
  bool nsp = false;
  if (want_nsp) {
    for (int b = 0; b < B; ++b) {
      hp->nsp_rows[b] = g.sot_rows[b] >= prefix(b) ? g.sot_rows[b] - g.plens[b] + Pl : -1;
      nsp = nsp || hp->nsp_rows[b] >= 0;
    }
    if (nsp) WIS_HIP_CHECK(hipMemcpyAsync(m->d_nsp_rows, hp->nsp_rows, (size_t)B * 4, hipMemcpyHostToDevice, st));
  }
  WIS_RET(upload_rows(m, tok, pos, slot, ls, false));
  WIS_RET(dec_forward(m, B * Pl, Pl, B, true, beam, 0));
  if (nsp) WIS_RET(launch_no_speech_rows(st, m->logits, m->n_vocab_pad, B, Pl, m->d_nsp_rows, c.n_vocab, c.no_speech, m->d_nsp));
  return sampling_tail(g, {Pl, 0, Pl - 1}, TAIL_TAPS | TAIL_NO_CACHE);
}

// The decoder rows of window steps s0 .. s0 + Rw - 1 of a beam trajectory (hd: [step][MAX_R][2] = token, origin; one utterance, k beams), step-major:
// row (s, j) feeds the token live beam j got at step s - 1 at position P - 1 + s and keeps its K / V in slot j; ha[row][ANC_W] = the slot of the
// row's ancestor at every window step (entry 0 doubles as the slot that holds everything before the window).  Padded to whole groups of 16 rows
// with copies of the last row (they write the same K / V to the same place).  Returns the padded row count.
static int fill_tree_window(const int* hd, int s0, int Rw, int k, int P, std::vector<int>& tok, std::vector<int>& pos, std::vector<int>& slot, std::vector<int>& ls, int* ha) {
  const int Mreal = k * Rw, Mpad = cdiv(Mreal, 16) * 16;
  tok.assign(Mpad, 0); pos.assign(Mpad, 0); slot.assign(Mpad, 0); ls.assign(Mpad, 0);
  for (int t = 0; t < Rw; ++t) for (int j = 0; j < k; ++j) {
    const int s_ = s0 + t, r = t * k + j;
    tok[r] = hd[((s_ - 1) * MAX_R + j) * 2]; pos[r] = P - 1 + s_; slot[r] = j; ls[r] = j;
    int a = j;                                    // ancestor of (s_, j) at window step sp, walking the origins back to s0
    for (int sp = s_; sp >= s0; --sp) { ha[r * ANC_W + (sp - s0)] = a; a = hd[((sp - 1) * MAX_R + a) * 2 + 1]; }
    for (int u = t + 1; u < ANC_W; ++u) ha[r * ANC_W + u] = ha[r * ANC_W + t];
  }
  for (int r = Mreal; r < Mpad; ++r) {
    tok[r] = tok[Mreal - 1]; pos[r] = pos[Mreal - 1]; slot[r] = slot[Mreal - 1]; ls[r] = ls[Mreal - 1];
    for (int u = 0; u < ANC_W; ++u) ha[r * ANC_W + u] = ha[(Mreal - 1) * ANC_W + u];
  }
  return Mpad;
}

// ---- verify the draft of a BEAM SEARCH (round 6; BASELINE configs[4] at the reference's long-audio beam, main.py:582-586).  The draft is
// the trajectory of an earlier search over (most of) the same audio: per step s the live set it left - k tokens and the beam slot each
// continued from.  If the search over THIS window has followed it up to step s0 - 1, the decoder rows of steps s0 .. s0 + Rw - 1 are
// known without running those steps: row (s, j) feeds the draft's token of live beam j after step s - 1 at position P - 1 + s.  They form a
// TREE (a beam's history is a path through earlier live sets), so the pass runs the self-attention by ancestor table (dec_self_attn_kernel
// TREE: node (s, j) keeps its K / V in slot j, row (s, j) reads position P - 1 + s' from the slot of its ancestor at step s') and the
// cross-attention as groups of 16 rows over the utterance's one K / V.  One weight stream then yields the logits of Rw steps x k beams;
// the steps are REPLAYED on them by the ordinary sampling kernels (logit_stats, beam_step: search state and hypothesis list end up exactly
// where Rw ordinary steps would leave them), each followed by draft_match_kernel: if the live set a replayed step produced is the draft's -
// as a SET: near-tied candidates swap slots between two searches all the time, so live beam j may be any draft node as long as every beam is
// found once; the next step reads beam j's logits from the row of its node - the next step's rows were the right ones; the first step with a
// beam the draft does not have still stands (its own inputs were verified), parks the search (done = 2), and ordinary steps resume behind
// it.  The cache: the pass left node (s, i)'s K / V in slot i of the draft's numbering; the matching kernel keeps every live beam's path
// through those slots and kv_gather_kernel turns the paths into "slot j = beam j's history" once per window.  A whole window is queued
// without a host round trip; the host looks once per window.  Exact by construction: every accepted step ran beam_step_kernel on the logits
// of its true inputs (summed in the multi-row order, as any other batch shape of the engine).
static int seed_beam_draft(const GenCtx& g, Seed* sd) {
  wis_model* m = g.m; hipStream_t st = g.st; const wis_config_t& c = m->cfg; PinnedScratch* hp = m->h_pin;
  const int P = g.P, beam = g.beam, max_new = g.max_new, ctx = c.n_text_ctx;
  const SampleCfg& sc = g.sc;
  const int k = beam;
  const int nd = std::min(g.n_draft, max_new - 1);
  int* hd = hp->draft;                                // the draft in BeamState::traj's layout ([step][MAX_R][2])
  pack_traj(hd, g.draft, g.draft_org, nd, k);
  int* hv = hp->vstate;                               // staging of the verification state (dec_kernels.hip draft_match_kernel: vs), read back per window
  for (int i = 0; i < 32; ++i) hv[i] = 0;
  for (int j = 0; j < MAX_R; ++j) { hv[DRAFT_VS_PERM + j] = j; hv[DRAFT_VS_BASE + j] = j; }
  if (nd > 0) WIS_HIP_CHECK(hipMemcpyAsync(m->d_draft, hd, (size_t)nd * MAX_R * 2 * 4, hipMemcpyHostToDevice, st));
  WIS_HIP_CHECK(hipMemcpyAsync(m->d_vstate, hv, 32 * 4, hipMemcpyHostToDevice, st));
  // merged prefill + first step as in the ordinary call (a tap build stamps neither kernel here), then: is the search where the draft's step 0 says?
  WIS_RET(dec_forward(m, P, P, 1, true, beam, 0));
  WIS_RET(sampling_tail(g, {P, 0, P - 1}, 0));
  WIS_RET(launch_draft_match(st, m->bs, m->d_draft, nd, k, m->d_vstate, 0));
  const int RW = std::min(ANC_W, MAX_ROWS / k);       // steps per window: k x RW rows (beam 2 / 3: 32 steps, 5: 19, 8: 12), padded to whole groups of 16
  const int s_last = std::min(nd, max_new - 1);       // last step a window can hold: rows from the draft's entry s - 1; step max_new - 1 ends every search
  int* ha = hp->anc;                                  // ancestor table of the window rows, [rows][ANC_W]
  int* hb = hp->base;                                 // ... and the slot holding each row's history before the window, [rows]
  int* hw2 = hp->path_reset;                          // per-window reset of the path bookkeeping: vs[2] = 0, vs[16 + j] = j
  int done_flag = 0, step_dev = 0;
  int pinv[MAX_R];                                    // real slot of draft node i at the window's start (the matching read back at the previous sync)
  for (int j = 0; j < MAX_R; ++j) pinv[j] = j;        // (first window: every slot holds the same prompt rows - any assignment is right)
  for (int s0 = 1;; ) {
    const int Rw = std::min(RW, s_last - s0 + 1);
    if (Rw >= 1) {
      std::vector<int> tok, pos, slot, ls;
      const int Mpad = fill_tree_window(hd, s0, Rw, k, P, tok, pos, slot, ls, ha);
      for (int r = 0; r < Mpad; ++r) hb[r] = pinv[ha[r * ANC_W]];      // the row's window-step-0 ancestor is draft node ha[r][0]: its earlier history sits in that node's REAL slot
      // the window's rows go through a row table of their own: the search's table (next input rows, written by the last beam step that
      // counted) must survive a window that turns out to sit behind a parked search (queued before the host has looked)
      const RowMeta rm_search = m->rm;
      m->rm = m->rm_win;
      int rc = upload_rows(m, tok, pos, slot, ls, false, &hp->win_rows);      // (the prompt rows' staging copy may still be pending: own area; windows are a sync apart)
      if (!rc && (hipMemcpyAsync(m->d_anc, ha, (size_t)Mpad * ANC_W * 4, hipMemcpyHostToDevice, st) != hipSuccess ||
                  hipMemcpyAsync(m->d_base, hb, (size_t)Mpad * 4, hipMemcpyHostToDevice, st) != hipSuccess)) { set_error("draft window: ancestor table upload failed"); rc = WIS_E_HIP; }
      TreeWin tw{m->d_anc, P - 1 + s0, ANC_W}; tw.base = m->d_base;
      if (!rc) rc = dec_forward(m, Mpad, 16, Mpad / 16, true, 1, 0, &tw);
      m->rm = rm_search;
      WIS_RET(rc);
      hw2[0] = 0; for (int j = 0; j < MAX_R; ++j) hw2[1 + j] = j;
      WIS_HIP_CHECK(hipMemcpyAsync(m->d_vstate + 2, hw2, 4, hipMemcpyHostToDevice, st));
      WIS_HIP_CHECK(hipMemcpyAsync(m->d_vstate + DRAFT_VS_BASE, hw2 + 1, MAX_R * 4, hipMemcpyHostToDevice, st));
      for (int t = 0; t < Rw; ++t) {      // replay: beam j's logits come from the row of the draft node it is matched to (rowmap); no cache traffic per step
        WIS_RET(launch_logit_stats(st, m->logits, g.bias_all, m->bias_begin, m->bs.step_u, m->st_max, m->st_sum, m->st_val, m->st_idx, 1, sc, beam, 1, t * k, nullptr, m->d_vstate + DRAFT_VS_PERM));
        WIS_RET(launch_beam_step(st, m->st_max, m->st_sum, m->st_val, m->st_idx, m->bs, m->rm, 1, P, ctx, sc));
        WIS_RET(launch_draft_match(st, m->bs, m->d_draft, nd, k, m->d_vstate, 1));
      }
      // the window's paths applied to the cache at once: slot j = live beam j's history, as ordinary steps (and the next window) expect it
      WIS_RET(launch_kv_gather(st, m->kc_all, m->vc_all, m->kv_layer_stride, c.n_dec_layers, m->d_vstate, m->bs.done, beam, P - 1 + s0, ctx, c.d_model));
    }
    WIS_HIP_CHECK(hipMemcpyAsync(hv, m->d_vstate, 16 * 4, hipMemcpyDeviceToHost, st));      // steps verified, ..., the matching
    WIS_HIP_CHECK(hipMemcpyAsync(&hp->win_done, m->bs.done, 4, hipMemcpyDeviceToHost, st));
    WIS_HIP_CHECK(hipMemcpyAsync(&hp->win_step, m->bs.step_u, 4, hipMemcpyDeviceToHost, st));
    WIS_HIP_CHECK(hipStreamSynchronize(st));
    done_flag = hp->win_done; step_dev = hp->win_step;
    if (Rw < 1 || done_flag != 0) break;
    for (int j = 0; j < k; ++j) { const int n_ = hv[DRAFT_VS_PERM + j]; if (n_ >= 0 && n_ < k) pinv[n_] = j; }
    s0 += Rw;
  }
  sd->accepted = hv[0];
  __atomic_store_n(&m->h_prog[HP_REC], 0ull, __ATOMIC_RELAXED);      // the replayed steps' progress records count launches, not steps: the pacing loop starts from `steps`
  if (done_flag == 1) {      // the replayed steps ended the search: hypotheses ranked, result written by beam_step_kernel
    sd->beam_fin = true; sd->steps = step_dev + 1;
  } else {                   // parked behind a step that stands (or nothing to verify): ordinary steps resume
    sd->steps = step_dev;
    if (sd->steps < 1) { set_error("wis_generate_draft_beam: verification completed no step"); return WIS_E_STATE; }
    WIS_RET(reseed_tick(m, sd->steps));
    WIS_HIP_CHECK(hipMemsetAsync(m->bs.done, 0, 4, st));
  }
  return WIS_OK;
}

// ---- verify the draft: the prompt and the draft tokens go through the decoder as teacher-forced rows, 16 positions per pass
// (causal by position inside the utterance's KV slot, like the merged prompt pass); row i's logits are what a greedy step fed
// seq[i] after seq[0..i-1] sees, so as long as every earlier draft token equalled the greedy pick, row P-1+g yields generated
// token g.  The first disagreement ends the verification WITH the right token for that index (its prefix was right); the K / V
// rows of the accepted prefix are in the cache, and the ordinary step loop continues from there.  Per pass one weight stream
// for up to 16 tokens instead of one per token.
static int seed_greedy_draft(const GenCtx& g, Seed* sd) {
  wis_model* m = g.m; hipStream_t st = g.st; const wis_config_t& c = m->cfg; PinnedScratch* hp = m->h_pin;
  const int P = g.P, max_new = g.max_new;
  const int32_t* draft = g.draft;
  const int nd = std::min(g.n_draft, max_new - 1);
  std::vector<int> seq(P + nd);
  for (int i = 0; i < P; ++i) seq[i] = g.prompt[i];
  for (int i = 0; i < nd; ++i) seq[P + i] = draft[i];
  // (r6) up to 96 positions per pass: more than 16 rows of one utterance go through the row-group form of the tree pass (a chain is a tree whose
  // every ancestor sits in slot 0: dec_self_attn_kernel<TREE> with an all-zero table is "causal by position in the slot", the cross-attention
  // takes the rows as groups of 16 over the one K / V) - the 100 rows of a 96-token draft are 2 passes (3.5 + 1.3 ms) instead of 7 x 1.35 ms.
  // WIS_DRAFT_ROWS=16: the round-5 schedule (A/B)
  static const int env_rows = getenv("WIS_DRAFT_ROWS") ? atoi(getenv("WIS_DRAFT_ROWS")) : 0;
  const int R = (env_rows >= 16 && env_rows <= MAX_ROWS) ? env_rows / 16 * 16 : MAX_ROWS;
  bool stop = false; int n_acc = 0;
  for (int t0 = 0; t0 < P + nd && !stop; t0 += R) {
    const int rows = std::min(R, P + nd - t0);
    const int f = std::max(P - 1 - t0, 0), nv = rows - f;      // rows f .. rows-1 of this pass predict generated tokens
    const int Mp = rows > 16 ? cdiv(rows, 16) * 16 : rows;      // (row groups: padded with copies of the last row - same K / V to the same place)
    std::vector<int> tok(Mp), pos(Mp), slot(Mp, 0), ls(Mp, 0);
    for (int i = 0; i < Mp; ++i) { const int ii = std::min(i, rows - 1); tok[i] = seq[t0 + ii]; pos[i] = t0 + ii; }
    WIS_RET(upload_rows(m, tok, pos, slot, ls));
    if (rows > 16) {
      WIS_HIP_CHECK(hipMemsetAsync(m->d_anc, 0, (size_t)Mp * 16 * 4, st));
      const TreeWin tw{m->d_anc, t0, 16};
      WIS_RET(dec_forward(m, Mp, 16, Mp / 16, nv > 0, 1, 0, &tw));
    } else
    WIS_RET(dec_forward(m, rows, rows, 1, nv > 0, 1, 0));
    if (nv <= 0) continue;
    int* hv = hp->vstep;
    for (int i = 0; i < nv; ++i) hv[i] = t0 + f + i - (P - 1);      // the step index of each verified row (first-step / EOT masks of logit_stats_kernel)
    WIS_HIP_CHECK(hipMemcpyAsync(m->vstep, hv, (size_t)nv * 4, hipMemcpyHostToDevice, st));
    WIS_RET(launch_logit_stats(st, m->logits, g.bias_all, m->bias_begin, m->vstep, m->st_max, m->st_sum, m->st_val, m->st_idx, nv, g.sc, 1, 0, f));
    WIS_RET(launch_greedy_pick(st, m->st_max, m->st_sum, m->st_val, m->st_idx, nv, g.sc, m->pick_tok, m->pick_lp));
    int* ht = hp->pick_tok; float* hl = hp->pick_lp;
    WIS_HIP_CHECK(hipMemcpyAsync(ht, m->pick_tok, (size_t)nv * 4, hipMemcpyDeviceToHost, st));
    WIS_HIP_CHECK(hipMemcpyAsync(hl, m->pick_lp, (size_t)nv * 4, hipMemcpyDeviceToHost, st));
    WIS_HIP_CHECK(hipStreamSynchronize(st));
    for (int i = 0; i < nv && !stop; ++i) {
      const int gi = hv[i];
      sd->spec_cum = hl[i] + sd->spec_cum;                 // beam_step_kernel: (logit - lse) + cum
      sd->spec_gen.push_back(ht[i]);
      const bool eos = ht[i] == c.eot, is_last = gi + 1 >= max_new;
      if (eos || is_last) { sd->spec_done = true; sd->spec_len = eos ? gi : gi + 1; stop = true; }
      else if (gi < nd && ht[i] == draft[gi]) ++n_acc;
      else stop = true;                                  // first disagreement (or the row behind the last draft token): ht[i] is generated token gi
    }
  }
  sd->accepted = n_acc;
  const int steps = sd->steps = (int)sd->spec_gen.size();
  if (steps < 1) { set_error("wis_generate_draft: verification produced no token"); return WIS_E_STATE; }
  if (!sd->spec_done) {
    // the search state a run of `steps` ordinary steps would have left: history, cumulative score, next input row, counters
    int* hs = hp->hist;
    for (int t = 0; t < steps; ++t) hs[t] = sd->spec_gen[t];
    WIS_HIP_CHECK(hipMemcpyAsync(m->bs.alive, hs, (size_t)steps * 4, hipMemcpyHostToDevice, st));
    auto& hw = hp->seed;
    hw.step = steps; hw.tok = sd->spec_gen.back(); hw.pos = P - 1 + steps; hw.slot = 0; hw.cum = sd->spec_cum;
    WIS_HIP_CHECK(hipMemcpyAsync(m->bs.step_u, &hw.step, 4, hipMemcpyHostToDevice, st));
    WIS_HIP_CHECK(hipMemcpyAsync(m->rm.tok, &hw.tok, 4, hipMemcpyHostToDevice, st));
    WIS_HIP_CHECK(hipMemcpyAsync(m->rm.pos, &hw.pos, 4, hipMemcpyHostToDevice, st));
    WIS_HIP_CHECK(hipMemcpyAsync(m->rm.slot, &hw.slot, 4, hipMemcpyHostToDevice, st));
    WIS_HIP_CHECK(hipMemcpyAsync(m->rm.lslot, &hw.slot, 4, hipMemcpyHostToDevice, st));
    WIS_HIP_CHECK(hipMemcpyAsync(m->bs.cum, &hw.cum, 4, hipMemcpyHostToDevice, st));
    WIS_RET(reseed_tick(m, steps));
  }
  return WIS_OK;
}

// The decode step - one decoder pass over the search's rows and its sampling tail - captured once per shape into a HIP graph and replayed.
// The step graph comes in up to three forms that differ in ONE kernel argument set: how many 8-position blocks of its rows' K / V history the self-attention
// asks for (dec_self_attn_kernel NB).  Every row of the pass that follows s beam steps has P + s positions - known HERE, by the step index, although the graph's
// kernel arguments are frozen - so the pass is launched from the graph whose self-attention asks for 16 / 32 / 64 positions (WIS_SA_NB=0: always 64, A/B switch).
struct StepGraph {
  const GenCtx& g;
  ~StepGraph() { g.m->sa_nb = 8; }      // (everything outside the step loops - prefill, verification windows, taps - asks for 64)

  int nb_for(int passes_done) const {
    static const bool sa_short = !(getenv("WIS_SA_NB") && atoi(getenv("WIS_SA_NB")) == 0);
    const int len = g.P + passes_done;
    return (!sa_short || g.long_p) ? 8 : (len <= 16 ? 2 : (len <= 32 ? 4 : 8));
  }
  int one_step() const {
    g.m->sa_plen = g.plen; g.m->sa_w0 = g.P;      // (the long-prompt route: the pass's self-attention over the shared prefix)
    const int rc = dec_forward(g.m, g.B * g.beam, g.beam, g.B, true, g.beam, 1);
    g.m->sa_plen = nullptr;
    WIS_RET(rc);
    return sampling_tail(g, {g.beam, 1, 0}, TAIL_TAPS | (g.sampling() ? TAIL_NO_CACHE : 0));      // (a sample's row continues itself: nothing to reorder after the first step)
  }
  int graph_for(int nb, hipGraphExec_t* out) const {
    wis_model* m = g.m; const SampleCfg& sc = g.sc;
    GraphKey key; memset(&key, 0, sizeof(key));
    key.B = g.B; key.beam = g.beam; key.P = (g.long_p && sa_long_kernel(m)) ? -1 : g.P /* one sentinel for the whole long-prompt route (its TREE form keeps w0 = P as a kernel argument) */; key.max_new = g.max_new; key.fixed_new = sc.fixed_new; key.suppress_blank = sc.suppress_blank;
    key.suppress_default = g.o->suppress_default; key.early_exit = sc.allow_early_exit; key.lp = sc.length_penalty; key.patience = g.patience; key.spin = m->spin_now ? 1 : 0;
    key.sa_nb = nb;
    key.timestamps = g.ts ? 1 : 0; key.max_init = g.ts ? g.ts_max_init : 0;
    key.rep_pen = g.rep_pen == 1.f ? 0.f : g.rep_pen; key.rep_ngram = g.rep_ngram;      // (off: the zeroes of a key that never knew the fields)
    key.samp_topk = g.sp.topk; key.samp_T = g.sampling() ? g.sp.T : 0.f; key.n_hyp = g.n_res > 1 ? g.n_res : 0;      // (the seeds are device memory: no part of the key)
    key.phrases = g.phrases ? (g.phr_mass ? 2 : 1) : 0;      // (the set is device memory behind a pointer that never changes: installing another needs no new graph)
    key.hotwords = g.hotwords ? 1 : 0;      // (the set, its record count and the boost are device memory behind pointers that never change: one graph serves every set and every boost)
    auto it = m->graphs.find(key);
    if (it != m->graphs.end()) { *out = it->second; return WIS_OK; }
    hipGraph_t graph = nullptr; hipGraphExec_t ge = nullptr;
    WIS_HIP_CHECK(hipStreamBeginCapture(g.st, hipStreamCaptureModeThreadLocal));
    int rc = one_step();
    hipError_t e = hipStreamEndCapture(g.st, &graph);
    if (rc) { if (graph) hipGraphDestroy(graph); return rc; }
    if (e != hipSuccess) { set_error("graph capture failed: %s", hipGetErrorString(e)); return WIS_E_HIP; }
    e = hipGraphInstantiate(&ge, graph, nullptr, nullptr, 0);
    hipGraphDestroy(graph);
    if (e != hipSuccess) { set_error("graph instantiate failed: %s", hipGetErrorString(e)); return WIS_E_HIP; }
    m->graphs[key] = ge;
    *out = ge;
    return WIS_OK;
  }
  int launch_pass(int passes_done) const {      // the decoder pass + sampling that follows `passes_done` passes
    wis_model* m = g.m;
    m->sa_nb = nb_for(passes_done);
    if (!m->use_graph) return one_step();
    hipGraphExec_t ge = nullptr;
    WIS_RET(graph_for(m->sa_nb, &ge));
    WIS_HIP_CHECK(hipGraphLaunch(ge, g.st));
    return WIS_OK;
  }
};

// what a step loop leaves behind
struct LoopResult {
  int steps;                    // decoder passes enqueued (the seed's included)
  int needed = 0;               // steps after which the last utterance had finished (natural termination)
  bool gave_up = false;         // a combiner's bounded spin ran out: the results are garbage, the call is repeated
  bool from_host = false;       // the results are in the host-mapped progress block
  float decode_ms_dev = -1.f;   // decode time by the device clock (from_host)
};
// the search's progress record: {generation, steps, give-up, utterances done} - a record of another generation reads as nothing
static void unpack_progress(const wis_model* m, int* st_, int* dn_, int* gu_) {
  const unsigned long long r = __atomic_load_n(&m->h_prog[HP_REC], __ATOMIC_ACQUIRE);
  if ((r >> 48) != (unsigned long long)m->gen) { *st_ = 0; *dn_ = 0; *gu_ = 0; return; }
  *st_ = (int)((r >> 32) & 0xFFFFu); *gu_ = (int)((r >> 16) & 0xFFFFu); *dn_ = (int)(r & 0xFFFFu);
}
static int check_terminated(const GenCtx& g, LoopResult* lr, int dn_, int gu_) {
  lr->gave_up = gu_ != 0;
  if (!lr->gave_up && dn_ < g.B) { set_error("decode did not terminate within %d steps (done %d of %d)", lr->steps, dn_, g.B); return WIS_E_STATE; }
  return WIS_OK;
}

static inline void cpu_relax() {
#if !defined(__HIP_DEVICE_COMPILE__) && defined(__x86_64__)
  __builtin_ia32_pause();
#endif
}

// With the measurement convention the step count is known (fixed_new tokens + the forced EOT): every step goes out in one burst, nothing to
// find out from the device before the last one
static int run_burst(const GenCtx& g, const StepGraph& sg, int limit, LoopResult* lr) {
  wis_model* m = g.m;
  for (; lr->steps < limit; ++lr->steps) WIS_RET(sg.launch_pass(lr->steps));
  WIS_HIP_CHECK(hipEventRecord(m->ev[5], g.st));
  WIS_HIP_CHECK(hipStreamSynchronize(g.st));
  int st_, dn_, gu_; unpack_progress(m, &st_, &dn_, &gu_);
  WIS_RET(check_terminated(g, lr, dn_, gu_));
  lr->needed = lr->steps;
  return WIS_OK;
}

// A search that ends on EOT (every real request: the reference passes no max_length, main.py:687-693).  The host keeps `depth`
// steps enqueued beyond the last one it has seen complete (one running, one waiting behind it: the device never idles between
// steps) and reads the search's progress from the host-mapped record beam_step_kernel writes at the end of every step - no
// stream drain, no copy.  When the record says every utterance has finished, at most depth - 1 further steps are in the queue;
// they run on finished utterances (every sampling workgroup returns at its `done` test, results stay as they are) and this
// call does not wait for them: the results are already in host memory, the next call on the handle queues behind them.
// base_done: passes a draft verification stands for - done before the first progress record of this call.
static int run_paced(const GenCtx& g, const StepGraph& sg, int limit, int base_done, LoopResult* lr) {
  wis_model* m = g.m; const int B = g.B;
  int& steps = lr->steps;
  const auto t_dec0 = std::chrono::steady_clock::now();
  const int depth = g.o->queue_depth > 0 ? g.o->queue_depth : 2;
  auto t_last = std::chrono::steady_clock::now();
  int seen = -1, st_ = 0, dn_ = 0, gu_ = 0;
  static const bool trace = getenv("WIS_EOT_TRACE") != nullptr;      // per-step record of the pacing loop on stderr (tuning)
  struct Tr { int step; unsigned long long dev; double host_us; int launched; };
  std::vector<Tr> tr;
  const auto t_loop = std::chrono::steady_clock::now();
  for (unsigned spins = 0;; ++spins) {
    unpack_progress(m, &st_, &dn_, &gu_);
    if (st_ < base_done) st_ = base_done;
    if (dn_ >= B || gu_) break;
    if (st_ >= limit) break;                 // (cannot happen: the max_new-th step finishes every utterance)
    if (steps < limit && steps - st_ < depth) {
      const auto tl0 = std::chrono::steady_clock::now();
      WIS_RET(sg.launch_pass(steps));
      ++steps;
      if (trace) tr.push_back({-steps, 0ull, std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - tl0).count(), steps});      // (negative step: a launch, host_us = its duration)
      continue;
    }
    if (st_ != seen) {
      seen = st_; t_last = std::chrono::steady_clock::now(); spins = 0;
      if (trace) tr.push_back({st_, m->h_prog[HP_STAMP], std::chrono::duration<double, std::micro>(t_last - t_loop).count(), steps});
    }
    else if ((spins & 1023u) == 1023u) {
      const double idle = std::chrono::duration<double>(std::chrono::steady_clock::now() - t_last).count();
      if (idle > 30.0) { set_error("decode made no progress for 30 s (step %d of %d enqueued)", st_, steps); return WIS_E_HIP; }
      if (idle > 200e-6) { struct timespec ts = {0, 20000}; nanosleep(&ts, nullptr); }      // long steps (big batches): stop burning the core
    }
    cpu_relax();
  }
  if (trace) {
    unsigned long long prev_dev = 0;
    for (size_t i = 0; i < tr.size(); ++i) {
      if (tr[i].step < 0) { fprintf(stderr, "[eot-trace]   launch of step %d took the host %.1f us\n", -tr[i].step, tr[i].host_us); continue; }
      fprintf(stderr, "[eot-trace] step %d seen by the host at %.1f us (device clock +%.1f us since the previous record), %d steps enqueued\n", tr[i].step, tr[i].host_us,
              prev_dev ? (double)(tr[i].dev - prev_dev) * 0.01 : 0.0, tr[i].launched);
      prev_dev = tr[i].dev;
    }
    fprintf(stderr, "[eot-trace] done seen at %.1f us: %d of %d utterances, %d steps enqueued\n", std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t_loop).count(), dn_, B, steps);
  }
  WIS_RET(check_terminated(g, lr, dn_, gu_));
  if (!lr->gave_up) {
    lr->from_host = true;
    lr->needed = (int)m->h_prog[HP_DONE_STEP];
    const unsigned long long s0 = m->h_prog[HP_STAMP0], s1 = m->h_prog[HP_DONE_STAMP];
    lr->decode_ms_dev = s1 > s0 ? (float)((double)(s1 - s0) * 1e-5) : 0.f;      // 100 MHz constant clock; from the end of the first beam step (ev[4] is one kv_reorder later)
    if (g.drafting) lr->decode_ms_dev = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t_dec0).count();      // (no first beam step of its own: host clock)
  }
  return WIS_OK;
}

// ---- results: out_ids is [B][max_new] (beam_step_kernel indexes by the resolved max_new; the allocations are [.][MAX_STEPS])
// the verification rows already contained the end of the utterance: beam_step_kernel's finalisation, on the host
static void results_from_verification(const GenCtx& g, const Seed& sd, int32_t* out_ids, int32_t* out_len, float* out_score) {
  float sfin = sd.spec_cum;
  if (g.sc.length_penalty != 0.f) sfin /= powf((float)sd.spec_len, g.sc.length_penalty);
  out_len[0] = sd.spec_len;
  for (int t = 0; t < g.max_new; ++t) out_ids[t] = t < sd.spec_len ? sd.spec_gen[t] : 0;
  if (out_score) out_score[0] = sfin;
}
// the record beam_step_kernel left in the host-mapped progress block when the last utterance finished
static int results_from_record(const GenCtx& g, int32_t* out_ids, int32_t* out_len, float* out_score) {
  const wis_model* m = g.m; const int max_new = g.max_new;
  const int* hl = hp_out_len(m->h_prog); const float* hs = hp_out_score(m->h_prog); const int* hi = hp_out_ids(m->h_prog);
  for (int b = 0; b < g.B * g.n_res; ++b) {      // (result i of utterance u at u n_res + i)
    int n = hl[b];
    if (n < 0 || n > max_new) { set_error("decode result %d of utterance %d has length %d outside [0, %d]", b % g.n_res, b / g.n_res, n, max_new); return WIS_E_STATE; }
    out_len[b] = n;
    for (int t = 0; t < max_new; ++t) out_ids[(size_t)b * max_new + t] = t < n ? hi[(size_t)b * max_new + t] : 0;
    if (out_score) out_score[b] = hs[b];
  }
  return WIS_OK;
}
// a copy of the search's device-side result (drains the stream)
static int results_from_device(wis_model* m, int B, int max_new, int32_t* out_ids, int32_t* out_len, float* out_score) {
  hipStream_t st = m->st;
  std::vector<int32_t> ids((size_t)B * MAX_STEPS);
  std::vector<float> sc_h(B);
  WIS_HIP_CHECK(hipMemcpyAsync(ids.data(), m->bs.out_ids, (size_t)B * MAX_STEPS * 4, hipMemcpyDeviceToHost, st));
  WIS_HIP_CHECK(hipMemcpyAsync(out_len, m->bs.out_len, (size_t)B * 4, hipMemcpyDeviceToHost, st));
  WIS_HIP_CHECK(hipMemcpyAsync(sc_h.data(), m->bs.out_score, (size_t)B * 4, hipMemcpyDeviceToHost, st));
  WIS_HIP_CHECK(hipStreamSynchronize(st));
  for (int b = 0; b < B; ++b) {
    if (out_len[b] > max_new) out_len[b] = max_new;
    for (int t = 0; t < max_new; ++t) out_ids[(size_t)b * max_new + t] = t < out_len[b] ? ids[(size_t)b * max_new + t] : 0;
    if (out_score) out_score[b] = sc_h[b];
  }
  return WIS_OK;
}

static void record_timing(const GenCtx& g, const LoopResult& lr) {
  wis_model* m = g.m;
  const auto t1 = std::chrono::steady_clock::now();
  float ms;
  hipEventElapsedTime(&ms, m->ev[0], m->ev[1]); m->timing.logmel_ms = ms;
  hipEventElapsedTime(&ms, m->ev[1], m->ev[2]); m->timing.encoder_ms = ms;
  if (m->front_skipped) m->timing.logmel_ms = m->timing.encoder_ms = 0.f;      // encoder output was handed in: the stages did not run
  hipEventElapsedTime(&ms, m->ev[2], m->ev[3]); m->timing.crosskv_ms = ms;
  hipEventElapsedTime(&ms, m->ev[3], m->ev[4]); m->timing.prefill_ms = ms;
  if (lr.from_host) m->timing.decode_ms = lr.decode_ms_dev; else { hipEventElapsedTime(&ms, m->ev[4], m->ev[5]); m->timing.decode_ms = ms; }
  m->timing.total_ms = std::chrono::duration<float, std::milli>(t1 - g.t0).count();
  m->timing.decode_steps = lr.steps;            // steps enqueued (the merged prefill + first step included)
  m->timing.decode_steps_needed = lr.needed;    // steps after which every utterance had finished: steps - needed = over-run
}

// accepted: draft tokens (wis_generate_draft) / steps (wis_generate_draft_beam) verified
static int generate_impl(wis_model_t* m, const float* input, int B, const int32_t* prompt, int P,
                 const wis_gen_opts_t* o, int32_t* out_ids, int32_t* out_len, float* out_score, bool* retry,
                 const int32_t* draft = nullptr, int n_draft = 0, int* accepted = nullptr, const int32_t* draft_org = nullptr,
                 const uint64_t* seeds = nullptr, bool single = true, const int32_t* plen_v = nullptr) {
  *retry = false;
  if (accepted) *accepted = 0;
  m->nsp_B = 0; m->phr_mass_B = 0;
  WIS_HIP_CHECK(hipSetDevice(m->device));
  SpinClaim claim(m, B);
  GenCtx g;
  WIS_RET(make_gen_ctx(m, input, B, prompt, P, o, draft, n_draft, draft_org, seeds, single, plen_v, &g));
  hipStream_t st = g.st;
  if (g.phr_mass) WIS_RET(phrase_mass_begin(m, B, st));
  if (g.hotwords) WIS_RET(hotword_begin(m, g.hot_boost, st));
  WIS_RET(stage_search(g));
  WIS_RET(front_half(g));

  Seed sd;
  if (g.long_p) WIS_RET(seed_prefill_long(g));
  else if (!g.drafting) WIS_RET(seed_prefill(g));
  else {
    TicketScope ticket(m);
    WIS_RET(g.beam_draft ? seed_beam_draft(g, &sd) : seed_greedy_draft(g, &sd));
    if (accepted) *accepted = sd.accepted;
  }
  WIS_HIP_CHECK(hipEventRecord(m->ev[4], st));
  if (sd.beam_fin) WIS_HIP_CHECK(hipEventRecord(m->ev[5], st));

  const StepGraph sg{g};
  LoopResult lr; lr.steps = sd.steps;
  // with the measurement convention the step count is known: fixed_new tokens + the forced EOT
  const int known = (g.sc.fixed_new > 0) ? std::min(g.max_new, g.sc.fixed_new + 1) : 0;
  if (sd.spec_done || sd.beam_fin) lr.needed = sd.steps;
  else if (known) WIS_RET(run_burst(g, sg, known, &lr));
  else WIS_RET(run_paced(g, sg, g.max_new, g.drafting ? sd.steps : 0, &lr));
  // the granule hand-off's give-up flag (a combiner's bounded spin ran out: another handle's chain held the CUs its producers needed).
  // Not an error for the caller: the handle keeps to the ticket hand-off from now on and the call is run again (generate_with_retry).
  if (lr.gave_up) {
    WIS_HIP_CHECK(hipMemsetAsync(m->ca_epoch, 0, 4, st));
    WIS_HIP_CHECK(hipStreamSynchronize(st));
    m->spin_off = true; *retry = true; ++m->handoff_retries;
    fprintf(stderr, "[wis_hip] device %d: decoder cross-attention granule hand-off timed out; this handle uses the ticket hand-off from now on, the call is repeated\n", m->device);
    return WIS_OK;
  }
  if (sd.spec_done) { results_from_verification(g, sd, out_ids, out_len, out_score); lr.from_host = true; lr.decode_ms_dev = 0.f; }
  else if (lr.from_host) WIS_RET(results_from_record(g, out_ids, out_len, out_score));
  else WIS_RET(results_from_device(m, B * g.n_res, g.max_new, out_ids, out_len, out_score));
  record_timing(g, lr);
  if (lr.steps > lr.needed) { claim.defer(st); m->overrun_left = true; }      // an over-run step is still queued: its combiners keep their share of the spin budget until it has run
  if (g.nsp()) m->nsp_B = B;
  if (g.phr_mass) WIS_RET(phrase_mass_end(m, B, g.n_res, g.max_new, st));      // (behind an over-run step too: a finished utterance's rows write no slot)
  return WIS_OK;
}

// runs the call, and once more if the granule hand-off gave up: the second run takes the ticket hand-off (spin_off is set), which cannot time out
static int generate_with_retry(const char* who, wis_model_t* m, const float* input, int B, const int32_t* prompt, int P, const wis_gen_opts_t* o,
                               int32_t* out_ids, int32_t* out_len, float* out_score,
                               const int32_t* draft = nullptr, int n_draft = 0, int* accepted = nullptr, const int32_t* draft_org = nullptr,
                               const uint64_t* seeds = nullptr, bool single = true, const int32_t* plen_v = nullptr) {
  bool retry = false;
  for (int attempt = 0; attempt < 2; ++attempt) {
    WIS_RET(generate_impl(m, input, B, prompt, P, o, out_ids, out_len, out_score, &retry, draft, n_draft, accepted, draft_org, seeds, single, plen_v));
    if (!retry) return WIS_OK;
  }
  set_error("%s: hand-off flag raised without the granule path", who);
  return WIS_E_STATE;
}

// wis_debug_search / wis_debug_search_n: the sampling tail over a caller's logits table (single: one hypothesis per utterance)
static int debug_search_impl(const char* who, wis_model_t* m, const float* logits, int n_steps, int B, const wis_gen_opts_t* o, const uint64_t* seeds, const uint32_t* noise,
                             bool single, int32_t* out_ids, int32_t* out_len, float* out_score, int32_t* out_finish_step, int32_t* out_parent) {
  WIS_HIP_CHECK(hipSetDevice(m->device));
  m->phr_mass_B = 0;
  const wis_config_t& c = m->cfg;
  SampleCtx g;      // a search over given logits: a one-token prompt
  int beam = 1;     // rows per utterance: beams, or the samples of a sampled decode
  WIS_RET(resolve_sample_opts(o, single, false, &g, &beam));
  WIS_RET(check_batch(m, B, beam));
  if (!g.sampling()) WIS_RET(check_patience(beam, o->patience));
  int max_new = o->max_new_tokens > 0 ? std::min(o->max_new_tokens, MAX_STEPS) : n_steps;
  WIS_RET(resolve_hotword_opts(m, o, false, &g));
  WIS_RET(resolve_phrase_opts(m, o, false, &g, &max_new));
  if (max_new > n_steps) { set_error("%s: %d steps of logits for max_new_tokens %d", who, n_steps, max_new); return WIS_E_ARG; }
  hipStream_t st = m->st;
  if (g.phr_mass) WIS_RET(phrase_mass_begin(m, B, st));
  if (g.hotwords) WIS_RET(hotword_begin(m, g.hot_boost, st));
  const int Mrows = B * beam, V = c.n_vocab;
  float patience;
  WIS_RET(resolve_rep_opts(o, &g));
  if (noise && !g.sampling()) { set_error("%s: a noise table without sampling", who); return WIS_E_ARG; }
  struct DevBlock { void* p = nullptr; ~DevBlock() { if (p) hipFree(p); } } d_noise;      // one step of the noise table [Mrows][V]
  if (noise && hipMalloc(&d_noise.p, (size_t)Mrows * V * 4) != hipSuccess) { (void)hipGetLastError(); set_error("%s: out of device memory", who); return WIS_E_NOMEM; }
  WIS_RET(init_beam_state(m, B, beam, g.sampling(), g.sampling() ? beam : g.n_res));
  if (g.sampling()) WIS_RET(upload_seeds(m, seeds, B));
  g.m = m; g.st = st; g.B = B; g.P = 1; g.beam = beam;
  g.sc = make_sample_cfg(m, o, beam, max_new, &patience);
  apply_sample_opts(m, &g);
  g.sp.noise = static_cast<const unsigned*>(d_noise.p);
  g.bias_all = o->suppress_default ? m->bias_all : nullptr;
  g.ts = o->timestamps != 0;
  g.ts_max_init = o->max_initial_timestamp_index < 0 ? -1 : o->max_initial_timestamp_index;
  std::vector<int> done(B, 0), fin(B, -1), par(Mrows);
  for (int s = 0; s < max_new; ++s) {
    WIS_HIP_CHECK(hipMemcpy2DAsync(m->logits, (size_t)m->n_vocab_pad * 4, logits + (size_t)s * Mrows * V, (size_t)V * 4, (size_t)V * 4, Mrows, hipMemcpyHostToDevice, st));
    if (noise) WIS_HIP_CHECK(hipMemcpyAsync(d_noise.p, noise + (size_t)s * Mrows * V, (size_t)Mrows * V * 4, hipMemcpyHostToDevice, st));
    // step 0 samples every beam of an utterance from ONE row (wis_generate: the last prompt row; here row b*beam), later steps row b*beam + j
    WIS_RET(sampling_tail(g, {beam, s == 0 ? 0 : 1, 0}, TAIL_NO_CACHE));
    WIS_HIP_CHECK(hipMemcpyAsync(done.data(), m->bs.done, (size_t)B * 4, hipMemcpyDeviceToHost, st));
    WIS_HIP_CHECK(hipMemcpyAsync(par.data(), m->bs.parent, (size_t)Mrows * 4, hipMemcpyDeviceToHost, st));
    WIS_HIP_CHECK(hipStreamSynchronize(st));
    bool all = true;
    for (int b = 0; b < B; ++b) { if (done[b] && fin[b] < 0) fin[b] = s; all = all && done[b]; }
    if (out_parent) for (int r = 0; r < Mrows; ++r) out_parent[(size_t)s * Mrows + r] = par[r];
    if (all) break;
  }
  for (int b = 0; b < B; ++b) if (fin[b] < 0) { set_error("%s: utterance %d did not finish within %d steps", who, b, max_new); return WIS_E_STATE; }
  WIS_RET(results_from_device(m, B * g.n_res, max_new, out_ids, out_len, out_score));
  if (g.phr_mass) WIS_RET(phrase_mass_end(m, B, g.n_res, max_new, st));
  if (out_finish_step) for (int b = 0; b < B; ++b) out_finish_step[b] = fin[b];
  return WIS_OK;
}

}  // namespace

extern "C" {

int wis_generate(wis_model_t* m, const float* input, int B, const int32_t* prompt, int P,
                 const wis_gen_opts_t* o, int32_t* out_ids, int32_t* out_len, float* out_score) {
  if (!m || !input || !prompt || !o || !out_ids || !out_len) { set_error("wis_generate: bad argument"); return WIS_E_ARG; }
  WIS_ENTER(m, "wis_generate")
  return generate_with_retry("wis_generate", m, input, B, prompt, P, o, out_ids, out_len, out_score);
}

int wis_generate_n(wis_model_t* m, const float* input, int B, const int32_t* prompt, int P, const wis_gen_opts_t* o, const uint64_t* seeds,
                   int32_t* out_ids, int32_t* out_len, float* out_score) {
  if (!m || !input || !prompt || !o || !out_ids || !out_len) { set_error("wis_generate_n: bad argument"); return WIS_E_ARG; }
  WIS_ENTER(m, "wis_generate_n")
  return generate_with_retry("wis_generate_n", m, input, B, prompt, P, o, out_ids, out_len, out_score, nullptr, 0, nullptr, nullptr, seeds, false);
}

// prompts of different lengths in one device batch; equal lengths are wis_generate_n, launch for launch
int wis_generate_ragged(wis_model_t* m, const float* input, int B, const int32_t* prompt, const int32_t* plen, const wis_gen_opts_t* o, const uint64_t* seeds,
                        int32_t* out_ids, int32_t* out_len, float* out_score) {
  if (!m || !input || !prompt || !plen || !o || !out_ids || !out_len || B < 1) { set_error("wis_generate_ragged: bad argument"); return WIS_E_ARG; }
  WIS_ENTER(m, "wis_generate_ragged")
  bool uniform = true;
  for (int b = 1; b < B && b < MAX_ROWS; ++b) uniform = uniform && plen[b] == plen[0];      // (a batch beyond MAX_ROWS is refused by the uniform call's check_batch)
  if (uniform) return generate_with_retry("wis_generate_ragged", m, input, B, prompt, plen[0], o, out_ids, out_len, out_score, nullptr, 0, nullptr, nullptr, seeds, false);
  return generate_with_retry("wis_generate_ragged", m, input, B, prompt, 0, o, out_ids, out_len, out_score, nullptr, 0, nullptr, nullptr, seeds, false, plen);
}

int wis_generate_draft(wis_model_t* m, const float* input, const int32_t* prompt, int P, const wis_gen_opts_t* o,
                       const int32_t* draft, int n_draft, int32_t* out_ids, int32_t* out_len, float* out_score, int32_t* accepted) {
  if (!m || !input || !prompt || !o || !out_ids || !out_len || (n_draft > 0 && !draft) || n_draft < 0) { set_error("wis_generate_draft: bad argument"); return WIS_E_ARG; }
  if (o->timestamps) { set_error("wis_generate_draft: timestamps are not available for drafted decodes"); return WIS_E_UNSUPPORTED; }
  if (o->phrases) { set_error("wis_generate_draft: phrases are not available for drafted decodes"); return WIS_E_UNSUPPORTED; }
  if (o->hotwords) { set_error("wis_generate_draft: hotwords are not available for drafted decodes"); return WIS_E_UNSUPPORTED; }
  if ((o->repetition_penalty != 0.f && o->repetition_penalty != 1.f) || o->no_repeat_ngram_size != 0) { set_error("wis_generate_draft: repetition_penalty / no_repeat_ngram_size are not available for drafted decodes"); return WIS_E_UNSUPPORTED; }
  if ((o->sampling_topk != 0 && o->sampling_topk != 1) || (o->sampling_temperature != 0.f && o->sampling_temperature != 1.f) || (o->num_hypotheses != 0 && o->num_hypotheses != 1)) { set_error("wis_generate_draft: sampling_topk / sampling_temperature / num_hypotheses are not available for drafted decodes"); return WIS_E_UNSUPPORTED; }
  WIS_ENTER(m, "wis_generate_draft")
  int acc = 0;
  WIS_RET(generate_with_retry("wis_generate_draft", m, input, 1, prompt, P, o, out_ids, out_len, out_score, draft, n_draft, &acc));
  if (accepted) *accepted = acc;
  return WIS_OK;
}

int wis_generate_draft_beam(wis_model_t* m, const float* input, const int32_t* prompt, int P, const wis_gen_opts_t* o,
                            const int32_t* draft_tok, const int32_t* draft_org, int n_steps, int32_t* out_ids, int32_t* out_len, float* out_score, int32_t* accepted_steps) {
  if (!m || !input || !prompt || !o || !out_ids || !out_len || n_steps < 0 || (n_steps > 0 && (!draft_tok || !draft_org))) { set_error("wis_generate_draft_beam: bad argument"); return WIS_E_ARG; }
  if (o->timestamps) { set_error("wis_generate_draft_beam: timestamps are not available for drafted decodes"); return WIS_E_UNSUPPORTED; }
  if (o->phrases) { set_error("wis_generate_draft_beam: phrases are not available for drafted decodes"); return WIS_E_UNSUPPORTED; }
  if (o->hotwords) { set_error("wis_generate_draft_beam: hotwords are not available for drafted decodes"); return WIS_E_UNSUPPORTED; }
  if ((o->repetition_penalty != 0.f && o->repetition_penalty != 1.f) || o->no_repeat_ngram_size != 0) { set_error("wis_generate_draft_beam: repetition_penalty / no_repeat_ngram_size are not available for drafted decodes"); return WIS_E_UNSUPPORTED; }
  if ((o->sampling_topk != 0 && o->sampling_topk != 1) || (o->sampling_temperature != 0.f && o->sampling_temperature != 1.f) || (o->num_hypotheses != 0 && o->num_hypotheses != 1)) { set_error("wis_generate_draft_beam: sampling_topk / sampling_temperature / num_hypotheses are not available for drafted decodes"); return WIS_E_UNSUPPORTED; }
  WIS_ENTER(m, "wis_generate_draft_beam")
  int acc = 0;
  WIS_RET(generate_with_retry("wis_generate_draft_beam", m, input, 1, prompt, P, o, out_ids, out_len, out_score, n_steps > 0 ? draft_tok : nullptr, n_steps, &acc,
                              n_steps > 0 ? draft_org : nullptr));
  if (accepted_steps) *accepted_steps = acc;
  return WIS_OK;
}

int wis_debug_search(wis_model_t* m, const float* logits, int n_steps, int B, const wis_gen_opts_t* o,
                     int32_t* out_ids, int32_t* out_len, float* out_score, int32_t* out_finish_step, int32_t* out_parent) {
  if (!m || !logits || !o || !out_ids || !out_len || n_steps < 1 || n_steps > MAX_STEPS) { set_error("wis_debug_search: bad argument"); return WIS_E_ARG; }
  WIS_ENTER(m, "wis_debug_search")
  return debug_search_impl("wis_debug_search", m, logits, n_steps, B, o, nullptr, nullptr, true, out_ids, out_len, out_score, out_finish_step, out_parent);
}

int wis_debug_search_n(wis_model_t* m, const float* logits, int n_steps, int B, const wis_gen_opts_t* o, const uint64_t* seeds, const uint32_t* noise,
                       int32_t* out_ids, int32_t* out_len, float* out_score, int32_t* out_finish_step, int32_t* out_parent) {
  if (!m || !logits || !o || !out_ids || !out_len || n_steps < 1 || n_steps > MAX_STEPS) { set_error("wis_debug_search_n: bad argument"); return WIS_E_ARG; }
  WIS_ENTER(m, "wis_debug_search_n")
  return debug_search_impl("wis_debug_search_n", m, logits, n_steps, B, o, seeds, noise, false, out_ids, out_len, out_score, out_finish_step, out_parent);
}

// the rows of ONE draft window of a given beam trajectory through the tree pass (seed_beam_draft's first window, without the replay): their logits
int wis_debug_tree_logits(wis_model_t* m, const float* input, int input_kind, const int32_t* prompt, int P, int beam,
                          const int32_t* tok, const int32_t* org, int n_steps, float* logits) {
  if (!m || !input || !prompt || !tok || !org || !logits || P < 1 || P > 16 || beam < 1 || beam > MAX_R || n_steps < 1 || n_steps > std::min(32, MAX_ROWS / std::max(beam, 1))) {
    set_error("wis_debug_tree_logits: bad argument (1 <= n_steps <= min(32, %d / beam))", MAX_ROWS); return WIS_E_ARG;
  }
  WIS_ENTER(m, "wis_debug_tree_logits")
  WIS_HIP_CHECK(hipSetDevice(m->device));
  WIS_RET(check_batch(m, 1, beam));
  const wis_config_t& c = m->cfg; hipStream_t st = m->st;
  const int k = beam, V = c.n_vocab;
  for (int i = 0; i < n_steps * k; ++i) if (tok[i] < 0 || tok[i] >= V || org[i] < 0 || org[i] >= k) { set_error("wis_debug_tree_logits: token / origin out of range"); return WIS_E_ARG; }
  WIS_RET(run_front(m, input, input_kind, 1));
  m->spin_now = false;
  // the prompt: rows at positions 0 .. P-1 of slot 0, then every slot gets a copy (what the first step's kv_reorder does)
  std::vector<int> ptok(P), ppos(P), pslot(P, 0), pls(P, 0);
  for (int i = 0; i < P; ++i) { ptok[i] = prompt[i]; ppos[i] = i; }
  WIS_RET(upload_rows(m, ptok, ppos, pslot, pls));
  WIS_RET(dec_forward(m, P, P, 1, false, beam, 0));
  auto& hs = m->h_pin->tree_seed;
  for (int j = 0; j < MAX_R; ++j) hs.parent[j] = 0;
  hs.step = 1; hs.done = 0;
  WIS_HIP_CHECK(hipMemcpyAsync(m->bs.parent, hs.parent, (size_t)k * 4, hipMemcpyHostToDevice, st));
  WIS_HIP_CHECK(hipMemcpyAsync(m->bs.step_u, &hs.step, 4, hipMemcpyHostToDevice, st));
  WIS_HIP_CHECK(hipMemcpyAsync(m->bs.done, &hs.done, 4, hipMemcpyHostToDevice, st));
  WIS_RET(launch_kv_reorder(st, m->kc_all, m->vc_all, m->kv_layer_stride, c.n_dec_layers, m->bs, 1, beam, P, c.n_text_ctx, c.d_model));
  // one window: steps 1 .. n_steps, rows from trajectory entries 0 .. n_steps - 1
  std::vector<int> hd((size_t)n_steps * MAX_R * 2, 0);
  pack_traj(hd.data(), tok, org, n_steps, k);
  std::vector<int> wt, wp, wsl, wls;
  int* ha = m->h_pin->anc;
  const int Mpad = fill_tree_window(hd.data(), 1, n_steps, k, P, wt, wp, wsl, wls, ha);
  WIS_RET(upload_rows(m, wt, wp, wsl, wls, false, &m->h_pin->win_rows));
  WIS_HIP_CHECK(hipMemcpyAsync(m->d_anc, ha, (size_t)Mpad * ANC_W * 4, hipMemcpyHostToDevice, st));
  const TreeWin tw{m->d_anc, P, ANC_W};
  WIS_RET(dec_forward(m, Mpad, 16, Mpad / 16, true, 1, 0, &tw));
  WIS_HIP_CHECK(hipMemcpy2DAsync(logits, (size_t)V * 4, m->logits, (size_t)m->n_vocab_pad * 4, (size_t)V * 4, (size_t)n_steps * k, hipMemcpyDeviceToHost, st));
  WIS_HIP_CHECK(hipStreamSynchronize(st));
  return WIS_OK;
}

}  // extern "C"
