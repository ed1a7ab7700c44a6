/* wis_hip.h — C-ABI of libwis_hip.so: the MI355X-native Whisper ASR hot path for
 * Willow Inference Server (WIS).
 *
 * The reference has no FFI of its own for this path: the boundary is the set of Python
 * call sites in reference main.py / wis/audio.py.  Each entry point below
 * names the reference expression it replaces.  Everything is `extern "C"`, plain pointers
 * and sizes; the caller owns every host buffer, the library owns device memory (except
 * where a `*_dev` pointer is explicitly handed in).  All functions return WIS_OK (0) or a
 * negative WIS_E_* code; the message is available from wis_last_error() (thread-local).
 * No exceptions cross the boundary.  No CPU fallback exists: without a gfx950 device every
 * compute entry point fails with WIS_E_HIP.
 */
#ifndef WIS_HIP_H
#define WIS_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define WIS_ABI_VERSION 1

#define WIS_OK             0
#define WIS_E_ARG         -1   /* bad argument */
#define WIS_E_FORMAT      -2   /* malformed audio container / weight index */
#define WIS_E_NOMEM       -3
#define WIS_E_CHECKSUM    -4   /* FLAC MD5 mismatch */
#define WIS_E_HIP         -5   /* HIP runtime error or no usable device */
#define WIS_E_STATE       -6   /* capacity exceeded / handle misuse */
#define WIS_E_UNSUPPORTED -7

/* audio front-end constants: reference wis/audio.py:17-25 */
#define WIS_SAMPLE_RATE 16000
#define WIS_N_FFT       400
#define WIS_HOP         160
#define WIS_N_MELS      80
#define WIS_N_SAMPLES   480000   /* 30 s window */
#define WIS_N_FRAMES    3000

typedef struct wis_model wis_model_t;

/* ---- library ------------------------------------------------------------------------ */
int         wis_version(void);              /* returns WIS_ABI_VERSION */
const char* wis_last_error(void);           /* valid until the next call on this thread */
int         wis_device_count(void);         /* replaces torch.cuda.device_count(), main.py:252-262 */
/* replaces ctranslate2.get_supported_compute_types(device), main.py:454 — writes a
 * NUL-terminated comma list ("float16,float32") */
int         wis_supported_compute_types(int device, char* out, size_t out_cap);

/* ---- a1: container decode (replaces librosa.load(audio_file, sr=16000, mono=True),
 * main.py:579).  FLAC or RIFF/WAVE bytes -> malloc'ed mono f32 PCM; free with
 * wis_audio_free.  md5_status_out: 1 verified, -1 no signature present (WAV / unsigned).
 * The bytes are untrusted: WIS_E_FORMAT for anything malformed (a sample rate of 0 and bytes
 * before or behind the stream included), WIS_E_CHECKSUM for a FLAC signature that is present
 * and wrong, WIS_E_NOMEM; on an error *pcm_out is not written.  Supported features:
 * INTEGRATION.md section 5. */
int  wis_audio_decode(const void* bytes, size_t n_bytes, float** pcm_out,
                      int64_t* n_samples_out, int* sample_rate_out, int* md5_status_out);
void wis_audio_free(float* pcm);

/* ---- a1, second half: sample-rate conversion to 16 kHz (the resampling librosa.load(audio_file, sr=16000) does, main.py:579 and
 * :815; x-audio-sample-rate on /api/willow), csrc/resample.hip.  up = 16000 / g, down = sr_in / g, g = gcd(sr_in, 16000); the
 * prototype low-pass h has n_taps = 64 max(up, down) + 1 taps: Kaiser-windowed sinc, 32 zero crossings each side at the lower
 * rate, beta 14.769656459379492, cut-off 0.945 of the lower Nyquist, taps summing to `up`; n_out = ceil(n_in up / down) and
 * y[m] = sum over k in [0, n_in) of x[k] h[m down - k up + 32 max(up, down)], zeros outside the signal on both sides
 * (wis_hip.audio._resample_filter / resample define the same filter and the same sum on the host).
 * A ratio is served on the device while n_taps <= 2^20 (every rate from 8 to 96 kHz that shares a sensible divisor with 16 kHz);
 * above that the entries answer WIS_E_UNSUPPORTED and the caller resamples on the host.
 *
 * wis_resample_plan: host only, no GPU.  Any out pointer may be NULL.  taps_per_phase = ceil(n_taps / up): the terms of every
 * output's sum.  sr_in <= 0 or n_in < 0: WIS_E_ARG; above the tap cap: WIS_E_UNSUPPORTED (the values are still written). */
int wis_resample_plan(int sr_in, int64_t n_in, int* up, int* down, int64_t* n_out, int* taps_per_phase, int64_t* n_taps);
/* the fp64 prototype the engine rounds to f32 for its device tables: h[0 .. 64 max(up, down)], cap = room in h (fewer than
 * n_taps: WIS_E_ARG).  Host only, no GPU. */
int wis_resample_filter(int up, int down, double* h, int64_t cap);
/* host PCM at sr_in in, host PCM at 16 kHz out: out[0 .. *n_out).  *n_out is written whenever the arguments name a length;
 * out_cap < *n_out: WIS_E_ARG and `out` is not touched.  sr_in == 16000 copies the input (no GPU needed); n_in == 0 gives
 * *n_out = 0.  The bits of out[m] depend on the signal, the ratio and m alone: long inputs run in segments over a bounded
 * workspace and the result does not depend on where the segments fall.  Re-entrant like wis_logmel_n: every call has a stream
 * and a workspace of its own. */
int wis_resample(int device, const float* pcm, int64_t n_in, int sr_in, float* out, int64_t out_cap, int64_t* n_out);
/* the same with the segment length forced: segment_samples input samples per segment (0: the built-in length) */
int wis_resample_ex(int device, const float* pcm, int64_t n_in, int sr_in, float* out, int64_t out_cap, int64_t* n_out,
                    int64_t segment_samples);

/* ---- a2+a3: log-mel front-end (replaces wis.audio.log_mel_spectrogram(pad_or_trim(x)),
 * wis/audio.py:28-51,72-103; call sites main.py:606-614).
 * pcm: n_win windows, window w has n_samples[w] valid samples starting at pcm + w*stride
 * (zero-padded / truncated to 480000 on device: pad_or_trim).  mel_out: [n_win][80][3000] f32.
 * pcm_on_device / mel_on_device select host or device pointers for each side. */
int wis_logmel(int device, const float* pcm, int64_t stride, const int64_t* n_samples, int n_win,
               int pcm_on_device, float* mel_out, int mel_on_device);
/* the same with n_mels = 80 (tiny .. large-v2; wis_logmel) or 128 (large-v3 / large-v3-turbo, librosa's Slaney bank of 128
 * filters): mel_out [n_win][n_mels][3000].  Any other n_mels: WIS_E_UNSUPPORTED. */
int wis_logmel_n(int device, int n_mels, const float* pcm, int64_t stride, const int64_t* n_samples, int n_win,
                 int pcm_on_device, float* mel_out, int mel_on_device);

/* ---- 8(f)3: incremental log-mel over arriving PCM (streaming / long-form sessions).  One handle = ONE 30 s window being
 * filled on one device.  Frames are local (400 samples around 160 t, wis/audio.py:96-101), so every 16-frame tile whose samples
 * have all arrived is transformed inside wis_melstream_feed; only the clamp at (window max - 8) and the scaling (wis/audio.py:
 * 100-102) need the whole window and run in wis_melstream_finish, together with the tail tiles against the zero padding of
 * pad_or_trim.  The result equals wis_logmel of the complete window bit for bit (same kernels, same per-tile arithmetic).
 * The features stay in HBM: finish hands back a DEVICE pointer (f32 [80][3000], valid until the next reset / destroy) that
 * wis_generate / wis_detect_language take as WIS_IN_MEL_DEV on the same device; mel_host_or_null additionally copies them out.
 * A handle is used by one thread at a time; different handles are independent (own stream and buffers). */
typedef struct wis_melstream wis_melstream_t;
int  wis_melstream_create(int device, wis_melstream_t** out);
/* a session for n_mels = 80 (= wis_melstream_create) or 128 bins: finish then hands back [n_mels][3000], equal bit for bit to
 * wis_logmel_n(n_mels) of the complete window.  Any other n_mels: WIS_E_UNSUPPORTED. */
int  wis_melstream_create_n(int device, int n_mels, wis_melstream_t** out);
int  wis_melstream_reset(wis_melstream_t* s);
int  wis_melstream_feed(wis_melstream_t* s, const float* pcm, int64_t n_samples);   /* host PCM, appended; beyond 480000: ignored */
int  wis_melstream_finish(wis_melstream_t* s, float* mel_host_or_null, float** mel_dev_out);
int64_t wis_melstream_samples(const wis_melstream_t* s);       /* samples received so far (<= 480000) */
int  wis_melstream_tiles_done(const wis_melstream_t* s);       /* 16-frame tiles already transformed (0..188) */
void wis_melstream_destroy(wis_melstream_t* s);

/* ---- whole-recording log-mel for long-form transcription (openai-whisper's transcribe(): one log-mel over the recording with 30 s
 * of zeros appended, sliced mel[:, seek : seek + 3000]).  One handle = one recording's log10 spectrum in HBM on one device.
 * Definition: the recording of n_samples samples continues with zeros on the right without end; its left edge is reflect-padded by
 * 200 samples (torch.stft's centre padding); there is no reflection on the right.  Frame t covers the samples 160 t - 200 ..
 * 160 t + 199, for t = 0 .. n_samples / 160 + 2999.  lg[m][t] = log10(max(mel, 1e-10)) with the DFT table, the filter bank and
 * the order of every sum of wis_logmel_n (the same per-tile code: the bits of a frame depend on its 400 samples alone - not on the
 * recording's length, on the upload segment or launch that produced it, or on the window that reads it).  A frame that touches no
 * sample has lg = -10.0f exactly.  gmax = the maximum of lg over all those frames, so never below -10.  A window's entry for the
 * frame g = seek + f, f < 3000, is (max(lg[m][g], gmax - 8) + 4) / 4: the floor is the RECORDING's, not the window's.
 * Only the frames up to the last one that touches a sample, rounded up to a 16-frame tile, are stored (4 n_mels bytes per frame:
 * 230 MB for two hours at 80 bins); the window kernel supplies -10.0f beyond them.  While n_samples <= 479800 the window at seek 0
 * equals wis_logmel_n of the same samples bit for bit.  From 479801 samples on frame 3000 touches a sample: it enters gmax here and is no
 * frame of wis_logmel_n, so the floors differ if that frame holds the maximum; above 479958 wis_logmel_n's right-hand reflection reads real
 * samples as well.
 * Host PCM is uploaded in segments over a bounded staging buffer.  n_samples above WIS_LONGMEL_MAX_SAMPLES (4 hours), n_mels
 * other than 80 or 128, a NULL pcm with n_samples > 0: WIS_E_ARG, and *out is NULL. */
#define WIS_LONGMEL_MAX_SAMPLES 230400000LL
typedef struct wis_longmel wis_longmel_t;
int  wis_longmel_create(int device, int n_mels, const float* pcm, int64_t n_samples, int pcm_on_device, wis_longmel_t** out);
/* the same with the upload segment forced: segment_samples host samples per segment (0: the built-in length; below 2800, one
 * tile's span: WIS_E_ARG).  Ignored for device PCM. */
int  wis_longmel_create_ex(int device, int n_mels, const float* pcm, int64_t n_samples, int pcm_on_device, int64_t segment_samples,
                           wis_longmel_t** out);
int64_t wis_longmel_frames(const wis_longmel_t* h);            /* content frames = n_samples / 160, floor (NULL: 0) */
int  wis_longmel_max(wis_longmel_t* h, float* gmax_out);       /* gmax, the value behind the ordered key (tests) */
/* mel_out f32 [n_win][n_mels][3000] (host or device): window w = frames seek_frames[w] .. seek_frames[w] + 2999, one launch for all
 * of them; a device mel_out is WIS_IN_MEL_DEV input of wis_generate on the same device.  Every seek in [0, frames + 2999], n_win up
 * to 1024; otherwise, and for a NULL handle, WIS_E_ARG with nothing launched.  Returns with nothing in flight.  Calls on one handle
 * are serialised; different handles are independent (own stream and buffers). */
int  wis_longmel_window(wis_longmel_t* h, const int64_t* seek_frames, int n_win, float* mel_out, int mel_on_device);
void wis_longmel_destroy(wis_longmel_t* h);

/* ---- a6: model lifecycle (replaces ctranslate2.models.Whisper(path, device=..,
 * compute_type=.., device_index=[..]), main.py:341-444).  One handle = one replica on one
 * GPU; the Python shim creates one per listed device_index entry. */
typedef struct {
  int32_t d_model, n_heads, n_enc_layers, n_dec_layers;
  int32_t n_vocab;        /* 51865 multilingual; 51866 large-v3 */
  int32_t n_audio_ctx;    /* 1500 */
  int32_t n_text_ctx;     /* 448 */
  int32_t n_mels;         /* 80, or 128 (large-v3 / large-v3-turbo) */
  int32_t max_batch;      /* utterances (30 s windows) per device batch */
  int32_t max_beam;       /* largest beam_size that will be requested */
  int32_t eot, sot, no_timestamps, no_speech;   /* 50257, 50258, 50363, 50362 */
  const int32_t* suppress_ids;       int32_t n_suppress;        /* CT2 config.json:suppress_ids */
  const int32_t* suppress_ids_begin; int32_t n_suppress_begin;  /* [220, 50257] */
  const int32_t* lang_ids;           int32_t n_lang;            /* 50259..50357 */
  int32_t decoder_weight_bits;  /* 0 / 16: f16 decoder weights (compute type "float16"); 8: per-row int8 weights with f16
                                 * activations ("int8_float16", the reference's GPU default main.py:242) - halves the decode
                                 * weight stream; encoder, embedding lookup and the cross K/V projection stay f16 */
} wis_config_t;

#define WIS_DT_F32 0
#define WIS_DT_F16 1
/* One weight tensor inside the arena.  Names follow the CTranslate2 WhisperSpec variable
 * names, e.g. "encoder/layer_0/self_attention/linear_0/weight". */
typedef struct {
  const char* name;
  int32_t     dtype;       /* WIS_DT_* */
  int32_t     rank;
  int64_t     shape[4];
  uint64_t    offset;      /* byte offset into the arena */
} wis_tensor_t;

/* arena: ONE contiguous block holding every tensor (host memory, or device memory on
 * `device` when arena_on_device != 0 — e.g. the buffer a RCCL broadcast just filled).
 * Weights are re-packed on the GPU into the kernels' layouts; the arena is not retained. */
int  wis_model_create(const wis_config_t* cfg, const void* arena, size_t arena_bytes,
                      int arena_on_device, const wis_tensor_t* tensors, int n_tensors,
                      int device, wis_model_t** out);
void wis_model_destroy(wis_model_t* m);
size_t wis_model_device_bytes(const wis_model_t* m);
/* Another replica on the SAME GPU that shares `parent`'s converted weights (read-only device memory, reference-counted: either
 * handle may be destroyed first) and owns its stream, activations and KV caches.  CTranslate2's `inter_threads` (reference
 * main.py:341-355: parallel batches per model) maps onto this: several device batches in flight on one GPU, each decode chain
 * filling the gaps of the others. */
int  wis_model_clone(wis_model_t* parent, wis_model_t** out);

/* ---- a7-a13: generate (replaces whisper_model.generate(features, [prompt]*B,
 * beam_size=.., return_scores=False) and results[i].sequences_ids[0], main.py:685-693,707,713;
 * decoding defaults are CTranslate2 4.1.0's because WIS passes none). */
#define WIS_IN_MEL_HOST 0   /* f32 [B][n_mels][3000] host   (StorageView.from_array, main.py:638,685) */
#define WIS_IN_MEL_DEV  1   /* same, device memory */
#define WIS_IN_PCM_HOST 2   /* f32 [B][480000] host: log-mel runs on the GPU, mel never leaves HBM */
#define WIS_IN_PCM_DEV  3
/* encoder OUTPUT handed back in (wis_encode below): the entry point skips the log-mel and the encoder and starts at the cross-K/V projection */
#define WIS_IN_ENC_DEV  4   /* f16 [B][n_audio_ctx][d_model], device memory on the handle's device: the bits wis_encode left there */
#define WIS_IN_ENC_HOST 5   /* the same values as f32 in host memory (f16 -> f32 -> f16 is exact: a host round trip loses nothing) */

typedef struct {
  int32_t input_kind;       /* WIS_IN_* */
  int32_t beam_size;        /* 1 = greedy (CT2 GreedySearch), >1 = beam search */
  int32_t max_new_tokens;   /* 0 => min(n_text_ctx/2, n_text_ctx - P) = 224 */
  float   length_penalty;   /* CT2 default 1 */
  float   patience;         /* CT2 default 1 */
  int32_t suppress_blank;   /* CT2 default 1: suppress_ids_begin masked at the first step */
  int32_t suppress_default; /* CT2 suppress_tokens=[-1]: mask cfg.suppress_ids every step */
  int32_t fixed_new_tokens; /* measurement convention: EOT masked until this many
                               tokens were generated, then forced.  0 = off (product default) */
  int32_t queue_depth;      /* searches that end on EOT: decode steps kept enqueued beyond the last one the host has seen
                               complete (the host polls a progress record the device writes to mapped host memory after every
                               step - no stream round trip); 0 => 2: one step running, one queued, over-run <= 1 step */
  int32_t timestamps;       /* 1: Whisper's timestamp rules every step (openai-whisper ApplyTimestampRules, what CTranslate2 applies
                               when the prompt lacks <|notimestamps|>): no <|notimestamps|>, timestamps in pairs except before EOT,
                               never decreasing, the first step a timestamp, text masked when the timestamps' total probability beats
                               every text token.  Order: suppress_default, suppress_blank, these rules, fixed_new_tokens (EOT masked
                               before the rules' decision; its forced EOT overrides them) - the order is restated, not pinned against
                               CTranslate2.  0: off (today's search).  wis_generate / wis_debug_search; drafts answer WIS_E_UNSUPPORTED */
  int32_t max_initial_timestamp_index;   /* timestamps: the first timestamp is at most <|0.00|> + this (CTranslate2 default 50);
                                            < 0: no cap */
  int32_t no_speech_prob;   /* 1: keep P(<|nospeech|>) of the softmax over the raw logits at <|startoftranscript|> per utterance
                               (wis_last_no_speech_prob) */
  /* The two CTranslate2 4.1.0 processors against a hypothesis that loops (RepetitionPenalty, NoRepeatNgram; restated, not pinned against
   * CTranslate2).  A live beam's HISTORY is what this search has generated for it so far, after the last beam step's reordering; the start
   * sequence and a decoder prefix are not counted (CTranslate2 also counts the last start token: the default suppress list masks that token
   * in every prompt form the server builds, so the two agree there and differ only with suppress_default = 0).  EOT never enters a history
   * that continues, so neither rule touches EOT; fixed_new_tokens keeps its override.  Both are no-ops at the first step (all beams sample
   * from the one prompt row).  Order: repetition_penalty on the raw logits, then the masks (suppress lists, n-gram bans), then the timestamp
   * rules - whose text / timestamp decision therefore sees penalised, banned values.  wis_generate / wis_debug_search; drafts answer
   * WIS_E_UNSUPPORTED.  A negative or non-finite penalty, a negative n-gram size: WIS_E_ARG, nothing enqueued. */
  float   repetition_penalty;     /* p > 0: for every DISTINCT token t of the history, logit x of t becomes x * p if x < 0, else x / p (fp32, a true
                                     division; once however often t occurs).  1 - and 0, what a caller that never knew the field passes - : off */
  int32_t no_repeat_ngram_size;   /* n >= 1: with a history h of L >= n tokens, every i in [0, L - n] with h[i .. i+n-2] == h[L-n+1 .. L-1] masks
                                     h[i+n-1] (n = 1: every history token).  0: off */
  /* Random sampling and n-best results (CTranslate2 4.1.0 RandomSampler / GreedySearch and num_hypotheses; restated, not pinned against
   * CTranslate2).  Appended fields: 0 is what a caller that never knew them passes, and means today's search.
   * THE SAMPLING RULE.  Sampling applies at beam_size 1.  The logits processors run first, in the order above (repetition rules, suppress lists,
   * timestamp rules, fixed_new_tokens); call the result x, masked ids at -inf.  The allowed set K is every unmasked id (whole vocabulary) or the k
   * largest x (top-k; value descending, then id ascending).  The token is drawn from softmax(x[K] / T); its contribution to the hypothesis score is
   * (x[t] - logsumexp(x over ALL unmasked ids)) / T, the temperature-scaled log-probability; the final score is normalised as the greedy path's
   * (/ len^length_penalty).  num_hypotheses = n decodes n independent samples per utterance (n decoder rows that share the utterance's cross K / V, where
   * n beams would sit: B n <= 96 rows, n <= max_beam); results come back in sample order, unsorted.
   * The draw is a Gumbel-max: t = argmax over K of (x[t] / T + g(t)) in fp32 (a true division, one addition), ties to the lower id, with noise that
   * is specified bit for bit:  w = Philox4x32-10(counter = (token id, step index, sample index j within the utterance, 0), key = (seed_lo, seed_hi))[0],
   * u = ((w >> 9) + 0.5) 2^-23  (inside (5.96e-8, 0.99999994) for every w; the 24-bit form rounds to 1 for w = 0xFFFFFFFF),  g = -log(-log(u)) with
   * an accurate logf.  The seed is per UTTERANCE (wis_generate_n: seeds [B]) and the counter carries the sample index, not the device row: an
   * utterance's samples do not depend on its slot in the device batch.  A finished sample keeps its result; its row is fed <|endoftext|> until the
   * utterance's last sample has finished.
   * Errors: sampling with beam_size > 1, num_hypotheses > 1 at beam_size 1 without sampling, num_hypotheses > beam_size in a beam search, a
   * temperature that is not finite and > 0, num_hypotheses outside 1 .. 8: WIS_E_ARG; sampling_topk > 16: WIS_E_UNSUPPORTED; drafted decodes with
   * any of the three on: WIS_E_UNSUPPORTED.  Nothing is enqueued by a refused call.  wis_generate / wis_debug_search return one hypothesis:
   * num_hypotheses > 1 there is WIS_E_ARG (wis_generate_n / wis_debug_search_n). */
  int32_t sampling_topk;          /* 0 or 1: off (arg-max).  -1: sample from the whole vocabulary.  2 .. 16: from the k best.  Larger: WIS_E_UNSUPPORTED */
  float   sampling_temperature;   /* T; 0 means 1 */
  int32_t num_hypotheses;         /* n; 0 means 1.  Beam search (no sampling): the n best finished hypotheses by normalised score, best first, the first
                                     registered among equal scores; CTranslate2's early exit then needs n finished hypotheses */
  /* Phrase-constrained decoding.  Appended field: 0 is what a caller that never knew it passes, and means today's search.
   * THE PHRASE RULE.  The handle holds a PHRASE SET (wis_model_set_phrases): token sequences of 1 .. 32 ids, every id a text token (< eot) outside the
   * model's suppress_ids, no first id in suppress_ids_begin - so no allowed token is masked by the suppress lists and no row ends up all -inf.  The
   * set is a trie.  A live row's NODE is found by walking the row's generated history (the repetition rules' history: what this search has generated
   * for the beam so far, after the last beam step's reordering; no start sequence, no prompt, no <|startofprev|> text) from the root.
   *   - The history is a path of the trie: every id of [0, n_vocab) except the node's children - and <|endoftext|> when the node ends a phrase - is
   *     stored as -inf; the kept ids keep their values bit for bit.
   *   - The history is no path (only a slot whose cumulative score is already -inf can hold one: every finite continuation was masked): the row
   *     is left as it is.
   *   - The first step: every beam samples from the one shared prompt row, every history is empty; that row is masked to the root's children.
   *   - Finished utterances: nothing.  Ids in [n_vocab, n_vocab_pad) and every other row are never written.
   * Order: the repetition penalty and bans first, then this mask, then everything else of the tail (a mask commutes with the suppress lists; an
   * n-gram ban CAN take a node's last child - that slot's row is then all -inf and the slot dies, as any such row's does).  A
   * hypothesis' score is the model's log-probability renormalised over what the set allows at each step; a beam search with num_hypotheses = n
   * ranks the n best phrases (results whose score is -inf are fillers: the set reached fewer phrases than the search wanted).
   * max_new_tokens = 0 resolves to min(the usual value, longest phrase + 1) - the bound that ends a search whose set holds fewer phrases than the
   * beam needs hypotheses; an explicit value below longest phrase + 1: WIS_E_ARG.  With timestamps, fixed_new_tokens > 0, sampling, or through the
   * drafted entry points: WIS_E_UNSUPPORTED; on with no set installed: WIS_E_STATE; a value other than 0 / 1: WIS_E_ARG.  Nothing is enqueued
   * by a refused call.  wis_generate, wis_generate_n, wis_generate_ragged, wis_debug_search, wis_debug_search_n. */
  int32_t phrases;                /* 1: constrain the search by the handle's phrase set.  0: off */
  /* The in-grammar mass of a phrase-constrained search.  Appended field: 0 is what a caller that never knew it passes, and changes nothing - the same
   * launches, captured steps and buffers as before the field existed.
   * THE PHRASE MASS RULE.  A live row of utterance b (cumulative score above -inf; at the first step the one shared prompt row) whose history is a
   * path of the trie ending at record r (record 0: the root).  x: the row as the repetition rules left it.  u[t], t in [0, n_vocab): x[t] under exactly
   * the masks the sampling statistics apply to the row of a call without timestamps, in fp32:
   *     u[t] = x[t] + (suppress_default ? bias_all[t] : 0),  then  u[t] = u[t] + bias_begin[t]  at the first step (no token generated yet) when suppress_blank is on
   * (bias_all: -inf at the model's suppress_ids, else 0; bias_begin: -inf at suppress_ids_begin, else 0).  A: the node's children, plus <|endoftext|>
   * when the node ends a phrase.  M = max u; num = sum over A of exp(u[t] - M); den = the same sum over [0, n_vocab) (an entry equal to M counts as
   * exactly 1, also when M is +inf);
   *     logmass[b][r] = min(0, log(num) - log(den)),   -inf when M is -inf or num is 0 (every allowed entry is -inf, or M is +inf and none is);
   * (the engine sums the allowed entries about their own maximum, so a share below fp32's exp range is still a number, not an underflow to -inf)
   * never NaN for a row without NaN in [0, n_vocab) (with a NaN there: unspecified).  Ids in [n_vocab, n_vocab_pad) never enter.  It is the log of the
   * share of the model's probability that the set allows at that step, computed where the mask is applied (num and den are reduced in one fixed order,
   * csrc/dec_kernels.hip phrase_rules_mass_kernel; a row whose finite entries are all allowed gives exactly 0), and the masked row is bit for bit the row
   * of a call with the option off - so are ids and scores.
   * Nothing is accumulated per beam: a live row's node is a function of its history, distinct live beams of an utterance hold distinct histories, and a
   * node at depth L is visited at step L alone - so the step's value is stored per (utterance, record), and a RESULT's phrase_logmass is the fp32
   * sum, in path order from the root, of logmass[b][r] over the len + 1 nodes of its own path; -inf for a filler result (score -inf) and for a result
   * that is no phrase of the set.  The sum equals log P_unconstrained(phrase, <|endoftext|>) - log P_constrained(phrase, <|endoftext|>): what a second,
   * unconstrained decode would have been compared for.  A slot the search did not write is NaN (the slots of the installed set are filled with NaN
   * when the call starts), and a NaN slot propagates into the sum.
   * 1 needs phrases = 1 (else WIS_E_ARG); a value other than 0 / 1: WIS_E_ARG.  wis_last_phrase_mass reads the sums.  The entry points of `phrases`. */
  int32_t phrase_mass;            /* 1: compute the in-grammar mass of every result (wis_last_phrase_mass).  0: off */
  /* Hotword boosting (contextual biasing): free-form decoding goes on, tokens that start or continue a listed entry get a log-domain bonus.
   * Appended fields: 0 is what a caller that never knew them passes, and means today's search - the same launches, captured steps and buffers.
   * THE HOTWORD RULE.  The handle holds a HOTWORD SET (wis_model_set_hotwords), apart from the phrase set: installing one never disturbs the other.
   * The two share record format, limits and token rules: 16-byte edge records in tree order; at most 65535 records, 4096 children per node, 32
   * tokens per entry; text tokens only (< eot), outside suppress_ids, no first token in suppress_ids_begin; every leaf ends an entry.
   * For a live row, h[0 .. L) is the generated history as the repetition rules define it: what this search has generated for the beam so far, after
   * the last reordering - no start sequence, prompt or prefix -, L = min(steps taken, max_new).
   *   - For k = 0 .. min(L, 31) the suffix S_k = h[L-k .. L) is ACTIVE when it is a path of the trie from the root.  S_0, the empty suffix, is always
   *     active and sits at the root.  A history id outside [0, n_vocab) breaks every suffix that contains it.
   *   - The BOOST SET T is the union, over the active suffixes, of the children of the node each suffix ends at.
   *   - Every t in T gets exactly ONE fp32 addition, row[t] = row[t] + hotword_boost, round to nearest - however many suffixes name t.  -inf stays
   *     -inf, NaN stays NaN.  <|endoftext|> is never in T; "ends an entry" flags play no part.
   *   - Ids in [n_vocab, n_vocab_pad), rows of finished utterances and all other memory are never written.
   *   - The first step: every beam samples from the one shared prompt row; that row gets the root's children boosted ONCE (the utterance's first
   *     workgroup alone acts, as under the phrase rule).  The forced-EOT step of fixed_new_tokens: nothing, as under the repetition rules.
   * Order: the repetition penalty and n-gram bans first, then this addition, then everything else of the tail (an addition commutes with the -inf
   * masks of the suppress lists: a banned or suppressed hot token stays banned); the timestamp rules' text / timestamp decision sees boosted values.
   * A hypothesis' score is the log-softmax of the BOOSTED row at each step - not the model's own log-probability.
   * The rule has NO BACK-OFF: a hypothesis that abandons an entry half-way keeps what it gained (shallow fusion that takes the accumulated bonus
   * back needs per-beam state that follows the reorder: not part of this rule).
   * hotwords: a value other than 0 / 1 is WIS_E_ARG.  hotword_boost: finite and > 0 when hotwords = 1, else WIS_E_ARG; ignored when hotwords = 0 (no
   * default is offered: a useful value depends on the checkpoint).  hotwords = 1 with no set installed: WIS_E_STATE; together with phrases = 1:
   * WIS_E_ARG; through the drafted entry points: WIS_E_UNSUPPORTED.  (More than 256 new tokens, which the repetition rules answer with
   * WIS_E_UNSUPPORTED, cannot arise: every entry point caps max_new_tokens at 256.)  Nothing is enqueued by a refused call.  Combines with
   * timestamps, the repetition options, sampling and num_hypotheses, prompts of any supported length.  wis_generate, wis_generate_n,
   * wis_generate_ragged, wis_debug_search, wis_debug_search_n. */
  int32_t hotwords;               /* 1: boost by the handle's hotword set.  0: off */
  float   hotword_boost;          /* the bonus, in the logits' (natural-log) units */
} wis_gen_opts_t;

/* out_ids: [B][max_new] (max_new = resolved max_new_tokens), out_len: [B], out_score: [B]
 * (length-normalised log-prob of the returned hypothesis) or NULL.  Blocking.  Thread safety
 * (SURVEY 8b): any number of threads may call into DIFFERENT handles; a handle itself runs one
 * compute call at a time (single-instance activations / KV caches) - a second thread entering a
 * busy handle gets WIS_E_STATE at once, nothing is corrupted.  The shim's micro-batcher feeds each
 * replica from one worker thread and coalesces concurrent requests into device batches.
 * prompt: i32 [B][P], one common length P in 1 .. n_text_ctx / 2 + 4 (228; beyond: WIS_E_UNSUPPORTED).  P <= 16 (with B P <= 96) runs as one
 * merged prefill + first step pass.  Longer prompts - text behind <|startofprev|>, a prefix behind the start sequence - are prefilled in windows of
 * 16 positions, their K / V is kept once per utterance and read there by every beam, and one captured step serves every length; the drafted entry
 * points (wis_generate_draft, wis_generate_draft_beam) answer them with WIS_E_UNSUPPORTED.  max_new_tokens = 0 resolves to
 * min(n_text_ctx / 2, n_text_ctx - P). */
int wis_generate(wis_model_t* m, const float* input, int B, const int32_t* prompt, int P,
                 const wis_gen_opts_t* opts, int32_t* out_ids, int32_t* out_len, float* out_score);
/* wis_generate with n = opts->num_hypotheses results per utterance: out_ids [B][n][max_new], out_len [B][n], out_score [B][n] or NULL.
 * seeds: uint64 [B], one per utterance, or NULL = all 0 (read by sampled decodes only).  They are written to device memory at the start of
 * the call - never a kernel argument of a captured step: one step graph serves every seed. */
int wis_generate_n(wis_model_t* m, const float* input, int B, const int32_t* prompt, int P, const wis_gen_opts_t* opts, const uint64_t* seeds,
                   int32_t* out_ids, int32_t* out_len, float* out_score);
/* wis_generate_n for prompts of DIFFERENT lengths in one device batch.  prompt: the B prompts back to back (sum of plen[b] ids), in utterance order;
 * plen i32 [B], each in 1 .. min(228, n_text_ctx / 2 + 4) (anything else: WIS_E_UNSUPPORTED).  seeds and the outputs as in wis_generate_n
 * (num_hypotheses results per utterance, out_ids rows of the resolved max_new).
 *   - All lengths equal: the call IS wis_generate_n(..., P, ...) - the same launches, the same bits, for every P.
 *   - Otherwise every utterance takes the long-prompt route, whatever its own length (1 .. 16 included): its prompt's K / V is kept once in its first
 *     slot, the step kernels read its length from a device word, and the step graphs are the ones a uniform long-prompt call of the same (B, beam,
 *     options, max_new) captures - either kind of call replays what the other captured.  The prefix windows of 16 positions carry only the utterances
 *     that still have prompt left, in runs of consecutive utterances: any order of lengths is correct, the longest prompts first needs the fewest
 *     passes.  The last pass is right-aligned (row i of utterance b reads position plen[b] - Pl + i, Pl = min(16, 96 / B)).
 *   - max_new_tokens = 0 resolves to min(n_text_ctx / 2, n_text_ctx - max plen); an explicit value with max plen + max_new_tokens > n_text_ctx
 *     is WIS_E_ARG.  One max_new serves the batch.
 *   - no_speech_prob: every prompt must hold <|startoftranscript|> (else WIS_E_ARG); the row is found per utterance.
 *   - Timestamps, the repetition options, sampling and n-best, fixed_new_tokens and the suppress options apply as in the uniform call.
 *   - WIS_E_UNSUPPORTED while the TREE form of the step's self-attention is selected (WIS_SA_LONG=0 / wis_debug_sa_long(m, 0): its prompt length
 *     is a kernel argument).  There is no drafted form, and wis_last_trajectory answers WIS_E_STATE after a ragged call (the rows of utterances
 *     of different prompt lengths do not line up with what a drafted call replays). */
int wis_generate_ragged(wis_model_t* m, const float* input, int B, const int32_t* prompt, const int32_t* plen, const wis_gen_opts_t* opts,
                        const uint64_t* seeds, int32_t* out_ids, int32_t* out_len, float* out_score);

/* ---- 8(f)3, BASELINE configs[4]: the FINAL decode of a recording that was heard while it arrived (one utterance, beam_size 1 - the
 * reference's default, settings.py:14).  `draft`: the token ids of an earlier hypothesis for (most of) the same audio, e.g. the last
 * interim transcript of a streaming session.  The encoder runs on the final window as in wis_generate; the draft is then verified
 * in teacher-forced passes of 16 positions (one decoder weight stream per 16 tokens instead of one per token), the longest prefix
 * that greedy decoding of the FINAL window reproduces is kept, and ordinary greedy steps continue behind it.  The result is the
 * greedy decode of the final window - what wis_generate returns for it (same kernels; the multi-row passes sum in a different
 * order than the one-row step, so a decision closer than ~1e-3 in logit can fall differently, as between any two batch shapes).
 * accepted: draft tokens kept (may be NULL).  n_draft == 0 is wis_generate. */
int wis_generate_draft(wis_model_t* m, const float* input, const int32_t* prompt, int P, const wis_gen_opts_t* opts,
                       const int32_t* draft, int n_draft, int32_t* out_ids, int32_t* out_len, float* out_score, int32_t* accepted);

/* ---- the same for a BEAM SEARCH (round 6; the reference decodes every recording of 12 s or more at long_beam_size = 3, main.py:582-586,
 * settings.py:14-18 - BASELINE configs[4]'s 29 s fixture included).  The draft is the TRAJECTORY of an earlier search over (most of) the same
 * audio, as wis_last_trajectory returns it: per step the k live beams it left - draft_tok [n_steps][beam_size] their newest tokens, draft_org
 * [n_steps][beam_size] the live beam (0 .. beam_size-1 of the step before) each continued from.  While the search over the final window
 * follows the draft, up to 32 steps cost ONE decoder pass: the rows of all steps x beam_size tree nodes (<= 96) go through the decoder together,
 * the steps are replayed on their logits by the ordinary sampling kernels, and ordinary steps resume behind the first step whose live set
 * differs from the draft's AS A SET (the slot order of the live beams does not matter: near-tied candidates swap slots between two searches).
 * Every step that counts ran the engine's beam step on the logits of its true inputs: the result is the beam search of the final window,
 * what wis_generate returns for it (up to the summation order of the multi-row passes, as between any two batch shapes).
 * accepted_steps: steps whose live set equalled the draft's (may be NULL).  n_steps == 0 is wis_generate. */
int wis_generate_draft_beam(wis_model_t* m, const float* input, const int32_t* prompt, int P, const wis_gen_opts_t* opts,
                            const int32_t* draft_tok, const int32_t* draft_org, int n_steps,
                            int32_t* out_ids, int32_t* out_len, float* out_score, int32_t* accepted_steps);
/* The trajectory of utterance b of the LAST generate call on this handle (any of the three forms; beam_size k of that call): tok / org
 * [cap_steps][k], *n_steps = steps recorded (the step that ended the search leaves no live set).  Synchronises the handle's stream. */
int wis_last_trajectory(wis_model_t* m, int b, int32_t* tok, int32_t* org, int cap_steps, int32_t* n_steps);

/* no_speech_prob of the first B utterances of the LAST wis_generate on this handle, which must have set opts->no_speech_prob
 * (otherwise WIS_E_STATE): softmax(logits at the <|startoftranscript|> prompt position)[cfg.no_speech] over the whole vocabulary,
 * no logits processor applied (openai-whisper probs_at_sot).  Synchronises the handle's stream. */
int wis_last_no_speech_prob(wis_model_t* m, int B, float* out);
/* phrase_logmass (wis_gen_opts_t::phrase_mass states the rule) of the n results of each of the first B utterances of the LAST search on this handle
 * (wis_generate, wis_generate_n, wis_generate_ragged, wis_debug_search, wis_debug_search_n), which must have set opts->phrase_mass (otherwise
 * WIS_E_STATE): out [B][n], n = that call's results per utterance (anything else: WIS_E_ARG).  Synchronises the handle's stream. */
int wis_last_phrase_mass(wis_model_t* m, int B, int n, float* out);

/* ---- a14: language detection (replaces whisper_model.detect_language(features),
 * main.py:637-643): probabilities over cfg.lang_ids, [B][n_lang]. */
int wis_detect_language(wis_model_t* m, const float* input, int input_kind, int B, float* lang_probs);

/* ---- one encoder pass for every decode of a window (replaces ctranslate2.models.Whisper.encode(features, to_cpu)).
 * input / input_kind: one of the four WIS_IN_MEL_* / WIS_IN_PCM_* forms, B <= max_batch windows.  Runs the log-mel (PCM kinds) and the
 * encoder, then leaves the encoder's output - B * n_audio_ctx * d_model halves - in enc_out_dev_f16, a block of the CALLER's on the
 * handle's device; enc_out_host_or_null != NULL additionally receives the same values as f32 [B][n_audio_ctx][d_model] in host memory.
 * The handle's stream is synchronised before the call returns: the block can be read from any stream of that device afterwards, by this
 * handle, by a clone, or by any other handle of the same model on that device.
 * wis_generate* (opts->input_kind), wis_detect_language, wis_align, wis_debug_align_matrix and the logits taps take the block back as
 * WIS_IN_ENC_DEV (any B consecutive utterances of it: a pointer offset of whole utterances is fine) or its host copy as WIS_IN_ENC_HOST and
 * then compute, bit for bit, what they compute from the features at the same B - the cross-K/V projection and everything behind it
 * are the same launches on the same values.
 * WHERE THE BLOCK IS READ.  WIS_IN_ENC_DEV: the cross-K/V GEMM reads the caller's block IN PLACE as its A operand, no copy.  Every
 * A-operand loader of the encoder GEMM clamps its row index to M - 1 = B * n_audio_ctx - 1 (the guard is on the stores), and K = d_model
 * is a whole number of k-tiles, so nothing beyond the B * n_audio_ctx * d_model halves is touched - the GEMM does not rely on the size of
 * the handle's own encoder buffer.  The address handed in must be 16-byte aligned (the loaders read A in 16-byte pieces; a device allocation
 * is, and so is any offset of whole utterances inside one: n_audio_ctx * d_model halves are a multiple of 16 bytes) - nothing checks it.
 * The block must stay allocated until the call that reads it has returned (the GEMM has run by then).
 * WIS_IN_ENC_HOST: host -> device, f32 -> f16 into the handle's own encoder buffer, then the same GEMM.
 * wis_last_timing after a wis_generate from encoder output reports logmel_ms = encoder_ms = 0: the stages did not run.
 * Refused before anything is enqueued: enc_out_dev_f16 or input NULL (WIS_E_ARG), input_kind WIS_IN_ENC_* (WIS_E_UNSUPPORTED: that is
 * encoder output already) or unknown (WIS_E_ARG), B outside [1, max_batch] (WIS_E_ARG); wis_last_error names the argument. */
int wis_encode(wis_model_t* m, const float* input, int input_kind, int B, void* enc_out_dev_f16, float* enc_out_host_or_null);

/* ---- parity taps (teacher-forced); not used by the product path -------------------- */
/* encoder output [B][1500][d] f32 */
int wis_debug_encode(wis_model_t* m, const float* input, int input_kind, int B, float* enc_out);
/* logits [B][T][n_vocab] f32 for decoder inputs dec_in [B][T] (no suppression applied) */
int wis_debug_logits(wis_model_t* m, const float* input, int input_kind, int B,
                     const int32_t* dec_in, int T, float* logits);
/* the same logits computed R (1..16) positions of every utterance per decoder pass: a pass then has B*R rows, i.e. with
 * B*R > 8 it runs the batched-row route of the decode step (the one 8 utterances x beam 5 take, main.py:685-693 with
 * concurrent requests) instead of the <= 8-row route; B*R <= 96 (MAX_ROWS) */
int wis_debug_logits_rows(wis_model_t* m, const float* input, int input_kind, int B,
                          const int32_t* dec_in, int T, int R, float* logits);
/* ---- phrase-constrained decoding (wis_gen_opts_t::phrases states the rule) ------------------------------------------------------
 * Installs a phrase set on a handle, as a flat trie of n_records 16-byte records, one per EDGE:
 *   trie[4 i + 0] token of the edge            trie[4 i + 1] index of the first record of the child's own children (0: it has none)
 *   trie[4 i + 2] number of those children     trie[4 i + 3] 1: the child ends a phrase, else 0
 * Record 0 is the root's pseudo-edge {-1, 1, children of the root, 0}.  The children of one node are contiguous, in strictly ascending token
 * order, and the blocks lie in TREE ORDER: walking the records by index, every node's children start where the previous node's ended
 * (breadth-first), and the last block ends at n_records.  Every leaf ends a phrase.  A walk costs one dependent 16-byte load round per
 * history token.  The whole table is validated on the host before anything reaches the device - ranges, tree order, sorted children, the
 * token rules of the phrase rule, leaves - and anything malformed is WIS_E_ARG with the set that was installed before left in place.
 * Limits: 65535 records, 4096 children per node, 32 tokens per phrase; beyond them WIS_E_UNSUPPORTED.  n_records = 0 removes the set.
 * The device buffer has a fixed capacity and never moves: installing another set is a copy, captured decode steps stay valid (the resolved
 * max_new_tokens is part of a captured step's key, as ever: sets whose longest phrases are equally long share their steps).  A clone
 * (wis_model_clone) has a buffer of its own and starts without a set.  Not part of wis_config_t. */
int wis_model_set_phrases(wis_model_t* m, const int32_t* trie, int n_records);
/* ---- hotword boosting (wis_gen_opts_t::hotwords states THE HOTWORD RULE) ----------------------------------------------------------
 * Installs a hotword set on a handle: wis_model_set_phrases' table, validator, limits and answers, in a buffer of its own - the phrase set is
 * not touched, and the other way round.  The "ends an entry" flags are validated and otherwise unused.  The buffer has a fixed capacity and
 * never moves; the record count and the boost live in device memory beside it, so ONE captured step serves every set and every boost.
 * n_records = 0 removes the set; a malformed table is WIS_E_ARG with the previous set left in place; a clone starts without a set. */
int wis_model_set_hotwords(wis_model_t* m, const int32_t* trie, int n_records);
/* ---- word-level timestamps: cross-attention alignment + dynamic time warping (csrc/align.hip) --------------------------------
 * The alignment heads of a handle: n (layer, head) pairs; n == 0 restores openai-whisper's default, every head of the upper half
 * of the decoder layers (layer >= n_dec_layers / 2).  Clones made afterwards inherit them.  Not part of wis_config_t. */
int wis_model_set_alignment_heads(wis_model_t* m, const int32_t* layer_head_pairs, int n);
/* What CTranslate2's Whisper.align / openai-whisper's find_alignment compute.  Per utterance b the decoder is teacher-forced on
 * start_seq[P] + [no_timestamps] + text_b + (eot is predicted, not fed); the alignment heads' softmax(q.K^T) over all n_audio_ctx
 * keys, cropped to num_frames[b] / 2 frames, for the text_len[b] + 1 rows from the no_timestamps input on, is normalised over the
 * token axis per head ((w - mean) / population std), median-filtered along frames (odd width <= 63, reflect padding), averaged over
 * the heads, negated, and warped (openai-whisper dtw_cpu's recurrence and tie rules, bit for bit).
 *   text: the utterances' tokens back to back, text_len[B]; P + 1 + text_len[b] <= n_text_ctx (else WIS_E_ARG); B <= max_batch
 *   path_text / path_time [B][n_text_ctx + n_audio_ctx], path_len [B]: the warping path in forward order
 *   token_probs [B][n_text_ctx]: softmax(logits over ids < eot)[text_b[i]] at the row that predicts it (entries >= text_len[b] untouched)
 * The first call of a handle allocates the align scratch (wis_model_device_bytes grows then, not at create). */
int wis_align(wis_model_t* m, const float* input, int input_kind, int B, const int32_t* start_seq, int P,
              const int32_t* text, const int32_t* text_len, const int32_t* num_frames, int median_filter_width,
              int32_t* path_text, int32_t* path_time, int32_t* path_len, float* token_probs);
/* the matrix wis_align warps, alone: out = the utterances' dense fp32 [text_len[b] + 1][num_frames[b] / 2] matrices back to back (host) */
int wis_debug_align_matrix(wis_model_t* m, const float* input, int input_kind, int B, const int32_t* start_seq, int P,
                           const int32_t* text, const int32_t* text_len, const int32_t* num_frames, int median_filter_width, float* out);
/* GPU milliseconds of the handle's last wis_align: ms[6] = encoder + cross K/V, decoder passes, matrix, DTW, and of the matrix:
 * attention weights alone, normalise + filter alone */
int wis_align_last_timing(wis_model_t* m, float* ms);
/* op taps (device pointers), the launch helpers wis_align uses:
 * wis_op_dtw: x fp32 [N][M] (N <= 511) -> text_idx / time_idx (room for N + M - 1 entries each), len[1]
 * wis_op_align_matrix: q fp32 [n_heads_sel][T_tokens][64] finished queries, kx_f16 [n_heads_sel][8][T][8] (the cross-attention K
 * image of those heads), softmax over T keys, cropped to `frames` -> out fp32 [T_tokens][frames] */
int wis_op_dtw(int device, const float* x, int N, int M, int32_t* text_idx, int32_t* time_idx, int32_t* len);
int wis_op_align_matrix(int device, const float* q, const void* kx_f16, int T_tokens, int n_heads_sel, int T, int frames, int width, float* out);
/* the alignment kernels stage by stage, with wis_align's batched index arithmetic in the caller's hands.  N / F / M / koff / target / dst /
 * sel_head are HOST arrays (the taps check them: anything that would index out of bounds is WIS_E_ARG before a launch); every other pointer is
 * device memory that the caller fills beforehand (sentinels) and may read back whole.
 * wis_op_align_stage: B utterances of N[b] <= nmax <= ncap tokens and F[b] <= fmax <= T frames.  stage 0: q fp32 [B][nsel][ncap][64] (rows
 *   >= N[b] are not read) -> f16 -> scores + softmax over all T keys; head s of utterance b reads its K image ([8][T][8] f16) at kx_f16 +
 *   koff[s] + b kbstride (elements, multiples of 8, inside k_elems).  stage 1: (w - mean) / std in place on the caller's W.  stage 2: median of
 *   `width` + head sum of the caller's W into acc [B][nmax][T].  stage 3: the chain as wis_align runs it.  heads_per_chunk = 0: G from the 96 MB
 *   rule, else G = min(heads_per_chunk, nsel).  Stages 0 - 2 keep chunk c = heads c G .. at W + c B G nmax T, laid out [B][Gc][nmax][T] with Gc
 *   the chunk's own head count (w_elems >= ceil(nsel / G) B G nmax T); stage 3 reuses the first region for every chunk (w_elems >= B G nmax T).
 * wis_op_dtw_batch: table b (N[b] x M[b], rows `pitch` >= fmax apart) at x + b xbstride -> text_idx / time_idx [B][cap], len [B]; cap >= nmax + fmax (a path has up to
 *   N + M - 1 entries, N + M when non-finite costs send it along the borders); nmax > 511 is WIS_E_UNSUPPORTED.
 * wis_op_align_probs: logits fp32 [rows][vpad] -> probs[dst[r]] = softmax(logits[r][: eot])[target[r]] for rows with target[r] >= 0.
 * wis_op_align_capture: dq fp32 [M][d], row r = utterance ub0 + r / 16, matrix row t0 + r % 16 - P (rows outside [0, ncap) are skipped); heads
 *   sel_head[s0 .. s0 + n_layer_heads - 1] of the nsel selected -> qsel f16 [utterance][nsel][ncap][64] (qsel_elems elements). */
int wis_op_align_stage(int device, int stage, const float* q, const void* kx_f16, long long k_elems, const long long* koff, long long kbstride,
                       const int32_t* N, const int32_t* F, int B, int nsel, int ncap, int nmax, int fmax, int T, int width, int heads_per_chunk,
                       float* W, long long w_elems, float* acc, long long acc_elems);
int wis_op_dtw_batch(int device, const float* x, long long x_elems, long long xbstride, int pitch, const int32_t* N, const int32_t* M, int B, int nmax, int fmax, int cap,
                     int32_t* text_idx, int32_t* time_idx, int32_t* len);
int wis_op_align_probs(int device, const float* logits, int rows, int vpad, int eot, const int32_t* target, const int32_t* dst, float* probs, int probs_len);
int wis_op_align_capture(int device, const float* dq, int M, int d, const int32_t* sel_head, int s0, int n_layer_heads, int nsel, int ub0, int t0, int P, int ncap,
                         void* qsel_f16, long long qsel_elems);
/* the decoder pass wis_generate_draft_beam verifies a window with, alone: the tree rows of steps 1 .. n_steps of a beam trajectory (tok / org
 * [n_steps][beam]: per step the live beams' newest tokens and the beam each continued from) behind `prompt`, in ONE pass (tree self-attention by
 * ancestor table, cross-attention as row groups over the utterance's one K / V); logits [n_steps][beam][n_vocab]: row (s, j) = what a step fed
 * tok[s][j] after its chain of ancestors sees - comparable with wis_debug_logits on that chain.  n_steps <= min(32, 96 / beam). */
int wis_debug_tree_logits(wis_model_t* m, const float* input, int input_kind, const int32_t* prompt, int P, int beam,
                          const int32_t* tok, const int32_t* org, int n_steps, float* logits);

/* rows a11-a13 on caller-supplied logits: the SAMPLING kernels wis_generate runs after every decoder pass (logits processors,
 * log-softmax statistics, candidate selection, CTranslate2's beam bookkeeping - dec_kernels.hip logit_stats_kernel /
 * beam_step_kernel) driven by `logits` f32 [n_steps][B*beam][n_vocab] (host) instead of the decoder's output: at step s live beam j of
 * utterance b reads row s*B*beam + b*beam + j (step 0: row b*beam for every beam, like the merged prefill + first step).  Integer
 * bookkeeping only, so the result is compared EXACTLY with the oracle's search over the same table (tests/test_gpu_search.py):
 * an EOT arriving at any step, hypotheses of unequal length, refill from the secondary candidates, patience / early exit,
 * utterances of one device batch finishing at different steps.  opts->max_new_tokens (0 => n_steps) <= n_steps <= 256.
 * out_ids [B][max_new], out_len [B], out_score [B] or NULL, out_finish_step [B] or NULL (step index at which the utterance ended),
 * out_parent [n_steps][B*beam] or NULL (KV slot every live beam continues from after each step: what kv_reorder_kernel applies). */
int wis_debug_search(wis_model_t* m, const float* logits, int n_steps, int B, const wis_gen_opts_t* opts,
                     int32_t* out_ids, int32_t* out_len, float* out_score, int32_t* out_finish_step, int32_t* out_parent);
/* the same with n = opts->num_hypotheses results per utterance and the sampling options: logits f32 [n_steps][B*R][n_vocab], R = rows per utterance
 * (beam_size in a beam search, n in a sampled one).  Sampled: sample j of utterance b reads row s*B*n + b*n + j, step 0 row b*n for every sample.
 * out_ids [B][n][max_new], out_len / out_score [B][n]; out_finish_step [B]; out_parent [n_steps][B*R].  seeds [B] or NULL as wis_generate_n.
 * noise (tests; NULL: Philox): uint32 [n_steps][B*n][n_vocab] (host) - the word w of (step, row, token id) in place of the Philox word. */
int wis_debug_search_n(wis_model_t* m, const float* logits, int n_steps, int B, const wis_gen_opts_t* opts, const uint64_t* seeds, const uint32_t* noise,
                       int32_t* out_ids, int32_t* out_len, float* out_score, int32_t* out_finish_step, int32_t* out_parent);

/* the decoder cross-attention's granule hand-off (small grids; dec_kernels.hip SPIN): retries = calls on this handle that were run
 * again in the ticket form because a combiner's bounded spin ran out (a request never fails for it; expected 0 - the granule form is
 * only taken while B * heads * live handles on the GPU <= 192), spin_disabled = the handle has switched to the ticket form for good.
 * raise_flag != 0 raises the give-up flag by hand, so that the NEXT compute call exercises the repeat path (tests). */
int wis_debug_handoff(wis_model_t* m, int raise_flag, int* retries, int* spin_disabled);
/* captured decode-step graphs the handle holds (one per shape and option set; prompts of more than 16 tokens share one whatever their length) */
int wis_debug_graph_count(wis_model_t* m, int* count);
/* the self-attention form of the long-prompt route's decode step on this handle: 1 = dec_self_attn_long_kernel, 0 = the TREE form of dec_self_attn_kernel
 * (what WIS_SA_LONG=0 selects for the process), -1 = back to the switch.  For A/B measurements in one process (tools/prompt_bench.py). */
int wis_debug_sa_long(wis_model_t* m, int form);

/* ---- timing taps: wall/device ms of the stages of the LAST wis_generate on this handle */
typedef struct {
  float logmel_ms, encoder_ms, crosskv_ms, prefill_ms, decode_ms, total_ms;
  int32_t decode_steps;          /* decoder passes enqueued (the merged prefill + first step counts as one) */
  int32_t decode_steps_needed;   /* passes after which every utterance had finished; decode_steps - this = over-run */
} wis_timing_t;
int wis_last_timing(const wis_model_t* m, wis_timing_t* t);

/* ---- tuning tap: shader-clock stamps of the phases of decoder layer 0's kernels for one decode forward at
 * text position `pos` (out: [6][16] uint64: QKV gemv, out-proj gemv, cross-attn, self-attn, FFN1 gemv, FFN2 gemv; more than 8 rows: the
 * batched-row kernels, the fourth row is the cross-attention output projection; the cross-attention row carries two stamp sets, entries 0-5 and 7-13:
 * the first K wave and the first V wave of workgroup (0, 0, 0)) */
int wis_debug_phase_cycles(wis_model_t* m, int B, int beam, int pos, uint64_t* out);
/* ... and, behind such a call at <= 8 rows with the cross-Q fold on, the stamps of the fused out-projection + cross-Q launch's OTHER arm (the folded
 * cross-Q, workgroup 0 of its side of the grid) -> out[16]; the out-proj row above is the out-projection arm */
int wis_debug_phase_cycles_cq_arm(wis_model_t* m, uint64_t* out);

/* ---- tuning tap: device timeline of one decode forward (B x beam rows at text position `pos`): for each of the
 * n_dec_layers * 8 layer kernels (QKV, self-attn, out-proj, cross-Q, cross-attn, cross-out, FFN1, FFN2) the 100 MHz
 * constant-clock time of its first workgroup start and last workgroup end -> out[k][2].  use_graph = 1 replays the
 * forward as a HIP graph (what wis_generate does), 0 launches it eagerly. */
int wis_debug_timeline(wis_model_t* m, int B, int beam, int pos, int use_graph, uint64_t* out, int n_out);
/* ---- tuning tap (tap builds): shader-clock phase stamps of the last beam_step_kernel launch of utterance 0 -> out[2][16]
 * (row 0 reserved for the logit statistics kernel, row 1 = beam step) */
int wis_debug_sampling_cycles(wis_model_t* m, uint64_t* out);

/* ---- roofline tap (bench.py): launch the decoder's weight-streaming skinny-GEMM kernel once over
 * EVERY decoder weight matrix of the model (6 per layer + the vocabulary projection = the weight
 * stream of one decode step, >> the 256 MiB Infinity Cache for the large sizes), `passes` times,
 * with M activation rows, bracketed by HIP events on the model's stream.  Outputs: total device
 * milliseconds, launches per pass, algorithmic (weight) bytes per pass. */
int wis_bench_weight_stream(wis_model_t* m, int M, int passes, float* total_ms, int* launches_per_pass,
                            double* bytes_per_pass);

/* ---- raw device helpers + single-kernel entry points (used by tests/, bench.py roofline
 * timing and __graft_entry__; all pointers below are DEVICE pointers on `device`) -------- */
int wis_dev_alloc(int device, size_t bytes, void** out);
int wis_dev_free(int device, void* p);
int wis_dev_h2d(int device, void* dst, const void* src, size_t bytes);
int wis_dev_d2h(int device, void* dst, const void* src, size_t bytes);
int wis_dev_sync(int device);
/* device-to-device copy between two GPUs of the node (hipMemcpyPeer: over xGMI where the devices are peers).  The replica pool
 * (ctranslate2.models.Whisper(device_index=[0..n-1]), reference main.py:295) uploads the weight arena from the host ONCE and
 * fans it out to the other replicas with this, in a doubling tree. */
int wis_dev_copy_peer(int dst_device, void* dst, int src_device, const void* src, size_t bytes);

/* C[M][N] = epilogue(A[M][K](lda) . W[N][K]^T + bias): the encoder MFMA GEMM.
 * flags: 1 = GELU, 2 = add residual (f32, [M][N]) , 4 = output f32 (else f16), 8 = split-K x2 variant (with 2|4 only) */
int wis_op_gemm(int device, const void* A_f16, int lda, const void* W_f16, const float* bias,
                const float* residual, void* C, int M, int N, int K, int flags);
/* y f16 [M][d] = LayerNorm(x f32 [M][d]) * gamma + beta, eps 1e-5 */
int wis_op_layernorm(int device, const float* x, const float* gamma, const float* beta,
                     void* y_f16, int M, int d);
/* non-causal MHA over T keys: qk f16 [B*T][2d] (Q pre-scaled | K), vt f16 [B][H][64][Tpad] with key t stored at
 * (t & ~12) | ((t & 4) << 1) | ((t & 8) >> 1) (bits 2, 3 swapped inside groups of 16: the P.V MFMA fragment order),
 * out f16 [B*T][d] */
int wis_op_enc_attention(int device, const void* qk_f16, const void* vt_f16, void* out_f16,
                         int B, int T, int Tpad, int H);
/* the same attention with the kernel named: form bit 0 = the lazy-reference loop (enc_attn_lazy_kernel: Q must already carry
 * log2(e) / sqrt(64), as the engine's query projection delivers it; the tap makes no scaled copy), clear = enc_attn_kernel (Q carries
 * 1 / sqrt(64)); bit 1 = the split-key pair (two workgroups per query tile and head, merged in the launch), WIS_E_ARG when
 * cdiv(T, 64) < 4.  wis_op_enc_attention above chooses as the encoder does (and scales a private copy of Q for the lazy loop).
 * Both entries, and the encoder: the V^T positions of keys >= T up to Tpad must hold FINITE values.  Those keys get weight exactly 0,
 * but the P.V product still multiplies them (0 x NaN or 0 x inf would poison the whole row); the engine zeroes the image once at
 * allocation and nothing writes those positions afterwards.  K rows >= T are never read (the loaders clamp to row T - 1). */
int wis_op_enc_attention_ex(int device, const void* qk_f16, const void* vt_f16, void* out_f16,
                            int B, int T, int Tpad, int H, int form);
/* skinny GEMM used by the decoder: y[M][N] = epi(LN?(x)[M][K] . W[N][K]^T + bias); W is the
 * plain row-major f16 matrix (packed internally for the call).
 * flags: 1 = GELU, 2 = residual add in place into y f32, 4 = y f32 (else f16), 8 = fuse LayerNorm
 * (x is f32 [M][K], gamma/beta given); without 8, x is f16 [M][K]; 32 = quantise W to per-row int8 first (int8_float16). */
int wis_op_gemv(int device, const void* x, const float* gamma, const float* beta,
                const void* W_f16, const float* bias, void* y, int M, int N, int K, int flags);
/* the one-utterance FFN2 / cross-attention out-projection form of that GEMM (x f16 [M][K], K = 1280 or 5120, M x K / 8 <= 3328, M <= 16) on
 * sixteen-column (cols = 16) or eight-column (cols = 8) workgroup tiles of the same W; N a multiple of cols.  flags: 1, 2, 4 as above;
 * y16: optional f16 copy of the rows under flag 2, else null. */
/* cols = 5: the stage as the decode step assembles it for a projection that carries the sixteen-column image and, where the model loader would add one,
 * the five-column image (FFN2: K = 5120, f16 rows, N a multiple of 5, N / 5 workgroups in one dispatch round on the device).  The step's own predicate
 * picks the kernel: a shape it refuses runs on sixteen-column tiles (N a multiple of 4 then; any M <= 16 and K % 128 == 0 that launch_gemv serves).
 * flags with cols = 5: additionally 32 = quantise W to per-row int8 first (no five-column image then). */
int wis_op_gemv_cols(int device, const void* x_f16, const void* W_f16, const float* bias, void* y, void* y16,
                     int M, int N, int K, int flags, int cols);

/* decoder self-attention of ONE new token per row over its cached history (the kernel inside every decode step):
 * q f32 [M][d] (pre-scaled by 1/sqrt(64)), kc / vc f16 [slots][ctx][d] (row m reads positions 0..pos[m] of logical slot
 * (m / rpu) * sstride + (m % rpu) * rmul), pos i32 [M] -> out f16 [M][d].  64 <= ctx <= 512, d = 64 H. */
int wis_op_dec_self_attn(int device, const float* q, const void* kc_f16, const void* vc_f16, const int32_t* pos, void* out_f16,
                         int M, int H, int ctx, int rpu, int sstride, int rmul);
/* decoder cross-attention of the R (<= 16) query rows of each of B utterances over that utterance's T encoder keys, split into
 * `chunks` key chunks (6 -> 256-key, 12 -> 128-key chunks for T = 1500) with the in-launch combine:
 * q f32 [B*R][d] (pre-scaled), kx f16 [B][H][8][T][8] (element (t, 8 c + j) of head h at ((h*8 + c)*T + t)*8 + j),
 * vt f16 [B][H][64][Tpad] (V transposed, zero padded to Tpad = T rounded up to 64) -> out f16 [B*R][d]. */
int wis_op_dec_cross_attn(int device, const float* q, const void* kx_f16, const void* vt_f16, void* out_f16,
                          int B, int R, int H, int T, int chunks);
/* the same with the LayerNorm-folded query of the one-utterance decode step (model.hip fused_out_cq): q_raw f32 [B*R][d] is the folded
 * projection of the UN-normalised rows, xres f32 [B*R][d] the rows themselves; the kernel reduces mean / rstd of every row and
 * finishes q = rstd (q_raw - mean qcs) + qb (qcs, qb f32 [d]: column sums and bias of the folded projection).  R <= 8, d <= 1280. */
int wis_op_dec_cross_attn_folded(int device, const float* q_raw, const float* xres, const float* qcs, const float* qb,
                                 const void* kx_f16, const void* vt_f16, void* out_f16, int B, int R, int H, int T, int chunks);

/* ---- taps of the forms the decode step launches (tests/test_gpu_dec_step_ops.py).  They add arguments and the loader's preparation only: which
 * kernel instantiation runs is decided by the product's own launch_* functions, as in a decode step. */
/* cross-attention with the query folded from ROW PARTIALS (dec_forward / dec_forward_frag at <= 8 rows per utterance): q (+ q2, optional) f32 [B*R][d]
 * the halves of q_raw, stat f32 [B*R][d/16][2] the (sum x, sum (x - tile mean)^2) pairs per 16 columns of the un-normalised rows; the kernel merges
 * mean / rstd from them and finishes q = rstd (q + q2 - mean qcs) + qb.  R <= 8, d <= 2048.  stat = qcs = qb = q2 = NULL: the plain form (q finished).
 * out_mb > 0: out is the MFMA fragment image of out_mb >= ceil(B R / 16) row blocks (zero-filled first; element (m, k) at
 * (((k / 32) out_mb + m / 16) 64 + m % 16 + 16 ((k / 8) % 4)) 8 + k % 8), else f16 [B*R][d].  kv_shared = 1: every group b reads utterance 0's K / V
 * (draft verification).  no_spin = 1: no granule hand-off buffers are passed (the ticket form), as a handle does after a give-up; they are also
 * withheld above 192 (utterance, head) pairs.  Three launches per call on one set of tickets / epochs. */
int wis_op_dec_cross_attn_stat(int device, const float* q, const float* q2, const float* stat, const float* qcs, const float* qb,
                               const void* kx_f16, const void* vt_f16, void* out_f16, int B, int R, int H, int T, int chunks,
                               int out_mb, int kv_shared, int no_spin);
/* wis_op_dec_self_attn with the step's other choices: nb = 2 / 4 / 8 eight-position blocks per pass (the step graphs: 2 up to 16 cached positions,
 * 4 up to 32), out_mb > 0: the fragment image as above, and the TREE form (anc != NULL; draft verification): anc i32 [M][aw] - row m reads positions
 * < w0 from slot base[m] (base NULL: anc[m][0]) and position w0 + t from slot anc[m][min(t, aw - 1)]; rpu / sstride / rmul are unused then. */
int wis_op_dec_self_attn_ex(int device, const float* q, const void* kc_f16, const void* vc_f16, const int32_t* pos, void* out_f16,
                            int M, int H, int ctx, int rpu, int sstride, int rmul, int nb, int out_mb,
                            const int32_t* anc, int w0, int aw, const int32_t* base);
/* the decode step's self-attention behind a prompt of more than 16 tokens (the long-prompt route): B utterances of k <= 8 rows, row m = b k + j.  Row m
 * reads positions < plen[b] from slot b k - the prompt prefix, kept once per utterance - and positions plen[b] .. pos[m] from its own slot b k + j; nothing
 * else is read unmasked (reads beyond a row's length come from clamped positions of those two slots).  q f32 [B k][d], kc / vc f16 [B k][ctx][d], pos i32
 * [B k] (>= plen[b] - 1), plen i32 [B] in [1, 256] (device memory, as pos) -> out f16 [B k][d], or the fragment image of out_mb row blocks as above. */
int wis_op_dec_self_attn_long(int device, const float* q, const void* kc_f16, const void* vc_f16, const int32_t* pos, const int32_t* plen, void* out_f16,
                              int B, int k, int H, int ctx, int out_mb);
/* the self-attention QKV projection behind its LayerNorm with the scatter epilogue (GV_LN | GV_QKV), prepared as the loader prepares it (LayerNorm
 * fold, 1/8 on the query rows, packing): x f32 [M][d], W f16 [3d][d], bias f32 [3d] -> q f32 [M][d]; row m's key / value rows go to
 * kc / vc f16 [slots][ctx][d] at (slot[m], pos[m]).  M <= 8: the LDS-staged form; more rows: fragment image + row partials (launch_gemv_frag). */
int wis_op_gemv_qkv(int device, const float* x, const float* gamma, const float* beta, const void* W_f16, const float* bias,
                    const int32_t* slot, const int32_t* pos, float* q, void* kc_f16, void* vc_f16, int M, int d, int ctx);
/* the fused stage behind the self-attention: x1 = x0 + Wo a + bo with the LayerNorm partials of x1, and q_raw = W'q x0 + (W'q Wo) a + W'q bo of the
 * cross-attention query folded THROUGH the out-projection (W'q = (Wq o gamma) / 8; model.hip build_cq_fold, the loader's own code).
 * a f16 [M][d], x0 f32 [M][d], Wo / Wq f16 [d][d], bo / bq / gamma / beta f32 [d] -> x1 f32 [M][d], stat f32 [M][d/16][2], qcs / qb f32 [d] (column
 * sums and bias of the folded projection: what wis_op_dec_cross_attn_stat takes).  M <= 8 and force_frag = 0: one launch_gemv_dual, q = q_raw, q2
 * untouched (may be NULL); otherwise launch_gemv_frag3: q = W'q x0 + W'q bo, q2 = (W'q Wo) a. */
int wis_op_gemv_out_cq(int device, const void* a_f16, const float* x0, const void* Wo_f16, const float* bo, const void* Wq_f16, const float* bq,
                       const float* gamma, const float* beta, float* x1, float* stat, float* q, float* q2, float* qcs, float* qb,
                       int M, int d, int force_frag);
/* the wave reductions of the LayerNorm-folded projections' tail, side by side: ONE wave takes x f32 [N][64] (value i of lane l at x[i][l]) and runs
 * wave_sum on each of the N values and then wave_sums<N> on the same registers, in one launch -> out_old / out_new f32 [N][64], every lane's result of
 * either (all 64 words of a value are equal, and out_new equals out_old bit for bit: the tree is the contract).  N = 6, 10 or 16: the 2 RM sums of
 * the three row-register forms of gemv_kernel MODE 1; any other N is WIS_E_ARG. */
int wis_op_wave_sums(int device, const float* x, int N, float* out_old, float* out_new);
/* ONE projection stage of the batched decode route (9 .. 96 rows), assembled by the builders the decoder forward itself uses; W f16 [N][K] row-major and
 * bias f32 [N] are prepared as the loader does (w8 != 0: quantised to per-row int8 first; stages 1 / 2: the LayerNorm gamma / beta folded in).
 *   stage 0  residual: y f32 [M][N] += x W^T + bias in place; y_xf (optional) the produced rows' f16 fragment image of ceil(M / 16) row blocks
 *            ([N/32][blocks][64][8], rows >= M untouched); stat_out (optional) f32 [M][N/16][2] = per 16 columns (sum, sum of squares about the tile mean)
 *   stage 1  LayerNorm-folded + GELU, f16 rows into the fragment image y_xf (FFN1); y unused
 *   stage 2  LayerNorm-folded, y f32 [M][N] (cross-Q, vocabulary)
 * x, x_is_image = 0: row-major [M][K], f16 for stage 0, f32 for stages 1 / 2 (the tap builds image and partials as wis_op_gemv does; xmb = 0).
 * x_is_image = 1: a ready f16 fragment image of xmb row blocks (0: ceil(M / 16)) and, for stages 1 / 2, stat_in f32 [M][K/16][2]: what an earlier stage 0
 * call or wis_op_dec_embed left in y_xf / stat_out - the hand-off between the stages of a layer.
 * ksplit: -1 = what the decoder forward asks for (stage 0: its FFN2 rule, two K slices where K / 128 is even - honoured by the launcher at one row block;
 * else none), 1 .. 8 = that many slices; with slices the launch runs twice on one set of tickets (stage 0: the residual rows put back in between). */
int wis_op_gemv_frag_stage(int device, int stage, const void* x, int x_is_image, int xmb, const float* stat_in, const float* gamma, const float* beta,
                           const void* W_f16, const float* bias, int w8, float* y, void* y_xf_f16, float* stat_out, int M, int N, int K, int ksplit);
/* the decoder's embedding launches: x f32 [M][d] = emb[tok[m]] + pos_emb[pos[m]] (f16 tables [n_vocab][d], [n_ctx][d]; tok / pos HOST arrays, checked).
 * xf given (with stat): the batched form - x, the rows' f16 fragment image of ceil(M / 16) row blocks and partials f32 [M][d/16][2] in one pass (xh null);
 * else the form of <= 8 rows: x and, if xh is given, its f16 copy [M][d] (stat null). */
int wis_op_dec_embed(int device, const void* emb_f16, const void* pos_f16, const int32_t* tok, const int32_t* pos, float* x, void* xh_f16, void* xf_f16,
                     float* stat, int M, int d, int n_vocab, int n_ctx);

/* ---- taps of what the encoder and the cross K/V projection launch (tests/test_gpu_enc_ops.py).  The same rule: arguments and the loader's preparation
 * only - the GEMM descriptions are the helpers run_encoder itself calls, the tile and kernel are chosen by launch_gemm_* / gemm_pick_tile from the
 * shape, as in the encoder.  B and T are free (the encoder: T = 3000 / 1500).  All pointers are device memory. */
/* mel f32 [B][n_mels][3000] -> conv1 input image f16 [B][3002][C] rows 1..3000 (C = 96 for 80 bins, channels 80..95 zero; 128 for 128 bins); rows 0
 * and 3001 are not written.  Any other n_mels: WIS_E_UNSUPPORTED. */
int wis_op_mel_to_image(int device, const float* mel, void* img_f16, int B, int n_mels);
/* the encoder's convs as implicit-im2col GEMMs (kernel 3, padding 1); W [N][Cin][3] f32 or f16 (w_is_f16), packed here as the loader packs it.
 * which = 1 (stride 1): img f16 [B][T+2][C] (Cin = 80 -> C = 96, K = 320; Cin = 128 -> C = 128, K = 384; anything else WIS_E_UNSUPPORTED) followed
 *   by 64 readable elements (the zero-weighted columns of the last row read 32 past the image at Cin = 80) -> out f16 [B][T+2][N], GELU(conv + bias)
 *   at row t + 1; rows 0 and T + 1 of every utterance are not written.  pos unused.
 * which = 2 (stride 2): img f16 [B][2T+2][Cin] (Cin % 64 == 0) -> out f32 [B*T][N] = GELU(conv + bias) + pos[m % T] (pos f32 [T][N]).
 * N % 128 == 0. */
int wis_op_enc_conv(int device, int which, const void* img_f16, const void* W, int w_is_f16, const float* bias, const float* pos, void* out,
                    int B, int T, int Cin, int N);
/* the encoder layer's fused QKV projection (d = 64 H): xn f16 [B*T][d], W f16 [3d][d], bias f32 [3d] -> qk f16 [B*T][2d] = [Q | K] rows and the V^T image
 * vt f16 [B][H][64][Tpad] that wis_op_enc_attention reads (key t at (t & ~12) | ((t & 4) << 1) | ((t & 8) >> 1); Tpad = T rounded up to 64; positions
 * that belong to no key < T are not written).  T % 4 != 0: WIS_E_ARG (the transposed V tiles store 4 consecutive keys of one utterance). */
int wis_op_enc_qkv(int device, const void* xn_f16, const void* W_f16, const float* bias, void* qk_f16, void* vt_f16, int B, int T, int H);
/* every decoder layer's cross-attention K / V projection of the encoder memory in one GEMM: mem f16 [B*T][d], W f16 [L*2d][d] (per layer: d key rows,
 * then d value rows), bias f32 [L*2d] -> layer l's images at kx + l kx_lstride (f16 [B][H][8][T][8]) and vt + l vt_lstride (f16 [B][H][64][Tpad], keys
 * >= T not written): what wis_op_dec_cross_attn reads.  Strides in elements, multiples of 8 and at least the image size; T % 4 != 0: WIS_E_ARG. */
int wis_op_enc_crosskv(int device, const void* mem_f16, const void* W_f16, const float* bias, void* kx_f16, void* vt_f16, int B, int T, int H, int L,
                       int64_t kx_lstride, int64_t vt_lstride);
/* the encoder's K-split FFN2 with the fused reduction + LayerNorm: X f32 [M][N] (residual in) += A f16 [M][K] . W f16 [N][K]^T + bias, and
 * Y f16 [M][N] = LayerNorm(new X) gamma + beta.  splits = 0: what the encoder takes for N = d at M rows (none: WIS_E_UNSUPPORTED); the fused form
 * exists for 2 and 4 splits and N <= 2048, K % (64 splits) == 0 (otherwise the launch function's error code). */
int wis_op_gemm_splitk_ln(int device, const void* A_f16, const void* W_f16, const float* bias, float* X, const float* gamma, const float* beta,
                          void* Y_f16, int M, int N, int K, int splits);

/* ---- the resampler's kernel alone (tests/test_gpu_resample_ops.py): outputs m0 .. m0 + count - 1 (out f32 [count]) of a signal of
 * n_in_total samples at the reduced ratio up / down to 16 kHz, from the slice x_slice f32 [n_slice] = samples k_base .. k_base +
 * n_slice - 1 of that signal (device pointers).  The slice must hold every sample of the signal those outputs read (else
 * WIS_E_ARG); samples outside [0, n_in_total) are zeros.  k_base and m0 are 64-bit: positions past 2^31 are ordinary. */
int wis_op_resample_segment(int device, const float* x_slice, int64_t n_slice, int64_t k_base, int64_t n_in_total, int64_t m0, int64_t count,
                            int up, int down, float* out);

/* ---- the log-mel front end's kernels on caller-supplied device memory, their scratch exposed (tests/test_gpu_logmel_ops.py).  d_pcm: n_win windows,
 * window w at d_pcm + w stride with n_samples[w] valid samples (n_samples is a HOST array and reaches the kernel unclamped: values below 0 or above
 * 480000 are the kernel's to handle; samples behind n_samples[w] are never read as signal).  d_logspec f32 [n_win][n_mels][3000] is the log10 mel
 * spectrum before the floor, d_gmax u32 [n_win] the order-preserving key of each window's maximum.
 * (tile0, n_tiles) == (0, 188): the whole window as the model's input stage runs it - d_mel f32 [n_win][n_mels][3000] and / or the conv1 image
 *   d_img_f16 [n_win][3002][C] (C = 96 for 80 bins, 128 for 128; rows 0 and 3001 are not written), either may be null.
 * any other range: d_gmax is zeroed and the 16-frame tiles [tile0, tile0 + n_tiles) alone are computed, as a streaming session does: no other frame of
 *   d_logspec is written, d_gmax is the maximum over the range, and there is no finalize pass - d_mel and d_img_f16 must be null (WIS_E_ARG); a range
 *   outside [0, 188] is WIS_E_ARG.
 * n_mels other than 80 / 128: WIS_E_UNSUPPORTED. */
int wis_op_logmel(int device, int n_mels, const float* d_pcm, int64_t stride, const int64_t* n_samples, int n_win, int tile0, int n_tiles,
                  float* d_logspec, unsigned* d_gmax, float* d_mel, void* d_img_f16);

/* ---- taps of what runs behind the logits (tests/test_gpu_sample_ops.py): the product's launch functions on caller-supplied device memory. */
/* the cache permutation after a beam step, in place: kc / vc f16, layer l at + l layer_stride_elems, [slots][ctx][d] each (d % 8 == 0); for every
 * utterance b with done[b] == 0, slot b beam + j becomes a copy of slot parent[b beam + j] (a slot of the same utterance) at positions
 * < P - 1 + step_u[b] (<= ctx: the caller's duty), all L layers, K and V; nothing else is written.  beam = 1: nothing runs. */
int wis_op_kv_reorder(int device, void* kc_f16, void* vc_f16, int64_t layer_stride_elems, int L, const int32_t* parent, const int32_t* step_u,
                      const int32_t* done, int B, int beam, int P, int ctx, int d);
/* wis_op_kv_reorder behind a long prompt: plen i32 [B] (device memory) in P's place, and a lower bound - for every utterance b with done[b] == 0, slot
 * b beam + j becomes a copy of slot parent[b beam + j] at positions [plen[b], plen[b] - 1 + step_u[b]) only; positions < plen[b] of every slot (the prompt
 * prefix lives in slot b beam alone) and everything else stay as they are. */
int wis_op_kv_reorder_from(int device, void* kc_f16, void* vc_f16, int64_t layer_stride_elems, int L, const int32_t* parent, const int32_t* step_u,
                           const int32_t* done, const int32_t* plen, int B, int beam, int ctx, int d);
/* the cache gather after a verified draft window (one utterance), in place: vstate i32 [32 + 8 x 32]: [2] = window steps nwin (<= 32, w0 + nwin <= ctx:
 * the caller's duty), [16 + j] = the slot that holds beam j's positions < w0, [32 + 32 j + u] = the slot that holds its position w0 + u; slot j (< beam)
 * becomes that history.  done[0] == 1 or nwin <= 0: nothing is written (done[0] == 2, a parked search, still gathers). */
int wis_op_kv_gather(int device, void* kc_f16, void* vc_f16, int64_t layer_stride_elems, int L, const int32_t* vstate, const int32_t* done,
                     int beam, int w0, int ctx, int d);
/* out[b] = softmax(logits row b rs + r0 over ids [0, V))[ns]; logits f32, row stride ld >= V.  ns outside [0, V): WIS_E_ARG. */
int wis_op_no_speech(int device, const float* logits, int ld, int B, int rs, int r0, int V, int ns, float* out);
/* the same with one row per utterance (wis_generate_ragged): rows i32 [B] in device memory; out[b] = softmax(logits row b rs + rows[b])[ns] where rows[b]
 * lies in [0, rs), and out[b] is left as it is otherwise (the utterance is not in this pass). */
int wis_op_no_speech_rows(int device, const float* logits, int ld, int B, int rs, const int32_t* rows, int V, int ns, float* out);
/* probs f32 [B][n_lang] = softmax over the n_lang listed ids of logits row b (row stride ld) */
int wis_op_lang_probs(int device, const float* logits, int ld, const int32_t* lang_ids, int n_lang, float* probs, int B);
/* the teacher-forced greedy pick: logit statistics (suppress_blank on, no fixed length, n_cand = 2) of B x beam rows, then the k = 1 pick of each.
 * Row (b, j) reads logits row b lr_b + (rowmap ? rowmap[j] : j) lr_j + lr_off (row stride n_vocab_pad) at step step_u[b]: bias_begin (f32 [n_vocab])
 * is added at step 0 only, bias_all (f32 [n_vocab] or NULL) always.  tok_out i32 / lp_out f32 [B x beam]: token (lowest id among equal maxima) and
 * its log-probability.  rowmap i32 [beam] or NULL.  Scratch is the tap's own. */
int wis_op_greedy_rows(int device, const float* logits, int n_vocab, int n_vocab_pad, int eot, const float* bias_all, const float* bias_begin,
                       const int32_t* step_u, int B, int beam, int lr_b, int lr_j, int lr_off, const int32_t* rowmap, int32_t* tok_out, float* lp_out);
/* the phrase mask of one step (phrase_rules_kernel), in place, all pointers device memory: logits f32 rows of stride n_vocab_pad - row (b, j) is
 * b lr_b + j lr_j + lr_off, lr_j = 0: the utterance's beams share one row and its first workgroup masks it -, trie i32 [n_rec][4] (the layout of
 * wis_model_set_phrases; NOT validated here: the kernel itself refuses every child range and token outside the table / the vocabulary, such a
 * row stays as it is), alive i32 [B x beam][max_new] histories of which the first min(step_u[b], max_new) entries count, step_u / done i32 [B].
 * 1 <= n_rec <= 65535, 0 <= eot < n_vocab <= n_vocab_pad, 1 <= max_new <= 256, beam <= 8, B x beam <= 96: anything else WIS_E_ARG. */
int wis_op_phrase_rules(int device, float* logits, int n_vocab, int n_vocab_pad, int eot, const int32_t* trie, int n_rec, const int32_t* alive,
                        const int32_t* step_u, const int32_t* done, int B, int beam, int max_new, int lr_b, int lr_j, int lr_off);
/* the phrase mask with the in-grammar mass (phrase_rules_mass_kernel; wis_gen_opts_t::phrase_mass states the rule): wis_op_phrase_rules' arguments and
 * its mask, bit for bit, plus bias_all f32 [n_vocab] or NULL (no list), bias_begin f32 [n_vocab] (added when step_u[b] == 0 and suppress_blank != 0) and
 * logmass f32 [B][n_rec]: the row's value is stored at logmass[b n_rec + record index of the row's node], every other slot keeps its bits (finished
 * utterances, histories off the trie, beams j > 0 of a shared row write nothing; every other row counts as live).  n_vocab <= 65536. */
int wis_op_phrase_mass(int device, float* logits, int n_vocab, int n_vocab_pad, int eot, const int32_t* trie, int n_rec, const int32_t* alive,
                       const int32_t* step_u, const int32_t* done, int B, int beam, int max_new, int lr_b, int lr_j, int lr_off,
                       const float* bias_all, const float* bias_begin, int suppress_blank, float* logmass);
/* the sums along finished results (phrase_mass_gather_kernel): ids i32 [B n][id_ld], len i32 [B n], score f32 [B n] or NULL (a result whose score is not
 * above -inf is a filler), trie i32 [n_rec][4], logmass f32 [B][n_rec] -> out f32 [B n].  All device memory; B n <= 96, 1 <= id_ld <= 256. */
int wis_op_phrase_mass_gather(int device, const int32_t* ids, const int32_t* len, const float* score, const int32_t* trie, int n_rec,
                              const float* logmass, int B, int n, int id_ld, float* out);
/* the hotword boost of one step (hotword_rules_kernel; THE HOTWORD RULE), in place: wis_op_phrase_rules' arguments, all pointers device memory,
 * plus fixed_new (> 0: utterances with min(step_u[b], max_new) >= fixed_new are left alone, the forced-EOT step) and the boost (finite, > 0).
 * UNLIKE that tap the table IS validated - read back and checked on the host by the engine's validator (token rules against eot / n_vocab, no
 * suppress lists) - and a malformed one is WIS_E_ARG before anything is launched.  n_vocab <= 65536. */
int wis_op_hotword_rules(int device, float* logits, int n_vocab, int n_vocab_pad, int eot, const int32_t* trie, int n_rec, const int32_t* alive,
                         const int32_t* step_u, const int32_t* done, int B, int beam, int max_new, int fixed_new, float boost,
                         int lr_b, int lr_j, int lr_off);

/* ---- speaker verification (replaces the reference's WavLMForXVector embedder, main.py:306-316 / do_sv 797-879): one handle = the
 * WavLM-base-plus-sv x-vector model on one GPU.  Input: mono 16 kHz f32 PCM in host memory, already through the reference's
 * preprocessing (sox gain + trim, the feature extractor's zero-mean / unit-variance normalisation: wis_hip/sv.py); output: the
 * 512-float embedding (`.embeddings`, un-normalised) in host memory.  Cosine scoring against the enrolled speakers stays on the host.
 * A handle runs one call at a time (the Python wrapper holds a lock). */
typedef struct wis_sv wis_sv_t;
typedef struct {
  int32_t conv_dim;                 /* 512: every feature-encoder layer */
  int32_t n_conv_layers;            /* 7 */
  int32_t conv_kernel[8], conv_stride[8];     /* 10,3,3,3,3,2,2 / 5,2,2,2,2,2,2 */
  int32_t hidden_size, n_heads, n_layers, intermediate_size;      /* 768, 12, 12, 3072 */
  int32_t num_conv_pos_embeddings, num_conv_pos_embedding_groups; /* 128, 16 */
  int32_t num_buckets, max_bucket_distance;                       /* 320, 800 */
  int32_t n_tdnn;                   /* 5 */
  int32_t tdnn_dim[8], tdnn_kernel[8], tdnn_dilation[8];          /* 512,512,512,512,1500 / 5,3,3,1,1 / 1,2,3,1,1 */
  int32_t xvector_output_dim;       /* 512 */
  int64_t max_samples;              /* longest input a call may pass; buffers are sized for it at creation (0 => 160000 = 10 s) */
} wis_sv_config_t;
/* tensors: Hugging Face state-dict names of WavLMForXVector ("wavlm.encoder.layers.0.attention.q_proj.weight", "tdnn.0.kernel.weight",
 * "layer_weights", ...), with two layout conventions the Python loader applies: the feature-encoder conv weights are stored
 * [out][k][in] (the order the channels-last GEMM reads its im2col rows in), and the positional conv's weight norm is folded into
 * "wavlm.encoder.pos_conv_embed.conv.weight" as [out][k][in / groups].  Any other architecture: WIS_E_UNSUPPORTED. */
int    wis_sv_create(const wis_sv_config_t* cfg, const void* arena, size_t arena_bytes, int arena_on_device,
                     const wis_tensor_t* tensors, int n_tensors, int device, wis_sv_t** out);
void   wis_sv_destroy(wis_sv_t* sv);
size_t wis_sv_device_bytes(const wis_sv_t* sv);
/* emb: [512] f32.  n > max_samples: WIS_E_STATE; audio too short to leave two frames after the TDNN layers: WIS_E_ARG. */
int    wis_sv_embed(wis_sv_t* sv, const float* pcm, int64_t n, float* emb);
/* host only (no device needed): the relative-position buckets of HF WavLMAttention._relative_positions_bucket for the n distances
 * first, first + 1, ... (key position - query position) -> out[n] */
int    wis_sv_rel_buckets(int num_buckets, int max_distance, int first, int n, int32_t* out);
/* parity tap (tests): runs the forward pass on `pcm` and copies out, as f32 row-major [rows][cols]:
 * tap 0 = feature-encoder output [T][512]; tap 1 = hidden state `layer` [T][768] (0 = encoder input after the positional conv and
 * LayerNorm, l = output of layer l, HF hidden_states[l]); tap 2 = output of the last TDNN layer after its ReLU [T - 14][1500]. */
int    wis_debug_sv_taps(wis_sv_t* sv, const float* pcm, int64_t n, int tap, int layer, float* out, int64_t cap_floats,
                         int32_t* rows, int32_t* cols);
/* single-kernel taps of the speaker-verification kernels (tests): every pointer is device memory, each call launches the kernels
 * sv_forward launches, with the same grids, on the device's op stream and synchronises.
 * conv 0 + GroupNorm(512 groups, eps 1e-5) + GELU: pcm f32 [n], w0 f32 [512][10], gamma / beta f32 [512] -> y f16 [T0][512],
 * T0 = (n - 10) / 5 + 1 */
int    wis_op_sv_conv0(int device, const float* pcm, int64_t n, const float* w0, const float* gamma, const float* beta, void* y_f16);
/* positional conv (k128, pad 64, 16 groups, last output dropped) + bias, GELU, + residual: x f32 [T][768], W f16 [768][128][48],
 * bias f32 [768] -> out f32 [T][768] */
int    wis_op_sv_posconv(int device, const float* x, const void* W_f16, const float* bias, float* out, int T);
/* gated relative-position attention of 12 heads: qkv f16 [T][2304] (Q pre-scaled by 1/8 | K | V), xin f32 [T][768] (the layer input,
 * for the gate), gw f32 [8][64], gb f32 [8], gconst f32 [12], tab f32 [12][2L - 1] (entry key - query + L - 1), L >= T -> out f16 [T][768] */
int    wis_op_sv_attention(int device, const void* qkv_f16, const float* xin, const float* gw, const float* gb, const float* gconst,
                           const float* tab, int L, void* out_f16, int T);
/* LayerNorm (eps 1e-5) of x [M][d] (f16 if in_f16, else f32), d = 512 or 768 -> y16 f16, y32 f32 (optional); wmode 1: ws = wl y,
 * 2: ws += wl y (f32 [M][d]); ws16 (optional): f16 copy of the updated ws */
int    wis_op_sv_layernorm(int device, const void* x, int in_f16, const float* gamma, const float* beta, void* y16, float* y32,
                           float* ws, void* ws16, float wl, int wmode, int M, int d);
/* x-vector tail: stats [2n] = mean and unbiased std over T rows of ReLU(z[t][0 .. n - 1]) (z f32, row stride ldz >= n), then
 * emb [512] = W_fe [512][2n] . stats + b_fe */
int    wis_op_sv_xvector_tail(int device, const float* z, int ldz, int T, int n, const float* W_fe, const float* b_fe,
                              float* stats, float* emb);

#ifdef __cplusplus
}
#endif
#endif /* WIS_HIP_H */
