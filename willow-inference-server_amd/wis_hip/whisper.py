"""The ASR orchestrator: what the reference's `do_whisper` does (main.py:554-770), on the wis_hip engine.

Same call signature, same per-request selection surface (model in {tiny, base, small, medium, large} - and, beyond the reference,
large-v3 / large-v3-turbo (128 mel bins, 51866 tokens; V3_MODEL_SIZES) - beam_size,
detect_language, force_language, translate; main.py:564-573) and the same 6-tuple result
    (language, text, infer_time_ms, translation, infer_speedup, audio_duration_ms)          (main.py:763-770)
including the reference's behaviours: >= long_beam_size_threshold ms switches to long_beam_size (main.py:582-586),
> 30 s is chunked into 22 s windows with 4 s context, decoded `concurrent_gpu_chunks` at a time and stitched with
find_longest_common_sequence (main.py:588-611, 677-711).

`timestamps=True` decodes without <|notimestamps|> (CTranslate2 then applies Whisper's timestamp rules) and attaches
`.segments` = [{start, end, text}] (segments_from_tokens); `text` stays free of timestamp tokens.  One 30 s window - or, with
long_form="seek", a recording of any length through openai-whisper's seek loop (wis_hip.longform) over one whole-recording log-mel.

No tokenizer files exist offline (the reference loads HF WhisperProcessor from the model dir, main.py:329-334):
prompt ids are the fixed multilingual ids; `text` is produced by an optional tokenizer
(`tokenizers` JSON next to the model) and otherwise is the space-joined token ids.  The returned tuple also
carries `.tokens`.
"""
import math
import os
import threading
import time
from types import SimpleNamespace

import numpy as np

from . import audio, ctranslate2, weights as W
from .languages import LANGUAGE_CODES, LANGUAGE_CODES_V3, LANGUAGES
from .settings import get_api_settings

MODEL_SIZES = ("tiny", "base", "small", "medium", "large")
V3_MODEL_SIZES = ("large-v3", "large-v3-turbo")      # served on request; preload only by their own settings (preload_whisper_model_large_v3[_turbo])
SPECIAL_IDS = list(range(W.EOT, W.N_VOCAB))     # <|endoftext|> ... timestamps: everything >= 50257 is special


TIMESTAMP_BEGIN = W.NO_TIMESTAMPS + 1      # <|0.00|>; timestamp token t means (t - TIMESTAMP_BEGIN) * 0.02 s
TIME_PRECISION = 0.02
WINDOW_S = 30.0


class WhisperResult(tuple):
    """6-tuple like the reference's return value, plus the raw token ids (and, decoded with timestamps, the segments)."""
    tokens = None
    translation_tokens = None
    segments = None
    seek = None          # long_form="seek": one record per decoded window (longform.transcribe)


def model_special_tokens(model):
    """The special-id table of a loaded model (ctranslate2.Whisper.special); the 51865-token table for anything that has none."""
    st = getattr(model, "special", None)
    return st if isinstance(st, W.SpecialTokens) else W.special_tokens(W.N_VOCAB)


def segments_from_tokens(ids, tokenizer, offset=0.0, duration=WINDOW_S, special=None, keep_tokens=False):
    """Timed segments of one decoded window, split as openai-whisper's transcribe() splits a window's tokens: two consecutive
    timestamps close one segment and open the next; a single timestamp before the end (EOT) closes the last segment; text that
    no timestamp closes ends at the window's `duration`.  A window with no consecutive pair is one segment from `offset` to its last
    timestamp (or to `duration` when that is <|0.00|> or there is none).  -> [{"start", "end", "text"}], seconds + `offset`.
    special: the model's SpecialTokens (default: the 51865-token vocabulary)."""
    tb, eot = (TIMESTAMP_BEGIN, W.EOT) if special is None else (special.timestamp_begin, special.eot)
    toks = [int(t) for t in ids if int(t) != eot]
    is_ts = [t >= tb for t in toks]

    def seg(start, end, piece):
        d = {"start": round(offset + start, 2), "end": round(offset + end, 2), "text": tokenizer.decode([t for t in piece if t < eot]).strip()}
        if keep_tokens:      # (word_timestamps: the segment's text tokens, for the alignment)
            d["tokens"] = [t for t in piece if t < eot]
        return d

    def at(t):
        return (t - tb) * TIME_PRECISION
    slices = [i + 1 for i in range(len(toks) - 1) if is_ts[i] and is_ts[i + 1]]
    single_ending = is_ts[-2:] == [False, True]
    out = []
    if slices:
        if single_ending:
            slices.append(len(toks))
        last = 0
        for cur in slices:
            piece = toks[last:cur]
            out.append(seg(at(piece[0]), at(piece[-1]), piece))
            last = cur
        tail = toks[last:]
        if any(not f for f in is_ts[last:]):
            out.append(seg(at(tail[0]) if tail[0] >= tb else out[-1]["end"] - offset, duration, tail))
    elif toks:
        stamps = [t for t in toks if t >= tb]
        end = at(stamps[-1]) if stamps and stamps[-1] != tb else duration
        out.append(seg(0.0, end, toks))
    return out


def special_ids_from_tokenizer_json(path):
    """`tokenizer.all_special_ids` as HF computes it for a fast tokenizer: the ids of the `added_tokens` entries flagged
    `special: true` in tokenizer.json (for the Whisper checkpoints: <|endoftext|>, <|startoftranscript|>, the language and
    task tokens, <|nospeech|>, <|notimestamps|> - NOT the <|0.00|>... timestamp tokens, which are added but not special).
    The reference strips exactly this list before stitching windows (wis/audio.py:141-146)."""
    import json
    with open(path, "r", encoding="utf-8") as f:
        tj = json.load(f)
    return sorted({int(t["id"]) for t in tj.get("added_tokens", []) if t.get("special")})


# ---- words (openai-whisper tokenizer.split_to_word_tokens + timing.merge_punctuations, restated) ---------------------------------------
NO_SPACE_LANGUAGES = ("zh", "ja", "th", "lo", "my", "yue")
PREPEND_PUNCTUATIONS = "\"'“¿([{-"
APPEND_PUNCTUATIONS = "\"'.。,，!！?？:：”)]}、"
_PUNCTUATION = "!\"#$%&'()*+,-./:;<=>?@[\\]^_`{|}~"      # string.punctuation


def split_tokens_on_unicode(tokens, decode):
    """Pieces that decode to whole unicode characters: a token that ends inside a multi-byte character (the decoder shows U+FFFD
    where the full text has none) is held back until the character is complete."""
    full, rep = decode(tokens), "\ufffd"
    words, word_tokens, cur, off = [], [], [], 0
    for t in tokens:
        cur.append(int(t))
        dec = decode(cur)
        if rep not in dec or full[off + dec.index(rep)] == rep:
            words.append(dec)
            word_tokens.append(cur)
            cur = []
            off += len(dec)
    return words, word_tokens


def split_tokens_on_spaces(tokens, decode, eot):
    subwords, subword_tokens = split_tokens_on_unicode(tokens, decode)
    words, word_tokens = [], []
    for sw, st in zip(subwords, subword_tokens):
        if st[0] >= eot or sw.startswith(" ") or sw.strip() in _PUNCTUATION or not words:
            words.append(sw)
            word_tokens.append(list(st))
        else:
            words[-1] += sw
            word_tokens[-1].extend(st)
    return words, word_tokens


def split_to_word_tokens(tokens, decode, language, eot):
    """one word per unicode piece for the languages written without spaces, else pieces merged up to the next leading space"""
    if language in NO_SPACE_LANGUAGES:
        return split_tokens_on_unicode(tokens, decode)
    return split_tokens_on_spaces(tokens, decode, eot)


def merge_punctuations(words, word_tokens, prepended=PREPEND_PUNCTUATIONS, appended=APPEND_PUNCTUATIONS):
    """opening punctuation joins the word after it, closing punctuation the word before it; returns the non-empty words"""
    words, word_tokens = list(words), [list(t) for t in word_tokens]
    i, j = len(words) - 2, len(words) - 1
    while i >= 0:
        if words[i].startswith(" ") and words[i].strip() in prepended:
            words[j], word_tokens[j] = words[i] + words[j], word_tokens[i] + word_tokens[j]
            words[i], word_tokens[i] = "", []
        else:
            j = i
        i -= 1
    i, j = 0, 1
    while j < len(words):
        if not words[i].endswith(" ") and words[j] in appended:
            words[i], word_tokens[i] = words[i] + words[j], word_tokens[i] + word_tokens[j]
            words[j], word_tokens[j] = "", []
        else:
            i = j
        j += 1
    keep = [k for k in range(len(words)) if word_tokens[k]]
    return [words[k] for k in keep], [word_tokens[k] for k in keep]


def words_from_alignment(segments, alignment, probs, tokenizer, language, special, duration):
    """`words` of every segment ({"tokens": text tokens} as segments_from_tokens(keep_tokens=True) leaves them) from ONE alignment of the
    window's text tokens: a word starts at the jump time of its first token and ends at the jump time of the next word's first token
    (find_alignment: time_index / 50 at the path rows where text_index advances; the row after the last token is eot's);
    its probability is the mean of its tokens'."""
    jumps, last = [], -1
    for ti, fi in alignment:
        if ti != last:
            jumps.append(min(fi * TIME_PRECISION, duration))
            last = ti
    n_text = sum(len(sg["tokens"]) for sg in segments)
    if len(jumps) != n_text + 1:
        raise RuntimeError(f"alignment covers {len(jumps)} rows, the text has {n_text} tokens + eot")
    o = 0
    for sg in segments:
        words, word_tokens = merge_punctuations(*split_to_word_tokens(sg["tokens"], tokenizer.decode, language, special.eot))
        sg["words"] = []
        for w, toks in zip(words, word_tokens):
            sg["words"].append({"word": w, "start": round(jumps[o], 2), "end": round(jumps[o + len(toks)], 2),
                                "probability": float(np.mean(probs[o:o + len(toks)]))})
            o += len(toks)
    return segments


class _Tokenizer:
    # id-only form (no tokenizer files, synthetic weights): every id from <|endoftext|> up is treated as special
    all_special_ids = SPECIAL_IDS

    def __init__(self, path=None, special_ids=None):
        self._tok = None
        if special_ids is not None:         # id-only form of another vocabulary (large-v3: up to 51865)
            self.all_special_ids = list(special_ids)
        if path and os.path.exists(os.path.join(path, "tokenizer.json")):
            from tokenizers import Tokenizer
            self._tok = Tokenizer.from_file(os.path.join(path, "tokenizer.json"))
            ids = special_ids_from_tokenizer_json(os.path.join(path, "tokenizer.json"))
            if ids:                     # the checkpoint's own list, as `WhisperProcessor.tokenizer.all_special_ids` (wis/audio.py:141)
                self.all_special_ids = ids

    @property
    def has_vocabulary(self):
        return self._tok is not None

    def decode(self, ids):
        """`WhisperProcessor.decode(tokens)` (main.py:714): the ids generate returns carry no special tokens besides what the
        model emitted itself; they are kept (skip_special_tokens defaults to False there too)."""
        ids = [int(t) for t in ids]
        if self._tok is not None:
            return self._tok.decode(ids, skip_special_tokens=False)
        return " ".join(str(t) for t in ids)

    def encode(self, text):
        """text -> token ids, no special tokens added (a prompt's text); needs the checkpoint's vocabulary"""
        if self._tok is None:
            raise ValueError("a text prompt needs the checkpoint's tokenizer vocabulary (tokenizer.json next to the model); pass token ids instead")
        return [int(t) for t in self._tok.encode(text, add_special_tokens=False).ids]

    @staticmethod
    def language_token_id(code):
        return W.LANG_IDS[LANGUAGE_CODES.index(code)]


class WhisperModels:
    """Lazy per-size registry (reference `LazyModels`, main.py:319-448): a model is built on first use; preload_* /
    warm-up mirror load_models / warm_models (main.py:451-511)."""

    def __init__(self, settings=None, device_index=None):
        self.settings = settings or get_api_settings()
        self._models, self._lock = {}, threading.Lock()
        n = ctranslate2._lib.device_count()
        self.device_index = list(range(n)) if device_index is None else list(device_index)
        self.tokenizer = _Tokenizer(None)      # id-only tokenizer (synthetic weights); real checkpoints get their own below
        self.tokenizers = {}

    def path_for(self, size):
        return self.settings.whisper_model_path.format(size=size)

    def get(self, size):
        if size not in MODEL_SIZES and size not in V3_MODEL_SIZES:
            raise ValueError(f"unknown model {size!r}")
        with self._lock:
            if size not in self._models:
                path = self.path_for(size)
                synthetic = path.startswith("synthetic:")
                if not synthetic:
                    if not os.path.isdir(path):
                        raise FileNotFoundError(
                            f"Whisper model directory {path!r} not found (setting whisper_model_path; the reference layout is "
                            "models/tovera-wis-whisper-<size>).  Seeded synthetic weights are only served when asked for explicitly: "
                            "whisper_model_path=synthetic:{size}")
                    tok = _Tokenizer(path)
                    if not tok.has_vocabulary and not self.settings.allow_token_id_text:
                        raise FileNotFoundError(f"{path}: no tokenizer.json - text output needs the checkpoint's tokenizer (the reference "
                                                "loads WhisperProcessor from the model dir, main.py:329-334); set allow_token_id_text=1 to serve "
                                                "token ids as text")
                    self.tokenizers[size] = tok
                max_beam = min(max(int(self.settings.max_beam), int(self.settings.beam_size), int(self.settings.long_beam_size)), ctranslate2.MAX_BEAM)
                self._models[size] = ctranslate2.models.Whisper(path, device="cuda", compute_type=self.settings.compute_type,
                                                                inter_threads=self.settings.ctranslate2_threads,
                                                                device_index=self.device_index, max_batch=self.settings.max_batch,
                                                                replicas_per_device=self.settings.replicas_per_gpu, max_beam=max_beam)
                st = model_special_tokens(self._models[size])
                if synthetic and st.n_vocab != W.N_VOCAB:
                    self.tokenizers[size] = _Tokenizer(None, special_ids=st.special_ids)
                import logging
                logging.getLogger("wis_hip").info("whisper %s loaded: beam_size 1..%d served (max_beam), device batches of up to %d utterances, %d replica(s)",
                                                  size, max_beam, self.settings.max_batch, len(self._models[size]._replicas))
            # (the batcher's pooled key for prompted requests is the model's to build: it reads the setting where it builds its keys)
            self._models[size].batch_ragged_prompts = bool(getattr(self.settings, "batch_ragged_prompts", False))
            return self._models[size]

    def tokenizer_for(self, size):
        return self.tokenizers.get(size, self.tokenizer)

    def preload(self):
        s = self.settings
        for size in MODEL_SIZES:
            if s.preload_all_models or getattr(s, f"preload_whisper_model_{size}"):
                self.get(size)
        for size in V3_MODEL_SIZES:          # (setting names spell the model's '-' as '_')
            if getattr(s, "preload_whisper_model_" + size.replace("-", "_"), False):
                self.get(size)

    def warm(self, clip):
        for _ in range(3):
            for size in list(self._models):
                do_whisper(clip, size, self.settings.beam_size, "transcribe", False, "en", models=self)


_default_models = None


def default_models():
    global _default_models
    if _default_models is None:
        _default_models = WhisperModels()
    return _default_models


class InvalidAudio(ValueError):
    """The container could not be decoded (the REST layer answers HTTP 400 "Invalid audio", main.py:1311-1314)."""


def check_language(language, special=None):
    """`language` names a language token of the model (special: its SpecialTokens; default the 99 of the 51865-token vocabulary)."""
    return language in (LANGUAGES if special is None else special.lang_codes)


def check_model_language(language, size):
    """`language` is one of model `size`'s languages, known before the model is loaded (yue: large-v3 / large-v3-turbo only)."""
    return language in (LANGUAGE_CODES_V3 if size in V3_MODEL_SIZES else LANGUAGES)


def chunkit(lst, num):
    for i in range(0, len(lst), num):
        yield lst[i:i + num]


def compression_ratio(text):
    """openai-whisper's: bytes of the text over bytes of its zlib image (a looping transcript compresses well: > 2.4 is its retry mark)."""
    import zlib
    raw = text.encode("utf-8")
    return len(raw) / len(zlib.compress(raw)) if raw else 0.0


def parse_temperatures(temperatures, best_of):
    """-> (tuple of temperatures, best_of), validated: finite values >= 0, best_of 1 .. the engine's rows per utterance.  ValueError otherwise."""
    try:
        ts = tuple(float(t) for t in (temperatures.split(",") if isinstance(temperatures, str) else (temperatures or ())) if str(t).strip() != "")
        n = int(best_of)
        if n != float(best_of):
            raise ValueError
    except (TypeError, ValueError, OverflowError):
        raise ValueError(f"temperatures {temperatures!r} / best_of {best_of!r}: a list of numbers and an integer") from None
    if any(not (0 <= t < float("inf")) for t in ts):
        raise ValueError(f"temperatures {temperatures!r}: finite values >= 0")
    if not 1 <= n <= ctranslate2.MAX_BEAM:
        raise ValueError(f"best_of {best_of!r} outside 1..{ctranslate2.MAX_BEAM}")
    return ts, n


def decode_with_fallback(decode, temperatures, best_of=5, compression_ratio_threshold=None, logprob_threshold=None, text_of=None):
    """openai-whisper's decode_with_fallback as a pure host function.  decode(temperature, n) -> [(tokens, score), ...]: the ordinary search at
    temperature 0 (n = 1), n samples at a later one; `score` is the engine's (cumulative log-probability, the end token's included, over the
    token count), so the average log-probability is score * len / (len + 1) as openai-whisper counts it.  Of a temperature's candidates the one
    with the best average log-probability is kept (the first among equals).  It needs a retry when its text's zlib compression ratio is above
    `compression_ratio_threshold` (only with `text_of`, tokens -> text: without a tokenizer vocabulary there is no text to compress) or its average
    log-probability is below `logprob_threshold`; None switches a test off.  The first acceptable result ends the schedule; the last one stands.
    -> dict(tokens, score, avg_logprob, compression_ratio (None without text_of), temperature, attempts)"""
    out = None
    for i, t in enumerate(temperatures):
        cands = decode(t, 1 if t == 0 else best_of)
        best = None
        for tokens, score in cands:
            avg = score * len(tokens) / (len(tokens) + 1)
            if best is None or avg > best[2]:
                best = (list(tokens), score, avg)
        ratio = compression_ratio(text_of(best[0])) if text_of is not None else None
        out = dict(tokens=best[0], score=best[1], avg_logprob=best[2], compression_ratio=ratio, temperature=t, attempts=i + 1)
        retry = (compression_ratio_threshold is not None and ratio is not None and ratio > compression_ratio_threshold) or \
                (logprob_threshold is not None and not best[2] >= logprob_threshold)
        if not retry:
            break
    return out


MAX_PREFIX_TOKENS = 64      # a decoder prefix is a few words, never half the context


def prompt_ids(value, tokenizer, special, what):
    """`initial_prompt` / `prefix` of do_whisper -> text token ids.  A string is encoded as " " + text.strip() with the checkpoint's tokenizer
    (openai-whisper's convention; no vocabulary: ValueError), a list of ids is taken as it is (text ids, below <|endoftext|>).  None / empty: []."""
    if value is None or (isinstance(value, (str, list, tuple)) and len(value) == 0):
        return []
    if isinstance(value, str):
        if not value.strip():
            return []
        if not getattr(tokenizer, "has_vocabulary", False):
            raise ValueError(f"{what}: a text prompt needs the checkpoint's tokenizer vocabulary (tokenizer.json next to the model); pass token ids instead")
        return tokenizer.encode(" " + value.strip())
    try:
        ids = [int(t) for t in value]
        if any(isinstance(t, (bool, float)) for t in value):
            raise TypeError
    except (TypeError, ValueError):
        raise ValueError(f"{what}: a string or a list of token ids") from None
    if any(not 0 <= t < special.eot for t in ids):
        raise ValueError(f"{what}: token ids must be text tokens (0 .. {special.eot - 1})")
    return ids


MAX_PHRASES = 20000      # entries of a request's phrase list (the engine's own limit is 65535 trie records)


def load_phrases_file(path):
    """The setting `phrases_file`: one phrase per line (blank lines and lines that start with # are skipped).  Empty path: no list.  A file that
    cannot be read raises (OSError): the server's start fails, not every request."""
    if not path:
        return []
    key = (path, os.stat(path).st_mtime_ns)      # (read once per version of the file, not once per request)
    if _phrases_file_cache.get("key") != key:
        with open(path, "r", encoding="utf-8") as f:
            _phrases_file_cache.update(key=key, phrases=[ln.strip() for ln in f if ln.strip() and not ln.lstrip().startswith("#")])
    return list(_phrases_file_cache["phrases"])


_phrases_file_cache = {}


def phrase_ids(phrases, tokenizer, special):
    """do_whisper's `phrases` -> ([token ids per phrase], {ids tuple: the caller's text for it}).  An entry is a string - encoded as
    " " + text.strip() with the checkpoint's tokenizer, like a prompt (no vocabulary: ValueError) - or a list of text token ids."""
    if isinstance(phrases, (str, bytes)) or not hasattr(phrases, "__iter__"):
        raise ValueError("phrases: a list of strings or token id lists")
    phrases = list(phrases)
    if not 1 <= len(phrases) <= MAX_PHRASES:
        raise ValueError(f"phrases: {len(phrases)} entries (1..{MAX_PHRASES})")
    out, names = [], {}
    for i, ph in enumerate(phrases):
        ids = prompt_ids(ph, tokenizer, special, f"phrases[{i}]")
        if not ids:
            raise ValueError(f"phrases[{i}]: an empty phrase")
        out.append(ids)
        if isinstance(ph, str):
            names.setdefault(tuple(ids), ph.strip())
    return out, names


def load_hotwords_file(path):
    """The setting `hotwords_file`: one entry per line, by `phrases_file`'s rules (blank lines and # lines skipped; empty path: no list; an
    unreadable file raises: the server's start fails, not every request)."""
    if not path:
        return []
    key = (path, os.stat(path).st_mtime_ns)
    if _hotwords_file_cache.get("key") != key:
        with open(path, "r", encoding="utf-8") as f:
            _hotwords_file_cache.update(key=key, hotwords=[ln.strip() for ln in f if ln.strip() and not ln.lstrip().startswith("#")])
    return list(_hotwords_file_cache["hotwords"])


_hotwords_file_cache = {}


def hotword_ids(hotwords, tokenizer, special):
    """do_whisper's `hotwords` -> [token ids per entry]: strings are encoded as `phrase_ids` encodes them (" " + text.strip() with the checkpoint's
    tokenizer; no vocabulary: ValueError), lists of text token ids pass as they are."""
    if isinstance(hotwords, (str, bytes)) or not hasattr(hotwords, "__iter__"):
        raise ValueError("hotwords: a list of strings or token id lists")
    hotwords = list(hotwords)
    if not 1 <= len(hotwords) <= MAX_PHRASES:
        raise ValueError(f"hotwords: {len(hotwords)} entries (1..{MAX_PHRASES})")
    out = []
    for i, hw in enumerate(hotwords):
        ids = prompt_ids(hw, tokenizer, special, f"hotwords[{i}]")
        if not ids:
            raise ValueError(f"hotwords[{i}]: an empty entry")
        out.append(ids)
    return out


def _hotword_opts(settings, hotwords, hotword_boost):
    """do_whisper's hotwords / hotword_boost, resolved against the settings -> (the list, the boost) or (None, 0.0) when the option is off.
    hotwords None: the setting's list (`hotwords_file`); empty: off.  hotword_boost None: the setting (`hotword_boost`, default 0.0 = off).
    The settings' list with a boost of 0 is off; a list the REQUEST names needs a boost from somewhere (ValueError); a boost is finite and > 0."""
    explicit = hotwords is not None
    if explicit and (isinstance(hotwords, (str, bytes)) or not hasattr(hotwords, "__iter__")):
        raise ValueError("hotwords: a list of strings or token id lists")
    lst = list(hotwords) if explicit else load_hotwords_file(getattr(settings, "hotwords_file", ""))
    boost = getattr(settings, "hotword_boost", 0.0) if hotword_boost is None else hotword_boost
    try:
        boost = float(0.0 if boost is None else boost)
    except (TypeError, ValueError):
        raise ValueError(f"hotword_boost {hotword_boost!r}: a finite number > 0") from None
    if hotword_boost is not None and not (math.isfinite(boost) and boost > 0):
        raise ValueError(f"hotword_boost {hotword_boost!r}: a finite number > 0")
    if not lst:
        return None, 0.0
    if boost == 0.0:
        if explicit:
            raise ValueError("hotwords need a hotword_boost (the request's, or the setting): there is no default boost")
        return None, 0.0
    if not (math.isfinite(boost) and boost > 0):
        raise ValueError(f"hotword_boost {boost!r}: a finite number > 0")
    return lst, boost


def in_grammar(logmass, n_tokens):
    """exp(logmass / (n_tokens + 1)): the geometric mean, per step, of the share of the model's probability a phrase list allowed along a phrase of
    n_tokens tokens and its <|endoftext|>; in [0, 1] (-inf -> 0; NaN stays NaN)."""
    return float(math.exp(float(logmass) / (int(n_tokens) + 1)))


def _phrase_mass_opts(opt, constrained, phrase_mass, phrase_threshold, phrase_fallback):
    """do_whisper's phrase_mass / phrase_threshold / phrase_fallback, resolved against the settings -> (mass on, threshold or 0.0, fallback on)."""
    if not constrained:
        for v, name in ((phrase_mass, "phrase_mass"), (phrase_threshold, "phrase_threshold"), (phrase_fallback, "phrase_fallback")):
            if v:
                raise ValueError(f"{name} needs phrases")
        return False, 0.0, False
    thr = opt(phrase_threshold, "phrase_threshold", 0.0)
    try:
        thr = float(0.0 if thr is None else thr)
    except (TypeError, ValueError):
        raise ValueError(f"phrase_threshold {phrase_threshold!r}: a number in [0, 1]") from None
    if not 0.0 <= thr <= 1.0:      # (a NaN fails both comparisons)
        raise ValueError(f"phrase_threshold {thr!r}: a number in [0, 1] (0: no threshold)")
    fb = bool(opt(phrase_fallback, "phrase_fallback", False))
    if fb and thr == 0.0:
        raise ValueError("phrase_fallback needs a phrase_threshold in (0, 1]")
    return bool(opt(phrase_mass, "phrase_mass", False)) or thr > 0.0, thr, fb


def assemble_prompt(start, special, initial_prompt_ids=(), prefix_ids=(), n_text_ctx=448):
    """openai-whisper's decoder prompt: [<|startofprev|>] + initial_prompt_ids[-(n_ctx / 2 - 1):] + start sequence + prefix_ids.  The engine takes
    n_ctx / 2 + 4 tokens (228): with a prefix the prompt part is cut further from the left.  A prefix of more than MAX_PREFIX_TOKENS is a ValueError."""
    prefix_ids, initial_prompt_ids = list(prefix_ids), list(initial_prompt_ids)
    if len(prefix_ids) > MAX_PREFIX_TOKENS:
        raise ValueError(f"prefix: {len(prefix_ids)} tokens (at most {MAX_PREFIX_TOKENS})")
    if not initial_prompt_ids:
        return list(start) + prefix_ids
    keep = min(n_text_ctx // 2 - 1, n_text_ctx // 2 + 4 - 1 - len(start) - len(prefix_ids))
    return [special.startofprev] + initial_prompt_ids[-keep:] + list(start) + prefix_ids


def _threshold(value, sign=1):
    """A threshold of the temperature fallback / the seek loop as they take it: None when it is off (None, or >= 1e30; sign -1: <= -1e30)."""
    return None if value is None or sign * value >= 1e30 else value


def _n_text_ctx(whisper_model):
    return int((getattr(whisper_model, "arch", None) or {}).get("n_text_ctx", 448))


def _request_prompt_ids(q, tokenizer, special, seek=False):
    """(initial_prompt ids, prefix ids) of a request, and its two refusals.  seek: the loop always decodes under the timestamp rules."""
    ip_ids = prompt_ids(q.initial_prompt, tokenizer, special, "initial_prompt")
    px_ids = prompt_ids(q.prefix, tokenizer, special, "prefix")
    if px_ids and (q.timestamps or seek):
        # text behind the start sequence makes the prompt a plain-search prompt for the engine (ctranslate2.timestamp_prompt): its timestamp rules
        # read the GENERATED history, which a prefix is not part of - refused rather than decoded without the rules
        raise ValueError("prefix cannot be combined with timestamps / word_timestamps (initial_prompt can)"
                         + (", and long_form=seek always decodes with timestamps" if seek else ""))
    if q.word_timestamps and not getattr(tokenizer, "has_vocabulary", False):
        raise ValueError("word_timestamps need the checkpoint's tokenizer vocabulary (tokenizer.json next to the model)")
    return ip_ids, px_ids


def _request_hotwords(q, tokenizer, special):
    """generate's hotword arguments of a request ({}: the option is off) - handed to every decode of the request"""
    if q.hotwords is None:
        return {}
    return dict(hotwords=hotword_ids(q.hotwords, tokenizer, special), hotword_boost=q.hotword_boost)


def _request_language(q, settings, special, detect):
    """The request's language: detected (detect() -> detect_language's result for the first window), forced, or the setting; one of the model's."""
    language = settings.language
    if q.detect_language and not q.force_language:
        lang_token, _probability = detect()[0][0]
        language = lang_token.strip("<|>")
    elif q.force_language:
        language = q.force_language
    if not check_language(language, special):
        raise ValueError(f"unsupported language {language!r}")
    return language


def _search(q, t, n):
    """generate's search arguments at temperature t of the fallback: the search at the request's beam size at 0, n samples at beam 1 otherwise."""
    return dict(beam_size=q.beam_size) if t == 0 else dict(beam_size=1, num_hypotheses=n, sampling_topk=0, sampling_temperature=t)


def _text_of(tokenizer, below):
    """tokens -> the text whose compression ratio the fallback judges (ids from `below` up dropped); None without a vocabulary: no text to
    compress, the log-probability threshold alone decides."""
    if not getattr(tokenizer, "has_vocabulary", False):
        return None
    return lambda toks: tokenizer.decode([t for t in toks if t < below])


def do_whisper(audio_file, model, beam_size=None, task="transcribe", detect_language=False, force_language=None, translate=False,
               models=None, fixed_new_tokens=None, timestamps=False, word_timestamps=False, repetition_penalty=None, no_repeat_ngram_size=None,
               temperatures=None, best_of=None, compression_ratio_threshold=None, logprob_threshold=None, initial_prompt=None, prefix=None,
               long_form=None, condition_on_previous_text=None, no_speech_threshold=None, phrases=None, phrase_nbest=1,
               phrase_mass=None, phrase_threshold=None, phrase_fallback=None, hotwords=None, hotword_boost=None):
    """hotwords / hotword_boost (None: the settings' list, `hotwords_file`, and `hotword_boost`, 0.0 = off; an empty list: off): contextual biasing
    toward a list of entries - strings (tokenised as " " + text.strip() with the checkpoint's tokenizer; no vocabulary: ValueError) or lists of
    text token ids.  Free-form decoding goes on; every token that starts an entry, or continues one the hypothesis has begun, gets the boost added
    to its logit (include/wis_hip.h, THE HOTWORD RULE; no back-off; scores are those of the boosted rows).  The option reaches every decode of the
    request - the translation pass, every temperature of the fallback, every window of long_form=seek and of the chunked form - but not language
    detection or the word alignment.  There is no default boost: calibrate it on the checkpoint in use; a list named by the request without any
    boost, a boost that is not finite and > 0, and a request that names hotwords together with phrases are a ValueError; the settings' list
    does not apply to a constrained request.
    phrases (None: the setting's list, `phrases_file`; empty: off): the transcript is restricted to a phrase list - strings (tokenised as
    " " + text.strip() with the checkpoint's tokenizer; no vocabulary: ValueError) or lists of text token ids.  The search can only produce
    one of the phrases (include/wis_hip.h states the rule); `text` is the best one, and the result gains
    `matches = [{"text", "score"}]`, best first: the `phrase_nbest` best phrases of the beam search (at most beam_size; fewer when the search
    reached fewer) with the engine's length-normalised log-probability, renormalised over what the list allows at each step.  initial_prompt and
    the repetition options combine with it; prefix, timestamps, word_timestamps, temperatures, long_form=seek and a recording over 30 s are a
    ValueError.  Language detection is unaffected; the translation pass stays unconstrained, as it stays unprompted.
    phrase_mass / phrase_threshold / phrase_fallback (None: the settings of those names - off, 0 = no threshold, off; they act on constrained
    requests only, and an explicit one without phrases is a ValueError): the out-of-grammar signal.  With phrase_mass every entry of `matches` gains
    `logmass` - the log of the share of the model's probability the list allowed, summed over the phrase's tokens and its <|endoftext|>
    (include/wis_hip.h, THE PHRASE MASS RULE: what an unconstrained decode would have been compared for) - and
    `in_grammar = exp(logmass / (tokens + 1))`, the geometric-mean share per step in [0, 1], comparable across phrase lengths.  A phrase_threshold
    in (0, 1] implies phrase_mass and the result gains `matched`: in_grammar of the best match >= threshold (outside [0, 1]: ValueError).  There is
    no default threshold: a useful one has to be calibrated on the deployment's checkpoint and phrase list.  phrase_fallback (needs a threshold:
    ValueError): when the best phrase is not matched, the same window is decoded once more without the phrase options - through the encoder view
    when `encode_once` is on - and `text` is that transcript; `matches` stay.
    long_form ("chunk" | "seek"; None: the setting, "chunk"): how a recording over 30 s is served.  "chunk": the reference's fixed windows merged by
    longest common sequence - no timestamps, no fallback (ValueError).  "seek": openai-whisper's transcribe() loop (wis_hip.longform) over one
    whole-recording log-mel kept on one of the model's GPUs (audio.LongMel) - timestamps, word_timestamps, the temperature fallback, initial_prompt
    and the repetition options all apply per window; condition_on_previous_text (None: the setting, True) and no_speech_threshold (None: the setting,
    0.6; >= 1e30: never skip) are the loop's.  Every word of word_timestamps lies inside its segment (held at the segment's bounds where the
    alignment puts it outside).  translate=True runs the loop a second time with the translate task: unprompted, one search per window, the
    repetition options and the skip rule applied; it carries no segments.  Recordings of up to 30 s are not affected by the option.  The result's `.seek` then holds the loop's
    per-window record.
    initial_prompt / prefix: openai-whisper's options of those names, each a string or a list of token ids (None: the settings' values; empty:
    off).  The decoder prompt becomes [<|startofprev|>] + prompt ids + start sequence + prefix ids (assemble_prompt; the prompt is cut from the left
    to what the engine takes, 228 tokens in all).  Every window of a long recording gets the same prompt; language detection, the translation pass and
    the word alignment stay unprompted; the repetition options and the temperature fallback combine with both options, timestamps / word_timestamps
    with initial_prompt only: together with a prefix they are a ValueError (the engine's timestamp rules read the generated history, which a prefix
    is not part of).  `text` is what the engine GENERATED: the prefix is not repeated in it.
    temperatures / best_of / compression_ratio_threshold / logprob_threshold: openai-whisper's temperature fallback (decode_with_fallback; None:
    the settings' values, and the settings' default - no temperatures - is no fallback).  The first temperature's decode is judged, and while it
    loops or scores badly the window is decoded again at the next: 0 is the search at `beam_size`, anything else `generate(beam_size=1,
    num_hypotheses=best_of, sampling_topk=0, sampling_temperature=t)`.  The compression ratio needs the decoded TEXT, so it needs the
    checkpoint's tokenizer vocabulary: without one only the log-probability threshold applies.  One 30 s window (longer audio: ValueError).
    repetition_penalty / no_repeat_ngram_size: CTranslate2's options of those names (None: the settings' values, 1.0 and 0 = off), handed
    to every `generate` call of the request - chunked windows, the timestamped pass, the translation pass.
    word_timestamps=True implies timestamps=True: after the search the window's text tokens are aligned with the audio in one
    `Whisper.align` call (cross-attention of the alignment heads + DTW on the GPU) and every segment gains
    `words: [{word, start, end, probability}]`, grouped as openai-whisper's split_to_word_tokens + merge_punctuations group them.
    Out of scope: the pause / median-duration heuristics of openai-whisper's add_word_timestamps, audio over 30 s, and `translate`
    (the translation pass carries no words).  A model without a tokenizer vocabulary raises ValueError."""
    models = models or default_models()
    s = models.settings
    opt = lambda value, name, default: getattr(s, name, default) if value is None else value      # None means the setting
    temps, best_of = parse_temperatures(opt(temperatures, "temperatures", ()), opt(best_of, "best_of", 5))
    q = SimpleNamespace(      # the request, resolved once: what the 30 s path and _do_whisper_seek both read
        task=task, detect_language=detect_language, force_language=force_language, translate=translate, timestamps=timestamps or word_timestamps, word_timestamps=word_timestamps,
        beam_size=s.beam_size if beam_size is None else beam_size, fixed_new_tokens=s.fixed_new_tokens if fixed_new_tokens is None else fixed_new_tokens,
        rep=dict(repetition_penalty=opt(repetition_penalty, "repetition_penalty", 1.0), no_repeat_ngram_size=opt(no_repeat_ngram_size, "no_repeat_ngram_size", 0)),
        temps=temps, best_of=best_of,
        compression_ratio_threshold=_threshold(opt(compression_ratio_threshold, "compression_ratio_threshold", 2.4)),
        logprob_threshold=_threshold(opt(logprob_threshold, "logprob_threshold", -1.0), -1),
        long_form=opt(long_form, "long_form", "chunk"), condition_on_previous_text=bool(opt(condition_on_previous_text, "condition_on_previous_text", True)),
        no_speech_threshold=_threshold(opt(no_speech_threshold, "no_speech_threshold", 0.6)),
        initial_prompt=opt(initial_prompt, "initial_prompt", ""), prefix=opt(prefix, "prefix", ""),
        phrases=load_phrases_file(getattr(s, "phrases_file", "")) if phrases is None else phrases, phrase_nbest=phrase_nbest)
    constrained = not (q.phrases is None or (hasattr(q.phrases, "__len__") and len(q.phrases) == 0))
    q.phrase_mass, q.phrase_threshold, q.phrase_fallback = _phrase_mass_opts(opt, constrained, phrase_mass, phrase_threshold, phrase_fallback)
    q.hotwords, q.hotword_boost = _hotword_opts(s, hotwords, hotword_boost)
    if constrained and q.hotwords is not None:
        if hotwords is not None:      # (the request itself names both)
            raise ValueError("hotwords cannot be combined with phrases (a constrained search has nothing left to bias)")
        q.hotwords, q.hotword_boost = None, 0.0      # the SETTINGS' hotword list does not apply to a constrained request
    if constrained:
        try:
            q.phrase_nbest = int(phrase_nbest)
            if q.phrase_nbest != float(phrase_nbest) or q.phrase_nbest < 1:
                raise ValueError
        except (TypeError, ValueError, OverflowError):
            raise ValueError(f"phrase_nbest {phrase_nbest!r}: an integer >= 1") from None
        for on, what in ((q.prefix, "prefix"), (q.timestamps, "timestamps / word_timestamps"), (temps, "temperatures"), (q.long_form == "seek", "long_form=seek"),
                         (q.fixed_new_tokens, "fixed_new_tokens")):
            if on:
                raise ValueError(f"phrases cannot be combined with {what}")
    if q.long_form not in ("chunk", "seek"):
        raise ValueError(f"long_form {q.long_form!r}: seek or chunk")
    timestamps, rep, fixed_new_tokens = q.timestamps, q.rep, q.fixed_new_tokens
    whisper_model = models.get(model)
    special = model_special_tokens(whisper_model)
    first_time_start = time.perf_counter()

    # STEP 1 — load audio and extract features
    if isinstance(audio_file, np.ndarray):
        pcm, sr = audio_file.astype(np.float32), 16000
    else:
        # a container at another rate is resampled on one of the model's own GPUs (never on a device the server was not configured to use)
        rs_dev = whisper_model._replicas[0].device if getattr(s, "resample_on_gpu", False) and getattr(whisper_model, "_replicas", None) else None
        try:
            pcm, sr = audio.load_audio(audio_file, device=rs_dev)
        except Exception as e:
            raise InvalidAudio(str(e)) from e
    if pcm.shape[0] == 0:
        raise InvalidAudio("empty audio")
    audio_duration = int(pcm.shape[0] / sr * 1000)
    if audio_duration >= s.long_beam_size_threshold:
        q.beam_size = s.long_beam_size
    if q.long_form == "seek" and audio_duration > 30 * 1000:
        return _do_whisper_seek(q, models, model, whisper_model, pcm, audio_duration, first_time_start)
    if timestamps and audio_duration > 30 * 1000:
        raise ValueError("timestamps are available for audio of up to 30 s (one window)")
    if constrained and audio_duration > 30 * 1000:
        raise ValueError("phrases are available for audio of up to 30 s (one window)")
    if temps and audio_duration > 30 * 1000:
        raise ValueError("the temperature fallback is available for audio of up to 30 s (one window)")
    use_chunking = audio_duration > 30 * 1000 and s.support_chunking
    strides = []
    if use_chunking:
        windows = []
        for chunk, stride in audio.chunk_iter(pcm):
            windows.append(audio.pad_or_trim(chunk))
            strides.append(stride)
        windows = np.stack(windows)
    else:
        windows = audio.pad_or_trim(pcm)[None]
    if s.fuse_logmel:
        # the 30 s PCM windows go to the replica as they are: log-mel runs on THAT replica's GPU inside generate and the
        # features never leave HBM (WIS_IN_PCM_HOST) - same kernels, same results as the two-step form below
        features, kind = np.ascontiguousarray(windows, np.float32), ctranslate2._lib.WIS_IN_PCM_HOST
    else:
        # the reference's two-step form (main.py:606-614, 685): features to the host, then StorageView.from_array
        # (on one of the model's own GPUs - never on a device the server was not configured to use)
        dev = whisper_model._replicas[0].device if getattr(whisper_model, "_replicas", None) else None
        features, kind = audio.log_mel_spectrogram(windows, n_mels=getattr(whisper_model, "n_mels", audio.N_MELS), device=dev).numpy(), ctranslate2._lib.WIS_IN_MEL_HOST
    total_chunk_count = features.shape[0]
    tokenizer = models.tokenizer_for(model)
    ip_ids, px_ids = _request_prompt_ids(q, tokenizer, special)
    hot = _request_hotwords(q, tokenizer, special)
    phr = {}
    if constrained:
        if q.phrase_nbest > q.beam_size:
            raise ValueError(f"phrase_nbest {q.phrase_nbest}: a search at beam_size {q.beam_size} returns at most {q.beam_size} phrases")
        phr_ids, phr_names = phrase_ids(q.phrases, tokenizer, special)
        phr = dict(phrases=phr_ids, num_hypotheses=q.phrase_nbest)
        if q.phrase_mass:
            phr["return_phrase_mass"] = True
    ccg = s.concurrent_gpu_chunks
    translating = translate and total_chunk_count <= ccg
    # encode_once: a request that reads a window more than once - language detection, the temperature fallback, the word alignment, the
    # translation pass - encodes its windows ONCE (Whisper.encode, in the groups the decode uses) and hands the views to every pass; a request that
    # reads its windows once is served as ever: no encode call, the same input kind, the same batch key
    reads = int(bool(q.detect_language and not q.force_language)) + max(1, len(temps)) + int(bool(word_timestamps)) + int(bool(translating)) + int(bool(q.phrase_fallback))
    views = None
    if getattr(s, "encode_once", False) and reads > 1:
        views = [whisper_model.encode(ctranslate2.StorageView.from_array(np.ascontiguousarray(batch)), input_kind=kind) for batch in chunkit(features, ccg)]

    def windows_of(lo, hi):
        """(what generate / detect_language / align take for windows lo .. hi - 1 (inside one decode group), their input_kind argument)"""
        if views is None:
            return ctranslate2.StorageView.from_array(np.ascontiguousarray(features[lo:hi])), dict(input_kind=kind)
        g = lo // ccg
        return views[g][lo - g * ccg:hi - g * ccg], {}

    # STEP 2 — language
    def detect():
        f, k = windows_of(0, 1)
        return whisper_model.detect_language(f, **k)
    language = _request_language(q, s, special, detect)
    task_id = special.translate if task == "translate" else special.transcribe
    start = [special.sot, special.language_token_id(language), task_id] + ([] if timestamps else [special.notimestamps])
    prompt = assemble_prompt(start, special, ip_ids, px_ids, _n_text_ctx(whisper_model))

    # STEP 3 — run the model, `concurrent_gpu_chunks` windows per generate call
    results = []
    if temps:      # one window, openai-whisper's decode_with_fallback around it
        feats, fkind = windows_of(0, 1)

        def decode(t, n):
            r = whisper_model.generate(feats, [prompt], return_scores=True, fixed_new_tokens=fixed_new_tokens, **fkind, **_search(q, t, n), **rep, **hot)[0]
            return list(zip(r.sequences_ids, r.scores))
        fb = decode_with_fallback(decode, temps, best_of, q.compression_ratio_threshold, q.logprob_threshold, _text_of(tokenizer, special.timestamp_begin))
        results.append(ctranslate2.WhisperGenerationResult([fb["tokens"]], [fb["score"]]))
        results[0].fallback = fb
    for lo in ([] if temps else range(0, total_chunk_count, ccg)):
        hi = min(lo + ccg, total_chunk_count)
        feats, fkind = windows_of(lo, hi)
        results.extend(whisper_model.generate(feats, [prompt] * (hi - lo), beam_size=q.beam_size, return_scores=False,
                                              fixed_new_tokens=fixed_new_tokens, **fkind, **rep, **phr, **hot))
    assert len(results) == total_chunk_count, "Result length doesn't match expected total_chunk_count"
    if use_chunking:
        tokens = audio.find_longest_common_sequence([(results[i].sequences_ids[0], strides[i]) for i in range(total_chunk_count)],
                                                    tokenizer)
        tokens = [int(t) for t in tokens]
    else:
        tokens = results[0].sequences_ids[0]
    matches = matched = None
    if constrained:      # the caller's own spelling of a phrase it gave as text, the decoded ids otherwise
        matches = [dict(text=phr_names.get(tuple(ids)) or tokenizer.decode(ids).strip(), score=float(sc))
                   for ids, sc in zip(results[0].sequences_ids, results[0].scores)]
        if q.phrase_mass:
            for mt, ids, lm in zip(matches, results[0].sequences_ids, results[0].phrase_logmass):
                mt["logmass"], mt["in_grammar"] = float(lm), in_grammar(lm, len(ids))
        if q.phrase_threshold > 0:
            matched = bool(matches) and bool(matches[0]["in_grammar"] >= q.phrase_threshold)      # (a NaN share is no match)
            if not matched and q.phrase_fallback:      # the same window once more, without the phrase options: the plain transcript
                feats, fkind = windows_of(0, 1)
                tokens = whisper_model.generate(feats, [prompt], beam_size=q.beam_size, return_scores=False, fixed_new_tokens=fixed_new_tokens,
                                                **fkind, **rep)[0].sequences_ids[0]
    segments = None
    if timestamps:
        duration = min(audio_duration / 1000.0, WINDOW_S)
        segments = segments_from_tokens(tokens, tokenizer, 0.0, duration, special, keep_tokens=word_timestamps)
        if word_timestamps:
            text_tokens = [t for sg in segments for t in sg["tokens"]]
            num_frames = max(2, min(3000, -(-pcm.shape[0] // audio.HOP_LENGTH)))
            feats, fkind = windows_of(0, 1)
            al = whisper_model.align(feats, start[:3], [text_tokens], [num_frames], **fkind)[0]
            words_from_alignment(segments, al.alignments, al.text_token_probs, tokenizer, language, special, duration)
            for sg in segments:
                del sg["tokens"]
        text = tokenizer.decode([t for t in tokens if t < special.timestamp_begin]).strip()
    else:
        text = tokenizer.decode(tokens).strip()

    translation = None
    if translating:       # main.py:729-748 (its `len(int)` bug aside: short audio only)
        tprompt = [special.sot, special.language_token_id(language), special.translate, special.notimestamps]
        feats, fkind = windows_of(0, total_chunk_count)
        tres = whisper_model.generate(feats, [tprompt] * total_chunk_count, beam_size=q.beam_size, fixed_new_tokens=fixed_new_tokens, **fkind, **rep, **hot)
        translation = tokenizer.decode(tres[0].sequences_ids[0]).strip()
        out_translation_tokens = tres[0].sequences_ids[0]
    else:
        out_translation_tokens = None

    infer_time_milliseconds = (time.perf_counter() - first_time_start) * 1000
    infer_speedup = math.floor(audio_duration / infer_time_milliseconds)
    out = WhisperResult((language, text, infer_time_milliseconds, translation, infer_speedup, audio_duration))
    out.tokens = tokens
    out.translation_tokens = out_translation_tokens
    out.segments = segments
    out.fallback = getattr(results[0], "fallback", None)      # temperature fallback: what the kept decode was (decode_with_fallback)
    out.matches = matches
    out.matched = matched
    return out


def _do_whisper_seek(q, models, model, whisper_model, pcm, audio_duration, first_time_start):
    """do_whisper for a recording over 30 s with long_form="seek" (q: the request as do_whisper resolved it): the whole-recording log-mel on one of
    the model's GPUs for the length of the request, longform.transcribe around generate_from_device / align_from_device."""
    from . import longform
    special = model_special_tokens(whisper_model)
    tokenizer = models.tokenizer_for(model)
    ip_ids, _ = _request_prompt_ids(q, tokenizer, special, seek=True)
    hot = _request_hotwords(q, tokenizer, special)
    n_text_ctx = _n_text_ctx(whisper_model)
    replica = whisper_model.acquire_replica()
    long_mel = None
    try:
        long_mel = audio.LongMel(pcm, n_mels=getattr(whisper_model, "n_mels", audio.N_MELS), device=replica.device)
        # encode_once: a window the transcription loop reads more than once (the fallback's temperatures, the word alignment) is encoded once
        # (Whisper.encode from the window's device features) and its decodes and the alignment read the view; language detection shares the
        # first window's view with the loop.  A loop that reads its windows once is served as ever
        once = bool(getattr(models.settings, "encode_once", False))
        detecting = bool(q.detect_language and not q.force_language)
        multi = once and (q.word_timestamps or len(q.temps) > 1)
        first = {}      # the view of the window at seek 0, while language detection and the loop's first window share it

        def encoded(window):
            return whisper_model.encode(window, input_kind=ctranslate2._lib.WIS_IN_MEL_DEV, device=replica.device)

        def encode(window, seek):
            if seek == 0 and first:
                return first.pop(0)
            return encoded(window) if multi else window

        def detect():
            if not once:
                return whisper_model.detect_language(ctranslate2.StorageView.from_array(np.ascontiguousarray(long_mel.window(0, to_host=True)[None])))
            first[0] = encoded(long_mel.window(0))
            return whisper_model.detect_language(first[0])
        language = _request_language(q, models.settings, special, detect)
        start = [special.sot, special.language_token_id(language), special.translate if q.task == "translate" else special.transcribe]

        def decode(window, prompt, t, n):
            if isinstance(window, ctranslate2.StorageView):
                r = whisper_model.generate(window, [prompt], fixed_new_tokens=q.fixed_new_tokens, return_scores=True, return_no_speech_prob=True,
                                           **_search(q, t, n), **q.rep, **hot)[0]
            else:
                r = whisper_model.generate_from_device(replica.device, window, prompt, replica=replica, fixed_new_tokens=q.fixed_new_tokens, return_scores=True,
                                                       return_no_speech_prob=True, **_search(q, t, n), **q.rep, **hot)
            return list(zip(r.sequences_ids, r.scores)), r.no_speech_prob

        def on_window(window, seek, segment_size, segs):
            text_tokens = [t for sg in segs for t in sg["tokens"] if t < special.eot]
            if not text_tokens:
                for sg in segs:
                    sg["words"] = []
                return
            if isinstance(window, ctranslate2.StorageView):
                al = whisper_model.align(window, start, [text_tokens], max(2, segment_size))[0]
            else:
                al = whisper_model.align_from_device(replica.device, window, start, [text_tokens], max(2, segment_size), replica=replica)[0]
            timed = [dict(tokens=[t for t in sg["tokens"] if t < special.eot]) for sg in segs]
            words_from_alignment(timed, al.alignments, al.text_token_probs, tokenizer, language, special, segment_size * longform.FRAME_S)
            off = round(seek * longform.FRAME_S, 2)
            # a word lies inside its segment: the alignment places a word by the cross-attention alone, the segment's bounds are the decoder's
            # timestamp tokens, and where the two disagree the word is held at the bound (openai-whisper moves the segment's bounds to its words
            # instead; here the segments stay what the timestamps said - monotone, inside the recording, the same with and without words)
            for sg, tm in zip(segs, timed):
                inside = lambda t: round(min(max(t + off, sg["start"]), sg["end"]), 2)
                sg["words"] = [dict(w, start=inside(w["start"]), end=inside(w["end"])) for w in tm["words"]]
        loop = dict(special=special, n_text_ctx=n_text_ctx, logprob_threshold=q.logprob_threshold, no_speech_threshold=q.no_speech_threshold,
                    condition_on_previous_text=q.condition_on_previous_text)
        res = longform.transcribe(long_mel, decode, start=start, initial_prompt_ids=ip_ids, temperatures=q.temps, best_of=q.best_of,
                                  compression_ratio_threshold=q.compression_ratio_threshold, text_of=_text_of(tokenizer, special.eot),
                                  on_window=on_window if q.word_timestamps else None, encode=encode if once and (multi or first) else None, **loop)
        first.clear()
        translation = translation_tokens = None
        if q.translate:
            # the translation pass: the same loop with the translate task - unprompted, one search per window (no fallback), the repetition
            # options applied as to every decode of the request, the same skip rule as the transcription; it carries no segments
            tres = longform.transcribe(long_mel, decode, start=start[:2] + [special.translate], **loop)
            translation_tokens = [t for sg in tres["segments"] for t in sg["tokens"] if t < special.eot]
            translation = tokenizer.decode(translation_tokens).strip()
    finally:
        if long_mel is not None:
            long_mel.close()
        whisper_model.release_replica(replica)
    tokens, segments = [], []
    for sg in res["segments"]:
        text_tokens = [t for t in sg["tokens"] if t < special.eot]
        tokens.extend(sg["tokens"])
        out_sg = {"start": sg["start"], "end": sg["end"], "text": tokenizer.decode(text_tokens).strip()}
        if q.word_timestamps:
            out_sg["words"] = sg.get("words", [])
        segments.append(out_sg)
    text = " ".join(sg["text"] for sg in segments if sg["text"]).strip()
    infer_time_milliseconds = (time.perf_counter() - first_time_start) * 1000
    out = WhisperResult((language, text, infer_time_milliseconds, translation, math.floor(audio_duration / infer_time_milliseconds), audio_duration))
    out.tokens = tokens
    out.translation_tokens = translation_tokens
    out.segments = segments if q.timestamps else None
    out.fallback = res["fallback"] if q.temps else None
    out.seek = res["windows"]
    return out
