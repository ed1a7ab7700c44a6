"""Call-compatible stand-in for the slice of `ctranslate2` the reference uses:

    ctranslate2.models.Whisper(path, device=, compute_type=, inter_threads=, device_index=[..] | intra_threads=)
    ctranslate2.StorageView.from_array(ndarray f32 [B, n_mels, 3000])   (n_mels 80, or 128 for large-v3 / large-v3-turbo)
    model.generate(features, [prompt] * B, beam_size=int, return_scores=False) -> results[i].sequences_ids[0]
    model.detect_language(features) -> [[("<|xx|>", prob), ...], ...]
    model.encode(features, to_cpu=False) -> StorageView of the encoder output, which generate / detect_language / align take in place of features
    ctranslate2.get_supported_compute_types(device)

(reference main.py:341-444, 454, 535-537, 638-639, 685-693, 707, 713).  The arithmetic runs in the
hand-written HIP kernels of libwis_hip.so; there is no CPU fallback and no dependency on CTranslate2.

`model_path` is either a CTranslate2 Whisper model directory (model.bin [+ config.json]) or the
string "synthetic:<size>[:seed]" for seeded synthetic weights at the true shapes (no checkpoint exists
offline).
"""
import ctypes as C
import os
import threading
import weakref
from typing import NamedTuple, Optional

import numpy as np

from . import _lib, weights as W
from .batching import MicroBatcher


# ---- random sampling: where the seed of an unseeded request comes from (CTranslate2 has ctranslate2.set_random_seed)
_seed_lock = threading.Lock()
_seed_state = None      # None: every unseeded request draws 64 bits from os.urandom; [seed, counter] after set_random_seed


def set_random_seed(seed):
    """ctranslate2.set_random_seed: from now on the requests that pass no `sampling_seed` draw theirs from a deterministic counter over `seed`
    (the n-th unseeded utterance after this call always gets the same seed).  None: back to os.urandom."""
    global _seed_state
    with _seed_lock:
        _seed_state = None if seed is None else [int(seed) & 0xFFFFFFFFFFFFFFFF, 0]


def _next_seed():
    with _seed_lock:
        if _seed_state is None:
            return int.from_bytes(os.urandom(8), "little")
        _seed_state[1] += 1
        z = (_seed_state[0] + 0x9E3779B97F4A7C15 * _seed_state[1]) & 0xFFFFFFFFFFFFFFFF      # splitmix64 of (seed, counter)
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & 0xFFFFFFFFFFFFFFFF
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & 0xFFFFFFFFFFFFFFFF
    return z ^ (z >> 31)


def get_supported_compute_types(device="cuda", device_index=0):
    buf = C.create_string_buffer(64)
    _lib.check(_lib.load().wis_supported_compute_types(device_index, buf, 64))
    return set(buf.value.decode().split(","))


class StorageView:
    """Zero-copy wrapper of a host ndarray (ctranslate2.StorageView.from_array, main.py:638,685) - or, as `Whisper.encode` returns it, a view of
    encoder output in device memory: f16 [B, n_audio_ctx, d_model] inside a `_lib.DevBuf` that every view of it shares and the last one frees.
    `view[i:j]` (utterances, step 1) is another view into the same block: a pointer offset, no copy.  A device view has no `.array`;
    `to_cpu()` reads it back as a host view of the same values in f32 (exact), which `generate` / `detect_language` / `align` take as well."""

    def __init__(self, array, *, _block=None, _offset=0, _shape=None, _owner=None):
        self.array = array
        self._block, self._offset, self._dev_shape, self._owner = _block, int(_offset), _shape, _owner

    @classmethod
    def from_array(cls, array):
        a = np.asarray(array)
        if a.dtype != np.float32 or not a.flags["C_CONTIGUOUS"]:
            raise ValueError("StorageView.from_array expects a C-contiguous float32 array")
        return cls(a)

    @classmethod
    def _on_device(cls, block, shape, owner=None, offset=0):
        """a view of f16 `shape` at byte `offset` of the _lib.DevBuf `block`; owner: the Whisper model that encoded it"""
        return cls(None, _block=block, _offset=offset, _shape=[int(x) for x in shape], _owner=weakref.ref(owner) if owner is not None else None)

    @property
    def device(self):
        return "cpu" if self._block is None else "cuda"

    @property
    def device_index(self):
        return 0 if self._block is None else int(self._block.device)

    @property
    def dtype(self):
        return "float32" if self._block is None else "float16"

    @property
    def shape(self):
        return list(self.array.shape) if self._block is None else list(self._dev_shape)

    @property
    def device_ptr(self):
        """address of the view's first element in device memory (device views only)"""
        if self._block is None or not self._block.ptr:
            raise ValueError("StorageView: not a live device view")
        return int(self._block.ptr.value) + self._offset

    def __len__(self):
        return self.shape[0]

    def __getitem__(self, key):
        if self._block is None:
            return StorageView(np.ascontiguousarray(self.array[key]))
        if isinstance(key, (int, np.integer)):
            k = int(key) + (self._dev_shape[0] if key < 0 else 0)
            key = slice(k, k + 1)
        if not isinstance(key, slice):
            raise TypeError("a device StorageView is sliced by utterance: view[i:j]")
        i, j, step = key.indices(self._dev_shape[0])
        if step != 1:
            raise ValueError("a device StorageView is sliced with step 1 (a pointer offset, no copy)")
        j = max(i, j)
        row = 2 * int(np.prod(self._dev_shape[1:], dtype=np.int64))
        v = StorageView(None, _block=self._block, _offset=self._offset + i * row, _shape=[j - i] + self._dev_shape[1:])
        v._owner = self._owner
        return v

    def to_cpu(self):
        """host view of the same values (f32; f16 -> f32 is exact)"""
        if self._block is None:
            return self
        h = np.empty(self._dev_shape, np.float16)
        if h.size:
            _lib.check(_lib.load().wis_dev_d2h(self._block.device, _lib.ptr(h), C.c_void_p(self.device_ptr), h.nbytes))
        return StorageView(h.astype(np.float32))

    def __array__(self, dtype=None, copy=None):
        a = self.to_cpu().array
        return a if dtype is None else a.astype(dtype, copy=False)


class WhisperGenerationResult:
    def __init__(self, sequences_ids, scores, no_speech_prob=0.0, phrase_logmass=None):
        self.sequences_ids = sequences_ids
        self.sequences = [[str(t) for t in s] for s in sequences_ids]
        self.scores = scores
        self.no_speech_prob = no_speech_prob
        self.phrase_logmass = phrase_logmass      # generate(..., phrases=..., return_phrase_mass=True): one float per hypothesis, else None

    def __repr__(self):
        return f"WhisperGenerationResult(sequences_ids={self.sequences_ids}, scores={self.scores})"


class WhisperAlignmentResult:
    """CTranslate2's `WhisperAlignmentResult`: `alignments` = [(text_index, time_index), ...] (the DTW path), `text_token_probs`."""

    def __init__(self, alignments, text_token_probs):
        self.alignments = alignments
        self.text_token_probs = text_token_probs

    def __repr__(self):
        return f"WhisperAlignmentResult(alignments={self.alignments!r}, text_token_probs={self.text_token_probs!r})"


class _Replica:
    def __init__(self, handle, device, n_mels=W.N_MELS, enc_shape=(W.N_AUDIO_CTX, 0)):
        self.handle, self.device = handle, device
        self.mel_bytes = n_mels * 3000 * 4      # one utterance's features
        self.enc_shape = (int(enc_shape[0]), int(enc_shape[1]))      # one utterance's encoder output [n_audio_ctx, d_model], f16
        self.enc_bytes = self.enc_shape[0] * self.enc_shape[1] * 2
        self.lock = threading.Lock()
        self.inflight = 0
        self.stage = None           # device block for batches of device-resident features (lazy)
        self.phrase_digest = None   # digest of the phrase set installed on the handle (wis_model_set_phrases), None: none yet
        self.hotword_digest = None  # ... of the hotword set (wis_model_set_hotwords)


def special_tokens_for(a, special=None, lang_ids=None):
    """The model's special-id table (weights.SpecialTokens) from its vocabulary size, with the ids the checkpoint states on top."""
    ov = dict(special or {})
    if lang_ids is not None and "lang_ids" not in ov:
        ov["lang_ids"] = list(lang_ids)
    return W.special_tokens(a["n_vocab"], ov)


def make_config(a, max_batch, max_beam, *, suppress_ids=None, suppress_begin=None, lang_ids=None, n_vocab=None, weight_bits=16, special=None):
    """special: a weights.SpecialTokens (default: the table of the vocabulary a["n_vocab"]); the 51865 defaults are the module constants."""
    st = special if isinstance(special, W.SpecialTokens) else special_tokens_for(a, special, lang_ids)
    sup = np.asarray(st.default_suppress_ids() if suppress_ids is None else suppress_ids, np.int32)
    beg = np.asarray([220, st.eot] if suppress_begin is None else suppress_begin, np.int32)
    lang = np.asarray(st.lang_ids if lang_ids is None else lang_ids, np.int32)
    cfg = _lib.Config()
    cfg.d_model, cfg.n_heads = a["d_model"], a["n_heads"]
    cfg.n_enc_layers = a.get("n_enc_layers", a["n_layers"])
    cfg.n_dec_layers = a.get("n_dec_layers", a["n_layers"])
    cfg.n_vocab = n_vocab or a["n_vocab"]
    cfg.n_audio_ctx, cfg.n_text_ctx, cfg.n_mels = a["n_audio_ctx"], a["n_text_ctx"], a["n_mels"]
    cfg.max_batch, cfg.max_beam = max_batch, max_beam
    cfg.eot, cfg.sot, cfg.no_timestamps, cfg.no_speech = st.eot, st.sot, st.notimestamps, st.nospeech
    cfg.suppress_ids = sup.ctypes.data_as(C.POINTER(C.c_int32)); cfg.n_suppress = len(sup)
    cfg.suppress_ids_begin = beg.ctypes.data_as(C.POINTER(C.c_int32)); cfg.n_suppress_begin = len(beg)
    cfg.lang_ids = lang.ctypes.data_as(C.POINTER(C.c_int32)); cfg.n_lang = len(lang)
    cfg.decoder_weight_bits = int(weight_bits)
    cfg._keep = (sup, beg, lang)
    return cfg


def make_tensor_index(index):
    arr = (_lib.Tensor * len(index))()
    keep = []
    for i, e in enumerate(index):
        nm = e["name"].encode()
        keep.append(nm)
        arr[i].name = nm
        arr[i].dtype = _lib.WIS_DT_F16 if e["dtype"] == "f16" else _lib.WIS_DT_F32
        arr[i].rank = len(e["shape"])
        for j, s in enumerate(e["shape"]):
            arr[i].shape[j] = s
        arr[i].offset = e["offset"]
    arr._keep = keep
    return arr


def create_handle(a, arena, index, device, max_batch=8, max_beam=5, arena_device_ptr=None, n_vocab=None, **cfgkw):
    """arena: uint8 ndarray (host) or None with arena_device_ptr = (ptr, nbytes) already on `device`."""
    cfg = make_config(a, max_batch, max_beam, n_vocab=n_vocab, **cfgkw)
    tens = make_tensor_index(index)
    h = C.c_void_p()
    if arena_device_ptr is not None:
        p, nbytes = arena_device_ptr
        rc = _lib.load().wis_model_create(C.byref(cfg), C.c_void_p(p), nbytes, 1, tens, len(index), device, C.byref(h))
    else:
        rc = _lib.load().wis_model_create(C.byref(cfg), _lib.ptr(arena), arena.nbytes, 0, tens, len(index), device, C.byref(h))
    _lib.check(rc)
    return h


def clone_handle(h):
    """Another replica on the same GPU sharing `h`'s weights (wis_model_clone): own stream, activations and KV caches."""
    c = C.c_void_p()
    _lib.check(_lib.load().wis_model_clone(h, C.byref(c)))
    return c


def create_replicas(a, arena, index, devices, max_batch=8, max_beam=5, **cfgkw):
    """One replica per entry of `devices` from ONE host upload: the arena goes to the first device over PCIe, every other
    replica receives it device-to-device (wis_dev_copy_peer: xGMI between peers) in a doubling tree - 0 -> 1, then {0 -> 2,
    1 -> 3}, ... - and is created from the device-resident copy (wis_model_create(arena_on_device=1)).  This is the
    single-process form of the one-time weight broadcast (the one-process-per-GPU form is wis_hip.dist.broadcast_arena over
    RCCL); nothing crosses GPUs at request time.  Returns the handles in `devices` order."""
    if len(devices) == 1:
        return [create_handle(a, arena, index, devices[0], max_batch, max_beam, **cfgkw)]
    lib = _lib.load()
    bufs = [None] * len(devices)
    handles = []
    try:
        bufs[0] = _lib.DevBuf.from_numpy(arena, devices[0])
        have = 1
        while have < len(devices):          # doubling: every device that holds the arena feeds one that does not
            for src in range(have):
                dst = have + src
                if dst >= len(devices):
                    break
                bufs[dst] = _lib.DevBuf(arena.nbytes, devices[dst])
                _lib.check(lib.wis_dev_copy_peer(devices[dst], bufs[dst].ptr, devices[src], bufs[src].ptr, arena.nbytes))
            have *= 2
        # every copy is done (hipMemcpyPeer is synchronous): each device's arena copy is released as soon as ITS replica has
        # re-packed it, so a device never holds more than its own arena copy + its model
        for i, d in enumerate(devices):
            handles.append(create_handle(a, None, index, d, max_batch, max_beam, arena_device_ptr=(bufs[i].ptr.value, arena.nbytes), **cfgkw))
            bufs[i].free()
            bufs[i] = None
    except BaseException:
        for h in handles:                   # a failed fan-out leaves nothing behind on any GPU
            lib.wis_model_destroy(h)
        raise
    finally:
        for b in bufs:
            if b is not None:
                b.free()
    return handles


def _last_trajectory(r, b, beam):
    """(tok [n][beam], org [n][beam]) int32: the live sets the last search on replica r left after each step (wis_last_trajectory)."""
    tok = np.zeros((256, beam), np.int32)
    org = np.zeros((256, beam), np.int32)
    n = C.c_int32(0)
    i32p = C.POINTER(C.c_int32)
    _lib.check(_lib.load().wis_last_trajectory(r.handle, b, tok.ctypes.data_as(i32p), org.ctypes.data_as(i32p), 256, C.byref(n)))
    return tok[:n.value].copy(), org[:n.value].copy()


class _Draft:
    """The draft of one utterance: `tokens` (the ids of an earlier hypothesis, beam 1) or `trajectory` ((tok, org) int32 [steps][beam] of an earlier
    beam search).  Compared and hashed by identity: the DecodeOptions of a drafted utterance equal no other call's, so it never shares a device
    batch, and the arrays are never compared or hashed."""
    __slots__ = ("tokens", "trajectory")

    def __init__(self, tokens=None, trajectory=None):
        self.tokens, self.trajectory = tokens, trajectory


class DecodeOptions(NamedTuple):
    """Everything but features, prompt and seed that one engine call needs - and the micro-batcher's key: two utterances share a device batch
    exactly when their records are equal (a NamedTuple: the batcher compares keys under its lock, and tuple == runs in C).  The record is
    canonical - an option that is off holds its default (max_initial_timestamp_index is 50 unless timestamps is on, sampling_temperature 1.0
    unless something is sampled); Whisper._decode_options builds it from a call's arguments.
    draft: None or a _Draft (one utterance, verified in multi-row passes before ordinary steps go on).  return_trajectory: every result carries
    `.trajectory`, what a later call takes as its draft.  timestamps: Whisper's timestamp rules every step (max_initial_timestamp_index None: no
    cap on the first timestamp).  no_speech_prob: every result carries P(<|nospeech|>) at <|startoftranscript|>.  repetition_penalty /
    no_repeat_ngram_size: CTranslate2's two options against looping hypotheses (include/wis_hip.h; 1 / 0: off).  sampling_topk (the ENGINE's
    value, as _check_sampling returns it: 0 off, -1 the whole vocabulary, 2 .. 16), sampling_temperature, num_hypotheses: random sampling and n
    results per utterance; every result then carries num_hypotheses sequences and scores.
    prompt_len RAGGED_PROMPT (-1) is the POOLED key: the rows of the batch carry prompts of any length 1 .. MAX_PROMPT, max_new_tokens was resolved
    from the longest the call may hold, and the batch decodes through wis_generate_ragged."""
    prompt_len: int
    beam_size: int
    max_new_tokens: int
    length_penalty: float = 1.0
    patience: float = 1.0
    suppress_blank: bool = True
    suppress_default: bool = True
    fixed_new_tokens: int = 0
    input_kind: int = _lib.WIS_IN_MEL_HOST
    draft: Optional[_Draft] = None
    return_trajectory: bool = False
    timestamps: bool = False
    max_initial_timestamp_index: Optional[int] = 50
    no_speech_prob: bool = False
    repetition_penalty: float = 1.0
    no_repeat_ngram_size: int = 0
    sampling_topk: int = 0
    sampling_temperature: float = 1.0
    num_hypotheses: int = 1


class ConstrainedOptions(DecodeOptions):
    """The DecodeOptions of a phrase-constrained call (`generate(..., phrases=...)`): the same record - `_fields` and every value a plain call
    with these arguments would have, max_new_tokens capped at the longest phrase + 1 - that carries the call's phrase set beside it:
    `phrase_trie` (int32 [n][4], weights.build_phrase_trie) and `phrase_digest` (its SHA-256).  The digest takes part in equality and hash, the
    type too: two calls share a device batch exactly when their options AND their phrase sets are equal, and a constrained record never equals a
    plain one.  The batch runner installs the set on the replica when the replica's current digest differs (_generate_chunk).
    `phrase_mass` (return_phrase_mass=True: the engine also computes every result's in-grammar mass, wis_gen_opts_t::phrase_mass) is carried the
    same way and takes part in equality and hash: calls that differ in it never share a device batch."""

    def __new__(cls, base, trie, digest, phrase_mass=False):
        self = tuple.__new__(cls, base)
        self.phrase_trie, self.phrase_digest, self.phrase_mass = trie, digest, bool(phrase_mass)
        return self

    def __eq__(self, other):
        return (type(other) is ConstrainedOptions and tuple.__eq__(self, other) and self.phrase_digest == other.phrase_digest
                and self.phrase_mass == other.phrase_mass)

    def __ne__(self, other):
        return not self == other

    def __hash__(self):
        return hash((tuple.__hash__(self), self.phrase_digest, self.phrase_mass))

    def _replace(self, **kw):
        return ConstrainedOptions(DecodeOptions(*self)._replace(**kw), self.phrase_trie, self.phrase_digest, self.phrase_mass)

    def __reduce__(self):
        return (ConstrainedOptions, (DecodeOptions(*self), self.phrase_trie, self.phrase_digest, self.phrase_mass))


class BoostedOptions(DecodeOptions):
    """The DecodeOptions of a hotword-boosted call (`generate(..., hotwords=..., hotword_boost=b)`): the same record - `_fields` and every value a
    plain call with these arguments would have - that carries the call's hotword set and boost beside it: `hotword_trie` (int32 [n][4],
    weights.build_hotword_trie), `hotword_digest` (its SHA-256) and `hotword_boost` (a float).  Digest, boost and type take part in equality and
    hash: two calls share a device batch exactly when their options, their hotword sets AND their boosts are equal, and a boosted record never
    equals a plain or a constrained one.  The batch runner installs the set on the replica when the replica's current digest differs."""

    def __new__(cls, base, trie, digest, boost):
        self = tuple.__new__(cls, base)
        self.hotword_trie, self.hotword_digest, self.hotword_boost = trie, digest, float(boost)
        return self

    def __eq__(self, other):
        return (type(other) is BoostedOptions and tuple.__eq__(self, other) and self.hotword_digest == other.hotword_digest
                and self.hotword_boost == other.hotword_boost)

    def __ne__(self, other):
        return not self == other

    def __hash__(self):
        return hash((tuple.__hash__(self), self.hotword_digest, self.hotword_boost))

    def _replace(self, **kw):
        return BoostedOptions(DecodeOptions(*self)._replace(**kw), self.hotword_trie, self.hotword_digest, self.hotword_boost)

    def __reduce__(self):
        return (BoostedOptions, (DecodeOptions(*self), self.hotword_trie, self.hotword_digest, self.hotword_boost))


def _check_hotword_boost(boost):
    """-> the boost as a float: finite and > 0 (a ValueError otherwise; no default is offered: a useful value depends on the checkpoint)"""
    try:
        b = float(boost)
    except (TypeError, ValueError):
        raise ValueError(f"hotword_boost {boost!r}: a finite number > 0") from None
    with np.errstate(over="ignore", under="ignore"):
        b32 = np.float32(b)      # (what the engine takes: a value that is 0 or inf in float32 is refused here, not there)
    if not (np.isfinite(b) and b > 0 and np.isfinite(b32) and b32 > 0):
        raise ValueError(f"hotword_boost {boost!r}: a finite number > 0")
    return b


def _hotword_set(hotwords, special, decode_config):
    """-> (trie, digest) of a call's `hotwords` ([[token ids], ...]), validated against the MODEL's lists as a phrase list is"""
    import hashlib
    try:
        hotwords = [list(hw) for hw in hotwords]
    except TypeError:
        raise ValueError(f"hotwords {hotwords!r}: a list of token id lists") from None
    sup = decode_config.get("suppress_ids")
    beg = decode_config.get("suppress_ids_begin")
    trie = W.build_hotword_trie(hotwords, eot=special.eot, suppress_ids=special.default_suppress_ids() if sup is None else sup,
                                suppress_begin=[220, special.eot] if beg is None else beg)
    return trie, hashlib.sha256(trie.tobytes()).hexdigest()


def _phrase_set(phrases, special, decode_config):
    """-> (trie, digest, longest phrase) of a call's `phrases` ([[token ids], ...]), validated against the MODEL's lists (what the engine checks
    again): a ValueError names the offending phrase."""
    import hashlib
    try:
        phrases = [list(ph) for ph in phrases]
    except TypeError:
        raise ValueError(f"phrases {phrases!r}: a list of token id lists") from None
    sup = decode_config.get("suppress_ids")
    beg = decode_config.get("suppress_ids_begin")
    trie = W.build_phrase_trie(phrases, eot=special.eot, suppress_ids=special.default_suppress_ids() if sup is None else sup,
                               suppress_begin=[220, special.eot] if beg is None else beg)
    return trie, hashlib.sha256(trie.tobytes()).hexdigest(), max(len(ph) for ph in phrases)


RAGGED_PROMPT = -1         # DecodeOptions.prompt_len of the pooled key: prompts of different lengths in one device batch (wis_generate_ragged)


def _longest_first(prompts):
    """-> the rows' indices, longest prompt first (a stable sort: equal lengths keep their order) - the order in which wis_generate_ragged's
    windowed prefill needs the fewest passes"""
    return sorted(range(len(prompts)), key=lambda i: -len(prompts[i]))


def _gen_opts(opts):
    """The engine's wis_gen_opts_t of a DecodeOptions."""
    o = _lib.GenOpts(opts.input_kind, opts.beam_size, opts.max_new_tokens, opts.length_penalty, opts.patience, int(bool(opts.suppress_blank)),
                     int(bool(opts.suppress_default)), int(opts.fixed_new_tokens), 0)
    if opts.timestamps:
        o.timestamps = 1
        o.max_initial_timestamp_index = -1 if opts.max_initial_timestamp_index is None else int(opts.max_initial_timestamp_index)
    o.no_speech_prob = int(bool(opts.no_speech_prob))
    o.repetition_penalty, o.no_repeat_ngram_size = float(opts.repetition_penalty), int(opts.no_repeat_ngram_size)
    if opts.sampling_topk != 0 or opts.num_hypotheses > 1:
        o.sampling_topk, o.sampling_temperature, o.num_hypotheses = int(opts.sampling_topk), float(opts.sampling_temperature), int(opts.num_hypotheses)
    o.phrases = int(getattr(opts, "phrase_trie", None) is not None)
    o.phrase_mass = int(bool(getattr(opts, "phrase_mass", False)))
    if getattr(opts, "hotword_trie", None) is not None:      # (only a boosted call builds the full struct: every other call's record is what it was)
        full = _lib.HotGenOpts()
        C.memmove(C.addressof(full), C.addressof(o), C.sizeof(_lib.GenOpts))
        full.hotwords, full.hotword_boost = 1, float(opts.hotword_boost)
        return full
    return o


def _generate_chunk(r, mel, prompts, opts, *rest, device_ptr=None, seeds=None):
    """One engine call on replica r (the caller serialises access to r).  mel: host ndarray [B, ...] - or, with device_ptr, just the batch size B
    of features already resident on r.device.  opts: a DecodeOptions (its first nine fields may also be spelled out positionally: prompt length,
    beam, ...).  seeds: one uint64 per utterance (sampled calls).  opts.draft goes to wis_generate_draft_beam / wis_generate_draft, a sampled or
    n-best call to wis_generate_n, everything else to wis_generate.  Under the pooled key (prompt_len RAGGED_PROMPT) the rows go to
    wis_generate_ragged longest prompt first and the results come back in the rows' own order (features on the device lie where they lie: their
    rows keep their order, which the engine serves as well - _run_batch sorts those before it gathers them)."""
    if rest:
        opts = DecodeOptions(opts, *rest)
    B = int(mel) if device_ptr is not None else mel.shape[0]
    P, beam, n, draft = opts.prompt_len, opts.beam_size, int(opts.num_hypotheses), opts.draft
    o = _gen_opts(opts)
    trie = getattr(opts, "phrase_trie", None)
    if trie is not None and r.phrase_digest != opts.phrase_digest:      # (installing a set is a copy: no new step graph)
        r.phrase_digest = None
        _lib.check(_lib.load().wis_model_set_phrases(r.handle, trie.ctypes.data_as(C.POINTER(C.c_int32)), len(trie)))
        r.phrase_digest = opts.phrase_digest
    hot = getattr(opts, "hotword_trie", None)
    if hot is not None and getattr(r, "hotword_digest", None) != opts.hotword_digest:      # (a copy too; the set and the boost are no part of a step graph)
        r.hotword_digest = None
        _lib.check(_lib.load().wis_model_set_hotwords(r.handle, hot.ctypes.data_as(C.POINTER(C.c_int32)), len(hot)))
        r.hotword_digest = opts.hotword_digest
    order = None
    if P == RAGGED_PROMPT:
        if draft is not None or opts.return_trajectory:
            raise ValueError("prompts of different lengths cannot be combined with drafts or return_trajectory")
        prompts = [[int(t) for t in p] for p in prompts]
        P0 = len(prompts[0])
        if P0 <= SHORT_PROMPT and B * P0 > MAX_DECODER_ROWS and all(len(p) == P0 for p in prompts):
            # a pooled batch that happens to hold ONE short length is the default call to the engine (the merged prefill, B * P rows): more
            # utterances than that pass takes go in several such calls
            step, row_bytes, out = MAX_DECODER_ROWS // P0, (r.mel_bytes if opts.input_kind == _lib.WIS_IN_MEL_DEV else r.enc_bytes) if device_ptr is not None else 0, []
            for lo in range(0, B, step):
                hi = min(B, lo + step)
                out += _generate_chunk(r, hi - lo if device_ptr is not None else mel[lo:hi], prompts[lo:hi], opts._replace(prompt_len=P0),
                                       device_ptr=None if device_ptr is None else device_ptr + lo * row_bytes, seeds=None if seeds is None else seeds[lo:hi])
            return out
        if device_ptr is None:
            order = _longest_first(prompts)
            prompts, mel = [prompts[i] for i in order], np.ascontiguousarray(mel[order])
            if seeds is not None:
                seeds = [seeds[i] for i in order]
        plen = np.ascontiguousarray(np.asarray([len(p) for p in prompts], np.int32))
        pr = np.ascontiguousarray(np.asarray([t for p in prompts for t in p], np.int32))
    else:
        pr = np.ascontiguousarray(np.asarray(prompts, np.int32).reshape(B, P))
    ids = np.zeros((B, n, opts.max_new_tokens), np.int32)
    lens = np.zeros((B, n), np.int32)
    scores = np.zeros((B, n), np.float32)
    src = C.c_void_p(device_ptr) if device_ptr is not None else _lib.ptr(mel)
    i32p, lib = C.POINTER(C.c_int32), _lib.load()
    out_ptrs = (ids.ctypes.data_as(i32p), lens.ctypes.data_as(i32p), scores.ctypes.data_as(C.POINTER(C.c_float)))
    acc = None
    if P == RAGGED_PROMPT:
        sd = np.ascontiguousarray(np.asarray([0] * B if seeds is None else [int(x) & 0xFFFFFFFFFFFFFFFF for x in seeds], np.uint64))
        _lib.check(lib.wis_generate_ragged(r.handle, src, B, pr.ctypes.data_as(i32p), plen.ctypes.data_as(i32p), C.byref(o), sd.ctypes.data_as(C.POINTER(C.c_uint64)), *out_ptrs))
    elif draft is not None and draft.trajectory is not None:
        dt, do = (np.ascontiguousarray(np.asarray(a, np.int32)) for a in draft.trajectory)
        if dt.ndim != 2 or dt.shape != do.shape or dt.shape[1] != beam:
            raise ValueError(f"draft trajectory must be two [steps][{beam}] arrays, got {dt.shape} / {do.shape}")
        acc = C.c_int32(0)
        _lib.check(lib.wis_generate_draft_beam(r.handle, src, pr.ctypes.data_as(i32p), P, C.byref(o), dt.ctypes.data_as(i32p), do.ctypes.data_as(i32p), int(dt.shape[0]),
                                               *out_ptrs, C.byref(acc)))
    elif draft is not None and draft.tokens:
        d = np.ascontiguousarray(np.asarray(draft.tokens, np.int32))
        acc = C.c_int32(0)
        _lib.check(lib.wis_generate_draft(r.handle, src, pr.ctypes.data_as(i32p), P, C.byref(o), d.ctypes.data_as(i32p), int(d.shape[0]), *out_ptrs, C.byref(acc)))
    elif opts.sampling_topk != 0 or n > 1:
        sd = np.ascontiguousarray(np.asarray([0] * B if seeds is None else [int(x) & 0xFFFFFFFFFFFFFFFF for x in seeds], np.uint64))
        _lib.check(lib.wis_generate_n(r.handle, src, B, pr.ctypes.data_as(i32p), P, C.byref(o), sd.ctypes.data_as(C.POINTER(C.c_uint64)), *out_ptrs))
    else:
        _lib.check(lib.wis_generate(r.handle, src, B, pr.ctypes.data_as(i32p), P, C.byref(o), *out_ptrs))
    nsp = np.zeros(B, np.float32)
    if opts.no_speech_prob:
        _lib.check(lib.wis_last_no_speech_prob(r.handle, B, nsp.ctypes.data_as(C.POINTER(C.c_float))))
    # (a constrained search whose set reaches fewer than n phrases fills up with -inf hypotheses: those are dropped)
    keep = [[j for j in range(n) if trie is None or scores[b, j] != -np.inf] for b in range(B)]
    out = [WhisperGenerationResult([ids[b, j, :lens[b, j]].tolist() for j in keep[b]], [float(scores[b, j]) for j in keep[b]], float(nsp[b])) for b in range(B)]
    if getattr(opts, "phrase_mass", False):      # the in-grammar mass of every result, in the engine's (unsorted) batch order like everything above
        mass = np.zeros((B, n), np.float32)
        _lib.check(lib.wis_last_phrase_mass(r.handle, B, n, mass.ctypes.data_as(C.POINTER(C.c_float))))
        for b in range(B):
            out[b].phrase_logmass = [float(mass[b, j]) for j in keep[b]]
    if acc is not None:
        out[0].accepted_draft_tokens = int(acc.value)      # tokens (beam 1) or search steps (beam > 1) of the draft the final decode kept
    if opts.return_trajectory:
        for b in range(B):
            out[b].trajectory = _last_trajectory(r, b, beam)
    if order is not None:
        back = [None] * B
        for at, i in enumerate(order):
            back[i] = out[at]
        out = back
    return out


class EncodeKey(NamedTuple):
    """The micro-batcher's key of `Whisper.encode` rows: windows of concurrent requests share one encoder batch when their input kind is the
    same.  A type of its own, so it never equals a DecodeOptions - an encode row never lands in a decode batch or the other way round."""
    input_kind: int = _lib.WIS_IN_MEL_HOST

    def __eq__(self, other):
        return type(other) is EncodeKey and tuple.__eq__(self, other)

    def __ne__(self, other):
        return not self == other

    __hash__ = tuple.__hash__


_ENCODED_KINDS = (_lib.WIS_IN_ENC_DEV, _lib.WIS_IN_ENC_HOST)


def _encode_chunk(r, features, input_kind, device_ptr=None):
    """One wis_encode call on replica r (the caller serialises access to r) -> a device StorageView [B, n_audio_ctx, d_model] that owns its block.
    features: host ndarray [B, ...] - or, with device_ptr, just the batch size B of features already resident on r.device."""
    B = int(features) if device_ptr is not None else features.shape[0]
    T, d = r.enc_shape
    block = _lib.DevBuf(B * r.enc_bytes, r.device)
    src = C.c_void_p(device_ptr) if device_ptr is not None else _lib.ptr(features)
    _lib.check(_lib.load().wis_encode(r.handle, src, int(input_kind), B, block.ptr, None))
    return StorageView._on_device(block, [B, T, d])


def _gather_device_rows(replica, ptrs, row_bytes):
    """-> the address of len(ptrs) consecutive rows on replica.device (the caller holds replica.lock): the rows themselves when they already lie
    back to back (one utterance; the slices of one encode), else a device-to-device copy into the replica's staging block - nothing visits the host"""
    if all(ptrs[i + 1] == ptrs[i] + row_bytes for i in range(len(ptrs) - 1)):
        return ptrs[0]
    rb = max(replica.mel_bytes, replica.enc_bytes, int(row_bytes))      # the block serves every row kind; never smaller than the rows written now
    if replica.stage is None or replica.stage.nbytes < len(ptrs) * rb:
        replica.stage = _lib.DevBuf(max(len(ptrs), 8) * rb, replica.device)
    lib = _lib.load()
    for i, src in enumerate(ptrs):
        _lib.check(lib.wis_dev_copy_peer(replica.device, C.c_void_p(replica.stage.ptr.value + i * row_bytes), replica.device, C.c_void_p(src), row_bytes))
    return replica.stage.ptr.value


MAX_DECODER_ROWS = 96      # csrc/kernels.hpp MAX_ROWS: decoder rows per device pass
MAX_BEAM = 8               # csrc/kernels.hpp MAX_R: rows per utterance (beam size)
MAX_REPLICAS_PER_DEVICE = 4   # default ceiling for inter_threads -> replicas per GPU (measured on MI355X, bench.py "concurrent_device_batches": 118 / 152 / 165 / 173 / 160 utterances/s with 1..5 batches of 8 in flight)
SHORT_PROMPT = 16          # csrc/generate.hip SHORT_PROMPT: prompts up to here run as ONE merged prefill + first step pass (B * P decoder rows)
MAX_PROMPT = 228           # wis_generate: prompt tokens per utterance (n_text_ctx / 2 + 4: openai-whisper's 223 prompt tokens behind <|startofprev|>, the start sequence);
                           # more than SHORT_PROMPT take the long-prompt route (windowed prefill, shared prompt prefix)
MAX_HYPOTHESES = 24        # csrc/kernels.hpp MAX_HYP: finished hypotheses an utterance's search can hold
MAX_SAMPLING_TOPK = 16     # csrc/kernels.hpp MAX_CAND: the largest sampling_topk short of the whole vocabulary


def timestamp_prompt(prompt, special=None):
    """True when `prompt` asks for timestamps: from <|startoftranscript|> on it holds only the start sequence's special tokens
    (language, task; ids in [<|endoftext|>, <|notimestamps|>)) and no <|notimestamps|> - what CTranslate2 decodes under Whisper's
    timestamp rules.  A prompt without <|startoftranscript|>, with <|notimestamps|>, or with text or timestamp tokens after its start
    sequence (a decoder prefix) keeps the plain search the engine has always run for it.  special: the model's SpecialTokens
    (default: the 51865-token vocabulary)."""
    p = [int(t) for t in prompt]
    sot, eot, nts = (W.SOT, W.EOT, W.NO_TIMESTAMPS) if special is None else (special.sot, special.eot, special.notimestamps)
    if sot not in p:
        return False
    return all(eot <= t < nts for t in p[p.index(sot):])


def _check_repetition(repetition_penalty, no_repeat_ngram_size, drafted=False):
    """-> (penalty, n-gram size) as the engine takes them; a value CTranslate2 would not take, or either option together with a draft, is a
    request error (ValueError -> HTTP 400 in wis_hip.server)."""
    try:
        p = float(repetition_penalty)
        n = int(no_repeat_ngram_size)
        if n != float(no_repeat_ngram_size):
            raise ValueError
    except (TypeError, ValueError, OverflowError):
        raise ValueError(f"repetition_penalty {repetition_penalty!r} / no_repeat_ngram_size {no_repeat_ngram_size!r}: a number and an integer") from None
    if not (p > 0 and p != float("inf")):
        raise ValueError(f"repetition_penalty {repetition_penalty!r} must be a finite number > 0 (1: off)")
    if n < 0:
        raise ValueError(f"no_repeat_ngram_size {no_repeat_ngram_size!r} must be >= 0 (0: off)")
    if drafted and (p != 1.0 or n != 0):
        raise ValueError("repetition_penalty / no_repeat_ngram_size cannot be combined with draft_tokens / draft_trajectory")
    return p, n


class UnsupportedOption(ValueError, NotImplementedError):
    """A decoding option (or combination) this shim does not serve.  A ValueError like every other request error (HTTP 400 in wis_hip.server);
    also the NotImplementedError that `sampling_topk` / `num_hypotheses` raised before they existed, for the calls that stay unserved."""


def _check_sampling(beam_size, num_hypotheses, sampling_topk, sampling_temperature, drafted=False):
    """-> (top-k, temperature, n) as the ENGINE takes them (include/wis_hip.h: top-k 0 off, -1 the whole vocabulary, 2 .. 16); CTranslate2's
    sampling_topk counts 1 as off and 0 as the whole vocabulary.  Validated as the C side validates: a bad value is a ValueError.
    This face samples from the WHOLE vocabulary only (sampling_topk=0, what the temperature fallback calls): a top-k of 2 .. 16 is served by the
    engine (wis_generate_n / wis_debug_search_n) but answered UnsupportedOption here, as is num_hypotheses beyond what the search can return."""
    try:
        k, n, T = int(sampling_topk), int(num_hypotheses), float(sampling_temperature)
        if k != float(sampling_topk) or n != float(num_hypotheses):
            raise ValueError
    except (TypeError, ValueError, OverflowError):
        raise ValueError(f"sampling_topk {sampling_topk!r} / num_hypotheses {num_hypotheses!r} / sampling_temperature {sampling_temperature!r}: two integers and a number") from None
    if k < 0 or k > MAX_SAMPLING_TOPK:
        raise ValueError(f"sampling_topk {k} outside 0 (the whole vocabulary), 1 (off), 2..{MAX_SAMPLING_TOPK}")
    if not (T > 0 and T != float("inf")):
        raise ValueError(f"sampling_temperature {sampling_temperature!r} must be a finite number > 0")
    if not 1 <= n <= MAX_BEAM:
        raise ValueError(f"num_hypotheses {n} outside 1..{MAX_BEAM}")
    on = k != 1
    if k >= 2:
        raise UnsupportedOption(f"sampling_topk {k}: this face samples from the whole vocabulary (sampling_topk=0); the engine's top-k of 2..{MAX_SAMPLING_TOPK} "
                                "is reachable through wis_generate_n")
    if on and int(beam_size) != 1:
        raise ValueError(f"random sampling (sampling_topk {k}) needs beam_size 1, got {beam_size}")
    if not on and n > int(beam_size):
        raise UnsupportedOption(f"num_hypotheses {n} > beam_size {beam_size}" + (" (more than one hypothesis at beam_size 1 needs sampling_topk=0)" if int(beam_size) == 1 else ""))
    if drafted and (on or n != 1):
        raise ValueError("sampling_topk / num_hypotheses cannot be combined with draft_tokens / draft_trajectory")
    return (0 if not on else (-1 if k == 0 else k)), (T if on else 1.0), n


def _check_patience(beam_size, patience):
    """CTranslate2 searches until round(beam_size * patience) hypotheses have finished; the engine stores MAX_HYPOTHESES - beam_size + 1.
    A patience beyond that is a request error (it used to be clamped silently: a shorter search than CTranslate2's, other ids)."""
    p = float(patience) if float(patience) > 0 else 1.0
    if int(round(int(beam_size) * p)) > MAX_HYPOTHESES - int(beam_size) + 1:
        raise ValueError(f"patience {patience} at beam_size {beam_size} is beyond the engine's hypothesis storage (patience <= {(MAX_HYPOTHESES - int(beam_size) + 1) / int(beam_size):.3g} at this beam)")


def _seeds(opts, sampling_seed, B):
    """One seed per utterance of a call: `sampling_seed` (an int for the call, or one per utterance), or fresh ones; 0 when nothing is sampled."""
    if opts.sampling_topk == 0:
        return [0] * B
    if sampling_seed is None:
        return [_next_seed() for _ in range(B)]
    seeds = [int(sampling_seed)] * B if np.isscalar(sampling_seed) else [int(x) for x in sampling_seed]
    if len(seeds) != B:
        raise ValueError(f"sampling_seed: {len(seeds)} seeds for {B} utterances")
    return [sd & 0xFFFFFFFFFFFFFFFF for sd in seeds]


def _capacity(max_batch, opts):
    """Utterances per device batch: the decoder handles <= MAX_DECODER_ROWS rows per pass - utterances x beam while decoding,
    utterances x P in the merged prefill + first step (wis_generate enforces B * P <= MAX_ROWS and B * beam <= MAX_ROWS).
    A prompt of more than SHORT_PROMPT tokens is prefilled in windows whose last one shrinks with the batch (min(16, MAX_ROWS // B) rows per
    utterance): the capacity no longer divides by P.  An EncodeKey (Whisper.encode rows): the encoder takes max_batch windows."""
    if isinstance(opts, EncodeKey):
        return max(1, int(max_batch))
    P = opts.prompt_len
    rows = max(opts.beam_size, opts.num_hypotheses, 1)      # decoder rows per utterance: its beams, or its num_hypotheses samples
    if P > SHORT_PROMPT or P == RAGGED_PROMPT:      # (the pooled key: every utterance takes the long-prompt route)
        return max(1, min(max_batch, MAX_DECODER_ROWS // rows))
    return max(1, min(max_batch, MAX_DECODER_ROWS // rows, MAX_DECODER_ROWS // max(P, 1)))


def _run_batch(replica, opts, rows):
    """One device batch: rows = [(features, prompt, seed[, what keeps a device address alive])] of utterances whose DecodeOptions are equal (seed 0 when nothing is sampled) - or,
    under an EncodeKey, rows = [features] of windows to encode together: every row gets its one-utterance slice of the batch's view."""
    if isinstance(opts, EncodeKey):
        with replica.lock:
            if opts.input_kind == _lib.WIS_IN_MEL_DEV:
                view = _encode_chunk(replica, len(rows), opts.input_kind, device_ptr=_gather_device_rows(replica, [int(r) for r in rows], replica.mel_bytes))
            else:
                view = _encode_chunk(replica, np.ascontiguousarray(np.stack(rows)), opts.input_kind)
        return [view[i:i + 1] for i in range(len(rows))]
    if opts.prompt_len == RAGGED_PROMPT and opts.input_kind in (_lib.WIS_IN_MEL_DEV, _lib.WIS_IN_ENC_DEV):
        # rows on the device are gathered in the order they go to the engine: longest prompt first here, the results back in the rows' own order
        order = _longest_first([r[1] for r in rows])
        rows = [rows[i] for i in order]
        with replica.lock:
            ptr = _gather_device_rows(replica, [int(r[0]) for r in rows], replica.mel_bytes if opts.input_kind == _lib.WIS_IN_MEL_DEV else replica.enc_bytes)
            res = _generate_chunk(replica, len(rows), [r[1] for r in rows], opts, device_ptr=ptr, seeds=[r[2] for r in rows])
        back = [None] * len(rows)
        for at, i in enumerate(order):
            back[i] = res[at]
        return back
    prompts, seeds = [r[1] for r in rows], [r[2] for r in rows]
    if opts.input_kind in (_lib.WIS_IN_MEL_DEV, _lib.WIS_IN_ENC_DEV):
        # features (streaming sessions: audio.MelStream.finish) or encoder output (Whisper.encode) that already live in this replica's HBM: one
        # utterance goes in by pointer, several are gathered device-to-device into the replica's staging block - nothing visits the host
        rb = replica.mel_bytes if opts.input_kind == _lib.WIS_IN_MEL_DEV else replica.enc_bytes
        with replica.lock:
            ptr = _gather_device_rows(replica, [int(r[0]) for r in rows], rb)
            return _generate_chunk(replica, len(rows), prompts, opts, device_ptr=ptr, seeds=seeds)
    mel = np.ascontiguousarray(np.stack([r[0] for r in rows]))
    with replica.lock:
        return _generate_chunk(replica, mel, prompts, opts, seeds=seeds)


class Whisper:
    """One replica per entry of `device_index` (reference: `device_index=[*range(cuda_num_devices)]`, main.py:295)."""

    is_multilingual = True

    def __init__(self, model_path, device="cuda", device_index=0, compute_type="default", inter_threads=1, intra_threads=0,
                 max_batch=8, max_beam=5, weights=None, arch=None, replicas_per_device=None, **_ignored):
        if device not in ("cuda", "auto", "hip", "gpu"):
            raise ValueError(f"wis_hip runs on MI355X GPUs only (device={device!r}); there is no CPU path")
        _lib.require_gpu()
        # "float16" (default / "auto") or "int8_float16" (the reference's GPU default, main.py:242): per-row int8 DECODER
        # weights with f16 activations; everything else stays f16
        if compute_type in ("int8_float16", "int8"):
            self.compute_type = "int8_float16"
        elif compute_type in ("default", "auto", "float16", "float32"):
            self.compute_type = "float16"
        else:
            raise ValueError(f"unsupported compute_type {compute_type!r} (float16, int8_float16)")
        cfg = {}
        if weights is None:
            weights, arch, cfg = self._load(model_path)
        self.arch, self.decode_config = arch, cfg
        self.special = special_tokens_for(arch, cfg.get("special"), cfg.get("lang_ids"))
        devs = list(device_index) if isinstance(device_index, (list, tuple)) else [int(device_index)]
        if not 1 <= int(max_batch) <= MAX_DECODER_ROWS:
            raise ValueError(f"max_batch={max_batch}: a device batch holds 1..{MAX_DECODER_ROWS} utterances")
        if not 1 <= int(max_beam) <= MAX_BEAM:
            raise ValueError(f"max_beam={max_beam}: the engine decodes with beam sizes 1..{MAX_BEAM}")
        arena, index = W.build_arena(weights)
        kw = dict(suppress_ids=cfg.get("suppress_ids"), suppress_begin=cfg.get("suppress_ids_begin"), lang_ids=cfg.get("lang_ids"),
                  weight_bits=8 if self.compute_type == "int8_float16" else 16, special=self.special)
        enc_shape = (arch["n_audio_ctx"], arch["d_model"])
        self._replicas = [_Replica(h, d, arch["n_mels"], enc_shape) for h, d in zip(create_replicas(arch, arena, index, devs, max_batch, max_beam, **kw), devs)]
        # CTranslate2's `inter_threads` = batches a model runs in parallel (reference main.py:341-355 passes ctranslate2_threads).  Here:
        # replicas PER GPU that share one weight copy (wis_model_clone) and run their device batches concurrently on their own
        # streams - a decode chain is latency-bound and leaves most of the chip idle, a second batch in flight fills it.  The count is
        # bounded by `replicas_per_device` (each replica owns its activations and KV caches: ~0.7 GB per utterance slot for large-v2).
        per_dev = MAX_REPLICAS_PER_DEVICE if replicas_per_device is None else int(replicas_per_device)
        per_dev = max(1, min(int(inter_threads) if inter_threads else 1, per_dev))
        for r in list(self._replicas):
            for _ in range(per_dev - 1):
                self._replicas.append(_Replica(clone_handle(r.handle), r.device, arch["n_mels"], r.enc_shape))
        self._set_alignment_heads(cfg.get("alignment_heads"))
        self.max_batch, self.max_beam = max_batch, max_beam
        self._pick = threading.Lock()
        # concurrent generate() calls coalesce into device batches, one worker per GPU replica (wis_hip/batching.py)
        self._batcher = MicroBatcher(self._replicas, _run_batch, lambda opts: _capacity(max_batch, opts))

    @classmethod
    def from_handles(cls, handles, arch, max_batch=8, max_beam=5, decode_config=None):
        """Wrap replicas that already exist: [(wis_model handle, device), ...] - e.g. models created from a weight arena an
        RCCL broadcast delivered straight into device memory (`create_handle(arena_device_ptr=...)`, wis_hip/dist.py)."""
        self = cls.__new__(cls)
        self.compute_type = "float16"
        self.arch, self.decode_config = arch, decode_config or {}
        self.special = special_tokens_for(arch, self.decode_config.get("special"), self.decode_config.get("lang_ids"))
        self._replicas = [_Replica(h, d, arch["n_mels"], (arch["n_audio_ctx"], arch["d_model"])) for h, d in handles]
        self._set_alignment_heads(self.decode_config.get("alignment_heads"))
        self.max_batch, self.max_beam = max_batch, max_beam
        self._pick = threading.Lock()
        self._batcher = MicroBatcher(self._replicas, _run_batch, lambda opts: _capacity(max_batch, opts))
        return self

    @staticmethod
    def _load(model_path):
        """'synthetic:<size>[:seed]' (no checkpoint offline), a CTranslate2 model directory (what WIS ships) or a
        Hugging Face safetensors checkpoint directory."""
        if isinstance(model_path, str) and model_path.startswith("synthetic:"):
            parts = model_path.split(":")
            size = parts[1]
            seed = int(parts[2]) if len(parts) > 2 else 1234
            return W.synthetic_weights(size, seed=seed), W.arch(size), {}
        if not os.path.isdir(model_path):
            raise FileNotFoundError(f"{model_path}: not a model directory (CTranslate2 or Hugging Face; or use 'synthetic:<size>')")
        return W.load_model_dir(model_path)

    def close(self):
        b = self.__dict__.pop("_batcher", None)
        if b is not None:
            b.close()

    def __del__(self):
        try:
            self.close()
            for r in getattr(self, "_replicas", []):
                if r.handle:
                    _lib.load().wis_model_destroy(r.handle)
                    r.handle = None
        except Exception:
            pass

    def _acquire(self):
        with self._pick:
            r = min(self._replicas, key=lambda x: x.inflight)
            r.inflight += 1
        return r

    def _release(self, r):
        with self._pick:
            r.inflight -= 1

    @property
    def n_mels(self):
        return int((getattr(self, "arch", None) or {}).get("n_mels", W.N_MELS))

    def _features(self, features, input_kind=_lib.WIS_IN_MEL_HOST):
        nm = self.n_mels
        a = features.array if isinstance(features, StorageView) else np.asarray(features)
        if a.dtype != np.float32:
            a = a.astype(np.float32)
        a = np.ascontiguousarray(a)
        if input_kind == _lib.WIS_IN_PCM_HOST:
            if a.ndim != 2 or a.shape[1] != _lib.N_SAMPLES:
                raise ValueError(f"PCM input must be [batch, {_lib.N_SAMPLES}] float32 (pad_or_trim'ed 30 s windows), got {a.shape}")
        elif input_kind == _lib.WIS_IN_MEL_HOST:
            if a.ndim != 3 or a.shape[1:] != (nm, 3000):
                raise ValueError(f"features must be [batch, {nm}, 3000] float32 for this model ({nm} mel bins), got {a.shape}")
        else:
            raise ValueError("the Python face takes host arrays (WIS_IN_MEL_HOST or WIS_IN_PCM_HOST)")
        return a

    @property
    def _enc_shape(self):
        a = getattr(self, "arch", None) or {}
        return int(a.get("n_audio_ctx", W.N_AUDIO_CTX)), int(a.get("d_model", 0))

    def _check_open(self):
        if "_batcher" not in self.__dict__:
            raise ValueError("this Whisper model is closed")

    def _encoded(self, features):
        """Encoder output recognised by what it is.  -> None: `features` are features.  (WIS_IN_ENC_DEV, device, [address per utterance],
        [the block behind each address]): a device-resident StorageView of `encode` (or a list of them, utterances in order); whoever queues an
        address keeps its block referenced beside it until the engine call has returned.  (WIS_IN_ENC_HOST, f32 array [B, n_audio_ctx, d_model]):
        a host view or array of that shape - [B, n_mels, 3000] cannot be mistaken for it.  A device view that this model cannot decode - another
        width, another GPU than any replica's, a closed model's - is a ValueError before the engine is reached."""
        T, d = self._enc_shape
        views = list(features) if isinstance(features, (list, tuple)) and len(features) and all(isinstance(v, StorageView) for v in features) else [features]
        if any(isinstance(v, StorageView) and v.device == "cuda" for v in views):
            if not all(isinstance(v, StorageView) and v.device == "cuda" for v in views):
                raise ValueError("device-resident and host StorageViews cannot be mixed in one call")
            self._check_open()
            dev = views[0].device_index
            ptrs, blocks = [], []
            for v in views:
                if len(v.shape) != 3 or tuple(v.shape[1:]) != (T, d):
                    raise ValueError(f"encoder output must be [batch, {T}, {d}] for this model (d_model {d}), got {v.shape}")
                owner = v._owner() if v._owner is not None else self
                if owner is None or "_batcher" not in owner.__dict__:
                    raise ValueError("this encoder output belongs to a Whisper model that has been closed")
                if v.device_index != dev:
                    raise ValueError(f"encoder output on devices {dev} and {v.device_index} in one call")
                row = 2 * T * d
                ptrs.extend(v.device_ptr + b * row for b in range(v.shape[0]))
                blocks.extend([v._block] * v.shape[0])
            if not any(r.device == dev for r in self._replicas):
                raise ValueError(f"encoder output lives on device {dev}, where this model has no replica")
            return _lib.WIS_IN_ENC_DEV, dev, ptrs, blocks
        if len(views) != 1:
            return None
        a = features.array if isinstance(features, StorageView) else features
        if isinstance(a, np.ndarray) and a.ndim == 3 and d > 0 and tuple(a.shape[1:]) == (T, d):
            return _lib.WIS_IN_ENC_HOST, np.ascontiguousarray(a, np.float32)
        return None

    def _encoder_input(self, features, input_kind):
        """_encoded for a call that also takes `input_kind`: the argument keeps meaning what it means for host feature arrays (any other value
        than the default leaves the features to _features, which refuses device kinds as ever); WIS_IN_ENC_* insists on encoder output."""
        if input_kind != _lib.WIS_IN_MEL_HOST and input_kind not in _ENCODED_KINDS:
            return None
        enc = self._encoded(features)
        if enc is None and input_kind in _ENCODED_KINDS:
            T, d = self._enc_shape
            raise ValueError(f"input_kind {input_kind}: encoder output is a view `encode` returned or a float32 array [batch, {T}, {d}]")
        if enc is not None:
            self._check_open()
        return enc

    def _device_replica(self, device):
        """the least-loaded replica on `device`, counted as in use until _release"""
        with self._pick:
            r = min((x for x in self._replicas if x.device == device), key=lambda x: x.inflight)
            r.inflight += 1
        return r

    def encode(self, features, to_cpu=False, *, input_kind=_lib.WIS_IN_MEL_HOST, device=None):
        """CTranslate2's `Whisper.encode(features, to_cpu=False)`: the encoder's output for every window of `features`, once, for every later
        pass over them - `generate`, `detect_language` and `align` take the result in place of the features and then skip the log-mel and the
        encoder (bit for bit what they compute from the features in a batch of the same size).  to_cpu=False: a device-resident StorageView
        (device "cuda", dtype "float16", shape [B, n_audio_ctx, d_model]) that owns its block of device memory - freed with the last view of it -
        and decodes on its own GPU only; to_cpu=True: the same values as a host view of f32.
        `input_kind` (an extension of this shim): host mel windows, host PCM windows (WIS_IN_PCM_HOST), or - with `device`, the GPU they live on -
        log-mel windows already in device memory (WIS_IN_MEL_DEV, what the seek loop's whole-recording log-mel hands out; `features`: one device
        address or a list of them, one f32 [n_mels][3000] window each, which the caller keeps allocated until the call returns).
        The windows go through the micro-batcher under a key of their own (EncodeKey): concurrent requests share encoder batches of up to
        max_batch windows, as their decodes do.  Windows encoded in one engine call come back as they lie; more than max_batch, or windows that
        shared batches with other requests, are gathered device-to-device into one block."""
        self._check_open()
        kind = int(input_kind)
        if kind == _lib.WIS_IN_MEL_DEV:
            if device is None:
                raise ValueError("encode: features in device memory need `device`")
            rows = [int(features)] if np.isscalar(features) else [int(p) for p in features]
            dev = int(device)
            if not any(r.device == dev for r in self._replicas):
                raise ValueError(f"no replica on device {dev}")
        elif kind in (_lib.WIS_IN_MEL_HOST, _lib.WIS_IN_PCM_HOST):
            a = self._features(features, kind)
            rows = [np.ascontiguousarray(a[b]) for b in range(a.shape[0])]
            with self._pick:      # every window of the call on ONE GPU (the result is one block): the least loaded one
                dev = min(self._replicas, key=lambda x: x.inflight).device if device is None else int(device)
        else:
            raise ValueError(f"encode: input_kind {input_kind} (host mel or PCM windows, or mel windows in device memory; encoder output is not encoded again)")
        if not rows:
            raise ValueError("encode: no windows")
        parts = self._batcher.submit(EncodeKey(kind), rows, affinity=("device", dev))
        for p in parts:
            if p._owner is None:
                p._owner = weakref.ref(self)
        T, d = self._enc_shape
        if parts[0].device != "cuda":      # (a host-only stand-in for the engine)
            out = parts[0] if len(parts) == 1 else StorageView(np.ascontiguousarray(np.concatenate([p.array for p in parts])))
            return out
        row = 2 * T * d
        if all(p._block is parts[0]._block and p._offset == parts[0]._offset + i * row for i, p in enumerate(parts)):
            out = StorageView._on_device(parts[0]._block, [len(parts), T, d], self, parts[0]._offset)      # one engine call: as it lies
        else:
            block = _lib.DevBuf(len(parts) * row, dev)
            lib = _lib.load()
            for i, p in enumerate(parts):
                _lib.check(lib.wis_dev_copy_peer(dev, C.c_void_p(block.ptr.value + i * row), dev, C.c_void_p(p.device_ptr), row))
            out = StorageView._on_device(block, [len(parts), T, d], self)
        return out.to_cpu() if to_cpu else out

    def generate(self, features, prompts, *, asynchronous=False, beam_size=5, patience=1, num_hypotheses=1, length_penalty=1,
                 repetition_penalty=1, no_repeat_ngram_size=0, max_length=448, return_scores=False, return_no_speech_prob=False,
                 max_initial_timestamp_index=50, suppress_blank=True, suppress_tokens=(-1,), sampling_topk=1,
                 sampling_temperature=1, fixed_new_tokens=0, input_kind=_lib.WIS_IN_MEL_HOST, draft_tokens=None, draft_trajectory=None,
                 return_trajectory=False, sampling_seed=None, ragged_prompts=False, phrases=None, return_phrase_mass=False,
                 hotwords=None, hotword_boost=None):
        """`draft_tokens` (one utterance, beam_size 1): the ids of an earlier hypothesis for this audio - wis_generate_draft verifies them in
        multi-row passes and decodes on behind the accepted prefix; the result is the greedy decode of THESE features either way.
        `draft_trajectory` (one utterance, beam_size > 1): `(tok, org)` as an earlier result's `.trajectory` gives it (`return_trajectory=True`) -
        the beam search is replayed along it 16 steps per decoder pass (wis_generate_draft_beam); the result is the beam search of THESE features.
        Timestamps: a Whisper start sequence without <|notimestamps|> (<|startoftranscript|>, language, task - `timestamp_prompt`) decodes
        under Whisper's timestamp rules (first timestamp at most <|0.00|> + max_initial_timestamp_index; None: no cap); drafts cannot be
        combined with them.  A prompt that carries text after its start sequence (a decoder prefix) keeps the plain search.  return_no_speech_prob=True fills
        `no_speech_prob` (P(<|nospeech|>) at <|startoftranscript|>).
        `repetition_penalty` (> 0; 1: off) and `no_repeat_ngram_size` (>= 0; 0: off) are CTranslate2's: every distinct token the search has generated
        for a beam has its logit divided (multiplied when negative) by the penalty, and a token that would complete an n-gram the beam already holds is
        masked (include/wis_hip.h states both).  A bad value, or either option together with a draft, is a ValueError; calls with different values never
        share a device batch.
        Random sampling (`beam_size=1`, `sampling_topk=0` = the whole vocabulary, `sampling_temperature`; a top-k of 2..16 is the engine's, not yet this face's) and `num_hypotheses` are CTranslate2's
        (include/wis_hip.h states the rule): with sampling, `num_hypotheses=n` decodes n independent samples per utterance (results in sample order,
        unsorted) - openai-whisper's temperature fallback is `beam_size=1, num_hypotheses=best_of, sampling_topk=0, sampling_temperature=t`; in a beam
        search it returns the n best finished hypotheses, best first.  `sampling_seed` (an extension of this shim): an int for the call or one per
        utterance; None draws from os.urandom, or from a deterministic counter after `ctranslate2.set_random_seed`.  The same seed gives the same
        samples, whatever else shares the device batch.
        `features` may be what `encode` returned (a device-resident view, a slice or a list of them, or its host copy of shape [B, n_audio_ctx,
        d_model]): the call then starts at the cross-K/V projection (WIS_IN_ENC_DEV / WIS_IN_ENC_HOST in the options' input_kind; `input_kind`
        itself keeps describing host feature arrays).  A device view decodes on its own GPU.
        `ragged_prompts=True` (an extension of this shim; CTranslate2 takes such calls as they are): the prompts of the call may differ in length
        (1 .. 228 tokens each) and still decode in one device batch (wis_generate_ragged) - all with timestamps or none, `max_new_tokens` from the
        longest prompt, no drafts, no `return_trajectory`.  Equal prompts decode exactly as without the keyword.  The setting `batch_ragged_prompts`
        pools every call whose prompts are longer than 16 tokens under one batch key in the same way, so that prompted requests of concurrent callers
        share device batches.
        `phrases=[[token ids], ...]` (an extension of this shim): the search is restricted to the caller's phrase list - every result is one of the
        phrases, scored by the model's log-probabilities renormalised over what the list allows at each step (include/wis_hip.h states the rule);
        `num_hypotheses=n` in a beam search returns the n best phrases, best first (fewer when the search reached fewer).  A phrase holds 1 .. 32 text
        tokens outside the model's suppress lists (weights.build_phrase_trie; a ValueError names the phrase).  Not with timestamps, sampling,
        `fixed_new_tokens` or drafts (ValueError).  Calls share a device batch exactly when their options and their phrase sets are equal.
        `return_phrase_mass=True` (with `phrases`; without: ValueError) fills `phrase_logmass`, one float per returned hypothesis: the log of the share
        of the model's probability that the list allowed, summed over the phrase's steps and its <|endoftext|> - log P_unconstrained(phrase) -
        log P_constrained(phrase), near 0 when the audio says the phrase, strongly negative when the mask forced it (include/wis_hip.h, THE PHRASE
        MASS RULE).  Ids and scores are those of the call without it.
        `hotwords=[[token ids], ...], hotword_boost=b` (an extension of this shim): contextual biasing - free-form decoding goes on, and every token
        that starts an entry of the list, or continues one that the hypothesis' last tokens have begun, has `b` added to its logit once per step
        (include/wis_hip.h, THE HOTWORD RULE).  The scores are log-softmaxes of the BOOSTED rows.  There is no back-off: a hypothesis that leaves an
        entry half-way keeps what it gained.  An entry holds 1 .. 32 text tokens outside the model's suppress lists; `b` is finite and > 0 and has no
        default - calibrate it on the checkpoint in use.  Combines with timestamps, the repetition options, sampling, `num_hypotheses` and prompts of
        any supported length; not with `phrases` or drafts (ValueError).  Calls share a device batch exactly when their options, their hotword lists
        and their boosts are equal."""
        enc = self._encoder_input(features, input_kind)
        if enc is not None:
            n_utt = len(enc[2]) if enc[0] == _lib.WIS_IN_ENC_DEV else enc[1].shape[0]
        opts, mel = self._decode_options(features if enc is None else None, prompts, input_kind=input_kind if enc is None else enc[0], n_utt=1 if enc is None else n_utt,
                                         beam_size=beam_size, patience=patience, num_hypotheses=num_hypotheses,
                                         length_penalty=length_penalty, repetition_penalty=repetition_penalty, no_repeat_ngram_size=no_repeat_ngram_size,
                                         max_length=max_length, return_no_speech_prob=return_no_speech_prob, max_initial_timestamp_index=max_initial_timestamp_index,
                                         suppress_blank=suppress_blank, suppress_default=list(suppress_tokens) == [-1], sampling_topk=sampling_topk,
                                         sampling_temperature=sampling_temperature, fixed_new_tokens=fixed_new_tokens, draft_tokens=draft_tokens,
                                         draft_trajectory=draft_trajectory, return_trajectory=return_trajectory, ragged_prompts=ragged_prompts,
                                         pool_long_prompts=getattr(self, "batch_ragged_prompts", False), phrases=phrases,
                                         return_phrase_mass=return_phrase_mass, hotwords=hotwords, hotword_boost=hotword_boost)
        seeds = _seeds(opts, sampling_seed, len(prompts))
        if enc is not None and enc[0] == _lib.WIS_IN_ENC_DEV:
            # every row carries the block its address points into: the rows themselves keep the device memory allocated until _run_batch has returned
            return self._batcher.submit(opts, [(enc[2][b], [int(t) for t in prompts[b]], seeds[b], enc[3][b]) for b in range(len(prompts))], affinity=("device", enc[1]))
        if enc is not None:
            mel = enc[1]
        return self._batcher.submit(opts, [(np.ascontiguousarray(mel[b]), [int(t) for t in prompts[b]], seeds[b]) for b in range(len(prompts))])

    def _decode_options(self, features, prompts, *, input_kind, n_utt=1, beam_size, patience, num_hypotheses, length_penalty, repetition_penalty, no_repeat_ngram_size,
                        max_length, return_no_speech_prob, max_initial_timestamp_index, suppress_blank, suppress_default, sampling_topk, sampling_temperature,
                        fixed_new_tokens, draft_tokens, draft_trajectory, return_trajectory, ragged_prompts=False, pool_long_prompts=False, phrases=None,
                        return_phrase_mass=False, hotwords=None, hotword_boost=None):
        """Every check of a decode call, for `generate` (features: host arrays, one prompt each) and `generate_from_device` (features None: ONE
        utterance already on the device) -> (its DecodeOptions, the checked host features or None).  The engine's capacity limits are request
        errors (ValueError -> HTTP 400 in wis_hip.server), not internal ones.  ragged_prompts: the prompts may differ in length (the key then
        carries RAGGED_PROMPT).  pool_long_prompts (the setting batch_ragged_prompts): a call whose prompts are longer than SHORT_PROMPT gets the
        pooled key whatever their lengths.  phrases: the call's phrase list -> a ConstrainedOptions; None: the plain record, as it has always been built.
        hotwords / hotword_boost: the call's hotword list and bonus -> a BoostedOptions."""
        drafted = bool(draft_tokens is not None and len(draft_tokens) or draft_trajectory is not None and len(draft_trajectory[0]))
        s_k, s_T, s_n = _check_sampling(beam_size, num_hypotheses, sampling_topk, sampling_temperature, drafted)
        if max(int(beam_size), s_n) > self.max_beam:
            raise ValueError(f"num_hypotheses {s_n} outside 1..{self.max_beam} (setting max_beam: decoder rows per utterance)")
        rep_p, rep_n = _check_repetition(repetition_penalty, no_repeat_ngram_size, drafted)
        mel = None if features is None else self._features(features, input_kind)
        B = int(n_utt) if mel is None else mel.shape[0]      # (features None: utterances already on the device, or encoder output the caller resolved)
        if len(prompts) != B:
            raise ValueError("one prompt per batch item")
        P = len(prompts[0])
        if ragged_prompts and drafted:
            raise ValueError("ragged_prompts cannot be combined with draft_tokens / draft_trajectory")
        if ragged_prompts and return_trajectory:
            raise ValueError("ragged_prompts cannot be combined with return_trajectory")
        ragged = bool(ragged_prompts) and any(len(p) != P for p in prompts)      # (equal prompts: the call is the default one)
        if ragged:
            P = max(len(p) for p in prompts)      # (max_new_tokens comes from the longest prompt of the call)
        elif any(len(p) != P for p in prompts):
            raise ValueError("all prompts must have the same length")
        if not 1 <= int(beam_size) <= self.max_beam:
            raise ValueError(f"beam_size {beam_size} outside 1..{self.max_beam} (setting max_beam; engine ceiling {MAX_BEAM})")
        max_prompt = min(MAX_PROMPT, int((getattr(self, "arch", None) or {}).get("n_text_ctx", 448)) // 2 + 4)
        if not 1 <= P <= max_prompt:
            raise ValueError(f"prompt length {P} outside 1..{max_prompt}")
        if ragged and min(len(p) for p in prompts) < 1:
            raise ValueError(f"prompt length 0 outside 1..{max_prompt}")
        if P > SHORT_PROMPT and drafted:
            raise ValueError(f"a prompt of more than {SHORT_PROMPT} tokens cannot be combined with draft_tokens / draft_trajectory")
        _check_patience(beam_size, patience)
        ts_rows = [timestamp_prompt(p, getattr(self, "special", None)) for p in prompts]
        timestamps = any(ts_rows)
        if timestamps and not all(ts_rows):
            raise ValueError("prompts of one call must all ask for timestamps (a start sequence without <|notimestamps|>) or none")
        if timestamps and drafted:
            raise ValueError("timestamps (a prompt without <|notimestamps|>) cannot be combined with draft_tokens / draft_trajectory")
        if return_no_speech_prob and drafted:
            raise ValueError("return_no_speech_prob cannot be combined with draft_tokens / draft_trajectory")
        draft = None      # (a draft for several utterances, or of another beam size, cannot be followed: a plain call)
        if B == 1 and int(beam_size) == 1 and draft_tokens is not None and len(draft_tokens):
            draft = _Draft(tokens=tuple(int(t) for t in draft_tokens))
        elif B == 1 and int(beam_size) > 1 and draft_trajectory is not None and len(draft_trajectory[0]):
            tok, org = (np.ascontiguousarray(np.asarray(a, np.int32)) for a in draft_trajectory)
            if tok.ndim == 2 and tok.shape[1] == int(beam_size) and tok.shape == org.shape:
                draft = _Draft(trajectory=(tok, org))
        mi = None if max_initial_timestamp_index is None else int(max_initial_timestamp_index)
        pooled = ragged or (bool(pool_long_prompts) and P > SHORT_PROMPT and not drafted and not return_trajectory)
        opts = DecodeOptions(RAGGED_PROMPT if pooled else P, int(beam_size), min(max_length // 2, max_length - P), float(length_penalty), float(patience), bool(suppress_blank),
                             bool(suppress_default), int(fixed_new_tokens), int(input_kind), draft, bool(return_trajectory), timestamps,
                             mi if timestamps else 50, bool(return_no_speech_prob), rep_p, rep_n, s_k, s_T, s_n)
        if return_phrase_mass and phrases is None:
            raise ValueError("return_phrase_mass needs phrases (the mass is that of the call's phrase list)")
        if phrases is not None:
            if timestamps:
                raise ValueError("phrases cannot be combined with timestamps (a start sequence without <|notimestamps|>)")
            if drafted:
                raise ValueError("phrases cannot be combined with draft_tokens / draft_trajectory")
            if s_k != 0:
                raise ValueError("phrases cannot be combined with sampling (sampling_topk 1)")
            if int(fixed_new_tokens) > 0:
                raise ValueError("phrases cannot be combined with fixed_new_tokens")
            trie, digest, longest = _phrase_set(phrases, self.special, getattr(self, "decode_config", None) or {})
            if opts.max_new_tokens < longest + 1:
                raise ValueError(f"max_length {max_length} leaves {opts.max_new_tokens} steps behind a prompt of {P} tokens: the longest phrase needs {longest + 1}")
            opts = ConstrainedOptions(opts._replace(max_new_tokens=longest + 1), trie, digest, bool(return_phrase_mass))
        if hotwords is None and hotword_boost is not None:
            raise ValueError("hotword_boost needs hotwords (the list the boost applies to)")
        if hotwords is not None:
            if phrases is not None:
                raise ValueError("hotwords cannot be combined with phrases (a constrained search has nothing left to bias)")
            if drafted:
                raise ValueError("hotwords cannot be combined with draft_tokens / draft_trajectory")
            if hotword_boost is None:
                raise ValueError("hotwords need a hotword_boost (finite, > 0; there is no default: calibrate it on the checkpoint in use)")
            boost = _check_hotword_boost(hotword_boost)
            trie, digest = _hotword_set(hotwords, self.special, getattr(self, "decode_config", None) or {})
            opts = BoostedOptions(opts, trie, digest, boost)
        return opts, mel

    def load(self, device=None):
        """(utterances queued, device batches running[, on `device`]) in this model's micro-batcher"""
        return self._batcher.load(device)

    def replicas_on(self, device):
        return sum(1 for r in self._replicas if r.device == device)

    def acquire_replica(self):
        """The least-loaded replica, counted as in use until release_replica (a streaming session pins its log-mel front-end
        and its windows to ONE GPU for its lifetime; sessions spread over the replicas like requests do)."""
        return self._acquire()

    def release_replica(self, r):
        self._release(r)

    def replica_on(self, device):
        """A replica that lives on `device` (streaming sessions keep their features on one GPU)."""
        for r in self._replicas:
            if r.device == device:
                return r
        raise ValueError(f"no replica on device {device}")

    def generate_from_device(self, device, mel_device_ptr, prompt, *, beam_size=5, max_length=448, length_penalty=1, patience=1,
                             suppress_blank=True, fixed_new_tokens=0, replica=None, draft_tokens=None, draft_trajectory=None, return_trajectory=False,
                             repetition_penalty=1, no_repeat_ngram_size=0, num_hypotheses=1, sampling_topk=1, sampling_temperature=1, sampling_seed=None,
                             return_scores=False, return_no_speech_prob=False, max_initial_timestamp_index=50, phrases=None,
                             return_phrase_mass=False, hotwords=None, hotword_boost=None):
        """One utterance whose log-mel features ALREADY live in HBM on `device` (f32 [n_mels][3000] at `mel_device_ptr`, e.g. an
        audio.MelStream after finish()): WIS_IN_MEL_DEV - nothing is staged through the host.  Goes through the micro-batcher bound
        to that DEVICE: any replica of the GPU can read the features, so concurrent windows of several streaming sessions on one GPU
        coalesce into one device batch like REST requests do, whatever replica each session holds (round 4 bound a window to the
        session's own replica: sessions pinned to different replicas of a GPU never shared a batch).
        As in `generate`: a start sequence without <|notimestamps|> (`timestamp_prompt`) decodes under Whisper's timestamp rules with
        `max_initial_timestamp_index`, `return_no_speech_prob=True` fills `no_speech_prob`, and drafts cannot be combined with either;
        `return_scores` is accepted for symmetry (the scores are always filled); `phrases` restricts the search to a phrase list and
        `return_phrase_mass` fills `phrase_logmass`, as in `generate`; `hotwords` / `hotword_boost` bias the search toward a list, as in `generate`."""
        # `replica`: the replica the caller holds (a streaming session pins itself to the least-loaded one, acquire_replica: the load
        # accounting that spreads sessions over GPUs); it only has to live on the features' device
        r = replica if replica is not None else self.replica_on(device)
        if r.device != device:
            raise ValueError(f"replica lives on device {r.device}, the features on {device}")
        opts, _ = self._decode_options(None, [prompt], input_kind=_lib.WIS_IN_MEL_DEV, beam_size=beam_size, patience=patience,
                                       num_hypotheses=num_hypotheses, length_penalty=length_penalty, repetition_penalty=repetition_penalty,
                                       no_repeat_ngram_size=no_repeat_ngram_size, max_length=max_length, return_no_speech_prob=return_no_speech_prob,
                                       max_initial_timestamp_index=max_initial_timestamp_index, suppress_blank=suppress_blank, suppress_default=True,
                                       sampling_topk=sampling_topk, sampling_temperature=sampling_temperature, fixed_new_tokens=fixed_new_tokens,
                                       draft_tokens=draft_tokens, draft_trajectory=draft_trajectory, return_trajectory=return_trajectory, phrases=phrases,
                                       return_phrase_mass=return_phrase_mass, hotwords=hotwords, hotword_boost=hotword_boost)
        row = (int(mel_device_ptr), [int(t) for t in prompt], _seeds(opts, sampling_seed, 1)[0])
        return self._batcher.submit(opts, [row], affinity=("device", device))[0]

    def _generate_chunk(self, r, mel, prompts, P, beam, max_new, lp, patience, suppress_blank, suppress_default, fixed_new, kind):
        """One `wis_generate` call on replica r (the caller serialises access to r)."""
        return _generate_chunk(r, mel, prompts, DecodeOptions(P, beam, max_new, lp, patience, suppress_blank, suppress_default, fixed_new, kind))

    def _set_alignment_heads(self, heads):
        """[[layer, head], ...] from the checkpoint (config.json / generation_config.json); None or empty: every head of the upper
        half of the decoder layers (openai-whisper's default)."""
        pairs = np.ascontiguousarray(np.asarray(W.normalize_alignment_heads(heads), np.int32).reshape(-1, 2))
        self.alignment_heads = pairs.tolist()
        for r in self._replicas:
            if r.handle:      # (a host-only stand-in has no engine handle)
                _lib.check(_lib.load().wis_model_set_alignment_heads(r.handle, pairs.ctypes.data_as(C.POINTER(C.c_int32)), len(pairs)))

    def align(self, features, start_sequence, text_tokens, num_frames, *, median_filter_width=7, input_kind=_lib.WIS_IN_MEL_HOST):
        """CTranslate2's `Whisper.align(features, start_sequence, text_tokens, num_frames, *, median_filter_width=7)`: the text
        tokens of every utterance are aligned with its audio frames from the cross-attention of the model's alignment heads
        (dynamic time warping, all on the GPU: csrc/align.hip).  `start_sequence`: the prompt up to the task token (no
        `<|notimestamps|>`: the engine adds it), one for the batch; `text_tokens`: one list per utterance (no eot); `num_frames`:
        mel frames per utterance (an int serves the whole batch).  Returns a list of `WhisperAlignmentResult` with `.alignments`
        [(text_index, time_index)] (time_index counts encoder frames of 20 ms; text_index == len(text) is the eot row) and
        `.text_token_probs`.  Signature and result are restated from CTranslate2's documentation; the real library cannot be
        installed here to pin them against.  `input_kind` is an extension of this shim (host mel windows or host PCM windows, as `generate`
        takes them).  `features` on the device: `StorageView`s are host arrays in this shim; a device
        pointer goes through `align_from_device`.  Encoder output (`encode`'s view, a slice of it, or its host copy) is taken in place of
        the features, as in `generate`."""
        enc = self._encoder_input(features, input_kind)
        if enc is not None and enc[0] == _lib.WIS_IN_ENC_DEV:
            r = self._device_replica(enc[1])
            try:
                return self._align(None, None, _lib.WIS_IN_ENC_DEV, len(enc[2]), start_sequence, text_tokens, num_frames, width=median_filter_width,
                                   dev=(r, enc[2], r.enc_bytes))
            finally:
                self._release(r)
        if enc is not None:
            return self._align(enc[1], _lib.ptr, _lib.WIS_IN_ENC_HOST, enc[1].shape[0], start_sequence, text_tokens, num_frames, width=median_filter_width)
        mel = self._features(features, input_kind)
        return self._align(mel, _lib.ptr, input_kind, mel.shape[0], start_sequence, text_tokens, num_frames, width=median_filter_width)

    def align_from_device(self, device, mel_device_ptr, start_sequence, text_tokens, num_frames, *, median_filter_width=7, replica=None):
        """`align` on one [n_mels][3000] fp32 window already in `device`'s memory (what generate_from_device takes)."""
        r = replica or self.replica_on(device)
        return self._align(None, None, _lib.WIS_IN_MEL_DEV, 1, start_sequence, text_tokens, num_frames, width=median_filter_width, dev=(r, mel_device_ptr))

    def _align(self, mel, to_ptr, kind, B, start_sequence, text_tokens, num_frames, *, width, dev=None):
        if B < 1 or len(text_tokens) != B:
            raise ValueError(f"align: {len(text_tokens)} token lists for a batch of {B}")
        nf = [int(num_frames)] * B if np.isscalar(num_frames) else [int(x) for x in num_frames]
        if len(nf) != B:
            raise ValueError(f"align: {len(nf)} num_frames for a batch of {B}")
        start = np.ascontiguousarray(np.asarray(list(start_sequence), np.int32))
        n_ctx, n_audio = W.N_TEXT_CTX, W.N_AUDIO_CTX
        if int(width) < 1 or int(width) % 2 == 0 or int(width) > 63:
            raise ValueError(f"align: median_filter_width={width} must be odd and within 1..63")
        for t, f in zip(text_tokens, nf):
            if len(start) + 1 + len(t) > n_ctx:
                raise ValueError(f"align: {len(start)} start + 1 + {len(t)} text tokens exceed the decoder's {n_ctx} positions")
            if not 2 <= f <= 2 * n_audio:
                raise ValueError(f"align: num_frames={f} outside 2..{2 * n_audio}")
        i32 = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))
        out = []
        r = dev[0] if dev else self._acquire()
        try:
            with r.lock:
                for s in range(0, B, self.max_batch):
                    toks = [list(map(int, t)) for t in text_tokens[s:s + self.max_batch]]
                    b = len(toks)
                    flat = np.ascontiguousarray(np.asarray([x for t in toks for x in t] or [0], np.int32))
                    lens = np.asarray([len(t) for t in toks], np.int32)
                    frames = np.asarray(nf[s:s + b], np.int32)
                    cap = n_ctx + n_audio
                    pt, pf = np.zeros((b, cap), np.int32), np.zeros((b, cap), np.int32)
                    pl, probs = np.zeros(b, np.int32), np.zeros((b, n_ctx), np.float32)
                    if dev and len(dev) > 2:      # (replica, [address per utterance], bytes per utterance): encoder output on the replica's GPU
                        src = C.c_void_p(_gather_device_rows(r, dev[1][s:s + b], dev[2]))
                    else:
                        src = dev[1] if dev else to_ptr(np.ascontiguousarray(mel[s:s + b]))
                    _lib.check(_lib.load().wis_align(r.handle, src, kind, b, i32(start), len(start), i32(flat), i32(lens), i32(frames), int(width),
                                                     i32(pt), i32(pf), i32(pl), probs.ctypes.data_as(C.POINTER(C.c_float))))
                    for u in range(b):
                        n = int(pl[u])
                        out.append(WhisperAlignmentResult(list(zip(pt[u, :n].tolist(), pf[u, :n].tolist())), probs[u, :lens[u]].tolist()))
        finally:
            if not dev:
                self._release(r)
        return out

    def detect_language(self, features, input_kind=_lib.WIS_IN_MEL_HOST):
        """`features`: host feature windows, or encoder output as `generate` takes it (`encode`'s view, a slice of it, its host copy)."""
        enc = self._encoder_input(features, input_kind)
        ptrs = None
        if enc is not None and enc[0] == _lib.WIS_IN_ENC_DEV:
            input_kind, ptrs, B = _lib.WIS_IN_ENC_DEV, enc[2], len(enc[2])
        else:
            mel = self._features(features, input_kind) if enc is None else enc[1]
            input_kind, B = (input_kind if enc is None else _lib.WIS_IN_ENC_HOST), mel.shape[0]
        n_lang, codes = len(self.special.lang_ids), self.special.lang_codes
        out = []
        r = self._acquire() if ptrs is None else self._device_replica(enc[1])
        try:
            with r.lock:
                for s in range(0, B, self.max_batch):
                    if ptrs is not None:
                        b = len(ptrs[s:s + self.max_batch])
                        src = C.c_void_p(_gather_device_rows(r, ptrs[s:s + b], r.enc_bytes))
                    else:
                        m = np.ascontiguousarray(mel[s:s + self.max_batch])
                        b, src = m.shape[0], _lib.ptr(m)
                    probs = np.zeros((b, n_lang), np.float32)
                    _lib.check(_lib.load().wis_detect_language(r.handle, src, input_kind, b,
                                                               probs.ctypes.data_as(C.POINTER(C.c_float))))
                    for row in probs:
                        order = np.argsort(-row, kind="stable")
                        out.append([(f"<|{codes[i]}|>", float(row[i])) for i in order])
        finally:
            self._release(r)
        return out

    def handoff_state(self, raise_flag_on=None):
        """[(retries, spin_disabled)] per replica (wis_debug_handoff): calls that were repeated in the ticket form because the
        cross-attention's granule hand-off timed out - a request never fails for it.  raise_flag_on = replica index: raise the
        give-up flag there by hand (tests of the repeat path)."""
        out = []
        for i, r in enumerate(self._replicas):
            n, off = C.c_int(0), C.c_int(0)
            with r.lock:
                _lib.check(_lib.load().wis_debug_handoff(r.handle, int(raise_flag_on == i), C.byref(n), C.byref(off)))
            out.append((n.value, bool(off.value)))
        return out

    def last_timing(self, replica=0):
        t = _lib.Timing()
        _lib.check(_lib.load().wis_last_timing(self._replicas[replica].handle, C.byref(t)))
        return t.as_dict()


class models:  # namespace shim: `ctranslate2.models.Whisper`
    Whisper = Whisper
