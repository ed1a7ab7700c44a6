"""-m gpu: Whisper.encode - one encoder pass for every decode of a window.  tiny, seeded weights, the 3.84 s clip's log-mel, fixed_new_tokens 6.

Bars are the ones the suite already sets: encoder rel-L2 <= 2e-3 against WhisperRef.encode (tests/test_gpu_e2e.py::test_encoder_parity) and
check_utterance of tests/test_gpu_prompt.py (score within 3e-3 of the oracle's rescoring, ids compared where the oracle's margin exceeds 0.02).
On one handle and at the same batch size, generate / detect_language / align from encode's view return what they return from the features,
compared with ==: the cross-K/V projection and everything behind it are the same launches on the same values."""
import ctypes as C
import os
import threading

import numpy as np
import pytest
import torch  # noqa: F401  (before libwis_hip.so: one HIP runtime per process)

pytestmark = pytest.mark.gpu
SOT, NO_TIMESTAMPS = 50258, 50363
PROMPT = [SOT, 50259, 50359, NO_TIMESTAMPS]
TS_PROMPT = [SOT, 50259, 50359]
FIXED = 6
E_ARG, E_UNSUPPORTED = -1, -7


def _relerr(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / (np.linalg.norm(b) + 1e-30))


@pytest.fixture(scope="module")
def mel(golden_dir):
    return np.load(os.path.join(golden_dir, "logmel_3sec.npz"))["mel"].astype(np.float32)


@pytest.fixture(scope="module")
def mels(mel):
    """three different windows"""
    return np.ascontiguousarray(np.stack([np.roll(mel, 53 * i, axis=-1) for i in range(3)]))


@pytest.fixture(scope="module")
def rig(mels):
    """(model of max_batch 4, a second one of max_batch 2, oracle, oracle encoder output of the three windows)"""
    from oracle.whisper_ref import WhisperRef
    from wis_hip import ctranslate2 as ct2, weights as W
    w = W.synthetic_weights("tiny", seed=1234, std=0.02, emb_std=0.06, ln_jitter=0.1)
    a = W.arch("tiny")
    model = ct2.Whisper("unused", weights=w, arch=a, max_batch=4, max_beam=5)
    small = ct2.Whisper("unused", weights=w, arch=a, max_batch=2, max_beam=5)
    ref = WhisperRef(w, a["d_model"], a["n_layers"], a["n_heads"])
    yield model, small, ref, ref.encode(mels).numpy()
    model.close()
    small.close()


def _sv(x):
    from wis_hip import ctranslate2 as ct2
    return ct2.StorageView.from_array(np.ascontiguousarray(x))


def _same(a, b):
    assert [r.sequences_ids for r in a] == [r.sequences_ids for r in b], ([r.sequences_ids for r in a], [r.sequences_ids for r in b])
    assert [r.scores for r in a] == [r.scores for r in b], ([r.scores for r in a], [r.scores for r in b])
    assert [r.no_speech_prob for r in a] == [r.no_speech_prob for r in b]


# ---- 1. encoder parity ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 2, 3])
def test_encode_matches_the_oracle(rig, mels, B):
    """B = 3 on the model of max_batch 2: two engine calls gathered into one block"""
    _, small, _, exp = rig
    v = small.encode(_sv(mels[:B]))
    assert v.device == "cuda" and v.device_index == 0 and v.dtype == "float16" and v.shape == [B, 1500, 384]
    host = small.encode(_sv(mels[:B]), to_cpu=True)
    assert host.device == "cpu" and host.array.dtype == np.float32 and host.shape == [B, 1500, 384]
    for i in range(B):
        e = _relerr(host.array[i], exp[i])
        print(f"encode B {B} utterance {i}: rel-L2 {e:.3e}")
        assert e <= 2e-3
    back = np.empty((B, 1500, 384), np.float16)
    from wis_hip import _lib
    _lib.check(_lib.load().wis_dev_d2h(0, _lib.ptr(back), C.c_void_p(v.device_ptr), back.nbytes))
    assert np.array_equal(back.astype(np.float32), host.array)      # to_cpu=True == the device view read back, bit for bit
    assert np.array_equal(np.asarray(v), host.array)


def test_encode_from_pcm(rig, golden_dir):
    from wis_hip import _lib, audio
    model = rig[0]
    pcm, _ = audio.load_audio(os.path.join(golden_dir, "clips", "3sec.flac"))
    x = np.ascontiguousarray(audio.pad_or_trim(pcm)[None])
    m = audio.log_mel_spectrogram(x[0]).numpy()[None]
    r_mel = model.generate(model.encode(_sv(m)), [PROMPT], beam_size=5, fixed_new_tokens=FIXED)
    r_pcm = model.generate(model.encode(x, input_kind=_lib.WIS_IN_PCM_HOST), [PROMPT], beam_size=5, fixed_new_tokens=FIXED)
    assert r_mel[0].sequences_ids == r_pcm[0].sequences_ids


def test_encode_from_windows_in_device_memory(rig, mels):
    """WIS_IN_MEL_DEV (what the seek loop hands in): three windows in three allocations of their own are gathered device-to-device into the
    replica's staging block and encoded as one batch - the same bits as the host form at the same B; one window goes in by pointer"""
    from wis_hip import _lib
    model = rig[0]
    order = [1, 0, 2]
    bufs = [_lib.DevBuf.from_numpy(mels[i], 0) for i in range(3)]
    ptrs = [bufs[i].ptr.value for i in order]
    assert not all(ptrs[i + 1] == ptrs[i] + mels[0].nbytes for i in range(2))      # (not back to back: the gather runs)
    want = model.encode(_sv(mels[order]), to_cpu=True)
    got = model.encode(ptrs, to_cpu=True, input_kind=_lib.WIS_IN_MEL_DEV, device=0)
    assert got.shape == [3, 1500, 384] and np.array_equal(got.array, want.array)
    one = model.encode(ptrs[0], to_cpu=True, input_kind=_lib.WIS_IN_MEL_DEV, device=0)
    assert np.array_equal(one.array, model.encode(_sv(mels[1:2]), to_cpu=True).array)
    with pytest.raises(ValueError, match="device"):
        model.encode(ptrs, input_kind=_lib.WIS_IN_MEL_DEV)
    with pytest.raises(ValueError, match="input_kind"):
        model.encode(ptrs, input_kind=_lib.WIS_IN_PCM_DEV, device=0)
    for b in bufs:
        b.free()


def test_a_temporary_view_outlives_the_call(rig, mels):
    """generate(encode(x)[0:1]): nothing but the call holds the view; the queued row carries the block (tests/test_encode_cpu.py pins that)"""
    model = rig[0]
    want = model.generate(_sv(mels[:1]), [PROMPT], beam_size=5, fixed_new_tokens=FIXED)
    _same(model.generate(model.encode(_sv(mels[:1]))[0:1], [PROMPT], beam_size=5, fixed_new_tokens=FIXED), want)


# ---- 2. the same bits as the one-call form ----------------------------------------------------------------------------------------------
def test_generate_from_view_b1_beam5(rig, mels):
    model = rig[0]
    x = _sv(mels[:1])
    _same(model.generate(model.encode(x), [PROMPT], beam_size=5, fixed_new_tokens=FIXED), model.generate(x, [PROMPT], beam_size=5, fixed_new_tokens=FIXED))


def _long_prompt(P):
    return [50361] + [int(t) for t in np.random.default_rng(P).integers(0, 50257, P - 5)] + PROMPT


@pytest.mark.parametrize("case", ["b3_beam1", "timestamps_nsp", "sampled", "long_prompt", "host_round_trip"])
def test_generate_from_view_equals_generate_from_features(rig, mels, case):
    from wis_hip import ctranslate2 as ct2
    model = rig[0]
    B, prompt, kw = 1, PROMPT, dict(beam_size=5, fixed_new_tokens=FIXED)
    if case == "b3_beam1":
        B, kw = 3, dict(beam_size=1, fixed_new_tokens=FIXED)
    elif case == "timestamps_nsp":
        prompt, kw = TS_PROMPT, dict(beam_size=5, fixed_new_tokens=FIXED, return_no_speech_prob=True)
    elif case == "sampled":
        kw = dict(beam_size=1, sampling_topk=0, num_hypotheses=3, sampling_temperature=0.7, sampling_seed=77, fixed_new_tokens=FIXED)
    elif case == "long_prompt":
        prompt = _long_prompt(33)
    x = _sv(mels[:B])
    v = model.encode(x)
    if case == "host_round_trip":
        v = ct2.StorageView.from_array(np.asarray(model.encode(x, to_cpu=True)))
    got, want = model.generate(v, [prompt] * B, **kw), model.generate(x, [prompt] * B, **kw)
    _same(got, want)
    if case == "timestamps_nsp":
        assert 0.0 < got[0].no_speech_prob < 1.0
    if case == "sampled":
        assert len(got[0].sequences_ids) == 3


def test_detect_language_and_align_from_view(rig, mels):
    model = rig[0]
    x = _sv(mels[:2])
    v = model.encode(x)
    assert model.detect_language(v) == model.detect_language(x)
    assert model.detect_language(v.to_cpu()) == model.detect_language(x)
    text = [[1000 + i for i in range(9)], [2000 + i for i in range(5)]]
    a, b = model.align(v, TS_PROMPT, text, [384, 3000]), model.align(x, TS_PROMPT, text, [384, 3000])
    assert [r.alignments for r in a] == [r.alignments for r in b] and [r.text_token_probs for r in a] == [r.text_token_probs for r in b]
    assert len(a[0].text_token_probs) == 9 and len(a[1].text_token_probs) == 5


def test_slice_of_a_view(rig, mels):
    """view[1:2] of a B = 2 encode is utterance 1's encoder output: through a B = 2 call (slices 0 and 1 as a list) it decodes to the B = 2
    generate(x) result, and the slice is a pointer into the same block"""
    from test_gpu_prompt import check_utterance
    model, _, ref, exp = rig
    x = _sv(mels[:2])
    v = model.encode(x)
    s = v[1:2]
    assert s.shape == [1, 1500, 384] and s.device_ptr == v.device_ptr + 1500 * 384 * 2 and s._block is v._block
    want = model.generate(x, [PROMPT] * 2, beam_size=5, fixed_new_tokens=FIXED)
    _same(model.generate([v[0:1], s], [PROMPT] * 2, beam_size=5, fixed_new_tokens=FIXED), want)
    del v      # the slice keeps the block alive
    alone = model.generate(s, [PROMPT], beam_size=5, fixed_new_tokens=FIXED)[0]
    # decoded alone (B = 1) the cross-K/V GEMM tiles differ from the B = 2 call's, so bits are not promised: the oracle's bars, ids where its margin forces them
    _, forced, _ = check_utterance(ref, exp[1], PROMPT, alone.sequences_ids[0], alone.scores[0], 5, fixed_new=FIXED, tag="slice [1:2] alone")
    if forced:
        assert alone.sequences_ids == want[1].sequences_ids


# ---- 3. views from separate calls in one device batch -----------------------------------------------------------------------------------
def test_views_from_separate_calls_share_a_device_batch(rig, mels):
    from test_gpu_prompt import check_utterance
    model, _, ref, exp = rig
    views = [model.encode(_sv(mels[i:i + 1])) for i in range(3)]
    want = model.generate(_sv(mels), [PROMPT] * 3, beam_size=5, fixed_new_tokens=FIXED)
    got = model.generate(views, [PROMPT] * 3, beam_size=5, fixed_new_tokens=FIXED)
    out = [None] * 3

    def one(i):
        out[i] = model.generate(views[i], [PROMPT], beam_size=5, fixed_new_tokens=FIXED)[0]
    th = [threading.Thread(target=one, args=(i,)) for i in range(3)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    for name, res in (("one call", got), ("three threads", out)):
        for i in range(3):
            same, forced, _ = check_utterance(ref, exp[i], PROMPT, res[i].sequences_ids[0], res[i].scores[0], 5, fixed_new=FIXED, tag=f"{name}, utterance {i}")
            if forced:
                assert res[i].sequences_ids == want[i].sequences_ids


# ---- 4. the block is the caller's -------------------------------------------------------------------------------------------------------
def test_a_view_survives_other_calls(rig, mels):
    model = rig[0]
    x = _sv(mels[:1])
    short_before = [model.generate(_sv(mels[2:3]), [PROMPT], beam_size=k, fixed_new_tokens=FIXED)[0] for k in (1, 5)]
    want = model.generate(x, [PROMPT], beam_size=5, fixed_new_tokens=FIXED)
    v = model.encode(x)
    model.generate(_sv(mels[1:3]), [_long_prompt(33)] * 2, beam_size=5, fixed_new_tokens=FIXED)      # other audio, another route, through the handle's own buffers
    model.detect_language(_sv(mels[2:3]))
    _same(model.generate(v, [PROMPT], beam_size=5, fixed_new_tokens=FIXED), want)
    short_after = [model.generate(_sv(mels[2:3]), [PROMPT], beam_size=k, fixed_new_tokens=FIXED)[0] for k in (1, 5)]
    _same(short_before, short_after)
    model.generate(v, [PROMPT], beam_size=5, fixed_new_tokens=FIXED)
    t = model.last_timing()
    assert t["logmel_ms"] == 0.0 and t["encoder_ms"] == 0.0 and t["crosskv_ms"] > 0.0
    model.generate(x, [PROMPT], beam_size=5, fixed_new_tokens=FIXED)
    assert model.last_timing()["encoder_ms"] > 0.0


# ---- 5. refusals ------------------------------------------------------------------------------------------------------------------------
def test_refusals(rig, mels):
    from wis_hip import _lib, ctranslate2 as ct2, weights as W
    model, small = rig[0], rig[1]
    calls = []
    real = ct2._generate_chunk
    ct2._generate_chunk = lambda *a, **k: (calls.append(1), real(*a, **k))[1]
    try:
        v = model.encode(_sv(mels[:1]))
        base = ct2.Whisper("unused", weights=W.synthetic_weights("base", seed=1, std=0.02), arch=W.arch("base"), max_batch=1, max_beam=1)
        with pytest.raises(ValueError, match="d_model 512"):
            base.generate(v, [PROMPT], beam_size=1)                       # a view of another model's width
        with pytest.raises(ValueError):
            model.generate(_sv(np.zeros((1, 1500, 385), np.float32)), [PROMPT], beam_size=1)      # a wrong shape
        with pytest.raises(ValueError, match="one prompt per batch item"):
            model.generate(v, [PROMPT] * 2, beam_size=1)
        gone = ct2.Whisper("unused", weights=W.synthetic_weights("tiny", seed=2, std=0.02), arch=W.arch("tiny"), max_batch=1, max_beam=1)
        gv = gone.encode(_sv(mels[:1]))
        gone.close()
        with pytest.raises(ValueError, match="closed"):
            model.generate(gv, [PROMPT], beam_size=1)                     # a view from a closed model
        with pytest.raises(ValueError, match="closed"):
            gone.generate(v, [PROMPT], beam_size=1)
        with pytest.raises(ValueError, match="closed"):
            gone.encode(_sv(mels[:1]))
        base.close()
    finally:
        ct2._generate_chunk = real
    assert not calls
    # the engine's own refusals
    lib, h = _lib.load(), small._replicas[0].handle
    err = lambda: (lib.wis_last_error() or b"").decode()
    m1 = np.ascontiguousarray(mels[:1])
    blk = _lib.DevBuf(3 * 1500 * 384 * 2, 0)
    assert lib.wis_encode(h, _lib.ptr(m1), _lib.WIS_IN_MEL_HOST, 1, None, None) == E_ARG and "enc_out_dev_f16" in err()
    assert lib.wis_encode(h, None, _lib.WIS_IN_MEL_HOST, 1, blk.ptr, None) == E_ARG and "input" in err()
    assert lib.wis_encode(h, _lib.ptr(np.ascontiguousarray(mels)), _lib.WIS_IN_MEL_HOST, 3, blk.ptr, None) == E_ARG and "B = 3" in err()
    assert lib.wis_encode(h, blk.ptr, _lib.WIS_IN_ENC_DEV, 1, blk.ptr, None) == E_UNSUPPORTED and "input_kind" in err()
    assert lib.wis_encode(h, _lib.ptr(m1), 17, 1, blk.ptr, None) == E_ARG and "input_kind" in err()
    probs = np.zeros((3, 99), np.float32)
    assert lib.wis_detect_language(h, blk.ptr, _lib.WIS_IN_ENC_DEV, 3, probs.ctypes.data_as(C.POINTER(C.c_float))) != 0 and "batch 3" in err()      # B over the handle's batch
    assert lib.wis_detect_language(h, None, _lib.WIS_IN_ENC_DEV, 1, probs.ctypes.data_as(C.POINTER(C.c_float))) == E_ARG      # a null block
    # ... and the handle is as usable as before
    assert lib.wis_encode(h, _lib.ptr(m1), _lib.WIS_IN_MEL_HOST, 1, blk.ptr, None) == 0
    blk.free()


# ---- 6. do_whisper ----------------------------------------------------------------------------------------------------------------------
class _Vocab:
    """stand-in vocabulary (no tokenizer.json ships with the repository): every text id is a word of its own"""
    has_vocabulary, all_special_ids = True, []
    decode = staticmethod(lambda ids: "".join(f" w{int(t)}" for t in ids if int(t) < 50257))


@pytest.fixture(scope="module")
def models():
    from wis_hip.settings import APISettings
    from wis_hip.whisper import WhisperModels
    s = APISettings()
    s.whisper_model_path = "synthetic:{size}"
    s.fixed_new_tokens = 8
    m = WhisperModels(s, device_index=[0])
    m.get("tiny")
    m.tokenizers["tiny"] = _Vocab()
    yield m
    m.get("tiny").close()


REQUESTS = {
    "a_detect": dict(detect_language=True, force_language=None),
    "b_words": dict(word_timestamps=True),
    "c_detect_translate_words": dict(detect_language=True, force_language=None, translate=True, word_timestamps=True),
    "d_fallback": dict(temperatures=(0.0, 0.4, 0.8), best_of=2, logprob_threshold=100.0, timestamps=True),
    "e_plain": dict(),
}


def _record(r):
    return dict(language=r[0], text=r[1], translation=r[3], tokens=r.tokens, translation_tokens=r.translation_tokens, segments=r.segments,
                fallback=r.fallback, seek=r.seek)


def _spy_encode(fn):
    from wis_hip import ctranslate2 as ct2
    n, real = [], ct2._encode_chunk
    ct2._encode_chunk = lambda *a, **k: (n.append(1), real(*a, **k))[1]
    try:
        return fn(), len(n)
    finally:
        ct2._encode_chunk = real


@pytest.mark.parametrize("name", sorted(REQUESTS))
def test_do_whisper_encode_once(models, golden_dir, name):
    from wis_hip import ctranslate2 as ct2
    from wis_hip.whisper import do_whisper
    clip = os.path.join(golden_dir, "clips", "3sec.flac")
    kw = dict(dict(detect_language=False, force_language="en"), **REQUESTS[name])
    det, force = kw.pop("detect_language"), kw.pop("force_language")
    out = {}
    for on in (False, True):
        models.settings.encode_once = on
        ct2.set_random_seed(5)      # the fallback's sampled temperatures draw the same seeds on both sides
        try:
            r, n = _spy_encode(lambda: do_whisper(clip, "tiny", 5, "transcribe", det, force, models=models, **kw))
        finally:
            models.settings.encode_once = False
            ct2.set_random_seed(None)
        out[on] = _record(r)
        assert n == (1 if on and name != "e_plain" else 0), (name, on, n)
    assert out[True] == out[False]
    if name == "d_fallback":
        assert out[True]["fallback"]["attempts"] == 3
    if "words" in name:
        assert sum(len(sg["words"]) for sg in out[True]["segments"]) > 0


def test_do_whisper_seek_encode_once(models):
    from wis_hip.whisper import do_whisper
    rng = np.random.default_rng(65)
    t = np.arange(int(16000 * 65.0))
    pcm = (0.2 * np.sin(2 * np.pi * 220.0 * t / 16000.0) * (1.0 + 0.5 * np.sin(2 * np.pi * 0.7 * t / 16000.0)) + 0.02 * rng.standard_normal(t.shape[0])).astype(np.float32)
    out, passes = {}, {}
    for on in (False, True):
        models.settings.encode_once = on
        try:
            r, passes[on] = _spy_encode(lambda: do_whisper(pcm, "tiny", 5, "transcribe", False, "en", models=models, long_form="seek", word_timestamps=True,
                                                           no_speech_threshold=1e30))
        finally:
            models.settings.encode_once = False
        out[on] = _record(r)
    assert out[True] == out[False]
    assert passes[False] == 0 and passes[True] == len(out[True]["seek"]) >= 3      # one encoder pass per window
