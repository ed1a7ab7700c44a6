"""Whisper.encode and the encode_once setting over the fake engine (tools/fake_engine_app.py: everything but the engine is real): the call
sequence of do_whisper with the setting on and off, how encoder output is recognised, slices and lifetime of views, the batcher's encode key."""
import os
import sys
import threading

import numpy as np
import pytest

from wis_hip import _lib, ctranslate2 as ct2

ENC = (_lib.WIS_IN_ENC_DEV, _lib.WIS_IN_ENC_HOST)


class _Tok:
    has_vocabulary, all_special_ids = True, []
    decode = staticmethod(lambda ids: "".join(f" w{int(t)}" for t in ids if int(t) < 50257))


@pytest.fixture()
def fake(golden_dir, monkeypatch, request):
    """(models, model, calls): calls = [("encode" | "generate" | "detect" | "align", input kind, B)] in order.  Parametrised indirectly with a
    number: that many replicas on the one fake GPU (default: the fake engine's four)."""
    if getattr(request, "param", None):
        monkeypatch.setenv("WIS_FAKE_REPLICAS", str(request.param))
    sys.path.insert(0, os.path.join(os.path.dirname(golden_dir), "..", "tools"))
    import fake_engine_app
    monkeypatch.setenv("WIS_FAKE_MS", "1")
    monkeypatch.setenv("WIS_FAKE_MS_PER_UTT", "0")
    saved = ct2._generate_chunk, ct2._encode_chunk
    app = fake_engine_app.create_app()
    models = app.state.wis["models"]
    models.tokenizers["large"] = _Tok()
    model = models.get("large")
    calls = []
    gen, enc = ct2._generate_chunk, ct2._encode_chunk

    def spy_gen(r, mel, prompts, opts, **kw):
        calls.append(("generate", opts.input_kind, len(prompts)))
        return gen(r, mel, prompts, opts, **kw)

    def spy_enc(r, features, input_kind, **kw):
        calls.append(("encode", input_kind, features.shape[0]))
        return enc(r, features, input_kind, **kw)

    def kind_of(feats, kw):
        e = model._encoder_input(feats, kw.get("input_kind", _lib.WIS_IN_MEL_HOST))
        return kw.get("input_kind", _lib.WIS_IN_MEL_HOST) if e is None else e[0]
    model.detect_language = lambda feats, **kw: (calls.append(("detect", kind_of(feats, kw), feats.shape[0])), [[("<|en|>", 1.0)]])[1]
    model.align = lambda feats, start, texts, frames, **kw: (calls.append(("align", kind_of(feats, kw), len(texts))),
                                                             [ct2.WhisperAlignmentResult([(i, 5 * i) for i in range(len(t) + 1)], [0.5] * len(t)) for t in texts])[1]
    ct2._generate_chunk, ct2._encode_chunk = spy_gen, spy_enc
    try:
        yield models, model, calls
    finally:
        ct2._generate_chunk, ct2._encode_chunk = saved
        model.close()


REQUESTS = {
    "a": dict(detect_language=True, force_language=None),
    "b": dict(word_timestamps=True),
    "c": dict(detect_language=True, force_language=None, translate=True, word_timestamps=True),
    "d": dict(temperatures=(0.0, 0.4, 0.8), best_of=2, logprob_threshold=100.0),
    "e": dict(),
}


def _run(models, golden_dir, name, on):
    from wis_hip.whisper import do_whisper
    kw = dict(dict(detect_language=False, force_language="en"), **REQUESTS[name])
    det, force = kw.pop("detect_language"), kw.pop("force_language")
    models.settings.encode_once = on
    try:
        return do_whisper(os.path.join(golden_dir, "clips", "3sec.flac"), "large", 5, "transcribe", det, force, models=models, **kw)
    finally:
        models.settings.encode_once = False


@pytest.mark.parametrize("name", sorted(REQUESTS))
def test_do_whisper_call_sequence(fake, golden_dir, name):
    models, model, calls = fake
    off = _run(models, golden_dir, name, False)
    rec_off = list(calls)
    del calls[:]
    on = _run(models, golden_dir, name, True)
    rec_on = list(calls)
    assert not any(c[0] == "encode" for c in rec_off) and not any(c[1] in ENC for c in rec_off)      # off: the parent's records
    if name == "e":
        assert rec_on == rec_off and len(rec_on) == 1
    else:
        assert rec_on[0] == ("encode", rec_off[0][1], 1) and sum(c[0] == "encode" for c in rec_on) == 1      # one encode per window group
        assert [c[0] for c in rec_on[1:]] == [c[0] for c in rec_off] and all(c[1] in ENC for c in rec_on[1:])
        assert [c[2] for c in rec_on[1:]] == [c[2] for c in rec_off]
    assert (on[0], on[1], on[3], on.tokens, on.segments) == (off[0], off[1], off[3], off.tokens, off.segments)
    assert {"a": 2, "b": 2, "c": 4, "d": 3, "e": 1}[name] == len(rec_off)      # the passes the setting folds into one encoder pass


def test_shape_recognition(fake):
    _, model, _ = fake
    T, d = model._enc_shape
    assert (T, d) == (1500, 1280)
    assert model._encoded(np.zeros((2, 80, 3000), np.float32)) is None
    assert model._encoded(ct2.StorageView.from_array(np.zeros((1, 128, 3000), np.float32))) is None
    kind, a = model._encoded(np.zeros((2, T, d), np.float32))
    assert kind == _lib.WIS_IN_ENC_HOST and a.shape == (2, T, d)
    assert model._encoded(np.zeros((2, T, d + 1), np.float32)) is None
    with pytest.raises(ValueError, match="features must be"):
        model.generate(np.zeros((1, T, d + 1), np.float32), [[50258]], beam_size=1)
    with pytest.raises(ValueError, match="host arrays"):      # input_kind keeps its meaning for host arrays
        model.generate(np.zeros((1, 80, 3000), np.float32), [[50258]], beam_size=1, input_kind=_lib.WIS_IN_MEL_DEV)
    with pytest.raises(ValueError, match="encoder output"):
        model.generate(np.zeros((1, 80, 3000), np.float32), [[50258]], beam_size=1, input_kind=_lib.WIS_IN_ENC_HOST)
    with pytest.raises(ValueError, match="not encoded again"):
        model.encode(np.zeros((1, T, d), np.float32), input_kind=_lib.WIS_IN_ENC_HOST)
    opts, _ = model._decode_options(None, [[50258]] * 2, input_kind=_lib.WIS_IN_ENC_HOST, n_utt=2, beam_size=1, patience=1, num_hypotheses=1, length_penalty=1,
                                    repetition_penalty=1, no_repeat_ngram_size=0, max_length=448, return_no_speech_prob=False, max_initial_timestamp_index=50,
                                    suppress_blank=True, suppress_default=True, sampling_topk=1, sampling_temperature=1, fixed_new_tokens=0, draft_tokens=None,
                                    draft_trajectory=None, return_trajectory=False)
    assert opts.input_kind == _lib.WIS_IN_ENC_HOST and opts._fields == ct2.DecodeOptions._fields


class _Block:
    """a stand-in for _lib.DevBuf: an address and a record of its release"""
    freed = 0

    def __init__(self, device=0):
        self.device, self.ptr = device, type("P", (), {"value": 0x10000, "__bool__": lambda s: True})()

    def __del__(self):
        _Block.freed += 1


def test_slices_and_lifetime_of_device_views(fake):
    _, model, _ = fake
    T, d = model._enc_shape
    _Block.freed = 0
    v = ct2.StorageView._on_device(_Block(), [3, T, d], model)
    assert (v.device, v.device_index, v.dtype, v.shape, len(v)) == ("cuda", 0, "float16", [3, T, d], 3)
    s = v[1:3]
    assert s.shape == [2, T, d] and s.device_ptr == v.device_ptr + 2 * T * d and s._block is v._block
    assert s[1:2].device_ptr == v.device_ptr + 2 * 2 * T * d and v[-1].device_ptr == s[1:2].device_ptr and v[5:9].shape == [0, T, d]
    with pytest.raises(ValueError):
        v[::2]
    kind, dev, ptrs, blocks = model._encoded([v[0:1], s])
    assert blocks == [v._block] * 3 and kind == _lib.WIS_IN_ENC_DEV and dev == 0 and ptrs == [v.device_ptr + i * 2 * T * d for i in range(3)]
    del v, blocks
    assert _Block.freed == 0 and s.device_ptr      # a slice keeps the block alive
    del s
    assert _Block.freed == 1
    # refusals that reach no engine call: another width, another device, a closed model
    with pytest.raises(ValueError, match="d_model 1280"):
        model._encoded(ct2.StorageView._on_device(_Block(), [1, T, 384], model))
    with pytest.raises(ValueError, match="no replica"):
        model._encoded(ct2.StorageView._on_device(_Block(device=3), [1, T, d], model))
    with pytest.raises(ValueError, match="mixed"):
        model._encoded([ct2.StorageView._on_device(_Block(), [1, T, d], model), ct2.StorageView(np.zeros((1, T, d), np.float32))])


def test_encode_key_and_capacity(fake):
    k = ct2.EncodeKey(_lib.WIS_IN_MEL_HOST)
    assert k == ct2.EncodeKey(0) and k != ct2.EncodeKey(_lib.WIS_IN_PCM_HOST) and hash(k) == hash(ct2.EncodeKey(0))
    for o in (ct2.DecodeOptions(4, 5, 224), ct2.DecodeOptions(0, 0, 0), (0,), 0):
        assert k != o and o != k and not (k == o)      # the encode key never equals a decode key
    assert ct2._capacity(8, k) == 8 and ct2._capacity(2, k) == 2 and ct2._capacity(8, ct2.DecodeOptions(4, 5, 224)) == 8


def test_a_queued_decode_row_owns_its_block(fake):
    """generate(device view) queues (address, prompt, seed, block): the row itself keeps the device memory allocated until the batch has run,
    whatever the caller's frames still reference"""
    _, model, _ = fake
    T, d = model._enc_shape
    _Block.freed = 0
    seen = []
    real = model._batcher.submit

    def submit(key, rows, affinity=None):
        seen.append((key, [tuple(r) for r in rows], affinity))
        return [ct2.WhisperGenerationResult([[1]], [0.0]) for _ in rows]
    model._batcher.submit = submit
    try:
        model.generate(ct2.StorageView._on_device(_Block(), [2, T, d], model)[0:2], [[50258]] * 2, beam_size=1)
    finally:
        model._batcher.submit = real
    (key, rows, affinity), = seen
    assert key.input_kind == _lib.WIS_IN_ENC_DEV and affinity == ("device", 0)
    assert [r[0] for r in rows] == [0x10000, 0x10000 + 2 * T * d] and all(isinstance(r[3], _Block) and r[3] is rows[0][3] for r in rows)
    assert _Block.freed == 0      # (the recorded rows are the only reference left)
    del seen[:], rows, key
    assert _Block.freed == 1


@pytest.mark.parametrize("fake", [1], indirect=True)
def test_two_concurrent_encode_calls_share_one_encode_chunk(fake):
    """One replica, held by a generate call: two encode calls arrive meanwhile and are taken together - ONE _encode_chunk of B = 2, through
    Whisper.encode, the batcher's EncodeKey and _run_batch, and every caller gets its own [1, T, d] window back."""
    _, model, calls = fake
    T, d = model._enc_shape
    gate = threading.Event()
    spy_gen, spy_enc = ct2._generate_chunk, ct2._encode_chunk
    ct2._generate_chunk = lambda *a, **k: (gate.wait(10), spy_gen(*a, **k))[1]

    def tagged(r, features, input_kind, **kw):      # the stand-in's zeros, tagged with each window's first value: whose window is whose
        v = spy_enc(r, features, input_kind, **kw)
        v.array[:] = features.reshape(features.shape[0], -1)[:, :1, None]
        return v
    ct2._encode_chunk = tagged
    out = {}
    mel = lambda x: np.full((1, 80, 3000), float(x), np.float32)
    try:
        holder = threading.Thread(target=lambda: model.generate(mel(0), [[50258, 50259, 50359, 50363]], beam_size=1))
        holder.start()
        while model.load()[1] < 1:
            threading.Event().wait(0.001)
        ts = [threading.Thread(target=lambda i=i: out.__setitem__(i, model.encode(mel(i)))) for i in (1, 2)]
        for t in ts:
            t.start()
        while model.load()[0] < 2:
            threading.Event().wait(0.001)
        gate.set()
        for t in ts + [holder]:
            t.join()
    finally:
        gate.set()
        ct2._generate_chunk, ct2._encode_chunk = spy_gen, spy_enc
    assert [c for c in calls if c[0] == "encode"] == [("encode", _lib.WIS_IN_MEL_HOST, 2)]
    for i in (1, 2):
        assert out[i].shape == [1, T, d] and float(out[i].array.min()) == float(out[i].array.max()) == float(i)
        assert out[i]._owner() is model
