"""not gpu: Whisper timestamps on the host - the CPU statement of the rules (tests/ts_ref.py) against transformers'
WhisperTimeStampLogitsProcessor, segment splitting, what Whisper.generate asks the engine for, and the REST surface."""
import asyncio
import io
import wave

import numpy as np
import pytest
import torch

from ts_ref import EOT, NO_TIMESTAMPS, TB, V, apply_ts_rules, grammar_errors, hf_processor

PROMPT = [50258, 50259, 50359]


def _random_history(rng):
    """Histories that hit every branch: empty, one timestamp, text then a timestamp, a pair, text only, mixed."""
    kind = rng.integers(0, 6)
    t0 = TB + int(rng.integers(0, 40))
    text = [int(x) for x in rng.integers(0, EOT, size=int(rng.integers(1, 4)))]
    if kind == 0:
        return []
    if kind == 1:
        return [t0]
    if kind == 2:
        return [t0] + text + [t0 + int(rng.integers(0, 30))]
    if kind == 3:
        t1 = t0 + int(rng.integers(0, 30))
        return [t0] + text + [t1, t1 + int(rng.integers(0, 3))]
    if kind == 4:
        return text
    return [t0] + text + [t0 + 10, t0 + 11] + text


@pytest.mark.parametrize("max_init", [50, 0, 3, None])
def test_rules_match_transformers(max_init):
    rng = np.random.default_rng(7 + (max_init or 99))
    stats = {}
    hf = hf_processor(max_init, begin_index=len(PROMPT))
    checked = 0
    for trial in range(60):
        hist = _random_history(rng)
        lg = torch.from_numpy(rng.standard_normal((1, V)).astype(np.float32) * 2.0)
        lg[0, TB:] += float(rng.uniform(-5.0, 2.0))          # moves the decision both ways
        ours, margins = apply_ts_rules(lg, [hist], max_init, stats)
        ids = torch.tensor([PROMPT + hist])
        ref = hf(ids, lg.clone())
        if margins[0] < 1e-4:
            continue
        checked += 1
        assert torch.equal(torch.isinf(ours), torch.isinf(ref)), (trial, hist)
        fin = torch.isfinite(ours)
        assert torch.equal(ours[fin], ref[fin])
    assert checked >= 50
    want = {"after_pair", "open_segment", "monotonic", "monotonic_repeat_allowed", "decision_timestamp", "decision_text"}
    if max_init is not None:
        want.add("initial_cap")
    assert want <= set(stats), stats


def test_grammar_checker():
    assert grammar_errors([TB, 1, 2, TB + 5, TB + 5, 3, TB + 9]) == []
    assert grammar_errors([TB + 2, 7, TB + 4]) == []
    assert grammar_errors([7, TB]) != []                       # first token text
    assert grammar_errors([TB + 60, 7]) != []                  # beyond the initial cap
    assert grammar_errors([TB + 5, 7, TB + 3, TB + 3]) != []   # decreasing
    assert grammar_errors([TB, 7, TB + 3, 8]) != []            # unpaired inside the sequence
    assert grammar_errors([TB, 7, TB + 3, 50300]) == []        # ... but a special id may follow (only [0, EOT) is masked)
    assert grammar_errors([TB, 7, TB + 3, TB + 3, TB + 4]) != []


class _IdTok:
    @staticmethod
    def decode(ids):
        return " ".join(str(int(t)) for t in ids)


def test_segments_from_tokens():
    from wis_hip.whisper import segments_from_tokens
    T = lambda s: TB + int(round(s / 0.02))        # noqa: E731
    # pairs close and open segments; a single timestamp before EOT closes the last one
    ids = [T(0.0), 11, 12, T(1.5), T(1.5), 13, T(2.4), EOT]
    assert segments_from_tokens(ids, _IdTok) == [{"start": 0.0, "end": 1.5, "text": "11 12"}, {"start": 1.5, "end": 2.4, "text": "13"}]
    # an unclosed tail ends at the window's duration
    ids = [T(0.0), 11, T(1.0), T(1.2), 12, 13]
    assert segments_from_tokens(ids, _IdTok, offset=10.0, duration=3.0) == [{"start": 10.0, "end": 11.0, "text": "11"},
                                                                             {"start": 11.2, "end": 13.0, "text": "12 13"}]
    # no consecutive pair: one segment to the last timestamp ...
    assert segments_from_tokens([T(0.4), 11, 12, T(2.0)], _IdTok) == [{"start": 0.0, "end": 2.0, "text": "11 12"}]
    # ... or to the duration when there is none beyond <|0.00|>
    assert segments_from_tokens([T(0.0), 11], _IdTok, duration=4.0) == [{"start": 0.0, "end": 4.0, "text": "11"}]
    assert segments_from_tokens([], _IdTok) == []
    # a pair at the very end closes the last segment and leaves nothing open
    assert segments_from_tokens([T(0.0), 11, T(0.8), T(0.8)], _IdTok) == [{"start": 0.0, "end": 0.8, "text": "11"}]


def _stub_whisper(monkeypatch):
    from wis_hip import ctranslate2 as ct2
    calls = []

    def fake_chunk(r, mel, prompts, opts, device_ptr=None, seeds=None):
        calls.append(dict(B=len(prompts), timestamps=opts.timestamps, mi=opts.max_initial_timestamp_index, nsp=opts.no_speech_prob,
                          draft=opts.draft and opts.draft.tokens))
        return [ct2.WhisperGenerationResult([[TB, 5, TB + 3]], [0.0], 0.25 if opts.no_speech_prob else 0.0) for _ in prompts]
    monkeypatch.setattr(ct2, "_generate_chunk", fake_chunk)

    class R:
        device, lock = 0, __import__("threading").Lock()
    m = ct2.Whisper.__new__(ct2.Whisper)
    m.max_batch, m.max_beam = 8, 5
    keys = []
    m._batcher = type("B", (), {"submit": lambda self, key, rows: (keys.append(key), ct2._run_batch(R(), key, rows))[1]})()
    return m, calls, keys


def test_generate_sets_timestamp_options_from_the_prompt(monkeypatch):
    from wis_hip import ctranslate2 as ct2
    m, calls, keys = _stub_whisper(monkeypatch)
    feats = ct2.StorageView.from_array(np.zeros((1, 80, 3000), np.float32))
    m.generate(feats, [PROMPT + [NO_TIMESTAMPS]], beam_size=1)
    assert calls[-1]["timestamps"] is False and calls[-1]["nsp"] is False
    m.generate(feats, [PROMPT], beam_size=1)
    assert calls[-1]["timestamps"] is True and calls[-1]["mi"] == 50
    m.generate(feats, [PROMPT], beam_size=1, max_initial_timestamp_index=None)
    assert calls[-1]["timestamps"] is True and calls[-1]["mi"] is None
    r = m.generate(feats, [PROMPT + [NO_TIMESTAMPS]], beam_size=1, return_no_speech_prob=True)
    assert calls[-1]["nsp"] is True and calls[-1]["timestamps"] is False and r[0].no_speech_prob == 0.25
    # the micro-batcher never mixes these in one device batch: every option set has a key of its own
    assert len(set(keys)) == len(keys) == 4
    todays = ct2.DecodeOptions(prompt_len=4, beam_size=1, max_new_tokens=224, length_penalty=1.0, patience=1.0, suppress_blank=True, suppress_default=True,
                       fixed_new_tokens=0, input_kind=0, draft=None, return_trajectory=False, timestamps=False,
                       max_initial_timestamp_index=50, no_speech_prob=False, repetition_penalty=1.0, no_repeat_ngram_size=0, sampling_topk=0,
                       sampling_temperature=1.0, num_hypotheses=1)
    assert keys[0] == todays            # timestamps off: the key it always was
    # a prompt with a decoder prefix after its start sequence keeps the plain search (and its drafts), as before
    prefixed = [50258, 50259, 50359, 40763]
    m.generate(feats, [prefixed], beam_size=1)
    assert calls[-1]["timestamps"] is False and keys[-1] == todays
    m.generate(feats, [prefixed], beam_size=1, draft_tokens=[1, 2, 3])
    assert calls[-1]["timestamps"] is False and calls[-1]["draft"] == (1, 2, 3)
    assert not ct2.timestamp_prompt([50258, 50259, 50359, 50363]) and not ct2.timestamp_prompt([50259, 50359])
    assert ct2.timestamp_prompt([50258]) and ct2.timestamp_prompt([50361, 1000, 50258, 50259, 50358])      # (context before <|sot|>)
    assert not ct2.timestamp_prompt([50258, 50259, 50359, 50364])
    # drafts and timestamps do not mix
    with pytest.raises(ValueError):
        m.generate(feats, [PROMPT], beam_size=1, draft_tokens=[1, 2, 3])
    with pytest.raises(ValueError):
        m.generate(feats, [PROMPT], beam_size=2, draft_trajectory=(np.zeros((2, 2), np.int32), np.zeros((2, 2), np.int32)))
    with pytest.raises(ValueError):          # one call decodes with timestamps or without, not both
        m.generate(ct2.StorageView.from_array(np.zeros((2, 80, 3000), np.float32)), [PROMPT + [NO_TIMESTAMPS], PROMPT + [50360]], beam_size=1)


# ---- REST surface, with a stand-in engine -----------------------------------------------------------------------------------
class _FakeWhisper:
    def __init__(self):
        self.prompts = []

    def generate(self, feats, prompts, beam_size=5, return_scores=False, fixed_new_tokens=0, input_kind=0, **kw):
        self.prompts.append(list(prompts[0]))
        ts = NO_TIMESTAMPS not in prompts[0]
        from wis_hip import ctranslate2 as ct2
        ids = [TB, 11, 12, TB + 50, TB + 50, 13, TB + 90] if ts else [11, 12, 13]
        return [ct2.WhisperGenerationResult([ids], [0.0]) for _ in prompts]

    def detect_language(self, *a, **k):
        return [[("<|en|>", 1.0)]]


class _Models:
    def __init__(self):
        from wis_hip.settings import APISettings
        from wis_hip.whisper import _Tokenizer
        self.settings = APISettings()
        self.settings.fuse_logmel = True
        self.tokenizer = _Tokenizer(None)
        self.whisper = _FakeWhisper()

    def tokenizer_for(self, size):
        return self.tokenizer

    def get(self, size):
        return self.whisper


def _wav(seconds):
    buf = io.BytesIO()
    with wave.open(buf, "wb") as w:
        w.setnchannels(1); w.setsampwidth(2); w.setframerate(16000)
        w.writeframes((np.sin(np.arange(int(16000 * seconds)) * 0.05) * 8000).astype("<i2").tobytes())
    return buf.getvalue()


def _multipart(data):
    b = "tsBoundary42"
    body = (f"--{b}\r\nContent-Disposition: form-data; name=\"audio_file\"; filename=\"a.wav\"\r\nContent-Type: application/octet-stream\r\n\r\n").encode() \
        + data + f"\r\n--{b}--\r\n".encode()
    return body, {"content-type": f"multipart/form-data; boundary={b}"}


def test_server_timestamps():
    import httpx
    from wis_hip.server import create_app
    models = _Models()
    app = create_app(models=models)
    short, long_ = _wav(3.0), _wav(31.0)

    async def go():
        async with httpx.AsyncClient(transport=httpx.ASGITransport(app=app), base_url="http://wis") as c:
            body, hdr = _multipart(short)
            r = await c.post("/api/asr?model=tiny", content=body, headers=hdr)
            assert r.status_code == 200 and "segments" not in r.json() and r.json()["text"] == "11 12 13"
            assert set(r.json()) == {"infer_time", "infer_speedup", "audio_duration", "language", "text"}
            assert models.whisper.prompts[-1][-1] == NO_TIMESTAMPS
            r = await c.post("/api/asr?model=tiny&timestamps=true", content=body, headers=hdr)
            assert r.status_code == 200, r.text
            j = r.json()
            assert models.whisper.prompts[-1] == PROMPT
            assert j["text"] == "11 12 13"                                   # no timestamp tokens in the text
            assert j["segments"] == [{"start": 0.0, "end": 1.0, "text": "11 12"}, {"start": 1.0, "end": 1.8, "text": "13"}]
            r = await c.post("/api/willow?model=tiny", content=short, headers={"x-audio-codec": "wav"})
            assert r.status_code == 200 and r.json() == {"language": "en", "text": "11 12 13"}
            r = await c.post("/api/willow?model=tiny&timestamps=1", content=short, headers={"x-audio-codec": "wav"})
            assert r.status_code == 200 and r.json()["segments"][1] == {"start": 1.0, "end": 1.8, "text": "13"}
            body, hdr = _multipart(long_)
            r = await c.post("/api/asr?model=tiny&timestamps=true", content=body, headers=hdr)
            assert r.status_code == 400 and "30 s" in r.json()["error"]
            r = await c.post("/api/willow?model=tiny&timestamps=true", content=long_, headers={"x-audio-codec": "wav"})
            assert r.status_code == 400
    asyncio.run(go())
