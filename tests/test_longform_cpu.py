"""not gpu: the long-form seek loop (wis_hip.longform.transcribe) against a scripted decode step, and its opt-in through do_whisper and the REST surface
with a stand-in engine and a stand-in long-mel.  Every branch of the rule, the prompt each window is handed, and the request surface."""
import asyncio
import io
import os
import sys
import wave

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "willow-inference-server_amd"))

from wis_hip import longform, weights as W  # noqa: E402

SP = W.special_tokens(W.N_VOCAB)
TB, EOT, SOP = SP.timestamp_begin, SP.eot, SP.startofprev
START = [SP.sot, SP.language_token_id("en"), SP.transcribe]


class Mel:
    """stand-in for audio.LongMel: a window is its seek"""

    def __init__(self, frames):
        self.frames, self.asked = frames, []

    def window(self, seek):
        self.asked.append(seek)
        return seek


class Script:
    """decode step: per seek either (tokens, score, no_speech_prob) or {temperature: (tokens, score, no_speech_prob)}"""

    def __init__(self, by_seek):
        self.by_seek, self.calls = by_seek, []

    def __call__(self, window, prompt, t, n):
        self.calls.append((window, list(prompt), t, n))
        e = self.by_seek[window]
        toks, score, nsp = e[t] if isinstance(e, dict) else e
        return [(list(toks) + [EOT], score)] * n, nsp


def run(frames, by_seek, **kw):
    mel, dec = Mel(frames), Script(by_seek)
    kw.setdefault("no_speech_threshold", 0.6)
    res = longform.transcribe(mel, dec, start=START, special=SP, **kw)
    seeks = [w["seek"] for w in res["windows"]]
    assert seeks == mel.asked and all(b > a for a, b in zip(seeks, seeks[1:]))
    return res, dec, seeks


BRANCHES = {
    0: ([TB, 11, 12, TB + 50, TB + 50, 13, TB + 100, TB + 100, 14], -0.1, 0.0),      # pairs, text behind the last closed timestamp
    200: ([TB, 21, TB + 100, TB + 100, 22, TB + 250], -0.1, 0.0),                    # pairs and a single ending timestamp
    3200: ([TB, 31, 32, TB + 400], -0.1, 0.0),                                       # no pairs, a last timestamp
    6200: ([TB, 41, 42], -0.1, 0.0),                                                 # no pairs, the last timestamp is <|0.00|>; the short last window
}


def test_every_branch_of_the_rule():
    res, dec, seeks = run(7000, BRANCHES)
    assert seeks == [0, 200, 3200, 6200]
    assert [w["segment_size"] for w in res["windows"]] == [3000, 3000, 3000, 800]
    assert [w["advance"] for w in res["windows"]] == [200, 3000, 3000, 800]
    assert [(s["start"], s["end"], [t for t in s["tokens"] if t < EOT]) for s in res["segments"]] == [
        (0.0, 1.0, [11, 12]), (1.0, 2.0, [13]),                    # 14 sits behind the last closed timestamp: the next window decodes it again
        (2.0, 4.0, [21]), (4.0, 7.0, [22]),                        # time_offset 2.0; the single ending timestamp closes the final slice
        (32.0, 40.0, [31, 32]),                                    # from time_offset to the last timestamp seen
        (62.0, 70.0, [41, 42])]                                    # <|0.00|>: to the end of the (short, 8 s) window
    assert all(EOT not in w["tokens"] for w in res["windows"])
    assert all(c[2] == 0.0 and c[3] == 1 for c in dec.calls) and len(dec.calls) == 4      # no temperatures: one search per window
    # the prompt of each window: the text tokens of every kept segment so far behind <|startofprev|>, then the start sequence
    assert [w["prompt"] for w in res["windows"]] == [START, [SOP, 11, 12, 13] + START, [SOP, 11, 12, 13, 21, 22] + START,
                                                    [SOP, 11, 12, 13, 21, 22, 31, 32] + START]
    assert [c[1] for c in dec.calls] == [w["prompt"] for w in res["windows"]]


def test_no_speech_skip_and_its_logprob_exception():
    script = {0: ([TB, 11, TB + 100], -3.0, 0.9), 3000: ([TB, 12, TB + 100], -0.1, 0.9), 6000: ([TB, 13, TB + 100], -3.0, 0.5)}
    res, _, seeks = run(7000, script, logprob_threshold=-1.0)
    assert seeks == [0, 3000, 6000]
    assert [w["skipped"] for w in res["windows"]] == [True, False, False]      # silent and badly scored | silent but well scored | not silent
    assert [(s["start"], s["end"]) for s in res["segments"]] == [(30.0, 32.0), (60.0, 62.0)]
    assert res["windows"][1]["prompt"] == START                                # a skipped window leaves no text behind
    # without a log-probability threshold there is no exception; without a no-speech threshold there is no skip
    res, _, _ = run(7000, script, logprob_threshold=None)
    assert [w["skipped"] for w in res["windows"]] == [True, True, False]
    res, _, _ = run(7000, script, logprob_threshold=-1.0, no_speech_threshold=None)
    assert [w["skipped"] for w in res["windows"]] == [False, False, False]
    assert res["windows"][0]["avg_logprob"] == -3.0 * 3 / 4      # the engine's score over the tokens + 1, the end token not among them


def test_zero_advance_guard():
    # a pair that closes at <|0.00|>: the original loop would decode the same window for ever
    res, _, seeks = run(3500, {0: ([TB, TB, 51], -0.1, 0.0), 3000: ([TB, 52, TB + 10], -0.1, 0.0)})
    assert seeks == [0, 3000] and res["windows"][0]["advance"] == 3000
    assert [(s["start"], s["end"]) for s in res["segments"]] == [(0.0, 0.0), (30.0, 30.2)]


def test_times_stay_inside_a_short_last_window():
    # the last window holds 5 s of content; the decoder closes its segments at 4 s and at 10 s: the second is held at the recording's end
    res, _, seeks = run(3500, {0: ([TB, 50, TB + 1500], -0.1, 0.0), 3000: ([TB, 52, TB + 200, TB + 200, 53, TB + 500], -0.1, 0.0)})
    assert seeks == [0, 3000]
    assert [(s["start"], s["end"]) for s in res["segments"]] == [(0.0, 30.0), (30.0, 34.0), (34.0, 35.0)]


def test_prompts_conditioning_reset_and_cut():
    ip = [7, 8]
    res, _, _ = run(7000, BRANCHES, initial_prompt_ids=ip)
    assert [w["prompt"] for w in res["windows"]][:2] == [[SOP, 7, 8] + START, [SOP, 7, 8, 11, 12, 13] + START]
    res, _, _ = run(7000, BRANCHES, initial_prompt_ids=ip, condition_on_previous_text=False)
    assert all(w["prompt"] == [SOP, 7, 8] + START for w in res["windows"])      # conditioning off: the initial prompt alone, every window
    res, _, _ = run(7000, BRANCHES, condition_on_previous_text=False)
    assert all(w["prompt"] == START for w in res["windows"])
    # the reset above temperature 0.5: the window at 200 scores badly at 0 and at 0.4 and is kept at 0.8 - its text and everything before it leave the prompt
    script = dict(BRANCHES)
    script[200] = {0.0: ([TB, 20, TB + 250], -9.0, 0.0), 0.4: ([TB, 23, TB + 250], -9.0, 0.0), 0.8: ([TB, 21, TB + 100, TB + 100, 22, TB + 250], -0.1, 0.0)}
    res, dec, seeks = run(7000, script, initial_prompt_ids=ip, temperatures=(0.0, 0.4, 0.8), best_of=3, logprob_threshold=-1.0)
    assert seeks == [0, 200, 3200, 6200]
    assert [w["temperature"] for w in res["windows"]] == [0.0, 0.8, 0.0, 0.0]
    assert [(c[0], c[2], c[3]) for c in dec.calls] == [(0, 0.0, 1), (200, 0.0, 1), (200, 0.4, 3), (200, 0.8, 3), (3200, 0.0, 1), (6200, 0.0, 1)]
    assert res["windows"][2]["prompt"] == [SOP, 7, 8] + START and res["windows"][3]["prompt"] == [SOP, 7, 8, 31, 32] + START
    assert [t for s in res["segments"] for t in s["tokens"] if t < EOT] == [11, 12, 13, 21, 22, 31, 32, 41, 42]
    # a kept decode at 0.4 does not reset
    script[200] = {0.0: ([TB, 20, TB + 250], -9.0, 0.0), 0.4: ([TB, 21, TB + 250], -0.1, 0.0)}
    res, _, _ = run(7000, script, temperatures=(0.0, 0.4, 0.8), logprob_threshold=-1.0)
    assert res["windows"][2]["prompt"] == [SOP, 11, 12, 13, 21] + START
    # the left cut: 223 prompt tokens behind <|startofprev|>, the newest text kept, the initial prompt in front of it losing its head
    long_ip = list(range(1000, 1300))
    res, _, _ = run(7000, BRANCHES, initial_prompt_ids=long_ip)
    p0, p1 = res["windows"][0]["prompt"], res["windows"][1]["prompt"]
    assert len(p0) == len(p1) == 1 + 223 + 3 and p0 == [SOP] + long_ip[-223:] + START
    assert p1 == [SOP] + long_ip[-220:] + [11, 12, 13] + START


# ---- do_whisper and the REST surface, with a stand-in engine and a stand-in long-mel ------------------------------------------------------
class _Replica:
    device = 0


class _FakeWhisper:
    n_mels = 80

    def __init__(self):
        self.calls, self.prompts, self.held = [], [], 0
        self._replicas = [_Replica()]
        self.script = {0: [TB, 11, 12, TB + 500, TB + 500, 13, TB + 1400, TB + 1400], 2800: [TB, 14, TB + 100]}
        self.fail_at, self.nsp = None, 0.01

    def acquire_replica(self):
        self.held += 1
        return self._replicas[0]

    def release_replica(self, r):
        self.held -= 1

    def generate_from_device(self, device, ptr, prompt, **kw):
        from wis_hip import ctranslate2 as ct2
        assert W.NO_TIMESTAMPS not in prompt and kw.get("return_no_speech_prob") and kw.get("replica") is self._replicas[0]
        self.calls.append((ptr, kw))
        self.prompts.append(list(prompt))
        if self.fail_at == ptr:
            raise ValueError("scripted failure")
        return ct2.WhisperGenerationResult([self.script[ptr]], [-0.1], self.nsp)

    def generate(self, feats, prompts, **kw):
        from wis_hip import ctranslate2 as ct2
        self.prompts.append(list(prompts[0]))
        return [ct2.WhisperGenerationResult([[11, 12, 13]], [0.0]) for _ in prompts]

    def detect_language(self, *a, **k):
        return [[("<|en|>", 1.0)]]

    # encoder frames (20 ms) at which the alignment path reaches each text token and then <|endoftext|>, per window: monotone as a DTW path is,
    # and on purpose not inside the segments the timestamp tokens of `script` describe
    align_script = {0: [50, 600, 650, 1450], 2800: [0, 140]}

    def align_from_device(self, device, ptr, start_sequence, text_tokens, num_frames, replica=None, **kw):
        from wis_hip import ctranslate2 as ct2
        assert replica is self._replicas[0] and list(start_sequence) == START and num_frames == min(3000, 3100 - ptr)
        frames = self.align_script[ptr]
        assert len(frames) == len(text_tokens[0]) + 1
        return [ct2.WhisperAlignmentResult([(i, f) for i, f in enumerate(frames)], [0.5] * len(text_tokens[0]))]


class _Vocab:
    """stand-in vocabulary: every text id is a word of its own"""
    has_vocabulary, all_special_ids = True, []
    decode = staticmethod(lambda ids: "".join(f" w{int(t)}" for t in ids if int(t) < EOT))


class _FakeLongMel:
    live = []

    def __init__(self, pcm, n_mels=80, device=0, segment_samples=0):
        self.frames, self.closed = len(pcm) // 160, False
        _FakeLongMel.live.append(self)

    def window(self, seek, to_host=False):
        assert not self.closed
        return np.zeros((80, 3000), np.float32) if to_host else seek

    def close(self):
        self.closed = True


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


@pytest.fixture
def fake_longmel(monkeypatch):
    from wis_hip import audio
    _FakeLongMel.live = []
    monkeypatch.setattr(audio, "LongMel", _FakeLongMel)
    return _FakeLongMel


def _pcm(seconds):
    return (np.sin(np.arange(int(16000 * seconds)) * 0.05) * 0.25).astype(np.float32)


def test_do_whisper_seek(fake_longmel):
    from wis_hip.whisper import do_whisper
    models = _Models()
    pcm = _pcm(31.0)
    r = do_whisper(pcm, "tiny", 1, "transcribe", False, "en", models=models, long_form="seek", timestamps=True)
    assert r.segments == [{"start": 0.0, "end": 10.0, "text": "11 12"}, {"start": 10.0, "end": 28.0, "text": "13"}, {"start": 28.0, "end": 30.0, "text": "14"}]
    assert r[1] == "11 12 13 14" and r[5] == 31000 and [w["seek"] for w in r.seek] == [0, 2800]
    assert models.whisper.prompts == [START, [SOP, 11, 12, 13] + START]
    assert len(fake_longmel.live) == 1 and fake_longmel.live[0].closed and models.whisper.held == 0
    # without timestamps asked for: the same loop (it always decodes under the timestamp rules), no segments returned
    r = do_whisper(pcm, "tiny", 1, "transcribe", False, "en", models=models, long_form="seek")
    assert r.segments is None and r[1] == "11 12 13 14" and W.NO_TIMESTAMPS not in models.whisper.prompts[-1]
    # the options reach every window's decode
    r = do_whisper(pcm, "tiny", 1, "transcribe", False, "en", models=models, long_form="seek", repetition_penalty=1.2, no_repeat_ngram_size=3,
                   initial_prompt=[5, 6], condition_on_previous_text=False)
    assert all(kw["repetition_penalty"] == 1.2 and kw["no_repeat_ngram_size"] == 3 for _, kw in models.whisper.calls[-2:])
    assert models.whisper.prompts[-2:] == [[SOP, 5, 6] + START] * 2
    # the setting serves requests that do not say
    models.settings.long_form = "seek"
    assert do_whisper(pcm, "tiny", 1, "transcribe", False, "en", models=models, timestamps=True).segments[-1]["end"] == 30.0
    with pytest.raises(ValueError, match="30 s"):
        do_whisper(pcm, "tiny", 1, "transcribe", False, "en", models=models, timestamps=True, long_form="chunk")
    models.settings.long_form = "chunk"
    # refusals: a prefix, a bad value; the long-mel is destroyed and the replica released on a failing path too
    with pytest.raises(ValueError, match="prefix"):
        do_whisper(pcm, "tiny", 1, "transcribe", False, "en", models=models, long_form="seek", timestamps=True, prefix=[9])
    with pytest.raises(ValueError, match="long_form"):
        do_whisper(pcm, "tiny", 1, "transcribe", False, "en", models=models, long_form="both")
    models.whisper.fail_at = 2800
    n = len(fake_longmel.live)
    with pytest.raises(ValueError, match="scripted"):
        do_whisper(pcm, "tiny", 1, "transcribe", False, "en", models=models, long_form="seek")
    assert len(fake_longmel.live) == n + 1 and all(m.closed for m in fake_longmel.live) and models.whisper.held == 0
    models.whisper.fail_at = None
    # up to 30 s the option changes nothing: the one-window path, no long-mel
    n = len(fake_longmel.live)
    r = do_whisper(_pcm(3.0), "tiny", 1, "transcribe", False, "en", models=models, long_form="seek")
    assert r[1] == "11 12 13" and len(fake_longmel.live) == n and models.whisper.prompts[-1][-1] == W.NO_TIMESTAMPS


def test_do_whisper_seek_words_lie_inside_their_segments(fake_longmel):
    from wis_hip.whisper import do_whisper
    models = _Models()
    models.tokenizer = _Vocab()
    pcm = _pcm(31.0)
    plain = do_whisper(pcm, "tiny", 1, "transcribe", False, "en", models=models, long_form="seek", timestamps=True)
    r = do_whisper(pcm, "tiny", 1, "transcribe", False, "en", models=models, long_form="seek", word_timestamps=True)
    # the segments are what the timestamp tokens said, with and without words; monotone and inside the recording
    assert [{k: v for k, v in sg.items() if k != "words"} for sg in r.segments] == plain.segments
    assert [(sg["start"], sg["end"]) for sg in r.segments] == [(0.0, 10.0), (10.0, 28.0), (28.0, 30.0)]
    words = [[(w["word"], w["start"], w["end"]) for w in sg["words"]] for sg in r.segments]
    # the alignment put w11 at 1.0 .. 12.0, w12 at 12.0 .. 13.0, w13 at 13.0 .. 29.0 and w14 at 28.0 .. 30.8: each is held at its segment's bounds
    assert words == [[(" w11", 1.0, 10.0), (" w12", 10.0, 10.0)], [(" w13", 13.0, 28.0)], [(" w14", 28.0, 30.0)]]
    for sg in r.segments:
        assert "".join(w["word"] for w in sg["words"]).strip() == sg["text"]
        for w in sg["words"]:
            assert sg["start"] <= w["start"] <= w["end"] <= sg["end"] and w["probability"] == 0.5
    assert all(m.closed for m in fake_longmel.live) and models.whisper.held == 0


def test_do_whisper_seek_translate(fake_longmel):
    """translate=True with long_form="seek": the loop a second time with the translate task - unprompted, one search per window, the repetition options
    and the skip rule applied; the translation carries no segments"""
    from wis_hip.whisper import do_whisper
    models = _Models()
    pcm = _pcm(31.0)
    r = do_whisper(pcm, "tiny", 1, "transcribe", False, "en", translate=True, models=models, long_form="seek", timestamps=True, initial_prompt=[5, 6],
                   repetition_penalty=1.2, temperatures=(0.0, 0.4))
    tstart = START[:2] + [SP.translate]
    assert models.whisper.prompts == [[SOP, 5, 6] + START, [SOP, 5, 6, 11, 12, 13] + START, tstart, [SOP, 11, 12, 13] + tstart]
    assert all(kw["repetition_penalty"] == 1.2 and kw.get("beam_size") == models.settings.long_beam_size and "sampling_temperature" not in kw
               for _, kw in models.whisper.calls)      # (31 s is past long_beam_size_threshold)
    assert r[3] == "11 12 13 14" and r.translation_tokens == [11, 12, 13, 14] and r[1] == "11 12 13 14" and len(r.segments) == 3
    assert len(fake_longmel.live) == 1 and fake_longmel.live[0].closed and models.whisper.held == 0
    # the skip rule of the translation pass is the transcription's: a silent window is kept when its decode scores above logprob_threshold ...
    models.whisper.nsp = 0.9
    r = do_whisper(pcm, "tiny", 1, "transcribe", False, "en", translate=True, models=models, long_form="seek")
    assert r[1] == r[3] == "11 12 13 14"
    # ... and skipped in both passes when there is no such threshold (a skip advances by the window: the second window is at 3000)
    models.whisper.script[3000] = [TB, 15, TB + 50]
    r = do_whisper(pcm, "tiny", 1, "transcribe", False, "en", translate=True, models=models, long_form="seek", logprob_threshold=-1e30)
    assert r[1] == r[3] == "" and [w["skipped"] for w in r.seek] == [True, True]


def _wav(seconds):
    buf = io.BytesIO()
    with wave.open(buf, "wb") as w:
        w.setnchannels(1); w.setsampwidth(2); w.setframerate(16000)
        w.writeframes((np.sin(np.arange(int(16000 * seconds)) * 0.05) * 8000).astype("<i2").tobytes())
    return buf.getvalue()


def _multipart(data):
    b = "lfBoundary42"
    body = (f"--{b}\r\nContent-Disposition: form-data; name=\"audio_file\"; filename=\"a.wav\"\r\nContent-Type: application/octet-stream\r\n\r\n").encode() \
        + data + f"\r\n--{b}--\r\n".encode()
    return body, {"content-type": f"multipart/form-data; boundary={b}"}


def test_server_long_form(fake_longmel):
    import httpx
    from wis_hip.server import create_app
    models = _Models()
    app = create_app(models=models)
    long_ = _wav(31.0)

    async def go():
        async with httpx.AsyncClient(transport=httpx.ASGITransport(app=app), base_url="http://wis") as c:
            body, hdr = _multipart(long_)
            r = await c.post("/api/asr?model=tiny&long_form=seek&timestamps=true", content=body, headers=hdr)
            assert r.status_code == 200, r.text
            j = r.json()
            dur = j["audio_duration"] / 1000.0
            assert dur == 31.0 and j["text"] == "11 12 13 14" and len(j["segments"]) == 3
            ends = [0.0]
            for sg in j["segments"]:
                assert ends[-1] <= sg["start"] <= sg["end"] <= dur
                ends.append(sg["end"])
            r = await c.post("/api/asr?model=tiny&long_form=seek", content=body, headers=hdr)
            assert r.status_code == 200 and "segments" not in r.json() and r.json()["text"] == "11 12 13 14"
            r = await c.post("/api/willow?model=tiny&long_form=seek&timestamps=1&condition_on_previous_text=false&no_speech_threshold=0.5", content=long_,
                             headers={"x-audio-codec": "wav"})
            assert r.status_code == 200 and r.json()["segments"][-1] == {"start": 28.0, "end": 30.0, "text": "14"}
            assert models.whisper.prompts[-1] == START                     # (conditioning off reached the loop)
            for bad in ("long_form=both", "long_form=seek&no_speech_threshold=x", "long_form=SEEK", "long_form=seek&condition_on_previous_text=maybe"):
                r = await c.post(f"/api/asr?model=tiny&{bad}", content=body, headers=hdr)
                assert r.status_code == 400, bad
                r = await c.post(f"/api/willow?model=tiny&{bad}", content=long_, headers={"x-audio-codec": "wav"})
                assert r.status_code == 400, bad
            # the default is the parent's: timestamps on a recording over 30 s are refused
            r = await c.post("/api/asr?model=tiny&timestamps=true", content=body, headers=hdr)
            assert r.status_code == 400 and "30 s" in r.json()["error"]
            r = await c.post("/api/asr?model=tiny&timestamps=true&long_form=chunk", content=body, headers=hdr)
            assert r.status_code == 400 and "30 s" in r.json()["error"]
    asyncio.run(go())
    assert all(m.closed for m in fake_longmel.live) and models.whisper.held == 0
    # a bad setting fails the start of the server, not every request
    models.settings.long_form = "both"
    with pytest.raises(ValueError, match="long_form"):
        create_app(models=models)


# ---- the engine face for device windows: generate_from_device takes generate's timestamp tail (tools/fake_engine_app.py) ---------------------
def test_generate_from_device_timestamp_tail(monkeypatch):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    monkeypatch.syspath_prepend(os.path.join(root, "tools"))
    from wis_hip import _lib, ctranslate2 as ct2
    monkeypatch.setattr(ct2, "_generate_chunk", ct2._generate_chunk)      # (the factory replaces both: put back when the test ends)
    monkeypatch.setattr(_lib, "device_count", _lib.device_count)
    for k, v in (("WIS_FAKE_MS", "0"), ("WIS_FAKE_MS_PER_UTT", "0"), ("WIS_FAKE_REPLICAS", "1")):
        monkeypatch.setenv(k, v)
    import fake_engine_app
    app = fake_engine_app.create_app()
    model = app.state.wis["models"]._models["large"]
    calls, keys = [], []
    inner, submit = ct2._generate_chunk, model._batcher.submit
    monkeypatch.setattr(ct2, "_generate_chunk", lambda r, mel, prompts, opts, **kw: (calls.append(opts._asdict()), inner(r, mel, prompts, opts, **kw))[1])
    model._batcher.submit = lambda key, rows, **kw: (keys.append(key), submit(key, rows, **kw))[1]
    try:
        plain = ct2.DecodeOptions(prompt_len=4, beam_size=1, max_new_tokens=224, length_penalty=1.0, patience=1.0, suppress_blank=True, suppress_default=True,
                                  fixed_new_tokens=0, input_kind=_lib.WIS_IN_MEL_DEV, draft=None, return_trajectory=False, timestamps=False,
                                  max_initial_timestamp_index=50, no_speech_prob=False, repetition_penalty=1.0, no_repeat_ngram_size=0, sampling_topk=0,
                                  sampling_temperature=1.0, num_hypotheses=1)
        model.generate_from_device(0, 4096, START + [W.NO_TIMESTAMPS], beam_size=1)
        assert keys[-1] == plain                                            # <|notimestamps|>: the key and the call they always were
        model.generate_from_device(0, 4096, START, beam_size=1, return_scores=True)
        assert keys[-1] == plain._replace(prompt_len=3, timestamps=True)
        assert calls[-1]["timestamps"] is True and calls[-1]["max_initial_timestamp_index"] == 50 and calls[-1]["no_speech_prob"] is False
        model.generate_from_device(0, 4096, START, beam_size=1, max_initial_timestamp_index=None, return_no_speech_prob=True)
        assert keys[-1] == plain._replace(prompt_len=3, timestamps=True, max_initial_timestamp_index=None, no_speech_prob=True) and calls[-1]["max_initial_timestamp_index"] is None and calls[-1]["no_speech_prob"] is True
        model.generate_from_device(0, 4096, START + [W.NO_TIMESTAMPS], beam_size=1, return_no_speech_prob=True, max_initial_timestamp_index=7)
        assert keys[-1] == plain._replace(no_speech_prob=True) and calls[-1]["timestamps"] is False
        # the same record as generate's: the repetition and sampling fields beside the timestamp ones
        model.generate_from_device(0, 4096, [SOP, 11, 12] + START, beam_size=1, no_repeat_ngram_size=3, return_no_speech_prob=True)
        assert keys[-1] == plain._replace(prompt_len=6, timestamps=True, no_speech_prob=True, no_repeat_ngram_size=3)
        model.generate_from_device(0, 4096, START, beam_size=1, num_hypotheses=3, sampling_topk=0, sampling_temperature=0.4, sampling_seed=1, return_no_speech_prob=True)
        assert keys[-1] == plain._replace(prompt_len=3, timestamps=True, no_speech_prob=True, sampling_topk=-1, sampling_temperature=0.4, num_hypotheses=3) and calls[-1]["num_hypotheses"] == 3
        feats = ct2.StorageView.from_array(np.zeros((1, 80, 3000), np.float32))
        model.generate(feats, [START], beam_size=1, return_no_speech_prob=True)
        assert keys[-1] == plain._replace(prompt_len=3, input_kind=_lib.WIS_IN_MEL_HOST, timestamps=True, no_speech_prob=True)      # generate's record for the same options
        # a prefix behind the start sequence keeps the plain search, as in generate; drafts stay refused with these options
        model.generate_from_device(0, 4096, START + [400], beam_size=1)
        assert keys[-1] == plain and calls[-1]["timestamps"] is False
        n = len(keys)
        with pytest.raises(ValueError, match="draft"):
            model.generate_from_device(0, 4096, START, beam_size=1, draft_tokens=[400])
        with pytest.raises(ValueError, match="draft"):
            model.generate_from_device(0, 4096, START + [W.NO_TIMESTAMPS], beam_size=1, draft_tokens=[400], return_no_speech_prob=True)
        assert len(keys) == n
    finally:
        model.close()
