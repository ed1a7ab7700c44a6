"""Prompted decoding without a GPU: the assembly of the decoder prompt in do_whisper (openai-whisper's layout, the left truncation, the prefix cap, strings
with and without a vocabulary), the plumbing from the query string to `_generate_chunk` with the engine replaced by tools/fake_engine_app.py, and what
the micro-batcher does with long prompts (device-batch capacity, key separation by prompt length)."""
import asyncio
import os

import numpy as np
import pytest

SOT, PREV, NO_TS, EOT = 50258, 50361, 50363, 50257
START = [SOT, 50259, 50359, NO_TS]


def _special():
    from wis_hip import weights as W
    return W.special_tokens(51865, {})


class _Vocab:
    """a tokenizer with a vocabulary: one id per character"""
    has_vocabulary = True

    def encode(self, text):
        return [ord(c) for c in text]


class _NoVocab:
    has_vocabulary = False


# ---- assembly ---------------------------------------------------------------------------------------------------------------------------------
def test_layout_is_openai_whispers():
    from wis_hip.whisper import assemble_prompt
    sp = _special()
    assert sp.startofprev == PREV
    assert assemble_prompt(START, sp) == START                                                      # neither option: today's prompt
    assert assemble_prompt(START, sp, [7, 8, 9]) == [PREV, 7, 8, 9] + START
    assert assemble_prompt(START, sp, [], [11, 12]) == START + [11, 12]                             # a prefix alone: no <|startofprev|>
    assert assemble_prompt(START, sp, [7, 8], [11, 12]) == [PREV, 7, 8] + START + [11, 12]
    assert assemble_prompt(START[:3], sp, [7], [11]) == [PREV, 7] + START[:3] + [11]                # the timestamp start sequence


def test_prompt_is_cut_from_the_left():
    from wis_hip.whisper import assemble_prompt
    sp, ids = _special(), list(range(1000, 1400))
    p = assemble_prompt(START, sp, ids)
    assert len(p) == 228 and p == [PREV] + ids[-223:] + START                                       # n_ctx / 2 - 1 = 223 prompt tokens
    p = assemble_prompt(START[:3], sp, ids)
    assert len(p) == 227 and p == [PREV] + ids[-223:] + START[:3]
    p = assemble_prompt(START, sp, ids, list(range(50)))                                            # a prefix takes its room from the prompt
    assert len(p) == 228 and p == [PREV] + ids[-173:] + START + list(range(50))
    p = assemble_prompt(START, sp, ids, list(range(64)))
    assert len(p) == 228 and p[-64:] == list(range(64)) and p[1:160] == ids[-159:]
    assert assemble_prompt(START, sp, ids[:223]) == [PREV] + ids[:223] + START                      # exactly full: nothing cut
    with pytest.raises(ValueError, match="prefix"):
        assemble_prompt(START, sp, ids, list(range(65)))
    with pytest.raises(ValueError, match="prefix"):
        assemble_prompt(START, sp, [], list(range(65)))


def test_strings_and_ids():
    from wis_hip.whisper import prompt_ids
    sp = _special()
    assert prompt_ids(None, _NoVocab(), sp, "initial_prompt") == [] and prompt_ids("", _NoVocab(), sp, "prefix") == [] and prompt_ids([], _NoVocab(), sp, "prefix") == []
    assert prompt_ids("   ", _Vocab(), sp, "prefix") == []
    assert prompt_ids("  Kallax lamp ", _Vocab(), sp, "initial_prompt") == [ord(c) for c in " Kallax lamp"]      # " " + text.strip()
    with pytest.raises(ValueError, match="vocabulary"):
        prompt_ids("Kallax", _NoVocab(), sp, "initial_prompt")
    assert prompt_ids([5, 6, 7], _NoVocab(), sp, "initial_prompt") == [5, 6, 7]                      # ids need no vocabulary
    assert prompt_ids(np.array([5, 6]), _NoVocab(), sp, "prefix") == [5, 6]
    for bad in ([5, -1], [EOT], [SOT], [1.5], ["a"], 7, [True]):
        with pytest.raises(ValueError):
            prompt_ids(bad, _Vocab(), sp, "prefix")


# ---- do_whisper and REST over the fake engine -------------------------------------------------------------------------------------------------
@pytest.fixture()
def fake_app(monkeypatch):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    monkeypatch.syspath_prepend(os.path.join(root, "tools"))
    from wis_hip import _lib, ctranslate2 as ct2
    monkeypatch.setattr(ct2, "_generate_chunk", ct2._generate_chunk)      # (the factory replaces both: put back when the test ends)
    monkeypatch.setattr(_lib, "device_count", _lib.device_count)
    monkeypatch.setenv("WIS_FAKE_MS", "0")
    monkeypatch.setenv("WIS_FAKE_MS_PER_UTT", "0")
    monkeypatch.setenv("WIS_FAKE_REPLICAS", "1")
    import fake_engine_app
    app = fake_engine_app.create_app()
    model = app.state.wis["models"]._models["large"]
    calls = []      # (prompts, P, the DecodeOptions by field name) of every engine call
    inner = ct2._generate_chunk

    def spy(r, mel, prompts, opts, **kw):
        calls.append(([list(p) for p in prompts], opts.prompt_len, opts._asdict()))
        return inner(r, mel, prompts, opts, **kw)
    monkeypatch.setattr(ct2, "_generate_chunk", spy)
    yield app, calls, model
    model.close()


def _clip():
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "clips", "3sec.flac"), "rb") as f:
        return f.read()


def _multipart(data):
    b = "xYzBoundary123"
    body = (f"--{b}\r\nContent-Disposition: form-data; name=\"audio_file\"; filename=\"a.flac\"\r\nContent-Type: application/octet-stream\r\n\r\n").encode() \
        + data + f"\r\n--{b}--\r\n".encode()
    return body, {"content-type": f"multipart/form-data; boundary={b}"}


def test_do_whisper_hands_the_assembled_prompt_to_every_decode(fake_app):
    from wis_hip.settings import APISettings
    from wis_hip.whisper import do_whisper
    app, calls, _ = fake_app
    models = app.state.wis["models"]
    assert (APISettings().initial_prompt, APISettings().prefix) == ("", "")
    pcm = np.zeros(16000, np.float32)
    do_whisper(pcm, "large", 1, models=models)
    plain = calls[-1][0][0]
    assert calls[-1][1] == 4 and plain[0] == SOT and plain[-1] == NO_TS                             # off: today's prompt
    do_whisper(pcm, "large", 1, models=models, initial_prompt=[7, 8, 9], prefix=[11])
    assert calls[-1][0] == [[PREV, 7, 8, 9] + plain + [11]] and calls[-1][1] == 9
    do_whisper(pcm, "large", 1, models=models, initial_prompt=list(range(1000, 1400)))
    assert calls[-1][1] == 228 and calls[-1][0][0] == [PREV] + list(range(1177, 1400)) + plain
    # the fake engine's model has no vocabulary: a string is a ValueError before anything reaches the engine, ids still work (above)
    n0 = len(calls)
    with pytest.raises(ValueError, match="vocabulary"):
        do_whisper(pcm, "large", 1, models=models, initial_prompt="Kallax")
    with pytest.raises(ValueError, match="prefix"):
        do_whisper(pcm, "large", 1, models=models, prefix=list(range(65)))
    assert len(calls) == n0
    # a timestamped decode keeps its start sequence (no <|notimestamps|>) behind the prompt; the translation pass stays unprompted
    do_whisper(pcm, "large", 1, models=models, initial_prompt=[7], timestamps=True)
    assert calls[-1][0] == [[PREV, 7] + plain[:3]] and calls[-1][2]["timestamps"] is True
    # ... but a prefix would turn the prompt into one the engine decodes WITHOUT the timestamp rules: refused, nothing reaches the engine
    n0 = len(calls)
    for kw in (dict(timestamps=True), dict(word_timestamps=True)):
        with pytest.raises(ValueError, match="prefix cannot be combined with timestamps"):
            do_whisper(pcm, "large", 1, models=models, prefix=[11], **kw)
        with pytest.raises(ValueError, match="prefix cannot be combined with timestamps"):
            do_whisper(pcm, "large", 1, models=models, initial_prompt=[7], prefix=[11], **kw)
    models.settings.prefix = [11]                   # (a prefix from the settings is refused the same way)
    try:
        with pytest.raises(ValueError, match="prefix cannot be combined with timestamps"):
            do_whisper(pcm, "large", 1, models=models, timestamps=True)
        do_whisper(pcm, "large", 1, models=models, timestamps=True, prefix=[])      # the argument wins: no prefix, the rules apply
        assert calls[-1][0] == [plain[:3]] and calls[-1][2]["timestamps"] is True
    finally:
        models.settings.prefix = ""
    assert len(calls) == n0 + 1
    n0 = len(calls)
    do_whisper(pcm, "large", 1, models=models, initial_prompt=[7], prefix=[11], translate=True)
    assert len(calls) == n0 + 2 and calls[n0][0] == [[PREV, 7] + plain + [11]] and calls[n0 + 1][1] == 4 and PREV not in calls[n0 + 1][0][0]
    # every window of a long recording gets the same prompt
    n0 = len(calls)
    do_whisper(np.zeros(16000 * 70, np.float32), "large", 1, models=models, initial_prompt=[7, 8])
    windows = [p for c in calls[n0:] for p in c[0]]
    assert len(windows) >= 3 and all(p == [PREV, 7, 8] + plain for p in windows)
    # the settings are the defaults, the arguments win
    models.settings.initial_prompt = [21, 22]
    try:
        do_whisper(pcm, "large", 1, models=models)
        assert calls[-1][0] == [[PREV, 21, 22] + plain]
        do_whisper(pcm, "large", 1, models=models, initial_prompt=[])
        assert calls[-1][0] == [plain]
    finally:
        models.settings.initial_prompt = ""


def test_rest_parameters_and_400s(fake_app):
    import httpx
    app, calls, _ = fake_app
    body, hdr = _multipart(_clip())
    flac = _clip()

    async def go():
        async with httpx.AsyncClient(transport=httpx.ASGITransport(app=app), base_url="http://wis") as c:
            r = await c.post("/api/asr?model=large", content=body, headers=hdr)
            assert r.status_code == 200 and calls[-1][1] == 4
            plain = calls[-1][0][0]
            r = await c.post("/api/asr?model=large&initial_prompt=ids:7,8,9&prefix=ids:11", content=body, headers=hdr)
            assert r.status_code == 200, r.text
            assert calls[-1][0] == [[PREV, 7, 8, 9] + plain + [11]]
            r = await c.post("/api/willow?model=large&initial_prompt=ids:" + ",".join(str(1000 + i) for i in range(300)), content=flac, headers={"x-audio-codec": "flac"})
            assert r.status_code == 200 and calls[-1][1] == 228, r.text
            r = await c.post("/api/asr?model=large&initial_prompt=&prefix=", content=body, headers=hdr)      # empty: off
            assert r.status_code == 200 and calls[-1][0] == [plain]
            n0 = len(calls)
            for q in ("initial_prompt=ids:7,x", "prefix=ids:1.5", "initial_prompt=ids:-3", "prefix=ids:" + ",".join(["5"] * 65), "initial_prompt=ids:50257",
                      "initial_prompt=Kallax%20lamp",                 # text without a vocabulary
                      "prefix=ids:11&timestamps=true", "prefix=ids:11&word_timestamps=true", "initial_prompt=ids:7&prefix=ids:11&timestamps=true",
                      "prefix=" + "a" * 5000):
                r = await c.post(f"/api/asr?model=large&{q}", content=body, headers=hdr)
                assert r.status_code == 400 and ("initial_prompt" in r.json()["error"] or "prefix" in r.json()["error"]), (q, r.status_code, r.text)
                r = await c.post(f"/api/willow?model=large&{q}", content=flac, headers={"x-audio-codec": "flac"})
                assert r.status_code == 400, (q, r.status_code, r.text)
            assert len(calls) == n0                # nothing reached the engine

    asyncio.run(go())


# ---- the micro-batcher ------------------------------------------------------------------------------------------------------------------------
def test_capacity_does_not_divide_by_a_long_prompt():
    from wis_hip.ctranslate2 import MAX_DECODER_ROWS, MAX_PROMPT, SHORT_PROMPT, DecodeOptions, _capacity as capacity
    _capacity = lambda max_batch, key: capacity(max_batch, DecodeOptions(key[0], key[1], 224))      # key: (prompt length, beam size)
    assert (MAX_DECODER_ROWS, SHORT_PROMPT, MAX_PROMPT) == (96, 16, 228)
    # up to 16 tokens: what tests/test_loaders.py pins (rows of the merged prefill + first step)
    assert _capacity(32, (4, 1)) == 24 and _capacity(32, (4, 5)) == 19 and _capacity(16, (16, 1)) == 6 and _capacity(96, (1, 1)) == 96
    # beyond: the decode rows alone (the last prefill window shrinks with the batch)
    for P in (17, 33, 100, 228):
        assert _capacity(32, (P, 1)) == 32 and _capacity(96, (P, 1)) == 96 and _capacity(32, (P, 5)) == 19 and _capacity(16, (P, 5)) == 16 and _capacity(32, (P, 8)) == 12
    assert capacity(32, DecodeOptions(100, 1, 224, sampling_topk=-1, sampling_temperature=0.7, num_hypotheses=5)) == 19      # a sampled decode: five rows per utterance


def test_prompt_length_separates_device_batches_and_long_drafts_are_refused(fake_app):
    from wis_hip import _lib, ctranslate2 as ct2
    app, calls, _ = fake_app
    model = app.state.wis["models"].get("large")
    keys = []
    submit = model._batcher.submit
    model._batcher.submit = lambda key, rows, **kw: (keys.append(key), submit(key, rows, **kw))[1]
    pcm = ct2.StorageView.from_array(np.zeros((1, _lib.N_SAMPLES), np.float32))
    g = lambda prompt, **kw: model.generate(pcm, [prompt], beam_size=1, input_kind=_lib.WIS_IN_PCM_HOST, **kw)
    g(START)
    g([PREV] + [7] * 36 + START)
    g([PREV] + [7] * 37 + START)
    g([PREV] + [9] * 36 + START)
    assert [k.prompt_len for k in keys] == [4, 41, 42, 41] and keys[1] == keys[3] and len({keys[0], keys[1], keys[2]}) == 3
    todays = ct2.DecodeOptions(prompt_len=4, beam_size=1, max_new_tokens=224, length_penalty=1.0, patience=1.0, suppress_blank=True, suppress_default=True,
                               fixed_new_tokens=0, input_kind=_lib.WIS_IN_PCM_HOST, draft=None, return_trajectory=False, timestamps=False,
                               max_initial_timestamp_index=50, no_speech_prob=False, repetition_penalty=1.0, no_repeat_ngram_size=0, sampling_topk=0,
                               sampling_temperature=1.0, num_hypotheses=1)
    assert keys[0] == todays and keys[1] == todays._replace(prompt_len=41) and keys[2] == todays._replace(prompt_len=42)      # nothing but the length differs
    assert [k.max_new_tokens for k in keys] == [224] * 4 and g([PREV] + [7] * 223 + START)[0] is not None and keys[-1] == todays._replace(prompt_len=228, max_new_tokens=220)
    n0 = len(calls)
    with pytest.raises(ValueError, match="prompt length 229"):
        g([PREV] + [7] * 224 + START)
    with pytest.raises(ValueError, match="prompt length 0"):
        g([])
    with pytest.raises(ValueError, match="draft"):
        g([PREV] + [7] * 12 + START, draft_tokens=[5, 6, 7])
    assert len(calls) == n0
    g([PREV] + [7] * 11 + START, draft_tokens=[5, 6, 7])                                           # 16 tokens: the draft is taken
    assert len(calls) == n0 + 1
