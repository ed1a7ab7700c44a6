"""repetition_penalty / no_repeat_ngram_size without a GPU: the CPU statement of the two processors (tests/rep_ref.py, the reference of
tests/test_gpu_rep_rules.py) on hand-built rows, and the plumbing from the query string to `_generate_chunk` with the engine replaced by
tools/fake_engine_app.py."""
import asyncio
import os
import sys

import numpy as np
import pytest
import torch

from rep_ref import RepRaw, RepStepFn, ban, banned_tokens, penalise

NEG = float("-inf")


def _row(**vals):
    r = torch.zeros(1, 16)
    for k, v in vals.items():
        r[0, int(k[1:])] = v
    return r


def test_penalty_is_applied_once_per_distinct_token():
    row = _row(t3=4.0, t5=-3.0, t7=1.0)
    out = penalise(row, [[3, 3, 3, 5]], 2.0)
    assert out[0, 3] == 2.0                       # three occurrences, one division: 2, not 0.5
    assert out[0, 5] == -6.0                      # a negative logit is multiplied
    assert out[0, 7] == 1.0 and out[0, 0] == 0.0  # tokens outside the history are left alone
    assert row[0, 3] == 4.0                       # a copy: the raw rows are not modified
    rew = penalise(row, [[3, 5]], 0.5)            # p < 1 rewards
    assert rew[0, 3] == 8.0 and rew[0, 5] == -1.5
    assert penalise(row, [[3]], 1.0) is row and penalise(row, [[]], 2.0) is row


def test_penalty_is_fp32_true_division():
    x, p = np.float32(0.53), np.float32(1.3)
    row = torch.full((1, 4), float(x))
    out = penalise(row, [[2]], 1.3)
    assert out.dtype == torch.float32 and out[0, 2].item() == float(x / p)
    assert float(x / p) != float(x * (np.float32(1.0) / p))      # (the value was chosen so that a reciprocal multiply rounds differently)


def test_penalty_per_row_histories():
    rows = torch.ones(2, 8)
    out = penalise(rows, [[1], [2, 2]], 4.0)
    assert out[0].tolist() == [1, .25, 1, 1, 1, 1, 1, 1] and out[1].tolist() == [1, 1, .25, 1, 1, 1, 1, 1]


@pytest.mark.parametrize("seq,n,want", [
    ([5, 6, 7], 1, [5, 6, 7]),                    # n = 1: every history token
    ([], 1, []),
    ([5, 6, 5], 2, [6]),                          # ... 5 -> 6 seen: after another 5, 6 is banned
    ([5, 6, 7], 2, []),                           # the last token occurs once: nothing to complete
    ([5], 2, []),                                 # n = 2 needs one token of context: the token itself follows nothing yet
    ([1, 2, 3, 1, 2], 3, [3]),
    ([1, 2, 3, 9, 2], 3, []),
    ([1, 2], 3, []),                              # L < n
    ([1], 3, []),
    ([1, 2, 3, 1, 2, 4, 1, 2], 3, [3, 4]),        # the same prefix at two earlier positions bans two tokens
    ([7, 7, 7], 2, [7]),
    ([7, 7, 7], 3, [7]),
])
def test_ngram_bans(seq, n, want):
    assert banned_tokens(seq, n) == want
    rows = torch.zeros(1, 16)
    out = ban(rows, [seq], n)
    assert sorted(torch.nonzero(out[0] == NEG).flatten().tolist()) == want
    assert (rows == 0).all()


def test_ngram_off_and_short_history_do_nothing():
    rows = torch.zeros(2, 8)
    assert ban(rows, [[1, 2, 1], [3]], 0) is rows
    assert ban(rows, [[1, 2], [3]], 3) is rows


def test_step_fn_tracks_histories_through_origins():
    """Two beams; beam 1's successor descends from beam 0: the rules follow the reordered history.  Order: penalty on the raw rows, the
    processors (suppress list, suppress_blank at step 0), then the bans."""
    V = 12
    raw = lambda step, last, origin: torch.full((2, V), 2.0)
    fn = RepStepFn(raw, 2, suppress_ids=(9,), suppress_begin=(8,), suppress_blank=True, fixed_new=0, penalty=2.0, ngram=2, eot=11)
    lg = fn(0, None, None)
    assert lg[0, 9] == NEG and lg[0, 8] == NEG and (lg[:, :8] == 2.0).all()      # step 0: nothing but the processors
    fn(1, [3, 4], [0, 0])
    assert fn.hist == [[3], [4]]
    fn(2, [5, 3], [0, 0])                          # both beams continue beam 0's [3]
    assert fn.hist == [[3, 5], [3, 3]]
    lg = fn(3, [3, 6], [0, 0])                     # ... and again beam 0's [3, 5]
    assert fn.hist == [[3, 5, 3], [3, 5, 6]]
    assert lg[0, 3] == 1.0 and lg[0, 5] == NEG and lg[0, 6] == 2.0               # beam 0: 3, 5 penalised; 3 -> 5 seen, last is 3: 5 banned
    assert lg[1, 3] == 1.0 and lg[1, 5] == 1.0 and lg[1, 6] == 1.0 and lg[1, 9] == NEG and lg[1, 8] == 2.0
    rr = RepRaw(raw, 2, 2.0, 2)
    rr(0, None, None); rr(1, [3, 4], [0, 0]); rr(2, [5, 3], [0, 0])
    out = rr(3, [3, 6], [0, 0])
    assert out[0, 5] == NEG and out[0, 3] == 1.0 and out[0, 9] == 2.0             # the same two rules, none of the processors


def test_zero_penalty_means_off():
    raw = lambda step, last, origin: torch.full((1, 8), 2.0)
    fn = RepStepFn(raw, 1, (), (), False, 0, penalty=0.0, ngram=0)
    fn(0, None, None)
    assert (fn(1, [3], [0]) == 2.0).all()


# ---- plumbing: query string -> do_whisper -> Whisper.generate -> batcher key -> _generate_chunk (tools/fake_engine_app.py) -----------------
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
    calls = []
    inner = ct2._generate_chunk

    def spy(r, mel, prompts, opts, **kw):      # every engine call: its DecodeOptions by field name
        calls.append(opts._asdict())
        return inner(r, mel, prompts, opts, **kw)
    monkeypatch.setattr(ct2, "_generate_chunk", spy)
    yield app, calls, model
    model.close()


def _clip():
    root = os.path.dirname(os.path.abspath(__file__))
    with open(os.path.join(root, "golden", "clips", "3sec.flac"), "rb") as f:
        return f.read()


def _multipart(data):
    b = "xYzBoundary123"
    body = (f"--{b}\r\nContent-Disposition: form-data; name=\"audio_file\"; filename=\"a.flac\"\r\nContent-Type: application/octet-stream\r\n\r\n").encode() \
        + data + f"\r\n--{b}--\r\n".encode()
    return body, {"content-type": f"multipart/form-data; boundary={b}"}


def test_query_parameters_reach_the_engine_call_and_bad_values_are_400(fake_app):
    import httpx
    app, calls, _ = fake_app
    body, hdr = _multipart(_clip())
    flac = _clip()

    async def go():
        async with httpx.AsyncClient(transport=httpx.ASGITransport(app=app), base_url="http://wis") as c:
            r = await c.post("/api/asr?model=large&repetition_penalty=1.1&no_repeat_ngram_size=3", content=body, headers=hdr)
            assert r.status_code == 200, r.text
            assert calls[-1].get("repetition_penalty") == pytest.approx(1.1) and calls[-1].get("no_repeat_ngram_size") == 3, calls[-1]
            r = await c.post("/api/willow?model=large&no_repeat_ngram_size=2", content=flac, headers={"x-audio-codec": "flac"})
            assert r.status_code == 200, r.text
            assert calls[-1].get("no_repeat_ngram_size") == 2 and calls[-1].get("repetition_penalty") == 1.0, calls[-1]
            # the translation pass carries them too
            n0 = len(calls)
            r = await c.post("/api/asr?model=large&translate=true&repetition_penalty=1.3", content=body, headers=hdr)
            assert r.status_code == 200 and len(calls) == n0 + 2 and all(k.get("repetition_penalty") == pytest.approx(1.3) for k in calls[n0:]), calls[n0:]
            # ... and a request without them decodes as it always has: both are off in the engine call
            r = await c.post("/api/asr?model=large", content=body, headers=hdr)
            assert r.status_code == 200 and calls[-1]["repetition_penalty"] == 1.0 and calls[-1]["no_repeat_ngram_size"] == 0, calls[-1]
            n0 = len(calls)
            for q in ("repetition_penalty=abc", "repetition_penalty=0", "repetition_penalty=-1", "repetition_penalty=nan", "repetition_penalty=inf",
                      "no_repeat_ngram_size=-1", "no_repeat_ngram_size=1.5", "no_repeat_ngram_size=x"):
                r = await c.post(f"/api/asr?model=large&{q}", content=body, headers=hdr)
                assert r.status_code == 400 and ("repetition_penalty" in r.json()["error"] or "no_repeat_ngram_size" in r.json()["error"]), (q, r.status_code, r.text)
                r = await c.post(f"/api/willow?model=large&{q}", content=flac, headers={"x-audio-codec": "flac"})
                assert r.status_code == 400, (q, r.status_code, r.text)
            assert len(calls) == n0                # nothing reached the engine

    asyncio.run(go())


def test_settings_are_the_defaults_of_do_whisper(fake_app):
    from wis_hip.settings import APISettings
    from wis_hip.whisper import do_whisper
    app, calls, _ = fake_app
    assert (APISettings().repetition_penalty, APISettings().no_repeat_ngram_size) == (1.0, 0)
    models = app.state.wis["models"]
    pcm = np.zeros(16000, np.float32)
    do_whisper(pcm, "large", 1, models=models)
    assert calls[-1]["repetition_penalty"] == 1.0 and calls[-1]["no_repeat_ngram_size"] == 0
    models.settings.repetition_penalty, models.settings.no_repeat_ngram_size = 1.2, 4
    try:
        do_whisper(pcm, "large", 1, models=models)
        assert calls[-1]["repetition_penalty"] == pytest.approx(1.2) and calls[-1]["no_repeat_ngram_size"] == 4
        do_whisper(pcm, "large", 1, models=models, repetition_penalty=1.0, no_repeat_ngram_size=0)      # the arguments win
        assert calls[-1]["repetition_penalty"] == 1.0 and calls[-1]["no_repeat_ngram_size"] == 0
        do_whisper(pcm, "large", 1, models=models, timestamps=True)                                     # the timestamped pass
        assert calls[-1]["no_repeat_ngram_size"] == 4 and calls[-1]["timestamps"] is True
        with pytest.raises(ValueError):
            do_whisper(pcm, "large", 1, models=models, repetition_penalty=-2.0)
    finally:
        models.settings.repetition_penalty, models.settings.no_repeat_ngram_size = 1.0, 0


def test_batcher_keys(fake_app):
    """Default requests produce the key they always had; different values never share a device batch; drafts refuse both options."""
    from wis_hip import _lib, ctranslate2 as ct2
    app, calls, _ = fake_app
    model = app.state.wis["models"].get("large")
    keys = []
    submit = model._batcher.submit
    model._batcher.submit = lambda key, rows, **kw: (keys.append(key), submit(key, rows, **kw))[1]
    pcm = ct2.StorageView.from_array(np.zeros((1, _lib.N_SAMPLES), np.float32))
    prompt = [50258, 50259, 50359, 50363]
    g = lambda **kw: model.generate(pcm, [prompt], beam_size=1, input_kind=_lib.WIS_IN_PCM_HOST, **kw)
    g()
    g(repetition_penalty=1, no_repeat_ngram_size=0)
    g(repetition_penalty=1.0)
    todays = ct2.DecodeOptions(prompt_len=4, beam_size=1, max_new_tokens=224, length_penalty=1.0, patience=1.0, suppress_blank=True, suppress_default=True,
                               fixed_new_tokens=0, input_kind=_lib.WIS_IN_PCM_HOST, draft=None, return_trajectory=False, timestamps=False,
                               max_initial_timestamp_index=50, no_speech_prob=False, repetition_penalty=1.0, no_repeat_ngram_size=0, sampling_topk=0,
                               sampling_temperature=1.0, num_hypotheses=1)
    assert keys == [todays] * 3, keys
    g(repetition_penalty=1.1)
    g(repetition_penalty=1.2)
    g(no_repeat_ngram_size=3)
    g(repetition_penalty=1.1, no_repeat_ngram_size=3)
    g(repetition_penalty=1.1)
    assert len(set(keys[3:7])) == 4 and todays not in keys[3:] and keys[7] == keys[3], keys[3:]
    assert all(k == todays._replace(repetition_penalty=p, no_repeat_ngram_size=n) for k, (p, n) in zip(keys[3:7], ((1.1, 0), (1.2, 0), (1.0, 3), (1.1, 3)))), keys[3:7]
    # with the timestamp options and with a returned trajectory every other field keeps its value
    g(return_no_speech_prob=True, no_repeat_ngram_size=2)
    assert keys[-1] == todays._replace(no_speech_prob=True, no_repeat_ngram_size=2) and calls[-1]["no_speech_prob"] is True and calls[-1]["no_repeat_ngram_size"] == 2
    g(return_trajectory=True, repetition_penalty=1.5)
    assert keys[-1] == todays._replace(return_trajectory=True, repetition_penalty=1.5) and calls[-1]["return_trajectory"] is True and calls[-1]["repetition_penalty"] == 1.5
    ts_prompt = prompt[:3]
    model.generate(pcm, [ts_prompt], beam_size=1, input_kind=_lib.WIS_IN_PCM_HOST, no_repeat_ngram_size=3)
    assert keys[-1] == todays._replace(prompt_len=3, timestamps=True, no_repeat_ngram_size=3) and calls[-1]["timestamps"] is True
    # drafts
    n0 = len(keys)
    for kw in (dict(repetition_penalty=1.1), dict(no_repeat_ngram_size=2)):
        with pytest.raises(ValueError, match="draft"):
            g(draft_tokens=[400, 401], **kw)
        with pytest.raises(ValueError, match="draft"):
            model.generate(pcm, [prompt], beam_size=2, input_kind=_lib.WIS_IN_PCM_HOST,
                           draft_trajectory=(np.asarray([[400, 401]], np.int32), np.zeros((1, 2), np.int32)), **kw)
        with pytest.raises(ValueError, match="draft"):
            model.generate_from_device(0, 4096, prompt, beam_size=1, draft_tokens=[400], **kw)
    for kw in (dict(repetition_penalty=0), dict(repetition_penalty=-1), dict(repetition_penalty=float("nan")), dict(repetition_penalty="x"),
               dict(no_repeat_ngram_size=-1), dict(no_repeat_ngram_size=1.5)):
        with pytest.raises(ValueError):
            g(**kw)
    assert len(keys) == n0
    g(draft_tokens=[400, 401])                     # a draft with the defaults is today's drafted call
    assert keys[-1].draft.tokens == (400, 401) and keys[-1] == todays._replace(draft=keys[-1].draft)      # nothing but the draft differs
    for kw in (dict(sampling_topk=5), dict(num_hypotheses=2)):
        with pytest.raises(NotImplementedError):
            g(**kw)
    # the device-resident form takes the options too
    model.generate_from_device(0, 4096, prompt, beam_size=1, repetition_penalty=1.1, no_repeat_ngram_size=3)
    assert keys[-1] == todays._replace(input_kind=_lib.WIS_IN_MEL_DEV, repetition_penalty=1.1, no_repeat_ngram_size=3) and calls[-1]["repetition_penalty"] == 1.1
    model.generate_from_device(0, 4096, prompt, beam_size=1)
    assert keys[-1] == todays._replace(input_kind=_lib.WIS_IN_MEL_DEV)


def test_streaming_session_passes_the_options_only_without_a_draft():
    from wis_hip.streaming import StreamingSession

    class _W:
        def __init__(self):
            self.calls = []

        def generate(self, feats, prompts, **kw):
            from wis_hip.ctranslate2 import WhisperGenerationResult
            self.calls.append(kw)
            return [WhisperGenerationResult([[400, 401]], [-0.5])]

    s = StreamingSession.__new__(StreamingSession)
    s._whisper, s.fixed_new_tokens, s._rep = _W(), 0, dict(repetition_penalty=1.1, no_repeat_ngram_size=3)
    s._prompt = lambda language: [50258, 50259, 50359, 50363]
    pcm = np.zeros(16000, np.float32)
    s._window_decode(pcm, 1, "en")
    assert s._whisper.calls[-1]["repetition_penalty"] == 1.1 and s._whisper.calls[-1]["no_repeat_ngram_size"] == 3
    s._window_decode(pcm, 1, "en", draft={"draft_tokens": [400]})
    assert "repetition_penalty" not in s._whisper.calls[-1] and s._whisper.calls[-1]["draft_tokens"] == [400]
    s._window_decode(pcm, 3, "en", draft={"draft_trajectory": (np.zeros((1, 3), np.int32), np.zeros((1, 3), np.int32))}, want_traj=True)
    assert "no_repeat_ngram_size" not in s._whisper.calls[-1]
    s._window_decode(pcm, 3, "en", draft={}, want_traj=True)
    assert s._whisper.calls[-1]["no_repeat_ngram_size"] == 3 and s._whisper.calls[-1]["return_trajectory"] is True
