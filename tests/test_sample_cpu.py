"""not gpu: random sampling and n-best results on the host side - the reference's noise against published Philox answers, the reference sampler
against the softmax it must follow, and the plumbing: the shim's validation, the batcher key and capacity, openai-whisper's temperature
fallback as a pure function over a stub decode, the server's query parameters (tools/fake_engine_app.py: everything but the engine is real)."""
import asyncio
import os

import numpy as np
import pytest

import sample_ref as S


# ---- the noise ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("counter,key,want", [
    ((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
    ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), "d16cfe09 94fdcceb 5001e420 24126ea1")])
def test_philox_known_answers(counter, key, want):
    out = S.philox4x32_10([np.uint64(c) for c in counter], key)
    assert " ".join(f"{int(x):08x}" for x in out) == want
    # vectorised over the token id, as the sampler calls it
    ids = np.array([counter[0], 7, counter[0]], np.uint64)
    w = S.philox4x32_10((ids, np.uint64(counter[1]), np.uint64(counter[2]), np.uint64(counter[3])), key)[0]
    assert int(w[0]) == int(w[2]) == int(want.split()[0], 16) and w.dtype == np.uint32


def test_u_map_stays_inside_the_unit_interval_in_float32():
    lo, hi = S.u_of_word(np.uint32(0), np.float32), S.u_of_word(np.uint32(0xFFFFFFFF), np.float32)
    assert lo.dtype == np.float32 and 0.0 < float(lo) == 2.0 ** -24 and float(hi) == 1.0 - 2.0 ** -24 < 1.0
    # ... where the 24-bit form rounds to exactly 1 (g = +inf)
    assert np.float32((np.float32(0xFFFFFFFF >> 8) + np.float32(0.5)) * np.float32(2.0 ** -24)) == np.float32(1.0)
    g = S.gumbel_of_word(np.uint32([0, 0xFFFFFFFF]))
    assert np.isfinite(g).all() and -2.9 < g[0] < -2.8 and 16.6 < g[1] < 16.7
    assert np.array_equal(S.u_of_word(np.uint32([1 << 9, 511]), np.float32), np.float32([1.5 * 2.0 ** -23, 2.0 ** -24]))      # the low 9 bits are dropped


@pytest.mark.parametrize("topk,T", [(-1, 1.0), (-1, 0.5), (3, 1.7)])
def test_reference_sampler_follows_the_softmax(topk, T):
    toks = np.array([3, 900, 20000, 30000, 40000, 51000])
    x = np.array([1.2, 0.4, 0.0, -0.5, 0.9, -1.5], np.float32)
    lg = np.full(51865, -np.inf, np.float32); lg[toks] = x
    K = np.arange(6) if topk < 0 else np.argsort(-x, kind="stable")[:topk]
    p = np.exp(x[K].astype(np.float64) / T); p /= p.sum()
    counts = np.zeros(6, np.int64)
    lse = np.log(np.exp(x.astype(np.float64)).sum())
    for i in range(6000):
        t, gap, sc = S.draw(lg, T, topk, lambda idx, i=i: S.noise_words(idx, i % 7, i % 5, 1234 + i))
        k = int(np.flatnonzero(toks == t)[0])
        counts[k] += 1
        assert gap >= 0 and abs(sc - (float(x[k]) - lse) / float(np.float32(T))) < 1e-9          # the score: over ALL unmasked ids, also under top-k (T as the engine's fp32 holds it)
    assert counts[[i for i in range(6) if i not in K]].sum() == 0
    assert S.chi_square(counts[K], p) < S.CHI2_1E4[len(K) - 1], (counts, p)


def test_reference_search_rows_are_independent_and_frozen_at_eot():
    import torch
    V = 51865
    rows = torch.full((3, V), -np.inf)
    rows[:, [1000, 1001, S.EOT]] = torch.tensor([0.0, 0.0, 1.0])
    proc = dict(suppress_ids=(), suppress_begin=(), suppress_blank=False)
    r = S.sampled_search(lambda step, last: rows, 3, 6, -1, 1.0, 99, **proc)
    assert r["finish_step"] is not None and all(S.EOT not in s for s in r["ids"]) and len({len(s) for s in r["ids"]}) > 1
    one = [S.sampled_search(lambda step, last: rows[j:j + 1], 1, 6, -1, 1.0, 99, **proc) for j in range(1)]
    assert one[0]["ids"][0] == r["ids"][0]                                    # sample 0 alone = sample 0 of three (the counter carries j)
    a = S.sampled_search(lambda step, last: rows, 3, 6, 2, 0.7, 5, **proc)
    assert all(t in (1000, 1001, S.EOT) for s in a["ids"] for t in s) and all(1001 not in s for s in a["ids"])      # top-2: value desc, then id asc


# ---- the shim ---------------------------------------------------------------------------------------------------------------------------------------
def test_shim_validation_and_mapping():
    from wis_hip import ctranslate2 as ct2
    cs = ct2._check_sampling
    assert cs(5, 1, 1, 1) == (0, 1.0, 1) and cs(1, 1, 1, 0.3) == (0, 1.0, 1)          # off: today's call (the temperature is not read)
    assert cs(1, 5, 0, 0.7) == (-1, 0.7, 5) and cs(1, 1, 0, 1) == (-1, 1.0, 1) and cs(1, 8, 0, 2.0) == (-1, 2.0, 8)
    assert cs(5, 5, 1, 1) == (0, 1.0, 5) and cs(5, 2, 1, 1) == (0, 1.0, 2)            # n-best of a beam search
    for bad in ((1, 1, 17, 1), (1, 1, -1, 1), (1, 1, 2.5, 1), (1, 1, "x", 1), (1, 1, 0, 0), (1, 1, 0, -1), (1, 1, 0, float("nan")), (1, 1, 0, float("inf")),
                (1, 9, 0, 1), (1, 0, 0, 1), (1, 1.5, 0, 1), (2, 1, 0, 1), (5, 1, 4, 1), (1, 2, 1, 1), (3, 4, 1, 1), (1, 1, 1, 0)):
        with pytest.raises(ValueError):
            cs(*bad)
    # a top-k short of the whole vocabulary is the engine's, not this face's; more hypotheses than the search returns: both errors are the
    # ValueError of a bad request AND the NotImplementedError these options raised before they existed
    for unserved in ((1, 1, 2, 1), (1, 5, 16, 0.7), (1, 2, 1, 1), (3, 4, 1, 1)):
        with pytest.raises(NotImplementedError) as e:
            cs(*unserved)
        assert isinstance(e.value, ValueError)
    with pytest.raises(ValueError, match="draft"):
        cs(1, 1, 0, 1, drafted=True)
    with pytest.raises(ValueError, match="draft"):
        cs(5, 2, 1, 1, drafted=True)
    assert cs(1, 1, 1, 1, drafted=True) == (0, 1.0, 1)


def test_seed_source():
    from wis_hip import ctranslate2 as ct2
    try:
        ct2.set_random_seed(42)
        a = [ct2._next_seed() for _ in range(4)]
        ct2.set_random_seed(42)
        b = [ct2._next_seed() for _ in range(4)]
        ct2.set_random_seed(43)
        c = [ct2._next_seed() for _ in range(4)]
        assert a == b and a != c and len(set(a)) == 4 and all(0 <= x < 2 ** 64 for x in a)
    finally:
        ct2.set_random_seed(None)
    assert ct2._next_seed() != ct2._next_seed()          # os.urandom


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

    def spy(r, mel, prompts, opts, **kw):      # every engine call: its DecodeOptions by field name, the seeds, the batch size
        calls.append(dict(opts._asdict(), **kw, B=(int(mel) if kw.get("device_ptr") is not None else mel.shape[0])))
        return inner(r, mel, prompts, opts, **kw)
    monkeypatch.setattr(ct2, "_generate_chunk", spy)
    yield app, calls, model
    model.close()


def test_batcher_key_capacity_and_seeds(fake_app):
    from wis_hip import _lib, ctranslate2 as ct2
    app, calls, model = fake_app
    keys, rows_seen = [], []
    submit = model._batcher.submit
    model._batcher.submit = lambda key, rows, **kw: (keys.append(key), rows_seen.append(rows), submit(key, rows, **kw))[2]
    pcm = ct2.StorageView.from_array(np.zeros((2, _lib.N_SAMPLES), np.float32))
    prompt = [50258, 50259, 50359, 50363]
    g = lambda **kw: model.generate(pcm, [prompt] * 2, input_kind=_lib.WIS_IN_PCM_HOST, **kw)
    g(beam_size=1)
    g(beam_size=1, sampling_topk=1, num_hypotheses=1, sampling_temperature=0.5)
    todays = ct2.DecodeOptions(prompt_len=4, beam_size=1, max_new_tokens=224, length_penalty=1.0, patience=1.0, suppress_blank=True, suppress_default=True,
                               fixed_new_tokens=0, input_kind=_lib.WIS_IN_PCM_HOST, draft=None, return_trajectory=False, timestamps=False,
                               max_initial_timestamp_index=50, no_speech_prob=False, repetition_penalty=1.0, no_repeat_ngram_size=0, sampling_topk=0,
                               sampling_temperature=1.0, num_hypotheses=1)
    assert keys == [todays] * 2 and all(r[2] == 0 for rows in rows_seen for r in rows) and calls[-1]["sampling_topk"] == 0 and calls[-1]["num_hypotheses"] == 1
    g(beam_size=1, sampling_topk=0, sampling_temperature=0.6, num_hypotheses=5, sampling_seed=7)
    assert keys[-1] == todays._replace(sampling_topk=-1, sampling_temperature=0.6, num_hypotheses=5) and [r[2] for r in rows_seen[-1]] == [7, 7]
    assert (calls[-1]["sampling_topk"], calls[-1]["sampling_temperature"], calls[-1]["num_hypotheses"], calls[-1]["seeds"]) == (-1, 0.6, 5, [7, 7])
    g(beam_size=1, sampling_topk=0, sampling_temperature=0.6, num_hypotheses=5, sampling_seed=[8, 9])          # another seed: the same key
    assert keys[-1] == keys[-2] and calls[-1]["seeds"] == [8, 9]
    g(beam_size=1, sampling_topk=0, sampling_temperature=0.6, num_hypotheses=5, repetition_penalty=1.1)
    g(beam_size=1, sampling_topk=0, sampling_temperature=0.8, num_hypotheses=5)
    g(beam_size=1, sampling_topk=0, sampling_temperature=0.6, num_hypotheses=4)
    assert len(set(keys[-4:])) == 4 and keys[-3] == todays._replace(repetition_penalty=1.1, sampling_topk=-1, sampling_temperature=0.6, num_hypotheses=5)      # other values: other device batches
    assert len(set(calls[-1]["seeds"])) == 2                                                                 # unseeded: one draw per utterance
    g(beam_size=5, num_hypotheses=3)
    assert keys[-1] == todays._replace(beam_size=5, num_hypotheses=3) and calls[-1]["num_hypotheses"] == 3 and calls[-1]["sampling_topk"] == 0
    with pytest.raises(ValueError):
        g(beam_size=1, sampling_topk=0, sampling_seed=[1, 2, 3])
    with pytest.raises(ValueError):
        g(beam_size=5, num_hypotheses=6)                                                                     # beyond max_beam 5: rows per utterance
    with pytest.raises(ValueError, match="draft"):
        model.generate(ct2.StorageView.from_array(np.zeros((1, _lib.N_SAMPLES), np.float32)), [prompt], beam_size=1, input_kind=_lib.WIS_IN_PCM_HOST,
                       sampling_topk=0, draft_tokens=[400, 401])
    # capacity: max(beam, n) rows per utterance
    cap = lambda key: ct2._capacity(64, key)
    assert cap(todays) == 24 and cap(todays._replace(sampling_topk=-1, sampling_temperature=0.6, num_hypotheses=5)) == 19 and cap(todays._replace(sampling_topk=-1, num_hypotheses=8)) == 12
    assert cap(todays._replace(beam_size=5)) == 19 and cap(todays._replace(beam_size=5, num_hypotheses=3)) == 19
    # the device-resident form
    model.generate_from_device(0, 4096, prompt, beam_size=1, sampling_topk=0, sampling_temperature=0.4, sampling_seed=3)
    assert keys[-1] == todays._replace(input_kind=_lib.WIS_IN_MEL_DEV, sampling_topk=-1, sampling_temperature=0.4) and rows_seen[-1][0][2] == 3 and calls[-1]["seeds"] == [3]


# ---- the temperature fallback --------------------------------------------------------------------------------------------------------------------------
def test_fallback_rule_on_a_stub_decode():
    from wis_hip.whisper import compression_ratio, decode_with_fallback, parse_temperatures
    loop, fine = [7] * 60, list(range(100, 130))
    text_of = lambda toks: " ".join(f"w{t}" for t in toks)
    assert compression_ratio(text_of(loop)) > 2.4 > compression_ratio(text_of(fine)) > 0 and compression_ratio("") == 0.0
    seen = []

    def decode(table):
        def f(t, n):
            seen.append((t, n))
            return table[t]
        return f
    # the retry order, and a stop at the first acceptable result
    table = {0: [(loop, -0.2)], 0.2: [(loop, -0.3)] * 5, 0.4: [(fine, -0.5), (fine[:20], -0.4), (loop, -0.1)] + [(fine, -0.9)] * 2, 0.6: [(fine, -0.1)] * 5,
             0.8: [(fine, -0.05)] * 5}
    r = decode_with_fallback(decode(table), (0, 0.2, 0.4, 0.6, 0.8), 5, 2.4, -1.0, text_of)
    assert seen == [(0, 1), (0.2, 5), (0.4, 5), (0.6, 5)] and r["temperature"] == 0.6 and r["attempts"] == 4 and r["tokens"] == fine
    # best-of by AVERAGE log-probability (score * len / (len + 1)), the first among equals: at 0.4 the looping sample has the best one, so it is
    # what is judged - and retried; when the schedule ends there, the last result stands
    seen.clear()
    r = decode_with_fallback(decode(table), (0, 0.2, 0.4), 5, 2.4, -1.0, text_of)
    assert seen == [(0, 1), (0.2, 5), (0.4, 5)] and r["temperature"] == 0.4 and r["attempts"] == 3 and r["tokens"] == loop and r["compression_ratio"] > 2.4
    seen.clear()
    t2 = {0: [(fine, -1.5)], 0.5: [(fine, -0.7), (fine[:10], -0.6), (fine[:5], -0.6)]}
    r = decode_with_fallback(decode(t2), (0, 0.5), 3, 2.4, -1.0, text_of)               # a bad score retries; the best average wins, not the best score
    assert seen == [(0, 1), (0.5, 3)] and r["tokens"] == fine[:5] and r["avg_logprob"] == pytest.approx(-0.6 * 5 / 6)
    seen.clear()
    r = decode_with_fallback(decode(t2), (0, 0.5), 3, 2.4, None, text_of)               # threshold off: the first result stands
    assert seen == [(0, 1)] and r["temperature"] == 0 and r["avg_logprob"] == pytest.approx(-1.5 * 30 / 31)
    seen.clear()
    r = decode_with_fallback(decode(table), (0, 0.2), 5, 2.4, -1.0, None)               # no tokenizer vocabulary: no text, the log-probability alone decides
    assert seen == [(0, 1)] and r["compression_ratio"] is None
    r = decode_with_fallback(decode({0: [(fine, float("nan"))], 1.0: [(fine, -0.1)]}), (0, 1.0), 1, None, -1.0, None)      # NaN is not acceptable
    assert r["temperature"] == 1.0
    assert decode_with_fallback(decode(table), (), 5, 2.4, -1.0, text_of) is None
    assert parse_temperatures("0,0.2, 0.4", "5") == ((0.0, 0.2, 0.4), 5) and parse_temperatures((), 5) == ((), 5) and parse_temperatures([0, 1], 1) == ((0.0, 1.0), 1)
    for bad in (("a", 5), ("0,-0.2", 5), ("nan", 5), ("inf", 5), ("0", 0), ("0", 9), ("0", "x"), ("0", 2.5)):
        with pytest.raises(ValueError):
            parse_temperatures(*bad)


def _clip():
    root = os.path.dirname(os.path.abspath(__file__))
    with open(os.path.join(root, "golden", "clips", "3sec.flac"), "rb") as f:
        return f.read()


def test_do_whisper_fallback_and_the_servers_400s(fake_app):
    import httpx
    from wis_hip.settings import APISettings
    from wis_hip.whisper import do_whisper
    app, calls, _ = fake_app
    s = APISettings()
    assert (list(s.temperatures), s.best_of, s.compression_ratio_threshold, s.logprob_threshold) == ([], 5, 2.4, -1.0)
    models = app.state.wis["models"]
    pcm = np.zeros(16000, np.float32)
    do_whisper(pcm, "large", 1, models=models)                                           # the default: no fallback, today's single call
    assert len(calls) == 1 and calls[-1]["sampling_topk"] == 0 and calls[-1]["num_hypotheses"] == 1
    # the fake engine answers score -0.5 over 16 tokens: acceptable at once
    r = do_whisper(pcm, "large", 1, models=models, temperatures=(0, 0.4), best_of=3)
    assert len(calls) == 2 and calls[-1]["sampling_topk"] == 0 and calls[-1]["num_hypotheses"] == 1 and r.fallback["temperature"] == 0 and r.fallback["attempts"] == 1
    # a log-probability threshold nothing meets: every temperature is tried, the later ones sampled with best_of samples at beam 1
    r = do_whisper(pcm, "large", 5, models=models, temperatures=(0, 0.4, 0.8), best_of=3, logprob_threshold=-0.1)
    assert len(calls) == 5 and [(c["sampling_topk"], c["sampling_temperature"], c["num_hypotheses"]) for c in calls[2:]] == \
        [(0, 1.0, 1), (-1, 0.4, 3), (-1, 0.8, 3)]
    assert r.fallback["attempts"] == 3 and r.fallback["temperature"] == 0.8 and r.tokens == [400 + i for i in range(16)]
    with pytest.raises(ValueError):
        do_whisper(np.zeros(16000 * 31, np.float32), "large", 1, models=models, temperatures=(0, 0.4))
    with pytest.raises(ValueError):
        do_whisper(pcm, "large", 1, models=models, temperatures=(0, -1))
    flac = _clip()
    n0 = len(calls)

    async def go():
        async with httpx.AsyncClient(transport=httpx.ASGITransport(app=app), base_url="http://wis") as c:
            r = await c.post("/api/willow?model=large&temperatures=0,0.2,0.4&best_of=2", content=flac, headers={"x-audio-codec": "flac"})
            assert r.status_code == 200, r.text
            assert len(calls) == n0 + 1                  # accepted at temperature 0
            for q in ("temperatures=a", "temperatures=0,-0.2", "temperatures=0,nan", "best_of=0", "best_of=9", "best_of=x", "temperatures=0,0.2&best_of=1.5"):
                r = await c.post(f"/api/willow?model=large&{q}", content=flac, headers={"x-audio-codec": "flac"})
                assert r.status_code == 400 and ("temperatures" in r.json()["error"] or "best_of" in r.json()["error"]), (q, r.status_code, r.text)
            assert len(calls) == n0 + 1                  # nothing else reached the engine

    asyncio.run(go())
