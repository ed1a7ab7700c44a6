"""-m gpu: hotword boosting end to end - wis_generate / wis_generate_n / wis_generate_ragged inside captured step graphs, through
`ctranslate2.Whisper.generate(..., hotwords=, hotword_boost=)`, `do_whisper` and `/api/asr` - on the tiny and base models (seeded weights).

`generate` is compared against the ORACLE's search with the reference step function in front of its processors (tests/hotword_ref.py
generate_hot): ids identical whenever the oracle's decision margin exceeds the 0.02 tests/test_gpu_e2e.py uses, engine scores within that file's
3e-3 of the oracle's rescoring of the engine's ids under the boosted rows.  At most one case in eight may be excused by the margin: entries
and boost were chosen on the CPU (the entries are words over the best ids of the seeded models' own first step, so a boost of 3 decides) and the test
asserts the cap and prints the margins."""
import asyncio
import os
import threading

import numpy as np
import pytest

from hotword_ref import generate_hot, rescore_hot

pytestmark = pytest.mark.gpu
EOT = 50257
PROMPT = [50258, 50259, 50359, 50363]
LONG_PROMPT = [50361] + [1000 + 7 * i for i in range(30)] + PROMPT      # 35 tokens: the long-prompt route
MARGIN = 0.02
FIXED = 8
BOOST = 3.0
# the 40 best ids of the seeded models' first step behind PROMPT (the oracle's, computed on the CPU): what a moderate boost can make win
POOL = {
    "tiny": [50046, 29738, 20156, 38589, 51022, 31452, 39725, 47255, 3121, 20312, 5164, 40931, 36301, 33068, 23411, 9988, 32148, 32335, 17641, 29373, 9195, 18372, 5611,
             41829, 31602, 15049, 47183, 27740, 35350, 20399, 47688, 5810, 50758, 20658, 33489, 3087, 22293, 14456, 19156, 42282],
    "base": [7982, 13840, 22217, 17023, 15095, 39597, 798, 48092, 24937, 12750, 23384, 3662, 7083, 29050, 45437, 39741, 43407, 4107, 29362, 45564, 20735, 22568, 12254,
             6897, 4824, 44754, 49029, 162, 1396, 3105, 7362, 19828, 16191, 2567, 37905, 18733, 18911, 27747, 21121, 44326],
}
SET_SEED = {"tiny": 7, "base": 1}      # chosen on the CPU: the oracle's decision margins of the eight cases are 0.03 .. 0.84 with these sets


def _entries(which, seed=None):
    """eight entries over ten ids of the model's pool: nested ([a, b] / [a, b, c]), self-overlapping ([e, e, f]), one-token, a four-token one"""
    rng = np.random.default_rng(SET_SEED[which] if seed is None else seed)
    t = [int(x) for x in rng.choice(POOL[which], size=10, replace=False)]
    return [[t[0], t[1]], [t[0], t[1], t[2]], [t[3]], [t[4], t[4], t[5]], [t[5], t[6]], [t[7]], [t[8], t[0]], [t[9], t[9], t[7], t[3]]]


ENTRIES = _entries("tiny")
OTHER = [[27740, 5164], [47255]]


@pytest.fixture(scope="module")
def mels(golden_dir):
    return np.stack([np.load(os.path.join(golden_dir, f"logmel_{c}.npz"))["mel"] for c in ("3sec", "10sec")]).astype(np.float32)


def _make(size):
    from oracle.whisper_ref import WhisperRef
    from wis_hip import ctranslate2 as ct2, weights as W
    w = W.synthetic_weights(size, seed=1234, std=0.02, emb_std=0.06, ln_jitter=0.1)
    a = W.arch(size)
    model = ct2.Whisper("unused", weights=w, arch=a, max_batch=4, max_beam=5)
    return model, WhisperRef(w, a["d_model"], a["n_layers"], a["n_heads"])


@pytest.fixture(scope="module")
def tiny():
    m = _make("tiny")
    yield m
    m[0].close()


@pytest.fixture(scope="module")
def base():
    m = _make("base")
    yield m
    m[0].close()


@pytest.fixture(scope="module")
def memories(tiny, base, mels):
    """the oracle's encoder output of the 3 s clip, once per model"""
    return {"tiny": tiny[1].encode(mels[:1])[0].numpy(), "base": base[1].encode(mels[:1])[0].numpy()}


def _gen(model, mel, prompt, beam, **kw):
    from wis_hip import ctranslate2 as ct2
    return model.generate(ct2.StorageView.from_array(mel), [prompt] * mel.shape[0], beam_size=beam, return_scores=True, fixed_new_tokens=FIXED, **kw)


def _oracle(ref, memory, prompt, beam, entries, boost):
    from wis_hip import weights as W
    return generate_hot(ref, prompt, beam, entries, boost, W.SUPPRESS_IDS, W.SUPPRESS_IDS_BEGIN, memory, fixed_new=FIXED)


def _check_against_the_oracle(which, ref, memory, prompt, beam, got, entries, boost=BOOST):
    """-> (the oracle's search record, excused by the margin rule)"""
    from wis_hip import weights as W
    r = _oracle(ref, memory, prompt, beam, entries, boost)
    ids, gscore = got.sequences_ids[0], got.scores[0]
    margin = min(r["trace"])
    rescored = rescore_hot(ref, prompt, ids, entries, boost, W.SUPPRESS_IDS, W.SUPPRESS_IDS_BEGIN, memory, fixed_new=FIXED)
    print(f"  [hotwords] {which} beam {beam} prompt {len(prompt)}: oracle {r['ids']} score {r['score']:.5f} decision margin {margin:.4f} | engine {ids} score {gscore:.5f}, "
          f"oracle rescoring of the engine's ids {rescored:.5f} | identical {ids == r['ids']}")
    assert abs(gscore - rescored) <= 3e-3, (gscore, rescored)
    assert rescored >= r["score"] - 1e-2, (rescored, r["score"])
    if margin > MARGIN:
        assert ids == r["ids"], (ids, r["ids"])
    return r, not margin > MARGIN


def test_generate_equals_the_oracle(tiny, base, mels, memories):
    """The eight cases - tiny and base, beam 1 and 5, the short prompt and the long-prompt route - in one test: each against its oracle, then the
    cap over all eight (at most one in eight excused by the oracle's own margin) and at least one configuration whose boosted result differs from
    the plain one AND equals the oracle's boosted result (a kernel that does nothing could not pass)."""
    mel = np.ascontiguousarray(mels[:1])
    margins, excused, decided = [], 0, 0
    for which, (model, ref) in (("tiny", tiny), ("base", base)):
        entries = _entries(which)
        for beam in (1, 5):
            for prompt in (PROMPT, LONG_PROMPT):
                got = _gen(model, mel, prompt, beam, hotwords=entries, hotword_boost=BOOST)[0]
                r, skip = _check_against_the_oracle(which, ref, memories[which], prompt, beam, got, entries)
                plain = _gen(model, mel, prompt, beam)[0]
                margins.append(round(float(min(r["trace"])), 4))
                excused += int(skip)
                decided += int(plain.sequences_ids[0] != got.sequences_ids[0] and got.sequences_ids[0] == r["ids"])
    print(f"\n[hotwords] end to end: {len(margins)} cases, decision margins {margins}, {excused} excused, {decided} decided by the boost")
    assert len(margins) == 8 and excused <= len(margins) // 8, (margins, excused)
    assert decided >= 1, decided


def test_ragged_prompts(tiny, mels, memories):
    """prompts of different lengths in one device batch (wis_generate_ragged): each row equals its own oracle"""
    from wis_hip import ctranslate2 as ct2
    model, ref = tiny
    both = np.ascontiguousarray(np.concatenate([mels[:1], mels[:1]]))
    for beam in (1, 5):
        rr = model.generate(ct2.StorageView.from_array(both), [LONG_PROMPT, PROMPT], beam_size=beam, return_scores=True, fixed_new_tokens=FIXED, hotwords=ENTRIES,
                            hotword_boost=BOOST, ragged_prompts=True)
        for row, prompt in zip(rr, (LONG_PROMPT, PROMPT)):
            from wis_hip import weights as W
            r = _oracle(ref, memories["tiny"], prompt, beam, ENTRIES, BOOST)
            rescored = rescore_hot(ref, prompt, row.sequences_ids[0], ENTRIES, BOOST, W.SUPPRESS_IDS, W.SUPPRESS_IDS_BEGIN, memories["tiny"], fixed_new=FIXED)
            print(f"  [hotwords] ragged beam {beam} prompt {len(prompt)}: margin {min(r['trace']):.4f}, identical {row.sequences_ids[0] == r['ids']}")
            assert abs(row.scores[0] - rescored) <= 3e-3
            if min(r["trace"]) > MARGIN:
                assert row.sequences_ids[0] == r["ids"], (beam, len(prompt), row.sequences_ids[0], r["ids"])


def test_two_boosts_and_an_absorbed_one(tiny, mels, memories):
    """One step graph serves every boost: two calls with different boosts, one after the other on one handle, each equal to ITS oracle and no
    graph captured between them.  A boost every fp32 addition absorbs (2^-60) returns the plain call's ids and scores bit for bit; without
    `hotwords`, generate returns what it returned."""
    import ctypes as C
    from wis_hip import _lib
    model, ref = tiny
    mel = np.ascontiguousarray(mels[:1])

    def graphs():
        n = C.c_int(0)
        _lib.check(_lib.load().wis_debug_graph_count(model._replicas[0].handle, C.byref(n)))
        return n.value
    plain = _gen(model, mel, PROMPT, 5)[0]
    a = _gen(model, mel, PROMPT, 5, hotwords=ENTRIES, hotword_boost=2.0)[0]
    g = graphs()
    b = _gen(model, mel, PROMPT, 5, hotwords=ENTRIES, hotword_boost=6.0)[0]
    c = _gen(model, mel, PROMPT, 5, hotwords=OTHER, hotword_boost=6.0)[0]      # another set, of another size: the same graphs
    assert graphs() == g
    for got, entries, boost in ((a, ENTRIES, 2.0), (b, ENTRIES, 6.0), (c, OTHER, 6.0)):
        from wis_hip import weights as W
        r = _oracle(ref, memories["tiny"], PROMPT, 5, entries, boost)
        rescored = rescore_hot(ref, PROMPT, got.sequences_ids[0], entries, boost, W.SUPPRESS_IDS, W.SUPPRESS_IDS_BEGIN, memories["tiny"], fixed_new=FIXED)
        print(f"  [hotwords] boost {boost}: margin {min(r['trace']):.4f}, identical {got.sequences_ids[0] == r['ids']}")
        assert abs(got.scores[0] - rescored) <= 3e-3, (boost, got.scores[0], rescored)
        if min(r["trace"]) > MARGIN:
            assert got.sequences_ids[0] == r["ids"], (boost, got.sequences_ids[0], r["ids"])
    assert a.scores[0] != b.scores[0]
    tiny_boost = _gen(model, mel, PROMPT, 5, hotwords=ENTRIES, hotword_boost=2.0 ** -60)[0]
    assert tiny_boost.sequences_ids == plain.sequences_ids and tiny_boost.scores == plain.scores
    again = _gen(model, mel, PROMPT, 5)[0]
    assert again.sequences_ids == plain.sequences_ids and again.scores == plain.scores


def test_combined_with_timestamps_sampling_and_n_best(tiny, mels):
    """What combines, combines: a timestamp prompt, a sampled call with a fixed seed (the same seed gives the same samples, the boost changes
    them), n-best of a beam search, the repetition options.  A refused combination is a ValueError."""
    from wis_hip import ctranslate2 as ct2
    model, _ = tiny
    f = ct2.StorageView.from_array(np.ascontiguousarray(mels[:1]))
    hot = dict(hotwords=ENTRIES, hotword_boost=BOOST)
    from ts_ref import grammar_errors
    ts = model.generate(f, [PROMPT[:3]], beam_size=5, max_length=40, hotwords=ENTRIES, hotword_boost=6.0)[0]
    ts0 = model.generate(f, [PROMPT[:3]], beam_size=5, max_length=40)[0]
    # (the search under the timestamp rules is held to its reference exactly in tests/test_gpu_hotword_rules.py; here: the rules still hold, the boost acted)
    assert not grammar_errors(ts.sequences_ids[0]) and ts.sequences_ids[0] != ts0.sequences_ids[0], (ts.sequences_ids[0], ts0.sequences_ids[0])
    s1 = model.generate(f, [PROMPT], beam_size=1, num_hypotheses=3, sampling_topk=0, sampling_temperature=0.7, sampling_seed=5, fixed_new_tokens=FIXED, **hot)[0]
    s2 = model.generate(f, [PROMPT], beam_size=1, num_hypotheses=3, sampling_topk=0, sampling_temperature=0.7, sampling_seed=5, fixed_new_tokens=FIXED, **hot)[0]
    s0 = model.generate(f, [PROMPT], beam_size=1, num_hypotheses=3, sampling_topk=0, sampling_temperature=0.7, sampling_seed=5, fixed_new_tokens=FIXED)[0]
    assert s1.sequences_ids == s2.sequences_ids and s1.sequences_ids != s0.sequences_ids
    nb = model.generate(f, [PROMPT], beam_size=5, num_hypotheses=3, return_scores=True, fixed_new_tokens=FIXED, repetition_penalty=1.2, no_repeat_ngram_size=2, **hot)[0]
    assert len(nb.sequences_ids) == 3 and list(nb.scores) == sorted(nb.scores, reverse=True)
    for kw in (dict(phrases=[[2425]]), dict(beam_size=1, draft_tokens=[400, 401]), dict(hotword_boost=0.0), dict(hotword_boost=float("nan"))):
        with pytest.raises(ValueError):
            model.generate(f, [PROMPT], **{**dict(beam_size=5, **hot), **kw})


def test_concurrent_calls_with_different_lists_never_share_a_device_batch(tiny, mels, monkeypatch):
    from wis_hip import ctranslate2 as ct2
    model, _ = tiny
    mel = np.ascontiguousarray(mels[:1])
    solo = {name: _gen(model, mel, PROMPT, 5, hotwords=lst, hotword_boost=b)[0] for name, (lst, b) in dict(a=(ENTRIES, BOOST), b=(OTHER, BOOST), c=(ENTRIES, 5.0)).items()}
    seen, chunk = [], ct2._generate_chunk

    def recording(r, mel_, prompts, opts, *rest, **kw):
        seen.append((opts, int(mel_) if kw.get("device_ptr") is not None else mel_.shape[0]))
        return chunk(r, mel_, prompts, opts, *rest, **kw)
    monkeypatch.setattr(ct2, "_generate_chunk", recording)
    out = {}

    def call(name, lst, b, i):
        out[(name, i)] = _gen(model, mel, PROMPT, 5, hotwords=lst, hotword_boost=b)[0]
    th = [threading.Thread(target=call, args=(name, lst, b, i)) for i in range(2) for name, (lst, b) in dict(a=(ENTRIES, BOOST), b=(OTHER, BOOST), c=(ENTRIES, 5.0)).items()]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert len(out) == 6 and sum(n for _, n in seen) == 6
    for opts, n in seen:
        assert type(opts) is ct2.BoostedOptions and n <= 2      # a batch holds the rows of ONE (list, boost): two at the most here
    for (name, _), r in out.items():
        assert r.sequences_ids == solo[name].sequences_ids, name
    assert len({(o.hotword_digest, o.hotword_boost) for o, _ in seen}) == 3


class _Vocab:
    """a tokenizer with a vocabulary: every word is one token (its id spelled out), " " + text.strip() as a prompt is encoded"""
    has_vocabulary, all_special_ids = True, []
    decode = staticmethod(lambda ids: "".join(f" w{int(t)}" for t in ids if int(t) < EOT))

    @staticmethod
    def encode(text):
        assert text.startswith(" ")
        return [int(w[1:]) for w in text.split()]


def test_do_whisper_and_the_server(golden_dir, monkeypatch):
    """do_whisper(hotwords=[text or ids], hotword_boost=) equals generate with the same ids; one /api/asr request with the query parameters equals
    it; long_form=seek over a two-window recording hands the option to every window's decode."""
    import httpx
    from wis_hip import audio, ctranslate2 as ct2
    from wis_hip.server import create_app
    from wis_hip.settings import APISettings
    from wis_hip.whisper import WhisperModels, do_whisper
    s = APISettings()
    s.whisper_model_path = "synthetic:{size}"
    s.fixed_new_tokens = FIXED
    s.fuse_logmel = True      # (the 30 s PCM window goes to the engine as it is: what the direct generate call below hands over too)
    models = WhisperModels(s, device_index=[0])
    try:
        mdl = models.get("tiny")
        models.tokenizers["tiny"] = _Vocab()
        clip = os.path.join(golden_dir, "clips", "3sec.flac")
        pcm, _ = audio.load_audio(clip)
        texts = ["w29738 w38589", " w20156 ", [3121, 40931], "w5164"]
        ids = [[29738, 38589], [20156], [3121, 40931], [5164]]
        plain = do_whisper(pcm, "tiny", 5, "transcribe", False, "en", models=models)
        hot = do_whisper(pcm, "tiny", 5, "transcribe", False, "en", models=models, hotwords=texts, hotword_boost=6.0)
        assert hot.tokens != plain.tokens and hot.matches is None
        window = ct2.StorageView.from_array(np.ascontiguousarray(audio.pad_or_trim(pcm)[None], np.float32))
        direct = mdl.generate(window, [PROMPT], beam_size=5, fixed_new_tokens=FIXED, input_kind=ct2._lib.WIS_IN_PCM_HOST, hotwords=ids, hotword_boost=6.0)[0]
        assert hot.tokens == direct.sequences_ids[0], (hot.tokens, direct.sequences_ids[0])      # the text entries became exactly these ids
        dropped = mdl.generate(window, [PROMPT], beam_size=5, fixed_new_tokens=FIXED, input_kind=ct2._lib.WIS_IN_PCM_HOST, hotwords=ids[1:], hotword_boost=6.0)[0]
        unspaced = do_whisper(pcm, "tiny", 5, "transcribe", False, "en", models=models, hotwords=[t if isinstance(t, list) else " " + t.strip() for t in texts], hotword_boost=6.0)
        assert unspaced.tokens == hot.tokens      # (" " + text.strip(): the leading space is the tokeniser's business, not the caller's)
        print(f"  [hotwords] do_whisper == generate: {hot.tokens}; without the first entry: {dropped.sequences_ids[0]}")
        with pytest.raises(ValueError):
            do_whisper(pcm, "tiny", 5, "transcribe", False, "en", models=models, hotwords=texts)                       # no boost anywhere
        with pytest.raises(ValueError):
            do_whisper(pcm, "tiny", 5, "transcribe", False, "en", models=models, hotwords=texts, hotword_boost=6.0, phrases=[[2425]])
        # the settings' list and boost serve a request that names neither
        s.hotword_boost = 6.0
        monkeypatch.setattr("wis_hip.whisper.load_hotwords_file", lambda path: list(texts))
        assert do_whisper(pcm, "tiny", 5, "transcribe", False, "en", models=models).tokens == hot.tokens
        s.hotword_boost = 0.0
        assert do_whisper(pcm, "tiny", 5, "transcribe", False, "en", models=models).tokens == plain.tokens      # a list with a boost of 0: off
        monkeypatch.undo()
        # /api/asr with the query parameters
        app = create_app(models=models)
        b = "xYzBoundary123"
        flac = open(clip, "rb").read()
        body = (f"--{b}\r\nContent-Disposition: form-data; name=\"audio_file\"; filename=\"a.flac\"\r\nContent-Type: application/octet-stream\r\n\r\n").encode() + flac + f"\r\n--{b}--\r\n".encode()
        hdr = {"content-type": f"multipart/form-data; boundary={b}"}

        async def go():
            async with httpx.AsyncClient(transport=httpx.ASGITransport(app=app), base_url="http://wis", timeout=120) as c:
                q = "hotwords=w29738 w38589|w20156|ids:3121,40931|w5164&hotword_boost=6.0"
                r = await c.post(f"/api/asr?model=tiny&beam_size=5&detect_language=False&force_language=en&{q}", content=body, headers=hdr)
                assert r.status_code == 200, r.text
                r0 = await c.post("/api/asr?model=tiny&beam_size=5&detect_language=False&force_language=en", content=body, headers=hdr)
                r2 = await c.post("/api/asr?model=tiny&beam_size=5&hotwords=ids:3121", content=body, headers=hdr)
                return r.json()["text"], r0.json()["text"], r2.status_code
        text, text0, rc2 = asyncio.run(go())
        flac_hot = do_whisper(clip, "tiny", 5, "transcribe", False, "en", models=models, hotwords=texts, hotword_boost=6.0)
        flac_plain = do_whisper(clip, "tiny", 5, "transcribe", False, "en", models=models)
        assert text == flac_hot[1] and text0 == flac_plain[1] and text != text0 and rc2 == 400
        # long_form=seek over two windows: every window's decode carries the option
        seen, gfd = [], mdl.generate_from_device

        def spy(*a, **kw):
            seen.append((kw.get("hotwords"), kw.get("hotword_boost")))
            return gfd(*a, **kw)
        monkeypatch.setattr(mdl, "generate_from_device", spy)
        long_pcm = np.concatenate([pcm] * 10)[:16000 * 36]
        r = do_whisper(long_pcm, "tiny", 5, "transcribe", False, "en", models=models, long_form="seek", hotwords=texts, hotword_boost=6.0)
        assert len(r.seek) >= 2 and len(seen) >= 2 and all(h == ids and bst == 6.0 for h, bst in seen), (len(r.seek), seen)
        monkeypatch.undo()
        r0 = do_whisper(long_pcm, "tiny", 5, "transcribe", False, "en", models=models, long_form="seek")
        assert r0.tokens != r.tokens
    finally:
        models.get("tiny").close()
