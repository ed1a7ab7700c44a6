"""Hotword boosting, host side (no GPU): the brute-force statement of THE HOTWORD RULE (tests/hotword_ref.py boost_rows) against a second,
independently written formulation (an incremental set of active prefixes) on random sets and histories, the fixed cases the GPU tap test runs
(tests/test_gpu_hotword_ops.py) on the CPU first, the trie builder and its messages, BoostedOptions' equality / hash / pickle and the
micro-batcher's rule on a fake engine, do_whisper's option resolution against the settings, the server's 400s and `hotwords_file`."""
import asyncio
import os
import pickle
import time

import numpy as np
import pytest

from hotword_ref import active_nodes_boost_set, boost_rows, boost_set
from phrase_ref import prefix_dict, trie_to_prefix_dict

EOT = 50257
V = 51865
PROMPT = [50258, 50259, 50359, 50363]


def _pool():
    from wis_hip import weights as W
    bad = set(W.SUPPRESS_IDS) | set(W.SUPPRESS_IDS_BEGIN)
    return [t for t in range(EOT) if t not in bad]


def test_brute_force_equals_the_active_set_formulation():
    """A few hundred random sets over a small alphabet (so suffixes overlap, repeat and nest) and random histories of 0 .. 70 tokens, some with
    ids outside the vocabulary: both formulations give the same boost set; the cases are not trivial (asserted)."""
    rng = np.random.default_rng(11)
    deep = multi = broken = 0
    for case in range(300):
        alphabet = rng.choice(_pool()[:5000], size=int(rng.integers(2, 6)), replace=False).tolist()
        entries = [rng.choice(alphabet, size=int(rng.integers(1, 33 if case % 10 == 0 else 7))).tolist() for _ in range(int(rng.integers(1, 12)))]
        pre = prefix_dict(entries)
        for _ in range(6):
            hist = rng.choice(alphabet, size=int(rng.integers(0, 71))).tolist()
            if rng.random() < 0.2 and hist:
                hist[int(rng.integers(0, len(hist)))] = int(rng.choice([-1, V, V + 9, 2 ** 31 - 1]))
                broken += 1
            a, b = boost_set(pre, hist, V), active_nodes_boost_set(pre, hist, V)
            assert a == b, (entries, hist, a, b)
            assert set(pre[()][0]) <= set(a)                      # the root's children are always in
            active = [k for k in range(min(len(hist), 31) + 1) if tuple(hist[len(hist) - k:]) in pre and all(0 <= t < V for t in hist[len(hist) - k:])]
            multi += int(len(active) >= 3)
            deep += int(max(active) >= 4)
    assert multi >= 100 and deep >= 50 and broken >= 100, (multi, deep, broken)


def test_fixed_cases():
    """The cases tests/test_gpu_hotword_ops.py feeds the kernel, on the CPU first."""
    a, b, c, x = 400, 401, 402, 999
    pre = prefix_dict([[a, b], [a, b, c]])
    assert boost_set(pre, [x, a, b], V) == [a, c]                            # after `a b`: c (and the root's a); <|endoftext|> is not boosted at the entry's end
    assert EOT not in boost_set(pre, [a, b], V) and boost_set(pre, [a, b, c], V) == [a]
    pre = prefix_dict([[a, a, b]])
    assert boost_set(pre, [x, a, a, a], V) == [a, b]                         # suffixes (), (a), (a, a) are active: a named twice, b once
    row = np.zeros((1, V), np.float32)
    out = boost_rows(row, [[x, a, a, a]], pre, 2.5)
    assert out[0, a] == np.float32(2.5) and out[0, b] == np.float32(2.5) and np.count_nonzero(out) == 2      # x + boost, never x + 2 boost
    pre = prefix_dict([[c], [a, c], [b, a, c], [x, b, a, c]])                # c is named by the suffixes (), (a), (b, a), (x, b, a)
    out = boost_rows(row, [[x, b, a]], pre, 1.0)
    assert out[0, c] == 1.0 and boost_set(pre, [x, b, a], V) == sorted([a, b, c, x])
    # broken suffixes: an id outside [0, n_vocab) ends every suffix that holds it
    pre = prefix_dict([[a, b, c], [b, x]])
    assert boost_set(pre, [a, -1, b], V) == [a, b, x] and boost_set(pre, [a, V, b], V) == [a, b, x] and boost_set(pre, [a, b], V) == [a, b, c, x]
    assert boost_set(pre, [a, b, V + 3], V) == [a, b]
    # one float32 addition: -inf, +inf and NaN stay, a denormal and -0.0 take the boost
    vals = np.asarray([[-np.inf, np.inf, np.nan, 1e-42, -0.0]], np.float32)
    pre = prefix_dict([[0], [1], [2], [3], [4]])
    out = boost_rows(vals, [[]], pre, 3.0, n_vocab=5, eot=5)
    assert np.isneginf(out[0, 0]) and np.isposinf(out[0, 1]) and np.isnan(out[0, 2]) and out[0, 3] == np.float32(3.0) and out[0, 4] == np.float32(3.0)
    assert boost_rows(vals, [None], pre, 3.0, n_vocab=5, eot=5).view(np.uint32).tolist() == vals.view(np.uint32).tolist()
    # a boost below half an ulp of every value is absorbed
    row = np.full((1, 8), 1.5, np.float32)
    assert boost_rows(row, [[]], prefix_dict([[1], [2]]), 2.0 ** -60, n_vocab=8, eot=7).tobytes() == row.tobytes()
    # the longest suffix that counts holds 31 tokens: an entry of 32 is followed to its last token
    chain = [int(t) for t in _pool()[100:132]]
    pre = prefix_dict([chain])
    assert boost_set(pre, [x] * 40 + chain[:31], V) == sorted([chain[0], chain[31]]) and boost_set(pre, chain, V) == [chain[0]]


def test_builder_and_its_messages():
    from wis_hip import weights as W
    entries = [[400, 401, 402], [400, 401], [400, 500], [600]]
    trie = W.build_hotword_trie(entries)
    assert np.array_equal(trie, W.build_phrase_trie(entries)) and trie_to_prefix_dict(trie) == prefix_dict(entries)
    for bad, word in (([], "hotword list"), ([[400, EOT]], "hotword [400, 50257]"), ([[]], "hotword []"), ([[220]], "hotword [220]"),
                      ([[int(t) for t in _pool()[:33]]], "33 tokens")):
        with pytest.raises(ValueError) as e:
            W.build_hotword_trie(bad)
        assert word in str(e.value) and "phrase" not in str(e.value), (bad, str(e.value))
    assert len(W.build_hotword_trie([[7, 8]], suppress_ids=[], suppress_begin=[])) == 3


@pytest.fixture(scope="module")
def model():
    from wis_hip import ctranslate2 as ct2, weights as W
    m = ct2.Whisper.from_handles([(None, 0)], W.arch("large"))
    yield m
    m._batcher.close()


def _opts(model, prompts=(PROMPT,), **kw):
    from wis_hip import _lib
    args = dict(input_kind=_lib.WIS_IN_MEL_DEV, n_utt=len(prompts), beam_size=5, patience=1, num_hypotheses=1, length_penalty=1, repetition_penalty=1,
                no_repeat_ngram_size=0, max_length=448, return_no_speech_prob=False, max_initial_timestamp_index=50, suppress_blank=True,
                suppress_default=True, sampling_topk=1, sampling_temperature=1, fixed_new_tokens=0, draft_tokens=None, draft_trajectory=None,
                return_trajectory=False)
    args.update(kw)
    return model._decode_options(None, list(prompts), **args)[0]


def test_boosted_options(model):
    import ctypes as C
    from wis_hip import _lib, ctranslate2 as ct2
    a, b = [[400, 401], [500]], [[400, 401], [501]]
    plain = _opts(model)
    assert type(plain) is ct2.DecodeOptions and type(_opts(model, hotwords=None)) is ct2.DecodeOptions      # the record a plain call has always built
    ha, ha2, hb, ha3 = (_opts(model, hotwords=a, hotword_boost=2.5), _opts(model, hotwords=[[500], [400, 401], [500]], hotword_boost=2.5),
                        _opts(model, hotwords=b, hotword_boost=2.5), _opts(model, hotwords=a, hotword_boost=3.0))
    assert type(ha) is ct2.BoostedOptions and ha._fields == plain._fields and tuple(ha) == tuple(plain)      # every value as the plain record
    assert ha == ha2 and hash(ha) == hash(ha2) and not ha != ha2                    # the same SET and boost: one class
    assert ha != hb and ha != ha3 and len({ha, ha2, hb, ha3}) == 3                  # another set, another boost: other classes
    assert ha != plain and plain != ha and not ha == plain and not plain == ha and len({plain, ha}) == 2
    ca = _opts(model, phrases=a)
    assert ca != ha and ha != ca and not ha == ca and len({ca, ha}) == 2            # nor a constrained call's
    r = ha._replace(prompt_len=7)
    assert type(r) is ct2.BoostedOptions and r.prompt_len == 7 and r.hotword_digest == ha.hotword_digest and r.hotword_boost == 2.5 and r != ha
    p = pickle.loads(pickle.dumps(ha))
    assert type(p) is ct2.BoostedOptions and p == ha and hash(p) == hash(ha) and np.array_equal(p.hotword_trie, ha.hotword_trie) and p.hotword_boost == 2.5
    o = ct2._gen_opts(ha)      # a boosted call builds the struct in full; every other call the record it has always built
    assert type(o) is _lib.HotGenOpts and o.hotwords == 1 and o.hotword_boost == 2.5 and o.phrases == 0 and o.max_new_tokens == plain.max_new_tokens
    po = ct2._gen_opts(plain)
    assert type(po) is _lib.GenOpts and bytes(o)[:C.sizeof(_lib.GenOpts)] == bytes(po)
    assert _opts(model, hotwords=a, hotword_boost=2.5, beam_size=2) != ha and ct2._capacity(8, ha) == ct2._capacity(8, plain)
    # what combines: timestamps, sampling, n-best, the repetition options, a long prompt, ragged prompts
    long_prompt = [50361] + list(range(400, 430)) + PROMPT
    for kw in (dict(prompts=([50258, 50259, 50359],)), dict(beam_size=1, sampling_topk=0, num_hypotheses=3), dict(num_hypotheses=3),
               dict(repetition_penalty=1.3, no_repeat_ngram_size=2), dict(prompts=(long_prompt,)), dict(prompts=(long_prompt, PROMPT), ragged_prompts=True),
               dict(fixed_new_tokens=4)):
        assert type(_opts(model, hotwords=a, hotword_boost=1.0, **kw)) is ct2.BoostedOptions, kw


def test_the_options_struct_and_its_widening():
    """HotGenOpts is wis_gen_opts_t in full: GenOpts' fields where they lay, the two appended fields behind them.  Every entry point's options
    argument hands the engine the full struct: a GenOpts (as such, or through byref) is widened with zeros, a HotGenOpts goes as it is."""
    import ctypes as C
    from wis_hip import _lib
    G, H = _lib.GenOpts, _lib.HotGenOpts
    assert C.sizeof(H) == C.sizeof(G) + 8 and H.hotwords.offset == C.sizeof(G) and H.hotword_boost.offset == C.sizeof(G) + 4
    for name, _ in G._fields_:
        assert getattr(H, name).offset == getattr(G, name).offset, name
    g = G(0, 5, 7, 1.0, 1.0, 1, 1, 0, 0)
    g.phrases, g.phrase_mass = 1, 1
    for arg in (g, C.byref(g)):
        full = _lib._OptsArg.from_param(arg)._obj
        assert type(full) is H and full is not g and bytes(full)[:C.sizeof(G)] == bytes(g) and full.hotwords == 0 and full.hotword_boost == 0.0
    h = H(0, 5, 7, 1.0, 1.0, 1, 1, 0, 0)
    h.hotwords, h.hotword_boost = 1, 2.5
    assert _lib._OptsArg.from_param(C.byref(h))._obj is h and _lib._OptsArg.from_param(h)._obj is h
    with pytest.raises(TypeError):
        _lib._OptsArg.from_param(C.byref(C.c_int(3)))
    for name, _res, args in _lib.SYMBOLS:      # no prototype takes the short struct by pointer
        assert C.POINTER(G) not in args, name
    assert sum(_lib._OptsArg in args for _n, _r, args in _lib.SYMBOLS) == 7


def test_the_shims_refusals(model):
    ok = [[400, 401]]
    for kw in (dict(phrases=ok), dict(beam_size=1, draft_tokens=[400, 401]),
               dict(beam_size=2, draft_trajectory=(np.asarray([[400, 401]], np.int32), np.zeros((1, 2), np.int32)))):
        with pytest.raises(ValueError) as e:
            _opts(model, hotwords=ok, hotword_boost=2.0, **kw)
        assert "hotwords" in str(e.value), (kw, str(e.value))
    for boost in (None, 0, 0.0, -1.0, float("inf"), float("nan"), "much", 1e-50, 1e39):      # (the last two are 0 and inf in float32)
        with pytest.raises(ValueError) as e:
            _opts(model, hotwords=ok, hotword_boost=boost)
        assert "hotword_boost" in str(e.value), (boost, str(e.value))
    with pytest.raises(ValueError):
        _opts(model, hotword_boost=2.0)                      # a boost without a list
    for bad in ([[400, EOT]], [[]], [[220]], [], "lamp", [[400, 1]], 5, [[int(t) for t in _pool()[:33]]]):
        with pytest.raises(ValueError):
            _opts(model, hotwords=bad, hotword_boost=2.0)


def test_boosted_records_separate_device_batches(model):
    """The micro-batcher keys on the record: whatever it coalesces, a device batch (one `run` call of the fake engine) never holds rows of two
    hotword sets, of two boosts, or of a boosted and a plain or constrained call - and rows under equal records may share one."""
    import threading
    from wis_hip import ctranslate2 as ct2
    from wis_hip.batching import MicroBatcher
    a, b = [[400, 401]], [[400, 402]]
    recs = [_opts(model, hotwords=a, hotword_boost=2.0), _opts(model, hotwords=list(a), hotword_boost=2.0), _opts(model, hotwords=b, hotword_boost=2.0),
            _opts(model, hotwords=a, hotword_boost=4.0), _opts(model), _opts(model, phrases=a)]
    groups = {}
    for i, r in enumerate(recs):
        groups.setdefault(r, []).append(i)
    assert sorted(groups.values()) == [[0, 1], [2], [3], [4], [5]]
    seen = []
    gate = threading.Event()

    def run(ctx, key, payloads):
        gate.wait(5)                             # the "GPU" is busy with the first batch until every request is queued
        seen.append((key, sorted(payloads)))
        return list(payloads)
    mb = MicroBatcher(["gpu0"], run, lambda key: 8)
    th = [threading.Thread(target=mb.submit, args=(r, [i])) for i, r in enumerate(recs * 2)]
    for t in th:
        t.start()
    deadline = time.monotonic() + 5
    while mb.load()[0] < len(th) - 4 and time.monotonic() < deadline:      # (most requests are queued behind the busy "GPU")
        time.sleep(0.001)
    gate.set()
    for t in th:
        t.join()
    mb.close()
    assert sum(len(p) for _, p in seen) == 12
    for key, payloads in seen:
        assert {recs[i % 6] for i in payloads} == {key}, (payloads,)      # one record per device batch
    assert any(type(k) is ct2.BoostedOptions and len(p) > 1 for k, p in seen), seen      # equal records did share one


class _Models:
    def __init__(self, settings=None):
        from wis_hip.settings import APISettings
        self.settings = settings or APISettings()

    def get(self, size):
        raise AssertionError("the model is not reached")


def test_do_whisper_option_resolution(tmp_path):
    from wis_hip import whisper
    from wis_hip.settings import APISettings
    s = APISettings()
    assert s.hotwords_file == "" and s.hotword_boost == 0.0
    R = whisper._hotword_opts
    assert R(s, None, None) == (None, 0.0) and R(s, [], None) == (None, 0.0) and R(s, [], 2.0) == (None, 0.0)      # off
    assert R(s, ["lamp"], 2.5) == (["lamp"], 2.5) and R(s, [[400, 401]], 1) == ([[400, 401]], 1.0)
    with pytest.raises(ValueError) as e:                    # an explicit list without any boost
        R(s, ["lamp"], None)
    assert "hotword_boost" in str(e.value)
    for boost in (0, -2.0, float("nan"), float("inf"), "much"):
        with pytest.raises(ValueError):
            R(s, ["lamp"], boost)
    for bad in ("lamp", 7):
        with pytest.raises(ValueError):
            R(s, bad, 2.0)
    f = tmp_path / "hot.txt"
    f.write_text("Wohnzimmer\n\n# a comment\n  Esszimmer lamp \n", encoding="utf-8")
    s.hotwords_file = str(f)
    assert R(s, None, None) == (None, 0.0)                  # the settings' list with a boost of 0: off, not an error
    assert R(s, None, 3.0) == (["Wohnzimmer", "Esszimmer lamp"], 3.0)      # the request's boost over the settings' list
    s.hotword_boost = 1.5
    assert R(s, None, None) == (["Wohnzimmer", "Esszimmer lamp"], 1.5) and R(s, ["x"], None) == (["x"], 1.5) and R(s, [], None) == (None, 0.0)
    # do_whisper refuses before it reads audio: phrases with hotwords, a list without a boost, a bad boost
    pcm = np.zeros(16000, np.float32)
    for kw, word in ((dict(phrases=["turn on"], hotwords=["lamp"], hotword_boost=2.0), "hotwords cannot be combined with phrases"),
                     (dict(hotwords=["lamp"]), "hotword_boost"), (dict(hotwords=["lamp"], hotword_boost=-1), "hotword_boost"),
                     (dict(hotwords="lamp", hotword_boost=2.0), "hotwords")):
        with pytest.raises(ValueError) as e:
            whisper.do_whisper(pcm, "tiny", models=_Models(), **kw)
        assert word in str(e.value), (kw, str(e.value))
    # strings need the vocabulary; ids do not
    tok = whisper._Tokenizer(None)
    special = whisper.model_special_tokens(object())
    with pytest.raises(ValueError) as e:
        whisper.hotword_ids(["lamp"], tok, special)
    assert "vocabulary" in str(e.value)
    assert whisper.hotword_ids([[400, 401], (500,)], tok, special) == [[400, 401], [500]]
    for bad in ("lamp", [], [[]], [[1.5]], 7):
        with pytest.raises(ValueError):
            whisper.hotword_ids(bad, tok, special)

    class Vocab:
        has_vocabulary = True

        def encode(self, text):
            assert text.startswith(" ") and text == " " + text.strip()
            return [400 + len(w) for w in text.split()]
    assert whisper.hotword_ids(["  Wohnzimmer lamp ", [9, 10]], Vocab(), special) == [[410, 404], [9, 10]]
    q = type("Q", (), dict(hotwords=None, hotword_boost=0.0))()
    assert whisper._request_hotwords(q, tok, special) == {}
    q.hotwords, q.hotword_boost = [[400]], 2.0
    assert whisper._request_hotwords(q, tok, special) == dict(hotwords=[[400]], hotword_boost=2.0)


def test_the_settings_list_does_not_reach_a_constrained_request(tmp_path):
    """hotwords_file + hotword_boost in the settings and a request that carries `phrases`: the client named no hotwords, so the request is the
    constrained one (its generate call carries no hotword keyword) - only a request that names BOTH is refused."""
    from wis_hip import whisper
    from wis_hip.settings import APISettings
    calls = []

    class Result:
        sequences_ids, scores, no_speech_prob = [[400]], [-0.5], 0.0

    class FakeWhisper:
        n_mels, arch = 80, dict(n_text_ctx=448)

        def generate(self, feats, prompts, **kw):
            calls.append((kw.get("phrases"), kw.get("hotwords")))
            return [Result() for _ in prompts]

    class Models:
        settings = APISettings()

        def get(self, size):
            return FakeWhisper()

        def tokenizer_for(self, size):
            return whisper._Tokenizer(None)
    f = tmp_path / "hot.txt"
    f.write_text("ids\n", encoding="utf-8")
    Models.settings.fuse_logmel, Models.settings.hotwords_file, Models.settings.hotword_boost = True, str(f), 2.0
    pcm = np.zeros(16000, np.float32)
    whisper.do_whisper(pcm, "tiny", models=Models(), force_language="en", phrases=[[400], [401, 402]])
    assert calls == [([[400], [401, 402]], None)], calls
    with pytest.raises(ValueError) as e:
        whisper.do_whisper(pcm, "tiny", models=Models(), force_language="en", phrases=[[400]], hotwords=[[500]], hotword_boost=2.0)
    assert "hotwords cannot be combined with phrases" in str(e.value)


def test_hotwords_reach_every_decode(monkeypatch):
    """The translate pass and the main pass both carry the option; language detection does not (it takes no such keyword)."""
    from wis_hip import whisper
    from wis_hip.settings import APISettings
    calls = []

    class Result:
        sequences_ids, scores, no_speech_prob = [[400]], [-0.5], 0.0

    class FakeWhisper:
        n_mels, arch = 80, dict(n_text_ctx=448)

        def generate(self, feats, prompts, **kw):
            calls.append((prompts[0][2], kw.get("hotwords"), kw.get("hotword_boost")))
            return [Result() for _ in prompts]

    class Models:
        settings = APISettings()

        def get(self, size):
            return FakeWhisper()

        def tokenizer_for(self, size):
            return whisper._Tokenizer(None)
    Models.settings.fuse_logmel = True
    whisper.do_whisper(np.zeros(16000, np.float32), "tiny", models=Models(), force_language="en", translate=True, hotwords=[[400, 401]], hotword_boost=2.0)
    special = whisper.model_special_tokens(FakeWhisper())
    assert calls == [(special.transcribe, [[400, 401]], 2.0), (special.translate, [[400, 401]], 2.0)], calls
    del calls[:]
    whisper.do_whisper(np.zeros(16000, np.float32), "tiny", models=Models(), force_language="en")
    assert calls == [(special.transcribe, None, None)], calls


class _FakeModels:
    """Stands in for WhisperModels: request handling without a GPU; reaching the model is an error here."""

    def __init__(self, settings=None):
        from wis_hip.settings import APISettings
        from wis_hip.whisper import _Tokenizer
        self.settings = settings or APISettings()
        self.tokenizer = _Tokenizer(None)

    def tokenizer_for(self, size):
        return self.tokenizer

    def get(self, size):
        if size not in ("tiny", "base", "small", "medium", "large"):
            raise ValueError(f"unknown model {size!r}")
        return object()


def test_hotwords_file(tmp_path):
    from wis_hip import whisper
    from wis_hip.server import create_app
    from wis_hip.settings import APISettings
    assert whisper.load_hotwords_file("") == []
    f = tmp_path / "hot.txt"
    f.write_text("Wohnzimmer\n\n# names\n  Flurlicht  \n", encoding="utf-8")
    assert whisper.load_hotwords_file(str(f)) == ["Wohnzimmer", "Flurlicht"]
    s = APISettings()
    s.hotwords_file = str(tmp_path / "missing.txt")
    with pytest.raises(OSError):                    # an unreadable file fails the start
        create_app(models=_FakeModels(s))
    (tmp_path / "empty.txt").write_text("# nothing\n")
    s.hotwords_file = str(tmp_path / "empty.txt")
    with pytest.raises(ValueError):                 # and so does an empty one
        create_app(models=_FakeModels(s))
    s.hotwords_file = str(f)
    create_app(models=_FakeModels(s))               # a list with a boost of 0: off, no error
    s.hotword_boost = 2.0
    create_app(models=_FakeModels(s))
    s.hotword_boost = -1.0
    with pytest.raises(ValueError):
        create_app(models=_FakeModels(s))
    # settings that constrain every request leave the hotword list nothing to do: the start fails (a boost of 0 beside them is "off" and starts)
    p = tmp_path / "phrases.txt"
    p.write_text("turn on\n", encoding="utf-8")
    s.phrases_file, s.hotword_boost = str(p), 2.0
    with pytest.raises(ValueError) as e:
        create_app(models=_FakeModels(s))
    assert "phrases_file" in str(e.value) and "hotwords_file" in str(e.value)
    s.hotword_boost = 0.0
    create_app(models=_FakeModels(s))


def test_query_parameters_and_their_400s(golden_dir):
    import httpx
    from wis_hip.server import create_app
    app = create_app(models=_FakeModels())
    b = "xYzBoundary123"
    with open(os.path.join(golden_dir, "clips", "3sec.flac"), "rb") as f:
        clip = f.read()
    body = (f"--{b}\r\nContent-Disposition: form-data; name=\"audio_file\"; filename=\"a.flac\"\r\nContent-Type: application/octet-stream\r\n\r\n").encode() + clip + f"\r\n--{b}--\r\n".encode()
    hdr = {"content-type": f"multipart/form-data; boundary={b}"}

    async def go():
        async with httpx.AsyncClient(transport=httpx.ASGITransport(app=app), base_url="http://wis") as c:
            for q, word in (("hotword_boost=much&hotwords=ids:400", "hotword_boost"), ("hotword_boost=0&hotwords=ids:400", "hotword_boost"),
                            ("hotword_boost=-2&hotwords=ids:400", "hotword_boost"), ("hotword_boost=nan&hotwords=ids:400", "hotword_boost"),
                            ("hotword_boost=inf&hotwords=ids:400", "hotword_boost"),
                            ("hotwords=ids:1,x&hotword_boost=2", "hotwords"), ("hotwords=ids:&hotword_boost=2", "hotwords"), ("hotwords=ids:4,-2&hotword_boost=2", "hotwords"),
                            ("hotwords=lamp||desk&hotword_boost=2", "hotwords"),
                            ("hotwords=ids:400,401", "hotword_boost"),                                        # an explicit list without any boost
                            ("hotwords=ids:400,401&hotword_boost=2.5&phrases=ids:400", "hotwords cannot be combined with phrases"),
                            ("hotwords=Wohnzimmer|ids:400,401&hotword_boost=2.5", "vocabulary"),             # text without the checkpoint's tokenizer
                            ("hotwords=ids:400,50257&hotword_boost=2.5", "text tokens")):                    # <|endoftext|> inside an entry
                r = await c.post(f"/api/asr?model=tiny&{q}", content=body, headers=hdr)
                assert r.status_code == 400 and word in r.json()["error"], (q, r.status_code, r.text)
            r = await c.post("/api/willow?model=tiny&hotwords=ids:1,x&hotword_boost=2", content=clip, headers={"x-audio-codec": "flac"})
            assert r.status_code == 400 and "hotwords" in r.json()["error"]
            r = await c.post("/api/asr?model=tiny&hotwords=&hotword_boost=", content=body.replace(clip, b"this is not audio"), headers=hdr)      # empty values: the settings'
            assert r.status_code == 400 and r.json() == {"error": "Invalid audio"}

    asyncio.run(go())
