"""Phrase-constrained decoding, host side (no GPU): the trie builder against the dict-of-prefixes form (tests/phrase_ref.py, written without
it), the shim's refusals, the micro-batcher's rule - two calls share a device batch exactly when their options AND their phrase sets are
equal, and a plain call builds the record it has always built -, do_whisper's refusals, the setting and the query parameters on the server's
fake engine."""
import asyncio
import os

import numpy as np
import pytest

from phrase_ref import prefix_dict, trie_to_prefix_dict

EOT = 50257
PROMPT = [50258, 50259, 50359, 50363]


def _pool():
    from wis_hip import weights as W
    bad = set(W.SUPPRESS_IDS) | set(W.SUPPRESS_IDS_BEGIN)
    return [t for t in range(EOT) if t not in bad]


def _walk_is_sound(trie):
    """the layout rules of include/wis_hip.h, checked on the table itself: breadth-first blocks, ascending children, leaves end phrases"""
    cursor = 1
    for i, (tok, first, n, ends) in enumerate(trie.tolist()):
        assert i < cursor and ends in (0, 1)
        if n == 0:
            assert first == 0 and ends == 1
            continue
        assert first == cursor
        kids = trie[first:first + n, 0].tolist()
        assert kids == sorted(set(kids))
        cursor += n
    assert cursor == len(trie) and trie[0].tolist()[0] == -1 and trie[0].tolist()[3] == 0


def test_builder_equals_the_dict_form():
    from wis_hip import weights as W
    pool = _pool()
    rng = np.random.default_rng(1)
    sets = {
        "shared prefixes": [[400, 401, 402], [400, 401, 403], [400, 500], [600, 401, 402]],
        "a phrase that is a prefix of another": [[400], [400, 401], [400, 401, 402], [700, 701]],
        "duplicates": [[400, 401], [400, 401], [400], [400], [500, 501, 502], [500, 501, 502]],
        "one phrase": [[30]],
        "4096 children": [[int(t)] for t in pool[:4096]] + [[int(pool[5]), int(t)] for t in pool[100:4196]],
        "depth 32": [rng.choice(pool, size=32).tolist(), rng.choice(pool, size=31).tolist()],
        "random": [rng.choice(pool[:40], size=int(rng.integers(1, 9))).tolist() for _ in range(400)],
    }
    for what, phrases in sets.items():
        trie = W.build_phrase_trie(phrases)
        assert trie.dtype == np.int32 and trie.ndim == 2 and trie.shape[1] == 4 and trie.flags["C_CONTIGUOUS"], what
        _walk_is_sound(trie)
        assert trie_to_prefix_dict(trie) == prefix_dict(phrases), what
    dup = W.build_phrase_trie(sets["duplicates"])
    assert np.array_equal(dup, W.build_phrase_trie([[400, 401], [400], [500, 501, 502]]))      # duplicates merge
    interior = prefix_dict(sets["a phrase that is a prefix of another"])
    assert interior[(400,)] == ([401], True) and interior[(400, 401)] == ([402], True) and interior[(700,)] == ([701], False)


def test_builder_is_deterministic():
    from wis_hip import weights as W
    rng = np.random.default_rng(2)
    pool = _pool()
    phrases = [rng.choice(pool[:60], size=int(rng.integers(1, 7))).tolist() for _ in range(300)]
    a = W.build_phrase_trie(phrases)
    for _ in range(3):
        b = W.build_phrase_trie([phrases[i] for i in rng.permutation(len(phrases))])
        assert a.tobytes() == b.tobytes()
    assert a.tobytes() == W.build_phrase_trie([tuple(np.int64(t) for t in ph) for ph in phrases]).tobytes()      # (any integer type)


def test_builder_refusals_name_the_phrase():
    from wis_hip import weights as W
    pool = _pool()
    ok = [400, 401]
    cases = {
        "empty": [], "33 tokens": [int(t) for t in pool[:33]], "<|endoftext|>": [400, EOT], "a special token": [400, 50259], "a timestamp": [400, 50364],
        "negative": [400, -1], "beyond the vocabulary": [400, 60000], "suppressed": [400, W.SUPPRESS_IDS[3]], "suppressed first": [W.SUPPRESS_IDS[3], 400],
        "blank first": [220, 400], "a float": [400, 1.5], "a string": "turn on",
    }
    for what, ph in cases.items():
        with pytest.raises(ValueError) as e:
            W.build_phrase_trie([ok, ph])
        assert repr(ph if isinstance(ph, str) else list(ph))[:12] in str(e.value) or repr(ph) in str(e.value), (what, str(e.value))
    assert len(W.build_phrase_trie([[400, 220]])) == 3                       # suppress_ids_begin binds the first token only
    assert len(W.build_phrase_trie([[int(t) for t in pool[:32]]])) == 33     # 32 tokens fit
    with pytest.raises(ValueError):
        W.build_phrase_trie([])
    with pytest.raises(ValueError) as e:                                     # 4097 children of one node
        W.build_phrase_trie([[int(t)] for t in pool[:4097]])
    assert "4096" in str(e.value)
    assert len(W.build_phrase_trie([[int(t)] for t in pool[:4096]])) == 4097
    with pytest.raises(ValueError) as e:                                     # more than 65535 records
        W.build_phrase_trie([[int(a), int(b)] for a in pool[:20] for b in pool[:3400]])
    assert "65535" in str(e.value)
    # the model's own lists and <|endoftext|> decide (large-v3: another vocabulary)
    assert len(W.build_phrase_trie([[7, 8]], suppress_ids=[], suppress_begin=[])) == 3
    with pytest.raises(ValueError):
        W.build_phrase_trie([[400, 300]], eot=300)


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


def test_the_batching_rule(model):
    from wis_hip import ctranslate2 as ct2
    a, b = [[400, 401], [500]], [[400, 401], [501]]
    plain = _opts(model)
    assert type(plain) is ct2.DecodeOptions and plain == ct2.DecodeOptions(4, 5, 224, input_kind=plain.input_kind)      # the record a plain call has always built
    assert type(_opts(model, phrases=None)) is ct2.DecodeOptions
    ca, ca2, cb = _opts(model, phrases=a), _opts(model, phrases=[[500], [400, 401], [500]]), _opts(model, phrases=b)
    assert type(ca) is ct2.ConstrainedOptions and ca._fields == plain._fields
    assert ca == ca2 and hash(ca) == hash(ca2) and not ca != ca2                    # the same SET: one class, whatever the list's order
    assert ca != cb and cb != ca and len({ca, ca2, cb}) == 2                        # another set: another class
    assert ca != plain and plain != ca and not ca == plain and not plain == ca      # never a plain call's class, from either side
    assert len({plain, ca}) == 2
    assert ca.max_new_tokens == 3 and tuple(ca) == tuple(plain._replace(max_new_tokens=3))      # longest phrase + 1; everything else as the plain record
    assert _opts(model, phrases=a, beam_size=2) != ca and _opts(model, phrases=a, repetition_penalty=1.2) != ca      # the options still count
    r = ca._replace(prompt_len=7)
    assert type(r) is ct2.ConstrainedOptions and r.prompt_len == 7 and r.phrase_digest == ca.phrase_digest and r.phrase_trie is ca.phrase_trie and r != ca
    assert np.array_equal(ca.phrase_trie, ca2.phrase_trie) and ca.phrase_trie.dtype == np.int32
    o = ct2._gen_opts(ca)
    assert o.phrases == 1 and o.max_new_tokens == 3 and ct2._gen_opts(plain).phrases == 0
    nb = _opts(model, phrases=a, num_hypotheses=3)
    assert nb.num_hypotheses == 3 and nb != ca
    assert ct2._capacity(8, ca) == ct2._capacity(8, plain)


def test_the_shims_refusals(model):
    ok = [[400, 401]]
    for kw in (dict(prompts=([50258, 50259, 50359],)),                                    # a timestamp prompt
               dict(beam_size=1, sampling_topk=0), dict(fixed_new_tokens=4), dict(beam_size=1, draft_tokens=[400, 401]),
               dict(beam_size=2, draft_trajectory=(np.asarray([[400, 401]], np.int32), np.zeros((1, 2), np.int32))),
               dict(num_hypotheses=6), dict(max_length=6)):
        with pytest.raises(ValueError):
            _opts(model, phrases=ok, **kw)
    for bad in ([[400, EOT]], [[]], [[220]], [], "turn on", [[400, 1]], 5, [[int(t) for t in _pool()[:33]]]):
        with pytest.raises(ValueError):
            _opts(model, phrases=bad)
    # what combines: a long prompt, the repetition options, n-best, no_speech_prob
    long_prompt = [50361] + list(range(400, 430)) + PROMPT
    c = _opts(model, prompts=(long_prompt,), phrases=ok, repetition_penalty=1.3, no_repeat_ngram_size=2, num_hypotheses=2, return_no_speech_prob=True)
    assert c.prompt_len == len(long_prompt) and c.max_new_tokens == 3 and c.repetition_penalty == 1.3 and c.no_speech_prob


def test_do_whisper_refuses_before_it_reads_audio():
    from wis_hip import whisper
    from wis_hip.settings import APISettings

    class Models:
        settings = APISettings()

        def get(self, size):
            raise AssertionError("the model is not reached")
    for kw in (dict(prefix="turn"), dict(timestamps=True), dict(word_timestamps=True), dict(temperatures=[0.0, 0.4]), dict(long_form="seek"),
               dict(fixed_new_tokens=4), dict(phrase_nbest=0), dict(phrase_nbest="two"), dict(phrase_nbest=1.5)):
        with pytest.raises(ValueError) as e:
            whisper.do_whisper(np.zeros(16000, np.float32), "tiny", models=Models(), phrases=["turn on", "turn off"], **kw)
        assert "phrase" in str(e.value), (kw, str(e.value))
    # strings need the vocabulary; ids do not
    tok = whisper._Tokenizer(None)
    special = whisper.model_special_tokens(object())
    with pytest.raises(ValueError):
        whisper.phrase_ids(["turn on"], tok, special)
    ids, names = whisper.phrase_ids([[400, 401], (500,)], tok, special)
    assert ids == [[400, 401], [500]] and names == {}
    for bad in ("turn on", [], [[]], [[400, EOT]], [[1.5]], 7):
        with pytest.raises(ValueError):
            whisper.phrase_ids(bad, tok, special)

    class Vocab:      # a tokenizer with a vocabulary: " " + text.strip(), as a prompt is encoded
        has_vocabulary = True

        def encode(self, text):
            assert text.startswith(" ") and text == " " + text.strip()
            return [400 + len(w) for w in text.split()]
    ids, names = whisper.phrase_ids(["  turn on ", "off", [9, 10]], Vocab(), special)
    assert ids == [[404, 402], [403], [9, 10]] and names == {(404, 402): "turn on", (403,): "off"}


def test_phrases_file(tmp_path):
    from wis_hip import whisper
    from wis_hip.server import create_app
    from wis_hip.settings import APISettings
    assert APISettings().phrases_file == "" and whisper.load_phrases_file("") == []
    f = tmp_path / "phrases.txt"
    f.write_text("turn on the light\n\n# a comment\n  turn off the light  \nset the heating to twenty\n", encoding="utf-8")
    assert whisper.load_phrases_file(str(f)) == ["turn on the light", "turn off the light", "set the heating to twenty"]
    s = APISettings()
    s.phrases_file = str(tmp_path / "missing.txt")
    with pytest.raises(OSError):                    # an unreadable file fails the start
        create_app(models=_FakeModels(s))
    (tmp_path / "empty.txt").write_text("# nothing\n")
    s.phrases_file = str(tmp_path / "empty.txt")
    with pytest.raises(ValueError):
        create_app(models=_FakeModels(s))
    s.phrases_file = str(f)
    create_app(models=_FakeModels(s))


class _FakeModels:
    """Stands in for WhisperModels (tests/test_server_cpu.py's): request handling without a GPU; reaching the model is an error here."""

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
            for q, word in (("phrase_nbest=two", "phrase_nbest"), ("phrase_nbest=0", "phrase_nbest"), ("phrase_nbest=99", "phrase_nbest"),
                            ("phrases=ids:1,x", "phrases"), ("phrases=ids:", "phrases"), ("phrases=ids:4,-2", "phrases"), ("phrases=turn on||turn off", "phrases"),
                            ("phrases=turn on|turn off&timestamps=true", "phrases cannot be combined"), ("phrases=ids:400,401&word_timestamps=true", "phrases cannot be combined"),
                            ("phrases=ids:400,401&prefix=turn", "phrases cannot be combined"), ("phrases=ids:400,401&temperatures=0,0.4", "phrases cannot be combined"),
                            ("phrases=ids:400,401&long_form=seek", "phrases cannot be combined"),
                            ("phrases=ids:400,401&phrase_nbest=7&beam_size=5", "phrase_nbest"),           # more phrases than the beam holds
                            ("phrases=turn on|turn off", "vocabulary"),                                      # text without the checkpoint's tokenizer
                            ("phrases=ids:400,50257", "text tokens")):                                       # <|endoftext|> inside a phrase
                r = await c.post(f"/api/asr?model=tiny&{q}", content=body, headers=hdr)
                assert r.status_code == 400 and word in r.json()["error"], (q, r.status_code, r.text)
            r = await c.post("/api/willow?model=tiny&phrases=ids:1,x", content=clip, headers={"x-audio-codec": "flac"})
            assert r.status_code == 400 and "phrases" in r.json()["error"]
            r = await c.post("/api/asr?model=tiny&phrases=&phrase_nbest=", content=body.replace(clip, b"this is not audio"), headers=hdr)      # empty values: the settings', as ever
            assert r.status_code == 400 and r.json() == {"error": "Invalid audio"}

    asyncio.run(go())
