"""Prompts of different lengths in one device batch, without a GPU: the micro-batcher's pooled key (`DecodeOptions.prompt_len == -1`, the setting
`batch_ragged_prompts`), its capacity, and what `_generate_chunk` does under it - the rows to the engine longest prompt first, the results back in the
callers' order - with the engine replaced by tools/fake_engine_app.py (the keys) or by a recording stand-in for the library (the engine call)."""
import os

import numpy as np
import pytest

SOT, PREV, NO_TS = 50258, 50361, 50363
START = [SOT, 50259, 50359, NO_TS]


@pytest.fixture()
def fake_app(monkeypatch):
    """tests/test_prompt_cpu.py's fixture, copied: the re-hosted server over an engine that sleeps"""
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


def _keys_of(app, setting):
    """the batcher keys of requests with 4, 41, 42, 41, 100 and 228 prompt tokens under batch_ragged_prompts = setting"""
    from wis_hip import _lib, ctranslate2 as ct2
    models = app.state.wis["models"]
    models.settings.batch_ragged_prompts = setting
    try:
        model = models.get("large")      # (the model reads the setting where it builds its keys)
        keys = []
        submit = model._batcher.submit
        model._batcher.submit = lambda key, rows, **kw: (keys.append(key), submit(key, rows, **kw))[1]
        try:
            pcm = ct2.StorageView.from_array(np.zeros((1, _lib.N_SAMPLES), np.float32))
            for prompt in (START, [PREV] + [7] * 36 + START, [PREV] + [7] * 37 + START, [PREV] + [9] * 36 + START, [PREV] + [7] * 95 + START,
                           [PREV] + [7] * 223 + START):
                assert model.generate(pcm, [prompt], beam_size=1, input_kind=_lib.WIS_IN_PCM_HOST)[0] is not None
        finally:
            model._batcher.submit = submit
        return keys
    finally:
        models.settings.batch_ragged_prompts = False
        models.get("large")


def test_the_setting_is_off_by_default_and_read_from_the_environment(monkeypatch):
    from wis_hip.settings import APISettings
    assert APISettings().batch_ragged_prompts is False
    monkeypatch.setenv("BATCH_RAGGED_PROMPTS", "true")
    assert APISettings().batch_ragged_prompts is True


def test_keys_with_the_setting_off_are_todays(fake_app):
    from wis_hip import _lib, ctranslate2 as ct2
    app, calls, _ = fake_app
    keys = _keys_of(app, False)
    todays = ct2.DecodeOptions(prompt_len=4, beam_size=1, max_new_tokens=224, length_penalty=1.0, patience=1.0, suppress_blank=True, suppress_default=True,
                               fixed_new_tokens=0, input_kind=_lib.WIS_IN_PCM_HOST, draft=None, return_trajectory=False, timestamps=False,
                               max_initial_timestamp_index=50, no_speech_prob=False, repetition_penalty=1.0, no_repeat_ngram_size=0, sampling_topk=0,
                               sampling_temperature=1.0, num_hypotheses=1)
    assert keys == [todays, todays._replace(prompt_len=41), todays._replace(prompt_len=42), todays._replace(prompt_len=41), todays._replace(prompt_len=100),
                    todays._replace(prompt_len=228, max_new_tokens=220)]
    assert [c[1] for c in calls] == [4, 41, 42, 41, 100, 228]


def test_long_prompts_pool_under_one_key_with_the_setting_on(fake_app):
    from wis_hip import ctranslate2 as ct2
    app, calls, _ = fake_app
    off, on = _keys_of(app, False), _keys_of(app, True)
    assert ct2.RAGGED_PROMPT == -1
    assert on[0] == off[0] and on[0].prompt_len == 4                                   # up to 16 tokens: the exact key, as ever
    assert on[1] == on[2] == on[3] == on[4] and on[1].prompt_len == -1                 # 41, 42, 41 and 100 tokens meet
    assert on[1] == off[1]._replace(prompt_len=-1)                                     # nothing but the length word differs
    assert on[5].prompt_len == -1 and on[5].max_new_tokens == 220 and on[5] != on[4]   # P = 228: another max_new_tokens, apart - max plen + max_new stays inside the context
    assert [c[1] for c in calls[6:]] == [4, -1, -1, -1, -1, -1] and [len(c[0][0]) for c in calls[6:]] == [4, 41, 42, 41, 100, 228]


def test_the_keyword_alone_pools_only_prompts_that_differ(fake_app):
    from wis_hip import _lib, ctranslate2 as ct2
    app, calls, model = fake_app
    keys = []
    submit = model._batcher.submit
    model._batcher.submit = lambda key, rows, **kw: (keys.append(key), submit(key, rows, **kw))[1]
    pcm = ct2.StorageView.from_array(np.zeros((2, _lib.N_SAMPLES), np.float32))
    g = lambda prompts, **kw: model.generate(pcm, prompts, beam_size=1, input_kind=_lib.WIS_IN_PCM_HOST, **kw)
    with pytest.raises(ValueError, match="all prompts must have the same length"):
        g([START, [PREV, 7] + START])
    assert not keys
    g([START, [PREV, 7] + START], ragged_prompts=True)
    assert keys[-1].prompt_len == -1 and keys[-1].max_new_tokens == 224
    g([[PREV] + [7] * 223 + START, START], ragged_prompts=True)
    assert keys[-1].prompt_len == -1 and keys[-1].max_new_tokens == 220                # from the longest prompt of the call
    g([START, START], ragged_prompts=True)
    assert keys[-1].prompt_len == 4                                                    # equal prompts: the default call
    n0 = len(keys)
    for kw in (dict(draft_tokens=[5, 6]), dict(return_trajectory=True)):
        with pytest.raises(ValueError, match="ragged_prompts"):
            g([START, [PREV, 7] + START], ragged_prompts=True, **kw)
    with pytest.raises(ValueError, match="prompt length 229"):
        g([START, [PREV] + [7] * 224 + START], ragged_prompts=True)
    with pytest.raises(ValueError, match="prompt length 0"):
        g([START, []], ragged_prompts=True)
    with pytest.raises(ValueError, match="timestamps"):
        g([START, [PREV, 7] + START[:3]], ragged_prompts=True)
    assert len(keys) == n0


def test_capacity_of_the_pooled_key_is_a_long_prompts():
    from wis_hip.ctranslate2 import DecodeOptions, _capacity
    for max_batch in (8, 16, 32, 96):
        for beam, n in ((1, 1), (5, 1), (8, 1), (1, 5)):
            kw = dict(sampling_topk=-1, sampling_temperature=0.7, num_hypotheses=n) if n > 1 else {}
            assert _capacity(max_batch, DecodeOptions(-1, beam, 224, **kw)) == _capacity(max_batch, DecodeOptions(17, beam, 224, **kw))
    assert _capacity(32, DecodeOptions(-1, 5, 224)) == 19 and _capacity(8, DecodeOptions(-1, 5, 224)) == 8


def test_decode_options_fields_are_unchanged():
    from wis_hip import ctranslate2 as ct2
    assert ct2.DecodeOptions._fields == ("prompt_len", "beam_size", "max_new_tokens", "length_penalty", "patience", "suppress_blank", "suppress_default",
                                         "fixed_new_tokens", "input_kind", "draft", "return_trajectory", "timestamps", "max_initial_timestamp_index",
                                         "no_speech_prob", "repetition_penalty", "no_repeat_ngram_size", "sampling_topk", "sampling_temperature",
                                         "num_hypotheses")


class _RaggedLib:
    """Stand-in for the loaded library: wis_generate_ragged records what it was given and answers, per utterance, one token that names it (its prompt
    length, the first value of its features) - so a result can be traced back to the row it belongs to."""

    def __init__(self):
        self.calls = []

    def wis_generate_ragged(self, h, src, B, prompts, plen, opts, seeds, ids, lens, scores):
        import ctypes as C
        B = int(B)
        pl = [int(plen[b]) for b in range(B)]
        flat = [int(prompts[i]) for i in range(sum(pl))]
        feats = np.ctypeslib.as_array(C.cast(src, C.POINTER(C.c_float)), shape=(B, 4))
        max_new = opts._obj.max_new_tokens
        self.calls.append(dict(B=B, plen=pl, prompts=flat, seeds=[int(seeds[b]) for b in range(B)], first=[float(feats[b, 0]) for b in range(B)], max_new=max_new))
        for b in range(B):
            ids[b * max_new] = 1000 * pl[b] + int(feats[b, 0])
            lens[b] = 1
            scores[b] = -float(pl[b])
        return 0

    def wis_generate(self, h, src, B, prompts, P, opts, ids, lens, scores):
        import ctypes as C
        B, P = int(B), int(P)
        feats = np.ctypeslib.as_array(C.cast(src, C.POINTER(C.c_float)), shape=(B, 4))
        max_new = opts._obj.max_new_tokens
        self.calls.append(dict(entry="wis_generate", B=B, P=P, first=[float(feats[b, 0]) for b in range(B)]))
        for b in range(B):
            ids[b * max_new] = 1000 * P + int(feats[b, 0])
            lens[b] = 1
        return 0


def test_generate_chunk_hands_the_engine_the_longest_prompt_first(monkeypatch):
    from wis_hip import _lib, ctranslate2 as ct2
    lib = _RaggedLib()
    monkeypatch.setattr(_lib, "load", lambda: lib)

    class Replica:
        handle = None
    lengths = [5, 40, 17, 40, 228, 1]
    prompts = [[100 + i] * n for i, n in enumerate(lengths)]
    mel = np.zeros((6, 4), np.float32)
    mel[:, 0] = np.arange(6)                                      # utterance i's features start with i
    opts = ct2.DecodeOptions(ct2.RAGGED_PROMPT, 1, 220)
    out = ct2._generate_chunk(Replica(), mel, prompts, opts, seeds=[10, 11, 12, 13, 14, 15])
    (call,) = lib.calls
    assert call["plen"] == [228, 40, 40, 17, 5, 1] and call["max_new"] == 220
    assert call["first"] == [4.0, 1.0, 3.0, 2.0, 0.0, 5.0]         # a stable sort: the two 40-token rows keep their order; the features moved with the prompts
    assert call["seeds"] == [14, 11, 13, 12, 10, 15]               # ... and the seeds
    want = []
    for i in (4, 1, 3, 2, 0, 5):
        want += prompts[i]
    assert call["prompts"] == want                                  # back to back, in the engine's order
    # the results come back in the callers' order
    assert [r.sequences_ids for r in out] == [[[1000 * n + i]] for i, n in enumerate(lengths)]
    assert [r.scores for r in out] == [[-float(n)] for n in lengths]
    # no draft and no trajectory under the pooled key
    with pytest.raises(ValueError, match="different lengths"):
        ct2._generate_chunk(Replica(), mel, prompts, opts._replace(return_trajectory=True))
    assert len(lib.calls) == 1


def test_a_pooled_batch_of_one_short_length_fits_the_merged_prefill(monkeypatch):
    """Equal lengths are the default call to the engine: up to 16 tokens that is the merged prefill of B * P <= 96 rows, and the pooled key's capacity
    does not divide by P - eight utterances of 16 tokens go in two such calls (6 + 2), the results in the callers' order."""
    from wis_hip import _lib, ctranslate2 as ct2
    lib = _RaggedLib()
    monkeypatch.setattr(_lib, "load", lambda: lib)

    class Replica:
        handle = None
    mel = np.zeros((8, 4), np.float32)
    mel[:, 0] = np.arange(8)
    out = ct2._generate_chunk(Replica(), mel, [[7] * 16] * 8, ct2.DecodeOptions(ct2.RAGGED_PROMPT, 5, 224))
    assert [(c["entry"], c["B"], c["P"], c["first"]) for c in lib.calls] == [("wis_generate", 6, 16, [0.0, 1.0, 2.0, 3.0, 4.0, 5.0]), ("wis_generate", 2, 16, [6.0, 7.0])]
    assert [r.sequences_ids for r in out] == [[[16000 + i]] for i in range(8)]
    del lib.calls[:]
    ct2._generate_chunk(Replica(), mel[:6], [[7] * 16] * 6, ct2.DecodeOptions(ct2.RAGGED_PROMPT, 5, 224))      # 96 rows: one call, through the ragged entry
    assert len(lib.calls) == 1 and lib.calls[0]["plen"] == [16] * 6
