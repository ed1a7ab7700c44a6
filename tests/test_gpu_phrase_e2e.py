"""-m gpu: phrase-constrained decoding end to end - wis_generate / wis_generate_n / wis_generate_ragged inside captured step graphs, through
`ctranslate2.Whisper.generate(..., phrases=...)` and `do_whisper` - on the tiny model (seeded weights) and the 3 s golden clip.

Scores are checked against the engine's OWN teacher-forced logits (`wis_debug_logits`) scored in float64 by tests/phrase_ref.py's brute force
under the distribution renormalised over what the list allows at each step.  Tolerance: 0.1 = twice the 5e-2 max-abs bound tests/test_gpu_e2e.py
holds teacher-forced logits of this model size to (that file's bound, not re-measured here).  A ranking is asserted only between phrases whose
brute-force scores differ by more than twice that tolerance; the set holds such pairs (asserted)."""
import ctypes as C
import os

import numpy as np
import pytest

from phrase_ref import brute_force

pytestmark = pytest.mark.gpu
EOT = 50257
PROMPT = [50258, 50259, 50359, 50363]
TOL = 2 * 5e-2
# twelve phrases of 1 .. 6 tokens: shared prefixes, an interior phrase end ([2425]), two lengths of one stem
PHRASES = [[2425], [2425, 322], [2425, 322, 264, 1442], [2425, 766, 264, 1442], [3488, 264, 4222, 281, 945], [3488, 264, 4222, 281, 3217, 12],
           [1590], [8962, 493], [8962, 760, 264, 5523], [4813, 264, 2853], [4813, 264, 3133, 12309], [7405, 11, 437, 565, 307, 309]]
OTHER = [[11226, 264, 6892], [11226, 264, 1318, 293, 1590], [16225]]


@pytest.fixture(scope="module")
def mel(golden_dir):
    from wis_hip import audio
    pcm, _ = audio.load_audio(os.path.join(golden_dir, "clips", "3sec.flac"))
    return np.ascontiguousarray(audio.log_mel_spectrogram(audio.pad_or_trim(pcm)).numpy()[None])


@pytest.fixture(scope="module")
def model():
    from wis_hip import ctranslate2 as ct2, weights as W
    m = ct2.Whisper("unused", weights=W.synthetic_weights("tiny", seed=1234, std=0.02, emb_std=0.06, ln_jitter=0.1), arch=W.arch("tiny"), max_batch=4, max_beam=5)
    yield m
    m.close()


def _gen(model, mel, beam, phrases, prompt=PROMPT, **kw):
    from wis_hip import ctranslate2 as ct2
    return model.generate(ct2.StorageView.from_array(mel), [prompt] * mel.shape[0], beam_size=beam, phrases=phrases, return_scores=True, **kw)


def _graphs(model):
    from wis_hip import _lib
    n = C.c_int(0)
    _lib.check(_lib.load().wis_debug_graph_count(model._replicas[0].handle, C.byref(n)))
    return n.value


@pytest.fixture(scope="module")
def brute(model, mel):
    """the engine's teacher-forced logits behind PROMPT + every prefix of PHRASES (one wis_debug_logits call per phrase), scored in float64"""
    from wis_hip import _lib
    lib, P = _lib.load(), len(PROMPT)
    rows = {}
    for ph in PHRASES:
        dec_in = np.ascontiguousarray(np.asarray([PROMPT + ph], np.int32))
        T = dec_in.shape[1]
        out = np.zeros((1, T, 51865), np.float32)
        _lib.check(lib.wis_debug_logits(model._replicas[0].handle, _lib.ptr(mel), _lib.WIS_IN_MEL_HOST, 1, dec_in.ctypes.data_as(C.POINTER(C.c_int32)), T,
                                        out.ctypes.data_as(C.POINTER(C.c_float))))
        for i in range(len(ph) + 1):
            rows.setdefault(tuple(ph[:i]), out[0, P - 1 + i].copy())
    bf = brute_force(PHRASES, lambda h: rows[h])
    pairs = [(a, b) for i, a in enumerate(bf) for b in bf[i + 1:] if a[0] - b[0] > 2 * TOL]
    assert len(pairs) >= 1, [e[0] for e in bf]
    print(f"\n[phrases] brute force over the engine's teacher-forced logits: scores {[round(e[0], 3) for e in bf]}; {len(pairs)} of {len(bf) * (len(bf) - 1) // 2} pairs apart by more than {2 * TOL}")
    return bf


def _assert_ranked(ids, scores, brute, ctx):
    score_of = {e[2]: e[0] for e in brute}
    assert all(tuple(x) in score_of for x in ids) and len({tuple(x) for x in ids}) == len(ids), (ctx, ids)
    for x, s in zip(ids, scores):
        assert abs(s - score_of[tuple(x)]) <= TOL, (ctx, x, s, score_of[tuple(x)])
    assert list(scores) == sorted(scores, reverse=True), (ctx, scores)                       # best first, by the engine's own scores
    for i, a in enumerate(ids):                                                              # ... and by the brute force's where it is decisive
        for b in ids[i + 1:]:
            assert not score_of[tuple(b)] - score_of[tuple(a)] > 2 * TOL, (ctx, a, b)


@pytest.mark.parametrize("beam", [1, 5])
def test_the_answer_is_a_phrase_of_the_list(model, mel, brute, beam):
    r = _gen(model, mel, beam, PHRASES)[0]
    assert len(r.sequences_ids) == 1 and r.sequences_ids[0] in PHRASES, r.sequences_ids
    # (the score is the brute force's for THAT phrase; a beam search ends once beam_size hypotheses have finished, so with more phrases than
    # beams it ranks the phrases it reached - short ones finish first - and need not reach the brute force's best)
    _assert_ranked(r.sequences_ids, r.scores, brute, beam)
    from wis_hip import ctranslate2 as ct2
    plain = model.generate(ct2.StorageView.from_array(mel), [PROMPT], beam_size=beam, fixed_new_tokens=6)[0]
    assert plain.sequences_ids[0] not in PHRASES          # (seeded weights: the unconstrained decode is no phrase - the constraint decided)


def test_n_best(model, mel, brute):
    r = _gen(model, mel, 5, PHRASES, num_hypotheses=3)[0]
    assert len(r.sequences_ids) == 3 and len(r.scores) == 3
    _assert_ranked(r.sequences_ids, r.scores, brute, "n-best")
    assert r.sequences_ids[0] == _gen(model, mel, 5, PHRASES)[0].sequences_ids[0]
    few = _gen(model, mel, 5, OTHER[:2], num_hypotheses=4)[0]      # fewer phrases than results asked: the -inf fillers are dropped
    assert sorted(few.sequences_ids) == sorted(OTHER[:2]) and all(np.isfinite(few.scores)) and few.scores[0] >= few.scores[1], (few.sequences_ids, few.scores)


def test_two_utterances_equal_the_single_call(model, mel, golden_dir):
    ten = np.load(os.path.join(golden_dir, "logmel_10sec.npz"))["mel"].astype(np.float32)[None]
    both = np.ascontiguousarray(np.concatenate([mel, ten]))
    for beam, n in ((1, 1), (5, 3)):
        two = _gen(model, both, beam, PHRASES, num_hypotheses=n)
        for b, m1 in enumerate((mel, ten)):
            one = _gen(model, np.ascontiguousarray(m1), beam, PHRASES, num_hypotheses=n)[0]
            assert two[b].sequences_ids == one.sequences_ids, (beam, b, two[b].sequences_ids, one.sequences_ids)
            assert np.allclose(two[b].scores, one.scores, atol=2e-3), (beam, b, two[b].scores, one.scores)


def test_every_call_gets_its_own_set_and_no_new_graph(model, mel):
    """Two calls with different sets answer from their own; installing a set is a copy - the step graphs captured for one set serve every set
    whose longest phrase is as long - and a plain call between them is today's call from today's graph key."""
    from wis_hip import ctranslate2 as ct2
    # (beam 4: a shape no other test of this module decodes at, so what is captured here is captured by this test)
    f = ct2.StorageView.from_array(mel)
    plain = model.generate(f, [PROMPT], beam_size=4, fixed_new_tokens=6)[0].sequences_ids[0]
    g_plain = _graphs(model)
    assert model.generate(f, [PROMPT], beam_size=4, fixed_new_tokens=6)[0].sequences_ids[0] == plain and _graphs(model) == g_plain
    a = _gen(model, mel, 4, PHRASES)[0]
    g_a = _graphs(model)
    assert g_a > g_plain                                      # the constrained step is another graph (phrase_rules_kernel in the tail)
    b = _gen(model, mel, 4, OTHER)[0]
    assert a.sequences_ids[0] in PHRASES and b.sequences_ids[0] in OTHER
    a2 = _gen(model, mel, 4, PHRASES)[0]
    assert a2.sequences_ids == a.sequences_ids and a2.scores == a.scores
    same_len = [[2425, 322, 264, 1442, 13, 13], [1590, 12, 12, 12, 12, 12]]      # as long as PHRASES' longest: the same max_new, so the same graph key
    g_before = _graphs(model)                                 # (OTHER's longest phrase is shorter: max_new_tokens is part of every step graph's key)
    c = _gen(model, mel, 4, same_len)[0]
    assert c.sequences_ids[0] in same_len and _graphs(model) == g_before
    _gen(model, mel, 4, PHRASES)
    _gen(model, mel, 4, same_len)
    assert _graphs(model) == g_before                        # switching between installed sets captures nothing
    assert model.generate(f, [PROMPT], beam_size=4, fixed_new_tokens=6)[0].sequences_ids[0] == plain and _graphs(model) == g_before


def test_combined_with_a_long_prompt_and_the_repetition_options(model, mel, brute):
    """An initial prompt of more than 16 tokens takes the long-prompt route (windowed prefill, wis_generate's d_plen step): the history the walk
    reads still starts behind the prompt."""
    long_prompt = [50361] + [1000 + 7 * i for i in range(30)] + PROMPT
    for beam in (1, 5):
        r = _gen(model, mel, beam, PHRASES, prompt=long_prompt, num_hypotheses=min(beam, 2))[0]
        assert all(x in PHRASES for x in r.sequences_ids) and list(r.scores) == sorted(r.scores, reverse=True), (beam, r.sequences_ids)
    r = _gen(model, mel, 5, PHRASES, repetition_penalty=1.3, no_repeat_ngram_size=2)[0]
    assert r.sequences_ids[0] in PHRASES
    # prompts of different lengths in one device batch (wis_generate_ragged)
    from wis_hip import ctranslate2 as ct2
    both = np.ascontiguousarray(np.concatenate([mel, mel]))
    rr = model.generate(ct2.StorageView.from_array(both), [long_prompt, PROMPT], beam_size=5, phrases=PHRASES, ragged_prompts=True)
    assert rr[1].sequences_ids == _gen(model, mel, 5, PHRASES)[0].sequences_ids
    assert rr[0].sequences_ids == _gen(model, mel, 5, PHRASES, prompt=long_prompt)[0].sequences_ids


def test_generate_refusals(model, mel):
    from wis_hip import ctranslate2 as ct2
    f = ct2.StorageView.from_array(mel)
    for kw in (dict(beam_size=1, sampling_topk=0), dict(beam_size=5, fixed_new_tokens=4), dict(beam_size=1, draft_tokens=[400, 401]), dict(beam_size=5, num_hypotheses=6)):
        with pytest.raises(ValueError):
            model.generate(f, [PROMPT], phrases=PHRASES, **kw)
    with pytest.raises(ValueError):
        model.generate(f, [PROMPT[:3]], beam_size=5, phrases=PHRASES)      # a timestamp prompt
    with pytest.raises(ValueError) as e:
        model.generate(f, [PROMPT], beam_size=5, phrases=[[2425, EOT]])
    assert "[2425, 50257]" in str(e.value)


class _Vocab:
    """a tokenizer with a vocabulary: every word is one token (its id spelled out), " " + text.strip() as a prompt is encoded"""
    has_vocabulary, all_special_ids = True, []
    decode = staticmethod(lambda ids: "".join(f" w{int(t)}" for t in ids if int(t) < EOT))

    @staticmethod
    def encode(text):
        assert text.startswith(" ")
        return [int(w[1:]) for w in text.split()]


def test_do_whisper_matches(golden_dir):
    from wis_hip import audio
    from wis_hip.settings import APISettings
    from wis_hip.whisper import WhisperModels, do_whisper
    s = APISettings()
    s.whisper_model_path = "synthetic:{size}"
    models = WhisperModels(s, device_index=[0])
    try:
        models.get("tiny")
        models.tokenizers["tiny"] = _Vocab()
        pcm, _ = audio.load_audio(os.path.join(golden_dir, "clips", "3sec.flac"))
        texts = ["w2425 w322", " w1590 ", "w8962 w493", "w4813 w264 w2853"]
        r = do_whisper(pcm, "tiny", 5, "transcribe", False, "en", models=models, phrases=texts + [[7405, 11]], phrase_nbest=3)
        assert isinstance(r.matches, list) and len(r.matches) == 3
        assert all(set(m) == {"text", "score"} and isinstance(m["text"], str) and isinstance(m["score"], float) and np.isfinite(m["score"]) for m in r.matches), r.matches
        allowed = [t.strip() for t in texts] + ["w7405 w11"]
        assert all(m["text"] in allowed for m in r.matches) and len({m["text"] for m in r.matches}) == 3, r.matches
        assert [m["score"] for m in r.matches] == sorted((m["score"] for m in r.matches), reverse=True)
        assert r[1] == r.matches[0]["text"] and r.tokens in ([2425, 322], [1590], [8962, 493], [4813, 264, 2853], [7405, 11])      # `text` is the best phrase
        one = do_whisper(pcm, "tiny", 5, "transcribe", False, "en", models=models, phrases=texts, initial_prompt=[1000 + i for i in range(40)], repetition_penalty=1.2)
        assert len(one.matches) == 1 and one.matches[0]["text"] in allowed and one[1] == one.matches[0]["text"]
        assert do_whisper(pcm, "tiny", 5, "transcribe", False, "en", models=models, fixed_new_tokens=4).matches is None      # a plain request: no `matches`
        with pytest.raises(ValueError):
            do_whisper(pcm, "tiny", 5, "transcribe", False, "en", models=models, phrases=texts, phrase_nbest=6)
        with pytest.raises(ValueError):
            do_whisper(np.zeros(16000 * 31, np.float32), "tiny", 5, "transcribe", False, "en", models=models, phrases=texts)
    finally:
        models.get("tiny").close()
