"""-m gpu: the in-grammar mass of phrase-constrained decoding through the engine.

SEARCH ON SUPPLIED LOGITS (wis_debug_search / wis_debug_search_n with phrase_mass on): every beam of an utterance is given the SAME row at a
step, so the row behind a history is the step's row whatever slot the history sits in, and the float64 reference (tests/phrase_mass_ref.py) needs no
search of its own: a result's mass is the sum over its path of the rule on rows the test holds.  Ids and scores must be bit-equal to the same call
with the option off.  Tolerance per result: SAFETY x the derived bound of its worst node x the path length, plus the fp32 roundoff of the sum.
WHOLE ENGINE at synthetic:tiny: the best phrase's mass against float64 over the engine's own teacher-forced logits (wis_debug_logits), tolerance
2 (len + 1) delta with delta = 5e-2, the max-abs bound tests/test_gpu_e2e.py (and tests/test_gpu_phrase_e2e.py after it) holds teacher-forced logits
of this model size to - a logits error of delta moves log num and log den of one step by at most delta each."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import phrase_mass_ref as R
from phrase_ref import allowed, prefix_dict
from rep_ref import penalise
from test_gpu_phrase_e2e import OTHER, PHRASES, PROMPT, _Vocab, _graphs
from test_gpu_phrase_rules import _install, _pool, _run_engine

pytestmark = pytest.mark.gpu
V, EOT = 51865, 50257
NEG = float("-inf")
DELTA = 5e-2
WIS_E_ARG, WIS_E_STATE = -1, -6


@pytest.fixture(scope="module")
def engine():
    from wis_hip import ctranslate2 as ct2, weights as W
    model = ct2.Whisper("unused", weights=W.synthetic_weights("tiny", seed=1234), arch=W.arch("tiny"), max_batch=4, max_beam=5)
    yield model
    model.close()


def _last_mass(model, B, n):
    from wis_hip import _lib
    out = np.zeros((B, n), np.float32)
    rc = _lib.load().wis_last_phrase_mass(model._replicas[0].handle, B, n, out.ctypes.data_as(C.POINTER(C.c_float)))
    return rc, out


def _biases():
    from wis_hip import weights as W
    ba, bb = np.zeros(V, np.float32), np.zeros(V, np.float32)
    ba[list(W.SUPPRESS_IDS)] = NEG
    bb[list(W.SUPPRESS_IDS_BEGIN)] = NEG
    return ba, bb


def _path_reference(row_of, prefixes, path):
    """-> (float64 sum over the path's len + 1 nodes, the tolerance the module docstring states); row_of(step, history) -> u"""
    per, bounds = [], []
    for s in range(len(path) + 1):
        h = tuple(path[:s])
        u = row_of(s, h)
        keep = allowed(prefixes, h)
        per.append(R.logmass(u, keep)); bounds.append(R.logmass_bound(u, keep))
    n = len(per)
    return float(np.sum(per)), R.SAFETY * max(bounds) * n + n * R.U * float(np.sum(np.abs(per)))


def _scene(rng):
    """Five phrases of 1 .. 3 tokens, [a, b] a prefix of [a, b, a] (behind [a, b] the repetition penalty moves the child a); two utterances:
    utterance 0 says phrase [a, b] (its tokens, then <|endoftext|>, 25 above a N(0, 2^2) row); utterance 1's best token lies OUTSIDE the set at
    steps 0 and 1 (20 above the row), with a mild preference for [f, g] inside it.  (A beam search ends once beam_size hypotheses have finished:
    at beam 4 that is behind step 2, so both phrases are 2 tokens long.)"""
    pool = _pool()
    a, b, d, e, f, g, out = (int(t) for t in rng.choice(pool, size=7, replace=False))
    phrases = [[a, b, a], [a, b], [a, d], [e], [f, g]]
    steps = 4
    base = (2.0 * rng.standard_normal((steps, 2, V))).astype(np.float32)
    for s, t in enumerate([a, b, EOT]):
        base[s, 0, t] = 25.0
    for s, t in enumerate([f, g, EOT]):
        base[s, 1, t] = 6.0
    base[0, 1, out] = 20.0
    base[1, 1, out] = 20.0
    return phrases, base, [a, b], [f, g]


@pytest.mark.parametrize("beam,n_hyp,pen", [(1, 1, None), (4, 1, None), (4, 4, None), (4, 3, 1.3)])
def test_search_on_supplied_logits(engine, beam, n_hyp, pen):
    rng = np.random.default_rng(100 + beam + n_hyp)
    phrases, base, said, forced = _scene(rng)
    prefixes = prefix_dict(phrases)
    B, steps = 2, base.shape[0]
    table = np.ascontiguousarray(np.repeat(base, beam, axis=1))                      # row (b, j) of a step = the step's row of utterance b
    _install(engine, phrases)
    off = _run_engine(engine, table, B, beam, 3, n_hyp=n_hyp, p=pen)
    rc, _ = _last_mass(engine, B, n_hyp)
    assert rc == WIS_E_STATE                                                         # the last call did not compute the mass
    on = _run_engine(engine, table, B, beam, 3, n_hyp=n_hyp, p=pen, phrase_mass=1)
    assert on[0] == off[0] and on[1].tobytes() == off[1].tobytes() and np.array_equal(on[2], off[2]) and np.array_equal(on[3], off[3])      # ids, scores (bits), finish steps, parents
    rc, mass = _last_mass(engine, B, n_hyp)
    assert rc == 0 and not np.isnan(mass).any(), mass
    assert _last_mass(engine, B, n_hyp + 1)[0] == WIS_E_ARG and _last_mass(engine, B + 1, n_hyp)[0] == WIS_E_ARG
    ba, bb = _biases()

    def row_of(b):
        def f(s, h):
            x = base[s, b]
            if pen is not None:
                x = penalise(torch.from_numpy(x[None].copy()), [list(h)], pen)[0].numpy()
            return R.u_row(x, ba, bb, first=s == 0)
        return f
    ids = on[0] if n_hyp > 1 else [[x] for x in on[0]]
    scores = on[1].reshape(B, n_hyp)
    worst = 0.0
    for b in range(B):
        for k in range(n_hyp):
            if scores[b, k] == NEG:                                                  # a filler: the set reached fewer phrases than the search wanted
                assert mass[b, k] == NEG
                continue
            assert ids[b][k] in phrases
            ref, tol = _path_reference(row_of(b), prefixes, ids[b][k])
            assert abs(mass[b, k] - ref) <= tol, (b, k, ids[b][k], mass[b, k], ref, tol)
            worst = max(worst, abs(mass[b, k] - ref) / tol)
    assert ids[0][0] == said and ids[1][0] == forced
    assert -1e-2 < mass[0, 0] <= 0.0                                                 # in grammar: the list allowed (nearly) all of the model's probability
    assert mass[1, 0] < -20.0                                                        # forced: the best token lay outside the set at two steps
    print(f"\n[phrase mass] search beam {beam}, {n_hyp} results, penalty {pen}: mass {mass.round(4).tolist()}, worst error / tolerance {worst:.3f}")


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


def _teacher_forced_mass(model, mel, phrases, path):
    """float64 over the engine's own logits behind PROMPT + every prefix of `path` (one wis_debug_logits call)"""
    from wis_hip import _lib
    P = len(PROMPT)
    dec_in = np.ascontiguousarray(np.asarray([PROMPT + list(path)], np.int32))
    T = dec_in.shape[1]
    out = np.zeros((1, T, V), np.float32)
    _lib.check(_lib.load().wis_debug_logits(model._replicas[0].handle, _lib.ptr(mel), _lib.WIS_IN_MEL_HOST, 1, dec_in.ctypes.data_as(C.POINTER(C.c_int32)), T,
                                            out.ctypes.data_as(C.POINTER(C.c_float))))
    ba, bb = _biases()
    pre = prefix_dict(phrases)
    return float(sum(R.logmass(R.u_row(out[0, P - 1 + i], ba, bb, first=i == 0), allowed(pre, path[:i])) for i in range(len(path) + 1)))


def test_whole_engine_against_teacher_forced_logits(model, mel):
    from wis_hip import _lib, ctranslate2 as ct2
    f = ct2.StorageView.from_array(mel)
    gen = lambda phrases, **kw: model.generate(f, [PROMPT], beam_size=3, phrases=phrases, return_scores=True, **kw)[0]
    off = gen(PHRASES, num_hypotheses=2)
    g_off = _graphs(model)
    assert off.phrase_logmass is None
    rc, _ = _last_mass(model, 1, 2)
    assert rc == WIS_E_STATE
    on = gen(PHRASES, num_hypotheses=2, return_phrase_mass=True)
    g_on = _graphs(model)
    assert on.sequences_ids == off.sequences_ids and on.scores == off.scores          # the same search, bit for bit
    assert g_on > g_off                                                               # the step with the mass kernel is another graph ...
    assert gen(PHRASES, num_hypotheses=2).scores == off.scores and _graphs(model) == g_on      # ... and the option off still replays its own: nothing new
    assert len(on.phrase_logmass) == 2 and all(np.isfinite(on.phrase_logmass)) and all(v <= 0.0 for v in on.phrase_logmass)
    for ids, got in zip(on.sequences_ids, on.phrase_logmass):
        ref = _teacher_forced_mass(model, mel, PHRASES, ids)
        tol = 2 * (len(ids) + 1) * DELTA
        print(f"\n[phrase mass] tiny, beam 3: phrase {ids}: mass {got:.4f}, float64 over teacher-forced logits {ref:.4f} (tolerance {tol})")
        assert abs(got - ref) <= tol, (ids, got, ref, tol)
    # another set installed: its own values, nothing stale, no NaN
    other = gen(OTHER, return_phrase_mass=True)
    assert other.sequences_ids[0] in OTHER and np.isfinite(other.phrase_logmass[0])
    ref = _teacher_forced_mass(model, mel, OTHER, other.sequences_ids[0])
    assert abs(other.phrase_logmass[0] - ref) <= 2 * (len(other.sequences_ids[0]) + 1) * DELTA, (other.phrase_logmass, ref)
    again = gen(PHRASES, num_hypotheses=2, return_phrase_mass=True)
    assert again.phrase_logmass == on.phrase_logmass
    # fewer phrases than results asked: the fillers are dropped, their masses with them
    few = gen(OTHER[:2], num_hypotheses=3, return_phrase_mass=True)
    assert len(few.sequences_ids) == len(few.phrase_logmass) == 2 and all(np.isfinite(few.phrase_logmass))
    # a call without the option: the handle answers WIS_E_STATE again
    model.generate(f, [PROMPT], beam_size=3, fixed_new_tokens=4)
    assert _last_mass(model, 1, 1)[0] == WIS_E_STATE
    # the engine refuses the flag without phrases, and any other value
    lib, h = _lib.load(), model._replicas[0].handle
    ids = np.zeros((1, 8), np.int32); lens = np.zeros(1, np.int32); sc = np.zeros(1, np.float32)
    for phrases_v, mass_v in ((0, 1), (1, 2), (1, -1)):
        o = _lib.GenOpts(_lib.WIS_IN_MEL_HOST, 3, 0, 1.0, 1.0, 1, 1, 0, 0)
        o.phrases, o.phrase_mass = phrases_v, mass_v
        rc = lib.wis_generate(h, _lib.ptr(mel), 1, np.asarray(PROMPT, np.int32).ctypes.data_as(C.POINTER(C.c_int32)), len(PROMPT), C.byref(o),
                              ids.ctypes.data_as(C.POINTER(C.c_int32)), lens.ctypes.data_as(C.POINTER(C.c_int32)), sc.ctypes.data_as(C.POINTER(C.c_float)))
        assert rc == WIS_E_ARG, (phrases_v, mass_v, rc)
    with pytest.raises(ValueError):
        model.generate(f, [PROMPT], beam_size=3, return_phrase_mass=True)


def test_two_utterances_equal_the_single_calls(model, mel, golden_dir):
    from wis_hip import ctranslate2 as ct2
    ten = np.load(os.path.join(golden_dir, "logmel_10sec.npz"))["mel"].astype(np.float32)[None]
    both = np.ascontiguousarray(np.concatenate([mel, ten]))
    two = model.generate(ct2.StorageView.from_array(both), [PROMPT] * 2, beam_size=3, phrases=PHRASES, return_phrase_mass=True)
    for b, m1 in enumerate((mel, ten)):
        one = model.generate(ct2.StorageView.from_array(np.ascontiguousarray(m1)), [PROMPT], beam_size=3, phrases=PHRASES, return_phrase_mass=True)[0]
        assert two[b].sequences_ids == one.sequences_ids
        assert abs(two[b].phrase_logmass[0] - one.phrase_logmass[0]) <= 2 * (len(one.sequences_ids[0]) + 1) * DELTA, (b, two[b].phrase_logmass, one.phrase_logmass)


def test_do_whisper_logmass_threshold_and_fallback(golden_dir):
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
        dw = lambda **kw: do_whisper(pcm, "tiny", 5, "transcribe", False, "en", models=models, **kw)
        r = dw(phrases=texts, phrase_nbest=3, phrase_mass=True)
        assert len(r.matches) == 3 and r.matched is None
        for m in r.matches:
            assert set(m) == {"text", "score", "logmass", "in_grammar"} and np.isfinite(m["logmass"]) and m["logmass"] <= 0.0 and 0.0 <= m["in_grammar"] <= 1.0, m
            assert m["in_grammar"] == pytest.approx(np.exp(m["logmass"] / (len(m["text"].split()) + 1)))
        unconstrained = dw()
        assert unconstrained.matches is None and unconstrained[1] not in [t.strip() for t in texts]
        # a threshold of 1.0 needs a mass of exactly 0: the seeded model never gives one - not matched, and the fallback is the unconstrained transcript
        fb = dw(phrases=texts, phrase_nbest=2, phrase_threshold=1.0, phrase_fallback=True)
        assert fb.matched is False and fb[1] == unconstrained[1] and fb.tokens == unconstrained.tokens
        assert len(fb.matches) == 2 and fb.matches[0]["text"] == r.matches[0]["text"] and fb.matches[0]["logmass"] == r.matches[0]["logmass"]
        kept = dw(phrases=texts, phrase_threshold=1.0)
        assert kept.matched is False and kept[1] == r.matches[0]["text"]              # no fallback asked: the phrase stays
        low = dw(phrases=texts, phrase_threshold=1e-30, phrase_fallback=True)
        assert low.matched is True and low[1] == r.matches[0]["text"]
    finally:
        models.get("tiny").close()
