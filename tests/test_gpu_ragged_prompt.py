"""-m gpu: prompts of DIFFERENT lengths in one device batch - `generate(..., ragged_prompts=True)` and the engine's `wis_generate_ragged`: every utterance
on the long-prompt route whatever its own length, the prefix windows per run of utterances that still have prompt left, a right-aligned last pass, the
<|startoftranscript|> row found per utterance - against the oracle, one utterance at a time.

Bars as in tests/test_gpu_prompt.py (its helpers `_prompt`, `check_utterance`, `oracle_rescore` are copied here; the oracle's own search is computed once
per (prompt, beam, convention) and shared by the tests that need it): the engine's score == the oracle's teacher-forced score of the engine's ids within
3e-3; that score within 0.1 of the oracle's best; ids identical wherever the oracle's decision margin exceeds MARGIN.  One model serves one batch, so the
EOT ramp has one start for all utterances of a test: 54 where the searches end on EOT by themselves, 230 (behind every prompt) elsewhere.  The counts of
margin-forced decisions asserted below were established with the oracle alone, on the CPU."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch  # noqa: F401  (before libwis_hip.so: one HIP runtime per process)

pytestmark = pytest.mark.gpu
MARGIN = 0.02
EOT, SOT, PREV, NO_TIMESTAMPS, NO_SPEECH = 50257, 50258, 50361, 50363, 50362
BARE = [SOT, 50259, 50359, NO_TIMESTAMPS]
NATURAL = (30, 31, 33, 36, 40, 47, 52)          # test 1: two prefill groups, ramp start 54
MIXED = (4, 16, 17, 18, 33, 100, 228)           # test 2: both sides of SHORT_PROMPT and the longest prompt, ramp start 230
E_UNSUPPORTED, E_STATE, E_ARG = -7, -6, -1


def _prompt(P, i):
    """<|startofprev|> + P - 5 text ids + <|sot|> <|lang i|> <|transcribe|> <|notimestamps|>; 4 tokens: the bare start sequence"""
    if P == 4:
        return list(BARE)
    return [PREV] + [int(t) for t in np.random.default_rng(100 * P + i).integers(0, 50257, P - 5)] + [SOT, 50259 + 7 * i, 50359, NO_TIMESTAMPS]


@pytest.fixture(scope="module")
def mel(golden_dir):
    return np.load(os.path.join(golden_dir, "logmel_3sec.npz"))["mel"].astype(np.float32)


@pytest.fixture(scope="module")
def rigs(mel):
    """ramp start -> (engine, oracle, encoder memory)"""
    from eot_ramp import with_eot_ramp
    from oracle.whisper_ref import WhisperRef
    from wis_hip import ctranslate2 as ct2, weights as W
    made = {}

    def get(start):
        if start not in made:
            w = with_eot_ramp(W.synthetic_weights("tiny", seed=1234, std=0.02, emb_std=0.06, ln_jitter=0.1), start=start, slope=0.1)
            a = W.arch("tiny")
            model = ct2.Whisper("unused", weights=w, arch=a, max_batch=8, max_beam=8)
            ref = WhisperRef(w, a["d_model"], a["n_layers"], a["n_heads"])
            made[start] = (model, ref, ref.encode(mel[None])[0].numpy())
        return made[start]
    yield get
    for model, _, _ in made.values():
        model.close()


def _feats(mel, B=1):
    from wis_hip import ctranslate2 as ct2
    return ct2.StorageView.from_array(np.ascontiguousarray(np.repeat(mel[None], B, axis=0)))


def oracle_rescore(ref, memory, prompt, ids, max_new, length_penalty=1.0, fixed_new=0):
    """tests/test_gpu_prompt.py oracle_rescore: what CT2 reports for the hypothesis `ids` under the ORACLE's model"""
    from wis_hip import weights as W
    closed = len(ids) < max_new
    seq = list(prompt) + list(ids)
    if not closed:
        seq = seq[:-1]
    lg = ref.decode_logits(np.array([seq]), torch.as_tensor(memory)[None])[0]
    total, P = 0.0, len(prompt)
    for t, tok in enumerate(list(ids) + ([ref.eot] if closed else [])):
        row = ref.apply_processors(lg[P - 1 + t][None].double(), t, W.SUPPRESS_IDS, W.SUPPRESS_IDS_BEGIN, True, fixed_new, ref.eot)
        total += float(torch.log_softmax(row, dim=-1)[0, tok])
    if length_penalty == 0:
        return total
    return total / (len(ids) ** length_penalty) if len(ids) else float("-inf")


_ORACLE = {}      # (oracle, prompt, beam, fixed_new, max_new) -> (ids, score, trace, search record): the reference, computed once and left unchanged


def _oracle_search(ref, memory, prompt, beam, fixed_new, max_new):
    from wis_hip import weights as W
    key = (id(ref), tuple(prompt), beam, fixed_new, max_new)
    if key not in _ORACLE:
        ids, score, trace = ref.generate(None, prompt, beam_size=beam, suppress_ids=W.SUPPRESS_IDS, suppress_begin=W.SUPPRESS_IDS_BEGIN, memory=memory,
                                         max_new_tokens=max_new, fixed_new=fixed_new, return_trace=True)
        _ORACLE[key] = (list(ids), float(score), list(trace), dict(ref.last_search))
    return _ORACLE[key]


def check_utterance(ref, memory, prompt, got, gscore, beam, fixed_new=0, tag="", max_new=None):
    """tests/test_gpu_prompt.py check_utterance -> (identical, decision margin exceeded MARGIN, oracle search record).  max_new: the batch's (from its
    longest prompt); None: this prompt's own."""
    max_new = min(224, 448 - len(prompt)) if max_new is None else max_new
    ids, score, trace, s = _oracle_search(ref, memory, prompt, beam, fixed_new, max_new)
    rescored = oracle_rescore(ref, memory, prompt, got, max_new, fixed_new=fixed_new)
    same = got == ids
    print(f"  {tag} beam {beam}: oracle len {len(ids)} score {score:.5f} finish step {s['finish_step']} decision margin {min(trace):.4f} | hip len {len(got)} "
          f"score {gscore:.5f}, oracle rescoring of the hip ids {rescored:.5f} | identical {same}")
    assert all(0 <= t < 51865 for t in got) and EOT not in got
    assert abs(gscore - rescored) <= 3e-3, (gscore, rescored)
    assert rescored >= score - 0.1, (rescored, score)
    forced = min(trace) > MARGIN
    if forced:
        assert same, (got, ids)
    return same, forced, s


def _check_batch(ref, memory, prompts, res, beam, fixed_new=0, tag=""):
    """every utterance of a batch against the oracle -> (identical, forced) counts; res: [(ids, score)]"""
    max_new = min(224, 448 - max(len(p) for p in prompts))
    exact = forced = 0
    for j, (p, (ids, score)) in enumerate(zip(prompts, res)):
        same, f, _ = check_utterance(ref, memory, p, ids, score, beam, fixed_new=fixed_new, tag=f"{tag} utterance {j} (P {len(p)})", max_new=max_new)
        exact += same; forced += f
    print(f"{tag} beam {beam}: {exact} of {len(prompts)} identical ({forced} forced by the margin)")
    return exact, forced


def _pairs(results):
    return [(r.sequences_ids[0], r.scores[0]) for r in results]


# ---- the engine's entry points, below the Python face ------------------------------------------------------------------------------------------------
def _engine(model, mel, prompts, beam, *, fixed_new=0, max_new=0, ragged=True, no_speech=False):
    """wis_generate_ragged (or wis_generate_n: prompts of one length) on the model's first replica -> (rc, [(ids, score)], lens, raw ids, raw scores)"""
    from wis_hip import _lib
    lib, h = _lib.load(), model._replicas[0].handle
    B = len(prompts)
    i32p, f32p = C.POINTER(C.c_int32), C.POINTER(C.c_float)
    if not max_new:
        max_new = min(224, 448 - max(len(p) for p in prompts))
    o = _lib.GenOpts(0, beam, max_new, 1.0, 1.0, 1, 1, fixed_new, 0)
    o.no_speech_prob = int(no_speech)
    ids, lens, sc = np.zeros((B, max_new), np.int32), np.zeros(B, np.int32), np.zeros(B, np.float32)
    m = np.ascontiguousarray(np.repeat(mel[None], B, axis=0))
    flat = np.ascontiguousarray(np.asarray([t for p in prompts for t in p], np.int32))
    outs = (ids.ctypes.data_as(i32p), lens.ctypes.data_as(i32p), sc.ctypes.data_as(f32p))
    with model._replicas[0].lock:
        if ragged:
            plen = np.ascontiguousarray(np.asarray([len(p) for p in prompts], np.int32))
            rc = lib.wis_generate_ragged(h, _lib.ptr(m), B, flat.ctypes.data_as(i32p), plen.ctypes.data_as(i32p), C.byref(o), None, *outs)
        else:
            assert len({len(p) for p in prompts}) == 1
            rc = lib.wis_generate_n(h, _lib.ptr(m), B, flat.ctypes.data_as(i32p), len(prompts[0]), C.byref(o), None, *outs)
    return rc, [(ids[b, :lens[b]].tolist(), float(sc[b])) for b in range(B)], lens, ids, sc


def _graph_count(model):
    from wis_hip import _lib
    n = C.c_int(-1)
    _lib.check(_lib.load().wis_debug_graph_count(model._replicas[0].handle, C.byref(n)))
    return n.value


# ---- 1. natural EOT, seven utterances ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("beam", [1, 5])
def test_seven_lengths_end_on_eot(rigs, mel, beam):
    """Lengths 30 .. 52 behind one EOT ramp that starts at position 54: seven utterances are two prefill groups (MAX_ROWS / 16 = 6), the last pass has
    96 / 7 = 13 rows per utterance.  Oracle alone, on the CPU: at beam 1 the decision margin is at least 0.0263 for all seven (23 .. 44 generated tokens) -
    all seven are forced; at beam 5 no margin clears 0.02 (largest 0.0057) - the score bars alone, and a second call that returns the same bits."""
    model, ref, memory = rigs(54)
    prompts = [_prompt(P, j + 7) for j, P in enumerate(NATURAL)]
    res = model.generate(_feats(mel, 7), prompts, beam_size=beam, ragged_prompts=True)
    assert all(len(r.sequences_ids[0]) < 100 for r in res)      # ended on EOT by themselves, far from max_new
    exact, forced = _check_batch(ref, memory, prompts, _pairs(res), beam, tag="natural EOT")
    if beam == 1:
        assert forced == 7 and exact == 7
    else:
        again = model.generate(_feats(mel, 7), prompts, beam_size=beam, ragged_prompts=True)
        assert [r.sequences_ids for r in res] == [r.sequences_ids for r in again] and [r.scores for r in res] == [r.scores for r in again]


# ---- 2. short and long in one batch, 3. any order ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def mixed(rigs, mel):
    """beam -> the results of the seven MIXED utterances through generate (which hands them to the engine longest first), fixed_new_tokens = 8"""
    made = {}

    def get(beam):
        if beam not in made:
            model, _, _ = rigs(230)
            prompts = [_prompt(P, j) for j, P in enumerate(MIXED)]
            made[beam] = (prompts, _pairs(model.generate(_feats(mel, 7), prompts, beam_size=beam, fixed_new_tokens=8, ragged_prompts=True)))
        return made[beam]
    return get


@pytest.mark.parametrize("beam", [1, 5])
def test_short_and_long_prompts_in_one_batch(rigs, mel, mixed, beam):
    """Lengths 4, 16, 17, 18, 33, 100, 228: utterances of up to 16 tokens take the long-prompt route too (no prefix window at all: their prompt is shorter
    than the last pass, whose rows in front repeat the first), 228 runs 14 windows alone.  Oracle alone: at beam 1 the margins are at least 0.0203
    (P = 33 sits on the line) - at least six forced; at beam 5 P = 17 (0.0435) and P = 100 (0.0538) clear it - at least two."""
    _, ref, memory = rigs(230)
    prompts, res = mixed(beam)
    assert all(len(ids) == 8 for ids, _ in res)
    exact, forced = _check_batch(ref, memory, prompts, res, beam, fixed_new=8, tag="short and long")
    assert forced >= (6 if beam == 1 else 2) and exact >= forced


def test_short_prompts_alone_at_beam_8(rigs, mel):
    """the first three (4, 16, 17 tokens) at beam 8: the score bars"""
    model, ref, memory = rigs(230)
    prompts = [_prompt(P, j) for j, P in enumerate(MIXED[:3])]
    res = _pairs(model.generate(_feats(mel, 3), prompts, beam_size=8, fixed_new_tokens=8, ragged_prompts=True))
    assert all(len(ids) == 8 for ids, _ in res)
    _check_batch(ref, memory, prompts, res, 8, fixed_new=8, tag="short, beam 8")


def test_any_order_of_lengths(rigs, mel, mixed):
    """The same seven through wis_generate_ragged directly in ASCENDING order - the worst case of the run rule: window t carries a tail of the batch, the
    4-token utterance sits in front of everything.  Each meets the bars, and has the ids of the sorted call wherever the margin forces them."""
    model, ref, memory = rigs(230)
    prompts, sorted_res = mixed(1)
    assert [len(p) for p in prompts] == sorted(len(p) for p in prompts)
    rc, res, _, _, _ = _engine(model, mel, prompts, 1, fixed_new=8)
    assert rc == 0
    max_new = min(224, 448 - 228)
    for j, (p, (ids, score)) in enumerate(zip(prompts, res)):
        same, forced, _ = check_utterance(ref, memory, p, ids, score, 1, fixed_new=8, tag=f"ascending, utterance {j} (P {len(p)})", max_new=max_new)
        if forced:
            assert ids == sorted_res[j][0], (j, ids, sorted_res[j][0])
    # ... and after a ragged call the trajectory is not handed out (its rows do not line up with a drafted call's)
    from wis_hip import _lib
    tok, org, n = np.zeros((256, 1), np.int32), np.zeros((256, 1), np.int32), C.c_int32(0)
    i32p = C.POINTER(C.c_int32)
    assert _lib.load().wis_last_trajectory(model._replicas[0].handle, 0, tok.ctypes.data_as(i32p), org.ctypes.data_as(i32p), 256, C.byref(n)) == E_STATE


# ---- 4. the uniform case is today's ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P", [33, 4])
def test_equal_lengths_are_the_uniform_call(rigs, mel, P):
    model, _, _ = rigs(54)
    prompts = [_prompt(P, i) if P != 4 else [SOT, 50259 + 7 * i, 50359, NO_TIMESTAMPS] for i in range(3)]
    rc_n, _, len_n, ids_n, sc_n = _engine(model, mel, prompts, 5, ragged=False)
    rc_r, _, len_r, ids_r, sc_r = _engine(model, mel, prompts, 5, ragged=True)
    assert rc_n == 0 and rc_r == 0 and len_n.min() >= 1
    assert np.array_equal(ids_n, ids_r) and np.array_equal(len_n, len_r) and sc_n.tobytes() == sc_r.tobytes()
    plain = model.generate(_feats(mel, 3), prompts, beam_size=5)
    keyword = model.generate(_feats(mel, 3), prompts, beam_size=5, ragged_prompts=True)
    assert [r.sequences_ids for r in plain] == [r.sequences_ids for r in keyword] and [r.scores for r in plain] == [r.scores for r in keyword]
    assert [r.sequences_ids[0] for r in plain] == [ids_n[b, :len_n[b]].tolist() for b in range(3)]


# ---- 5. one step graph ---------------------------------------------------------------------------------------------------------------------------------
def test_ragged_calls_replay_the_uniform_calls_step_graph(rigs, mel):
    """The prompt lengths are device memory: a ragged call replays the step graphs a uniform long-prompt call of the same (B, beam, options, max_new)
    captured.  max_new is part of the graph key and resolves from the longest prompt (220 behind 228 tokens, 224 behind 40), so the three calls name the
    same max_new_tokens = 64 - through the engine's entry points, which take it as it is."""
    model, ref, memory = rigs(230)
    mk = lambda P: [PREV] + list(range(1000, 1000 + P - 5)) + BARE
    rc, _, _, _, _ = _engine(model, mel, [mk(40), mk(40)], 5, fixed_new=6, max_new=64, ragged=False)
    n0 = _graph_count(model)
    assert rc == 0 and n0 >= 1
    for lengths in ((40, 57), (23, 228)):
        prompts = [mk(P) for P in lengths]
        rc, res, _, _, _ = _engine(model, mel, prompts, 5, fixed_new=6, max_new=64)
        assert rc == 0 and _graph_count(model) == n0, lengths
        for p, (ids, score) in zip(prompts, res):
            assert len(ids) == 6
            check_utterance(ref, memory, p, ids, score, 5, fixed_new=6, tag=f"lengths {lengths}, P {len(p)}, fixed 6", max_new=64)
    rc, _, _, _, _ = _engine(model, mel, [mk(41), mk(41)], 5, fixed_new=6, max_new=64, ragged=False)      # ... and the other way round
    assert rc == 0 and _graph_count(model) == n0


# ---- 6. no_speech_prob ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [4, 8])
def test_no_speech_prob_row_by_utterance(rigs, mel, B):
    """A plain 100-token prompt (its <|startoftranscript|> row in the last pass), the 100-token prompt whose row sits 20 rows earlier (a prefix window -
    which the 20- and 4-token utterances are not part of), a 20-token and a 4-token prompt (rows of the last pass, behind repeated first rows)."""
    model, ref, memory = rigs(230)
    four = [_prompt(100, 1), _prompt(80, 1) + list(range(2000, 2020)), _prompt(20, 1), list(BARE)]
    assert [len(p) for p in four] == [100, 100, 20, 4]
    want = []
    for p in four:
        sot = p.index(SOT)
        lg = ref.decode_logits(np.array([p[:sot + 1]]), torch.as_tensor(memory)[None])[0, -1]
        want.append(float(torch.softmax(torch.as_tensor(lg).double(), -1)[NO_SPEECH]))
    prompts = four * (B // 4)
    res = model.generate(_feats(mel, B), prompts, beam_size=1, fixed_new_tokens=3, return_no_speech_prob=True, ragged_prompts=True)
    for b in range(B):
        print(f"  B {B} utterance {b} (P {len(prompts[b])}): no_speech_prob {res[b].no_speech_prob:.6f}, oracle {want[b % 4]:.6f}")
        assert abs(res[b].no_speech_prob - want[b % 4]) <= 1e-3 and res[b].no_speech_prob > 0.0, (B, b, res[b].no_speech_prob, want[b % 4])


# ---- 7. timestamps and repetition ------------------------------------------------------------------------------------------------------------------------
def _ts_prompt(P):
    return [PREV] + [int(t) for t in np.random.default_rng(P).integers(0, 50257, P - 4)] + [SOT, 50259, 50359]


@pytest.mark.parametrize("beam", [1, 5])
def test_timestamp_rules_hold_per_utterance(rigs, mel, beam):
    from ts_ref import grammar_errors
    model, _, _ = rigs(230)
    prompts = [_ts_prompt(33), _ts_prompt(61)]
    assert [len(p) for p in prompts] == [33, 61]
    for r in model.generate(_feats(mel, 2), prompts, beam_size=beam, max_length=100, ragged_prompts=True):
        ids = r.sequences_ids[0]
        assert ids and ids[0] > NO_TIMESTAMPS and NO_TIMESTAMPS not in ids and grammar_errors(ids) == [], ids


@pytest.mark.parametrize("beam", [1, 5])
def test_no_repeat_ngram_holds_per_utterance(rigs, mel, beam):
    model, _, _ = rigs(230)
    prompts = [_prompt(33, 0), _prompt(61, 0)]
    for r in model.generate(_feats(mel, 2), prompts, beam_size=beam, max_length=100, no_repeat_ngram_size=2, ragged_prompts=True):
        ids = r.sequences_ids[0]
        bigrams = list(zip(ids, ids[1:]))
        assert len(ids) >= 8 and len(bigrams) == len(set(bigrams)), ids


# ---- 8. sampling ------------------------------------------------------------------------------------------------------------------------------------------
def test_sampled_decode_is_seeded_per_utterance(rigs, mel):
    model, _, _ = rigs(230)
    prompts = [_prompt(17, 0), _prompt(100, 0)]
    kw = dict(beam_size=1, num_hypotheses=3, sampling_topk=0, sampling_temperature=0.7, sampling_seed=[20240607, 11], return_scores=True, max_length=160,
              ragged_prompts=True)
    a = model.generate(_feats(mel, 2), prompts, **kw)
    b = model.generate(_feats(mel, 2), prompts, **kw)
    assert [r.sequences_ids for r in a] == [r.sequences_ids for r in b] and [r.scores for r in a] == [r.scores for r in b]
    for r in a:
        assert len(r.sequences_ids) == 3 and all(len(s) >= 1 for s in r.sequences_ids) and all(np.isfinite(s) for s in r.scores)
        assert len({tuple(s) for s in r.sequences_ids}) > 1


# ---- 9. refusals ------------------------------------------------------------------------------------------------------------------------------------------
_CHILD = r"""
import ctypes as C, json, os, sys
import numpy as np
import torch  # noqa: F401
sys.path[:0] = [p for p in sys.argv[1].split(os.pathsep) if p]
from wis_hip import _lib, ctranslate2 as ct2, weights as W
mel = np.load(sys.argv[2])["mel"].astype(np.float32)
model = ct2.Whisper("unused", weights=W.synthetic_weights("tiny", seed=1234, std=0.02, emb_std=0.06, ln_jitter=0.1), arch=W.arch("tiny"), max_batch=2, max_beam=5)
mk = lambda P: [50361] + list(range(1000, 1000 + P - 5)) + [50258, 50259, 50359, 50363]
lib, h = _lib.load(), model._replicas[0].handle
i32p = C.POINTER(C.c_int32)
o = _lib.GenOpts(0, 1, 16, 1.0, 1.0, 1, 1, 4, 0)
m2 = np.ascontiguousarray(np.repeat(mel[None], 2, axis=0))
flat, plen = np.asarray(mk(20) + mk(33), np.int32), np.asarray([20, 33], np.int32)
ids, lens, sc = np.zeros((2, 16), np.int32), np.zeros(2, np.int32), np.zeros(2, np.float32)
rc = lib.wis_generate_ragged(h, _lib.ptr(m2), 2, flat.ctypes.data_as(i32p), plen.ctypes.data_as(i32p), C.byref(o), None, ids.ctypes.data_as(i32p),
                             lens.ctypes.data_as(i32p), sc.ctypes.data_as(C.POINTER(C.c_float)))
r = model.generate(ct2.StorageView.from_array(m2), [mk(33), mk(33)], beam_size=1, fixed_new_tokens=4)
model.close()
print("RESULT " + json.dumps({"ragged_rc": int(rc), "uniform_lens": [len(x.sequences_ids[0]) for x in r]}))
"""


def test_refusals(rigs, mel, golden_dir):
    model, _, _ = rigs(230)
    two = [_prompt(33, 0), _prompt(40, 0)]
    with pytest.raises(ValueError, match="all prompts must have the same length"):
        model.generate(_feats(mel, 2), two, beam_size=1)
    with pytest.raises(ValueError, match="draft"):
        model.generate(_feats(mel, 2), two, beam_size=1, ragged_prompts=True, draft_tokens=[1000, 1001, 1002])
    with pytest.raises(ValueError, match="return_trajectory"):
        model.generate(_feats(mel, 2), two, beam_size=5, ragged_prompts=True, return_trajectory=True)
    with pytest.raises(ValueError, match="prompt length 229"):
        model.generate(_feats(mel, 2), [two[0], [PREV] + [1000] * 224 + BARE], beam_size=1, ragged_prompts=True)
    with pytest.raises(ValueError, match="timestamps"):
        model.generate(_feats(mel, 2), [two[0], _ts_prompt(40)], beam_size=1, ragged_prompts=True)
    # the engine's own, below the Python face: a length outside 1 .. 228, max plen + max_new beyond the context, a prompt without <|startoftranscript|>
    assert _engine(model, mel, [two[0], [1000] * 229], 1)[0] == E_UNSUPPORTED
    assert _engine(model, mel, [two[0], [PREV] + [1000] * 223 + BARE], 1, max_new=221)[0] == E_ARG
    assert _engine(model, mel, [two[0], [PREV] + [1000] * 30], 1, fixed_new=3, no_speech=True)[0] == E_ARG
    assert _engine(model, mel, two, 1, fixed_new=3)[0] == 0
    # the TREE form of the step's self-attention keeps the prompt length as a kernel argument: no ragged batch there.  The switch is read once per process
    p = subprocess.run([sys.executable, "-c", _CHILD, os.pathsep.join(sys.path), os.path.join(golden_dir, "logmel_3sec.npz")],
                       env=dict(os.environ, WIS_SA_LONG="0"), capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    got = json.loads(next(l for l in p.stdout.splitlines() if l.startswith("RESULT "))[7:])
    assert got == {"ragged_rc": E_UNSUPPORTED, "uniform_lens": [4, 4]}, got
