"""-m gpu: prompted decoding - prompts of 17 .. 228 tokens (an `initial_prompt` behind <|startofprev|>, a `prefix` behind the start sequence) through
`ctranslate2.Whisper.generate`, i.e. the engine's long-prompt route: windowed prefill, the prompt length in device memory, the prompt's K / V shared in the
utterance's first slot (dec_self_attn_long_kernel, the cache reorder that leaves it alone), against the oracle.

Bars as in tests/test_gpu_eot.py (its helpers are copied here): the engine's score == the oracle's teacher-forced score of the engine's ids including the
closing EOT within 3e-3; that score within 0.1 of the oracle's best; ids identical wherever the oracle's decision margin exceeds MARGIN.  The weights carry
an EOT ramp that starts two positions behind the prompt, so every search ends on EOT by itself after 17 .. 28 tokens."""
import ctypes as C
import os

import numpy as np
import pytest
import torch  # noqa: F401  (before libwis_hip.so: one HIP runtime per process)

pytestmark = pytest.mark.gpu
MARGIN = 0.02
EOT, SOT, PREV, NO_TIMESTAMPS, NO_SPEECH = 50257, 50258, 50361, 50363, 50362
LENGTHS = (17, 33, 100, 228)


def _prompt(P, i):
    """<|startofprev|> + P - 5 text ids + <|sot|> <|lang i|> <|transcribe|> <|notimestamps|>"""
    return [PREV] + [int(t) for t in np.random.default_rng(100 * P + i).integers(0, 50257, P - 5)] + [SOT, 50259 + 7 * i, 50359, NO_TIMESTAMPS]


@pytest.fixture(scope="module")
def mel(golden_dir):
    return np.load(os.path.join(golden_dir, "logmel_3sec.npz"))["mel"].astype(np.float32)


@pytest.fixture(scope="module")
def rigs(mel):
    """P -> (engine, oracle, encoder memory): the EOT ramp starts behind the prompt, so the weights differ with P"""
    from eot_ramp import with_eot_ramp
    from oracle.whisper_ref import WhisperRef
    from wis_hip import ctranslate2 as ct2, weights as W
    made = {}

    def get(P):
        if P not in made:
            w = with_eot_ramp(W.synthetic_weights("tiny", seed=1234, std=0.02, emb_std=0.06, ln_jitter=0.1), start=P + 2, slope=0.1)
            a = W.arch("tiny")
            model = ct2.Whisper("unused", weights=w, arch=a, max_batch=8, max_beam=8)
            ref = WhisperRef(w, a["d_model"], a["n_layers"], a["n_heads"])
            made[P] = (model, ref, ref.encode(mel[None])[0].numpy())
        return made[P]
    yield get
    for model, _, _ in made.values():
        model.close()


def _feats(mel, B=1):
    from wis_hip import ctranslate2 as ct2
    return ct2.StorageView.from_array(np.ascontiguousarray(np.repeat(mel[None], B, axis=0)))


def oracle_rescore(ref, memory, prompt, ids, max_new, length_penalty=1.0, fixed_new=0):
    """tests/test_gpu_eot.py oracle_rescore (+ the fixed-length convention): what CT2 reports for the hypothesis `ids` under the ORACLE's model"""
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


def check_utterance(ref, memory, prompt, got, gscore, beam, fixed_new=0, tag=""):
    """tests/test_gpu_eot.py check_utterance -> (identical, decision margin exceeded MARGIN, oracle search record)"""
    from wis_hip import weights as W
    max_new = min(224, 448 - len(prompt))
    ids, score, trace = ref.generate(None, prompt, beam_size=beam, suppress_ids=W.SUPPRESS_IDS, suppress_begin=W.SUPPRESS_IDS_BEGIN, memory=memory,
                                     max_new_tokens=max_new, fixed_new=fixed_new, return_trace=True)
    s = ref.last_search
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


@pytest.mark.parametrize("beam", [1, 5, 8])
@pytest.mark.parametrize("P", LENGTHS)
def test_prompted_search_ends_on_eot(rigs, mel, P, beam):
    model, ref, memory = rigs(P)
    exact = forced = 0
    for i in range(3):
        r = model.generate(_feats(mel), [_prompt(P, i)], beam_size=beam)[0]
        same, f, s = check_utterance(ref, memory, _prompt(P, i), r.sequences_ids[0], r.scores[0], beam, tag=f"P {P} prompt {i}")
        assert s["finish_step"] < 100 and len(r.sequences_ids[0]) < 100      # ended on EOT by itself, far from max_new
        exact += same; forced += f
    print(f"P {P} beam {beam}, natural EOT: {exact} of 3 identical ({forced} forced by the margin)")
    # (the oracle on the CPU: the greedy margin exceeds MARGIN everywhere but at (17, 0), (33, 0), (228, 0); at beam 5 only at (33, 2))
    # checked on the CPU with the oracle: at least two of the three greedy searches of every P, and (33, beam 5, prompt 2), clear the margin - there the
    # ids are compared (check_utterance); observed on MI355X: 3 of 3 identical in all twelve (P, beam) cases, forced or not
    if beam == 1:
        assert forced >= 2
    if (P, beam) == (33, 5):
        assert forced >= 1


@pytest.mark.parametrize("B,beam,P", [(3, 5, 33), (7, 5, 33), (7, 1, 100), (3, 8, 228), (1, 5, 100)])
def test_batches_of_different_prompts_of_one_length(rigs, mel, B, beam, P):
    """Seven utterances are more than one prefill group holds (MAX_ROWS / 16 = 6): the windows run group by group, the last window shrinks to
    min(16, MAX_ROWS / B) rows per utterance."""
    model, ref, memory = rigs(P)
    prompts = [_prompt(P, i) for i in range(B)]
    res = model.generate(_feats(mel, B), prompts, beam_size=beam)
    again = model.generate(_feats(mel, B), prompts, beam_size=beam)
    assert [r.sequences_ids for r in res] == [r.sequences_ids for r in again] and [r.scores for r in res] == [r.scores for r in again]
    exact = forced = 0
    checked = list(range(B))      # (the batch of seven: both prefill groups)
    for i in checked:
        same, f, _ = check_utterance(ref, memory, prompts[i], res[i].sequences_ids[0], res[i].scores[0], beam, tag=f"batch {B} x {beam}, P {P}, utterance {i}")
        exact += same; forced += f
    print(f"{B} x beam {beam}, P {P}: {exact} of {len(checked)} checked utterances identical ({forced} forced)")      # observed on MI355X: all identical in all five shapes


@pytest.mark.parametrize("beam", [5, 8])
def test_fixed_length_behind_the_longest_prompt(rigs, mel, beam):
    """fixed_new_tokens = 8 at P = 228 (the burst loop: nine passes queued at once)"""
    model, ref, memory = rigs(228)
    for i in range(2):
        r = model.generate(_feats(mel), [_prompt(228, i)], beam_size=beam, fixed_new_tokens=8)[0]
        assert len(r.sequences_ids[0]) == 8
        check_utterance(ref, memory, _prompt(228, i), r.sequences_ids[0], r.scores[0], beam, fixed_new=8, tag=f"P 228 fixed 8 prompt {i}")


def _graph_count(model):
    from wis_hip import _lib
    n = C.c_int(-1)
    _lib.check(_lib.load().wis_debug_graph_count(model._replicas[0].handle, C.byref(n)))
    return n.value


def test_one_step_graph_serves_every_prompt_length(rigs, mel):
    """The prompt length is device memory on the long-prompt route: P = 41 replays what P = 40 captured.  (fixed_new_tokens keeps max_new - part of the
    graph key - out of the picture; both calls resolve it to 224.)"""
    model, ref, memory = rigs(33)
    mk = lambda P: [PREV] + list(range(1000, 1000 + P - 5)) + [SOT, 50259, 50359, NO_TIMESTAMPS]
    a = model.generate(_feats(mel), [mk(40)], beam_size=5, fixed_new_tokens=6)[0]
    n0 = _graph_count(model)
    assert n0 >= 1
    b = model.generate(_feats(mel), [mk(41)], beam_size=5, fixed_new_tokens=6)[0]
    assert _graph_count(model) == n0
    for P, r in ((40, a), (41, b)):
        check_utterance(ref, memory, mk(P), r.sequences_ids[0], r.scores[0], 5, fixed_new=6, tag=f"P {P} fixed 6")
    c = model.generate(_feats(mel), [mk(40)], beam_size=5, fixed_new_tokens=6)[0]
    assert c.sequences_ids == a.sequences_ids and c.scores == a.scores and _graph_count(model) == n0


def test_short_prompts_are_undisturbed(rigs, mel):
    model, _, _ = rigs(33)
    short = [SOT, 50259, 50359, NO_TIMESTAMPS]
    before = [model.generate(_feats(mel), [short], beam_size=k)[0] for k in (1, 5)]
    model.generate(_feats(mel), [_prompt(100, 0)], beam_size=5)
    model.generate(_feats(mel, 3), [_prompt(228, i) for i in range(3)], beam_size=1)
    after = [model.generate(_feats(mel), [short], beam_size=k)[0] for k in (1, 5)]
    assert [r.sequences_ids for r in before] == [r.sequences_ids for r in after] and [r.scores for r in before] == [r.scores for r in after]


def test_refusals(rigs, mel):
    model, _, _ = rigs(33)
    with pytest.raises(ValueError, match="prompt length 229"):
        model.generate(_feats(mel), [[PREV] + [1000] * 224 + [SOT, 50259, 50359, NO_TIMESTAMPS]], beam_size=1)
    with pytest.raises(ValueError, match="draft"):
        model.generate(_feats(mel), [_prompt(17, 0)], beam_size=1, draft_tokens=[1000, 1001, 1002])
    tok = np.full((3, 5), 1000, np.int32)
    with pytest.raises(ValueError, match="draft"):
        model.generate(_feats(mel), [_prompt(17, 0)], beam_size=5, draft_trajectory=(tok, np.zeros((3, 5), np.int32)))
    # the engine's own refusals, below the Python face
    from wis_hip import _lib
    lib, h = _lib.load(), model._replicas[0].handle
    i32p, f32p = C.POINTER(C.c_int32), C.POINTER(C.c_float)
    o = _lib.GenOpts(0, 1, 0, 1.0, 1.0, 1, 1, 0, 0)      # (mel from the host, beam 1, the defaults)
    ids, lens, sc = np.zeros(224, np.int32), np.zeros(1, np.int32), np.zeros(1, np.float32)
    m1 = np.ascontiguousarray(mel[None])
    p229, p17 = np.full(229, 1000, np.int32), np.asarray(_prompt(17, 0), np.int32)
    E_UNSUPPORTED = -7
    assert lib.wis_generate(h, _lib.ptr(m1), 1, p229.ctypes.data_as(i32p), 229, C.byref(o), ids.ctypes.data_as(i32p), lens.ctypes.data_as(i32p), sc.ctypes.data_as(f32p)) == E_UNSUPPORTED
    d, acc = np.full(3, 1000, np.int32), C.c_int32(0)
    assert lib.wis_generate_draft(h, _lib.ptr(m1), p17.ctypes.data_as(i32p), 17, C.byref(o), d.ctypes.data_as(i32p), 3, ids.ctypes.data_as(i32p), lens.ctypes.data_as(i32p),
                                  sc.ctypes.data_as(f32p), C.byref(acc)) == E_UNSUPPORTED


def test_no_speech_prob_behind_a_long_prompt(rigs, mel):
    """P(<|nospeech|>) at the <|startoftranscript|> row: in the last window (the plain prompt), and in an earlier one (a 20-token prefix behind the start
    sequence pushes the row out of the last 16)."""
    model, ref, memory = rigs(100)
    plain = _prompt(100, 1)
    prefixed = _prompt(80, 1) + list(range(2000, 2020))
    for prompt in (plain, prefixed):
        assert len(prompt) == 100
        sot = prompt.index(SOT)
        lg = ref.decode_logits(np.array([prompt[:sot + 1]]), torch.as_tensor(memory)[None])[0, -1]
        want = float(torch.softmax(torch.as_tensor(lg).double(), -1)[NO_SPEECH])
        for B in (1, 7):
            res = model.generate(_feats(mel, B), [prompt] * B, beam_size=2 if B == 1 else 1, fixed_new_tokens=3, return_no_speech_prob=True)
            for b in range(B):
                assert abs(res[b].no_speech_prob - want) <= 1e-3 and res[b].no_speech_prob > 0.0, (sot, B, b, res[b].no_speech_prob, want)


def test_timestamp_prompt_behind_an_initial_prompt(rigs, mel):
    """a start sequence without <|notimestamps|> behind 29 prompt tokens: the timestamp rules hold (tests/ts_ref.py's checker)"""
    from ts_ref import grammar_errors
    model, _, _ = rigs(33)
    for beam in (1, 5):
        prompt = [PREV] + [int(t) for t in np.random.default_rng(33).integers(0, 50257, 29)] + [SOT, 50259, 50359]
        assert len(prompt) == 33
        r = model.generate(_feats(mel), [prompt], beam_size=beam, max_length=100)[0]
        ids = r.sequences_ids[0]
        assert ids and ids[0] > NO_TIMESTAMPS and NO_TIMESTAMPS not in ids and grammar_errors(ids) == [], ids


# engine-against-oracle logit error (f16 weights and activations against float32: DESIGN section 4 reports 3.4e-3 max-abs over all text positions at
# large-v2, less at tiny): a draw is compared only when the reference's two best perturbed values are further apart than twice that, over T
ORACLE_LOGIT_NOISE = 4e-3


def test_sampled_decode_behind_a_long_prompt(rigs, mel):
    """sampling_topk = 0, three samples, seeded, at P = 100: every token is tests/sample_ref.py's draw on the ORACLE's teacher-forced logits of its prefix"""
    import sample_ref as S
    from wis_hip import weights as W
    model, ref, memory = rigs(100)
    prompt, seed, T, n, P = _prompt(100, 2), 20240607, 0.7, 3, 100
    res = model.generate(_feats(mel), [prompt], beam_size=1, num_hypotheses=n, sampling_topk=0, sampling_temperature=T, sampling_seed=seed, return_scores=True)[0]
    assert len(res.sequences_ids) == n and len({tuple(s) for s in res.sequences_ids}) > 1
    unit = max(1.0, 1.0 / T)
    checked = skipped = 0
    for j, sample in enumerate(res.sequences_ids):
        assert 1 <= len(sample) <= 224 and np.isfinite(res.scores[j])
        want = list(sample) + ([EOT] if len(sample) < 224 else [])
        rows = ref.decode_logits(np.array([list(prompt) + list(sample)]), torch.as_tensor(memory)[None])[0].float()
        cum, ok = 0.0, True
        for t, tok in enumerate(want):
            lg, tm = S.processed(rows[P - 1 + t:P + t], t, [list(sample[:t])], suppress_ids=W.SUPPRESS_IDS, suppress_begin=W.SUPPRESS_IDS_BEGIN)
            pick, gap, sc = S.draw(lg[0].numpy(), T, -1, lambda idx, t=t, j=j: S.noise_words(idx, t, j, seed))
            cum += sc
            if gap / unit < S.MARGIN + 2 * ORACLE_LOGIT_NOISE or tm < 2 * ORACLE_LOGIT_NOISE:
                skipped += 1
                ok = ok and pick == tok
                if not ok:
                    break          # (a near tie went the other way: what follows is another sample's history)
                continue
            checked += 1
            assert pick == tok, (j, t, pick, tok, gap)
        if ok:      # the score, as tests/test_gpu_sample.py checks it at P = 4: the temperature-scaled log-probabilities, the end token's included, over the token count
            w = cum / len(sample)
            assert abs(res.scores[j] - w) <= 2 * ORACLE_LOGIT_NOISE / T * (len(want) / len(sample)) + 2e-4 * max(1.0, abs(w)), (j, res.scores[j], w)
    print(f"P 100, {n} samples: {checked} draws identical, {skipped} near ties")
    assert checked >= 30 and skipped <= max(1, checked // 5)          # observed on MI355X: 88 draws identical, 0 near ties


_CHILD = r"""
import json, os, sys
import numpy as np
import torch  # noqa: F401
sys.path[:0] = [p for p in sys.argv[1].split(os.pathsep) if p]
from eot_ramp import with_eot_ramp
from wis_hip import ctranslate2 as ct2, weights as W
mel = np.load(sys.argv[2])["mel"].astype(np.float32)
out = {}
for P, beam, i, fixed in json.loads(sys.argv[3]):
    w = with_eot_ramp(W.synthetic_weights("tiny", seed=1234, std=0.02, emb_std=0.06, ln_jitter=0.1), start=P + 2, slope=0.1)
    model = ct2.Whisper("unused", weights=w, arch=W.arch("tiny"), max_batch=2, max_beam=5)
    prompt = [50361] + [int(t) for t in np.random.default_rng(100 * P + i).integers(0, 50257, P - 5)] + [50258, 50259 + 7 * i, 50359, 50363]
    r = model.generate(ct2.StorageView.from_array(np.ascontiguousarray(mel[None])), [prompt], beam_size=beam, fixed_new_tokens=fixed)[0]
    out[f"{P},{beam},{i},{fixed}"] = [r.sequences_ids[0], r.scores[0]]
    model.close()
print("RESULT " + json.dumps(out))
"""


def test_both_self_attention_forms_agree(golden_dir):
    """WIS_SA_LONG=0 runs the step's self-attention as the TREE form of dec_self_attn_kernel (the A/B form and fallback): on searches whose every decision
    the oracle's margin forces - greedy (33, 1), (228, 2), beam 5 (33, 2) - and on a fixed-length one both forms return the same ids.  The switch is read
    once per process: each form runs in a fresh child."""
    import json
    import subprocess
    import sys
    cases = [[33, 1, 1, 0], [228, 1, 2, 0], [33, 5, 2, 0], [228, 5, 0, 8]]
    got = {}
    for form in ("1", "0"):
        env = dict(os.environ, WIS_SA_LONG=form)
        p = subprocess.run([sys.executable, "-c", _CHILD, os.pathsep.join(sys.path), os.path.join(golden_dir, "logmel_3sec.npz"), json.dumps(cases)],
                           env=env, capture_output=True, text=True, timeout=300)
        assert p.returncode == 0, p.stderr[-2000:]
        got[form] = json.loads(next(l for l in p.stdout.splitlines() if l.startswith("RESULT "))[7:])
    for key in got["1"]:
        assert got["1"][key][0] == got["0"][key][0], (key, got["1"][key], got["0"][key])
        assert abs(got["1"][key][1] - got["0"][key][1]) <= 3e-3, (key, got["1"][key], got["0"][key])
