"""-m gpu: repetition_penalty and no_repeat_ngram_size in the sampling tail (rep_rules_kernel at the head of it) against the CPU statement
of the two CTranslate2 processors (tests/rep_ref.py) plugged into the oracle's search, BIT-EXACT.

`wis_debug_search` runs the tail on caller-supplied logits tables; `WhisperRef.search` with `rep_ref.RepStepFn` runs over the SAME tables.
Ids, lengths, finish steps and beam ancestry must be identical.  Random tables alone almost never repeat a token, so every utterance has a
small HOT SET of ids that every row raises by 8 to 12 (+ noise): histories repeat, and the rules decide the outcome - which every group
asserts on the reference (on != off in at least half of its checked cases).  A case is skipped - and counted - only when the oracle sees
two different-beam candidates closer than 2e-4 at a decision (tests/test_gpu_search.py's rule, same cap); the seeds were chosen on the CPU
so that the reference alone meets the cap.  Then the options end to end through `ctranslate2.Whisper.generate` on the tiny model."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from rep_ref import RepRaw, RepStepFn, banned_tokens

pytestmark = pytest.mark.gpu
V, EOT = 51865, 50257
MARGIN = 2e-4
WIS_E_ARG, WIS_E_UNSUPPORTED = -1, -7      # include/wis_hip.h
HOT_LO, HOT_HI = 1000, 40000               # hot ids are drawn from here (minus the default suppress list)


@pytest.fixture(scope="module")
def engine():
    from wis_hip import ctranslate2 as ct2, weights as W
    model = ct2.Whisper("unused", weights=W.synthetic_weights("tiny", seed=1234), arch=W.arch("tiny"), max_batch=16, max_beam=8)
    yield model
    model.close()


def _run_engine(model, table, B, beam, p=None, n=None, timestamps=False, max_init=50, max_new=0):
    """table f32 [steps][B*beam][V] -> (ids per utterance, scores, finish steps, parents [steps][B*beam]); p / n None: the fields are never set"""
    from wis_hip import _lib
    lib = _lib.load()
    steps = table.shape[0]
    o = _lib.GenOpts(0, beam, max_new, 1.0, 1.0, 1, 1, 0, 0)
    if timestamps:
        o.timestamps, o.max_initial_timestamp_index = 1, (-1 if max_init is None else max_init)
    if p is not None:
        o.repetition_penalty = p
    if n is not None:
        o.no_repeat_ngram_size = n
    ids = np.zeros((B, max_new or steps), np.int32); lens = np.zeros(B, np.int32); sc = np.zeros(B, np.float32)
    fin = np.zeros(B, np.int32); par = np.full((steps, B * beam), -1, np.int32)
    i32 = C.POINTER(C.c_int32)
    _lib.check(lib.wis_debug_search(model._replicas[0].handle, _lib.ptr(table), steps, B, C.byref(o), ids.ctypes.data_as(i32), lens.ctypes.data_as(i32),
                                    sc.ctypes.data_as(C.POINTER(C.c_float)), fin.ctypes.data_as(i32), par.ctypes.data_as(i32)))
    return [ids[b, :lens[b]].tolist() for b in range(B)], sc, fin, par


def _raw_of(table, b, beam):
    tt = torch.from_numpy(table)
    return lambda step, last, origin: tt[step, b * beam:(b + 1) * beam] if step > 0 else tt[0, b * beam].expand(beam, -1)


def _run_oracle(table, b, beam, p=1.0, n=0, step_cls=RepStepFn):
    from oracle.whisper_ref import WhisperRef
    from wis_hip import weights as W
    fn = step_cls(_raw_of(table, b, beam), beam, W.SUPPRESS_IDS, W.SUPPRESS_IDS_BEGIN, True, 0, p, n)
    return WhisperRef.search(fn, beam, V, EOT, table.shape[0], 1.0, 1.0)


def _hot_table(rng, steps, B, beam, n_hot=6, ramp_lo=0.15, ramp_hi=0.7, eot0=-8.0):
    """tests/test_gpu_search.py's _random_table - logits N(0, 2^2), an EOT column that starts `eot0` below the row's best and climbs at a
    per-utterance rate - with a hot set per utterance: n_hot ids every row of the utterance raises by U(8, 12) (drawn per step, row and id)."""
    from wis_hip import weights as W
    t = 2.0 * rng.standard_normal((steps, B * beam, V), dtype=np.float32)
    pool = np.setdiff1d(np.arange(HOT_LO, HOT_HI), np.asarray(W.SUPPRESS_IDS))
    hot = [np.sort(rng.choice(pool, size=n_hot, replace=False)) for _ in range(B)]
    for b in range(B):
        rows = slice(b * beam, (b + 1) * beam)
        t[:, rows, hot[b]] += rng.uniform(8.0, 12.0, size=(steps, beam, n_hot)).astype(np.float32)
    top = t.max(axis=2)
    ramp = rng.uniform(ramp_lo, ramp_hi, size=B).astype(np.float32)
    for b in range(B):
        for j in range(beam):
            r = b * beam + j
            t[:, r, EOT] = top[:, r] + eot0 + ramp[b] * np.arange(steps, dtype=np.float32) + 1.5 * rng.standard_normal(steps).astype(np.float32)
    return np.ascontiguousarray(t), hot


def _check(got, r, b, beam, ctx):
    ids, sc, fin, par = got
    assert ids[b] == r["ids"], (ctx, ids[b], r["ids"])
    assert fin[b] == r["finish_step"], (ctx, fin[b], r["finish_step"])
    if np.isfinite(r["score"]):
        assert abs(sc[b] - r["score"]) <= 2e-4 * max(1.0, abs(r["score"])), (ctx, sc[b], r["score"])
    else:
        assert sc[b] == r["score"], ctx
    for s, org in enumerate(r["origins"]):      # ancestry: after every step the utterance survives, live beam j continues from KV slot b*beam + origin[j]
        want = [b * beam + (0 if s == 0 else o) for o in org]
        assert par[s, b * beam:(b + 1) * beam].tolist() == want, (ctx, s, par[s, b * beam:(b + 1) * beam].tolist(), want)


def _compare(model, table, B, beam, p, n, stats, ctx=(), off=None):
    """One engine run against the reference, utterance by utterance; counts checked / skipped / cases the option decided.
    off: a dict that keeps the table's plain reference searches (computed once per table and utterance)."""
    got = _run_engine(model, table, B, beam, p, n)
    off = {} if off is None else off
    for b in range(B):
        r = _run_oracle(table, b, beam, p, n)
        if min(r["trace"]) < MARGIN:
            stats["skipped"] += 1
            continue
        stats["checked"] += 1
        if b not in off:
            off[b] = _run_oracle(table, b, beam)
        stats["decided"] += int(off[b]["ids"] != r["ids"] or off[b]["finish_step"] != r["finish_step"])
        stats["finish"].append(int(r["finish_step"]))
        stats["margin"] = min(stats["margin"], min(r["trace"]))
        _check(got, r, b, beam, (ctx, B, beam, p, n, b))
    return got


def _assert_group(stats, what):
    print(f"\n[rep-rules] {what}: {stats['checked']} searches identical to the reference, {stats['skipped']} skipped as fp32 near-ties, "
          f"{stats['decided']} decided by the option; finish steps {stats['finish']}; smallest decision margin {stats['margin']:.2e}")
    assert stats["checked"] >= 4 and stats["skipped"] <= max(1, stats["checked"] // 5), stats
    assert 2 * stats["decided"] >= stats["checked"], stats


def _stats():
    return dict(checked=0, skipped=0, decided=0, finish=[], margin=float("inf"))


OPTIONS = [(1.3, 0), (1.0, 2), (1.2, 3), (0.8, 0)]      # (repetition_penalty, no_repeat_ngram_size)
GRID = {1: (11, 2), 2: (12, 2), 5: (15, 1), 8: (18, 1)}      # beam -> (seed, tables): the oracle's sort over beam x V is what a case costs


@pytest.mark.parametrize("beam", [1, 2, 5, 8])
def test_basic_grid(engine, beam):
    rng = np.random.default_rng(GRID[beam][0])
    stats = _stats()
    for case in range(GRID[beam][1]):
        table, _ = _hot_table(rng, 16, 1, beam)
        off = {}
        for p, n in OPTIONS:
            _compare(engine, table, 1, beam, p, n, stats, case, off)
    _assert_group(stats, f"basic grid, beam {beam}")


class _NoReorder(RepStepFn):
    """The WRONG reference: histories that ignore the beam step's reordering (slot j keeps appending to slot j's own history)."""

    def advance(self, last, origin):
        if origin is not None:
            self.hist = [self.hist[j] + [int(last[j])] for j in range(len(origin))]


ANCESTRY_SEEDS = [21, 22, 23, 24]


def test_histories_follow_the_beam_ancestry(engine):
    """Beam 2: at some step beam 1's successor descends from beam 0 while the two histories differ - the penalty and the bans must be taken from
    the REORDERED history.  Asserted on the reference: such a step exists, and a reference that does not reorder gives another result."""
    stats = _stats()
    crossed = wrong_differs = 0
    for seed in ANCESTRY_SEEDS:
        table, _ = _hot_table(np.random.default_rng(seed), 16, 1, 2)
        r = _run_oracle(table, 0, 2, 1.2, 3)
        crossed += int(any(s > 0 and org[1] == 0 for s, org in enumerate(r["origins"])))
        wrong = _run_oracle(table, 0, 2, 1.2, 3, step_cls=_NoReorder)
        wrong_differs += int(wrong["ids"] != r["ids"])
        _compare(engine, table, 1, 2, 1.2, 3, stats, seed)
    assert crossed >= 3 and wrong_differs >= 2, (crossed, wrong_differs)
    _assert_group(stats, f"ancestry ({crossed} tables cross over, {wrong_differs} would differ without the reordering)")


def test_ragged_batch(engine):
    """B = 3 at beam 5 with different EOT ramps: utterances end at different steps while their rows keep flowing through the batch
    (rep_rules_kernel returns at `done`), and every utterance equals its own single-utterance reference."""
    stats = _stats()
    table, _ = _hot_table(np.random.default_rng(31), 18, 3, 5, ramp_lo=0.15, ramp_hi=1.2)
    off, fins = {}, []
    for p, n in ((1.2, 3), (0.8, 2)):
        got = _compare(engine, table, 3, 5, p, n, stats, (p, n), off)
        fins.append(got[2].tolist())
    assert all(len(set(f)) >= 2 for f in fins), fins
    _assert_group(stats, f"ragged batch, finish steps {fins}")


def test_unigram_leaves_the_hot_set(engine):
    """n = 1 with a hot set of 4 ids and 12 steps (EOT held down): every history token is banned, so the search must leave the hot set."""
    stats = _stats()
    for seed, beam in ((41, 1), (42, 2), (43, 1), (44, 5)):
        table, hot = _hot_table(np.random.default_rng(seed), 12, 1, beam, n_hot=4, ramp_lo=0.0, ramp_hi=0.0, eot0=-30.0)
        r = _run_oracle(table, 0, beam, 1.0, 1)
        assert len(r["ids"]) == 12 and len(set(r["ids"])) == 12, r["ids"]            # never a token twice
        assert set(hot[0].tolist()) <= set(r["ids"]), (hot, r["ids"])                # the hot set was used up, then left
        _compare(engine, table, 1, beam, 1.0, 1, stats, seed)
    _assert_group(stats, "unigram")


def test_full_history(engine):
    """Beam 1, 256 steps, EOT held down, p = 1.5 and n = 2.  Every step's pick is planted far above the noise (no near-ties), a fresh id
    per step except:
      step 253: the token of step 20 is planted again at 40 - penalised to 26.7 it loses to a fresh runner-up at 30;
      step 254: the token of step 10 is planted again, at 70 (46.7 after the penalty: still the pick);
      step 255: the history holds 255 tokens - the longest a search can have - and its LAST token (thread 254 of rep_rules_kernel) equals
                the token of step 10, so the token of step 11 is banned although, planted at 70, it is the row's best after the penalty too;
                the runner-up at 35 is taken."""
    steps = 256
    rng = np.random.default_rng(51)
    table = 2.0 * rng.standard_normal((steps, 1, V), dtype=np.float32)
    table[:, 0, EOT] = -40.0
    plan = [2000 + s for s in range(steps)]
    for s in range(steps):
        table[s, 0, plan[s]] = 40.0
    table[253, 0, plan[253]] = -5.0; table[253, 0, plan[20]] = 40.0; table[253, 0, 1998] = 30.0
    table[254, 0, plan[254]] = -5.0; table[254, 0, plan[10]] = 70.0
    table[255, 0, plan[255]] = -5.0; table[255, 0, plan[11]] = 70.0; table[255, 0, 1999] = 35.0
    want = plan[:253] + [1998, plan[10], 1999]
    on = _run_oracle(table, 0, 1, 1.5, 2)
    assert on["ids"] == want and min(on["trace"]) > 1.0, (on["ids"][250:], min(on["trace"]))
    _check(_run_engine(engine, table, 1, 1, 1.5, 2), on, 0, 1, "full history")
    plain = _run_engine(engine, table, 1, 1)[0][0]
    assert plain == plan[:253] + [plan[20], plan[10], plan[11]], plain[250:]      # without the rules: the planted repeats


TS_SEEDS = [(61, 1, 2), (62, 5, 1), (63, 2, 2)]      # (seed, beam, B)


def _ts_hot_table(rng, steps, B, beam):
    """tests/test_gpu_timestamps.py's table (the timestamp block shifted per row so that the decision goes both ways, tilted towards low timestamps)
    with a hot set of text ids per utterance."""
    from ts_ref import TB
    table, hot = _hot_table(rng, steps, B, beam, ramp_lo=0.3, ramp_hi=1.2, eot0=-7.0)
    table[:, :, TB:] += (4.0 + rng.uniform(-3.0, 3.0, size=(steps, B * beam, 1))).astype(np.float32)
    table[:, :, TB:] -= (0.004 * np.arange(V - TB, dtype=np.float32))[None, None, :]
    return np.ascontiguousarray(table), hot


def _run_ts_oracle(table, b, beam, p, n):
    from oracle.whisper_ref import WhisperRef
    from ts_ref import TsStepFn
    from wis_hip import weights as W
    fn = TsStepFn(RepRaw(_raw_of(table, b, beam), beam, p, n), beam, W.SUPPRESS_IDS, W.SUPPRESS_IDS_BEGIN, True, 0, 50)
    return WhisperRef.search(fn, beam, V, EOT, table.shape[0], 1.0, 1.0), fn


def test_combined_with_timestamps(engine):
    """timestamps = 1 with both options: the reference is ts_ref.TsStepFn over rep_ref.RepRaw - the penalty first, the bans in place before the
    text / timestamp decision.  The seeds keep the timestamp decision's own margin above 2e-4 in the reference (asserted): the only skip rule
    stays the search's."""
    stats = _stats()
    for seed, beam, B in TS_SEEDS:
        table, _ = _ts_hot_table(np.random.default_rng(seed), 20, B, beam)
        got = _run_engine(engine, table, B, beam, 1.2, 3, timestamps=True)
        for b in range(B):
            r, fn = _run_ts_oracle(table, b, beam, 1.2, 3)
            assert min(fn.margins) >= MARGIN, (seed, b, min(fn.margins))
            if min(r["trace"]) < MARGIN:
                stats["skipped"] += 1
                continue
            stats["checked"] += 1
            off, _ = _run_ts_oracle(table, b, beam, 1.0, 0)
            stats["decided"] += int(off["ids"] != r["ids"] or off["finish_step"] != r["finish_step"])
            stats["finish"].append(int(r["finish_step"]))
            stats["margin"] = min(stats["margin"], min(r["trace"]), min(fn.margins))
            _check(got, r, b, beam, ("timestamps", seed, beam, b))
    _assert_group(stats, "combined with timestamps")


def test_off_is_todays_search(engine):
    """p = 1, n = 0 and p = 0, n = 0 (zero means off) give what a call that never sets the fields gives - which is the plain oracle search."""
    table, _ = _hot_table(np.random.default_rng(71), 16, 2, 5)
    plain = _run_engine(engine, table, 2, 5)
    for p, n in ((1.0, 0), (0.0, 0)):
        got = _run_engine(engine, table, 2, 5, p, n)
        assert got[0] == plain[0] and got[2].tolist() == plain[2].tolist() and np.array_equal(got[3], plain[3]) and np.array_equal(got[1], plain[1]), (p, n)
    for b in range(2):
        r = _run_oracle(table, b, 5)
        if min(r["trace"]) >= MARGIN:
            _check(plain, r, b, 5, ("off", b))


def test_argument_checks(engine):
    from wis_hip import _lib
    table = np.zeros((2, 1, V), np.float32)
    for p, n in ((-1.0, 0), (1.0, -1), (float("nan"), 0), (float("inf"), 0)):
        with pytest.raises(_lib.WisError) as e:
            _run_engine(engine, table, 1, 1, p, n)
        assert e.value.code == WIS_E_ARG, (p, n, e.value)


def test_step0_row_is_shared_and_untouched(engine):
    """Step 0 samples every beam from ONE row and both rules are no-ops there; the same table twice in a row gives equal results (nothing of
    the first search - its patched rows, its histories - leaks into the second), and step 0 alone equals the plain search's step 0."""
    table, _ = _hot_table(np.random.default_rng(81), 16, 1, 5)
    a = _run_engine(engine, table, 1, 5, 1.2, 3)
    b = _run_engine(engine, table, 1, 5, 1.2, 3)
    assert a[0] == b[0] and np.array_equal(a[1], b[1]) and a[2].tolist() == b[2].tolist() and np.array_equal(a[3], b[3])
    one = _run_engine(engine, table[:1], 1, 5, 1.2, 3)
    one_plain = _run_engine(engine, table[:1], 1, 5)
    assert one[0] == one_plain[0] and np.array_equal(one[1], one_plain[1])


def test_drafted_calls_refuse_the_options(engine):
    """wis_generate_draft / wis_generate_draft_beam answer WIS_E_UNSUPPORTED (as for timestamps), before anything runs."""
    from wis_hip import _lib
    lib = _lib.load()
    h = engine._replicas[0].handle
    mel = np.zeros((1, 80, 3000), np.float32)
    prompt = np.asarray([50258, 50259, 50359, 50363], np.int32)
    i32 = C.POINTER(C.c_int32)
    ids, ln, sc, acc = np.zeros(224, np.int32), np.zeros(1, np.int32), np.zeros(1, np.float32), C.c_int32(0)
    for p, n in ((1.1, 0), (0.0, 3)):
        o = _lib.GenOpts(0, 1, 0, 1.0, 1.0, 1, 1, 8, 0)
        o.repetition_penalty, o.no_repeat_ngram_size = p, n
        d = np.asarray([400, 401], np.int32)
        rc = lib.wis_generate_draft(h, _lib.ptr(mel), prompt.ctypes.data_as(i32), 4, C.byref(o), d.ctypes.data_as(i32), 2, ids.ctypes.data_as(i32),
                                    ln.ctypes.data_as(i32), sc.ctypes.data_as(C.POINTER(C.c_float)), C.byref(acc))
        assert rc == WIS_E_UNSUPPORTED, rc
        o.beam_size = 2
        dt, do = np.asarray([[400, 401]], np.int32), np.zeros((1, 2), np.int32)
        rc = lib.wis_generate_draft_beam(h, _lib.ptr(mel), prompt.ctypes.data_as(i32), 4, C.byref(o), dt.ctypes.data_as(i32), do.ctypes.data_as(i32), 1,
                                         ids.ctypes.data_as(i32), ln.ctypes.data_as(i32), sc.ctypes.data_as(C.POINTER(C.c_float)), C.byref(acc))
        assert rc == WIS_E_UNSUPPORTED, rc


# ---- end to end: wis_generate through ctranslate2.Whisper.generate, tiny, the 3 s golden clip, 32 tokens --------------------------------
E2E_SEED = 1234
PROMPT = [50258, 50259, 50359, 50363]


def _repeated_bigrams(ids):
    seen, rep = set(), 0
    for a in zip(ids, ids[1:]):
        rep += a in seen
        seen.add(a)
    return rep


@pytest.fixture(scope="module")
def e2e(golden_dir):
    from wis_hip import audio, ctranslate2 as ct2, weights as W
    pcm, _ = audio.load_audio(os.path.join(golden_dir, "clips", "3sec.flac"))
    mel = np.ascontiguousarray(audio.log_mel_spectrogram(audio.pad_or_trim(pcm)).numpy()[None])
    model = ct2.Whisper("unused", weights=W.synthetic_weights("tiny", seed=E2E_SEED), arch=W.arch("tiny"), max_batch=4, max_beam=5)
    yield model, mel
    model.close()


def _gen(model, mel, beam, prompt=PROMPT, **kw):
    from wis_hip import ctranslate2 as ct2
    B = mel.shape[0]
    return [r.sequences_ids[0] for r in model.generate(ct2.StorageView.from_array(mel), [prompt] * B, beam_size=beam, fixed_new_tokens=32, **kw)]


@pytest.mark.parametrize("beam", [1, 5])
def test_generate_end_to_end(e2e, beam):
    model, mel = e2e
    plain = _gen(model, mel, beam)[0]
    assert len(plain) == 32
    assert _gen(model, mel, beam, repetition_penalty=1, no_repeat_ngram_size=0)[0] == plain         # the defaults, passed: the same call
    assert _repeated_bigrams(plain) > 0, plain                                                     # precondition: the plain decode loops
    nb = _gen(model, mel, beam, no_repeat_ngram_size=2)[0]
    assert len(nb) == 32 and _repeated_bigrams(nb) == 0, nb
    for t in range(2, 32):                                                                         # ... token by token: never a banned one
        assert nb[t] not in banned_tokens(nb[:t], 2), (t, nb)
    pen = _gen(model, mel, beam, repetition_penalty=1.5)[0]
    assert len(pen) == 32 and pen != plain, (pen, plain)
    both = _gen(model, mel, beam, repetition_penalty=1.1, no_repeat_ngram_size=3)[0]
    assert len(both) == 32
    for t in range(3, 32):
        assert both[t] not in banned_tokens(both[:t], 3), (t, both)
    # two utterances in one call: each is what it is alone
    two = _gen(model, np.ascontiguousarray(np.concatenate([mel, mel])), beam, no_repeat_ngram_size=2)
    assert two[0] == nb and two[1] == nb, (two, nb)
    print(f"\n[rep-rules] e2e beam {beam}: plain has {_repeated_bigrams(plain)} repeated bigrams; n = 2 none; p = 1.5 changes "
          f"{sum(a != b for a, b in zip(pen, plain))} of 32 tokens")


def test_generate_timestamped_prompt_with_ngrams(e2e):
    from ts_ref import grammar_errors
    from wis_hip import whisper
    model, mel = e2e
    ids = _gen(model, mel, 5, prompt=PROMPT[:3], no_repeat_ngram_size=3)[0]
    assert len(ids) == 32 and grammar_errors(ids) == [], ids
    segs = whisper.segments_from_tokens(ids, whisper._Tokenizer(None), special=model.special)      # (seeded weights: timestamps anywhere in the 30 s window)
    assert segs and all(s["end"] >= s["start"] >= 0.0 and isinstance(s["text"], str) for s in segs), segs


def test_generate_refuses_drafts_and_keeps_its_refusals(e2e):
    from wis_hip import ctranslate2 as ct2
    model, mel = e2e
    f = ct2.StorageView.from_array(mel)
    for kw in (dict(repetition_penalty=1.1), dict(no_repeat_ngram_size=3)):
        with pytest.raises(ValueError):
            model.generate(f, [PROMPT], beam_size=1, draft_tokens=[400, 401], **kw)
        with pytest.raises(ValueError):
            model.generate(f, [PROMPT], beam_size=2, draft_trajectory=(np.asarray([[400, 401]], np.int32), np.zeros((1, 2), np.int32)), **kw)
    for kw in (dict(repetition_penalty=-1), dict(repetition_penalty=float("nan")), dict(no_repeat_ngram_size=-1)):
        with pytest.raises(ValueError):
            model.generate(f, [PROMPT], beam_size=1, **kw)
    for kw in (dict(sampling_topk=5), dict(num_hypotheses=2)):
        with pytest.raises(NotImplementedError):
            model.generate(f, [PROMPT], beam_size=1, **kw)
