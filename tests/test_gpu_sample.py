"""-m gpu: random sampling and n-best results (include/wis_hip.h: sampling_topk / sampling_temperature / num_hypotheses) against the CPU
statement of the rule, tests/sample_ref.py.

`wis_debug_search_n` runs the sampled tail (logit_stats_kernel's sampling form, sample_step_kernel) on caller-supplied logits tables at
V = 51865; the reference draws from the SAME fp32 rows with the same Philox words, so ids, lengths and finish steps must be IDENTICAL.  A
case is skipped - and counted - only when the reference sees the two best perturbed values of a draw closer than 2e-4 * max(1, 1 / T) (fp32
rounding of x / T, one addition and a <= 2 ulp logf on |g| <= 17), or a timestamp decision closer than 2e-4.  The end-to-end cases run the
tiny synthetic model through `Whisper.generate` and replay every returned sample teacher-forced through `wis_debug_logits`.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import sample_ref as S

pytestmark = pytest.mark.gpu
V, EOT = 51865, 50257
i32p, u64p, u32p, f32p = C.POINTER(C.c_int32), C.POINTER(C.c_uint64), C.POINTER(C.c_uint32), C.POINTER(C.c_float)
E_ARG, E_UNSUPPORTED = -1, -7


@pytest.fixture(scope="module")
def engine():
    from wis_hip import ctranslate2 as ct2, weights as W
    w = W.synthetic_weights("tiny", seed=1234)
    model = ct2.Whisper("unused", weights=w, arch=W.arch("tiny"), max_batch=16, max_beam=8)
    yield model
    model.close()


def _opts(beam=1, max_new=0, topk=0, T=0.0, n=0, length_penalty=1.0, patience=1.0, suppress_blank=True, suppress_default=True, **more):
    from wis_hip import _lib
    o = _lib.GenOpts(0, beam, max_new, length_penalty, patience, int(suppress_blank), int(suppress_default), 0, 0)
    o.sampling_topk, o.sampling_temperature, o.num_hypotheses = topk, T, n
    for k, v in more.items():
        setattr(o, k, v)
    return o


def _search_n(model, table, B, o, seeds=None, noise=None, rc_only=False):
    """wis_debug_search_n -> (ids [B][n] lists, scores [B, n], finish steps [B])"""
    from wis_hip import _lib
    lib = _lib.load()
    steps = table.shape[0]
    n = max(1, o.num_hypotheses)
    max_new = o.max_new_tokens or steps
    ids = np.zeros((B, n, max_new), np.int32); lens = np.zeros((B, n), np.int32); sc = np.zeros((B, n), np.float32); fin = np.zeros(B, np.int32)
    sd = None if seeds is None else np.ascontiguousarray(np.asarray(seeds, np.uint64))
    nz = None if noise is None else np.ascontiguousarray(noise, np.uint32)
    rc = lib.wis_debug_search_n(model._replicas[0].handle, _lib.ptr(table), steps, B, C.byref(o), None if sd is None else sd.ctypes.data_as(u64p),
                                None if nz is None else nz.ctypes.data_as(u32p), ids.ctypes.data_as(i32p), lens.ctypes.data_as(i32p), sc.ctypes.data_as(f32p),
                                fin.ctypes.data_as(i32p), None)
    if rc_only:
        return rc
    _lib.check(rc)
    return [[ids[b, j, :lens[b, j]].tolist() for j in range(n)] for b in range(B)], sc, fin


def _search_1(model, table, B, o):
    from wis_hip import _lib
    steps = table.shape[0]
    max_new = o.max_new_tokens or steps
    ids = np.zeros((B, max_new), np.int32); lens = np.zeros(B, np.int32); sc = np.zeros(B, np.float32); fin = np.zeros(B, np.int32)
    _lib.check(_lib.load().wis_debug_search(model._replicas[0].handle, _lib.ptr(table), steps, B, C.byref(o), ids.ctypes.data_as(i32p), lens.ctypes.data_as(i32p),
                                            sc.ctypes.data_as(f32p), fin.ctypes.data_as(i32p), None))
    return ids, lens, sc, fin


def _random_table(rng, steps, rows_per, B, ramp_lo=0.3, ramp_hi=1.6):
    """tests/test_gpu_search.py's kind: logits N(0, 2^2) and an EOT column that starts ~6 below the row's best and climbs at a per-utterance rate."""
    t = (2.0 * rng.standard_normal((steps, B * rows_per, V), dtype=np.float32))
    top = t.max(axis=2)
    ramp = rng.uniform(ramp_lo, ramp_hi, size=B).astype(np.float32)
    for b in range(B):
        for j in range(rows_per):
            r = b * rows_per + j
            t[:, r, EOT] = top[:, r] - 6.0 + ramp[b] * np.arange(steps, dtype=np.float32) + 1.5 * rng.standard_normal(steps).astype(np.float32)
    return np.ascontiguousarray(t)


def _proc(**kw):
    from wis_hip import weights as W
    return dict(suppress_ids=W.SUPPRESS_IDS, suppress_begin=W.SUPPRESS_IDS_BEGIN, **kw)


def _check_scores(got, want):
    for g, w in zip(got, want):
        if np.isfinite(w):
            assert abs(g - w) <= 2e-4 * max(1.0, abs(w)), (g, w)
        else:
            assert g == w, (g, w)


# ---- 1. wis_debug_search_n against the reference, exactly ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", [0.2, 1.0, 1.7])
@pytest.mark.parametrize("topk", [-1, 2, 16])
@pytest.mark.parametrize("B,n", [(1, 1), (1, 5), (1, 8), (3, 1), (3, 5), (3, 8)])
def test_sampled_search_equals_the_reference(engine, B, n, topk, T):
    steps = 24
    stats = dict(checked=0, skipped=0, draws=0, fins=[])
    rng = np.random.default_rng(1000 * B + 100 * n + 10 * (topk + 1) + int(10 * T))
    table = _random_table(rng, steps, n, B)
    seeds = [int(x) for x in rng.integers(0, 2 ** 63, size=B, dtype=np.uint64)]
    ids, sc, fin = _search_n(engine, table, B, _opts(topk=topk, T=T, n=n), seeds)
    for b in range(B):
        r = S.sampled_search(S.table_fn(table, b, n), n, steps, topk, T, seeds[b], **_proc())
        stats["draws"] += r["draws"]
        if r["min_gap"] < S.MARGIN:
            stats["skipped"] += 1
            continue
        stats["checked"] += 1
        assert ids[b] == r["ids"], (B, n, topk, T, b, ids[b], r["ids"])
        assert fin[b] == r["finish_step"], (b, fin[b], r["finish_step"])
        _check_scores(sc[b], r["scores"])
        stats["fins"].append(int(fin[b]))
    print(f"B {B} n {n} top-k {topk} T {T}: {stats['checked']} utterances identical over {stats['draws']} draws, {stats['skipped']} skipped as near ties; finish steps {stats['fins']}")
    assert stats["checked"] + stats["skipped"] == B and stats["skipped"] <= max(1, stats["checked"] // 5)
    _TALLY["checked"] += stats["checked"]; _TALLY["skipped"] += stats["skipped"]


_TALLY = dict(checked=0, skipped=0)


def test_sampled_search_skips_stay_inside_the_cap():
    """Over all the cases above (the seeds are fixed; the reference alone decides what is skipped)."""
    assert _TALLY["skipped"] <= max(1, _TALLY["checked"] // 5), _TALLY


@pytest.mark.parametrize("topk,kw", [(-1, dict(timestamps=1, max_initial_timestamp_index=50)), (5, dict(timestamps=1, max_initial_timestamp_index=50)),
                                     (-1, dict(repetition_penalty=1.3, no_repeat_ngram_size=2)), (4, dict(repetition_penalty=1.3, no_repeat_ngram_size=2, timestamps=1, max_initial_timestamp_index=50))])
def test_sampled_search_behind_the_other_processors(engine, topk, kw):
    """The sampled tail behind the repetition rules and the timestamp rules: every sample row has its own history."""
    B, n, steps, T = 2, 3, 16, 0.9
    rng = np.random.default_rng(77 + topk + len(kw))
    table = _random_table(rng, steps, n, B)
    table[:, :, S.EOT + 107:] += 3.0          # timestamps likely enough for the pair rules to matter
    seeds = [11, 12]
    ids, sc, fin = _search_n(engine, table, B, _opts(topk=topk, T=T, n=n, **kw), seeds)
    checked = 0
    for b in range(B):
        r = S.sampled_search(S.table_fn(table, b, n), n, steps, topk, T, seeds[b],
                             **_proc(penalty=kw.get("repetition_penalty", 1.0), ngram=kw.get("no_repeat_ngram_size", 0), timestamps=bool(kw.get("timestamps")),
                                     max_init=kw.get("max_initial_timestamp_index", 50)))
        if r["min_gap"] < S.MARGIN or r["ts_margin"] < 2e-4:
            continue
        checked += 1
        assert ids[b] == r["ids"] and fin[b] == r["finish_step"], (b, ids[b], r["ids"])
        _check_scores(sc[b], r["scores"])
    assert checked >= 1


# ---- 2. a supplied noise table: the extreme words --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("topk", [-1, 8])
def test_noise_table_extreme_words(engine, topk):
    """Words 0 (u = 2^-24: the smallest g) and 0xFFFFFFFF (u = 1 - 2^-24: the largest, and what a 24-bit map would turn into +inf) on the row's
    largest and smallest live logits, both ways round: finite scores, the reference's pick."""
    rng = np.random.default_rng(5)
    table = np.ascontiguousarray(2.0 * rng.standard_normal((1, 1, V), dtype=np.float32))
    lg, _ = S.processed(torch.from_numpy(table[0]), 0, [[]], **_proc())
    x = lg[0].numpy()
    live = np.flatnonzero(x > -np.inf)
    hi_, lo_ = int(live[np.argmax(x[live])]), int(live[np.argmin(x[live])])
    for w_hi, w_lo in ((0, 0xFFFFFFFF), (0xFFFFFFFF, 0)):
        noise = rng.integers(0, 2 ** 32, size=(1, 1, V), dtype=np.uint64).astype(np.uint32)
        noise[0, 0, hi_], noise[0, 0, lo_] = w_hi, w_lo
        for T in (1.0, 0.05):
            ids, sc, fin = _search_n(engine, table, 1, _opts(topk=topk, T=T, n=1), [0], noise)
            r = S.sampled_search(S.table_fn(table, 0, 1), 1, 1, topk, T, 0, words_fn=lambda step, j, idx: noise[step, j, idx], **_proc())
            assert np.isfinite(sc[0, 0]) and r["min_gap"] >= S.MARGIN
            assert ids[0] == r["ids"] and len(ids[0][0]) == 1
            _check_scores(sc[0], r["scores"])
    assert np.isfinite(S.gumbel_of_word(np.uint32([0, 0xFFFFFFFF]))).all()


# ---- 3. seeds ----------------------------------------------------------------------------------------------------------------------------------------
def test_seeds_decide_the_samples(engine):
    rng = np.random.default_rng(9)
    steps, n = 12, 4
    table = _random_table(rng, steps, n, 3)
    o = _opts(topk=-1, T=1.0, n=n)
    a = _search_n(engine, table, 3, o, [5, 6, 7])
    b = _search_n(engine, table, 3, o, [5, 6, 7])
    assert a[0] == b[0] and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])           # the same seeds: the same output
    flat = np.zeros((steps, n, V), np.float32)                                                   # a flat row: the noise alone decides
    f1 = _search_n(engine, flat, 1, o, [1])[0]
    f2 = _search_n(engine, flat, 1, o, [2])[0]
    assert f1 != f2 and len({tuple(s) for s in f1[0]}) == n                                      # ... and the n samples of one seed differ too
    # an utterance alone, and with the same seed in slot 2 of a batch of 3: the counter carries the sample index, not the device row
    alone = _search_n(engine, np.ascontiguousarray(table[:, 2 * n:3 * n]), 1, o, [7])
    assert alone[0][0] == a[0][2] and alone[2][0] == a[2][2]
    assert _search_n(engine, table, 3, o, None)[0] == _search_n(engine, table, 3, o, [0, 0, 0])[0]      # no seeds: all 0


# ---- 4. the distribution -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("topk,T", [(-1, 0.8), (3, 1.3)])
def test_sampled_tokens_follow_the_softmax(engine, topk, T):
    toks = np.array([1000, 1001, 20000, 30000, 40000, 50000])
    x = np.array([1.2, 0.4, 0.0, -0.5, 0.9, -1.5], np.float32)
    B, n, calls = 12, 8, 105
    table = np.full((1, B * n, V), -np.inf, np.float32)
    table[0, :, toks] = x[:, None]
    K = np.arange(6) if topk < 0 else np.argsort(-x, kind="stable")[:topk]
    p = np.exp(x[K].astype(np.float64) / T); p /= p.sum()
    got, ref = np.zeros(6, np.int64), np.zeros(6, np.int64)
    o = _opts(topk=topk, T=T, n=n, max_new=1)
    lg = np.full(V, -np.inf, np.float32); lg[toks] = x
    for c in range(calls):
        seeds = [1_000_003 * c + 17 * b + 1 for b in range(B)]
        ids, _, _ = _search_n(engine, table, B, o, seeds)
        for b in range(B):
            for j in range(n):
                got[int(np.flatnonzero(toks == ids[b][j][0])[0])] += 1
                t, _, _ = S.draw(lg, T, topk, lambda idx, b=b, j=j: S.noise_words(idx, 0, j, seeds[b]))
                ref[int(np.flatnonzero(toks == t)[0])] += 1
    assert got.sum() == ref.sum() == B * n * calls >= 10000
    assert got[[i for i in range(6) if i not in K]].sum() == 0
    cg, cr = S.chi_square(got[K], p), S.chi_square(ref[K], p)
    print(f"top-k {topk} T {T}: counts {got[K].tolist()} (reference {ref[K].tolist()}), chi-square {cg:.2f} (reference {cr:.2f}) against {S.CHI2_1E4[len(K) - 1]}")
    assert cr < S.CHI2_1E4[len(K) - 1] and cg < S.CHI2_1E4[len(K) - 1]


# ---- 5. off is off -----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("beam", [1, 5])
def test_off_is_off(engine, beam):
    rng = np.random.default_rng(31 + beam)
    table = _random_table(rng, 14, beam, 2)
    base = _search_1(engine, table, 2, _opts(beam=beam))
    for kw in (dict(), dict(topk=0, T=0.0, n=0), dict(topk=1), dict(topk=1, T=1.0, n=1)):
        r = _search_1(engine, table, 2, _opts(beam=beam, **kw))
        assert all(np.array_equal(a, b) for a, b in zip(base, r)), kw
        ids, sc, fin = _search_n(engine, table, 2, _opts(beam=beam, **kw))
        assert [s[0] for s in ids] == [base[0][b, :base[1][b]].tolist() for b in range(2)] and np.array_equal(sc[:, 0], base[2]) and np.array_equal(fin, base[3])


# ---- 7. n-best of a beam search ----------------------------------------------------------------------------------------------------------------------------
def _oracle_nbest(table, b, beam, n, lp):
    from oracle.whisper_ref import WhisperRef
    from wis_hip import weights as W
    tt = torch.from_numpy(table)

    def fn(step, last, origin):
        rows = tt[step, b * beam:(b + 1) * beam] if step > 0 else tt[0, b * beam].expand(beam, -1)
        return WhisperRef.apply_processors(rows, step, W.SUPPRESS_IDS, W.SUPPRESS_IDS_BEGIN, True, 0, EOT)
    r = WhisperRef.search(fn, beam, V, EOT, table.shape[0], lp, 1.0)

    def norm(h):
        s, toks = h
        if lp == 0:
            return s
        den = float(len(toks)) ** lp
        return s / den if den != 0 else float("-inf")
    sc = [norm(h) for h in r["hyps"]]
    order = sorted(range(len(sc)), key=lambda i: (-sc[i], i))[:n]          # best first, the first registered among equal scores
    gaps = [sc[order[i]] - sc[order[i + 1]] for i in range(len(order) - 1)]
    if len(sc) > n:
        gaps.append(sc[order[-1]] - max(sc[i] for i in range(len(sc)) if i not in order))
    decisions = r["trace"][:-1] if len(sc) > 1 else r["trace"]          # (the search appends its own best-of ranking gap behind the steps' margins)
    return r, [r["hyps"][i][1] for i in order], [sc[i] for i in order], min(gaps + list(decisions))


@pytest.mark.parametrize("n,lp", [(2, 1.0), (5, 1.0), (5, 0.0)])
def test_n_best_of_a_beam_search(engine, n, lp, monkeypatch):
    """The n best finished hypotheses by normalised score, best first.  length_penalty 0 (CTranslate2's early exit): the search needs n finished
    hypotheses behind a finished top candidate - at n = beam the oracle's "max_candidates" rule."""
    import oracle.whisper_ref as WR
    beam, B, steps = 5, 3, 18
    if lp == 0.0:
        assert n == beam
        monkeypatch.setattr(WR, "EARLY_EXIT_NEEDS", "max_candidates")
    checked = 0
    for case in range(3):
        rng = np.random.default_rng(400 + 10 * n + case)
        table = _random_table(rng, steps, beam, B)
        ids, sc, fin = _search_n(engine, table, B, _opts(beam=beam, n=n, length_penalty=lp))
        for b in range(B):
            r, want_ids, want_sc, margin = _oracle_nbest(table, b, beam, n, lp)
            if margin < 2e-4:
                continue
            checked += 1
            assert fin[b] == r["finish_step"], (b, fin[b], r["finish_step"])
            assert ids[b] == want_ids, (b, ids[b], want_ids)
            _check_scores(sc[b], want_sc)
    assert checked >= 5


# ---- 8. errors -----------------------------------------------------------------------------------------------------------------------------------------------
def test_bad_options_are_refused_and_enqueue_nothing(engine):
    from wis_hip import _lib
    rng = np.random.default_rng(3)
    table = _random_table(rng, 10, 2, 1)
    good = _search_1(engine, table[:, :1].copy(), 1, _opts())
    for o, want in ((_opts(topk=17), E_UNSUPPORTED), (_opts(topk=-2), E_ARG), (_opts(topk=-1, T=-0.5), E_ARG), (_opts(topk=-1, T=float("nan")), E_ARG),
                    (_opts(topk=-1, T=float("inf")), E_ARG), (_opts(topk=-1, n=9), E_ARG), (_opts(topk=-1, n=-1), E_ARG), (_opts(beam=2, topk=-1), E_ARG),
                    (_opts(beam=2, topk=4, n=2), E_ARG), (_opts(beam=1, n=2), E_ARG), (_opts(beam=2, n=3), E_ARG)):
        assert _search_n(engine, table, 1, o, rc_only=True) == want, (o.beam_size, o.sampling_topk, o.sampling_temperature, o.num_hypotheses)
        again = _search_1(engine, table[:, :1].copy(), 1, _opts())
        assert all(np.array_equal(a, b) for a, b in zip(good, again))
    # the one-hypothesis entry points refuse n > 1; drafted decodes refuse all three options
    lib, h = _lib.load(), engine._replicas[0].handle
    ids = np.zeros((2, 10), np.int32); lens = np.zeros(2, np.int32); sc = np.zeros(2, np.float32)
    assert lib.wis_debug_search(h, _lib.ptr(table), 10, 1, C.byref(_opts(beam=2, n=2)), ids.ctypes.data_as(i32p), lens.ctypes.data_as(i32p), sc.ctypes.data_as(f32p), None, None) == E_ARG
    mel = np.zeros((1, 80, 3000), np.float32)
    prompt = np.array([50258, 50259, 50359, 50363], np.int32)
    draft = np.array([1000, 1001], np.int32); org = np.zeros((2, 2), np.int32); tok = np.full((2, 2), 1000, np.int32)
    acc = C.c_int32(0)
    for kw in (dict(topk=-1), dict(T=0.5), dict(n=2), dict(topk=3, T=0.5, n=2)):
        o = _opts(max_new=8, **kw)
        assert lib.wis_generate_draft(h, _lib.ptr(mel), prompt.ctypes.data_as(i32p), 4, C.byref(o), draft.ctypes.data_as(i32p), 2, ids.ctypes.data_as(i32p),
                                      lens.ctypes.data_as(i32p), sc.ctypes.data_as(f32p), C.byref(acc)) == E_UNSUPPORTED, kw
        o.beam_size = 2
        assert lib.wis_generate_draft_beam(h, _lib.ptr(mel), prompt.ctypes.data_as(i32p), 4, C.byref(o), tok.ctypes.data_as(i32p), org.ctypes.data_as(i32p), 2,
                                           ids.ctypes.data_as(i32p), lens.ctypes.data_as(i32p), sc.ctypes.data_as(f32p), C.byref(acc)) == E_UNSUPPORTED, kw
    assert lib.wis_generate(h, _lib.ptr(mel), 1, prompt.ctypes.data_as(i32p), 4, C.byref(_opts(beam=2, n=2, max_new=8)), ids.ctypes.data_as(i32p),
                            lens.ctypes.data_as(i32p), sc.ctypes.data_as(f32p)) == E_ARG
    again = _search_1(engine, table[:, :1].copy(), 1, _opts())
    assert all(np.array_equal(a, b) for a, b in zip(good, again))


# ---- 3 (the seed is not a captured value) and 6: end to end on tiny, through ctranslate2.Whisper.generate ---------------------------------------------
PROMPT = [50258, 50259, 50359, 50363]
MAX_LENGTH = 48          # max_new = 24
# The teacher-forced rows come from a decoder pass of another shape than the decode steps that drew the tokens: f16 activations summed in another
# order, ~1e-3 in logit between any two batch shapes of the engine (include/wis_hip.h, wis_generate_draft).  A draw is compared only when the
# reference's two best perturbed values are further apart than twice that, over T, on top of the sampler's own margin.
E2E_LOGIT_NOISE = 2e-3


@pytest.fixture(scope="module")
def e2e(golden_dir):
    import os
    from wis_hip import audio, ctranslate2 as ct2, weights as W
    pcm, _ = audio.load_audio(os.path.join(golden_dir, "clips", "3sec.flac"))
    mel = np.ascontiguousarray(audio.log_mel_spectrogram(audio.pad_or_trim(pcm)).numpy()[None])
    model = ct2.Whisper("unused", weights=W.synthetic_weights("tiny", seed=1234), arch=W.arch("tiny"), max_batch=4, max_beam=5)
    yield model, mel
    model.close()


def _teacher_forced(model, mel, seq):
    from wis_hip import _lib
    dec_in = np.ascontiguousarray(np.asarray(seq, np.int32)[None])
    out = np.zeros((1, dec_in.shape[1], V), np.float32)
    _lib.check(_lib.load().wis_debug_logits(model._replicas[0].handle, _lib.ptr(mel), _lib.WIS_IN_MEL_HOST, 1, dec_in.ctypes.data_as(i32p), dec_in.shape[1],
                                            out.ctypes.data_as(f32p)))
    return out[0]


@pytest.mark.parametrize("prompt,kw", [(PROMPT, dict()), (PROMPT[:3], dict()), (PROMPT, dict(repetition_penalty=1.1, no_repeat_ngram_size=3))])
def test_generate_samples_end_to_end(e2e, prompt, kw):
    """Every token of every returned sample is what the reference draws from the teacher-forced logits of its prefix, under the call's seed, the
    sample's index and the step.  With timestamps on (a prompt without <|notimestamps|>) and behind the repetition rules."""
    from wis_hip import ctranslate2 as ct2
    model, mel = e2e
    seed, T, n, P = 20240607, 0.7, 5, len(prompt)
    max_new = min(MAX_LENGTH // 2, MAX_LENGTH - P)
    res = model.generate(ct2.StorageView.from_array(mel), [prompt], beam_size=1, num_hypotheses=n, sampling_topk=0, sampling_temperature=T, sampling_seed=seed,
                         max_length=MAX_LENGTH, return_scores=True, **kw)[0]
    assert len(res.sequences_ids) == n == len(res.scores) and len({tuple(s) for s in res.sequences_ids}) > 1
    ts = len(prompt) == 3
    unit = max(1.0, 1.0 / T)
    checked = skipped = 0
    for j, sample in enumerate(res.sequences_ids):
        assert 1 <= len(sample) <= max_new and np.isfinite(res.scores[j])
        want = list(sample) + ([EOT] if len(sample) < max_new else [])
        rows = _teacher_forced(model, mel, list(prompt) + list(sample))
        cum = 0.0
        ok = True
        for t, tok in enumerate(want):
            lg, tm = S.processed(torch.from_numpy(rows[P - 1 + t:P + t]), t, [list(sample[:t])], **_proc(penalty=kw.get("repetition_penalty", 1.0),
                                 ngram=kw.get("no_repeat_ngram_size", 0), timestamps=ts))
            pick, gap, sc = S.draw(lg[0].numpy(), T, -1, lambda idx, t=t, j=j: S.noise_words(idx, t, j, seed))
            cum += sc
            if gap / unit < S.MARGIN + 2 * E2E_LOGIT_NOISE or tm < 2 * E2E_LOGIT_NOISE:
                skipped += 1
                ok = ok and pick == tok
                continue
            checked += 1
            assert pick == tok, (j, t, pick, tok, gap)
        if ok:      # the score: the temperature-scaled log-probabilities, the end token's included, over the token count (length_penalty 1)
            w = cum / len(sample)      # (every term carries the rows' logit noise over T; the engine's own fp32 sum the usual 2e-4)
            assert abs(res.scores[j] - w) <= 2 * E2E_LOGIT_NOISE / T * (len(want) / len(sample)) + 2e-4 * max(1.0, abs(w)), (j, res.scores[j], w)
    print(f"prompt of {P}, {kw}: {checked} draws identical, {skipped} near ties")
    assert checked >= 60 and skipped <= max(1, checked // 5)
    if ts:
        from ts_ref import grammar_errors
        assert all(grammar_errors(s) == [] for s in res.sequences_ids)


def test_one_step_graph_serves_every_seed(e2e):
    """The seeds live in device memory written at the start of the call: a second call with another seed replays the first call's step graphs and must
    not replay its samples."""
    from wis_hip import ctranslate2 as ct2
    model, mel = e2e
    g = lambda m, **kw: model.generate(ct2.StorageView.from_array(m), [PROMPT] * m.shape[0], beam_size=1, num_hypotheses=3, sampling_topk=0, sampling_temperature=1.0,
                                       max_length=MAX_LENGTH, **kw)
    a = g(mel, sampling_seed=1)[0].sequences_ids
    b = g(mel, sampling_seed=2)[0].sequences_ids
    a2 = g(mel, sampling_seed=1)[0].sequences_ids
    assert a == a2 and a != b
    two = g(np.ascontiguousarray(np.concatenate([mel, mel])), sampling_seed=[2, 1])          # per utterance, whatever its slot
    assert two[0].sequences_ids == b and two[1].sequences_ids == a
    # the n best of a beam search through the same face: best first, the single-result call's answer in front
    one = model.generate(ct2.StorageView.from_array(mel), [PROMPT], beam_size=5, max_length=MAX_LENGTH, return_scores=True)[0]
    nb = model.generate(ct2.StorageView.from_array(mel), [PROMPT], beam_size=5, num_hypotheses=3, max_length=MAX_LENGTH, return_scores=True)[0]
    assert nb.sequences_ids[0] == one.sequences_ids[0] and nb.scores[0] == one.scores[0] and len(nb.sequences_ids) == 3
    assert nb.scores[0] >= nb.scores[1] >= nb.scores[2] and len({tuple(s) for s in nb.sequences_ids}) == 3
    # today's calls are untouched by what ran before them
    assert model.generate(ct2.StorageView.from_array(mel), [PROMPT], beam_size=5, max_length=MAX_LENGTH, return_scores=True)[0].sequences_ids == one.sequences_ids
