"""-m gpu: hotword boosting in the sampling tail (hotword_rules_kernel behind rep_rules_kernel) against the CPU statement of THE HOTWORD RULE
(tests/hotword_ref.py: a brute force over the history's suffixes) plugged into the oracle's search, EXACTLY.

`wis_debug_search` / `wis_debug_search_n` run the tail on caller-supplied logits tables; `WhisperRef.search` over `hotword_ref.HotwordStepFn` runs
over the SAME tables.  Ids, lengths, finish steps and beam ancestry must be identical, scores within the search tests' 2e-4.  Random tables alone
almost never walk into a hotword entry, so every utterance has a small HOT ALPHABET of ids that every row raises by 8 to 12 (+ noise) and the
entries are words over that alphabet: the beams' histories run through the trie at different depths, they reorder at nearly every step, and the
boost decides the outcome - each group asserts that on the reference.  A case is skipped - and counted - only when the oracle sees a decision
margin below 2e-4 (tests/test_gpu_search.py's rule, same cap); the seeds were chosen on the CPU so that the reference alone meets the cap."""
import ctypes as C

import numpy as np
import pytest
import torch

import sample_ref as S
from hotword_ref import HotwordRaw, HotwordStepFn, PerSlotHotwordRaw, SampledHotwordRaw, boost_set
from phrase_ref import prefix_dict
from rep_ref import RepRaw, RepStepFn

pytestmark = pytest.mark.gpu
V, EOT = 51865, 50257
MARGIN = 2e-4
WIS_E_ARG, WIS_E_STATE, WIS_E_UNSUPPORTED = -1, -6, -7      # include/wis_hip.h
HOT_LO, HOT_HI = 1000, 40000
i32p, f32p, u64p, u32p = C.POINTER(C.c_int32), C.POINTER(C.c_float), C.POINTER(C.c_uint64), C.POINTER(C.c_uint32)


@pytest.fixture(scope="module")
def engine():
    from wis_hip import ctranslate2 as ct2, weights as W
    model = ct2.Whisper("unused", weights=W.synthetic_weights("tiny", seed=1234), arch=W.arch("tiny"), max_batch=16, max_beam=8)
    yield model
    model.close()


def _set_trie(model, trie):
    from wis_hip import _lib
    trie = np.ascontiguousarray(np.asarray(trie, np.int32).reshape(-1, 4))
    return _lib.load().wis_model_set_hotwords(model._replicas[0].handle, trie.ctypes.data_as(i32p), len(trie))


def _install(model, entries):
    from wis_hip import _lib, weights as W
    _lib.check(_set_trie(model, W.build_hotword_trie(entries)))


def _opts(beam, boost=None, **fields):
    """boost None: the struct a caller that never knew the two fields builds (GenOpts); else the full struct with hotwords = 1"""
    from wis_hip import _lib
    o = (_lib.GenOpts if boost is None and not any(k.startswith("hotword") for k in fields) else _lib.HotGenOpts)(0, beam, 0, 1.0, 1.0, 1, 1, 0, 0)
    if boost is not None:
        o.hotwords, o.hotword_boost = 1, boost
    for k, v in fields.items():
        setattr(o, k, v)
    return o


def _run_engine(model, table, B, beam, boost=None, rc_only=False, **fields):
    """table f32 [steps][B*beam][V] -> (ids per utterance, scores, finish steps, parents [steps][B*beam])"""
    from wis_hip import _lib
    steps = table.shape[0]
    o = _opts(beam, boost, **fields)
    ids = np.zeros((B, o.max_new_tokens or steps), np.int32); lens = np.zeros(B, np.int32); sc = np.zeros(B, np.float32)
    fin = np.zeros(B, np.int32); par = np.full((steps, B * beam), -1, np.int32)
    rc = _lib.load().wis_debug_search(model._replicas[0].handle, _lib.ptr(table), steps, B, C.byref(o), ids.ctypes.data_as(i32p), lens.ctypes.data_as(i32p),
                                      sc.ctypes.data_as(f32p), fin.ctypes.data_as(i32p), par.ctypes.data_as(i32p))
    if rc_only:
        return rc
    _lib.check(rc)
    return [ids[b, :lens[b]].tolist() for b in range(B)], sc, fin, par


def _run_engine_n(model, table, B, o, seeds=None, noise=None):
    """wis_debug_search_n -> (ids [B][n] lists, scores [B, n], finish steps [B])"""
    from wis_hip import _lib
    steps, n = table.shape[0], max(1, o.num_hypotheses)
    ids = np.zeros((B, n, steps), np.int32); lens = np.zeros((B, n), np.int32); sc = np.zeros((B, n), np.float32); fin = np.zeros(B, np.int32)
    sd = None if seeds is None else np.ascontiguousarray(np.asarray(seeds, np.uint64))
    nz = None if noise is None else np.ascontiguousarray(noise, np.uint32)
    _lib.check(_lib.load().wis_debug_search_n(model._replicas[0].handle, _lib.ptr(table), steps, B, C.byref(o), None if sd is None else sd.ctypes.data_as(u64p),
                                              None if nz is None else nz.ctypes.data_as(u32p), ids.ctypes.data_as(i32p), lens.ctypes.data_as(i32p),
                                              sc.ctypes.data_as(f32p), fin.ctypes.data_as(i32p), None))
    return [[ids[b, j, :lens[b, j]].tolist() for j in range(n)] for b in range(B)], sc, fin


def _raw_of(table, b, beam):
    tt = torch.from_numpy(table)
    return lambda step, last, origin: tt[step, b * beam:(b + 1) * beam] if step > 0 else tt[0, b * beam].expand(beam, -1)


def _run_oracle(table, b, beam, entries, boost, p=1.0, n=0, raw_cls=HotwordRaw, lp=1.0):
    """-> (the reference search over the boosted rows, its step function); p / n: the repetition rules in front (rep_ref.RepRaw);
    entries None: the plain search"""
    from oracle.whisper_ref import WhisperRef
    from wis_hip import weights as W
    raw = _raw_of(table, b, beam)
    if entries is None:
        fn = RepStepFn(raw, beam, W.SUPPRESS_IDS, W.SUPPRESS_IDS_BEGIN, True, 0, p, n)
        return WhisperRef.search(fn, beam, V, EOT, table.shape[0], lp, 1.0), fn
    if p != 1.0 or n != 0:
        raw = RepRaw(raw, beam, p, n)
    fn = HotwordStepFn(raw, beam, W.SUPPRESS_IDS, W.SUPPRESS_IDS_BEGIN, prefix_dict(entries), boost, V)
    if raw_cls is not HotwordRaw:
        fn.boosted = raw_cls(raw, beam, prefix_dict(entries), boost, V)
    fn.seen, advance = [], fn.boosted.advance      # the beams' histories at every step, for _note_shape

    def recording(last, origin):
        advance(last, origin)
        fn.seen.append([list(h) for h in fn.boosted.hist])
    fn.boosted.advance = recording
    return WhisperRef.search(fn, beam, V, EOT, table.shape[0], lp, 1.0), fn


def _hot_table(rng, steps, B, beam, n_hot=5, ramp_lo=0.15, ramp_hi=0.7, eot0=-8.0):
    """tests/test_gpu_rep_rules.py's table: logits N(0, 2^2), an EOT column that starts `eot0` below the row's best and climbs at a per-utterance
    rate, and a hot alphabet per utterance - n_hot ids every row of the utterance raises by U(8, 12) (drawn per step, row and id)."""
    from wis_hip import weights as W
    t = 2.0 * rng.standard_normal((steps, B * beam, V), dtype=np.float32)
    pool = np.setdiff1d(np.arange(HOT_LO, HOT_HI), np.asarray(list(W.SUPPRESS_IDS) + list(W.SUPPRESS_IDS_BEGIN)))
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


def _entries(rng, hot, n=10, lo=2, hi=5):
    """words over the utterances' hot alphabets, some self-overlapping ([a, a, b]), some prefixes of others; one set for the whole batch"""
    out = []
    for h in hot:
        h = [int(t) for t in h]
        out += [[h[0], h[0], h[1]], [h[0], h[1]], [h[0], h[1], h[2]], [h[2]]]
        out += [rng.choice(h, size=int(rng.integers(lo, hi + 1))).tolist() for _ in range(n)]
    return [[int(t) for t in e] for e in out]


def _check(got, r, b, beam, ctx):
    ids, sc, fin, par = got
    assert ids[b] == r["ids"], (ctx, ids[b], r["ids"])
    assert fin[b] == r["finish_step"], (ctx, fin[b], r["finish_step"])
    if np.isfinite(r["score"]):
        assert abs(sc[b] - r["score"]) <= 2e-4 * max(1.0, abs(r["score"])), (ctx, sc[b], r["score"])
    else:
        assert sc[b] == r["score"], ctx
    for s, org in enumerate(r["origins"]):      # ancestry: after every step the utterance survives, live beam j continues from slot b*beam + origin[j]
        want = [b * beam + (0 if s == 0 else o) for o in org]
        assert par[s, b * beam:(b + 1) * beam].tolist() == want, (ctx, s, par[s, b * beam:(b + 1) * beam].tolist(), want)


def _stats():
    return dict(checked=0, skipped=0, decided=0, reordered=0, depths=0, finish=[], margin=float("inf"))


def _note_shape(stats, r, fn, entries):
    """on the reference: steps whose beams do not continue slot for slot, and steps at which sibling beams sit at different trie depths"""
    pre = prefix_dict(entries)
    stats["reordered"] += sum(1 for s, org in enumerate(r["origins"]) if s > 0 and org != list(range(len(org))))
    for hists in fn.seen:
        depth = {max(k for k in range(min(len(h), 31) + 1) if tuple(h[len(h) - k:]) in pre) for h in hists}
        stats["depths"] += int(len(depth) > 1)


def _compare(model, table, B, beam, entries, boost, stats, ctx=(), p=None, n=None, off=None):
    fields = {}
    if p is not None:
        fields["repetition_penalty"] = p
    if n is not None:
        fields["no_repeat_ngram_size"] = n
    got = _run_engine(model, table, B, beam, boost, **fields)
    off = {} if off is None else off
    for b in range(B):
        r, fn = _run_oracle(table, b, beam, entries, boost, 1.0 if p is None else p, 0 if n is None else n)
        if min(r["trace"]) < MARGIN:
            stats["skipped"] += 1
            continue
        stats["checked"] += 1
        if b not in off:
            off[b] = _run_oracle(table, b, beam, None, 0.0, 1.0 if p is None else p, 0 if n is None else n)[0]
        stats["decided"] += int(off[b]["ids"] != r["ids"] or off[b]["finish_step"] != r["finish_step"])
        stats["finish"].append(int(r["finish_step"]))
        stats["margin"] = min(stats["margin"], min(r["trace"]))
        _note_shape(stats, r, fn, entries)
        _check(got, r, b, beam, (ctx, B, beam, boost, p, n, b))
    return got


def _assert_group(stats, what, decided=True):
    print(f"\n[hotwords] {what}: {stats['checked']} searches identical to the reference, {stats['skipped']} skipped as fp32 near-ties, "
          f"{stats['decided']} decided by the boost, {stats['reordered']} reordering steps, {stats['depths']} steps with beams at different depths; "
          f"finish steps {stats['finish']}; smallest decision margin {stats['margin']:.2e}")
    assert stats["checked"] >= 4 and stats["skipped"] <= max(1, stats["checked"] // 5), stats
    if decided:
        assert 2 * stats["decided"] >= stats["checked"], stats


GRID = {1: (111, 3), 5: (115, 2), 8: (118, 2)}      # beam -> (seed, tables)


@pytest.mark.parametrize("beam", [1, 5, 8])
def test_basic_grid(engine, beam):
    rng = np.random.default_rng(GRID[beam][0])
    stats = _stats()
    for case in range(GRID[beam][1]):
        table, hot = _hot_table(rng, 16, 1, beam)
        entries = _entries(rng, hot)
        _install(engine, entries)
        off = {}
        for boost in (3.0, 6.5):
            _compare(engine, table, 1, beam, entries, boost, stats, case, off=off)
    if beam > 1:
        assert stats["reordered"] >= stats["checked"] and stats["depths"] >= stats["checked"], stats      # (several such steps per search)
    _assert_group(stats, f"basic grid, beam {beam}")


def _planted_crossing(rng):
    """Beam 2, four steps, one entry [a, b, c].  Step 0 leaves the beams [d] and [a]; at step 1 they CROSS - [a, b] from slot 1 becomes beam 0, [d, b]
    from slot 0 beam 1 - so at step 2 row 0 belongs to the history [a, b] (c is boosted: 8 + 4 beats x at 10) and row 1 to [d, b] (nothing beyond the
    root).  A kernel that kept its state per slot would hold [d, b] for row 0 and pick x.  Every decision is planted at least 0.1 apart."""
    from wis_hip import weights as W
    pool = np.setdiff1d(np.arange(HOT_LO, HOT_HI), np.asarray(list(W.SUPPRESS_IDS) + list(W.SUPPRESS_IDS_BEGIN)))
    a, b, c, d, x, y, z = (int(t) for t in rng.choice(pool, size=7, replace=False))
    t = 0.3 * rng.standard_normal((4, 2, V), dtype=np.float32)
    t[:3, :, EOT] = -30.0
    t[0, 0, a], t[0, 0, d] = 20.0, 24.2                      # a: 24 with the boost, d: 24.2
    t[1, 0, b], t[1, 0, y] = 14.0, 13.5                      # behind [d]: b and y share the row
    t[1, 1, b] = 10.0                                        # behind [a]: b alone, boosted to 14
    t[2, 0, c], t[2, 0, x] = 8.0, 10.0                       # behind [a, b] after the crossing
    t[2, 1, z], t[2, 1, c] = 10.0, -5.0
    t[3, :, EOT] = 30.0
    return np.ascontiguousarray(t), [[a, b, c]], dict(a=a, b=b, c=c, d=d, x=x, z=z)


def test_state_kept_per_slot_would_differ(engine):
    """The boost set must be taken from the REORDERED history.  Asserted on the reference: the beams cross, and a reference that keeps its
    histories per slot gives another answer."""
    table, entries, t = _planted_crossing(np.random.default_rng(121))
    r, fn = _run_oracle(table, 0, 2, entries, 4.0)
    wrong, _ = _run_oracle(table, 0, 2, entries, 4.0, raw_cls=PerSlotHotwordRaw)
    plain, _ = _run_oracle(table, 0, 2, None, 0.0)
    assert r["origins"][1] == [1, 0] and min(r["trace"]) > 0.05, (r["origins"], r["trace"])
    assert r["ids"] == [t["a"], t["b"], t["c"]] and wrong["ids"] == [t["a"], t["b"], t["x"]] and plain["ids"] != r["ids"], (r["ids"], wrong["ids"], plain["ids"])
    _install(engine, entries)
    _check(_run_engine(engine, table, 1, 2, 4.0), r, 0, 2, "planted crossing")
    _check(_run_engine(engine, table, 1, 2), plain, 0, 2, "planted crossing, off")


def test_ragged_batch(engine):
    """B = 8 at beam 5 with different EOT ramps: the utterances end at different steps while their rows keep flowing through the batch (the
    kernel returns at `done`), and every utterance equals its own single-utterance reference."""
    stats = _stats()
    rng = np.random.default_rng(131)
    table, hot = _hot_table(rng, 18, 8, 5, ramp_lo=0.15, ramp_hi=1.4)
    entries = _entries(rng, hot, n=4)
    _install(engine, entries)
    got = _compare(engine, table, 8, 5, entries, 4.0, stats, "ragged")
    assert len(set(got[2].tolist())) >= 3, got[2]
    _assert_group(stats, f"ragged batch of 8, finish steps {got[2].tolist()}")


def test_combined_with_the_repetition_rules(engine):
    """repetition_penalty + no_repeat_ngram_size in front of the boost (the reference: HotwordStepFn over rep_ref.RepRaw).  A banned hot token
    stays banned: with n = 1 every history token is banned however much it is boosted, so no result holds a token twice - and the boost set did
    name banned tokens (asserted on the reference)."""
    stats = _stats()
    for seed, beam in ((141, 1), (142, 5)):
        rng = np.random.default_rng(seed)
        table, hot = _hot_table(rng, 14, 1, beam)
        entries = _entries(rng, hot)
        _install(engine, entries)
        for p, n in ((1.2, 3), (1.5, 0)):
            _compare(engine, table, 1, beam, entries, 5.0, stats, (seed, p, n), p=p, n=n)
    _assert_group(stats, "combined with the repetition rules", decided=False)
    banned_and_boosted = 0
    stats = _stats()
    for seed, beam in ((143, 1), (144, 2), (145, 5), (146, 1)):
        rng = np.random.default_rng(seed)
        table, hot = _hot_table(rng, 10, 1, beam, n_hot=4, ramp_lo=0.0, ramp_hi=0.0, eot0=-30.0)
        entries = _entries(rng, hot)
        _install(engine, entries)
        r, fn = _run_oracle(table, 0, beam, entries, 9.0, 1.0, 1)
        assert len(r["ids"]) == 10 and len(set(r["ids"])) == 10, r["ids"]            # never a token twice, whatever the boost
        pre = prefix_dict(entries)
        banned_and_boosted += sum(1 for i in range(1, 10) if set(boost_set(pre, r["ids"][:i], V)) & set(r["ids"][:i]))
        _compare(engine, table, 1, beam, entries, 9.0, stats, seed, p=1.0, n=1)
    assert banned_and_boosted >= 8, banned_and_boosted
    _assert_group(stats, f"unigram bans over boosted tokens ({banned_and_boosted} steps had a banned token in the boost set)", decided=False)


def _ts_hot_table(rng, steps, B, beam):
    """tests/test_gpu_rep_rules.py's timestamp table: the timestamp block shifted per row so that the text / timestamp decision goes both ways"""
    from ts_ref import TB
    table, hot = _hot_table(rng, steps, B, beam, ramp_lo=0.3, ramp_hi=1.2, eot0=-7.0)
    table[:, :, TB:] += (4.0 + rng.uniform(-3.0, 3.0, size=(steps, B * beam, 1))).astype(np.float32)
    table[:, :, TB:] -= (0.004 * np.arange(V - TB, dtype=np.float32))[None, None, :]
    return np.ascontiguousarray(table), hot


def _run_ts_oracle(table, b, beam, entries, boost):
    from oracle.whisper_ref import WhisperRef
    from ts_ref import TsStepFn
    from wis_hip import weights as W
    raw = _raw_of(table, b, beam)
    if entries is not None:
        raw = HotwordRaw(raw, beam, prefix_dict(entries), boost, V)
    fn = TsStepFn(raw, beam, W.SUPPRESS_IDS, W.SUPPRESS_IDS_BEGIN, True, 0, 50)
    return WhisperRef.search(fn, beam, V, EOT, table.shape[0], 1.0, 1.0), fn


def test_combined_with_timestamps(engine):
    """timestamps = 1: the reference is ts_ref.TsStepFn over HotwordRaw - the text / timestamp decision sees boosted values.  The seeds keep the
    timestamp decision's own margin above 2e-4 in the reference (asserted)."""
    stats = _stats()
    for seed, beam, B in ((151, 1, 2), (152, 5, 1), (153, 2, 2)):
        rng = np.random.default_rng(seed)
        table, hot = _ts_hot_table(rng, 18, B, beam)
        entries = _entries(rng, hot)
        _install(engine, entries)
        got = _run_engine(engine, table, B, beam, 5.0, timestamps=1, max_initial_timestamp_index=50)
        for b in range(B):
            r, fn = _run_ts_oracle(table, b, beam, entries, 5.0)
            assert min(fn.margins) >= MARGIN, (seed, b, min(fn.margins))
            if min(r["trace"]) < MARGIN:
                stats["skipped"] += 1
                continue
            stats["checked"] += 1
            off, _ = _run_ts_oracle(table, b, beam, None, 0.0)
            stats["decided"] += int(off["ids"] != r["ids"] or off["finish_step"] != r["finish_step"])
            stats["finish"].append(int(r["finish_step"]))
            stats["margin"] = min(stats["margin"], min(r["trace"]), min(fn.margins))
            _check(got, r, b, beam, ("timestamps", seed, beam, b))
    _assert_group(stats, "combined with timestamps")


def test_combined_with_num_hypotheses(engine):
    """wis_debug_search_n, beam 5, the 3 best finished hypotheses of the boosted search, best first"""
    beam, B, n = 5, 2, 3
    checked = 0
    for seed in (161, 163):
        rng = np.random.default_rng(seed)
        table, hot = _hot_table(rng, 16, B, beam, ramp_lo=0.4, ramp_hi=1.2)
        entries = _entries(rng, hot)
        _install(engine, entries)
        ids, sc, fin = _run_engine_n(engine, table, B, _opts(beam, 4.0, num_hypotheses=n))
        for b in range(B):
            r, _ = _run_oracle(table, b, beam, entries, 4.0)
            norm = [s / float(len(t)) if len(t) else float("-inf") for s, t in r["hyps"]]
            order = sorted(range(len(norm)), key=lambda i: (-norm[i], i))[:n]
            gaps = [norm[order[i]] - norm[order[i + 1]] for i in range(len(order) - 1)]
            if len(norm) > n:
                gaps.append(norm[order[-1]] - max(norm[i] for i in range(len(norm)) if i not in order))
            decisions = r["trace"][:-1] if len(norm) > 1 else r["trace"]
            if min(gaps + list(decisions)) < MARGIN:
                continue
            checked += 1
            assert fin[b] == r["finish_step"] and ids[b] == [r["hyps"][i][1] for i in order], (seed, b, ids[b])
            for g, w in zip(sc[b], [norm[i] for i in order]):
                assert abs(g - w) <= 2e-4 * max(1.0, abs(w)), (g, w)
    assert checked >= 4, checked


@pytest.mark.parametrize("topk", [-1, 4])
def test_combined_with_sampling(engine, topk):
    """The sampled form with fixed seeds, and with the `noise` input in place of the Philox words: every sample's row has its own history, the
    boost patches the row before logit_stats_kernel's sampling form reads it."""
    B, n, steps, T = 2, 3, 14, 0.8
    rng = np.random.default_rng(171 + topk)
    table, hot = _hot_table(rng, steps, B, n, ramp_lo=0.4, ramp_hi=1.0)
    entries = _entries(rng, hot)
    _install(engine, entries)
    from wis_hip import weights as W
    proc = dict(suppress_ids=W.SUPPRESS_IDS, suppress_begin=W.SUPPRESS_IDS_BEGIN)
    seeds = [21, 22]
    noise = rng.integers(0, 2 ** 32, size=(steps, B * n, V), dtype=np.uint32)
    checked = differs = 0
    for nz in (None, noise):
        o = _opts(1, 4.0, sampling_topk=topk, sampling_temperature=T, num_hypotheses=n)
        ids, sc, fin = _run_engine_n(engine, table, B, o, seeds, nz)
        for b in range(B):
            words = None if nz is None else (lambda step, j, idx, b=b: nz[step, b * n + j, idx])
            r = S.sampled_search(SampledHotwordRaw(S.table_fn(table, b, n), n, prefix_dict(entries), 4.0, V), n, steps, topk, T, seeds[b], words_fn=words, **proc)
            plain = S.sampled_search(S.table_fn(table, b, n), n, steps, topk, T, seeds[b], words_fn=words, **proc)
            if r["min_gap"] < S.MARGIN:
                continue
            checked += 1
            differs += int(plain["ids"] != r["ids"])
            assert ids[b] == r["ids"] and fin[b] == r["finish_step"], (topk, b, ids[b], r["ids"])
            for g, w in zip(sc[b], r["scores"]):
                assert abs(g - w) <= 2e-4 * max(1.0, abs(w)), (g, w)
    assert checked >= 3 and differs >= 1, (checked, differs)


def test_the_boost_is_no_captured_value(engine):
    """Two calls with different boosts, one after the other on one handle, each equal to ITS reference; then the option off (and never set):
    the plain reference, bit for bit what a handle that never saw the option answers."""
    rng = np.random.default_rng(181)
    table, hot = _hot_table(rng, 16, 2, 5)
    entries = _entries(rng, hot)
    plain_before = _run_engine(engine, table, 2, 5)
    _install(engine, entries)
    stats = _stats()
    a = _compare(engine, table, 2, 5, entries, 2.0, stats, "boost 2")
    b = _compare(engine, table, 2, 5, entries, 7.0, stats, "boost 7")
    a2 = _compare(engine, table, 2, 5, entries, 2.0, stats, "boost 2 again")
    assert a[0] != b[0] and a[0] == a2[0] and np.array_equal(a[1], a2[1]), (a[0], b[0])
    for off in (_run_engine(engine, table, 2, 5), _run_engine(engine, table, 2, 5, hotwords=0, hotword_boost=7.0)):      # never set | off with a boost lying around
        assert off[0] == plain_before[0] and np.array_equal(off[1], plain_before[1]) and off[2].tolist() == plain_before[2].tolist() and np.array_equal(off[3], plain_before[3])
    for bb in range(2):
        r, _ = _run_oracle(table, bb, 5, None, 0.0)
        if min(r["trace"]) >= MARGIN:
            _check(plain_before, r, bb, 5, ("off", bb))
    assert stats["checked"] >= 4, stats
    # another set of another size on the same handle: the captured step serves it too
    other = [[int(hot[0][3]), int(hot[0][4])], [int(hot[1][3])]]
    _install(engine, other)
    _compare(engine, table, 2, 5, other, 2.0, stats, "another set")


def test_refused_calls_enqueue_nothing(engine):
    from wis_hip import _lib
    lib = _lib.load()
    rng = np.random.default_rng(191)
    table, hot = _hot_table(rng, 10, 1, 2)
    entries = _entries(rng, hot)
    good = _run_engine(engine, table, 1, 2)

    def still_plain():
        again = _run_engine(engine, table, 1, 2)
        assert again[0] == good[0] and np.array_equal(again[1], good[1]) and np.array_equal(again[3], good[3])
    _lib.check(_set_trie(engine, np.zeros((0, 4), np.int32)))
    assert _run_engine(engine, table, 1, 2, 2.0, rc_only=True) == WIS_E_STATE      # no set installed
    still_plain()
    _install(engine, entries)
    for kw, code in ((dict(hotwords=2, hotword_boost=2.0), WIS_E_ARG), (dict(hotwords=-1, hotword_boost=2.0), WIS_E_ARG), (dict(hotwords=1, hotword_boost=0.0), WIS_E_ARG),
                     (dict(hotwords=1, hotword_boost=-1.0), WIS_E_ARG), (dict(hotwords=1, hotword_boost=float("nan")), WIS_E_ARG),
                     (dict(hotwords=1, hotword_boost=float("inf")), WIS_E_ARG), (dict(hotwords=1, hotword_boost=2.0, phrases=1), WIS_E_ARG)):
        assert _run_engine(engine, table, 1, 2, rc_only=True, **kw) == code, kw
        still_plain()
    assert _run_engine(engine, table, 1, 2, rc_only=True, hotwords=0, hotword_boost=float("nan")) == 0      # the boost is ignored when the option is off
    # a malformed table: WIS_E_ARG, the set installed before stays in place
    before = _run_engine(engine, table, 1, 2, 3.0)
    assert _set_trie(engine, [[-1, 1, 5, 0], [400, 0, 0, 1]]) == WIS_E_ARG
    after = _run_engine(engine, table, 1, 2, 3.0)
    assert after[0] == before[0] and np.array_equal(after[1], before[1])
    # the hotword set and the phrase set do not disturb each other
    _lib.check(lib.wis_model_set_phrases(engine._replicas[0].handle, np.ascontiguousarray(np.asarray([[-1, 1, 1, 0], [400, 0, 0, 1]], np.int32)).ctypes.data_as(i32p), 2))
    after = _run_engine(engine, table, 1, 2, 3.0)
    assert after[0] == before[0] and np.array_equal(after[1], before[1])
    _lib.check(lib.wis_model_set_phrases(engine._replicas[0].handle, None, 0))
    # the drafted entry points refuse before anything runs
    h = engine._replicas[0].handle
    mel = np.zeros((1, 80, 3000), np.float32)
    prompt = np.asarray([50258, 50259, 50359, 50363], np.int32)
    ids, ln, sc, acc = np.zeros(224, np.int32), np.zeros(1, np.int32), np.zeros(1, np.float32), C.c_int32(0)
    o = _opts(1, 2.0)
    d = np.asarray([400, 401], np.int32)
    rc = lib.wis_generate_draft(h, _lib.ptr(mel), prompt.ctypes.data_as(i32p), 4, C.byref(o), d.ctypes.data_as(i32p), 2, ids.ctypes.data_as(i32p),
                                ln.ctypes.data_as(i32p), sc.ctypes.data_as(f32p), C.byref(acc))
    assert rc == WIS_E_UNSUPPORTED, rc
    o.beam_size = 2
    dt, do = np.asarray([[400, 401]], np.int32), np.zeros((1, 2), np.int32)
    rc = lib.wis_generate_draft_beam(h, _lib.ptr(mel), prompt.ctypes.data_as(i32p), 4, C.byref(o), dt.ctypes.data_as(i32p), do.ctypes.data_as(i32p), 1,
                                     ids.ctypes.data_as(i32p), ln.ctypes.data_as(i32p), sc.ctypes.data_as(f32p), C.byref(acc))
    assert rc == WIS_E_UNSUPPORTED, rc
    still_plain()
