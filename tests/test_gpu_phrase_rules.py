"""-m gpu: phrase-constrained decoding in the sampling tail (phrase_rules_kernel behind rep_rules_kernel) against the CPU statement of the
rule (tests/phrase_ref.py: a dict of prefixes, written without the engine's trie) plugged into the oracle's search, EXACTLY.

`wis_debug_search` / `wis_debug_search_n` run the tail on caller-supplied logits tables; `WhisperRef.search` over `phrase_ref.PhraseStepFn`
runs over the SAME tables.  Ids, lengths, finish steps and the ancestry of the finite-score beams must be identical (which -inf filler a dead
slot carries is not specified: tests/test_gpu_search_edges.py compares the same way).  A case is skipped - and counted - only when the oracle
sees a decision margin below 2e-4 (tests/test_gpu_search.py's rule, same cap: at most a fifth of the checked cases, at least 4 checked per
group); the seeds were chosen on the CPU so that the reference alone meets the cap."""
import ctypes as C

import numpy as np
import pytest
import torch

from phrase_ref import NoReorderPhraseStepFn, PhraseStepFn, brute_force, prefix_dict
from rep_ref import RepRaw

pytestmark = pytest.mark.gpu
V, EOT = 51865, 50257
MARGIN = 2e-4
WIS_E_ARG, WIS_E_STATE, WIS_E_UNSUPPORTED = -1, -6, -7      # include/wis_hip.h


@pytest.fixture(scope="module")
def engine():
    from wis_hip import ctranslate2 as ct2, weights as W
    model = ct2.Whisper("unused", weights=W.synthetic_weights("tiny", seed=1234), arch=W.arch("tiny"), max_batch=16, max_beam=8)
    yield model
    model.close()


def _set_trie(model, trie):
    from wis_hip import _lib
    trie = np.ascontiguousarray(np.asarray(trie, np.int32).reshape(-1, 4))
    return _lib.load().wis_model_set_phrases(model._replicas[0].handle, trie.ctypes.data_as(C.POINTER(C.c_int32)), len(trie))


def _install(model, phrases):
    from wis_hip import _lib, weights as W
    _lib.check(_set_trie(model, W.build_phrase_trie(phrases)))


def _run_engine(model, table, B, beam, longest, phrases=1, max_new=0, n_hyp=1, p=None, n=None, **fields):
    """table f32 [steps][B*beam][V] -> (ids per utterance (n_hyp > 1: per utterance and result), scores, finish steps, parents [steps][B*beam]);
    phrases None: the field is never set.  longest: the installed set's longest phrase (max_new_tokens 0 resolves by it)."""
    from wis_hip import _lib
    lib = _lib.load()
    steps = table.shape[0]
    o = _lib.GenOpts(0, beam, max_new, 1.0, 1.0, 1, 1, 0, 0)
    if phrases is not None:
        o.phrases = phrases
    if p is not None:
        o.repetition_penalty = p
    if n is not None:
        o.no_repeat_ngram_size = n
    for k, v in fields.items():
        setattr(o, k, v)
    width = max_new or (min(steps, longest + 1) if phrases else steps)
    fin = np.zeros(B, np.int32); par = np.full((steps, B * beam), -1, np.int32)
    i32, f32 = C.POINTER(C.c_int32), C.POINTER(C.c_float)
    h = model._replicas[0].handle
    if n_hyp > 1:
        o.num_hypotheses = n_hyp
        ids = np.zeros((B, n_hyp, width), np.int32); lens = np.zeros((B, n_hyp), np.int32); sc = np.zeros((B, n_hyp), np.float32)
        _lib.check(lib.wis_debug_search_n(h, _lib.ptr(table), steps, B, C.byref(o), None, None, ids.ctypes.data_as(i32), lens.ctypes.data_as(i32), sc.ctypes.data_as(f32),
                                          fin.ctypes.data_as(i32), par.ctypes.data_as(i32)))
        return [[ids[b, j, :lens[b, j]].tolist() for j in range(n_hyp)] for b in range(B)], sc, fin, par
    ids = np.zeros((B, width), np.int32); lens = np.zeros(B, np.int32); sc = np.zeros(B, np.float32)
    _lib.check(lib.wis_debug_search(h, _lib.ptr(table), steps, B, C.byref(o), ids.ctypes.data_as(i32), lens.ctypes.data_as(i32), sc.ctypes.data_as(f32),
                                    fin.ctypes.data_as(i32), par.ctypes.data_as(i32)))
    return [ids[b, :lens[b]].tolist() for b in range(B)], sc, fin, par


def _raw_of(table, b, beam):
    tt = torch.from_numpy(table)
    return lambda step, last, origin: tt[step, b * beam:(b + 1) * beam] if step > 0 else tt[0, b * beam].expand(beam, -1)


def _run_oracle(table, b, beam, phrases, p=1.0, n=0, step_cls=PhraseStepFn):
    """-> (the reference search over the masked rows, its step function); p / n: the repetition rules in front (rep_ref.RepRaw)"""
    from oracle.whisper_ref import WhisperRef
    from wis_hip import weights as W
    raw = _raw_of(table, b, beam)
    if p != 1.0 or n != 0:
        raw = RepRaw(raw, beam, p, n)
    fn = step_cls(raw, beam, W.SUPPRESS_IDS, W.SUPPRESS_IDS_BEGIN, prefix_dict(phrases))
    longest = max(len(ph) for ph in phrases)
    return WhisperRef.search(fn, beam, V, EOT, min(table.shape[0], longest + 1), 1.0, 1.0), fn


def _pool():
    from wis_hip import weights as W
    bad = set(W.SUPPRESS_IDS) | set(W.SUPPRESS_IDS_BEGIN)
    return np.asarray([t for t in range(EOT) if t not in bad])


def _random_set(rng, n_phrases, lo, hi, alphabet=None, n_roots=None):
    """n_phrases different phrases of lo .. hi tokens that SHARE PREFIXES (a new phrase branches off a random prefix of an earlier one, or - a
    third of the time - IS such a prefix: an interior phrase end).  alphabet: the ids to draw from (default: every allowed text token);
    n_roots: at most this many different first tokens."""
    pool = _pool() if alphabet is None else np.asarray(alphabet)
    out, seen = [], set()
    while len(out) < n_phrases:
        L = int(rng.integers(lo, hi + 1))
        if out and rng.random() < 0.75:
            base = out[int(rng.integers(0, len(out)))]
            cut = int(rng.integers(1, len(base) + 1))
            ph = list(base[:cut]) if rng.random() < 0.33 else list(base[:cut]) + rng.choice(pool, size=max(L - cut, 1)).tolist()
        else:
            ph = rng.choice(pool, size=L).tolist()
            if n_roots is not None and len({p[0] for p in out}) >= n_roots:
                ph[0] = out[int(rng.integers(0, len(out)))][0]
        ph = [int(t) for t in ph][:hi]
        if len(ph) >= lo and tuple(ph) not in seen:
            seen.add(tuple(ph)); out.append(ph)
    return out


def _table(rng, steps, B, beam):
    """logits N(0, 2^2); under the mask only the set's children and <|endoftext|> count, and those are as random as the rest"""
    return np.ascontiguousarray(2.0 * rng.standard_normal((steps, B * beam, V), dtype=np.float32))


def _check(got, r, fn, b, beam, ctx):
    ids, sc, fin, par = got
    assert ids[b] == r["ids"], (ctx, ids[b], r["ids"])
    assert fin[b] == r["finish_step"], (ctx, fin[b], r["finish_step"])
    assert np.isfinite(r["score"]), ctx                    # (a phrase set always leaves a finite hypothesis)
    assert abs(sc[b] - r["score"]) <= 2e-4 * max(1.0, abs(r["score"])), (ctx, sc[b], r["score"])
    for s, org in enumerate(r["origins"]):                 # ancestry of the beams whose cumulative score is finite behind step s
        keep = fn.alive[s]
        want = [b * beam + (0 if s == 0 else o) for o, k in zip(org, keep) if k]
        have = [h for h, k in zip(par[s, b * beam:(b + 1) * beam].tolist(), keep) if k]
        assert have == want, (ctx, s, have, want)


def _stats():
    return dict(checked=0, skipped=0, finish=[], margin=float("inf"), dead=0)


def _compare(model, table, B, beam, phrases, stats, ctx=(), p=None, n=None, installed=False):
    if not installed:
        _install(model, phrases)
    longest = max(len(ph) for ph in phrases)
    got = _run_engine(model, table, B, beam, longest, p=p, n=n)
    for b in range(B):
        r, fn = _run_oracle(table, b, beam, phrases, 1.0 if p is None else p, 0 if n is None else n)
        if min(r["trace"]) < MARGIN:
            stats["skipped"] += 1
            continue
        stats["checked"] += 1
        stats["finish"].append(int(r["finish_step"]))
        stats["margin"] = min(stats["margin"], min(r["trace"]))
        stats["dead"] += sum(1 for a in fn.alive if not all(a))
        assert r["ids"] in phrases, (ctx, r["ids"])          # the answer is one of the caller's phrases
        _check(got, r, fn, b, beam, (ctx, B, beam, b))
    return got


def _assert_group(stats, what):
    print(f"\n[phrases] {what}: {stats['checked']} searches identical to the reference, {stats['skipped']} skipped as fp32 near-ties; finish steps "
          f"{stats['finish']}; steps with a dead (-inf) slot {stats['dead']}; smallest decision margin {stats['margin']:.2e}")
    assert stats["checked"] >= 4 and stats["skipped"] <= max(1, stats["checked"] // 5), stats


# beam -> seed.  Per beam four kinds of set: fewer phrases than the beam (beam 1: a single phrase), more than 2 * beam, shared prefixes with
# interior phrase ends on a narrow root, and a root of more than 256 children; tables of 8 .. 33 steps
GRID = {1: 101, 2: 102, 5: 105, 8: 108}


def _grid_sets(rng, beam):
    few = _random_set(rng, max(1, beam - 1), 3, 7)
    many = _random_set(rng, 2 * beam + 3, 4, 10)
    shared = _random_set(rng, beam + 1, 2, 12, n_roots=2)
    longest = max(shared, key=len)
    shared.append(next(longest[:c] for c in range(len(longest) - 1, 0, -1) if longest[:c] not in shared))      # an interior phrase end for certain
    wide = [[int(t)] + rng.choice(_pool(), size=int(rng.integers(1, 4))).tolist() for t in rng.choice(_pool(), size=300, replace=False)]
    deep = _random_set(rng, beam, 20, 31, n_roots=1)
    base = max(deep, key=len)
    deep.append(base + rng.choice(_pool(), size=32 - len(base)).tolist())      # a 32-token phrase: 33 steps
    return [("few", few), ("many", many), ("shared", shared), ("wide root", wide), ("long", deep)]


@pytest.mark.parametrize("beam", [1, 2, 5, 8])
def test_basic_grid(engine, beam):
    rng = np.random.default_rng(GRID[beam])
    stats, steps_seen = _stats(), []
    for what, phrases in _grid_sets(rng, beam):
        pre = prefix_dict(phrases)
        if what == "shared":
            assert any(ends and kids for kids, ends in pre.values()), "no interior phrase end"
        if what == "wide root":
            assert len(pre[()][0]) > 256
        steps = max(8, max(len(ph) for ph in phrases) + 1)
        steps_seen.append(steps)
        _compare(engine, _table(rng, steps, 1, beam), 1, beam, phrases, stats, what)
    assert min(steps_seen) == 8 and max(steps_seen) == 33, steps_seen
    if beam > 1:
        assert stats["dead"] > 0, stats          # fewer phrases than beams: dead slots were carried
    _assert_group(stats, f"basic grid, beam {beam}")


BRUTE = [(201, 2, 2), (202, 5, 4), (203, 5, 5), (204, 8, 7), (205, 8, 8)]      # (seed, beam, phrases <= beam)


def test_brute_force_ranking(engine):
    """Rows equal over the beams (the logits depend on the step alone) and beam >= the number of phrases: the search is exhaustive, so its n
    best are the float64 brute force's, in its order, with its scores (2e-4 relative).  Precondition: adjacent brute-force scores >= 1e-3 apart."""
    for seed, beam, n_ph in BRUTE:
        rng = np.random.default_rng(seed)
        phrases = _random_set(rng, n_ph, 2, 6, n_roots=2)
        steps = max(len(ph) for ph in phrases) + 1
        row = 2.0 * rng.standard_normal((steps, 1, V), dtype=np.float32)
        table = np.ascontiguousarray(np.repeat(row, beam, axis=1))
        bf = brute_force(phrases, lambda h: row[len(h), 0])
        gaps = [a[0] - b[0] for a, b in zip(bf[:-1], bf[1:])]
        assert min(gaps) >= 1e-3, (seed, gaps)
        _install(engine, phrases)
        one = _run_engine(engine, table, 1, beam, steps - 1)
        assert tuple(one[0][0]) == bf[0][2] and abs(one[1][0] - bf[0][0]) <= 2e-4 * max(1.0, abs(bf[0][0])), (seed, one[0], bf[0])
        ids, sc, _, _ = _run_engine(engine, table, 1, beam, steps - 1, n_hyp=n_ph)
        assert [tuple(x) for x in ids[0]] == [e[2] for e in bf], (seed, ids[0], bf)
        for j, e in enumerate(bf):
            assert abs(sc[0, j] - e[0]) <= 2e-4 * max(1.0, abs(e[0])), (seed, j, sc[0, j], e[0])
        if beam > n_ph:      # more results asked than phrases exist: the rest are -inf fillers, behind every phrase
            ids, sc, _, _ = _run_engine(engine, table, 1, beam, steps - 1, n_hyp=beam)
            assert [tuple(x) for x in ids[0][:n_ph]] == [e[2] for e in bf] and np.all(np.isneginf(sc[0, n_ph:])), (seed, ids[0], sc[0])


ANCESTRY_SEEDS = [301, 302, 303, 304, 305, 306]


def _ancestry_case(seed):
    rng = np.random.default_rng(seed)
    alphabet = rng.choice(_pool(), size=5, replace=False)
    phrases = _random_set(rng, 12, 4, 8, alphabet=alphabet)
    return phrases, _table(rng, 9, 1, 2)


def test_histories_follow_the_beam_ancestry(engine):
    """Beam 2: at some step the beams cross over (beam 1's successor descends from beam 0, or both from one) while their nodes differ - the
    mask must be taken from the REORDERED history.  Asserted on the reference: such steps exist, and a reference that does not reorder gives
    another answer."""
    stats = _stats()
    crossed = wrong_differs = 0
    for seed in ANCESTRY_SEEDS:
        phrases, table = _ancestry_case(seed)
        r, fn = _run_oracle(table, 0, 2, phrases)
        crossed += int(any(s > 0 and org != [0, 1] for s, org in enumerate(r["origins"])))
        wrong, _ = _run_oracle(table, 0, 2, phrases, step_cls=NoReorderPhraseStepFn)
        wrong_differs += int(wrong["ids"] != r["ids"])
        _compare(engine, table, 1, 2, phrases, stats, seed)
    assert crossed >= 4 and wrong_differs >= 2, (crossed, wrong_differs)
    _assert_group(stats, f"ancestry ({crossed} tables cross over, {wrong_differs} would differ without the reordering)")


def test_ragged_batch(engine):
    """B = 3 with phrases of different lengths in one set: the utterances end at different steps while their rows keep flowing through the batch
    (phrase_rules_kernel returns at `done`), and every utterance equals its own single-utterance reference."""
    stats = _stats()
    fins = []
    for seed, beam in ((407, 2), (402, 5)):      # (chosen on the CPU: three different finish steps each)
        rng = np.random.default_rng(seed)
        phrases = _random_set(rng, 3 * beam, 1, 14)
        table = _table(rng, 15, 3, beam)
        got = _compare(engine, table, 3, beam, phrases, stats, seed)
        fins.append(got[2].tolist())
    assert all(len(set(f)) >= 2 for f in fins), fins
    _assert_group(stats, f"ragged batch, finish steps {fins}")


def test_depth_32(engine):
    """Beam 1: a 32-token phrase beside one that leaves it at the last token and one that ends half way - 33 steps, the longest walk."""
    rng = np.random.default_rng(501)
    deep = rng.choice(_pool(), size=32, replace=False).tolist()
    other = int(_pool()[4242])
    phrases = [deep, deep[:31] + [other], deep[:16]]
    table = _table(rng, 33, 1, 1)
    table[:, 0, EOT] = -40.0                       # the search goes all the way: EOT loses at the interior end
    table[31, 0, deep[31]], table[31, 0, other] = 1.0, 3.0
    r, fn = _run_oracle(table, 0, 1, phrases)
    assert r["ids"] == deep[:31] + [other] and r["finish_step"] == 32 and min(r["trace"]) > 1.0, (r["ids"][-3:], r["finish_step"])
    _install(engine, phrases)
    _check(_run_engine(engine, table, 1, 1, 32), r, fn, 0, 1, "depth 32")
    table[31, 0, deep[31]] = 5.0
    r, fn = _run_oracle(table, 0, 1, phrases)
    assert r["ids"] == deep
    _check(_run_engine(engine, table, 1, 1, 32), r, fn, 0, 1, "depth 32, the other leaf")


REP_CASES = [(610, 1), (697, 1), (614, 2), (665, 2), (645, 5), (671, 5)]      # (seed, beam): chosen on the CPU - no live row ends all -inf, the rules decide


def test_combined_with_the_repetition_rules(engine):
    """repetition_penalty / no_repeat_ngram_size with the constraint: the reference is PhraseStepFn over rep_ref.RepRaw (the penalty and the bans
    first, then the mask).  The phrases are drawn from five tokens, so histories repeat and the rules decide (asserted on the reference).  A ban
    can take a node's LAST child: that live row is all -inf, a regime the oracle does not specify (its log-softmax is NaN there) - the seeds keep
    every case out of it (asserted on the reference: no hypothesis carries a NaN)."""
    stats = _stats()
    decided = 0
    for seed, beam in REP_CASES:
        rng = np.random.default_rng(seed)
        alphabet = rng.choice(_pool(), size=5, replace=False)
        phrases = _random_set(rng, 14, 3, 7, alphabet=alphabet)
        table = _table(rng, 8, 1, beam)
        _install(engine, phrases)
        plain, _ = _run_oracle(table, 0, beam, phrases)
        for p, n in ((1.0, 2), (3.0, 0), (1.5, 3)):
            r, _ = _run_oracle(table, 0, beam, phrases, p, n)
            assert np.isfinite(r["score"]) and all(h[0] == h[0] for h in r["hyps"]), (seed, beam, p, n)
            decided += int(r["ids"] != plain["ids"])
            _compare(engine, table, 1, beam, phrases, stats, (seed, p, n), p=p, n=n, installed=True)
    assert 2 * decided >= 3 * len(REP_CASES), decided      # (half of the 18 cases)
    _assert_group(stats, f"combined with the repetition rules ({decided} cases decided by them)")


def test_off_is_todays_search(engine):
    """phrases = 0 - with a set installed - gives what a call that never sets the field gives, bit for bit: the plain oracle search."""
    from oracle.whisper_ref import WhisperRef
    from rep_ref import RepStepFn
    from wis_hip import weights as W
    rng = np.random.default_rng(701)
    table = _table(rng, 10, 2, 5)
    table[:, :, EOT] = table.max(axis=2) - 6.0 + 0.9 * np.arange(10, dtype=np.float32)[:, None]
    _install(engine, _random_set(rng, 6, 2, 5))
    never = _run_engine(engine, table, 2, 5, 0, phrases=None)
    off = _run_engine(engine, table, 2, 5, 0, phrases=0)
    assert never[0] == off[0] and np.array_equal(never[1], off[1]) and never[2].tolist() == off[2].tolist() and np.array_equal(never[3], off[3])
    for b in range(2):
        r = WhisperRef.search(RepStepFn(_raw_of(table, b, 5), 5, W.SUPPRESS_IDS, W.SUPPRESS_IDS_BEGIN), 5, V, EOT, 10, 1.0, 1.0)
        if min(r["trace"]) >= MARGIN:
            assert off[0][b] == r["ids"] and off[2][b] == r["finish_step"], (b, off[0][b], r["ids"])


def test_set_twice(engine):
    """The same table twice in a row gives equal results; a second set installed between two calls answers with ITS phrases - nothing of the
    first set (its records beyond the second's, its longest phrase) leaks; removing the set turns the option into WIS_E_STATE."""
    from wis_hip import _lib
    rng = np.random.default_rng(801)
    first = _random_set(rng, 40, 6, 12)
    second = _random_set(rng, 3, 2, 3)
    table = _table(rng, 13, 1, 5)
    stats = _stats()
    a = _compare(engine, table, 1, 5, first, stats, "first")
    b = _run_engine(engine, table, 1, 5, 12)
    assert a[0] == b[0] and np.array_equal(a[1], b[1]) and a[2].tolist() == b[2].tolist() and np.array_equal(a[3], b[3])
    c = _compare(engine, table, 1, 5, second, stats, "second")
    assert c[0][0] in second and c[0][0] not in first and c[2][0] <= 3, c
    d = _compare(engine, table, 1, 5, first, stats, "first again")
    assert d[0] == a[0] and np.array_equal(d[1], a[1])
    _lib.check(_set_trie(engine, np.zeros((0, 4), np.int32)))
    with pytest.raises(_lib.WisError) as e:
        _run_engine(engine, table, 1, 5, 12)
    assert e.value.code == WIS_E_STATE, e.value
    assert stats["checked"] + stats["skipped"] == 3 and stats["checked"] >= 2, stats


def test_malformed_tries_are_refused(engine):
    """Everything is validated on the host (nothing reaches the device); the set installed before stays in place."""
    from wis_hip import _lib, weights as W
    good = [[400, 401], [400, 402, 403], [500]]
    _install(engine, good)
    ok = W.build_phrase_trie(good)          # [[-1,1,2,0],[400,3,2,0],[500,0,0,1],[401,0,0,1],[402,5,1,0],[403,0,0,1]]
    assert ok.tolist() == [[-1, 1, 2, 0], [400, 3, 2, 0], [500, 0, 0, 1], [401, 0, 0, 1], [402, 5, 1, 0], [403, 0, 0, 1]]

    def bad(i, col, val):
        t = ok.copy(); t[i, col] = val
        return t
    cases = {
        "child index out of range": bad(4, 1, 6), "child index into an earlier block": bad(4, 1, 3), "child count beyond the table": bad(1, 2, 40),
        "unsorted children": bad(1, 0, 600), "equal children": bad(4 - 1, 0, 402), "a leaf that ends nothing": bad(5, 3, 0), "end flag 2": bad(5, 3, 2),
        "a suppressed token": bad(3, 0, W.SUPPRESS_IDS[5]), "a suppressed first token": bad(1, 0, 220), "<|endoftext|>": bad(5, 0, EOT),
        "a timestamp": bad(5, 0, V - 1), "beyond the vocabulary": bad(5, 0, V + 7), "a negative token": bad(5, 0, -3), "an empty phrase": bad(0, 3, 1),
        "a root token": bad(0, 0, 5), "no children at the root": np.asarray([[-1, 0, 0, 0]], np.int32), "an orphan record": np.concatenate([ok, [[700, 0, 0, 1]]]).astype(np.int32),
        "a negative count": bad(4, 2, -1),
    }
    for what, t in cases.items():
        assert _set_trie(engine, t) == WIS_E_ARG, what
    assert 220 not in W.SUPPRESS_IDS and _set_trie(engine, bad(3, 0, 220)) == 0       # suppress_ids_begin binds the FIRST token only
    _install(engine, good)
    # the limits: 4096 children fit, 4097 do not; 32 tokens fit, 33 do not; 65535 records
    pool = _pool()
    wide = np.asarray([[-1, 1, 4097, 0]] + [[int(t), 0, 0, 1] for t in pool[:4097]], np.int32)
    assert _set_trie(engine, wide) == WIS_E_UNSUPPORTED
    wide = wide[:4097].copy(); wide[0, 2] = 4096
    assert _set_trie(engine, wide) == 0
    chain = lambda n: np.asarray([[-1, 1, 1, 0]] + [[int(pool[100 + i]), i + 2 if i < n - 1 else 0, 1 if i < n - 1 else 0, int(i == n - 1)] for i in range(n)], np.int32)
    assert _set_trie(engine, chain(32)) == 0 and _set_trie(engine, chain(33)) == WIS_E_UNSUPPORTED
    assert _set_trie(engine, np.zeros((65536, 4), np.int32)) == WIS_E_UNSUPPORTED
    # a refused table left the last good one (the 32-token chain) in place
    table = _table(np.random.default_rng(5), 33, 1, 1)
    table[:, 0, EOT] = -40.0
    assert _run_engine(engine, table, 1, 1, 32)[0][0] == [int(pool[100 + i]) for i in range(32)]


def test_refused_combinations(engine):
    from wis_hip import _lib
    lib = _lib.load()
    _install(engine, [[400, 401, 402], [500]])
    table = np.zeros((6, 1, V), np.float32)
    for kw, code in ((dict(timestamps=1), WIS_E_UNSUPPORTED), (dict(fixed_new_tokens=3), WIS_E_UNSUPPORTED), (dict(sampling_topk=-1), WIS_E_UNSUPPORTED),
                     (dict(sampling_topk=4), WIS_E_UNSUPPORTED), (dict(phrases=2), WIS_E_ARG), (dict(phrases=-1), WIS_E_ARG), (dict(max_new_tokens=3), WIS_E_ARG)):
        with pytest.raises(_lib.WisError) as e:
            _run_engine(engine, table, 1, 1, 3, **kw)
        assert e.value.code == code, (kw, e.value)
    assert _run_engine(engine, table, 1, 1, 3, max_new=4)[0][0] in ([400, 401, 402], [500])      # longest + 1: accepted
    with pytest.raises(_lib.WisError) as e:                                                       # fewer steps of logits than the longest phrase needs
        _run_engine(engine, table[:3], 1, 1, 3)
    assert e.value.code == WIS_E_ARG, e.value
    # the drafted entry points refuse before anything runs
    h = engine._replicas[0].handle
    mel = np.zeros((1, 80, 3000), np.float32)
    prompt = np.asarray([50258, 50259, 50359, 50363], np.int32)
    i32 = C.POINTER(C.c_int32)
    ids, ln, sc, acc = np.zeros(224, np.int32), np.zeros(1, np.int32), np.zeros(1, np.float32), C.c_int32(0)
    o = _lib.GenOpts(0, 1, 0, 1.0, 1.0, 1, 1, 0, 0)
    o.phrases = 1
    d = np.asarray([400, 401], np.int32)
    rc = lib.wis_generate_draft(h, _lib.ptr(mel), prompt.ctypes.data_as(i32), 4, C.byref(o), d.ctypes.data_as(i32), 2, ids.ctypes.data_as(i32),
                                ln.ctypes.data_as(i32), sc.ctypes.data_as(C.POINTER(C.c_float)), C.byref(acc))
    assert rc == WIS_E_UNSUPPORTED, rc
    o.beam_size = 2
    dt, do = np.asarray([[400, 401]], np.int32), np.zeros((1, 2), np.int32)
    rc = lib.wis_generate_draft_beam(h, _lib.ptr(mel), prompt.ctypes.data_as(i32), 4, C.byref(o), dt.ctypes.data_as(i32), do.ctypes.data_as(i32), 1,
                                     ids.ctypes.data_as(i32), ln.ctypes.data_as(i32), sc.ctypes.data_as(C.POINTER(C.c_float)), C.byref(acc))
    assert rc == WIS_E_UNSUPPORTED, rc
