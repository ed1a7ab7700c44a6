"""-m gpu: the sampling tail on CONSTRUCTED logits, through `wis_debug_search`, exact against `WhisperRef.search`.

tests/test_gpu_search.py feeds i.i.d. normal logits: the 2k best tokens of a row then sit in 2k different sub-chunks, lanes and pool
quarters, so a selection that keeps too few candidates per sub-chunk or per wave, drops the second value of a lane, clamps the short
last sub-chunk wrongly or retires the wrong pool entry would pass it.  The tables here put the candidates where the hierarchy of
logit_stats_kernel (64 sub-chunks of SL = ceil(V / 64) = 811 ids, one wave each, 13 values per lane, top n_cand per sub-chunk) and
beam_step_kernel (four waves, the top n_cand of a quarter of the pool each, then a rank over the 4 n_cand survivors) has to do all the
work: a low floor (0.5 N(0, 1) - 12) and per row a LADDER of 3k + 2 high values, steps >= 0.3 apart, permuted over ids that a
placement chooses, a per-beam offset against cross-beam near-ties and an EOT column that climbs so hypotheses end mid-search.
Placements: one sub-chunk (a different one per row and step); the sub-chunk that holds EOT; one lane of a sub-chunk; the short last sub-chunk with
its first and last ids; ids 0, c - 2 .. c + 1 around a sub-chunk boundary and suppressed ids with the row's largest raw logits; one row that
supplies all 2k candidates of a step.  Then exact ties, rows with fewer finite logits than candidates, fixed_new_tokens, and the 51866-token vocabulary.

Conventions of tests/test_gpu_search.py: ids, hypothesis length, finish step and the ancestry of every step are compared EXACTLY; a
case is skipped - and counted - only when the oracle's decision margin min(trace) is below 2e-4.  `python tests/test_gpu_search_edges.py`
prints, from the oracle alone (no GPU), the figures the caps of every (placement, beam) are asserted on.
"""
import ctypes as C
import os
import sys
import zlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
EOT = 50257
SUB = 64                       # kernels.hpp STAT_SUB
STEPS = 10
SALT = 4                       # of every table's seed: one under which no (placement, beam) loses more than a fifth of its cases to near-ties
SEEDS = {1: (0, 1, 2, 3), 5: (0, 1, 2, 3), 8: (0, 1, 2)}      # x OPTS = 12 / 12 / 9 searches per (placement, beam)
OPTS = (dict(), dict(length_penalty=0.0), dict(patience=2.0))
# EOT logit of a row = the row's ladder top + EOT_RAMP[beam][0] + EOT_RAMP[beam][1] * step (+ 0.3 N(0, 1) per row): chosen per beam so that
# the ORACLE alone meets the caps below on every placement (the __main__ block prints the counts)
EOT_RAMP = {1: (-3.0, 0.9), 5: (-3.0, 0.9), 8: (-3.0, 0.9)}
DOM_STEPS = range(2, 5)        # placement "dominate": the steps at which one row supplies all 2k candidates
EOT_RAMP_DOM = {1: (-3.0, 1.2), 5: (-3.0, 1.2), 8: (-3.0, 1.8)}      # ... its EOT ramp counts from the last of them


def _sl(V):
    return -(-V // SUB)


@pytest.fixture(scope="module")
def engine():
    from wis_hip import ctranslate2 as ct2, weights as W
    w = W.synthetic_weights("tiny", seed=1234)
    model = ct2.Whisper("unused", weights=w, arch=W.arch("tiny"), max_batch=16, max_beam=8)
    yield model
    model.close()


@pytest.fixture(scope="module")
def engine_v3():
    """the tiny geometry with the 51866-token vocabulary (large-v3's layout: one more language, every id from <|translate|> up moved by one)"""
    from wis_hip import ctranslate2 as ct2, weights as W
    w = W.synthetic_weights("tiny", seed=1234, n_vocab=W.N_VOCAB_V3)
    a = W.arch_from_weights(w, 6)
    assert a["n_vocab"] == 51866
    model = ct2.Whisper("unused", weights=w, arch=a, max_batch=2, max_beam=5)
    yield model
    model.close()


def _suppress(V):
    from wis_hip import weights as W
    return W.SUPPRESS_IDS if V == W.N_VOCAB else W.special_tokens(V).default_suppress_ids()


def _run_engine(model, table, B, beam, **opts):
    """table f32 [steps][B*beam][V] -> (ids per utterance, scores, finish steps, parents [steps][B*beam])"""
    from wis_hip import _lib
    lib = _lib.load()
    steps = table.shape[0]
    o = _lib.GenOpts(0, beam, opts.get("max_new", 0), opts.get("length_penalty", 1.0), opts.get("patience", 1.0),
                     int(opts.get("suppress_blank", True)), int(opts.get("suppress_default", True)), int(opts.get("fixed_new_tokens", 0)), 0)
    max_new = opts.get("max_new", 0) or steps
    ids = np.zeros((B, max_new), np.int32); lens = np.zeros(B, np.int32); sc = np.zeros(B, np.float32)
    fin = np.zeros(B, np.int32); par = np.full((steps, B * beam), -1, np.int32)
    i32 = C.POINTER(C.c_int32)
    _lib.check(lib.wis_debug_search(model._replicas[0].handle, _lib.ptr(table), steps, B, C.byref(o), ids.ctypes.data_as(i32), lens.ctypes.data_as(i32),
                                    sc.ctypes.data_as(C.POINTER(C.c_float)), fin.ctypes.data_as(i32), par.ctypes.data_as(i32)))
    return [ids[b, :lens[b]].tolist() for b in range(B)], sc, fin, par


def _run_oracle(table, beam, **opts):
    """One utterance (table [steps][beam][V]).  The result also carries `alive` [continued step][beam]: whether the live beam's cumulative
    score is finite (its token had a finite processed logit in the row of a beam that was itself alive)."""
    import torch
    from oracle.whisper_ref import WhisperRef
    from wis_hip import weights as W
    V = table.shape[2]
    tt = torch.from_numpy(table)
    sup = _suppress(V) if opts.get("suppress_default", True) else ()
    alive, state = [], dict(rows=None, ok=[True] + [False] * (beam - 1))

    def fn(step, last, origin):
        if step > 0:      # the beams that step - 1 left: alive when their parent was and the token's processed logit is finite
            prev = state["rows"]
            ok = [state["ok"][o] and bool(torch.isfinite(prev[o, t])) for o, t in zip(origin, last)]
            alive.append(ok); state["ok"] = ok
        rows = tt[step, :beam] if step > 0 else tt[0, 0].expand(beam, -1)
        state["rows"] = WhisperRef.apply_processors(rows, step, sup, W.SUPPRESS_IDS_BEGIN, opts.get("suppress_blank", True), opts.get("fixed_new_tokens", 0), EOT)
        return state["rows"]
    r = WhisperRef.search(fn, beam, V, EOT, opts.get("max_new", 0) or table.shape[0], opts.get("length_penalty", 1.0), opts.get("patience", 1.0))
    r["alive"] = alive
    return r


# ---- tables ---------------------------------------------------------------------------------------------------------------------------
def _ladder(rng, n, lo_step=0.37, spread=0.2):
    """n values from 0 downwards, neighbours lo_step + U(0, spread) apart (>= 0.3)"""
    return -np.concatenate([[0.0], np.cumsum(lo_step + spread * rng.random(n - 1))]).astype(np.float32)


def _pick(rng, lo, hi, n, banned, forced=()):
    """n distinct ids of [lo, hi) outside `banned`, the forced ones first"""
    out = list(forced)
    seen = set(out) | banned
    assert len(seen) == len(out) + len(banned), (forced, sorted(set(forced) & banned))
    while len(out) < n:
        i = int(rng.integers(lo, hi))
        if i not in seen:
            out.append(i); seen.add(i)
    return np.array(out)


def _ids_one_subchunk(rng, n, V, banned, step, row):
    s = int(rng.integers(0, SUB)); lo = s * _sl(V)
    return _pick(rng, lo, min(lo + _sl(V), V), n, banned)


def _ids_eot_subchunk(rng, n, V, banned, step, row):
    """the sub-chunk that holds EOT: it has to report EOT AND the ladder (at beam 1 its n_cand = 2 entries are EOT and the token the search goes on
    with once EOT is taken as a hypothesis and patience asks for another)"""
    lo = EOT // _sl(V) * _sl(V)
    return _pick(rng, lo, min(lo + _sl(V), V), n, banned)


def _ids_one_lane(rng, n, V, banned, step, row):
    """lo + lane + 64 i: the 12 - 13 values of one lane of a sub-chunk, then lane + 1, lane + 2 for the rest"""
    s = int(rng.integers(0, SUB)); lo = s * _sl(V); hi = min(lo + _sl(V), V)
    lane = int(rng.integers(0, 60))
    ids = []
    for l in range(lane, 64):
        ids += [lo + l + 64 * i for i in range(13) if lo + l + 64 * i < hi and lo + l + 64 * i not in banned]
        if len(ids) >= n:
            return np.array(ids[:n])
    raise AssertionError("lane run too short")


def _ids_last_subchunk(rng, n, V, banned, step, row):
    lo = (SUB - 1) * _sl(V)
    return _pick(rng, lo, V, n, banned, forced=(lo, lo + 1, V - 2, V - 1))


def _ids_boundaries(rng, n, V, banned, step, row):
    """ids 0, and c - 2 .. c + 1 around a sub-chunk boundary c = m SL (id 1 is a suppressed id: _table gives it a high raw logit of its own)"""
    while True:
        c = int(rng.integers(1, SUB)) * _sl(V)
        if not ({c - 2, c - 1, c, c + 1} & banned):
            break
    return _pick(rng, 0, V, n, banned, forced=(0, c - 2, c - 1, c, c + 1))


def _ids_scattered(rng, n, V, banned, step, row):
    return _pick(rng, 0, V, n, banned)


PLACEMENTS = {"one_subchunk": _ids_one_subchunk, "eot_subchunk": _ids_eot_subchunk, "one_lane": _ids_one_lane, "last_subchunk": _ids_last_subchunk, "boundaries": _ids_boundaries,
              "dominate": _ids_scattered}


def _table(placement, beam, seed, V=51865, steps=STEPS, eot_ramp=None, eot_top=None):
    """-> (table f32 [steps][beam][V], dom): dom[s] = the row that dominates step s (placement "dominate", steps DOM_STEPS), else -1.
    "dominate": the other rows of such a step are flat (floor noise 0.02, no ladder, no EOT): their best log-probability is ~ -log V = -10.9,
    while the dominating row's 2k-th ladder value stays above -7.5 (steps 0.3 + U(0, 0.08) in this placement) - so all 2k candidates come from the
    one row as long as its beam's cumulative score is within ~3 of the best beam's.  (Raising one row's raw logits by 30 instead would change
    nothing: log-softmax removes it; -log V is as low as a row's best log-probability gets.)  That is why the dominating slot is one of the first
    four (slot j holds the j-th best candidate) and why EOT stays out of the way (14 below the ladder top) during these steps: a slot refilled
    from the secondary candidates can sit 6 below the best beam.  The EOT ramp starts behind them (EOT_RAMP_DOM).
    eot_top: the EOT logit is the row's ladder top + eot_top at every step (fixed_new_tokens tests: EOT is the row maximum from step 0 on)."""
    rng = np.random.default_rng([SALT, seed, beam, zlib.crc32(placement.encode()), V])
    sup = set(_suppress(V))
    banned = sup | {EOT, 220}
    n = 3 * beam + 2
    a0, a1 = eot_ramp if eot_ramp is not None else (EOT_RAMP_DOM if placement == "dominate" else EOT_RAMP)[beam]
    t = (0.5 * rng.standard_normal((steps, beam, V), dtype=np.float32) - 12.0).astype(np.float32)
    dom = [-1] * steps
    for s in range(steps):
        d = int(rng.integers(0, min(beam, 4))) if placement == "dominate" and s in DOM_STEPS else -1
        dom[s] = d
        for j in range(beam):
            if d >= 0 and j != d:
                t[s, j] = (0.02 * rng.standard_normal(V, dtype=np.float32) - 12.0).astype(np.float32)
                continue
            ids = PLACEMENTS[placement](rng, n, V, banned, s, j)
            lad = _ladder(rng, n, 0.3, 0.08) if placement == "dominate" else _ladder(rng, n)
            top = np.float32(0.11 * j)
            t[s, j, ids] = top + lad[rng.permutation(n)]
            if eot_top is not None:
                t[s, j, EOT] = top + eot_top
            elif placement == "dominate":
                t[s, j, EOT] = top + (-14.0 if s <= DOM_STEPS[-1] else a0 + a1 * (s - DOM_STEPS[-1]) + 0.3 * rng.standard_normal())
            else:
                t[s, j, EOT] = top + a0 + a1 * s + 0.3 * rng.standard_normal()
            if placement == "boundaries":      # suppressed ids with the row's largest RAW logits: masked, never picked
                t[s, j, 1] = top + 0.7
                t[s, j, int(rng.choice(sorted(sup - {1})))] = top + 1.0
    return np.ascontiguousarray(t), dom


def _cases(placement, beam, V=51865):
    for seed in SEEDS[beam]:
        table, dom = _table(placement, beam, seed, V)
        for opts in OPTS:
            yield seed, table, dom, opts


def _new_stats():
    return dict(checked=0, skipped=0, finish=[], lens=[], eot_hyps=0)


def _oracle_case(table, beam, dom, stats, **opts):
    """-> the oracle's result, or None for a case the near-tie rule skips; counts what the caps are asserted on"""
    r = _run_oracle(table, beam, **opts)
    if min(r["trace"]) < 2e-4:            # two candidates of different beams within fp32 summation noise at a decision
        stats["skipped"] += 1
        return None
    stats["checked"] += 1
    stats["finish"].append(int(r["finish_step"]))
    stats["lens"].append(sorted({len(h[1]) for h in r["hyps"]}))
    stats["eot_hyps"] += sum(1 for h in r["hyps"] if len(h[1]) <= r["finish_step"])      # ended on EOT before the last step
    for s, org in enumerate(r["origins"]):      # "dominate": every live beam descends from the dominating slot
        if dom[s] >= 0:
            assert org == [dom[s]] * beam, (s, org, dom[s])
    return r


def _assert_caps(stats, beam, n_cases):
    assert stats["checked"] >= 8 and stats["skipped"] <= n_cases // 5, stats
    assert stats["eot_hyps"] >= 3 and len(set(stats["finish"])) >= 2, stats
    if beam > 1:
        assert any(len(l) > 1 for l in stats["lens"]), stats         # hypotheses of different lengths were ranked


def _assert_same(got, r, beam, finite_only=False):
    ids, sc, fin, par = got
    assert ids[0] == r["ids"], (ids[0], r["ids"])
    assert fin[0] == r["finish_step"], (fin[0], r["finish_step"])
    if np.isfinite(r["score"]):
        assert abs(sc[0] - r["score"]) <= 2e-4 * max(1.0, abs(r["score"])), (sc[0], r["score"])
    else:
        assert sc[0] == r["score"]
    # ancestry: after every step the utterance survives, live beam j continues from KV slot origin[j] (finite_only: of the beams whose
    # cumulative score is finite - which -inf filler a dead slot carries is not specified by CTranslate2)
    for s, org in enumerate(r["origins"]):
        want = [0 if s == 0 else o for o in org]
        have = par[s, :beam].tolist()
        if finite_only:
            keep = r["alive"][s]
            want, have = [w for w, k in zip(want, keep) if k], [h for h, k in zip(have, keep) if k]
        assert have == want, (s, have, want)


def _summary(what, stats):
    return (f"{what}: {stats['checked']} searches identical to the oracle ({stats['skipped']} skipped as fp32 near-ties); finish steps "
            f"{sorted(set(stats['finish']))}; hypotheses that ended on EOT mid-search: {stats['eot_hyps']}; unequal-length sets: "
            f"{sum(1 for l in stats['lens'] if len(l) > 1)}")


# ---- placements -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("beam", [1, 5, 8])
@pytest.mark.parametrize("placement", list(PLACEMENTS))
def test_placed_candidates_search_is_exact(engine, placement, beam):
    stats, n = _new_stats(), 0
    for seed, table, dom, opts in _cases(placement, beam):
        n += 1
        r = _oracle_case(table, beam, dom, stats, **opts)
        if r is None:
            continue
        got = _run_engine(engine, table, 1, beam, **opts)
        _assert_same(got, r, beam)
        for s in range(len(r["origins"])):      # one beam dominates: every live beam continues from its slot
            if dom[s] >= 0:
                assert got[3][s, :beam].tolist() == [dom[s]] * beam, (s, got[3][s, :beam].tolist(), dom[s])
    print(_summary(f"{placement}, beam {beam}", stats))
    _assert_caps(stats, beam, n)


@pytest.mark.parametrize("placement", ["last_subchunk", "boundaries"])
def test_placed_candidates_in_the_51866_vocabulary(engine_v3, placement):
    """SL stays 811; the last sub-chunk ends at id 51865; every special id from <|translate|> up sits one higher (so do the suppressed ones)"""
    beam, V = 5, 51866
    stats, n = _new_stats(), 0
    for seed, table, dom, opts in _cases(placement, beam, V):
        n += 1
        r = _oracle_case(table, beam, dom, stats, **opts)
        if r is not None:
            _assert_same(_run_engine(engine_v3, table, 1, beam, **opts), r, beam)
    print(_summary(f"{placement}, beam {beam}, 51866 tokens", stats))
    _assert_caps(stats, beam, n)


# ---- exact ties (no skip rule: equal logits of one row are bit-equal on both sides, the row's normaliser and cumulative score are common) ----
def _spread_ids(rng, n, V, banned):
    """n ids in n different sub-chunks and n different lanes, returned in ascending order"""
    sl = _sl(V)
    while True:
        subs = sorted(rng.choice(SUB, size=n, replace=False).tolist())
        lanes = rng.choice(64, size=n, replace=False).tolist()
        ids = [s * sl + l + 64 * int(rng.integers(0, 12)) for s, l in zip(subs, lanes)]
        if all(i < V and i not in banned for i in ids):
            return ids


def test_equal_maxima_greedy_takes_the_lowest_id(engine):
    V, steps = 51865, 6
    banned = set(_suppress(V)) | {EOT, 220}
    checked = 0
    for seed in range(6):
        rng = np.random.default_rng(900 + seed)
        t = (0.5 * rng.standard_normal((steps, 1, V), dtype=np.float32) - 12.0).astype(np.float32)
        want = []
        for s in range(steps):
            ids = _spread_ids(rng, 2 + (s + seed) % 2, V, banned)
            t[s, 0, ids] = np.float32(1.25)
            t[s, 0, ids[0] + 1 if ids[0] + 1 not in banned else ids[0] + 3] = np.float32(0.9)      # a lower value next to the winner
            want.append(ids[0])
        table = np.ascontiguousarray(t)
        r = _run_oracle(table, 1)
        ids, sc, fin, par = _run_engine(engine, table, 1, 1)
        assert r["ids"] == want and ids[0] == want, (ids[0], r["ids"], want)
        assert fin[0] == r["finish_step"] == steps - 1
        checked += 1
    print(f"greedy, 2 - 3 equal maxima in different sub-chunks and lanes: {checked} searches identical to the oracle (0 skipped), lowest id at every step")


def _tie_table(seed, beam=5, V=51865, steps=7):
    """Every step's candidates come from ONE row (step 0: row 0 by construction; later steps: a random row d, the others flat as in placement
    "dominate"); that row's ladder is [a, a, b, b, c, d, ...]: two pairs of bit-equal logits inside the first k = 5 candidates, each pair's ids
    in different sub-chunks (and lanes), ranks k and k + 1 (c, d) >= 0.3 apart.  No EOT: every beam runs to the last step."""
    rng = np.random.default_rng(7000 + seed)
    banned = set(_suppress(V)) | {EOT, 220}
    n = 3 * beam + 2
    t = (0.02 * rng.standard_normal((steps, beam, V), dtype=np.float32) - 12.0).astype(np.float32)
    dom, pairs = [], []
    for s in range(steps):
        d = 0 if s == 0 else int(rng.integers(0, beam))
        dom.append(d)
        t[s, d] = (0.5 * rng.standard_normal(V, dtype=np.float32) - 12.0).astype(np.float32)
        lad = _ladder(rng, n - 2, 0.3, 0.08)
        tie = _spread_ids(rng, 4, V, banned)
        tie = [tie[i] for i in rng.permutation(4)]                  # which ids pair up: any two of the four
        rest = _pick(rng, 0, V, n - 4, banned | set(tie))
        t[s, d, tie[0]] = t[s, d, tie[1]] = lad[0]
        t[s, d, tie[2]] = t[s, d, tie[3]] = lad[1]
        t[s, d, rest] = lad[2:]
        t[s, d, EOT] = np.float32(-14.0)
        pairs.append((sorted(tie[:2]), sorted(tie[2:])))
    return np.ascontiguousarray(t), dom, pairs


def test_equal_candidates_take_slots_in_id_order(engine):
    beam, checked = 5, 0
    for seed in range(6):
        table, dom, pairs = _tie_table(seed, beam)
        for opts in (dict(), dict(patience=2.0)):
            r = _run_oracle(table, beam, **opts)
            # the ties sit inside the first k: no decision of a step rests on them (the last entry is the final ranking of the two equal best
            # hypotheses: the first registered wins on both sides, `score > best`)
            assert min(r["trace"][:-1]) >= 0.25 and r["trace"][-1] == 0.0, r["trace"]
            got = _run_engine(engine, table, 1, beam, **opts)
            _assert_same(got, r, beam)
            for s in range(1, len(r["origins"])):
                assert got[3][s, :beam].tolist() == [dom[s]] * beam
            # the token history follows the dominating slot of every step: slots 0 .. 3 hold the pairs in id order (a-low, a-high, b-low, b-high)
            for s in range(len(r["ids"]) - 1):
                d = dom[s + 1]
                if d < 4:
                    assert r["ids"][s] == pairs[s][d // 2][d % 2] == got[0][0][s], (s, d, r["ids"][s], got[0][0][s], pairs[s])
            assert got[0][0][-1] == pairs[len(r["ids"]) - 1][0][0]      # the last step's best of two equal hypotheses: the first registered, the lower id
            checked += 1
    print(f"beam {beam}, two pairs of equal candidates inside the first k: {checked} searches identical to the oracle (0 skipped), slots in id order")


# ---- fewer finite values than candidates ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("beam", [1, 5, 8])
def test_rows_with_fewer_finite_logits_than_candidates(engine, beam):
    """Every row holds f finite logits, f in {1, 2, k, 2k - 1}, the rest is -inf (never a row of -inf alone): the candidate list runs into -inf
    entries at every step.  ids, score, finish step and length as always; the ancestry only of beams whose cumulative score is finite."""
    V, steps = 51865, 6
    banned = set(_suppress(V)) | {EOT, 220}
    stats = _new_stats()
    for f in sorted({1, 2, beam, 2 * beam - 1}):
        for seed in range(5 if beam == 1 else 2):
            rng = np.random.default_rng([31, beam, f, seed])
            t = np.full((steps, beam, V), -np.inf, np.float32)
            for s in range(steps):
                for j in range(beam):
                    where = (_ids_scattered, _ids_one_subchunk, _ids_last_subchunk)[int(rng.integers(0, 3))]      # (the last sub-chunk's forced ids first)
                    ids = where(rng, max(f, 4), V, banned, s, j)[:f]
                    if f >= 2 and s >= 2 and rng.random() < 0.5:      # EOT among the finite values: hypotheses end while -inf candidates fill the list
                        ids[int(rng.integers(0, f))] = EOT
                    t[s, j, ids] = np.float32(0.11 * j) + _ladder(rng, f)[rng.permutation(f)]
            table = np.ascontiguousarray(t)
            for opts in ((dict(),) if beam == 1 else (dict(), dict(patience=2.0))):
                r = _oracle_case(table, beam, [-1] * steps, stats, **opts)
                if r is not None:
                    _assert_same(_run_engine(engine, table, 1, beam, **opts), r, beam, finite_only=True)
    print(_summary(f"f finite logits per row, beam {beam}", stats))
    assert stats["checked"] >= 8 and stats["skipped"] <= (stats["checked"] + stats["skipped"]) // 5, stats


# ---- fixed_new_tokens: EOT masked until `fixed_new` tokens exist, then forced -----------------------------------------------------------------
@pytest.mark.parametrize("fixed_new", [1, 6])
@pytest.mark.parametrize("beam", [1, 5])
def test_fixed_new_tokens_masks_then_forces_eot(engine, beam, fixed_new):
    checked = 0
    for seed in range(3):
        table, _ = _table("one_subchunk", beam, 50 + seed, steps=fixed_new + 3, eot_top=1.5)      # EOT is the row maximum from step 0 on
        assert all(table[s, j].argmax() == EOT for s in range(table.shape[0]) for j in range(beam))
        for opts in (dict(), dict(length_penalty=0.0)):      # (patience 2 asks for 2k hypotheses: the k forced EOTs of one step do not end that search)
            o = dict(opts, fixed_new_tokens=fixed_new)
            r = _run_oracle(table, beam, **o)
            got = _run_engine(engine, table, 1, beam, **o)
            ids, sc, fin, par = got
            assert EOT not in ids[0] and len(ids[0]) == fixed_new, ids[0]       # never taken before step fixed_new ...
            assert fin[0] == fixed_new == r["finish_step"], (fin[0], r["finish_step"])      # ... and every beam ends exactly there
            if min(r["trace"]) >= 2e-4:
                _assert_same(got, r, beam)
                checked += 1
    print(f"fixed_new_tokens {fixed_new}, beam {beam}: {checked} searches identical to the oracle ({6 - checked} compared on length and finish step only)")
    assert checked >= 4


if __name__ == "__main__":      # the oracle-only conditions of every (placement, beam), without a GPU
    ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path[:0] = [ROOT, os.path.join(ROOT, "willow-inference-server_amd")]
    for V, names, beams in ((51865, list(PLACEMENTS), (1, 5, 8)), (51866, ["last_subchunk", "boundaries"], (5,))):
        for placement in names:
            for beam in beams:
                stats, n = _new_stats(), 0
                for seed, table, dom, opts in _cases(placement, beam, V):
                    n += 1
                    _oracle_case(table, beam, dom, stats, **opts)
                print(_summary(f"[oracle only] V {V}, {placement}, beam {beam}", stats).replace("identical to the oracle", "checkable"), flush=True)
                _assert_caps(stats, beam, n)
