"""-m gpu: phrase_rules_mass_kernel (wis_op_phrase_mass) and phrase_mass_gather_kernel (wis_op_phrase_mass_gather) alone, on caller-supplied rows,
histories, tries and buffers.

THE MASK: the rows after wis_op_phrase_mass are bit for bit the rows after wis_op_phrase_rules on the same inputs (tests/test_gpu_phrase_ops.py's
scene and row patterns: -0.0, denormals, -inf, 3.4e38 - but no NaN inside [0, n_vocab), where the mass is unspecified; the pad holds +inf and
NaN), guard rows, pads and unowned rows included.
THE SLOTS: logmass [B][n_rec] starts as a canary (a NaN with a payload); exactly the slots of live on-trie rows change, every other slot keeps
the canary's bits - finished utterances, histories off the trie, beams j > 0 of a shared prompt row.
THE VALUES: against the float64 statement of the rule within the bound tests/phrase_mass_ref.py derives from the kernel's documented reduction
order, times its stated SAFETY = 2; where the value is exact by construction (-inf; exactly 0 when only allowed ids are finite) the bound is 0.
Each test prints its worst error / bound ratio."""
import numpy as np
import pytest

import phrase_mass_ref as R
from phrase_ref import allowed, prefix_dict
from test_gpu_phrase_ops import _children, _expect, _same_bits, _scene, _tap as _plain_tap, _token_pool

pytestmark = pytest.mark.gpu
EOT = 50257
NEG = float("-inf")
CANARY = 0x7FC0BEEF
WIS_E_ARG = -1


def _mass_tap(rows, V, eot, trie, alive, step_u, done, B, beam, lr, bias_all, bias_begin, sb):
    """-> (the rows after one launch, logmass u32 bits [B][n_rec] that started as the canary)"""
    from wis_hip import _lib
    lib = _lib.load()
    ld, max_new, n_rec = rows.shape[1], alive.shape[1], len(trie)
    lm = np.full((B, n_rec), CANARY, np.uint32)
    arrs = [rows, np.asarray(trie, np.int32), alive.astype(np.int32), np.asarray(step_u, np.int32), np.asarray(done, np.int32),
            np.asarray(bias_begin, np.float32), lm] + ([] if bias_all is None else [np.asarray(bias_all, np.float32)])
    bufs = [_lib.DevBuf.from_numpy(np.ascontiguousarray(a)) for a in arrs]
    try:
        _lib.check(lib.wis_op_phrase_mass(0, bufs[0].ptr, V, ld, eot, bufs[1].ptr, n_rec, bufs[2].ptr, bufs[3].ptr, bufs[4].ptr, B, beam, max_new, *lr,
                                          None if bias_all is None else bufs[7].ptr, bufs[5].ptr, sb, bufs[6].ptr))
        return bufs[0].to_numpy(np.float32, rows.shape), bufs[6].to_numpy(np.uint32, lm.shape)
    finally:
        for b in bufs:
            b.free()


def _record_of(trie, hist):
    """index of the record a history arrives at (0: the root), None off the trie"""
    at = 0
    for t in hist:
        first, n = int(trie[at, 1]), int(trie[at, 2])
        hit = np.nonzero(trie[first:first + n, 0] == t)[0] if n else []
        if len(hit) == 0:
            return None
        at = first + int(hit[0])
    return at


def _check_slots(rows, got_lm, V, eot, trie, prefixes, alive, step_u, done, B, beam, lr, bias_all, bias_begin, sb, ctx):
    """every slot: the value within the bound where a live on-trie row owns it, the canary's bits elsewhere -> worst error / bound"""
    want = {}
    for b in range(B):
        for j in range(beam):
            if done[b] or (lr[1] == 0 and j != 0):
                continue
            h = alive[b * beam + j, :min(int(step_u[b]), alive.shape[1])].tolist()
            keep = allowed(prefixes, h, eot)
            if keep is None:
                continue
            u = R.u_row(rows[b * lr[0] + j * lr[1] + lr[2], :V], bias_all, bias_begin, first=bool(sb) and step_u[b] == 0)
            key = (b, _record_of(trie, h))
            assert key not in want, (ctx, "two rows of one utterance at one node", key)
            want[key] = (R.logmass(u, keep), R.logmass_bound(u, keep))
    worst = 0.0
    got = got_lm.view(np.float32)
    for b in range(B):
        for r in range(len(trie)):
            if (b, r) not in want:
                assert got_lm[b, r] == CANARY, (ctx, b, r, hex(got_lm[b, r]))
                continue
            ref, bound = want[(b, r)]
            g = float(got[b, r])
            assert g == g and g <= 0.0, (ctx, b, r, g)
            if bound == 0.0:
                assert g == ref, (ctx, b, r, g, ref)
            else:
                assert abs(g - ref) <= R.SAFETY * bound, (ctx, b, r, g, ref, bound)
                worst = max(worst, abs(g - ref) / bound)
    assert want, ctx
    return worst, want


def _rows(rng, n, ld, V, scale=3.0):
    """test_gpu_phrase_ops' bit patterns, without NaN inside [0, V); the pad [V, ld) holds +inf and NaN"""
    x = (scale * rng.standard_normal((n, ld))).astype(np.float32)
    flat = x.reshape(-1)
    pick = rng.choice(flat.size, size=flat.size // 50, replace=False)
    special = np.array([-0.0, 0.0, 1e-42, -1e-42, -np.inf, 3.4e38], np.float32)
    flat[pick] = special[rng.integers(0, len(special), size=pick.size)]
    if ld > V:
        x[:, V:] = np.where(np.arange(ld - V) % 2 == 0, np.float32(np.inf), np.float32(np.nan))
    return x


def _biases(V, eot=EOT):
    from wis_hip import weights as W
    ba, bb = np.zeros(V, np.float32), np.zeros(V, np.float32)
    ba[[t for t in W.SUPPRESS_IDS if t < V]] = NEG
    bb[[t for t in W.SUPPRESS_IDS_BEGIN if t < V]] = NEG
    return ba, bb


@pytest.mark.parametrize("V", [51865, 51866])
@pytest.mark.parametrize("n_kids", [1, 255, 256, 257, 1500])
def test_mask_bits_slots_and_values(V, n_kids):
    """test_gpu_phrase_ops' scene (a phrase end with a child, the wide node of n_kids children, a leaf, a one-child node, the three ways off the
    trie, a finished utterance), its first utterance moved off the root (two own rows at ONE node would race for one slot: the engine's live
    beams never share a node); ld = n_vocab and a padded ld; the suppress lists on for the one, off for the other."""
    from wis_hip import weights as W
    rng = np.random.default_rng(2000 + n_kids + V)
    B, beam, max_new = 6, 2, 33
    worst = 0.0
    for ld, lists in ((V, True), ((V + 63) // 64 * 64, False)):
        phrases, hist, done = _scene(rng, V, n_kids, ld)
        deep = phrases[0]
        hist[0] = (2, deep[:2], [deep[0], int(_token_pool(V, EOT)[555])])      # one child, no EOT | off the trie at its last token
        trie, prefixes = W.build_phrase_trie(phrases), prefix_dict(phrases)
        alive = rng.integers(0, EOT, size=(B * beam, max_new)).astype(np.int32)
        step_u = []
        for b, (L, h0, h1) in enumerate(hist):
            alive[2 * b, :L], alive[2 * b + 1, :L] = h0, h1
            step_u.append(L)
        rows = _rows(rng, B * beam + 2, ld, V)
        rows[5, :V] = 3.4e38                                                     # (the leaf's row, every id equal: a sum of exp(0) terms)
        lr = (beam, 1, 1)                                                        # a guard row in front, one behind
        ba, bb = _biases(V)
        got_rows, got_lm = _mass_tap(rows, V, EOT, trie, alive, step_u, done, B, beam, lr, ba if lists else None, bb, 1)
        _same_bits(got_rows, _plain_tap(rows, V, EOT, trie, alive, step_u, done, B, beam, lr), (V, n_kids, ld, "vs wis_op_phrase_rules"))
        want_rows, masked = _expect(rows, V, EOT, prefixes, alive, step_u, done, B, beam, lr)
        _same_bits(got_rows, want_rows, (V, n_kids, ld, "vs the rule"))
        w, want = _check_slots(rows, got_lm, V, EOT, trie, prefixes, alive, step_u, done, B, beam, lr, ba if lists else None, bb, 1, (V, n_kids, ld))
        worst = max(worst, w)
        assert len(want) == len(masked) == (6 if n_kids >= 2 else 5), (want.keys(), masked)      # every masked row wrote its slot, nothing else did
    print(f"\n[phrase mass] V {V}, {n_kids} children: worst error / bound {worst:.3f}")


@pytest.mark.parametrize("n_kids", [1, 255, 256, 257, 1500])
def test_shared_prompt_row_step_0(n_kids):
    """lr_j = 0: the utterance's first workgroup masks the shared row and writes the ROOT's slot once; beams j > 0 and a finished utterance write
    nothing.  With and without suppress_blank: the begin list binds step 0 (a root child in it counts for nothing then)."""
    from wis_hip import weights as W
    V, B, beam = 51865, 3, 5
    rng = np.random.default_rng(70 + n_kids)
    pool = _token_pool(V, EOT)
    kids = _children(rng, pool, n_kids, V)
    phrases = [[t, int(pool[900])] for t in kids]
    trie, prefixes = W.build_phrase_trie(phrases), prefix_dict(phrases)
    alive = rng.integers(0, EOT, size=(B * beam, 8)).astype(np.int32)
    rows = _rows(rng, B * beam, V, V)
    ba, bb = _biases(V)
    bb[kids[0]] = NEG                    # (a tap caller's own begin list: masks an ALLOWED id at step 0)
    bb[int(pool[123])] = NEG
    worst = 0.0
    for lr, sb in (((beam, 0, 0), 1), ((beam, 0, 3), 0)):
        step_u, done = [0, 0, 0], [0, 1, 0]
        got_rows, got_lm = _mass_tap(rows, V, EOT, trie, alive, step_u, done, B, beam, lr, ba, bb, sb)
        _same_bits(got_rows, _plain_tap(rows, V, EOT, trie, alive, step_u, done, B, beam, lr), (n_kids, lr))
        w, want = _check_slots(rows, got_lm, V, EOT, trie, prefixes, alive, step_u, done, B, beam, lr, ba, bb, sb, (n_kids, lr, sb))
        assert sorted(want) == [(0, 0), (2, 0)]
        worst = max(worst, w)
    if n_kids == 1:                      # the one allowed id is in the begin list: -inf at step 0 with suppress_blank, a number without
        u1 = R.u_row(rows[0, :V], ba, bb, True)
        assert R.logmass(u1, [kids[0]]) == NEG and np.isfinite(R.logmass(R.u_row(rows[3, :V], ba, bb, False), [kids[0]]))
    print(f"\n[phrase mass] shared prompt row, {n_kids} children: worst error / bound {worst:.3f}")


def _small_scene(V):
    """eot = V - 1; a root with two children, one an interior phrase end with a child"""
    eot = V - 1
    a, b, c = 0, min(2, V - 2), 1
    trie = np.asarray([[-1, 1, 2, 0], [a, 3, 1, 1], [b, 0, 0, 1], [c, 0, 0, 1]], np.int32)      # phrases [a], [a, c], [b]
    return eot, trie, prefix_dict([[a], [a, c], [b]])


@pytest.mark.parametrize("V", [5, 255, 256, 257])
def test_small_vocabularies(V):
    """n_vocab 5: 251 threads own no element (their running maximum stays -inf: exp(-inf - -inf) must not appear); 255 / 256 / 257: around one
    element per thread.  ld = n_vocab and a padded ld whose pad holds +inf and NaN."""
    rng = np.random.default_rng(V)
    eot, trie, prefixes = _small_scene(V)
    B, beam = 4, 1
    alive = np.asarray([[0, 0], [0, 0], [min(2, V - 2), 0], [1, 0]], np.int32)      # root | [a] | [b] | off the trie
    step_u, done = [0, 1, 1, 1], [0, 0, 0, 0]
    worst = 0.0
    for ld in (V, V + 11):
        rows = _rows(rng, B + 2, ld, V)
        zero = np.zeros(V, np.float32)
        for sb in (0, 1):
            bb = zero.copy()
            bb[eot] = NEG
            got_rows, got_lm = _mass_tap(rows, V, eot, trie, alive, step_u, done, B, beam, (1, 1, 1), None, bb, sb)
            _same_bits(got_rows, _plain_tap(rows, V, eot, trie, alive, step_u, done, B, beam, (1, 1, 1)), (V, ld, sb))
            w, want = _check_slots(rows, got_lm, V, eot, trie, prefixes, alive, step_u, done, B, beam, (1, 1, 1), None, bb, sb, (V, ld, sb))
            assert sorted(want) == [(0, 0), (1, 1), (2, 2)]
            worst = max(worst, w)
    print(f"\n[phrase mass] n_vocab {V}: worst error / bound {worst:.3f}")


def test_value_edges():
    """One utterance per row, all at the node behind [a] (children c0, c1; the node ends a phrase: <|endoftext|> is allowed):
    0 allowed ids all -inf -> -inf | 1 only allowed ids finite -> exactly 0 | 2 the row all -inf -> -inf | 3, 4 logits of magnitude 1e4 (the best
    id outside / inside the set) | 5 an allowed id masked by the caller's own bias list | 6 every id equal | 7 the allowed ids 100 below the row's
    best (beyond fp32's exp range about the row maximum, not about their own) | 8 the suppress list takes the row's best id."""
    from wis_hip import weights as W
    V = 51865
    rng = np.random.default_rng(9)
    pool = _token_pool(V, EOT)
    a, c0, c1, out = (int(pool[i]) for i in (300, 40, 20000, 777))
    phrases = [[a], [a, c0], [a, c1]]
    trie, prefixes = W.build_phrase_trie(phrases), prefix_dict(phrases)
    keep = [c0, c1, EOT]
    B = 9
    rows = (3.0 * rng.standard_normal((B, V))).astype(np.float32)
    rows[0, keep] = NEG
    rows[1] = NEG; rows[1, keep] = [1.5, -2.0, 0.25]
    rows[2] = NEG
    rows[3] = (1e4 * rng.standard_normal(V)).astype(np.float32); rows[3, out] = 5e4
    rows[4] = (1e4 * rng.standard_normal(V)).astype(np.float32); rows[4, c1] = 5e4
    rows[6] = 0.125
    rows[7] = 0.0; rows[7, keep] = [-100.0, -101.0, -130.0]; rows[7, out] = 12.0
    ba, bb = _biases(V)
    ba[c0] = NEG                          # (no model's list holds a phrase token; a tap caller's may)
    sup = int(np.nonzero(np.isneginf(ba))[0][0])
    rows[8, sup] = 40.0
    alive = np.full((B, 4), a, np.int32)
    step_u, done = [1] * B, [0] * B
    got_rows, got_lm = _mass_tap(rows, V, EOT, trie, alive, step_u, done, B, 1, (1, 1, 0), ba, bb, 1)
    _same_bits(got_rows, _plain_tap(rows, V, EOT, trie, alive, step_u, done, B, 1, (1, 1, 0)), "value edges")
    worst, want = _check_slots(rows, got_lm, V, EOT, trie, prefixes, alive, step_u, done, B, 1, (1, 1, 0), ba, bb, 1, "value edges")
    at = _record_of(trie, [a])
    ref = {b: want[(b, at)][0] for b in range(B)}
    assert ref[0] == NEG and ref[1] == 0.0 and ref[2] == NEG and want[(1, at)][1] == 0.0
    assert ref[3] < -1e4 and -1e-3 < ref[4] <= 0.0 and np.isfinite(ref[3])
    assert abs(ref[6] - np.log(2.0 / (V - int(np.isneginf(ba).sum())))) < 1e-9      # c0 is masked: two of the unmasked ids
    assert -114.0 < ref[7] < -112.0                                                  # (c0 is masked: -101 and -130 under a row whose log-sum is 12.3)
    u5 = R.u_row(rows[5], ba, bb, False)
    assert u5[c0] == NEG and abs(ref[5] - R.logmass(u5, [c1, EOT])) == 0.0          # the masked allowed id counts for nothing
    assert ref[8] > R.logmass(rows[8], keep) + 20.0                                  # ... and a suppressed id is no part of the denominator
    print(f"\n[phrase mass] value edges: worst error / bound {worst:.3f}; values {[round(ref[b], 4) for b in range(B)]}")


def _gather(ids, lens, score, trie, lm, B, n):
    from wis_hip import _lib
    lib = _lib.load()
    arrs = [np.asarray(ids, np.int32), np.asarray(lens, np.int32), np.asarray(trie, np.int32), np.asarray(lm, np.float32), np.zeros(B * n, np.float32)]
    if score is not None:
        arrs.append(np.asarray(score, np.float32))
    bufs = [_lib.DevBuf.from_numpy(np.ascontiguousarray(a)) for a in arrs]
    try:
        _lib.check(lib.wis_op_phrase_mass_gather(0, bufs[0].ptr, bufs[1].ptr, None if score is None else bufs[5].ptr, bufs[2].ptr, len(trie), bufs[3].ptr,
                                                 B, n, arrs[0].shape[1], bufs[4].ptr))
        return bufs[4].to_numpy(np.float32, (B, n))
    finally:
        for b in bufs:
            b.free()


def test_gather():
    """paths of 1 and 32 tokens, an interior phrase end, a filler, three non-paths (a token that is no child, a prefix that ends no phrase, the empty
    result), a length beyond the table; a NaN slot propagates; utterance b reads ITS slots.  The sum is the fp32 sum in path order: exact."""
    from wis_hip import weights as W
    rng = np.random.default_rng(21)
    pool = _token_pool(51865, EOT)
    deep = rng.choice(pool[1000:], size=32, replace=False).tolist()
    one = int(pool[50])
    phrases = [deep, deep[:3], [one], [one, int(pool[60])] + deep[:2]]
    trie = W.build_phrase_trie(phrases)
    n_rec, B, n, id_ld = len(trie), 2, 5, 40
    lm = -(10.0 * rng.random((B, n_rec))).astype(np.float32)
    lm[1, _record_of(trie, deep[:2])] = np.nan
    res = [deep, deep[:3], [one], deep[:2], deep[:4] + [one]]                     # per utterance: 32 tokens, interior end, 1 token, no phrase end, no child
    ids = rng.integers(0, EOT, size=(B * n, id_ld)).astype(np.int32)
    lens = np.zeros(B * n, np.int32)
    for b in range(B):
        for i, ph in enumerate(res):
            ids[b * n + i, :len(ph)] = ph
            lens[b * n + i] = len(ph)
    score = -rng.random(B * n).astype(np.float32)
    got = _gather(ids, lens, score, trie, lm, B, n)

    def path_sum(b, ph):
        acc = np.float32(lm[b, 0])
        for i in range(len(ph)):
            acc = np.float32(acc + lm[b, _record_of(trie, ph[:i + 1])])
        return acc
    for b in range(B):
        for i, ph in enumerate(res[:3]):
            want = path_sum(b, ph)
            if b == 1 and len(ph) >= 2:
                assert np.isnan(got[b, i]) and np.isnan(want), (b, i, got[b, i])  # the NaN slot lies on deep's path behind its second token
            else:
                assert got[b, i] == want and np.isfinite(want), (b, i, got[b, i], want)
        assert got[b, 3] == NEG and got[b, 4] == NEG, got[b]
    assert got[1, 2] == path_sum(1, [one]) and got[1, 2] != got[0, 2]
    # a filler (score -inf: whatever its ids), the empty result, a length past the table / the ids' stride
    score2 = score.copy(); score2[0] = NEG
    lens2 = lens.copy(); lens2[1] = 0; lens2[2] = 33; lens2[7] = -1
    got2 = _gather(ids, lens2, score2, trie, lm, B, n)
    assert got2[0, 0] == NEG and got2[0, 1] == NEG and got2[0, 2] == NEG and got2[1, 2] == NEG and got2[1, 0] != got2[1, 0]
    assert _gather(ids, lens, None, trie, lm, B, n).tobytes() == got.tobytes()    # no scores: nothing is a filler


def test_argument_checks():
    from wis_hip import _lib
    lib = _lib.load()
    d = _lib.DevBuf(4096)
    try:
        for V, ld, eot, n_rec, B, beam, max_new in ((100, 50, 10, 1, 1, 1, 4), (100, 100, 100, 1, 1, 1, 4), (100, 100, 10, 0, 1, 1, 4), (100, 100, 10, 70000, 1, 1, 4),
                                                    (100, 100, 10, 1, 0, 1, 4), (100, 100, 10, 1, 1, 9, 4), (100, 100, 10, 1, 13, 8, 4), (100, 100, 10, 1, 1, 1, 0),
                                                    (100, 100, 10, 1, 1, 1, 257), (65537, 65537, 10, 1, 1, 1, 4)):
            rc = lib.wis_op_phrase_mass(0, d.ptr, V, ld, eot, d.ptr, n_rec, d.ptr, d.ptr, d.ptr, B, beam, max_new, 1, 1, 0, None, d.ptr, 1, d.ptr)
            assert rc == WIS_E_ARG, (V, ld, eot, n_rec, B, beam, max_new, rc)
        assert lib.wis_op_phrase_mass(0, d.ptr, 100, 100, 10, d.ptr, 1, d.ptr, d.ptr, d.ptr, 1, 1, 4, 1, 1, 0, None, None, 1, d.ptr) == WIS_E_ARG      # no begin list
        assert lib.wis_op_phrase_mass(0, d.ptr, 100, 100, 10, d.ptr, 1, d.ptr, d.ptr, d.ptr, 1, 1, 4, 1, 1, 0, None, d.ptr, 1, None) == WIS_E_ARG       # no buffer
        for n_rec, B, n, id_ld in ((0, 1, 1, 4), (70000, 1, 1, 4), (1, 0, 1, 4), (1, 1, 0, 4), (1, 13, 8, 4), (1, 1, 1, 0), (1, 1, 1, 257)):
            assert lib.wis_op_phrase_mass_gather(0, d.ptr, d.ptr, None, d.ptr, n_rec, d.ptr, B, n, id_ld, d.ptr) == WIS_E_ARG, (n_rec, B, n, id_ld)
        assert lib.wis_op_phrase_mass_gather(0, None, d.ptr, None, d.ptr, 1, d.ptr, 1, 1, 4, d.ptr) == WIS_E_ARG
    finally:
        d.free()
