"""-m gpu: hotword_rules_kernel alone (wis_op_hotword_rules) on caller-supplied rows, histories, step counters and done flags, BIT FOR BIT against
the brute-force statement of THE HOTWORD RULE (tests/hotword_ref.py boost_rows): the rule is one float32 addition per element of the boost set,
so there is no tolerance (a NaN is compared by isnan).  Every element the rule does not name keeps its bits: the pad [n_vocab, ld), the rows of
finished utterances, every other row, and a guard row in front of and behind the rows the call owns.
Shapes: vocabularies 51865 and 51866 on a padded stride and a small one whose rows start off 16-byte boundaries; 1, 5 and 96 rows; histories of 0,
1, 30, 31, 32, 33, 255 and 256 tokens and a step counter past the buffer; sets with one one-token entry, one 32-token entry, a root of 4096
children, a node of 257, 65535 records, nested and self-overlapping entries; -inf, +inf, NaN, a denormal and -0.0 under the boost; histories that
hold -1 and ids >= n_vocab.  No malformed table reaches the kernel: the tap validates on the host and answers WIS_E_ARG."""
import numpy as np
import pytest

from hotword_ref import boost_rows, boost_set
from phrase_ref import prefix_dict

pytestmark = pytest.mark.gpu
EOT = 50257
WIS_E_ARG = -1
LENGTHS = [0, 1, 30, 31, 32, 33, 255, 256]


def _tap(rows, V, eot, trie, alive, step_u, done, B, beam, lr, boost, fixed_new=0, rc_only=False):
    """rows f32 [n][ld] -> the rows after one launch"""
    from wis_hip import _lib
    lib = _lib.load()
    ld, max_new = rows.shape[1], alive.shape[1]
    trie = np.ascontiguousarray(np.asarray(trie, np.int32).reshape(-1, 4))
    bufs = [_lib.DevBuf.from_numpy(np.ascontiguousarray(a)) for a in (rows, trie, alive.astype(np.int32), np.asarray(step_u, np.int32), np.asarray(done, np.int32))]
    try:
        rc = lib.wis_op_hotword_rules(0, bufs[0].ptr, V, ld, eot, bufs[1].ptr, len(trie), bufs[2].ptr, bufs[3].ptr, bufs[4].ptr, B, beam, max_new, fixed_new,
                                      float(boost), *lr)
        if rc_only:
            return rc, bufs[0].to_numpy(np.float32, rows.shape)
        _lib.check(rc)
        return bufs[0].to_numpy(np.float32, rows.shape)
    finally:
        for b in bufs:
            b.free()


def _expect(rows, V, eot, prefixes, alive, step_u, done, B, beam, lr, boost, fixed_new=0):
    """-> (the rows the rule asks for, {row: size of its boost set})"""
    out, sizes = rows.copy(), {}
    max_new = alive.shape[1]
    for b in range(B):
        for j in range(beam):
            L = min(int(step_u[b]), max_new)
            if done[b] or (lr[1] == 0 and j != 0) or (fixed_new > 0 and L >= fixed_new):
                continue
            r = b * lr[0] + j * lr[1] + lr[2]
            h = alive[b * beam + j, :L].tolist()
            out[r:r + 1, :V] = boost_rows(out[r:r + 1, :V], [h], prefixes, boost, V, eot)
            sizes[r] = len(boost_set(prefixes, h, V, eot))
    return out, sizes


def _same(got, want, ctx):
    gn, wn = np.isnan(got), np.isnan(want)
    g, w = got.view(np.uint32), want.view(np.uint32)
    bad = (gn != wn) | (~wn & (g != w))
    if bad.any():
        at = np.argwhere(bad)
        raise AssertionError((ctx, len(at), at[:8].tolist(), got[tuple(at[0])], want[tuple(at[0])]))


def _rows(rng, n, ld):
    """random rows sprinkled with the values an addition must treat by IEEE's book"""
    x = (3.0 * rng.standard_normal((n, ld))).astype(np.float32)
    flat = x.reshape(-1)
    pick = rng.choice(flat.size, size=flat.size // 40, replace=False)
    special = np.array([-0.0, 0.0, 1e-42, -1e-42, -np.inf, np.inf, 3.4e38, np.nan], np.float32)
    flat[pick] = special[rng.integers(0, len(special), size=pick.size)]
    return x


def _pool(eot=EOT):
    from wis_hip import weights as W
    bad = set(W.SUPPRESS_IDS) | set(W.SUPPRESS_IDS_BEGIN)
    return [t for t in range(eot) if t not in bad]


def _scene(rng, pool):
    """A set over a five-token alphabet (suffixes overlap, repeat and nest) beside a wide root, a node of 257 children, a 32-token entry and a
    one-token entry; and a generator of histories of a given length that END inside the set in several ways at once."""
    alpha = [int(t) for t in rng.choice(pool[:3000], size=5, replace=False)]
    a, b, c = alpha[:3]
    entries = [[a, b], [a, b, c], [a, a, b], [c], [a, c], [b, a, c], [alpha[3], b, a, c]]
    entries += [rng.choice(alpha, size=int(rng.integers(2, 7))).tolist() for _ in range(12)]
    deep = [int(t) for t in rng.choice(pool[3000:6000], size=32, replace=False)]
    fan = int(pool[7000])
    entries += [deep, [int(pool[6500])]] + [[fan, int(t)] for t in pool[8000:8257]] + [[int(t)] for t in pool[10000:10000 + 600]]
    far = int(pool[9000])      # a token that starts nothing

    def history(L, kind):
        if L == 0:
            return []
        body = rng.choice(alpha, size=L).tolist()                   # dense in the alphabet: several suffixes are active
        if kind == 1:
            body[-min(L, 31):] = deep[:min(L, 31)]                  # the longest suffix that counts, down the 32-token entry
        elif kind == 2:
            body[-1] = fan                                          # the node of 257 children
        elif kind == 3 and L >= 3:
            body[-3:] = [a, a, a]                                   # the self-overlapping entry
        elif kind == 4:
            body[-min(L, 2)] = -1 if L % 2 else 60000               # an id outside the vocabulary near the end: the suffixes break there
        elif kind == 5:
            body[-1] = far
        return [int(t) for t in body]
    return entries, history, dict(a=a, b=b, c=c, deep=deep, fan=fan)


@pytest.mark.parametrize("B,beam", [(1, 1), (1, 5), (12, 8)])
@pytest.mark.parametrize("V,ld,eot", [(51865, 51904, EOT), (51866, 51904, EOT), (12003, 12003, 12000)])
def test_boost_bit_for_bit(V, ld, eot, B, beam):
    """1, 5 and 96 rows; the small vocabulary's odd stride puts the rows on every 4-byte phase of a 16-byte line"""
    from wis_hip import weights as W
    rng = np.random.default_rng(V + 17 * B + beam)
    small = V < 50000
    pool = list(range(1, eot)) if small else _pool()
    entries, history, names = _scene(rng, pool)
    kw = dict(eot=eot, suppress_ids=[], suppress_begin=[]) if small else {}
    trie, prefixes = W.build_hotword_trie(entries, **kw), prefix_dict(entries)
    max_new, boost = 256, 2.5
    lr = (beam, 1, 1)                                                  # a guard row in front, one behind
    # utterance b takes LENGTHS[b]; utterance 8 a counter past the buffer, utterance 9 is finished; a single utterance runs every length in turn
    plans = [[L] for L in LENGTHS + [300]] if B == 1 else [(LENGTHS + [300, 31, 5, 33])[:B]]
    seen_sizes = []
    n_root = len(prefixes[()][0])
    assert n_root > 256                                                # (the root's children take more than one 256-wide round)
    for pi, plan in enumerate(plans):
        alive = rng.integers(0, eot, size=(B * beam, max_new)).astype(np.int32)      # (entries behind the history are garbage on purpose)
        done = [int(B > 1 and b == 9) for b in range(B)]
        for b, Lb in enumerate(plan):
            L = min(Lb, max_new)
            for j in range(beam):
                alive[b * beam + j, :L] = history(L, (b + j + pi) % 6)
        rows = _rows(rng, B * beam + 2, ld)
        got = _tap(rows, V, eot, trie, alive, plan, done, B, beam, lr, boost)
        want, sizes = _expect(rows, V, eot, prefixes, alive, plan, done, B, beam, lr, boost)
        _same(got, want, (V, ld, B, beam, plan))
        assert set(sizes) == {b * beam + j + 1 for b in range(B) for j in range(beam) if not done[b]}
        assert min(sizes.values()) >= n_root                           # the root's children are in every boost set
        seen_sizes += list(sizes.values())
    assert max(seen_sizes) > n_root                                    # some histories reached beyond the root


def test_fixed_sets():
    """The issue's list, one launch each on a single row; the boost set's size is asserted on the reference, the bits on the kernel."""
    from wis_hip import weights as W
    V, ld = 51865, 51904
    rng = np.random.default_rng(5)
    pool = _pool()
    a, b, c, x = (int(pool[i]) for i in (400, 401, 402, 999))
    chain = [int(t) for t in pool[100:132]]
    wide = [[int(t)] for t in pool[:4096]]
    node257 = [[a, int(t)] for t in pool[2000:2257]]
    big = [[int(f), int(s)] for f in pool[:62] for s in pool[5000:6056]]
    cases = [
        ("one one-token entry", [[a]], [x, x], 1),
        ("one 32-token entry, followed to its last token", [chain], [x] * 9 + chain[:31], 2),
        ("one 32-token entry, completed", [chain], chain, 1),
        ("a root of 4096 children", wide, [x], 4096),
        ("a node of 257 children", node257, [x, a], 258),
        ("65535 records", big, [x, int(pool[61])], 62 + 1056),
        ("[a, b] beside [a, b, c]: c is boosted, <|endoftext|> is not", [[a, b], [a, b, c]], [x, a, b], 2),
        ("[a, a, b] under a a a: a is named twice, boosted once", [[a, a, b]], [x, a, a, a], 2),
        ("a token named by three suffixes", [[c], [a, c], [b, a, c]], [x, b, a], 3),
        ("-1 in the history", [[a, b, c], [b, x]], [a, -1, b], 3),
        ("an id >= n_vocab in the history", [[a, b, c], [b, x]], [a, V, b], 3),
        ("the last id >= n_vocab", [[a, b, c]], [a, b, 2 ** 31 - 1], 1),
    ]
    assert len(W.build_hotword_trie(big)) == 65535
    for what, entries, hist, n_boosted in cases:
        trie, prefixes = W.build_hotword_trie(entries), prefix_dict(entries)
        alive = np.full((1, 64), 7, np.int32)
        alive[0, :len(hist)] = hist
        rows = _rows(rng, 3, ld)
        got = _tap(rows, V, EOT, trie, alive, [len(hist)], [0], 1, 1, (1, 1, 1), 2.5)
        want, sizes = _expect(rows, V, EOT, prefixes, alive, [len(hist)], [0], 1, 1, (1, 1, 1), 2.5)
        assert sizes == {1: n_boosted}, (what, sizes)
        _same(got, want, what)
        assert np.array_equal(got[1, EOT:].view(np.uint32), rows[1, EOT:].view(np.uint32)), what      # <|endoftext|> and everything above it
    # x + boost, never x + 2 boost - on known values
    trie = W.build_hotword_trie([[a, a, b]])
    rows = np.zeros((1, ld), np.float32)
    alive = np.asarray([[x, a, a, a]], np.int32)
    got = _tap(rows, V, EOT, trie, alive, [4], [0], 1, 1, (1, 1, 0), 2.5)
    assert got[0, a] == np.float32(2.5) and got[0, b] == np.float32(2.5) and np.count_nonzero(got) == 2


def test_values_under_the_boost():
    """-inf, +inf, NaN, a denormal, -0.0 and the largest finite value at boosted ids: one IEEE addition each"""
    from wis_hip import weights as W
    V, ld = 51865, 51904
    pool = _pool()
    ids = [int(t) for t in pool[300:307]]
    vals = np.asarray([-np.inf, np.inf, np.nan, 1e-42, -0.0, 3.4e38, -2.5], np.float32)
    trie, prefixes = W.build_hotword_trie([[t] for t in ids]), prefix_dict([[t] for t in ids])
    rows = np.zeros((1, ld), np.float32)
    rows[0, ids] = vals
    for boost in (2.5, 2.0 ** -60, 3.0e38):
        got = _tap(rows, V, EOT, trie, np.zeros((1, 4), np.int32), [0], [0], 1, 1, (1, 1, 0), boost)
        want, _ = _expect(rows, V, EOT, prefixes, np.zeros((1, 4), np.int32), [0], [0], 1, 1, (1, 1, 0), boost)
        _same(got, want, boost)
        assert np.isneginf(got[0, ids[0]]) and np.isposinf(got[0, ids[1]]) and np.isnan(got[0, ids[2]])
    got = _tap(rows, V, EOT, trie, np.zeros((1, 4), np.int32), [0], [0], 1, 1, (1, 1, 0), 2.5)
    assert got[0, ids[3]] == np.float32(2.5) and got[0, ids[4]] == np.float32(2.5) and got[0, ids[6]] == 0.0 and not np.signbit(got[0, ids[6]])


def test_shared_first_step_row():
    """lr_j = 0 (the pass that carries the prompt): the beams of an utterance share ONE row; the utterance's first workgroup boosts the root's
    children ONCE - five workgroups adding would leave x + 5 boost -, the other rows of the block are not written, a finished utterance's neither."""
    from wis_hip import weights as W
    V, B, beam = 51865, 3, 5
    rng = np.random.default_rng(8)
    pool = _pool()
    entries = [[int(t), int(pool[900])] for t in rng.choice(pool, size=300, replace=False)]
    trie, prefixes = W.build_hotword_trie(entries), prefix_dict(entries)
    alive = rng.integers(0, EOT, size=(B * beam, 8)).astype(np.int32)
    rows = _rows(rng, B * beam, V)
    for lr in ((beam, 0, 0), (beam, 0, 3)):
        got = _tap(rows, V, EOT, trie, alive, [0, 0, 0], [0, 1, 0], B, beam, lr, 1.5)
        want, sizes = _expect(rows, V, EOT, prefixes, alive, [0, 0, 0], [0, 1, 0], B, beam, lr, 1.5)
        assert sizes == {lr[2]: 300, 2 * beam + lr[2]: 300}, sizes
        _same(got, want, lr)


def test_forced_eot_step_is_left_alone():
    """fixed_new_tokens: on the forced-EOT step (L >= fixed_new) nothing is done, as in rep_rules_kernel; one step earlier the boost applies"""
    from wis_hip import weights as W
    V = 51865
    rng = np.random.default_rng(9)
    a = int(_pool()[400])
    trie, prefixes = W.build_hotword_trie([[a]]), prefix_dict([[a]])
    alive = np.full((2, 8), 7, np.int32)
    rows = _rows(rng, 2, V)
    rows[:, a] = 1.0
    got = _tap(rows, V, EOT, trie, alive, [3, 4], [0, 0], 2, 1, (1, 1, 0), 2.0, fixed_new=4)
    want, sizes = _expect(rows, V, EOT, prefixes, alive, [3, 4], [0, 0], 2, 1, (1, 1, 0), 2.0, fixed_new=4)
    assert sizes == {0: 1} and want[0, a] == 3.0 and want[1, a] == 1.0
    _same(got, want, "forced EOT")


def test_malformed_tables_are_refused_on_the_host():
    """The tap reads the table back and runs the engine's validator: WIS_E_ARG, nothing launched, the rows keep their bits."""
    V = 51865
    rng = np.random.default_rng(10)
    rows = _rows(rng, 2, V)
    alive = np.asarray([[100], [100]], np.int32)
    ok = [[-1, 1, 2, 0], [400, 3, 1, 0], [500, 0, 0, 1], [401, 0, 0, 1]]
    rc, got = _tap(rows, V, EOT, ok, alive, [1, 1], [0, 0], 2, 1, (1, 1, 0), 2.0, rc_only=True)
    assert rc == 0 and not np.array_equal(got.view(np.uint32), rows.view(np.uint32))
    bad_tables = {
        "the root claims 5 children, the table holds 1": [[-1, 1, 5, 0], [100, 0, 0, 1]],
        "a child range that starts at n_rec": [[-1, 1, 1, 0], [100, 2, 1, 0]],
        "a negative range": [[-1, 1, 1, 0], [100, -7, 3, 0]],
        "more children than a node may have": [[-1, 1, 1, 0], [100, 1, 70000, 0]],
        "unsorted children": [[-1, 1, 2, 0], [500, 0, 0, 1], [400, 0, 0, 1]],
        "a leaf that ends nothing": [[-1, 1, 1, 0], [400, 0, 0, 0]],
        "<|endoftext|> as a token": [[-1, 1, 1, 0], [EOT, 0, 0, 1]],
        "a token beyond the vocabulary": [[-1, 1, 1, 0], [V + 5, 0, 0, 1]],
        "a root token": [[5, 1, 1, 0], [400, 0, 0, 1]],
        "an orphan record": ok + [[700, 0, 0, 1]],
        "a cycle": [[-1, 1, 1, 0], [400, 1, 1, 0]],
    }
    for what, table in bad_tables.items():
        rc, got = _tap(rows, V, EOT, table, alive, [1, 1], [0, 0], 2, 1, (1, 1, 0), 2.0, rc_only=True)
        assert rc == WIS_E_ARG, (what, rc)
        assert np.array_equal(got.view(np.uint32), rows.view(np.uint32)), what


def test_argument_checks():
    from wis_hip import _lib
    lib = _lib.load()
    d = _lib.DevBuf(64)
    try:
        for V, ld, eot, n_rec, B, beam, max_new, fixed_new, boost in (
                (100, 50, 10, 1, 1, 1, 4, 0, 1.0), (100, 100, 100, 1, 1, 1, 4, 0, 1.0), (100, 100, 10, 0, 1, 1, 4, 0, 1.0), (100, 100, 10, 70000, 1, 1, 4, 0, 1.0),
                (100, 100, 10, 1, 0, 1, 4, 0, 1.0), (100, 100, 10, 1, 1, 9, 4, 0, 1.0), (100, 100, 10, 1, 13, 8, 4, 0, 1.0), (100, 100, 10, 1, 1, 1, 0, 0, 1.0),
                (100, 100, 10, 1, 1, 1, 257, 0, 1.0), (100, 100, 10, 1, 1, 1, 4, -1, 1.0), (70000, 70000, 10, 1, 1, 1, 4, 0, 1.0),
                (100, 100, 10, 1, 1, 1, 4, 0, 0.0), (100, 100, 10, 1, 1, 1, 4, 0, -1.0), (100, 100, 10, 1, 1, 1, 4, 0, float("inf")), (100, 100, 10, 1, 1, 1, 4, 0, float("nan"))):
            rc = lib.wis_op_hotword_rules(0, d.ptr, V, ld, eot, d.ptr, n_rec, d.ptr, d.ptr, d.ptr, B, beam, max_new, fixed_new, boost, 1, 1, 0)
            assert rc == WIS_E_ARG, (V, ld, eot, n_rec, B, beam, max_new, fixed_new, boost, rc)
        assert lib.wis_op_hotword_rules(0, None, 100, 100, 10, d.ptr, 1, d.ptr, d.ptr, d.ptr, 1, 1, 4, 0, 1.0, 1, 1, 0) == WIS_E_ARG
    finally:
        d.free()
