"""-m gpu: phrase_rules_kernel alone (wis_op_phrase_rules) on caller-supplied rows, histories, step counters and done flags, ELEMENT BY
ELEMENT against the dict-of-prefixes statement of the rule (tests/phrase_ref.py):
  allowed ids keep their bits (the rows hold -0.0, denormals, -inf and a NaN payload on purpose), every other id of [0, n_vocab) is exactly
  -inf, the pad [n_vocab, ld) and every row the call does not own (a guard row on either side, the rows of finished utterances, rows whose
  history leaves the trie) keep their bits.
Shapes: a node's children are scanned 256 per round, so 1, 255, 256, 257 and 1500 children - at the root and one level down; children at ids
0, 3, 4 and eot - 1 and around the row's float4 boundaries (the fill is a scalar head, float4 body, scalar tail; the row stride decides the
alignment: ld = n_vocab puts every second row on another phase, a padded ld keeps them aligned); histories of 0, 1 and 32 tokens; both
vocabularies."""

import numpy as np
import pytest

from phrase_ref import allowed, prefix_dict

pytestmark = pytest.mark.gpu
EOT = 50257
WIS_E_ARG = -1


def _tap(rows, V, eot, trie, alive, step_u, done, B, beam, lr):
    """rows f32 [n][ld] -> the rows after one launch"""
    from wis_hip import _lib
    lib = _lib.load()
    ld, max_new = rows.shape[1], alive.shape[1]
    bufs = [_lib.DevBuf.from_numpy(np.ascontiguousarray(a)) for a in (rows, np.asarray(trie, np.int32), alive.astype(np.int32), np.asarray(step_u, np.int32),
                                                                      np.asarray(done, np.int32))]
    try:
        _lib.check(lib.wis_op_phrase_rules(0, bufs[0].ptr, V, ld, eot, bufs[1].ptr, len(trie), bufs[2].ptr, bufs[3].ptr, bufs[4].ptr, B, beam, max_new, *lr))
        return bufs[0].to_numpy(np.float32, rows.shape)
    finally:
        for b in bufs:
            b.free()


def _expect(rows, V, eot, prefixes, alive, step_u, done, B, beam, lr):
    out = rows.copy()
    max_new = alive.shape[1]
    masked = []
    for b in range(B):
        for j in range(beam):
            if done[b] or (lr[1] == 0 and j != 0):
                continue
            L = min(int(step_u[b]), max_new)
            keep = allowed(prefixes, alive[b * beam + j, :L].tolist(), eot)
            if keep is None:
                continue
            r = b * lr[0] + j * lr[1] + lr[2]
            vals = rows[r, keep].copy()
            out[r, :V] = -np.inf
            out[r, keep] = vals
            masked.append((r, len(keep)))
    return out, masked


def _same_bits(got, want, ctx):
    g, w = got.view(np.uint32), want.view(np.uint32)
    if not np.array_equal(g, w):
        bad = np.argwhere(g != w)
        raise AssertionError((ctx, len(bad), bad[:8].tolist(), got[tuple(bad[0])], want[tuple(bad[0])]))


def _rows(rng, n, ld):
    """random rows with the bit patterns a mask must not disturb"""
    x = (3.0 * rng.standard_normal((n, ld))).astype(np.float32)
    flat = x.reshape(-1)
    pick = rng.choice(flat.size, size=flat.size // 50, replace=False)
    special = np.array([-0.0, 0.0, 1e-42, -1e-42, -np.inf, 3.4e38], np.float32)
    flat[pick] = special[rng.integers(0, len(special), size=pick.size)]
    flat.view(np.uint32)[rng.choice(flat.size, size=64, replace=False)] = 0x7FC12345      # a NaN with a payload
    return x


def _token_pool(V, eot):
    from wis_hip import weights as W
    bad = set(W.SUPPRESS_IDS) | set(W.SUPPRESS_IDS_BEGIN)
    return [t for t in range(eot) if t not in bad]


def _children(rng, pool, n, ld, must=()):
    """n distinct ids: `must`, the ids around the float4 boundaries of rows of stride ld (both phases), the rest random"""
    edge = [0, 3, 4, 5, EOT - 1, EOT - 2]
    for base in (4096, 20000):
        for ph in range(4):                      # row r starts at element r * ld: its phase is (r * ld) % 4
            edge += [base + ph - 1, base + ph, base + ph + 3, base + ph + 4]
    ok = set(pool)
    first = [t for t in dict.fromkeys(list(must) + edge) if t in ok][:n]
    rest = rng.permutation([t for t in pool if t not in set(first)])[:n - len(first)].tolist()
    return sorted(first + rest)


def _scene(rng, V, n_kids, ld):
    """The phrase set and the histories of one call: B = 6 utterances x beam 2"""
    pool = _token_pool(V, EOT)
    deep = rng.choice(pool[1000:], size=32, replace=False).tolist()             # D: a 32-token phrase; D[:1] is a phrase too (an interior end)
    fan = int(pool[777])                                                        # [fan, c] for n_kids different c: a wide node one level down
    x = int(pool[555])                                                          # a token no phrase holds at the places it is put
    kids = _children(rng, pool, n_kids, ld)
    firsts = _children(rng, [t for t in pool if t != x], n_kids, ld, must=[deep[0], fan] if n_kids >= 2 else [deep[0]])
    phrases = [deep, deep[:1]] + [[fan, c] for c in kids if n_kids >= 2] + [[t] for t in firsts if t not in (deep[0], fan)]
    assert x not in deep and x != fan and x not in firsts
    hist = [
        (0, [], []),                                                            # the root, twice (own rows: lr_j = 1)
        (1, deep[:1], [fan] if n_kids >= 2 else [x]),                           # a phrase end with a child: d1 and EOT | the wide node, no EOT (or: off the trie)
        (32, deep, deep[:31] + [x]),                                            # a leaf: EOT alone | leaves the trie at its LAST token
        (5, deep[:5], [x] + deep[1:5]),                                         # one child, no EOT | leaves at its FIRST token
        (5, deep[:2] + [x] + deep[3:5], deep[:5]),                              # leaves in the MIDDLE | on the path
        (5, deep[:5], deep[:5]),                                                # a finished utterance
    ]
    return phrases, hist, [0, 0, 0, 0, 0, 1]


@pytest.mark.parametrize("V", [51865, 51866])
@pytest.mark.parametrize("n_kids", [1, 255, 256, 257, 1500])
def test_mask_element_by_element(V, n_kids):
    from wis_hip import weights as W
    rng = np.random.default_rng(1000 + n_kids + V)
    B, beam, max_new = 6, 2, 33
    for ld in (V, (V + 63) // 64 * 64):
        phrases, hist, done = _scene(rng, V, n_kids, ld)
        trie, prefixes = W.build_phrase_trie(phrases), prefix_dict(phrases)
        alive = rng.integers(0, EOT, size=(B * beam, max_new)).astype(np.int32)      # (entries behind the history are garbage on purpose)
        step_u = []
        for b, (L, h0, h1) in enumerate(hist):
            alive[2 * b, :L], alive[2 * b + 1, :L] = h0, h1
            step_u.append(L)
        rows = _rows(rng, B * beam + 2, ld)
        lr = (beam, 1, 1)                                                            # a guard row in front, one behind
        got = _tap(rows, V, EOT, trie, alive, step_u, done, B, beam, lr)
        want, masked = _expect(rows, V, EOT, prefixes, alive, step_u, done, B, beam, lr)
        _same_bits(got, want, (V, n_kids, ld))
        # the scene holds what the docstring promises (asserted on the reference): root twice, an end with a child, a leaf, a one-child node
        kept = dict(masked)
        n_root = len(prefixes[()][0])
        assert kept[1] == kept[2] == n_root and n_root >= n_kids and kept[3] == 2 and kept[5] == 1 and kept[7] == 1 and kept[10] == 1, kept
        assert (4 in kept) == (n_kids >= 2) and (kept.get(4, n_kids) == n_kids), kept
        assert not {6, 8, 9, 11, 12} & set(kept), kept                               # the three ways off the trie, the finished utterance
        assert np.isneginf(want[5, :V]).sum() == V - 1 + int(np.isneginf(rows[5, EOT]))      # the leaf: <|endoftext|> alone


@pytest.mark.parametrize("n_kids", [3, 300])
def test_shared_prompt_row(n_kids):
    """lr_j = 0 (the pass that carries the prompt): the beams of an utterance share ONE row, the utterance's first workgroup masks it to the
    root's children, the other rows of the block - what the beams will own one step later - are not written."""
    from wis_hip import weights as W
    V, B, beam = 51865, 3, 5
    rng = np.random.default_rng(7 + n_kids)
    pool = _token_pool(V, EOT)
    phrases = [[t, int(pool[900])] for t in _children(rng, pool, n_kids, V)]
    trie, prefixes = W.build_phrase_trie(phrases), prefix_dict(phrases)
    alive = rng.integers(0, EOT, size=(B * beam, 8)).astype(np.int32)
    rows = _rows(rng, B * beam, V)
    for lr in ((beam, 0, 0), (beam, 0, 3)):
        got = _tap(rows, V, EOT, trie, alive, [0, 0, 0], [0, 1, 0], B, beam, lr)
        want, masked = _expect(rows, V, EOT, prefixes, alive, [0, 0, 0], [0, 1, 0], B, beam, lr)
        assert masked == [(lr[2], n_kids), (2 * beam + lr[2], n_kids)], masked
        _same_bits(got, want, (n_kids, lr))


def test_step_counter_beyond_the_history_buffer():
    """L = min(step_u, max_new): a counter past the buffer reads max_new tokens, never more"""
    from wis_hip import weights as W
    V = 51865
    rng = np.random.default_rng(3)
    pool = _token_pool(V, EOT)
    ph = rng.choice(pool, size=4, replace=False).tolist()
    phrases = [ph + [int(pool[10])], ph + [int(pool[11])]]
    trie, prefixes = W.build_phrase_trie(phrases), prefix_dict(phrases)
    alive = np.asarray([ph], np.int32)
    rows = _rows(rng, 1, V)
    got = _tap(rows, V, EOT, trie, alive, [9], [0], 1, 1, (1, 1, 0))
    want, masked = _expect(rows, V, EOT, prefixes, alive, [9], [0], 1, 1, (1, 1, 0))
    assert masked == [(0, 2)]
    _same_bits(got, want, "step_u > max_new")


def test_table_that_points_outside_itself_leaves_the_row():
    """The tap does not validate its table (wis_model_set_phrases does); the kernel refuses every child range outside [1, n_rec) and every
    token outside the vocabulary on its own: such rows stay as they are, a child id >= n_vocab is simply not kept."""
    V = 51865
    rng = np.random.default_rng(4)
    rows = _rows(rng, 2, V)
    alive = np.asarray([[100], [100]], np.int32)
    for trie in ([[-1, 1, 5, 0], [100, 0, 0, 1]],                      # the root claims 5 children, the table holds 1
                 [[-1, 1, 1, 0], [100, 2, 1, 0]],                      # the child's range starts at n_rec
                 [[-1, 1, 1, 0], [100, -7, 3, 0]],                     # a negative range
                 [[-1, 1, 1, 0], [100, 1, 70000, 0]]):                 # more children than a node may have
        got = _tap(rows, V, EOT, np.asarray(trie, np.int32), alive, [1, 1], [0, 0], 2, 1, (1, 1, 0))
        _same_bits(got, rows, trie)
    trie = np.asarray([[-1, 1, 2, 0], [100, 0, 0, 1], [V + 5, 0, 0, 1]], np.int32)      # a child beyond the vocabulary: not kept, nothing written there
    rows = _rows(rng, 1, V + 64)
    got = _tap(rows, V, EOT, trie, alive[:1], [0], [0], 1, 1, (1, 1, 0))
    want = rows.copy(); want[0, :V] = -np.inf; want[0, 100] = rows[0, 100]
    _same_bits(got, want, "child beyond the vocabulary")


def test_argument_checks():
    from wis_hip import _lib
    lib = _lib.load()
    d = _lib.DevBuf(64)
    try:
        for V, ld, eot, n_rec, B, beam, max_new in ((100, 50, 10, 1, 1, 1, 4), (100, 100, 100, 1, 1, 1, 4), (100, 100, 10, 0, 1, 1, 4), (100, 100, 10, 70000, 1, 1, 4),
                                                    (100, 100, 10, 1, 0, 1, 4), (100, 100, 10, 1, 1, 9, 4), (100, 100, 10, 1, 13, 8, 4), (100, 100, 10, 1, 1, 1, 0),
                                                    (100, 100, 10, 1, 1, 1, 257)):
            rc = lib.wis_op_phrase_rules(0, d.ptr, V, ld, eot, d.ptr, n_rec, d.ptr, d.ptr, d.ptr, B, beam, max_new, 1, 1, 0)
            assert rc == WIS_E_ARG, (V, ld, eot, n_rec, B, beam, max_new, rc)
        assert lib.wis_op_phrase_rules(0, None, 100, 100, 10, d.ptr, 1, d.ptr, d.ptr, d.ptr, 1, 1, 4, 1, 1, 0) == WIS_E_ARG
    finally:
        d.free()
