"""-m gpu: the two kernels of the long-prompt route's decode step, op by op, through their taps (include/wis_hip.h):

  wis_op_dec_self_attn_long   dec_self_attn_long_kernel - one workgroup per (utterance, head) over the prompt prefix shared in the utterance's first slot
                              and every row's own suffix - against float64 (tests/prefix_attn_ref.py: the reference, the poisoned cache, the bound
                              |err| <= 2^-10 max|V read|).  The TREE form of wis_op_dec_self_attn_ex (base[m] = b k, anc[m][0] = own slot, w0 = plen,
                              aw = 1) expresses the same read pattern: it runs on the same inputs and must meet the same bound.
  wis_op_kv_reorder_from      the cache reorder that leaves the prefix alone: bit-compared.

Shapes: H = 2 (d = 128), ctx 448 and 64, 1 and 3 utterances of 1 / 2 / 5 / 8 rows, prefix lengths on both sides of the 32- and 64-position block edges
(17, 63, 64, 65) and the longest prompt (228), utterances of one batch with different prefix lengths, suffixes of 0 / 1 / 7 / 8 / 9 / 64 positions and up to
the end of the cache, both output layouts."""
import numpy as np
import pytest

import prefix_attn_ref as R

pytestmark = pytest.mark.gpu

H = 2
D = 64 * H
SUFFIXES = [0, 1, 7, 8, 9, 64, -1]      # -1: up to ctx - plen (a full cache)


def _i32(a):
    return np.ascontiguousarray(np.asarray(a, np.int32))


def _run_long(lib, q, kc, vc, pos, plen, B, k, ctx, out_mb):
    from wis_hip._lib import DevBuf, check
    M = B * k
    bufs = [DevBuf.from_numpy(a) for a in (q, kc, vc, _i32(pos), _i32(plen))]
    n_out = R.xf_elems(D, out_mb) if out_mb else M * D
    d_out = DevBuf.from_numpy(np.full(n_out, np.nan, np.float16))
    check(lib.wis_op_dec_self_attn_long(0, *[x.ptr for x in bufs], d_out.ptr, B, k, H, ctx, out_mb))
    flat = d_out.to_numpy(np.float16, (n_out,))
    if out_mb:
        image = np.zeros(n_out, bool)
        m, c = np.meshgrid(np.arange(M), np.arange(D), indexing="ij")
        image[R.xf_index(m, c, out_mb)] = True
        assert not flat[~image].any(), "fragment image: elements of rows >= M must stay zero"
        return R.from_fragment_image(flat, M, D, out_mb).astype(np.float64)
    return flat.reshape(M, D).astype(np.float64)


def _run_tree(lib, q, kc, vc, pos, plen, B, k, ctx):
    """the same read pattern through dec_self_attn_kernel<TREE>: one call per utterance (w0 is one value per call)"""
    from wis_hip._lib import DevBuf, check
    d_kc, d_vc = DevBuf.from_numpy(kc), DevBuf.from_numpy(vc)
    out = np.zeros((B * k, D))
    for b in range(B):
        rows = slice(b * k, (b + 1) * k)
        d_q, d_pos = DevBuf.from_numpy(np.ascontiguousarray(q[rows])), DevBuf.from_numpy(_i32(pos[rows]))
        d_anc, d_base = DevBuf.from_numpy(_i32(np.arange(b * k, (b + 1) * k))), DevBuf.from_numpy(_i32([b * k] * k))
        d_out = DevBuf(k * D * 2)
        check(lib.wis_op_dec_self_attn_ex(0, d_q.ptr, d_kc.ptr, d_vc.ptr, d_pos.ptr, d_out.ptr, k, H, ctx, k, k, 1, 8, 0, d_anc.ptr, int(plen[b]), 1, d_base.ptr))
        out[rows] = d_out.to_numpy(np.float16, (k, D)).astype(np.float64)
    return out


def _suffixes(B, k, ctx, plen, rot):
    return [(ctx - plen[m // k]) if SUFFIXES[(m + rot) % 7] < 0 else min(SUFFIXES[(m + rot) % 7], ctx - plen[m // k]) for m in range(B * k)]


# (ctx, prefix length per utterance): one utterance at every length, three with a length each, and the short cache
CASES = [(448, (17,)), (448, (63,)), (448, (64,)), (448, (65,)), (448, (228,)), (448, (17, 228, 64)), (448, (65, 63, 65)), (448, (228, 228, 228)),
         (64, (17,)), (64, (17, 17, 17))]


@pytest.mark.parametrize("k", [1, 2, 5, 8])
@pytest.mark.parametrize("ctx,plen", CASES)
def test_long_self_attn_vs_float64(lib, ctx, plen, k):
    B = len(plen)
    worst = 0.0
    for rot in range(7 if B * k < 7 else 2):      # every suffix length meets every row count
        rng = np.random.default_rng([ctx, k, rot] + list(plen))
        q, kc, vc, pos = R.build_case(rng, B, k, H, ctx, plen, _suffixes(B, k, ctx, plen, rot))
        exp, vmax = R.reference(q, kc, vc, pos, plen, k, H)
        for out_mb in (0, (B * k + 15) // 16, (B * k + 15) // 16 + 1):
            got = _run_long(lib, q, kc, vc, pos, plen, B, k, ctx, out_mb)
            worst = max(worst, R.check(got, exp, vmax, f"long kernel, rot {rot}, out_mb {out_mb}"))
        worst = max(worst, R.check(_run_tree(lib, q, kc, vc, pos, plen, B, k, ctx), exp, vmax, f"TREE form, rot {rot}"))
    print(f"ctx {ctx} plen {plen} k {k}: worst error {worst:.3f} x bound")


def _peak(kc, q, slot, p, h, gain):
    """make position p of `slot` the one key of head h that lines up with every row's query (rows share a direction: see the test)"""
    sl = slice(64 * h, 64 * h + 64)
    u = q[0, sl] / np.linalg.norm(q[0, sl])
    kc[slot, p, sl] = (gain * u).astype(np.float16)


@pytest.mark.parametrize("pattern", ["max_in_prefix", "max_in_suffix", "max_in_other_wave", "one_position_has_all", "equal_scores"])
def test_long_self_attn_score_patterns(lib, pattern):
    """One constructed score pattern per edge of the four-wave merge: where the maximum lies decides which partial is rescaled by how much."""
    ctx, B, k, plen = 448, 2, 5, (65, 228)
    rng = np.random.default_rng(sorted(pattern.encode()))
    q, kc, vc, pos = R.build_case(rng, B, k, H, ctx, plen, [40 + 3 * m for m in range(B * k)])
    q[:] = q[0] + 0.02 * q          # (|q| ~ 3.2 per head: a key of gain g scores ~3.2 g, the random keys ~N(0, 1.6^2)) every row's query close to one direction: one key can dominate all of them
    for b in range(B):
        n = plen[b]
        for h in range(H):
            if pattern == "max_in_prefix":
                _peak(kc, q, b * k, 3, h, 3.0)                      # wave 0's share of the prefix
            elif pattern == "max_in_suffix":
                for j in range(k):
                    _peak(kc, q, b * k + j, n + 1, h, 3.0)          # wave 0's share of the suffix
            elif pattern == "max_in_other_wave":
                _peak(kc, q, b * k, 32 + 27, h, 3.0)                # prefix, wave 3
                for j in range(k):
                    _peak(kc, q, b * k + j, n + 32 + 11, h, 2.8)    # suffix, second chunk, wave 1
            elif pattern == "one_position_has_all":
                for j in range(k):
                    _peak(kc, q, b * k + j, n + 19, h, 20.0)         # score ~ +60 above the rest: every other weight vanishes
    if pattern == "equal_scores":
        kc[np.isfinite(kc)] = 0
    exp, vmax = R.reference(q, kc, vc, pos, plen, k, H)
    for out_mb in (0, 1):
        R.check(_run_long(lib, q, kc, vc, pos, plen, B, k, ctx, out_mb), exp, vmax, f"long kernel, {pattern}, out_mb {out_mb}")
    R.check(_run_tree(lib, q, kc, vc, pos, plen, B, k, ctx), exp, vmax, f"TREE form, {pattern}")


# ---- wis_op_kv_reorder_from ---------------------------------------------------------------------------------------------------------------
def _random_f16_bits(rng, shape):
    a = rng.integers(0, 1 << 16, size=shape, dtype=np.uint16)
    a.reshape(-1)[:8] = [0x7E00, 0x7C01, 0xFFFF, 0xFC00, 0x7C00, 0x8000, 0x0001, 0x7DFF]
    return a


def _parent_tables(rng, B, beam):
    base = np.repeat(np.arange(B) * beam, beam)
    rel = {"identity": np.tile(np.arange(beam), B), "rotation": np.tile((np.arange(beam) + 1) % beam, B),
           "swap": np.tile(np.array([1, 0] + list(range(2, beam))), B), "fan_out": np.tile(np.full(beam, beam - 1), B),
           "random": rng.integers(0, beam, size=B * beam)}
    return {name: _i32(base + v) for name, v in rel.items()}


@pytest.mark.parametrize("L,B,beam,d,ctx,plen,step", [(2, 1, 5, 384, 64, (17,), 9), (2, 3, 8, 1280, 96, (17, 40, 64), 20), (1, 2, 2, 128, 64, (33, 33), 1),
                                                      (2, 2, 5, 2304, 256, (228, 100), 12)])
def test_kv_reorder_from_moves_only_the_suffix(lib, L, B, beam, d, ctx, plen, step):
    """Positions < plen[b] of every slot stay bit for bit; [plen[b], plen[b] - 1 + step_u[b]) of slot j become the old slot parent[j]; finished utterances,
    positions behind the range and the slots behind the batch are untouched.  (step 1: the range is empty - what follows the prefill pass.)"""
    from wis_hip._lib import DevBuf, check
    rng = np.random.default_rng([L, B, beam, d])
    slots = B * beam + 2
    old_k, old_v = _random_f16_bits(rng, (L, slots, ctx, d)), _random_f16_bits(rng, (L, slots, ctx, d))
    step_u = [max(1, step - 3 * b) for b in range(B)]
    for name, parent in _parent_tables(rng, B, beam).items():
        for done in ([0] * B,) if B == 1 else ([0] * B, [0] * (B - 1) + [1], [1] + [0] * (B - 1)):
            dk, dv = DevBuf.from_numpy(old_k), DevBuf.from_numpy(old_v)
            ctl = [DevBuf.from_numpy(_i32(a)) for a in (parent, step_u, done, plen)]
            check(lib.wis_op_kv_reorder_from(0, dk.ptr, dv.ptr, slots * ctx * d, L, *[c.ptr for c in ctl], B, beam, ctx, d))
            for old, new in ((old_k, dk.to_numpy(np.uint16, old_k.shape)), (old_v, dv.to_numpy(np.uint16, old_v.shape))):
                want = old.copy()
                for b in range(B):
                    if not done[b]:
                        lo, hi = plen[b], plen[b] - 1 + step_u[b]
                        for j in range(beam):
                            want[:, b * beam + j, lo:hi] = old[:, parent[b * beam + j], lo:hi]
                assert np.array_equal(new, want), (name, done)
