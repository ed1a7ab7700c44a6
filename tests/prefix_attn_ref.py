"""float64 reference of the decode step's self-attention behind a shared prompt prefix (csrc/dec_kernels.hip dec_self_attn_long_kernel, and the TREE form
of dec_self_attn_kernel that expresses the same read pattern), its error bound, and the cache builder the op tests share.

The read rule (include/wis_hip.h wis_op_dec_self_attn_long): B utterances of k rows, row m = b k + j reads positions < plen[b] from slot b k and positions
plen[b] .. pos[m] from its own slot b k + j.

The bound.  With the f16 cache values and the f32 query taken as exact, the true output element o[m][c] = sum_p w_p V[p][c] is a CONVEX combination
(w_p >= 0, sum w_p = 1) of the V values the row reads in column c, so |o| <= Vmax := max |V read by the row|.  The kernels differ from it by
  - the final rounding to f16: at most half an ulp, |o| 2^-11 <= Vmax 2^-11 (normal range; the test values are O(1));
  - f32 arithmetic before that: dot products of 64 terms, at most 448 weights and accumulation terms each with relative error ~2^-24, and __expf (relative
    error of a few 2^-22 times the magnitude of its argument, arguments down to about -60 in the peaked cases); the errors of the weights largely cancel in
    the normalisation.  Together a few 2^-16 Vmax - given as much room again as the rounding.
Hence |err| <= 2^-10 Vmax.  The tests take Vmax per (row, head), which is never larger than the row's."""
import numpy as np

BOUND_REL = 2.0 ** -10


def xf_index(m, k, MB):
    """element (row m, column k) of a fragment image of MB row blocks (csrc/kernels.hpp xf_index)"""
    return (((k >> 5) * MB + (m >> 4)) * 64 + (m & 15) + 16 * ((k >> 3) & 3)) * 8 + (k & 7)


def xf_elems(K, MB):
    return (K // 32) * MB * 64 * 8


def from_fragment_image(img, M, d, MB):
    """f16 fragment image (flat) -> [M][d]"""
    m, k = np.meshgrid(np.arange(M), np.arange(d), indexing="ij")
    return img[xf_index(m, k, MB)]


def build_case(rng, B, k, H, ctx, plen, suffix, extra_slots=1):
    """A cache in which ONLY what the read rule allows is finite: the prefix [0, plen[b]) of slot b k, the suffix [plen[b], pos[m]] of every row's own slot.
    Everything else - the prefix positions of beams 1 .. k-1, slot b k beyond plen[b] where row 0 has no suffix there, everything behind a row's length, the
    slots behind the batch - is NaN: a read from the wrong place surfaces as NaN in the output.
    plen [B], suffix [B k] (positions a row holds behind the prefix) -> q f32 [B k][d], kc / vc f16 [slots][ctx][d], pos i32 [B k]"""
    d, M = 64 * H, B * k
    slots = M + extra_slots
    kc = np.full((slots, ctx, d), np.nan, np.float16)
    vc = np.full((slots, ctx, d), np.nan, np.float16)
    pos = np.zeros(M, np.int32)
    for b in range(B):
        n = int(plen[b])
        kc[b * k, :n] = (rng.standard_normal((n, d)) * 0.5).astype(np.float16)
        vc[b * k, :n] = rng.standard_normal((n, d)).astype(np.float16)
        for j in range(k):
            m, s = b * k + j, int(suffix[b * k + j])
            assert n + s <= ctx
            kc[m, n:n + s] = (rng.standard_normal((s, d)) * 0.5).astype(np.float16)
            vc[m, n:n + s] = rng.standard_normal((s, d)).astype(np.float16)
            pos[m] = n + s - 1
    q = (rng.standard_normal((M, d)) * 0.4).astype(np.float32)
    return q, kc, vc, pos


def history(kc, vc, pos, plen, k, m):
    """the K and V rows ([len][d] f16) row m reads, in position order"""
    b, n = m // k, int(plen[m // k])
    ln = int(pos[m]) + 1
    K = np.concatenate([kc[b * k, :min(n, ln)], kc[m, n:ln]])
    V = np.concatenate([vc[b * k, :min(n, ln)], vc[m, n:ln]])
    return K, V


def reference(q, kc, vc, pos, plen, k, H):
    """-> (out f64 [M][d], vmax f64 [M][H]: the largest |V| row m reads in head h)"""
    M, d = q.shape
    out, vmax = np.zeros((M, d)), np.zeros((M, H))
    for m in range(M):
        K, V = history(kc, vc, pos, plen, k, m)
        K, V = K.astype(np.float64), V.astype(np.float64)
        assert np.isfinite(K).all() and np.isfinite(V).all()
        for h in range(H):
            sl = slice(64 * h, 64 * h + 64)
            s = K[:, sl] @ q[m, sl].astype(np.float64)
            w = np.exp(s - s.max())
            out[m, sl] = (w / w.sum()) @ V[:, sl]
            vmax[m, h] = np.abs(V[:, sl]).max()
    return out, vmax


def check(got, exp, vmax, what):
    """got f64 [M][d] against the reference under the bound of this file; NaN (a read from a poisoned place) fails"""
    M, d = exp.shape
    H = d // 64
    assert np.isfinite(got).all(), f"{what}: NaN / inf in the output - a read outside the row's history"
    err = np.abs(got - exp).reshape(M, H, 64).max(axis=2)
    ratio = (err / (BOUND_REL * vmax)).max()
    assert ratio <= 1.0, f"{what}: error {ratio:.2f} x the bound 2^-10 max|V| (worst row, head: {np.unravel_index(np.argmax(err / vmax), err.shape)})"
    return ratio
