"""-m gpu: the three kernels of wis_align's one-pass route (csrc/align_pass.hip) through their taps, against float64 numpy computed from the f16-rounded
operands the kernels read.  Rows are ragged: a table of utterance lengths, row off[b] + i = position i of utterance b.

Bounds (tests/test_gpu_prefill_ops.py has the derivation).  u = 2^-11 (f16 unit roundoff), e = 2^-24 (f32).
  projection   |err| <= 2 K e S + u |y| + 1e-6, S = rstd (sum|a w| + |mu csum|) + |bias| (+ |residual|).  The kernel takes mean / rstd itself, the variance as
               E[x^2] - mean^2 in f32: sums of K terms, relative error K e each, on E[x^2] = var + mean^2 <= 1.05 var for these rows (mean 0.3, std 1.5) -
               about 1.1 K e relative on var, half of that on rstd, so at most 0.55 K e S more on y: with the MFMA sum's K e S still inside 2 K e S.
  attention    P is rounded to f16, the f32 sums add n e: |err| <= (2 u + 4 n e) max|V read| + u |out|  (n keys)."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
U, E32 = 2.0 ** -11, 2.0 ** -24
LN_F16, RESID, LN_GELU, LN_F32 = 0, 1, 2, 3
TABLES = [[1], [16], [17], [5, 40], [15, 17, 1], [448]]
_i32 = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))


def _dev(*arrays):
    from wis_hip._lib import DevBuf
    return [DevBuf.from_numpy(np.ascontiguousarray(a)) for a in arrays]


def _gelu(x):
    from math import erf
    return 0.5 * x * (1.0 + np.vectorize(erf)(x / np.sqrt(2.0)))


def _softmax_rows(s):
    p = np.exp(s - s.max(-1, keepdims=True))
    return p / p.sum(-1, keepdims=True)


def _off(table):
    return np.concatenate([[0], np.cumsum(table)]).astype(np.int32)


# tiny's d x d, QKV, FFN1 and FFN2 shapes; N = 400 is 25 tiles: a last column group of one tile
@pytest.mark.parametrize("epi,N,K", [(LN_F16, 1152, 384), (LN_F16, 400, 384), (RESID, 384, 384), (RESID, 384, 1536), (LN_GELU, 1536, 384), (LN_F32, 400, 384)])
@pytest.mark.parametrize("M", [1, 257, 272, 448, 449])
def test_proj_vs_float64(lib, M, N, K, epi):
    from wis_hip._lib import check
    rng = np.random.default_rng([M, N, K, epi])
    ln = epi != RESID
    W = (rng.standard_normal((N, K)) * 0.05).astype(np.float16)
    bias = rng.standard_normal(N).astype(np.float32)
    x = (rng.standard_normal((M, K)) * 1.5 + 0.3).astype(np.float32 if ln else np.float16)
    gamma = (1.0 + 0.2 * rng.standard_normal(K)).astype(np.float32)
    beta = (0.1 * rng.standard_normal(K)).astype(np.float32)
    x64 = x.astype(np.float64)
    if ln:      # the kernel's arithmetic on exact numbers: f16(W gamma) against the f16 raw rows, mean / rstd of the f32 rows
        wg = (W.astype(np.float32) * gamma).astype(np.float16).astype(np.float64)
        a = x.astype(np.float16).astype(np.float64)
        mu, rs = x64.mean(1, keepdims=True), 1.0 / np.sqrt(x64.var(1, keepdims=True) + 1e-5)
        b2 = bias.astype(np.float64) + W.astype(np.float64) @ beta.astype(np.float64)
        exp = rs * (a @ wg.T - mu * wg.sum(1)) + b2
        S = rs * (np.abs(a) @ np.abs(wg).T + np.abs(mu * wg.sum(1))) + np.abs(b2)
    else:
        y0 = rng.standard_normal((M, N)).astype(np.float32)
        exp = y0.astype(np.float64) + x64 @ W.astype(np.float64).T + bias
        S = np.abs(y0) + np.abs(x64) @ np.abs(W.astype(np.float64)).T + np.abs(bias)
    if epi == LN_GELU:
        exp = _gelu(exp)
    f32_out = epi in (RESID, LN_F32)
    bound = 2 * K * E32 * S + (0 if f32_out else U * np.abs(exp)) + 1e-6
    # one guard row behind the output: it must keep its bits
    y_init = np.vstack([y0, np.full((1, N), 7.0, np.float32)]) if epi == RESID else np.full((M + 1, N), np.nan, np.float32 if f32_out else np.float16)
    d_x, d_W, d_b, d_g, d_be, d_y = _dev(x, W, bias, gamma, beta, y_init)
    check(lib.wis_op_align_pass_proj(0, epi, d_x.ptr, d_g.ptr if ln else None, d_be.ptr if ln else None, d_W.ptr, d_b.ptr, d_y.ptr, M, N, K))
    out = d_y.to_numpy(y_init.dtype, (M + 1, N))
    assert out[M].tobytes() == y_init[M].tobytes(), "the row behind the last one changed"
    err = np.abs(out[:M].astype(np.float64) - exp) / bound
    print(f"M {M} N {N} K {K} epi {epi}: worst error {err.max():.3f} x bound")
    assert np.isfinite(out[:M]).all() and err.max() <= 1.0


@pytest.mark.parametrize("table", TABLES, ids=str)
def test_self_attn_vs_float64(lib, table):
    from wis_hip._lib import check
    H, d, off = 6, 384, _off(table)
    M = int(off[-1])
    rng = np.random.default_rng([len(table), M])
    qkv = rng.standard_normal((M, 3 * d)).astype(np.float16)
    qkv[:, :d] *= 0.5
    # head 0, constructed: key i lines up with query i (its own, the diagonal) and far more with query i - 1 of the SAME table row order - for which it is
    # masked, or belongs to the previous utterance where i is an utterance's first row
    u = qkv[:, :64].astype(np.float64)
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    qkv[:, d:d + 64] = (8.0 * u + 30.0 * np.vstack([np.zeros((1, 64)), u[:-1]])).astype(np.float16)
    exp, vmax = np.zeros((M, d)), np.zeros((M, d))
    for b, L in enumerate(table):
        rows = slice(off[b], off[b] + L)
        for h in range(H):
            sl = slice(64 * h, 64 * h + 64)
            q, k, v = (qkv[rows, j * d + 64 * h:j * d + 64 * h + 64].astype(np.float64) for j in range(3))
            exp[rows, sl] = _softmax_rows(np.where(np.tril(np.ones((L, L), bool)), q @ k.T, -np.inf)) @ v
            vmax[rows, sl] = np.maximum.accumulate(np.abs(v).max(1))[:, None]
    guard = np.full((M + 1, d), np.nan, np.float16)
    d_qkv, d_o = _dev(qkv, guard)
    check(lib.wis_op_align_pass_self_attn(0, d_qkv.ptr, _i32(off), d_o.ptr, len(table), H))
    out = d_o.to_numpy(np.float16, (M + 1, d))
    assert np.isnan(out[M]).all(), "the row behind the last one was written"
    err = np.abs(out[:M].astype(np.float64) - exp) / ((2 * U + 4 * max(table) * E32) * vmax + U * np.abs(exp))
    print(f"rows {table}: worst error {err.max():.3f} x bound")
    assert np.isfinite(out[:M]).all() and err.max() <= 1.0


@pytest.mark.parametrize("table", TABLES, ids=str)
def test_cross_attn_and_capture_vs_float64(lib, table):
    from wis_hip._lib import check
    H, T, Tpad, P, ncap, nsel = 6, 1500, 1536, 3, 448, 3
    B, d, off = len(table), 64 * H, _off(table)
    M = int(off[-1])
    head_sel = np.array([-1, 2, -1, -1, 0, -1], np.int32)      # heads 1 and 4 are selected entries 2 and 0; entry 1 belongs to another layer
    rng = np.random.default_rng([B, M, 7])
    q = (rng.standard_normal((M, d)) * 0.5).astype(np.float16)
    k = rng.standard_normal((B, H, T, 64)).astype(np.float16)
    v = rng.standard_normal((B, H, T, 64)).astype(np.float16)
    k[:, :, T - 1] = (2.0 * np.sign(q[:1, :64].astype(np.float32))).astype(np.float16)      # the last real key matters
    kx = np.ascontiguousarray(k.reshape(B, H, T, 8, 8).transpose(0, 1, 3, 2, 4))             # [B][H][8][T][8]
    vt = np.full((B, H, 64, Tpad), 3.0e4, np.float16)                                       # the tail: large, finite
    vt[..., :T] = v.transpose(0, 1, 3, 2)
    exp = np.zeros((M, d))
    qsel0 = rng.standard_normal((B, nsel, ncap, 64)).astype(np.float16)
    want_qsel = qsel0.copy()
    for b, L in enumerate(table):
        rows = slice(off[b], off[b] + L)
        for h in range(H):
            sl = slice(64 * h, 64 * h + 64)
            exp[rows, sl] = _softmax_rows(q[rows, sl].astype(np.float64) @ k[b, h].astype(np.float64).T) @ v[b, h].astype(np.float64)
            if head_sel[h] >= 0 and L > P:
                want_qsel[b, head_sel[h], :L - P] = q[off[b] + P:off[b] + L, sl]
    vmax = np.repeat(np.repeat(np.abs(v).max((2, 3)), table, axis=0), 64, axis=1)           # [M][d]: the row's utterance, the column's head
    d_q, d_kx, d_vt, d_o, d_qs = _dev(q, kx, vt, np.full((M + 1, d), np.nan, np.float16), qsel0)
    check(lib.wis_op_align_pass_cross_attn(0, d_q.ptr, _i32(off), d_kx.ptr, d_vt.ptr, d_o.ptr, B, H, T, Tpad, _i32(head_sel), d_qs.ptr, qsel0.size, nsel, ncap, P))
    out = d_o.to_numpy(np.float16, (M + 1, d))
    assert np.isnan(out[M]).all(), "the row behind the last one was written"
    # the captured queries are the f16 queries of the selected heads, bit for bit, and nothing else of qsel moved
    assert d_qs.to_numpy(np.float16, qsel0.shape).tobytes() == want_qsel.tobytes()
    err = np.abs(out[:M].astype(np.float64) - exp) / ((2 * U + 4 * T * E32) * vmax + U * np.abs(exp))
    print(f"rows {table}: worst error {err.max():.3f} x bound")
    assert np.isfinite(out[:M]).all() and err.max() <= 1.0
