"""-m gpu: the three kernels of the one-pass prefix route (csrc/prefill.hip) through their taps, against float64 numpy computed from the f16-rounded
operands the kernels read.

Bounds.  u = 2^-11 (f16 unit roundoff), e = 2^-24 (f32).
  projection   a sum of K exact f16 products accumulated in f32: |err| <= K e sum|a w| (first order); the LayerNorm fold multiplies by rstd and subtracts
               mu csum (two more f32 roundings of terms of that size), f16 outputs add u |y|.  Asserted: |err| <= 2 K e S + u |y| + 1e-6 with
               S = rstd (sum|a w| + |mu csum|) + |bias| (+ |residual|); the f16 rounding of the raw rows is part of the reference, not of the bound.
  attention    P is rounded to f16 (u, relative, per term), the f32 sums add n e: |err| <= (2 u + 4 n e) max|V read| + u |out|  (n keys), exp by the
               hardware approximation (2 ulp of f32) inside the 2 u."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
U, E32 = 2.0 ** -11, 2.0 ** -24
QKV, RESID, LN_F16, LN_GELU = 0, 1, 2, 3


def _dev(*arrays):
    from wis_hip._lib import DevBuf
    return [DevBuf.from_numpy(np.ascontiguousarray(a)) for a in arrays]


def _gelu(x):
    from math import erf
    return 0.5 * x * (1.0 + np.vectorize(erf)(x / np.sqrt(2.0)))


# tiny's d x d, FFN1 and FFN2 shapes under every epilogue that takes them (the QKV epilogue is N = 3 K)
SHAPES = [(QKV, 1152, 384)] + [(e, n, k) for e in (RESID, LN_F16, LN_GELU) for n, k in ((384, 384), (1536, 384), (384, 1536))]


@pytest.mark.parametrize("epi,N,K", SHAPES)
@pytest.mark.parametrize("M", [1, 15, 16, 17, 96, 97, 228, 256])
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
    bound = 2 * K * E32 * S + (0 if epi == RESID else U * np.abs(exp)) + 1e-6
    d_x, d_W, d_b, d_g, d_be = _dev(x, W, bias, gamma, beta)
    B, ctx, sstride = (2, 130, 3) if (epi == QKV and M % 2 == 0) else (1, 260, 2)
    Np, slots = M // B, B * sstride + 1
    kc0 = rng.standard_normal((2, slots, ctx, K)).astype(np.float16)
    d_kc, d_vc = _dev(kc0[0], kc0[1])
    (d_y,) = _dev(y0 if epi == RESID else np.full((M, K if epi == QKV else N), np.nan, np.float16))
    check(lib.wis_op_dec_prefill_proj(0, epi, d_x.ptr, d_g.ptr if ln else None, d_be.ptr if ln else None, d_W.ptr, d_b.ptr, d_y.ptr, d_kc.ptr, d_vc.ptr,
                                      M, N, K, Np, sstride, ctx))
    if epi == RESID:
        got = d_y.to_numpy(np.float32, (M, N)).astype(np.float64)
    elif epi != QKV:
        got = d_y.to_numpy(np.float16, (M, N)).astype(np.float64)
    else:
        kc, vc = d_kc.to_numpy(np.float16, (slots, ctx, K)), d_vc.to_numpy(np.float16, (slots, ctx, K))
        got = np.empty((M, N))
        got[:, :K] = d_y.to_numpy(np.float16, (M, K))
        for b in range(B):
            got[b * Np:(b + 1) * Np, K:2 * K] = kc[b * sstride, :Np]
            got[b * Np:(b + 1) * Np, 2 * K:] = vc[b * sstride, :Np]
            kc[b * sstride, :Np] = kc0[0][b * sstride, :Np]
            vc[b * sstride, :Np] = kc0[1][b * sstride, :Np]
        assert kc.tobytes() == kc0[0].tobytes() and vc.tobytes() == kc0[1].tobytes(), "the caches changed outside positions 0 .. Np - 1 of slot b sstride"
    err = np.abs(got - exp) / bound
    print(f"M {M} N {N} K {K} epi {epi}: worst error {err.max():.3f} x bound")
    assert np.isfinite(got).all() and err.max() <= 1.0


def _softmax_rows(s):
    p = np.exp(s - s.max(-1, keepdims=True))
    return p / p.sum(-1, keepdims=True)


def _self_case(rng, B, Np, H, ctx, sstride):
    d = 64 * H
    q = (rng.standard_normal((B * Np, d)) * 0.5).astype(np.float16)
    kc = rng.standard_normal((B * sstride, ctx, d)).astype(np.float16)
    vc = rng.standard_normal((B * sstride, ctx, d)).astype(np.float16)
    return q, kc, vc


def _self_ref(q, kc, vc, B, Np, H, sstride):
    exp, vmax = np.zeros(q.shape), np.zeros(q.shape)
    causal = np.tril(np.ones((Np, Np), bool))
    for b in range(B):
        for h in range(H):
            sl = slice(64 * h, 64 * h + 64)
            k, v = kc[b * sstride, :Np, sl].astype(np.float64), vc[b * sstride, :Np, sl].astype(np.float64)
            s = np.where(causal, q[b * Np:(b + 1) * Np, sl].astype(np.float64) @ k.T, -np.inf)
            exp[b * Np:(b + 1) * Np, sl] = _softmax_rows(s) @ v
            vmax[b * Np:(b + 1) * Np, sl] = np.maximum.accumulate(np.abs(v).max(1))[:, None]
    return exp, vmax


def _run_self(lib, q, kc, vc, B, Np, H, ctx, sstride):
    from wis_hip._lib import check
    d_q, d_kc, d_vc, d_o = _dev(q, kc, vc, np.full(q.shape, np.nan, np.float16))
    check(lib.wis_op_dec_prefill_self_attn(0, d_q.ptr, d_kc.ptr, d_vc.ptr, d_o.ptr, B, Np, H, ctx, sstride))
    return d_o.to_numpy(np.float16, q.shape).astype(np.float64)


@pytest.mark.parametrize("B", [1, 2])
@pytest.mark.parametrize("H", [6, 20])
@pytest.mark.parametrize("Np", [1, 2, 16, 17, 63, 64, 65, 228])
def test_self_attn_vs_float64(lib, Np, H, B):
    ctx, sstride = 230, 2
    rng = np.random.default_rng([Np, H, B])
    q, kc, vc = _self_case(rng, B, Np, H, ctx, sstride)
    # head 0, constructed: key i lines up with query i (its own, the diagonal: about 32) and far more with query i - 1 (about 120), for which it is masked
    for b in range(B):
        u = q[b * Np:(b + 1) * Np, :64].astype(np.float64)
        u /= np.linalg.norm(u, axis=1, keepdims=True)
        kc[b * sstride, :Np, :64] = (8.0 * u + 30.0 * np.vstack([np.zeros((1, 64)), u[:-1]])).astype(np.float16)
    exp, vmax = _self_ref(q, kc, vc, B, Np, H, sstride)
    got = _run_self(lib, q, kc, vc, B, Np, H, ctx, sstride)
    err = np.abs(got - exp) / ((2 * U + 4 * Np * E32) * vmax + U * np.abs(exp))
    print(f"Np {Np} H {H} B {B}: worst error {err.max():.3f} x bound")
    assert np.isfinite(got).all() and err.max() <= 1.0


@pytest.mark.parametrize("B", [1, 2])
@pytest.mark.parametrize("Np", [1, 17, 228])
def test_cross_attn_vs_float64(lib, Np, B):
    from wis_hip._lib import check
    H, T, Tpad = 6, 1500, 1536
    d = 64 * H
    rng = np.random.default_rng([Np, B])
    q = (rng.standard_normal((B * Np, d)) * 0.5).astype(np.float16)
    k = rng.standard_normal((B, H, T, 64)).astype(np.float16)
    v = rng.standard_normal((B, H, T, 64)).astype(np.float16)
    k[:, :, T - 1] = (2.0 * np.sign(q[:1, :64].astype(np.float32))).astype(np.float16)      # the last real key matters: a tail that starts one key early shows
    kx = np.ascontiguousarray(k.reshape(B, H, T, 8, 8).transpose(0, 1, 3, 2, 4))             # [B][H][8][T][8]
    vt = np.full((B, H, 64, Tpad), 3.0e4, np.float16)                                       # the tail: large, finite
    vt[..., :T] = v.transpose(0, 1, 3, 2)
    exp, vmax = np.zeros(q.shape), np.zeros(q.shape)
    for b in range(B):
        for h in range(H):
            sl = slice(64 * h, 64 * h + 64)
            s = q[b * Np:(b + 1) * Np, sl].astype(np.float64) @ k[b, h].astype(np.float64).T
            exp[b * Np:(b + 1) * Np, sl] = _softmax_rows(s) @ v[b, h].astype(np.float64)
            vmax[b * Np:(b + 1) * Np, sl] = np.abs(v[b, h]).max()
    d_q, d_kx, d_vt, d_o = _dev(q, kx, vt, np.full(q.shape, np.nan, np.float16))
    check(lib.wis_op_dec_prefill_cross_attn(0, d_q.ptr, d_kx.ptr, d_vt.ptr, d_o.ptr, B, Np, H, T, Tpad))
    got = d_o.to_numpy(np.float16, q.shape).astype(np.float64)
    err = np.abs(got - exp) / ((2 * U + 4 * T * E32) * vmax + U * np.abs(exp))
    print(f"Np {Np} B {B}: worst error {err.max():.3f} x bound")
    assert np.isfinite(got).all() and err.max() <= 1.0
