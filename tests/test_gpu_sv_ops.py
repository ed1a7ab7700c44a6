"""-m gpu: each speaker-verification kernel of csrc/sv.hip, called alone through its wis_op_sv_* entry (the production launch), against
the float64 restatement in tests/sv_ref.py, at the shapes and inputs where such kernels go wrong: ragged tiles, the shortest input,
a bias table longer than the input, planted bias winners, large common offsets, padded columns.  Plus the speaker-verification shapes
of the shared encoder GEMM through wis_op_gemm.  Every check is a whole-tensor rel-L2 and a per-row bound, and output rows past the
end are guarded by a sentinel."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sv_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

GUARD = 16                       # sentinel rows after every output


def _dev(a):
    from wis_hip._lib import DevBuf
    return DevBuf.from_numpy(np.ascontiguousarray(a))


def _guarded(rows, cols, dtype, fill):
    """a device output of rows + GUARD rows, every element `fill`"""
    return _dev(np.full((rows + GUARD, cols), fill, dtype))


def _read(buf, rows, cols, dtype):
    """-> (the rows, the guard rows) as numpy"""
    a = buf.to_numpy(dtype, (rows + GUARD, cols))
    return a[:rows], a[rows:]


def _close(got, ref, rel, row_atol, row_rtol, what):
    """rel-L2 over the tensor, and every row within row_atol + row_rtol * (that row's max |ref|) elementwise"""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert np.isfinite(got).all(), what
    e = R.rel_l2(got, ref)
    assert e <= rel, (what, "rel-L2", e)
    err = np.abs(got - ref).max(axis=-1)
    lim = row_atol + row_rtol * np.abs(ref).max(axis=-1)
    bad = np.nonzero(err > lim)[0]
    assert bad.size == 0, (what, "rows", bad[:8], err[bad[:8]], lim[bad[:8]])
    return e


# ---- gated relative-position attention ------------------------------------------------------------------------------------------
def _attn_case(T, L, seed):
    """operands where the bias, its direction and the gate all decide the output: tab N(0, 3), gate weights std 0.5 with N(0, 1)
    biases, gconst spread over the heads, and in every head one planted distance whose bias alone picks the winning key (some
    positive and large, so the winner arrives in the last key blocks, after the running maximum has settled elsewhere)"""
    rng = np.random.default_rng(seed)
    qkv = rng.standard_normal((T, 3 * R.D)) * 0.5
    qkv[:, :R.D] *= 0.25                                                  # Q . K spread ~0.5: the bias dominates
    qkv = qkv.astype(np.float16)
    xin = rng.standard_normal((T, R.D)).astype(np.float32)
    gw = (rng.standard_normal((8, R.DH)) * 0.5 / 8).astype(np.float32)   # |proj| ~ 0.5 per output
    gb = (rng.standard_normal(8) * 0.5).astype(np.float32)                # nonzero, and the sigmoids stay off their rails
    gconst = np.linspace(0.3, 3.0, R.H).astype(np.float32)[rng.permutation(R.H)]
    tab = (rng.standard_normal((R.H, 2 * L - 1)) * 3.0).astype(np.float32)
    dists = [1, -1, 3, -4, T - 1, -(T - 1), (T - 1) // 2, -((T - 1) // 2), T - 2, 7, -9, T // 3]
    for h, d in enumerate(dists):
        d = int(np.clip(d, -(T - 1), T - 1))
        tab[h, d + L - 1] = 25.0
    return qkv, xin, gw, gb, gconst, tab


@pytest.mark.parametrize("T,L", [(16, 16), (17, 17), (31, 31), (32, 32), (33, 33), (149, 149), (499, 499), (17, 499)])
def test_sv_attention_vs_float64(lib, T, L):
    from wis_hip._lib import check
    qkv, xin, gw, gb, gconst, tab = _attn_case(T, L, 100 + T + L)
    sentinel = np.float16(-1234.5)
    d_out = _guarded(T, R.D, np.float16, sentinel)
    bufs = [_dev(a) for a in (qkv, xin, gw, gb, gconst, tab)]
    check(lib.wis_op_sv_attention(0, *(b.ptr for b in bufs), L, d_out.ptr, T))
    got, guard = _read(d_out, T, R.D, np.float16)
    assert (guard == sentinel).all()
    ref = R.attention(qkv.astype(np.float64), xin, gw, gb, gconst, tab, L)
    # P is rounded to f16 before P.V and the output is f16: ~1e-3 relative
    e = _close(got, ref, 2e-3, 2e-3, 4e-3, f"attention T={T} L={L}")
    # the operands are strong enough that a wrong bias direction or a wrong gate would be far outside that
    g = R.gate(xin, gw, gb, gconst)
    swapped = R.gate(xin, np.concatenate([gw[4:], gw[:4]]), np.concatenate([gb[4:], gb[:4]]), gconst)
    assert g.std(axis=1).mean() > 0.05 and np.abs(g - swapped).max() > 0.3         # varies per query; gate_a / gate_b not symmetric
    print(f"sv attention T={T} L={L}: rel-L2 {e:.2e}")


def test_sv_attention_planted_winner_and_direction(lib):
    """one head where only the planted bias distinguishes the keys (Q = K = 0): the output row must be V[q + d] for every query
    whose key q + d exists, with d = key - query as HF defines it"""
    from wis_hip._lib import check
    T, L = 149, 499
    qkv, xin, gw, gb, gconst, tab = _attn_case(T, L, 7)
    qkv[:, :2 * R.D] = 0
    tab[:] = 0
    d = 37
    tab[:, d + L - 1] = 40.0
    d_out = _guarded(T, R.D, np.float16, np.float16(0))
    bufs = [_dev(a) for a in (qkv, xin, gw, gb, gconst, tab)]
    check(lib.wis_op_sv_attention(0, *(b.ptr for b in bufs), L, d_out.ptr, T))
    got, _ = _read(d_out, T, R.D, np.float16)
    v = qkv[:, 2 * R.D:].astype(np.float64)
    np.testing.assert_allclose(got[: T - d], v[d:], atol=2e-3)
    # rows without that key: a uniform average over the keys (the bias is 0 everywhere else)
    np.testing.assert_allclose(got[T - d:], np.broadcast_to(v.mean(axis=0), (d, R.D)), atol=2e-3)


# ---- positional convolution -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", [16, 17, 63, 64, 65, 127, 128, 129, 499])
def test_sv_posconv_vs_float64(lib, T):
    from wis_hip._lib import check
    rng = np.random.default_rng(200 + T)
    x = rng.standard_normal((T, R.D)).astype(np.float32)
    W = (rng.standard_normal((R.D, R.PK, R.D // R.PG)) * 0.015).astype(np.float16)
    bias = (rng.standard_normal(R.D) * 0.5).astype(np.float32)
    sentinel = np.float32(-7777.0)
    d_out = _guarded(T, R.D, np.float32, sentinel)
    dx, dW, db = _dev(x), _dev(W), _dev(bias)
    check(lib.wis_op_sv_posconv(0, dx.ptr, dW.ptr, db.ptr, d_out.ptr, T))
    got, guard = _read(d_out, T, R.D, np.float32)
    assert (guard == sentinel).all()
    ref = R.posconv(x, W.astype(np.float64), bias)
    # compare the GELU term alone (the residual would dilute the norm); f32 sums of exact f16 products
    e = _close(got - x, ref - x, 1e-4, 1e-4, 1e-5, f"posconv T={T}")
    print(f"sv posconv T={T}: rel-L2 {e:.2e}")


# ---- conv 0 + GroupNorm + GELU --------------------------------------------------------------------------------------------------
def _conv0_weights(seed):
    rng = np.random.default_rng(seed)
    w0 = (rng.standard_normal((R.C0, 10)) * 0.3).astype(np.float32)
    gamma = (1 + 0.2 * rng.standard_normal(R.C0)).astype(np.float32)
    beta = (0.5 * rng.standard_normal(R.C0)).astype(np.float32)
    return w0, gamma, beta


def _run_conv0(lib, pcm, w0, gamma, beta):
    from wis_hip._lib import check
    T0 = (pcm.size - 10) // 5 + 1
    sentinel = np.float16(-999.0)
    d_y = _guarded(T0, R.C0, np.float16, sentinel)
    dp, dw, dg, db = _dev(pcm), _dev(w0), _dev(gamma), _dev(beta)
    check(lib.wis_op_sv_conv0(0, dp.ptr, pcm.size, dw.ptr, dg.ptr, db.ptr, d_y.ptr))
    got, guard = _read(d_y, T0, R.C0, np.float16)
    assert (guard == sentinel).all()
    return got


@pytest.mark.parametrize("T0", [64, 65, 127, 4096, 4097, 4159, 31999])          # T0 mod 64 in {0, 1, 63}; 31999 = 10 s
def test_sv_conv0_lengths(lib, T0):
    rng = np.random.default_rng(T0)
    n = 5 * (T0 - 1) + 10 + int(rng.integers(0, 5))                            # the samples past the last full window are unused
    pcm = rng.standard_normal(n).astype(np.float32)
    w0, gamma, beta = _conv0_weights(1)
    got = _run_conv0(lib, pcm, w0, gamma, beta)
    assert got.shape == (T0, R.C0)
    e = _close(got, R.conv0_groupnorm_gelu(pcm, w0, gamma, beta), 1e-3, 2e-3, 2e-3, f"conv0 T0={T0}")
    print(f"sv conv0 T0={T0}: rel-L2 {e:.2e}")


def test_sv_conv0_dc_offset(lib):
    """50 + N(0, 0.01): the conv outputs sit ~10 s.d. of the weights' sum away from 0 with a spread 5000x smaller - a sum /
    sum-of-squares variance cancels to noise here, the chunked (mean, M2) merge must not.  The f32 conv itself loses ~1e-3 of the
    normalised value at this ratio (15 / 0.003 in ulps), hence the looser bound."""
    rng = np.random.default_rng(3)
    T0 = 9599
    pcm = (50.0 + 0.01 * rng.standard_normal(5 * (T0 - 1) + 10)).astype(np.float32)
    w0, gamma, beta = _conv0_weights(2)
    got = _run_conv0(lib, pcm, w0, gamma, beta)
    ref = R.conv0_groupnorm_gelu(pcm, w0, gamma, beta)
    assert ref.std() > 0.3                                              # the normalised output is O(1), not collapsed
    e = _close(got, ref, 3e-3, 2e-2, 1e-2, "conv0 dc offset")
    print(f"sv conv0 DC offset: rel-L2 {e:.2e}")


def test_sv_conv0_silence_and_square_wave(lib):
    w0, gamma, beta = _conv0_weights(4)
    T0 = 3199
    n = 5 * (T0 - 1) + 10
    got = _run_conv0(lib, np.zeros(n, np.float32), w0, gamma, beta)
    ref = np.broadcast_to(R.gelu(beta.astype(np.float64)), (T0, R.C0))     # variance 0: (0 - 0) * rstd -> GELU(beta)
    _close(got, ref, 1e-3, 1e-3, 1e-3, "conv0 silence")
    t = np.arange(n)
    sq = np.clip(3.0 * np.sign(np.sin(2 * np.pi * t / 73.0 + 0.1)), -1.0, 1.0).astype(np.float32)    # a clipped square wave
    got = _run_conv0(lib, sq, w0, gamma, beta)
    e = _close(got, R.conv0_groupnorm_gelu(sq, w0, gamma, beta), 1e-3, 2e-3, 2e-3, "conv0 square wave")
    print(f"sv conv0 square wave: rel-L2 {e:.2e}")


# ---- LayerNorm with the weighted layer sum --------------------------------------------------------------------------------------
@pytest.mark.parametrize("d,in_f16", [(512, True), (768, False), (768, True), (512, False)])
def test_sv_layernorm_weighted_sum(lib, d, in_f16):
    """wmode 1 then twelve wmode-2 calls (the encoder's 13 hidden states) must equal the float64 weighted sum of 13 LayerNorms;
    rows 0-3 carry a large common offset (1000 on f32 input, 200 on f16 input)"""
    from wis_hip._lib import check
    rng = np.random.default_rng(d + in_f16)
    M = 37                                                             # not a multiple of the 4 rows per workgroup
    lw = np.exp(rng.standard_normal(13))
    lw = (lw / lw.sum()).astype(np.float32)
    dt = np.float16 if in_f16 else np.float32
    d_y16, d_y32 = _guarded(M, d, np.float16, np.float16(-5.0)), _guarded(M, d, np.float32, np.float32(-5.0))
    d_ws, d_ws16 = _guarded(M, d, np.float32, np.float32(-5.0)), _guarded(M, d, np.float16, np.float16(-5.0))
    acc = np.zeros((M, d))
    for layer in range(13):
        x = rng.standard_normal((M, d)) * (1 + layer)
        x[:4] += 1000.0 if not in_f16 else 200.0
        x = x.astype(dt)
        g = (1 + 0.3 * rng.standard_normal(d)).astype(np.float32)
        b = (0.3 * rng.standard_normal(d)).astype(np.float32)
        dx, dg, db = _dev(x), _dev(g), _dev(b)
        last = layer == 12
        check(lib.wis_op_sv_layernorm(0, dx.ptr, int(in_f16), dg.ptr, db.ptr, d_y16.ptr, d_y32.ptr, d_ws.ptr, d_ws16.ptr if last else None,
                                      float(lw[layer]), 1 if layer == 0 else 2, M, d))
        ref = R.layernorm(x.astype(np.float64), g, b)
        acc += float(lw[layer]) * ref
        y32, g32 = _read(d_y32, M, d, np.float32)
        y16, g16 = _read(d_y16, M, d, np.float16)
        assert (g32 == np.float32(-5.0)).all() and (g16 == np.float16(-5.0)).all()
        _close(y32, ref, 2e-4, 1e-3, 1e-4, f"layernorm d={d} f16={in_f16} layer {layer}")
        assert np.array_equal(y16, y32.astype(np.float16))
    ws, gws = _read(d_ws, M, d, np.float32)
    ws16, gws16 = _read(d_ws16, M, d, np.float16)
    assert (gws == np.float32(-5.0)).all() and (gws16 == np.float16(-5.0)).all()
    e = _close(ws, acc, 2e-4, 1e-3, 1e-4, f"weighted sum d={d} f16={in_f16}")
    assert np.array_equal(ws16, ws.astype(np.float16))
    print(f"sv layernorm d={d} in_f16={in_f16}: weighted-sum rel-L2 {e:.2e}")


# ---- x-vector tail ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", [2, 3, 485])
def test_sv_xvector_tail(lib, T):
    """statistics pooling of ReLU(z) over T rows (std / (T - 1)) and the Linear 3000 -> 512; z's padded columns 1500-1535
    hold 1e4 and must not be read"""
    from wis_hip._lib import check
    rng = np.random.default_rng(300 + T)
    n, ldz = 1500, 1536
    z = (rng.standard_normal((T, ldz)) + 0.3 * rng.standard_normal(ldz)).astype(np.float32)     # about 40 % negative
    z[:, n:] = 1e4
    W = (rng.standard_normal((512, 2 * n)) * 0.03).astype(np.float32)
    b = rng.standard_normal(512).astype(np.float32)
    dz, dW, db = _dev(z), _dev(W), _dev(b)
    d_st, d_emb = _dev(np.full(2 * n + 64, -3.0, np.float32)), _dev(np.full(512 + 64, -3.0, np.float32))
    check(lib.wis_op_sv_xvector_tail(0, dz.ptr, ldz, T, n, dW.ptr, db.ptr, d_st.ptr, d_emb.ptr))
    st = d_st.to_numpy(np.float32, (2 * n + 64,))
    emb = d_emb.to_numpy(np.float32, (512 + 64,))
    assert (st[2 * n:] == -3.0).all() and (emb[512:] == -3.0).all()
    ref_st, ref_emb = R.xvector_tail(z, T, n, W, b)
    _close(st[None, :n], ref_st[None, :n], 1e-5, 1e-5, 1e-5, f"mean T={T}")
    _close(st[None, n:2 * n], ref_st[None, n:], 1e-5, 1e-5, 1e-5, f"std T={T}")
    e = _close(emb[None, :512], ref_emb[None], 1e-5, 1e-5, 1e-5, f"embedding T={T}")
    # the biased std (/ T) is a different number: (T / (T - 1))^0.5 - 1 >= 0.1 % even at T = 485
    biased = np.maximum(z[:T, :n].astype(np.float64), 0).std(axis=0)
    assert R.rel_l2(st[n:2 * n], biased) > 5e-4
    print(f"sv x-vector tail T={T}: embedding rel-L2 {e:.2e}")


# ---- the speaker-verification shapes of the shared encoder GEMM ----------------------------------------------------------------------
def _gemm(lib, A, lda, M, Wt, bias, flags, resid=None):
    from wis_hip._lib import check
    N, K = Wt.shape
    pad = np.zeros((256, A.shape[1]), A.dtype)             # rows past the last im2col window (the production buffers have them too)
    dA, dW, db = _dev(np.concatenate([A, pad])), _dev(Wt), _dev(bias)
    dr = _dev(resid) if resid is not None else None
    out_dt = np.float32 if flags & 4 else np.float16
    sentinel = out_dt(-4321.0)
    dC = _guarded(M, N, out_dt, sentinel)
    check(lib.wis_op_gemm(0, dA.ptr, lda, dW.ptr, db.ptr, dr.ptr if dr else None, dC.ptr, M, N, K, flags))
    got, guard = _read(dC, M, N, out_dt)
    assert (guard == sentinel).all()
    return got


def _im2col(A, lda_rows, M, k):
    """row t = A[lda_rows t : lda_rows t + k] flattened (the implicit im2col of a channels-last conv)"""
    return np.stack([A[lda_rows * t: lda_rows * t + k].reshape(-1) for t in range(M)])


@pytest.mark.parametrize("M,k", [(15999, 3), (7999, 3), (3999, 3), (1999, 3), (999, 2), (499, 2), (49, 2), (16, 2)])
def test_sv_gemm_feature_conv(lib, M, k):
    """conv 1-6: stride 2 over [T][512] f16 rows, lda 1024, K = 512 k, N 512, GELU, zero bias (conv_bias = False)"""
    rng = np.random.default_rng(M)
    Tin = 2 * (M - 1) + k
    A = (rng.standard_normal((Tin, 512)) * 0.5).astype(np.float16)
    Wt = (rng.standard_normal((512, 512 * k)) * 0.03).astype(np.float16)
    got = _gemm(lib, A, 1024, M, Wt, np.zeros(512, np.float32), 1)
    ref = R.gelu(_im2col(A.astype(np.float64), 2, M, k) @ Wt.astype(np.float64).T)
    e = _close(got, ref, 1e-3, 2e-3, 2e-3, f"conv gemm M={M} k={k}")
    print(f"sv conv GEMM M={M} k={k}: rel-L2 {e:.2e}")


@pytest.mark.parametrize("T", [16, 17, 149, 499])
def test_sv_gemm_tdnn(lib, T):
    """TDNN 0: k5 windows overlapping by 4 rows (lda 512, K 2560), f32 out; TDNN 4: N 1500 padded to 1536 with zero weight rows
    and bias, whose columns must come out exactly 0"""
    rng = np.random.default_rng(400 + T)
    A = (rng.standard_normal((T, 512)) * 0.5).astype(np.float16)
    Wt = (rng.standard_normal((512, 2560)) * 0.03).astype(np.float16)
    b = rng.standard_normal(512).astype(np.float32)
    M = T - 4
    got = _gemm(lib, A, 512, M, Wt, b, 4)
    ref = _im2col(A.astype(np.float64), 1, M, 5) @ Wt.astype(np.float64).T + b
    _close(got, ref, 1e-5, 1e-4, 1e-5, f"tdnn0 T={T}")
    W4 = np.zeros((1536, 512), np.float16)
    W4[:1500] = (rng.standard_normal((1500, 512)) * 0.05).astype(np.float16)
    b4 = np.zeros(1536, np.float32)
    b4[:1500] = rng.standard_normal(1500)
    M4 = T - 14 if T > 15 else 2
    got = _gemm(lib, A, 512, M4, W4, b4, 4)
    assert (got[:, 1500:] == 0).all()
    _close(got, A[:M4].astype(np.float64) @ W4.astype(np.float64).T + b4, 1e-5, 1e-4, 1e-5, f"tdnn4 T={T}")


@pytest.mark.parametrize("M", [16, 17, 149, 499])
@pytest.mark.parametrize("K,N,flags", [(768, 768, 2 | 4), (3072, 768, 2 | 4), (768, 2304, 0), (768, 3072, 1)])
def test_sv_gemm_encoder_layer(lib, M, K, N, flags):
    """the encoder layer's GEMMs at speaker-verification lengths: out-projection and FFN2 with the f32 residual (flags 2|4), QKV, FFN1"""
    rng = np.random.default_rng(M * 11 + K + N)
    A = (rng.standard_normal((M, K)) * 0.5).astype(np.float16)
    Wt = (rng.standard_normal((N, K)) * 0.03).astype(np.float16)
    b = rng.standard_normal(N).astype(np.float32)
    res = rng.standard_normal((M, N)).astype(np.float32) if flags & 2 else None
    got = _gemm(lib, A, K, M, Wt, b, flags, res)
    ref = A.astype(np.float64) @ Wt.astype(np.float64).T + b
    if flags & 1:
        ref = R.gelu(ref)
    if flags & 2:
        ref = ref + res
    tol = 1e-5 if flags & 4 else 1e-3
    _close(got, ref, tol, 10 * tol, tol, f"gemm M={M} K={K} N={N} flags={flags}")
