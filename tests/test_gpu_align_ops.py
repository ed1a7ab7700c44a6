"""-m gpu: the alignment kernels one by one through their C-ABI taps (wis_op_dtw, wis_op_align_matrix, include/wis_hip.h) against
tests/align_ref.py.

DTW: exact equality of both index arrays and the length with align_ref.dtw (openai-whisper dtw_cpu's loop), ties included.

Matrix: e = max |GPU - float64 reference|.  The bound is not tuned to the kernel: e_f16 is what storing K (and the query the MFMA /
dot product reads) in f16 costs the reference itself (float64 from the f32 inputs against float64 from the f16-rounded inputs); the
GPU may be at most 4 e_f16 + 3e-3 x max|matrix| (the 3e-3 of test_gpu_dec_attn.py, relative: different exp and summation order).
Heads whose weights are constant over the tokens (std 0: the reference yields NaN or inf depending on rounding) are not among the
inputs, except the one-token case, where every std is 0 and both sides must be NaN everywhere."""
import ctypes as C

import numpy as np
import pytest

import align_ref as R

pytestmark = pytest.mark.gpu


def _gpu_dtw(lib, x):
    from wis_hip import _lib
    N, M = x.shape
    cap, G = N + M - 1, 8
    d_x = _lib.DevBuf.from_numpy(np.ascontiguousarray(x, np.float32))
    sent = np.full(cap + 2 * G, -77, np.int32)
    d_t, d_f, d_l = _lib.DevBuf.from_numpy(sent), _lib.DevBuf.from_numpy(sent), _lib.DevBuf.from_numpy(np.full(1 + 2 * G, -77, np.int32))
    off = lambda d, n: C.c_void_p(d.ptr.value + 4 * n)
    _lib.check(lib.wis_op_dtw(0, d_x.ptr, N, M, off(d_t, G), off(d_f, G), off(d_l, G)))
    t, f, l = d_t.to_numpy(np.int32, sent.shape), d_f.to_numpy(np.int32, sent.shape), d_l.to_numpy(np.int32, (1 + 2 * G,))
    n = int(l[G])
    assert (l[:G] == -77).all() and (l[G + 1:] == -77).all()
    assert 1 <= n <= cap
    for a in (t, f):
        assert (a[:G] == -77).all() and (a[G + n:] == -77).all(), "guard words overwritten"
    return t[G:G + n].astype(np.int64), f[G:G + n].astype(np.int64)


@pytest.mark.parametrize("N,M", [(1, 1), (1, 9), (7, 1), (50, 20), (20, 50), (33, 17), (224, 1500), (448, 1500)])
@pytest.mark.parametrize("quant", [0, 2, 1])
def test_dtw_exact(N, M, quant, lib):
    rng = np.random.default_rng(1000 * N + M + quant)
    x = rng.standard_normal((N, M)).astype(np.float32)
    if quant:
        x = (np.round(x * quant) / quant).astype(np.float32)      # a few distinct values: ties everywhere
    ref_t, ref_f = R.dtw_fast(x)
    if N * M <= 2000:
        slow = R.dtw(x)
        assert np.array_equal(slow[0], ref_t) and np.array_equal(slow[1], ref_f)
    got_t, got_f = _gpu_dtw(lib, x)
    assert len(got_t) == len(ref_t), (len(got_t), len(ref_t))
    assert np.array_equal(got_t, ref_t) and np.array_equal(got_f, ref_f)


def _k_image(K16):
    """K f16 [H][T][64] -> the cross-attention image [H][8][T][8]"""
    H, T, _ = K16.shape
    return np.ascontiguousarray(K16.reshape(H, T, 8, 8).transpose(0, 2, 1, 3))


def _gpu_matrix(lib, q, K16, frames, width):
    from wis_hip import _lib
    H, N, _ = q.shape
    T = K16.shape[1]
    d_q, d_k = _lib.DevBuf.from_numpy(np.ascontiguousarray(q, np.float32)), _lib.DevBuf.from_numpy(_k_image(K16))
    d_o = _lib.DevBuf(N * frames * 4)
    _lib.check(lib.wis_op_align_matrix(0, d_q.ptr, d_k.ptr, N, H, T, frames, width, d_o.ptr))
    return d_o.to_numpy(np.float32, (N, frames)).astype(np.float64)


def _refs(q, K, frames, width):
    """float64 from the f32 inputs; float64 from the inputs as the engine stores / feeds them (K and q rounded to f16)"""
    a = R.matrix(R.attention_weights(q, K)[:, :, :frames], width)
    b = R.matrix(R.attention_weights(q.astype(np.float16), K.astype(np.float16))[:, :, :frames], width)
    return a, b


CASES = [(1, 1, 1500, 7), (1, 5, 1, 7), (3, 17, 3, 7), (2, 30, 4, 7), (1, 30, 750, 7), (6, 100, 1500, 7), (1, 224, 1500, 7), (320, 40, 750, 7),
         (320, 224, 1500, 7), (4, 61, 1500, 1), (2, 9, 40, 21)]


@pytest.mark.parametrize("H,N,frames,width", CASES)
def test_align_matrix_vs_ref(H, N, frames, width, lib):
    T = 1500
    rng = np.random.default_rng(31 * H + 7 * N + frames + width)
    K = (rng.standard_normal((H, T, 64)) * 0.6).astype(np.float32)
    q = (rng.standard_normal((H, N, 64)) * 0.5).astype(np.float32)
    ref, ref16 = _refs(q, K, frames, width)
    got = _gpu_matrix(lib, q, K.astype(np.float16), frames, width)
    if N == 1:      # one token: every std is 0, (w - mean) / std = 0 / 0
        assert np.isnan(ref).all() and np.isnan(got).all()
        return
    assert np.isfinite(ref).all() and np.isfinite(got).all()
    e, e16, scale = np.abs(got - ref).max(), np.abs(ref16 - ref).max(), np.abs(ref).max()
    print(f"align matrix heads={H} tokens={N} frames={frames} width={width}: e {e:.3e}  e_f16 {e16:.3e}  max|x| {scale:.3f}  bound {4 * e16 + 3e-3 * scale:.3e}")
    assert e <= 4 * e16 + 3e-3 * scale, (e, e16, scale)


@pytest.mark.parametrize("N,F,Hn", [(20, 400, 1), (12, 750, 2), (100, 1500, 3), (60, 1500, 6)])
def test_planted_alignment(N, F, Hn, lib):
    rng = np.random.default_rng(N + F + Hn)
    q, K, f = R.planted_inputs(rng, N, F, Hn)
    s = np.einsum("hnd,htd->hnt", q.astype(np.float64), K.astype(np.float16).astype(np.float64))
    on = np.array([[s[h, i, f[i]:f[i + 1]].min() for i in range(N)] for h in range(Hn)])
    offb = np.array([[np.delete(s[h, i], np.arange(f[i], f[i + 1])).max() for i in range(N)] for h in range(Hn)])
    assert (on - offb).min() >= 8.0, (on - offb).min()
    x = _gpu_matrix(lib, q, K.astype(np.float16), F, 7).astype(np.float32)
    ti, fi = _gpu_dtw(lib, x)
    jumps = np.pad(np.diff(ti), (1, 0), constant_values=1).astype(bool)
    assert jumps.sum() == N
    assert np.array_equal(fi[jumps], f[:-1]), (fi[jumps], f[:-1])
