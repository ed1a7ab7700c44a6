"""The eight-column workgroup tiles of the one-utterance FFN2 / cross-attention out-projection (dec_kernels.hip gemv_body NC = 8:
gemv_kernel<1, 2, 40 | 10, 1, false, 1, 8> on N / 8 workgroups), through the wis_op_gemv_cols tap, which packs the image like the loader does and
calls launch_gemv with GemvP::rows = 8 (cols = 16: the sixteen-column form of the same shapes, gemv_kernel<1, 2, 40 | 10, 1, false>).

K is what the two instantiations fix (1280, 5120); N = 8, 24, 136: one tile, an odd tile count, more tiles than a small grid's first dispatch round, and
1280 once; rows 1, 5 and the most the register staging of the rows holds (M K / 8 <= 13 x 256: 16 at K = 1280, 5 at K = 5120).  The float64 bounds are
test_gpu_ops.py test_gemv's for the same K and the same input distribution (relative L2 error 1e-3 for an fp32 output, 2e-3 for f16; no element off by
more than 0.05 (1 + max |ref|))."""
import ctypes
import functools

import numpy as np
import pytest

F = np.float64
KS = (1280, 5120)
GV_GELU, GV_RESID, GV_OUT_F32 = 1, 2, 4
GUARD = 512      # sentinel elements on either side of an output


def _rows(K):
    return (1, 5, 16) if K == 1280 else (1, 5)


def pack_nc8(W):
    """dec_kernels.hip pack_gemv_nc8_kernel: [N/8][K/64][64 lanes][8] - lane l carries column 8 nt + (l & 7), k-step 2 kp + ((l >> 3) & 1), k-quarter l >> 4."""
    N, K = W.shape
    l = np.arange(64)
    n = 8 * np.arange(N // 8)[:, None, None, None] + (l & 7)[None, None, :, None]
    k = 64 * np.arange(K // 64)[None, :, None, None] + (32 * ((l >> 3) & 1) + 8 * (l >> 4))[None, None, :, None] + np.arange(8)[None, None, None, :]
    return W[n, k]


def unpack_nc8(img, N, K):
    """what gemv_body NC = 8 multiplies: per request the registers as they land (A-fragment rows 0-7 = lanes with l & 15 < 8: the even k-step), then rotated by
    eight lanes within each row of 16 (the odd k-step); A-fragment lane l = row (l & 15), k-quarter (l >> 4)."""
    img = img.reshape(N // 8, K // 64, 64, 8)
    W = np.zeros((N, K), img.dtype)
    lanes = np.arange(64)
    for half, src in ((0, lanes), (1, lanes ^ 8)):
        a = img[:, :, src, :]                    # the MFMA's A operand of this issue
        for l in lanes[(lanes & 15) < 8]:        # rows 0-7 of the fragment: the columns the epilogue stores
            for nt in range(N // 8):
                n = 8 * nt + (l & 15)
                kk = 64 * np.arange(K // 64)[:, None] + 32 * half + 8 * (l >> 4) + np.arange(8)[None, :]
                W[n, kk] = a[nt, :, l, :]
    return W


@pytest.mark.parametrize("N", [8, 24, 136, 1280])
@pytest.mark.parametrize("K", KS)
def test_eight_column_image_round_trip(N, K):
    rng = np.random.default_rng(N + K)
    W = rng.standard_normal((N, K)).astype(np.float16)
    img = pack_nc8(W)
    assert img.shape == (N // 8, K // 64, 64, 8) and img.size == W.size
    assert np.array_equal(unpack_nc8(img, N, K).view(np.uint16), W.view(np.uint16))


@functools.lru_cache(maxsize=None)
def _case(M, N, K):
    """test_gemv's inputs; the float64 product of the f16 values, computed once"""
    rng = np.random.default_rng(M * 31 + N + K)
    W = (rng.standard_normal((N, K)) * 0.05).astype(np.float16)
    bias = rng.standard_normal(N).astype(np.float32)
    x = rng.standard_normal((M, K)).astype(np.float16)
    y0 = rng.standard_normal((M, N)).astype(np.float32)
    prod = x.astype(F) @ W.astype(F).T
    for a in (W, bias, x, y0, prod):
        a.setflags(write=False)
    return W, bias, x, y0, prod


def _gelu(v):
    from math import erf
    return 0.5 * v * (1.0 + np.vectorize(erf)(v / np.sqrt(2.0)))


def _run(lib, M, N, K, flags, with_bias, cols, want_y16=False):
    """-> (y with its guards, y16 with its guards or None) as raw arrays; y is fp32 under GV_RESID / GV_OUT_F32 else f16"""
    from wis_hip._lib import DevBuf, check
    W, bias, x, y0, _ = _case(M, N, K)
    f32 = bool(flags & (GV_RESID | GV_OUT_F32))
    ydt = np.float32 if f32 else np.float16
    host = np.full(M * N + 2 * GUARD, -77.0, ydt)
    if flags & GV_RESID:
        host[GUARD:GUARD + M * N] = y0.reshape(-1)
    dx, dW, db, dy = DevBuf.from_numpy(x), DevBuf.from_numpy(W), DevBuf.from_numpy(bias), DevBuf.from_numpy(host)
    h16 = np.full(M * N + 2 * GUARD, -77.0, np.float16)
    d16 = DevBuf.from_numpy(h16) if want_y16 else None
    at = lambda b, es: ctypes.c_void_p(b.ptr.value + GUARD * es)
    check(lib.wis_op_gemv_cols(0, dx.ptr, dW.ptr, db.ptr if with_bias else None, at(dy, host.itemsize), at(d16, 2) if want_y16 else None, M, N, K, flags, cols))
    return dy.to_numpy(ydt, host.shape), (d16.to_numpy(np.float16, h16.shape) if want_y16 else None)


def _body(a, M, N):
    return a[GUARD:GUARD + M * N].reshape(M, N)


def _guards_intact(a, M, N):
    s = np.array([-77.0], a.dtype).view(np.uint16 if a.itemsize == 2 else np.uint32)[0]
    v = a.view(np.uint16 if a.itemsize == 2 else np.uint32)
    return bool((v[:GUARD] == s).all() and (v[GUARD + M * N:] == s).all())


# residual + bias (the product's epilogue), neither (fp32 output), bias + GELU to f16
VARIANTS = [(GV_RESID, True), (GV_OUT_F32, False), (GV_GELU, True)]
SHAPES = [(M, N, K) for K in KS for N in (8, 24, 136) for M in _rows(K)] + [(5, 1280, 1280), (5, 1280, 5120)]


@pytest.mark.gpu
@pytest.mark.parametrize("M,N,K", SHAPES)
def test_eight_columns_vs_fp64(lib, M, N, K):
    W, bias, x, y0, prod = _case(M, N, K)
    for flags, with_bias in VARIANTS:
        ref = prod + (bias if with_bias else 0.0)
        if flags & GV_GELU:
            ref = _gelu(ref)
        if flags & GV_RESID:
            ref = ref + y0
        raw, raw16 = _run(lib, M, N, K, flags, with_bias, 8, want_y16=bool(flags & GV_RESID))
        out = _body(raw, M, N).astype(F)
        e = float(np.linalg.norm(out - ref) / (np.linalg.norm(ref) + 1e-30)); worst = float(np.abs(out - ref).max())
        print(f"gemv 8 columns M{M} N{N} K{K} flags{flags} bias{int(with_bias)}: rel err {e:.3e} max abs {worst:.3e}")
        assert e < (1e-3 if raw.dtype == np.float32 else 2e-3), (flags, e)
        assert worst < 0.05 * (1 + float(np.abs(ref).max())), (flags, worst)
        if raw16 is not None:       # the f16 copy of the residual rows: the fp32 rows, rounded
            assert np.array_equal(_body(raw16, M, N).view(np.uint16), _body(raw, M, N).astype(np.float16).view(np.uint16))


@pytest.mark.gpu
@pytest.mark.parametrize("M,N,K", [(M, N, K) for K in KS for N in (16, 48, 144) for M in _rows(K)] + [(5, 1280, 1280), (5, 1280, 5120)])
def test_eight_columns_bit_equal_to_sixteen(lib, M, N, K):
    """every output element sees its wave's k-steps in the sixteen-column order through the same MFMA, and the same cross-wave sum"""
    for flags, with_bias in VARIANTS:
        y16 = bool(flags & GV_RESID)
        a, a16 = _run(lib, M, N, K, flags, with_bias, 8, want_y16=y16)
        b, b16 = _run(lib, M, N, K, flags, with_bias, 16, want_y16=y16)
        v = np.uint32 if a.dtype == np.float32 else np.uint16
        assert np.array_equal(a.view(v), b.view(v)), (flags, int((a.view(v) != b.view(v)).sum()))
        if y16:
            assert np.array_equal(a16.view(np.uint16), b16.view(np.uint16))


@pytest.mark.gpu
@pytest.mark.parametrize("M,N,K", SHAPES)
def test_eight_columns_write_nothing_else(lib, M, N, K):
    for flags, with_bias in VARIANTS:
        raw, raw16 = _run(lib, M, N, K, flags, with_bias, 8, want_y16=bool(flags & GV_RESID))
        assert _guards_intact(raw, M, N), (flags, "a store outside the M x N output")
        assert not (_body(raw, M, N) == -77.0).any()
        if raw16 is not None:
            assert _guards_intact(raw16, M, N), (flags, "a store outside the f16 copy")


@pytest.mark.gpu
def test_shapes_without_the_form_are_errors(lib):
    from wis_hip._lib import DevBuf
    d = DevBuf(1 << 20)
    assert lib.wis_op_gemv_cols(0, d.ptr, d.ptr, None, d.ptr, None, 6, 8, 5120, GV_OUT_F32, 8) == -7       # six rows of K = 5120 do not fit the register staging
    assert lib.wis_op_gemv_cols(0, d.ptr, d.ptr, None, d.ptr, None, 5, 8, 1024, GV_OUT_F32, 8) == -7       # K not instantiated
    assert lib.wis_op_gemv_cols(0, d.ptr, d.ptr, None, d.ptr, None, 5, 12, 1280, GV_OUT_F32, 8) != 0       # N not a multiple of the tile
