"""The five-column slabs of the one-utterance FFN2 (dec_kernels.hip gemv_nc5_kernel<40> on N / 5 workgroups), through the wis_op_gemv_cols tap at cols = 5: it
prepares the projection as the loader does (sixteen-column image, five-column image from launch_pack_gemv_nc5) and lets the step's own stage builder
(gemv_small) pick the kernel.  The image's numpy model covers both wave K-ranges of the layout (40 k-steps: remainder one; 20: remainder two).

The same-bits claim: for the same inputs cols = 5 writes the words cols = 16 writes.  The sixteen-column kernel stores four columns at a time and needs
N % 16 == 0 through this tap, so its run gets the matrix padded with zero rows to the next multiple of 16 (bias, residual rows and output padded alike) and its
first N columns are compared: a column's sum does not depend on its neighbours.
K = 5120; N = 5 (one slab), 15 (an odd slab count), 35, and 1280 once (256 workgroups); rows 1 and 5; residual epilogue with and without the f16 copy.
The float64 bounds are test_gpu_ops.py test_gemv's for the same K and input distribution (relative L2 error 1e-3 for an fp32 output; no element off by more than
0.05 (1 + max |ref|)).  (FFN1 on such slabs was built and measured slower than its two-tile kernel - DESIGN.md section 4 - and is not in the library.)"""
import ctypes
import functools

import numpy as np
import pytest

F = np.float64
GV_GELU, GV_RESID, GV_OUT_F32 = 1, 2, 4
GUARD = 512      # sentinel elements on either side of an output


# ---- the image and the three rotated issues, in numpy ------------------------------------------------------------------------------------------------------
def pack_nc5(W, kw):
    """dec_kernels.hip pack_gemv_nc5_kernel: [N/5 slabs][K/32/kw wave K-ranges][ceil(kw/3) requests][64 lanes][8] - lane l carries A-fragment row l & 15 and
    k-quarter l >> 4; rows 5j .. 5j + 4 (j = 0, 1, 2) hold the slab's five columns for k-step 3u + j of the K-range, row 15 and k-steps past the range are zero."""
    N, K = W.shape
    rq, nr = (kw + 2) // 3, K // 32 // kw
    img = np.zeros((N // 5, nr, rq, 64, 8), W.dtype)
    for l in range(64):
        row, kq = l & 15, l >> 4
        if row == 15:
            continue
        j, c = divmod(row, 5)
        for u in range(rq):
            if 3 * u + j >= kw:
                continue
            for rg in range(nr):
                k = 32 * (rg * kw + 3 * u + j) + 8 * kq
                img[:, rg, u, l, :] = W[c::5, k:k + 8]
    return img


def unpack_nc5(img, N, K, kw):
    """what the slab kernels multiply: per request the registers as they landed, then rotated LEFT by five lanes within each row of 16 (lane l takes lane
    (l + 5) & 15 of its row: DPP row_ror:11), then by ten (row_ror:6); of each issue's A operand, rows 0-4 are the columns the epilogue stores."""
    rq, nr = (kw + 2) // 3, K // 32 // kw
    img = img.reshape(N // 5, nr, rq, 64, 8)
    W = np.zeros((N, K), img.dtype)
    seen = np.zeros((N, K), bool)
    lanes = np.arange(64)
    for j in range(3):
        a = img[:, :, :, (lanes & ~15) | ((lanes + 5 * j) & 15), :]      # the MFMA's A operand of issue j
        for l in lanes[(lanes & 15) < 5]:
            for u in range(rq):
                if 3 * u + j >= kw:      # the kernel issues no MFMA for a k-step past the range
                    continue
                for rg in range(nr):
                    k = 32 * (rg * kw + 3 * u + j) + 8 * (l >> 4)
                    W[(l & 15)::5, k:k + 8] = a[:, rg, u, l, :]
                    seen[(l & 15)::5, k:k + 8] = True
    assert seen.all()
    return W


@pytest.mark.parametrize("N", [5, 15, 35, 1280])
@pytest.mark.parametrize("K,kw", [(1280, 40), (1280, 20), (5120, 40), (5120, 20)])
def test_five_column_image_round_trip(N, K, kw):
    """both wave K-ranges (40 k-steps: thirteen requests of three and one of one; 20: six of three and one of two) at both depths"""
    rng = np.random.default_rng(N + K + kw)
    W = rng.standard_normal((N, K)).astype(np.float16)
    img = pack_nc5(W, kw)
    rq = (kw + 2) // 3
    assert img.shape == (N // 5, K // 32 // kw, rq, 64, 8)
    assert np.array_equal(unpack_nc5(img, N, K, kw).view(np.uint16), W.view(np.uint16))
    # row 15 of every request and the k-steps past a range are zero; nothing else is lost: the image holds each weight once
    assert not img[:, :, :, 15::16, :].any()
    assert np.count_nonzero(img) == np.count_nonzero(W)
    # the wrong direction (rows 11-15 into rows 0-4) does not reproduce the matrix
    lanes = np.arange(64)
    wrong = img[:, :, :, (lanes & ~15) | ((lanes - 5) & 15), :]
    assert not np.array_equal(wrong[:, 0, 0, :5, :], W[:, 32:40].reshape(N // 5, 5, 8))


# ---- GPU ---------------------------------------------------------------------------------------------------------------------------------------------------
def _pad16(a, axis):
    n = a.shape[axis]
    pad = [(0, 0)] * a.ndim
    pad[axis] = (0, -n % 16)
    return np.pad(a, pad)


def _guarded(body, dtype):
    host = np.full(body.size + 2 * GUARD, -77.0, dtype)
    host[GUARD:GUARD + body.size] = body.reshape(-1)
    return host


def _guards_intact(a, n):
    v = a.view(np.uint16 if a.itemsize == 2 else np.uint32)
    s = np.array([-77.0], a.dtype).view(v.dtype)[0]
    return bool((v[:GUARD] == s).all() and (v[GUARD + n:] == s).all())


def _at(buf, itemsize):
    return ctypes.c_void_p(buf.ptr.value + GUARD * itemsize)


@functools.lru_cache(maxsize=None)
def _ffn2_case(M, N):
    """test_gemv's inputs at K = 5120; the float64 product of the f16 values, computed once"""
    K = 5120
    rng = np.random.default_rng(M * 31 + N + K)
    W = (rng.standard_normal((N, K)) * 0.05).astype(np.float16)
    bias = rng.standard_normal(N).astype(np.float32)
    x = rng.standard_normal((M, K)).astype(np.float16)
    y0 = rng.standard_normal((M, N)).astype(np.float32)
    ref = x.astype(F) @ W.astype(F).T + bias + y0
    for a in (W, bias, x, y0, ref):
        a.setflags(write=False)
    return W, bias, x, y0, ref


def _run_ffn2(lib, M, N, cols, want_y16):
    """-> (y [M][N] fp32, y16 [M][N] or None, guards intact); cols = 16 runs on the matrix padded to a multiple of 16 columns"""
    from wis_hip._lib import DevBuf, check
    W, bias, x, y0, _ = _ffn2_case(M, N)
    if cols == 16:
        W, bias, y0 = _pad16(W, 0), _pad16(bias, 0), _pad16(y0, 1)
    Nr = W.shape[0]
    host = _guarded(y0, np.float32)
    h16 = np.full(M * Nr + 2 * GUARD, -77.0, np.float16)
    dx, dW, db, dy = DevBuf.from_numpy(x), DevBuf.from_numpy(np.ascontiguousarray(W)), DevBuf.from_numpy(bias), DevBuf.from_numpy(host)
    d16 = DevBuf.from_numpy(h16) if want_y16 else None
    check(lib.wis_op_gemv_cols(0, dx.ptr, dW.ptr, db.ptr, _at(dy, 4), _at(d16, 2) if want_y16 else None, M, Nr, 5120, GV_RESID, cols))
    raw = dy.to_numpy(np.float32, host.shape)
    raw16 = d16.to_numpy(np.float16, h16.shape) if want_y16 else None
    ok = _guards_intact(raw, M * Nr) and (raw16 is None or _guards_intact(raw16, M * Nr))
    body = lambda a: a[GUARD:GUARD + M * Nr].reshape(M, Nr)[:, :N]
    return body(raw), (body(raw16) if want_y16 else None), ok


FFN2_SHAPES = [(M, N) for N in (5, 15, 35) for M in (1, 5)] + [(5, 1280)]


@pytest.mark.gpu
@pytest.mark.parametrize("M,N", FFN2_SHAPES)
def test_ffn2_five_columns(lib, M, N):
    """bit-equal to the sixteen-column kernel (every element sees its wave's k-steps in that order through the same MFMA, then the same cross-wave sum and
    epilogue), inside test_gemv's float64 bounds, and nothing written but the M x N outputs - with and without the f16 copy"""
    ref = _ffn2_case(M, N)[4]
    for want_y16 in (True, False):
        a, a16, a_ok = _run_ffn2(lib, M, N, 5, want_y16)
        b, b16, b_ok = _run_ffn2(lib, M, N, 16, want_y16)
        e = float(np.linalg.norm(a.astype(F) - ref) / (np.linalg.norm(ref) + 1e-30)); worst = float(np.abs(a.astype(F) - ref).max())
        print(f"FFN2 5 columns M{M} N{N} y16={int(want_y16)}: rel err {e:.3e} max abs {worst:.3e}, words differing from 16 columns {int((a.view(np.uint32) != b.view(np.uint32)).sum())}")
        assert a_ok and b_ok, "a store outside the M x N output"
        assert not (a == -77.0).any()
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
        assert e < 1e-3 and worst < 0.05 * (1 + float(np.abs(ref).max()))
        if want_y16:
            assert np.array_equal(a16.view(np.uint16), b16.view(np.uint16))
            assert np.array_equal(a16.view(np.uint16), a.astype(np.float16).view(np.uint16))      # the f16 copy: the fp32 rows, rounded


@functools.lru_cache(maxsize=None)
def _other_case(M, N):
    rng = np.random.default_rng(M * 31 + N + 5120)
    W = (rng.standard_normal((N, 5120)) * 0.05).astype(np.float16)
    bias = rng.standard_normal(N).astype(np.float32)
    x = rng.standard_normal((M, 5120)).astype(np.float16)
    y0 = rng.standard_normal((M, N)).astype(np.float32)
    return W, bias, x, y0


@pytest.mark.gpu
@pytest.mark.parametrize("M,N,w8", [(5, 1024, 0), (9, 1280, 0), (5, 1280, 1)])
def test_shapes_the_predicate_refuses_take_the_other_kernels(lib, M, N, w8):
    """cols = 5 on what gemv_nc5_shape (or the missing image) refuses: N no multiple of five, more rows than the register staging holds, 8-bit weights (tap flag
    32) - the sixteen-column kernels run, and the results stand inside test_gemv's float64 bounds"""
    from wis_hip._lib import DevBuf, check
    W, bias, x, y0 = _other_case(M, N)
    Wref = W.astype(F)
    if w8:
        from wis_hip.weights import quantize_rows
        q, sc = quantize_rows(W)
        Wref = q.astype(F) * sc.astype(F)[:, None]
    ref = x.astype(F) @ Wref.T + bias + y0
    host = _guarded(y0, np.float32)
    dx, dW, db, dy = DevBuf.from_numpy(x), DevBuf.from_numpy(W), DevBuf.from_numpy(bias), DevBuf.from_numpy(host)
    check(lib.wis_op_gemv_cols(0, dx.ptr, dW.ptr, db.ptr, _at(dy, 4), None, M, N, 5120, GV_RESID | (32 if w8 else 0), 5))
    raw = dy.to_numpy(np.float32, host.shape)
    a = raw[GUARD:GUARD + M * N].reshape(M, N).astype(F)
    e = float(np.linalg.norm(a - ref) / (np.linalg.norm(ref) + 1e-30)); worst = float(np.abs(a - ref).max())
    print(f"FFN2 stage, cols = 5 refused, M{M} N{N} w8={w8}: rel err {e:.3e} max abs {worst:.3e}")
    assert _guards_intact(raw, M * N)
    assert e < 1e-3 and worst < 0.05 * (1 + float(np.abs(ref).max()))
