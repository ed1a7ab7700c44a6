"""-m gpu: the int8 encoder's three kernels through their taps, at the shapes the model takes and at the edges tests/test_gpu_enc_i8.py leaves out.

GEMM: that file's bound per written element (c = 4, 5 with the residual), the fill pattern kept outside the outputs, two runs equal word for word
(tests/enc_i8_taps.py gemm_case) - at the K the FFN2 and FFN1 of every model width have on every tile form, on grids the workgroup regrouping
really permutes, and with utterance boundaries inside a tile.  Quantisers: bytes and scale words equal wis_hip.weights.quantize_rows over 4096
scales and at every round-count boundary.  Refusals: the launcher's code, and nothing written.  Figures: profiles/enc_int8_tests.md."""
import numpy as np
import pytest

from enc_i8_taps import BOUNDARY_CASES, _buf, _kept, gemm_case

pytestmark = pytest.mark.gpu
E_ARG, E_UNSUPPORTED = -1, -7


# (epilogue, form, M or (B, T), N or H, K) as in test_gpu_enc_i8.py.  Deep K: 40, 16 and 10 k-tiles - FFN2 of d = 1280 / 512 and the d = 1280 projections - on the
# forms that stage a k-tile ahead (2, 3) and on 128 x 128, one row more than the form's height
@pytest.mark.parametrize("epi,form,m,n,k", [
    (2, 2, 65, 128, 5120), (2, 3, 257, 256, 5120), (2, 1, 129, 128, 2048), (1, 2, 65, 128, 1280), (1, 3, 257, 256, 1280), (3, 3, (1, 260), 20, 1280)])
def test_gemm_i8_deep_k(lib, epi, form, m, n, k):
    gemm_case(lib, epi, form, m, n, k)


# 9, 15, 9 and 16 workgroups: from 8 on the kernel's regrouping of the workgroup id (q = nwg >> 3, r = nwg & 7) is a real permutation, with r != 0 in the first
# three.  A tile computed from another tile's operands, or left out, breaks the per-element bound or the fill check: nothing else to assert
@pytest.mark.parametrize("form,M,N,nwg", [(1, 257, 384, 9), (2, 129, 640, 15), (3, 513, 768, 9), (2, 193, 512, 16)])
def test_gemm_i8_regrouped_grids(lib, form, M, N, nwg):
    bm, bn = {1: (128, 128), 2: (64, 128), 3: (256, 256)}[form]
    assert -(-M // bm) * (N // bn) == nwg >= 8
    gemm_case(lib, 0, form, M, N, 128)


@pytest.mark.parametrize("epi,form,bt,h,k", BOUNDARY_CASES)
def test_gemm_i8_utterance_boundary_inside_a_tile(lib, epi, form, bt, h, k):
    gemm_case(lib, epi, form, bt, h, k)


def _quant(lib, rows, M_fill=2):
    """wis_op_quant_rows on f16 rows -> (bytes, scales) of the rows, after checking the fill pattern behind them"""
    from wis_hip._lib import DevBuf, check
    M, K = rows.shape
    q_d, s_d, x_d = DevBuf.from_numpy(_buf((M + M_fill) * K, np.int8)), DevBuf.from_numpy(_buf(M + M_fill, np.float32)), DevBuf.from_numpy(rows)
    check(lib.wis_op_quant_rows(0, x_d.ptr, q_d.ptr, s_d.ptr, M, K))
    q, s = q_d.to_numpy(np.int8, (M + M_fill, K)), s_d.to_numpy(np.float32, (M + M_fill,))
    assert _kept(q[M:]) and _kept(s[M:])
    return q[:M], s[:M]


def _fused(lib, x, g, b, with_y):
    """wis_op_layernorm_quant on f32 rows -> (bytes, scales, wis_op_layernorm's f16 rows of the same input); the kernel's own f16 rows, when asked
    for, equal those; the fill pattern stays behind every output, and in the f16 rows when they are not asked for"""
    from wis_hip._lib import DevBuf, check
    M, d = x.shape
    q_d, s_d, y_d = DevBuf.from_numpy(_buf((M + 2) * d, np.int8)), DevBuf.from_numpy(_buf(M + 2, np.float32)), DevBuf.from_numpy(_buf((M + 2) * d, np.float16))
    x_d, g_d, b_d, y0_d = DevBuf.from_numpy(x), DevBuf.from_numpy(g), DevBuf.from_numpy(b), DevBuf(M * d * 2)
    check(lib.wis_op_layernorm(0, x_d.ptr, g_d.ptr, b_d.ptr, y0_d.ptr, M, d))
    rows = y0_d.to_numpy(np.float16, (M, d))
    check(lib.wis_op_layernorm_quant(0, x_d.ptr, g_d.ptr, b_d.ptr, q_d.ptr, s_d.ptr, y_d.ptr if with_y else None, M, d))
    q, s, y = q_d.to_numpy(np.int8, (M + 2, d)), s_d.to_numpy(np.float32, (M + 2,)), y_d.to_numpy(np.float16, (M + 2, d))
    assert _kept(q[M:]) and _kept(s[M:]) and _kept(y[M if with_y else 0:])
    assert not with_y or np.array_equal(y[:M].view(np.uint16), rows.view(np.uint16))
    return q[:M], s[:M], rows


def _same(q, s, rows):
    from wis_hip import weights as W
    qr, sr = W.quantize_rows(rows)
    bad = np.flatnonzero((q != qr).any(1) | (s.view(np.uint32) != sr.view(np.uint32)))
    assert bad.size == 0, (bad.size, bad[:8], [int((q[i] != qr[i]).sum()) for i in bad[:8]])


def test_quant_rows_over_4096_scales(lib):
    """enc_i8_ref.scale_family: 4096 rows, 4096 scales over f16's whole normal range, half of every row on the rounding boundaries.  A reciprocal one ulp
    off, or a division in place of the multiplication by it, changes hundreds of these bytes (tests/test_enc_i8_cpu.py counts them)"""
    from enc_i8_ref import scale_family
    rows = scale_family(4096, 128, seed=8)
    _same(*_quant(lib, rows), rows)


def test_layernorm_quant_over_many_scales(lib):
    """enc_i8_ref.ln_scale_family, d = 256, 4096 rows: as many different scales as a LayerNorm's output can have (about 1900 - that docstring says why
    not 4096); the off-by-an-ulp variants change some tens of these bytes (tests/test_enc_i8_cpu.py counts them on a numpy LayerNorm of the rows)"""
    from enc_i8_ref import ln_scale_family
    q, s, rows = _fused(lib, *ln_scale_family(4096, 256, seed=256), True)
    assert np.unique(s).size > 1500 and s.max() > 3 * s.min()
    _same(q, s, rows)


def _edge_rows(rng, M, K, tail):
    """[M][K] float32: row 0 absmax (positive) inside the last `tail` values, row 1 absmax negative at column 3 mod K, row 2 all zero, row 3 absmax
    negative at the very last value, the rest random"""
    x = rng.standard_normal((M, K)).astype(np.float32)
    x[0, K - 1 - (K // 3) % tail], x[1, 3 % K], x[2], x[3, K - 1] = 9.5, -11.25, 0, -7.75
    return x


# the row quantiser's rounds of 64 x 8 values: K = 8 one lane, 512 one full round, 520 one lane of the second, 1536 three rounds, 2048 all four of quant_rows_kernel<4>,
# 2056 the first K of quant_rows_kernel<10>, 3072 six of its ten rounds, 4096 eight.  M = 4: one whole workgroup of four rows; 5: a second one with three idle waves
@pytest.mark.parametrize("M", [4, 5])
@pytest.mark.parametrize("K", [8, 512, 520, 1536, 2048, 2056, 3072, 4096])
def test_quant_rows_round_boundaries(lib, M, K):
    rows = (_edge_rows(np.random.default_rng(K + M), M, K, 8) * 0.7).astype(np.float16)
    q, s = _quant(lib, rows)
    _same(q, s, rows)
    assert s[2] == 1 and not q[2].any() and q[0].max() == 127 and q[1].min() == -127 and q[3, -1] == -127


# the fused kernel's eight rounds of 64 x 4 values: d = 4 one lane, 256 one round, 260 one lane of the second, 512 / 768 / 1024 the model widths below 1280 (two, three,
# four rounds), 2048 all eight - the launcher's limit
@pytest.mark.parametrize("with_y", [False, True])
@pytest.mark.parametrize("M", [4, 5])
@pytest.mark.parametrize("d", [4, 256, 260, 512, 768, 1024, 2048])
def test_layernorm_quant_round_boundaries(lib, M, d, with_y):
    rng = np.random.default_rng(d + M)
    x = _edge_rows(rng, M, d, 4) * 3 + 1
    x[2] = 0.25      # a constant row: the output is beta - all zero in the second run
    x = x.astype(np.float32)
    g, b = (1 + 0.05 * rng.standard_normal(d)).astype(np.float32), (0.01 * rng.standard_normal(d)).astype(np.float32)
    for beta in (b, np.zeros(d, np.float32)):
        q, s, rows = _fused(lib, x, g, beta, with_y)
        _same(q, s, rows)
        if d >= 256:      # (the planted outliers dominate their rows: the absmax is where it was put, with its sign)
            assert q[0, d - 1 - (d // 3) % 4] == 127 and q[1, 3] == -127 and q[3, -1] == -127
    assert s[2] == 1 and not q[2].any() and not rows[2].any()


def test_refusals_write_nothing(lib):
    """every case returns before any launch (csrc/enc_kernels.hip: launch_quant_rows, launch_layernorm_quant, launch_gemm_i8_t, launch_gemm_i8_generic;
    csrc/taps.hip: wis_op_gemm_i8's own check of the cross-K/V geometry): the launcher's code, and every output buffer still holds its fill pattern"""
    from wis_hip._lib import DevBuf
    n = 8 * 5128
    x_d, g_d = DevBuf.from_numpy(np.zeros(n, np.float32)), DevBuf.from_numpy(np.ones(5128, np.float32))
    outs = [DevBuf.from_numpy(_buf(n, np.int8)), DevBuf.from_numpy(_buf(64, np.float32)), DevBuf.from_numpy(_buf(n, np.float16))]
    q_d, s_d, y_d = outs
    for K in (12, 5128):
        assert lib.wis_op_quant_rows(0, x_d.ptr, q_d.ptr, s_d.ptr, 4, K) == E_UNSUPPORTED and b"quant_rows" in lib.wis_last_error(), K
    for d in (6, 2052):
        assert lib.wis_op_layernorm_quant(0, x_d.ptr, g_d.ptr, g_d.ptr, q_d.ptr, s_d.ptr, y_d.ptr, 4, d) == E_UNSUPPORTED and b"layernorm_quant" in lib.wis_last_error(), d
    a_d, w_d = DevBuf.from_numpy(np.ones(4 * 384, np.int8)), DevBuf.from_numpy(np.ones(1024 * 384, np.int8))
    sa_d, sw_d = DevBuf.from_numpy(np.ones(4, np.float32)), DevBuf.from_numpy(np.ones(1024, np.float32))
    c_d, v_d = DevBuf.from_numpy(_buf(8 * 1024, np.float32)), DevBuf.from_numpy(_buf(8 * 1024, np.float32))
    outs += [c_d, v_d]
    gemm = lambda M, N, K, epi, flags, form, dims=(0, 0, 0, 0), out2=None, ls=(0, 0): lib.wis_op_gemm_i8(
        0, a_d.ptr, sa_d.ptr, w_d.ptr, sw_d.ptr, sw_d.ptr, None, c_d.ptr, out2, M, N, K, epi, flags, form, *dims, *ls)
    assert gemm(4, 192, 128, 0, 0, 1) == E_UNSUPPORTED and b"N=192" in lib.wis_last_error()
    assert gemm(4, 128, 192, 0, 0, 1) == E_UNSUPPORTED and b"K=192" in lib.wis_last_error()
    assert gemm(4, 384, 128, 0, 4, 3) == E_ARG and b"256 x 256" in lib.wis_last_error()
    assert gemm(4, 128, 128, 0, 2, 1) == E_ARG and b"without a residual" in lib.wis_last_error()
    # cross K/V, d = 128 (H = 2), B T = 1 x 4: N = 384 is a layer and a half; the layer strides are those of a valid call
    assert gemm(4, 384, 128, 4, 0, 1, (1, 4, 2, 1), v_d.ptr, (4 * 128 + 8, 128 * 64 + 8)) == E_ARG and b"cross K/V" in lib.wis_last_error()
    for o in outs:
        assert _kept(o.to_numpy(np.uint8, (o.nbytes,)))
    # (the last call again with N = 256, one whole layer: it runs and writes the 512 K values - it was refused for its N alone)
    assert gemm(4, 256, 128, 4, 0, 1, (1, 4, 2, 1), v_d.ptr, (4 * 128 + 8, 128 * 64 + 8)) == 0
    c = c_d.to_numpy(np.float16, (1024,))
    assert not _kept(c[:512]) and _kept(c[512:])
