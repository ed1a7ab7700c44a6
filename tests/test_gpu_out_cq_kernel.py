"""-m gpu: the fused out-projection + folded cross-Q stage's own kernel (dec_kernels.hip gemv_out_cq_kernel, selected by launch_gemv_dual for f16
weights, <= 8 rows, d = 384 / 1280) through wis_op_gemv_out_cq, as RAW 32-BIT WORDS against the same two problems run one at a time through
wis_op_gemv on the sixteen-column stand-alone kernel (gemv_kernel<1, 2, SC, 1, false>: the same k-steps per wave in the same order, the same
cross-wave sum, the same epilogue arithmetic):

  arm A   x1 = x0 + a Wo^T + bo              wis_op_gemv(x = a, W = Wo, bias = bo, y = x0 in place, GV_RESID), K = d
  arm B   q_raw = [f16(x0) | a] Wc^T + bc    wis_op_gemv(x = the host-side concatenation, W = Wc, bias = bc, GV_OUT_F32), K = 2 d

Wc = [W'q | W'q Wo] and bc = W'q bo are built on the device by the tap (build_cq_fold: a GEMM and a row-times-vector kernel, each with a summation
order of its own).  The weights here are signed powers of two on a quarter of the places, bo multiples of 1/8 and gamma = 1, so every product and
every partial sum of that preparation is exact in f16 / fp32 whatever the order, and the host builds the very same Wc and bc with integer
arithmetic.  The activations are ordinary random numbers: the kernels' own sums round at every step, and equal words mean equal order.

The stand-alone kernel has no tap that returns LayerNorm partials, so x1's partials are compared with an fp32 restatement of the epilogue's
arithmetic on the reference x1 (numpy float32 is IEEE, the library is compiled without contraction): per row and sixteen-column tile, with
q_i = (x0 + x1) + (x2 + x3) over the tile's four column quads, sum = (q_0 + q_1) + (q_2 + q_3), m = sum / 16 and, with
s_i = ((x0 - m)^2 + (x1 - m)^2) + ((x2 - m)^2 + (x3 - m)^2), M2 = (s_0 + s_1) + (s_2 + s_3).

Shapes: M in {1, 5, 8}; d = 384 (the smallest width the stage exists at) and 1280 (large's: the instantiation the kernel was written for; its
weights are 10 MB); d = 512, where the selection falls back to gemv_dual_kernel<4, 8> - the same comparison holds for it; rows with a large common
offset; matrices whose last column tile is the only non-zero one.  One fp64 comparison with the bounds of tests/test_gpu_dec_step_ops.py
(_out_cq_case: 1e-3 relative L2 and 0.05 (1 + max |ref|) for x1 and the finished query)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
F = np.float64
GV_RESID, GV_OUT_F32 = 2, 4      # csrc/kernels.hpp


def _sparse_pow2(rng, shape, mag):
    """+- mag on a quarter of the places, zero elsewhere"""
    return (rng.integers(-1, 2, size=shape) * (rng.random(shape) < 0.375) * mag).astype(np.float16)


def _inputs(M, d, offset, last_tile_only):
    rng = np.random.default_rng([M, d, int(offset), int(last_tile_only)])
    a = (rng.standard_normal((M, d)) + (30.0 if offset else 0.0)).astype(np.float16)
    x0 = (rng.standard_normal((M, d)) * 2 + (200.0 if offset else 0.3)).astype(np.float32)
    Wo, Wq = _sparse_pow2(rng, (d, d), 0.25), _sparse_pow2(rng, (d, d), 0.5)
    if last_tile_only:
        Wo[:d - 16] = 0; Wq[:d - 16] = 0
    bo = (rng.integers(-16, 17, size=d) / 8.0).astype(np.float32)
    bq = rng.standard_normal(d).astype(np.float32)
    g = np.ones(d, np.float32); be = (0.1 * rng.standard_normal(d)).astype(np.float32)
    return a, x0, Wo, bo, Wq, bq, g, be


def _fold_on_host(Wo, bo, Wq):
    """[W'q | W'q Wo] f16 [d][2d] and W'q bo: exact (multiples of 1/64 below 32 in size; of 1/128), so float64 holds them and the casts do not round"""
    wq = Wq.astype(F) * 0.125
    prod = wq @ Wo.astype(F)
    assert np.abs(prod).max() < 32 and np.array_equal(prod * 64, np.round(prod * 64))
    Wc = np.concatenate([wq, prod], axis=1).astype(np.float16)
    assert np.array_equal(Wc.astype(F), np.concatenate([wq, prod], axis=1))
    bc = wq @ bo.astype(F)
    assert np.array_equal(bc.astype(np.float32).astype(F), bc)
    return Wc, bc.astype(np.float32)


def _partials_f32(x1):
    """the residual epilogue's partials, restated in fp32 (module docstring): [M][d / 16][2]"""
    t = x1.reshape(x1.shape[0], -1, 4, 4)                    # [row][tile][quad][column of the quad]
    q = (t[..., 0] + t[..., 1]) + (t[..., 2] + t[..., 3])
    s = (q[..., 0] + q[..., 1]) + (q[..., 2] + q[..., 3])
    u = t - (s * np.float32(0.0625))[..., None, None]
    u = u * u
    p = (u[..., 0] + u[..., 1]) + (u[..., 2] + u[..., 3])
    m2 = (p[..., 0] + p[..., 1]) + (p[..., 2] + p[..., 3])
    assert s.dtype == np.float32 and m2.dtype == np.float32
    return np.stack([s, m2], -1)


def _gemv(lib, x, W, bias, y0, M, N, K, flags):
    from wis_hip._lib import DevBuf, check
    dx, dW, db, dy = (DevBuf.from_numpy(v) for v in (x, W, bias, y0))
    check(lib.wis_op_gemv(0, dx.ptr, None, None, dW.ptr, db.ptr, dy.ptr, M, N, K, flags))
    return dy.to_numpy(np.float32, (M, N))


def _run(lib, M, d, offset=False, last_tile_only=False):
    from wis_hip._lib import DevBuf, check
    ins = _inputs(M, d, offset, last_tile_only)
    a, x0, Wo, bo, Wq, bq, g, be = ins
    nt = d // 16
    bufs = [DevBuf.from_numpy(v) for v in ins]
    outs = {k: DevBuf.from_numpy(np.full(n, 77.0, np.float32)) for k, n in (("x1", M * d), ("stat", M * nt * 2), ("q", M * d), ("qcs", d), ("qb", d))}
    check(lib.wis_op_gemv_out_cq(0, *[b.ptr for b in bufs], outs["x1"].ptr, outs["stat"].ptr, outs["q"].ptr, None, outs["qcs"].ptr, outs["qb"].ptr, M, d, 0))
    x1 = outs["x1"].to_numpy(np.float32, (M, d)); stat = outs["stat"].to_numpy(np.float32, (M, nt, 2)); q = outs["q"].to_numpy(np.float32, (M, d))
    # the two problems one at a time on the stand-alone kernel
    Wc, bc = _fold_on_host(Wo, bo, Wq)
    x1_ref = _gemv(lib, a, Wo, bo, x0, M, d, d, GV_RESID)
    xcat = np.concatenate([x0.astype(np.float16), a], axis=1)
    q_ref = _gemv(lib, xcat, Wc, bc, np.full((M, d), 55.0, np.float32), M, d, 2 * d, GV_OUT_F32)
    stat_ref = _partials_f32(x1_ref)
    for name, got, ref in (("x1", x1, x1_ref), ("partials", stat, stat_ref), ("q_raw", q, q_ref)):
        diff = got.view(np.uint32) != ref.view(np.uint32)
        print(f"out+cq kernel M{M} d{d} offset={offset} last_tile_only={last_tile_only} {name}: {int(diff.sum())} of {diff.size} words differ")
        assert not diff.any(), (name, np.argwhere(diff)[:4].tolist())
    return ins, x1, q, outs["qcs"].to_numpy(np.float32, (d,)), outs["qb"].to_numpy(np.float32, (d,))


@pytest.mark.parametrize("d", [384, 1280])
@pytest.mark.parametrize("M", [1, 5, 8])
def test_out_cq_kernel_words_equal_the_stand_alone_kernel(lib, M, d):
    _run(lib, M, d)


def test_out_cq_falls_back_to_the_dual_kernel_at_other_widths(lib):
    """d = 512: launch_gemv_dual keeps gemv_dual_kernel<4, 8> (two instantiations of the stand-alone kernel's body)"""
    _run(lib, 5, 512)


@pytest.mark.parametrize("d", [384, 1280])
def test_out_cq_kernel_rows_with_a_large_common_offset(lib, d):
    """x0 at 200 +- 2, the attention output at 30 +- 1: the partials' M2 is small beside sum^2 / 16, the sums of arm B are large beside their terms"""
    _run(lib, 5, d, offset=True)


@pytest.mark.parametrize("M,d", [(8, 384), (5, 1280)])
def test_out_cq_kernel_only_the_last_column_tile_is_non_zero(lib, M, d):
    """every tile but the last gives x1 = x0 + bo and q_raw = 0 (bc = 0 there): a workgroup that addressed another tile's weights or columns shows"""
    (a, x0, Wo, bo, Wq, bq, g, be), x1, q, _, _ = _run(lib, M, d, last_tile_only=True)
    assert np.array_equal(x1[:, :d - 16], x0[:, :d - 16] + bo[:d - 16]) and not q[:, :d - 16].view(np.uint32).any()
    assert np.abs(q[:, d - 16:]).max() > 0 and not np.array_equal(x1[:, d - 16:], x0[:, d - 16:] + bo[d - 16:])


def test_out_cq_kernel_vs_fp64(lib):
    """M = 5, d = 1280 against float64 with _out_cq_case's bounds (tests/test_gpu_dec_step_ops.py): x1, and the query finished in float64 with the
    statistics of the reference x1 against LN(x1_ref) Wq^T + bq (times the folded 1/8)"""
    M, d = 5, 1280
    (a, x0, Wo, bo, Wq, bq, g, be), x1, q, qcs, qb = _run(lib, M, d)
    x1_ref = x0.astype(F) + a.astype(F) @ Wo.astype(F).T + bo
    rel = lambda u, v: float(np.linalg.norm(u.astype(F) - v) / (np.linalg.norm(v) + 1e-30))
    e, worst = rel(x1, x1_ref), float(np.abs(x1 - x1_ref).max())
    print(f"out+cq kernel vs fp64 x1: rel err {e:.3e} max abs {worst:.3e}")
    assert e < 1e-3 and worst < 0.05 * (1 + float(np.abs(x1_ref).max())), (e, worst)
    mu = x1_ref.mean(1, keepdims=True); rs = 1.0 / np.sqrt(x1_ref.var(1, keepdims=True) + 1e-5)
    q_ref = (((x1_ref - mu) * rs * g + be) @ Wq.astype(F).T + bq) * 0.125
    q_fin = rs * (q.astype(F) - mu * qcs.astype(F)) + qb.astype(F)
    e, worst = rel(q_fin, q_ref), float(np.abs(q_fin - q_ref).max())
    print(f"out+cq kernel vs fp64 q: rel err {e:.3e} max abs {worst:.3e}")
    assert e < 1e-3 and worst < 0.05 * (1 + float(np.abs(q_ref).max())), (e, worst)
