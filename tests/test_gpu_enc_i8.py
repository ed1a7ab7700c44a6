"""-m gpu: the int8 encoder (models.Whisper(encoder_compute_type="int8")) - its three kernels through their taps, then the whole encoder.

Quantisers: bytes and scales equal wis_hip.weights.quantize_rows of the f16 rows, bit for bit.
GEMM, per written element: |out - ref| <= c 2^-24 (|sa sw acc| + |bias| + |residual|) + r, ref in float64 from the exact integer product.
c counts the f32 roundings of the epilogue as written (csrc/enc_kernels.hip, gemm_i8_kernel and the functors): int32 -> f32, sa[m] * sw[n],
their product, + bias = 4, and + residual = 5; r = 2^-10 |ref| for f16 outputs; behind the GELU the first term is taken on the pre-activation
and multiplied by GELU's Lipschitz constant 1.13 (tests/test_gpu_enc_ops.py).  Everything else in the output buffers keeps its fill pattern.
Whole encoder: rel-L2 against tests/enc_i8_ref.py in float64 <= 4 max(s, e16); s = that reference in float32 against itself in float64,
e16 = the f16 engine against the unquantised reference in float64, both measured in the run (figures: profiles/enc_int8_tests.md)."""
import numpy as np
import pytest

from enc_i8_taps import EPS, _buf, _gemm, _kept, gemm_case, tiny_rig

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("M", [1, 5])
@pytest.mark.parametrize("K,fused", [(384, False), (5120, False), (384, True), (1280, True)])
def test_quantisers(lib, M, K, fused):
    """rows: ties at exact .5 multiples of the scale (absmax 127: scale 1), all zero, absmax in the last column, one f16-max entry, random;
    fused: LayerNorm + quantise on f32 rows (row 0 constant: the output is beta) against wis_op_layernorm's f16 rows"""
    from wis_hip import weights as W
    from wis_hip._lib import DevBuf, check
    rng = np.random.default_rng(K + M)
    q_d, s_d, y_d = DevBuf.from_numpy(_buf((M + 2) * K, np.int8)), DevBuf.from_numpy(_buf(M + 2, np.float32)), DevBuf.from_numpy(_buf((M + 2) * K, np.float16))
    if fused:
        x = (rng.standard_normal((M, K)) * 3 + 1).astype(np.float32)
        x[0] = 0.25
        g, b = (1 + 0.1 * rng.standard_normal(K)).astype(np.float32), (0.1 * rng.standard_normal(K)).astype(np.float32)
        x_d, g_d, b_d, y0_d = DevBuf.from_numpy(x), DevBuf.from_numpy(g), DevBuf.from_numpy(b), DevBuf(M * K * 2)
        check(lib.wis_op_layernorm(0, x_d.ptr, g_d.ptr, b_d.ptr, y0_d.ptr, M, K))
        rows = y0_d.to_numpy(np.float16, (M, K))
        check(lib.wis_op_layernorm_quant(0, x_d.ptr, g_d.ptr, b_d.ptr, q_d.ptr, s_d.ptr, y_d.ptr if M == 5 else None, M, K))
        y = y_d.to_numpy(np.float16, (M + 2, K))
        assert _kept(y[M if M == 5 else 0:]) and (M != 5 or np.array_equal(y[:M].view(np.uint16), rows.view(np.uint16)))
    else:
        rows = (rng.standard_normal((5, K)) * 0.7).astype(np.float16)
        rows[0] = ((np.arange(K) % 127) + 0.5) * np.where(np.arange(K) % 2, -1, 1)
        rows[0, K // 2], rows[1], rows[2, -1], rows[3, 7] = 127, 0, 9.5, 65504
        rows = np.ascontiguousarray(rows[:M])
        x_d = DevBuf.from_numpy(rows)
        check(lib.wis_op_quant_rows(0, x_d.ptr, q_d.ptr, s_d.ptr, M, K))
    q, s = q_d.to_numpy(np.int8, (M + 2, K)), s_d.to_numpy(np.float32, (M + 2,))
    qr, sr = W.quantize_rows(rows)
    assert np.array_equal(q[:M], qr) and np.array_equal(s[:M].view(np.uint32), sr.view(np.uint32))
    assert _kept(q[M:]) and _kept(s[M:])


# (epilogue 0 generic / 1 GELU / 2 residual / 3 QKV / 4 cross K/V, form 1 = 128 x 128 / 2 = 64 x 128 / 3 = 256 x 256 / 0 = the encoder's pick, M or (B, T), N or H,
# K or L): one row more than the form's height (QKV / cross K/V: four, T % 4 == 0) or one row; one and three tiles wide; K of one / two / three k-tiles
@pytest.mark.parametrize("epi,form,m,n,k", [
    (0, 1, 129, 384, 384), (0, 2, 65, 384, 128), (0, 3, 257, 768, 256), (0, 1, 1, 128, 128), (0, 2, 1, 128, 256), (0, 3, 1, 256, 384), (0, 0, 70, 128, 128),
    (1, 1, 129, 128, 256), (1, 2, 65, 384, 384), (1, 3, 257, 256, 128),
    (2, 1, 129, 384, 128), (2, 2, 65, 128, 384), (2, 3, 257, 768, 384), (2, 2, 1, 128, 128),
    (3, 1, (1, 132), 2, 128), (3, 2, (2, 36), 2, 128), (3, 3, (1, 260), 4, 256),
    (4, 1, (1, 132), 2, 3), (4, 2, (2, 36), 2, 1), (4, 3, (1, 260), 4, 2)])
def test_gemm_i8(lib, epi, form, m, n, k):
    gemm_case(lib, epi, form, m, n, k)      # (tests/enc_i8_taps.py: the bound of the docstring above, the fill pattern, two runs equal)


def test_gemm_i8_is_exact_in_the_integer_part(lib):
    """K = 5120, every operand byte +-127, sa = sw = 1, no bias, fp32 output: column n has f(n) sign flips, acc = 127^2 (5120 - 2 f).  |acc| reaches
    8.2e7 > 2^24 (an f32 accumulation would lose bits there): the output is the f32 nearest acc - the bound with its one rounding - and exact below 2^24"""
    M, N, K = 3, 128, 5120
    sgn = np.where(np.arange(K) % 2, -1, 1)
    A = np.outer([1, -1, 1], 127 * sgn).astype(np.int8)
    flips = np.concatenate([[0, K], (np.arange(2, N) * 41) % (K + 1)])
    Wq = np.stack([127 * sgn * np.where(np.arange(K) < f, -1, 1) for f in flips]).astype(np.int8)
    out, _ = _gemm(lib, 0, 0, A, np.ones(M, np.float32), Wq, np.ones(N, np.float32), None, None, 4, (0, 0, 0, 0))
    acc = A.astype(np.int64) @ Wq.astype(np.int64).T
    assert np.abs(acc).max() == 127 * 127 * K > 2 ** 24 and (np.abs(acc) < 2 ** 24).any()
    assert (np.abs(out - acc) <= EPS * np.abs(acc)).all() and np.array_equal(out, acc.astype(np.float32).astype(np.float64))      # (exact below 2^24)


@pytest.fixture(scope="module")
def rig(golden_dir):
    import torch  # noqa: F401  (before libwis_hip.so: one HIP runtime per process)
    from wis_hip import ctranslate2 as ct2
    w, a, mels, refs = tiny_rig(golden_dir)
    mk = lambda **kw: ct2.Whisper("unused", weights=w, arch=a, max_batch=2, max_beam=1, **kw)
    models = {"plain": mk(), "f16": mk(encoder_compute_type="float16"), "int8": mk(encoder_compute_type="int8")}
    yield models, mels, refs
    for m in models.values():
        m.close()


@pytest.mark.parametrize("B", [1, 2])
def test_encoder_int8(rig, B):
    from wis_hip import ctranslate2 as ct2
    models, mels, refs = rig
    rel = lambda a, b: float(np.linalg.norm(a.astype(np.float64) - b) / np.linalg.norm(b))
    x = ct2.StorageView.from_array(mels[:B])
    got, f16 = models["int8"].encode(x, to_cpu=True).array, models["f16"].encode(x, to_cpu=True).array
    assert np.array_equal(f16.view(np.uint32), models["plain"].encode(x, to_cpu=True).array.view(np.uint32)), "the option switched off changed the encoder"
    for i in range(B):
        s, e16 = rel(refs["q32"][i], refs["q64"][i]), rel(f16[i], refs["f64"][i])
        e8, cost = rel(got[i], refs["q64"][i]), rel(got[i], refs["f64"][i])
        print(f"encoder int8 B {B} utterance {i}: s {s:.3e}  e16 {e16:.3e}  int8 engine vs int8 reference {e8:.3e}  int8 engine vs f16 oracle {cost:.3e}")
        assert e8 <= 4 * max(s, e16), (e8, s, e16)
    # run_cross_kv's int8 route, on the handle's own memory and on a caller's block (encode()'s view handed back in): the same decode, compared with ==
    kw = dict(beam_size=1, fixed_new_tokens=4)
    prompts = [[50258, 50259, 50359, 50363]] * B
    a, b = models["int8"].generate(x, prompts, **kw), models["int8"].generate(models["int8"].encode(x), prompts, **kw)
    assert [r.sequences_ids for r in a] == [r.sequences_ids for r in b] and [r.scores for r in a] == [r.scores for r in b]
