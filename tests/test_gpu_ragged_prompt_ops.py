"""-m gpu: no_speech_rows_kernel (wis_op_no_speech_rows) - the no_speech_prob reader of a batch whose prompts differ in length: one logits row per
utterance, named by a device word (a value outside [0, rs): the utterance is not in this pass, its output stays as it is) - against a float64 softmax.

The bar, per output, is the one tests/test_gpu_sample_ops.py sets for no_speech_kernel, whose arithmetic and reduction order this kernel shares: 4 x
the error of a numpy fp32 restatement of the kernel's reduction (256 strided partial sums, a tree over them, an accurate fp32 exponential) against
float64 on the same row, with a floor of 4 fp32 ulps.  The restatement never sees the kernel's output."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ULP = 2.0 ** -23
WIS_E_ARG = -1
GUARD = 4                      # untouched words in front of and behind the B outputs


def _biteq(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))


def _softmax64(row):
    x = row.astype(np.float64)
    e = np.exp(x - x.max())
    return e / e.sum()


def _tree(a):
    """sum of the last axis (a power of two) by halving, in the array's precision"""
    while a.shape[-1] > 1:
        h = a.shape[-1] // 2
        a = a[..., :h] + a[..., h:]
    return a[..., 0]


def _no_speech_f32(row, ns):
    """tests/test_gpu_sample_ops.py's restatement of no_speech_kernel (this kernel's arithmetic) in numpy fp32: thread t sums exp(row[i] - max) over
    i = t, t + 256, ..; four wave sums; (w0 + w1) + (w2 + w3)"""
    V = row.shape[0]
    mx = row.max()
    pad = np.full((-V) % 256, -np.inf, np.float32)
    e = np.exp(np.concatenate([row, pad]).reshape(-1, 256) - mx).astype(np.float32)
    part = np.add.reduce(e, axis=0, dtype=np.float32)
    w = _tree(part.reshape(4, 64))
    s = np.float32(np.float32(w[0] + w[1]) + np.float32(w[2] + w[3]))
    return np.float32(np.exp(np.float32(row[ns] - mx))) / s


def _tables(B, rs):
    """row tables: every utterance in the pass (first and last row among them), some skipped (-1), all skipped but one"""
    rng = np.random.default_rng([B, rs])
    t = [np.asarray([(0, rs - 1, rs // 2)[b % 3] for b in range(B)], np.int32)]
    mixed = rng.integers(0, rs, B).astype(np.int32)
    mixed[::2] = -1
    if B == 1:
        mixed[0] = rs - 1
    t.append(mixed)
    lone = np.full(B, -1, np.int32)
    lone[B - 1] = 0
    t.append(lone)
    return t


@pytest.mark.parametrize("B,rs", [(1, 16), (3, 16), (8, 12)])
@pytest.mark.parametrize("V", [51865, 51866])
def test_no_speech_rows_against_float64(lib, V, B, rs):
    from wis_hip._lib import DevBuf, check
    ld = (V + 31) // 32 * 32
    rng = np.random.default_rng([V, B, rs])
    worst = (0.0, 0.0, 0.0)
    for case, rows in enumerate(_tables(B, rs)):
        ns = (0, V // 2 + 7, V - 1)[case]
        buf = (3.0 * rng.standard_normal((B * rs, ld)) + 4.0).astype(np.float32)
        buf[:, V:] = np.float32(1e4)                     # the padding columns would swamp the sum
        live = [b for b in range(B) if rows[b] >= 0]
        # one read row holds a value near the f32 maximum IN FRONT OF its maximum (a running sum that is not rescaled by the true maximum overflows)
        big = live[0] * rs + rows[live[0]]
        buf[big, 5] = np.float32(3.0e38)
        buf[big, V - 3] = np.float32(3.2e38)
        buf[big, ns] = np.float32(3.2e38)                # (<|nospeech|> ties with the maximum: a probability near 1 / 2, not 0)
        before = rng.standard_normal(B + 2 * GUARD).astype(np.float32)
        d_l, d_r, d_o = DevBuf.from_numpy(buf), DevBuf.from_numpy(rows), DevBuf.from_numpy(before)
        check(lib.wis_op_no_speech_rows(0, d_l.ptr, ld, B, rs, d_r.ptr, V, ns, d_o.ptr.value + 4 * GUARD))
        got = d_o.to_numpy(np.float32, (B + 2 * GUARD,))
        assert _biteq(got[:GUARD], before[:GUARD]) and _biteq(got[GUARD + B:], before[GUARD + B:])
        for b in range(B):
            if rows[b] < 0:
                assert _biteq(got[GUARD + b:GUARD + b + 1], before[GUARD + b:GUARD + b + 1]), (b, rows)
                continue
            x = buf[b * rs + rows[b], :V]
            p64 = _softmax64(x)[ns]
            g = float(got[GUARD + b])
            assert np.isfinite(g) and g >= 0.0
            if p64 < 1e-30:                              # (behind a 3e38 logit every other id underflows: exactly 0 in both)
                assert g <= 1e-30, (b, g, p64)
                continue
            ref_err = abs(float(_no_speech_f32(x, ns)) - p64) / p64
            bar = max(4 * ref_err, 4 * ULP)
            err = abs(g - p64) / p64
            print(f"  V {V} B {B} rs {rs} table {case} utterance {b} row {rows[b]}: p {p64:.6e} restatement error {ref_err:.3e} bar {bar:.3e} kernel error {err:.3e}")
            if err / bar >= worst[2] / max(worst[1], 1e-300):
                worst = (ref_err, bar, err)
            assert err <= bar, (b, rows[b], ns, g, p64, ref_err, err, bar)
    print(f"no_speech_rows V {V} B {B} rs {rs}: nearest its bar: restatement error {worst[0]:.3e}, bar {worst[1]:.3e}, kernel error {worst[2]:.3e}")


def test_no_speech_rows_skips_rows_outside_the_pass_and_refuses_bad_arguments(lib):
    from wis_hip._lib import DevBuf, check
    V, ld, B, rs = 51865, 51872, 3, 4
    buf = np.random.default_rng(5).standard_normal((B * rs, ld)).astype(np.float32)
    before = np.asarray([7.0, 8.0, 9.0], np.float32)
    d_l, d_o = DevBuf.from_numpy(buf), DevBuf.from_numpy(before)
    d_r = DevBuf.from_numpy(np.asarray([-1, rs, 1 << 20], np.int32))        # -1, one past the last row, far outside: nothing is read or written
    check(lib.wis_op_no_speech_rows(0, d_l.ptr, ld, B, rs, d_r.ptr, V, 11, d_o.ptr))
    assert _biteq(d_o.to_numpy(np.float32, (B,)), before)
    for ns in (-1, V, V + 3):
        assert lib.wis_op_no_speech_rows(0, d_l.ptr, ld, B, rs, d_r.ptr, V, ns, d_o.ptr) == WIS_E_ARG
    assert lib.wis_op_no_speech_rows(0, d_l.ptr, ld, B, rs, None, V, 11, d_o.ptr) == WIS_E_ARG
    assert lib.wis_op_no_speech_rows(0, d_l.ptr, V - 1, B, rs, d_r.ptr, V, 11, d_o.ptr) == WIS_E_ARG
