"""gpu: the resampler (csrc/resample.hip: wis_resample, wis_resample_ex, wis_op_resample_segment) element by element against the
fp64 direct form of tests/resample_ref.py under its derived bound  |y_gpu[m] - y64[m]| <= (T + 3) 2^-24 B[m]  - ratios and
lengths that straddle workgroup boundaries and are shorter than the filter's reach, signals that read the edge taps, the DC gain
of every phase and a wide exponent spread - plus the entry points' memory safety, segment independence, 64-bit positions, one
full-size clip and concurrent callers."""
import ctypes as C
import os
import sys
import threading

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from resample_ref import bound, ratio, resample_ref  # noqa: E402

pytestmark = pytest.mark.gpu
WIS_E_ARG, WIS_E_UNSUPPORTED = -1, -7
GUARD = 16
SENTINEL = np.uint32(0x7FC0DEAD)      # a quiet NaN no resampler produces

CASES = [(48000, n) for n in (1, 2, 50, 3 * 255 + 1, 3 * 256, 3 * 256 + 2, 3 * 513 + 1)] + \
        [(44100, 441 * 3 + 1), (22050, 2 * 441 + 7), (8000, 129), (11025, 1000), (96000, 6 * 300 + 5)]


def signals(n, seed):
    rng = np.random.default_rng(seed)
    first, last = np.zeros(n), np.zeros(n)
    first[0], last[n - 1] = 1.0, 1.0
    out = {"gauss": rng.standard_normal(n) * 0.1, "impulse_first": first, "impulse_last": last, "ones": np.ones(n),
           "alternating": np.where(np.arange(n) % 2 == 0, 1.0, -1.0), "exponents": rng.standard_normal(n) * 2.0 ** (-20.0 * rng.random(n))}
    return {k: v.astype(np.float32) for k, v in out.items()}


def n_out_of(sr, n_in):
    up, down = ratio(sr)
    return -(-n_in * up // down)


def run(lib, x, sr, segment=None, cap=None):
    """-> (rc, n_out the call reported, the whole host buffer as uint32: n_out results then GUARD sentinels)"""
    x = np.ascontiguousarray(x, np.float32)
    n_out = n_out_of(sr, x.shape[0])
    buf = np.full(n_out + GUARD, SENTINEL, np.uint32)
    n = C.c_int64(-1)
    cap = n_out if cap is None else cap
    if segment is None:
        rc = lib.wis_resample(0, x.ctypes.data_as(C.c_void_p), x.shape[0], sr, buf.ctypes.data_as(C.c_void_p), cap, C.byref(n))
    else:
        rc = lib.wis_resample_ex(0, x.ctypes.data_as(C.c_void_p), x.shape[0], sr, buf.ctypes.data_as(C.c_void_p), cap, C.byref(n), segment)
    return rc, n.value, buf


def resampled(lib, x, sr, segment=None):
    rc, n, buf = run(lib, x, sr, segment)
    assert rc == 0, lib.wis_last_error()
    assert n == buf.shape[0] - GUARD
    assert np.all(buf[n:] == SENTINEL), "wrote behind out[n_out]"
    return buf[:n].view(np.float32).copy()


def check(y, x, sr, what):
    y64, B, T = resample_ref(x, sr)
    assert y.shape == y64.shape
    assert np.all(np.isfinite(y)), what
    err, lim = np.abs(y.astype(np.float64) - y64), bound(B, T)
    worst = float((err / np.maximum(lim, 1e-300)).max()) if y.shape[0] else 0.0
    print(f"{what}: n_out {y.shape[0]}, T {T}, worst error {worst:.3f} of the bound")
    bad = np.nonzero(err > lim)[0]
    assert bad.size == 0, (what, bad[:8], err[bad[:8]], lim[bad[:8]])


@pytest.mark.parametrize("sr,n_in", CASES)
def test_matches_fp64_direct_form(lib, sr, n_in):
    for name, x in signals(n_in, sr + n_in).items():
        check(resampled(lib, x, sr), x, sr, f"{sr} Hz n_in {n_in} {name}")


def test_ratio_whose_span_does_not_fit_lds(lib):
    """256 kHz (1 / 16, 1025 taps per output): 256 outputs span 5123 samples, more than the kernel stages, so it reads HBM - the same sum"""
    sr, n_in = 256000, 16 * 300 + 5
    sig = signals(n_in, 256)
    for name in ("gauss", "impulse_first", "impulse_last", "ones", "exponents"):
        check(resampled(lib, sig[name], sr), sig[name], sr, f"{sr} Hz n_in {n_in} {name}")
    assert np.array_equal(resampled(lib, sig["gauss"], sr, segment=1000).view(np.uint32), resampled(lib, sig["gauss"], sr).view(np.uint32))


@pytest.mark.parametrize("sr,n_in", [(48000, 1), (48000, 3 * 256 + 2), (44100, 441 * 3 + 1), (8000, 129)])
def test_short_buffer_is_refused_untouched(lib, sr, n_in):
    x = signals(n_in, 3)["gauss"]
    rc, n, buf = run(lib, x, sr, cap=n_out_of(sr, n_in) - 1)
    assert rc == WIS_E_ARG and n == n_out_of(sr, n_in)
    assert np.all(buf == SENTINEL)
    rc, n, buf = run(lib, x, sr, segment=1000, cap=n_out_of(sr, n_in) - 1)
    assert rc == WIS_E_ARG and np.all(buf == SENTINEL)


def test_edges_of_the_interface(lib):
    n = C.c_int64(-1)
    x = signals(64, 5)["gauss"]
    out = np.zeros(64, np.float32)
    p, q = x.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p)
    assert lib.wis_resample(0, p, 0, 48000, q, 64, C.byref(n)) == 0 and n.value == 0
    assert lib.wis_resample(0, p, 64, 16000, q, 64, C.byref(n)) == 0 and n.value == 64 and np.array_equal(out, x)
    assert lib.wis_resample(0, p, 64, 47999, q, 64, C.byref(n)) == WIS_E_UNSUPPORTED
    assert lib.wis_resample(0, p, 64, 0, q, 64, C.byref(n)) == WIS_E_ARG
    assert lib.wis_resample(0, p, -1, 48000, q, 64, C.byref(n)) == WIS_E_ARG
    assert lib.wis_resample_ex(0, p, 64, 48000, q, 64, C.byref(n), -5) == WIS_E_ARG


@pytest.mark.parametrize("sr", [44100, 48000])
def test_segments_do_not_change_a_bit(lib, sr):
    x = signals(20000, sr)["gauss"]
    whole = resampled(lib, x, sr)
    check(whole, x, sr, f"{sr} Hz n_in 20000")
    for seg in (1000, 4097):
        assert np.array_equal(resampled(lib, x, sr, segment=seg).view(np.uint32), whole.view(np.uint32)), seg


@pytest.mark.parametrize("sr", [48000, 44100, 96000])
def test_positions_past_2_to_the_40(lib, sr):
    """the same 4000 samples as a slice at k_base = down J of a very long signal, outputs from m0 = up J on (m0 down > 2^40), and at
    k_base = 0: the taps are identical, so the outputs are, bit for bit.  n_in_total keeps both edges of the signal out of both slices."""
    from wis_hip import _lib
    up, down = ratio(sr)
    n_slice = 4000
    x = signals(n_slice, 17)["gauss"]
    L = 64 * max(up, down) + 1
    half, tpp = (L - 1) // 2, -(-L // up)
    ms = np.arange(-(-n_slice * up // down), dtype=np.int64)
    k_hi = (ms * down + half) // up
    inside = ms[(k_hi - (tpp - 1) >= 0) & (k_hi <= n_slice - 1)]       # outputs whose whole reach lies in the slice
    ma, count = int(inside[0]), int(inside.shape[0])
    assert count > 256 and np.array_equal(inside, np.arange(ma, ma + count))
    J = (2 ** 40) // (up * down) + 12345
    assert (up * J + ma) * down > 2 ** 40
    dx = _lib.DevBuf.from_numpy(x)
    got = []
    for k_base, m0 in ((0, ma), (down * J, up * J + ma)):
        dy = _lib.DevBuf.from_numpy(np.full(count + GUARD, SENTINEL, np.uint32))
        rc = lib.wis_op_resample_segment(0, dx.ptr, n_slice, k_base, k_base + 10 ** 6, m0, count, up, down, dy.ptr)
        assert rc == 0, lib.wis_last_error()
        buf = dy.to_numpy(np.uint32, (count + GUARD,))
        assert np.all(buf[count:] == SENTINEL)
        got.append(buf[:count])
        dy.free()
    assert np.array_equal(got[0], got[1])
    # ... and they are the outputs of the slice taken as a signal of its own, where its edges are out of reach
    y64, B, T = resample_ref(x, sr)
    assert np.all(np.abs(got[0].view(np.float32).astype(np.float64) - y64[ma:ma + count]) <= bound(B, T)[ma:ma + count])
    # a slice that does not hold the outputs' support is refused, nothing is launched
    dy = _lib.DevBuf.from_numpy(np.full(count + GUARD, SENTINEL, np.uint32))
    assert lib.wis_op_resample_segment(0, dx.ptr, n_slice, down * J, down * J + 10 ** 6, up * J + ma + count, 8, up, down, dy.ptr) == WIS_E_ARG
    assert lib.wis_op_resample_segment(0, dx.ptr, n_slice, down * J, down * J + 10 ** 6, up * J, 8, up, down, dy.ptr) == WIS_E_ARG
    assert np.all(dy.to_numpy(np.uint32, (count + GUARD,)) == SENTINEL)
    dy.free()
    dx.free()


@pytest.fixture(scope="module")
def full_size():
    x = (np.random.default_rng(292).standard_normal(int(29.2 * 48000)) * 0.1).astype(np.float32)
    return x, resample_ref(x, 48000)


def test_full_size_clip(lib, full_size):
    x, (y64, B, T) = full_size
    y = resampled(lib, x, 48000)
    assert y.shape[0] == int(29.2 * 16000)
    err, lim = np.abs(y.astype(np.float64) - y64), bound(B, T)
    print(f"29.2 s at 48 kHz: worst error {float((err / lim).max()):.3f} of the bound (T = {T})")
    assert np.all(err <= lim)
    assert np.array_equal(resampled(lib, x, 48000).view(np.uint32), y.view(np.uint32))


def test_concurrent_callers(lib):
    rates = (48000, 44100, 8000, 22050)
    xs = {sr: signals(6000 + 7 * i, sr)["gauss"] for i, sr in enumerate(rates)}
    alone = {sr: resampled(lib, xs[sr], sr) for sr in rates}
    wrong, start = [], threading.Barrier(len(rates))

    def caller(sr):
        start.wait()
        for it in range(20):
            try:
                if not np.array_equal(resampled(lib, xs[sr], sr).view(np.uint32), alone[sr].view(np.uint32)):
                    wrong.append((sr, it, "bits"))
            except Exception as e:  # noqa: BLE001
                wrong.append((sr, it, repr(e)))
                return

    th = [threading.Thread(target=caller, args=(sr,)) for sr in rates]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert not wrong, wrong[:4]


def test_python_entry(lib):
    from wis_hip import audio
    x = signals(5000, 9)["gauss"]
    y = audio.resample(x, 44100, device=0)
    assert y.dtype == np.float32 and np.array_equal(y, resampled(lib, x, 44100))
    assert np.array_equal(audio.resample_gpu(x, 44100, 0, segment_samples=777), y)
    # a ratio the device does not serve falls back to the host resampler
    assert np.array_equal(audio.resample(x[:200], 47999, device=0), audio.resample(x[:200], 47999))
