"""gpu: the whole-recording log-mel (wis_longmel_*, csrc/logmel.hip: longmel_stft_kernel, longmel_window_kernel) at both bin counts.

  equal        window(seek = 0) equals wis_logmel_n of the same samples bit for bit up to 479000 samples (from 479801 on frame 3000 touches a sample and
               enters the maximum here, above 479958 the 30 s front end's right-hand reflection reads real samples: the two differ by design)
  independent  every absolute frame of a 65 s recording has the same bits whichever window reads it (seeks on a tile, off a tile, beyond one window),
               whether the upload ran in the built-in segments or in segments of 4096 samples, and whether the seeks went in one call or one by one
  float64      every entry of the windows at seeks 0, 3000 and content - 100 of the 65 s recording of tests/longmel_ref.py lies inside the reference's
               interval; the recording's maximum lies inside its interval and equals it where that is a point; the floor is the recording's, not the
               window's (tests/test_longmel_ref_cpu.py shows that the reference separates the two)
  edges        frames beyond the stored range, the first and the last seek served, argument errors that leave the handle usable, guard words

The output buffers are pre-filled with a bit pattern nothing produces.  Timing is not in scope."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import logmel_ref as R  # noqa: E402
import longmel_ref as L  # noqa: E402

pytestmark = pytest.mark.gpu
WIS_E_ARG = -1
PAT32 = 0x5A5A5A5A                     # f32 1.5e16: nothing these kernels produce
F32, NF = np.float32, R.N_FRAMES
BINS = (80, 128)
SEEKS = (0, 1, 15, 16, 17, 2999, 3000, 3500)


def silent_out(gmax):
    """the entry of a frame that touches no sample, in f32 as the kernel computes it"""
    return (np.maximum(F32(-10.0), F32(gmax) - F32(8.0)) + F32(4.0)) / F32(4.0)


@pytest.fixture(scope="module")
def lib():
    from wis_hip import _lib
    _lib.require_gpu()
    return _lib.load()


@pytest.fixture(scope="module")
def rec():
    return L.recording_65s()


@pytest.fixture(scope="module")
def rec_sp(rec):
    """the float64 sums of the recording's active frames, shared by both banks"""
    return L.active_spectrum(rec)


@pytest.fixture(scope="module")
def rec_windows(rec):
    """bits of the windows at SEEKS of the 65 s recording, per bin count, with the recording's maximum: computed once, never changed"""
    from wis_hip import audio
    out = {}
    for nm in BINS:
        with audio.LongMel(rec, nm, 0) as lm:
            assert lm.frames == L.content_frames(rec.shape[0]) == 6500
            w = lm.window(list(SEEKS), to_host=True)
            out[nm] = (w.view(np.uint32).copy(), lm.max)
    return out


def windows_raw(lib, h, seeks, n_mels, guard=64, device=False):
    """wis_longmel_window on a pattern-filled buffer with guard words behind it -> (rc, u32 [n][n_mels][3000])"""
    from wis_hip import _lib
    n = len(seeks)
    words = n * n_mels * NF
    arr = (C.c_int64 * max(n, 1))(*seeks)
    if device:
        d = _lib.DevBuf.from_numpy(np.full(words + guard, PAT32, np.uint32))
        rc = lib.wis_longmel_window(h, arr, n, d.ptr, 1)
        buf = d.to_numpy(np.uint32, (words + guard,))
        d.free()
    else:
        buf = np.full(words + guard, PAT32, np.uint32)
        rc = lib.wis_longmel_window(h, arr, n, _lib.ptr(buf), 0)
    assert np.all(buf[words:] == PAT32), "wrote behind mel_out"
    if rc != 0:
        assert np.all(buf == PAT32), "an argument error wrote to mel_out"
    return rc, buf[:words].reshape(n, n_mels, NF)


@pytest.mark.parametrize("n_mels", BINS)
def test_seek_0_equals_the_30s_front_end(lib, n_mels):
    from wis_hip import _lib, audio
    x = R.signals(n=479000, seed=11)["gauss_0.1"]
    for n in (0, 1, 159, 160, 161, 200, 2559, 2560, 2561, 40001, 479000):
        ref = np.full((1, n_mels, NF), PAT32, np.uint32)
        src = np.ascontiguousarray(x[:max(n, 1)])
        _lib.check(lib.wis_logmel_n(0, n_mels, _lib.ptr(src), 0, (C.c_int64 * 1)(n), 1, 0, _lib.ptr(ref), 0))
        with audio.LongMel(x[:n], n_mels, 0) as lm:
            assert lm.frames == n // 160
            rc, got = windows_raw(lib, lm._h, [0], n_mels)
            assert rc == 0, lib.wis_last_error()
            rc, got_d = windows_raw(lib, lm._h, [0], n_mels, device=True)
            assert rc == 0, lib.wis_last_error()
        assert not np.any(got == PAT32)
        assert np.array_equal(got, ref), f"n_samples {n}: {int((got != ref).sum())} entries differ from wis_logmel_n"
        assert np.array_equal(got_d, ref), f"n_samples {n}: the device window differs"


@pytest.mark.parametrize("n_mels", BINS)
def test_a_frame_has_the_same_bits_in_every_window(lib, rec, rec_windows, n_mels):
    from wis_hip import audio
    w, gmax = rec_windows[n_mels]
    assert not np.any(w == PAT32)
    total = max(SEEKS) + NF
    canon = np.zeros((n_mels, total), np.uint32)
    seen = np.zeros(total, bool)
    for i, s in enumerate(SEEKS):
        old = seen[s:s + NF]
        assert np.array_equal(w[i][:, old], canon[:, s:s + NF][:, old]), f"the window at seek {s} differs from an earlier one on a shared frame"
        canon[:, s:s + NF] = w[i]
        seen[s:s + NF] = True
    assert seen.all()
    # the same recording uploaded in segments of 4096 samples (one tile per launch): the same bits, the same maximum
    with audio.LongMel(rec, n_mels, 0, segment_samples=4096) as lm:
        w2 = lm.window(list(SEEKS), to_host=True).view(np.uint32)
        assert np.array_equal(w2, w), "the upload segment changes the bits"
        assert F32(lm.max).view(np.uint32) == F32(gmax).view(np.uint32)
        # ... and one seek per call equals the seeks of one call
        for i, s in enumerate(SEEKS):
            rc, one = windows_raw(lib, lm._h, [s], n_mels)
            assert rc == 0 and np.array_equal(one[0], w[i]), f"seek {s} alone differs from the same seek in a call of {len(SEEKS)}"


@pytest.mark.parametrize("n_mels", BINS)
def test_windows_against_float64(lib, rec, rec_sp, rec_windows, n_mels):
    ls = L.log_spectrum(rec, n_mels, sp=rec_sp)
    glo, ghi = L.gmax_interval(ls)
    w, gmax = rec_windows[n_mels]
    print(f"n_mels {n_mels}: maximum {gmax!r} in [{glo!r}, {ghi!r}]")
    assert glo <= gmax <= ghi
    content = L.content_frames(rec.shape[0])
    from wis_hip import audio
    with audio.LongMel(rec, n_mels, 0) as lm:
        last = lm.window(content - 100, to_host=True)
    for seek, got in ((0, w[SEEKS.index(0)].view(F32)), (3000, w[SEEKS.index(3000)].view(F32)), (content - 100, last)):
        iv = L.window(ls, seek)
        bad = R.outside(got, iv)
        r = R.ratio(got, iv)
        print(f"n_mels {n_mels} seek {seek}: worst |got - centre| / half-width {float(r.max()):.3f}, {int(bad.sum())} of {bad.size} outside")
        assert not bad.any(), f"seek {seek}: {int(bad.sum())} entries outside the reference's interval, first at {np.argwhere(bad)[0].tolist()}"
    # the floor is the recording's: the window at 30 s .. 60 s, whose own maximum is more than 8 below it, is clamped there throughout - and is
    # outside the interval a window-maximum floor would give on nearly every entry
    got = w[SEEKS.index(3000)].view(F32)
    assert np.all(got == (F32(gmax) - F32(8.0) + F32(4.0)) / F32(4.0))
    own = L.window_own_max(ls, 3000)
    assert R.outside(got, own).mean() > 0.99


@pytest.mark.parametrize("n_mels", BINS)
def test_maximum_where_the_reference_is_a_point(lib, n_mels):
    from wis_hip import audio
    rng = np.random.default_rng(3)
    # no frame holds a non-zero sample: the reference's interval of the maximum is the point -10, and the key must be that of -10.0f
    for x in (np.zeros(5000, F32), np.zeros(0, F32)):
        ls = L.log_spectrum(x, n_mels)
        assert L.gmax_interval(ls) == (-10.0, -10.0)
        with audio.LongMel(x, n_mels, 0) as lm:
            assert F32(lm.max).view(np.uint32) == 0xC1200000
            got = lm.window(0, to_host=True)
        assert np.all(got.view(np.uint32) == F32(-1.5).view(np.uint32))
    # noise whose every mel energy is below the clamp: active frames, so the interval has the width of the log10 rounding allowance - inside it
    x = (1e-9 * rng.standard_normal(5000)).astype(F32)
    ls = L.log_spectrum(x, n_mels)
    glo, ghi = L.gmax_interval(ls)
    assert glo == -10.0 and ghi < -10.0 + 1e-5
    with audio.LongMel(x, n_mels, 0) as lm:
        print(f"n_mels {n_mels}: clamped noise, maximum {lm.max!r} in [{glo!r}, {ghi!r}]")
        assert glo <= lm.max <= ghi
        assert not R.outside(lm.window(0, to_host=True), L.window(ls, 0)).any()


@pytest.mark.parametrize("n_mels", BINS)
def test_edges(lib, n_mels):
    from wis_hip import _lib, audio
    n = 40001
    x = R.signals(n=n, seed=7)["gauss_0.1"]
    content, stored = L.content_frames(n), L.stored_frames(n)
    ls = L.log_spectrum(x, n_mels)
    with audio.LongMel(x, n_mels, 0) as lm:
        h = lm._h
        assert lm.frames == content == 250
        gmax = F32(lm.max)
        fill = silent_out(gmax).view(np.uint32)
        rc, base = windows_raw(lib, h, [0], n_mels)
        assert rc == 0
        # frames beyond the stored range are exactly -10 clamped and scaled; so are the silent frames of the last stored tile
        assert np.all(base[0][:, L.touched_frames(n):] == fill) and stored < NF
        # the first and the last seek of the recording's frame range are served
        rc, w = windows_raw(lib, h, [content - 1, content + NF - 1], n_mels)
        assert rc == 0, lib.wis_last_error()
        assert np.array_equal(w[0][:, :NF - (content - 1)], base[0][:, content - 1:]) and np.all(w[0][:, NF - (content - 1):] == fill)
        assert np.all(w[1] == fill)
        assert not R.outside(w[0].view(F32), L.window(ls, content - 1)).any()
        # argument errors: nothing is written, nothing stays in flight, the handle goes on working
        for seeks in ([-1], [content + NF], [0, -5], [0, 2 ** 40]):
            rc, _ = windows_raw(lib, h, seeks, n_mels)
            assert rc == WIS_E_ARG, seeks
        buf = np.full(n_mels * NF, PAT32, np.uint32)
        one = (C.c_int64 * 1)(0)
        assert lib.wis_longmel_window(None, one, 1, _lib.ptr(buf), 0) == WIS_E_ARG
        assert lib.wis_longmel_window(h, None, 1, _lib.ptr(buf), 0) == WIS_E_ARG
        assert lib.wis_longmel_window(h, one, 1, None, 0) == WIS_E_ARG
        assert lib.wis_longmel_window(h, one, -1, _lib.ptr(buf), 0) == WIS_E_ARG
        assert np.all(buf == PAT32)
        assert lib.wis_longmel_frames(None) == 0
        rc, again = windows_raw(lib, h, [0], n_mels)
        assert rc == 0 and np.array_equal(again, base)
        rc, none = windows_raw(lib, h, [], n_mels)
        assert rc == 0
    hh = C.c_void_p(0x1234)
    small = np.zeros(16, F32)
    assert lib.wis_longmel_create(0, 64, _lib.ptr(small), 16, 0, C.byref(hh)) == WIS_E_ARG and not hh.value
    hh = C.c_void_p(0x1234)
    assert lib.wis_longmel_create(0, n_mels, _lib.ptr(small), audio.LONGMEL_MAX_SAMPLES + 1, 0, C.byref(hh)) == WIS_E_ARG and not hh.value
    assert b"cap" in lib.wis_last_error()
    hh = C.c_void_p(0x1234)
    assert lib.wis_longmel_create(0, n_mels, None, 16, 0, C.byref(hh)) == WIS_E_ARG and not hh.value
    assert lib.wis_longmel_create(0, n_mels, _lib.ptr(small), -1, 0, C.byref(hh)) == WIS_E_ARG
    assert lib.wis_longmel_create_ex(0, n_mels, _lib.ptr(small), 16, 0, 2799, C.byref(hh)) == WIS_E_ARG
    assert lib.wis_longmel_create(0, n_mels, _lib.ptr(small), 16, 0, None) == WIS_E_ARG
    lib.wis_longmel_destroy(None)
    with pytest.raises(ValueError):
        audio.LongMel(small, 64, 0)
    lm = audio.LongMel(small, n_mels, 0)
    lm.close()
    lm.close()
    with pytest.raises(ValueError):
        lm.window(0)


def test_device_pcm_and_the_smallest_segment(lib):
    """PCM that already lives on the device gives the bits of the host upload; so does the smallest segment (2800 samples: one tile's span)"""
    from wis_hip import _lib, audio
    x = R.signals(n=40001, seed=9)["gauss_exponents"]
    with audio.LongMel(x, 80, 0) as lm:
        want = lm.window([0, 100], to_host=True).view(np.uint32)
    with audio.LongMel(x, 80, 0, segment_samples=2800) as lm:
        assert np.array_equal(lm.window([0, 100], to_host=True).view(np.uint32), want)
    d = _lib.DevBuf.from_numpy(x)
    h = C.c_void_p()
    _lib.check(lib.wis_longmel_create(0, 80, d.ptr, x.shape[0], 1, C.byref(h)))
    try:
        rc, got = windows_raw(lib, h, [0, 100], 80)
        assert rc == 0 and np.array_equal(got, want)
    finally:
        lib.wis_longmel_destroy(h)
        d.free()
