"""not gpu: the float64 yardstick of the whole-recording log-mel tests (tests/longmel_ref.py) proves itself before a kernel is held against it.

  pinned     on a recording of 300000 samples the window at seek 0 equals logmel_ref.logmel_full of that recording's pad_or_trim window to float64
             rounding - because no sample the 30 s window reflects at its right edge and no frame behind frame 2999 is non-zero, which is checked
  counted    content, total, touched and stored frames at the lengths the GPU tests use
  left edge  frame 0 reflects samples 1 .. 200, nothing is reflected on the right, and a frame far inside equals the plain slice
  separates  on the 65 s recording of the GPU tests the window at seek 3000 has a maximum of its own more than 8 below the recording's, and the
             intervals under the two floors are disjoint on nearly every entry: a kernel that clamps against the window's maximum cannot pass
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import logmel_ref as R  # noqa: E402
import longmel_ref as L  # noqa: E402


def test_window_at_seek_0_is_the_30s_front_end():
    n = 300000
    x = R.signals(n=n, seed=5)["gauss_0.1"]
    win = R.window_of(x)
    # what makes the two definitions agree here: the 30 s window reflects the samples 479800 .. 479998 at its right edge, all zero, and every frame
    # of the recording from 3000 on is silent
    assert not np.any(win[R.N_SAMPLES - R.N_FFT // 2 - 1:]) and n < R.N_SAMPLES - R.N_FFT // 2 - 1
    assert L.touched_frames(n) <= R.N_FRAMES and not np.any(L.active_frames(x)[R.N_FRAMES:])
    assert np.array_equal(L.active_frames(x), R.active_frames(win)[:L.touched_frames(n)]) and not np.any(R.active_frames(win)[L.touched_frames(n):])
    for n_mels in (80, 128):
        ls = L.log_spectrum(x, n_mels)
        w = L.window(ls, 0)
        full = R.logmel_full(win, n_mels)
        assert w["centre"].shape == full.shape == (n_mels, R.N_FRAMES)
        assert np.max(np.abs(w["centre"] - full)) < 1e-12
        assert np.all(w["lo"] < w["centre"]) and np.all(w["centre"] < w["hi"])


@pytest.mark.parametrize("n,content,touched,stored", [(0, 0, 0, 0), (1, 0, 2, 16), (159, 0, 3, 16), (160, 1, 3, 16), (161, 1, 3, 16), (200, 1, 3, 16),
                                                      (2559, 15, 18, 32), (2560, 16, 18, 32), (2561, 16, 18, 32), (40001, 250, 252, 256),
                                                      (479000, 2993, 2995, 3008), (1040000, 6500, 6502, 6512)])
def test_frame_counts(n, content, touched, stored):
    assert L.content_frames(n) == content and L.total_frames(n) == content + 3000
    assert L.touched_frames(n) == touched and L.stored_frames(n) == stored
    # by hand: frame t touches a sample exactly when there is one and its first sample 160 t - 200 is at most n - 1
    assert touched == sum(1 for t in range(content + 3000) if n > 0 and 160 * t - 200 <= n - 1)
    assert stored % 16 == 0 and touched <= stored < touched + 16


def test_left_reflection_only():
    x = np.arange(1, 1001, dtype=np.float32)
    fr = L.frames_of(x, [0, 2, 6, 7, 9])
    assert np.array_equal(fr[0, :200], x[1:201][::-1]) and np.array_equal(fr[0, 200:], x[:200])
    assert np.array_equal(fr[1], x[120:520])
    assert np.array_equal(fr[2, :240], x[760:1000]) and not np.any(fr[2, 240:])      # zeros behind the last sample, no reflection
    assert np.array_equal(fr[3, :80], x[920:]) and not np.any(fr[3, 80:])
    assert not np.any(fr[4])
    assert L.active_frames(x).tolist() == [True] * L.touched_frames(1000) and L.touched_frames(1000) == 8
    # a recording shorter than the reflection: the reflected positions behind its end are zeros
    assert np.array_equal(L.frames_of(np.ones(1, np.float32), [0, 1]), np.array([[0.0] * 200 + [1.0] + [0.0] * 199, [0.0] * 40 + [1.0] + [0.0] * 359]))


def test_the_two_floors_separate():
    x = L.recording_65s()
    assert x.shape == (L.N_65S,) and not np.any(x[400000:560000])
    ls = L.log_spectrum(x, 80)
    glo, ghi = L.gmax_interval(ls)
    own_hi = float(L.gather(ls["hi"], 3000).max())
    assert ghi - glo < 1e-4                        # the maximum sits on a broadband frame: its interval is narrow
    assert own_hi < glo - 8.0                      # the window at 30 s .. 60 s: its own maximum more than 8 below the recording's
    a, b = L.window(ls, 3000), L.window_own_max(ls, 3000)
    assert np.all(a["lo"] > -1e9) and np.all(a["hi"] - a["lo"] < 1e-4 + 2 * L.ROUND)      # every entry is at the recording's floor
    disjoint = (a["lo"] > b["hi"]) | (a["hi"] < b["lo"])
    assert disjoint.mean() > 0.99
    # the silent stretch is longer than a tile, and the windows the GPU tests read see unclamped entries too
    act = L.active_frames(x)
    assert not np.any(act[2502:3498]) and act[2501] and act[3499]
    w0 = L.window(ls, 0)
    assert (w0["lo"] > (glo - 8.0 + 4.0) / 4.0 + 1e-3).mean() > 0.3
