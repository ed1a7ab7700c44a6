"""The resampler's host entries (wis_resample_plan, wis_resample_filter: no GPU) against wis_hip.audio's definitions, and the
tests' fp64 yardstick (tests/resample_ref.py) against `audio.resample`, the function the existing tests pin."""
import ctypes as C
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from resample_ref import ratio, resample_ref  # noqa: E402

from wis_hip import audio  # noqa: E402

WIS_E_ARG, WIS_E_UNSUPPORTED = -1, -7
RATES = (8000, 11025, 22050, 24000, 32000, 44100, 48000, 96000)


def _plan(lib, sr_in, n_in):
    up, down, tpp, n_out, n_taps = C.c_int(), C.c_int(), C.c_int(), C.c_int64(), C.c_int64()
    rc = lib.wis_resample_plan(sr_in, n_in, C.byref(up), C.byref(down), C.byref(n_out), C.byref(tpp), C.byref(n_taps))
    return rc, up.value, down.value, n_out.value, tpp.value, n_taps.value


@pytest.mark.parametrize("sr_in", RATES)
def test_plan_matches_audio_resample(lib, sr_in):
    g = math.gcd(sr_in, 16000)
    up, down = 16000 // g, sr_in // g
    n_taps = audio._resample_filter(up, down).shape[0]
    for n_in in (0, 1, 2, down - 1, down, down + 1, 12345):
        rc, u, d, n_out, tpp, nt = _plan(lib, sr_in, n_in)
        assert rc == 0
        assert (u, d, nt) == (up, down, n_taps)
        assert tpp == -(-n_taps // up)
        assert n_out == audio.resample(np.zeros(n_in, np.float32), sr_in).shape[0] == -(-n_in * up // down)


def test_plan_errors(lib):
    assert _plan(lib, 47999, 100)[0] == WIS_E_UNSUPPORTED
    assert b"taps" in lib.wis_last_error()
    for sr in (0, -1, -16000):
        assert _plan(lib, sr, 100)[0] == WIS_E_ARG
    assert _plan(lib, 48000, -1)[0] == WIS_E_ARG
    assert lib.wis_resample_plan(48000, 10, None, None, None, None, None) == 0      # every out pointer is optional


@pytest.mark.parametrize("up,down", [(1, 3), (160, 441), (320, 441), (2, 1), (640, 441), (1, 2), (2, 3), (1, 6)])
def test_prototype_matches_numpy(lib, up, down):
    """two fp64 evaluations of one closed form: 2^-30 of the peak tap is 32 times under half an f32 ulp (the f32 tables agree
    except at rounding ties) and four orders above fp64 evaluation noise"""
    ref = audio._resample_filter(up, down)
    h = np.full(ref.shape[0] + 3, 7.0, np.float64)
    assert lib.wis_resample_filter(up, down, h.ctypes.data_as(C.POINTER(C.c_double)), ref.shape[0]) == 0
    assert np.all(h[ref.shape[0]:] == 7.0)
    err = float(np.abs(h[:ref.shape[0]] - ref).max())
    print(f"{up}/{down}: {ref.shape[0]} taps, max |C - numpy| = {err:.3e} = {err / np.abs(ref).max():.3e} of the peak")
    assert err <= 2.0 ** -30 * np.abs(ref).max()
    assert lib.wis_resample_filter(up, down, h.ctypes.data_as(C.POINTER(C.c_double)), ref.shape[0] - 1) == WIS_E_ARG


def test_filter_errors(lib):
    h = np.zeros(8, np.float64)
    p = h.ctypes.data_as(C.POINTER(C.c_double))
    assert lib.wis_resample_filter(0, 1, p, 8) == WIS_E_ARG
    assert lib.wis_resample_filter(1, 47999, p, 8) == WIS_E_UNSUPPORTED


def test_same_rate_and_empty_need_no_gpu(lib):
    x = np.random.default_rng(0).standard_normal(100).astype(np.float32)
    out = np.zeros(100, np.float32)
    n = C.c_int64(-1)
    assert lib.wis_resample(0, x.ctypes.data_as(C.c_void_p), 100, 16000, out.ctypes.data_as(C.c_void_p), 100, C.byref(n)) == 0
    assert n.value == 100 and np.array_equal(out, x)
    assert lib.wis_resample(0, None, 0, 48000, None, 0, C.byref(n)) == 0 and n.value == 0
    assert lib.wis_resample(0, x.ctypes.data_as(C.c_void_p), 100, 47999, out.ctypes.data_as(C.c_void_p), 100, C.byref(n)) == WIS_E_UNSUPPORTED


def test_python_host_path_is_untouched_without_a_device():
    x = np.random.default_rng(1).standard_normal(500).astype(np.float32)
    assert np.array_equal(audio.resample(x, 48000), audio.resample(x, 48000, 16000, device=None))
    assert np.array_equal(audio.resample(x, 16000, 48000, device=0), audio.resample(x, 16000, 48000))      # sr_out != 16000: numpy
    assert audio.resample(np.zeros(0, np.float32), 48000, device=0).shape == (0,)
    with pytest.raises(ValueError):
        audio.resample(x, 0, device=0)


@pytest.mark.parametrize("sr_in,n_in", [(48000, 3 * 513 + 1), (44100, 441 * 3 + 1), (8000, 129), (11025, 1000), (96000, 6 * 300 + 5), (22050, 2 * 441 + 7)])
def test_yardstick_equals_audio_resample(sr_in, n_in):
    """resample_ref's fp64 direct form, rounded to f32, IS audio.resample on the same input"""
    rng = np.random.default_rng(sr_in)
    for x in (rng.standard_normal(n_in) * 0.1, np.ones(n_in), np.eye(1, n_in, 0)[0], np.eye(1, n_in, n_in - 1)[0]):
        x = x.astype(np.float32)
        y64, B, T = resample_ref(x, sr_in)
        up, down = ratio(sr_in)
        assert y64.shape[0] == -(-n_in * up // down)
        assert 1 <= T <= -(-audio._resample_filter(up, down).shape[0] // up)
        assert np.all(np.abs(y64) <= B * (1 + 1e-12))
        assert np.array_equal(y64.astype(np.float32), audio.resample(x, sr_in))
