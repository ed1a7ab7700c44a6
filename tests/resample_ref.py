"""The yardstick of the resampler tests: `wis_hip.audio.resample`'s sum restated in direct form and evaluated in fp64 over the
fp64 prototype, with what the comparison bound needs.

    y[m] = sum over k in [0, n_in) of x[k] h[m down - k up + half],   h = audio._resample_filter(up, down)

The bound on an f32 engine (csrc/resample.hip) against y64 is derived, not measured:
  * every tap is rounded to f32 once: 2^-24 relative per term;
  * one more ulp per term for the C and the numpy prototype differing below f32 resolution (two fp64 evaluations of one
    closed form agree to ~1e-13 of the peak tap; where that moves an f32 rounding it moves it by one ulp);
  * a T-term f32 sum in any order (fused or not): (T - 1) 2^-24 relative to the sum of magnitudes, to first order;
  * the final product's own rounding is inside the (T - 1) + 1 = T of the sum.
So  |y_gpu[m] - y64[m]| <= (T + 3) 2^-24 B[m],  B[m] = sum_k |x[k] h[tap]|, T the largest number of terms of any output.
"""
import math

import numpy as np

from wis_hip import audio

EPS32 = 2.0 ** -24


def ratio(sr_in, sr_out=16000):
    g = math.gcd(int(sr_in), int(sr_out))
    return sr_out // g, int(sr_in) // g


def resample_ref(x, sr_in):
    """-> (y64 [n_out] fp64, B [n_out] fp64, T int): the direct-form sum, its sum of magnitudes, the largest term count of an output"""
    x = np.asarray(x, np.float64).reshape(-1)
    up, down = ratio(sr_in)
    h = audio._resample_filter(up, down)
    L = h.shape[0]
    half = (L - 1) // 2
    n_in = x.shape[0]
    n_out = -(-n_in * up // down)
    tpp = -(-L // up)
    m = np.arange(n_out, dtype=np.int64)
    c = m * down + half
    k_hi = c // up                                   # the last sample with a tap
    t0 = c - k_hi * up                               # its tap, 0 <= t0 < up; sample k_hi - j meets tap t0 + j up
    hp = np.concatenate([h, np.zeros(up * tpp - L + up)])
    xp = np.concatenate([np.zeros(tpp), x, np.zeros(tpp + down + 2)])
    y = np.zeros(n_out, np.float64)
    B = np.zeros(n_out, np.float64)
    for j in range(tpp):
        k = k_hi - j
        term = xp[np.clip(k, -tpp, n_in + tpp) + tpp] * hp[t0 + j * up]
        y += term
        B += np.abs(term)
    j_max = np.minimum((L - 1 - t0) // up, k_hi)      # taps inside the prototype and samples k >= 0
    j_min = np.maximum(0, k_hi - (n_in - 1))         # samples k < n_in
    T = int(np.maximum(j_max - j_min + 1, 0).max()) if n_out else 0
    return y, B, T


def bound(B, T):
    return (T + 3) * EPS32 * B
