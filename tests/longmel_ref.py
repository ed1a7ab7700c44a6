"""The yardstick of the whole-recording log-mel tests (wis_longmel_*, csrc/logmel.hip): the definition of include/wis_hip.h restated in numpy and
evaluated in float64, on the tables, the sums and the per-entry intervals of tests/logmel_ref.py (imported unchanged).

    the recording of n samples continues with zeros on the right without end; its left edge is reflect-padded by 200 samples; no reflection on the right
    frame t = samples 160 t - 200 .. 160 t + 199,  t = 0 .. n // 160 + 2999
    lg[m][t] = log10(max(mel, 1e-10)), interval as logmel_ref.intervals derives it; a frame that touches no non-zero sample is -10 exactly (a point)
    gmax = max lg over all those frames: inside [max lo, max hi] (the f32 maximum of values that each lie in their interval)
    window(seek)[m][f] = (max(lg[m][seek + f], gmax - 8) + 4) / 4

The last line is three f32 operations on values below 32 in magnitude: the subtraction and the addition round once each (at most 32 u each, u = 2^-24), the
division by 4 is exact: the entry lies in [(max(lo, gmax_lo - 8) + 4) / 4 - 16 u, (max(hi, gmax_hi - 8) + 4) / 4 + 16 u].

numpy only: nothing of the product is imported here.
"""
import numpy as np

import logmel_ref as R

U, HOP, N_FFT, N_FRAMES, FT = R.U, R.HOP, R.N_FFT, R.N_FRAMES, R.FT
SILENT = -10.0
ROUND = 16.0 * U


def content_frames(n):
    return n // HOP


def total_frames(n):
    return n // HOP + N_FRAMES


def touched_frames(n):
    """one past the last frame whose span holds a sample of the recording: 160 t - 200 <= n - 1"""
    return (n + N_FFT // 2 - 1) // HOP + 1 if n > 0 else 0


def stored_frames(n):
    return -(-touched_frames(n) // FT) * FT


def frames_of(x, idx):
    """x f32 [n], idx frame numbers -> f32 [len(idx)][400]: reflected on the left, zeros behind the last sample"""
    x = np.asarray(x, np.float32).reshape(-1)
    p = np.asarray(idx, np.int64)[:, None] * HOP - N_FFT // 2 + np.arange(N_FFT)[None, :]
    p = np.abs(p)
    inside = p < x.shape[0]
    out = np.zeros(p.shape, np.float32)
    out[inside] = x[p[inside]]
    return out


def active_frames(x):
    """-> bool [touched_frames(n)]: the frame's span holds a non-zero sample"""
    x = np.asarray(x, np.float32).reshape(-1)
    t = touched_frames(x.shape[0])
    if t == 0:
        return np.zeros(0, bool)
    return (frames_of(x, np.arange(t)) != 0).any(axis=1)


def log_spectrum(x, n_mels, D=None, sp=None):
    """-> dict centre, lo, hi: float64 [n_mels][touched_frames(n)]; inactive frames are the point -10.  sp: spectrum() of the active frames (shared
    between the two banks)"""
    x = np.asarray(x, np.float32).reshape(-1)
    act = active_frames(x)
    idx = np.nonzero(act)[0]
    out = {k: np.full((n_mels, act.shape[0]), SILENT) for k in ("centre", "lo", "hi")}
    if idx.shape[0]:
        sp = R.spectrum(frames_of(x, idx), D) if sp is None else sp
        iv = R.intervals(sp, R.mel_bank(n_mels))
        for k in out:
            out[k][:, idx] = iv[k]
    return out


def active_spectrum(x, D=None):
    x = np.asarray(x, np.float32).reshape(-1)
    return R.spectrum(frames_of(x, np.nonzero(active_frames(x))[0]), D)


def gmax_interval(ls):
    """(lo, hi) of the recording's maximum; never below -10 (the frames behind the recording)"""
    if ls["lo"].size == 0:
        return SILENT, SILENT
    return max(float(ls["lo"].max()), SILENT), max(float(ls["hi"].max()), SILENT)


def gather(a, seek, fill=SILENT):
    """a [n_mels][T] -> [n_mels][3000]: frames seek .. seek + 2999, `fill` behind T"""
    out = np.full((a.shape[0], N_FRAMES), fill)
    k = max(0, min(N_FRAMES, a.shape[1] - seek))
    out[:, :k] = a[:, seek:seek + k]
    return out


def window(ls, seek, gmax=None):
    """-> dict centre, lo, hi: float64 [n_mels][3000], the window's entries.  gmax: (lo, hi) to clamp against (default: the recording's)"""
    glo, ghi = gmax_interval(ls) if gmax is None else gmax
    gc = max(float(ls["centre"].max()) if ls["centre"].size else SILENT, SILENT) if gmax is None else 0.5 * (glo + ghi)
    return {"centre": (np.maximum(gather(ls["centre"], seek), gc - 8.0) + 4.0) / 4.0,
            "lo": (np.maximum(gather(ls["lo"], seek), glo - 8.0) + 4.0) / 4.0 - ROUND,
            "hi": (np.maximum(gather(ls["hi"], seek), ghi - 8.0) + 4.0) / 4.0 + ROUND}


def window_own_max(ls, seek):
    """the same window clamped against ITS OWN maximum: what a front end that recomputes a pad_or_trim window's floor would give"""
    own = {k: gather(ls[k], seek) for k in ("lo", "hi")}
    return window(ls, seek, gmax=(float(own["lo"].max()), float(own["hi"].max())))


# ---- the 65 s recording of the tests -----------------------------------------------------------------------------------------------
N_65S = 1040000


def recording_65s(seed=20):
    """f32 [1040000] from logmel_ref.signals kinds: 10 s of gauss_0.1, 5 s of gauss_3e4 scaled to an amplitude of 30 (the recording's maximum), 5 s each
    of a tone at bins 7 and 8 (last / first bin of a column tile of the packed DFT table), 10 s of silence (62 tiles), then gauss_1e-4 to the end: the window
    at seek 3000 (30 s .. 60 s) holds silence and the quiet noise only, its own maximum some 11 below the recording's."""
    sg = R.signals(n=480000, seed=seed)
    x = np.zeros(N_65S, np.float32)
    x[0:160000] = sg["gauss_0.1"][:160000]
    x[160000:240000] = sg["gauss_3e4"][:80000] * np.float32(1e-3)
    x[240000:320000] = sg["tone7_cos"][:80000]
    x[320000:400000] = sg["tone8_sin"][:80000]
    x[560000:] = sg["gauss_1e-4"][:N_65S - 560000]
    return x
