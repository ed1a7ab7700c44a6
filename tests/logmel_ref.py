"""The yardstick of the log-mel tests (csrc/logmel.hip): the front end restated in numpy and evaluated in float64, with an interval for
every entry that is derived from the number formats and the order of the kernel's sums, never from what the kernel gives.

    window w of 480000 samples (pad_or_trim), reflect-padded by 200; frame t = samples 160 t - 200 .. 160 t + 199, t < 3000
    re[t][k] = sum_n x_n D[n][k],  im[t][k] = sum_n x_n D[n][201 + k],   D[n][k] = w_n cos(2 pi (n k % 400) / 400), D[n][201 + k] = -w_n sin(..),
                                                                          w the periodic Hann window; D rounded to f32 as the kernel's table is
    p = re^2 + im^2;  mel = F p  (F: the Slaney bank, built in float64 and rounded to f32);  lg = log10(max(mel, 1e-10))
    the window's value: (max(lg, max lg - 8) + 4) / 4

The kernel's sum runs in 100 steps j, each adding the four products of n = 4 j .. 4 j + 3 to the accumulator (v_mfma_f32_16x16x4_f32).  With
u = 2^-24, every product, the 4 + 1 term sum of a step and every f32 coefficient rounded to nearest once:

    S = sum_j |s_j|  (s_j the partial sum after step j),  A = sum_n |x_n| |D_n|
    E    = u (4 S + 8 A)                                         on re and on im
    dp   = 2 (|re| E_re + |im| E_im) + E_re^2 + E_im^2 + 4 u p   on the power
    dmel = F dp + (L + 2) u mel                                  L the widest filter row in bins (an fma chain over non-negative terms)
    lg in [log10(max(mel - dmel, 1e-10)) - e, log10(max(mel + dmel, 1e-10)) + e],  e = 8 u max(1, |log10 mel|)   (log10f, the f32 clamp constant)

No entry is excluded: an entry whose power nearly cancels has a wide interval, and it is still an interval.  Bin 200 (8 kHz) has zero weight in
both banks, so nothing of it can be observed in the output and nothing here tests it.

numpy only: nothing of the product is imported here.
"""
import numpy as np

U = 2.0 ** -24
SAMPLE_RATE, N_FFT, HOP, N_SAMPLES, N_FRAMES, N_BIN = 16000, 400, 160, 480000, 3000, 201
FT = 16                        # frames per tile of the kernel
N_TILES = -(-N_FRAMES // FT)   # 188
CONTENT = 40001                # samples of a short case: 251 frames, ends inside a frame and inside a tile
BROADBAND = ("gauss_0.1", "gauss_3e4", "gauss_1e-4", "gauss_exponents")


# ---- tables ---------------------------------------------------------------------------------------------------------------------
def _hz_to_mel(f):
    f = np.asarray(f, np.float64)
    f_sp, min_log_hz = 200.0 / 3, 1000.0
    return np.where(f >= min_log_hz, min_log_hz / f_sp + np.log(np.maximum(f, 1e-300) / min_log_hz) / (np.log(6.4) / 27.0), f / f_sp)


def _mel_to_hz(m):
    m = np.asarray(m, np.float64)
    f_sp, min_log_hz = 200.0 / 3, 1000.0
    min_log_mel = min_log_hz / f_sp
    return np.where(m >= min_log_mel, min_log_hz * np.exp((np.log(6.4) / 27.0) * (m - min_log_mel)), f_sp * m)


def mel_bank(n_mels):
    """-> f32 [n_mels][201]: Slaney-scale triangles with Slaney area normalisation, float64 then rounded once"""
    freqs = (SAMPLE_RATE / 2.0) * np.arange(N_BIN) / (N_BIN - 1)
    pts = _mel_to_hz(np.linspace(_hz_to_mel(0.0), _hz_to_mel(SAMPLE_RATE / 2.0), n_mels + 2))
    lower = (freqs[None, :] - pts[:-2, None]) / (pts[1:-1] - pts[:-2])[:, None]
    upper = (pts[2:, None] - freqs[None, :]) / (pts[2:] - pts[1:-1])[:, None]
    w = np.maximum(0.0, np.minimum(lower, upper)) * (2.0 / (pts[2:] - pts[:-2]))[:, None]
    return w.astype(np.float32)


def bank_width(bank):
    """L: the widest row, first to last non-zero weight, in bins"""
    nz = bank != 0
    first = nz.argmax(axis=1)
    last = N_BIN - 1 - nz[:, ::-1].argmax(axis=1)
    return int((last - first + 1)[nz.any(axis=1)].max())


def hann(periodic=True):
    return 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(N_FFT) / (N_FFT if periodic else N_FFT - 1))


def dft_matrix(rounded=True, window=None):
    """-> [400][402]: cos columns, then -sin columns; angles reduced as (n k) % 400.  rounded: to f32 (returned as float64 of the f32 values)"""
    w = hann() if window is None else window
    n, k = np.arange(N_FFT)[:, None], np.arange(N_BIN)[None, :]
    ang = 2.0 * np.pi * ((n * k) % N_FFT) / N_FFT
    D = np.concatenate([w[:, None] * np.cos(ang), -w[:, None] * np.sin(ang)], axis=1)
    return D.astype(np.float32).astype(np.float64) if rounded else D


# ---- frames -----------------------------------------------------------------------------------------------------------------------
def window_of(x, n_valid=None):
    """pad_or_trim: the first min(n_valid, 480000) samples of x, zeros behind them -> f32 [480000]"""
    x = np.asarray(x, np.float32).reshape(-1)
    n = x.shape[0] if n_valid is None else int(n_valid)
    n = max(0, min(n, N_SAMPLES, x.shape[0]))
    out = np.zeros(N_SAMPLES, np.float32)
    out[:n] = x[:n]
    return out


def padded(win):
    return np.pad(np.asarray(win), (N_FFT // 2, N_FFT // 2), mode="reflect")


def frames_of(win, idx):
    """-> [len(idx)][400]: frame t = padded[160 t : 160 t + 400]"""
    y = padded(win)
    return y[np.asarray(idx, np.int64)[:, None] * HOP + np.arange(N_FFT)[None, :]]


def active_frames(win):
    """-> bool [3000]: the frame's 400-sample span holds a non-zero sample"""
    c = np.concatenate([[0], np.cumsum(padded(win) != 0)])
    t = np.arange(N_FRAMES) * HOP
    return c[t + N_FFT] > c[t]


def active_tiles(win):
    """-> bool [188]: the tile's 2800-sample span holds a non-zero sample (the kernel's all-silent shortcut is taken on the others)"""
    a = np.concatenate([active_frames(win), np.zeros(N_TILES * FT - N_FRAMES, bool)])
    return a.reshape(N_TILES, FT).any(axis=1)


# ---- the float64 sums in the kernel's order -------------------------------------------------------------------------------------
def spectrum(fr, D=None):
    """fr [T][400] -> dict of float64 [T][201] arrays: re, im, and the error bounds E_re, E_im of an f32 engine that sums in 100 steps of four"""
    D = dft_matrix() if D is None else D
    fr = np.asarray(fr, np.float64)
    acc = np.zeros((fr.shape[0], 2 * N_BIN))
    S = np.zeros_like(acc)
    for j in range(N_FFT // 4):
        acc = acc + fr[:, 4 * j:4 * j + 4] @ D[4 * j:4 * j + 4]
        S += np.abs(acc)
    A = np.abs(fr) @ np.abs(D)
    E = U * (4.0 * S + 8.0 * A)
    return {"re": acc[:, :N_BIN], "im": acc[:, N_BIN:], "E_re": E[:, :N_BIN], "E_im": E[:, N_BIN:]}


def intervals(sp, bank):
    """sp: spectrum(); bank f32 [n_mels][201] -> dict of float64 [n_mels][T]: centre, lo, hi (log10 units), mel, dmel"""
    F = bank.astype(np.float64)
    re, im, Er, Ei = sp["re"], sp["im"], sp["E_re"], sp["E_im"]
    p = re * re + im * im
    dp = 2.0 * (np.abs(re) * Er + np.abs(im) * Ei) + Er * Er + Ei * Ei + 4.0 * U * p
    mel = F @ p.T
    dmel = F @ dp.T + (bank_width(bank) + 2) * U * mel
    centre = np.log10(np.maximum(mel, 1e-10))
    e = 8.0 * U * np.maximum(1.0, np.abs(centre))
    lo = np.log10(np.maximum(mel - dmel, 1e-10)) - e
    hi = np.log10(np.maximum(mel + dmel, 1e-10)) + e
    return {"centre": centre, "lo": lo, "hi": hi, "mel": mel, "dmel": dmel}


def logmel_ref(win, n_mels, idx=None, D=None, bank=None):
    """win f32 [480000] (window_of), idx: the frames wanted (default: the active ones) -> (idx, intervals() of those frames)"""
    idx = np.nonzero(active_frames(win))[0] if idx is None else np.asarray(idx, np.int64)
    bank = mel_bank(n_mels) if bank is None else bank
    return idx, intervals(spectrum(frames_of(win, idx), D), bank)


def ratio(lg, iv):
    """|lg - centre| / half-width, with the half-width of the side lg lies on: <= 1 exactly when lg is inside [lo, hi]"""
    lg = np.asarray(lg, np.float64)
    d = lg - iv["centre"]
    half = np.where(d >= 0, iv["hi"] - iv["centre"], iv["centre"] - iv["lo"])
    return np.abs(d) / half


def outside(lg, iv):
    lg = np.asarray(lg, np.float64)
    return (lg < iv["lo"]) | (lg > iv["hi"]) | ~np.isfinite(lg)


def floor_scale(lg, dtype=np.float64):
    """the window's value from its whole log10 spectrum [n_mels][3000]: (max(lg, max lg - 8) + 4) / 4, every step one operation of dtype"""
    lg = np.asarray(lg, dtype)
    return (np.maximum(lg, lg.max() - dtype(8.0)) + dtype(4.0)) / dtype(4.0)


def logmel_full(win, n_mels=80, rounded=True):
    """-> float64 [n_mels][3000]: the whole window through floor and scale (rounded=False: the DFT table in full float64)"""
    lg = np.full((n_mels, N_FRAMES), -10.0)
    idx, iv = logmel_ref(win, n_mels, D=dft_matrix(rounded))
    lg[:, idx] = iv["centre"]
    return floor_scale(lg)


# ---- the signals of the tests ---------------------------------------------------------------------------------------------------
TONE_BINS = (0, 1, 7, 8, 199)      # the packed DFT table holds 8 bins per column tile: first / last of a tile, DC, and the last observable bin


def signals(n=CONTENT, seed=20):
    """-> dict name -> f32 [n]; seeded.  BROADBAND names the ones whose intervals are narrow everywhere (white spectra)"""
    rng = np.random.default_rng(seed)
    t = np.arange(n, dtype=np.float64)
    out = {"gauss_0.1": 0.1 * rng.standard_normal(n), "gauss_3e4": 3e4 * rng.standard_normal(n), "gauss_1e-4": 1e-4 * rng.standard_normal(n),
           "gauss_exponents": rng.standard_normal(n) * 2.0 ** (-12.0 * rng.random(n)),
           "gauss_2e-6": 2e-6 * rng.standard_normal(n)}      # straddles the 1e-10 clamp; the window's maximum is negative
    f0, f1 = 50.0, 7900.0
    out["chirp"] = 0.5 * np.sin(2.0 * np.pi * (f0 * t + 0.5 * (f1 - f0) * t * t / max(n, 1)) / SAMPLE_RATE)
    for b in TONE_BINS:
        ang = 2.0 * np.pi * ((b * np.arange(n)) % N_FFT) / N_FFT
        out[f"tone{b}_cos"] = 0.5 * np.cos(ang) + 1e-3 * rng.standard_normal(n)
        out[f"tone{b}_sin"] = 0.5 * np.sin(ang) + 1e-3 * rng.standard_normal(n)
    return {k: v.astype(np.float32) for k, v in out.items()}


def place(x, right=False):
    """the content at the left edge of the window, or in its last len(x) samples -> f32 [480000]"""
    out = np.zeros(N_SAMPLES, np.float32)
    if right:
        out[N_SAMPLES - x.shape[0]:] = x
    else:
        out[:x.shape[0]] = x
    return out
