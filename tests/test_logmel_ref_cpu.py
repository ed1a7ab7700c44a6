"""not gpu: the float64 yardstick of the log-mel tests (tests/logmel_ref.py) is sound and sharp before any kernel is held against it.

  sound   an f32 emulation of the kernel's arithmetic (f32 table, f32 frames, the accumulator rounded after every step of four, f32 power, bank and
          log10) lies inside every interval, for every signal of tests/test_gpu_logmel_ops.py, both banks, both edges of the window
  sharp   on the broadband signals at least 95 % of the entries of the non-silent frames have an interval narrower than 1e-4 in log10 units
          (2.5e-5 in output units); the tones and the chirp, whose spectra have deep valleys, are not under this cap
  honest  four mistakes a kernel could make, planted into the emulation, fall outside the intervals on every broadband signal
  pinned  the reference in float64, through floor and scale, equals the oracle's float64 front end to 1e-9 and the real reference's golden
          vector within the 5e-5 that pins the oracle
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import logmel_ref as R  # noqa: E402

F32 = np.float32
SHARP_WIDTH, SHARP_SHARE = 1e-4, 0.95


def emulate(fr, bank, D=None):
    """fr [T][400] -> f32 [n_mels][T]: the kernel's arithmetic in f32"""
    D32 = (R.dft_matrix() if D is None else D).astype(F32)
    fr = np.asarray(fr, F32)
    acc = np.zeros((fr.shape[0], 2 * R.N_BIN), F32)
    for j in range(R.N_FFT // 4):
        acc = (acc + (fr[:, 4 * j:4 * j + 4] @ D32[4 * j:4 * j + 4]).astype(F32)).astype(F32)
    re, im = acc[:, :R.N_BIN], acc[:, R.N_BIN:]
    p = (re * re + im * im).astype(F32)
    mel = (p @ bank.T).astype(F32)
    return np.log10(np.maximum(mel, F32(1e-10))).astype(F32).T


@pytest.fixture(scope="module")
def banks():
    return {n: R.mel_bank(n) for n in (80, 128)}


@pytest.fixture(scope="module")
def cases():
    """(name, right) -> (win, idx, frames, spectrum): computed once, shared by every test below, never modified"""
    out = {}
    for name, x in R.signals().items():
        for right in (False, True):
            win = R.place(x, right)
            idx = np.nonzero(R.active_frames(win))[0]
            fr = R.frames_of(win, idx)
            out[name, right] = (win, idx, fr, R.spectrum(fr))
    return out


def test_tables(golden_dir, banks):
    ref = np.load(os.path.join(golden_dir, "mel_filters.npz"))["mel_80"]
    assert banks[80].shape == (80, 201) and banks[80].dtype == F32 and banks[128].shape == (128, 201)
    assert np.abs(banks[80] - ref).max() <= 2e-9 and ((banks[80] != 0) == (ref != 0)).all()
    for n, b in banks.items():
        assert np.all(b[:, 200] == 0) and np.all(b >= 0) and np.all((b != 0).sum(axis=1) >= 1), n      # bin 200 cannot be observed
    D = R.dft_matrix()
    assert D.shape == (400, 402) and np.array_equal(D, D.astype(F32).astype(np.float64))
    assert np.all(D[0] == 0) and np.all(D[:, 201] == 0)      # w_0 = 0; sin(0) = 0
    assert np.abs(R.dft_matrix(False) - D).max() <= 2.0 ** -24


def test_frames_and_activity():
    win = np.zeros(R.N_SAMPLES, F32)
    win[:3] = (1, 2, 3)
    win[-2:] = (8, 9)
    fr = R.frames_of(win, [0, 1, 2999])
    assert fr[0, 198:203].tolist() == [3, 2, 1, 2, 3] and fr[1, 40:43].tolist() == [1, 2, 3]      # reflect: sample 0 is not repeated
    # frame 2999 spans samples 479640 .. 480039: 479998, 479999, then the reflection 479998
    assert fr[2, 358:362].tolist() == [8, 9, 8, 0]
    a = R.active_frames(win)
    assert a[:2].all() and not a[2:2999].any() and a[2999]      # frame 2 starts at sample 120; frame 2998 ends at 479879
    t = R.active_tiles(win)
    assert t[0] and t[187] and not t[1:187].any()
    assert R.window_of(np.ones(5, F32), 3)[:5].tolist() == [1, 1, 1, 0, 0] and not R.window_of(np.ones(5, F32), -5).any()


def test_emulation_is_inside_every_interval(cases, banks):
    for (name, right), (win, idx, fr, sp) in cases.items():
        for n, bank in banks.items():
            iv = R.intervals(sp, bank)
            lg = emulate(fr, bank)
            r = R.ratio(lg, iv)
            print(f"{name} {'right' if right else 'left'} {n}: {idx.size} frames, emulation worst {float(r.max()):.3f} of the half-width")
            assert not R.outside(lg, iv).any(), (name, right, n, int(R.outside(lg, iv).sum()))
            assert np.all(iv["lo"] <= iv["centre"]) and np.all(iv["centre"] <= iv["hi"])


def test_broadband_intervals_are_narrow(cases, banks):
    for (name, right), (win, idx, fr, sp) in cases.items():
        for n, bank in banks.items():
            iv = R.intervals(sp, bank)
            width = iv["hi"] - iv["lo"]
            share = float((width < SHARP_WIDTH).mean())
            print(f"{name} {'right' if right else 'left'} {n}: share narrower than {SHARP_WIDTH:g}: {share:.3f}, median width {float(np.median(width)):.2e}")
            if name in R.BROADBAND:
                assert share >= SHARP_SHARE, (name, right, n, share)


def test_the_small_signal_straddles_the_clamp(cases, banks):
    win, idx, fr, sp = cases["gauss_2e-6", False]
    for n, bank in banks.items():
        mel = R.intervals(sp, bank)["mel"]
        assert (mel < 1e-10).any() and (mel > 1e-10).any() and mel.max() < 1.0      # both sides of the clamp; log10 of the maximum is negative


def _rejected(lg, iv, what):
    n = int(R.outside(lg, iv).sum())
    print(f"{what}: {n} entries outside")
    return n


@pytest.mark.parametrize("name", R.BROADBAND)
def test_planted_mistakes_are_rejected(cases, banks, name):
    sym = R.dft_matrix(window=R.hann(periodic=False))
    for n, bank in banks.items():
        for right in (False, True):
            win, idx, fr, sp = cases[name, right]
            iv = R.intervals(sp, bank)
            side = "right" if right else "left"
            # one weight of one filter off by a thousandth: the peak of a narrow row
            m = n // 8
            bad = bank.copy()
            bad[m, bank[m].argmax()] *= F32(1.001)
            lg = emulate(fr, bad)
            assert _rejected(lg, iv, f"{name} {side} {n}: bank weight [{m}][{int(bank[m].argmax())}] * 1.001") > 0
            assert not R.outside(np.delete(lg, m, axis=0), {k: np.delete(v, m, axis=0) for k, v in iv.items()}).any()      # ... and only in that row
            # the symmetric Hann window (divides by 399) in place of the periodic one
            assert _rejected(emulate(fr, bank, sym), iv, f"{name} {side} {n}: symmetric Hann window") > idx.size * n // 4
        # frame 0 padded by repeating the edge sample (symmetric) in place of reflect
        win, idx, fr, sp = cases[name, False]
        assert idx[0] == 0
        y = np.pad(win, (R.N_FFT // 2, R.N_FFT // 2), mode="symmetric")
        out = R.outside(emulate(y[None, :R.N_FFT], bank), {k: v[:, :1] for k, v in R.intervals(sp, bank).items()})
        print(f"{name} {n}: symmetric padding on frame 0: {int(out.sum())} / {n} entries outside")
        assert out.sum() >= n // 2
        # frame 2999 padded with zeros in place of reflect
        win, idx, fr, sp = cases[name, True]
        assert idx[-1] == R.N_FRAMES - 1
        y = np.pad(win, (R.N_FFT // 2, R.N_FFT // 2))
        f2999 = y[None, (R.N_FRAMES - 1) * R.HOP:(R.N_FRAMES - 1) * R.HOP + R.N_FFT]
        out = R.outside(emulate(f2999, bank), {k: v[:, -1:] for k, v in R.intervals(sp, bank).items()})
        print(f"{name} {n}: zero padding on frame 2999: {int(out.sum())} / {n} entries outside")
        assert out.sum() >= n // 2


def test_agrees_with_the_oracle_in_float64():
    from oracle import audio_ref
    sig = R.signals()
    for name, right in (("gauss_0.1", False), ("chirp", True), ("gauss_2e-6", False)):
        win = R.place(sig[name], right)
        mine = R.logmel_full(win, 80, rounded=False)
        ref = audio_ref.log_mel_spectrogram(win, np.float64)
        err = float(np.abs(mine - ref).max())
        print(f"{name}: float64 reference against the float64 oracle: max abs {err:.2e}")
        assert mine.shape == ref.shape == (80, 3000) and err <= 1e-9


def test_agrees_with_the_golden_vector(golden_dir):
    from wis_hip import audio
    pcm, sr = audio.load_audio(os.path.join(golden_dir, "clips", "3sec.flac"))
    assert sr == 16000
    ref = np.load(os.path.join(golden_dir, "logmel_3sec.npz"))["mel"]
    mine = R.logmel_full(R.window_of(pcm), 80)
    err = float(np.abs(mine - ref).max())
    print(f"3sec clip: float64 reference against the real reference's output: max abs {err:.2e}")
    assert err <= 5e-5


def test_floor_scale_is_the_kernel_expression():
    lg = np.array([[-10.0, -1.0, -3.5], [0.25, -7.75, -7.7500005]], F32)
    out = R.floor_scale(lg, F32)
    assert out.dtype == F32 and out[0, 0] == F32((-7.75 + 4) / 4) and out[1, 0] == F32(4.25 / 4) and out[1, 1] == out[0, 0] == out[1, 2]
