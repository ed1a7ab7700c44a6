"""gpu: the log-mel front end (csrc/logmel.hip: logmel_stft_kernel, logmel_finalize_kernel) through the tap wis_op_logmel, which exposes the kernels'
scratch: every entry of the log10 spectrum against the float64 reference of tests/logmel_ref.py and its derived interval (the docstring there has the
derivation; tests/test_logmel_ref_cpu.py shows that it is sound and sharp), and everything behind the spectrum - the maximum key, the floor and scale,
the conv1 image the product reads - against numpy expressions on the GPU's own spectrum, bit for bit.

Common to every run (run_op): the output buffers are pre-filled with a bit pattern nothing produces, the run is made twice and both must agree to the
bit, the device PCM holds non-zero garbage wherever the window has no valid sample.  check_spectrum evaluates the reference on frames whose 400-sample
span holds a non-zero sample; every other frame must be -10.0f exactly.  The window is always 480000 samples (3000 frames): the content is the shape -
about 40001 samples (251 frames) unless the case is about a longer one.

Bin 200 (8 kHz) has zero weight in both banks: a wrong column 200 of the DFT table cannot be observed, and no case here pretends to test it.
NaN / Inf samples and timing are not in scope."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import logmel_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
WIS_E_ARG, WIS_E_UNSUPPORTED = -1, -7
PAT16, PAT32 = 0x5A5A, 0x5A5A5A5A      # f16 203.25 / f32 1.5e16: nothing these kernels produce
MINUS_TEN = 0xC1200000                 # -10.0f: log10f of the clamp constant
NS, NF, NT = R.N_SAMPLES, R.N_FRAMES, R.N_TILES
F32 = np.float32
BANKS = {n: R.mel_bank(n) for n in (80, 128)}
DFT = R.dft_matrix()


def conv_c(n_mels):
    return 96 if n_mels == 80 else n_mels


def device_pcm(contents, stride, seed=1):
    """contents: per window the valid samples (f32, at most 480000) -> f32 [(n_win - 1) stride + 480000], non-zero garbage everywhere else"""
    rng = np.random.default_rng(seed)
    buf = (7.5 + rng.random((len(contents) - 1) * stride + NS)).astype(F32)
    for w, x in enumerate(contents):
        buf[w * stride:w * stride + x.shape[0]] = x
    return buf


class Out:
    pass


def run_once(lib, n_mels, d_pcm, stride, nsamp, tile0, n_tiles, want_mel, want_img):
    from wis_hip import _lib
    n_win = len(nsamp)
    ns = (C.c_int64 * n_win)(*nsamp)
    d_lg = _lib.DevBuf.from_numpy(np.full(n_win * n_mels * NF, PAT32, np.uint32))
    d_gm = _lib.DevBuf.from_numpy(np.full(max(n_win, 4), PAT32, np.uint32))
    d_mel = _lib.DevBuf.from_numpy(np.full(n_win * n_mels * NF, PAT32, np.uint32)) if want_mel else None
    d_img = _lib.DevBuf.from_numpy(np.full(n_win * (NF + 2) * conv_c(n_mels), PAT16, np.uint16)) if want_img else None
    o = Out()
    o.rc = lib.wis_op_logmel(0, n_mels, d_pcm.ptr, stride, ns, n_win, tile0, n_tiles, d_lg.ptr, d_gm.ptr, d_mel.ptr if d_mel else None, d_img.ptr if d_img else None)
    o.lg = d_lg.to_numpy(np.uint32, (n_win, n_mels, NF))
    o.gmax = d_gm.to_numpy(np.uint32, (max(n_win, 4),))
    assert np.all(o.gmax[n_win:] == PAT32), "wrote behind d_gmax[n_win]"
    o.gmax = o.gmax[:n_win]
    o.mel = d_mel.to_numpy(np.uint32, (n_win, n_mels, NF)) if d_mel else None
    o.img = d_img.to_numpy(np.uint16, (n_win, NF + 2, conv_c(n_mels))) if d_img else None
    for b in (d_lg, d_gm, d_mel, d_img):
        if b:
            b.free()
    return o


def run_op(lib, n_mels, pcm, stride, nsamp, tile0=0, n_tiles=NT, want_mel=True, want_img=True):
    """two runs on fresh pattern-filled buffers, which must agree to the bit -> the outputs as raw bits"""
    from wis_hip import _lib
    d_pcm = _lib.DevBuf.from_numpy(pcm)
    a, b = (run_once(lib, n_mels, d_pcm, stride, nsamp, tile0, n_tiles, want_mel, want_img) for _ in range(2))
    d_pcm.free()
    assert a.rc == 0 and b.rc == 0, lib.wis_last_error()
    for k in ("lg", "gmax", "mel", "img"):
        if getattr(a, k) is not None:
            assert np.array_equal(getattr(a, k), getattr(b, k)), f"two runs differ in {k}"
    return a


def fkey_inv(k):
    k = np.asarray(k, np.uint32)
    return np.where(k & np.uint32(0x80000000), k & np.uint32(0x7FFFFFFF), ~k).astype(np.uint32).view(F32)


def check_spectrum(lg_bits, win, n_mels, what, frames=None, sp_cache=None):
    """lg_bits u32 [n_mels][3000] of the window `win` (f32 [480000], zeros where nothing is valid); frames: the frames to hold against the float64
    reference (default: all), of which the active ones are evaluated.  Every inactive frame of the window must be -10.0f.  -> worst ratio"""
    active = R.active_frames(win)
    assert np.all(lg_bits[:, ~active] == MINUS_TEN), (what, "a silent frame is not -10.0f")
    sel = active if frames is None else active & np.isin(np.arange(NF), frames)
    idx = np.nonzero(sel)[0]
    if idx.size == 0:
        print(f"{what}: no active frame")
        return 0.0
    key = (id(win), idx.tobytes())
    if sp_cache is not None and key in sp_cache:
        sp = sp_cache[key]
    else:
        sp = R.spectrum(R.frames_of(win, idx), DFT)
        if sp_cache is not None:
            sp_cache[key] = sp
    iv = R.intervals(sp, BANKS[n_mels])
    lg = lg_bits[:, idx].view(F32)
    r = R.ratio(lg, iv)
    worst = float(r.max())
    print(f"{what}: {idx.size} frames x {n_mels} bins, worst |lg - centre| / half-width {worst:.3f}")
    bad = np.argwhere(R.outside(lg, iv))
    assert bad.shape[0] == 0, (what, bad.shape[0], [(int(m), int(idx[t]), float(lg[m, t]), float(iv["lo"][m, t]), float(iv["hi"][m, t])) for m, t in bad[:6]])
    return worst


def check_finalize(o, n_mels, what):
    """everything behind the spectrum, from the GPU's own spectrum, bit for bit"""
    for w in range(o.lg.shape[0]):
        L = o.lg[w].view(F32)
        assert np.all(np.isfinite(L)), what
        assert fkey_inv(o.gmax[w]).view(np.uint32) == L.max().view(np.uint32), (what, w, "d_gmax is not the key of the window's maximum")
        want = R.floor_scale(L, F32)
        if o.mel is not None:
            assert want.dtype == F32 and np.array_equal(o.mel[w], want.view(np.uint32)), (what, w, "d_mel")
        if o.img is not None:
            img = o.img[w]
            assert np.array_equal(img[1:NF + 1, :n_mels], want.astype(np.float16).T.view(np.uint16)), (what, w, "image rows 1 .. 3000")
            assert np.all(img[0] == PAT16) and np.all(img[NF + 1] == PAT16), (what, w, "image rows 0 / 3001 were written")
            assert np.all(img[1:NF + 1, n_mels:] == 0), (what, w, "pad columns")


def same_bits(a, b, w_a=0, w_b=0):
    return all(np.array_equal(getattr(a, k)[w_a], getattr(b, k)[w_b]) for k in ("lg", "gmax", "mel", "img") if getattr(a, k) is not None and getattr(b, k) is not None)


@pytest.fixture(scope="module")
def sig():
    return R.signals()


@pytest.fixture(scope="module")
def long_noise():
    return (0.1 * np.random.default_rng(480).standard_normal(NS)).astype(F32)


# ---- signals, at both edges of the window ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(R.signals(8)))
def test_signals_at_both_edges(lib, sig, name):
    x = sig[name]
    for right in (False, True):
        win = R.place(x, right)
        # left: the content is the valid length; right: the whole window is valid (its zeros are samples), so the reflection at 479999 and
        # tile 187 (8 valid frames) are reached
        pcm, n = (device_pcm([x], NS), x.shape[0]) if not right else (win, NS)
        cache = {}
        for n_mels in (80, 128):
            what = f"{name} {'right' if right else 'left'} {n_mels}"
            o = run_op(lib, n_mels, pcm, NS, [n])
            check_spectrum(o.lg[0], win, n_mels, what, sp_cache=cache)
            check_finalize(o, n_mels, what)


def test_floor_cases(lib, sig):
    """the floor on both sides, the negative maximum, the all-silent window"""
    x = sig["gauss_0.1"]
    o = run_op(lib, 80, device_pcm([x], NS), NS, [x.shape[0]])
    L = o.lg[0].view(F32)
    floor_ = L.max() - F32(8)
    assert (L < floor_).any() and (L > floor_).any() and L.max() > -8      # silence is below the floor, the signal above it
    assert (o.mel[0].view(F32) == (floor_ + F32(4)) / F32(4)).any()
    check_finalize(o, 80, "both sides of the floor")
    x = sig["gauss_2e-6"]
    o = run_op(lib, 80, device_pcm([x], NS), NS, [x.shape[0]])
    L = o.lg[0].view(F32)
    assert -10 < L.max() < 0 and (L == F32(-10)).any() and (o.gmax[0] & 0x80000000) == 0      # negative maximum: the key is the complement
    check_finalize(o, 80, "negative maximum")
    o = run_op(lib, 128, device_pcm([x[:0]], NS), NS, [0])
    assert np.all(o.lg == MINUS_TEN) and fkey_inv(o.gmax[0]) == F32(-10) and np.all(o.mel.view(F32) == F32(-1.5))
    check_finalize(o, 128, "all-silent window")


# ---- content lengths ------------------------------------------------------------------------------------------------------------------------
ALL_FRAMES = (479799, 479999, 480000)


@pytest.mark.parametrize("n", [0, 1, 199, 200, 201, 2360, 2361, 2559, 2560, 2600, 2601, 40001, 479799, 479800, 479801, 479999, 480000])
def test_content_lengths(lib, long_noise, n):
    """gaussian 0.1 on [0, n), garbage behind it: lengths that end inside a frame, inside a tile, where tile 1 stops being all-silent (its span
    starts at sample 2360), around the end of tile 0's span (2600) and within 200 samples of the right edge, where the reflection reads past n"""
    x = long_noise[:n]
    win = R.window_of(long_noise, n)
    pcm = device_pcm([x], NS)
    if n in ALL_FRAMES:
        frames = None
    else:
        t = n // R.HOP
        frames = np.concatenate([np.arange(16), np.arange(NF - 16, NF), np.arange(max(t - 4, 0), min(t + 5, NF))])
    cache = {}
    for n_mels in (80, 128):
        o = run_op(lib, n_mels, pcm, NS, [n], want_img=False)
        check_spectrum(o.lg[0], win, n_mels, f"n = {n}, {n_mels} bins", frames, cache)
        check_finalize(o, n_mels, f"n = {n}")
        # which tiles are silent is visible in the spectrum only as -10.0f frames: check_spectrum has held every one of them


def test_lengths_outside_the_window(lib, long_noise):
    """n_samples reaches the kernel unclamped: above 480000 it is the full window, below 0 the empty one"""
    pcm = long_noise.copy()
    full = run_op(lib, 80, pcm, NS, [NS])
    empty = run_op(lib, 80, pcm, NS, [0])
    assert np.all(empty.lg == MINUS_TEN)
    for n, want in ((NS + 1, full), (10 ** 12, full), (-5, empty)):
        o = run_op(lib, 80, pcm, NS, [n])
        assert same_bits(o, want), n


# ---- impulses -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pos", [0, 1234, 2360, 2399, 2400, 2599, 479999])
def test_impulse(lib, pos):
    """one sample of 0.5 in a valid window of zeros.  Tile j stages samples 2560 j - 200 .. 2560 j + 2599: 2599 is the last sample of tile 0's span,
    2360 the first of tile 1's.  A tile whose span holds the impulse must compute (its active frames are held against the reference), every other
    tile may take the all-silent shortcut, and either way an inactive frame is -10.0f."""
    win = np.zeros(NS, F32)
    win[pos] = 0.5
    tiles = np.nonzero(R.active_tiles(win))[0].tolist()
    assert tiles == {0: [0], 1234: [0], 2360: [0, 1], 2399: [0, 1], 2400: [0, 1], 2599: [0, 1], 479999: [187]}[pos]
    cache = {}
    for n_mels in (80, 128):
        o = run_op(lib, n_mels, win, NS, [NS], want_img=False)
        check_spectrum(o.lg[0], win, n_mels, f"impulse at {pos}, {n_mels} bins", sp_cache=cache)
        check_finalize(o, n_mels, f"impulse at {pos}")


# ---- batch and strides ----------------------------------------------------------------------------------------------------------------------
def test_batch_and_strides(lib, sig, long_noise):
    xs = [sig["gauss_3e4"], np.zeros(0, F32), (long_noise * F32(1e-3)).astype(F32)]      # amplitudes 3e4 / - / 1e-4: three floors
    ns = [x.shape[0] for x in xs]
    assert ns == [R.CONTENT, 0, NS]
    wins = [R.window_of(x) for x in xs]
    for n_mels in (80, 128):
        alone = [run_op(lib, n_mels, device_pcm([x], NS), NS, [n]) for x, n in zip(xs, ns)]
        for stride in (NS, NS + 37):
            o = run_op(lib, n_mels, device_pcm(xs, stride), stride, ns)
            check_finalize(o, n_mels, f"batch, stride {stride}")
            assert len({int(k) for k in o.gmax}) == 3
            for w in range(3):
                assert same_bits(o, alone[w], w, 0), (n_mels, stride, w)
        check_spectrum(alone[0].lg[0], wins[0], n_mels, f"batch window 0 (3e4), {n_mels} bins")
        check_spectrum(alone[2].lg[0], wins[2], n_mels, f"batch window 2 (1e-4), {n_mels} bins", np.concatenate([np.arange(16), np.arange(1490, 1510), np.arange(NF - 16, NF)]))
        o = run_op(lib, n_mels, device_pcm(xs[:1], NS), 0, [ns[0]] * 3)      # stride 0: the same window three times
        for w in range(3):
            assert same_bits(o, alone[0], w, 0), (n_mels, "stride 0", w)


# ---- the product's form: image only ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_mels", [80, 128])
def test_image_only_form(lib, sig, long_noise, n_mels):
    """stage_input runs logmel_device with d_mel null and the image alone: the same image bits as the two-output run"""
    for x in (sig["gauss_0.1"], long_noise):
        pcm = device_pcm([x], NS)
        both = run_op(lib, n_mels, pcm, NS, [x.shape[0]])
        only = run_op(lib, n_mels, pcm, NS, [x.shape[0]], want_mel=False)
        check_finalize(both, n_mels, "mel and image")
        check_finalize(only, n_mels, "image only")
        assert only.mel is None and np.array_equal(only.img, both.img) and np.array_equal(only.lg, both.lg) and np.array_equal(only.gmax, both.gmax)


# ---- tile ranges ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_mels", [80, 128])
def test_tile_ranges(lib, long_noise, n_mels):
    """a range of tiles, as a streaming session runs them: its frames as in the whole run, no other frame touched, the maximum over the range"""
    xs = [long_noise, (long_noise[::-1] * F32(3.0)).astype(F32)]
    pcm = device_pcm(xs, NS + 37)
    whole = run_op(lib, n_mels, pcm, NS + 37, [NS, NS], want_mel=False, want_img=False)
    for tile0, n_tiles in ((0, 1), (187, 1), (93, 2)):
        o = run_op(lib, n_mels, pcm, NS + 37, [NS, NS], tile0, n_tiles, want_mel=False, want_img=False)
        f0, f1 = 16 * tile0, min(16 * (tile0 + n_tiles), NF)
        assert np.array_equal(o.lg[:, :, f0:f1], whole.lg[:, :, f0:f1]), (tile0, n_tiles)
        assert np.all(o.lg[:, :, :f0] == PAT32) and np.all(o.lg[:, :, f1:] == PAT32), (tile0, n_tiles, "a frame outside the range was written")
        for w in range(2):
            assert fkey_inv(o.gmax[w]).view(np.uint32) == o.lg[w, :, f0:f1].view(F32).max().view(np.uint32), (tile0, n_tiles, w)


def test_refusals(lib, long_noise):
    """a range outside [0, 188], mel or image asked of a range (there is no finalize pass), a bank that does not exist: refused, nothing written"""
    from wis_hip import _lib
    d_pcm = _lib.DevBuf.from_numpy(long_noise)
    for n_mels, tile0, n_tiles, mel, img, want in ((80, 187, 2, False, False, WIS_E_ARG), (80, -1, 1, False, False, WIS_E_ARG), (128, 188, 1, False, False, WIS_E_ARG),
                                                   (80, 0, 1, True, False, WIS_E_ARG), (128, 93, 2, False, True, WIS_E_ARG), (80, 1, 187, True, True, WIS_E_ARG),
                                                   (64, 0, NT, False, False, WIS_E_UNSUPPORTED), (64, 0, 1, False, False, WIS_E_UNSUPPORTED)):
        o = _refused(lib, n_mels, d_pcm, tile0, n_tiles, mel, img)
        assert o.rc == want, (n_mels, tile0, n_tiles, mel, img, o.rc, lib.wis_last_error())
        assert np.all(o.lg == PAT32) and (o.mel is None or np.all(o.mel == PAT32)) and (o.img is None or np.all(o.img == PAT16))
    d_pcm.free()


def _refused(lib, n_mels, d_pcm, tile0, n_tiles, mel, img):
    """run_once with buffers sized for 128 bins whatever n_mels says"""
    from wis_hip import _lib
    ns = (C.c_int64 * 1)(NS)
    d_lg = _lib.DevBuf.from_numpy(np.full(128 * NF, PAT32, np.uint32))
    d_gm = _lib.DevBuf.from_numpy(np.full(4, PAT32, np.uint32))
    d_mel = _lib.DevBuf.from_numpy(np.full(128 * NF, PAT32, np.uint32)) if mel else None
    d_img = _lib.DevBuf.from_numpy(np.full((NF + 2) * 128, PAT16, np.uint16)) if img else None
    o = Out()
    o.rc = lib.wis_op_logmel(0, n_mels, d_pcm.ptr, NS, ns, 1, tile0, n_tiles, d_lg.ptr, d_gm.ptr, d_mel.ptr if d_mel else None, d_img.ptr if d_img else None)
    o.lg = d_lg.to_numpy(np.uint32, (128 * NF,))
    o.mel = d_mel.to_numpy(np.uint32, (128 * NF,)) if d_mel else None
    o.img = d_img.to_numpy(np.uint16, ((NF + 2) * 128,)) if d_img else None
    for b in (d_lg, d_gm, d_mel, d_img):
        if b:
            b.free()
    return o


# ---- the public entries run the same kernels ------------------------------------------------------------------------------------------------
def test_public_entries(lib, sig, long_noise):
    from wis_hip import _lib
    xs = [sig["gauss_0.1"], long_noise]
    ns = [x.shape[0] for x in xs]
    stride = NS + 37
    pcm = device_pcm(xs, stride)
    nsv = (C.c_int64 * 2)(*ns)
    host = np.zeros((2, NS), F32)
    for w, x in enumerate(xs):
        host[w, :x.shape[0]] = x
    for n_mels in (80, 128):
        tap = run_op(lib, n_mels, pcm, stride, ns, want_img=False).mel

        def public(fn, args_mel, p, s, on_dev, mel_dev):
            out = np.full((2, n_mels, NF), PAT32, np.uint32)
            d_out = _lib.DevBuf.from_numpy(out) if mel_dev else None
            rc = fn(0, *args_mel, p, s, nsv, 2, on_dev, d_out.ptr if mel_dev else out.ctypes.data_as(C.c_void_p), mel_dev)
            assert rc == 0, lib.wis_last_error()
            if mel_dev:
                out = d_out.to_numpy(np.uint32, (2, n_mels, NF))
                d_out.free()
            return out

        assert np.array_equal(public(lib.wis_logmel_n, (n_mels,), host.ctypes.data_as(C.c_void_p), NS, 0, 0), tap), (n_mels, "host PCM")
        d_pcm = _lib.DevBuf.from_numpy(pcm)
        for mel_dev in (0, 1):
            assert np.array_equal(public(lib.wis_logmel_n, (n_mels,), d_pcm.ptr, stride, 1, mel_dev), tap), (n_mels, "device PCM", mel_dev)
        if n_mels == 80:
            assert np.array_equal(public(lib.wis_logmel, (), d_pcm.ptr, stride, 1, 0), tap), "wis_logmel"
            assert np.array_equal(public(lib.wis_logmel, (), host.ctypes.data_as(C.c_void_p), NS, 0, 0), tap), "wis_logmel, host PCM"
        d_pcm.free()
