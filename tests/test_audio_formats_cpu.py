"""not gpu: the upload decoder (csrc/audio_io.c, `wis_audio_decode` in libwis_hip.so) on every container feature it claims, with exact
answers.  FLAC streams come from tests/flac_writer.py (an explicit plan per frame: no encoder exists here to ask), WAV files from
`struct` / `wave`.  Expected PCM is float32(int / 2^(bps-1)); several channels are summed in float32 in channel order and divided by
their count - the decoder's documented mono mix - so every comparison is bit for bit."""
import ctypes as C
import io
import os
import struct
import wave

import numpy as np
import pytest

import flac_writer as fw
from flac_writer import Constant, Fixed, Frame, Lpc, Partition, Residual, Verbatim

WIS_E_FORMAT, WIS_E_NOMEM, WIS_E_CHECKSUM = -2, -3, -4


def decode(data):
    """(rc, pcm, sample_rate, md5_status) of wis_audio_decode on `data`; no resampling in the way"""
    from wis_hip import _lib
    lib = _lib.load()
    data = bytes(data)
    p, n, sr, md = C.POINTER(C.c_float)(), C.c_int64(-1), C.c_int(-1), C.c_int(-7)
    rc = lib.wis_audio_decode(data, len(data), C.byref(p), C.byref(n), C.byref(sr), C.byref(md))
    if rc != 0:
        assert not p, "an error left a buffer behind"
        return rc, None, None, md.value
    try:
        pcm = np.ctypeslib.as_array(p, shape=(max(n.value, 1),))[:n.value].copy()
    finally:
        lib.wis_audio_free(p)
    return rc, pcm, sr.value, md.value


def expected_pcm(samples, bps):
    a = np.asarray(samples, np.int64)
    if a.ndim == 1:
        a = a[None]
    f = a.astype(np.float32) * np.float32(2.0 ** -(bps - 1))          # (a power of two: the product is the exact quotient, rounded once)
    if a.shape[0] == 1:
        return f[0]
    acc = np.zeros(a.shape[1], np.float32)
    for c in range(a.shape[0]):
        acc = acc + f[c]
    return acc / np.float32(a.shape[0])


def check_flac(stream, samples, bps, sample_rate, md5_status=1):
    rc, pcm, sr, md = decode(stream)
    assert rc == 0, rc
    exp = expected_pcm(samples, bps)
    assert pcm.dtype == np.float32 and pcm.shape == exp.shape
    assert np.array_equal(pcm.view(np.uint32), exp.view(np.uint32)), int(np.flatnonzero(pcm != exp)[0])
    assert sr == sample_rate and md == md5_status


def lohi(bps):
    return -(1 << (bps - 1)), (1 << (bps - 1)) - 1


def rice(k, method=None, order=0):
    return Residual(method=(1 if k > 14 else 0) if method is None else method, order=order, partitions=[Partition(k=k)])


# ---------------------------------------------------------------------------------------------------------------------------------
# the writer itself, against the only outside evidence here: three clips from a real encoder
def _frame_starts(raw, first, numbers):
    """offsets of the frames whose coded frame number is in `numbers`, found with the WRITER's routines: a sync code whose header,
    rebuilt by fw.frame_header from the fields it announces, equals the stored bytes including the CRC-8"""
    found = {}
    want = {fw.utf8_number(k): k for k in numbers}
    pos = raw.find(b"\xff\xf8", first)
    while pos >= 0:
        for num, k in want.items():
            if raw[pos + 4:pos + 4 + len(num)] == num and k not in found:
                bs_code, sr_code, ch_code, bps_code = raw[pos + 2] >> 4, raw[pos + 2] & 15, raw[pos + 3] >> 4, (raw[pos + 3] >> 1) & 7
                at = pos + 4 + len(num)
                bs = fw.BLOCKSIZE_TABLE.get(bs_code) or (raw[at] + 1 if bs_code == 6 else int.from_bytes(raw[at:at + 2], "big") + 1)
                head = fw.frame_header(bs, bs_code, 16000, sr_code, ch_code, bps_code, False, k)
                if raw[pos:pos + len(head)] == head:
                    found[k] = (pos, bs)
        pos = raw.find(b"\xff\xf8", pos + 1)
    return found


@pytest.mark.parametrize("clip,n", [("3sec", 61440), ("10sec", 171008), ("30sec", 467968)])
def test_writer_routines_reproduce_the_golden_clips(golden_dir, clip, n):
    """STREAMINFO, the coded frame numbers, the header CRC-8 and the frame CRC-16 of the first and the last frame of each clip, rebuilt
    by the writer's own routines, equal the bytes a real encoder stored"""
    raw = open(os.path.join(golden_dir, "clips", clip + ".flac"), "rb").read()
    assert raw[:4] == b"fLaC" and raw[4] & 0x7f == fw.STREAMINFO and int.from_bytes(raw[5:8], "big") == 34
    si = raw[8:42]
    min_bs, max_bs = int.from_bytes(si[0:2], "big"), int.from_bytes(si[2:4], "big")
    min_fs, max_fs = int.from_bytes(si[4:7], "big"), int.from_bytes(si[7:10], "big")
    rc, pcm, sr, md = decode(raw)
    assert rc == 0 and md == 1 and pcm.shape[0] == n
    ints = np.round(pcm.astype(np.float64) * 32768.0).astype(np.int64)
    assert fw.streaminfo(min_bs, max_bs, min_fs, max_fs, 16000, 1, 16, n, fw.pcm_md5(ints[None], 16)) == si      # (the MD5 too)
    off, last = 4, 0
    while not last:
        last, off = raw[off] >> 7, off + 4 + int.from_bytes(raw[off + 1:off + 4], "big")
    assert min_bs == max_bs
    n_frames = -(-n // max_bs)
    found = _frame_starts(raw, off, [0, 1, n_frames - 1])
    assert sorted(found) == [0, 1, n_frames - 1] and found[0][0] == off
    assert found[0][1] == max_bs and found[n_frames - 1][1] == n - (n_frames - 1) * max_bs
    first = raw[found[0][0]:found[1][0]]
    tail = raw[found[n_frames - 1][0]:]
    for frame in (first, tail):
        assert fw.crc16(frame[:-2]) == int.from_bytes(frame[-2:], "big")


def test_writer_number_coding_lengths():
    for v, nbytes in ((0, 1), (127, 1), (128, 2), (2047, 2), (2048, 3), (65535, 3), (65536, 4), ((1 << 31) - 1, 6), ((1 << 36) - 1, 7)):
        b = fw.utf8_number(v)
        assert len(b) == nbytes
        if v < (1 << 20) and not 0xd800 <= v < 0xe000:
            assert b == chr(v).encode("utf-8")          # where UTF-8 proper is defined, it is UTF-8


# ---------------------------------------------------------------------------------------------------------------------------------
# FLAC: bit depths x subframe types
def _depth_signal(bps, rng):
    """two blocks of 192: the first hugs the top of the range and touches it, the second the bottom - so that a FIXED order-4 residual
    still fits its 32 bits at 32 bits per sample; at 24 bits and below the rest is drawn over the whole range"""
    lo, hi = lohi(bps)
    if bps <= 24:
        x = rng.integers(lo, hi + 1, 384)
    else:
        x = np.concatenate([hi - rng.integers(0, 4000, 192), lo + rng.integers(0, 4000, 192)])
    x[[5, 200] if bps <= 24 else [5]] = hi
    x[[100, 383] if bps <= 24 else [383]] = lo
    return x.astype(np.int64)


@pytest.mark.parametrize("kind", ["verbatim", "fixed0", "fixed1", "fixed2", "fixed3", "fixed4"])
@pytest.mark.parametrize("bps", [8, 12, 16, 20, 24, 32])
def test_flac_bit_depths(bps, kind):
    x = _depth_signal(bps, np.random.default_rng(bps))
    k = min(bps + 3, 30) if bps <= 24 else 14
    if (bps, kind) == (32, "fixed0"):          # the residual is the sample: -2^31 is the one value no residual may take
        x[x == lohi(32)[0]] += 1
        k = 30
    sf = Verbatim() if kind == "verbatim" else Fixed(int(kind[-1]), rice(k))
    check_flac(fw.write_stream(x, bps, 16000, [Frame(192, [sf]), Frame(192, [sf])]), x, bps, 16000)


def test_flac_bits_per_sample_from_streaminfo():
    """sample-size code 0 ("see STREAMINFO"): the only way to 4..32 bits outside the table, 15 and 17 here, and the narrowest, 4"""
    for bps in (4, 15, 17, 31):
        lo, hi = lohi(bps)
        x = np.random.default_rng(bps).integers(lo, hi + 1, 64)
        x[:2] = lo, hi
        fr = Frame(64, [Fixed(1, rice(min(bps + 1, 30)))], explicit_bps=False)
        check_flac(fw.write_stream(x, bps, 16000, [fr]), x, bps, 16000)


# ---------------------------------------------------------------------------------------------------------------------------------
# LPC
@pytest.mark.parametrize("shift", [0, 7, 14])
@pytest.mark.parametrize("precision", [2, 12, 15])
@pytest.mark.parametrize("order", [1, 2, 8, 12, 32])
def test_flac_lpc(order, precision, shift):
    """random coefficients over the whole range of the precision, the most negative one included; the amplitude is what keeps the
    residual inside 32 bits"""
    rng = np.random.default_rng(1000 * order + 10 * precision + shift)
    clo, chi = lohi(precision)
    coefs = rng.integers(clo, chi + 1, order)
    coefs[0] = clo
    amp = min(32767, ((1 << 29) << shift) // (order << (precision - 1)))
    x = rng.integers(-amp, amp + 1, 64 + order)
    x[order - 1] = -amp
    res = rice(min(30, max(0, int(amp).bit_length() + precision + int(order).bit_length() - shift)), method=1)
    frames = [Frame(64, [Lpc(coefs, precision, shift, res)]), Frame(order, [Lpc(coefs, precision, shift, res)])]   # the last block is all warm-up
    check_flac(fw.write_stream(x, 16, 16000, frames), x, 16, 16000)


def test_flac_lpc_wide_products():
    """a predictor sum far past 32 bits: 24-bit full-scale noise under 32 coefficients of 15 bits, and a full-scale 32-bit sine under
    a double-root predictor (coefficient x sample = 2^45)"""
    rng = np.random.default_rng(7)
    lo, hi = lohi(24)
    x = rng.integers(lo, hi + 1, 256)
    coefs = rng.integers(-(1 << 14), 1 << 14, 32)
    check_flac(fw.write_stream(x, 24, 48000, [Frame(256, [Lpc(coefs, 15, 14, rice(30))])]), x, 24, 48000)
    t = np.arange(512)
    s = np.round(((1 << 31) - 1) * np.sin(2 * np.pi * t / 97.0)).astype(np.int64)
    assert s.max() > 0.999 * (1 << 31) and s.min() < -0.999 * (1 << 31)
    check_flac(fw.write_stream(s, 32, 44100, [Frame(512, [Lpc([16383, -8192], 15, 13, rice(24))])]), s, 32, 44100)


# ---------------------------------------------------------------------------------------------------------------------------------
# Rice coding
@pytest.mark.parametrize("method", [0, 1])
@pytest.mark.parametrize("order", [0, 1, 4, 8])
def test_flac_rice_partition_orders(method, order):
    """256 samples: order 8 is the largest the block allows (one residual per partition); every partition its own parameter"""
    rng = np.random.default_rng(order)
    x = rng.integers(-3000, 3000, 256)
    parts = [Partition(k=int(k)) for k in rng.integers(4, 15, 1 << order)]
    check_flac(fw.write_stream(x, 16, 16000, [Frame(256, [Fixed(0, Residual(method, order, parts))])]), x, 16, 16000)


def test_flac_rice_first_partition_empty():
    """16 samples, FIXED order 1, partition order 4: one sample per partition and the warm-up takes the first partition's"""
    x = np.random.default_rng(3).integers(-300, 300, 16)
    check_flac(fw.write_stream(x, 16, 16000, [Frame(16, [Fixed(1, Residual(0, 4, [Partition(k=5)]))])]), x, 16, 16000)


@pytest.mark.parametrize("method,k", [(0, 0), (1, 0), (0, 14), (1, 30)])
def test_flac_rice_parameter_extremes(method, k):
    rng = np.random.default_rng(k + method)
    amp = 40 if k == 0 else (1 << (k + 1)) - 1          # (k = 30: the whole 32-bit residual range but its excluded minimum)
    x = rng.integers(-amp, amp + 1, 192)
    x[:2] = -amp, amp
    bps = 32 if k else 16
    check_flac(fw.write_stream(x, bps, 16000, [Frame(192, [Fixed(0, Residual(method, 0, [Partition(k=k)]))])]), x, bps, 16000)


@pytest.mark.parametrize("k", [0, 3])
def test_flac_rice_long_unary(k):
    """unary runs of 56, 57, 112 and 113 zeros (the 56-bit stride of the decoder's zero count and its boundary), each at all eight
    bit alignments"""
    vals = []
    for lead in range(8):
        vals += [1] * lead                               # (u = 2: with k = 0 three bits each, so the alignment walks)
        for q in (56, 57, 112, 113, 55, 111, 168, 169):
            u = (q << k) | (q & ((1 << k) - 1))
            vals.append(u >> 1 if u % 2 == 0 else -((u + 1) >> 1))
    vals += [0] * (-len(vals) % 16)
    x = np.array(vals, np.int64)
    check_flac(fw.write_stream(x, 16, 16000, [Frame(len(x), [Fixed(0, Residual(0, 0, [Partition(k=k)]))])]), x, 16, 16000)


@pytest.mark.parametrize("method", [0, 1])
@pytest.mark.parametrize("width", [0, 1, 16, 31])
def test_flac_escape_partitions(method, width):
    """a Rice partition, an escape partition of `width` raw bits, then Rice again"""
    rng = np.random.default_rng(width)
    x = rng.integers(-100, 100, 64)
    x[16:32] = rng.integers(-(1 << (width - 1)), 1 << (width - 1), 16) if width else 0
    if width:
        x[16:18] = -(1 << (width - 1)), (1 << (width - 1)) - 1
    parts = [Partition(k=4), Partition(escape_bits=width), Partition(k=4), Partition(k=6)]
    check_flac(fw.write_stream(x, 32, 16000, [Frame(64, [Fixed(0, Residual(method, 2, parts))])]), x, 32, 16000)


# ---------------------------------------------------------------------------------------------------------------------------------
# wasted bits
@pytest.mark.parametrize("kind", ["constant", "verbatim", "fixed"])
@pytest.mark.parametrize("wasted", [1, 5])
def test_flac_wasted_bits(wasted, kind):
    rng = np.random.default_rng(wasted)
    lo, hi = lohi(16 - wasted)
    x = rng.integers(lo, hi + 1, 192) << wasted
    x[:2] = lo << wasted, hi << wasted
    if kind == "constant":
        x[:] = lo << wasted
    sf = {"constant": Constant(wasted), "verbatim": Verbatim(wasted), "fixed": Fixed(2, rice(14), wasted)}[kind]
    check_flac(fw.write_stream(x, 16, 16000, [Frame(192, [sf])]), x, 16, 16000)


def test_flac_wasted_bits_leave_one_significant_bit():
    x = np.where(np.random.default_rng(1).integers(0, 2, 64) == 1, -32768, 0)
    for sf in (Verbatim(15), Fixed(0, rice(0), 15), Fixed(1, rice(0), 15)):
        check_flac(fw.write_stream(x, 16, 16000, [Frame(64, [sf])]), x, 16, 16000)
    check_flac(fw.write_stream(np.full(64, -128), 8, 16000, [Frame(64, [Constant(7)])]), np.full(64, -128), 8, 16000)


# ---------------------------------------------------------------------------------------------------------------------------------
# stereo
@pytest.mark.parametrize("assignment", [fw.INDEPENDENT, fw.LEFT_SIDE, fw.SIDE_RIGHT, fw.MID_SIDE])
@pytest.mark.parametrize("bps", [16, 24, 32])
def test_flac_stereo(bps, assignment):
    """left at the top of the range and right at the bottom (then swapped): the side channel uses all of its bps + 1 bits - 33 at 32
    bits per sample - with odd and even sides and mids of both signs; verbatim, FIXED and LPC subframes"""
    rng = np.random.default_rng(bps)
    lo, hi = lohi(bps)
    n = 64
    top, bot = hi - rng.integers(0, 2000, 3 * n), lo + rng.integers(0, 2000, 3 * n)
    left, right = np.concatenate([top, bot, rng.integers(-9, 9, n)]), np.concatenate([bot, top, rng.integers(-9, 9, n)])
    left[[0, 3 * n + 1]], right[[0, 3 * n + 1]] = (hi, lo), (lo, hi)
    left[1], right[1] = hi, lo + 1
    x = np.stack([left, right]).astype(np.int64)
    lpc = Lpc([3, -1], 3, 1, rice(14))
    plan = [(Verbatim(), Verbatim()), (Fixed(1, rice(14)), Fixed(2, rice(14))), (lpc, lpc)]
    frames = [Frame(n, list(p), assignment) for p in plan + plan] + [Frame(n, [Fixed(0, rice(3))], assignment)]
    check_flac(fw.write_stream(x, bps, 48000, frames), x, bps, 48000)


def test_flac_mid_side_odd_sides_and_negative_mids():
    left = np.array([-5, -4, 3, 0, -1, 7, -32768, 32767, -32768, -1], np.int64).repeat(2)[:16]
    right = np.array([-2, 3, -4, -1, 0, -8, 32767, -32768, -32767, -2, 5, 6, -7, 8, -9, 10], np.int64)
    x = np.stack([left, right])
    assert np.any((left - right) % 2 == 1) and np.any((left + right) < 0)
    check_flac(fw.write_stream(x, 16, 44100, [Frame(16, [Verbatim()], fw.MID_SIDE)]), x, 16, 44100)


@pytest.mark.parametrize("nch", [3, 6, 8])
def test_flac_independent_channels(nch):
    rng = np.random.default_rng(nch)
    lo, hi = lohi(24)
    x = rng.integers(lo, hi + 1, (nch, 192))
    x[:, 0], x[:, 1] = lo, hi
    subs = [[Verbatim(), Fixed(2, rice(26)), Constant(), Lpc([1], 2, 0, rice(26))][c % 4] for c in range(nch)]
    x[2::4] = x[2::4, :1]
    check_flac(fw.write_stream(x, 24, 48000, [Frame(192, subs)]), x, 24, 48000)


# ---------------------------------------------------------------------------------------------------------------------------------
# block sizes and coded numbers
@pytest.mark.parametrize("code", sorted(fw.BLOCKSIZE_TABLE))
def test_flac_blocksize_table_codes(code):
    bs = fw.BLOCKSIZE_TABLE[code]
    x = np.concatenate([np.full(bs, -1234), np.full(bs, 32767)])
    check_flac(fw.write_stream(x, 16, 16000, [Frame(bs, [Constant()], bs_code=code)] * 2), x, 16, 16000)


@pytest.mark.parametrize("code,bs", [(6, 16), (6, 17), (6, 255), (6, 256), (7, 257), (7, 4097), (7, 65535), (7, 192)])
def test_flac_blocksize_explicit_forms(code, bs):
    x = np.concatenate([np.full(bs, 77), np.full(bs, -32768), np.arange(min(bs, 9))])
    frames = [Frame(bs, [Constant()], bs_code=code)] * 2 + [Frame(min(bs, 9), [Verbatim()], bs_code=code)]
    check_flac(fw.write_stream(x, 16, 16000, frames), x, 16, 16000)


def test_flac_final_frame_of_one_sample():
    x = np.random.default_rng(5).integers(-32768, 32768, 33)
    check_flac(fw.write_stream(x, 16, 16000, [Frame(16, [Fixed(2, rice(14))])] * 2 + [Frame(1, [Verbatim()])]), x, 16, 16000)
    check_flac(fw.write_stream(x[:1], 16, 16000, [Frame(1, [Constant()])]), x[:1], 16, 16000)


@pytest.mark.parametrize("n_frames", [130, 2050])
def test_flac_frame_numbers_of_two_and_three_bytes(n_frames):
    x = np.random.default_rng(n_frames).integers(-128, 128, 16 * n_frames)
    stream, offs = fw.write_stream(x, 8, 16000, [Frame(16, [Verbatim()])] * n_frames, return_offsets=True)
    assert len(fw.utf8_number(n_frames - 1)) == (2 if n_frames < 2048 else 3) and stream[offs[-1] + 4] >= 0xc0
    check_flac(stream, x, 8, 16000)


def test_flac_variable_blocksize_stream_with_sample_numbers():
    sizes = [192, 33, 1000, 256, 1, 4096, 17]
    x = np.random.default_rng(9).integers(-32768, 32768, sum(sizes))
    stream, offs = fw.write_stream(x, 16, 16000, [Frame(s, [Fixed(1, rice(14))]) for s in sizes], variable=True, return_offsets=True)
    assert all(stream[o + 1] == 0xf9 for o in offs) and stream[offs[-1] + 4:offs[-1] + 7] == fw.utf8_number(sum(sizes[:-1]))
    check_flac(stream, x, 16, 16000)
    # sample numbers of four bytes: CONSTANT blocks of 65535
    y = np.repeat([5, -6, 7], 65535)
    stream, offs = fw.write_stream(y, 16, 16000, [Frame(65535, [Constant()])] * 3, variable=True, return_offsets=True)
    assert len(fw.utf8_number(2 * 65535)) == 4 and stream[offs[2] + 4] >> 3 == 0b11110
    check_flac(stream, y, 16, 16000)


# ---------------------------------------------------------------------------------------------------------------------------------
# streaming and metadata
def test_flac_unknown_total_grows_past_the_first_allocation():
    """total samples 0 (a streaming encoder) and more than 2^20 samples: the output buffer has to grow"""
    vals = np.random.default_rng(2).integers(-32768, 32768, 33)
    x = np.repeat(vals, 32768)
    assert x.shape[0] > (1 << 20)
    check_flac(fw.write_stream(x, 16, 16000, [Frame(32768, [Constant()])] * 33, total=0), x, 16, 16000)


def test_flac_every_metadata_block_type_and_zero_md5():
    x = np.random.default_rng(4).integers(-32768, 32768, 192)
    fr = [Frame(192, [Fixed(2, rice(14))])]
    blocks = [fw.padding_block(), fw.application_block(), fw.seektable_block(), fw.vorbis_comment_block(), fw.picture_block(), fw.padding_block(0)]
    check_flac(fw.write_stream(x, 16, 16000, fr, after=blocks), x, 16, 16000)
    for b in blocks:
        check_flac(fw.write_stream(x, 16, 16000, fr, after=[b]), x, 16, 16000)
    check_flac(fw.write_stream(x, 16, 16000, fr, before=[fw.padding_block()], after=[fw.vorbis_comment_block()]), x, 16, 16000)
    check_flac(fw.write_stream(x, 16, 16000, fr, md5="zero", after=blocks[:1]), x, 16, 16000, md5_status=-1)
    # a stream whose signature is present and wrong is refused, whatever else is right
    bad = bytearray(fw.write_stream(x, 16, 16000, fr))
    bad[8 + 18] ^= 1
    assert decode(bad)[0] == WIS_E_CHECKSUM


_RATES = {0: 12345, 12: 200000, 13: 11025, 14: 352800, **fw.SAMPLE_RATE_TABLE}


@pytest.mark.parametrize("code", sorted(_RATES))
def test_flac_sample_rate_codes(code):
    x = np.random.default_rng(code).integers(-32768, 32768, (2, 128))
    check_flac(fw.write_stream(x, 16, _RATES[code], [Frame(64, [Verbatim()], sr_code=code)] * 2), x, 16, _RATES[code])


# ---------------------------------------------------------------------------------------------------------------------------------
# FLAC: what is refused
def _plain_stream(bps=16, rate=16000, explicit_bps=True, sr_code=0, n=64):
    lo, hi = lohi(bps)
    x = np.random.default_rng(11).integers(lo // 2, hi // 2, n)
    return x, fw.write_stream(x, bps, rate, [Frame(n, [Verbatim()], explicit_bps=explicit_bps, sr_code=sr_code)])


def _set_streaminfo(stream, sample_rate=None, bps=None):
    s = bytearray(stream)
    v = int.from_bytes(s[18:26], "big")            # 20 bits rate, 3 channels - 1, 5 bps - 1, 36 total
    if sample_rate is not None:
        v = (v & ~(0xfffff << 44)) | (sample_rate << 44)
    if bps is not None:
        v = (v & ~(31 << 36)) | ((bps - 1) << 36)
    s[18:26] = v.to_bytes(8, "big")
    return bytes(s)


def test_flac_frame_header_must_agree_with_streaminfo():
    """a frame that names its own sample size or rate, and names another than STREAMINFO: refused.  (STREAMINFO 15 bits over frames of
    16 used to decode at twice the amplitude with a passing MD5, both widths being two bytes.)"""
    x, s = _plain_stream(16, 16000, explicit_bps=True, sr_code=5)
    check_flac(s, x, 16, 16000)
    for bps in (15, 12, 17, 24):
        assert decode(_set_streaminfo(s, bps=bps))[0] == WIS_E_FORMAT, bps
    for rate in (8000, 16001, 48000, 0):
        assert decode(_set_streaminfo(s, sample_rate=rate))[0] == WIS_E_FORMAT, rate
    # code 0 defers to STREAMINFO: the same edit is then a different, self-consistent stream (of other samples: the signature objects)
    x, s = _plain_stream(16, 16000, explicit_bps=False, sr_code=0)
    rc, pcm, sr, md = decode(_set_streaminfo(s, sample_rate=8000))
    assert rc == 0 and sr == 8000 and np.array_equal(pcm, expected_pcm(x, 16))
    assert decode(_set_streaminfo(s, bps=15))[0] in (WIS_E_FORMAT, WIS_E_CHECKSUM)


def test_flac_reserved_codes_are_refused():
    x = np.random.default_rng(12).integers(-9000, 9000, 64)
    s, (off,) = fw.write_stream(x, 16, 16000, [Frame(64, [Verbatim()])], return_offsets=True)
    assert s[off:off + 2] == b"\xff\xf8" and s[off + 2] >> 4 == 6          # header: 4 bytes, frame number, block size - 1, CRC-8

    def patched(byte, mask, value):
        f = bytearray(s[off:])
        f[byte] = (f[byte] & ~mask) | value
        f[6] = fw.crc8(f[:6])
        f[-2:] = fw.crc16(f[:-2]).to_bytes(2, "big")
        return s[:off] + bytes(f)

    assert decode(patched(2, 0, 0))[0] == 0
    assert decode(patched(2, 0xf0, 0x00))[0] == WIS_E_FORMAT           # block-size code 0
    assert decode(patched(2, 0x0f, 0x0f))[0] == WIS_E_FORMAT           # sample-rate code 15
    assert decode(patched(3, 0xf0, 0xb0))[0] == WIS_E_FORMAT           # channel assignment 11
    assert decode(patched(3, 0x0e, 0x06))[0] == WIS_E_FORMAT           # sample-size code 3
    assert decode(patched(3, 0x01, 0x01))[0] == WIS_E_FORMAT           # the reserved bit behind it
    assert decode(patched(7, 0x7e, 0x04))[0] == WIS_E_FORMAT           # subframe type 2
    assert decode(patched(7, 0x80, 0x80))[0] == WIS_E_FORMAT           # subframe padding bit


def test_flac_leading_and_trailing_bytes_are_refused(golden_dir):
    """pinned so that a change is deliberate: an ID3v2 tag ahead of `fLaC` and bytes behind the last frame are both format errors"""
    x, s = _plain_stream()
    raw = open(os.path.join(golden_dir, "clips", "3sec.flac"), "rb").read()
    id3 = b"ID3\x04\x00\x00" + bytes([0, 0, 0, 10]) + bytes(10)
    for stream in (s, raw):
        assert decode(stream)[0] == 0
        assert decode(id3 + stream)[0] == WIS_E_FORMAT
        for tail in (b"\0", b"\xff", b"\0\0", b"TAG" + bytes(125), b"\xff\xf8"):
            assert decode(stream + tail)[0] == WIS_E_FORMAT, tail


def test_flac_sample_out_of_its_range_is_refused():
    """a residual that carries a sample out of its subframe's range cannot come from an encoder: refused, not wrapped and not passed
    on (frames coded by the writer from samples one step outside 16 bits, both CRCs right, no signature to object)"""
    cases = ((32767, 32768, Fixed(1, rice(2))), (-32768, -32769, Fixed(0, rice(14, method=1))), (32767, 32768, Lpc([1], 2, 0, rice(2))),
             (32766, 32768, Fixed(2, rice(14), wasted=1)), (-32768, -32770, Verbatim(wasted=1)))
    for good, bad, sf in cases:
        for x in (np.full(16, good, np.int64), None):
            if x is None:
                if isinstance(sf, Verbatim):
                    continue                    # (nothing to predict: its width cannot say more than the range)
                x = np.full(16, bad, np.int64)
                x[:2] = good
            frame = fw.write_frame(Frame(16, [sf]), [x], 16, 16000, False, 0)
            stream, _ = fw.assemble([frame], [16], 16000, 1, 16, 16, bytes(16))
            if np.abs(x).max() < 32768 + (x.min() < 0):
                check_flac(stream, x, 16, 16000, md5_status=-1)
            else:
                assert decode(stream)[0] == WIS_E_FORMAT, (bad, type(sf).__name__)


# ---------------------------------------------------------------------------------------------------------------------------------
# WAV
PCM, FLOAT, EXTENSIBLE = 1, 3, 0xfffe
_GUID_TAIL = bytes.fromhex("000000001000800000aa00389b71")


def wav_bytes(tag, channels, rate, bits, data, fmt_len=16, sub_tag=None, before_data=(), data_len=None, fmt_first=True, with_fmt=True):
    fmt = struct.pack("<HHIIHH", tag, channels, rate, (rate * channels * bits // 8) & 0xffffffff, channels * bits // 8, bits)
    if fmt_len == 18:
        fmt += struct.pack("<H", 0)
    elif fmt_len == 40:
        fmt += struct.pack("<HHI", 22, bits, 0) + struct.pack("<H", sub_tag if sub_tag is not None else tag) + _GUID_TAIL
    assert len(fmt) == fmt_len

    def chunk(cid, body, length=None):
        return cid + struct.pack("<I", len(body) if length is None else length) + body + (b"\0" if len(body) & 1 else b"")

    chunks = [chunk(b"fmt ", fmt)] if with_fmt else []
    chunks += [chunk(c, b) for c, b in before_data]
    d = cid_data = chunk(b"data", data, data_len)
    if data_len is not None and len(data) & 1:
        d = cid_data[:-1]                                       # a streaming writer never came back to pad either
    chunks = chunks + [d] if fmt_first else [d] + chunks
    body = b"WAVE" + b"".join(chunks)
    return b"RIFF" + struct.pack("<I", len(body) if data_len is None else data_len) + body


def _wav_ints(bits, channels, n=50, seed=0):
    rng = np.random.default_rng(seed + bits + channels)
    lo, hi = lohi(bits)
    x = rng.integers(lo, hi + 1, (n, channels))
    x[0], x[1] = lo, hi
    return x.astype(np.int64)


def _pack_ints(x, bits):
    if bits == 8:
        return (x + 128).astype(np.uint8).tobytes()
    raw = x.astype("<i8").view(np.uint8).reshape(-1, 8)[:, :bits // 8]
    return np.ascontiguousarray(raw).tobytes()


def check_wav(blob, exp, rate):
    rc, pcm, sr, md = decode(blob)
    assert rc == 0 and sr == rate and md == -1
    assert pcm.shape == exp.shape and np.array_equal(pcm.view(np.uint32), exp.view(np.uint32))


@pytest.mark.parametrize("channels", [1, 2, 3, 6])
@pytest.mark.parametrize("bits", [8, 16, 24, 32])
def test_wav_pcm(bits, channels):
    x = _wav_ints(bits, channels)
    exp = expected_pcm(x.T, bits)
    assert channels > 1 or (exp[0] == -1.0 and exp[1] == np.float32(lohi(bits)[1]) * np.float32(2.0 ** -(bits - 1)))
    blob = wav_bytes(PCM, channels, 44100, bits, _pack_ints(x, bits))
    check_wav(blob, exp, 44100)
    if bits in (8, 16, 32):                                     # (what `wave` writes and scipy reads back)
        from scipy.io import wavfile
        buf = io.BytesIO()
        with wave.open(buf, "wb") as w:
            w.setnchannels(channels); w.setsampwidth(bits // 8); w.setframerate(44100)
            w.writeframes(_pack_ints(x, bits))
        check_wav(buf.getvalue(), exp, 44100)
        rate, back = wavfile.read(io.BytesIO(blob))
        assert rate == 44100 and np.array_equal(back.reshape(-1, channels).astype(np.int64) - (128 if bits == 8 else 0), x)


@pytest.mark.parametrize("channels", [1, 2, 3, 6])
def test_wav_float32(channels):
    rng = np.random.default_rng(channels)
    f = rng.uniform(-1, 1, (50, channels)).astype(np.float32)
    f[0], f[1] = -1.0, 1.0
    acc = np.zeros(50, np.float32)
    for c in range(channels):
        acc = acc + f[:, c]
    exp = f[:, 0] if channels == 1 else acc / np.float32(channels)
    check_wav(wav_bytes(FLOAT, channels, 48000, 32, f.astype("<f4").tobytes()), exp, 48000)
    check_wav(wav_bytes(EXTENSIBLE, channels, 48000, 32, f.astype("<f4").tobytes(), fmt_len=40, sub_tag=FLOAT), exp, 48000)


@pytest.mark.parametrize("fmt_len", [16, 18, 40])
def test_wav_fmt_chunk_sizes_and_extensible_pcm(fmt_len):
    for bits in (16, 24):
        x = _wav_ints(bits, 2)
        tag = EXTENSIBLE if fmt_len == 40 else PCM
        check_wav(wav_bytes(tag, 2, 22050, bits, _pack_ints(x, bits), fmt_len=fmt_len, sub_tag=PCM), expected_pcm(x.T, bits), 22050)


def test_wav_odd_chunks_before_data_use_the_pad_byte():
    x = _wav_ints(16, 1)
    extra = [(b"LIST", b"INFOISFT\x05\x00\x00\x00abcde"), (b"fact", struct.pack("<I", 50)), (b"junk", b"data\x04\x00\x00")]
    assert any(len(b) & 1 for _, b in extra)
    check_wav(wav_bytes(PCM, 1, 16000, 16, _pack_ints(x, 16), before_data=extra), expected_pcm(x.T, 16), 16000)


@pytest.mark.parametrize("data_len", [0xffffffff, 0])
def test_wav_streaming_lengths(data_len):
    """a writer that could not seek back leaves the lengths at 0xffffffff or at 0: the audio is what follows, to the end of the file"""
    for n in (50, 51):
        x = _wav_ints(24, 2, n)
        check_wav(wav_bytes(PCM, 2, 48000, 24, _pack_ints(x, 24), data_len=data_len), expected_pcm(x.T, 24), 48000)
    rc, pcm, sr, md = decode(wav_bytes(PCM, 2, 48000, 24, b""))                  # an honest empty file stays empty
    assert rc == 0 and pcm.shape == (0,) and sr == 48000


def test_wav_trailing_partial_frame_is_dropped():
    x = _wav_ints(24, 3)
    data = _pack_ints(x, 24)
    for cut in (1, 4, 8):
        check_wav(wav_bytes(PCM, 3, 16000, 24, data[:-cut]), expected_pcm(x[:-1].T, 24), 16000)


def test_wav_refused_formats():
    d = bytes(96)
    good = wav_bytes(PCM, 2, 16000, 16, d)
    assert decode(good)[0] == 0
    refused = {
        "float64": wav_bytes(FLOAT, 1, 16000, 64, d),
        "float64 extensible": wav_bytes(EXTENSIBLE, 1, 16000, 64, d, fmt_len=40, sub_tag=FLOAT),
        "a-law": wav_bytes(6, 1, 8000, 8, d),
        "mu-law": wav_bytes(7, 1, 8000, 8, d),
        "ms adpcm": wav_bytes(2, 1, 16000, 4, d),
        "ima adpcm": wav_bytes(0x11, 1, 16000, 4, d),
        "a-law extensible": wav_bytes(EXTENSIBLE, 1, 8000, 8, d, fmt_len=40, sub_tag=6),
        "12-bit": wav_bytes(PCM, 1, 16000, 12, d),
        "float16": wav_bytes(FLOAT, 1, 16000, 16, d),
        "zero channels": wav_bytes(PCM, 0, 16000, 16, d),
        "missing fmt": wav_bytes(PCM, 1, 16000, 16, d, with_fmt=False),
        "data before fmt": wav_bytes(PCM, 1, 16000, 16, d, fmt_first=False),
        "short fmt": good[:16] + struct.pack("<I", 14) + good[20:34] + good[36:],
        "RIFF of another kind": good[:8] + b"AVI " + good[12:],
        "RIFX": b"RIFX" + good[4:],
    }
    for name, blob in refused.items():
        assert decode(blob)[0] == WIS_E_FORMAT, name


# ---------------------------------------------------------------------------------------------------------------------------------
def test_sample_rate_zero_never_reaches_the_resampler():
    """load_audio on a container that says 0 Hz: WisError or ValueError, never ZeroDivisionError, never audio"""
    from wis_hip import _lib, audio
    x, s = _plain_stream(16, 0)
    blobs = [s, wav_bytes(PCM, 1, 0, 16, bytes(64)), wav_bytes(FLOAT, 2, 0, 32, bytes(64)), wav_bytes(PCM, 1, 0x80000000, 16, bytes(64))]
    for blob in blobs:
        with pytest.raises((_lib.WisError, ValueError)):
            audio.load_audio(blob)
        assert decode(blob)[0] == WIS_E_FORMAT
