"""A FLAC stream writer for the container-decoder tests (test infrastructure, like tests/ts_ref.py).

Written from the format's definition (RFC 9639), not from csrc/audio_io.c: it shares no table and no routine with the decoder, and its
CRCs are computed bit by bit.  It searches for nothing: the caller gives the samples `[channels][n]` and an explicit plan per frame
(block size and its code, sample-rate code, channel assignment, one subframe description per channel), because coverage is the point,
not compression.  A correct decoder reproduces the samples bit for bit: residuals come from the exact integer predictor.

    stream = write_stream(samples, bps=16, sample_rate=16000, frames=[Frame(blocksize=192, subframes=[Fixed(2)]), ...])

Python ints / int64 arrays throughout (33-bit side channels and 2^53 predictor sums do not fit int32).
"""
import hashlib

import numpy as np

# ---------------------------------------------------------------------------------------------------------------------------------
# CRCs, bit by bit (MSB first, zero initial value, no reflection, no final xor)


def _crc(data, poly, width):
    top, mask, c = 1 << (width - 1), (1 << width) - 1, 0
    for byte in bytes(data):
        c ^= byte << (width - 8)
        for _ in range(8):
            c = ((c << 1) ^ poly) & mask if c & top else (c << 1) & mask
    return c


def crc8(data):
    """x^8 + x^2 + x + 1 over the frame header"""
    return _crc(data, 0x07, 8)


def crc16(data):
    """x^16 + x^15 + x^2 + 1 over the whole frame"""
    return _crc(data, 0x8005, 16)


# ---------------------------------------------------------------------------------------------------------------------------------
class BitWriter:
    """MSB-first bit accumulator"""

    def __init__(self):
        self.out, self.acc, self.nacc = bytearray(), 0, 0

    def bits(self, value, n):
        if n == 0:
            return
        value = int(value)
        assert 0 <= value < (1 << n), (value, n)
        self.acc = (self.acc << n) | value
        self.nacc += n
        if self.nacc >= 64:
            k = self.nacc & ~7
            rest = self.nacc - k
            self.out += (self.acc >> rest).to_bytes(k // 8, "big")
            self.acc &= (1 << rest) - 1
            self.nacc = rest

    def sbits(self, value, n):
        """two's complement in n bits"""
        value = int(value)
        assert -(1 << (n - 1)) <= value < (1 << (n - 1)) if n else value == 0, (value, n)
        self.bits(value & ((1 << n) - 1), n)

    def unary(self, q):
        """q zero bits, then a one"""
        while q >= 32:
            self.bits(0, 32)
            q -= 32
        self.bits(1, q + 1)

    def raw(self, data):
        assert self.nacc % 8 == 0
        for byte in bytes(data):
            self.bits(byte, 8)

    def align(self):
        if self.nacc % 8:
            self.bits(0, 8 - self.nacc % 8)

    def getvalue(self):
        assert self.nacc % 8 == 0
        return bytes(self.out) + (self.acc.to_bytes(self.nacc // 8, "big") if self.nacc else b"")


def utf8_number(v):
    """the frame header's coded number: UTF-8's scheme extended to 36 bits (1 to 7 bytes)"""
    v = int(v)
    assert 0 <= v < (1 << 36)
    if v < 0x80:
        return bytes([v])
    n = 2
    while v >= (1 << (5 * n + 1)):          # n bytes carry (7 - n) + 6 (n - 1) = 5 n + 1 bits
        n += 1
    lead = ((0xff << (8 - n)) & 0xff) | (v >> (6 * (n - 1)))
    return bytes([lead] + [0x80 | ((v >> (6 * i)) & 0x3f) for i in range(n - 2, -1, -1)])


# ---------------------------------------------------------------------------------------------------------------------------------
# metadata
STREAMINFO, PADDING, APPLICATION, SEEKTABLE, VORBIS_COMMENT, CUESHEET, PICTURE = range(7)


def streaminfo(min_bs, max_bs, min_fs, max_fs, sample_rate, channels, bps, total, md5):
    w = BitWriter()
    w.bits(min_bs, 16); w.bits(max_bs, 16); w.bits(min_fs, 24); w.bits(max_fs, 24)
    w.bits(sample_rate, 20); w.bits(channels - 1, 3); w.bits(bps - 1, 5); w.bits(total, 36)
    w.raw(md5)
    body = w.getvalue()
    assert len(body) == 34 and len(md5) == 16
    return body


def metadata_block(btype, body, last=False):
    assert len(body) < (1 << 24)
    return bytes([(0x80 if last else 0) | btype]) + len(body).to_bytes(3, "big") + bytes(body)


def padding_block(n=17):
    return PADDING, bytes(n)


def application_block():
    return APPLICATION, b"wisT" + bytes(range(1, 12))


def seektable_block(points=((0, 0, 16), (1 << 40, 7, 0))):
    """seek points (sample number, byte offset, samples in the frame); the second default is not a real point, any reader may ignore it"""
    return SEEKTABLE, b"".join(int(a).to_bytes(8, "big") + int(b).to_bytes(8, "big") + int(c).to_bytes(2, "big") for a, b, c in points)


def vorbis_comment_block(vendor=b"flac_writer.py", comments=(b"TITLE=fLaC \xff\xf8 inside a tag",)):
    body = len(vendor).to_bytes(4, "little") + vendor + len(comments).to_bytes(4, "little")
    return VORBIS_COMMENT, body + b"".join(len(c).to_bytes(4, "little") + c for c in comments)


def picture_block(data=b"\xff\xf8\xc9\x18\x00 not a frame"):
    mime, desc = b"image/png", b""
    body = (3).to_bytes(4, "big") + len(mime).to_bytes(4, "big") + mime + len(desc).to_bytes(4, "big") + desc
    body += b"".join(int(v).to_bytes(4, "big") for v in (1, 1, 24, 0)) + len(data).to_bytes(4, "big") + data
    return PICTURE, body


def pcm_md5(samples, bps):
    """STREAMINFO's signature: the interleaved samples, each little-endian in the whole bytes its width needs"""
    a = np.asarray(samples, np.int64)
    nbytes = (bps + 7) // 8
    inter = np.ascontiguousarray(a.T).astype("<i8")
    raw = inter.view(np.uint8).reshape(-1, 8)[:, :nbytes]
    return hashlib.md5(np.ascontiguousarray(raw).tobytes()).digest()


# ---------------------------------------------------------------------------------------------------------------------------------
# residual coding
class Partition:
    """one residual partition: Rice parameter `k`, or an escape partition of `escape_bits` raw bits per residual"""

    def __init__(self, k=None, escape_bits=None):
        assert (k is None) != (escape_bits is None)
        self.k, self.escape_bits = k, escape_bits


class Residual:
    """method 0 (4-bit parameters, escape 15) or 1 (5-bit, escape 31); 2^order partitions; one Partition each (one given = all alike)"""

    def __init__(self, method=0, order=0, partitions=None):
        self.method, self.order = method, order
        parts = partitions if partitions is not None else [Partition(k=min(14, 10))]
        self.partitions = list(parts) * (1 << order) if len(parts) == 1 else list(parts)
        assert len(self.partitions) == 1 << order


def write_residual(w, res, values, blocksize, pred_order):
    pbits, esc = (5, 31) if res.method else (4, 15)
    w.bits(res.method, 2)
    w.bits(res.order, 4)
    assert blocksize % (1 << res.order) == 0 and (blocksize >> res.order) >= pred_order
    per, i = blocksize >> res.order, 0
    for p, part in enumerate(res.partitions):
        cnt = per - pred_order if p == 0 else per
        vals = values[i:i + cnt]
        i += cnt
        if part.escape_bits is not None:
            w.bits(esc, pbits)
            w.bits(part.escape_bits, 5)
            for v in vals:
                w.sbits(v, part.escape_bits)
        else:
            assert 0 <= part.k < esc
            w.bits(part.k, pbits)
            for v in vals:
                v = int(v)
                assert -(1 << 31) < v < (1 << 31)              # a residual fits 32 bits, its most negative value excluded
                u = 2 * v if v >= 0 else -2 * v - 1            # zig-zag folding
                w.unary(u >> part.k)
                w.bits(u & ((1 << part.k) - 1), part.k)
    assert i == len(values)


# ---------------------------------------------------------------------------------------------------------------------------------
# subframes.  `wasted`: the k low zero bits every sample of the subframe shares are dropped before coding.
class Constant:
    def __init__(self, wasted=0):
        self.wasted = wasted


class Verbatim:
    def __init__(self, wasted=0):
        self.wasted = wasted


class Fixed:
    def __init__(self, order, residual=None, wasted=0):
        assert 0 <= order <= 4
        self.order, self.residual, self.wasted = order, residual or Residual(), wasted


class Lpc:
    """prediction = (sum_j coefs[j] * s[i - 1 - j]) >> shift, arithmetic shift, exact integers"""

    def __init__(self, coefs, precision, shift, residual=None, wasted=0):
        assert 1 <= len(coefs) <= 32 and 1 <= precision <= 15 and 0 <= shift <= 15
        assert all(-(1 << (precision - 1)) <= c < (1 << (precision - 1)) for c in coefs)
        self.coefs, self.precision, self.shift, self.residual, self.wasted = [int(c) for c in coefs], precision, shift, residual or Residual(), wasted


_FIXED = {0: [], 1: [1], 2: [2, -1], 3: [3, -3, 1], 4: [4, -6, 4, -1]}


def predict_residual(s, coefs, shift):
    """s[i] - ((sum_j coefs[j] s[i-1-j]) >> shift) for i >= order, in Python integers (no width to overflow)"""
    order = len(coefs)
    s = [int(v) for v in s]
    return [s[i] - (sum(c * s[i - 1 - j] for j, c in enumerate(coefs)) >> shift) for i in range(order, len(s))]


def write_subframe(w, sf, samples, bps):
    s = [int(v) for v in samples]
    n = len(s)
    k = sf.wasted
    if k:
        assert all(v % (1 << k) == 0 for v in s), "wasted bits must be zero in every sample"
        s = [v >> k for v in s]
        bps -= k
        assert bps >= 1
    if isinstance(sf, Constant):
        code = 0
    elif isinstance(sf, Verbatim):
        code = 1
    elif isinstance(sf, Fixed):
        code = 8 | sf.order
    else:
        code = 32 | (len(sf.coefs) - 1)
    w.bits(0, 1)
    w.bits(code, 6)
    if k:
        w.bits(1, 1)
        w.unary(k - 1)
    else:
        w.bits(0, 1)
    if isinstance(sf, Constant):
        assert all(v == s[0] for v in s)
        w.sbits(s[0], bps)
    elif isinstance(sf, Verbatim):
        for v in s:
            w.sbits(v, bps)
    elif isinstance(sf, Fixed):
        for v in s[:sf.order]:
            w.sbits(v, bps)
        write_residual(w, sf.residual, predict_residual(s, _FIXED[sf.order], 0), n, sf.order)
    else:
        order = len(sf.coefs)
        for v in s[:order]:
            w.sbits(v, bps)
        w.bits(sf.precision - 1, 4)
        w.sbits(sf.shift, 5)
        for c in sf.coefs:
            w.sbits(c, sf.precision)
        write_residual(w, sf.residual, predict_residual(s, sf.coefs, sf.shift), n, order)


# ---------------------------------------------------------------------------------------------------------------------------------
# frames
INDEPENDENT, LEFT_SIDE, SIDE_RIGHT, MID_SIDE = "independent", "left_side", "side_right", "mid_side"
BLOCKSIZE_TABLE = {1: 192, 2: 576, 3: 1152, 4: 2304, 5: 4608, 8: 256, 9: 512, 10: 1024, 11: 2048, 12: 4096, 13: 8192, 14: 16384, 15: 32768}
SAMPLE_RATE_TABLE = {1: 88200, 2: 176400, 3: 192000, 4: 8000, 5: 16000, 6: 22050, 7: 24000, 8: 32000, 9: 44100, 10: 48000, 11: 96000}
BPS_TABLE = {8: 1, 12: 2, 16: 4, 20: 5, 24: 6, 32: 7}


class Frame:
    """blocksize: samples per channel.  bs_code: None = the table code if the size has one, else the 8-bit form if it fits, else the
    16-bit form; or 6 / 7 / a table code to force one.  sr_code: 0 = "see STREAMINFO", a table code, or 12 (kHz, 8 bits) / 13 (Hz,
    16 bits) / 14 (tens of Hz, 16 bits).  explicit_bps: write the sample-size code (else 0 = "see STREAMINFO").  subframes: one per
    channel (one given = all alike).  number: the coded frame / sample number (None = the running one)."""

    def __init__(self, blocksize, subframes, assignment=INDEPENDENT, bs_code=None, sr_code=0, explicit_bps=True, number=None):
        self.blocksize, self.subframes, self.assignment = blocksize, list(subframes), assignment
        self.bs_code, self.sr_code, self.explicit_bps, self.number = bs_code, sr_code, explicit_bps, number


def frame_header(blocksize, bs_code, sample_rate, sr_code, channel_code, bps_code, variable, number):
    """the frame header including its CRC-8"""
    w = BitWriter()
    w.bits(0b11111111111110, 14)
    w.bits(0, 1)
    w.bits(1 if variable else 0, 1)
    if bs_code is None:
        inv = {v: k for k, v in BLOCKSIZE_TABLE.items()}
        bs_code = inv.get(blocksize, 6 if blocksize <= 256 else 7)
    w.bits(bs_code, 4)
    w.bits(sr_code, 4)
    w.bits(channel_code, 4)
    w.bits(bps_code, 3)
    w.bits(0, 1)
    w.raw(utf8_number(number))
    if bs_code == 6:
        w.bits(blocksize - 1, 8)
    elif bs_code == 7:
        w.bits(blocksize - 1, 16)
    else:
        assert BLOCKSIZE_TABLE[bs_code] == blocksize
    if sr_code == 12:
        assert sample_rate % 1000 == 0
        w.bits(sample_rate // 1000, 8)
    elif sr_code == 13:
        w.bits(sample_rate, 16)
    elif sr_code == 14:
        assert sample_rate % 10 == 0
        w.bits(sample_rate // 10, 16)
    elif sr_code:
        assert SAMPLE_RATE_TABLE[sr_code] == sample_rate
    head = w.getvalue()
    return head + bytes([crc8(head)])


def write_frame(fr, chans, bps, sample_rate, variable, number):
    """chans: [channels][blocksize] integers of this frame"""
    nch = len(chans)
    subs = fr.subframes * nch if len(fr.subframes) == 1 else fr.subframes
    assert len(subs) == nch
    widths = [bps] * nch
    if fr.assignment == INDEPENDENT:
        code = nch - 1
    else:
        assert nch == 2
        left, right = [int(v) for v in chans[0]], [int(v) for v in chans[1]]
        side = [a - b for a, b in zip(left, right)]
        if fr.assignment == LEFT_SIDE:
            code, chans, widths = 8, [left, side], [bps, bps + 1]
        elif fr.assignment == SIDE_RIGHT:
            code, chans, widths = 9, [side, right], [bps + 1, bps]
        else:
            code, chans, widths = 10, [[(a + b) >> 1 for a, b in zip(left, right)], side], [bps, bps + 1]
    bps_code = BPS_TABLE[bps] if fr.explicit_bps else 0
    w = BitWriter()
    w.raw(frame_header(fr.blocksize, fr.bs_code, sample_rate, fr.sr_code, code, bps_code, variable, number))
    for sf, ch, width in zip(subs, chans, widths):
        assert len(ch) == fr.blocksize
        write_subframe(w, sf, ch, width)
    w.align()
    body = w.getvalue()
    return body + crc16(body).to_bytes(2, "big")


def write_stream(samples, bps, sample_rate, frames, variable=False, md5="real", total="real", before=(), after=(), return_offsets=False):
    """samples: [channels][n]; frames: the plan, whose block sizes add up to n.  md5: "real" or "zero"; total: "real" or 0 (unknown).
    before / after: (type, body) metadata blocks ahead of / behind STREAMINFO.  Frame numbers run from 0 (sample numbers when
    `variable`) unless a Frame names its own."""
    a = np.asarray(samples, np.int64)
    if a.ndim == 1:
        a = a[None]
    nch, n = a.shape
    assert sum(f.blocksize for f in frames) == n and 1 <= nch <= 8
    lo, hi = -(1 << (bps - 1)), (1 << (bps - 1)) - 1
    assert all(lo <= int(v) <= hi for v in (a.min(), a.max()))
    body, pos = [], 0
    for i, fr in enumerate(frames):
        number = fr.number if fr.number is not None else (pos if variable else i)
        body.append(write_frame(fr, [a[c, pos:pos + fr.blocksize] for c in range(nch)], bps, sample_rate, variable, number))
        pos += fr.blocksize
    digest = pcm_md5(a, bps) if md5 == "real" else bytes(16)
    out, offsets = assemble(body, [f.blocksize for f in frames], sample_rate, nch, bps, n if total == "real" else 0, digest, before, after, variable)
    return (out, offsets) if return_offsets else out


def assemble(frame_bytes, sizes, sample_rate, channels, bps, total, digest, before=(), after=(), variable=False):
    """"fLaC", the metadata blocks and already coded frames -> (stream, offset of every frame); also the way to wrap a frame that
    write_stream would not plan (write_frame on samples outside their range, a hand-made header)"""
    lens = [len(b) for b in frame_bytes]
    if variable:
        min_bs, max_bs = min(sizes), max(sizes)
    else:
        min_bs = max_bs = sizes[0]
        assert all(s == sizes[0] for s in sizes[:-1]) and sizes[-1] <= sizes[0], "fixed blocking: only the last frame may be shorter"
    si = streaminfo(max(min_bs, 16), max(max_bs, 16), min(lens), max(lens), sample_rate, channels, bps, total, digest)
    blocks = list(before) + [(STREAMINFO, si)] + list(after)
    out = b"fLaC" + b"".join(metadata_block(t, b, last=(i == len(blocks) - 1)) for i, (t, b) in enumerate(blocks))
    offsets = []
    for b in frame_bytes:
        offsets.append(len(out))
        out += b
    return out, offsets
