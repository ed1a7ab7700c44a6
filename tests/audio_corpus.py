"""The hostile-input corpus of the upload decoder (csrc/audio_io.c): seven seed files and a fixed list of damaged copies of each.

    corpus = build()                       # tests/test_audio_hostile_cpu.py
    python tests/audio_corpus.py OUTDIR    # one file per case, for tools/audio_io_harness.c (CPU only, under sanitizers)

Everything comes from constant seeds, so the corpus never changes: a case that is refused today and accepted tomorrow is a change of
the decoder.  FLAC seeds: the real-encoder clip 3sec.flac and three streams from tests/flac_writer.py; WAV seeds from `struct`.
Per seed: truncation at every length up to 300 bytes and at 64 drawn lengths beyond, every single-bit flip in the first 100 bytes, 500
overwrites of 1-4 random bytes anywhere; then cases aimed at single header fields."""
import os
import struct
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import flac_writer as fw  # noqa: E402
from flac_writer import Constant, Fixed, Frame, Lpc, Partition, Residual  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SEED = 20260719


class Seed:
    def __init__(self, name, kind, data, samples=None, bps=None, first_frame=None):
        self.name, self.kind, self.data, self.samples, self.bps, self.first_frame = name, kind, bytes(data), samples, bps, first_frame


class Case:
    """expect_refused: a case that must not decode, whatever else holds"""

    def __init__(self, seed, label, data, expect_refused=False):
        self.seed, self.label, self.data, self.expect_refused = seed, label, bytes(data), expect_refused


def _rice(k, method=None):
    return Residual(method=(1 if k > 14 else 0) if method is None else method, order=0, partitions=[Partition(k=k)])


def _wav(tag, channels, rate, bits, data, extensible_sub=None, data_len=None):
    fmt = struct.pack("<HHIIHH", tag, channels, rate, rate * channels * bits // 8, channels * bits // 8, bits)
    if extensible_sub is not None:
        fmt += struct.pack("<HHIH", 22, bits, 3, extensible_sub) + bytes.fromhex("000000001000800000aa00389b71")
    body = b"WAVE" + b"fmt " + struct.pack("<I", len(fmt)) + fmt
    body += b"LIST" + struct.pack("<I", 13) + b"INFOISFTa\0\0\0x" + b"\0"
    body += b"data" + struct.pack("<I", len(data) if data_len is None else data_len) + data
    return b"RIFF" + struct.pack("<I", len(body) if data_len is None else data_len) + body


def seeds():
    rng = np.random.default_rng(SEED)
    out = []
    raw = open(os.path.join(GOLDEN, "clips", "3sec.flac"), "rb").read()
    off, last = 4, 0
    while not last:
        last, off = raw[off] >> 7, off + 4 + int.from_bytes(raw[off + 1:off + 4], "big")
    out.append(Seed("clip3sec", "flac", raw, first_frame=off))

    # 24-bit stereo, mid/side, LPC: a correlated pair so that the residuals are small and the file short
    t = np.arange(4096)
    left = np.round(6.0e6 * np.sin(2 * np.pi * t / 61.0) + rng.normal(0, 300, 4096)).astype(np.int64)
    right = np.round(5.5e6 * np.sin(2 * np.pi * t / 61.0 + 0.2) + rng.normal(0, 300, 4096)).astype(np.int64)
    x = np.stack([left, right])
    lpc = Lpc([16220, -8192], 15, 13, _rice(17))
    s, offs = fw.write_stream(x, 24, 48000, [Frame(1024, [lpc, lpc], fw.MID_SIDE, sr_code=10)] * 4, after=[fw.padding_block(40)], return_offsets=True)
    out.append(Seed("midside24", "flac", s, x, 24, offs[0]))

    # escape partitions (17 bits and 0 bits) between Rice partitions, both methods, 16-bit mono
    y = rng.integers(-2000, 2000, 1024).astype(np.int64)
    y[256:320] = rng.integers(-32768, 32768, 64)
    parts = [Partition(k=11), Partition(escape_bits=17), Partition(k=12), Partition(escape_bits=0)] * 4
    y[192:256] = y[191]
    y[192 + 256:256 + 256] = y[191 + 256]
    y[192 + 512:256 + 512] = y[191 + 512]
    y[192 + 768:256 + 768] = y[191 + 768]
    frames = [Frame(256, [Fixed(1, Residual(m, 2, parts[:4]))], sr_code=5) for m in (0, 1, 0, 1)]
    s, offs = fw.write_stream(y, 16, 16000, frames, return_offsets=True)
    out.append(Seed("escape16", "flac", s, y, 16, offs[0]))

    # unknown total, more samples than the decoder's first allocation
    vals = rng.integers(-32768, 32768, 33).astype(np.int64)
    z = np.repeat(vals, 32768)
    s, offs = fw.write_stream(z, 16, 16000, [Frame(32768, [Constant()], sr_code=5)] * 33, total=0, return_offsets=True)
    out.append(Seed("total0", "flac", s, z, 16, offs[0]))

    pcm = rng.integers(-32768, 32768, 2 * 2000).astype("<i2").tobytes()
    out.append(Seed("wav16stereo", "wav", _wav(1, 2, 44100, 16, pcm)))
    flt = rng.uniform(-1, 1, 3 * 700).astype("<f4").tobytes()
    out.append(Seed("wavfloat_ext", "wav", _wav(0xfffe, 3, 48000, 32, flt, extensible_sub=3)))
    out.append(Seed("wavstreaming", "wav", _wav(1, 1, 16000, 24, bytes(rng.integers(0, 256, 3 * 1000, dtype=np.uint8)), data_len=0xffffffff)))
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
def _generic(seed, rng):
    d = seed.data
    n = len(d)
    cases = [Case(seed.name, f"trunc{k:06d}", d[:k]) for k in range(0, min(n, 301))]
    if n > 301:
        for k in sorted(int(v) for v in rng.choice(np.arange(301, n), size=min(64, n - 301), replace=False)):
            cases.append(Case(seed.name, f"trunc{k:06d}", d[:k]))
    for bit in range(8 * min(n, 100)):
        m = bytearray(d)
        m[bit >> 3] ^= 0x80 >> (bit & 7)
        cases.append(Case(seed.name, f"flip{bit:04d}", m))
    for i in range(500):
        m = bytearray(d)
        k = int(rng.integers(1, 5))
        at = int(rng.integers(0, n - k + 1))
        m[at:at + k] = bytes(int(v) for v in rng.integers(0, 256, k))
        cases.append(Case(seed.name, f"over{i:03d}_{at:06d}", m))
    return cases


def _streaminfo_field(data, shift, width, value):
    """STREAMINFO's last 64 header bits before the MD5: 20 rate, 3 channels - 1, 5 bps - 1, 36 total (STREAMINFO is the first block)"""
    m = bytearray(data)
    v = int.from_bytes(m[18:26], "big")
    v = (v & ~(((1 << width) - 1) << shift)) | (value << shift)
    m[18:26] = v.to_bytes(8, "big")
    return m


def _header_len(f):
    """bytes of a frame header before its CRC-8, as the codes IN the header say"""
    lead, n = f[4], 1
    if lead & 0x80:
        n = 0
        while lead & (0x80 >> n):
            n += 1
    bs_code, sr_code = f[2] >> 4, f[2] & 15
    return 4 + max(n, 1) + (1 if bs_code == 6 else 2 if bs_code == 7 else 0) + (1 if sr_code == 12 else 2 if sr_code in (13, 14) else 0)


def _flac_fields(seed):
    d, ff = seed.data, seed.first_frame
    total = int.from_bytes(d[18:26], "big") & ((1 << 36) - 1)
    true_total = total or (len(seed.samples[-1]) if seed.samples is not None and np.ndim(seed.samples) > 1 else len(seed.samples))
    cases = [Case(seed.name, "total_2p36m1", _streaminfo_field(d, 0, 36, (1 << 36) - 1), expect_refused=True),
             Case(seed.name, "total_plus1", _streaminfo_field(d, 0, 36, true_total + 1), expect_refused=True),
             Case(seed.name, "total_minus1", _streaminfo_field(d, 0, 36, true_total - 1), expect_refused=True)]
    cases += [Case(seed.name, f"si_bps{v + 1:02d}", _streaminfo_field(d, 36, 5, v)) for v in range(32)]
    cases += [Case(seed.name, f"si_ch{v + 1}", _streaminfo_field(d, 41, 3, v)) for v in range(8)]
    for field, at in (("minbs", 8), ("maxbs", 10)):
        for v in (0, 15):
            m = bytearray(d)
            m[at:at + 2] = v.to_bytes(2, "big")
            cases.append(Case(seed.name, f"si_{field}{v}", m, expect_refused=(field == "maxbs")))
    # every code of the first frame header, CRC-8 put right (where the codes now say it is) so that the subframes are reached
    for name, byte, shift, count in (("bs", 2, 4, 16), ("sr", 2, 0, 16), ("ch", 3, 4, 16), ("bps", 3, 1, 8)):
        for v in range(count):
            m = bytearray(d)
            m[ff + byte] = (m[ff + byte] & ~((count - 1) << shift)) | (v << shift)
            h = _header_len(m[ff:ff + 16])
            m[ff + h] = fw.crc8(m[ff:ff + h])
            cases.append(Case(seed.name, f"hdr_{name}{v:02d}", m))
    return cases


def _full_scale_predictor_cases():
    """frames whose warm-up samples and residuals are all at full scale, both CRCs right, so that the predictor runs to the end of the
    block: LPC with 32 coefficients at either end of 15 bits, FIXED order 4 on alternating extremes.  No encoder writes these (the
    samples leave their range at once); write_frame codes them all the same.  Built at 32, 24 and 16 bits."""
    cases = []
    for bps in (32, 24, 16):
        hi, lo = (1 << (bps - 1)) - 1, -(1 << (bps - 1))
        n = 512
        for name, sf, warm, resid in (
                ("lpc_pos", Lpc([16383] * 32, 15, 0, Residual(1, 0, [Partition(escape_bits=31)])), [hi] * 32, (1 << 30) - 1),
                ("lpc_alt", Lpc([-16384, 16383] * 16, 15, 0, Residual(1, 0, [Partition(k=30)])), [hi, lo] * 16, -(1 << 31) + 1),
                ("lpc_shift14", Lpc([16383] * 32, 15, 14, Residual(1, 0, [Partition(k=30)])), [lo] * 32, -(1 << 31) + 1),
                ("fixed4", Fixed(4, Residual(1, 0, [Partition(k=30)])), [hi, lo, hi, lo], (1 << 31) - 1),
                ("fixed2", Fixed(2, Residual(0, 0, [Partition(escape_bits=31)])), [lo, hi], -(1 << 30))):
            order = len(warm)
            coefs = sf.coefs if isinstance(sf, Lpc) else fw._FIXED[sf.order]
            shift = sf.shift if isinstance(sf, Lpc) else 0
            x = list(warm)
            for i in range(order, n):                 # the samples that give exactly this residual everywhere (Python integers: no width)
                x.append(resid + (sum(c * x[i - 1 - j] for j, c in enumerate(coefs)) >> shift))
            frame = fw.write_frame(Frame(n, [sf], explicit_bps=True), [x], bps, 16000, False, 0)
            for md5 in (bytes(16), bytes(range(1, 17))):
                stream, _ = fw.assemble([frame], [n], 16000, 1, bps, n, md5)
                cases.append(Case("predictor", f"{name}_{bps}_{'nomd5' if md5[0] == 0 else 'md5'}", stream, expect_refused=True))
    return cases


def _wav_fields(seed):
    d = seed.data
    fmt_at = d.index(b"fmt ") + 8
    cases = []
    for name, at, size in (("tag", 0, 2), ("channels", 2, 2), ("rate", 4, 4), ("byterate", 8, 4), ("align", 12, 2), ("bits", 14, 2)):
        for v in (0, 0xffff, 0x7fffffff):
            m = bytearray(d)
            m[fmt_at + at:fmt_at + at + size] = (v & ((1 << (8 * size)) - 1)).to_bytes(size, "little")
            cases.append(Case(seed.name, f"fmt_{name}_{v:x}", m))
    for cid in (b"RIFF", b"fmt ", b"LIST", b"data"):
        at = d.index(cid) + 4
        for v in (len(d), len(d) - at - 3, 0x7fffffff, 0x80000000, 0xfffffffe, 0xffffffff, 1, 0):
            m = bytearray(d)
            m[at:at + 4] = v.to_bytes(4, "little")
            cases.append(Case(seed.name, f"len_{cid.decode().strip()}_{v:x}", m))
    return cases


def build():
    """-> (seeds, cases): the whole corpus, the same on every call"""
    ss = seeds()
    cases = []
    for i, s in enumerate(ss):
        cases += _generic(s, np.random.default_rng([SEED, i]))
        cases += _flac_fields(s) if s.kind == "flac" else _wav_fields(s)
    cases += _full_scale_predictor_cases()          # (seed name "predictor": made from nothing)
    return ss, cases


if __name__ == "__main__":
    out_dir = sys.argv[1]
    os.makedirs(out_dir, exist_ok=True)
    all_seeds, all_cases = build()
    for s in all_seeds:
        if s.data:
            with open(os.path.join(out_dir, f"{s.name}__seed"), "wb") as f:
                f.write(s.data)
    for c in all_cases:
        with open(os.path.join(out_dir, f"{c.seed}__{c.label}"), "wb") as f:
            f.write(c.data)
    print(f"{len(all_cases)} cases and {sum(1 for s in all_seeds if s.data)} seeds in {out_dir}")
