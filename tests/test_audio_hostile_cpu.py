"""not gpu: the upload decoder (csrc/audio_io.c) on bytes from strangers - the fixed corpus of tests/audio_corpus.py against the normal
library build.  The same files run under AddressSanitizer / UBSan and an allocation limit in tools/audio_io_harness.c (a stand-alone
CPU program, tools/README.md; never from pytest)."""
import ctypes as C

import numpy as np
import pytest

import audio_corpus
from test_audio_formats_cpu import WIS_E_CHECKSUM, WIS_E_FORMAT, WIS_E_NOMEM, expected_pcm

_CORPUS = None


def corpus():
    global _CORPUS
    if _CORPUS is None:
        _CORPUS = audio_corpus.build()
    return _CORPUS


def raw_decode(lib, data):
    p, n, sr, md = C.POINTER(C.c_float)(), C.c_int64(-1), C.c_int(-1), C.c_int(-7)
    rc = lib.wis_audio_decode(data, len(data), C.byref(p), C.byref(n), C.byref(sr), C.byref(md))
    if rc != 0:
        assert not p, "on an error the output pointer stays null"
        return rc, None, md.value
    try:
        assert n.value >= 0 and bool(p)
        pcm = np.ctypeslib.as_array(p, shape=(max(n.value, 1),))[:n.value].copy()
    finally:
        lib.wis_audio_free(p)
    return rc, pcm, md.value


SEED_NAMES = ["clip3sec", "midside24", "escape16", "total0", "wav16stereo", "wavfloat_ext", "wavstreaming"]


def test_corpus_is_complete_and_never_changes():
    seeds, cases = corpus()
    assert [s.name for s in seeds] == SEED_NAMES and all(0 < len(s.data) < 400 * 1024 for s in seeds)
    again = audio_corpus.build()[1]
    assert len(again) == len(cases) and all(a.data == b.data and a.label == b.label for a, b in zip(again[::37], cases[::37]))
    for s in seeds:
        mine = [c.label for c in cases if c.seed == s.name]
        assert len(set(mine)) == len(mine)
        n = len(s.data)
        assert sum(lb.startswith("trunc") for lb in mine) == min(n, 301) + min(64, max(n - 301, 0))
        assert sum(lb.startswith("flip") for lb in mine) == 800 and sum(lb.startswith("over") for lb in mine) == 500
        if s.kind == "flac":
            for want in ("total_2p36m1", "total_plus1", "total_minus1", "si_bps01", "si_bps32", "si_ch1", "si_ch8", "si_minbs0", "si_maxbs15",
                         "hdr_bs00", "hdr_bs15", "hdr_sr15", "hdr_ch15", "hdr_bps07"):
                assert want in mine, want
        else:
            assert sum(lb.startswith("fmt_") for lb in mine) == 18 and sum(lb.startswith("len_") for lb in mine) == 32
    assert sum(c.seed == "predictor" for c in cases) == 30


GROUPS = {"truncations": ("trunc",), "bit_flips": ("flip",), "overwrites": ("over",), "fields": ("total", "si_", "hdr_", "fmt_", "len_")}


@pytest.mark.parametrize("group", list(GROUPS))
@pytest.mark.parametrize("name", SEED_NAMES)
def test_hostile_corpus(lib, name, group):
    """every case of one seed and one kind of damage: an allowed return code and nothing left behind; what a FLAC signature vouches for is
    the seed's audio to the bit; at least one case of each kind survives (the test is not refusing everything)"""
    accepted = _run_cases(lib, name, [c for c in corpus()[1] if c.seed == name and c.label.startswith(GROUPS[group])], group)
    if group in ("bit_flips", "fields"):          # every seed has cases that must survive: flips in padding, a rate or a size STREAMINFO only reports,
        assert accepted > 0                        # a `fmt ` byte rate nobody reads (a truncated or overwritten FLAC stream never does: CRC, total, MD5)


def test_hostile_full_scale_predictors(lib):
    """frames with right CRCs whose warm-up samples and residuals drive the predictors as far as numbers go: all refused"""
    mine = [c for c in corpus()[1] if c.seed == "predictor"]
    assert len(mine) == 30
    assert _run_cases(lib, "predictor", mine, "crafted") == 0


def test_every_corpus_case_is_run():
    cases = corpus()[1]
    n = sum(1 for c in cases if c.seed == "predictor" or c.label.startswith(tuple(p for g in GROUPS.values() for p in g)))
    assert n == len(cases)


def _run_cases(lib, name, mine, group):
    seeds, cases = corpus()
    seed = next((s for s in seeds if s.name == name), None)
    ref = None
    if seed is not None:
        rc, ref, md = raw_decode(lib, seed.data)
        assert rc == 0 and md == (1 if seed.kind == "flac" else -1)
        if seed.samples is not None:
            assert np.array_equal(ref, expected_pcm(seed.samples, seed.bps))
    accepted, refused = 0, {WIS_E_FORMAT: 0, WIS_E_CHECKSUM: 0, WIS_E_NOMEM: 0}
    for c in mine:
        rc, pcm, md = raw_decode(lib, c.data)
        assert rc == 0 or rc in refused, (c.label, rc)
        if rc != 0:
            refused[rc] += 1
            continue
        accepted += 1
        assert not c.expect_refused, c.label
        if seed is not None and seed.kind == "flac":
            if md == 1:          # a signature that is present and right: the seed's audio, to the bit - same amplitude, not just same integers
                assert pcm.shape == ref.shape and np.array_equal(pcm, ref), c.label
            else:
                assert md == -1 and c.data[26:42] == bytes(16), c.label
        else:
            assert pcm.shape[0] <= len(c.data), c.label
    print(f"{name} / {group}: {len(mine)} cases, {accepted} accepted, refused: {refused[WIS_E_FORMAT]} format, {refused[WIS_E_CHECKSUM]} checksum, "
          f"{refused[WIS_E_NOMEM]} out of memory")
    assert accepted + sum(refused.values()) == len(mine)          # (nothing skipped)
    return accepted
