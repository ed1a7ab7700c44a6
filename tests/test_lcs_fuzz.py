"""not gpu: `find_longest_common_sequence` (product wis_hip.audio and the oracle restatement) must be BIT-EXACT with
the reference's wis/audio.py:139-159 — integer work.  Two layers:

* always: the committed golden cases (tests/golden/chunker_lcs.json, produced by the reference's own code) — see
  test_host_logic.py / test_oracle_audio.py — plus the hand-checked broadcast case of the round-1 review;
* a 3 000-case fuzz of small random windows — including running sequences of 0, 1 and 2 tokens and windows shorter than
  the overlap — against the outputs of the IMPORTED reference function (tests/golden/lcs_fuzz.json, written by
  tests/golden/make_golden.py), run under its pinned numpy's array-comparison semantics (tests/golden/np123_shim.py), plus
  the subset the installed numpy evaluated natively (no shim at all) to the same ids."""
import hashlib
import json
import os

import numpy as np

from oracle import audio_ref

FUZZ_N, FUZZ_SEED = 3000, 2024
SPECIAL = [50257, 50258, 50259, 50359, 50363]


class Tok:
    all_special_ids = SPECIAL


def _cases(n, seed):
    rng = np.random.default_rng(seed)
    for _ in range(n):
        vocab = int(rng.integers(2, 5))
        k = int(rng.integers(2, 5))
        first = int(rng.choice([0, 1, 1, 2, 3, 6]))
        lists = [[int(v) for v in rng.integers(0, vocab, size=first)]]
        for _ in range(k - 1):
            lists.append([int(v) for v in rng.integers(0, vocab, size=int(rng.integers(0, 9)))])
        if rng.random() < 0.2:      # sprinkle special ids (dropped before matching)
            lists = [[SPECIAL[0]] + l + [SPECIAL[1]] for l in lists]
        yield lists


def test_review_case_broadcast():
    from wis_hip import audio
    seqs = [([2], (1, 0, 0)), ([3, 2, 2, 3, 0], (1, 0, 0))]
    assert audio.find_longest_common_sequence(seqs, Tok).tolist() == [2, 3, 0]
    assert audio_ref.find_longest_common_sequence(seqs, SPECIAL).tolist() == [2, 3, 0]


def test_product_equals_oracle_on_fuzz():
    from wis_hip import audio
    for lists in _cases(1500, 11):
        seqs = [(l, (1, 0, 0)) for l in lists]
        assert audio.find_longest_common_sequence(seqs, Tok).tolist() == audio_ref.find_longest_common_sequence(seqs, SPECIAL).tolist(), lists


def test_fuzz_against_imported_reference(golden_dir):
    from wis_hip import audio
    with open(os.path.join(golden_dir, "lcs_fuzz.json")) as f:
        g = json.load(f)
    cases = list(_cases(FUZZ_N, FUZZ_SEED))
    # the same windows the reference ran on (a change of the generator or of numpy's random streams would void the fixture)
    assert (g["n"], g["seed"]) == (FUZZ_N, FUZZ_SEED) and hashlib.sha256(json.dumps(cases).encode()).hexdigest() == g["cases_sha256"]
    n = native = 0
    for lists, want, raw_agrees in zip(cases, g["want"], g["native"], strict=True):
        seqs = [(l, (1, 0, 0)) for l in lists]
        assert audio.find_longest_common_sequence(seqs, Tok).tolist() == want, lists
        assert audio_ref.find_longest_common_sequence(seqs, SPECIAL).tolist() == want, lists
        if raw_agrees is not None:      # where the installed numpy evaluated the reference without the shim it agreed as well
            assert raw_agrees, lists
            native += 1
        n += 1
    assert n == 3000 and native > 500
