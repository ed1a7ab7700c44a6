"""`DecodeOptions` (wis_hip/ctranslate2.py) carries a call's options from `Whisper.generate` / `generate_from_device` to the engine call and is the
micro-batcher's key.  tests/golden/decode_calls.json is what tools/record_decode_calls.py recorded at the commit BEFORE the record replaced the
positional key tuple: per table entry the engine calls (entry point, every field of wis_gen_opts_t, B, P, prompts, seeds, drafts) or the
refusal, and the partition of the entries into device-batch classes.  The table is replayed here and must give the same, field for field."""
import itertools
import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def replay():
    """(golden record, today's record): the table is driven once for the module"""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import record_decode_calls
    finally:
        sys.path.remove(os.path.join(ROOT, "tools"))
    with open(os.path.join(ROOT, "tests", "golden", "decode_calls.json")) as f:
        golden = json.load(f)
    return golden, json.loads(json.dumps(record_decode_calls.record())), record_decode_calls.table()


def test_the_table_covers_what_it_claims(replay):
    golden, now, table = replay
    assert [(e["name"], e["form"]) for e in now["entries"]] == [(e["name"], e["form"]) for e in golden["entries"]]
    assert len(table) >= 30 and sum(1 for e in golden["entries"] if e["form"] == "device") >= 30
    entries = {c["entry"] for e in golden["entries"] for c in e.get("calls", [])}
    assert entries == {"wis_generate", "wis_generate_n", "wis_generate_draft", "wis_generate_draft_beam", "wis_last_no_speech_prob", "wis_last_trajectory"}
    for e in golden["entries"]:      # a refusal never reaches the engine, everything else does
        assert ("error" in e) == e["name"].startswith("refuse_") and ("calls" in e) != ("error" in e), e["name"]
        assert "error" in e or len(e["calls"]) >= 1


def test_the_engine_receives_the_same_calls(replay):
    golden, now, _ = replay
    for want, got in zip(golden["entries"], now["entries"]):
        if "calls" in want:
            assert got.get("calls") == want["calls"], (want["name"], want["form"])


def test_refusals_are_generates_under_both_entry_points(replay):
    """Same exception type, same message: `generate`'s checks, order and texts are the reference, and the device form now runs the same validator
    (before, its own copy answered some of these cases with another message or checked in another order)."""
    golden, now, _ = replay
    want = {e["name"]: e["error"] for e in golden["entries"] if "error" in e and e["form"] == "host"}
    assert len(want) >= 30
    seen = set()
    for e in now["entries"]:
        if e["name"] in want:
            assert e.get("error") == want[e["name"]], (e["name"], e["form"])
            seen.add((e["name"], e["form"]))
    assert {n for n, f in seen if f == "host"} == set(want) and sum(1 for n, f in seen if f == "device") >= 25


def test_two_calls_share_a_device_batch_exactly_when_they_did(replay):
    golden, now, _ = replay
    assert set(now["classes"]) == set(golden["classes"])
    assert len(set(golden["classes"].values())) > 40      # (the table is not one class)
    for a, b in itertools.combinations(sorted(golden["classes"]), 2):
        assert (now["classes"][a] == now["classes"][b]) == (golden["classes"][a] == golden["classes"][b]), (a, b)


def test_the_record_is_canonical_and_a_draft_compares_by_identity():
    import numpy as np
    from wis_hip import _lib, ctranslate2 as ct2
    plain = ct2.DecodeOptions(4, 5, 224)
    assert plain == (4, 5, 224, 1.0, 1.0, True, True, 0, _lib.WIS_IN_MEL_HOST, None, False, False, 50, False, 1.0, 0, 0, 1.0, 1)
    assert plain._fields == ("prompt_len", "beam_size", "max_new_tokens", "length_penalty", "patience", "suppress_blank", "suppress_default", "fixed_new_tokens",
                             "input_kind", "draft", "return_trajectory", "timestamps", "max_initial_timestamp_index", "no_speech_prob", "repetition_penalty",
                             "no_repeat_ngram_size", "sampling_topk", "sampling_temperature", "num_hypotheses")
    for f in plain._fields:      # every field takes part in equality
        other = plain._replace(**{f: ct2._Draft(tokens=(1,)) if f == "draft" else (None if f == "max_initial_timestamp_index" else getattr(plain, f) + 1)})
        assert other != plain and hash(other) != hash(plain), f
    traj = (np.zeros((2, 5), np.int32), np.zeros((2, 5), np.int32))
    a, b = ct2._Draft(trajectory=traj), ct2._Draft(trajectory=traj)
    assert a != b and a == a and plain._replace(draft=a) != plain._replace(draft=b) and plain._replace(draft=a) == plain._replace(draft=a)
    assert len({plain._replace(draft=a), plain._replace(draft=b), plain}) == 3      # hashed without touching the arrays
    assert ct2._Draft(tokens=(1, 2)) != ct2._Draft(tokens=(1, 2))


def test_capacity_is_the_formula_of_its_docstring():
    """<= 96 decoder rows per pass: utterances x max(beam, num_hypotheses) while decoding, and - up to 16 prompt tokens, the merged prefill - utterances x P."""
    from wis_hip import ctranslate2 as ct2
    for P, beam, n, max_batch in itertools.product((1, 4, 16, 17, 228), (1, 5, 8), (1, 5, 8), (8, 32, 96)):
        want = min(max_batch, 96 // max(beam, n))
        if P <= 16:
            want = min(want, 96 // P)
        assert ct2._capacity(max_batch, ct2.DecodeOptions(P, beam, 224, num_hypotheses=n)) == max(1, want), (P, beam, n, max_batch)
