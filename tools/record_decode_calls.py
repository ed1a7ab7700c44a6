"""What the engine receives from the Python face (no GPU, no library needed): a fixed table of `Whisper.generate` / `generate_from_device` calls
is driven through a host-only model whose `_lib.load()` is a stand-in that answers 0 and records every entry point's arguments.

    python tools/record_decode_calls.py > tests/golden/decode_calls.json

Per table entry: the engine calls it made (entry point, every field of the `wis_gen_opts_t` behind the byref, B, P, the prompt array, the seeds
array, the draft arrays) or the error it raised (type and message, for `generate` and for the device form), and the entry's batch class: two
entries share a class exactly when their micro-batcher keys are equal.  tests/test_decode_options_cpu.py replays the table and compares with the
committed record, which was written by this tool at the commit before `DecodeOptions` replaced the positional batch key."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (os.path.join(ROOT, "willow-inference-server_amd"),):
    if _p not in sys.path:
        sys.path.insert(0, _p)

PLAIN = [50258, 50259, 50359, 50363]      # <|startoftranscript|> <|en|> <|transcribe|> <|notimestamps|>
TS = PLAIN[:3]                            # ... without <|notimestamps|>: Whisper's timestamp rules
LONG = [50361] + list(range(1000, 1036)) + PLAIN      # 41 tokens: <|startofprev|>, 36 text tokens, the start sequence
DRAFT = [400, 401, 402]
TRAJ = ([[400 + i + j for j in range(5)] for i in range(3)], [[(i + j) % 5 for j in range(5)] for i in range(3)])
DEV_PTR = 0x10000
SAMPLED = dict(beam_size=1, sampling_topk=0, sampling_temperature=0.7)


def table():
    """[(name, form, prompts, keyword arguments)]: form "both" runs through generate (one utterance) and generate_from_device, "host" through
    generate alone (what the device form has no argument for, or more than one utterance).  A name that starts with "refuse_" must raise."""
    t = [
        ("plain", "both", [PLAIN], {}),
        ("beam_5_spelled", "both", [PLAIN], dict(beam_size=5)),
        ("beam_1", "both", [PLAIN], dict(beam_size=1)),
        ("patience_2", "both", [PLAIN], dict(beam_size=2, patience=2.0)),
        ("patience_off", "both", [PLAIN], dict(patience=1)),
        ("length_penalty", "both", [PLAIN], dict(length_penalty=0.8)),
        ("length_penalty_off", "both", [PLAIN], dict(length_penalty=1.0)),
        ("suppress_blank_off", "both", [PLAIN], dict(suppress_blank=False)),
        ("suppress_blank_on", "both", [PLAIN], dict(suppress_blank=True)),
        ("fixed_new_tokens", "both", [PLAIN], dict(fixed_new_tokens=6)),
        ("max_length_100", "both", [PLAIN], dict(max_length=100)),
        ("return_scores", "both", [PLAIN], dict(return_scores=True)),
        ("timestamps", "both", [TS], {}),
        ("timestamps_cap_none", "both", [TS], dict(max_initial_timestamp_index=None)),
        ("timestamps_cap_50", "both", [TS], dict(max_initial_timestamp_index=50)),
        ("timestamps_cap_0", "both", [TS], dict(max_initial_timestamp_index=0)),
        ("cap_without_timestamps", "both", [PLAIN], dict(max_initial_timestamp_index=0)),
        ("no_speech_prob", "both", [PLAIN], dict(return_no_speech_prob=True)),
        ("no_speech_prob_cap_7", "both", [PLAIN], dict(return_no_speech_prob=True, max_initial_timestamp_index=7)),
        ("no_speech_prob_timestamps", "both", [TS], dict(return_no_speech_prob=True)),
        ("no_speech_prob_off", "both", [PLAIN], dict(return_no_speech_prob=False)),
        ("repetition_penalty", "both", [PLAIN], dict(repetition_penalty=1.1)),
        ("no_repeat_ngram", "both", [PLAIN], dict(no_repeat_ngram_size=3)),
        ("repetition_both", "both", [PLAIN], dict(repetition_penalty=1.1, no_repeat_ngram_size=3)),
        ("repetition_off", "both", [PLAIN], dict(repetition_penalty=1.0, no_repeat_ngram_size=0)),
        ("repetition_timestamps", "both", [TS], dict(no_repeat_ngram_size=2)),
        ("sample_seed", "both", [PLAIN], dict(SAMPLED, sampling_seed=7)),
        ("sample_other_seed", "both", [PLAIN], dict(SAMPLED, sampling_seed=2 ** 64 + 9)),
        ("sample_no_seed", "both", [PLAIN], dict(SAMPLED)),
        ("sample_n_3", "both", [PLAIN], dict(SAMPLED, num_hypotheses=3, sampling_seed=7)),
        ("sample_temperature_default", "both", [PLAIN], dict(beam_size=1, sampling_topk=0, sampling_seed=7)),
        ("sample_off", "both", [PLAIN], dict(beam_size=1, sampling_topk=1, sampling_temperature=0.5, num_hypotheses=1, sampling_seed=7)),
        ("sample_no_speech_prob", "both", [TS], dict(SAMPLED, num_hypotheses=3, sampling_seed=1, return_no_speech_prob=True)),
        ("sample_repetition", "both", [PLAIN], dict(SAMPLED, num_hypotheses=5, repetition_penalty=1.1, sampling_seed=7)),
        ("n_best_5", "both", [PLAIN], dict(beam_size=5, num_hypotheses=5)),
        ("n_best_3", "both", [PLAIN], dict(beam_size=5, num_hypotheses=3)),
        ("draft", "both", [PLAIN], dict(beam_size=1, draft_tokens=DRAFT)),
        ("draft_again", "both", [PLAIN], dict(beam_size=1, draft_tokens=DRAFT)),
        ("draft_empty", "both", [PLAIN], dict(beam_size=1, draft_tokens=[])),
        ("draft_at_beam_5", "both", [PLAIN], dict(beam_size=5, draft_tokens=DRAFT)),
        ("draft_trajectory", "both", [PLAIN], dict(beam_size=5, draft_trajectory=TRAJ)),
        ("draft_trajectory_other_beam", "both", [PLAIN], dict(beam_size=4, draft_trajectory=TRAJ)),
        ("draft_return_trajectory", "both", [PLAIN], dict(beam_size=1, draft_tokens=DRAFT, return_trajectory=True)),
        ("return_trajectory", "both", [PLAIN], dict(return_trajectory=True)),
        ("return_trajectory_repetition", "both", [PLAIN], dict(return_trajectory=True, repetition_penalty=1.5)),
        ("prompt_41", "both", [LONG], {}),
        ("prompt_41_beam_1", "both", [LONG], dict(beam_size=1)),
        ("prompt_16_draft", "both", [[50361] + [7] * 11 + PLAIN], dict(beam_size=1, draft_tokens=DRAFT)),
        ("two_utterances", "host", [PLAIN, PLAIN], {}),
        ("two_sampled_one_seed", "host", [PLAIN, PLAIN], dict(SAMPLED, sampling_seed=7)),
        ("two_sampled_two_seeds", "host", [PLAIN, PLAIN], dict(SAMPLED, sampling_seed=[8, 9])),
        ("two_sampled_no_seed", "host", [PLAIN, PLAIN], dict(SAMPLED)),
        ("two_with_a_draft", "host", [PLAIN, PLAIN], dict(beam_size=1, draft_tokens=DRAFT)),
        ("suppress_tokens_none", "host", [PLAIN], dict(suppress_tokens=())),
        ("suppress_tokens_default", "host", [PLAIN], dict(suppress_tokens=[-1])),
        ("pcm_input", "host", [PLAIN], dict(input_kind=2)),               # WIS_IN_PCM_HOST
        # ---- refusals
        ("refuse_beam_0", "both", [PLAIN], dict(beam_size=0)),
        ("refuse_beam_9", "both", [PLAIN], dict(beam_size=9)),
        ("refuse_beam_9_and_penalty_0", "both", [PLAIN], dict(beam_size=9, repetition_penalty=0)),
        ("refuse_prompt_229", "both", [[50361] + [7] * 224 + PLAIN], {}),
        ("refuse_prompt_0", "both", [[]], {}),
        ("refuse_long_prompt_draft", "both", [LONG], dict(beam_size=1, draft_tokens=DRAFT)),
        ("refuse_long_prompt_beam_9", "both", [[50361] + [7] * 224 + PLAIN], dict(beam_size=9)),
        ("refuse_patience", "both", [PLAIN], dict(patience=100)),
        ("refuse_patience_prompt_229", "both", [[50361] + [7] * 224 + PLAIN], dict(patience=100)),
        ("refuse_penalty_draft", "both", [PLAIN], dict(beam_size=1, draft_tokens=DRAFT, repetition_penalty=1.1)),
        ("refuse_ngram_trajectory", "both", [PLAIN], dict(beam_size=5, draft_trajectory=TRAJ, no_repeat_ngram_size=2)),
        ("refuse_penalty_0", "both", [PLAIN], dict(repetition_penalty=0)),
        ("refuse_penalty_text", "both", [PLAIN], dict(repetition_penalty="x")),
        ("refuse_ngram_negative", "both", [PLAIN], dict(no_repeat_ngram_size=-1)),
        ("refuse_ngram_fraction", "both", [PLAIN], dict(no_repeat_ngram_size=1.5)),
        ("refuse_sample_draft", "both", [PLAIN], dict(SAMPLED, draft_tokens=DRAFT)),
        ("refuse_topk_5", "both", [PLAIN], dict(beam_size=1, sampling_topk=5)),
        ("refuse_topk_negative", "both", [PLAIN], dict(beam_size=1, sampling_topk=-1)),
        ("refuse_topk_17", "both", [PLAIN], dict(beam_size=1, sampling_topk=17)),
        ("refuse_temperature_0", "both", [PLAIN], dict(beam_size=1, sampling_topk=0, sampling_temperature=0)),
        ("refuse_hypotheses_0", "both", [PLAIN], dict(num_hypotheses=0)),
        ("refuse_hypotheses_9", "both", [PLAIN], dict(num_hypotheses=9)),
        ("refuse_hypotheses_text", "both", [PLAIN], dict(num_hypotheses="x")),
        ("refuse_sample_beam_5", "both", [PLAIN], dict(beam_size=5, sampling_topk=0)),
        ("refuse_hypotheses_over_beam", "both", [PLAIN], dict(beam_size=1, num_hypotheses=3)),
        ("refuse_hypotheses_over_beam_3", "both", [PLAIN], dict(beam_size=3, num_hypotheses=4)),
        ("refuse_samples_over_max_beam", "both", [PLAIN], dict(SAMPLED, num_hypotheses=8)),
        ("refuse_sample_penalty_0", "both", [PLAIN], dict(beam_size=5, sampling_topk=0, repetition_penalty=0)),
        ("refuse_timestamps_draft", "both", [TS], dict(beam_size=1, draft_tokens=DRAFT)),
        ("refuse_timestamps_trajectory", "both", [TS], dict(beam_size=5, draft_trajectory=TRAJ)),
        ("refuse_no_speech_prob_draft", "both", [PLAIN], dict(beam_size=1, draft_tokens=DRAFT, return_no_speech_prob=True)),
        ("refuse_prompt_count", "host", [PLAIN, PLAIN, PLAIN], {}),
        ("refuse_prompt_lengths", "host", [PLAIN, TS], {}),
        ("refuse_mixed_timestamps", "host", [TS, [50258, 50259, 50363]], {}),
        ("refuse_seed_count", "host", [PLAIN, PLAIN], dict(SAMPLED, sampling_seed=[1, 2, 3])),
        ("refuse_input_kind", "host", [PLAIN], dict(input_kind=1)),       # WIS_IN_MEL_DEV
    ]
    assert len({e[0] for e in t}) == len(t)
    return t


APPENDED_FIELDS = ("phrases", "phrase_mass")      # wis_gen_opts_t fields younger than tests/golden/decode_calls.json


class RecordingLib:
    """Stand-in for the loaded library: the decode entry points answer 0 and append what they were given to `calls`."""

    def __init__(self):
        self.calls = []

    @staticmethod
    def _opts(ref):
        o = ref._obj      # (the struct behind ctypes.byref)
        # a field appended to wis_gen_opts_t AFTER the golden record was made is recorded when a call sets it: 0 is what a caller that never knew
        # the field passes, so a call of the table that reaches the engine with such a field on shows up as a key the golden record lacks
        return {name: getattr(o, name) for name, _ in type(o)._fields_ if name not in APPENDED_FIELDS or getattr(o, name) != 0}

    def _record(self, name, src, B, prompts, P, opts, **more):
        o = self._opts(opts)
        rec = dict(entry=name, opts=o, B=int(B), P=int(P), prompts=[int(x) for x in prompts[:int(B) * int(P)]], **more)
        if o["input_kind"] == 1:      # WIS_IN_MEL_DEV, device-resident features: the pointer is the caller's
            rec["src"] = src.value
        self.calls.append(rec)
        return 0

    def wis_generate(self, h, src, B, prompts, P, opts, ids, lens, scores):
        return self._record("wis_generate", src, B, prompts, P, opts)

    def wis_generate_n(self, h, src, B, prompts, P, opts, seeds, ids, lens, scores):
        return self._record("wis_generate_n", src, B, prompts, P, opts, seeds=[int(x) for x in seeds[:int(B)]])

    def wis_generate_draft(self, h, src, prompts, P, opts, draft, n, ids, lens, scores, acc):
        return self._record("wis_generate_draft", src, 1, prompts, P, opts, draft=[int(x) for x in draft[:int(n)]])

    def wis_generate_draft_beam(self, h, src, prompts, P, opts, tok, org, steps, ids, lens, scores, acc):
        n = int(steps) * self._opts(opts)["beam_size"]
        return self._record("wis_generate_draft_beam", src, 1, prompts, P, opts, steps=int(steps), draft_tok=[int(x) for x in tok[:n]], draft_org=[int(x) for x in org[:n]])

    def wis_last_no_speech_prob(self, h, B, out):
        self.calls.append(dict(entry="wis_last_no_speech_prob", B=int(B)))
        return 0

    def wis_last_trajectory(self, h, b, tok, org, cap, n):
        self.calls.append(dict(entry="wis_last_trajectory", b=int(b), cap=int(cap)))
        return 0

    def wis_dev_copy_peer(self, dst_dev, dst, src_dev, src, nbytes):
        self.calls.append(dict(entry="wis_dev_copy_peer", dst_device=int(dst_dev), src_device=int(src_dev), src=src.value, nbytes=int(nbytes)))
        return 0


def record():
    """-> {"entries": [{name, form, calls | error}], "classes": {"name/form": class index}}"""
    from wis_hip import _lib, ctranslate2 as ct2, weights as W
    lib, saved = RecordingLib(), _lib.load
    _lib.load = lambda: lib
    model = ct2.Whisper.from_handles([(None, 0)], W.arch("large"))
    model._batcher.close()
    keys = []

    class Batcher:      # synchronous: every submit is its own device batch on the one replica
        def submit(self, key, rows, affinity=None):
            keys.append(key)
            return ct2._run_batch(model._replicas[0], key, rows)

        def close(self):
            pass
    model._batcher = Batcher()

    def run(name, form, prompts, kw):
        del lib.calls[:], keys[:]
        ct2.set_random_seed(1234)      # (an unseeded sampled call then draws the same seeds every time)
        try:
            if form == "device":
                model.generate_from_device(0, DEV_PTR, prompts[0], **kw)
            else:
                B = 2 if name == "refuse_prompt_count" else len(prompts)      # (three prompts for two utterances)
                shape = (B, 480000) if kw.get("input_kind") == 2 else (B, 80, 3000)
                model.generate(ct2.StorageView.from_array(np.zeros(shape, np.float32)), prompts, **kw)
        except Exception as e:
            return dict(error=[type(e).__name__, str(e)]), None
        return dict(calls=list(lib.calls)), keys[0]
    try:
        entries, entry_keys = [], []
        for name, form, prompts, kw in table():
            for f in (("host", "device") if form == "both" else ("host",)):
                out, key = run(name, f, prompts, kw)
                entries.append(dict(name=name, form=f, **out))
                entry_keys.append(key)
    finally:
        _lib.load = saved
        ct2.set_random_seed(None)
        model._replicas = []
    reps, classes = [], {}      # the partition the batcher sees: entries whose keys compare equal
    for e, k in zip(entries, entry_keys):
        if k is None:
            continue
        for i, r in enumerate(reps):
            if r == k:
                break
        else:
            i = len(reps)
            reps.append(k)
        classes[f"{e['name']}/{e['form']}"] = i
    return dict(entries=entries, classes=classes)


def main():
    out = record()
    print("{\n \"entries\": [\n  " + ",\n  ".join(json.dumps(e) for e in out["entries"]) + "\n ],\n \"classes\": " + json.dumps(out["classes"]) + "\n}")


if __name__ == "__main__":
    main()
