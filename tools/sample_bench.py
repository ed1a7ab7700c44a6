"""Milliseconds per decode step of a sampled decode beside the searches it stands next to, in one process: greedy, sampling with one sample,
sampling with five (whole vocabulary, T = 0.6: openai-whisper's fallback call `beam_size=1, num_hypotheses=5, sampling_topk=0`) and beam 5, at
one and at eight utterances of the 3.84 s clip (large-v2).  The sampled n = 5 step runs the beam-5 step's decoder pass - five rows per utterance
over one cross K / V - and a tail without a pool ranking across rows or a cache reorder: it is judged against the beam-5 step of the SAME run.
Every form runs a fixed number of decoder passes (fixed_new_tokens); `--pairs` repeats the whole set, so the spread between repeats is in the
output next to the medians.

    python tools/sample_bench.py [--size large-v2] [--iters 10] [--warmup 3] [--tokens 24] [--pairs 3]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "willow-inference-server_amd"))

PROMPT = [50258, 50259, 50359, 50363]          # <|startoftranscript|><|en|><|transcribe|><|notimestamps|>
FORMS = (("greedy", dict(beam_size=1)),
         ("sample_n1", dict(beam_size=1, sampling_topk=0, sampling_temperature=0.6, sampling_seed=1)),
         ("sample_n5", dict(beam_size=1, num_hypotheses=5, sampling_topk=0, sampling_temperature=0.6, sampling_seed=1)),
         ("beam5", dict(beam_size=5)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", default="large-v2")
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--tokens", type=int, default=24)
    ap.add_argument("--pairs", type=int, default=3)
    a = ap.parse_args()
    import numpy as np
    from wis_hip import audio, ctranslate2 as ct2, weights as W
    pcm, _ = audio.load_audio(os.path.join(ROOT, "tests", "golden", "clips", "3sec.flac"))
    mel = audio.log_mel_spectrogram(audio.pad_or_trim(pcm)).numpy()
    model = ct2.Whisper("unused", weights=W.synthetic_weights(a.size), arch=W.arch(a.size), max_batch=8, max_beam=5)
    res = {}
    try:
        for B in (1, 8):
            feats = ct2.StorageView.from_array(np.ascontiguousarray(np.repeat(mel[None], B, axis=0)))
            row = {name: [] for name, _ in FORMS}
            for rep in range(a.pairs):
                for name, kw in FORMS:
                    step_ms = []
                    for i in range((a.warmup if rep == 0 else 1) + a.iters):
                        model.generate(feats, [PROMPT] * B, fixed_new_tokens=a.tokens, **kw)
                        t = model.last_timing()
                        if i >= (a.warmup if rep == 0 else 1):
                            step_ms.append(t["decode_ms"] / max(1, t["decode_steps"] - 1))      # (the merged prefill + first step is not a decode step)
                    row[name].append(round(float(np.median(step_ms)), 4))
            out = {name: dict(median=round(float(np.median(v)), 4), repeats=v) for name, v in row.items()}
            d = [s - b for s, b in zip(row["sample_n5"], row["beam5"])]
            out["sample_n5_minus_beam5"] = dict(median=round(float(np.median(d)), 4), repeats=[round(x, 4) for x in d],
                                                beam5_spread=round(max(row["beam5"]) - min(row["beam5"]), 4))
            res[f"B{B}"] = out
    finally:
        model.close()
    print(json.dumps({"metric": "decode_step_ms", "size": a.size, "tokens": a.tokens, "shapes": res}))


if __name__ == "__main__":
    main()
