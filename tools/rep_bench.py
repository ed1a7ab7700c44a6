"""Milliseconds per decode step with repetition_penalty / no_repeat_ngram_size off and on (rep_rules_kernel at the head of the sampling tail
of every step graph), at the headline shape (large-v2, beam 5, the 3.84 s clip) and at 8 utterances x beam 5, in one process.  Both forms
run a fixed number of decoder passes (fixed_new_tokens), so the difference is the pre-pass.

    python tools/rep_bench.py [--size large-v2] [--iters 10] [--warmup 3] [--tokens 24] [--penalty 1.1] [--ngram 3]
    rocprofv3 --kernel-trace --stats -d OUT -o rep -- python tools/rep_bench.py --iters 5      # the pre-pass kernel's own time
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "willow-inference-server_amd"))

PROMPT = [50258, 50259, 50359, 50363]          # <|startoftranscript|><|en|><|transcribe|><|notimestamps|>


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", default="large-v2")
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--tokens", type=int, default=24)
    ap.add_argument("--penalty", type=float, default=1.1)
    ap.add_argument("--ngram", type=int, default=3)
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
            row = {}
            for name, kw in (("off", {}), ("on", dict(repetition_penalty=a.penalty, no_repeat_ngram_size=a.ngram))):
                step_ms = []
                for i in range(a.warmup + a.iters):
                    model.generate(feats, [PROMPT] * B, beam_size=5, fixed_new_tokens=a.tokens, **kw)
                    t = model.last_timing()
                    if i >= a.warmup:
                        step_ms.append(t["decode_ms"] / max(1, t["decode_steps"] - 1))      # (the merged prefill + first step is not a decode step)
                row[name] = round(float(np.median(step_ms)), 4)
            row["rep_share"] = round((row["on"] - row["off"]) / row["on"], 4)
            res[f"B{B}_beam5"] = row
    finally:
        model.close()
    print(json.dumps({"metric": "decode_step_ms", "size": a.size, "tokens": a.tokens, "penalty": a.penalty, "ngram": a.ngram, "shapes": res}))


if __name__ == "__main__":
    main()
