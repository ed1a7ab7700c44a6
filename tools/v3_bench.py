"""large-v3 / large-v3-turbo against large-v2 on one MI355X, seeded synthetic weights: per utterance the fused log-mel (80 against 128
bins), the encoder, cross-K/V, the prefill and the decode step, for the 3.84 s and 29.2 s clips at beam 5 and beam 1.  Decode lengths
follow the headline's fixed convention (bench.py FIXED_NEW: 16 tokens for 3sec, 96 for 30sec), so every size runs the same number of
decoder passes and the rows compare per-stage time, not transcripts.

    python tools/v3_bench.py [--sizes large-v2,large-v3,large-v3-turbo] [--iters 10] [--warmup 3]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "willow-inference-server_amd"))

FIXED_NEW = {"3sec": 16, "30sec": 96}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="large-v2,large-v3,large-v3-turbo")
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    import numpy as np
    from wis_hip import _lib, audio, ctranslate2 as ct2, weights as W
    clips = {}
    for c in FIXED_NEW:
        pcm, _ = audio.load_audio(os.path.join(ROOT, "tests", "golden", "clips", f"{c}.flac"))
        clips[c] = (np.ascontiguousarray(audio.pad_or_trim(pcm)[None], np.float32), 1000.0 * pcm.shape[0] / 16000)
    rows = {}
    for size in a.sizes.split(","):
        arch = W.arch(size)
        model = ct2.Whisper("unused", weights=W.synthetic_weights(size), arch=arch, max_batch=1, max_beam=5)
        st = model.special
        prompt = [st.sot, st.lang_ids[0], st.transcribe, st.notimestamps]
        try:
            for c, (x, ms_audio) in clips.items():
                for beam in (5, 1):
                    keys = ("logmel_ms", "encoder_ms", "crosskv_ms", "prefill_ms", "decode_ms", "total_ms")
                    acc = {k: [] for k in keys + ("step_ms", "wall_ms")}
                    for i in range(a.warmup + a.iters):
                        t0 = time.perf_counter()
                        model.generate(ct2.StorageView.from_array(x), [prompt], beam_size=beam, fixed_new_tokens=FIXED_NEW[c],
                                       input_kind=_lib.WIS_IN_PCM_HOST)
                        wall = 1e3 * (time.perf_counter() - t0)
                        t = model.last_timing()
                        if i >= a.warmup:
                            for k in keys:
                                acc[k].append(t[k])
                            acc["step_ms"].append(t["decode_ms"] / max(1, t["decode_steps"] - 1))     # (the merged prefill + first step is not a step)
                            acc["wall_ms"].append(wall)
                    row = {k: round(float(np.median(v)), 4) for k, v in acc.items()}
                    row["audio_ms"] = round(ms_audio, 1)
                    row["encoder_share"] = round((row["logmel_ms"] + row["encoder_ms"] + row["crosskv_ms"]) / row["total_ms"], 4)
                    rows[f"{size}/{c}/beam{beam}"] = row
                    print(f"{size:15s} {c:6s} beam {beam}: " + " ".join(f"{k} {row[k]}" for k in ("logmel_ms", "encoder_ms", "crosskv_ms", "prefill_ms", "step_ms", "total_ms", "encoder_share")),
                          file=sys.stderr, flush=True)
        finally:
            model.close()
            del model
    print(json.dumps({"metric": "v3_stage_ms", "iters": a.iters, "fixed_new": FIXED_NEW, "rows": rows}))


if __name__ == "__main__":
    main()
