"""Milliseconds per wis_sv_embed (speaker-verification embedding, host PCM -> host embedding) for the three golden clips, seeded
weights at the true WavLM-base-plus-sv architecture.

    python tools/sv_bench.py [--iters 50] [--warmup 5]
    rocprofv3 --kernel-trace --stats -d OUT -o sv -- python tools/sv_bench.py --iters 20     # per-kernel (stage) times
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "willow-inference-server_amd"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    import numpy as np
    from wis_hip import audio, sv
    eng = sv.SpeakerVerifier(sv.SYNTHETIC)
    res = {}
    for name in ("3sec", "10sec", "30sec"):
        pcm, _ = audio.load_audio(os.path.join(ROOT, "tests", "golden", "clips", f"{name}.flac"))
        x = sv.preprocess(pcm)
        for _ in range(a.warmup):
            eng.embed_input(x)
        ts = []
        for _ in range(a.iters):
            t0 = time.perf_counter()
            eng.embed_input(x)
            ts.append((time.perf_counter() - t0) * 1e3)
        res[name] = {"samples": int(x.size), "ms_median": round(float(np.median(ts)), 3), "ms_min": round(float(np.min(ts)), 3)}
    print(json.dumps({"metric": "sv_embed_ms", "device_bytes": eng.device_bytes, "clips": res}))


if __name__ == "__main__":
    main()
