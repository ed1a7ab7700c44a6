"""What resampling an upload costs on the host (wis_hip.audio.resample, numpy) and on the GPU (wis_resample, csrc/resample.hip).

    python tools/resample_bench.py                       # the two resamplers alone: host PCM in -> host PCM out, four rates x two lengths
    python tools/resample_bench.py --e2e [--tree DIR]    # do_whisper on 48 kHz WAVs of 3sec.flac / 30sec.flac beside the 16 kHz originals
    python tools/resample_bench.py --ab PARENT_DIR       # --e2e on this tree and on a built checkout of the parent commit, alternating
                                                         # pairs of processes (P N N P P N N P P N), medians and their spread as markdown

Every time is a host clock around a call that returns host data, i.e. that ends in a device synchronise.  --tree DIR runs the package
of another built checkout (DIR/willow-inference-server_amd) with this file's measurement, so both sides of --ab are timed by one code.
The 48 kHz WAVs are made here (the host resampler, 16 bit) in a temporary directory."""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RATES = (8000, 22050, 44100, 48000)
SECONDS = (3.84, 29.2)
ORDER = "PNNPPNNPPN"


def median(v):
    v = sorted(v)
    return v[len(v) // 2] if len(v) % 2 else 0.5 * (v[len(v) // 2 - 1] + v[len(v) // 2])


def timed(fn, warmup, iters):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(iters):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return median(ts)


def bench_resamplers(a):
    import numpy as np
    from wis_hip import _lib, audio
    _lib.require_gpu()
    rows = {}
    for sr in RATES:
        for sec in SECONDS:
            x = (np.random.default_rng(sr).standard_normal(int(round(sec * sr))) * 0.1).astype(np.float32)
            host = timed(lambda: audio.resample(x, sr), 1, a.iters)
            gpu = timed(lambda: audio.resample_gpu(x, sr, a.device), a.warmup, a.iters)
            y_h, y_g = audio.resample(x, sr), audio.resample_gpu(x, sr, a.device)
            rows[f"{sr}Hz_{sec}s"] = dict(host_ms=round(host, 3), gpu_ms=round(gpu, 3), max_abs_diff=float(np.abs(y_h - y_g).max()))
    print(json.dumps({"metric": "resample_ms_host_pcm_to_host_pcm", "iters": a.iters, "rows": rows}))


def make_wavs(audio, tmp):
    """{"3sec": (16 kHz original, 48 kHz WAV), "30sec": ...}"""
    import wave
    import numpy as np
    out = {}
    for clip in ("3sec", "30sec"):
        flac = os.path.join(ROOT, "tests", "golden", "clips", clip + ".flac")
        pcm, _ = audio.load_audio(flac)
        s16 = np.clip(np.round(audio.resample(pcm, 16000, 48000) * 32768.0), -32768, 32767).astype("<i2")
        path = os.path.join(tmp, clip + "_48k.wav")
        with wave.open(path, "wb") as w:
            w.setparams((1, 2, 48000, 0, "NONE", "NONE"))
            w.writeframes(s16.tobytes())
        out[clip] = (flac, path)
    return out


def bench_e2e(a):
    from wis_hip import audio
    from wis_hip.settings import APISettings
    from wis_hip.whisper import WhisperModels, do_whisper
    s = APISettings()
    s.whisper_model_path = "synthetic:{size}"
    s.fixed_new_tokens = a.tokens
    s.resample_on_gpu = bool(a.resample_on_gpu)       # (a checkout without the setting ignores it: the host resampler)
    models = WhisperModels(s, device_index=[a.device])
    res = {"tree": a.tree or ROOT, "resample_on_gpu": bool(a.resample_on_gpu) and hasattr(audio, "resample_gpu"), "model": a.model}
    with tempfile.TemporaryDirectory() as tmp:
        for clip, (orig, wav48) in make_wavs(audio, tmp).items():
            t16 = timed(lambda: do_whisper(orig, a.model, a.beam, models=models), a.warmup, a.iters)
            t48 = timed(lambda: do_whisper(wav48, a.model, a.beam, models=models), a.warmup, a.iters)
            res[clip] = dict(ms_16k=round(t16, 3), ms_48k=round(t48, 3), diff_ms=round(t48 - t16, 3))
    print("RESULT " + json.dumps(res))


def bench_ab(a):
    runs = {"P": [], "N": []}
    for i, who in enumerate(ORDER):
        cmd = [sys.executable, os.path.abspath(__file__), "--e2e", "--model", a.model, "--beam", str(a.beam), "--iters", str(a.iters), "--warmup", str(a.warmup),
               "--tokens", str(a.tokens), "--device", str(a.device), "--resample-on-gpu", str(a.resample_on_gpu)] + (["--tree", a.ab] if who == "P" else [])
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=a.child_timeout)
        line = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
        if r.returncode != 0 or not line:
            sys.stderr.write(r.stdout[-2000:] + r.stderr[-2000:])
            raise SystemExit(f"run {i + 1} ({who}) failed with exit status {r.returncode}")      # nothing more is started after a failed run
        runs[who].append(json.loads(line[0][7:]))
        print(f"run {i + 1} {who}: {line[0][7:]}", flush=True)
    print("\n| pair | clip | parent 16 kHz | parent 48 kHz | parent diff | new 16 kHz | new 48 kHz | new diff |\n|---|---|---|---|---|---|---|---|")
    for clip in ("3sec", "30sec"):
        for j, (p, n) in enumerate(zip(runs["P"], runs["N"])):
            print(f"| {j + 1} | {clip} | {p[clip]['ms_16k']} | {p[clip]['ms_48k']} | {p[clip]['diff_ms']} | {n[clip]['ms_16k']} | {n[clip]['ms_48k']} | {n[clip]['diff_ms']} |")
        for name, f in (("median", median), ("min", min), ("max", max)):
            cells = [round(f([r[clip][k] for r in runs[w]]), 3) for w in "PN" for k in ("ms_16k", "ms_48k", "diff_ms")]
            print(f"| {name} | {clip} | " + " | ".join(str(c) for c in cells) + " |")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--e2e", action="store_true")
    ap.add_argument("--ab", default=None, metavar="PARENT_DIR")
    ap.add_argument("--tree", default=None)
    ap.add_argument("--model", default="large")
    ap.add_argument("--beam", type=int, default=5)
    ap.add_argument("--tokens", type=int, default=24)
    ap.add_argument("--iters", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--resample-on-gpu", type=int, default=1)
    ap.add_argument("--child-timeout", type=int, default=300)
    a = ap.parse_args()
    sys.path.insert(0, os.path.join(os.path.abspath(a.tree) if a.tree else ROOT, "willow-inference-server_amd"))
    if a.ab:
        bench_ab(a)
    elif a.e2e:
        bench_e2e(a)
    else:
        bench_resamplers(a)


if __name__ == "__main__":
    main()
