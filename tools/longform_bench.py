"""What long-form transcription costs on a synthetic 65 s recording at large-v2 shapes (seeded weights, a fixed decode length per window):

  front end   wis_longmel_create + every window the seek loop asked for (one wis_longmel_window call each, features left on the device) against the same
              number of wis_logmel window calls on host PCM (features left on the device)
  request     do_whisper(long_form="seek") against do_whisper(long_form="chunk") of the same run: whole requests, wall clock

There is no pass mark: the seek loop exists for the definition (one log-mel over the recording, the next window at the last closed timestamp) and for the
options it makes possible, not for speed; seeded weights put their timestamps anywhere, so the number of windows is the weights', not a recording's.
The forms ALTERNATE over `--reps` rounds; every figure is the median of the rounds (min .. max).  Numbers of one run on one box: never compare across
boxes or runs.

    python tools/longform_bench.py [--size large] [--reps 5] [--tokens 24] [--out profiles/longform_ab.md]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "willow-inference-server_amd"))


def recording(seconds=65.0, seed=65):
    import numpy as np
    rng = np.random.default_rng(seed)
    t = np.arange(int(16000 * seconds))
    x = 0.2 * np.sin(2 * np.pi * 220.0 * t / 16000.0) * (1.0 + 0.5 * np.sin(2 * np.pi * 0.7 * t / 16000.0)) + 0.02 * rng.standard_normal(t.shape[0])
    return x.astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", default="large")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--tokens", type=int, default=24)
    ap.add_argument("--out", default=None, help="write the table (markdown) here")
    a = ap.parse_args()
    import numpy as np
    from wis_hip import _lib, audio
    from wis_hip.settings import APISettings
    from wis_hip.whisper import WhisperModels, do_whisper
    s = APISettings()
    s.whisper_model_path = "synthetic:{size}"
    s.fixed_new_tokens = a.tokens
    models = WhisperModels(s, device_index=[0])
    model = models.get(a.size)
    n_mels = model.n_mels
    pcm = recording()
    lib = _lib.load()
    run = lambda mode: do_whisper(pcm, a.size, 5, "transcribe", False, "en", models=models, long_form=mode, no_speech_threshold=1e30)
    try:
        seeks = [w["seek"] for w in run("seek").seek]      # (warm-up of the seek request; the windows the loop asks for on these weights)
        run("chunk")
        n_win = len(seeks)
        d_out = _lib.DevBuf(n_mels * 3000 * 4, 0)
        one = (C.c_int64 * 1)(0)
        ns = (C.c_int64 * 1)(audio.N_SAMPLES)
        wins = [np.ascontiguousarray(audio.pad_or_trim(pcm[160 * k:160 * k + audio.N_SAMPLES])) for k in seeks]
        t_long, t_win, t_seek, t_chunk = [], [], [], []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            h = C.c_void_p()
            _lib.check(lib.wis_longmel_create(0, n_mels, _lib.ptr(pcm), pcm.shape[0], 0, C.byref(h)))
            for k in seeks:
                one[0] = k
                _lib.check(lib.wis_longmel_window(h, one, 1, d_out.ptr, 1))
            lib.wis_longmel_destroy(h)
            t_long.append((time.perf_counter() - t0) * 1e3)
            t0 = time.perf_counter()
            for w in wins:
                _lib.check(lib.wis_logmel_n(0, n_mels, _lib.ptr(w), audio.N_SAMPLES, ns, 1, 0, d_out.ptr, 1))
            t_win.append((time.perf_counter() - t0) * 1e3)
            t0 = time.perf_counter()
            run("seek")
            t_seek.append((time.perf_counter() - t0) * 1e3)
            t0 = time.perf_counter()
            run("chunk")
            t_chunk.append((time.perf_counter() - t0) * 1e3)
        d_out.free()
    finally:
        model.close()
    n_chunk = sum(1 for _ in audio.chunk_iter(pcm))

    def cell(v):
        return f"{np.median(v):.2f} ({min(v):.2f} .. {max(v):.2f})"
    lines = [f"# Long-form transcription: 65 s synthetic recording, {a.size} shapes (seeded weights), {a.tokens} fixed tokens per window, beam 5",
             "",
             f"`python tools/longform_bench.py --size {a.size} --reps {a.reps} --tokens {a.tokens}`: one process, the forms alternate over {a.reps} rounds; every cell is "
             "the median of the rounds (min .. max), in ms of wall clock.  No pass mark.",
             "",
             "## front end",
             "",
             f"| | windows | ms |", "|---|---|---|",
             f"| wis_longmel_create (host PCM, {pcm.shape[0]} samples) + wis_longmel_window per seek + destroy | {n_win} | {cell(t_long)} |",
             f"| wis_logmel_n per window (host PCM of 480000 samples each) | {n_win} | {cell(t_win)} |",
             "",
             "## whole request",
             "",
             "| do_whisper | windows decoded | ms |", "|---|---|---|",
             f"| long_form=seek (seeks {seeks}) | {n_win} | {cell(t_seek)} |",
             f"| long_form=chunk | {n_chunk} | {cell(t_chunk)} |",
             "",
             "The seek loop decodes one window after the other (each needs the previous one's last timestamp and text); the chunked request decodes its "
             f"windows `concurrent_gpu_chunks` ({s.concurrent_gpu_chunks}) at a time."]
    text = "\n".join(lines) + "\n"
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)
    print(text)
    print(json.dumps({"metric": "longform_ms", "size": a.size, "windows_seek": n_win, "windows_chunk": n_chunk, "longmel_ms": round(float(np.median(t_long)), 3),
                      "logmel_windows_ms": round(float(np.median(t_win)), 3), "seek_request_ms": round(float(np.median(t_seek)), 3),
                      "chunk_request_ms": round(float(np.median(t_chunk)), 3)}))


if __name__ == "__main__":
    main()
