"""Milliseconds of one word-alignment call (ctranslate2.Whisper.align -> wis_align) split into its phases - encoder + cross K/V, the
teacher-forced decoder passes, attention weights, normalise + median filter, DTW (GPU events, wis_align_last_timing) - beside the
plain `timestamps` generate call it follows in do_whisper, with seeded large-v2 (the 320-head default) and large-v3-turbo weights on
the 3.84 s and 29.2 s clips; then do_whisper with `timestamps` and with `word_timestamps` on both clips (a stand-in vocabulary: one
word per token).  The generate call beside an n-token align decodes min(n, 200) tokens (fixed_new_tokens): at 223 tokens it is 10 %
shorter than the text aligned.

    python tools/align_bench.py [--sizes large-v2,large-v3-turbo] [--iters 10] [--warmup 3] [--tokens 24,223]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "willow-inference-server_amd"))


class Vocab:
    """stand-in vocabulary: one word per text token"""
    has_vocabulary, all_special_ids = True, []
    decode = staticmethod(lambda ids: "".join(f" w{int(t)}" for t in ids if int(t) < 50257))


def align_rows(a, size, clips, res):
    import numpy as np
    from wis_hip import _lib, audio, ctranslate2 as ct2, weights as W
    arch = W.arch(size)
    model = ct2.Whisper("unused", weights=W.synthetic_weights(size), arch=arch, max_batch=8, max_beam=5)
    st = model.special
    start = [st.sot, st.lang_ids[0], st.transcribe]
    rng = np.random.default_rng(0)
    try:
        for clip, pcm in clips.items():
            num_frames = min(3000, -(-pcm.shape[0] // audio.HOP_LENGTH))
            mel = audio.log_mel_spectrogram(audio.pad_or_trim(pcm), n_mels=arch["n_mels"]).numpy()
            feats = ct2.StorageView.from_array(np.ascontiguousarray(mel[None]))
            for n in [int(t) for t in a.tokens.split(",")]:
                text = rng.integers(0, 50000, size=n).tolist()
                gen_ms, wall_ms, phases = [], [], []
                for i in range(a.warmup + a.iters):
                    t0 = time.perf_counter()
                    model.generate(feats, [start], beam_size=5, fixed_new_tokens=min(n, 200))
                    t1 = time.perf_counter()
                    model.align(feats, start, [text], [num_frames])
                    t2 = time.perf_counter()
                    ms = (C.c_float * 6)()
                    _lib.check(_lib.load().wis_align_last_timing(model._replicas[0].handle, ms))
                    if i >= a.warmup:
                        gen_ms.append((t1 - t0) * 1e3), wall_ms.append((t2 - t1) * 1e3), phases.append(list(ms))
                p = np.median(np.asarray(phases), axis=0)
                res[f"{size}_{clip}_{n}tok"] = {
                    "heads": len(model.alignment_heads) or arch["n_heads"] * (arch["n_dec_layers"] - arch["n_dec_layers"] // 2),
                    "timestamps_generate_ms": round(float(np.median(gen_ms)), 3), "generate_tokens": min(n, 200), "align_ms": round(float(np.median(wall_ms)), 3),
                    "encode_ms": round(float(p[0]), 3), "decoder_pass_ms": round(float(p[1]), 3), "attention_weights_ms": round(float(p[4]), 3),
                    "normalise_filter_ms": round(float(p[5]), 3), "dtw_ms": round(float(p[3]), 3)}
    finally:
        model.close()


def do_whisper_rows(a, size, clips, e2e):
    import numpy as np
    label, size = size, ("large" if size == "large-v2" else size)      # (the model registry's name of large-v2)
    from wis_hip.settings import APISettings
    from wis_hip.whisper import WhisperModels, do_whisper
    st = APISettings()
    st.whisper_model_path, st.fixed_new_tokens = "synthetic:{size}", 24
    models = WhisperModels(st, device_index=[0])
    models.get(size)
    models.tokenizers[size] = Vocab()
    try:
        for clip, pcm in clips.items():
            row = {}
            for name, kw in (("timestamps", dict(timestamps=True)), ("word_timestamps", dict(word_timestamps=True))):
                ms = []
                for i in range(a.warmup + a.iters):
                    t0 = time.perf_counter()
                    do_whisper(pcm, size, 5, models=models, **kw)
                    if i >= a.warmup:
                        ms.append((time.perf_counter() - t0) * 1e3)
                row[name + "_ms"] = round(float(np.median(ms)), 3)
            e2e[f"{label}_{clip}"] = row
    finally:
        models.get(size).close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="large-v2,large-v3-turbo")
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--tokens", default="24,223")
    a = ap.parse_args()
    from wis_hip import audio
    clips = {n: audio.load_audio(os.path.join(ROOT, "tests", "golden", "clips", n + ".flac"))[0] for n in ("3sec", "30sec")}
    res, e2e = {}, {}
    for size in a.sizes.split(","):
        align_rows(a, size, clips, res)
        do_whisper_rows(a, size, clips, e2e)
    print(json.dumps({"metric": "align_ms", "shapes": res, "do_whisper_24_tokens": e2e}))


if __name__ == "__main__":
    main()
