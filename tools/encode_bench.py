"""The encode_once setting, off against on: do_whisper on the 3.84 s clip at beam 5 with seeded large-v2 and large-v3-turbo weights, the two sides in
alternating pairs in one process (`--rounds` repeated medians of `--iters` pairs each give the spread), for the requests

    a  detect_language                                   d  a fallback forced through three temperatures (an unreachable logprob_threshold)
    b  word_timestamps                                   e  the plain one-pass request
    c  detect_language + translate + word_timestamps

with the encoder passes counted on each side (wis_encode calls + engine calls that were handed features).  Then `encode` alone at B = 1 and 8
(wall; the call synchronises the handle's stream), `generate` from a view against `generate` from features at B = 1 and 8 (separately encoded views: the
B = 8 call gathers eight blocks device-to-device), and the gather alone.

    python tools/encode_bench.py [--sizes large-v2,large-v3-turbo] [--iters 7] [--rounds 3] [--warmup 2]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "willow-inference-server_amd"))

REQUESTS = {
    "a_detect": dict(detect_language=True, force_language=None),
    "b_words": dict(word_timestamps=True),
    "c_detect_translate_words": dict(detect_language=True, force_language=None, translate=True, word_timestamps=True),
    "d_fallback_3_temperatures": dict(temperatures=(0.0, 0.4, 0.8), best_of=2, logprob_threshold=100.0),
    "e_plain": dict(),
}


class Vocab:
    """stand-in vocabulary: one word per text token"""
    has_vocabulary, all_special_ids = True, []
    decode = staticmethod(lambda ids: "".join(f" w{int(t)}" for t in ids if int(t) < 50257))


class Passes:
    """encoder passes: wis_encode calls, and every other engine call that was handed features instead of encoder output"""

    def __init__(self, ct2, model):
        from wis_hip import _lib
        self.n, self.ct2, self.model = 0, ct2, model
        enc_kinds = (_lib.WIS_IN_ENC_DEV, _lib.WIS_IN_ENC_HOST)
        self.saved = ct2._generate_chunk, ct2._encode_chunk, model.detect_language, model.align
        gen, enc, det, al = self.saved

        def count(by):
            self.n += by
        ct2._generate_chunk = lambda r, mel, prompts, opts, **kw: (count(opts.input_kind not in enc_kinds), gen(r, mel, prompts, opts, **kw))[1]
        ct2._encode_chunk = lambda *a, **kw: (count(1), enc(*a, **kw))[1]
        seen = lambda f, kw: model._encoder_input(f, kw.get("input_kind", _lib.WIS_IN_MEL_HOST)) is None
        model.detect_language = lambda f, **kw: (count(seen(f, kw)), det(f, **kw))[1]
        model.align = lambda f, *a, **kw: (count(seen(f, kw)), al(f, *a, **kw))[1]

    def close(self):
        self.ct2._generate_chunk, self.ct2._encode_chunk = self.saved[:2]
        del self.model.detect_language, self.model.align


def do_whisper_rows(a, label, pcm, out):
    import numpy as np
    size = "large" if label == "large-v2" else label      # (the model registry's name of large-v2)
    from wis_hip import ctranslate2 as ct2
    from wis_hip.settings import APISettings
    from wis_hip.whisper import WhisperModels, do_whisper
    st = APISettings()
    st.whisper_model_path, st.fixed_new_tokens = "synthetic:{size}", 24
    models = WhisperModels(st, device_index=[0])
    model = models.get(size)
    models.tokenizers[size] = Vocab()
    spy = Passes(ct2, model)
    try:
        for name, kw in REQUESTS.items():
            kw = dict(dict(detect_language=False, force_language="en"), **kw)
            det, force = kw.pop("detect_language"), kw.pop("force_language")

            def run(on):
                st.encode_once = on
                spy.n = 0
                ct2.set_random_seed(5)
                t0 = time.perf_counter()
                do_whisper(pcm, size, 5, "transcribe", det, force, models=models, **kw)
                return (time.perf_counter() - t0) * 1e3
            for _ in range(a.warmup):
                run(False), run(True)
            meds, passes = {False: [], True: []}, {}
            for _ in range(a.rounds):
                ms = {False: [], True: []}
                for _ in range(a.iters):
                    for on in (False, True):      # alternating pairs
                        ms[on].append(run(on))
                        passes[on] = spy.n
                for on in (False, True):
                    meds[on].append(float(np.median(ms[on])))
            row = {}
            for on, side in ((False, "off"), (True, "on")):
                row[side + "_ms"] = round(float(np.median(meds[on])), 3)
                row[side + "_spread_ms"] = round(max(meds[on]) - min(meds[on]), 3)
                row[side + "_encoder_passes"] = passes[on]
            out[f"{label}_{name}"] = row
    finally:
        st.encode_once = False
        ct2.set_random_seed(None)
        spy.close()
        model.close()


def call_rows(a, size, pcm, out):
    import ctypes as C
    import numpy as np
    from wis_hip import _lib, audio, ctranslate2 as ct2, weights as W
    arch = W.arch(size)
    model = ct2.Whisper("unused", weights=W.synthetic_weights(size), arch=arch, max_batch=8, max_beam=5)
    st = model.special
    prompt = [st.sot, st.lang_ids[0], st.transcribe, st.notimestamps]
    mel = audio.log_mel_spectrogram(audio.pad_or_trim(pcm), n_mels=arch["n_mels"]).numpy()

    def med(fn):
        ms = []
        for i in range(a.warmup + a.iters * a.rounds):
            t0 = time.perf_counter()
            fn()
            if i >= a.warmup:
                ms.append((time.perf_counter() - t0) * 1e3)
        return round(float(np.median(ms)), 3)
    try:
        for B in (1, 8):
            x = ct2.StorageView.from_array(np.ascontiguousarray(np.repeat(mel[None], B, axis=0)))
            row = {"encode_ms": med(lambda: model.encode(x))}
            one = model.encode(x)
            parts = [model.encode(ct2.StorageView.from_array(np.ascontiguousarray(mel[None]))) for _ in range(B)]
            kw = dict(beam_size=5, fixed_new_tokens=24)
            row["generate_from_features_ms"] = med(lambda: model.generate(x, [prompt] * B, **kw))
            row["generate_from_one_view_ms"] = med(lambda: model.generate(one, [prompt] * B, **kw))
            row["generate_from_separate_views_ms"] = med(lambda: model.generate(parts, [prompt] * B, **kw))
            t = model.last_timing()
            row["from_view_logmel_encoder_crosskv_ms"] = [round(t[k], 3) for k in ("logmel_ms", "encoder_ms", "crosskv_ms")]
            r = model._replicas[0]
            ptrs = [p.device_ptr for p in parts]
            if B > 1:
                row["gather_alone_ms"] = med(lambda: ct2._gather_device_rows(r, ptrs, r.enc_bytes))
            out[f"{size}_B{B}"] = row
    finally:
        model.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="large-v2,large-v3-turbo")
    ap.add_argument("--iters", type=int, default=7)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    from wis_hip import audio
    pcm = audio.load_audio(os.path.join(ROOT, "tests", "golden", "clips", "3sec.flac"))[0]
    e2e, calls = {}, {}
    for size in a.sizes.split(","):
        do_whisper_rows(a, size, pcm, e2e)
        call_rows(a, size, pcm, calls)
    print(json.dumps({"metric": "encode_once_ms", "do_whisper_24_tokens": e2e, "calls": calls}))


if __name__ == "__main__":
    main()
