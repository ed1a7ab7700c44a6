"""What the in-grammar mass of phrase-constrained decoding costs (wis_gen_opts_t::phrase_mass: phrase_rules_mass_kernel in phrase_rules_kernel's
place in every step, phrase_mass_gather_kernel and a copy behind the search), at the headline shape (large-v2, seeded weights, beam 5, the 3.84 s
clip) and at 8 utterances x beam 5, in one process, in tools/phrase_bench.py's shape: 24-token phrases, so every search takes 25 passes.

Per shape and phrase set (about 20 phrases; about 2000 with 300 different first tokens):
  step_ms      the decode step with phrases on, without and with the mass (medians of repeated medians, their spread beside them), and the difference
  call_ms      the whole call by the engine's own clock (total_ms), without and with the mass
  gather_ms    the end-of-call part alone: wis_op_phrase_mass_gather on B x 5 results of 24 tokens (launch + synchronise, wall clock), and
  copy_ms      wis_last_phrase_mass behind a finished call (the copy of B x n floats and the stream synchronisation, wall clock)
No pass mark.

    python tools/phrase_mass_bench.py [--size large-v2] [--iters 10] [--warmup 3] [--repeats 3] [--tokens 24]
    rocprofv3 --kernel-trace --stats -d OUT -o mass -- python tools/phrase_mass_bench.py --iters 5 --repeats 1      # the kernels' own times
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "willow-inference-server_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from phrase_bench import PROMPT, phrase_sets  # noqa: E402


def gather_ms(phrases, B, n, iters):
    """wall clock of one wis_op_phrase_mass_gather call (launch + synchronise) over B x n results that are phrases of the set"""
    import numpy as np
    from wis_hip import _lib, weights as W
    lib = _lib.load()
    trie = W.build_phrase_trie(phrases)
    L = len(phrases[0])
    ids = np.asarray([phrases[i % len(phrases)] for i in range(B * n)], np.int32)
    arrs = [ids, np.full(B * n, L, np.int32), trie, np.zeros((B, len(trie)), np.float32), np.zeros(B * n, np.float32)]
    bufs = [_lib.DevBuf.from_numpy(np.ascontiguousarray(x)) for x in arrs]
    try:
        t = []
        for _ in range(iters + 3):
            t0 = time.perf_counter()
            _lib.check(lib.wis_op_phrase_mass_gather(0, bufs[0].ptr, bufs[1].ptr, None, bufs[2].ptr, len(trie), bufs[3].ptr, B, n, L, bufs[4].ptr))
            t.append((time.perf_counter() - t0) * 1e3)
        return float(np.median(t[3:]))
    finally:
        for b in bufs:
            b.free()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", default="large-v2")
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--tokens", type=int, default=24)
    a = ap.parse_args()
    if not 1 <= a.tokens <= 32:
        ap.error("--tokens: 1..32 (a phrase holds at most 32 tokens)")
    import numpy as np
    from wis_hip import _lib, audio, ctranslate2 as ct2, weights as W
    pcm, _ = audio.load_audio(os.path.join(ROOT, "tests", "golden", "clips", "3sec.flac"))
    mel = audio.log_mel_spectrogram(audio.pad_or_trim(pcm)).numpy()
    sets = phrase_sets(a.tokens)
    model = ct2.Whisper("unused", weights=W.synthetic_weights(a.size), arch=W.arch(a.size), max_batch=8, max_beam=5)
    forms = [(f"{k}_{m}", dict(phrases=v, return_phrase_mass=(m == "mass"))) for k, v in sets.items() for m in ("plain", "mass")]
    res = {}
    try:
        lib, h = _lib.load(), model._replicas[0].handle
        for B in (1, 8):
            feats = ct2.StorageView.from_array(np.ascontiguousarray(np.repeat(mel[None], B, axis=0)))
            meds, calls, copies = {n: [] for n, _ in forms}, {n: [] for n, _ in forms}, []
            for _ in range(a.repeats):
                for name, kw in forms:      # (the forms alternate inside a repeat: drift of the clocks hits them alike)
                    step_ms, call_ms = [], []
                    for i in range(a.warmup + a.iters):
                        model.generate(feats, [PROMPT] * B, beam_size=5, **kw)
                        t = model.last_timing()
                        if i >= a.warmup:
                            step_ms.append(t["decode_ms"] / max(1, t["decode_steps_needed"] - 1))      # (the merged prefill + first step is not a decode step)
                            call_ms.append(t["total_ms"])
                            if kw["return_phrase_mass"]:
                                out = np.zeros((B, 1), np.float32)
                                t0 = time.perf_counter()
                                _lib.check(lib.wis_last_phrase_mass(h, B, 1, out.ctypes.data_as(C.POINTER(C.c_float))))
                                copies.append((time.perf_counter() - t0) * 1e3)
                    meds[name].append(float(np.median(step_ms)))
                    calls[name].append(float(np.median(call_ms)))
            row = {}
            for k, v in sets.items():
                p, m = meds[f"{k}_plain"], meds[f"{k}_mass"]
                row[k] = dict(step_ms=round(float(np.median(p)), 4), step_ms_mass=round(float(np.median(m)), 4),
                              spread_ms=round(max(max(p) - min(p), max(m) - min(m)), 4), delta_ms=round(float(np.median(m)) - float(np.median(p)), 4),
                              call_ms=round(float(np.median(calls[f"{k}_plain"])), 3), call_ms_mass=round(float(np.median(calls[f"{k}_mass"])), 3),
                              gather_ms=round(gather_ms(v, B, 5, a.iters), 4))
            row["copy_ms"] = round(float(np.median(copies)), 4)
            res[f"B{B}_beam5"] = row
    finally:
        model.close()
    print(json.dumps({"metric": "phrase_mass_cost_ms", "size": a.size, "tokens": a.tokens, "repeats": a.repeats, "shapes": res}))


if __name__ == "__main__":
    main()
