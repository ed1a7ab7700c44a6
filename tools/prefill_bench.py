"""What the one-pass prefix route buys: prefill_ms and the whole call of a 24-token generate at P = 17, 64 and 228, 1 and 8 utterances, beam 5, seeded
large-v2 weights - the SAME handle in both modes (wis_model_set_prefill 0 / 1), alternating call by call in one process.  At 8 utterances only prompts of up
to 48 tokens fit the route's 256 prefix rows: P = 64 and 228 fall back there, and the table says so instead of hiding the rows.

`--reps` rounds; a round runs warm-up calls and then `--iters` timed PAIRS (windowed, one-pass); every cell is the median of the rounds' medians and
(min .. max) of them.  Two modes differ only where their difference exceeds that spread.  Numbers of one run on one box.

    python tools/prefill_bench.py [--size large-v2] [--reps 5] [--iters 5] [--warmup 2] [--tokens 24] [--out profiles/prefill_one_pass_ab.md]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "willow-inference-server_amd"))

START = [50258, 50259, 50359, 50363]
MODES = ("windowed", "one_pass")


def prompt(P):
    return START if P == 4 else [50361] + [1000 + 7 * i for i in range(P - 5)] + START


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", default="large-v2")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--tokens", type=int, default=24)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import numpy as np
    from wis_hip import _lib, audio, ctranslate2 as ct2, weights as W
    pcm, _ = audio.load_audio(os.path.join(ROOT, "tests", "golden", "clips", "3sec.flac"))
    mel = audio.log_mel_spectrogram(audio.pad_or_trim(pcm)).numpy()
    arch = W.arch(a.size)
    model = ct2.Whisper("unused", weights=W.synthetic_weights(a.size), arch=arch, max_batch=8, max_beam=5)
    lib, handle = _lib.load(), model._replicas[0].handle
    cases = [(B, P) for B in (1, 8) for P in (17, 64, 228)]
    pre = {(c, m): [] for c in cases for m in MODES}
    tot = {(c, m): [] for c in cases for m in MODES}
    try:
        for B, P in cases:
            feats = ct2.StorageView.from_array(np.ascontiguousarray(np.repeat(mel[None], B, axis=0)))
            for rep in range(a.reps):
                p, t = {m: [] for m in MODES}, {m: [] for m in MODES}
                for i in range(a.warmup + a.iters):
                    for mode in MODES:
                        _lib.check(lib.wis_model_set_prefill(handle, MODES.index(mode)))
                        model.generate(feats, [prompt(P)] * B, beam_size=5, fixed_new_tokens=a.tokens)
                        tm = model.last_timing()
                        if i >= a.warmup:
                            p[mode].append(tm["prefill_ms"]); t[mode].append(tm["total_ms"])
                for mode in MODES:
                    pre[((B, P), mode)].append(float(np.median(p[mode]))); tot[((B, P), mode)].append(float(np.median(t[mode])))
        _lib.check(lib.wis_model_set_prefill(handle, 0))
    finally:
        model.close()

    def cell(v):
        return f"{np.median(v):.2f} ({min(v):.2f} .. {max(v):.2f})"
    # the floor of the prefix pass: every decoder matrix but the last layer's tail read once (f16)
    d, L = arch["d_model"], arch["n_layers"]
    floor_bytes = (12 * d * d * (L - 1) + 3 * d * d) * 2
    lines = [f"# One-pass prefill of long prompts: A/B, {a.size} (seeded weights), beam 5, {a.tokens} fixed tokens", "",
             f"`python tools/prefill_bench.py --size {a.size} --reps {a.reps} --iters {a.iters} --warmup {a.warmup} --tokens {a.tokens}`: one handle, the two modes alternate "
             f"call by call; cells are the median of {a.reps} rounds' medians (min .. max), in ms.  prefill_ms = everything between the cross-K/V projection and the end of "
             "the first sampling tail (the last 16 prompt rows and the first step included in both modes).", "",
             "| utterances | P | prefix rows | route taken | prefill_ms windowed | prefill_ms one-pass | total_ms windowed | total_ms one-pass |", "|---|---|---|---|---|---|---|---|"]
    res = {}
    for B, P in cases:
        rows = B * (P - min(16, 96 // B))
        took = "one pass" if rows <= 256 else "falls back (more than 256 rows)"
        lines.append(f"| {B} | {P} | {rows} | {took} | {cell(pre[((B, P), 'windowed')])} | {cell(pre[((B, P), 'one_pass')])} | {cell(tot[((B, P), 'windowed')])} | {cell(tot[((B, P), 'one_pass')])} |")
        res[f"B{B}_P{P}"] = {m: round(float(np.median(pre[((B, P), m)])), 3) for m in MODES}
    lines += ["", f"The prefix pass reads {floor_bytes / 1e9:.2f} GB of decoder weights once (the last layer stops behind its QKV projection)."]
    text = "\n".join(lines) + "\n"
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)
    print(text)
    print(json.dumps({"metric": "prefill_ms", "size": a.size, "cases": res}))


if __name__ == "__main__":
    main()
