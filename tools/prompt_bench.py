"""What a long prompt costs: milliseconds per decode step at P = 4 (the merged-prefill route every unprompted request takes) and at P = 228 on the
long-prompt route - with dec_self_attn_long_kernel and with the TREE form of dec_self_attn_kernel in its place (what WIS_SA_LONG=0 selects) - and the
prefill time at P = 4, 64 and 228.  Seeded large-v2 weights, beam 5 and beam 1, 1 and 8 utterances, a fixed decode length (fixed_new_tokens), one process.

The forms ALTERNATE: `--reps` rounds, each running every form once (warm-up calls, then `--iters` timed calls, the round's median); the table gives the
median of the rounds' medians and their spread (min .. max).  Two forms differ only where their difference exceeds that spread.  Numbers of one run on one
box: never compare across boxes or runs.

    python tools/prompt_bench.py [--size large-v2] [--reps 5] [--iters 5] [--warmup 2] [--tokens 24] [--out profiles/prompt_ab.md]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "willow-inference-server_amd"))

START = [50258, 50259, 50359, 50363]          # <|startoftranscript|><|en|><|transcribe|><|notimestamps|>


def prompt(P):
    """<|startofprev|> + text ids + the start sequence, P tokens in all (P = 4: the start sequence alone)"""
    return START if P == 4 else [50361] + [1000 + 7 * i for i in range(P - 5)] + START


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", default="large-v2")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--tokens", type=int, default=24)
    ap.add_argument("--long-tokens", type=int, default=128, help="second decode length (beam 5 only): the suffix loop of the new kernel takes several passes")
    ap.add_argument("--long-reps", type=int, default=3)
    ap.add_argument("--out", default=None, help="write the table (markdown) here")
    a = ap.parse_args()
    import numpy as np
    from wis_hip import _lib, audio, ctranslate2 as ct2, weights as W
    pcm, _ = audio.load_audio(os.path.join(ROOT, "tests", "golden", "clips", "3sec.flac"))
    mel = audio.log_mel_spectrogram(audio.pad_or_trim(pcm)).numpy()
    model = ct2.Whisper("unused", weights=W.synthetic_weights(a.size), arch=W.arch(a.size), max_batch=8, max_beam=5)
    lib, handle = _lib.load(), model._replicas[0].handle
    # (name, prompt length, self-attention form of the long-prompt route: 1 the new kernel, 0 the TREE form, -1 not on that route)
    forms = [("P4", 4, -1), ("P228_long", 228, 1), ("P228_tree", 228, 0), ("P64_long", 64, 1), ("P64_tree", 64, 0), ("P17_long", 17, 1), ("P17_tree", 17, 0)]
    long_forms = [f for f in forms if f[0] in ("P4", "P228_long", "P228_tree", "P17_long", "P17_tree")]
    long_shapes = [(1, 5), (8, 5)]
    long_step = {(s, f[0]): [] for s in long_shapes for f in long_forms}
    shapes = [(1, 5), (8, 5), (1, 1), (8, 1)]
    step = {(s, f[0]): [] for s in shapes for f in forms}
    prefill = {(s, f[0]): [] for s in shapes for f in forms}
    try:
        for B, beam in shapes:
            feats = ct2.StorageView.from_array(np.ascontiguousarray(np.repeat(mel[None], B, axis=0)))
            for rep in range(a.reps):
                for name, P, form in forms:
                    _lib.check(lib.wis_debug_sa_long(handle, form))
                    st, pf = [], []
                    for i in range(a.warmup + a.iters):
                        model.generate(feats, [prompt(P)] * B, beam_size=beam, fixed_new_tokens=a.tokens)
                        t = model.last_timing()
                        if i >= a.warmup:
                            st.append(t["decode_ms"] / max(1, t["decode_steps"] - 1))      # (the prefill + first step is not a decode step)
                            pf.append(t["prefill_ms"])
                    step[((B, beam), name)].append(float(np.median(st)))
                    prefill[((B, beam), name)].append(float(np.median(pf)))
        for B, beam in long_shapes:      # the same at a transcript of --long-tokens tokens: histories of up to P + 128 positions
            feats = ct2.StorageView.from_array(np.ascontiguousarray(np.repeat(mel[None], B, axis=0)))
            for rep in range(a.long_reps):
                for name, P, form in long_forms:
                    _lib.check(lib.wis_debug_sa_long(handle, form))
                    st = []
                    for i in range(1 + 3):
                        model.generate(feats, [prompt(P)] * B, beam_size=beam, fixed_new_tokens=a.long_tokens)
                        t = model.last_timing()
                        if i >= 1:
                            st.append(t["decode_ms"] / max(1, t["decode_steps"] - 1))
                    long_step[((B, beam), name)].append(float(np.median(st)))
        _lib.check(lib.wis_debug_sa_long(handle, -1))
    finally:
        model.close()

    def cell(v):
        return f"{np.median(v):.3f} ({min(v):.3f} .. {max(v):.3f})"
    lines = [f"# Prompted decoding: decode step and prefill, {a.size} (seeded weights), {a.tokens} fixed tokens",
             "",
             f"`python tools/prompt_bench.py --size {a.size} --reps {a.reps} --iters {a.iters} --warmup {a.warmup} --tokens {a.tokens}`: one process, the forms alternate over "
             f"{a.reps} rounds; every cell is the median of the rounds' medians (min .. max of them), in ms.",
             "",
             "## ms per decode step",
             "",
             "| utterances x beam | P = 4 (merged prefill route) | P = 228, dec_self_attn_long_kernel | P = 228, TREE form (WIS_SA_LONG=0) | long kernel - TREE |",
             "|---|---|---|---|---|"]
    res = {}
    for s in shapes:
        lo, tr = step[(s, "P228_long")], step[(s, "P228_tree")]
        diff = float(np.median(lo) - np.median(tr))
        spread = max(max(lo) - min(lo), max(tr) - min(tr))
        verdict = "within the spread" if abs(diff) <= spread else ("long kernel faster" if diff < 0 else "TREE form faster")
        lines.append(f"| {s[0]} x {s[1]} | {cell(step[(s, 'P4')])} | {cell(lo)} | {cell(tr)} | {diff:+.3f} (spread {spread:.3f}): {verdict} |")
        res[f"B{s[0]}_beam{s[1]}"] = {n: round(float(np.median(step[(s, n)])), 4) for n, _, _ in forms}
    def versus(lo, tr):
        diff = float(np.median(lo) - np.median(tr))
        spread = max(max(lo) - min(lo), max(tr) - min(tr))
        return f"{diff:+.3f} (spread {spread:.3f}): " + ("within the spread" if abs(diff) <= spread else ("long kernel faster" if diff < 0 else "TREE form faster"))
    lines += ["", "## ms per decode step at shorter prompts (the kernel always requests 256 prefix positions)", "",
              "| utterances x beam | P = 17, long kernel | P = 17, TREE form | long - TREE | P = 64, long kernel | P = 64, TREE form | long - TREE |", "|---|---|---|---|---|---|---|"]
    for s in shapes:
        lines.append(f"| {s[0]} x {s[1]} | {cell(step[(s, 'P17_long')])} | {cell(step[(s, 'P17_tree')])} | {versus(step[(s, 'P17_long')], step[(s, 'P17_tree')])} | "
                     f"{cell(step[(s, 'P64_long')])} | {cell(step[(s, 'P64_tree')])} | {versus(step[(s, 'P64_long')], step[(s, 'P64_tree')])} |")
    lines += ["", f"## ms per decode step over {a.long_tokens} fixed tokens ({a.long_reps} rounds): the suffix loop of the new kernel takes up to {(a.long_tokens + 31) // 32} passes", "",
              "| utterances x beam | P = 4 | P = 17, long kernel | P = 17, TREE form | long - TREE | P = 228, long kernel | P = 228, TREE form | long - TREE |", "|---|---|---|---|---|---|---|---|"]
    for s in long_shapes:
        L = lambda n: long_step[(s, n)]
        lines.append(f"| {s[0]} x {s[1]} | {cell(L('P4'))} | {cell(L('P17_long'))} | {cell(L('P17_tree'))} | {versus(L('P17_long'), L('P17_tree'))} | "
                     f"{cell(L('P228_long'))} | {cell(L('P228_tree'))} | {versus(L('P228_long'), L('P228_tree'))} |")
    lines += ["", "## prefill_ms (everything between the cross-K/V projection and the end of the first sampling tail)", "",
              "| utterances x beam | P = 4 | P = 64 | P = 228 |", "|---|---|---|---|"]
    for s in shapes:
        lines.append(f"| {s[0]} x {s[1]} | {cell(prefill[(s, 'P4')])} | {cell(prefill[(s, 'P64_long')])} | {cell(prefill[(s, 'P228_long')] + prefill[(s, 'P228_tree')])} |")
    text = "\n".join(lines) + "\n"
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)
    print(text)
    print(json.dumps({"metric": "decode_step_ms", "size": a.size, "tokens": a.tokens, "shapes": res}))


if __name__ == "__main__":
    main()
