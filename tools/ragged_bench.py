"""Prompts of different lengths in one device batch (wis_generate_ragged): what the batch costs against the same requests decoded one after the other,
and that uniform calls cost what they cost before.  Seeded large-v2 weights, the 3.84 s clip, beam 5, a fixed decode length (fixed_new_tokens), one GPU.

(a), (c)  one process, the forms ALTERNATE over `--reps` rounds (warm-up calls, then `--iters` timed calls, the round's median); a cell is the median of
          the rounds' medians with their spread (min .. max):
            ragged     eight utterances with prompts of 20, 45, 70, 100, 130, 170, 200 and 228 tokens in ONE call (ragged_prompts=True)
            singles    the same eight as eight single calls, one after the other - what the micro-batcher does with them while their keys differ
            uniform    eight utterances with the 228-token prompt: the same step graph as `ragged` replays
          per form: ms per decode step, prefill_ms, and the whole call on the host's clock (singles: the sum over the eight calls).
(b)       `--ab TREE`: the uniform step (P = 4 and P = 228 at one and eight utterances) of this tree against another checkout's (the parent commit, built),
          in alternating PAIRS of child processes (`--pairs`); a cell is the median of the processes' medians with their spread.

    python tools/ragged_bench.py [--reps 5] [--iters 5] [--warmup 2] [--tokens 24] [--ab PARENT_TREE --pairs 3] [--out profiles/ragged_prompt_ab.md]

Numbers of one run on one box: never compare across boxes or runs."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
START = [50258, 50259, 50359, 50363]          # <|startoftranscript|><|en|><|transcribe|><|notimestamps|>
LENGTHS = (20, 45, 70, 100, 130, 170, 200, 228)


def prompt(P):
    """<|startofprev|> + text ids + the start sequence, P tokens in all (P = 4: the start sequence alone)"""
    return START if P == 4 else [50361] + [1000 + 7 * i for i in range(P - 5)] + START


def load(tree, size):
    """-> (numpy, ctranslate2 shim, model, mel of the clip) from the checkout at `tree`"""
    sys.path.insert(0, os.path.join(tree, "willow-inference-server_amd"))
    import numpy as np
    from wis_hip import audio, ctranslate2 as ct2, weights as W
    pcm, _ = audio.load_audio(os.path.join(ROOT, "tests", "golden", "clips", "3sec.flac"))
    mel = audio.log_mel_spectrogram(audio.pad_or_trim(pcm)).numpy()
    model = ct2.Whisper("unused", weights=W.synthetic_weights(size), arch=W.arch(size), max_batch=8, max_beam=5)
    return np, ct2, model, mel


def timed(model, call):
    """one call -> (ms per decode step, prefill_ms, the call on the host's clock in ms)"""
    t0 = time.perf_counter()
    call()
    wall = (time.perf_counter() - t0) * 1e3
    t = model.last_timing()
    return t["decode_ms"] / max(1, t["decode_steps"] - 1), t["prefill_ms"], wall


def uniform_child(a):
    """the uniform step of the checkout `a.tree`: one JSON line {form: median ms per step}"""
    np, ct2, model, mel = load(a.tree, a.size)
    out = {}
    try:
        for B in (1, 8):
            feats = ct2.StorageView.from_array(np.ascontiguousarray(np.repeat(mel[None], B, axis=0)))
            for P in (4, 228):
                st = []
                for i in range(a.warmup + a.iters):
                    s, _, _ = timed(model, lambda: model.generate(feats, [prompt(P)] * B, beam_size=5, fixed_new_tokens=a.tokens))
                    if i >= a.warmup:
                        st.append(s)
                out[f"P{P}x{B}"] = float(np.median(st))
    finally:
        model.close()
    print("UNIFORM " + json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", default="large-v2")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--tokens", type=int, default=24)
    ap.add_argument("--ab", default=None, help="another checkout of the project (built): the uniform step of both, in alternating pairs of processes")
    ap.add_argument("--pairs", type=int, default=3)
    ap.add_argument("--skip-ragged", action="store_true", help="only the --ab part")
    ap.add_argument("--uniform-child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--tree", default=ROOT, help=argparse.SUPPRESS)
    ap.add_argument("--out", default=None, help="write the tables (markdown) here")
    a = ap.parse_args()
    if a.uniform_child:
        return uniform_child(a)
    import numpy as np

    def cell(v, digits=3):
        return f"{np.median(v):.{digits}f} ({min(v):.{digits}f} .. {max(v):.{digits}f})"
    lines = [f"# Prompts of different lengths in one device batch, {a.size} (seeded weights), beam 5, {a.tokens} fixed tokens, the 3.84 s clip", ""]
    res = {}
    if not a.skip_ragged:
        _, ct2, model, mel = load(ROOT, a.size)
        forms = ("ragged", "singles", "uniform")
        step, prefill, wall = ({f: [] for f in forms} for _ in range(3))
        feats8 = ct2.StorageView.from_array(np.ascontiguousarray(np.repeat(mel[None], 8, axis=0)))
        feats1 = ct2.StorageView.from_array(np.ascontiguousarray(mel[None]))
        ragged_prompts = [prompt(P) for P in LENGTHS]
        kw = dict(beam_size=5, fixed_new_tokens=a.tokens)

        def run(form):
            """-> (ms per decode step, prefill_ms, host ms) of one round's call (singles: mean step, summed prefill, summed host time of the eight)"""
            if form == "ragged":
                return timed(model, lambda: model.generate(feats8, ragged_prompts, ragged_prompts=True, **kw))
            if form == "uniform":
                return timed(model, lambda: model.generate(feats8, [prompt(228)] * 8, **kw))
            parts = [timed(model, lambda p=p: model.generate(feats1, [p], **kw)) for p in ragged_prompts]
            return float(np.mean([x[0] for x in parts])), float(np.sum([x[1] for x in parts])), float(np.sum([x[2] for x in parts]))
        try:
            for rep in range(a.reps):
                for form in forms:
                    got = [run(form) for _ in range(a.warmup + a.iters)][a.warmup:]
                    step[form].append(float(np.median([g[0] for g in got])))
                    prefill[form].append(float(np.median([g[1] for g in got])))
                    wall[form].append(float(np.median([g[2] for g in got])))
        finally:
            model.close()
        lines += [f"`python tools/ragged_bench.py --reps {a.reps} --iters {a.iters} --warmup {a.warmup} --tokens {a.tokens}`: one process, the forms alternate over {a.reps} "
                  "rounds; every cell is the median of the rounds' medians (min .. max of them), in ms.", "",
                  f"## (a), (c) eight prompted requests of {', '.join(str(P) for P in LENGTHS)} prompt tokens", "",
                  "| form | ms per decode step | prefill_ms | whole call, host clock |", "|---|---|---|---|",
                  f"| one ragged call of eight | {cell(step['ragged'])} | {cell(prefill['ragged'], 2)} | {cell(wall['ragged'], 2)} |",
                  f"| eight single calls, one after the other (step: their mean; prefill and call: their sum) | {cell(step['singles'])} | {cell(prefill['singles'], 2)} | {cell(wall['singles'], 2)} |",
                  f"| one uniform call of eight, P = 228 | {cell(step['uniform'])} | {cell(prefill['uniform'], 2)} | {cell(wall['uniform'], 2)} |", ""]
        diff = float(np.median(step["ragged"]) - np.median(step["uniform"]))
        spread = max(max(step[f]) - min(step[f]) for f in ("ragged", "uniform"))
        lines += [f"Ragged step - uniform P = 228 step at eight utterances: {diff:+.3f} ms (spread {spread:.3f}): " + ("within the spread" if abs(diff) <= spread else "beyond the spread"),
                  f"Eight single calls take {np.median(wall['singles']) / np.median(wall['ragged']):.2f} x the host time of the one ragged call "
                  f"({a.tokens} steps each; the singles' {a.tokens} x 8 steps at {np.median(step['singles']):.3f} ms against {a.tokens} steps at {np.median(step['ragged']):.3f} ms).", ""]
        res["ragged"] = {f: dict(step_ms=round(float(np.median(step[f])), 4), prefill_ms=round(float(np.median(prefill[f])), 3), call_ms=round(float(np.median(wall[f])), 3)) for f in forms}
    if a.ab:
        sides = {"this tree": ROOT, "other tree": os.path.abspath(a.ab)}
        got = {s: [] for s in sides}
        for pair in range(a.pairs):
            for side, tree in sides.items():
                p = subprocess.run([sys.executable, os.path.abspath(__file__), "--uniform-child", "--tree", tree, "--size", a.size, "--iters", str(a.iters), "--warmup", str(a.warmup),
                                    "--tokens", str(a.tokens)], capture_output=True, text=True, timeout=900)
                if p.returncode != 0:
                    sys.stderr.write(p.stderr[-3000:])
                    raise SystemExit(f"uniform child of {side} failed ({p.returncode})")
                got[side].append(json.loads(next(l for l in p.stdout.splitlines() if l.startswith("UNIFORM "))[8:]))
                print(f"pair {pair} {side}: {got[side][-1]}", flush=True)
        lines += [f"## (b) the uniform step, this tree against `{a.ab}` ({a.pairs} alternating pairs of processes; median of the processes' medians, min .. max), ms per decode step", "",
                  "| form | this tree | other tree | difference | spread |", "|---|---|---|---|---|"]
        for form in ("P4x1", "P4x8", "P228x1", "P228x8"):
            new, old = [g[form] for g in got["this tree"]], [g[form] for g in got["other tree"]]
            diff, spread = float(np.median(new) - np.median(old)), max(max(new) - min(new), max(old) - min(old))
            lines.append(f"| P = {form[1:].split('x')[0]}, {form.split('x')[1]} utterance(s) | {cell(new, 4)} | {cell(old, 4)} | {diff:+.4f} | {spread:.4f}: "
                         + ("within the spread" if abs(diff) <= spread else "beyond the spread") + " |")
            res[form] = dict(this=round(float(np.median(new)), 4), other=round(float(np.median(old)), 4))
        lines.append("")
    text = "\n".join(lines) + "\n"
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)
    print(text)
    print(json.dumps({"metric": "ragged_prompt_ms", "size": a.size, "tokens": a.tokens, "results": res}))


if __name__ == "__main__":
    main()
