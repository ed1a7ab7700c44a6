"""Milliseconds per decode step with hotword boosting off and on (hotword_rules_kernel behind rep_rules_kernel in the sampling tail of every step
graph), at the headline shape (large-v2, seeded weights, beam 5, the 3.84 s clip) and at 8 utterances x beam 5, in one process - and, in the SAME
run, phrase_rules_kernel's small-set "on" case (tools/phrase_bench.py's) for comparison.

Two hotword sets of entries of 1 .. 8 tokens: about 20 entries, and about 2000 entries with more than 256 different first tokens (the root's
children are boosted in more than one round of 256).  Every form takes the same number of passes: the phrases are padded to `--tokens` ids, so the
constrained search takes tokens + 1 passes, and the free-form decodes (off, and both hotword forms) run with max_length chosen so that they take as
many (seeded weights never emit <|endoftext|>), through the same step loop.  The medians are repeated; the spread of the repeated medians is
reported beside them.  No pass mark.

    python tools/hotword_bench.py [--size large-v2] [--iters 10] [--warmup 3] [--repeats 3] [--tokens 24] [--boost 3.0]
    rocprofv3 --kernel-trace --stats -d OUT -o hotword -- python tools/hotword_bench.py --iters 5 --repeats 1      # the pre-pass kernel's own time
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "willow-inference-server_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

PROMPT = [50258, 50259, 50359, 50363]          # <|startoftranscript|><|en|><|transcribe|><|notimestamps|>


def hotword_sets(seed=11):
    """-> {"20": ..., "2000": ...}: entries of 1 .. 8 ids; the large set has 300 different first tokens"""
    import numpy as np
    from wis_hip import weights as W
    bad = set(W.SUPPRESS_IDS) | set(W.SUPPRESS_IDS_BEGIN)
    pool = np.asarray([t for t in range(300, 50000) if t not in bad])
    rng = np.random.default_rng(seed)
    small = [rng.choice(pool, size=int(rng.integers(1, 9))).tolist() for _ in range(20)]
    firsts = rng.choice(pool, size=300, replace=False)
    large = [[int(firsts[i % 300])] + rng.choice(pool, size=int(rng.integers(0, 8))).tolist() for i in range(2000)]
    return {"20": small, "2000": large}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", default="large-v2")
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--tokens", type=int, default=24)
    ap.add_argument("--boost", type=float, default=3.0)
    a = ap.parse_args()
    if not 1 <= a.tokens <= 32:
        ap.error("--tokens: 1..32 (a phrase holds at most 32 tokens)")
    import numpy as np
    from phrase_bench import phrase_sets
    from wis_hip import audio, ctranslate2 as ct2, weights as W
    pcm, _ = audio.load_audio(os.path.join(ROOT, "tests", "golden", "clips", "3sec.flac"))
    mel = audio.log_mel_spectrogram(audio.pad_or_trim(pcm)).numpy()
    sets = hotword_sets()
    tries = {k: int(len(W.build_hotword_trie(v))) for k, v in sets.items()}
    roots = {k: len({e[0] for e in v}) for k, v in sets.items()}
    model = ct2.Whisper("unused", weights=W.synthetic_weights(a.size), arch=W.arch(a.size), max_batch=8, max_beam=5)
    free = dict(max_length=2 * (a.tokens + 1))      # max_new_tokens = min(max_length // 2, max_length - P) = tokens + 1 passes, as the constrained search takes
    forms = [("off", free)] + [(f"hot_{k}", dict(hotwords=v, hotword_boost=a.boost, **free)) for k, v in sets.items()] + [("phrases_20", dict(phrases=phrase_sets(a.tokens)["20"]))]
    res = {}
    try:
        for B in (1, 8):
            feats = ct2.StorageView.from_array(np.ascontiguousarray(np.repeat(mel[None], B, axis=0)))
            meds = {name: [] for name, _ in forms}
            steps = {}
            for _ in range(a.repeats):
                for name, kw in forms:      # (the forms alternate inside a repeat: drift of the clocks hits them alike)
                    step_ms = []
                    for i in range(a.warmup + a.iters):
                        model.generate(feats, [PROMPT] * B, beam_size=5, **kw)
                        t = model.last_timing()
                        if i >= a.warmup:
                            step_ms.append(t["decode_ms"] / max(1, t["decode_steps_needed"] - 1))      # (the merged prefill + first step is not a decode step)
                    meds[name].append(float(np.median(step_ms)))
                    steps[name] = int(t["decode_steps_needed"])
            row = {}
            for name, _ in forms:
                row[name] = dict(step_ms=round(float(np.median(meds[name])), 4), spread_ms=round(max(meds[name]) - min(meds[name]), 4), passes=steps[name])
            for name, _ in forms[1:]:
                row[name]["delta_ms"] = round(row[name]["step_ms"] - row["off"]["step_ms"], 4)
            res[f"B{B}_beam5"] = row
    finally:
        model.close()
    print(json.dumps({"metric": "decode_step_ms", "size": a.size, "tokens": a.tokens, "boost": a.boost, "repeats": a.repeats, "trie_records": tries,
                      "root_children": roots, "shapes": res}))


if __name__ == "__main__":
    main()
