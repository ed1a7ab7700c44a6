"""The int8 encoder against the f16 encoder (models.Whisper(encoder_compute_type=...)), seeded weights:

  * `encode` at B = 1 and 8 per model size, the two sides as two models in one process, called in alternating pairs; `--rounds` medians of `--iters`
    pairs each give the spread (wall; the call synchronises the handle's stream);
  * the four layer GEMMs (and cross K/V's per-layer shape) at M = 1500 and M = 12000, f16 as the encoder picks its tile against every int8 tile form,
    and the two quantise launches, us per launch between two events (wis_bench_enc_gemm: operands streamed from HBM);
  * device bytes of a handle on each side.

    python tools/enc_int8_bench.py [--sizes large-v2,large-v3-turbo] [--iters 7] [--rounds 3] [--warmup 2] [--reps 400]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "willow-inference-server_amd"))


def encode_rows(a, size, out):
    import numpy as np
    from wis_hip import _lib, ctranslate2 as ct2, weights as W
    arch, w = W.arch(size), W.synthetic_weights(size)
    models = {t: ct2.Whisper("unused", weights=w, arch=arch, max_batch=8, max_beam=1, encoder_compute_type=t) for t in ("float16", "int8")}
    try:
        out[f"{size}_device_bytes"] = {t: int(_lib.load().wis_model_device_bytes(m._replicas[0].handle)) for t, m in models.items()}
        mel = np.random.default_rng(0).standard_normal((8, arch["n_mels"], 3000)).astype(np.float32)
        for B in (1, 8):
            x = ct2.StorageView.from_array(np.ascontiguousarray(mel[:B]))
            for _ in range(a.warmup):
                for m in models.values():
                    m.encode(x)
            meds = {t: [] for t in models}
            for _ in range(a.rounds):
                ms = {t: [] for t in models}
                for _ in range(a.iters):
                    for t, m in models.items():      # alternating pairs
                        t0 = time.perf_counter()
                        m.encode(x)
                        ms[t].append((time.perf_counter() - t0) * 1e3)
                for t in models:
                    meds[t].append(float(np.median(ms[t])))
            out[f"{size}_B{B}_encode_ms"] = {t: {"median": round(float(np.median(v)), 3), "spread": round(max(v) - min(v), 3)} for t, v in meds.items()}
    finally:
        for m in models.values():
            m.close()


def gemm_rows(a, d, out):
    from wis_hip import _lib
    lib, us = _lib.load(), C.c_float()

    def t(bits, M, N, K, form=0):
        _lib.check(lib.wis_bench_enc_gemm(0, bits, M, N, K, form, a.reps, C.byref(us)))
        return round(us.value, 2)
    for M in (1500, 12000):
        for name, N, K in (("qkv", 3 * d, d), ("out", d, d), ("ffn1", 4 * d, d), ("ffn2", d, 4 * d)):
            row = {"f16": t(16, M, N, K), "int8_picked": t(8, M, N, K)}
            row.update({f"int8_form{f}": t(8, M, N, K, f) for f in (1, 2, 3) if f != 3 or N % 256 == 0})
            out[f"d{d}_M{M}_{name}_us"] = row
        out[f"d{d}_M{M}_quantise_us"] = {"rows_K_d": t(1, M, d, d), "rows_K_4d": t(1, M, 4 * d, 4 * d), "layernorm_quant": t(2, M, d, d)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="large-v2,large-v3-turbo")
    ap.add_argument("--iters", type=int, default=7)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=400)
    a = ap.parse_args()
    import torch  # noqa: F401  (before libwis_hip.so: one HIP runtime per process)
    out = {}
    gemm_rows(a, 1280, out)
    for size in [s for s in a.sizes.split(",") if s]:
        encode_rows(a, size, out)
    print(json.dumps({"metric": "enc_int8", **out}))


if __name__ == "__main__":
    main()
