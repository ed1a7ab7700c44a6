"""A/B of the int8 cross K/V (models.Whisper(cross_kv_compute_type="int8")) against the f16 images, in ONE process: seeded large-v2 weights, beam 5, a
fixed decode length; two handles on one GPU, measured in alternation.  Per batch size: milliseconds per decode step (wis_last_timing: decode_ms /
decode_steps, device clock) and of the cross-K/V build (crosskv_ms), each as the median of `--iters` calls, that median taken `--repeats` times - the
figure is the median of the repeated medians, the spread their minimum and maximum.  wis_model_device_bytes of both handles beside them.

    python tools/cross_kv_bench.py [--batches 1,8,16] [--iters 5] [--repeats 3] [--new 32] [--encoder int8] [--two-launch]

--two-launch adds a third handle, "int8_2l": the int8 images built the earlier way (WIS_CKV_FUSED=0 at create: the projection of four layers at a time into
f16 staging blocks, then cross_kv_quant_kernel), in the same alternation - the A/B of the fused projection kernel on one box and in one process.
"""
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "willow-inference-server_amd"))
PROMPT = [50258, 50259, 50359, 50363]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", default="large-v2")
    ap.add_argument("--batches", default="1,8,16")
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--new", type=int, default=32)
    ap.add_argument("--encoder", default="float16", help="encoder_compute_type of every handle")
    ap.add_argument("--two-launch", action="store_true")
    a = ap.parse_args()
    import numpy as np
    import torch  # noqa: F401  (before libwis_hip.so: one HIP runtime per process)
    from wis_hip import _lib, ctranslate2 as ct2, weights as W
    lib, arch, batches = _lib.load(), W.arch(a.size), [int(b) for b in a.batches.split(",")]
    w = W.synthetic_weights(a.size, seed=1234)
    models = {}
    for k in ("float16", "int8") + (("int8_2l",) if a.two_launch else ()):
        if k == "int8_2l":
            os.environ["WIS_CKV_FUSED"] = "0"      # (read when the handle is created)
        models[k] = ct2.Whisper("unused", weights=w, arch=arch, max_batch=max(batches), max_beam=5, cross_kv_compute_type=k[:4] if k != "float16" else k,
                                encoder_compute_type=a.encoder)
        os.environ.pop("WIS_CKV_FUSED", None)
    handles = {k: m._replicas[0].handle for k, m in models.items()}
    mel = np.load(os.path.join(ROOT, "tests", "golden", "logmel_3sec.npz"))["mel"].astype(np.float32)
    i32, f32 = C.POINTER(C.c_int32), C.POINTER(C.c_float)

    def call(h, B):
        x, o = np.ascontiguousarray(np.repeat(mel[None], B, 0)), _lib.GenOpts(_lib.WIS_IN_MEL_HOST, 5, 0, 1.0, 1.0, 1, 1, a.new, 0)
        prompt, ids, lens, sc = np.ascontiguousarray(np.tile(np.asarray(PROMPT, np.int32), (B, 1))), np.zeros((B, 224), np.int32), np.zeros(B, np.int32), np.zeros(B, np.float32)
        _lib.check(lib.wis_generate(h, _lib.ptr(x), B, prompt.ctypes.data_as(i32), 4, C.byref(o), ids.ctypes.data_as(i32), lens.ctypes.data_as(i32), sc.ctypes.data_as(f32)))
        t = _lib.Timing()
        _lib.check(lib.wis_last_timing(h, C.byref(t)))
        return t.decode_ms / max(t.decode_steps, 1), t.crosskv_ms

    res = {"encoder": a.encoder, "device_bytes": {k: int(lib.wis_model_device_bytes(h)) for k, h in handles.items()}, "beam": 5, "new_tokens": a.new, "rows": {}}
    try:
        for B in batches:
            for h in handles.values():      # warm: graphs captured, weights touched
                call(h, B), call(h, B)
            med = {k: [] for k in handles}
            for _ in range(a.repeats):
                runs = {k: [] for k in handles}
                for _ in range(a.iters):      # alternating: f16, int8, f16, int8, ...
                    for k, h in handles.items():
                        runs[k].append(call(h, B))
                for k in handles:
                    med[k].append(np.median(np.asarray(runs[k]), axis=0))
            row = {}
            for k in handles:
                m = np.asarray(med[k])
                for j, name in enumerate(("step_ms", "crosskv_ms")):
                    row[f"{k}_{name}"] = {"median": round(float(np.median(m[:, j])), 4), "min": round(float(m[:, j].min()), 4), "max": round(float(m[:, j].max()), 4)}
            res["rows"][f"B{B}"] = row
    finally:
        for m in models.values():
            m.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
