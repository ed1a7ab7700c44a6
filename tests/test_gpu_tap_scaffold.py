"""-m gpu: the scaffold every single-kernel tap (wis_op_*) runs in - device context, the device's op mutex, private scratch, the
synchronise / free / report epilogue (csrc/taps.hip, "how to write a tap") - and the two pairs of entry points that share one body.

* Refusals decided on the host before any launch leave the mutex free and the stream clean: the next valid call works.
* wis_op_dec_self_attn is wis_op_dec_self_attn_ex(nb = 8, out_mb = 0, no tree), wis_debug_logits is wis_debug_logits_rows(R = 1): the same
  host path and the same kernels behind both names, so the results are compared bit for bit."""
import ctypes as C

import numpy as np
import pytest
import torch  # noqa: F401  (before libwis_hip.so: one HIP runtime per process)

pytestmark = pytest.mark.gpu
WIS_E_ARG, WIS_E_UNSUPPORTED = -1, -7      # include/wis_hip.h
GV_OUT_F32 = 4                             # csrc/kernels.hpp


def test_refusals_then_a_good_call(lib):
    from wis_hip._lib import DevBuf, check
    d = DevBuf(1 << 16)      # stands for every non-null pointer: no refused call launches anything
    p = d.ptr
    refusals = [
        ("wis_op_enc_attention_ex", (0, p, p, p, 1, 192, 192, 1, 4), WIS_E_ARG),                        # form = 4
        ("wis_op_enc_attention_ex", (0, p, p, p, 1, 192, 192, 1, 2), WIS_E_ARG),                        # split form, three key tiles
        ("wis_op_gemv_cols", (0, p, p, None, p, None, 5, 1280, 1280, GV_OUT_F32, 12), WIS_E_ARG),       # cols = 12
        ("wis_op_gemv_cols", (0, p, p, None, p, None, 1, 8, 128, GV_OUT_F32, 8), WIS_E_UNSUPPORTED),    # not an eight-column shape
        ("wis_op_gemm", (0, p, 64, p, None, p, p, 128, 128, 64, 2 | 4 | 8), WIS_E_ARG),                 # flag 8 without bias
        ("wis_op_dec_self_attn_ex", (0, p, p, p, p, p, 2, 2, 16, 1, 1, 1, 3, 0, None, 0, 0, None), WIS_E_ARG),      # nb = 3
        ("wis_op_dec_self_attn", (0, p, p, p, p, p, 2, 0, 16, 1, 1, 1), WIS_E_ARG),                     # H = 0
        # the parent commit's wis_op_dtw / wis_op_sv_posconv answer a null pointer with "bad argument", WIS_E_ARG
        ("wis_op_dtw", (0, p, 4, 6, p, p, None), WIS_E_ARG),                                            # null output (len)
        ("wis_op_sv_posconv", (0, p, p, p, None, 8), WIS_E_ARG),                                        # null output
        # the alignment stage taps: the null pointer is found before any host array (N, F, koff, target, dst, sel_head) is read
        ("wis_op_align_stage", (0, 3, None, p, 4096, p, 0, p, p, 1, 1, 4, 4, 4, 8, 7, 0, p, 1 << 14, p, 1 << 14), WIS_E_ARG),      # chain without q
        ("wis_op_align_stage", (0, 2, None, None, 0, None, 0, p, p, 1, 1, 4, 4, 4, 8, 7, 0, p, 1 << 14, None, 0), WIS_E_ARG),      # median without acc
        ("wis_op_dtw_batch", (0, p, 64, 0, 8, p, p, 1, 4, 6, 16, p, p, None), WIS_E_ARG),               # null output (len)
        ("wis_op_align_probs", (0, p, 4, 64, 60, p, p, None, 8), WIS_E_ARG),                            # null output (probs)
        ("wis_op_align_capture", (0, p, 32, 128, p, 0, 1, 1, 0, 0, 4, 16, None, 1 << 14), WIS_E_ARG),   # null output (qsel)
    ]
    for name, args, want in refusals:
        rc = getattr(lib, name)(*args)
        msg = (lib.wis_last_error() or b"").decode()
        print(f"{name}{args[1:]!r}: rc {rc}, {msg!r}")
        assert rc == want, (name, rc, msg)
        assert msg.startswith(name + ":"), (name, msg)
    # the mutex is free and the stream clean: tests/test_gpu_ops.py test_layernorm's smallest shape, at its tolerance
    M, dm = 5, 384
    rng = np.random.default_rng(dm)
    x = (rng.standard_normal((M, dm)) * 3 + 0.7).astype(np.float32)
    g = rng.standard_normal(dm).astype(np.float32); b = rng.standard_normal(dm).astype(np.float32)
    mu = x.astype(np.float64).mean(1, keepdims=True); var = x.astype(np.float64).var(1, keepdims=True)
    ref = (x - mu) / np.sqrt(var + 1e-5) * g + b
    dx, dg, db = DevBuf.from_numpy(x), DevBuf.from_numpy(g), DevBuf.from_numpy(b)
    dy = DevBuf(M * dm * 2)
    check(lib.wis_op_layernorm(0, dx.ptr, dg.ptr, db.ptr, dy.ptr, M, dm))
    out = dy.to_numpy(np.float16, (M, dm)).astype(np.float64)
    e = float(np.linalg.norm(out - ref) / np.linalg.norm(ref))
    print(f"layernorm after the refusals: rel err {e:.3e}")
    assert e < 1e-3


@pytest.mark.parametrize("ctx", [16, 64])
def test_self_attn_entry_points_agree(lib, ctx):
    """M = 2, H = 2, pos = [0, 9] through both names: the same return code and the same output bits.  launch_dec_self_attn takes caches of
    64 .. 512 positions, so at ctx = 16 both names must refuse alike (WIS_E_UNSUPPORTED, nothing written); ctx = 64, the smallest cache
    the kernel runs on, is where the launch behind both is compared."""
    from wis_hip._lib import DevBuf
    M, H = 2, 2
    d = 64 * H
    rng = np.random.default_rng(29)
    kc = (rng.standard_normal((M, ctx, d)) * 0.5).astype(np.float16)
    vc = rng.standard_normal((M, ctx, d)).astype(np.float16)
    q = (rng.standard_normal((M, d)) * 0.4).astype(np.float32)
    pos = np.array([0, 9], np.int32)
    d_kc, d_vc, d_q, d_pos = (DevBuf.from_numpy(a) for a in (kc, vc, q, pos))
    rcs, outs = [], []
    for ex in (False, True):
        d_out = DevBuf.from_numpy(np.full(M * d, 77.0, np.float16))
        args = (0, d_q.ptr, d_kc.ptr, d_vc.ptr, d_pos.ptr, d_out.ptr, M, H, ctx, 1, 1, 1)      # every row in a slot of its own
        rcs.append(lib.wis_op_dec_self_attn_ex(*args, 8, 0, None, 0, 0, None) if ex else lib.wis_op_dec_self_attn(*args))
        outs.append(d_out.to_numpy(np.float16, (M, d)))
    print(f"ctx {ctx}: return codes {rcs}")
    assert rcs == ([WIS_E_UNSUPPORTED] * 2 if ctx < 64 else [0, 0])
    assert np.array_equal(outs[0].view(np.uint16), outs[1].view(np.uint16))
    if ctx >= 64:      # position 0 attends to one key: the output is that value row, to the f16 bar of tests/test_gpu_dec_attn.py (two equal but empty results would pass the line above)
        assert np.abs(outs[0][0].astype(np.float64) - vc[0, 0].astype(np.float64)).max() <= 2e-3
    else:
        assert (outs[0] == 77.0).all()


def test_debug_logits_entry_points_agree(lib, golden_dir):
    import os
    from wis_hip import _lib, ctranslate2 as ct2, weights as W
    w = W.synthetic_weights("tiny", seed=1234, std=0.02, emb_std=0.06, ln_jitter=0.1)
    a = W.arch("tiny")
    model = ct2.Whisper("unused", weights=w, arch=a, max_batch=2, max_beam=1)
    h = model._replicas[0].handle
    mels = np.stack([np.load(os.path.join(golden_dir, f"logmel_{c}.npz"))["mel"] for c in ("3sec", "10sec")]).astype(np.float32)
    B, T, V = 2, 3, a["n_vocab"]
    dec_in = np.ascontiguousarray(np.tile(np.array([50258, 50259, 50359], np.int32), (B, 1)))
    dec_in[1, 2] = 1234
    ip, fp = C.POINTER(C.c_int32), C.POINTER(C.c_float)
    one, rows = np.zeros((B, T, V), np.float32), np.ones((B, T, V), np.float32)
    _lib.check(lib.wis_debug_logits(h, _lib.ptr(mels), _lib.WIS_IN_MEL_HOST, B, dec_in.ctypes.data_as(ip), T, one.ctypes.data_as(fp)))
    _lib.check(lib.wis_debug_logits_rows(h, _lib.ptr(mels), _lib.WIS_IN_MEL_HOST, B, dec_in.ctypes.data_as(ip), T, 1, rows.ctypes.data_as(fp)))
    assert np.isfinite(one).all() and one.std() > 0
    assert np.array_equal(one.view(np.uint32), rows.view(np.uint32))
    # a token outside [0, n_vocab) is refused on the host by both names (it would index the embedding table out of bounds)
    bad = dec_in.copy(); bad[1, 1] = V
    rc = lib.wis_debug_logits(h, _lib.ptr(mels), _lib.WIS_IN_MEL_HOST, B, bad.ctypes.data_as(ip), T, one.ctypes.data_as(fp))
    msg = (lib.wis_last_error() or b"").decode()
    assert rc == WIS_E_ARG and msg.startswith("wis_debug_logits:") and "out of range" in msg, (rc, msg)
