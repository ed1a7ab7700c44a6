"""-m gpu: kernel-level parity of the hand-written HIP kernels, called through the C-ABI
(wis_op_* / wis_logmel), against numpy / the oracle on seeded inputs."""
import ctypes as C
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _relerr(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / (np.linalg.norm(b) + 1e-30))


def _gelu(x):
    from scipy.special import erf
    return 0.5 * x * (1.0 + erf(x / np.sqrt(2.0)))


# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("clip", ["3sec", "10sec", "30sec"])
def test_logmel_reference_clips(golden_dir, clip):
    """HIP log-mel vs the REAL reference's output (golden fixture), tolerance 5e-5."""
    from wis_hip import audio
    pcm, sr = audio.load_audio(os.path.join(golden_dir, "clips", clip + ".flac"))
    mel = audio.log_mel_spectrogram(audio.pad_or_trim(pcm)).numpy()
    ref = np.load(os.path.join(golden_dir, f"logmel_{clip}.npz"))["mel"]
    assert mel.shape == (80, 3000) and mel.dtype == np.float32
    err = np.abs(mel - ref).max()
    print(f"logmel {clip}: max abs err {err:.3e}")
    assert err <= 5e-5


def test_logmel_noise_and_batch(golden_dir):
    from wis_hip import audio
    rng = np.random.default_rng(1234)
    g = np.load(os.path.join(golden_dir, "logmel_noise.npz"))
    xs = [(0.1 * rng.standard_normal(n)).astype(np.float32) for n in (61440, 480000)]
    batch = np.stack([audio.pad_or_trim(x) for x in xs])
    mel = audio.log_mel_spectrogram(batch).numpy()
    for i, n in enumerate((61440, 480000)):
        err = np.abs(mel[i] - g[f"mel_{n}"]).max()
        print(f"logmel noise {n}: max abs err {err:.3e}")
        assert err <= 5e-5
    # edge cases: all-zero window (every tile takes the silent shortcut) and a single impulse
    from oracle import audio_ref
    z = np.zeros(480000, np.float32)
    imp = z.copy(); imp[1234] = 0.5
    out = audio.log_mel_spectrogram(np.stack([z, imp])).numpy()
    assert np.abs(out[0] - audio_ref.log_mel_spectrogram(z)).max() <= 5e-5
    assert np.abs(out[1] - audio_ref.log_mel_spectrogram(imp)).max() <= 5e-5


# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,N,K,flags", [(300, 256, 320, 0), (128, 128, 64, 4), (1500, 384, 1152, 1), (257, 1280, 1280, 2 | 4),
                                         (3000, 512, 5120, 1 | 4), (77, 128, 64, 2 | 4 | 1),
                                         (1500, 1280, 5120, 2 | 4 | 8), (200, 128, 128, 2 | 4 | 8),      # split-K x2 (encoder FFN2)
                                         (1500, 1280, 1280, 2 | 4), (65, 256, 64, 0), (1500, 3840, 1280, 0), (3000, 1280, 320, 1),   # 64-row tiles; QKV / conv1 shapes
                                         (6321, 2048, 192, 2 | 4), (12000, 1280, 128, 1),                 # 256x256 tiles, 8 waves (batched encoder), ragged M
                                         (1500, 5120, 1280, 1), (1411, 2560, 192, 0), (1500, 3840, 1280, 2 | 4),      # 128x256 8-phase tile (one utterance): FFN1, ragged M / 3 k-tiles, residual epilogue
                                         (1500, 4096, 128, 1 | 4)])                                       # ... two k-tiles (the prologue alone)
def test_gemm(lib, M, N, K, flags):
    from wis_hip._lib import DevBuf, check
    rng = np.random.default_rng(M * 7 + N)
    A = (rng.standard_normal((M, K)) * 0.5).astype(np.float16)
    Wt = (rng.standard_normal((N, K)) * 0.1).astype(np.float16)
    bias = rng.standard_normal(N).astype(np.float32)
    res = rng.standard_normal((M, N)).astype(np.float32)
    ref = A.astype(np.float64) @ Wt.astype(np.float64).T + bias
    if flags & 1:
        ref = _gelu(ref)
    if flags & 2:
        ref = ref + res
    dA, dW, db, dr = DevBuf.from_numpy(A), DevBuf.from_numpy(Wt), DevBuf.from_numpy(bias), DevBuf.from_numpy(res)
    out_dt = np.float32 if flags & 4 else np.float16
    dC = DevBuf(M * N * np.dtype(out_dt).itemsize)
    check(lib.wis_op_gemm(0, dA.ptr, K, dW.ptr, db.ptr, dr.ptr, dC.ptr, M, N, K, flags))
    out = dC.to_numpy(out_dt, (M, N))
    e = _relerr(out, ref)
    print(f"gemm M{M} N{N} K{K} flags{flags}: rel err {e:.3e}")
    assert e < (2e-3 if out_dt == np.float16 else 1e-4)
    # row/column placement check on a few exact entries (transpose-detecting: A, W asymmetric random)
    assert np.allclose(out[M - 1, N - 1], ref[M - 1, N - 1], rtol=5e-3, atol=5e-3)


def test_gemm_implicit_im2col_conv(lib):
    """conv1d(k=3, pad=1, stride s) as a GEMM over overlapping rows of the zero-padded time-major image
    is what the encoder does; checked here through wis_op_gemm's lda (row pitch C*s, K = 3C rounded up to the 64-deep
    k-tile with zero weight columns, exactly like the engine's conv1: 288 -> 320)."""
    import torch
    import torch.nn.functional as F
    from wis_hip._lib import DevBuf, check
    rng = np.random.default_rng(5)
    for Cin, Cout, T in ((96, 128, 300), (128, 256, 130)):
        Kp = ((3 * Cin + 63) // 64) * 64
        for stride in (1, 2):
            x = (rng.standard_normal((Cin, T)) * 0.5).astype(np.float16)
            w = (rng.standard_normal((Cout, Cin, 3)) * 0.1).astype(np.float16)
            ref = F.conv1d(torch.from_numpy(x.astype(np.float32))[None], torch.from_numpy(w.astype(np.float32)), stride=stride, padding=1)[0].numpy().T
            img = np.zeros((T + 2) * Cin + 64, np.float16); img[Cin:(T + 1) * Cin] = x.T.reshape(-1)     # + tail for the zero-weighted over-read
            wp = np.zeros((Cout, Kp), np.float16); wp[:, :3 * Cin] = w.transpose(0, 2, 1).reshape(Cout, 3 * Cin)     # [out][k*C + c]
            Tout = ref.shape[0]
            dA, dW = DevBuf.from_numpy(img), DevBuf.from_numpy(wp)
            dC = DevBuf(Tout * Cout * 4)
            check(lib.wis_op_gemm(0, dA.ptr, Cin * stride, dW.ptr, None, None, dC.ptr, Tout, Cout, Kp, 4))
            out = dC.to_numpy(np.float32, (Tout, Cout))
            e = _relerr(out, ref)
            print(f"conv-as-gemm C{Cin} stride {stride}: rel err {e:.3e}")
            assert e < 1e-4


@pytest.mark.parametrize("M,d", [(5, 384), (1500, 1280), (33, 512)])
def test_layernorm(lib, M, d):
    from wis_hip._lib import DevBuf, check
    rng = np.random.default_rng(d)
    x = (rng.standard_normal((M, d)) * 3 + 0.7).astype(np.float32)
    g = rng.standard_normal(d).astype(np.float32); b = rng.standard_normal(d).astype(np.float32)
    mu = x.astype(np.float64).mean(1, keepdims=True); var = x.astype(np.float64).var(1, keepdims=True)
    ref = (x - mu) / np.sqrt(var + 1e-5) * g + b
    dx, dg, db = DevBuf.from_numpy(x), DevBuf.from_numpy(g), DevBuf.from_numpy(b)
    dy = DevBuf(M * d * 2)
    check(lib.wis_op_layernorm(0, dx.ptr, dg.ptr, db.ptr, dy.ptr, M, d))
    out = dy.to_numpy(np.float16, (M, d))
    e = _relerr(out, ref)
    print(f"layernorm M{M} d{d}: rel err {e:.3e}")
    assert e < 1e-3


# grids of <= 256 workgroups with >= 4 key tiles take the split-key form (two workgroups per query tile and head, merged in the
# launch by whichever arrives last): (1, 200, 2), (2, 1500, 3) and the large-v2 shape (1, 1500, 20); (3, 1500, 20) and the short ones do not
@pytest.mark.parametrize("B,T,H", [(1, 200, 2), (2, 1500, 3), (1, 64, 1), (1, 129, 2), (1, 1500, 20), (3, 1500, 20)])
def test_enc_attention(lib, B, T, H):
    from wis_hip._lib import DevBuf, check
    rng = np.random.default_rng(T + H)
    d = H * 64
    Tpad = ((T + 63) // 64) * 64
    q = (rng.standard_normal((B, T, H, 64)) * 0.35).astype(np.float16)      # already scaled by 1/8 in the engine
    k = (rng.standard_normal((B, T, H, 64))).astype(np.float16)
    v = (rng.standard_normal((B, T, H, 64))).astype(np.float16)
    q[0, 3, 0] *= 6.0     # a spiky query row exercises the online-softmax rescale
    # keys planted late in the sequence that beat everything before them by > 15 in the log2 domain for a few queries: the lazy
    # softmax reference (enc_attn_lazy_kernel) has to be raised in the MIDDLE of the key loop, in either half of a split pair
    for t_key, t_q in ((T * 2 // 5, 5), (T * 4 // 5, 40), (T - 1, 7)):
        if T > 128 and t_q < T:
            k[0, t_key, 0] = (q[0, t_q, 0].astype(np.float32) / np.linalg.norm(q[0, t_q, 0].astype(np.float32)) * 9.0).astype(np.float16)
    qk = np.concatenate([q.reshape(B, T, d), k.reshape(B, T, d)], axis=2).reshape(B * T, 2 * d)
    # V^T image as the encoder's QKV epilogue writes it: keys in groups of 16 with bits 2 and 3 of the index swapped
    tt = np.arange(T); tp = (tt & ~12) | ((tt & 4) << 1) | ((tt & 8) >> 1)
    vt = np.zeros((B, H, 64, Tpad), np.float16); vt[:, :, :, tp] = v.transpose(0, 2, 3, 1)
    s = np.einsum("bqhd,bkhd->bhqk", q.astype(np.float64), k.astype(np.float64))
    p = np.exp(s - s.max(-1, keepdims=True)); p /= p.sum(-1, keepdims=True)
    ref = np.einsum("bhqk,bkhd->bqhd", p, v.astype(np.float64)).reshape(B * T, d)
    dqk, dvt = DevBuf.from_numpy(qk), DevBuf.from_numpy(vt)
    do = DevBuf(B * T * d * 2)
    outs = []
    for rep in range(3):      # bit-identical whichever workgroup of a pair merges
        check(lib.wis_op_enc_attention(0, dqk.ptr, dvt.ptr, do.ptr, B, T, Tpad, H))
        outs.append(do.to_numpy(np.float16, (B * T, d)).copy())
    assert np.array_equal(outs[0], outs[1]) and np.array_equal(outs[1], outs[2])
    out = outs[0]
    e = _relerr(out, ref)
    print(f"enc_attention B{B} T{T} H{H}: rel err {e:.3e}, max abs {np.abs(out - ref).max():.3e}")
    assert e < 3e-3


@pytest.mark.parametrize("M,N,K,flags", [(5, 1280, 1280, 8 | 4), (1, 384, 384, 0), (5, 1280, 5120, 2), (17, 512, 2048, 1),
                                         (40, 1280, 1280, 8 | 1), (5, 51865 // 4 * 4, 384, 8 | 4), (3, 1004, 128, 4), (48, 256, 5120, 2),
                                         # more workgroups than CUs + several 16-row blocks + fused LN: the shapes that exposed a
                                         # cross-wave statistics hazard in round 1 (last row wrong in ~0.5 % of workgroups)
                                         (20, 5120, 640, 8 | 1), (24, 5120, 1280, 8 | 1), (40, 7680, 1280, 8 | 1), (40, 5120, 1280, 8 | 4),
                                         (8, 5120, 1280, 8 | 4), (5, 1280, 5120, 0), (16, 1280, 4096, 2),
                                         # int8_float16 (flag 32): per-row int8 weights, every kernel mode (LN-fused, f16 activations, generic ring, batched rows)
                                         (5, 1280, 1280, 32 | 8 | 4), (5, 1280, 1280, 32 | 2), (5, 1280, 5120, 32 | 2), (5, 3840, 1280, 32 | 8 | 4),
                                         (40, 1280, 5120, 32 | 2), (40, 5120, 1280, 32 | 1), (3, 1004, 384, 32 | 4), (1, 51872, 1280, 32 | 8 | 4),
                                         # 49-96 rows (up to 16 utterances x beam 5): four to six row blocks, six-deep fragment ring
                                         (64, 1280, 1280, 8 | 4), (80, 5120, 1280, 8 | 1), (80, 1280, 5120, 2), (96, 3840, 1280, 8 | 4), (80, 1280, 1280, 32 | 2),
                                         (72, 768, 384, 8 | 4),
                                         # K = 4d on f16 rows asks for the step's K split (two slices), but from 17 rows on and up to 85 n-tiles launch_gemv_frag runs the
                                         # M split instead: these three land on gemv_frag_ms_kernel<1 | 2 | 1> (3, 3 and 2 row-block groups, no K split, no merge).  Of this
                                         # list only (16, 1280, 4096, 2) above splits K: gemv_frag_kernel<1, 8>, two slices merged in the launch.  The merge at two and at
                                         # four slices, with its tickets re-armed between two launches: tests/test_gpu_dec_frag_ops.py
                                         (40, 1280, 5120, 4), (96, 1280, 5120, 0), (24, 1024, 4096, 1),
                                         # two n-tiles per workgroup (more than 256 n-tiles behind a folded LayerNorm): int8 weights, the vocabulary shape, ragged rows
                                         (40, 5120, 1280, 32 | 8 | 1), (80, 51872, 1280, 8 | 4), (33, 8192, 1280, 8 | 4),
                                         # the one-utterance step's LayerNorm-folded N = 4d / 3d projections at 4-5 rows (two n-tiles per workgroup of the LDS-staged form)
                                         (5, 5120, 1280, 8 | 4 | 1), (4, 5120, 1280, 8 | 1), (5, 3840, 1280, 8 | 4), (5, 4096, 1280, 8)])
def test_gemv(lib, M, N, K, flags):
    from wis_hip._lib import DevBuf, check
    rng = np.random.default_rng(M * 31 + N + K)
    Wt = (rng.standard_normal((N, K)) * 0.05).astype(np.float16)
    bias = rng.standard_normal(N).astype(np.float32)
    g = (1 + 0.1 * rng.standard_normal(K)).astype(np.float32); b = (0.1 * rng.standard_normal(K)).astype(np.float32)
    if flags & 8:
        x = (rng.standard_normal((M, K)) * 2 + 0.3).astype(np.float32)
        mu = x.astype(np.float64).mean(1, keepdims=True); var = x.astype(np.float64).var(1, keepdims=True)
        xin = (((x - mu) / np.sqrt(var + 1e-5)) * g + b).astype(np.float16).astype(np.float64)   # engine rounds LN output to f16
    else:
        x = rng.standard_normal((M, K)).astype(np.float16)
        xin = x.astype(np.float64)
    Wref = Wt.astype(np.float64)
    if flags & 32:            # the engine quantises the rows itself: the reference uses the de-quantised matrix
        from wis_hip.weights import quantize_rows
        if flags & 8:         # a projection behind a LayerNorm is stored gamma-folded, and quantised in that form
            from wis_hip.weights import quantize_folded
            Wref = quantize_folded(Wt, g).astype(np.float64)
        else:
            q, sc = quantize_rows(Wt)
            Wref = q.astype(np.float64) * sc.astype(np.float64)[:, None]
            assert np.abs(Wref - Wt.astype(np.float64)).max() <= 0.5 * sc.max() * 1.0001     # within half a quantisation step
    ref = xin @ Wref.T + bias
    if flags & 1:
        ref = _gelu(ref)
    y0 = rng.standard_normal((M, N)).astype(np.float32)
    if flags & 2:
        ref = ref + y0
    out_f32 = bool(flags & (2 | 4))
    dx, dW, dbias, dg, db = DevBuf.from_numpy(x), DevBuf.from_numpy(Wt), DevBuf.from_numpy(bias), DevBuf.from_numpy(g), DevBuf.from_numpy(b)
    dy = DevBuf.from_numpy(y0) if out_f32 else DevBuf(M * N * 2)
    check(lib.wis_op_gemv(0, dx.ptr, dg.ptr, db.ptr, dW.ptr, dbias.ptr, dy.ptr, M, N, K, flags))
    for rep in range(3):          # repeated: the hazard was timing dependent
        if rep:
            check(lib.wis_dev_h2d(0, dy.ptr, y0.ctypes.data_as(__import__("ctypes").c_void_p), y0.nbytes)) if out_f32 else None
            check(lib.wis_op_gemv(0, dx.ptr, dg.ptr, db.ptr, dW.ptr, dbias.ptr, dy.ptr, M, N, K, flags))
        out = dy.to_numpy(np.float32 if out_f32 else np.float16, (M, N))
        e = _relerr(out, ref)
        worst = float(np.abs(out.astype(np.float64) - ref).max())
        print(f"gemv M{M} N{N} K{K} flags{flags} rep{rep}: rel err {e:.3e} max abs {worst:.3e}")
        assert e < (1e-3 if out_f32 else 2e-3)
        assert worst < 0.05 * (1 + float(np.abs(ref).max()))          # no single corrupted row hiding inside the L2 norm


@pytest.mark.parametrize("K", [384, 512, 1024, 1280])
def test_gemv_layernorm_on_f16_rows(lib, K):
    """GV_LN16 (tap flag 64; WIS_B1_LN=f16 in the model): the LayerNorm-folded projection on the F16 copy of the rows - one 16-byte chunk of
    every row per thread (K / 8 threads: 48 .. 160 of the workgroup's 256, i.e. partial waves), statistics from those f16 values.  Every
    row count 1..8 (the three register-row instantiations), rows with a common offset, against float64 on the same f16 values."""
    from wis_hip._lib import DevBuf, check
    N = 1280
    for M in range(1, 9):
        rng = np.random.default_rng(K + M)
        x = ((rng.standard_normal((M, K)) * 2 + 0.3 + 5.0 * (M % 3))).astype(np.float16)
        Wt = (rng.standard_normal((N, K)) * 0.05).astype(np.float16)
        bias = rng.standard_normal(N).astype(np.float32)
        g = (1 + 0.1 * rng.standard_normal(K)).astype(np.float32); b = (0.1 * rng.standard_normal(K)).astype(np.float32)
        x64 = x.astype(np.float64)
        mu = x64.mean(1, keepdims=True); var = x64.var(1, keepdims=True)
        Wg = (Wt.astype(np.float32) * g).astype(np.float16).astype(np.float64)
        ref = ((x64 - mu) / np.sqrt(var + 1e-5)) @ Wg.T + Wt.astype(np.float64) @ b.astype(np.float64) + bias
        dx, dW, dbias, dg, db = DevBuf.from_numpy(x), DevBuf.from_numpy(Wt), DevBuf.from_numpy(bias), DevBuf.from_numpy(g), DevBuf.from_numpy(b)
        dy = DevBuf(M * N * 4)
        check(lib.wis_op_gemv(0, dx.ptr, dg.ptr, db.ptr, dW.ptr, dbias.ptr, dy.ptr, M, N, K, 64 | 4))
        out = dy.to_numpy(np.float32, (M, N))
        e = _relerr(out, ref)
        print(f"gemv + LayerNorm on f16 rows, K{K} M{M}: rel err {e:.3e}")
        assert e < 2e-3, (K, M, e)


@pytest.mark.parametrize("M", [5, 40])
def test_gemv_layernorm_rows_with_a_large_common_offset(lib, M):
    """A projection behind a LayerNorm on rows whose mean is large against their spread (|mean| = 200, std 2.4): the row
    statistics must not lose the variance to E[x^2] - mean^2 cancellation - at <= 8 rows the kernel shifts by x[r][0], above
    8 rows (batched decode) the per-16-column partials are (sum, M2 about the tile mean) pairs merged Welford-style.  The rows
    are exact in f16 (multiples of 1/4 in [128, 256)), so the raw-row cast of the folded form adds no error of its own."""
    from wis_hip._lib import DevBuf, check
    rng = np.random.default_rng(11 + M)
    N, K = 1280, 1280
    x = (200.0 + rng.integers(-16, 17, size=(M, K)) / 4.0).astype(np.float32)
    x[:, ::7] += 8.0          # tile means differ from the row mean
    Wt = (rng.standard_normal((N, K)) * 0.05).astype(np.float16)
    bias = rng.standard_normal(N).astype(np.float32)
    g = (1 + 0.1 * rng.standard_normal(K)).astype(np.float32); b = (0.1 * rng.standard_normal(K)).astype(np.float32)
    mu = x.astype(np.float64).mean(1, keepdims=True); var = x.astype(np.float64).var(1, keepdims=True)
    # the folded form: W' = f16(W * gamma) on the raw rows, statistics in the epilogue (dec_kernels.hip fold_ln_kernel)
    Wg = (Wt.astype(np.float32) * g).astype(np.float16).astype(np.float64)
    ref = ((x.astype(np.float64) - mu) / np.sqrt(var + 1e-5)) @ Wg.T + Wt.astype(np.float64) @ b.astype(np.float64) + bias
    dx, dW, dbias, dg, db = DevBuf.from_numpy(x), DevBuf.from_numpy(Wt), DevBuf.from_numpy(bias), DevBuf.from_numpy(g), DevBuf.from_numpy(b)
    dy = DevBuf(M * N * 4)
    check(lib.wis_op_gemv(0, dx.ptr, dg.ptr, db.ptr, dW.ptr, dbias.ptr, dy.ptr, M, N, K, 8 | 4))
    out = dy.to_numpy(np.float32, (M, N))
    e = _relerr(out, ref)
    print(f"gemv + LayerNorm, rows at 200 +- 2.4, M{M}: rel err {e:.3e}")
    assert e < 2e-3
