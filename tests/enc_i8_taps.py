"""What the int8 encoder's GPU test files share (tests/test_gpu_enc_i8.py, test_gpu_enc_i8_shapes.py, test_gpu_enc_i8_model.py): the fill-pattern
buffers, the output layouts of the five GEMM epilogues, the GEMM tap's driver and its per-element check, and the seeded tiny weight set with its
float64 encoder references (computed once per process)."""
import functools

import numpy as np

EPS, F16_R, GELU_LIP = 2.0 ** -24, 2.0 ** -10, 1.13


# GEMM tap cases with an utterance boundary (b = m / T) inside a row tile and inside a 32-row block, as (epilogue, form, (B, T), H, K or L):
# T = 44 / 52: Tpad = 64 != T and a partial 16-group of the V^T image's key swizzle; the last is tiny's own cross-K/V geometry (d = 384: the K-to-V
# switch at column 384 of a layer lies inside a 256-wide tile).  tests/test_enc_i8_cpu.py checks _where on them, tests/test_gpu_enc_i8_shapes.py runs them
BOUNDARY_CASES = [(3, 1, (3, 44), 2, 128), (3, 3, (5, 52), 4, 256), (4, 1, (3, 44), 2, 2), (4, 3, (5, 52), 4, 2), (4, 3, (1, 260), 6, 2)]


def _buf(n, dt):
    return np.full(n * np.dtype(dt).itemsize, 0x5A, np.uint8).view(dt)


def _kept(a):
    return bool((np.ascontiguousarray(a).view(np.uint8) == 0x5A).all())


def _where(epi, M, N, B, T, H, L):
    """-> (index of output (m, n) in the concatenation [C | out2], elements of C, elements of out2); 64 / 8 spare elements behind every image"""
    m, n = np.meshgrid(np.arange(M), np.arange(N), indexing="ij")
    if epi < 3:
        return m * N + n, (M + 3) * N, 0
    d, Tpad, b, t = 64 * H, (T + 63) // 64 * 64, m // T, m % T
    if epi == 3:      # [Q | K] rows; V^T image [B][H][64][Tpad], key t at bits 2 and 3 of t swapped
        nn, tp = n - 2 * d, (t & ~12) | ((t & 4) << 1) | ((t & 8) >> 1)
        return np.where(n < 2 * d, m * 2 * d + n, M * 2 * d + 64 + ((b * H + nn // 64) * 64 + nn % 64) * Tpad + tp), M * 2 * d + 64, B * d * Tpad + 8
    l, nl, kls, vls = n // (2 * d), n % (2 * d), M * d + 8, B * d * Tpad + 8      # per layer: K image [B][H][8][T][8], V^T image [B][H][64][Tpad]
    h, dh = (nl % d) // 64, nl % 64
    kx = l * kls + (((b * H + h) * 8 + dh // 8) * T + t) * 8 + dh % 8
    return np.where(nl < d, kx, L * kls + 64 + l * vls + ((b * H + h) * 64 + dh) * Tpad + t), L * kls + 64, L * vls


def _gemm(lib, epi, form, A, sa, Wq, sw, bias, res, flags, dims):
    """-> (outputs as float64 [M][N] in GEMM order, the raw buffers' words), after checking that nothing else was written"""
    from wis_hip._lib import DevBuf, check
    (M, K), N, (B, T, H, L) = A.shape, Wq.shape[0], dims
    dt = np.float32 if (epi == 2 or flags & 4) else np.float16
    idx, nc, nv = _where(epi, M, N, *dims)
    c = _buf(nc, dt)
    if epi == 2:
        c[:M * N] = res.ravel()      # in place: C holds the residual
    ins = [DevBuf.from_numpy(a) if a is not None else None for a in (A, sa, Wq, sw, bias)]
    c_d, v_d = DevBuf.from_numpy(c), DevBuf.from_numpy(_buf(max(nv, 1), dt))
    check(lib.wis_op_gemm_i8(0, *[i and i.ptr for i in ins], c_d.ptr if epi == 2 else None, c_d.ptr, v_d.ptr if nv else None, M, N, K, epi, flags, form, B, T, H, L,
                             M * 64 * H + 8, B * 64 * H * ((T + 63) // 64 * 64) + 8))
    buf = np.concatenate([c_d.to_numpy(dt, (nc,)), v_d.to_numpy(dt, (max(nv, 1),))])
    assert _kept(np.delete(buf, idx.ravel())), "wrote outside its outputs"
    return buf[idx].astype(np.float64), buf.view(np.uint8)


def gemm_case(lib, epi, form, m, n, k):
    """One case of the GEMM tap, random +-127 operands: m = M or (B, T), n = N or H, k = K or L (test_gpu_enc_i8.py's table has the legend).
    Nothing outside the outputs written, two runs equal word for word, and per element |out - ref| <= bound (test_gpu_enc_i8.py's docstring).
    -> the worst |out - ref| / bound"""
    from scipy.special import erf
    dims = (m[0], m[1], n, k) if epi >= 3 else (0, 0, 0, 0)
    M, N, K = (m[0] * m[1], (3 if epi == 3 else 2 * k) * 64 * n, 64 * n) if epi >= 3 else (m, n, k)
    rng = np.random.default_rng(epi * 1000 + form * 100 + M + N + K)
    A, Wq = rng.integers(-127, 128, (M, K), dtype=np.int8), rng.integers(-127, 128, (N, K), dtype=np.int8)
    sa, sw = rng.uniform(0.002, 0.02, M).astype(np.float32), rng.uniform(0.001, 0.004, N).astype(np.float32)
    bias, res = rng.standard_normal(N).astype(np.float32), (rng.standard_normal((M, N)).astype(np.float32) if epi == 2 else None)
    flags = 4 if (epi == 0 and form == 3) else 0      # the generic functor's fp32 output
    out, raw = _gemm(lib, epi, form, A, sa, Wq, sw, bias, res, flags, dims)
    assert np.array_equal(raw, _gemm(lib, epi, form, A, sa, Wq, sw, bias, res, flags, dims)[1]), "two runs differ"
    prod = (A.astype(np.float64) @ Wq.astype(np.float64).T) * (sa.astype(np.float64)[:, None] * sw.astype(np.float64)[None, :])
    S, pre = np.abs(prod) + np.abs(bias) + (np.abs(res) if epi == 2 else 0), prod + bias + (res if epi == 2 else 0)
    ref = 0.5 * pre * (1.0 + erf(pre / np.sqrt(2.0))) if epi == 1 else pre
    bound = (5 if epi == 2 else 4) * EPS * S * (GELU_LIP if epi == 1 else 1.0) + (0.0 if (epi == 2 or flags & 4) else F16_R * np.abs(ref))
    err = np.abs(out - ref)
    worst = float((err / bound).max())
    print(f"gemm_i8 epi {epi} form {form} M{M} N{N} K{K}: worst |out - ref| / bound = {worst:.3f}")
    assert np.isfinite(out).all() and (err <= bound).all(), worst
    return worst


@functools.lru_cache(maxsize=None)
def tiny_rig(golden_dir):
    """-> (weights, arch, mels [2][80][3000]: the 3.84 s clip and a rolled copy, references [2][1500][384] by name: the int8 rule in float64 / in
    float32, the unquantised encoder in float64).  Read-only: every test of the process shares the one result."""
    from enc_i8_ref import encode
    from wis_hip import weights as W
    mel = np.load(golden_dir + "/logmel_3sec.npz")["mel"].astype(np.float32)
    mels = np.ascontiguousarray(np.stack([mel, np.roll(mel, 53, axis=-1)]))
    w, a = W.synthetic_weights("tiny", seed=1234, std=0.02, emb_std=0.06, ln_jitter=0.1), W.arch("tiny")
    refs = {k: np.stack([encode(w, a, m, quant=q, dtype=dt) for m in mels]) for k, (q, dt) in
            {"q64": (True, np.float64), "q32": (True, np.float32), "f64": (False, np.float64)}.items()}
    for v in refs.values():
        v.setflags(write=False)
    return w, a, mels, refs


def rel(a, b):
    return float(np.linalg.norm(np.asarray(a, np.float64) - b) / np.linalg.norm(b))
