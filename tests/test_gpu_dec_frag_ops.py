"""-m gpu: the projection chain of the BATCHED decode step (dec_forward_frag, 9 .. 96 rows), one stage at a time and stage to stage, against float64 -
element by element.  The taps (include/wis_hip.h: wis_op_gemv_frag_stage, wis_op_dec_embed) assemble every stage with the builders the forward itself uses
(model.hip frag_resid / frag_ln_gelu_xf / frag_ln_f32, ffn2_ksplit); the kernel is launch_gemv_frag's choice.  What each case lands on (instantiations are
<row blocks, fragment ring depth, 8-bit weights>; the ring is 10 deep where a wave streams K / slices = 1280 columns, else 8 - 6 from four row blocks on in gemv_frag_kernel - and 6 / 4 in the two-tile kernel;
a kernel trace of this file confirmed the table: profiles/dec_frag_ops_tests.md):

  residual stage (GV_RESID: y in place + y_xf + stat_out), N = d = 384 (24 n-tiles) and 1280 (80), K = d and K = 4d, f16 and 8-bit weights
    M  9, 16   K = d    gemv_frag_kernel<1, 8 | 10>      one row block, grid (n-tiles, 1)
    M  9, 16   K = 4d   gemv_frag_kernel<1, 8>           grid (n-tiles, 2): the step's two K slices, merged in the launch by the last arriver;
                                                         explicit 1 slice: <1, 8>, 4 slices: <1, 8> at K = 1536, <1, 10> at K = 5120 (grid (n-tiles, 4))
    M 17       any K    gemv_frag_ms_kernel<1, 8 | 10>   M split INSTEAD of any K split (two row blocks, <= 85 n-tiles): grid (n-tiles, 1, 2), second block one row
    M 40                gemv_frag_ms_kernel<1, ..>       three groups of one row block
    M 49                gemv_frag_ms_kernel<2, ..>       2 + 2 row blocks
    M 80                gemv_frag_ms_kernel<2, ..>       2 + 2 + 1: the third group loads a valid block in its second place and discards the sums
    M 96                gemv_frag_ms_kernel<2, ..>       2 + 2 + 2
  LayerNorm-folded + GELU into a fragment image (GV_LN | GV_GELU, ymb), M = 9, 17, 48, 80
    N = 1536, K = 384   gemv_frag_kernel<1 | 2 | 3, 8>, <5, 6>   96 n-tiles: above the M split's 85, below the two-tile kernel's 256
    N = 5120, K = 1280  gemv_frag2_kernel<1 | 2 | 3 | 5, 6 | 4>  320 n-tiles, two per workgroup; f16 and 8-bit weights
  LayerNorm-folded, fp32 out (GV_LN | GV_OUT_F32), M = 9, 17, 48, 80
    N = 4128, K = 1280  gemv_frag2_kernel<..>            258 n-tiles: the smallest even count above 256
    N = 4112, K = 1280  gemv_frag_kernel<1 | 2 | 3, 10>, <5, 6>   257 n-tiles: odd, one tile per workgroup
    N = 1004, K = 384   gemv_frag_kernel<1, 8> at M = 9, gemv_frag_ms_kernel<1 | 2, 8> above (63 n-tiles); the last tile has 12 of its 16 columns
  embedding: dec_embed_kernel (x, optional f16 copy) at M = 1, 5, 8; dec_embed_xf_kernel (x, image, partials) at M = 9, 17, 96
  chains (producer's y_xf / stat_out handed to the consumer untouched): dec_embed_xf_kernel -> LN fp32 out; residual M 16, K = 4d (two-slice merge) -> FFN1;
    residual M 80 (ragged M-split group) -> FFN1; residual rows at 200 +- 2.4 -> LN fp32 out

References are float64 on exactly the values the kernels read: the f16 image values, W' = f16(W gamma) as fold_ln_kernel makes it (the exact product rounded
once; 8 bits: its rows quantised as weights.quantize_rows does), the column sums of THOSE values, b' = b + W beta, and mean / rstd merged in float64 from the fp32 partials the
consumer reads (xf_pack_kernel's: _partials32 below restates them bit for bit, which the embedding test pins on the same device function).

The bound has test_gpu_enc_ops.py's form:  |out - ref| <= r + c 2^-24 S,  r = 2^-10 |ref| for f16 outputs (0 for fp32), S = the sum of the absolute terms
of the expression evaluated - sum |w| |x| + |b| + |res| for a residual stage, rs (sum |w'| |x| + |mu| |c|) + |b'| for a folded one, times GELU's Lipschitz
constant 1.13 behind a GELU.  c is NOT taken from the kernels: _restate() below evaluates each stage in float32 the way the kernels are specified (exact
products; every wave's quarter of the k-steps accumulated k-step by k-step; the four waves, then the K slices in index order; the epilogue in float32) and
C_BOUND is four times its worst (|restatement - ref| - r) / (2^-24 S) per stage over this file's cases, rounded up to a power of two: a kernel may be four
times worse than a plain float32 evaluation of the same sums, no more.  `python tests/test_gpu_dec_frag_ops.py` prints those ratios (no GPU needed);
profiles/dec_frag_ops_tests.md records them beside what an MI355X showed."""
import ctypes as C
import functools

import numpy as np
import pytest

from test_gpu_dec_step_ops import _from_xf, _merge, _partials, xf_index

pytestmark = pytest.mark.gpu

F = np.float64
f32 = np.float32
EPS = 2.0 ** -24
F16_R = 2.0 ** -10
GELU_LIP = 1.13
WIS_E_UNSUPPORTED = -7      # include/wis_hip.h
RESID, LN_GELU, LN_F32 = 0, 1, 2      # wis_op_gemv_frag_stage's stages
# per stage: 4 x the float32 restatement's worst ratio over this file's cases, rounded up to a power of two (profiles/dec_frag_ops_tests.md)
C_BOUND = {RESID: 8, LN_GELU: 0.5, LN_F32: 8}
PAT16, PAT32 = 0x5A5A, 0x5A5A5A5A      # f16 203.25 / f32 1.5e16: nothing these stages produce
GUARD = 64                             # sentinel elements on either side of every output buffer

MS_ROWS = [9, 16, 17, 40, 49, 80, 96]
LN_ROWS = [9, 17, 48, 80]


def _pattern(n, dt):
    dt = np.dtype(dt)
    return np.full(n, PAT16 if dt.itemsize == 2 else PAT32, np.uint16 if dt.itemsize == 2 else np.uint32).view(dt)


def _bits(a):
    return a.view(np.uint16 if a.dtype.itemsize == 2 else np.uint32)


def _gelu(x):
    from scipy.special import erf
    return 0.5 * x * (1.0 + erf(x / np.sqrt(2.0)))


def _mm(a, b):
    """a [M][K] . b [N][K]^T in float64 (torch: the conftest keeps it to <= 16 threads)"""
    import torch
    return (torch.from_numpy(np.ascontiguousarray(a, F)) @ torch.from_numpy(np.ascontiguousarray(b, F)).T).numpy()


def _relerr(a, b):
    a, b = np.asarray(a, F), np.asarray(b, F)
    return float(np.linalg.norm(a - b) / (np.linalg.norm(b) + 1e-30))


class _Out:
    """an output buffer between two runs of sentinels; read() checks the sentinels and returns the body"""

    def __init__(self, body):
        from wis_hip._lib import DevBuf
        body = np.ascontiguousarray(body)
        self.dt, self.n = body.dtype, body.size
        pat = _pattern(GUARD, self.dt)
        self.buf = DevBuf.from_numpy(np.concatenate([pat, body.reshape(-1), pat]))
        self.ptr = C.c_void_p(self.buf.ptr.value + GUARD * self.dt.itemsize)

    @classmethod
    def filled(cls, n, dt):
        return cls(_pattern(n, dt))

    def read(self, shape):
        a = self.buf.to_numpy(self.dt, (self.n + 2 * GUARD,))
        pat = _bits(_pattern(GUARD, self.dt))
        assert np.array_equal(_bits(a[:GUARD]), pat) and np.array_equal(_bits(a[-GUARD:]), pat), "a store outside the output buffer"
        return a[GUARD:-GUARD].reshape(shape).copy()


def _image_rows(img, M, N, MB):
    """rows [M][N] of a fragment image that was filled with the sentinel; every element that belongs to no row < M must still hold it"""
    idx = xf_index(np.arange(M)[:, None], np.arange(N)[None, :], MB)
    rest = np.ones(img.size, bool)
    rest[idx.reshape(-1)] = False
    assert (_bits(img)[rest] == PAT16).all(), "a store outside the rows' places in the fragment image"
    clean = img.copy()
    _bits(clean)[rest] = 0
    return _from_xf(clean, M, N, MB)


def _xf_elems(K, MB):
    return (K // 32) * MB * 64 * 8


def _partials32(x):
    """xf_emit4 / the residual epilogue in float32, operation for operation (the library is built without FMA contraction): a lane's four columns
    (a + b) + (c + d), then the quad's lanes (q0 + q1) + (q2 + q3); the mean is that sum / 16; the squared deviations are summed the same way."""
    v = np.ascontiguousarray(x, f32).reshape(x.shape[0], -1, 4, 4)
    q = (v[..., 0] + v[..., 1]) + (v[..., 2] + v[..., 3])
    t1 = (q[..., 0] + q[..., 1]) + (q[..., 2] + q[..., 3])
    dv = v - (t1 * f32(0.0625))[..., None, None]
    sq = dv * dv
    p = (sq[..., 0] + sq[..., 1]) + (sq[..., 2] + sq[..., 3])
    t2 = (p[..., 0] + p[..., 1]) + (p[..., 2] + p[..., 3])
    return np.stack([t1, t2], -1).astype(f32)


# ---- inputs and float64 references --------------------------------------------------------
@functools.lru_cache(maxsize=3)
def _matrix(N, K, w8, fold, exact=False):
    """one projection: W f16 [N][K], bias, gamma, beta and what the kernel streams - Wd [N][K] float64 (de-quantised under w8; the gamma-folded matrix when
    fold), its magnitudes, the column sums and bias the epilogue uses, in float64; q / sc: the 8-bit rows and their scales."""
    from wis_hip.weights import quantize_rows
    rng = np.random.default_rng(7 * N + K + 2 * w8 + fold + 5 * exact)
    if exact:
        # every row: one entry of +-1/8 in each sixteenth of K (every wave of every K slice adds something) and 127/512 in column 0, which sets the 8-bit row
        # scale to 2^-9 exactly (1/8 = 64 steps); the activations of column 0 are zero
        W = np.zeros((N, K), np.float16)
        cols = 1 + rng.integers(0, K // 16 - 1, size=(N, 16)) + (K // 16) * np.arange(16)[None, :]
        W[np.arange(N)[:, None], cols] = rng.choice([-0.125, 0.125], size=(N, 16))
        W[:, 0] = 127.0 / 512.0
        bias = (rng.integers(-4, 5, size=N) / 4.0).astype(f32)
    else:
        W = (rng.standard_normal((N, K)) * 0.05).astype(np.float16)
        bias = rng.standard_normal(N).astype(f32)
    g = (1 + 0.1 * rng.standard_normal(K)).astype(f32)
    be = (0.1 * rng.standard_normal(K)).astype(f32)
    # fold_ln_kernel's f16(W gamma): the compiled kernel multiplies and converts in ONE instruction (v_fma_mixlo_f16), i.e. the exact product rounded once.
    # Rounding through float32 first gives another f16 value in ~1e-4 of the elements - one f16 step of one weight is 30 .. 500 x 2^-24 S here, and a
    # different 8-bit step after quantisation thousands - so the reference has to round the way the kernel does
    Ws = (W.astype(F) * g.astype(F)).astype(np.float16) if fold else W
    q = sc = None
    if w8:
        q, sc = quantize_rows(Ws)
        Wd = q.astype(F) * sc.astype(F)[:, None]
    else:
        Wd = Ws.astype(F)
    cs = Wd.sum(1)
    bf = bias.astype(F) + (W.astype(F) @ be.astype(F) if fold else 0.0)
    return dict(W=W, bias=bias, g=g, be=be, Ws=Ws, Wd=Wd, Wa=np.abs(Wd), cs=cs, bf=bf, q=q, sc=sc, N=N, K=K, w8=w8, fold=fold)


def _resid_inputs(M, N, K, exact=False):
    rng = np.random.default_rng(31 * M + N + K + exact)
    if exact:      # x in {-2, 0, 2}: every product +-1/4; rows of multiples of 1/4 at 200 +- 2 (the out-cq test's rows): all sums and both partials exact in fp32
        x = (2 * rng.integers(-1, 2, size=(M, K))).astype(np.float16)
        x[:, 0] = 0
        res = (200.0 + rng.integers(-8, 9, size=(M, N)) / 4.0).astype(f32)
    else:
        x = rng.standard_normal((M, K)).astype(np.float16)
        res = rng.standard_normal((M, N)).astype(f32)
    return x, res


def _resid_ref(m, x, res):
    x64 = x.astype(F)
    ref = res.astype(F) + _mm(x64, m["Wd"]) + m["bf"]
    S = _mm(np.abs(x64), m["Wa"]) + np.abs(m["bf"]) + np.abs(res.astype(F))
    return ref, S


def _ln_inputs(M, K):
    rng = np.random.default_rng(17 * M + K)
    return (rng.standard_normal((M, K)) * 2 + 0.3).astype(f32)


def _ln_ref(m, x16, stat, gelu):
    """y = rs (W' x - mu c) + b' on the f16 image values x16, mean / rstd merged in float64 from the fp32 partials `stat`; returns (ref, unit = 2^-24 S ...)"""
    mu, rs = _merge(stat)
    x64 = x16.astype(F)
    pre = rs * (_mm(x64, m["Wd"]) - mu * m["cs"]) + m["bf"]
    S = rs * (_mm(np.abs(x64), m["Wa"]) + np.abs(mu) * np.abs(m["cs"])) + np.abs(m["bf"])
    return (_gelu(pre), S * GELU_LIP) if gelu else (pre, S)


def _ratio(out, ref, S, f16_out):
    err = np.abs(out.astype(F) - ref)
    r = F16_R * np.abs(ref) if f16_out else 0.0
    return np.maximum(err - r, 0.0) / (EPS * S)


def _check(tag, stage, out, ref, S, f16_out):
    ratio = _ratio(out, ref, S, f16_out)
    worst = float(ratio.max())
    i = tuple(int(v) for v in np.unravel_index(int(ratio.argmax()), ratio.shape))
    print(f"{tag}: max (|out - ref| - r) / (2^-24 S) = {worst:.3f} at {i} (c = {C_BOUND[stage]}); rel-L2 {_relerr(out, ref):.3e}")
    assert np.isfinite(out.astype(F)).all(), tag
    if worst > C_BOUND[stage]:
        bad = np.argwhere(ratio > C_BOUND[stage])
        print(f"{tag}: {len(bad)} elements over the bound; the first: " + ", ".join(f"{tuple(int(v) for v in q)}: out {float(out[tuple(q)])!r} ref {float(ref[tuple(q)])!r}" for q in bad[:8]))
    assert worst <= C_BOUND[stage], (tag, worst, C_BOUND[stage], i)
    return worst


# ---- the float32 restatement (CPU): what C_BOUND is derived from --------------------------
def _restate_gemm(x16, m, ks):
    """sum_k w x in float32 the way gemv_frag_body is specified: products exact, one MFMA = the exact 32-term dot added to the wave's accumulator (one
    rounding per k-step), wave w of slice s owns the k-steps [(4 s + w) S, (4 s + w + 1) S), S = K / (128 ks); then ((w0 + w1) + w2) + w3 and the slices
    in index order; 8-bit weights: the integer rows, times the row scale afterwards."""
    M, K = x16.shape
    Wt = m["q"].astype(F) if m["w8"] else m["Ws"].astype(F)
    N, ksteps = Wt.shape[0], K // 32
    S = ksteps // (4 * ks)
    P = np.matmul(x16.astype(F).reshape(M, ksteps, 32).transpose(1, 0, 2), Wt.reshape(N, ksteps, 32).transpose(1, 2, 0))      # [ksteps][M][N]: exact dots
    tot = None
    for s in range(ks):
        acc4 = None
        for w in range(4):
            acc = np.zeros((M, N), f32)
            for u in range(S):
                acc = (acc.astype(F) + P[(4 * s + w) * S + u]).astype(f32)
            acc4 = acc if acc4 is None else acc4 + acc
        tot = acc4 if tot is None else tot + acc4
    if m["w8"]:
        tot = tot * m["sc"].astype(f32)[None, :]
    return tot.astype(f32)


def _wave_sum32(v):
    """[N][64] float32 lane values -> butterfly sum"""
    n = 64
    while n > 1:
        n //= 2
        v = v[:, :n] + v[:, n:2 * n]
    return v[:, 0]


def _restate_fold(m):
    """fold_ln_kernel / csum8_kernel in float32: lane l sums the columns l, l + 64, ... in order, then the wave; b' = b + W beta, c = sum W' (8 bits: the
    integer sum times the row scale)."""
    N, K = m["N"], m["K"]
    W32, be = m["W"].astype(f32), m["be"]
    c = np.zeros((N, 64), f32); wb = np.zeros((N, 64), f32)
    for j in range(K // 64):
        sl = slice(64 * j, 64 * j + 64)
        c = c + m["Ws"][:, sl].astype(f32)
        wb = wb + W32[:, sl] * be[sl]
    cs = _wave_sum32(c)
    if m["w8"]:
        cs = m["q"].astype(F).sum(1).astype(f32) * m["sc"]
    return cs, m["bias"] + _wave_sum32(wb)


def _restate_stats(stat, K):
    """the consumer's merge of the row partials in float32: per quarter of the tiles sequentially about c = the first tile's mean, then (q0 + q1) + (q2 + q3)"""
    s, m2 = stat[..., 0].astype(f32), stat[..., 1].astype(f32)
    nq = K // 64
    c = s[:, 0] * f32(0.0625)
    t1 = []; t2 = []
    for kq in range(4):
        a1 = np.zeros(s.shape[0], f32); a2 = np.zeros(s.shape[0], f32)
        for i in range(nq):
            dm = s[:, kq * nq + i] * f32(0.0625) - c
            a1 = a1 + dm
            a2 = a2 + (m2[:, kq * nq + i] + f32(16.0) * dm * dm)
        t1.append(a1); t2.append(a2)
    t1 = (t1[0] + t1[1]) + (t1[2] + t1[3]); t2 = (t2[0] + t2[1]) + (t2[2] + t2[3])
    invK = f32(1.0) / f32(K)
    dmu = t1 * f32(16.0) * invK
    mu = c + dmu
    rs = f32(1.0) / np.sqrt(np.maximum(t2 * invK - dmu * dmu, f32(0.0)) + f32(1e-5))
    return mu[:, None].astype(f32), rs[:, None].astype(f32)


def _restate(stage, m, x, res=None, stat=None, ks=1):
    """the whole stage in float32; x: the f16 image values"""
    s = _restate_gemm(x, m, ks)
    if stage == RESID:
        return res + (s + m["bias"][None, :])
    cs, bf = _restate_fold(m)
    mu, rs = _restate_stats(stat, m["K"])
    pre = rs * (s - mu * cs[None, :]) + bf[None, :]
    if stage == LN_F32:
        return pre
    return _gelu_as32(pre).astype(np.float16)


def _gelu_as32(x):
    """common.hpp gelu_erf in float32: erf by Abramowitz & Stegun 7.1.26 (|error| <= 1.5e-7) - the expression the kernels evaluate; the reference is the true GELU"""
    z = x * f32(0.70710678118654752440)
    az = np.abs(z)
    t = f32(1.0) / (f32(0.3275911) * az + f32(1.0))
    p = f32(1.061405429) * t + f32(-1.453152027)
    for k in (1.421413741, -0.284496736, 0.254829592):
        p = p * t + f32(k)
    r = f32(1.0) - p * t * np.exp(-az * az)
    return (f32(0.5) * x * (f32(1.0) + np.copysign(r, z))).astype(f32)


# ---- the cases ----------------------------------------------------------------------------
# (N, K): d x d and FFN2 at d = 384 and 1280
_RESID_SHAPES = [(384, 384), (1280, 1280), (384, 1536), (1280, 5120)]
# ksplit: the d x d stages ask for none (1), as the step does; FFN2 asks for the step's own (-1: ffn2_ksplit), and for 1 and 4 explicitly where a K split is
# honoured at all (one row block)
_RESID_CASES = [(M, N, K, w8, -1 if K > N else 1) for (N, K) in _RESID_SHAPES for w8 in (0, 1) for M in MS_ROWS] + \
               [(M, N, K, w8, ks) for (N, K) in _RESID_SHAPES[2:] for w8 in (0, 1) for M in (9, 16) for ks in (1, 4)]
_EXACT_CASES = [(M, N, K, w8, ks) for (N, K, ks) in ((384, 384, 1), (1280, 5120, -1), (1280, 5120, 4)) for w8 in (0, 1) for M in (9, 16, 17, 80)]
_LN_CASES = [(LN_GELU, M, 1536, 384, w8) for w8 in (0, 1) for M in LN_ROWS] + [(LN_GELU, M, 5120, 1280, w8) for w8 in (0, 1) for M in LN_ROWS] + \
            [(LN_F32, M, N, K, w8) for (N, K, w8) in ((4128, 1280, 0), (4128, 1280, 1), (4112, 1280, 0), (1004, 384, 0)) for M in LN_ROWS]


def _slices(ksplit, M, N, K):
    """K slices the launch really uses: the step's FFN2 asks for two where K / 128 is even; launch_gemv_frag honours a split at one row block only
    (from two row blocks on and <= 85 n-tiles the M split takes over)"""
    ks = ksplit if ksplit > 0 else (2 if (K // 32) % 8 == 0 else 1)
    return ks if M <= 16 else 1


# ---- calling the taps ---------------------------------------------------------------------
def _dev(a):
    from wis_hip._lib import DevBuf
    return DevBuf.from_numpy(a)


def _p(b):
    return b.ptr if b is not None else None


def _call_stage(lib, stage, m, M, x=None, image=None, stat_in=None, res=None, ksplit=-1, want_image=True, want_stat=True, xmb=0, raw=False):
    """one call of the tap on fresh output buffers; returns (y, image rows or None, stat or None, raw image or None).  x: row-major rows; image (+ stat_in): a
    producer's outputs on the device."""
    from wis_hip._lib import check
    N, K, MB = m["N"], m["K"], (M + 15) // 16
    keep = [_dev(m["W"]), _dev(m["bias"]), _dev(m["g"]), _dev(m["be"])]
    d_x = _dev(x) if image is None else image
    y = _Out(res) if stage == RESID else (_Out.filled(M * N, f32) if stage == LN_F32 else None)
    y_xf = _Out.filled(_xf_elems(N, MB), np.float16) if (stage == LN_GELU or (stage == RESID and want_image)) else None
    st = _Out.filled(M * (N // 16) * 2, f32) if (stage == RESID and want_stat) else None
    rc = lib.wis_op_gemv_frag_stage(0, stage, d_x.ptr, int(image is not None), xmb, _p(stat_in), keep[2].ptr, keep[3].ptr, keep[0].ptr, keep[1].ptr, m["w8"],
                                    _p(y), _p(y_xf), _p(st), M, N, K, ksplit)
    if raw:
        return rc, y, y_xf, st
    check(rc)
    img = y_xf.read((_xf_elems(N, MB),)) if y_xf else None
    return (y.read((M, N)) if y else None, _image_rows(img, M, N, MB) if y_xf else None, st.read((M, N // 16, 2)) if st else None, (y_xf, st))


# ---- residual stage -----------------------------------------------------------------------
def _resid_case(lib, M, N, K, w8, ksplit, exact):
    m = _matrix(N, K, w8, 0, exact)
    x, res = _resid_inputs(M, N, K, exact)
    ref, S = _resid_ref(m, x, res)
    runs = [_call_stage(lib, RESID, m, M, x=x, res=res, ksplit=ksplit)[:3] for _ in range(3)]
    y, rows, stat = runs[0]
    for other in runs[1:]:      # the slices are added in index order whichever arrives last; the tickets re-arm
        assert all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(runs[0], other)), "repeats differ"
    tag = f"resid M{M} N{N} K{K} w8={w8} ksplit={ksplit}{' exact' if exact else ''}"
    worst = _check(tag, RESID, y, ref, S, False)
    assert np.array_equal(_bits(rows), _bits(y.astype(np.float16))), "y_xf is not the f16 rounding of the y this launch stored"
    pref = _partials(y)
    ds = float(np.abs(stat[..., 0] - pref[..., 0]).max()); dm = np.abs(stat[..., 1] - pref[..., 1])
    print(f"{tag} partials: sums off by {ds:.3e}, M2 by {float((dm / pref[..., 1].max(1, keepdims=True)).max()):.3e} of the row's largest")
    if exact:
        assert np.array_equal(y.astype(F), ref), "sums of exactly representable terms"
        assert np.array_equal(stat.astype(F), pref)
    else:       # test_gpu_dec_step_ops._out_cq_case's bounds for the same partial arithmetic
        assert ds <= 16 * 2.0 ** -23 * float(np.abs(y).max())
        assert (dm <= 1e-5 * pref[..., 1].max(1, keepdims=True)).all()
    return worst


@pytest.mark.parametrize("M,N,K,w8,ksplit", _RESID_CASES)
def test_residual_stage_vs_fp64(M, N, K, w8, ksplit, lib):
    """y = res + x W^T + b element by element, y_xf bit-equal to f16(y), nothing else of the image touched, stat_out against float64 partials of the stored y,
    three calls (six launches with a K split) bit-identical."""
    _resid_case(lib, M, N, K, w8, ksplit, False)


@pytest.mark.parametrize("M,N,K,w8,ksplit", _EXACT_CASES)
def test_residual_stage_is_exact_on_representable_rows(M, N, K, w8, ksplit, lib):
    """weights of +-1/8 (8 bits: a row scale of exactly 2^-9), activations in {-2, 0, 2}, rows of multiples of 1/4 near 200: every sum, in any order, and
    both partials are exact in fp32 - y and stat_out equal float64 bit for bit (M2 about zero instead of the tile mean would need 31 bits here)."""
    _resid_case(lib, M, N, K, w8, ksplit, True)


# ---- LayerNorm-folded stages --------------------------------------------------------------
@pytest.mark.parametrize("stage,M,N,K,w8", _LN_CASES)
def test_folded_stage_vs_fp64(stage, M, N, K, w8, lib):
    """rs (W' x - mu c) + b' (then GELU into the fragment image, or fp32 rows) on rows packed by launch_xf_pack; twice, bit-identical."""
    m = _matrix(N, K, w8, 1)
    x = _ln_inputs(M, K)
    ref, S = _ln_ref(m, x.astype(np.float16), _partials32(x), stage == LN_GELU)
    a, b = (_call_stage(lib, stage, m, M, x=x)[:2] for _ in range(2))
    out = a[1] if stage == LN_GELU else a[0]
    assert np.array_equal(_bits(out), _bits(b[1] if stage == LN_GELU else b[0])), "repeats differ"
    _check(f"{'ffn1+gelu' if stage == LN_GELU else 'ln f32'} M{M} N{N} K{K} w8={w8}", stage, out, ref, S, stage == LN_GELU)


# ---- chains: a producer's image and partials are the consumer's input ---------------------
def _chain_bar(tag, out, ref, f16_out):
    e = _relerr(out, ref); worst = float(np.abs(out.astype(F) - ref).max())
    print(f"{tag}: rel err {e:.3e} max abs {worst:.3e}")
    assert e < 2e-3, (tag, e)                                            # test_gemv_layernorm_rows_with_a_large_common_offset's bar
    assert worst < 0.05 * (1 + float(np.abs(ref).max())), (tag, worst)   # test_gemv: no single corrupted element hiding inside the norm


def _true_ln(y64, m):
    """LayerNorm in float64 of float64 rows, then the UN-folded projection"""
    mu = y64.mean(1, keepdims=True); var = y64.var(1, keepdims=True)
    return _mm((y64 - mu) / np.sqrt(var + 1e-5) * m["g"].astype(F) + m["be"].astype(F), m["W"].astype(F)) + m["bias"].astype(F)


def _chain(lib, tag, M, prod, x, res, ksplit, cons_stage, cons):
    _, _, _, (d_img, d_stat) = _call_stage(lib, RESID, prod, M, x=x, res=res, ksplit=ksplit)
    y, rows, _, _ = _call_stage(lib, cons_stage, cons, M, image=d_img, stat_in=d_stat)
    d_img.read((d_img.n,)); d_stat.read((d_stat.n,))      # (the consumer left them alone: sentinels intact)
    y_ref = res.astype(F) + _mm(x.astype(F), prod["W"].astype(F)) + prod["bias"].astype(F)
    ref = _true_ln(y_ref, cons)
    if cons_stage == LN_GELU:
        _chain_bar(tag, rows, _gelu(ref), True)
    else:
        _chain_bar(tag, y, ref, False)


@pytest.mark.parametrize("d", [384, 1280])
def test_chain_two_slice_ffn2_feeds_ffn1(d, lib):
    """FFN2 at 16 rows (gemv_frag_kernel, the step's two K slices) -> its y_xf and stat_out -> the next layer's-style folded projection with GELU"""
    x, res = _resid_inputs(16, d, 4 * d)
    _chain(lib, f"chain ffn2(2 slices) -> ffn1 d{d}", 16, _matrix(d, 4 * d, 0, 0), x, res, -1, LN_GELU, _matrix(4 * d, d, 0, 1))


@pytest.mark.parametrize("d", [384, 1280])
def test_chain_ragged_m_split_feeds_ffn1(d, lib):
    """a d x d residual stage at 80 rows (gemv_frag_ms_kernel<2>, groups of 2 + 2 + 1 row blocks) -> FFN1 with GELU"""
    x, res = _resid_inputs(80, d, d)
    _chain(lib, f"chain resid(M split 2+2+1) -> ffn1 d{d}", 80, _matrix(d, d, 0, 0), x, res, 1, LN_GELU, _matrix(4 * d, d, 0, 1))


@pytest.mark.parametrize("M", [16, 40])
def test_chain_rows_with_a_large_common_offset(M, lib):
    """the producer leaves rows at 200 +- 2.4, multiples of 1/4 (exact in f16, so its image costs nothing): the consumer has to survive the
    E[x^2] - mean^2 cancellation with partials that came from a residual EPILOGUE, merged about the first tile's mean"""
    d = 1280
    prod = _matrix(d, d, 0, 0, True)
    rng = np.random.default_rng(11 + M)
    x = (2 * rng.integers(-1, 2, size=(M, d))).astype(np.float16); x[:, 0] = 0
    res = (200.0 + rng.integers(-16, 17, size=(M, d)) / 4.0).astype(f32)
    res[:, ::7] += 8.0          # tile means differ from the row mean
    _chain(lib, f"chain rows at 200 -> ln f32 M{M}", M, prod, x, res, 1, LN_F32, _matrix(d, d, 0, 1))


# ---- embedding ------------------------------------------------------------------------------
@functools.lru_cache(maxsize=2)
def _tables(n_vocab, d):
    """embedding tables: random rows where the tests look (first, last, a few between), zero elsewhere"""
    rng = np.random.default_rng(n_vocab + d)
    emb = np.zeros((n_vocab, d), np.float16)
    used = np.unique(np.concatenate([[0, n_vocab - 1], rng.integers(0, n_vocab, size=96)]))
    emb[used] = (rng.standard_normal((used.size, d)) * 0.06).astype(np.float16)
    pos = (rng.standard_normal((448, d)) * 0.02).astype(np.float16)
    return emb, pos, used, _dev(emb), _dev(pos)


def _embed_rows(M, used, n_vocab, seed):
    rng = np.random.default_rng(seed)
    tok = rng.choice(used, size=M).astype(np.int32)
    pos = rng.integers(0, 448, size=M).astype(np.int32)
    tok[0], pos[0] = n_vocab - 1, 447
    if M > 1:
        tok[-1], pos[-1] = 0, 0
    return tok, pos


def _embed_call(lib, d_emb, d_pos, tok, pos, M, d, n_vocab, form):
    """form: "x" | "xh" (dec_embed_kernel without / with the f16 copy) | "xf" (dec_embed_xf_kernel)"""
    from wis_hip._lib import check
    MB = (M + 15) // 16
    x = _Out.filled(M * d, f32)
    xh = _Out.filled(M * d, np.float16) if form == "xh" else None
    xf = _Out.filled(_xf_elems(d, MB), np.float16) if form == "xf" else None
    st = _Out.filled(M * (d // 16) * 2, f32) if form == "xf" else None
    ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))
    check(lib.wis_op_dec_embed(0, d_emb.ptr, d_pos.ptr, ip(tok), ip(pos), x.ptr, _p(xh), _p(xf), _p(st), M, d, n_vocab, 448))
    return x, xh, xf, st


@pytest.mark.parametrize("n_vocab", [51865, 51866])
@pytest.mark.parametrize("d", [384, 1280])
def test_embedding_kernels_bit_exact(d, n_vocab, lib):
    """x = E[tok] + P[pos]: f16 + f16 is exact in fp32, so x is compared bit for bit; the f16 copy / image is its rounding; the partials are the float32
    evaluation in the kernel's order; image rows >= M and everything around the buffers keep their sentinel.  Tokens 0 and n_vocab - 1, positions 0 and 447."""
    emb, pe, used, d_emb, d_pos = _tables(n_vocab, d)
    for M in (1, 5, 8, 9, 17, 96):
        tok, pos = _embed_rows(M, used, n_vocab, 3 * M + d)
        want = emb[tok].astype(f32) + pe[pos].astype(f32)
        assert np.array_equal(want.astype(F), emb[tok].astype(F) + pe[pos].astype(F))
        for form in (("x", "xh") if M <= 8 else ("xf",)):
            x, xh, xf, st = _embed_call(lib, d_emb, d_pos, tok, pos, M, d, n_vocab, form)
            got = x.read((M, d))
            assert np.array_equal(_bits(got), _bits(want)), (M, form)
            if xh:
                assert np.array_equal(_bits(xh.read((M, d))), _bits(want.astype(np.float16)))
            if xf:
                MB = (M + 15) // 16
                assert np.array_equal(_bits(_image_rows(xf.read((xf.n,)), M, d, MB)), _bits(want.astype(np.float16)))
                assert np.array_equal(_bits(st.read((M, d // 16, 2))), _bits(_partials32(want))), "partials differ from the float32 evaluation in the kernel's order"


def test_embedding_out_of_range_rows_are_refused(lib):
    from wis_hip._lib import WisError
    emb, pe, used, d_emb, d_pos = _tables(51865, 384)
    for tok, pos in (([51865], [0]), ([0], [448]), ([-1], [0])):
        with pytest.raises(WisError):
            _embed_call(lib, d_emb, d_pos, np.array(tok, np.int32), np.array(pos, np.int32), 1, 384, 51865, "x")


@pytest.mark.parametrize("M,d", [(10, 384), (40, 1280)])
def test_chain_embedding_feeds_folded_projection(M, d, lib):
    """dec_embed_xf_kernel's image and partials straight into a LayerNorm-folded fp32-out stage (what the first layer's projections read)"""
    n_vocab = 51865
    emb, pe, used, d_emb, d_pos = _tables(n_vocab, d)
    tok, pos = _embed_rows(M, used, n_vocab, M + d)
    x, _, xf, st = _embed_call(lib, d_emb, d_pos, tok, pos, M, d, n_vocab, "xf")
    cons = _matrix(d, d, 0, 1)
    y = _call_stage(lib, LN_F32, cons, M, image=xf, stat_in=st)[0]
    xf.read((xf.n,)); st.read((st.n,))
    _chain_bar(f"chain embed -> ln f32 M{M} d{d}", y, _true_ln(emb[tok].astype(F) + pe[pos].astype(F), cons), False)


# ---- what launch_gemv_frag refuses ----------------------------------------------------------
def test_unsupported_stages_are_errors(lib):
    """the launcher's own answers, through the tap: nothing is launched, every output keeps its sentinel"""
    from wis_hip._lib import DevBuf

    def refused(what, stage, m, M, **kw):
        rc, y, y_xf, st = _call_stage(lib, stage, m, M, raw=True, **kw)
        assert rc == WIS_E_UNSUPPORTED, (what, rc, lib.wis_last_error())
        for o in (y, y_xf, st):
            if o is y and stage == RESID:
                assert np.array_equal(_bits(o.read((o.n,))), _bits(kw["res"].reshape(-1))), what      # the residual rows as they were
            elif o is not None:
                assert (_bits(o.read((o.n,))) == (PAT16 if o.dt.itemsize == 2 else PAT32)).all(), what
    x16, res = _resid_inputs(16, 1004, 384)
    refused("residual rows with N % 16 != 0", RESID, _matrix(1004, 384, 0, 0), 16, x=x16, res=res)
    refused("a K split behind a folded LayerNorm", LN_F32, _matrix(384, 1280, 0, 1), 16, x=_ln_inputs(16, 1280), ksplit=2)      # (K / 32 = 40: two slices would divide)
    m = _matrix(384, 384, 0, 0)
    img = DevBuf.from_numpy(np.zeros(_xf_elems(384, 3), np.float16))
    refused("an image of more row blocks than ceil(M / 16)", RESID, m, 16, image=img, res=_resid_inputs(16, 384, 384)[1], xmb=2)
    x97, res97 = _resid_inputs(97, 384, 384)
    refused("more than 96 rows", RESID, m, 97, x=x97, res=res97)


# ---- `python tests/test_gpu_dec_frag_ops.py`: the float32 restatement's ratios, per stage (CPU only) ------------------------
def _restatement_ratios():
    worst = {RESID: 0.0, LN_GELU: 0.0, LN_F32: 0.0}
    for (M, N, K, w8, ksplit) in _RESID_CASES:
        m = _matrix(N, K, w8, 0)
        x, res = _resid_inputs(M, N, K)
        ref, S = _resid_ref(m, x, res)
        r = float(_ratio(_restate(RESID, m, x, res=res, ks=_slices(ksplit, M, N, K)), ref, S, False).max())
        print(f"resid M{M} N{N} K{K} w8={w8} slices={_slices(ksplit, M, N, K)}: {r:.3f}", flush=True)
        worst[RESID] = max(worst[RESID], r)
    for (stage, M, N, K, w8) in _LN_CASES:
        m = _matrix(N, K, w8, 1)
        x = _ln_inputs(M, K)
        stat = _partials32(x)
        ref, S = _ln_ref(m, x.astype(np.float16), stat, stage == LN_GELU)
        r = float(_ratio(_restate(stage, m, x.astype(np.float16), stat=stat), ref, S, stage == LN_GELU).max())
        print(f"{'ffn1+gelu' if stage == LN_GELU else 'ln f32'} M{M} N{N} K{K} w8={w8}: {r:.3f}", flush=True)
        worst[stage] = max(worst[stage], r)
    for stage, name in ((RESID, "residual"), (LN_GELU, "LN + GELU -> image"), (LN_F32, "LN -> fp32")):
        c = 2.0 ** -6
        while c < 4 * worst[stage]:
            c *= 2
        print(f"{name}: worst restatement ratio {worst[stage]:.3f} -> c = {c} (C_BOUND has {C_BOUND[stage]})")


if __name__ == "__main__":
    import os
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path[:0] = [root, os.path.join(root, "willow-inference-server_amd")]
    _restatement_ratios()
