"""The load-time weight preparation (csrc/model.hip prep_projection / build_cq_fold; csrc/dec_kernels.hip fold_ln_kernel, pack_gemv_kernel, row_scale_kernel,
pack_gemv8_kernel, csum8_kernel) as a numpy specification, the deliberately wrong variants that tests/test_prep_ref_cpu.py tells apart from it, and the seeded
input families shared by that test and tests/test_gpu_prep_ops.py.

Exact outputs (compared word for word): the folded staging, the f16 image, the 8-bit image, the row scales, the 8-bit column sums.  numpy's float32 products,
quotients and float32 -> float16 casts are IEEE round-to-nearest-even, subnormals included; the library is built without fast-math and without contraction.
Bounded outputs: the column sums and the bias addend of the fold, W'q bo, and the product half of the cross-Q fold - sums whose ORDER belongs to the kernel.
Their references are float64 sums of the very fp32 terms the kernel adds, and the bounds are derived, not measured:

  a wave's sum of K terms: a lane adds its ceil(K / 64) terms in turn, six more additions close the wave (four inside a row of sixteen lanes, two across the rows):
  ceil(K / 64) + 5 roundings on any term's path, each relative 2^-24.  ACC(K) = (ceil(K / 64) + 7) 2^-24 sum |term| holds that with the second-order terms, and
  the stored word is one more fp32 rounding of the result (c * qscale and wb * qscale are exact: qscale is a power of two).
  the product half of the cross-Q fold: one f16 rounding of the GEMM's fp32 sum, whose order the GEMM owns: 2^-11 |P| + d 2^-24 sum |term|."""
import numpy as np

f32, f16, F = np.float32, np.float16, np.float64
U32, U24 = 2.0 ** -24, 2.0 ** -24      # fp32 unit roundoff
U16 = 2.0 ** -11                       # f16 unit roundoff
SENTINEL = 0x7fc5a5a5                  # include/wis_hip.h WIS_PREP_CSUM_SENTINEL


def _pow2(x):
    m, _ = np.frexp(float(x))
    return m == 0.5


def words16(a):
    """the f16 words of a staging or an image, a negative zero written as zero.  The sign of a zero is the one thing these comparisons leave open:
    v_fma_mixlo_f16 (fold() below) gets a +0 addend from hipcc, so a product that is exactly zero under a negative sign - a zero gamma, a negative weight -
    comes out as +0 where IEEE multiplication gives -0.  No consumer can tell the two zeros apart: the MFMA adds +-0 to a sum, rint(+-0) is the 8-bit value 0,
    and c starts from +0.  Every non-zero word, subnormals included, is compared as it is."""
    v = np.ascontiguousarray(a).view(np.uint16).copy()
    v[v == 0x8000] = 0
    return v


def row_factor(N, n_scale, qscale):
    f = np.ones(N, f32)
    f[:n_scale] = f32(qscale)
    return f


# ---- fold --------------------------------------------------------------------------------------------------------------------------------------------------
def fold(W, gamma):
    """W' = f16(W * gamma), the EXACT product (35 bits: float64 holds it) rounded to f16 once, to nearest even: exact.  This is what the compiled
    fold_ln_kernel stores - hipcc turns its (f16)(w * gamma[k]) into one v_fma_mixlo_f16 - and what tests/test_gpu_dec_frag_ops.py and DESIGN.md already pin;
    fold_f32 below, the source's reading and the host-side quantize_folded's, gives another f16 word for about one weight in 10^4 (profiles/prep_tests.md)."""
    return (W.astype(F) * np.asarray(gamma, f32).astype(F)[None, :]).astype(f16)


def fold_f32(W, gamma):
    """f16(f32(W) * gamma) with the product rounded to fp32 first: wis_hip.weights.quantize_folded's formula, NOT the device's word everywhere"""
    return (W.astype(f32) * np.asarray(gamma, f32)[None, :]).astype(f16)


def acc_bound(abs_sum, K):
    return (-(-K // 64) + 7) * U32 * abs_sum


def _sum_ref(terms, K, f, addend=None):
    """float64 sum of fp32 terms per row, times the row factor (+ addend) -> (reference, bound): ACC(K) and one fp32 rounding of the stored result"""
    assert terms.dtype == f32
    s = terms.sum(axis=1, dtype=F) * f.astype(F)
    a = acc_bound(np.abs(terms).sum(axis=1, dtype=F), K) * f.astype(F)
    ref = s if addend is None else s + addend.astype(F)
    return ref, a + U32 * (np.abs(ref) + a)


def fold_sums(W, gamma, beta, bias_in, n_scale, qscale, c_terms=None):
    """-> (c_ref, c_bound, b_ref, b_bound): c from the ROUNDED products (what the MFMA multiplies), the bias addend from the fp32 products f32(W) * beta; rows
    < n_scale hold c * qscale and bias_in + wb * qscale"""
    assert _pow2(qscale)
    N, K = W.shape
    f = row_factor(N, n_scale, qscale)
    ct = fold(W, gamma).astype(f32) if c_terms is None else c_terms
    c, cb = _sum_ref(ct, K, f)
    b, bb = _sum_ref(W.astype(f32) * np.asarray(beta, f32)[None, :], K, f, np.asarray(bias_in, f32))
    return c, cb, b, bb


def csum_unrounded(W, gamma, beta, bias_in, n_scale, qscale):
    """WRONG: the column sums taken from the fp32 products, before their rounding to f16"""
    return fold_sums(W, gamma, beta, bias_in, n_scale, qscale, c_terms=W.astype(f32) * np.asarray(gamma, f32)[None, :])


# ---- the f16 image -----------------------------------------------------------------------------------------------------------------------------------------
def _image(a, rows):
    """[Npad][K] -> pack_gemv_kernel's order [Npad/rows][K/32][4 k-quarters][rows][8]"""
    Npad, K = a.shape
    assert Npad % rows == 0 and K % 32 == 0
    return np.ascontiguousarray(a.reshape(Npad // rows, rows, K // 32, 4, 8).transpose(0, 2, 3, 1, 4)).reshape(-1)


def scaled_rows(Wst, Npad, n_scale, scale):
    """rows < n_scale: f16(f32(w) * scale) - a second rounding where the product is an f16 subnormal; rows >= N: zero"""
    N, K = Wst.shape
    out = np.zeros((Npad, K), f16)
    out[:N] = Wst
    out[:n_scale] = (Wst[:n_scale].astype(f32) * f32(scale)).astype(f16)
    return out


def pack(Wst, Npad, rows, n_scale, scale):
    return _image(scaled_rows(Wst, Npad, n_scale, scale), rows)


def pack_scale_after_round(Wst, Npad, rows, n_scale, scale):
    """WRONG: the scaling done on the rounded f16 word as an exponent shift with no second rounding - bits shifted out below the f16 subnormal spacing
    (2^-24) are dropped, where the packer rounds to nearest even.  (scale = 2^-s.)"""
    assert _pow2(scale) and scale <= 1
    N, K = Wst.shape
    out = np.zeros((Npad, K), f16)
    out[:N] = Wst
    v = Wst[:n_scale].astype(F) * float(scale)
    out[:n_scale] = (np.trunc(v * 2.0 ** 24) * 2.0 ** -24).astype(f16)      # a multiple of 2^-24 below 2^-14, or v itself: the cast is exact
    return _image(out, rows)


# ---- the 8-bit image ---------------------------------------------------------------------------------------------------------------------------------------
def quantise(Wst, Npad, n_scale, qscale, scale=None, absmax_div=127.0, rnd=np.rint):
    """CTranslate2's per-row scheme in fp32 -> (q int16 [Npad][K], scale f32 [Npad]); padding rows: q = 0 (byte 128), scale 0.  `scale`: quantise on these
    row scales (the device's) instead of deriving them."""
    N, K = Wst.shape
    w = Wst.astype(f32)
    f = row_factor(N, n_scale, qscale)
    if scale is None:
        mx = np.abs(w).max(axis=1)
        with np.errstate(divide="ignore", invalid="ignore"):
            sc = (np.where(mx > 0, mx / f32(absmax_div), f32(1.0)).astype(f32) * f).astype(f32)
    else:
        sc = np.asarray(scale, f32)[:N]
    inv = (f32(1.0) / (sc / f).astype(f32)).astype(f32)
    q = np.clip(rnd((w * inv[:, None]).astype(f32)), -127, 127).astype(np.int16)
    qp = np.zeros((Npad, K), np.int16); qp[:N] = q
    sp = np.zeros(Npad, f32); sp[:N] = sc
    return qp, sp


def quant_trunc(Wst, Npad, n_scale, qscale):
    """WRONG: truncation instead of round-half-even"""
    return quantise(Wst, Npad, n_scale, qscale, rnd=np.trunc)


def quant_128(Wst, Npad, n_scale, qscale):
    """WRONG: absmax / 128"""
    return quantise(Wst, Npad, n_scale, qscale, absmax_div=128.0)


def pack8(q):
    """offset-binary bytes in the sixteen-row fragment order"""
    return _image((q + 128).astype(np.uint8), 16)


def csum8(Wst, q, scale, n_scale, qscale):
    """c = scale[n] * sum_k q: an integer sum below 2^24 is exact in fp32 in any order, so the word is f32(scale * f32(sum q)), bit for bit"""
    N = Wst.shape[0]
    s = q[:N].astype(np.int64).sum(axis=1)
    assert np.abs(s).max(initial=0) < 2 ** 24
    return (s.astype(f32) * scale[:N]).astype(f32)


def csum8_from_f16(Wst, q, scale, n_scale, qscale):
    """WRONG: the 8-bit projection's column sums taken from the f16 values it was quantised from"""
    N = Wst.shape[0]
    return (Wst.astype(f32).sum(axis=1, dtype=F) * row_factor(N, n_scale, qscale)).astype(f32)


# ---- the cross-Q fold --------------------------------------------------------------------------------------------------------------------------------------
def cq_fold(Wq, gamma, beta, bq, Wo, bo):
    """-> dict: wq = W'q f16 [d][d] (exact), P / P_bound (the product half, float64 on the f16 operands), qcs / qb with bounds (fold_sums at n_scale = d,
    qscale = 1/8, the bias scaled first as the loader does).  b_cqo is taken from the device's fcat: b_cqo_ref()."""
    d = Wq.shape[0]
    qs = f32(0.125)
    wq = (fold(Wq, gamma).astype(f32) * qs).astype(f16)
    wo = np.asarray(Wo).astype(f16)      # (transposed on the device: the GEMM's operand layout, the same values)
    P = wq.astype(F) @ wo.astype(F)
    Pb = U16 * np.abs(P) + d * U32 * (np.abs(wq).astype(F) @ np.abs(wo).astype(F))
    c, cb, b, bb = fold_sums(Wq, gamma, beta, (np.asarray(bq, f32) * qs).astype(f32), d, 0.125)
    return dict(wq=wq, P=P, P_bound=Pb, qcs=c, qcs_bound=cb, qb=b, qb_bound=bb)


def b_cqo_ref(fcat, bo):
    """b_cqo = fcat[:, :d] bo: fp32 products f32(w) * bo summed by one wave per row"""
    d = fcat.shape[0]
    return _sum_ref(fcat[:, :d].astype(f32) * np.asarray(bo, f32)[None, :], d, np.ones(d, f32))


# ---- input families (seeded; W f16 [N][K], gamma / beta f32 [K], bias f32 [N]) ------------------------------------------------------------------------------
FAMILIES = ("gauss", "outlier", "zero_rows", "gamma_neg_zero", "subnormal", "beta10", "ties", "clamp")
ROW_FAMILIES = ("gauss", "outlier", "zero_rows", "subnormal", "ties", "clamp")      # what `mixed` interleaves row by row
SIGMA = 0.05
TIE_EXP = 12      # the tie rows hold m 2^-12, |m| <= 254, with 254 present: absmax = 127 2^-11, scale = 2^-11 exactly, w / scale = m / 2


def _rows(fam, n, K, rng):
    """n rows of what the quantiser / packer is to see (for `ties` and `clamp` AFTER the fold: W = T / gamma with gamma a signed power of two)"""
    g = (rng.standard_normal((n, K)) * SIGMA).astype(f16)
    if fam == "outlier":      # one element of 30 sigma per row: the other 8-bit values are almost all 0 or +-1
        g[np.arange(n), rng.integers(0, K, n)] = (30 * SIGMA * rng.choice([-1.0, 1.0], n)).astype(f16)
    elif fam == "zero_rows":
        g[[0, n // 2, n - 1]] = 0
    elif fam == "subnormal":      # +- 2^u, u uniform in [-17, -13]: every product with 1/8 is an f16 subnormal, and W * gamma often is
        g = (rng.choice([-1.0, 1.0], (n, K)) * 2.0 ** rng.uniform(-17, -13, (n, K))).astype(f16)
    elif fam == "ties":          # half of the m odd: w / scale lands on exact .5 ties; rint goes to the even neighbour, away-from-zero and truncation do not
        m = rng.integers(-253, 254, (n, K))
        m[np.arange(n), rng.integers(0, K, n)] = 254 * rng.choice([-1, 1], n)
        g = (m * 2.0 ** -TIE_EXP).astype(f16)
        assert np.array_equal(g.astype(F) * 2.0 ** TIE_EXP, m)
    elif fam == "clamp":         # +absmax and -absmax in one row
        a = np.abs(g).max(axis=1)
        i = rng.integers(0, K // 2, n)
        g[np.arange(n), i] = a; g[np.arange(n), i + K // 2] = -a
    return g


def make_case(fam, N, K, with_gamma, seed=0):
    """-> (W f16 [N][K], gamma, beta f32 [K] (None without gamma), bias f32 [N]).  fam in FAMILIES, or "mixed": row n of ROW_FAMILIES[n % 6] (and rows 0, N / 2,
    N - 1 zero) under a gamma with negative entries and a stretch of zeros and a beta of magnitude 10."""
    rng = np.random.default_rng([FAMILIES.index(fam) if fam in FAMILIES else 99, N, K, int(with_gamma), seed])
    if fam == "mixed":
        W = np.zeros((N, K), f16)
        nf = len(ROW_FAMILIES)
        for i, rf in enumerate(ROW_FAMILIES):
            n = len(range(i, N, nf))
            if n:
                W[i::nf] = 0 if rf == "zero_rows" else _rows(rf, max(n, 3), K, rng)[:n]
        W[[0, N // 2, N - 1]] = 0
    else:
        W = _rows(fam if fam in ROW_FAMILIES else "gauss", N, K, rng)
    bias = rng.standard_normal(N).astype(f32)
    if not with_gamma:
        return W, None, None, bias
    gamma = (1 + 0.1 * rng.standard_normal(K)).astype(f32)
    beta = (0.1 * rng.standard_normal(K)).astype(f32)
    if fam in ("gamma_neg_zero", "mixed"):
        gamma = rng.standard_normal(K).astype(f32)
        gamma[0] = -abs(gamma[0])
        gamma[K // 4:K // 4 + max(1, K // 8)] = 0
    if fam in ("beta10", "mixed"):
        beta = (10 * rng.choice([-1.0, 1.0], K) * rng.uniform(0.5, 1.5, K)).astype(f32)
    if fam in ("ties", "clamp"):      # the fold is exact and undoes the division: the quantiser sees the rows as built
        gamma = (rng.choice([-1.0, 1.0], K) * rng.choice([0.5, 1.0, 2.0], K)).astype(f32)
        W = (W.astype(f32) / gamma).astype(f16)
        assert np.array_equal(fold(W, gamma).astype(f32) / gamma, W.astype(f32))
    return W, gamma, beta, bias
