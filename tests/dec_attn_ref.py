"""Inputs, float64 reference, error bound and numpy models for the decoder's attention kernels (csrc/dec_kernels.hip: dec_self_attn_kernel<TREE, NB>,
dec_self_attn_long_kernel, dec_cross_attn_kernel<TPW, CM, FOLD, SPIN>, dec_cross_attn_rs_kernel<SPIN, NT, 2>), shared by tests/test_gpu_dec_attn_edges.py
and tests/test_dec_attn_model_cpu.py.  The encoder's twin is tests/enc_attn_ref.py; structure and acceptance rule are the same.

Scores.  The kernels take the query with 1 / 8 already folded in and no other scale: s_k = q . k_k, natural-log domain.  Dims 0 and 1 of q and k carry the
structure (q_0 = 4, k_0 = level / 4 with level / 4 exact in f16, k_1 = 0), the other dims carry small noise (none in the keys of `one`, whose scores must
be exact, and q = 0 altogether in `flat`).  Self-attention reads q as fp32: its noise dims hold fp32 values that f16 cannot represent, so a kernel that
rounded q would be off by ~2^-12 per term.  Cross-attention rounds the finished query to f16 itself: its q values ARE f16 values (noise on the grid
j / 64, 1 <= |j| <= 16, so that one f16 ulp is at least 2^-16), and the fold forms are given operands whose finished query lies within 1 / 16 ulp of them
(fold_operands / fold_query_check), so the rounding is the same whatever fp32 order a kernel uses.
A "block" is what one pass of a loop covers (8 NB positions of dec_self_attn_kernel, 32 of the long kernel), a "chunk" the 128 or 256 keys of one
cross-attention workgroup; `levels` places every pattern relative to that size.

Bound.  With normalised weights p_k, every written element must obey
    |out - ref| <= factor * unit + 2^-10 |ref|,        factor 2 on the GPU, 1 for the numpy models below
    unit_d = sum_k (p_k eps_k + z_k) |v_kd - ref_d|  +  (a + sum_k z_k) (sum_k p_k |v_kd| + |ref_d|)  +  (2^-25 where |ref_d| < 2^-14)
2^-10 |ref| is the project's r for an f16 output (cross-attention spends it: 2^-11 for the output's rounding, 2^-11 for P being rounded where the row sum
is not - see below); factor 2 covers second-order terms and the last bit of v_exp_f32, as in enc_attn_ref.py.

  eps_k, the relative error of weight k (errors common to all weights of a row cancel in the normalisation):
    self-attention (P stays fp32):    eps_k = 2^-24 (67 sum_j |q_j| |k_kj| + 4 (|s_k| + max_k |s_k|) + 4)
      67 sum |q||k|: the fp32 dot product, 64 fma terms in 8 lane chains plus the three DPP adds, worst case;
      4 (|s_k| + max |s|): the subtraction s_k - m_run rounds (2^-24 |s_k - m_run|), __expf scales its argument by log2(e) in fp32 (a relative error of
        2^-24 on the argument: 2^-24 |s_k - m_run| on the weight), and the same two for the chain of rescales alpha = __expf(m_old - m_new), whose
        arguments telescope to m_final - m_run <= max |s| + |s_k|;
      4: v_exp_f32's last bit for the weight and the rescales that still matter.
    cross-attention:                  eps_k = 2^-11 + 2^-24 (65 sum_j |q_j| |k_kj| + 4 (|s_k| + max_k |s_k|) + 4)
      2^-11: P rounded to f16 (the row sum adds the UNROUNDED exponentials: the part of that error that is common to O and l does not exist, hence
        the second 2^-11 |ref| inside r); the fp32 MFMA chain (64 terms + the C operand); the exponential about the chunk maximum and the combine
        weight exp(m_c - M) as above.
      z_k = 2^-25 exp(m_c(k) - M) / L where that exceeds 2^-11 p_k: P is an f16 number about the CHUNK maximum, so a weight below 2^-14 of it is a denormal
        with an absolute error of 2^-25 (and below 2^-25 an exact zero).  This term is not in enc_attn_ref.py; it was added here by derivation before
        any kernel ran (a chunk of 256 keys 15 below its maximum moves an element by 256 x 2^-25, more than `unit` of a row whose mass sits on one
        key).  It multiplies |v - ref| + (sum p |v| + |ref|) because it is an absolute error of O alone.
  a, the fp32 accumulation of O and l (absolute errors of the two sums, which do not share roundings, so they scale with sum p |v| and |ref|, not with
  |v - ref|):  a = 2^-24 n_acc, n_acc = the roundings on the longest path:
      dec_self_attn_kernel<., NB>:  passes (NB + 9) + 8    (per pass NB fma / adds, the alpha multiply, the wave sum's 6 levels; the slot reduce, 1 / l)
      dec_self_attn_long_kernel:    40 + 10 suffix passes  (8 prefix blocks, the wave tree, the four-wave merge; per suffix pass as above)
      cross-attention:              CL + 2 chunks + 16     (the P.V MFMA chain over the chunk's keys, the row sum, the combine's fma per chunk)
  2^-25 where |ref_d| < 2^-14: the f16 OUTPUT is a denormal there, and its rounding is an absolute 2^-25 that r = 2^-10 |ref| does not cover below
  |ref| = 2^-15.  This term was missing from the first derivation and was found by the first MI355X run: dec_self_attn_kernel<true, 8>, `tail`, aw 32,
  w0 70, with a base table, H 3, row 5, head 2, element 9 stood at 1.43 with ref = 2.03e-5, out = 2.0266e-5 - and self_model, on the CPU, gives the same
  output and the same 1.43: the distance is the f16 denormal grid, 2^-24 (test_dec_attn_model_cpu.py has the models write such outputs on purpose).
  Weights below 2^-126 of the row maximum are flushed to 0 by v_exp_f32: an absolute error of 1e-38, ignored."""
import numpy as np

F16_R = 2.0 ** -10
U24 = 2.0 ** -24
NAN16 = 0x7E00
PAT16 = 0x5A5A      # f16 203.25: nothing these kernels produce from the inputs below

STEPS = (3, 20, 150)
PATTERNS = (["control"] + [f"up{s}" for s in STEPS] + [f"down{s}" for s in STEPS] + ["tail", "head", "edge_last", "edge_first", "flat"]
            + [f"far{g}_{w}" for g in (150, 600) for w in ("first", "last")] + ["one"])
# cross-attention adds the places inside a chunk where the rs kernel's K waves (keys 127 | 128) and 16-key MFMA tiles (15 | 16) meet
CROSS_PATTERNS = PATTERNS + ["edge_k127", "edge_k128", "edge_k15", "edge_k16"]
PEAK = 12.0         # the level of a single marked position: the rest of its chunk becomes f16 denormals (e^-12 = 2^-17.3) in cross-attention's P
PLENS = [1, 7, 8, 31, 32, 33, 255, 256]      # dec_self_attn_long_kernel: prompt lengths, and the generated lengths mixed within an utterance
SUFFIXES = [1, 2, 32, 33, 65]


def self_lens(nb, ctx):
    """history lengths on both sides of every pass boundary of dec_self_attn_kernel<., nb>, the shortest and the longest the cache holds"""
    return sorted({n for n in (1, 8 * nb - 1, 8 * nb, 8 * nb + 1, 16 * nb, 16 * nb + 1, ctx) if n <= ctx})


def cdiv(a, b):
    return -(-a // b)


def levels(pattern, n, blk):
    """natural-log level of positions 0 .. n - 1 for blocks / chunks of `blk` positions; None: no structure (control)

    control      random scores: the ordinary path
    up<s>        every block beats the previous one by s: every pass rescales; at s = 150 every earlier partial underflows to an exact 0
    down<s>      the reverse: later weights run through denormals to exact zeros, a later chunk's exp(m_c - M) is 0
    tail         the largest score at the last valid position n - 1: clamped copies / masked lanes behind it must contribute nothing
    head         the largest score at position 0
    edge_last    the largest score at the last position of block 0 (the position before the first pass / chunk boundary)
    edge_first   the largest score at the first position of block 1
    edge_k<j>    (cross) the largest score at key j of chunk 1 (chunk 0 if there is one chunk): 127 | 128 is where the rs kernel's two K waves exchange
                 their maxima, 15 | 16 a 16-key MFMA tile boundary
    flat         all scores equal (q = 0): the plain mean of V, the largest summation error
    far<g>_first the first block g above all others (g = 150, 600): every later partial's weight in the combine / merge is an exact 0
    far<g>_last  the last block g above all others: every earlier partial is rescaled to an exact 0
    one          one position 600 above all others (self-attention also runs it on a history of one position): out = that v, exactly"""
    if pattern == "control":
        return None
    p = np.arange(n)
    b = p // blk
    lv = np.zeros(n)
    if pattern.startswith("up"):
        lv = float(pattern[2:]) * b
    elif pattern.startswith("down"):
        lv = -float(pattern[4:]) * b
    elif pattern == "tail":
        lv[n - 1] = PEAK
    elif pattern == "head":
        lv[0] = PEAK
    elif pattern == "edge_last":
        lv[min(blk - 1, n - 1)] = PEAK
    elif pattern == "edge_first":
        lv[min(blk, n - 1)] = PEAK
    elif pattern.startswith("edge_k"):
        lv[min((blk if n > blk else 0) + int(pattern[6:]), n - 1)] = PEAK
    elif pattern == "flat":
        pass
    elif pattern.startswith("far"):
        g, where = pattern[3:].split("_")
        lv = np.where(b == (0 if where == "first" else b[-1]), float(g), 0.0)
    elif pattern == "one":
        lv[n // 2] = 600.0
    else:
        raise ValueError(pattern)
    return np.asarray(lv, np.float64)


def make_qkv(pattern, lv, R, rng, q_f16):
    """one attention problem over n = len(lv) positions: q [R][64] float32 (f16 values if q_f16), k, v f16 [n][64]; lv = levels(...) or any other level
    array (the callers that place a pattern across slots or a prefix | suffix boundary build their own)"""
    n = len(lv) if lv is not None else None
    if pattern == "control":
        raise ValueError("control takes make_control")
    k = rng.standard_normal((n, 64)).astype(np.float16)
    v = rng.standard_normal((n, 64)).astype(np.float16)
    if q_f16:
        j = rng.integers(1, 17, size=(R, 64)) * rng.choice([-1, 1], size=(R, 64))
        q = (j / 64.0).astype(np.float32)
    else:
        q = (rng.standard_normal((R, 64)) * 0.1).astype(np.float32)
        assert (q[:, 2:].astype(np.float16).astype(np.float32) != q[:, 2:]).mean() > 0.9      # not f16 values
    q[:, 0] = 4.0
    k0 = (np.asarray(lv) / 4.0).astype(np.float16)
    assert np.array_equal(k0.astype(np.float64) * 4.0, np.asarray(lv)), "a level that is not exact in f16"
    k[:, 0], k[:, 1] = k0, 0.0
    if pattern == "flat":
        q[:] = 0.0
    if pattern == "one":
        k[:, 2:] = 0.0
    return q, k, v


def make_control(n, R, rng, q_f16):
    k = (rng.standard_normal((n, 64)) * 0.6).astype(np.float16)
    v = rng.standard_normal((n, 64)).astype(np.float16)
    if q_f16:
        q = np.clip(np.rint(rng.standard_normal((R, 64)) * 0.45 * 64), -128, 128)
        q = np.where(q == 0, 1.0, q) / 64.0
    else:
        q = rng.standard_normal((R, 64)) * 0.4
    return q.astype(np.float32), k, v


def problem(pattern, n, blk, R, rng, q_f16):
    if pattern == "control":
        return make_control(n, R, rng, q_f16)
    return make_qkv(pattern, levels(pattern, n, blk), R, rng, q_f16)


def long_levels(pattern, plen, n):
    """levels of a row of dec_self_attn_long_kernel: the shared prefix [0, plen), then the row's own positions [plen, n).  Blocks of 32 are counted
    in the two parts separately (prefix block rows, suffix chunks), and the single marks move to where that kernel's paths meet:
    head = position 0 (the shared prefix), edge_last | edge_first = plen - 1 | plen (the prefix | suffix boundary), one = the middle of the row's own
    suffix, tail = its last position; far_first = the first prefix block, far_last = the row's last suffix chunk.  The prefix part depends on
    (pattern, plen) alone, so the rows of an utterance share it."""
    if pattern == "control":
        return None
    p = np.arange(n)
    b = np.where(p < plen, p // 32, cdiv(plen, 32) + (p - plen) // 32)
    lv = np.zeros(n)
    if pattern.startswith("up"):
        lv = float(pattern[2:]) * b
    elif pattern.startswith("down"):
        lv = -float(pattern[4:]) * b
    elif pattern == "tail":
        lv[n - 1] = PEAK
    elif pattern == "head":
        lv[0] = PEAK
    elif pattern == "edge_last":
        lv[plen - 1] = PEAK
    elif pattern == "edge_first":
        lv[plen] = PEAK
    elif pattern == "flat":
        pass
    elif pattern.startswith("far"):
        g, where = pattern[3:].split("_")
        lv = np.where(b == (0 if where == "first" else b[-1]), float(g), 0.0)
    elif pattern == "one":
        lv[plen + (n - plen) // 2] = 600.0
    else:
        raise ValueError(pattern)
    return np.asarray(lv, np.float64)


def long_problem(pattern, plen, sufs, rng):
    """one utterance of the long kernel: rows j with sufs[j] generated positions behind a shared prefix of plen.
    -> q f32 [k][64], kp, vp f16 [plen][64], [(ko, vo) f16 [sufs[j]][64]]: row j reads kp ++ ko_j"""
    k = len(sufs)
    if pattern == "control":
        q, kp, vp = make_control(plen, k, rng, False)
        own = [make_control(s, 1, rng, False)[1:] for s in sufs]
        return q, kp, vp, own
    q = None
    own = []
    for j, s in enumerate(sufs):
        qj, kk, vv = make_qkv(pattern, long_levels(pattern, plen, plen + s), k, rng, False)
        if j == 0:
            q, kp, vp = qj, kk[:plen], vv[:plen]
        else:
            assert np.array_equal(kk[:plen, :2], kp[:, :2])
        own.append((kk[plen:], vv[plen:]))
    return q, kp, vp, own


# ---------------------------------------------------------------------------------------
def n_acc_self(n, nb):
    return cdiv(n, 8 * nb) * (nb + 9) + 8


def n_acc_long(n, plen):
    return 40 + 10 * cdiv(max(n - plen, 1), 32)


def n_acc_cross(T, CL):
    return CL + 2 * cdiv(T, CL) + 16


def reference(q, k, v, n_acc, chunk=None):
    """float64 softmax attention of R query rows over the n positions they may read, from exactly the values the kernel reads:
    q [R][64], k, v [n][64] -> ref [R][64], unit [R][64].  chunk = None: the self-attention bound; chunk = CL: cross-attention's"""
    q, k, v = (np.asarray(a, np.float64) for a in (q, k, v))
    s = q @ k.T
    sabs = np.abs(q) @ np.abs(k).T
    smax = np.abs(s).max(1, keepdims=True)
    M = s.max(1, keepdims=True)
    e = np.exp(s - M)
    L = e.sum(1, keepdims=True)
    p = e / L
    ref = p @ v
    if chunk is None:
        pe = p * (U24 * (67 * sabs + 4 * (np.abs(s) + smax) + 4))
        z = np.zeros_like(p)
    else:
        pe = p * (2.0 ** -11 + U24 * (65 * sabs + 4 * (np.abs(s) + smax) + 4))
        n = s.shape[1]
        pad = cdiv(n, chunk) * chunk - n
        mc = np.pad(s, ((0, 0), (0, pad)), constant_values=-np.inf).reshape(s.shape[0], -1, chunk).max(2)
        zc = 2.0 ** -25 * np.exp(mc - M) / L
        z = np.repeat(zc, chunk, axis=1)[:, :n]
        z = np.where(z > 2.0 ** -11 * p, z, 0.0)
    dv = np.abs(v[None, :, :] - ref[:, None, :])                       # [R][n][64]
    zs = z.sum(1, keepdims=True)
    unit = np.einsum("rk,rkd->rd", pe + z, dv) + (U24 * n_acc + zs) * (p @ np.abs(v) + np.abs(ref))
    unit = unit + np.where(np.abs(ref) < 2.0 ** -14, 2.0 ** -25, 0.0)      # an f16 denormal output
    return ref, unit


def ratios(out, ref, unit):
    """(|out - ref| - r) / unit per element, 0 where the error is inside r (inf where it is not and unit is 0)"""
    excess = np.maximum(np.abs(np.asarray(out, np.float64) - ref) - F16_R * np.abs(ref), 0.0)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(excess > 0, excess / unit, 0.0)


# ---------------------------------------------------------------------------------------
# layouts (include/wis_hip.h)
def xf_index(m, k, MB):
    """kernels.hpp xf_index: element (row m, column k) of an activation fragment image of MB 16-row blocks"""
    m, k = np.asarray(m, np.int64), np.asarray(k, np.int64)
    return (((k >> 5) * MB + (m >> 4)) * 64 + (m & 15) + 16 * ((k >> 3) & 3)) * 8 + (k & 7)


def xf_elems(d, MB):
    return (d // 32) * MB * 64 * 8


def k_image(K):
    """natural K f16 [B][T][d] -> [B][H][8][T][8]"""
    B, T, d = K.shape
    return np.ascontiguousarray(K.reshape(B, T, d // 64, 8, 8).transpose(0, 2, 3, 1, 4))


def vt_image(V, Tpad, fill=0):
    """natural V f16 [B][T][d] -> V^T [B][H][64][Tpad]; positions [T, Tpad) hold the 16-bit pattern `fill`"""
    B, T, d = V.shape
    vt = np.full((B, d // 64, 64, Tpad), fill, np.uint16).view(np.float16)
    vt[:, :, :, :T] = V.reshape(B, T, d // 64, 64).transpose(0, 2, 3, 1)
    return vt


def partials(x):
    """per-16-column (sum x, sum (x - tile mean)^2) of fp32 rows, in float64: [M][d/16][2]"""
    t = np.asarray(x, np.float64).reshape(x.shape[0], -1, 16)
    s = t.sum(-1)
    return np.stack([s, ((t - s[..., None] / 16) ** 2).sum(-1)], -1)


def merge_partials(stat, dtype=np.float64):
    """mean / rstd of the rows from fp32 partials: in float64, or in float32 about the first tile's mean as the kernels merge them"""
    s, m2 = stat[..., 0].astype(dtype), stat[..., 1].astype(dtype)
    d = dtype(16 * s.shape[1])
    c0 = s[:, :1] * dtype(0.0625) if dtype is np.float32 else np.zeros((s.shape[0], 1))
    dm = s * dtype(0.0625) - c0
    dmu = dm.sum(1, keepdims=True, dtype=dtype) * dtype(16) / d
    var = (m2 + dtype(16) * dm * dm).sum(1, keepdims=True, dtype=dtype) / d - dmu * dmu
    return (c0 + dmu).astype(dtype), (dtype(1) / np.sqrt(np.maximum(var, 0) + dtype(1e-5))).astype(dtype)


def fold_operands(q16, rng, zero_cols=None):
    """operands of the fold forms whose finished query rs (q_raw [+ q2] - mu qcs) + qb is q16 (float32 [M][d] holding f16 values), built as
    _cross_stat_case (tests/test_gpu_dec_step_ops.py) builds them.  zero_cols: columns whose query is exactly 0 (`flat`): qcs = qb = q_raw = 0 there.
    -> dict(x, stat, qcs, qb, q_one, q_a, q_b)"""
    M, d = q16.shape
    x = (rng.standard_normal((M, d)) * 2.4 + 0.7).astype(np.float32)
    stat = partials(x).astype(np.float32)
    mu, rs = merge_partials(stat)
    qcs = rng.standard_normal(d).astype(np.float32)
    qb = (0.1 * rng.standard_normal(d)).astype(np.float32)
    if zero_cols is not None:
        qcs[zero_cols], qb[zero_cols] = 0.0, 0.0
    q_raw = (q16.astype(np.float64) - qb) / rs + mu * qcs
    q_one = q_raw.astype(np.float32)
    q_a = (0.5 * q_raw + q_raw.std() * rng.standard_normal((M, d))).astype(np.float32)
    if zero_cols is not None:
        q_a[:, zero_cols] = 0.0
    q_b = (q_raw - q_a.astype(np.float64)).astype(np.float32)
    return dict(x=x, stat=stat, qcs=qcs, qb=qb, q_one=q_one, q_a=q_a, q_b=q_b)


def fold_query_check(q16, ops, from_rows=False):
    """the finished query of both operand forms, evaluated in float64 and in float32 (statistics merged in float32 too), lies within 1 / 16 f16 ulp of
    q16 in every element: whatever fp32 order a kernel uses, its f16 rounding gives q16.  from_rows: FOLD 1, statistics from the rows x themselves.
    -> the worst distance in ulps"""
    want = q16.astype(np.float64)
    mag = np.abs(want)
    with np.errstate(divide="ignore"):
        ulp = np.where(mag < 2.0 ** -14, 2.0 ** -24, 2.0 ** (np.floor(np.log2(np.maximum(mag, 2.0 ** -14))) - 10))
    ulp = np.where(mag == 0, 0.0, ulp)      # an exact zero has to come out as an exact zero
    worst = 0.0
    for dtype in (np.float64, np.float32):
        if from_rows:
            x = ops["x"].astype(dtype)
            c0 = x[:, :1]
            ms = (x - c0).sum(1, keepdims=True, dtype=dtype) / dtype(x.shape[1])
            var = ((x - c0) ** 2).sum(1, keepdims=True, dtype=dtype) / dtype(x.shape[1]) - ms * ms
            mu, rs = c0 + ms, dtype(1) / np.sqrt(np.maximum(var, 0) + dtype(1e-5))
        else:
            mu, rs = merge_partials(ops["stat"], dtype)
        for qa, q2 in ((ops["q_one"], None), (ops["q_a"], ops["q_b"])):
            qs = qa.astype(dtype) + (q2.astype(dtype) if q2 is not None else dtype(0))
            fin = rs * (qs - mu * ops["qcs"].astype(dtype)) + ops["qb"].astype(dtype)
            assert fin.dtype == dtype
            dist = np.abs(fin.astype(np.float64) - want)
            assert (dist <= ulp / 16).all(), (dtype, float((dist / np.maximum(ulp, 1e-300)).max()))
            with np.errstate(divide="ignore", invalid="ignore"):
                worst = max(worst, float(np.where(ulp > 0, dist / ulp, 0.0).max()))
    return worst


# ---------------------------------------------------------------------------------------
# numpy fp32 models: the kernels' masking rule, clamping rule and order where it matters
f32 = np.float32
LOG2E = f32(1.4426950408889634)


def expf(x):
    """__expf: v_exp_f32 of the argument scaled by log2(e) in fp32; results below 2^-126 are flushed to 0"""
    x = np.asarray(x, f32)
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        y = np.exp2((x * LOG2E).astype(np.float64)).astype(f32)
    return np.where(y < f32(2.0 ** -126), f32(0), y)


def _fma(a, b, c):
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(f32)


def _dots(q, k):
    """the lanes' dot products: q f32 [64], k f16 [P][64] -> f32 [P]; 8 chains of 8 fma, then the three DPP adds (a tree over the 8 chunk lanes)"""
    kk = k.astype(f32).reshape(-1, 8, 8)
    qq = np.asarray(q, f32).reshape(8, 8)
    dot = np.zeros(kk.shape[:2], f32)
    for j in range(8):
        dot = _fma(kk[:, :, j], qq[None, :, j], dot)
    dot = dot[:, 0::2] + dot[:, 1::2]
    dot = dot[:, 0::2] + dot[:, 1::2]
    return (dot[:, 0] + dot[:, 1]).astype(f32)


def _tree8(a):
    """sum over a leading axis of 8 as a balanced tree"""
    a = a[0::2] + a[1::2]
    a = a[0::2] + a[1::2]
    return (a[0] + a[1]).astype(f32)


def _slot_reduce(acc):
    """acc [8 position slots][64] -> [64]: slot pairs by DPP, the four 16-lane rows through LDS"""
    r = (acc[0::2] + acc[1::2]).astype(f32)
    return ((r[0] + r[1]).astype(f32) + (r[2] + r[3]).astype(f32)).astype(f32)


def self_model(q, kh, vh, n, nb):
    """dec_self_attn_kernel<., nb> for one (row, head): q f32 [64]; kh, vh f16 [>= max(n, 8 nb)][64] = the row's history as the kernel addresses it
    (position p -> row p; rows >= n are what the first pass loads and masks).  -> out f16 [64], log"""
    m_run, l_run = f32(-np.inf), f32(0)
    acc = np.zeros((8, 64), f32)
    log = dict(passes=0, rescales=0, zero_weights=0, clamped=0, alphas=[])
    p0 = 0
    while True:
        pos = p0 + np.arange(8 * nb)                        # block i, slot pl: p0 + 8 i + pl
        ok = pos < n
        pc = pos if p0 == 0 else np.where(ok, pos, n - 1)      # later passes: clamped copies of the last position
        log["clamped"] += int((~ok).sum()) if p0 else 0
        sc = np.where(ok, _dots(q, kh[pc]), f32(-np.inf)).astype(f32)
        m_new = np.maximum(m_run, sc.max())
        with np.errstate(invalid="ignore"):
            alpha = expf(m_run - m_new)
        pw = expf(sc - m_new)
        log["zero_weights"] += int((pw[ok] == 0).sum())
        log["rescales"] += int(p0 > 0 and m_new > m_run)
        log["alphas"].append(float(alpha))
        acc = (acc * alpha).astype(f32)
        lsum = np.zeros(8, f32)
        for i in range(nb):
            sl = slice(8 * i, 8 * i + 8)
            lsum = (lsum + pw[sl]).astype(f32)
            upd = _fma(pw[sl, None], vh[pc[sl]].astype(f32), acc)
            acc = np.where(ok[sl, None], upd, acc)
        l_run = f32(l_run * alpha + _tree8(lsum))
        m_run = m_new
        log["passes"] += 1
        p0 += 8 * nb
        if p0 >= n:
            break
    o = _slot_reduce(acc)
    return (o / l_run).astype(f32).astype(np.float16), log


def long_model(q, kp, vp, ko, vo, plen, last, maxlast):
    """dec_self_attn_long_kernel for one (row, head): q f32 [64]; kp, vp f16 [ctx][64] the utterance's first slot (the prefix), ko, vo the row's own
    slot; the row reads prefix positions < plen and own positions plen .. last; maxlast = the largest `last` of the utterance's rows (the suffix loop
    runs that long for every row).  -> out f16 [64], log"""
    ctx = kp.shape[0]
    m_w, l_w, o_w = np.zeros(4, f32), np.zeros(4, f32), np.zeros((4, 64), f32)
    log = dict(empty_waves=0, zero_merge=0, suffix_passes=0, zero_weights=0, clamped=0)
    for w in range(4):
        pos = (32 * np.arange(8)[:, None] + 8 * w + np.arange(8)[None, :]).reshape(-1)      # block i, slot pl
        ok = (pos < plen) & (pos <= last)
        pc = np.minimum(pos, ctx - 1)
        sc = np.where(ok, _dots(q, kp[pc]), f32(-np.inf)).astype(f32)
        mx = sc.max()
        ms = f32(0) if mx == -np.inf else mx
        pw = expf(sc - ms)
        log["zero_weights"] += int((pw[ok] == 0).sum())
        acc = np.zeros((8, 64), f32)
        lsum = np.zeros(8, f32)
        for i in range(8):
            sl = slice(8 * i, 8 * i + 8)
            lsum = (lsum + pw[sl]).astype(f32)
            acc = np.where(ok[sl, None], _fma(pw[sl, None], vp[pc[sl]].astype(f32), acc), acc)
        m_run, l_run = mx, _tree8(lsum)
        p0 = plen
        while True:
            pos = p0 + 8 * w + np.arange(8)
            ok = pos <= last
            pc = np.where(pos < last, np.maximum(pos, 0), last)
            log["clamped"] += int((~ok).sum())
            sc = np.where(ok, _dots(q, ko[pc]), f32(-np.inf)).astype(f32)
            m_new = np.maximum(m_run, sc.max())
            ms = f32(0) if m_new == -np.inf else m_new
            with np.errstate(invalid="ignore"):
                alpha, pw = expf(m_run - ms), expf(sc - ms)
            log["zero_weights"] += int((pw[ok] == 0).sum())
            acc = (acc * alpha).astype(f32)
            acc = np.where(ok[:, None], _fma(pw[:, None], vo[pc].astype(f32), acc), acc)
            l_run = f32(l_run * alpha + _tree8(pw))
            m_run = m_new
            p0 += 32
            if w == 0:
                log["suffix_passes"] += 1
            if p0 > maxlast:
                break
        m_w[w], l_w[w], o_w[w] = m_run, l_run, _slot_reduce(acc)
        log["empty_waves"] += int(m_run == -np.inf)
    M = m_w.max()
    ww = expf(m_w - M)
    log["zero_merge"] = int(((ww == 0) & (m_w > -np.inf)).sum())
    L = f32(f32(l_w[0] * ww[0] + l_w[1] * ww[1]) + f32(l_w[2] * ww[2] + l_w[3] * ww[3]))
    t = (o_w * ww[:, None]).astype(f32)
    o = ((t[0] + t[1]).astype(f32) + (t[2] + t[3]).astype(f32)).astype(f32)
    return (o / L).astype(f32).astype(np.float16), log


def cross_model(q16, k16, v16, CL):
    """one (utterance, head) of the cross-attention kernels: q16 [R][64] (f16 values), k16, v16 f16 [T][64]; chunks of CL keys, each with exponentials
    about its own maximum, P rounded to f16, the row sum of the unrounded exponentials; the partials combined in chunk order.  -> out f16 [R][64], log"""
    R, T = q16.shape[0], k16.shape[0]
    C = cdiv(T, CL)
    q, k, v = np.asarray(q16, f32), k16.astype(f32), v16.astype(f32)
    mc, lc, oc = np.zeros((C, R), f32), np.zeros((C, R), f32), np.zeros((C, R, 64), f32)
    log = dict(chunks=C, masked=0, zero_p=0, zero_combine=0, denormal_p=0)
    for c in range(C):
        keys = np.arange(c * CL, (c + 1) * CL)
        ok = keys < T
        kc = np.minimum(keys, T - 1)                        # clamped loads, masked by kl < n
        log["masked"] += int((~ok).sum())
        s = (q.astype(np.float64) @ k[kc].astype(np.float64).T).astype(f32)
        s[:, ~ok] = -np.inf
        mc[c] = s.max(1)
        e = expf(s - mc[c][:, None])
        p16 = e.astype(np.float16)
        log["zero_p"] += int((p16[:, ok] == 0).sum())
        log["denormal_p"] += int(((p16[:, ok] != 0) & (p16[:, ok] < np.float16(2.0 ** -14))).sum())
        lc[c] = e.sum(1, dtype=f32)
        oc[c] = (p16.astype(np.float64) @ v[kc].astype(np.float64)).astype(f32)      # (masked keys: P exactly 0)
    M = mc.max(0)
    L, O = np.zeros(R, f32), np.zeros((R, 64), f32)
    for c in range(C):
        w = expf(mc[c] - M)
        log["zero_combine"] += int((w == 0).sum())
        L = _fma(lc[c], w, L)
        O = _fma(oc[c], w[:, None], O)
    inv = (f32(1) / L).astype(f32)
    return (O * inv[:, None]).astype(f32).astype(np.float16), log
