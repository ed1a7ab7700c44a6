"""Reference restatement of word-level alignment for the tests (numpy, float64 unless stated): cross-attention weights of chosen
heads, normalise / median / head-mean / negate, dynamic time warping (openai-whisper dtw_cpu's loop: cost table in f32, trace 0 / 1 / 2,
borders trace[0][:] = 2 and trace[:][0] = 1), and the word grouping of openai-whisper's split_to_word_tokens + merge_punctuations with
the jump times of find_alignment.  Restated from the public openai-whisper / transformers sources; nothing here imports the engine.

The second half of the file serves tests/test_gpu_align_stages.py and its CPU twin tests/test_align_model_cpu.py: float32 models of the
alignment kernels in their stated operation order, the inputs of every case, and PER-ELEMENT bounds on |fp32 result - float64 reference|.
The GPU may reach 2 x bound, the models must stay within 1 x.  U = 2^-24 is fp32's unit roundoff, gamma(n) = n U / (1 - n U) what n
roundings compound to.  Every constant below is a count of roundings or is called a margin, with its reason.

(a) scores + softmax (scores_bound).  Reference: float64 from the f16 values the kernel reads (q rounded to f16 as the kernel's cast rounds
    it, K as stored).  f16 x f16 products are exact in fp32.  A score is 32 two-term dot steps into one accumulator: at most 2 roundings a
    step, 64 accumulations, so |s^ - s| <= e_s = gamma(64) sum_d |q_d k_d| + flush, where flush = sum of |q_d k_d| over the dimensions with
    an f16-denormal operand (margin: the dot instruction may read f16 denormals as zero; exact when it does not).
    p_t = exp(s_t - m) / sum_j exp(s_j - m) does not depend on m, so the computed maximum costs nothing.  Relative error of p_t, first order,
    compounded with expm1: A = 2 max_j e_s (numerator's own score, the p-weighted mean of the others: "twice the largest score error of the
    row") + U (|x_t| + sum_j p_j |x_j|) + 4 U max e_s (one rounding of each subtraction x = s - m, numerator and p-weighted denominator)
    + gamma(ceil(T / 64) + 5) (a lane adds ceil(T / 64) terms: ceil(T / 64) - 1 roundings; the wave tree has 6 levels)
    + 2 E (expf in the numerator, and p-weighted in the denominator) + U (the quotient).
    E is not guessed: expf_allowance() measures numpy's float32 exp against float64 on the case's own arguments and doubles it (margin:
    another libm); measured here 2.5 - 3.4 U, i.e. below 2 ulp.  bound = p expm1(A) + 2^-125 (results below 2^-126 are denormal or
    flushed: 2^-126 for expf's result, 2^-126 for the quotient).
    The token probabilities (probs_bound) are the same without e_s: A = U (|x_t| + sum p |x|) + gamma(ceil(eot / 256) + 8)
    (ceil(eot / 256) - 1 per thread, 6 levels per wave, 3 to combine the four waves) + 2 E + U.
(b) norm (norm_bound, norm_terms).  Reference: float64 from the very fp32 column the kernel read.  n0 = ceil(N / 4) rows per partition.
    mean: n0 - 1 roundings inside a partition + 3 to combine + 1 for / N: |mean^ - mean| <= e_mu = gamma(n0 + 3) mean|w|.
    dlt_r = fl(w_r - mean^) = (d_r - D)(1 + rho), D = mean^ - mean.  Because sum d_r = 0, sum dlt^2 = (N std^2 + N D^2)(1 + 2 rho): the
    mean's error enters the variance only as D^2, i.e. relatively as X = (e_mu / std)^2 - this is where 1 / std appears.  The fp32 sum carries
    that (1 + rho)^2 (2), the square (1), the partition and combine additions (n0 + 2), / N (1), sqrtf (1, halved under the root but counted whole), one for
    squares that leave the normal range (asserted: std >= 2^-50): sd^ = std sqrt(1 + x)(1 + e), 0 <= x <= X, |e| <= eps = gamma(n0 + 8).
    z^_r = fl(dlt_r / sd^): with k = (1 + rho)^2 / (sqrt(1 + x)(1 + e)), |z^_r - z_r| <= (|d_r| |k - 1| + e_mu k) / std, and
    |k - 1| <= kappa = max(1 - (1 - 2U - U^2) / (sqrt(1 + X)(1 + eps)), (1 + U)^2 / (1 - eps) - 1).  No first-order shortcut: a column of
    small std gets its large allowance through X and e_mu / std, a column of ordinary std stays near (n0 + 11) U |z|.
    The kernel's operations are all correctly rounded fp32 ones in a fixed order, so norm_model32 also gives its very bits (asserted on
    the GPU).  Columns with float64 std < 2^-40 |mean| take no part (fp32 may reach std = 0 there); utterances of ONE token, whose every std
    is 0 by construction, are checked exactly (all NaN) and are not counted in the 1 % share the tests assert.
(c) median selection and head sum are exact (median_select32, median_sum_model32): np.sort of the reflect-padded window, element width // 2,
    NaN last; the inputs hold no -0, the one thing whose place among equal values no sort defines.
(d) chain (chain_bound).  p moves by at most bp (a) inside its column: the mean by m_b = mean(bp), a deviation by bp_r + m_b, the std by at
    most s_b = rms(bp + m_b) (triangle inequality of the rms norm; s_b < std / 2 is asserted), so z by (bp_r + m_b) / (std - s_b) +
    |d_r| s_b / (std (std - s_b)); plus (b) evaluated at the inflated |d|, mean|w| and deflated std.  A median moves by at most the largest
    perturbation in its window (the max over the same reflect-padded window); the head mean takes the mean of those and
    gamma(nsel + chunks + 1) mean_h(|median_h| + its bound) for the fp32 head sum (nsel additions, one more per chunk, the division)."""
import string

import numpy as np

TOKENS_PER_SECOND = 50


def attention_weights(q, K):
    """q [H][N][64], K [H][T][64] (queries already scaled) -> softmax over ALL T keys, float64 [H][N][T]."""
    s = np.einsum("hnd,htd->hnt", np.asarray(q, np.float64), np.asarray(K, np.float64))
    s -= s.max(-1, keepdims=True)
    e = np.exp(s)
    return e / e.sum(-1, keepdims=True)


def median_filter(x, width):
    """odd width along the last axis with reflect padding; unchanged when frames <= width // 2 (transformers _median_filter).
    NaN sorts last, as torch.sort places it."""
    pad = width // 2
    if pad == 0 or x.shape[-1] <= pad:
        return x
    xp = np.pad(x, [(0, 0)] * (x.ndim - 1) + [(pad, pad)], mode="reflect")
    win = np.lib.stride_tricks.sliding_window_view(xp, width, axis=-1)
    return np.sort(win, axis=-1)[..., pad]


def matrix(weights, width, dtype=np.float64):
    """weights [H][N][F] (already cropped to the frames) -> -(mean over heads of median((w - mean) / std over tokens)), [N][F]."""
    w = np.asarray(weights, dtype)
    with np.errstate(invalid="ignore", divide="ignore"):
        mean = w.mean(-2, keepdims=True)
        std = np.sqrt(((w - mean) ** 2).mean(-2, keepdims=True))
        w = (w - mean) / std
    return -median_filter(w, width).mean(0)


def dtw(x):
    """x [N][M] -> (text_indices, time_indices): dtw_cpu's recurrence, the cost table in f32, backtrace from (N, M)."""
    x = np.asarray(x, np.float32)
    N, M = x.shape
    cost = np.full((N + 1, M + 1), np.inf, np.float32)
    trace = -np.ones((N + 1, M + 1), np.int8)
    cost[0, 0] = 0
    for j in range(1, M + 1):
        for i in range(1, N + 1):
            c0, c1, c2 = cost[i - 1, j - 1], cost[i - 1, j], cost[i, j - 1]
            if c0 < c1 and c0 < c2:
                c, t = c0, 0
            elif c1 < c0 and c1 < c2:
                c, t = c1, 1
            else:
                c, t = c2, 2
            cost[i, j] = np.float32(x[i - 1, j - 1] + c)
            trace[i, j] = t
    return backtrace(trace)


def dtw_fast(x):
    """the same table by anti-diagonals (vectorised): every cell is one f32 add of values fixed by its predecessors, so the bits equal dtw()'s."""
    x = np.asarray(x, np.float32)
    N, M = x.shape
    cost = np.full((N + 1, M + 1), np.inf, np.float32)
    trace = -np.ones((N + 1, M + 1), np.int8)
    cost[0, 0] = 0
    for d in range(2, N + M + 1):
        i = np.arange(max(1, d - M), min(N, d - 1) + 1)
        j = d - i
        c0, c1, c2 = cost[i - 1, j - 1], cost[i - 1, j], cost[i, j - 1]
        with np.errstate(invalid="ignore"):
            t = np.where((c0 < c1) & (c0 < c2), 0, np.where((c1 < c0) & (c1 < c2), 1, 2))
        c = np.where(t == 0, c0, np.where(t == 1, c1, c2))
        with np.errstate(invalid="ignore"):
            cost[i, j] = (x[i - 1, j - 1] + c).astype(np.float32)
        trace[i, j] = t
    return backtrace(trace)


def backtrace(trace):
    i, j = trace.shape[0] - 1, trace.shape[1] - 1
    trace[0, :] = 2
    trace[:, 0] = 1
    a, b = [], []
    while i > 0 or j > 0:
        a.append(i - 1)
        b.append(j - 1)
        t = trace[i, j]
        if t == 0:
            i -= 1
            j -= 1
        elif t == 1:
            i -= 1
        else:
            j -= 1
    return np.array(a[::-1], np.int64), np.array(b[::-1], np.int64)


def path_cost(x, ti, fi):
    return float(np.asarray(x, np.float64)[ti, fi].sum())


def dtw_optimum(x):
    """the least path cost in float64 (for the validity bound of a path found on a slightly different matrix)."""
    x = np.asarray(x, np.float64)
    N, M = x.shape
    prev = np.full(M + 1, np.inf)
    prev[0] = 0.0
    for i in range(1, N + 1):
        cur = np.full(M + 1, np.inf)
        for j in range(1, M + 1):
            cur[j] = x[i - 1, j - 1] + min(prev[j - 1], prev[j], cur[j - 1])
        prev = cur
    return float(prev[M])


def jump_times(text_indices, time_indices):
    """find_alignment: the frame at every row where text_index advances, in seconds."""
    ti = np.asarray(text_indices)
    jumps = np.pad(np.diff(ti), (1, 0), constant_values=1).astype(bool)
    return np.asarray(time_indices)[jumps] / TOKENS_PER_SECOND


def planted_inputs(rng, N, F, Hn, margin=8.0, T=1500):
    """q, K whose logits put token i on frames [f_i, f_{i+1}): q_i = sqrt(margin) e_i-ish codes, K_t carries the code of its block"""
    while True:
        cuts = np.sort(rng.choice(np.arange(1, F // 10), N - 1, replace=False)) * 10
        f = np.concatenate([[0], cuts, [F]])
        if np.all(np.diff(f) >= 10):
            break
    # 64-dim random sign codes, one per token: <c_i, c_j> = 64 (i = j), about N(0, 64) otherwise; scaled so that on-block - off-block >= margin
    codes = rng.choice([-1.0, 1.0], size=(N, 64))
    gram = codes @ codes.T
    off = np.max(gram - np.diag(np.diag(gram)) - 1e9 * np.eye(N)) if N > 1 else 0.0
    gap = 64.0 - max(off, 0.0)
    assert gap > 0
    sc = np.sqrt((margin + 5.0) / gap)      # + 5: head room for the N(0, 0.5) noise (the gap is asserted below)
    q = np.zeros((Hn, N, 64), np.float32)
    K = np.zeros((Hn, T, 64), np.float32)
    blk = np.searchsorted(f, np.arange(T), side="right") - 1
    for h in range(Hn):
        q[h] = codes * sc
        K[h] = np.where((blk < N)[:, None], codes[np.clip(blk, 0, N - 1)] * sc, 0.0)
        K[h] += rng.standard_normal((T, 64)) * (0.5 / (sc * 8.0))      # logit noise of std 0.5
    return q, K, f


# ---- words ------------------------------------------------------------------------------------------------------------------------
NO_SPACE_LANGUAGES = {"zh", "ja", "th", "lo", "my", "yue"}
PREPEND_PUNCTUATIONS = "\"'“¿([{-"
APPEND_PUNCTUATIONS = "\"'.。,，!！?？:：”)]}、"


def split_tokens_on_unicode(tokens, decode):
    """decode: list of ids -> str with errors='replace'"""
    full = decode(tokens)
    rep = "�"
    words, word_tokens, cur, off = [], [], [], 0
    for t in tokens:
        cur.append(t)
        dec = decode(cur)
        if rep not in dec or full[off + dec.index(rep)] == rep:
            words.append(dec)
            word_tokens.append(cur)
            cur = []
            off += len(dec)
    return words, word_tokens


def split_tokens_on_spaces(tokens, decode, eot):
    subwords, subword_tokens = split_tokens_on_unicode(tokens, decode)
    words, word_tokens = [], []
    for sw, st in zip(subwords, subword_tokens):
        special = st[0] >= eot
        with_space = sw.startswith(" ")
        punctuation = sw.strip() in string.punctuation
        if special or with_space or punctuation or len(words) == 0:
            words.append(sw)
            word_tokens.append(list(st))
        else:
            words[-1] = words[-1] + sw
            word_tokens[-1].extend(st)
    return words, word_tokens


def split_to_word_tokens(tokens, decode, language, eot):
    if language in NO_SPACE_LANGUAGES:
        return split_tokens_on_unicode(tokens, decode)
    return split_tokens_on_spaces(tokens, decode, eot)


def merge_punctuations(words, word_tokens, prepended=PREPEND_PUNCTUATIONS, appended=APPEND_PUNCTUATIONS):
    """words: list of str, word_tokens: list of lists; merged in place as openai-whisper does (emptied entries stay, callers drop them)."""
    i, j = len(words) - 2, len(words) - 1
    while i >= 0:
        if words[i].startswith(" ") and words[i].strip() in prepended:
            words[j] = words[i] + words[j]
            word_tokens[j] = word_tokens[i] + word_tokens[j]
            words[i] = ""
            word_tokens[i] = []
        else:
            j = i
        i -= 1
    i, j = 0, 1
    while j < len(words):
        if not words[i].endswith(" ") and words[j] in appended:
            words[i] = words[i] + words[j]
            word_tokens[i] = word_tokens[i] + word_tokens[j]
            words[j] = ""
            word_tokens[j] = []
        else:
            i = j
        j += 1
    return words, word_tokens


def word_timings(text_tokens, text_indices, time_indices, probs, decode, language, eot):
    """find_alignment's tail: [(word, start, end, probability)] for the text tokens (eot appended as the last 'word' and dropped)."""
    words, word_tokens = split_to_word_tokens(list(text_tokens) + [eot], decode, language, eot)
    if len(word_tokens) <= 1:
        return []
    words, word_tokens = merge_punctuations(words[:-1], word_tokens[:-1])      # (the eot "word" takes no part)
    bounds = np.pad(np.cumsum([len(t) for t in word_tokens]), (1, 0))
    jt = jump_times(text_indices, time_indices)
    out = []
    for w, toks, s, e in zip(words, word_tokens, bounds[:-1], bounds[1:]):
        if not toks:
            continue
        out.append((w, float(jt[s]), float(jt[e]), float(np.mean(probs[s:e]))))
    return out


# ---- the matrix stage by stage: float32 models in the kernels' operation order, inputs, per-element bounds ---------------------------------
U = 2.0 ** -24          # unit roundoff of fp32
ABS_P = 2.0 ** -125     # a probability below 2^-126 is a denormal or flushed: once for expf's result, once for the quotient


def gamma(n):
    """n roundings compounded: (1 + U)^n - 1 <= n U / (1 - n U)"""
    return n * U / (1.0 - n * U)


def expf_allowance(x32):
    """relative error allowed to one expf: numpy's float32 exp against float64 over these arguments (results in the normal range), times 2
    (margin: another libm).  Returns (allowance, measured), both relative."""
    x = np.asarray(x32, np.float32).ravel()
    x = x[np.isfinite(x) & (x > -87.0)]
    if x.size == 0:
        return 0.0, 0.0
    want = np.exp(x.astype(np.float64))
    meas = float(np.max(np.abs(np.exp(x).astype(np.float64) - want) / want))
    return 2.0 * meas, meas


def k_image(K16):
    """K f16 [T][64] -> the cross-attention image [8][T][8]"""
    T = K16.shape[0]
    return np.ascontiguousarray(K16.reshape(T, 8, 8).transpose(1, 0, 2))


def scores_model32(q16, K16):
    """align_scores_kernel in fp32: 32 two-term dot steps in dimension order into one fp32 accumulator, row maximum, expf(s - max) summed per
    lane (keys lane, lane + 64, ...) and over the 64 lanes pairwise, then the quotient.  -> (p f32 [N][T], the expf arguments f32)"""
    q, K = np.asarray(q16, np.float64), np.asarray(K16, np.float64)
    N, T = q.shape[0], K.shape[0]
    acc = np.zeros((N, T), np.float32)
    for d in range(0, 64, 2):
        acc = (np.outer(q[:, d], K[:, d]) + np.outer(q[:, d + 1], K[:, d + 1]) + acc).astype(np.float32)
    x = acc - acc.max(-1, keepdims=True)
    e = np.exp(x)
    Tp = -(-T // 64) * 64
    ep = np.zeros((N, Tp), np.float32)
    ep[:, :T] = e
    lanes = ep.reshape(N, Tp // 64, 64)
    su = lanes[:, 0]
    for k in range(1, Tp // 64):
        su = su + lanes[:, k]
    while su.shape[-1] > 1:
        su = su[:, 0::2] + su[:, 1::2]
    return e / su, x


def scores_bound(q16, K16):
    """float64 softmax(q K^T) over all T keys from the f16 values the kernel reads, and the per-element bound of module-level derivation (a).
    -> (p [N][T], bound [N][T], (allowance, measured) of expf)"""
    q, K = np.asarray(q16, np.float64), np.asarray(K16, np.float64)
    T = K.shape[0]
    s = q @ K.T
    aq, aK = np.abs(q), np.abs(K)
    absdot = aq @ aK.T
    nq, nK = aq * (aq >= 2.0 ** -14), aK * (aK >= 2.0 ** -14)      # what is left when f16 denormal operands are read as zero
    es = gamma(64) * absdot + (absdot - nq @ nK.T)
    x = s - s.max(-1, keepdims=True)
    e = np.exp(x)
    p = e / e.sum(-1, keepdims=True)
    E, meas = expf_allowance(x.astype(np.float32))
    esm = es.max(-1, keepdims=True)
    A = 2.0 * esm + U * ((np.abs(x) + 2.0 * esm) + (p * np.abs(x)).sum(-1, keepdims=True) + 2.0 * esm) + gamma(-(-T // 64) + 5) + 2.0 * E + U
    return p, p * np.expm1(A) + ABS_P, (E, meas)


def norm_model32(w):
    """align_norm_kernel on one (utterance, head): w f32 [N][F] -> (w - mean) / std over the rows, four row partitions r = p (mod 4) summed
    in order and combined ((p0 + p1) + p2) + p3, two passes, population std.  Every operation is a correctly rounded fp32 one."""
    w = np.asarray(w, np.float32)
    N, F = w.shape
    nf = np.float32(N)

    def part_sum(v):
        sp = []
        for p in range(4):
            a = np.zeros(F, np.float32)
            for r in range(p, N, 4):
                a = a + v[r]
            sp.append(a)
        return ((sp[0] + sp[1]) + sp[2]) + sp[3]
    with np.errstate(all="ignore"):
        mean = part_sum(w) / nf
        dlt = w - mean
        sd = np.sqrt(part_sum(dlt * dlt) / nf)
        return dlt / sd


def norm_terms(absd, sd, meanabs, N):
    """derivation (b): |z_gpu - z| <= (|d| kappa + e_mu (1 + U)^2 / (1 - eps)) / sd"""
    n0 = -(-N // 4)
    emu = gamma(n0 + 3) * meanabs
    eps = gamma(n0 + 8)
    with np.errstate(all="ignore"):
        X = (emu / sd) ** 2
        up = (1.0 + U) ** 2
        kappa = np.maximum(1.0 - (2.0 - up) / (np.sqrt(1.0 + X) * (1.0 + eps)), up / (1.0 - eps) - 1.0)
        return (absd * kappa + emu * up / (1.0 - eps)) / sd


def norm_bound(w):
    """w [N][F] (the very fp32 values the kernel read) -> float64 (w - mean) / std, its per-element bound, and the columns that take no part
    (float64 std below 2^-40 |mean|: there fp32 may reach std = 0)"""
    w = np.asarray(w, np.float64)
    N = w.shape[0]
    mu = w.mean(0)
    d = w - mu
    sd = np.sqrt((d * d).mean(0))
    excl = ~(sd >= 2.0 ** -40 * np.abs(mu))
    with np.errstate(all="ignore"):
        z = d / sd
    return z, norm_terms(np.abs(d), sd, np.abs(w).mean(0), N), excl


def _windows(x, width):
    pad = width // 2
    if pad == 0 or x.shape[-1] <= pad:
        return None
    xp = np.pad(x, [(0, 0)] * (x.ndim - 1) + [(pad, pad)], mode="reflect")
    return np.lib.stride_tricks.sliding_window_view(xp, width, axis=-1)


def median_select32(x, width):
    """align_median_kernel's selection on f32 rows: the element of rank width // 2 of every reflect-padded window, NaN last, equal values in
    index order (a stable sort); unchanged when frames <= width // 2"""
    x = np.asarray(x, np.float32)
    win = _windows(x, width)
    return x if win is None else np.sort(win, axis=-1, kind="stable")[..., width // 2]


def median_sum_model32(chunks, width, nsel):
    """chunks: per chunk f32 [Gc][N][F] of one utterance -> acc f32 [N][F]: per chunk a = 0 + m_0 + m_1 + ... in head order, later chunks
    + acc, the last one -(a / nsel)"""
    acc = None
    with np.errstate(all="ignore"):
        for c, Wc in enumerate(chunks):
            a = np.zeros(Wc.shape[1:], np.float32)
            for g in range(Wc.shape[0]):
                a = a + median_select32(Wc[g], width)
            if c > 0:
                a = a + acc
            acc = -(a / np.float32(nsel)) if c == len(chunks) - 1 else a
    return acc


def chain_model32(q16, K16, F, width, nsel, G):
    """the three models chained as the launcher chunks them: q16 [nsel][N][64], K16 [nsel][T][64] -> acc f32 [N][F]"""
    chunks = []
    for g0 in range(0, nsel, G):
        chunks.append(np.stack([norm_model32(scores_model32(q16[s], K16[s])[0][:, :F]) for s in range(g0, min(g0 + G, nsel))]))
    return median_sum_model32(chunks, width, nsel)


def chain_bound(q16, K16, F, width, nchunks):
    """derivation (d): q16 [H][N][64], K16 [H][T][64] -> (-mean_h median(norm(p_h)) float64 [N][F], bound [N][F], excluded outputs [F] =
    those whose window holds an excluded column of some head, worst s_b / std seen)"""
    H, N = q16.shape[0], q16.shape[1]
    med, ew, ex = [], [], []
    worst = 0.0
    for h in range(H):
        p, bp, _ = scores_bound(q16[h], K16[h])
        p, bp = p[:, :F], bp[:, :F]
        z, _, excl = norm_bound(p)
        mu = p.mean(0)
        d = np.abs(p - mu)
        sd = np.sqrt((d * d).mean(0))
        mb = bp.mean(0)
        sb = np.sqrt(((bp + mb) ** 2).mean(0))
        with np.errstate(all="ignore"):
            worst = max(worst, float(np.max(np.where(excl, 0.0, sb / sd), initial=0.0)))
            ez = (bp + mb) / (sd - sb) + d * sb / (sd * (sd - sb)) + norm_terms(d + bp + mb, sd - sb, np.abs(p).mean(0) + mb, N)
        ez = np.where(excl[None, :], 0.0, ez)
        w_e, w_x = _windows(ez, width), _windows(np.broadcast_to(excl[None, :].astype(np.float64), ez.shape), width)
        med.append(median_filter(z, width))
        ew.append(ez if w_e is None else w_e.max(-1))
        ex.append(excl if w_x is None else w_x.max(-1)[0] > 0)
    med, ew = np.array(med), np.array(ew)
    bound = ew.mean(0) + gamma(H + nchunks + 1) * (np.abs(med) + ew).mean(0)
    return -med.mean(0), bound, np.any(np.array(ex), axis=0), worst


def probs_model32(logits, eot, tg):
    """align_prob_kernel on one row: maximum and sum over ids < eot by 256 threads (id t, t + 256, ...), each wave's 64 pairwise, the four
    waves ((s0 + s1) + s2) + s3, then expf(l[tg] - max) / sum"""
    l = np.asarray(logits, np.float32)[:eot]
    with np.errstate(all="ignore"):
        x = l - l.max()
        e = np.exp(x)
        n = -(-eot // 256) * 256
        ep = np.zeros(n, np.float32)
        ep[:eot] = e
        su = ep.reshape(-1, 256)
        a = su[0]
        for k in range(1, su.shape[0]):
            a = a + su[k]
        a = a.reshape(4, 64)
        while a.shape[-1] > 1:
            a = a[:, 0::2] + a[:, 1::2]
        a = a[:, 0]
        return np.exp(np.float32(logits[tg]) - l.max()) / (((a[0] + a[1]) + a[2]) + a[3])


def probs_bound(logits, eot, tg):
    """float64 softmax(logits[: eot])[tg] and its bound (derivation (a) without a score error) -> (p, bound, (allowance, measured))"""
    l = np.asarray(logits, np.float64)[:eot]
    with np.errstate(all="ignore"):
        x = l - l.max()
        e = np.exp(x)
        p = e / e.sum()
        xt = float(logits[tg]) - l.max()
        pt = np.exp(xt) / e.sum()
        E, meas = expf_allowance(x.astype(np.float32))
        ax = np.where(p > 0, p * np.abs(x), 0.0).sum()
        A = U * ((abs(xt) if np.isfinite(xt) else 0.0) + ax) + gamma(-(-eot // 256) + 8) + 2.0 * E + U
    return pt, pt * np.expm1(A) + ABS_P, (E, meas)


def canon(a):
    """f32 -> uint32 with every NaN made the same word: exact comparison, NaN included"""
    a = np.ascontiguousarray(a, np.float32)
    return np.where(np.isnan(a), np.uint32(0x7FC00000), a.view(np.uint32))


def sentinel(n, base=-1000.0):
    """a pattern no kernel writes by accident: distinct neighbours, exact in f32"""
    return (base - (np.arange(n) % 997)).astype(np.float32)


# -- inputs (shared by tests/test_align_model_cpu.py and tests/test_gpu_align_stages.py) ---------------------------------------------------
def _case(i, **kw):
    kw["seed"] = 7000 + i
    return kw


_NS = [(1, 7, 8), (9, 17, 1), (8, 9, 7), (17, 1, 9), (7, 8, 17), (1, 9, 8), (17, 7, 1)]
SCORES_CASES = [_case(i, T=T, B=3, nsel=2, N=_NS[i], F=(1, max(T - 1, 1), T), spread=(0, 20, 80)[i % 3], hpc=i % 2, extra=3)
                for i, T in enumerate([1, 63, 64, 65, 100, 129, 300])]
SCORES_CASES.append(_case(7, T=1500, B=3, nsel=2, N=(17, 8, 1), F=(1, 1499, 1500), spread=20, hpc=0, extra=5))
SCORES_CASES.append(_case(8, T=100, B=3, nsel=2, N=(7, 9, 8), F=(1, 99, 100), spread=0, hpc=1, extra=1))
SCORES_CASES.append(_case(9, T=129, B=3, nsel=2, N=(8, 1, 17), F=(128, 1, 129), spread=80, hpc=0, extra=2))


def case_id(c):
    return "-".join(f"{k}{'x'.join(map(str, v)) if isinstance(v, tuple) else v}" for k, v in c.items() if k not in ("seed", "extra"))


def scores_inputs(c):
    """q fp32 [B][nsel][ncap][64] (rows >= N[b]: NaN, never read), the K buffer (f16; the nsel images of an utterance in permuted slots of
    nsel + 1, the spare one NaN), koff, kbstride, and the f16 values per (b, s): q16 [N[b]][64], K16 [T][64].  Every query has a common
    component g, and key t* >= F[b] (where F[b] < T) carries g scaled to `spread`: the row maximum and most of the mass lie beyond the crop."""
    rng = np.random.default_rng(c["seed"])
    B, nsel, T, N, F, spread = c["B"], c["nsel"], c["T"], c["N"], c["F"], c["spread"]
    nmax = max(N)
    ncap = nmax + c["extra"]
    q = np.full((B, nsel, ncap, 64), np.nan, np.float32)
    slots = nsel + 1
    kbstride = slots * T * 64
    Kbuf = np.full(B * kbstride, np.nan, np.float16)
    koff = (rng.permutation(slots)[:nsel] * T * 64).astype(np.int64)
    q16, K16 = {}, {}
    for b in range(B):
        for s in range(nsel):
            g = rng.standard_normal(64)
            g /= np.linalg.norm(g)
            qq = 2.0 * g + rng.standard_normal((N[b], 64)) * 0.05
            qq[1::2, 7] = 2e-6      # an f16 denormal
            K = rng.standard_normal((T, 64)) * (0.6 if spread else 0.0)
            ts = int(rng.integers(F[b], T)) if F[b] < T else T - 1
            K[ts] += g * (spread / 2.0)
            q[b, s, :N[b]] = qq
            q16[b, s] = qq.astype(np.float32).astype(np.float16)
            K16[b, s] = K.astype(np.float16)
            o = b * kbstride + int(koff[s])
            Kbuf[o:o + T * 64] = k_image(K16[b, s]).ravel()
    return dict(q=q, Kbuf=Kbuf, koff=koff, kbstride=kbstride, ncap=ncap, nmax=nmax, fmax=max(F), q16=q16, K16=K16)


NORM_CASES = [_case(100 + i, T=T, B=1, nsel=2, N=(N,), F=(F,), hpc=i % 2) for i, (N, F, T) in enumerate(
    [(2, 1, 1), (3, 63, 63), (4, 64, 64), (5, 65, 65), (8, 65, 100), (447, 64, 65), (2, 63, 129), (447, 1, 63), (3, 65, 300)])]
NORM_CASES.append(_case(120, T=100, B=3, nsel=2, N=(5, 1, 9), F=(65, 3, 17), hpc=0))
NORM_CASES.append(_case(121, T=65, B=3, nsel=3, N=(5, 1, 9), F=(65, 3, 17), hpc=2))


def norm_inputs(c):
    """W per (b, s): f32 [N[b]][F[b]] of positive weights, column scales from 1 to 1e-6; every third column has a large mean and a small
    spread (std / mean about 1e-3 and 1e-5)"""
    rng = np.random.default_rng(c["seed"])
    out = {}
    for b in range(c["B"]):
        for s in range(c["nsel"]):
            N, F = c["N"][b], c["F"][b]
            w = rng.random((N, F)) * 10.0 ** -rng.uniform(0, 6, F)
            tight = np.arange(F) % 3 == 2
            w[:, tight] = (0.5 + rng.random((N, F)) * np.where(np.arange(F) % 2, 1e-3, 1e-5))[:, tight]
            out[b, s] = w.astype(np.float32)
    return out


def pack_w(c, per, G, T):
    """per[(b, s)] f32 [N[b]][F[b]] -> the stage tap's W: chunk k at k B G nmax T, laid out [B][Gc][nmax][T], everything else sentinel"""
    B, nsel, nmax = c["B"], c["nsel"], max(c["N"])
    region = B * G * nmax * T
    nch = -(-nsel // G)
    W = sentinel(nch * region)
    for k in range(nch):
        Gc = min(G, nsel - k * G)
        v = W[k * region:k * region + B * Gc * nmax * T].reshape(B, Gc, nmax, T)
        for b in range(B):
            for g in range(Gc):
                a = per[b, k * G + g]
                v[b, g, :a.shape[0], :a.shape[1]] = a
    return W


def unpack_w(c, W, G, T):
    """the reverse: (per[(b, s)] f32 [N[b]][T] (whole rows), mask of the elements of W inside some [b][g][row < N[b]][:])"""
    B, nsel, nmax = c["B"], c["nsel"], max(c["N"])
    region = B * G * nmax * T
    per, inside = {}, np.zeros(W.shape, bool)
    for k in range(-(-nsel // G)):
        Gc = min(G, nsel - k * G)
        v = W[k * region:k * region + B * Gc * nmax * T].reshape(B, Gc, nmax, T)
        m = inside[k * region:k * region + B * Gc * nmax * T].reshape(B, Gc, nmax, T)
        for b in range(B):
            for g in range(Gc):
                per[b, k * G + g] = v[b, g, :c["N"][b]].copy()
                m[b, g, :c["N"][b]] = True
    return per, inside


def _median_cases():
    chunkings = [(3, 1), (3, 2), (3, 0), (5, 1), (5, 2), (5, 0)]
    out, i = [], 0
    for width in (1, 3, 7, 21, 63):
        pad = width // 2
        Fs = sorted({1, max(pad, 1), pad + 1, max(2 * pad, 1), 255, 256, 257, 300})
        for j in range(0, len(Fs), 3):
            F = tuple((Fs[j:j + 3] + Fs[:3])[:3])
            nsel, hpc = chunkings[i % 6]
            out.append(_case(200 + i, T=300, B=3, nsel=nsel, N=(2, 1, 3), F=F, hpc=hpc, width=width))
            i += 1
    return out


MEDIAN_CASES = _median_cases()


def median_inputs(c, planted=False):
    """W per (b, s): f32 [N[b]][F[b]] on a grid of halves (ties everywhere); planted: single NaNs, NaN runs longer than the
    half width, +inf and -inf among them"""
    rng = np.random.default_rng(c["seed"] + (50 if planted else 0))
    pad = c["width"] // 2
    out = {}
    for b in range(c["B"]):
        for s in range(c["nsel"]):
            N, F = c["N"][b], c["F"][b]
            w = (np.round(rng.standard_normal((N, F)) * 2) / 2 + 0.0).astype(np.float32)      # (+ 0.0: no -0, whose place among zeros no sort defines)
            if planted:
                for r in range(N):
                    for _ in range(1 + F // 40):
                        w[r, rng.integers(0, F)] = np.nan
                        w[r, rng.integers(0, F)] = np.inf
                        w[r, rng.integers(0, F)] = -np.inf
                    a = int(rng.integers(0, F))
                    w[r, a:a + pad + 2] = np.nan
                    if r == 0:
                        w[r, :min(F, pad + 1)] = np.nan      # a run across the reflected edge
            out[b, s] = w
    return out


CHAIN_CASE = _case(300, T=100, B=3, nsel=3, N=(9, 4, 17), F=(65, 100, 30), spread=3, extra=4, width=7)
PROBS_EOT = [1, 63, 255, 256, 257, 50257]


def probs_inputs(eot):
    """logits f32 [8][vpad], target [8], dst [8] (a permutation into 12 slots): ids >= eot hold +50 (they must not count), rows 2 and 4 have
    no target, row 3 is all -inf, rows 5 and 6 hold -inf entries (row 6's target is one of them), targets at id 0 and eot - 1"""
    rng = np.random.default_rng(400 + eot)
    rows, vpad = 8, eot + 7
    lg = (rng.standard_normal((rows, vpad)) * 3.0).astype(np.float32)
    lg[:, eot:] = 50.0
    lg[3, :eot] = -np.inf
    lg[5, rng.integers(0, eot, max(1, eot // 5))] = -np.inf
    tg = np.array([0, eot - 1, -1, 0, -1, int(rng.integers(0, eot)), eot // 2, int(rng.integers(0, eot))], np.int32)
    lg[6, tg[6]] = -np.inf
    if eot > 1:
        lg[6, (tg[6] + 1) % eot] = 1.0      # (something finite in the row)
    dst = rng.permutation(12)[:rows].astype(np.int32)
    return lg, tg, dst


def capture_expected(dq, sel_head, s0, n, nsel, ub0, t0, P, ncap, qsel):
    """align_capture_kernel by its definition, on a copy of qsel (f16 [utterances][nsel][ncap][64])"""
    out = qsel.copy()
    for r in range(dq.shape[0]):
        b, i = ub0 + r // 16, t0 + r % 16 - P
        if 0 <= i < ncap:
            for s in range(s0, s0 + n):
                with np.errstate(over="ignore"):
                    out[b, s, i] = dq[r, sel_head[s] * 64:sel_head[s] * 64 + 64].astype(np.float16)
    return out
