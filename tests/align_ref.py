"""Reference restatement of word-level alignment for the tests (numpy, float64 unless stated): cross-attention weights of chosen
heads, normalise / median / head-mean / negate, dynamic time warping (openai-whisper dtw_cpu's loop: cost table in f32, trace 0 / 1 / 2,
borders trace[0][:] = 2 and trace[:][0] = 1), and the word grouping of openai-whisper's split_to_word_tokens + merge_punctuations with
the jump times of find_alignment.  Restated from the public openai-whisper / transformers sources; nothing here imports the engine."""
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
