"""Test helper (not product code): the engine's random sampling on the CPU (include/wis_hip.h states the rule).

  noise   w = Philox4x32-10(counter = (token id, step, sample index j within the utterance, 0), key = (seed_lo, seed_hi))[0],
          u = ((w >> 9) + 0.5) 2^-23, g = -log(-log(u)) - here in float64;
  draw    x = the processed logits (repetition rules, suppress lists, timestamp rules, fixed_new_tokens: tests/rep_ref.py, tests/ts_ref.py,
          WhisperRef.apply_processors), K = every unmasked id or the k largest x (value descending, id ascending),
          t = argmax over K of (x[t] / T + g(t)), ties to the lower id;
  score   sum of (x[t] - logsumexp(x over all unmasked ids)) / T, then / len ** length_penalty as the greedy path.
`sampled_search` runs n independent samples of one utterance over a logits function and records, per draw, the gap between the two best
perturbed values: the engine forms x / T + g in fp32 with a <= 2 ulp logf, so a draw closer than MARGIN * max(1, 1 / T) may fall either way."""
import math

import numpy as np
import torch

from rep_ref import ban, penalise
from ts_ref import apply_ts_rules

EOT = 50257
MARGIN = 2e-4
M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
_U32 = np.uint64(0xFFFFFFFF)


def philox4x32_10(counter, key):
    """counter: four uint32 arrays (broadcastable), key: two -> the four output words (uint32 arrays)."""
    c = [np.asarray(x, np.uint64) & _U32 for x in counter]
    k0, k1 = (np.uint64(int(k) & 0xFFFFFFFF) for k in key)
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c[0], np.uint64(M1) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k0, p1 & _U32, (p0 >> np.uint64(32)) ^ c[3] ^ k1, p0 & _U32]
        k0, k1 = (k0 + np.uint64(W0)) & _U32, (k1 + np.uint64(W1)) & _U32
    return [x.astype(np.uint32) for x in c]


def noise_words(ids, step, j, seed):
    """The word of every token id in `ids` at (step, sample j) under the utterance's 64-bit seed."""
    ids = np.asarray(ids, np.uint64)
    return philox4x32_10((ids, np.uint64(step), np.uint64(j), np.uint64(0)), (int(seed) & 0xFFFFFFFF, (int(seed) >> 32) & 0xFFFFFFFF))[0]


def u_of_word(w, dtype=np.float64):
    """((w >> 9) + 0.5) 2^-23 (every operation is exact in float32 as well as in float64)."""
    return ((np.asarray(w, np.uint32) >> np.uint32(9)).astype(dtype) + dtype(0.5)) * dtype(2.0 ** -23)


def gumbel_of_word(w):
    return -np.log(-np.log(u_of_word(w)))


def draw(x, T, topk, words_of):
    """x: processed logits [V] float32 (masked: -inf); topk -1: whole vocabulary, k >= 2: the k best; words_of(ids) -> uint32 noise words.
    -> (token, gap between the two best perturbed values, (x[t] - lse) / T)."""
    x = np.asarray(x, np.float32)
    x64 = x.astype(np.float64)
    alive = np.flatnonzero(x > -np.inf)
    K = alive if topk < 0 else np.argsort(-x, kind="stable")[:topk]
    K = K[x[K] > -np.inf]
    p = x64[K] / float(np.float32(T)) + gumbel_of_word(words_of(K))
    pm = p.max()
    t = int(K[p == pm].min())                         # perturbed value descending, then id ascending
    gap = float(pm - np.partition(p, -2)[-2]) if len(K) > 1 else math.inf
    mx = x64[alive].max()
    lse = mx + math.log(np.exp(x64[alive] - mx).sum())
    return t, gap, (x64[t] - lse) / float(np.float32(T))


def processed(raw, step, hists, suppress_ids, suppress_begin, suppress_blank=True, fixed_new=0, penalty=1.0, ngram=0, timestamps=False, max_init=50):
    """raw [rows, V] float tensor -> (the rows as the sampling kernels see them, the timestamp decision's smallest margin)."""
    from oracle.whisper_ref import WhisperRef
    lg = penalise(raw.float(), hists, 1.0 if penalty == 0 else penalty)
    lg = WhisperRef.apply_processors(lg, step, suppress_ids, suppress_begin, suppress_blank, fixed_new, EOT)
    lg = ban(lg, hists, ngram)
    ts_margin = math.inf
    if timestamps and not (fixed_new > 0 and step >= fixed_new):
        lg, m = apply_ts_rules(lg, hists, max_init)
        ts_margin = min(m)
    return lg, ts_margin


def sampled_search(raw_fn, n, max_new, topk, T, seed, length_penalty=1.0, words_fn=None, eot=EOT, **proc):
    """n samples of one utterance.  raw_fn(step, last tokens [n] or None) -> raw logits [n, V] (float tensor; finished rows are fed EOT and
    ignored).  words_fn(step, j, ids) replaces the Philox words (a test's noise table).  proc: processed()'s keywords.
    -> dict(ids [n lists], scores [n], finish_step, draws, min_gap (relative to the margin unit: gap / max(1, 1 / T)), ts_margin)"""
    hists = [[] for _ in range(n)]
    cum = [0.0] * n
    done = [False] * n
    out_len, scores = [0] * n, [0.0] * n
    last, min_gap, ts_margin, draws, finish_step = None, math.inf, math.inf, 0, None
    unit = max(1.0, 1.0 / float(T))
    for step in range(max_new):
        lg, tm = processed(raw_fn(step, last), step, hists, **proc)
        lg = lg.numpy()
        is_last = step + 1 >= max_new
        nxt = []
        for j in range(n):
            if done[j]:
                hists[j] = hists[j] + [eot]           # (what the engine's history collects; a finished row's result is frozen)
                nxt.append(eot)
                continue
            ts_margin = min(ts_margin, tm)
            wf = (lambda ids, j=j: words_fn(step, j, ids)) if words_fn else (lambda ids, j=j: noise_words(ids, step, j, seed))
            t, gap, sc = draw(lg[j], T, topk, wf)
            draws += 1
            min_gap = min(min_gap, gap / unit)
            cum[j] += sc
            hists[j] = hists[j] + [t]
            if t == eot or is_last:
                done[j] = True
                out_len[j] = step if t == eot else step + 1
                s = cum[j]
                if length_penalty != 0:
                    den = float(out_len[j]) ** length_penalty
                    s = s / den if den != 0 else (-math.inf if s < 0 else math.nan)
                scores[j] = s
                nxt.append(eot)
            else:
                nxt.append(t)
        last = nxt
        if all(done):
            finish_step = step
            break
    return dict(ids=[hists[j][:out_len[j]] for j in range(n)], scores=scores, finish_step=finish_step, draws=draws, min_gap=min_gap, ts_margin=ts_margin)


def table_fn(table, b, n):
    """raw_fn over a wis_debug_search_n table [steps][B*n][V]: sample j of utterance b reads row s*B*n + b*n + j, step 0 row b*n for every sample."""
    tt = torch.from_numpy(table)
    return lambda step, last: tt[step, b * n:(b + 1) * n] if step > 0 else tt[0, b * n].expand(n, -1)


def chi_square(counts, probs):
    counts, probs = np.asarray(counts, np.float64), np.asarray(probs, np.float64)
    e = counts.sum() * probs
    return float(((counts - e) ** 2 / e).sum())


# upper 1e-4 quantiles of chi-square (scipy.stats.chi2.isf(1e-4, df)), by degrees of freedom
CHI2_1E4 = {1: 15.137, 2: 18.421, 3: 21.108, 4: 23.513, 5: 25.745, 6: 27.856, 7: 29.878}
