"""Test helper (not product code): CTranslate2's `repetition_penalty` and `no_repeat_ngram_size` on the CPU, for the oracle's search.

The two processors are CTranslate2 4.1.0's RepetitionPenalty and NoRepeatNgram, restated (unpinned: no CTranslate2 here), over the
history the engine documents (include/wis_hip.h): what the search has generated for a beam so far - no start sequence, no decoder prefix.
  penalty p: every DISTINCT history token's raw logit x becomes x * p if x < 0 else x / p, in float32 with a true division, once however
             often the token occurs; applied to the raw rows, before every other processor;
  n-gram n:  with a history h of L >= n tokens, every i in [0, L - n] with h[i .. i+n-2] == h[L-n+1 .. L-1] masks h[i+n-1].
`RepStepFn` plugs them into `oracle.whisper_ref.WhisperRef.search` around `WhisperRef.apply_processors` (penalty, processors, bans),
tracking every live beam's history through the search's `last` / `origin` arguments.  `RepRaw` is the same pair of rules as a wrapper of a
raw-logits function - the bans are masks and commute with the other masks - for composing with `ts_ref.TsStepFn`: the penalty comes first
and the bans stand before the timestamp decision."""
import numpy as np
import torch

EOT = 50257
NEG = float("-inf")


def penalise(rows, hists, p):
    """rows [k, V] float32 tensor -> copy with the penalty applied per row to the distinct tokens of hists[row] (fp32, true division);
    p = 1, or no history yet: the rows themselves."""
    if p == 1 or not any(hists):
        return rows
    out = rows.clone().float()
    pt = torch.tensor(float(np.float32(p)), dtype=torch.float32)
    for r, seq in enumerate(hists):
        if not seq:
            continue
        idx = torch.tensor(sorted(set(int(t) for t in seq)), dtype=torch.long)
        x = out[r, idx]                                   # gather, penalise, scatter: no compounding
        out[r, idx] = torch.where(x < 0, x * pt, x / pt)
    return out


def banned_tokens(seq, n):
    """The tokens NoRepeatNgram masks after history `seq` (a sorted list)."""
    L = len(seq)
    if n < 1 or L < n:
        return []
    tail = list(seq[L - n + 1:])
    return sorted({int(seq[i + n - 1]) for i in range(L - n + 1) if list(seq[i:i + n - 1]) == tail})


def ban(rows, hists, n):
    """rows with every row's banned tokens at -inf (a copy when anything is banned)."""
    bans = [banned_tokens(seq, n) for seq in hists]
    if not any(bans):
        return rows
    out = rows.clone()
    for r, b in enumerate(bans):
        if b:
            out[r, b] = NEG
    return out


class _Hist:
    def __init__(self, k):
        self.hist = [[] for _ in range(k)]

    def advance(self, last, origin):
        if origin is not None:
            self.hist = [self.hist[o] + [int(last[j])] for j, o in enumerate(origin)]


class RepStepFn(_Hist):
    """step_fn for WhisperRef.search: raw(step, last, origin) -> raw logits [k, V]."""

    def __init__(self, raw, k, suppress_ids, suppress_begin, suppress_blank=True, fixed_new=0, penalty=1.0, ngram=0, eot=EOT):
        super().__init__(k)
        self.raw, self.kw = raw, (suppress_ids, suppress_begin, suppress_blank, fixed_new, eot)
        self.penalty, self.ngram = (1.0 if penalty == 0 else penalty), ngram

    def __call__(self, step, last, origin):
        from oracle.whisper_ref import WhisperRef
        self.advance(last, origin)
        lg = penalise(self.raw(step, last, origin), self.hist, self.penalty)
        lg = WhisperRef.apply_processors(lg, step, *self.kw)
        return ban(lg, self.hist, self.ngram)


class RepRaw(_Hist):
    """raw(step, last, origin) -> the raw rows with both rules applied (for a step_fn that does the rest, e.g. ts_ref.TsStepFn)."""

    def __init__(self, raw, k, penalty=1.0, ngram=0):
        super().__init__(k)
        self.raw, self.penalty, self.ngram = raw, (1.0 if penalty == 0 else penalty), ngram

    def __call__(self, step, last, origin):
        self.advance(last, origin)
        return ban(penalise(self.raw(step, last, origin), self.hist, self.penalty), self.hist, self.ngram)
