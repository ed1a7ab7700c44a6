"""Test helper (not product code): phrase-constrained decoding on the CPU, for the oracle's search.

The rule is the one include/wis_hip.h states, written here WITHOUT the engine's trie: a phrase set is a dict of prefixes,
    prefixes[tuple(prefix)] = (sorted tokens that continue the prefix, True when the prefix itself is a phrase),
with the empty tuple for the root.  A live row whose generated history is a key of the dict keeps its children's values - and <|endoftext|>'s
when the history is a phrase - bit for bit; every other id of the row becomes -inf.  A row whose history is no key is left as it is.
`PhraseStepFn` plugs the mask into `oracle.whisper_ref.WhisperRef.search` BEHIND `WhisperRef.apply_processors` (a mask commutes with the
other masks), tracking every live beam's history through the search's `last` / `origin` arguments as `rep_ref._Hist` does.  `brute_force`
scores every phrase in float64 under the distribution renormalised over what the set allows at each step."""
import numpy as np
import torch

from rep_ref import _Hist

EOT = 50257
NEG = float("-inf")


def prefix_dict(phrases):
    """[[ids], ...] -> {prefix tuple: (sorted continuing tokens, prefix is a phrase)}"""
    kids, ends = {(): set()}, set()
    for ph in phrases:
        ph = tuple(int(t) for t in ph)
        ends.add(ph)
        for i in range(len(ph)):
            kids.setdefault(ph[:i], set()).add(ph[i])
            kids.setdefault(ph[:i + 1], set())
    return {p: (sorted(c), p in ends) for p, c in kids.items()}


def trie_to_prefix_dict(trie):
    """The engine's flat table (int32 [n][4], include/wis_hip.h) read back into the dict form."""
    trie = np.asarray(trie).reshape(-1, 4)
    out, todo = {}, [((), 0)]
    while todo:
        prefix, i = todo.pop()
        _, first, n, ends = (int(x) for x in trie[i])
        toks = [int(trie[first + c, 0]) for c in range(n)]
        out[prefix] = (toks, bool(ends))
        todo += [(prefix + (t,), first + c) for c, t in enumerate(toks)]
    return out


def allowed(prefixes, hist, eot=EOT):
    """ids a row with history `hist` keeps, or None when the history is no path (the row stays as it is)"""
    node = prefixes.get(tuple(int(t) for t in hist))
    if node is None:
        return None
    return list(node[0]) + ([eot] if node[1] else [])


def mask_rows(rows, hists, prefixes, eot=EOT):
    """rows [k, V] tensor -> copy with the phrase mask applied per row (off-path rows untouched)"""
    out = rows.clone()
    for r, h in enumerate(hists):
        keep = allowed(prefixes, h, eot)
        if keep is None:
            continue
        vals = rows[r, keep].clone()
        out[r, :] = NEG
        out[r, keep] = vals
    return out


class PhraseStepFn(_Hist):
    """step_fn for WhisperRef.search: raw(step, last, origin) -> raw logits [k, V]; the phrase mask behind apply_processors.
    .alive[s - 1] = which beams' histories are paths of the set when step s >= 1 is computed - the beams whose cumulative score is finite
    behind step s - 1 (what the `finite_only` ancestry comparison keeps)."""

    def __init__(self, raw, k, suppress_ids, suppress_begin, prefixes, suppress_blank=True, eot=EOT):
        super().__init__(k)
        self.raw, self.kw, self.prefixes, self.eot = raw, (suppress_ids, suppress_begin, suppress_blank, 0, eot), prefixes, eot
        self.alive = []

    def __call__(self, step, last, origin):
        from oracle.whisper_ref import WhisperRef
        self.advance(last, origin)
        if step > 0:
            self.alive.append([tuple(h) in self.prefixes for h in self.hist])
        lg = WhisperRef.apply_processors(self.raw(step, last, origin), step, *self.kw)
        return mask_rows(lg, self.hist, self.prefixes, self.eot)


class NoReorderPhraseStepFn(PhraseStepFn):
    """The WRONG reference: histories that ignore the beam step's reordering."""

    def advance(self, last, origin):
        if origin is not None:
            self.hist = [self.hist[j] + [int(last[j])] for j in range(len(origin))]


def brute_force(phrases, row_of, eot=EOT, length_penalty=1.0):
    """Every phrase scored in float64: row_of(history tuple) -> the processed logits row [V] (numpy) the model gives behind that history.
    Per step log p = x[t] - logsumexp(x over the ids the set allows behind the history); the phrase's raw score adds <|endoftext|>'s term at
    its end, the normalised one divides by len(phrase) ** length_penalty (the engine's length counts the phrase's tokens, not EOT).
    -> [(normalised score, raw score, phrase tuple)] best first (ties: the phrase tuple ascending)."""
    pre = prefix_dict(phrases)
    out = []
    for ph in sorted({tuple(int(t) for t in p) for p in phrases}):
        raw = 0.0
        for i in range(len(ph) + 1):
            h = ph[:i]
            x = np.asarray(row_of(h), np.float64)
            keep = allowed(pre, h, eot)
            v = x[keep]
            mx = v.max()
            lse = mx + np.log(np.exp(v - mx).sum())
            raw += float(x[ph[i] if i < len(ph) else eot] - lse)
        out.append((raw / float(len(ph)) ** length_penalty, raw, ph))
    return sorted(out, key=lambda e: (-e[0], e[2]))
