"""Test helper (not product code): hotword boosting on the CPU, for the oracle's search.

The rule is the one include/wis_hip.h states (THE HOTWORD RULE), written here WITHOUT the engine's trie and without any cleverness: a hotword set
is `phrase_ref.prefix_dict`'s dict of prefixes, and for a row with generated history h of L tokens the BOOST SET is the union, over
k = 0 .. min(L, 31), of the tokens that continue the suffix h[L-k:] when that suffix is a key of the dict (the empty suffix always is: the
root).  A suffix that holds an id outside [0, n_vocab) is no key.  Every token of the boost set gets ONE float32 addition of the boost, however
many suffixes name it; <|endoftext|> is never boosted; "ends an entry" plays no part.
`boost_rows` is that brute force.  `active_nodes_boost_set` is a second, independently written formulation (an incremental set of active
prefixes, advanced token by token as an Aho-Corasick automaton without failure links would be) that tests/test_hotword_cpu.py holds against it.
`HotwordRaw` wraps a raw-logits function - BEHIND rep_ref.RepRaw (the penalty does not commute with an addition), AHEAD of every mask (an
addition commutes with -inf) - and `HotwordStepFn` plugs it into `oracle.whisper_ref.WhisperRef.search` in front of `apply_processors`, tracking
every live beam's history through the search's `last` / `origin` arguments as `rep_ref._Hist` does."""
import numpy as np
import torch

from rep_ref import _Hist

EOT = 50257
MAX_SUFFIX = 31      # the longest suffix that can still be continued: an entry holds at most 32 tokens


def boost_set(prefixes, hist, n_vocab, eot=EOT):
    """-> the sorted boost set of a row with generated history `hist` (brute force over the suffixes)"""
    hist = [int(t) for t in hist]
    L = len(hist)
    out = set()
    for k in range(0, min(L, MAX_SUFFIX) + 1):
        suffix = tuple(hist[L - k:])
        if any(t < 0 or t >= n_vocab for t in suffix):
            continue
        node = prefixes.get(suffix)
        if node is not None:
            out.update(int(t) for t in node[0])
    out.discard(eot)
    return sorted(t for t in out if 0 <= t < n_vocab)


def active_nodes_boost_set(prefixes, hist, n_vocab, eot=EOT):
    """The second formulation: the set of ACTIVE prefixes is advanced one history token at a time - every active prefix that the token continues
    stays (one token longer), the empty prefix joins after every token, an id outside the vocabulary clears the set, and prefixes of more than 31
    tokens cannot be continued - and the boost set is what continues the set's members at the end."""
    active = {()}
    for t in (int(t) for t in hist):
        if t < 0 or t >= n_vocab:
            active = {()}
            continue
        active = {p + (t,) for p in active if p + (t,) in prefixes and len(p) + 1 <= MAX_SUFFIX} | {()}
    out = set()
    for p in active:
        out.update(int(t) for t in prefixes[p][0])
    out.discard(eot)
    return sorted(t for t in out if 0 <= t < n_vocab)


def boost_rows(rows, hists, prefixes, boost, n_vocab=None, eot=EOT):
    """rows [k, >= n_vocab] float32 (numpy array or torch tensor) -> a copy with every row's boost set raised by `boost` in ONE float32 addition
    per element (round to nearest; -inf stays -inf, NaN stays NaN); hists[r] None: the row is left alone."""
    is_torch = isinstance(rows, torch.Tensor)
    out = rows.detach().clone().float().numpy() if is_torch else np.array(rows, np.float32, copy=True)
    V = out.shape[1] if n_vocab is None else n_vocab
    b = np.float32(boost)
    for r, h in enumerate(hists):
        if h is None:
            continue
        idx = boost_set(prefixes, h, V, eot)
        if idx:
            with np.errstate(invalid="ignore", over="ignore"):
                out[r, idx] = out[r, idx] + b
    return torch.from_numpy(out) if is_torch else out


class HotwordRaw(_Hist):
    """raw(step, last, origin) -> the raw rows with the boost applied (for a step_fn that does the rest: HotwordStepFn, ts_ref.TsStepFn).
    fixed_new > 0: nothing on the forced-EOT step."""

    def __init__(self, raw, k, prefixes, boost, n_vocab, fixed_new=0, eot=EOT):
        super().__init__(k)
        self.raw, self.prefixes, self.boost, self.V, self.fixed_new, self.eot = raw, prefixes, boost, n_vocab, fixed_new, eot

    def __call__(self, step, last, origin):
        self.advance(last, origin)
        lg = self.raw(step, last, origin)
        if self.fixed_new > 0 and step >= self.fixed_new:
            return lg
        return boost_rows(lg, self.hist, self.prefixes, self.boost, self.V, self.eot)


class HotwordStepFn:
    """step_fn for WhisperRef.search: raw(step, last, origin) -> raw logits [k, V] (rep_ref.RepRaw around it when the repetition rules are on);
    the boost, then apply_processors."""

    def __init__(self, raw, k, suppress_ids, suppress_begin, prefixes, boost, n_vocab, suppress_blank=True, fixed_new=0, eot=EOT):
        self.boosted = HotwordRaw(raw, k, prefixes, boost, n_vocab, fixed_new, eot)
        self.kw = (suppress_ids, suppress_begin, suppress_blank, fixed_new, eot)

    @property
    def hist(self):
        return self.boosted.hist

    def __call__(self, step, last, origin):
        from oracle.whisper_ref import WhisperRef
        return WhisperRef.apply_processors(self.boosted(step, last, origin), step, *self.kw)


class PerSlotHotwordRaw(HotwordRaw):
    """The WRONG reference: histories that ignore the beam step's reordering (what a kernel that kept state per slot would compute)."""

    def advance(self, last, origin):
        if origin is not None:
            self.hist = [self.hist[j] + [int(last[j])] for j in range(len(origin))]


class SampledHotwordRaw:
    """raw_fn(step, last) for sample_ref.sampled_search: a sample's row continues itself, so the histories are the rows' own tokens."""

    def __init__(self, raw_fn, n, prefixes, boost, n_vocab, eot=EOT):
        self.raw_fn, self.prefixes, self.boost, self.V, self.eot = raw_fn, prefixes, boost, n_vocab, eot
        self.hist = [[] for _ in range(n)]

    def __call__(self, step, last):
        if last is not None:
            self.hist = [h + [int(t)] for h, t in zip(self.hist, last)]
        return boost_rows(self.raw_fn(step, last), self.hist, self.prefixes, self.boost, self.V, self.eot)


def generate_hot(ref, prompt, beam_size, entries, boost, suppress_ids, suppress_begin, memory, fixed_new=0, max_new_tokens=0):
    """oracle.whisper_ref.WhisperRef.generate with the boost in front of its processors (the same decoder arithmetic, tests/ts_ref.py generate_ts's
    way): -> the search record.  memory: the oracle's encoder output [n_audio_ctx, d]; entries None: the plain search."""
    from oracle.whisper_ref import WhisperRef
    from phrase_ref import prefix_dict
    memory = torch.as_tensor(np.asarray(memory, np.float32))
    P, k = len(prompt), beam_size
    max_new = max_new_tokens if max_new_tokens > 0 else min(ref.ctx // 2, ref.ctx - P)
    ckv = ref.cross_kv(memory)
    state = {"cache": [None] * ref.L}
    if P > 1:
        ref.decoder_step(np.asarray([prompt[:-1]]), 0, state["cache"], ckv)
        state["cache"] = [(kk.expand(k, -1, -1).contiguous(), vv.expand(k, -1, -1).contiguous()) for kk, vv in state["cache"]]

    def raw(step, last, origin):
        if origin is not None:
            idx = torch.tensor(origin)
            state["cache"] = [(kk[idx], vv[idx]) for kk, vv in state["cache"]]
        toks = [prompt[-1]] * k if last is None else last
        return ref.decoder_step(np.asarray(toks)[:, None], P - 1 + step, state["cache"], ckv).float()
    if entries is None:
        fn = lambda step, last, origin: WhisperRef.apply_processors(raw(step, last, origin), step, suppress_ids, suppress_begin, True, fixed_new, ref.eot)
    else:
        fn = HotwordStepFn(raw, k, suppress_ids, suppress_begin, prefix_dict(entries), boost, ref.V, True, fixed_new, ref.eot)
    return WhisperRef.search(fn, k, ref.V, ref.eot, max_new, 1.0, 1.0)


def rescore_hot(ref, prompt, ids, entries, boost, suppress_ids, suppress_begin, memory, fixed_new=0):
    """Mean log-prob the ORACLE assigns to `ids` under the boosted rows (teacher-forced over prompt + ids): what the engine should report for them."""
    from phrase_ref import prefix_dict
    pre = prefix_dict(entries)
    lg = ref.decode_logits(np.array([list(prompt) + list(ids)[:-1]]), torch.as_tensor(np.asarray(memory, np.float32))[None])[0]
    total = 0.0
    for t, tok in enumerate(ids):
        row = lg[len(prompt) - 1 + t][None].float()
        if not (fixed_new > 0 and t >= fixed_new):
            row = boost_rows(row, [list(ids[:t])], pre, boost, ref.V, ref.eot)
        row = ref.apply_processors(row.double(), t, suppress_ids, suppress_begin, True, fixed_new, ref.eot)
        total += float(torch.log_softmax(row, dim=-1)[0, tok])
    return total / max(len(ids), 1)
