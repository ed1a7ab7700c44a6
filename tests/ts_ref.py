"""Test helper (not product code): Whisper's timestamp rules on the CPU, for the oracle's search.

The rules are openai-whisper's `ApplyTimestampRules` (CTranslate2 applies them when the prompt lacks <|notimestamps|>;
transformers' `WhisperTimeStampLogitsProcessor` states the same).  Processor order, as the engine documents it (unpinned):
suppress_tokens, suppress_blank at step 0, the measurement convention's EOT mask, then these rules; the convention's forced EOT
overrides them.  `step_fn` plugs all of that into `oracle.whisper_ref.WhisperRef.search`, tracking every live beam's history
through the search's `origin` argument and recording the timestamp decision's margin |logsumexp(timestamps) - max(text)| per step
(a near tie there may legitimately flip under another summation order, like a near tie of two candidates)."""
import math

import numpy as np
import torch

EOT, SOT, NO_TIMESTAMPS = 50257, 50258, 50363
TB = NO_TIMESTAMPS + 1
V = 51865
NEG = float("-inf")


def apply_ts_rules(lg, hists, max_init=50, stats=None):
    """lg [rows, V] float tensor (processed so far; modified copy), hists: generated tokens per row -> (lg, margins per row)."""
    lg = lg.clone()
    Vr = lg.shape[1]
    lg[:, NO_TIMESTAMPS] = NEG
    margins = []
    for r, seq in enumerate(hists):
        last_ts = len(seq) >= 1 and seq[-1] >= TB
        pen_ts = len(seq) < 2 or seq[-2] >= TB
        if last_ts:
            if pen_ts:
                lg[r, TB:] = NEG
                _count(stats, "after_pair")
            else:
                lg[r, :EOT] = NEG
                _count(stats, "open_segment")
        stamps = [t for t in seq if t >= TB]
        if stamps:
            t_last = stamps[-1] if (last_ts and not pen_ts) else stamps[-1] + 1
            lg[r, TB:t_last] = NEG
            _count(stats, "monotonic_repeat_allowed" if (last_ts and not pen_ts) else "monotonic")
        if not seq:
            lg[r, :TB] = NEG
            if max_init is not None:
                lg[r, TB + max_init + 1:] = NEG
                _count(stats, "initial_cap")
    for r in range(lg.shape[0]):
        row = lg[r].double()
        ts = row[TB:Vr]
        mt = float(row[:TB].max())
        lse = float(torch.logsumexp(ts, 0)) if bool(torch.isfinite(ts).any()) else NEG
        if lse > mt:
            lg[r, :TB] = NEG
            if hists[r]:
                _count(stats, "decision_timestamp")
        elif hists[r]:
            _count(stats, "decision_text")
        margins.append(abs(lse - mt) if math.isfinite(lse) and math.isfinite(mt) else float("inf"))
    return lg, margins


def _count(stats, key):
    if stats is not None:
        stats[key] = stats.get(key, 0) + 1


class TsStepFn:
    """step_fn for WhisperRef.search: raw(step, last, origin) -> raw logits [k, V]; applies the processors, then the rules.
    `.margins` = the smallest decision margin of each step (inf where nothing was decided)."""

    def __init__(self, raw, k, suppress_ids, suppress_begin, suppress_blank=True, fixed_new=0, max_init=50, stats=None):
        self.raw, self.k = raw, k
        self.kw = (suppress_ids, suppress_begin, suppress_blank, fixed_new)
        self.max_init, self.stats = max_init, stats
        self.hist = [[] for _ in range(k)]
        self.margins = []

    def __call__(self, step, last, origin):
        from oracle.whisper_ref import WhisperRef
        if origin is not None:
            self.hist = [self.hist[o] + [int(last[j])] for j, o in enumerate(origin)]
        suppress_ids, suppress_begin, suppress_blank, fixed_new = self.kw
        lg = WhisperRef.apply_processors(self.raw(step, last, origin).float(), step, suppress_ids, suppress_begin, suppress_blank, fixed_new, EOT)
        if fixed_new > 0 and step >= fixed_new:          # the forced EOT overrides every rule
            self.margins.append(float("inf"))
            return lg
        lg, m = apply_ts_rules(lg, self.hist, self.max_init, self.stats)
        self.margins.append(min(m))
        return lg


def hf_processor(max_init=50, begin_index=4):
    """transformers' WhisperTimeStampLogitsProcessor with the multilingual ids (the statement of the rules the tests pin against)."""
    from types import SimpleNamespace
    from transformers.generation.logits_process import WhisperTimeStampLogitsProcessor
    cfg = SimpleNamespace(no_timestamps_token_id=NO_TIMESTAMPS, eos_token_id=EOT, bos_token_id=EOT, max_initial_timestamp_index=max_init,
                          _detect_timestamp_from_logprob=True)
    return WhisperTimeStampLogitsProcessor(cfg, begin_index=begin_index)


def generate_ts(ref, mel, prompt, beam_size, suppress_ids, suppress_begin, fixed_new=0, max_new_tokens=0, max_init=50, stats=None):
    """WhisperRef.generate with the timestamp rules: -> (search record, TsStepFn).  Same decoder arithmetic as the oracle's generate."""
    memory = torch.as_tensor(np.asarray(ref.encode(np.asarray(mel, np.float32)[None])[0], np.float32))
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
        return ref.decoder_step(np.asarray(toks)[:, None], P - 1 + step, state["cache"], ckv)
    fn = TsStepFn(raw, k, suppress_ids, suppress_begin, True, fixed_new, max_init, stats)
    from oracle.whisper_ref import WhisperRef
    r = WhisperRef.search(fn, k, ref.V, ref.eot, max_new, 1.0, 1.0)
    return r, fn


def grammar_errors(ids, max_init=50):
    """What a sequence decoded under the rules must obey: first token a timestamp <= <|0.00|> + max_init, timestamps non-decreasing,
    timestamps in pairs except the last one before EOT (a lone timestamp after text, then more text, is a violation)."""
    errs = []
    if not ids:
        return errs
    if ids[0] < TB or (max_init is not None and ids[0] > TB + max_init):
        errs.append(f"first token {ids[0]}")
    stamps = [t for t in ids if t >= TB]
    if any(b < a for a, b in zip(stamps, stamps[1:])):
        errs.append(f"decreasing timestamps {stamps}")
    if NO_TIMESTAMPS in ids:
        errs.append("<|notimestamps|> generated")
    # pairs: a timestamp that follows text must be followed by a timestamp or end the sequence (the rule masks text [0, EOT) only:
    # EOT and the special ids [EOT, <|0.00|>) that no suppression list covers stay allowed)
    for i in range(1, len(ids) - 1):
        if ids[i] >= TB and ids[i - 1] < TB and ids[i + 1] < EOT:
            errs.append(f"unpaired timestamp at {i}")
    if len(ids) >= 2 and ids[0] >= TB and ids[1] >= TB:      # the opening timestamp is followed by text
        errs.append("two timestamps at the start")
    for i in range(1, len(ids) - 1):          # after a pair comes text: never three timestamps in a row
        if ids[i - 1] >= TB and ids[i] >= TB and ids[i + 1] >= TB:
            errs.append(f"three timestamps at {i}")
    return errs
