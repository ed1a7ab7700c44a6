"""Test helper (not product code): the in-grammar mass of phrase-constrained decoding (include/wis_hip.h, THE PHRASE MASS RULE) in float64, over the
dict-of-prefixes statement of a phrase set (tests/phrase_ref.py), and the fp32 error bound of the engine's reduction order.

THE RULE.  u [V]: a live row under the masks the sampling statistics give it (u_row forms it in fp32, as the kernel does: the value the rule is
stated over).  A: the ids the row's node allows (phrase_ref.allowed).  M = max u, num = sum over A of exp(u - M), den = sum over [0, V) of exp(u - M),
an entry equal to M counting as exactly 1;  logmass = min(0, log num - log den), -inf when M is -inf or num is 0.  Here num is summed about the
allowed entries' own maximum MA (log num = (MA - M) + log sum exp(u_A - MA)): the same number, without float64's own underflow 745 below M.

THE BOUND (logmass_bound), from the order csrc/dec_kernels.hip phrase_rules_mass_kernel documents.  U = 2^-24 (fp32 unit roundoff).
  One term of a sum reaches the total as a product of factors exp(a_k), a_k <= 0, whose exponents add up to -(x) with x = (the sum's maximum) - u[t]:
  exp(v - chunk maximum), one rescale exp(old - new maximum) per later chunk of its thread, one exp(thread maximum - M).  A thread owns
  C = ceil(V / 2048) chunks, so at most C + 1 factors.  Each factor: the subtraction rounds (relative U on a_k: the factor moves by |a_k| U), __expf
  multiplies by log2(e) (one rounding, and the constant's own representation error: together below 2 |a_k| U) and takes v_exp_f32 (1 ulp = 2 U).
  Over the chain the |a_k| add up to x:  3 x U + 2 (C + 1) U.  The at most C rescale multiplications and the final one: (C + 1) U.  The additions
  behind the term: at most 8 C in its thread (sequential), 6 levels of wave_sum, 2 levels over the waves: (8 C + 8) U for sums of non-negative terms.
      relative error of one term  <=  (3 x + K) U,   K = 2 (C + 1) + (C + 1) + 8 C + 8 = 11 C + 11
  so a sum S = sum exp(-x) is off by at most  sum exp(-x) (3 x + K) U  (+ V 2^-126 for terms flushed below the normal range; S >= 1: its maximum's
  own term is exactly 1).  logf is accurate to 1 ulp (2 U |log S|); MA - M rounds once (U |MA - M|); the subtraction of the logs and the final
  addition round once each.  The bound is the sum of these first-order terms; a test multiplies it by SAFETY = 2 for everything of second order.
It is evaluated on the row under test (in float64) - it depends on how the row's mass is spread, not on what the kernel returned."""
import numpy as np

from phrase_ref import EOT, allowed, prefix_dict

U = 2.0 ** -24
SAFETY = 2.0
NEG = float("-inf")


def u_row(x, bias_all=None, bias_begin=None, first=False):
    """The row the rule is stated over, formed in fp32 as logit_stats_kernel forms it: x + (bias_all or 0), then + bias_begin at the first step with
    suppress_blank (`first`)."""
    with np.errstate(invalid="ignore"):
        u = np.asarray(x, np.float32) + (np.float32(0) if bias_all is None else np.asarray(bias_all, np.float32))
        if first:
            u = u + np.asarray(bias_begin, np.float32)
    return u.astype(np.float32)


def _sum_about_max(v):
    """-> (max, sum of exp(v - max) with entries equal to the max counting 1) in float64; (-inf, 0) for nothing finite"""
    v = np.asarray(v, np.float64)
    if v.size == 0 or v.max() == NEG:
        return NEG, 0.0
    m = v.max()
    with np.errstate(invalid="ignore", over="ignore"):
        e = np.where(v == m, 1.0, np.exp(v - m))
    return m, float(e.sum())


def logmass(u, keep):
    """THE RULE for one row: u [V] (already masked: u_row), keep = the allowed ids"""
    u = np.asarray(u, np.float64)
    M, den = _sum_about_max(u)
    MA, num = _sum_about_max(u[list(keep)])
    if M == NEG or MA == NEG:
        return NEG
    if M == np.inf and MA != np.inf:
        return NEG
    return min(0.0, (0.0 if MA == M else MA - M) + np.log(num) - np.log(den))


def _sum_error(v, K):
    """first-order bound of the relative error of the engine's sum of exp(v - max v)"""
    v = np.asarray(v, np.float64)
    m = v.max()
    fin = v[np.isfinite(v)] if np.isfinite(m) else v[v == m]
    x = (m - fin) if np.isfinite(m) else np.zeros(len(fin))
    e = np.exp(-x)
    return float((e * (3.0 * x + K)).sum() * U + v.size * 2.0 ** -126) / float(e.sum())


def logmass_bound(u, keep):
    """fp32 error bound of phrase_rules_mass_kernel's value for the row (first order; the module docstring derives it).  0 where the value is exact
    by construction: -inf results and rows whose finite entries are all allowed (num and den take the same operations: exactly 0)."""
    u = np.asarray(u, np.float64)
    V = len(u)
    ref = logmass(u, keep)
    if ref == NEG:
        return 0.0
    keep = list(keep)
    rest = np.ones(V, bool)
    rest[keep] = False
    if not np.isfinite(u[rest]).any() and not (u[rest] == np.inf).any():
        return 0.0
    C = -(-V // 2048)
    K = 11 * C + 11
    M, den = _sum_about_max(u)
    MA, num = _sum_about_max(u[keep])
    d = 0.0 if MA == M else abs(MA - M)
    logs = abs(np.log(num)) + abs(np.log(den))
    return _sum_error(u, K) + _sum_error(u[keep], K) + U * (d + 2.0 * logs + abs(np.log(num) - np.log(den)) + abs(ref))


def path_logmass(phrases, row_of, phrase, eot=EOT):
    """phrase_logmass of `phrase` in float64: the sum over the len + 1 nodes of its path, the root first, of the node's logmass;
    row_of(history tuple) -> u [V] behind that history.  -> (sum, [per node])"""
    pre = prefix_dict(phrases)
    per = []
    for i in range(len(phrase) + 1):
        h = tuple(int(t) for t in phrase[:i])
        per.append(logmass(row_of(h), allowed(pre, h, eot)))
    return float(np.sum(per)), per


def log_softmax_at(u, t):
    """plain float64 log-softmax of u at id t (the unconstrained model's log-probability)"""
    u = np.asarray(u, np.float64)
    m = u.max()
    return float(u[t] - (m + np.log(np.exp(u - m).sum())))
