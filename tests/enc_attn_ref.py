"""Inputs, float64 reference, error bound and a numpy model for the encoder self-attention kernels (csrc/enc_kernels.hip:
enc_attn_lazy_kernel<SPLIT>, enc_attn_kernel<SPLIT>), shared by tests/test_gpu_enc_attn_ops.py and tests/test_enc_attn_model_cpu.py.

Scores.  The patterns are built from f16 values whose products are exact: dims 0 and 1 of q and k carry the structure (q = +-4 or 0,
k a multiple of 1/4 ... 1/100), the other dims carry noise (none at all in the threshold pattern, whose scores must be exact).  A
"step of s" means s in the domain of the loop that reads the data: log2 for the lazy loop (its Q carries log2(e) / 8), natural log
for the plain one (its Q carries 1 / 8) - the same f16 values feed both, the reference takes base 2 or e accordingly.

Bound.  With normalised weights p_k, independent relative weight errors eps_k move out_d by at most
    unit_d = sum_k p_k eps_k |v_kd - ref_d|                                              (first order)
    eps_k  = 2^-11 + c 2^-24 65 (sum_j |q_j| |k_kj| + max_k |s_k|),   c = ln 2 (base 2) or 1 (base e)
(2^-11: P rounded to f16; the second term: the worst case of the 64-term fp32 chain plus the C operand / the fma that subtracts
the reference, passed through the exponential), and every written element must obey
    |out - ref| <= factor * unit + 2^-10 |ref|
factor 2 on the GPU (second-order terms, the fp32 sums of l and O over at most 520 keys, v_exp_f32's last bit), 1 for the model
below; 2^-10 |ref| is the project's r for an f16 output."""
import numpy as np

PATTERNS = ["control", "up14", "up17", "up40", "up200", "down12", "threshold", "diverge", "tail",
            "split_up150", "split_down150", "split_mass_hi", "split_mass_lo"]
T_LIST = [64, 65, 129, 200, 256, 257, 321, 520]
SPLIT_MIN_T = 193      # cdiv(T, 64) >= 4: the launcher's precondition for the split-key pair
BIG = 32768.0
F16_R = 2.0 ** -10


def swz(t):
    """V^T position of key t: bits 2 and 3 swapped inside groups of 16 (the P.V MFMA fragment order)"""
    return (t & ~12) | ((t & 4) << 1) | ((t & 8) >> 1)


def vt_image(v16, Tpad, fill=0):
    """v f16 [B][T][H][64] -> V^T image f16 [B][H][64][Tpad]; positions of no key < T hold the 16-bit pattern `fill`"""
    B, T, H, _ = v16.shape
    vt = np.full((B, H, 64, Tpad), fill, np.uint16).view(np.float16)
    vt[:, :, :, swz(np.arange(T))] = v16.transpose(0, 2, 3, 1)
    return vt


def qk_image(q16, k16):
    B, T, H, _ = q16.shape
    return np.ascontiguousarray(np.concatenate([q16.reshape(B, T, H * 64), k16.reshape(B, T, H * 64)], axis=2).reshape(B * T, 2 * H * 64))


def make_inputs(pattern, B, T, H, seed=0):
    """q, k, v f16 [B][T][H][64], different in every (b, h)"""
    rng = np.random.default_rng([seed, PATTERNS.index(pattern), B, T, H])
    t = np.arange(T)
    tile = t // 64
    nt = (T + 63) // 64
    nt_half = (nt + 1) // 2
    qn = 0.35 if pattern == "control" else 0.1
    q = (rng.standard_normal((B, T, H, 64)) * qn).astype(np.float16)
    k = rng.standard_normal((B, T, H, 64)).astype(np.float16)
    v = rng.standard_normal((B, T, H, 64)).astype(np.float16)
    if pattern == "control":
        return q, k, v
    q[..., 0], q[..., 1] = 4.0, 0.0
    k[..., 0], k[..., 1] = 0.0, 0.0
    col = lambda a: np.asarray(a, np.float64)[None, :, None]
    if pattern.startswith("up"):            # every tile beats the previous one by the step
        k[..., 0] = col(float(pattern[2:]) / 4 * tile)
    elif pattern == "down12":               # every tile sits 12 below the previous one: weights run through f16 denormals to exact zeros
        k[..., 0] = col(-3.0 * tile)
    elif pattern == "threshold":
        # exact scores: tile 0 all 0 (reference 0), tile 1 at 9.96 (32 keys per lane x 2^9.96 < 2^15: fast path), tile 2 at exactly 10
        # (32 x 2^10 == 2^15: the raise), later tiles low and varied
        q[..., 1:] = 0.0
        k[...] = 0.0
        k0 = np.where(tile == 1, 2.49, np.where(tile == 2, 2.5, 0.0))
        k[..., 0] = col(k0)
        later = tile >= 3
        k[..., 0] = np.where(col(later), (rng.standard_normal((B, T, H)) * 0.5 - 1.0).astype(np.float16), k[..., 0])
    elif pattern == "diverge":
        # per 128-query tile: query 5 (wave 0) alone needs the raise in key tile 1 (and again, by 45, in the second tile of the upper
        # half); query 37 (wave 1) needs it through keys of the hi = 1 half only ((key % 8) >= 4); every other query sees those keys
        # far BELOW its reference (delta must clamp to 0)
        q[..., 0], q[..., 1] = -4.0, -4.0
        qa, qb = t % 128 == 5, t % 128 == 37
        q[:, qa, :, 0], q[:, qa, :, 1] = 4.0, 0.0
        q[:, qb, :, 0], q[:, qb, :, 1] = 0.0, 4.0
        lvl = np.where(tile == 1, 5.0, np.where((tile == nt_half + 1) & (nt_half + 1 < nt) & (nt_half >= 2), 11.25, 0.0))
        k[..., 0] = col(lvl)
        k[..., 1] = col(np.where(t % 8 >= 4, lvl, 0.0))
    elif pattern == "tail":                 # the row's largest score at key T - 1: the clamped copies of that K row behind it must be masked
        k[:, T - 1, :, 0] = 5.0
    elif pattern in ("split_up150", "split_down150", "split_mass_hi", "split_mass_lo"):
        lvl = 37.5 if "150" in pattern else 150.0      # the halves of a split pair end on references 150 / 600 apart
        upper = pattern in ("split_up150", "split_mass_hi")
        k[..., 0] = col(np.where((tile >= nt_half) == upper, lvl, 0.0))
    else:
        raise ValueError(pattern)
    return q, k, v


def reference(q16, k16, v16, base2):
    """float64 softmax attention of one (b, h) from the f16 values: q, k, v [T][64] -> ref [T][64], unit [T][64]"""
    q, k, v = (np.asarray(a, np.float64) for a in (q16, k16, v16))
    T = q.shape[0]
    s = q @ k.T
    sabs = np.abs(q) @ np.abs(k).T
    c = np.log(2.0) if base2 else 1.0
    eps = 2.0 ** -11 + c * 2.0 ** -24 * 65 * (sabs + np.abs(s).max(1, keepdims=True))
    z = s - s.max(1, keepdims=True)
    p = np.exp2(z) if base2 else np.exp(z)
    p /= p.sum(1, keepdims=True)
    ref = p @ v
    # unit over [q][k][d] in slabs of 64 queries (torch: elementwise work on several threads; numpy takes 2 s per (2, 3, 520) case)
    import torch
    pe_t, v_t, ref_t = torch.from_numpy(p * eps), torch.from_numpy(v), torch.from_numpy(ref)
    unit = torch.empty((T, 64), dtype=torch.float64)
    for q0 in range(0, T, 64):
        unit[q0:q0 + 64] = torch.einsum("qk,qkd->qd", pe_t[q0:q0 + 64], (v_t[None, :, :] - ref_t[q0:q0 + 64, None, :]).abs())
    unit = unit.numpy()
    return ref, unit


def ratios(out, ref, unit):
    """(|out - ref| - r) / unit per element, 0 where the error is inside r"""
    excess = np.maximum(np.abs(np.asarray(out, np.float64) - ref) - F16_R * np.abs(ref), 0.0)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(excess > 0, excess / unit, 0.0)


# ---------------------------------------------------------------------------------------
def _exp2_f32(x):
    """v_exp_f32: fp32 in, fp32 out, denormal results flushed to 0"""
    with np.errstate(over="ignore", under="ignore"):
        y = np.exp2(x.astype(np.float32)).astype(np.float32)
    return np.where(y < np.float32(2.0 ** -126), np.float32(0), y)


def _lazy_state(q16, k16, v16, T, t_beg, t_end):
    """the lazy loop over key tiles [t_beg, t_end) for every wave of 32 queries (rows >= T read row T - 1, as the kernel's do):
    -> m [Tq], l [Tq][2] (one per key half), O [Tq][64], slow [waves][tiles] (True where the wave took the reference step)"""
    f32 = np.float32
    nq = ((T + 31) // 32) * 32
    qi = np.minimum(np.arange(nq), T - 1)
    q, k, v = q16[qi].astype(f32), k16.astype(f32), v16.astype(f32)
    m, l, o = np.zeros(nq, f32), np.zeros((nq, 2), f32), np.zeros((nq, 64), f32)
    slow_log = []
    for kt in range(t_beg, t_end):
        keys = np.arange(kt * 64, kt * 64 + 64)
        kc = np.minimum(keys, T - 1)
        hi = (keys % 8 >= 4).astype(int)
        dead = keys >= T
        first = kt == t_beg

        def scores():
            st = ((q @ k[kc].T).astype(f32) - m[:, None]).astype(f32)
            st[:, dead] = -np.inf
            return st

        def weights(st):
            with np.errstate(over="ignore"):
                p = _exp2_f32(st).astype(np.float16)                     # (beyond 65504: inf, as v_cvt_f16_f32 gives)
            pf = p.astype(f32)
            rs = np.stack([pf[:, hi == 0].sum(1, dtype=f32), pf[:, hi == 1].sum(1, dtype=f32)], axis=1)
            return p, rs

        st = scores()
        p, rs = weights(st)
        lane_slow = ~(rs < f32(BIG))                                     # per lane (query, key half)
        slow = np.repeat(lane_slow.reshape(-1, 64).any(1), 32) | first      # per wave: __any
        if slow.any():
            mx = st.max(1)                                               # both key halves of a query share one reference
            delta = np.where(slow, mx if first else np.maximum(mx, f32(0)), f32(0)).astype(f32)
            alpha = np.where(slow, f32(0) if first else _exp2_f32(-delta), f32(1)).astype(f32)
            m = (m + delta).astype(f32)
            l = (l * alpha[:, None]).astype(f32)
            o = (o * alpha[:, None]).astype(f32)
            p2, rs2 = weights((st - delta[:, None]).astype(f32))
            p = np.where(slow[:, None], p2, p)
            rs = np.where(slow[:, None], rs2, rs)
        l = (l + rs).astype(f32)
        o = (o + p.astype(f32) @ v[kc]).astype(f32)                      # (dead keys: weight exactly 0)
        slow_log.append(slow[::32].copy())
    return m, l, o, np.stack(slow_log, axis=1)


def lazy_model(q16, k16, v16, split):
    """numpy model of enc_attn_lazy_kernel<split> for one (b, h): fp32 arithmetic, f16 P, the kernel's raise rule and merge.
    -> out f16 [T][64], slow [waves][tiles] bool"""
    f32 = np.float32
    T = q16.shape[0]
    nt = (T + 63) // 64
    if not split:
        m, l, o, slow = _lazy_state(q16, k16, v16, T, 0, nt)
    else:
        assert nt >= 4
        nh = (nt + 1) // 2
        m0, l0, o0, s0 = _lazy_state(q16, k16, v16, T, 0, nh)
        m1, l1, o1, s1 = _lazy_state(q16, k16, v16, T, nh, nt)
        mm = np.maximum(m0, m1)
        a0, a1 = _exp2_f32(m0 - mm), _exp2_f32(m1 - mm)
        l = (l0 * a0[:, None]).astype(f32) + (l1 * a1[:, None]).astype(f32)
        o = (o0 * a0[:, None]).astype(f32) + (o1 * a1[:, None]).astype(f32)
        slow = np.concatenate([s0, s1], axis=1)
    inv = (f32(1) / (l[:, 0] + l[:, 1]).astype(f32)).astype(f32)
    return (o * inv[:, None]).astype(f32)[:T].astype(np.float16), slow
