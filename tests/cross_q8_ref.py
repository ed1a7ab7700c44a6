"""Layouts and the float64 reference of the int8 cross K/V (csrc/cross_q8.hip; include/wis_hip.h cross_kv_bits), for tests/test_gpu_cross_q8.py.
Bound: dec_attn_ref.reference on the values the kernel reads, K = Kq sk and V = Vq sv (exact in float64).  The int8 kernel adds two f32 multiplications:
score = (MFMA result) * sk[t] rounds once, 2^-24 |s_k| on the exponential's argument = relative on weight k, and so did the chunk maximum it is taken
about (not common to the weights of other chunks; bounded by |s_k| for the peak key, which is both): 2^-24 * 2 |s_k|.  p * sv[t] rounds once before P
becomes f16: 2^-24.  The issue states the sum as 2^-24 (2 |s_k| + 2); the second unit is slack, no rounding stands behind it.  `unit` grows by
sum_k p_k 2^-24 (2 |s_k| + 2) |v_kd - ref_d|."""
import numpy as np

import dec_attn_ref as D


def images(K16, V16, Tpad):
    """f16 K, V [B][T][d] -> the engine's four images (include/wis_hip.h cross_kv_bits): quantize_rows on every 64-value head row, then pack"""
    from wis_hip.weights import quantize_rows
    B, T, d = K16.shape
    (kq, sk), (vq, sv) = (quantize_rows(np.asarray(x).reshape(-1, 64)) for x in (K16, V16))
    return pack(kq.reshape(B, T, d), sk.reshape(B, T, -1).transpose(0, 2, 1), vq.reshape(B, T, d), sv.reshape(B, T, -1).transpose(0, 2, 1), Tpad)


def pack(Kq, sk, Vq, sv, Tpad):      # int8 [B][T][d], scales [B][H][T] -> the four images; keys [T, Tpad) zeros and scale 1
    B, T, d = Kq.shape
    k, v = np.zeros((B, Tpad, d // 64, 2, 4, 8), np.int8), np.zeros((B, Tpad, d // 64, 64), np.int8)
    k[:, :T], v[:, :T] = Kq.reshape(B, T, d // 64, 2, 4, 8), Vq.reshape(B, T, d // 64, 64)      # dh = 32 e + 8 j + i
    v = v.reshape(B, Tpad // 64, 2, 4, 8, d // 64, 64)                                          # t = 64 g + 32 e + 8 j + i
    out = [k.transpose(0, 2, 4, 1, 3, 5).reshape(B, d // 64, 4, Tpad, 16), v.transpose(0, 5, 6, 1, 3, 2, 4).reshape(B, d // 64, 64, Tpad)]
    for s in (sk, sv):
        out.append(np.ones((B, d // 64, Tpad), np.float32))
        out[-1][..., :T] = s
    return [np.ascontiguousarray(a) for a in out]


def reference(q, Kq, sk, Vq, sv):
    """one (utterance, head): q [R][64], Kq / Vq int8 [T][64], sk / sv [T] -> (ref, unit) in float64, 256-key chunks"""
    k, v = Kq.astype(np.float64) * sk[:, None], Vq.astype(np.float64) * sv[:, None]
    ref, unit = D.reference(q, k, v, D.n_acc_cross(k.shape[0], 256), chunk=256)
    s = np.asarray(q, np.float64) @ k.T
    p = np.exp(s - s.max(1, keepdims=True))
    return ref, unit + np.einsum("rk,rkd->rd", p / p.sum(1, keepdims=True) * D.U24 * (2 * np.abs(s) + 2), np.abs(v[None] - ref[:, None]))
