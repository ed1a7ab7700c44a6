"""numpy restatement of the engine's encoder for tests: the int8 rule of include/wis_hip.h (wis_model_ext_t) on the four linears of every layer when
`quant`, the engine's f16 roundings (features, weights, conv1 output, xn, qk / V, ao, hbuf, mem) when `f16`, everything else in `dtype`.
quant=False, f16=False is the oracle's encoder (oracle/whisper_ref.py) in `dtype`."""
import numpy as np
from scipy.special import erf

from wis_hip import weights as W

_gelu = lambda x: x * 0.5 * (1.0 + erf(x / np.sqrt(2.0))).astype(x.dtype)
_norm = lambda c: c / np.sqrt((c ** 2).mean(-1, keepdims=True) + c.dtype.type(1e-5))      # of centred rows


def encode(w, arch, mel, quant=True, dtype=np.float64, f16=True, lazy=True):
    """mel [n_mels][3000] -> encoder output [1500][d].  lazy: the engine's default attention loop (log2(e) folded into the query rows, base-2 softmax)."""
    d, H, L = arch["d_model"], arch["n_heads"], arch.get("n_enc_layers", arch["n_layers"])
    r16 = (lambda x: x.astype(np.float16).astype(dtype)) if f16 else (lambda x: x.astype(dtype))
    get = lambda n: np.asarray(w[n], np.float32)
    ln = lambda x, p: r16(_norm(x - x.mean(-1, keepdims=True)) * get(p + "/gamma").astype(dtype) + get(p + "/beta").astype(dtype))

    def lin(x, p, n_scale=0, qs=np.float32(1)):
        Wm, b = get(p + "/weight").copy(), get(p + "/bias").copy()
        Wm[:n_scale] *= qs; b[:n_scale] *= qs                      # the query scale folded in f32, as the loader does
        if not quant:
            return x @ r16(Wm).T + b.astype(dtype)
        (qa, sa), (qw, sw) = W.quantize_rows(x.astype(np.float16)), W.quantize_rows(Wm.astype(np.float16))
        return (qa.astype(dtype) @ qw.astype(dtype).T) * (sa.astype(dtype)[:, None] * sw.astype(dtype)[None, :]) + b.astype(dtype)

    def conv(x, p, stride):                                          # x [T][C] -> [T / stride][N], kernel 3, padding 1
        Wm = r16(get(p + "/weight"))                                 # [N][C][3]
        xp = np.concatenate([np.zeros((1, x.shape[1]), dtype), x, np.zeros((1, x.shape[1]), dtype)])
        T = x.shape[0] // stride
        cols = np.concatenate([xp[k:k + stride * T:stride] for k in range(3)], axis=1)      # [T][3 C], k-major
        return _gelu(cols @ Wm.transpose(0, 2, 1).reshape(Wm.shape[0], -1).T + get(p + "/bias").astype(dtype))

    x = conv(r16(conv(r16(np.asarray(mel).T), "encoder/conv1", 1)), "encoder/conv2", 2)
    x = x + get("encoder/position_encodings/encodings").astype(dtype)      # (the seeded weight sets carry the table)
    qs = np.float32(0.125) * np.float32(1.4426950408889634) if lazy else np.float32(0.125)
    for l in range(L):
        p = f"encoder/layer_{l}/"
        xn = ln(x, p + "self_attention/layer_norm")
        q, k, v = r16(lin(xn, p + "self_attention/linear_0", d, qs)).reshape(1500, 3, H, 64).transpose(1, 2, 0, 3)      # [H][T][64] each
        s = q @ k.transpose(0, 2, 1)
        s = s - s.max(-1, keepdims=True)
        pr = np.exp2(s) if lazy else np.exp(s)
        ao = r16(((pr / pr.sum(-1, keepdims=True)) @ v).transpose(1, 0, 2).reshape(1500, d))
        x = x + lin(ao, p + "self_attention/linear_1")
        xn = ln(x, p + "ffn/layer_norm")
        x = x + lin(r16(_gelu(lin(xn, p + "ffn/linear_0"))), p + "ffn/linear_1")
    return ln(x, "encoder/layer_norm")
