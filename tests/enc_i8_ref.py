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


def cross_kv_parts(w, arch, mem):
    """What the int8 cross-K/V projection multiplies: the memory rows [T][d] (rounded to f16, as the engine keeps them) through quantize_rows ->
    (qa, sa), and per decoder layer the f16 rows of attention/linear_1 ([K rows | V rows], 2 d of them) through quantize_rows, with the bias ->
    [(qw, sw, bias)]."""
    L = arch.get("n_dec_layers", arch["n_layers"])
    qa, sa = W.quantize_rows(np.asarray(mem).astype(np.float16))
    layers = []
    for l in range(L):
        p = f"decoder/layer_{l}/attention/linear_1/"
        layers.append((*W.quantize_rows(np.asarray(w[p + "weight"], np.float32).astype(np.float16)), np.asarray(w[p + "bias"], np.float32)))
    return qa, sa, layers


def cross_kv_from(qa, sa, layers, dtype=np.float64, f16=True):
    """[(K, V)] per layer, [T][d] each: the exact integer product, times sa[m] sw[n], plus the bias, in `dtype`; then rounded to f16 (the engine's K / V
    images are f16) when `f16`."""
    d, out = qa.shape[1], []
    for qw, sw, b in layers:
        acc = qa.astype(np.float64) @ qw.astype(np.float64).T      # (exact: |acc| <= 127^2 d < 2^53)
        kv = acc.astype(dtype) * (sa.astype(dtype)[:, None] * sw.astype(dtype)[None, :]) + b.astype(dtype)
        kv = kv.astype(np.float16).astype(dtype) if f16 else kv
        out.append((kv[:, :d], kv[:, d:]))
    return out


def cross_kv(w, arch, mem, quant=True, dtype=np.float64, f16=True):
    """Encoder memory [T][d] -> per decoder layer (K, V), [T][d] each, as run_cross_kv leaves them: by the int8 rule when `quant` (cross_kv_parts,
    cross_kv_from), else the f16 memory times the f16 weight rows plus the bias in `dtype`; rounded to f16 when `f16`.
    quant=False, f16=False is the oracle's cross_kv (oracle/whisper_ref.py) in `dtype`."""
    if quant:
        return cross_kv_from(*cross_kv_parts(w, arch, mem), dtype=dtype, f16=f16)
    r16 = (lambda x: np.asarray(x).astype(np.float16).astype(dtype)) if f16 else (lambda x: np.asarray(x).astype(dtype))
    d, out, m = arch["d_model"], [], r16(mem)
    for l in range(arch.get("n_dec_layers", arch["n_layers"])):
        p = f"decoder/layer_{l}/attention/linear_1/"
        kv = r16(m @ r16(np.asarray(w[p + "weight"], np.float32)).T + np.asarray(w[p + "bias"], np.float32).astype(dtype))
        out.append((kv[:, :d], kv[:, d:]))
    return out


def decoder_logits(w, arch, ckv, tokens, dtype=np.float64):
    """Teacher-forced logits [T][n_vocab] behind `tokens` for ONE utterance whose cross K / V are `ckv` (cross_kv's result): the oracle's decoder_step
    (oracle/whisper_ref.py), one position at a time, on tensors of `dtype`."""
    import torch
    from oracle.whisper_ref import WhisperRef
    td = torch.float64 if dtype == np.float64 else torch.float32
    ref = WhisperRef(w, arch["d_model"], arch.get("n_dec_layers", arch["n_layers"]), arch["n_heads"], n_vocab=arch["n_vocab"])
    ref.w = {k: v.to(td) for k, v in ref.w.items() if k.startswith("decoder/")}
    tck = [(torch.from_numpy(np.ascontiguousarray(k, dtype))[None], torch.from_numpy(np.ascontiguousarray(v, dtype))[None]) for k, v in ckv]
    cache, rows = [None] * ref.L, []
    for t, tok in enumerate(tokens):
        rows.append(ref.decoder_step(np.asarray([[tok]]), t, cache, tck)[0].numpy())
    return np.stack(rows)


def scale_family(M, K, seed):
    """f16 rows [M][K] for the row quantiser, every row with a scale of its own: absmax one of f16's normal values, drawn without repetition and uniformly
    over their bit patterns (log-uniform from 2^-14 to 65504), at a random column; half of the other entries at the f16 value nearest (k + 0.5) * scale, k uniform in [0, 126], random sign - the rounding boundaries, where
    rint(r * inv) and rint(r / scale), or an inv one ulp off, part ways - the rest uniform in +- absmax."""
    rng = np.random.default_rng(seed)
    mx = rng.choice(np.arange(0x0400, 0x7C00), M, replace=False).astype(np.uint16).view(np.float16).astype(np.float32)
    scale = (mx / np.float32(127.0)).astype(np.float32)
    rows = (rng.uniform(-1, 1, (M, K)) * mx[:, None]).astype(np.float32)
    ties = (rng.integers(0, 127, (M, K)).astype(np.float32) + np.float32(0.5)) * scale[:, None] * rng.choice(np.float32([-1, 1]), (M, K))
    rows = np.where(rng.permuted(np.tile(np.arange(K) % 2 == 0, (M, 1)), axis=1), ties, rows).astype(np.float16)
    rows[np.arange(M), rng.integers(0, K, M)] = mx * rng.choice(np.float32([-1, 1]), M)
    assert (np.abs(rows.astype(np.float32)).max(1) == mx).all()
    return rows


def ln_scale_family(M, d, seed):
    """f32 rows [M][d], gamma, beta for LayerNorm + quantise, the scales spread as far as a LayerNorm lets them: it fixes a row's variance, so the
    absmax of its output lies between about 2.5 (the largest of d normal values) and sqrt(d - 1) gamma (one outlier).  One entry of every row is
    raised by a factor log-uniform over that range; the rows then get a gain and an offset of their own, which the LayerNorm takes out again.
    With d = 256 the absmax covers three binades of f16 - some 3000 values, so 4096 rows have about 1900 different scales (the unfused quantiser,
    which can be handed any row, gets f16's whole range: scale_family)."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((M, d)).astype(np.float32)
    x[np.arange(M), rng.integers(0, d, M)] = np.exp(rng.uniform(np.log(2.0), np.log(200.0), M)) * rng.choice([-1.0, 1.0], M)
    x = (x * np.exp(rng.uniform(-3, 3, (M, 1))) + rng.standard_normal((M, 1))).astype(np.float32)
    return x, (1 + 0.1 * rng.standard_normal(d)).astype(np.float32), (0.1 * rng.standard_normal(d)).astype(np.float32)
