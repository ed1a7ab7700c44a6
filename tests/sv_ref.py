"""Test helper (not product code): the speaker-verification kernels of csrc/sv.hip restated in float64 numpy, from the definitions of
Hugging Face WavLMForXVector (transformers/models/wavlm/modeling_wavlm.py), plus the `sharpened` model and the ablations that the
whole-model tests need.

Each function takes the operands as the kernel reads them (already rounded to f16 where the kernel holds them in f16) and computes in
float64, so a test can keep its tolerance near the kernel's own rounding.  Layouts follow include/wis_hip.h."""
import contextlib

import numpy as np
import torch
from scipy.special import erf

C0, D, H, DH, PK, PG = 512, 768, 12, 64, 128, 16


def gelu(x):
    """erf GELU (HF ACT2FN["gelu"])"""
    return 0.5 * x * (1.0 + erf(x / np.sqrt(2.0)))


def f16(x):
    """x rounded to f16, returned as float64"""
    return np.asarray(x).astype(np.float16).astype(np.float64)


def conv0_groupnorm_gelu(pcm, w0, gamma, beta, eps=1e-5):
    """WavLMGroupNormConvLayer 0: Conv1d(1, 512, 10, stride 5, no bias), GroupNorm(512 groups) over time, GELU.
    pcm [n], w0 [512][10] -> [T0][512]"""
    x = np.asarray(pcm, np.float64)
    T0 = (x.size - 10) // 5 + 1
    idx = 5 * np.arange(T0)[:, None] + np.arange(10)[None, :]
    y = x[idx] @ np.asarray(w0, np.float64).T                   # [T0][512]
    mean = y.mean(axis=0)
    var = ((y - mean) ** 2).mean(axis=0)
    return gelu((y - mean) / np.sqrt(var + eps) * np.asarray(gamma, np.float64) + np.asarray(beta, np.float64))


def posconv(x, W, bias):
    """WavLMPositionalConvEmbedding + the encoder's residual: x + GELU(conv1d(x, padding 64, groups 16)[:, :, :-1] + bias)
    (WavLMSamePadLayer drops the last output).  x [T][768] (the kernel reads it as f16), W [768][128][48] ([out][k][in / groups]),
    bias [768] -> [T][768]"""
    x = np.asarray(x, np.float64)
    xt = torch.from_numpy(f16(x).T[None].copy())                                            # [1][768][T]
    wt = torch.from_numpy(np.asarray(W, np.float64).transpose(0, 2, 1).copy())             # [768][48][128]
    c = torch.nn.functional.conv1d(xt, wt, torch.from_numpy(np.asarray(bias, np.float64)), padding=PK // 2, groups=PG)
    c = c[0, :, :-1].numpy().T
    return x + gelu(c)


def gate(xin, gw, gb, gconst):
    """the gated relative-position gate of every (head, query): HF WavLMAttention.forward steps 1-3.
    xin [T][768] (layer input), gw [8][64], gb [8], gconst [12] -> [12][T]"""
    xh = np.asarray(xin, np.float64).reshape(-1, H, DH).transpose(1, 0, 2)                # [H][T][64]
    proj = xh @ np.asarray(gw, np.float64).T + np.asarray(gb, np.float64)                 # [H][T][8]
    s = proj.reshape(H, -1, 2, 4).sum(-1)
    sg = 1.0 / (1.0 + np.exp(-s))
    ga, gbv = sg[..., 0], sg[..., 1]
    return ga * (gbv * np.asarray(gconst, np.float64)[:, None] - 1.0) + 2.0


def attention(qkv, xin, gw, gb, gconst, tab, L):
    """softmax(Q K^T + gate[h][q] tab[h][key - q + L - 1]) V per head.  qkv [T][2304] (Q already scaled by 1/8), tab [12][2L - 1]
    -> [T][768]"""
    qkv = np.asarray(qkv, np.float64)
    T = qkv.shape[0]
    g = gate(xin, gw, gb, gconst)
    rel = np.arange(T)[None, :] - np.arange(T)[:, None] + L - 1                           # [q][key]: key - q + L - 1
    tab = np.asarray(tab, np.float64)
    out = np.zeros((T, D))
    for h in range(H):
        q, k, v = (qkv[:, j * D + h * DH: j * D + (h + 1) * DH] for j in range(3))
        s = q @ k.T + g[h][:, None] * tab[h][rel]
        s -= s.max(axis=1, keepdims=True)
        p = np.exp(s)
        out[:, h * DH:(h + 1) * DH] = (p / p.sum(axis=1, keepdims=True)) @ v
    return out


def layernorm(x, g, b, eps=1e-5):
    x = np.asarray(x, np.float64)
    m = x.mean(axis=-1, keepdims=True)
    v = ((x - m) ** 2).mean(axis=-1, keepdims=True)
    return (x - m) / np.sqrt(v + eps) * np.asarray(g, np.float64) + np.asarray(b, np.float64)


def xvector_tail(z, T, n, W_fe, b_fe):
    """statistics pooling of ReLU(z[:T, :n]) (mean, unbiased std: torch .std) and the Linear 2n -> 512 -> (stats [2n], emb [512])"""
    r = np.maximum(np.asarray(z, np.float64)[:T, :n], 0.0)
    stats = np.concatenate([r.mean(axis=0), r.std(axis=0, ddof=1)])
    return stats, np.asarray(W_fe, np.float64) @ stats + np.asarray(b_fe, np.float64)


# ---- whole-model helpers (HF modules) -----------------------------------------------------------------------------------------
def sharpen(hf, seed=0):
    """Make the features that set WavLM apart from a plain transformer matter (in place, returns hf): the relative-position bias
    table x 100, gate projections N(0, 0.4) with N(0, 1) biases, gru_rel_pos_const = linspace(0.3, 3, 12) per head, and q_proj /
    k_proj x 3.  At HF's default init the bias is ~0.04 logits and the gate ~1.75 everywhere, so a kernel could drop either unseen."""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        layers = hf.wavlm.encoder.layers
        layers[0].attention.rel_attn_embed.weight.mul_(100.0)
        for lyr in layers:
            a = lyr.attention
            w = a.gru_rel_pos_linear
            w.weight.copy_(torch.randn(w.weight.shape, generator=g, dtype=torch.float32).to(w.weight.dtype) * 0.4)
            w.bias.copy_(torch.randn(w.bias.shape, generator=g, dtype=torch.float32).to(w.bias.dtype))
            a.gru_rel_pos_const.copy_(torch.linspace(0.3, 3.0, H).view(1, H, 1, 1))
            for p in (a.q_proj, a.k_proj):
                p.weight.mul_(3.0)
                p.bias.mul_(3.0)
    return hf


# what tests/test_gpu_sv.py holds the engine to on the sharpened model (rel-L2 of every hidden state against HF float64); the power
# check in tests/test_sv_cpu.py asks every ablation below to move some hidden state by 10x this
SHARP_HIDDEN_LIMIT = 5e-3

ABLATIONS = ("no_bias", "mirrored_bias", "gate_frozen", "gate_swapped", "gconst_one")


@contextlib.contextmanager
def ablated(hf, kind):
    """A wrong variant of the attention, applied to the HF model in place for the duration:
    no_bias: no relative-position bias; mirrored_bias: the table read at query - key; gate_frozen: the gate projection's weights
    zeroed (one gate per head, whatever the input); gate_swapped: gate_a and gate_b exchanged; gconst_one: gru_rel_pos_const = 1."""
    layers = hf.wavlm.encoder.layers
    a0 = layers[0].attention
    saved = {}
    with torch.no_grad():
        if kind == "no_bias":
            saved["e"] = a0.rel_attn_embed.weight.clone()
            a0.rel_attn_embed.weight.zero_()
        elif kind == "mirrored_bias":
            orig = a0.compute_bias
            a0.compute_bias = lambda ql, kl: orig(ql, kl).transpose(-1, -2)
        elif kind in ("gate_frozen", "gate_swapped"):
            for i, lyr in enumerate(layers):
                w = lyr.attention.gru_rel_pos_linear
                saved[i] = (w.weight.clone(), w.bias.clone())
                if kind == "gate_frozen":
                    w.weight.zero_()
                else:
                    w.weight.copy_(torch.cat([saved[i][0][4:], saved[i][0][:4]]))
                    w.bias.copy_(torch.cat([saved[i][1][4:], saved[i][1][:4]]))
        elif kind == "gconst_one":
            for i, lyr in enumerate(layers):
                saved[i] = lyr.attention.gru_rel_pos_const.clone()
                lyr.attention.gru_rel_pos_const.fill_(1.0)
        else:
            raise ValueError(kind)
    try:
        yield hf
    finally:
        with torch.no_grad():
            if kind == "no_bias":
                a0.rel_attn_embed.weight.copy_(saved["e"])
            elif kind == "mirrored_bias":
                del a0.compute_bias
            elif kind in ("gate_frozen", "gate_swapped"):
                for i, lyr in enumerate(layers):
                    lyr.attention.gru_rel_pos_linear.weight.copy_(saved[i][0])
                    lyr.attention.gru_rel_pos_linear.bias.copy_(saved[i][1])
            else:
                for i, lyr in enumerate(layers):
                    lyr.attention.gru_rel_pos_const.copy_(saved[i])


def hf_forward(hf, x):
    """HF WavLMForXVector in its own dtype -> (feature-encoder output [T][512], hidden states [13][T][768], TDNN output [T - 14][1500],
    embedding [512]), all float64 numpy"""
    taps = {}
    hooks = [hf.wavlm.feature_extractor.register_forward_hook(lambda m, i, o: taps.__setitem__("f", o[0].T)),
             hf.tdnn[-1].register_forward_hook(lambda m, i, o: taps.__setitem__("t", o[0]))]
    dt = next(hf.parameters()).dtype
    try:
        with torch.inference_mode():
            r = hf(torch.from_numpy(np.ascontiguousarray(x)).to(dt)[None], output_hidden_states=True)
    finally:
        for h in hooks:
            h.remove()
    f = lambda t: t.detach().double().numpy()
    return f(taps["f"]), [f(s[0]) for s in r.hidden_states], f(taps["t"]), f(r.embeddings[0])


def rel_l2(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / (np.linalg.norm(b) + 1e-300))


def worst_row(a, b):
    """max over rows of the row's rel-L2 error (one bad row cannot hide inside the whole tensor's norm)"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float((np.linalg.norm(a - b, axis=-1) / (np.linalg.norm(b, axis=-1) + 1e-300)).max())
