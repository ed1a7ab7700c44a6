"""Speaker verification (`/api/willow?voice_auth=true`): the reference's WavLM-base-plus-sv x-vector embedder on the HIP path.

Reference: main.py:306-316 (model load), 797-879 (`do_sv`).  The embedding runs in libwis_hip.so (csrc/sv.hip, `wis_sv_*`); this
module loads the checkpoint, applies the reference's preprocessing on the host, and scores against the enrolled speakers.

    python -m wis_hip.sv enroll NAME AUDIO [--dir speakers/voice_auth] [--model PATH]   # writes NAME.npy

Checkpoints: a Hugging Face directory (config.json, preprocessor_config.json, model.safetensors or pytorch_model.bin), or
"synthetic:wavlm-base-plus-sv[:SEED]" - seeded random weights at the true architecture (tests, benchmarks; needs `transformers`).
"""
import ctypes as C
import json
import os
import re
import threading

import numpy as np

from . import _lib

SAMPLE_RATE = 16000
MAX_SECONDS = 10                    # sox "trim 0 10" (main.py:814)
NORM_DB = 8.0                       # sox "norm 8" (main.py:813)
SYNTHETIC = "synthetic:wavlm-base-plus-sv"

# WavLMConfig(use_weighted_layer_sum=True, conv_bias=False, feat_extract_norm="group", do_stable_layer_norm=False): the architecture
# csrc/sv.hip serves (wis_sv_create refuses any other)
ARCH = dict(conv_dim=[512] * 7, conv_kernel=[10, 3, 3, 3, 3, 2, 2], conv_stride=[5, 2, 2, 2, 2, 2, 2], hidden_size=768,
            num_attention_heads=12, num_hidden_layers=12, intermediate_size=3072, num_conv_pos_embeddings=128,
            num_conv_pos_embedding_groups=16, num_buckets=320, max_bucket_distance=800, tdnn_dim=[512, 512, 512, 512, 1500],
            tdnn_kernel=[5, 3, 3, 1, 1], tdnn_dilation=[1, 2, 3, 1, 1], xvector_output_dim=512)
POS_G = "wavlm.encoder.pos_conv_embed.conv.weight_g"
POS_V = "wavlm.encoder.pos_conv_embed.conv.weight_v"
POS_G2 = "wavlm.encoder.pos_conv_embed.conv.parametrizations.weight.original0"
POS_V2 = "wavlm.encoder.pos_conv_embed.conv.parametrizations.weight.original1"
POS_W = "wavlm.encoder.pos_conv_embed.conv.weight"


# ---- preprocessing (host) ------------------------------------------------------------------------------------------------------
def sox_norm_gain(pcm, db=NORM_DB):
    """sox `norm 8`: one gain for the whole signal that brings its peak to +8 dBFS, i.e. x * 10^(8/20) / max|x|, then clipped to
    [-1, 1] (sox clips what leaves the effects chain).  A silent signal is returned unchanged."""
    x = np.asarray(pcm, dtype=np.float32)
    peak = float(np.max(np.abs(x))) if x.size else 0.0
    if peak <= 0.0:
        return x.copy()
    gain = np.float32(10.0 ** (db / 20.0) / peak)
    return np.clip(x * gain, -1.0, 1.0).astype(np.float32)


def trim(pcm, seconds=MAX_SECONDS, sr=SAMPLE_RATE):
    """sox `trim 0 10`: the first 10 s."""
    return np.asarray(pcm, dtype=np.float32)[: int(seconds * sr)]


def zero_mean_unit_var(x):
    """Wav2Vec2FeatureExtractor do_normalize: (x - mean) / sqrt(var + 1e-7)"""
    x = np.asarray(x, dtype=np.float32)
    return ((x - x.mean()) / np.sqrt(x.var() + 1e-7)).astype(np.float32)


def preprocess(pcm, do_normalize=True):
    """The reference's chain (main.py:812-827): sox norm 8, trim 0 10, then the feature extractor."""
    x = trim(sox_norm_gain(pcm))
    return zero_mean_unit_var(x) if do_normalize else x


# ---- checkpoint -> engine tensors ---------------------------------------------------------------------------------------------
def fold_weight_norm(g, v):
    """torch weight_norm(dim=2): W = g * v / ||v||, the norm over every axis but 2 (one per kernel tap)."""
    v = np.asarray(v, dtype=np.float32)
    n = np.sqrt((v.astype(np.float64) ** 2).sum(axis=(0, 1), keepdims=True)).astype(np.float32)
    return (np.asarray(g, dtype=np.float32).reshape(1, 1, -1) * v / n).astype(np.float32)


def conv_weight_kin(w):
    """Conv1d weight [out][in][k] -> [out][k][in]: the row of the channels-last GEMM's implicit im2col (x[t + j][c] at j * in + c)."""
    return np.ascontiguousarray(np.asarray(w, dtype=np.float32).transpose(0, 2, 1))


def engine_tensors(sd):
    """HF state dict (numpy) -> {name: array} in the layouts wis_sv_create expects (include/wis_hip.h): conv weights [out][k][in],
    the positional conv's weight norm folded.  Heads the embedding does not use (classifier, objective, masked_spec_embed) are left out."""
    out = {}
    for k, v in sd.items():
        if k.startswith(("classifier.", "objective.")) or k == "wavlm.masked_spec_embed" or k in (POS_G, POS_V, POS_G2, POS_V2):
            continue
        v = np.asarray(v, dtype=np.float32)
        if re.fullmatch(r"wavlm\.feature_extractor\.conv_layers\.\d+\.conv\.weight", k):
            v = conv_weight_kin(v)
        out[k] = v
    if POS_W not in sd:
        if POS_G in sd:
            g, v = sd[POS_G], sd[POS_V]
        elif POS_G2 in sd:
            g, v = sd[POS_G2], sd[POS_V2]
        else:
            raise ValueError("positional conv weight missing (weight_g / weight_v or parametrizations.weight.original0 / 1)")
        w = fold_weight_norm(g, v)
    else:
        w = np.asarray(sd[POS_W], dtype=np.float32)
    out[POS_W] = conv_weight_kin(w)           # [768][48][128] -> [768][128][48]
    return out


def check_arch(cfg):
    bad = [k for k, v in ARCH.items() if k in cfg and (list(cfg[k]) if isinstance(v, list) else cfg[k]) != v]
    if not cfg.get("use_weighted_layer_sum", True) or cfg.get("do_stable_layer_norm", False) or cfg.get("feat_extract_norm", "group") != "group" \
            or cfg.get("conv_bias", False):
        bad.append("layer-sum / layer-norm / conv-bias flavour")
    if bad:
        raise ValueError(f"unsupported WavLM x-vector architecture: {bad}")


def load_state_dict(path):
    """HF checkpoint directory -> (config dict, state dict of numpy arrays, preprocessor config dict)"""
    with open(os.path.join(path, "config.json")) as f:
        cfg = json.load(f)
    pre = {}
    pp = os.path.join(path, "preprocessor_config.json")
    if os.path.exists(pp):
        with open(pp) as f:
            pre = json.load(f)
    st = os.path.join(path, "model.safetensors")
    if os.path.exists(st):
        from safetensors.numpy import load_file
        sd = load_file(st)
    else:
        import torch
        sd = {k: v.float().numpy() for k, v in torch.load(os.path.join(path, "pytorch_model.bin"), map_location="cpu", weights_only=True).items()}
    return cfg, sd, pre


def hf_config(**over):
    from transformers import WavLMConfig
    kw = dict(use_weighted_layer_sum=True, conv_bias=False, feat_extract_norm="group", do_stable_layer_norm=False)
    kw.update(over)
    return WavLMConfig(**kw)


def synthetic_model(seed=0):
    """A seeded HF WavLMForXVector at the true architecture (eval mode, fp32)."""
    import torch
    from transformers import WavLMForXVector
    torch.manual_seed(seed)
    return WavLMForXVector(hf_config()).eval()


def resolve(path):
    """model path or synthetic spec -> (config dict, state dict, preprocessor config)"""
    if path.startswith(SYNTHETIC):
        seed = int(path.split(":")[2]) if path.count(":") >= 2 else 0
        m = synthetic_model(seed)
        return m.config.to_dict(), {k: v.detach().numpy() for k, v in m.state_dict().items()}, {"do_normalize": True}
    if not os.path.isdir(path):
        raise FileNotFoundError(f"speaker-verification model directory {path!r} not found")
    return load_state_dict(path)


def build_arena(tensors):
    """{name: f32 array} -> (arena bytes, ctypes Tensor array, keep-alive)"""
    names, offs, off = [], [], 0
    for k, v in tensors.items():
        off = (off + 255) & ~255
        names.append(k)
        offs.append(off)
        off += v.size * 4
    arena = np.zeros(max(off, 16) // 4 + 1, dtype=np.float32)
    tv = (_lib.Tensor * len(names))()
    keep = []
    for i, (k, o) in enumerate(zip(names, offs)):
        v = np.ascontiguousarray(tensors[k], dtype=np.float32)
        arena[o // 4: o // 4 + v.size] = v.ravel()
        nb = k.encode()
        keep.append(nb)
        tv[i].name = nb
        tv[i].dtype = _lib.WIS_DT_F32
        shp = list(v.shape)[:4] if v.ndim <= 4 else [v.size]
        tv[i].rank = len(shp)
        for j, s in enumerate(shp):
            tv[i].shape[j] = s
        tv[i].offset = o
    return arena, tv, keep


def sv_config(max_samples=MAX_SECONDS * SAMPLE_RATE, cfg=None):
    a = dict(ARCH)
    for k in ARCH:
        if cfg and k in cfg:
            a[k] = list(cfg[k]) if isinstance(cfg[k], (list, tuple)) else cfg[k]
    c = _lib.SvConfig()
    c.conv_dim, c.n_conv_layers = a["conv_dim"][0], len(a["conv_dim"])
    for i, (k, s) in enumerate(zip(a["conv_kernel"], a["conv_stride"])):
        c.conv_kernel[i], c.conv_stride[i] = k, s
    c.hidden_size, c.n_heads, c.n_layers, c.intermediate_size = a["hidden_size"], a["num_attention_heads"], a["num_hidden_layers"], a["intermediate_size"]
    c.num_conv_pos_embeddings, c.num_conv_pos_embedding_groups = a["num_conv_pos_embeddings"], a["num_conv_pos_embedding_groups"]
    c.num_buckets, c.max_bucket_distance = a["num_buckets"], a["max_bucket_distance"]
    c.n_tdnn = len(a["tdnn_dim"])
    for i in range(c.n_tdnn):
        c.tdnn_dim[i], c.tdnn_kernel[i], c.tdnn_dilation[i] = a["tdnn_dim"][i], a["tdnn_kernel"][i], a["tdnn_dilation"][i]
    c.xvector_output_dim = a["xvector_output_dim"]
    c.max_samples = max_samples
    return c


def frames(n):
    """frames after the feature encoder for n samples (0: too short for a stage), as the engine counts them"""
    t = int(n)
    for k, s in zip(ARCH["conv_kernel"], ARCH["conv_stride"]):
        if t < k:
            return 0
        t = (t - k) // s + 1
    return t


def rel_buckets(first, n, num_buckets=320, max_distance=800):
    """the engine's relative-position bucket table (host function of libwis_hip.so, no GPU needed)"""
    out = np.zeros(n, dtype=np.int32)
    _lib.check(_lib.load().wis_sv_rel_buckets(num_buckets, max_distance, first, n, out.ctypes.data_as(C.POINTER(C.c_int32))))
    return out


class SpeakerVerifier:
    """One wis_sv handle (one GPU); calls are serialised by a lock (the handle runs one forward pass at a time)."""

    def __init__(self, path=SYNTHETIC, device=0, max_samples=MAX_SECONDS * SAMPLE_RATE, state=None):
        cfg, sd, pre = state if state is not None else resolve(path)
        check_arch(cfg)
        self.do_normalize = bool(pre.get("do_normalize", True))
        self.max_samples = int(max_samples)
        self.device = int(device)
        lib = _lib.load()
        _lib.require_gpu()
        arena, tv, keep = build_arena(engine_tensors(sd))
        h = C.c_void_p()
        _lib.check(lib.wis_sv_create(C.byref(sv_config(self.max_samples, cfg)), _lib.ptr(arena), arena.nbytes, 0, tv, len(tv), device, C.byref(h)))
        del keep
        self._h, self._lock = h, threading.Lock()

    @property
    def device_bytes(self):
        return _lib.load().wis_sv_device_bytes(self._h)

    def embed_input(self, x):
        """model input (already preprocessed) -> embedding [512] f32 (WavLMForXVector(...).embeddings)"""
        x = np.ascontiguousarray(x, dtype=np.float32)
        out = np.zeros(512, dtype=np.float32)
        with self._lock:
            _lib.check(_lib.load().wis_sv_embed(self._h, _lib.ptr(x), x.size, out.ctypes.data_as(C.POINTER(C.c_float))))
        return out

    def embed(self, pcm):
        """16 kHz mono PCM -> embedding, through the reference's preprocessing"""
        return self.embed_input(preprocess(pcm, self.do_normalize))

    def taps(self, x, tap, layer=0):
        x = np.ascontiguousarray(x, dtype=np.float32)
        cap = max(512 * 1536, frames(x.size) * 1536)   # the widest tap: [T - 14][1500]
        out = np.zeros(cap, dtype=np.float32)
        r, c = C.c_int32(), C.c_int32()
        with self._lock:
            _lib.check(_lib.load().wis_debug_sv_taps(self._h, _lib.ptr(x), x.size, tap, layer, out.ctypes.data_as(C.POINTER(C.c_float)), cap,
                                                     C.byref(r), C.byref(c)))
        return out[: r.value * c.value].reshape(r.value, c.value).copy()

    def close(self):
        if getattr(self, "_h", None):
            _lib.load().wis_sv_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# ---- scoring (host, as in the reference) ----------------------------------------------------------------------------------------
def load_speakers(speakers_dir):
    """{name: embedding} of every NAME.npy in the directory (stored as written, not re-normalised: cosine does not care)"""
    out = {}
    if not os.path.isdir(speakers_dir):
        return out
    for f in sorted(os.listdir(speakers_dir)):
        if f.endswith(".npy"):
            out[re.sub(r"(.npy)$", "", f)] = np.load(os.path.join(speakers_dir, f)).astype(np.float32).reshape(-1)
    return out


def cosine(a, b, eps=1e-8):
    """torch.nn.CosineSimilarity(dim=-1)"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.dot(a, b) / max(np.linalg.norm(a) * np.linalg.norm(b), eps))


def score(emb, speakers, threshold):
    """{name: "0.912"} of the speakers at or above the threshold, highest first (main.py:851-862)"""
    res = {}
    for name, e in speakers.items():
        sim = cosine(e, emb)
        if sim >= threshold:
            res[name] = "{:.3f}".format(sim)
    return dict(sorted(res.items(), key=lambda kv: kv[1], reverse=True))


def _resample_device(verifier, resample_on_gpu):
    """the GPU that resamples a recording for `verifier`: the verifier's own (None = on the host); resample_on_gpu None = the settings' value"""
    if resample_on_gpu is None:
        from .settings import get_api_settings
        resample_on_gpu = getattr(get_api_settings(), "resample_on_gpu", False)
    return getattr(verifier, "device", None) if resample_on_gpu else None


def do_sv(audio_file, threshold, verifier, speakers_dir="speakers/voice_auth", resample_on_gpu=None):
    """main.py:797-879: embed the request, compare with every enrolled speaker.  Audio too short for the model scores nothing
    (the reference's NaN similarity), so the request ends as unauthorised.  A recording at another rate than 16 kHz is resampled
    on the verifier's GPU (resample_on_gpu; None: the settings' value)."""
    from . import audio
    try:
        pcm, _ = audio.load_audio(audio_file, device=_resample_device(verifier, resample_on_gpu))
    except Exception as e:
        raise ValueError(f"invalid audio: {e}") from e
    try:
        emb = verifier.embed(pcm)
    except _lib.WisError as e:
        if e.code == -1:        # WIS_E_ARG: too short
            return {}
        raise
    emb = emb / max(float(np.linalg.norm(emb)), 1e-12)
    return score(emb, load_speakers(speakers_dir), threshold)


def enroll(name, audio_file, speakers_dir="speakers/voice_auth", verifier=None, model_path=None, resample_on_gpu=None):
    """Write speakers_dir/NAME.npy: the L2-normalised embedding of the recording (what do_sv compares requests with)."""
    from . import audio
    if not re.fullmatch(r"[A-Za-z0-9_.\- ]+", name) or name.startswith("."):
        raise ValueError(f"invalid speaker name {name!r}")
    v = verifier or SpeakerVerifier(model_path or os.environ.get("SV_MODEL_PATH", "./models/microsoft-wavlm-base-plus-sv"))
    pcm, _ = audio.load_audio(audio_file, device=_resample_device(v, resample_on_gpu))
    emb = v.embed(pcm)
    emb = (emb / max(float(np.linalg.norm(emb)), 1e-12)).astype(np.float32)
    os.makedirs(speakers_dir, exist_ok=True)
    path = os.path.join(speakers_dir, name + ".npy")
    np.save(path, emb)
    return path


def main(argv=None):
    import argparse
    from .settings import get_api_settings
    s = get_api_settings()
    ap = argparse.ArgumentParser(prog="python -m wis_hip.sv", description="speaker verification tools")
    sub = ap.add_subparsers(dest="cmd", required=True)
    e = sub.add_parser("enroll", help="write a speaker's embedding (NAME.npy) from a recording")
    e.add_argument("name")
    e.add_argument("audio")
    e.add_argument("--dir", default=s.sv_speakers_dir)
    e.add_argument("--model", default=s.sv_model_path)
    a = ap.parse_args(argv)
    print(enroll(a.name, a.audio, a.dir, model_path=a.model, resample_on_gpu=getattr(s, "resample_on_gpu", False)))


if __name__ == "__main__":
    main()
