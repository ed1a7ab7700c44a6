"""not gpu: the host side of speaker verification (wis_hip/sv.py, `voice_auth`): the engine's relative-position bucket table, the
weight layouts the loader hands to wis_sv_create, checkpoint loading, the reference's preprocessing and scoring, and the
/api/willow voice_auth paths with a fake embedder."""
import asyncio
import io
import json
import os
import wave

import numpy as np
import pytest

torch = pytest.importorskip("torch")


def _tiny_cfg():
    from wis_hip import sv
    return sv.hf_config(hidden_size=32, num_attention_heads=2, num_hidden_layers=1, intermediate_size=64, conv_dim=(16,) * 7,
                        num_conv_pos_embeddings=8, num_conv_pos_embedding_groups=2, tdnn_dim=(16, 16, 16, 16, 24), xvector_output_dim=8)


def test_rel_buckets_equal_hf():
    from transformers import WavLMForXVector
    from wis_hip import sv
    attn = WavLMForXVector(_tiny_cfg()).wavlm.encoder.layers[0].attention
    L = 2999                       # a handle built for 60 s: distances past max_bucket_distance (800) saturate
    tab = sv.rel_buckets(-(L - 1), 2 * L - 1)
    for T in list(range(1, 40)) + [97, 250, 498, 499, 800, 801, 802, 1249, 2998, 2999]:
        rel = torch.arange(T)[None, :] - torch.arange(T)[:, None]
        ref = attn._relative_positions_bucket(rel).numpy()
        got = tab[(rel + L - 1).numpy()]
        assert np.array_equal(got, ref), T
    assert tab[0] == 159 and tab[-1] == 319              # the two saturated ends


def test_sharpened_model_sees_every_attention_ablation():
    """The power of tests/test_gpu_sv.py's sharpened model: each wrong variant of the gated relative-position attention
    (tests/sv_ref.py ABLATIONS: no bias, the bias table mirrored, the gate frozen, gate_a / gate_b swapped, gru_rel_pos_const = 1)
    applied to HF float64 must move some hidden state by at least 10x the limit the GPU test holds the engine to.  At HF's default
    init the same ablations move them by less than the limit (the gap this model closes), so a weaker model would fail here."""
    import sys
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import sv_ref as R
    from wis_hip import sv
    hf = R.sharpen(sv.synthetic_model(seed=11)).double()
    x = sv.preprocess(np.random.default_rng(5).standard_normal(48000).astype(np.float32) * 0.1)       # 3 s: T = 149
    _, ref, _, emb = R.hf_forward(hf, x)
    assert max(float(np.abs(h).max()) for h in ref) < 100          # the engine holds the hidden states' f16 copies: well inside range
    moved = {}
    for kind in R.ABLATIONS:
        with R.ablated(hf, kind):
            _, hid, _, _ = R.hf_forward(hf, x)
        moved[kind] = max(R.rel_l2(a, b) for a, b in zip(hid, ref))
    _, again, _, emb2 = R.hf_forward(hf, x)
    assert np.array_equal(emb, emb2)                                # every ablation was undone
    assert min(moved.values()) >= 10 * R.SHARP_HIDDEN_LIMIT, moved


def test_weight_norm_fold_and_conv_layout_match_hf():
    from wis_hip import sv
    torch.manual_seed(3)
    conv = torch.nn.Conv1d(12, 12, kernel_size=8, padding=4, groups=3)
    conv = torch.nn.utils.parametrizations.weight_norm(conv, name="weight", dim=2)
    with torch.no_grad():
        conv.parametrizations.weight.original0.mul_(torch.rand_like(conv.parametrizations.weight.original0) + 0.5)
    g = conv.parametrizations.weight.original0.detach().numpy()
    v = conv.parametrizations.weight.original1.detach().numpy()
    w = sv.fold_weight_norm(g, v)
    np.testing.assert_allclose(w, conv.weight.detach().numpy(), rtol=1e-5, atol=1e-6)
    # [out][k][in] channels-last rows: conv1d(x, W) == im2col rows . W_kin^T, row t = x[t*s : t*s + k] flattened tap-major
    x = torch.randn(1, 6, 40)
    cw = torch.randn(5, 6, 3)
    ref = torch.nn.functional.conv1d(x, cw, stride=2)[0].T.numpy()       # [T'][out]
    wk = sv.conv_weight_kin(cw.numpy()).reshape(5, -1)
    xl = x[0].T.numpy()                                                  # channels-last [T][in]
    rows = np.stack([xl[2 * t: 2 * t + 3].reshape(-1) for t in range(ref.shape[0])])
    np.testing.assert_allclose(rows @ wk.T, ref, rtol=1e-5, atol=1e-5)


@pytest.mark.parametrize("spelling", ["parametrizations", "weight_g"])
def test_loader_round_trips_save_pretrained(tmp_path, spelling):
    from safetensors.numpy import save_file
    from transformers import WavLMForXVector
    from wis_hip import sv
    torch.manual_seed(5)
    m = WavLMForXVector(_tiny_cfg()).eval()
    m.save_pretrained(tmp_path)
    (tmp_path / "preprocessor_config.json").write_text(json.dumps({"do_normalize": False, "sampling_rate": 16000}))
    cfg, sd, pre = sv.load_state_dict(str(tmp_path))
    if spelling == "weight_g":           # the older checkpoints' spelling of the same weight
        sd = dict(sd)
        sd[sv.POS_G] = sd.pop(sv.POS_G2, None) if sv.POS_G2 in sd else sd.pop(sv.POS_G)
        sd[sv.POS_V] = sd.pop(sv.POS_V2, None) if sv.POS_V2 in sd else sd.pop(sv.POS_V)
        save_file({k: np.ascontiguousarray(v) for k, v in sd.items()}, str(tmp_path / "model.safetensors"))
        cfg, sd, pre = sv.load_state_dict(str(tmp_path))
        assert sv.POS_G in sd and sv.POS_G2 not in sd
    assert pre["do_normalize"] is False and cfg["hidden_size"] == 32
    t = sv.engine_tensors(sd)
    ref = m.state_dict()
    eff = m.wavlm.encoder.pos_conv_embed.conv.weight.detach().numpy()           # HF's effective (weight-normed) weight
    np.testing.assert_allclose(t[sv.POS_W], eff.transpose(0, 2, 1), rtol=1e-5, atol=1e-6)
    w1 = ref["wavlm.feature_extractor.conv_layers.1.conv.weight"].numpy()
    assert np.array_equal(t["wavlm.feature_extractor.conv_layers.1.conv.weight"], w1.transpose(0, 2, 1))
    assert np.array_equal(t["tdnn.2.kernel.weight"], ref["tdnn.2.kernel.weight"].numpy())
    assert not any(k.startswith(("classifier.", "objective.")) for k in t)
    with pytest.raises(ValueError):
        sv.check_arch(cfg)                 # the tiny config is not the architecture the engine serves
    sv.check_arch(sv.hf_config().to_dict())


def test_preprocessing_formula():
    from wis_hip import sv
    rng = np.random.default_rng(0)
    x = (rng.standard_normal(200000) * 0.05).astype(np.float32)
    x[1234] = 0.25
    y = sv.sox_norm_gain(x)
    g = 10 ** (8 / 20) / 0.25
    np.testing.assert_allclose(y, np.clip(x * np.float32(g), -1, 1), rtol=1e-6)
    assert np.max(np.abs(y)) == 1.0                        # +8 dBFS peak clips
    t = sv.trim(y)
    assert t.shape == (160000,) and np.array_equal(t, y[:160000])
    z = sv.preprocess(x, do_normalize=True)
    assert abs(float(z.mean())) < 1e-5 and abs(float(z.std()) - 1) < 1e-4
    np.testing.assert_allclose(sv.preprocess(x, do_normalize=False), t)
    short = np.full(100, 0.01, np.float32)
    assert sv.preprocess(short, False).shape == (100,)
    assert np.array_equal(sv.sox_norm_gain(np.zeros(10, np.float32)), np.zeros(10, np.float32))


def _wav_bytes(seconds=0.5, rate=16000):
    pcm = (np.sin(np.arange(int(seconds * rate)) * 0.05) * 8000).astype("<i2")
    f = io.BytesIO()
    with wave.open(f, "wb") as w:
        w.setparams((1, 2, rate, 0, "NONE", "NONE"))
        w.writeframes(pcm.tobytes())
    return f.getvalue(), pcm


class _FakeSV:
    def __init__(self, emb):
        self.emb, self.calls = np.asarray(emb, np.float32), 0

    def embed(self, pcm):
        self.calls += 1
        return self.emb.copy()


def test_do_sv_threshold_format_and_order(tmp_path):
    from wis_hip import sv
    e = np.zeros(512, np.float32)
    e[0] = 1
    d = tmp_path / "spk"
    d.mkdir()
    ang = {"alice": 0.1, "bob": 0.5, "carol": 0.3, "dave": 1.2}
    for name, a in ang.items():
        v = np.zeros(512, np.float32)
        v[0], v[1] = np.cos(a), np.sin(a)
        np.save(d / f"{name}.npy", v * 3.0)              # stored files are not re-normalised: cosine ignores the scale
    (d / "notes.txt").write_text("x")
    data, _ = _wav_bytes()
    res = sv.do_sv(io.BytesIO(data), 0.9, _FakeSV(e * 7), str(d))
    assert list(res) == ["alice", "carol"]                # cos 0.995, 0.955 pass; bob 0.878 and dave do not
    assert res == {"alice": "{:.3f}".format(np.cos(0.1)), "carol": "{:.3f}".format(np.cos(0.3))}
    assert sv.do_sv(io.BytesIO(data), 0.999, _FakeSV(e), str(d)) == {}
    with pytest.raises(ValueError):
        sv.do_sv(io.BytesIO(b"not audio"), 0.5, _FakeSV(e), str(d))
    assert sv.score(e, {}, 0.0) == {}


def test_enroll_writes_normalised_embedding(tmp_path):
    from wis_hip import sv
    data, _ = _wav_bytes()
    p = tmp_path / "a.wav"
    p.write_bytes(data)
    e = np.arange(512, dtype=np.float32)
    out = sv.enroll("Alice", str(p), str(tmp_path / "spk"), verifier=_FakeSV(e))
    v = np.load(out)
    assert out.endswith("Alice.npy") and abs(np.linalg.norm(v) - 1) < 1e-6 and sv.cosine(v, e) > 0.999999
    with pytest.raises(ValueError):
        sv.enroll("../x", str(p), str(tmp_path / "spk"), verifier=_FakeSV(e))


def test_settings_read_sv_fields(monkeypatch):
    from wis_hip.settings import APISettings
    s = APISettings()
    assert (s.support_sv, s.sv_threshold, s.sv_model_path, s.sv_speakers_dir) == (False, 0.75, "./models/microsoft-wavlm-base-plus-sv", "speakers/voice_auth")
    monkeypatch.setenv("SUPPORT_SV", "true")
    monkeypatch.setenv("SV_THRESHOLD", "0.5")
    monkeypatch.setenv("SV_MODEL_PATH", "/m")
    monkeypatch.setenv("SV_SPEAKERS_DIR", "/s")
    s = APISettings()
    assert (s.support_sv, s.sv_threshold, s.sv_model_path, s.sv_speakers_dir) == (True, 0.5, "/m", "/s")


def _server_app(tmp_path, emb, support_sv=True, threshold=0.75):
    import sys
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    from test_server_cpu import _FakeModels
    from wis_hip import whisper
    from wis_hip.server import create_app
    models = _FakeModels()
    models.settings.support_sv = support_sv
    models.settings.sv_threshold = threshold
    models.settings.sv_speakers_dir = str(tmp_path / "spk")
    (tmp_path / "spk").mkdir(exist_ok=True)
    v = np.zeros(512, np.float32)
    v[0] = 1
    np.save(tmp_path / "spk" / "alice.npy", v)
    calls = []

    def fake_whisper(audio_file, model, beam_size, task, detect_language, force_language, translate, models=None):
        calls.append(audio_file.tell())
        return "en", "hello", 12.5, None, 3.0, 500

    fake = _FakeSV(emb)
    return create_app(models=models, sv=fake), fake, calls, fake_whisper


def test_willow_voice_auth_with_fake_sv(tmp_path, monkeypatch):
    import httpx
    from wis_hip import server
    e = np.zeros(512, np.float32)
    e[0], e[1] = 1.0, 0.1
    app, fake, calls, fw = _server_app(tmp_path, e)
    monkeypatch.setattr(server, "do_whisper", fw)
    data, _ = _wav_bytes()

    async def go(app):
        async with httpx.AsyncClient(transport=httpx.ASGITransport(app=app), base_url="http://wis") as c:
            r = await c.post("/api/willow?model=tiny&voice_auth=true", content=data, headers={"x-audio-codec": "wav"})
            return r

    r = asyncio.run(go(app))
    assert r.status_code == 200, r.text
    j = r.json()
    assert j["voice_auth"] == {"alice": "{:.3f}".format(1 / np.sqrt(1.01))} and j["speaker_status"] == "I heard alice say:"
    assert j["text"] == "hello" and {"infer_time", "infer_speedup", "audio_duration", "language"} <= set(j)     # stats forced on
    assert fake.calls == 1 and calls == [0]              # SV first, then Whisper from the start of the audio
    # nobody passes: 406 plain text, Whisper never runs
    e2 = np.zeros(512, np.float32)
    e2[3] = 1
    app, fake, calls, fw = _server_app(tmp_path, e2)
    monkeypatch.setattr(server, "do_whisper", fw)
    r = asyncio.run(go(app))
    assert r.status_code == 406 and r.text == "Unauthorized voice" and calls == []
    # SV disabled (the default): still the 400
    app, fake, calls, fw = _server_app(tmp_path, e, support_sv=False)
    monkeypatch.setattr(server, "do_whisper", fw)
    r = asyncio.run(go(app))
    assert r.status_code == 400 and fake.calls == 0 and calls == []
