"""gpu: the WavLM x-vector embedder (csrc/sv.hip, wis_hip/sv.py) against Hugging Face WavLMForXVector in fp32 on the CPU, with seeded
weights at the true architecture saved by save_pretrained and loaded through the product loader: stage taps, embeddings of the
golden clips and of noise, short / too-short input, determinism, and /api/willow?voice_auth=true end to end."""
import asyncio
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")


def _rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


def _cos(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(a @ b / (np.linalg.norm(a) * np.linalg.norm(b)))


@pytest.fixture(scope="module")
def model(tmp_path_factory):
    from wis_hip import sv
    hf = sv.synthetic_model(seed=11)
    d = tmp_path_factory.mktemp("wavlm")
    hf.save_pretrained(str(d))
    (d / "preprocessor_config.json").write_text('{"do_normalize": true, "sampling_rate": 16000, "feature_size": 1}')
    eng = sv.SpeakerVerifier(str(d))
    yield hf, eng
    eng.close()


@pytest.fixture(scope="module")
def inputs(golden_dir):
    from wis_hip import audio, sv
    out = {}
    for name in ("3sec", "10sec", "30sec"):
        pcm, _ = audio.load_audio(os.path.join(golden_dir, "clips", f"{name}.flac"))
        out[name] = sv.preprocess(pcm)
    out["noise"] = sv.preprocess(np.random.default_rng(7).standard_normal(160000).astype(np.float32) * 0.1)
    return out


def _hf(hf, x):
    feats = {}
    h = hf.wavlm.feature_extractor.register_forward_hook(lambda m, i, o: feats.__setitem__("f", o[0].T.detach().numpy()))
    try:
        with torch.inference_mode():
            r = hf(torch.from_numpy(np.ascontiguousarray(x))[None], output_hidden_states=True)
    finally:
        h.remove()
    return feats["f"], [s[0].numpy() for s in r.hidden_states], r.embeddings[0].numpy()


@pytest.fixture(scope="module")
def oracle(model, inputs):
    hf, _ = model
    return {k: _hf(hf, x) for k, x in inputs.items()}


def test_stage_taps_match_hf(model, inputs, oracle):
    _, eng = model
    x = inputs["10sec"]
    feat, hidden, _ = oracle["10sec"]
    got = eng.taps(x, 0)
    assert got.shape == feat.shape == (499, 512)
    assert _rel(got, feat) <= 2e-3, _rel(got, feat)
    errs = []
    for layer in range(13):
        g = eng.taps(x, 1, layer)
        assert g.shape == hidden[layer].shape
        errs.append(_rel(g, hidden[layer]))
    assert max(errs) <= 5e-3, errs
    td = eng.taps(x, 2)
    assert td.shape == (499 - 14, 1500)


def test_embeddings_match_hf(model, inputs, oracle):
    _, eng = model
    ref = {k: v[2] for k, v in oracle.items()}
    floor = 1 - _cos(ref["3sec"], ref["noise"])       # how far apart two different inputs are under these (weakly discriminative) weights
    for a, b in (("10sec", "noise"), ("3sec", "30sec")):
        floor = min(floor, 1 - _cos(ref[a], ref[b]))
    assert floor > 0
    for k, x in inputs.items():
        got = eng.embed_input(x)
        assert got.shape == (512,)
        assert _rel(got, ref[k]) <= 1e-2, (k, _rel(got, ref[k]))
        assert 1 - _cos(got, ref[k]) <= 0.01 * floor, (k, 1 - _cos(got, ref[k]), floor)


def test_short_and_too_short_clips(model, inputs):
    from wis_hip import _lib
    hf, eng = model
    x = inputs["3sec"][:16000]                     # 1 s: 49 frames, 35 after the TDNN
    _, _, ref = _hf(hf, x)
    got = eng.embed_input(x)
    assert _rel(got, ref) <= 1e-2 and 1 - _cos(got, ref) <= 1e-4
    with pytest.raises(_lib.WisError) as e:
        eng.embed_input(inputs["3sec"][:4000])      # 12 frames: fewer than 2 left after the TDNN layers
    assert e.value.code == -1
    with pytest.raises(_lib.WisError) as e:
        eng.embed_input(np.zeros(160001, np.float32))
    assert e.value.code == -6


def test_repeat_calls_bit_identical(model, inputs):
    _, eng = model
    a = eng.embed_input(inputs["10sec"])
    eng.embed_input(inputs["noise"])
    b = eng.embed_input(inputs["10sec"])
    assert np.array_equal(a, b)


def test_willow_voice_auth_end_to_end(model, golden_dir, tmp_path):
    import httpx
    from wis_hip import audio, sv
    from wis_hip.server import create_app
    from wis_hip.settings import APISettings
    from wis_hip.whisper import WhisperModels
    _, eng = model
    clip = os.path.join(golden_dir, "clips", "10sec.flac")
    spk = tmp_path / "spk"
    sv.enroll("alice", clip, str(spk), verifier=eng)
    pcm, _ = audio.load_audio(clip)
    np.save(spk / "mallory.npy", -eng.embed(pcm))
    s = APISettings()
    s.whisper_model_path = "synthetic:{size}"
    s.fixed_new_tokens = 6
    s.support_sv = True
    s.sv_speakers_dir = str(spk)
    app = create_app(models=WhisperModels(s, device_index=[0]), sv=eng)
    data = open(clip, "rb").read()

    async def go():
        async with httpx.AsyncClient(transport=httpx.ASGITransport(app=app), base_url="http://wis", timeout=600) as c:
            return await c.post("/api/willow?model=tiny&voice_auth=true", content=data, headers={"x-audio-codec": "flac"})

    r = asyncio.run(go())
    assert r.status_code == 200, r.text
    j = r.json()
    assert list(j["voice_auth"]) == ["alice"] and float(j["voice_auth"]["alice"]) >= 0.999
    assert j["speaker_status"] == "I heard alice say:" and "infer_time" in j and "text" in j
