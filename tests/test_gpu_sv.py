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


# ---- a model under which the attention's own features matter --------------------------------------------------------------------
# At HF's default init the relative-position bias and its gate barely move the output (tests/sv_ref.py sharpen()); the sharpened
# seed-11 model makes a dropped, mirrored or mis-gated bias visible (tests/test_sv_cpu.py checks that power on HF itself).  The oracle
# is HF in float64.
def _sv_ref():
    import sys
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import sv_ref
    return sv_ref


SHARP_LENGTHS = (5200, 5520, 10320, 48000, 160000)            # T = 16 (the shortest accepted), 17, 32, 149, 499


@pytest.fixture(scope="module")
def sharp(tmp_path_factory):
    from wis_hip import sv
    R = _sv_ref()
    hf = R.sharpen(sv.synthetic_model(seed=11))
    d = tmp_path_factory.mktemp("wavlm_sharp")
    hf.save_pretrained(str(d))
    (d / "preprocessor_config.json").write_text('{"do_normalize": true, "sampling_rate": 16000, "feature_size": 1}')
    eng = sv.SpeakerVerifier(str(d))
    yield hf.double(), eng, str(d)
    eng.close()


@pytest.fixture(scope="module")
def long_input(golden_dir):
    """the 30 s golden clip through the reference's gain and normalisation, untrimmed (slices of it are the inputs below)"""
    from wis_hip import audio, sv
    pcm, _ = audio.load_audio(os.path.join(golden_dir, "clips", "30sec.flac"))
    return sv.zero_mean_unit_var(sv.sox_norm_gain(pcm))


@pytest.fixture(scope="module")
def sharp_oracle(sharp, long_input):
    """HF float64 of each input length, computed once"""
    hf = sharp[0]
    R = _sv_ref()
    cache = {}

    def get(n):
        if n not in cache:
            cache[n] = R.hf_forward(hf, long_input[:n])
        return cache[n]
    return get


def _check_taps(eng, x, ref, what):
    R = _sv_ref()
    feat, hidden, tdnn, emb = ref
    T = feat.shape[0]
    got = eng.taps(x, 0)
    assert got.shape == (T, 512)
    assert R.rel_l2(got, feat) <= 2e-3 and R.worst_row(got, feat) <= 1e-2, (what, R.rel_l2(got, feat), R.worst_row(got, feat))
    errs, rows = [], []
    for layer in range(13):
        g = eng.taps(x, 1, layer)
        assert g.shape == (T, 768)
        errs.append(R.rel_l2(g, hidden[layer]))
        rows.append(R.worst_row(g, hidden[layer]))
    assert max(errs) <= R.SHARP_HIDDEN_LIMIT and max(rows) <= 4 * R.SHARP_HIDDEN_LIMIT, (what, errs, rows)
    td = eng.taps(x, 2)
    assert td.shape == tdnn.shape == (T - 14, 1500)
    assert R.rel_l2(td, tdnn) <= 1e-2, (what, R.rel_l2(td, tdnn))
    e = eng.embed_input(x)
    assert R.rel_l2(e, emb) <= 1e-2, (what, R.rel_l2(e, emb))
    print(f"sharpened {what}: T={T} feat {R.rel_l2(got, feat):.2e}, hidden max {max(errs):.2e} (worst row {max(rows):.2e}), "
          f"tdnn {R.rel_l2(td, tdnn):.2e}, embedding {R.rel_l2(e, emb):.2e}")
    return e


@pytest.mark.parametrize("n", SHARP_LENGTHS)
def test_sharpened_taps_match_hf_float64(sharp, long_input, sharp_oracle, n):
    _, eng, _ = sharp
    _check_taps(eng, long_input[:n], sharp_oracle(n), f"n={n}")


def test_sharpened_too_short(sharp, long_input):
    from wis_hip import _lib
    _, eng, _ = sharp
    with pytest.raises(_lib.WisError) as e:
        eng.embed_input(long_input[:5199])        # T = 15: one frame after the TDNN layers
    assert e.value.code == -1


def test_sharpened_60s_handle(sharp, long_input, sharp_oracle):
    """a handle built for 60 s (bias table of 2 x 2999 - 1 distances, saturated past 800): bit-identical to the default handle on
    10 s, and HF parity on 25 s (T = 1249, distances up to 1248)"""
    from wis_hip import sv
    _, eng, path = sharp
    big = sv.SpeakerVerifier(path, max_samples=60 * 16000)
    try:
        x10 = long_input[:160000]
        assert np.array_equal(big.embed_input(x10), eng.embed_input(x10))
        _check_taps(big, long_input[:400000], sharp_oracle(400000), "n=400000 (60 s handle)")
    finally:
        big.close()
