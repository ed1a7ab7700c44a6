"""CPU: large-v3 / large-v3-turbo support on the host side - the per-model special-id table, checkpoints whose encoder and decoder
depths differ or that carry 128 mel bins (HF and CTranslate2 layouts), feature-shape checks, the 100-language table and the model
selection of do_whisper / the REST layer (fake engine: nothing here touches a GPU)."""
import asyncio
import json

import numpy as np
import pytest
import torch

V2_IDS = dict(eot=50257, sot=50258, translate=50358, transcribe=50359, startoflm=50360, startofprev=50361, nospeech=50362,
              notimestamps=50363, timestamp_begin=50364)
# openai-whisper's tokenizer for the 51866-token vocabulary (large-v3): <|yue|> = 50358 is the 100th language
V3_IDS = dict(eot=50257, sot=50258, translate=50359, transcribe=50360, startoflm=50361, startofprev=50362, nospeech=50363,
              notimestamps=50364, timestamp_begin=50365)


def test_special_table_matches_the_module_constants_and_the_v3_layout():
    from wis_hip import weights as W
    st = W.special_tokens(51865)
    assert {k: getattr(st, k) for k in V2_IDS} == V2_IDS
    assert (st.eot, st.sot, st.translate, st.transcribe, st.nospeech, st.notimestamps) == (W.EOT, W.SOT, W.TRANSLATE, W.TRANSCRIBE, W.NO_SPEECH, W.NO_TIMESTAMPS)
    assert st.lang_ids == W.LANG_IDS and st.default_suppress_ids() == W.SUPPRESS_IDS
    v3 = W.special_tokens(51866)
    assert {k: getattr(v3, k) for k in V3_IDS} == V3_IDS
    assert v3.lang_ids == list(range(50259, 50359)) and len(v3.lang_codes) == 100 and v3.lang_codes[-1] == "yue"
    assert v3.language_token_id("yue") == 50358 and v3.language_token_id("en") == 50259
    sup = v3.default_suppress_ids()
    assert [t for t in sup if t < 50257] == [t for t in W.SUPPRESS_IDS if t < 50257]
    assert [t for t in sup if t >= 50257] == [50258, 50359, 50360, 50361, 50362, 50363]
    with pytest.raises(ValueError, match="English-only"):
        W.special_tokens(51864)


def test_checkpoint_ids_take_priority(tmp_path):
    from wis_hip import weights as W
    gen = {"lang_to_id": {f"<|{c}|>": 50259 + i for i, c in enumerate(["en", "zh", "de"])}, "task_to_id": {"translate": 50400, "transcribe": 50401},
           "no_timestamps_token_id": 50500, "decoder_start_token_id": 50258}
    st = W.special_tokens(51866, W.special_overrides_from_generation_config(gen))
    assert st.lang_ids == [50259, 50260, 50261] and st.lang_codes == ("en", "zh", "de")
    assert (st.translate, st.transcribe, st.notimestamps, st.timestamp_begin) == (50400, 50401, 50500, 50501)
    # tokenizer.json: added tokens by content
    toks = [{"id": 50257, "content": "<|endoftext|>", "special": True}, {"id": 50258, "content": "<|startoftranscript|>", "special": True},
            {"id": 50259, "content": "<|en|>", "special": True}, {"id": 50260, "content": "<|yue|>", "special": True},
            {"id": 50261, "content": "<|translate|>", "special": True}, {"id": 50270, "content": "<|notimestamps|>", "special": True},
            {"id": 50271, "content": "<|0.00|>", "special": False}]
    p = tmp_path / "tokenizer.json"
    p.write_text(json.dumps({"added_tokens": toks}))
    st = W.special_tokens(51866, W.special_tokens_from_tokenizer_json(str(p)))
    assert st.lang_ids == [50259, 50260] and st.lang_codes == ("en", "yue")
    assert (st.translate, st.notimestamps, st.timestamp_begin) == (50261, 50270, 50271)
    # the engine config carries them
    from wis_hip import ctranslate2 as ct2
    a = W.arch("large-v3-turbo")
    cfg = ct2.make_config(a, 1, 1, special=st)
    assert (cfg.eot, cfg.sot, cfg.no_timestamps, cfg.no_speech, cfg.n_lang) == (50257, 50258, 50270, st.nospeech, 2)


def test_arch_table_and_synthetic_layouts():
    from wis_hip import weights as W
    v3, turbo = W.arch("large-v3"), W.arch("large-v3-turbo")
    assert (v3["d_model"], v3["n_enc_layers"], v3["n_dec_layers"], v3["n_heads"], v3["n_mels"], v3["n_vocab"]) == (1280, 32, 32, 20, 128, 51866)
    assert (turbo["n_enc_layers"], turbo["n_dec_layers"], turbo["n_layers"], turbo["n_mels"]) == (32, 4, 4, 128)
    assert W.arch("large") == dict(W.arch("large-v2"))
    idx, _ = W.synthetic_layout("large-v3-turbo")
    names = {e["name"]: e["shape"] for e in idx}
    assert names["encoder/conv1/weight"] == [1280, 128, 3] and names["decoder/embeddings/weight"] == [51866, 1280]
    assert "encoder/layer_31/ffn/linear_0/weight" in names and "decoder/layer_3/ffn/linear_0/weight" in names
    assert "decoder/layer_4/ffn/linear_0/weight" not in names
    from wis_hip import ctranslate2 as ct2
    cfg = ct2.make_config(turbo, 1, 5)
    assert (cfg.n_enc_layers, cfg.n_dec_layers, cfg.n_mels, cfg.n_vocab, cfg.n_lang) == (32, 4, 128, 51866, 100)
    assert (cfg.no_timestamps, cfg.no_speech) == (50364, 50363)


def _hf_checkpoint(path, n_mels, enc, dec, vocab, seed=3):
    from transformers import WhisperConfig, WhisperForConditionalGeneration
    torch.manual_seed(seed)
    cfg = WhisperConfig(vocab_size=vocab, d_model=384, encoder_layers=enc, decoder_layers=dec, encoder_attention_heads=6, decoder_attention_heads=6,
                        encoder_ffn_dim=1536, decoder_ffn_dim=1536, num_mel_bins=n_mels, max_source_positions=1500, max_target_positions=448,
                        pad_token_id=50257, bos_token_id=50257, eos_token_id=50257, decoder_start_token_id=50258, suppress_tokens=None,
                        begin_suppress_tokens=None)
    m = WhisperForConditionalGeneration(cfg).eval().half()
    m.save_pretrained(str(path), safe_serialization=True)
    return m


@pytest.mark.parametrize("geom", [(128, 4, 2, 51866), (80, 4, 2, 51865)], ids=["v3-128bin-4x2", "distil-80bin-4x2"])
def test_hf_and_ct2_checkpoints_load_with_their_geometry(tmp_path, geom):
    from wis_hip import ctranslate2 as ct2, weights as W
    n_mels, enc, dec, vocab = geom
    hf_dir, ct2_dir = tmp_path / "hf", tmp_path / "ct2"
    _hf_checkpoint(hf_dir, n_mels, enc, dec, vocab)
    W.convert_hf_to_ct2_dir(str(hf_dir), str(ct2_dir))
    n_lang = 100 if vocab == 51866 else 99
    with open(ct2_dir / "config.json") as f:
        cj = json.load(f)
    assert cj["lang_ids"] == list(range(50259, 50259 + n_lang))
    st = W.special_tokens(vocab)
    assert cj["suppress_ids"] == st.default_suppress_ids()
    for d in (hf_dir, ct2_dir):
        w, a, cfg = W.load_model_dir(str(d))
        assert (a["n_mels"], a["n_enc_layers"], a["n_dec_layers"], a["n_layers"], a["n_vocab"]) == (n_mels, enc, dec, dec, vocab)
        assert w["encoder/conv1/weight"].shape == (384, n_mels, 3)
        assert f"encoder/layer_{enc - 1}/ffn/linear_0/weight" in w and f"decoder/layer_{dec}/ffn/linear_0/weight" not in w
        special = ct2.special_tokens_for(a, cfg.get("special"), cfg.get("lang_ids"))
        assert len(special.lang_ids) == n_lang
        c = ct2.make_config(a, 2, 5, suppress_ids=cfg.get("suppress_ids"), lang_ids=cfg.get("lang_ids"), special=special)
        assert (c.n_enc_layers, c.n_dec_layers, c.n_mels, c.n_lang) == (enc, dec, n_mels, n_lang)
        assert c.no_timestamps == (50364 if vocab == 51866 else 50363)


def test_english_only_checkpoint_is_refused(tmp_path):
    from wis_hip import weights as W
    _hf_checkpoint(tmp_path, 80, 2, 2, 51864)
    with pytest.raises(ValueError, match="English-only"):
        W.load_model_dir(str(tmp_path))


def _bare_whisper(size):
    from wis_hip import ctranslate2 as ct2, weights as W
    m = ct2.Whisper.__new__(ct2.Whisper)
    m.arch = W.arch(size)
    m.special = W.special_tokens(m.arch["n_vocab"])
    return m


def test_feature_shapes_follow_the_model():
    from wis_hip import _lib, audio, ctranslate2 as ct2
    v3, v2 = _bare_whisper("large-v3-turbo"), _bare_whisper("large")
    with pytest.raises(ValueError, match="128"):
        v3._features(ct2.StorageView.from_array(np.zeros((1, 80, 3000), np.float32)))
    with pytest.raises(ValueError, match="80"):
        v2._features(ct2.StorageView.from_array(np.zeros((1, 128, 3000), np.float32)))
    assert v3._features(np.zeros((2, 128, 3000), np.float32)).shape == (2, 128, 3000)
    assert v3._features(np.zeros((1, _lib.N_SAMPLES), np.float32), _lib.WIS_IN_PCM_HOST).shape == (1, _lib.N_SAMPLES)
    with pytest.raises(ValueError):
        audio.log_mel_spectrogram(np.zeros(audio.N_SAMPLES, np.float32), n_mels=64)


def test_yue_only_for_v3():
    from wis_hip import weights as W
    from wis_hip.languages import LANGUAGE_CODES, LANGUAGE_CODES_V3
    from wis_hip.whisper import check_language
    assert len(LANGUAGE_CODES) == 99 and LANGUAGE_CODES_V3 == LANGUAGE_CODES + ("yue",)
    assert not check_language("yue") and check_language("en")
    assert check_language("yue", W.special_tokens(51866)) and not check_language("yue", W.special_tokens(51865))
    with pytest.raises(ValueError):
        W.special_tokens(51865).language_token_id("yue")


class _FakeEngine:
    """ctranslate2.models.Whisper stand-in: records what it is asked for, answers fixed ids."""
    built = []

    def __init__(self, path, **kw):
        from wis_hip import weights as W
        size = path.split(":")[1]
        self.path, self.arch = path, W.arch(size)
        self.special = W.special_tokens(self.arch["n_vocab"])
        self.n_mels = self.arch["n_mels"]
        self._replicas = [type("R", (), {"device": 0})()]
        self.prompts, self.features = [], []
        _FakeEngine.built.append(path)

    def generate(self, features, prompts, **kw):
        from wis_hip.ctranslate2 import WhisperGenerationResult
        self.prompts.append([list(p) for p in prompts])
        self.features.append(np.asarray(features.array).shape)
        return [WhisperGenerationResult([[400, 401, 402]], [0.0]) for _ in prompts]

    def detect_language(self, features, input_kind=0):
        return [[("<|yue|>", 0.9), ("<|en|>", 0.1)]]


@pytest.fixture
def fake_models(monkeypatch):
    from wis_hip import ctranslate2 as ct2, whisper
    from wis_hip.settings import APISettings
    monkeypatch.setattr(ct2.models, "Whisper", _FakeEngine)
    monkeypatch.setattr(ct2._lib, "device_count", lambda: 1)
    _FakeEngine.built = []
    s = APISettings()
    s.whisper_model_path = "synthetic:{size}"
    return whisper.WhisperModels(s, device_index=[0])


def test_do_whisper_selects_v3_models_with_their_ids(fake_models):
    from wis_hip.whisper import do_whisper
    pcm = np.zeros(16000, np.float32)
    r = do_whisper(pcm, "large-v3-turbo", 1, models=fake_models, force_language="yue")
    eng = fake_models.get("large-v3-turbo")
    assert eng.path == "synthetic:large-v3-turbo" and r.tokens == [400, 401, 402]
    assert eng.prompts[-1] == [[50258, 50358, 50360, 50364]]            # <|sot|> <|yue|> <|transcribe|> <|notimestamps|>
    r = do_whisper(pcm, "large-v3", 1, models=fake_models, detect_language=True, translate=True)
    eng = fake_models.get("large-v3")
    assert r[0] == "yue" and eng.prompts[-2] == [[50258, 50358, 50360, 50364]] and eng.prompts[-1] == [[50258, 50358, 50359, 50364]]
    do_whisper(pcm, "large-v3", 1, models=fake_models, force_language="en", timestamps=True)
    assert eng.prompts[-1] == [[50258, 50259, 50360]]
    # the 80-bin models keep the ids they always had, and refuse yue
    do_whisper(pcm, "large", 1, models=fake_models, force_language="en")
    assert fake_models.get("large").prompts[-1] == [[50258, 50259, 50359, 50363]]
    with pytest.raises(ValueError):
        do_whisper(pcm, "large", 1, models=fake_models, force_language="yue")
    with pytest.raises(ValueError):
        do_whisper(pcm, "large-v4", 1, models=fake_models)


def test_unfused_features_use_the_model_mel_bins(fake_models, monkeypatch):
    from wis_hip import audio
    from wis_hip.whisper import do_whisper
    seen = []

    def fake_logmel(x, n_mels=80, device=None):
        seen.append(n_mels)
        return audio.MelFeatures(np.zeros((x.shape[0], n_mels, 3000), np.float32))
    monkeypatch.setattr(audio, "log_mel_spectrogram", fake_logmel)
    fake_models.settings.fuse_logmel = False
    do_whisper(np.zeros(16000, np.float32), "large-v3-turbo", 1, models=fake_models, force_language="en")
    do_whisper(np.zeros(16000, np.float32), "medium", 1, models=fake_models, force_language="en")
    assert seen == [128, 80]
    assert fake_models.get("large-v3-turbo").features[-1] == (1, 128, 3000)


def test_default_preload_set_is_unchanged(fake_models, monkeypatch):
    from wis_hip import whisper
    assert whisper.MODEL_SIZES == ("tiny", "base", "small", "medium", "large")
    s = fake_models.settings
    assert s.preload_whisper_model_large_v3 is False and s.preload_whisper_model_large_v3_turbo is False
    fake_models.preload()
    assert _FakeEngine.built == [f"synthetic:{m}" for m in whisper.MODEL_SIZES]
    s.preload_all_models = True
    fake_models._models.clear()
    _FakeEngine.built = []
    fake_models.preload()
    assert _FakeEngine.built == [f"synthetic:{m}" for m in whisper.MODEL_SIZES]
    s.preload_whisper_model_large_v3_turbo = True
    fake_models.preload()
    assert _FakeEngine.built[-1] == "synthetic:large-v3-turbo" and "synthetic:large-v3" not in _FakeEngine.built


def test_asr_endpoint_serves_v3_model(fake_models):
    import httpx
    from wis_hip.server import create_app
    from wis_hip.settings import APISettings
    app = create_app(models=fake_models)
    import io
    import wave
    buf = io.BytesIO()
    with wave.open(buf, "wb") as w:
        w.setnchannels(1), w.setsampwidth(2), w.setframerate(16000)
        w.writeframes(np.zeros(16000, "<i2").tobytes())

    bd = "xYzBoundary123"
    body = (f"--{bd}\r\nContent-Disposition: form-data; name=\"audio_file\"; filename=\"a.wav\"\r\nContent-Type: application/octet-stream\r\n\r\n").encode() \
        + buf.getvalue() + f"\r\n--{bd}--\r\n".encode()
    hdr = {"content-type": f"multipart/form-data; boundary={bd}"}

    async def go():
        async with httpx.AsyncClient(transport=httpx.ASGITransport(app=app), base_url="http://wis") as c:
            r = await c.post("/api/asr?model=large-v3-turbo&force_language=yue", content=body, headers=hdr)
            assert r.status_code == 200, r.text
            assert r.json()["text"] == "400 401 402"
            r = await c.post("/api/asr?model=large&force_language=yue", content=body, headers=hdr)
            assert r.status_code == 400
    asyncio.run(go())
    assert fake_models.get("large-v3-turbo").prompts[-1] == [[50258, 50358, 50360, 50364]]
    assert APISettings().whisper_model_default == "medium"
