"""not gpu: the int8 encoder's host side - the keyword, the setting's way to the model, wis_model_create_ex's argument check, and the test reference."""
import ctypes as C

import numpy as np
import pytest


@pytest.mark.parametrize("bad", ["int8_float16", "float32", "", None, 8])
def test_encoder_compute_type_is_validated_before_any_device_is_touched(bad):
    from wis_hip import ctranslate2 as ct2
    with pytest.raises(ValueError, match="float16, int8"):
        ct2.Whisper("synthetic:tiny", encoder_compute_type=bad)
    with pytest.raises(TypeError):
        ct2.Whisper("synthetic:tiny", "cuda", 0, "default", 1, 0, 8, 5, None, None, None, "int8")      # keyword-only


@pytest.mark.parametrize("value", ["float16", "int8"])
def test_the_setting_reaches_the_model(monkeypatch, value):
    from types import SimpleNamespace
    from wis_hip import whisper
    from wis_hip.settings import APISettings
    seen = {}
    monkeypatch.setattr(whisper.ctranslate2.models, "Whisper", lambda path, **kw: seen.update(kw) or SimpleNamespace(_replicas=[]))
    assert APISettings().encoder_compute_type == "float16"
    models = whisper.WhisperModels(APISettings(whisper_model_path="synthetic:{size}", encoder_compute_type=value), device_index=[0])
    models.get("tiny")
    assert seen["encoder_compute_type"] == value and seen["compute_type"] == "float16"


@pytest.mark.parametrize("size,bits", [(8, 4), (8, 7), (8, -8), (4, 8), (0, 0)])
def test_create_ex_refuses_bad_options(lib, size, bits):
    from wis_hip import _lib
    ext, h = _lib.ModelExt(size, bits), C.c_void_p()
    assert lib.wis_model_create_ex(None, None, 0, 0, None, 0, 0, C.byref(h), C.byref(ext)) == -1      # WIS_E_ARG, before anything else is looked at
    assert b"encoder_weight_bits" in lib.wis_last_error()


def test_reference_without_quantisation_is_the_oracles_encoder(golden_dir):
    from enc_i8_ref import encode
    from oracle.whisper_ref import WhisperRef
    from wis_hip import weights as W
    w, a = W.synthetic_weights("tiny", seed=1234, std=0.02, emb_std=0.06, ln_jitter=0.1), W.arch("tiny")
    mel = np.load(golden_dir + "/logmel_3sec.npz")["mel"].astype(np.float32)
    want = WhisperRef(w, a["d_model"], a["n_layers"], a["n_heads"]).encode(mel[None]).numpy()[0].astype(np.float64)
    got = encode(w, a, mel, quant=False, f16=False)      # (base-2 softmax of log2(e)-scaled scores, as the engine's default loop: the same function)
    assert np.linalg.norm(got - want) / np.linalg.norm(want) < 1e-5      # the oracle is fp32
