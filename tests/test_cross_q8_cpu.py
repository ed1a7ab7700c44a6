"""The int8 cross K/V option's refusals and defaults, without a GPU (the kernels: tests/test_gpu_cross_q8.py)."""
from types import SimpleNamespace

import pytest


def test_settings_default_and_bad_value(monkeypatch):
    from wis_hip import ctranslate2 as ct2
    from wis_hip.settings import APISettings
    assert APISettings().cross_kv_compute_type == "float16"
    monkeypatch.setattr(ct2._lib, "require_gpu", lambda: pytest.fail("the value is checked before the GPU is looked for"))
    with pytest.raises(ValueError, match="cross_kv_compute_type"):
        ct2.Whisper("unused", cross_kv_compute_type="int4")


def test_align_raises_unsupported_option_on_an_int8_model():
    from wis_hip import ctranslate2 as ct2
    m = ct2.Whisper.__new__(ct2.Whisper)
    m.cross_kv_compute_type = "int8"
    with pytest.raises(ct2.UnsupportedOption, match="cross_kv_compute_type"):
        m._align(None, None, 0, 1, [1], [[2]], 3000, width=7)


def test_word_timestamps_are_refused_before_any_engine_call():
    from wis_hip import whisper
    from wis_hip.settings import APISettings
    models = SimpleNamespace(settings=APISettings(cross_kv_compute_type="int8"), get=lambda *a, **k: pytest.fail("the refusal comes before the model is touched"))
    with pytest.raises(ValueError, match="cross_kv_compute_type"):
        whisper.do_whisper(b"", "transcribe", "en", models=models, word_timestamps=True)
