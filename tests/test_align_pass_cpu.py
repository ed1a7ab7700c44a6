"""The one-pass align route's public surface without a GPU: constructor, setting and C entry point refuse bad values before anything touches a device."""
import pytest


def test_bad_align_forward_and_mode_are_refused(lib):
    from wis_hip import ctranslate2 as ct2
    from wis_hip.server import create_app
    from wis_hip.settings import APISettings
    with pytest.raises(ValueError, match="align_forward"):
        ct2.Whisper("synthetic:tiny", align_forward="x")
    assert ct2.ALIGN_FORWARDS == ("windowed", "one_pass") and APISettings().align_forward == "windowed"
    s = APISettings()
    s.align_forward = "x"
    with pytest.raises(ValueError, match="align_forward"):
        create_app(settings=s)
    assert lib.wis_model_set_align_pass(None, 2) == -1      # WIS_E_ARG
