"""The one-pass prefill's public surface without a GPU: the constructor and the setting refuse bad values (before anything touches a device), and the
C entry point is declared wherever the library's symbols are."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_constructor_refuses_bad_prompt_prefill():
    from wis_hip import ctranslate2 as ct2
    with pytest.raises(ValueError, match="prompt_prefill"):
        ct2.Whisper("synthetic:tiny", prompt_prefill="two_pass")
    assert ct2.PROMPT_PREFILLS == ("windowed", "one_pass")


def test_setting_refuses_bad_prompt_prefill():
    from wis_hip.server import create_app
    from wis_hip.settings import APISettings
    assert APISettings().prompt_prefill == "windowed"
    s = APISettings()
    s.prompt_prefill = "onepass"
    with pytest.raises(ValueError, match="prompt_prefill"):
        create_app(settings=s)


@pytest.mark.parametrize("name", ["wis_model_set_prefill", "wis_op_dec_prefill_proj", "wis_op_dec_prefill_self_attn", "wis_op_dec_prefill_cross_attn"])
def test_symbol_declared_everywhere(name):
    from wis_hip import _lib
    assert name in [s[0] for s in _lib.SYMBOLS]
    with open(os.path.join(ROOT, "include", "wis_hip.h")) as f:
        assert re.search(r"^int %s\(" % name, f.read(), re.M)
    with open(os.path.join(ROOT, "willow-inference-server_amd", "csrc", "exports.map")) as f:
        assert re.search(r"global:[^}]*\bwis_\*", f.read())      # every wis_ symbol is exported
