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


def test_create_ex_refuses_the_int8_encoder_beyond_d_1280(lib):
    """d_model 1344 (H = 21) with the option on: WIS_E_UNSUPPORTED from the configuration alone - the arena is one byte and the tensor list one empty
    record, so a call that went on to the weights would fail with another code; no device is opened before the check either"""
    from wis_hip import _lib
    cfg = _lib.Config(d_model=1344, n_heads=21, n_enc_layers=1, n_dec_layers=1, n_vocab=51865, n_audio_ctx=1500, n_text_ctx=448, n_mels=80, max_batch=1, max_beam=1)
    arena, tensors, h = (C.c_uint8 * 1)(), (_lib.Tensor * 1)(), C.c_void_p()
    for bits, want in ((8, -7), (7, -1)):      # WIS_E_UNSUPPORTED; (an invalid width is still WIS_E_ARG first)
        ext = _lib.ModelExt(8, bits)
        assert lib.wis_model_create_ex(C.byref(cfg), arena, 1, 0, tensors, 1, 0, C.byref(h), C.byref(ext)) == want and not h.value
    assert b"d_model 1344" in lib.wis_last_error() or b"encoder_weight_bits" in lib.wis_last_error()
    ext = _lib.ModelExt(8, 8)
    assert lib.wis_model_create_ex(C.byref(cfg), arena, 1, 0, tensors, 1, 0, C.byref(h), C.byref(ext)) == -7 and b"d_model 1344" in lib.wis_last_error()


def test_where_maps_the_boundary_cases_to_distinct_indices_in_range():
    """tests/enc_i8_taps.py's _where, which the GPU cases trust for "nothing else was written": every (m, n) of a case has an index of its own inside
    [C | out2], the [Q | K] / K-image part inside C and the V^T part inside out2, and - for the layouts' own statement - a K / V^T element sits where
    include/wis_hip.h says: K image [L][B][H][8][T][8], V^T image [B][H][64][Tpad] (QKV: keys with bits 2 and 3 swapped)"""
    from enc_i8_taps import BOUNDARY_CASES, _where
    for epi, form, (B, T), H, k in BOUNDARY_CASES:
        d, L = 64 * H, k if epi == 4 else 0
        M, N = B * T, 3 * d if epi == 3 else 2 * L * d
        idx, nc, nv = _where(epi, M, N, B, T, H, L)
        assert idx.shape == (M, N) and idx.min() >= 0 and idx.max() < nc + nv and np.unique(idx).size == M * N, (epi, form, B, T, H)
        first = (np.arange(N) < 2 * d) if epi == 3 else (np.arange(N) % (2 * d) < d)
        assert (idx[:, first] < nc).all() and (idx[:, ~first] >= nc).all()
        Tpad = (T + 63) // 64 * 64
        assert Tpad != T and M % 32 and (T % 32 or B == 1)      # (what the cases are for; B = 1 is the K-to-V switch's case)
        m, b, t = M - 1, B - 1, T - 1      # the last row, spelled out by hand
        if epi == 3:
            tp = (t & ~12) | ((t & 4) << 1) | ((t & 8) >> 1)
            assert idx[m, 2 * d + 64 + 3] == nc + ((b * H + 1) * 64 + 3) * Tpad + tp and idx[m, d + 5] == m * 2 * d + d + 5
        else:
            kls, vls = M * d + 8, B * d * Tpad + 8
            assert idx[m, 2 * d + 64 + 11] == kls + (((b * H + 1) * 8 + 1) * T + t) * 8 + 3      # layer 1, head 1, dh 11
            assert idx[m, 3 * d + 64 + 11] == nc + vls + ((b * H + 1) * 64 + 11) * Tpad + t


def test_the_scale_family_tells_the_quantiser_variants_apart():
    """tests/test_gpu_enc_i8_shapes.py compares the row quantiser's bytes with quantize_rows (inv = 1 / scale, rint(r * inv): the header's rule) on
    enc_i8_ref.scale_family.  Here: on that very family a quantiser that divides (rint(r / scale)), and one whose reciprocal is one ulp high or low,
    each leave other bytes - so the GPU comparison would see them"""
    from enc_i8_ref import ln_scale_family, scale_family
    from wis_hip import weights as W
    byte = lambda x: np.clip(np.rint(x), -127, 127).astype(np.int8)

    def counts(rows, name):
        q, scale = W.quantize_rows(rows)
        r, inv = rows.astype(np.float32), (np.float32(1.0) / scale).astype(np.float32)
        assert np.array_equal(q, byte(r * inv[:, None]))
        n_div = int((byte(r / scale[:, None]) != q).sum())
        n_up = int((byte(r * np.nextafter(inv, np.float32(np.inf))[:, None]) != q).sum())
        n_dn = int((byte(r * np.nextafter(inv, np.float32(0))[:, None]) != q).sum())
        print(f"{name}: {np.unique(scale).size} scales; bytes changed by rint(r / scale) {n_div}, by inv + 1 ulp {n_up}, by inv - 1 ulp {n_dn}")
        assert n_div > 0 and n_up > 0 and n_dn > 0
        return scale

    scale = counts(scale_family(4096, 128, seed=8), "scale family 4096 x 128")
    assert np.unique(scale).size == 4096 and scale.min() < 1e-6 and scale.max() > 100
    # the fused kernel's family, through a numpy LayerNorm (the GPU test quantises wis_op_layernorm's rows: other roundings, the same population)
    x, g, b = ln_scale_family(4096, 256, seed=256)
    c = x - x.mean(1, keepdims=True)
    scale = counts((c / np.sqrt((c ** 2).mean(1, keepdims=True) + np.float32(1e-5)) * g + b).astype(np.float16), "LayerNorm family 4096 x 256")
    assert np.unique(scale).size > 1500


@pytest.fixture(scope="module")
def ckv_rig():
    from wis_hip import weights as W
    w, a = W.synthetic_weights("tiny", seed=1234, std=0.02, emb_std=0.06, ln_jitter=0.1), W.arch("tiny")
    mem = (np.random.default_rng(5).standard_normal((1500, a["d_model"])) * 1.5).astype(np.float16).astype(np.float32)      # (LayerNorm-sized rows)
    mem[7], mem[8] = 0, mem[8] * 64
    return w, a, mem


def test_cross_kv_reference_without_quantisation_is_the_oracles(ckv_rig):
    from enc_i8_ref import cross_kv
    from oracle.whisper_ref import WhisperRef
    w, a, mem = ckv_rig
    want = WhisperRef(w, a["d_model"], a["n_layers"], a["n_heads"]).cross_kv(mem)
    got = cross_kv(w, a, mem, quant=False, dtype=np.float64, f16=False)
    assert len(got) == len(want) == 4
    for (k, v), (wk, wv) in zip(got, want):
        for x, y in ((k, wk), (v, wv)):
            y = y.numpy()[0].astype(np.float64)
            assert np.linalg.norm(x - y) / np.linalg.norm(y) < 1e-5      # the oracle is fp32


def test_cross_kv_reference_wrong_variants_move_the_logits(ckv_rig):
    """What tests/test_gpu_enc_i8_model.py compares the int8 engine's logits with must notice the mistakes run_cross_kv's int8 branch could make: each
    of three wrong variants of the rule moves the float64 logits by more than 100 times the reference's own float32-against-float64 difference"""
    from enc_i8_ref import cross_kv, cross_kv_from, cross_kv_parts, decoder_logits
    w, a, mem = ckv_rig
    toks = [50258, 50259, 50359, 50363, 1000, 2000, 3000, 4000]
    rel = lambda x, y: float(np.linalg.norm(x.astype(np.float64) - y) / np.linalg.norm(y))
    good = decoder_logits(w, a, cross_kv(w, a, mem), toks)
    noise = rel(decoder_logits(w, a, cross_kv(w, a, mem, dtype=np.float32), toks, np.float32), good)
    qa, sa, layers = cross_kv_parts(w, a, mem)
    d, L = a["d_model"], len(layers)
    wrong = {
        "layer l's scales used for layer l + 1": (qa, sa, [(qw, layers[l - 1][1], b) for l, (qw, _, b) in enumerate(layers)]),
        "the activation scale dropped": (qa, np.ones_like(sa), layers),
        "V with K's row scales": (qa, sa, [(qw, np.concatenate([sw[:d], sw[:d]]), b) for qw, sw, b in layers]),
    }
    print(f"cross K/V reference: float32 against float64 in the logits {noise:.3e}")
    assert L == 4 and 0 < noise < 1e-4
    for name, parts in wrong.items():
        moved = rel(decoder_logits(w, a, cross_kv_from(*parts), toks), good)
        print(f"   {name}: logits moved by {moved:.3e} = {moved / noise:.0f} x")
        assert moved > 100 * noise, (name, moved, noise)
