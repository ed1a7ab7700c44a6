"""-m gpu: large-v3 / large-v3-turbo end to end.  The 128-bin log-mel against transformers' WhisperFeatureExtractor; the engine at the
full large-v3 (32 / 32 layers, 128 bins, 51866 tokens), large-v3-turbo (32 / 4) and distil (32 / 2, 80 bins) geometries against
transformers' WhisperForConditionalGeneration run in fp32 on the CPU with the same f16-rounded weights, fed to the engine through the
Hugging Face loader (weights.from_hf_state_dict); searches, language detection, timestamps, int8_float16 and the REST path on v3 ids."""
import ctypes as C
import gc
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
EOT, SOT = 50257, 50258
V3 = dict(translate=50359, transcribe=50360, nospeech=50363, notimestamps=50364, timestamp_begin=50365)


def _clip(golden_dir, name):
    from wis_hip import audio
    with open(os.path.join(golden_dir, "clips", f"{name}.flac"), "rb") as f:
        pcm, sr = audio.load_audio(f)
    assert sr == 16000
    return audio.pad_or_trim(pcm.astype(np.float32))


def _pcms(golden_dir):
    noise = (np.random.default_rng(11).standard_normal(480000) * 0.1).astype(np.float32)
    return [_clip(golden_dir, c) for c in ("3sec", "10sec", "30sec")] + [noise]


def _logmel(lib, pcm, n_mels):
    from wis_hip import _lib
    x = np.ascontiguousarray(np.atleast_2d(pcm), np.float32)
    out = np.zeros((x.shape[0], n_mels, 3000), np.float32)
    ns = (C.c_int64 * x.shape[0])(*([480000] * x.shape[0]))
    _lib.check(lib.wis_logmel_n(0, n_mels, _lib.ptr(x), 480000, ns, x.shape[0], 0, _lib.ptr(out), 0))
    return out


def test_logmel_128_matches_feature_extractor_and_melstream(golden_dir, lib):
    from transformers import WhisperFeatureExtractor
    from wis_hip import _lib, audio
    fe = WhisperFeatureExtractor(feature_size=128)
    pcms = _pcms(golden_dir)
    for i, pcm in enumerate(pcms):
        got = _logmel(lib, pcm, 128)[0]
        exp = fe(pcm, sampling_rate=16000, return_tensors="np")["input_features"][0]
        err = np.abs(got - exp).max()
        print(f"clip {i}: 128-bin log-mel vs WhisperFeatureExtractor max abs {err:.2e}")
        assert got.shape == (128, 3000) and err <= 5e-5
        assert np.array_equal(audio.log_mel_spectrogram(pcm, n_mels=128).numpy(), got)
        # the streaming front-end, fed 20 ms at a time, is bit-identical
        st = audio.MelStream(0, n_mels=128)
        for s in range(0, 480000, 320):
            st.feed(pcm[s:s + 320])
        assert np.array_equal(st.finish(), got)
        st.close()
        # the 80-bin entry point is the n_mels = 80 form
        m80 = np.zeros((1, 80, 3000), np.float32)
        ns = (C.c_int64 * 1)(480000)
        _lib.check(lib.wis_logmel(0, _lib.ptr(np.ascontiguousarray(pcm[None])), 480000, ns, 1, 0, _lib.ptr(m80), 0))
        assert np.array_equal(m80, _logmel(lib, pcm, 80))
    out = np.zeros((1, 64, 3000), np.float32)
    ns = (C.c_int64 * 1)(480000)
    assert lib.wis_logmel_n(0, 64, _lib.ptr(np.ascontiguousarray(pcms[0][None])), 480000, ns, 1, 0, _lib.ptr(out), 0) == -7      # WIS_E_UNSUPPORTED
    h = C.c_void_p()
    assert lib.wis_melstream_create_n(0, 96, C.byref(h)) == -7      # WIS_E_UNSUPPORTED


def _hf_from_ct2(w, a):
    """transformers' Whisper (fp32, CPU) holding exactly the weights `w` (CTranslate2 names)."""
    from transformers import WhisperConfig, WhisperForConditionalGeneration
    d, H = a["d_model"], a["n_heads"]
    cfg = WhisperConfig(vocab_size=a["n_vocab"], d_model=d, encoder_layers=a["n_enc_layers"], decoder_layers=a["n_dec_layers"],
                        encoder_attention_heads=H, decoder_attention_heads=H, encoder_ffn_dim=4 * d, decoder_ffn_dim=4 * d,
                        num_mel_bins=a["n_mels"], max_source_positions=1500, max_target_positions=448, pad_token_id=EOT, bos_token_id=EOT,
                        eos_token_id=EOT, decoder_start_token_id=SOT, suppress_tokens=None, begin_suppress_tokens=None)
    f = lambda n: torch.from_numpy(np.asarray(w[n], np.float32))
    sd = {"model.encoder.conv1.weight": f("encoder/conv1/weight"), "model.encoder.conv1.bias": f("encoder/conv1/bias"),
          "model.encoder.conv2.weight": f("encoder/conv2/weight"), "model.encoder.conv2.bias": f("encoder/conv2/bias"),
          "model.encoder.embed_positions.weight": f("encoder/position_encodings/encodings"),
          "model.decoder.embed_tokens.weight": f("decoder/embeddings/weight"),
          "model.decoder.embed_positions.weight": f("decoder/position_encodings/encodings")}
    for side, n in (("encoder", a["n_enc_layers"]), ("decoder", a["n_dec_layers"])):
        sd[f"model.{side}.layer_norm.weight"], sd[f"model.{side}.layer_norm.bias"] = f(f"{side}/layer_norm/gamma"), f(f"{side}/layer_norm/beta")
        for l in range(n):
            p, q = f"{side}/layer_{l}/", f"model.{side}.layers.{l}."
            qkv, bqkv = f(p + "self_attention/linear_0/weight"), f(p + "self_attention/linear_0/bias")
            sd[q + "self_attn.q_proj.weight"], sd[q + "self_attn.k_proj.weight"], sd[q + "self_attn.v_proj.weight"] = qkv[:d], qkv[d:2 * d], qkv[2 * d:]
            sd[q + "self_attn.q_proj.bias"], sd[q + "self_attn.v_proj.bias"] = bqkv[:d], bqkv[2 * d:]
            sd[q + "self_attn.out_proj.weight"], sd[q + "self_attn.out_proj.bias"] = f(p + "self_attention/linear_1/weight"), f(p + "self_attention/linear_1/bias")
            sd[q + "self_attn_layer_norm.weight"], sd[q + "self_attn_layer_norm.bias"] = f(p + "self_attention/layer_norm/gamma"), f(p + "self_attention/layer_norm/beta")
            if side == "decoder":
                kv, bkv = f(p + "attention/linear_1/weight"), f(p + "attention/linear_1/bias")
                sd[q + "encoder_attn.q_proj.weight"], sd[q + "encoder_attn.q_proj.bias"] = f(p + "attention/linear_0/weight"), f(p + "attention/linear_0/bias")
                sd[q + "encoder_attn.k_proj.weight"], sd[q + "encoder_attn.v_proj.weight"], sd[q + "encoder_attn.v_proj.bias"] = kv[:d], kv[d:], bkv[d:]
                sd[q + "encoder_attn.out_proj.weight"], sd[q + "encoder_attn.out_proj.bias"] = f(p + "attention/linear_2/weight"), f(p + "attention/linear_2/bias")
                sd[q + "encoder_attn_layer_norm.weight"], sd[q + "encoder_attn_layer_norm.bias"] = f(p + "attention/layer_norm/gamma"), f(p + "attention/layer_norm/beta")
            sd[q + "final_layer_norm.weight"], sd[q + "final_layer_norm.bias"] = f(p + "ffn/layer_norm/gamma"), f(p + "ffn/layer_norm/beta")
            sd[q + "fc1.weight"], sd[q + "fc1.bias"] = f(p + "ffn/linear_0/weight"), f(p + "ffn/linear_0/bias")
            sd[q + "fc2.weight"], sd[q + "fc2.bias"] = f(p + "ffn/linear_1/weight"), f(p + "ffn/linear_1/bias")
    with torch.device("meta"):
        hf = WhisperForConditionalGeneration(cfg)
    hf.load_state_dict(sd, strict=False, assign=True)
    hf.proj_out.weight = hf.model.decoder.embed_tokens.weight
    assert not any(t.is_meta for t in hf.parameters()), [n for n, t in hf.named_parameters() if t.is_meta]
    return hf.eval()


GEOMS = {
    "large-v3": dict(size="large-v3", drop_dec=None),
    "large-v3-turbo": dict(size="large-v3-turbo", drop_dec=None),
    "distil-32x2": dict(size="large", drop_dec=2),
}


@pytest.fixture(scope="module")
def geom(request, golden_dir, lib):
    from wis_hip import ctranslate2 as ct2, weights as W
    g = GEOMS[request.param]
    w = W.synthetic_weights(g["size"], seed=77, std=0.02, emb_std=0.06, ln_jitter=0.1)
    if g["drop_dec"]:
        w = {k: v for k, v in w.items() if not (k.split("/")[1][6:].isdigit() and k.startswith("decoder/layer_") and int(k.split("/")[1][6:]) >= g["drop_dec"])}
    a0 = W.arch_from_weights(w, 20)
    hf = _hf_from_ct2(w, a0)
    del w
    # the engine gets the checkpoint through the Hugging Face loader: HF state dict -> CT2 names -> arch_from_weights
    w2 = W.from_hf_state_dict({k: v.detach().numpy() for k, v in hf.state_dict().items()})
    a = W.arch_from_weights(w2, 20)
    assert (a["n_enc_layers"], a["n_dec_layers"], a["n_mels"], a["n_vocab"]) == (a0["n_enc_layers"], a0["n_dec_layers"], a0["n_mels"], a0["n_vocab"])
    model = ct2.Whisper("unused", weights=w2, arch=a, max_batch=2, max_beam=5)
    del w2
    gc.collect()
    pcm = _clip(golden_dir, "3sec")
    mel = _logmel(lib, pcm, a["n_mels"])
    with torch.no_grad():
        enc = hf.model.encoder(torch.from_numpy(mel)).last_hidden_state
    yield request.param, hf, model, a, mel, enc
    model.close()
    del model, hf
    gc.collect()


def _masked_logprobs(lg, step, sup, beg):
    lg = lg.astype(np.float64).copy()
    lg[sup] = -np.inf
    if step == 0:
        lg[beg] = -np.inf
    m = lg.max()
    return lg - (m + np.log(np.exp(lg - m).sum())), lg


def _hf_step_logits(hf, enc, seq):
    with torch.no_grad():
        h = hf.model.decoder(input_ids=torch.tensor([seq]), encoder_hidden_states=enc).last_hidden_state
        return hf.proj_out(h)[0].numpy()


@pytest.mark.parametrize("geom", list(GEOMS), indirect=True)
def test_engine_matches_hf_at_v3_geometries(geom, lib):
    from wis_hip import _lib, ctranslate2 as ct2
    name, hf, model, a, mel, enc = geom
    h, V, d = model._replicas[0].handle, a["n_vocab"], a["d_model"]
    st = model.special
    out = np.zeros((1, 1500, d), np.float32)
    _lib.check(lib.wis_debug_encode(h, _lib.ptr(mel), _lib.WIS_IN_MEL_HOST, 1, out.ctypes.data_as(C.POINTER(C.c_float))))
    e = enc.numpy()
    rel = np.linalg.norm(out - e) / np.linalg.norm(e)
    print(f"[{name}] encoder vs HF fp32: rel-L2 {rel:.3e}")
    assert rel <= 2e-3
    prompt = [st.sot, st.lang_ids[0], st.transcribe, st.notimestamps]
    rng = np.random.default_rng(5)
    T = 16
    dec_in = np.ascontiguousarray(np.concatenate([np.array([prompt], np.int32), rng.integers(0, 50000, size=(1, T - 4)).astype(np.int32)], axis=1))
    exp = _hf_step_logits(hf, enc, dec_in[0].tolist())
    one = np.zeros((1, T, V), np.float32)
    _lib.check(lib.wis_debug_logits(h, _lib.ptr(mel), _lib.WIS_IN_MEL_HOST, 1, dec_in.ctypes.data_as(C.POINTER(C.c_int32)), T, one.ctypes.data_as(C.POINTER(C.c_float))))
    rows = np.zeros((1, T, V), np.float32)
    _lib.check(lib.wis_debug_logits_rows(h, _lib.ptr(mel), _lib.WIS_IN_MEL_HOST, 1, dec_in.ctypes.data_as(C.POINTER(C.c_int32)), T, 16,
                                         rows.ctypes.data_as(C.POINTER(C.c_float))))
    for route, lg in (("one-row", one[0]), ("batched-row (16 rows)", rows[0])):
        mx = np.abs(lg - exp).max()
        print(f"[{name}] {route} teacher-forced logits vs HF: max abs {mx:.3e} (logit std {exp.std():.2f})")
        assert mx <= 5e-2
    sup, beg = model.decode_config.get("suppress_ids") or st.default_suppress_ids(), [220, st.eot]
    # greedy == host greedy on HF logits (a flip only at a near-tie)
    S = 8
    res = model.generate(ct2.StorageView.from_array(mel), [prompt], beam_size=1, max_length=2 * S + 8, fixed_new_tokens=S)[0].sequences_ids[0]
    seq = list(prompt)
    for t, tok in enumerate(res):
        lp, ml = _masked_logprobs(_hf_step_logits(hf, enc, seq)[-1], t, sup, beg)
        order = np.argsort(ml)
        if int(order[-1]) != tok:
            assert ml[order[-1]] - ml[tok] < 0.05, (t, int(order[-1]), tok)
        seq.append(tok)
    print(f"[{name}] greedy: {len(res)} ids follow the HF arg-max chain")
    # beam 5: the engine's hypothesis against the host beam search (oracle/whisper_ref.py's search over this decoder, fed HF's encoder
    # output); a difference must be a near-tie of the two hypotheses rescored with HF
    from oracle.whisper_ref import WhisperRef
    from wis_hip import weights as W
    wd = W.from_hf_state_dict({k: v.detach().numpy() for k, v in hf.state_dict().items() if ".decoder." in k or "encoder.conv" in k or
                               "encoder.layer_norm" in k or "encoder.embed_positions" in k or "encoder.layers.0." in k})
    ref = WhisperRef(wd, d, a["n_dec_layers"], a["n_heads"], n_vocab=V)
    got = model.generate(ct2.StorageView.from_array(mel), [prompt], beam_size=5, fixed_new_tokens=S, return_scores=True)[0]
    ids, _score = ref.generate(None, prompt, beam_size=5, suppress_ids=sup, suppress_begin=beg, fixed_new=S, memory=e[0])

    def rescore(hyp):
        lg = _hf_step_logits(hf, enc, list(prompt) + list(hyp))
        return sum(_masked_logprobs(lg[len(prompt) - 1 + t], t, sup, beg)[0][tok] for t, tok in enumerate(hyp))
    eng = got.sequences_ids[0]
    if list(eng) != list(ids):
        a_s, b_s = rescore(eng), rescore(ids)
        print(f"[{name}] beam 5 differs from the host search: HF rescoring {a_s:.4f} vs {b_s:.4f}")
        assert abs(a_s - b_s) < 0.05
    else:
        print(f"[{name}] beam 5 ids identical to the host search")
    if name == "large-v3-turbo":
        # language detection over the 100 languages, against HF's <|startoftranscript|> logits
        probs = model.detect_language(ct2.StorageView.from_array(mel))[0]
        assert len(probs) == 100
        lg = _hf_step_logits(hf, enc, [st.sot])[-1][st.lang_ids].astype(np.float64)
        p = np.exp(lg - lg.max())
        p /= p.sum()
        got_p = {c.strip("<|>"): v for c, v in probs}
        err = max(abs(got_p[c] - p[i]) for i, c in enumerate(st.lang_codes))
        print(f"[{name}] detect_language over 100 languages vs HF: max abs {err:.2e}")
        assert err <= 2e-3 and "yue" in got_p


def test_v3_timestamps_int8_and_rest(golden_dir, lib):
    import asyncio
    import httpx
    from wis_hip import _lib, ctranslate2 as ct2
    from wis_hip.server import create_app
    from wis_hip.settings import APISettings
    from wis_hip.whisper import WhisperModels
    pcm = _clip(golden_dir, "3sec")
    mel = _logmel(lib, pcm, 128)
    model = ct2.Whisper("synthetic:large-v3-turbo", max_batch=2, max_beam=5)
    st = model.special
    assert (st.transcribe, st.nospeech, st.notimestamps, st.timestamp_begin) == (V3["transcribe"], V3["nospeech"], V3["notimestamps"], V3["timestamp_begin"])
    # timestamps: rules at timestamp_begin = 50365 - the first id is a timestamp, and no id of [<|endoftext|> + 1, 50365) is emitted
    for beam in (1, 5):
        r = model.generate(ct2.StorageView.from_array(mel), [[st.sot, st.lang_ids[0], st.transcribe]], beam_size=beam, return_no_speech_prob=True,
                           max_length=64)[0]
        ids = r.sequences_ids[0]
        print(f"timestamps beam {beam}: {ids[:12]} ... ({len(ids)} ids), no_speech_prob {r.no_speech_prob:.3e}")
        assert ids and st.timestamp_begin <= ids[0] <= st.timestamp_begin + 50
        assert all(t < EOT or t >= st.timestamp_begin for t in ids)
        assert 0.0 <= r.no_speech_prob <= 1.0
    model.close()
    # int8_float16 at the turbo geometry
    q = ct2.Whisper("synthetic:large-v3-turbo", compute_type="int8_float16", max_batch=2, max_beam=5)
    prompt = [st.sot, st.lang_ids[0], st.transcribe, st.notimestamps]
    r = q.generate(ct2.StorageView.from_array(np.ascontiguousarray(np.stack([mel[0], mel[0]]))), [prompt] * 2, beam_size=5, fixed_new_tokens=8)
    assert [len(x.sequences_ids[0]) for x in r] == [8, 8] and r[0].sequences_ids == r[1].sequences_ids
    assert all(0 <= t < EOT for t in r[0].sequences_ids[0])
    q.close()
    del q
    gc.collect()
    # REST: /api/asr?model=large-v3-turbo on synthetic weights answers what generate answers
    s = APISettings()
    s.whisper_model_path = "synthetic:{size}"
    models = WhisperModels(s, device_index=[0])
    app = create_app(models=models)
    import io
    import wave
    buf = io.BytesIO()
    with wave.open(buf, "wb") as wv:
        wv.setnchannels(1), wv.setsampwidth(2), wv.setframerate(16000)
        wv.writeframes((np.clip(pcm[:48000], -1, 1) * 32767).astype("<i2").tobytes())
    bd = "xYzBoundary123"
    body = (f"--{bd}\r\nContent-Disposition: form-data; name=\"audio_file\"; filename=\"a.wav\"\r\nContent-Type: application/octet-stream\r\n\r\n").encode() \
        + buf.getvalue() + f"\r\n--{bd}--\r\n".encode()

    async def go():
        async with httpx.AsyncClient(transport=httpx.ASGITransport(app=app), base_url="http://wis") as c:
            return await c.post("/api/asr?model=large-v3-turbo&force_language=en&beam_size=1",
                                content=body, headers={"content-type": f"multipart/form-data; boundary={bd}"})
    r = asyncio.run(go())
    assert r.status_code == 200, r.text
    from wis_hip import audio
    x, _ = audio.load_audio(io.BytesIO(buf.getvalue()))
    eng = models.get("large-v3-turbo")
    want = eng.generate(ct2.StorageView.from_array(np.ascontiguousarray(audio.pad_or_trim(x)[None], np.float32)), [prompt], beam_size=1,
                        fixed_new_tokens=s.fixed_new_tokens, input_kind=_lib.WIS_IN_PCM_HOST)[0].sequences_ids[0]
    print("REST large-v3-turbo:", r.json()["text"][:80])
    assert r.json()["text"] == " ".join(str(t) for t in want)
    eng.close()
