"""-m gpu: wis_align / wis_debug_align_matrix / ctranslate2.Whisper.align on whole seeded models - tiny, base, large-v2 (the 320-head
default) and large-v3-turbo (4 decoder layers, 128 mel bins) - against transformers (fp32, CPU, the same f16-rounded weights;
_hf_from_ct2 of test_gpu_v3.py), then do_whisper(word_timestamps=True) and /api/asr|/api/willow?word_timestamps=true on a golden clip.

Matrix: the reference takes the alignment heads' cross-attention queries and keys from the HF decoder (hooks on encoder_attn.q_proj /
k_proj), forms softmax(q.K^T / 8) in float64 and feeds align_ref.matrix.  e = max |GPU - reference|; e_f16 = what rounding q and K to
f16 (the engine's storage / MFMA operand format) costs the reference itself; bound 4 e_f16 + 3e-3 max|matrix|.  Seeded weights give
nearly flat attention and a DTW path is discontinuous in its input, so paths are not compared index by index: the GPU path must be a
valid warping path whose cost ON THE REFERENCE MATRIX is within 2 (N + M - 1) e of the reference optimum (|A - B| <= e on every cell).

Batch of 8: eight DIFFERENT windows (two clips, shifted / reversed / mixed, ragged frame counts) with ragged texts.  Utterance 0 is the
HF-checked case.  Every utterance is compared with its own single call: the matrices within the limit on e of the HF case with the same
token count (the batched encoder / decoder GEMM routes give other bits), the batch path by the same cost rule with the single call's
matrix as A and e = the measured difference, the token probabilities within the 5e-2 log-prob tolerance of test_gpu_v3.py."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import align_ref as R
from test_gpu_v3 import _hf_from_ct2

pytestmark = pytest.mark.gpu
_i32 = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))
_f32 = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))


def _windows(golden_dir, n_mels):
    """eight different 30 s windows [8][n_mels][3000] and their mel frame counts"""
    from wis_hip import audio
    a, _ = audio.load_audio(os.path.join(golden_dir, "clips", "3sec.flac"))
    b, _ = audio.load_audio(os.path.join(golden_dir, "clips", "10sec.flac"))
    pcms = [a, b, a[::-1].copy(), b[8000:], np.concatenate([a, 0.5 * a[::-1]]), b[::-1].copy(), a[16000:], 0.5 * b[:len(a)] + 0.5 * a]
    mels = np.stack([audio.log_mel_spectrogram(audio.pad_or_trim(p.astype(np.float32)), n_mels=n_mels).numpy() for p in pcms]).astype(np.float32)
    return np.ascontiguousarray(mels), [int(min(3000, -(-len(p) // 160))) for p in pcms]


@pytest.fixture(scope="module", params=["tiny", "base", "large-v2", "large-v3-turbo"])
def rig(request, golden_dir, lib):
    from wis_hip import ctranslate2 as ct2, weights as W
    size = request.param
    w = W.synthetic_weights(size, seed=77, emb_std=0.06, ln_jitter=0.1)
    a = W.arch(size)
    model = ct2.Whisper("unused", weights=w, arch=a, max_batch=8, max_beam=1, inter_threads=2, replicas_per_device=2)
    hf = _hf_from_ct2(w, a)
    mels, frames = _windows(golden_dir, a["n_mels"])
    torch.set_num_threads(16)
    with torch.no_grad():
        enc = hf.model.encoder(torch.from_numpy(mels[0:1])).last_hidden_state
    yield size, model, hf, a, mels, frames, enc
    model.close()


def _hf_ref(hf, a, enc, seq, heads):
    """float64 q [H][len][64] (scaled by 1/8), K [H][1500][64] of the chosen (layer, head) pairs + the logits of every position"""
    cap = {}
    hooks = []
    for l, layer in enumerate(hf.model.decoder.layers):
        hooks.append(layer.encoder_attn.q_proj.register_forward_hook(lambda m, i, o, l=l: cap.__setitem__(("q", l), o.detach()[0].double().numpy())))
        hooks.append(layer.encoder_attn.k_proj.register_forward_hook(lambda m, i, o, l=l: cap.__setitem__(("k", l), o.detach()[0].double().numpy())))
    with torch.no_grad():
        lg = hf(encoder_outputs=(enc,), decoder_input_ids=torch.tensor([seq])).logits[0].double().numpy()
    for h in hooks:
        h.remove()
    q = np.stack([cap[("q", l)][:, 64 * h:64 * h + 64] * 0.125 for l, h in heads])
    K = np.stack([cap[("k", l)][:, 64 * h:64 * h + 64] for l, h in heads])
    return q, K, lg


def _default_heads(a):
    return [(l, h) for l in range(a["n_dec_layers"] // 2, a["n_dec_layers"]) for h in range(a["n_heads"])]


def _check_path(x_ref, ti, fi, e):
    N, M = x_ref.shape
    assert (ti[0], fi[0]) == (0, 0) and (ti[-1], fi[-1]) == (N - 1, M - 1)
    steps = set(zip(np.diff(ti).tolist(), np.diff(fi).tolist()))
    assert steps <= {(1, 0), (0, 1), (1, 1)}, steps
    cost, opt = R.path_cost(x_ref, ti, fi), R.dtw_optimum(x_ref)
    print(f"   path cost on the reference matrix {cost:.4f}, optimum {opt:.4f}, slack {2 * (N + M - 1) * e:.4f}")
    assert cost <= opt + 2 * (N + M - 1) * e


@pytest.mark.parametrize("heads", ["explicit", "default"])
def test_align_matrix_path_and_probs(rig, heads, lib):
    from wis_hip import _lib
    size, model, hf, a, mels, frames, enc = rig
    mel = np.ascontiguousarray(mels[0:1])
    st = model.special
    sel = [(a["n_dec_layers"] - 1, 0), (a["n_dec_layers"] - 1, 3), (1, 2)] if heads == "explicit" else _default_heads(a)
    model._set_alignment_heads(sel if heads == "explicit" else None)
    sel = sorted(sel)
    start = np.array([st.sot, st.lang_ids[0], st.transcribe], np.int32)
    rng = np.random.default_rng(11)
    num_frames, width = frames[0], 7
    F = num_frames // 2
    h = model._replicas[0].handle
    texts = {n: rng.integers(0, 50000, size=n).astype(np.int32) for n in (30, 223, 5, 17)}
    mats = {}
    for n in (30, 223):
        text = texts[n]
        seq = start.tolist() + [st.notimestamps] + text.tolist()
        q, K, lg = _hf_ref(hf, a, enc, seq, sel)
        rows = slice(3, 3 + n + 1)
        ref = R.matrix(R.attention_weights(q[:, rows], K)[:, :, :F], width)
        ref16 = R.matrix(R.attention_weights(q[:, rows].astype(np.float16), K.astype(np.float16))[:, :, :F], width)
        out = np.zeros((n + 1, F), np.float32)
        ln, nf = np.array([n], np.int32), np.array([num_frames], np.int32)
        _lib.check(lib.wis_debug_align_matrix(h, _lib.ptr(mel), _lib.WIS_IN_MEL_HOST, 1, _i32(start), 3, _i32(text), _i32(ln), _i32(nf), width, _f32(out)))
        e, e16, scale = np.abs(out - ref).max(), np.abs(ref16 - ref).max(), np.abs(ref).max()
        print(f"[{size} {heads}] {n} tokens: e {e:.3e}  e_f16 {e16:.3e}  max|x| {scale:.3f}")
        limit = 4 * e16 + 3e-3 * scale
        assert e <= limit, (e, e16, scale)
        mats[n] = (out, limit)
        res = model.align(mel, start.tolist(), [text.tolist()], [num_frames], median_filter_width=width)[0]
        ti, fi = np.array([p[0] for p in res.alignments]), np.array([p[1] for p in res.alignments])
        _check_path(ref, ti, fi, e)
        lp = lg[3:3 + n, :st.eot]
        lp = lp - lp.max(-1, keepdims=True)
        lp = lp - np.log(np.exp(lp).sum(-1, keepdims=True))
        want = lp[np.arange(n), text]
        got = np.log(np.asarray(res.text_token_probs, np.float64))
        print(f"[{size} {heads}] {n} tokens: token log-probs vs HF max abs {np.abs(got - want).max():.3e}")
        assert len(got) == n and np.abs(got - want).max() <= 5e-2
    # a ragged batch of 8 different windows against each utterance's own single call
    order = [30, 5, 223, 17, 30, 5, 17, 223]
    flat = np.ascontiguousarray(np.concatenate([texts[n] for n in order]))
    ln, nf = np.array(order, np.int32), np.array(frames, np.int32)
    Fs = [f // 2 for f in frames]
    out = np.zeros(sum((n + 1) * f for n, f in zip(order, Fs)), np.float32)
    _lib.check(lib.wis_debug_align_matrix(h, _lib.ptr(mels), _lib.WIS_IN_MEL_HOST, 8, _i32(start), 3, _i32(flat), _i32(ln), _i32(nf), width, _f32(out)))
    batch = model.align(mels, start.tolist(), [texts[n].tolist() for n in order], frames)
    lim = {30: mats[30][1], 223: mats[223][1], 5: mats[30][1], 17: mats[30][1]}
    o = 0
    for k, (n, f) in enumerate(zip(order, Fs)):
        got = out[o:o + (n + 1) * f].reshape(n + 1, f)
        o += (n + 1) * f
        one = np.zeros((n + 1, f), np.float32)
        l1, f1 = np.array([n], np.int32), np.array([frames[k]], np.int32)
        _lib.check(lib.wis_debug_align_matrix(h, _lib.ptr(np.ascontiguousarray(mels[k:k + 1])), _lib.WIS_IN_MEL_HOST, 1, _i32(start), 3, _i32(texts[n]), _i32(l1), _i32(f1), width, _f32(one)))
        dlt = float(np.abs(got - one).max())
        print(f"   batch of 8, utterance {k} ({n} tokens, {f} frames) vs its single call: max abs {dlt:.3e} (limit {lim[n]:.3e})")
        assert dlt <= lim[n], (k, n, dlt)
        if k == 0:
            assert np.abs(got - mats[30][0]).max() <= mats[30][1]
        single = model.align(np.ascontiguousarray(mels[k:k + 1]), start.tolist(), [texts[n].tolist()], [frames[k]])[0]
        ti, fi = np.array([p[0] for p in batch[k].alignments]), np.array([p[1] for p in batch[k].alignments])
        _check_path(one.astype(np.float64), ti, fi, dlt)
        assert len(batch[k].text_token_probs) == n
        assert np.abs(np.log(batch[k].text_token_probs) - np.log(single.text_token_probs)).max() <= 5e-2
        if k == 7:      # a second single call takes the same route: the same bits
            again = model.align(np.ascontiguousarray(mels[k:k + 1]), start.tolist(), [texts[n].tolist()], [frames[k]])[0]
            assert again.alignments == single.alignments and again.text_token_probs == single.text_token_probs
    # a clone carries the heads (replica 1 is wis_model_clone of replica 0)
    h2 = model._replicas[1].handle
    out2 = np.zeros((31, F), np.float32)
    F = num_frames // 2
    ln, nf = np.array([30], np.int32), np.array([num_frames], np.int32)
    _lib.check(lib.wis_debug_align_matrix(h2, _lib.ptr(mel), _lib.WIS_IN_MEL_HOST, 1, _i32(start), 3, _i32(texts[30]), _i32(ln), _i32(nf), width, _f32(out2)))
    assert np.abs(out2 - mats[30][0]).max() <= mats[30][1]
    # over-long text: 3 + 1 + 445 > 448
    long = rng.integers(0, 50000, size=445).astype(np.int32)
    ln = np.array([445], np.int32)
    rc = lib.wis_debug_align_matrix(h, _lib.ptr(mel), _lib.WIS_IN_MEL_HOST, 1, _i32(start), 3, _i32(long), _i32(ln), _i32(nf), width, _f32(np.zeros((446, F), np.float32)))
    assert rc == -1      # WIS_E_ARG
    with pytest.raises(ValueError):
        model.align(mel, start.tolist(), [long.tolist()], [num_frames])


def test_device_bytes_unchanged_until_first_align(lib):
    from wis_hip import ctranslate2 as ct2, weights as W
    w, a = W.synthetic_weights("tiny", seed=3), W.arch("tiny")
    m1 = ct2.Whisper("unused", weights=w, arch=a, max_batch=2, max_beam=1)
    h = m1._replicas[0].handle
    before = lib.wis_model_device_bytes(h)
    m1._set_alignment_heads([[3, 1]])
    assert lib.wis_model_device_bytes(h) == before
    mel = np.zeros((1, 80, 3000), np.float32)
    m1.align(mel, [50258, 50259, 50359], [[1, 2, 3]], [200])
    grown = lib.wis_model_device_bytes(h)
    assert grown > before
    m1._set_alignment_heads(None)      # a larger head set: the smaller buffers are released, not kept beside the new ones
    m1.align(mel, [50258, 50259, 50359], [[1, 2, 3]], [200])
    new_q, old_q = 2 * 12 * 448 * 128, 2 * 1 * 448 * 128      # [max_batch][heads][n_text_ctx][64] f16
    assert grown < lib.wis_model_device_bytes(h) <= grown + new_q - old_q + 4096
    m1.close()


class _Vocab:
    """stand-in vocabulary (no tokenizer.json ships with the repository): every text id is a word of its own"""
    has_vocabulary, all_special_ids = True, []
    decode = staticmethod(lambda ids: "".join(f" w{int(t)}" for t in ids if int(t) < 50257))


def test_do_whisper_and_endpoints_word_timestamps(golden_dir):
    import asyncio
    import httpx
    from wis_hip.server import create_app
    from wis_hip.settings import APISettings
    from wis_hip.whisper import WhisperModels, do_whisper
    for fuse in (True, False):
        s = APISettings()
        s.whisper_model_path = "synthetic:{size}"
        s.fixed_new_tokens = 14
        s.fuse_logmel = fuse
        models = WhisperModels(s, device_index=[0])
        models.get("tiny")
        models.tokenizers["tiny"] = _Vocab()
        clip = os.path.join(golden_dir, "clips", "3sec.flac")
        plain = do_whisper(clip, "tiny", 5, models=models)
        ts = do_whisper(clip, "tiny", 5, models=models, timestamps=True)
        wt = do_whisper(clip, "tiny", 5, models=models, word_timestamps=True)
        assert wt.tokens == ts.tokens and wt[1] == ts[1]
        assert [{k: v for k, v in sg.items() if k != "words"} for sg in wt.segments] == ts.segments

        def check(segments):
            assert segments
            last = 0.0
            for sg in segments:
                if sg["text"]:
                    assert sg["words"]
                assert "".join(w["word"] for w in sg["words"]).strip() == sg["text"]
                for w in sg["words"]:
                    assert 0.0 <= last <= w["start"] <= w["end"] <= 3.84 and 0.0 < w["probability"] <= 1.0
                    last = w["start"]
        check(wt.segments)
        app = create_app(models=models)
        flac = open(clip, "rb").read()
        b = "wisBoundary7"
        body = (f"--{b}\r\nContent-Disposition: form-data; name=\"audio_file\"; filename=\"3sec.flac\"\r\nContent-Type: audio/flac\r\n\r\n").encode() + flac + f"\r\n--{b}--\r\n".encode()
        hdr = {"content-type": f"multipart/form-data; boundary={b}"}

        async def go():
            async with httpx.AsyncClient(transport=httpx.ASGITransport(app=app), base_url="http://wis", timeout=120) as c:
                r0 = await c.post("/api/asr?model=tiny&beam_size=5&detect_language=False", content=body, headers=hdr)
                r1 = await c.post("/api/asr?model=tiny&beam_size=5&detect_language=False&word_timestamps=true", content=body, headers=hdr)
                r2 = await c.post("/api/asr?model=tiny&beam_size=5&detect_language=False", content=body, headers=hdr)
                w1 = await c.post("/api/willow?model=tiny&beam_size=5&word_timestamps=true", content=flac, headers={"x-audio-codec": "flac"})
                w0 = await c.post("/api/willow?model=tiny&beam_size=5", content=flac, headers={"x-audio-codec": "flac"})
                return r0, r1, r2, w1, w0
        r0, r1, r2, w1, w0 = asyncio.run(go())
        assert all(r.status_code == 200 for r in (r0, r1, r2, w1, w0)), [r.text for r in (r0, r1, r2, w1, w0)]
        steady = lambda j: {k: v for k, v in j.items() if k not in ("infer_time", "infer_speedup")}
        assert steady(r0.json()) == steady(r2.json()) == {"audio_duration": 3840, "language": "en", "text": plain[1]}
        assert w0.json() == {"language": "en", "text": plain[1]}
        check(r1.json()["segments"])
        assert r1.json()["segments"] == wt.segments == w1.json()["segments"] and r1.json()["text"] == ts[1]
        model = models.get("tiny")
        model.close()
