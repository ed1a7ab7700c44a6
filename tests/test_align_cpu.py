"""No GPU: the alignment reference (tests/align_ref.py) against transformers' own _median_filter / _dynamic_time_warping, the planted
alignment with K rounded to f16, word grouping and punctuation merging (wis_hip/whisper.py against hand-written token lists and against
align_ref), the alignment_heads loader round trip, and ?word_timestamps=true on the fake-engine server."""
import json
import os

import numpy as np
import pytest
import torch

import align_ref as R


@pytest.mark.parametrize("N,M,quant", [(1, 1, 0), (1, 9, 0), (7, 1, 0), (20, 50, 0), (50, 20, 0), (30, 120, 3), (40, 90, 2), (25, 60, 1)])
def test_ref_dtw_equals_transformers(N, M, quant):
    from transformers.models.whisper.generation_whisper import _dynamic_time_warping
    rng = np.random.default_rng(N * 131 + M + quant)
    x = rng.standard_normal((N, M)).astype(np.float32)
    if quant:
        x = (np.round(x * quant) / quant).astype(np.float32)
    want = _dynamic_time_warping(x.astype(np.float64).copy())
    for f in (R.dtw, R.dtw_fast):
        got = f(x)
        assert np.array_equal(got[0], np.asarray(want[0])) and np.array_equal(got[1], np.asarray(want[1]))


@pytest.mark.parametrize("F,width", [(1, 7), (3, 7), (4, 7), (50, 7), (50, 1), (40, 21)])
def test_ref_median_and_matrix_equal_transformers(F, width):
    from transformers.models.whisper.generation_whisper import _median_filter
    rng = np.random.default_rng(F + width)
    w = rng.random((3, 9, F))
    w[0, :, : F // 2] = np.round(w[0, :, : F // 2] * 4) / 4      # ties
    assert np.array_equal(R.median_filter(w, width), _median_filter(torch.tensor(w), width).numpy())
    t = torch.tensor(w)[None]
    std, mean = torch.std_mean(t, dim=-2, keepdim=True, unbiased=False)
    want = -_median_filter((t - mean) / std, width).mean(1)[0].numpy()
    assert np.allclose(R.matrix(w, width), want, rtol=0, atol=1e-12)


@pytest.mark.parametrize("N,F,Hn", [(20, 400, 1), (12, 750, 2), (100, 1500, 3), (60, 1500, 6)])
def test_planted_alignment_reference_alone(N, F, Hn):
    rng = np.random.default_rng(N + F + Hn)
    q, K, f = R.planted_inputs(rng, N, F, Hn)
    for Kr in (K.astype(np.float64), K.astype(np.float16)):
        x = R.matrix(R.attention_weights(q, Kr)[:, :, :F], 7).astype(np.float32)
        ti, fi = R.dtw_fast(x)
        assert np.array_equal(np.rint(R.jump_times(ti, fi) * 50).astype(np.int64), f[:-1])


# a byte-level toy vocabulary: ids 0..255 are single bytes, 300.. are multi-byte pieces
_PIECES = {300: b" Hello", 301: b",", 302: b" wor", 303: b"ld", 304: b"!", 305: b" (", 306: b"ok", 307: b")", 308: b" ok", 310: "日".encode()[:2], 311: "日".encode()[2:] + "本".encode(),
           312: "語".encode()}
EOT = 1000


def _decode(ids):
    return b"".join(_PIECES.get(int(t), b"") for t in ids if int(t) < EOT).decode("utf-8", errors="replace")


def test_word_grouping_and_punctuation():
    from wis_hip import whisper as Wh
    toks = [300, 301, 302, 303, 304, 305, 306, 307]
    for mod in (Wh, R):
        words, wt = mod.split_to_word_tokens(toks, _decode, "en", EOT)
        assert words == [" Hello", ",", " world", "!", " (ok", ")"] and wt[2] == [302, 303]
    words, wt = Wh.merge_punctuations(*Wh.split_to_word_tokens(toks, _decode, "en", EOT))
    assert words == [" Hello,", " world!", " (ok)"] and wt == [[300, 301], [302, 303, 304], [305, 306, 307]]
    rw, rt = R.merge_punctuations(*R.split_to_word_tokens(toks, _decode, "en", EOT))
    assert [w for w in rw if w] == words and [t for t in rt if t] == wt
    words, wt = Wh.merge_punctuations(*Wh.split_to_word_tokens([300, 305, 308, 307], _decode, "en", EOT))      # opening punctuation joins the next word
    assert words == [" Hello", " ( ok)"] and wt == [[300], [305, 308, 307]]
    # a character split over two tokens stays with the piece that completes it; a language without spaces: one word per unicode piece
    jp = [310, 311, 312]
    for mod in (Wh, R):
        words, wt = mod.split_to_word_tokens(jp, _decode, "ja", EOT)
        assert words == ["日本", "語"] and wt == [[310, 311], [312]]
    words, wt = Wh.split_to_word_tokens(jp, _decode, "en", EOT)
    assert "".join(words) == "日本語" and sum(wt, []) == jp


def test_words_from_alignment_times():
    from wis_hip import whisper as Wh
    from wis_hip import weights as W

    class Tok:
        decode = staticmethod(_decode)
    st = W.special_tokens(W.N_VOCAB)
    segs = [{"start": 0.0, "end": 1.0, "text": "Hello, world!", "tokens": [300, 301, 302, 303, 304]}, {"start": 1.0, "end": 2.0, "text": "(ok)", "tokens": [305, 306, 307]}]
    path = [(0, 0), (0, 1), (1, 2), (2, 10), (2, 11), (3, 20), (4, 30), (5, 40), (6, 45), (7, 50), (8, 60), (8, 61)]
    probs = [0.5, 0.7, 0.2, 0.4, 0.6, 0.9, 0.8, 0.7]
    Wh.words_from_alignment(segs, path, probs, Tok, "en", st, 2.0)
    w0, w1 = segs[0]["words"], segs[1]["words"]
    assert [w["word"] for w in w0] == [" Hello,", " world!"] and [w["word"] for w in w1] == [" (ok)"]
    assert (w0[0]["start"], w0[0]["end"], w0[1]["start"], w0[1]["end"]) == (0.0, 0.2, 0.2, 0.8) and (w1[0]["start"], w1[0]["end"]) == (0.8, 1.2)
    assert abs(w0[0]["probability"] - 0.6) < 1e-9 and abs(w1[0]["probability"] - 0.8) < 1e-9
    want = R.word_timings([300, 301, 302, 303, 304], [p[0] for p in path[:8]] + [5], [p[1] for p in path[:8]] + [40], probs[:5], _decode, "en", EOT)
    assert [(w["word"], w["start"], w["end"]) for w in w0] == [(a, b, c) for a, b, c, _ in want]


def test_alignment_heads_survive_the_loaders(tmp_path):
    from wis_hip import weights as W
    assert W.normalize_alignment_heads(None) == [] and W.normalize_alignment_heads([[3, 1], [2, 0], [3, 1]]) == [[2, 0], [3, 1]]
    w = W.synthetic_weights("tiny", seed=1)
    for heads in ([[3, 1], [2, 5]], None):
        d = tmp_path / ("ct2_" + ("h" if heads else "none"))
        os.makedirs(d)
        W.write_ct2_model_bin(str(d / "model.bin"), w, aliases={"decoder/projection/weight": "decoder/embeddings/weight"})
        cfg = {"suppress_ids": [1], "suppress_ids_begin": [220, 50257], "lang_ids": list(range(50259, 50358))}
        if heads:
            cfg["alignment_heads"] = heads
        (d / "config.json").write_text(json.dumps(cfg))
        _, _, got = W.load_model_dir(str(d))
        assert got.get("alignment_heads", []) == (sorted(heads) if heads else [])


def test_alignment_heads_from_hf_through_convert(tmp_path):
    """generation_config.json -> load_hf_dir -> convert_hf_to_ct2_dir -> config.json -> load_model_dir; an HF directory without the
    list converts to one that loads with the default; a model.bin that carries the pairs as `decoder/alignment_heads` is read too."""
    from test_loaders import hf_checkpoint
    from wis_hip import weights as W
    heads = [[1, 1], [0, 1], [1, 0]]
    for name, hd in (("with", heads), ("without", None)):
        src, dst = tmp_path / f"hf_{name}", tmp_path / f"ct2_{name}"
        os.makedirs(src)
        hf_checkpoint(str(src))
        gj = json.loads((src / "generation_config.json").read_text())
        if hd:
            gj["alignment_heads"] = hd
        (src / "generation_config.json").write_text(json.dumps(gj))
        _, _, cfg = W.load_hf_dir(str(src))
        assert cfg.get("alignment_heads", []) == (sorted(hd) if hd else [])
        W.convert_hf_to_ct2_dir(str(src), str(dst))
        assert json.loads((dst / "config.json").read_text())["alignment_heads"] == (sorted(hd) if hd else [])
        _, _, cfg2 = W.load_model_dir(str(dst))
        assert cfg2.get("alignment_heads", []) == (sorted(hd) if hd else [])
    # the pairs as an attribute of model.bin, no list in config.json
    w, attrs = W.read_ct2_model_bin(str(tmp_path / "ct2_without" / "model.bin"), return_attrs=True)
    d = tmp_path / "ct2_attr"
    os.makedirs(d)
    extra = dict(w)
    extra["decoder/alignment_heads"] = np.array([[1, 0], [1, 1]], np.int16)
    W.write_ct2_model_bin(str(d / "model.bin"), extra, aliases={"decoder/projection/weight": "decoder/embeddings/weight"})
    _, _, cfg3 = W.load_model_dir(str(d))
    assert cfg3.get("alignment_heads") == [[1, 0], [1, 1]]


def test_server_word_timestamps_with_the_fake_engine(golden_dir, monkeypatch):
    """/api/asr on the fake engine (tools/fake_engine_app.py: everything but the engine is real): word_timestamps=true on a model without a
    tokenizer vocabulary is a 400; with an align stand-in and a vocabulary the segments carry words; without the parameter the response has
    the keys and values it had before."""
    import asyncio
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(golden_dir), "..", "tools"))
    import fake_engine_app
    from test_server_cpu import _client, _multipart
    from wis_hip import ctranslate2 as ct2
    monkeypatch.setenv("WIS_FAKE_MS", "1")
    monkeypatch.setenv("WIS_FAKE_MS_PER_UTT", "0")
    saved = ct2._generate_chunk
    try:
        app = fake_engine_app.create_app()
        with open(os.path.join(golden_dir, "clips", "3sec.flac"), "rb") as f:
            body, hdr = _multipart(f.read())

        async def go(query):
            async with _client(app) as c:
                return await c.post("/api/asr" + query, content=body, headers=hdr)
        plain = asyncio.run(go("?model=large")).json()
        assert set(plain) == {"infer_time", "infer_speedup", "audio_duration", "language", "text"} and "segments" not in plain
        r = asyncio.run(go("?model=large&word_timestamps=true"))
        assert r.status_code == 400 and "vocabulary" in r.json()["error"]

        class Tok:
            has_vocabulary, all_special_ids = True, []
            decode = staticmethod(lambda ids: "".join(f" w{int(t)}" for t in ids if int(t) < 50257))
        models = app.state.wis["models"]
        models.tokenizers["large"] = Tok()
        model = models.get("large")
        model.align = lambda feats, start, texts, frames, **kw: [ct2.WhisperAlignmentResult([(i, 5 * i) for i in range(len(t) + 1)], [0.5] * len(t)) for t in texts]
        steady = lambda j: {k: v for k, v in j.items() if k not in ("infer_time", "infer_speedup")}
        plain = asyncio.run(go("?model=large")).json()      # (with the stand-in vocabulary)
        out = asyncio.run(go("?model=large&word_timestamps=true")).json()
        assert out["segments"] and all(sg["words"] for sg in out["segments"])
        for sg in out["segments"]:
            assert set(sg) == {"start", "end", "text", "words"}
            assert "".join(w["word"] for w in sg["words"]).strip() == sg["text"]
            assert all(set(w) == {"word", "start", "end", "probability"} and 0 <= w["start"] <= w["end"] <= 3.84 for w in sg["words"])
        assert {k: v for k, v in steady(out).items() if k != "segments"} == steady(plain)
        again = asyncio.run(go("?model=large"))
        assert steady(again.json()) == steady(plain) and "segments" not in again.json()
        ts = asyncio.run(go("?model=large&timestamps=true")).json()
        assert all("words" not in sg for sg in ts["segments"])
        # /api/willow: the same parameter, the same words
        with open(os.path.join(golden_dir, "clips", "3sec.flac"), "rb") as f:
            flac = f.read()

        async def willow(query):
            async with _client(app) as c:
                return await c.post("/api/willow" + query, content=flac, headers={"x-audio-codec": "flac"})
        wplain = asyncio.run(willow("?model=large")).json()
        assert wplain == {"language": plain["language"], "text": plain["text"]}
        wout = asyncio.run(willow("?model=large&word_timestamps=true")).json()
        assert wout["segments"] == out["segments"] and {k: v for k, v in wout.items() if k != "segments"} == wplain
        del models.tokenizers["large"]
        r = asyncio.run(willow("?model=large&word_timestamps=true"))
        assert r.status_code == 400 and "vocabulary" in r.json()["error"]
    finally:
        ct2._generate_chunk = saved
