"""gpu: long-form transcription end to end on seeded tiny weights - do_whisper(long_form="seek") over a 65 s recording: the loop ends, its seeks
strictly increase, its segments are monotone and inside the recording, and every window's tokens equal a plain `generate` call on that window's
features copied to the host with the same prompt (the loop adds nothing to the decode).  long_form="chunk" is the request as it always was.
One case with the temperature fallback and one with word timestamps (a stand-in vocabulary: every text id a word of its own): every word
lies inside its segment, segment start <= word start <= word end <= segment end, and the words move no segment."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "willow-inference-server_amd"))

pytestmark = pytest.mark.gpu
S = 12               # tokens per window: seeded weights never emit <|endoftext|>
DURATION = 65.0


class _Vocab:
    """stand-in vocabulary (no tokenizer.json ships with the repository): every text id is a word of its own"""
    has_vocabulary, all_special_ids = True, []
    decode = staticmethod(lambda ids: "".join(f" w{int(t)}" for t in ids if int(t) < 50257))


@pytest.fixture(scope="module")
def pcm():
    rng = np.random.default_rng(65)
    t = np.arange(int(16000 * DURATION))
    x = 0.2 * np.sin(2 * np.pi * 220.0 * t / 16000.0) * (1.0 + 0.5 * np.sin(2 * np.pi * 0.7 * t / 16000.0)) + 0.02 * rng.standard_normal(t.shape[0])
    x[300000:340000] = 0.0
    return x.astype(np.float32)


@pytest.fixture(scope="module")
def models():
    from wis_hip.settings import APISettings
    from wis_hip.whisper import WhisperModels
    s = APISettings()
    s.whisper_model_path = "synthetic:{size}"
    s.fixed_new_tokens = S
    m = WhisperModels(s, device_index=[0])
    m.get("tiny")
    yield m
    m.get("tiny").close()


def check_shape(r):
    seeks = [w["seek"] for w in r.seek]
    assert seeks and seeks[0] == 0 and all(b > a for a, b in zip(seeks, seeks[1:])) and seeks[-1] < 6500
    assert all(w["segment_size"] == min(3000, 6500 - w["seek"]) for w in r.seek)
    assert r.segments
    last = 0.0
    for sg in r.segments:
        assert last <= sg["start"] <= sg["end"] <= DURATION, (last, sg)
        last = sg["end"]
    assert r[5] == 65000 and r[1] == " ".join(sg["text"] for sg in r.segments if sg["text"])
    return seeks


def test_seek_loop_adds_nothing_to_the_decode(models, pcm):
    from wis_hip import audio, ctranslate2 as ct2
    from wis_hip.whisper import do_whisper
    r = do_whisper(pcm, "tiny", 5, "transcribe", False, "en", models=models, long_form="seek", timestamps=True, no_speech_threshold=1e30)
    seeks = check_shape(r)
    print("seeks", seeks, "segments", [(sg["start"], sg["end"]) for sg in r.segments])
    model = models.get("tiny")
    beam = models.settings.long_beam_size
    with audio.LongMel(pcm, 80, 0) as lm:
        assert lm.frames == 6500
        feats = lm.window(seeks, to_host=True)
    for w, f in zip(r.seek, feats):
        assert not w["skipped"] and w["temperature"] == 0.0 and len(w["tokens"]) == S
        plain = model.generate(ct2.StorageView.from_array(np.ascontiguousarray(f[None])), [w["prompt"]], beam_size=beam, fixed_new_tokens=S, return_scores=True,
                               return_no_speech_prob=True)[0]
        assert [t for t in plain.sequences_ids[0] if t != 50257] == w["tokens"], f"window at seek {w['seek']}"
        assert abs(plain.no_speech_prob - w["no_speech_prob"]) < 1e-6
    # the prompt carries the text so far
    assert r.seek[0]["prompt"] == [50258, 50259, 50359]
    if len(r.seek) > 1 and len(r.seek[1]["prompt"]) > 3:
        text0 = [t for sg_t in [r.seek[0]["tokens"]] for t in sg_t if t < 50257]
        assert r.seek[1]["prompt"][0] == 50361 and set(r.seek[1]["prompt"][1:-3]) <= set(text0)
    # the same request without timestamps asked for: the same loop, the same text, no segments
    r2 = do_whisper(pcm, "tiny", 5, "transcribe", False, "en", models=models, long_form="seek", no_speech_threshold=1e30)
    assert r2.segments is None and r2[1] == r[1] and r2.tokens == r.tokens


def test_chunk_is_the_request_as_it_was(models, pcm):
    """long_form="chunk" against the chunked path rebuilt by hand from its parts: chunk_iter, pad_or_trim, the log-mel, one generate call per
    `concurrent_gpu_chunks` windows, find_longest_common_sequence"""
    from wis_hip import audio, ctranslate2 as ct2
    from wis_hip.whisper import do_whisper
    s, model = models.settings, models.get("tiny")
    a = do_whisper(pcm, "tiny", 5, "transcribe", False, "en", models=models)
    b = do_whisper(pcm, "tiny", 5, "transcribe", False, "en", models=models, long_form="chunk")
    assert a.tokens == b.tokens and a[1] == b[1] and a.segments is None and b.segments is None and a.seek is None and b.seek is None
    wins, strides = [], []
    for chunk, stride in audio.chunk_iter(pcm):
        wins.append(audio.pad_or_trim(chunk))
        strides.append(stride)
    assert len(wins) == 5
    feats = audio.log_mel_spectrogram(np.stack(wins), n_mels=80, device=0).numpy()
    prompt = [50258, 50259, 50359, 50363]
    results = []
    for i in range(0, len(wins), s.concurrent_gpu_chunks):
        batch = np.ascontiguousarray(feats[i:i + s.concurrent_gpu_chunks])
        results.extend(model.generate(ct2.StorageView.from_array(batch), [prompt] * len(batch), beam_size=s.long_beam_size, fixed_new_tokens=S))
    merged = audio.find_longest_common_sequence([(r.sequences_ids[0], st) for r, st in zip(results, strides)], models.tokenizer_for("tiny"))
    assert b.tokens == [int(t) for t in merged]
    assert b[1] == models.tokenizer_for("tiny").decode(b.tokens).strip() and b[5] == 65000
    for kw in (dict(timestamps=True), dict(word_timestamps=True), dict(temperatures=(0.0, 0.4))):
        with pytest.raises(ValueError, match="30 s"):
            do_whisper(pcm, "tiny", 5, "transcribe", False, "en", models=models, long_form="chunk", **kw)


def test_seek_with_the_temperature_fallback(models, pcm):
    from wis_hip.whisper import do_whisper
    r = do_whisper(pcm, "tiny", 5, "transcribe", False, "en", models=models, long_form="seek", timestamps=True, temperatures=(0.0, 0.4), best_of=3,
                   no_speech_threshold=1e30)
    check_shape(r)
    assert all(w["temperature"] in (0.0, 0.4) for w in r.seek) and r.fallback is not None and r.fallback["attempts"] in (1, 2)
    print("temperatures", [w["temperature"] for w in r.seek], "avg_logprob", [round(w["avg_logprob"], 2) for w in r.seek])


def test_seek_with_word_timestamps(models, pcm):
    from wis_hip.whisper import do_whisper
    models.tokenizers["tiny"] = _Vocab()
    try:
        r = do_whisper(pcm, "tiny", 5, "transcribe", False, "en", models=models, long_form="seek", word_timestamps=True, no_speech_threshold=1e30)
    finally:
        del models.tokenizers["tiny"]
    check_shape(r)
    plain = do_whisper(pcm, "tiny", 5, "transcribe", False, "en", models=models, long_form="seek", timestamps=True, no_speech_threshold=1e30)
    assert [(sg["start"], sg["end"]) for sg in r.segments] == [(sg["start"], sg["end"]) for sg in plain.segments]      # the words move no segment
    n_words = 0
    for sg in r.segments:
        assert "".join(w["word"] for w in sg["words"]).strip() == sg["text"]
        starts = [w["start"] for w in sg["words"]]
        assert starts == sorted(starts)
        for w in sg["words"]:
            assert sg["start"] <= w["start"] <= w["end"] <= sg["end"] and 0.0 < w["probability"] <= 1.0, (sg["start"], sg["end"], w)
        n_words += len(sg["words"])
    assert n_words > 0
