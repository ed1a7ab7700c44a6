"""gpu: uploads at 48 and 44.1 kHz through the public layers - load_audio(device=), do_whisper, do_sv, /api/asr and /api/willow -
with the resampling on the GPU (settings.resample_on_gpu) and on the host.  The fixtures are made here: the reference's 3.84 s clip
brought to the other rate by the host resampler, written as a 16-bit WAV."""
import asyncio
import ctypes as C
import io
import os
import sys
import wave

import numpy as np
import pytest
import torch  # noqa: F401  (before libwis_hip.so)

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from resample_ref import EPS32, bound, resample_ref  # noqa: E402

pytestmark = pytest.mark.gpu


def _wav_bytes(pcm, rate):
    s16 = np.clip(np.round(pcm * 32768.0), -32768, 32767).astype("<i2")
    f = io.BytesIO()
    with wave.open(f, "wb") as w:
        w.setparams((1, 2, rate, 0, "NONE", "NONE"))
        w.writeframes(s16.tobytes())
    return f.getvalue(), s16


def _decode(data):
    """the container's own samples and rate (wis_audio_decode, what load_audio resamples)"""
    from wis_hip import _lib
    lib = _lib.load()
    p, n, sr, md = C.POINTER(C.c_float)(), C.c_int64(), C.c_int(), C.c_int()
    _lib.check(lib.wis_audio_decode(data, len(data), C.byref(p), C.byref(n), C.byref(sr), C.byref(md)))
    try:
        return np.ctypeslib.as_array(p, shape=(n.value,)).copy(), sr.value
    finally:
        lib.wis_audio_free(p)


@pytest.fixture(scope="module")
def clips(golden_dir, tmp_path_factory):
    """{rate: (path, wav bytes, int16 samples, decoded f32 PCM at that rate)}"""
    from wis_hip import audio
    pcm, _ = audio.load_audio(os.path.join(golden_dir, "clips", "3sec.flac"))
    d = tmp_path_factory.mktemp("resample_e2e")
    out = {}
    for rate in (48000, 44100):
        data, s16 = _wav_bytes(audio.resample(pcm, 16000, rate), rate)
        path = str(d / f"3sec_{rate}.wav")
        with open(path, "wb") as f:
            f.write(data)
        x, sr = _decode(data)
        assert sr == rate and x.shape[0] == s16.shape[0]
        out[rate] = (path, data, s16, x)
    return out


@pytest.fixture(scope="module")
def models():
    from wis_hip.settings import APISettings
    from wis_hip.whisper import WhisperModels
    s = APISettings()
    s.whisper_model_path = "synthetic:{size}"
    s.max_batch = 8
    s.fixed_new_tokens = 12      # seeded weights never emit EOT by themselves
    s.resample_on_gpu = True
    return WhisperModels(s, device_index=[0])


@pytest.mark.parametrize("rate", [48000, 44100])
def test_load_audio_on_the_device_against_the_host(clips, rate):
    """host: an fp64 sum rounded to f32 once (2^-24 |y64|, plus the fp64 summation's T 2^-53 B); device: (T + 3) 2^-24 B"""
    from wis_hip import audio
    path, _, _, x = clips[rate]
    host, sr_h = audio.load_audio(path)
    dev, sr_d = audio.load_audio(path, device=0)
    assert sr_h == sr_d == 16000 and host.shape == dev.shape and dev.dtype == np.float32
    y64, B, T = resample_ref(x, rate)
    lim = bound(B, T) + EPS32 * np.abs(y64) + T * 2.0 ** -53 * B
    err = np.abs(dev.astype(np.float64) - host.astype(np.float64))
    print(f"{rate} Hz: worst |device - host| = {float((err / np.maximum(lim, 1e-300)).max()):.3f} of the bound")
    assert np.all(err <= lim)
    assert np.array_equal(dev, audio.resample_gpu(x, rate, 0))
    assert np.array_equal(host, audio.resample(x, rate))


def test_do_whisper_resamples_on_the_models_gpu(clips, models):
    from wis_hip import audio
    from wis_hip.whisper import do_whisper
    path, _, _, x = clips[48000]
    models.settings.resample_on_gpu = True
    got = do_whisper(path, "tiny", beam_size=1, models=models)
    want = do_whisper(audio.resample_gpu(x, 48000, 0), "tiny", beam_size=1, models=models)
    assert got.tokens == want.tokens and got[1] == want[1] and len(got.tokens) == 12
    assert got[5] == want[5] == 3840      # audio_duration: the file's
    try:
        models.settings.resample_on_gpu = False
        off = do_whisper(path, "tiny", beam_size=1, models=models)
        host = do_whisper(audio.resample(x, 48000), "tiny", beam_size=1, models=models)
        assert off.tokens == host.tokens and off[1] == host[1] and off[5] == 3840
    finally:
        models.settings.resample_on_gpu = True


def test_do_whisper_uses_no_device_when_the_setting_is_off(clips, models, monkeypatch):
    """the setting decides where the samples are made: on -> load_audio is handed the replica's device, off -> None"""
    from wis_hip import audio
    from wis_hip.whisper import do_whisper
    seen, real = [], audio.load_audio
    monkeypatch.setattr(audio, "load_audio", lambda f, device=None: (seen.append(device), real(f, device=device))[1])
    try:
        for on in (True, False):
            models.settings.resample_on_gpu = on
            do_whisper(clips[48000][0], "tiny", beam_size=1, models=models)
    finally:
        models.settings.resample_on_gpu = True
    assert seen == [models.get("tiny")._replicas[0].device, None]


def test_do_sv_resamples_on_the_verifiers_gpu(clips, tmp_path):
    from wis_hip import audio, sv
    path, _, _, x = clips[48000]

    class Recording(sv.SpeakerVerifier):
        def embed(self, pcm):
            self.heard = np.array(pcm, copy=True)
            return super().embed(pcm)

    v = Recording(sv.SYNTHETIC)
    try:
        dev_pcm = audio.resample_gpu(x, 48000, v.device)
        emb = v.embed(dev_pcm)
        np.save(str(tmp_path / "alice.npy"), emb / np.linalg.norm(emb))
        res = sv.do_sv(path, 0.5, v, str(tmp_path), resample_on_gpu=True)
        assert np.array_equal(v.heard, dev_pcm)
        assert res == sv.score(emb / max(float(np.linalg.norm(emb)), 1e-12), sv.load_speakers(str(tmp_path)), 0.5) and list(res) == ["alice"]
        sv.do_sv(path, 0.5, v, str(tmp_path), resample_on_gpu=False)
        assert np.array_equal(v.heard, audio.resample(x, 48000))
        p = sv.enroll("bob", path, str(tmp_path), verifier=v, resample_on_gpu=True)
        assert np.array_equal(v.heard, dev_pcm) and os.path.exists(p)
    finally:
        v.close()


def test_server_takes_48_khz_uploads(clips, models):
    import httpx
    from wis_hip.server import create_app
    from wis_hip.whisper import do_whisper
    models.settings.resample_on_gpu = True
    app = create_app(models=models)
    path, data, s16, _ = clips[48000]
    direct = do_whisper(path, "tiny", beam_size=1, models=models)
    b = "wisBoundary7"
    body = (f"--{b}\r\nContent-Disposition: form-data; name=\"audio_file\"; filename=\"a.wav\"\r\nContent-Type: audio/wav\r\n\r\n").encode() \
        + data + f"\r\n--{b}--\r\n".encode()

    async def go():
        async with httpx.AsyncClient(transport=httpx.ASGITransport(app=app), base_url="http://wis", timeout=120) as c:
            r = await c.post("/api/asr?model=tiny&beam_size=1&detect_language=False", content=body, headers={"content-type": f"multipart/form-data; boundary={b}"})
            assert r.status_code == 200, r.text
            assert r.json()["text"] == direct[1] and r.json()["audio_duration"] == 3840
            hw = {"x-audio-sample-rate": "48000", "x-audio-bits": "16", "x-audio-channel": "1", "x-audio-codec": "pcm", "x-willow-id": "test"}
            r = await c.post("/api/willow?model=tiny&beam_size=1", content=s16.tobytes(), headers=hw)
            assert r.status_code == 200, r.text
            assert r.json() == {"language": "en", "text": direct[1]}
            # InvalidAudio is what it was: a body that is no container answers 400
            r = await c.post("/api/willow?model=tiny&beam_size=1", content=b"not audio", headers={"x-audio-codec": "wav"})
            assert r.status_code == 400

    asyncio.run(go())
