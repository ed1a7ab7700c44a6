"""The in-grammar mass of phrase-constrained decoding, without a GPU: the float64 reference (tests/phrase_mass_ref.py) against the identity it
stands for - logmass(phrase) = log P_unconstrained(phrase, <|endoftext|>) - log P_constrained(phrase, <|endoftext|>), the constrained side from
phrase_ref.brute_force, the unconstrained one a plain log-softmax -, its -inf cases, the clamp, the begin list at the first step and the derived
fp32 bound (against an fp32 emulation of the engine's documented reduction order); then the host side on a stand-in engine: the shim's flag and
its batching rule, do_whisper's in_grammar / matched / fallback, the ValueErrors, the server's parameters and 400s."""
import asyncio
import io
import math
import wave

import numpy as np
import pytest

import phrase_mass_ref as R
from phrase_ref import allowed, brute_force, prefix_dict

EOT = 50257
PROMPT = [50258, 50259, 50359, 50363]
NEG = float("-inf")


# ---- the reference -----------------------------------------------------------------------------------------------------------------
def test_identity_unconstrained_minus_constrained():
    rng = np.random.default_rng(11)
    V, eot = 300, 299
    phrases = [[5, 6, 7], [5, 6], [5, 9], [40], [40, 41, 42, 43], [77, 5]]
    rows = {}

    def row_of(h):
        if h not in rows:
            rows[h] = (4.0 * rng.standard_normal(V)).astype(np.float32)
        return rows[h]
    scored = {ph: raw for _, raw, ph in brute_force(phrases, row_of, eot=eot)}
    for ph in {tuple(p) for p in phrases}:
        unc = sum(R.log_softmax_at(row_of(ph[:i]), ph[i] if i < len(ph) else eot) for i in range(len(ph) + 1))
        total, per = R.path_logmass(phrases, row_of, ph, eot=eot)
        assert len(per) == len(ph) + 1 and all(v <= 0.0 for v in per)
        assert abs(total - (unc - scored[ph])) <= 1e-10 * (1 + abs(total)), (ph, total, unc, scored[ph])


def test_minus_infinity_cases_and_the_clamp():
    u = np.asarray([1.0, 2.0, NEG, 0.5, NEG], np.float32)
    assert R.logmass(u, [2, 4]) == NEG                              # every allowed id is -inf
    assert R.logmass(np.full(5, NEG, np.float32), [0, 1]) == NEG    # the row is all -inf
    assert R.logmass(u, [0, 1, 3]) == 0.0                           # only allowed ids are finite: exactly 0
    assert R.logmass(u, [0, 1, 2, 3, 4]) == 0.0
    assert abs(R.logmass(u, [1]) - (2.0 - np.log(np.exp(1.0) + np.exp(2.0) + np.exp(0.5)))) < 1e-12
    assert R.logmass(np.asarray([0.0, 1e4, -1e4], np.float32), [0]) == -1e4 and R.logmass(np.asarray([0.0, 1e4, -1e4], np.float32), [2]) == -2e4
    assert R.logmass(np.asarray([np.inf, 1.0, np.inf], np.float32), [0]) == pytest.approx(-np.log(2.0)) and R.logmass(np.asarray([np.inf, 1.0], np.float32), [1]) == NEG
    for keep in ([0], [1, 3], [0, 1, 3]):                           # never above 0, never NaN without a NaN in the row
        v = R.logmass(u, keep)
        assert v <= 0.0 and v == v
    assert R.logmass_bound(u, [2, 4]) == 0.0 and R.logmass_bound(u, [0, 1, 3]) == 0.0 and 0 < R.logmass_bound(u, [1]) < 1e-4


def test_the_begin_list_binds_the_first_step_only():
    x = np.asarray([3.0, 1.0, 2.0, 0.0], np.float32)
    bias_all = np.asarray([0, 0, 0, NEG], np.float32)
    bias_begin = np.asarray([NEG, 0, 0, 0], np.float32)
    first = R.u_row(x, bias_all, bias_begin, first=True)
    later = R.u_row(x, bias_all, bias_begin, first=False)
    assert first.dtype == np.float32 and first.tolist() == [NEG, 1.0, 2.0, NEG] and later.tolist() == [3.0, 1.0, 2.0, NEG]
    assert R.u_row(x, None, bias_begin, first=False).tolist() == x.tolist()      # a null bias_all: no list
    lse = lambda v: np.log(np.exp(np.asarray(v, np.float64)).sum())
    assert abs(R.logmass(first, [1]) - (1.0 - lse([1.0, 2.0]))) < 1e-12
    assert abs(R.logmass(later, [1]) - (1.0 - lse([3.0, 1.0, 2.0]))) < 1e-12
    assert R.logmass(first, [0, 3]) == NEG                                         # an allowed id the lists mask counts for nothing


def _emulate_fp32(u, keep):
    """The engine's reduction order in numpy fp32 (accurate exp in float64 rounded to fp32: within the bound's allowance per factor)."""
    f = np.float32
    V = len(u)
    ok = np.zeros(V, bool)
    ok[list(keep)] = True
    E = lambda a, b: f(1.0) if a == b else f(np.exp(np.float64(f(a - b))))
    st = []
    with np.errstate(invalid="ignore", over="ignore"):
        for tid in range(256):
            mx, sd, ma, sn = f(NEG), f(0), f(NEG), f(0)
            for base in range(0, V, 2048):
                idx = [base + 256 * j + tid for j in range(8)]
                v = [f(u[i]) if i < V else f(NEG) for i in idx]
                o = [i < V and ok[i] for i in idx]
                cm, ca = max([mx] + v), max([ma] + [x if k else f(NEG) for x, k in zip(v, o)])
                mm, am = (f(0) if cm == NEG else cm), (f(0) if ca == NEG else ca)
                sd, sn = f(sd * E(mx, mm)), f(sn * E(ma, am))
                for x, k in zip(v, o):
                    sd = f(sd + E(x, mm))
                    sn = f(sn + (E(x, am) if k else f(0)))
                mx, ma = cm, ca
            st.append((mx, sd, ma, sn))
        M, MA = max(s[0] for s in st), max(s[2] for s in st)
        if M == NEG or MA == NEG:
            return NEG
        tree = lambda xs: xs[0] if len(xs) == 1 else f(tree(xs[:len(xs) // 2]) + tree(xs[len(xs) // 2:]))
        den = tree([f(s[1] * E(s[0], M)) for s in st])
        num = tree([f(s[3] * E(s[2], MA)) for s in st])
        d = f(0) if MA == M else f(MA - M)
        return float(min(f(0), f(d + f(f(np.log(np.float64(num))) - f(np.log(np.float64(den)))))))


def test_the_bound_covers_an_fp32_run_of_the_documented_order():
    rng = np.random.default_rng(5)
    for V, scale, n_keep in ((5, 3.0, 2), (257, 3.0, 7), (2500, 10.0, 3), (5000, 1e4, 40), (4099, 30.0, 1)):
        u = (scale * rng.standard_normal(V)).astype(np.float32)
        u[rng.choice(V, size=V // 10, replace=False)] = NEG
        keep = sorted(rng.choice(V, size=n_keep, replace=False).tolist())
        ref, bound, got = R.logmass(u, keep), R.logmass_bound(u, keep), _emulate_fp32(u, keep)
        if ref == NEG:
            assert got == NEG
            continue
        assert abs(got - ref) <= R.SAFETY * bound, (V, scale, got, ref, bound)
        assert bound <= 1e-3 * (1 + abs(ref)) * (1 + scale / 100)      # the bound says something: far below the values it bounds
    u = np.asarray([1.0, NEG, 2.0, NEG, 0.25], np.float32)
    assert _emulate_fp32(u, [0, 2, 4]) == 0.0 and _emulate_fp32(u, [1, 3]) == NEG


# ---- the shim ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def model():
    from wis_hip import ctranslate2 as ct2, weights as W
    m = ct2.Whisper.from_handles([(None, 0)], W.arch("large"))
    yield m
    m._batcher.close()


def _opts(model, **kw):
    from wis_hip import _lib
    args = dict(input_kind=_lib.WIS_IN_MEL_DEV, n_utt=1, beam_size=5, patience=1, num_hypotheses=1, length_penalty=1, repetition_penalty=1,
                no_repeat_ngram_size=0, max_length=448, return_no_speech_prob=False, max_initial_timestamp_index=50, suppress_blank=True,
                suppress_default=True, sampling_topk=1, sampling_temperature=1, fixed_new_tokens=0, draft_tokens=None, draft_trajectory=None,
                return_trajectory=False)
    args.update(kw)
    return model._decode_options(None, [PROMPT], **args)[0]


def test_the_flag_and_the_batching_rule(model):
    from wis_hip import _lib, ctranslate2 as ct2
    a = [[400, 401], [500]]
    off, on, on2 = _opts(model, phrases=a), _opts(model, phrases=a, return_phrase_mass=True), _opts(model, phrases=list(reversed(a)), return_phrase_mass=True)
    assert type(on) is ct2.ConstrainedOptions and on.phrase_mass is True and off.phrase_mass is False
    assert tuple(on) == tuple(off) and on.phrase_digest == off.phrase_digest      # nothing but the flag differs ...
    assert on != off and off != on and len({on, off}) == 2                        # ... and they never share a device batch
    assert on == on2 and hash(on) == hash(on2)
    r = on._replace(prompt_len=7)
    assert r.phrase_mass is True and r != on
    assert ct2._gen_opts(on).phrase_mass == 1 and ct2._gen_opts(on).phrases == 1 and ct2._gen_opts(off).phrase_mass == 0
    assert ct2._gen_opts(_opts(model)).phrase_mass == 0 and type(_opts(model)) is ct2.DecodeOptions
    assert [n for n, _ in _lib.GenOpts._fields_][-2:] == ["phrases", "phrase_mass"]      # appended: every earlier field lies where it lay
    with pytest.raises(ValueError) as e:
        _opts(model, return_phrase_mass=True)
    assert "phrases" in str(e.value)
    assert ct2.WhisperGenerationResult([[1]], [0.0]).phrase_logmass is None


def test_two_requests_that_differ_in_the_flag_land_in_different_batches(model):
    """through generate_from_device and the micro-batcher, with the replica's decode replaced: one batch per key"""
    import threading
    from wis_hip import ctranslate2 as ct2
    seen, gate = [], threading.Barrier(2)
    real = ct2._generate_chunk

    def fake(r, mel, prompts, opts, *rest, **kw):
        seen.append((getattr(opts, "phrase_mass", None), len(prompts)))
        out = [ct2.WhisperGenerationResult([[400, 401]], [-0.5]) for _ in prompts]
        if opts.phrase_mass:
            for o in out:
                o.phrase_logmass = [-1.5]
        return out
    ct2._generate_chunk = fake
    try:
        res = {}

        def call(flag):
            gate.wait()
            res[flag] = model.generate_from_device(0, 4096, PROMPT, phrases=[[400, 401]], return_phrase_mass=flag)
        ts = [threading.Thread(target=call, args=(f,)) for f in (False, True)]
        [t.start() for t in ts]
        [t.join() for t in ts]
    finally:
        ct2._generate_chunk = real
    assert sorted(seen) == [(False, 1), (True, 1)], seen
    assert res[True].phrase_logmass == [-1.5] and res[False].phrase_logmass is None


# ---- do_whisper and the server on a stand-in engine -------------------------------------------------------------------------------------
class _FakeWhisper:
    """phrases: the two best phrases with their masses; without: a plain transcript"""

    def __init__(self, mass=(-0.5, -12.0)):
        self.calls, self.mass = [], mass

    def generate(self, feats, prompts, **kw):
        from wis_hip import ctranslate2 as ct2
        self.calls.append(kw)
        if kw.get("phrases") is None:
            assert "return_phrase_mass" not in kw and "num_hypotheses" not in kw
            return [ct2.WhisperGenerationResult([[900, 901, 902]], [-0.3]) for _ in prompts]
        n = kw.get("num_hypotheses", 1)
        r = ct2.WhisperGenerationResult([kw["phrases"][i] for i in range(n)], [-0.1 * (i + 1) for i in range(n)])
        if kw.get("return_phrase_mass"):
            r.phrase_logmass = [self.mass[i] for i in range(n)]
        return [r for _ in prompts]

    def detect_language(self, *a, **k):
        return [[("<|en|>", 1.0)]]


class _Models:
    def __init__(self, **settings):
        from wis_hip.settings import APISettings
        from wis_hip.whisper import _Tokenizer
        self.settings = APISettings()
        self.settings.fuse_logmel = True
        self.settings.beam_size = 5
        for k, v in settings.items():
            setattr(self.settings, k, v)
        self.tokenizer = _Tokenizer(None)
        self.whisper = _FakeWhisper()

    def tokenizer_for(self, size):
        return self.tokenizer

    def get(self, size):
        return self.whisper


PCM = np.zeros(16000, np.float32)
PHRASES = [[400, 401, 402], [500]]


def test_do_whisper_in_grammar_matched_and_fallback():
    from wis_hip import whisper
    from wis_hip.settings import APISettings
    s = APISettings()
    assert (s.phrase_mass, s.phrase_threshold, s.phrase_fallback) == (False, 0.0, False)      # off, no threshold, off: none is shipped
    m = _Models()
    r = whisper.do_whisper(PCM, "tiny", models=m, phrases=PHRASES, phrase_nbest=2)
    assert "return_phrase_mass" not in m.whisper.calls[-1] and r.matched is None and set(r.matches[0]) == {"text", "score"}      # off: as ever
    r = whisper.do_whisper(PCM, "tiny", models=m, phrases=PHRASES, phrase_nbest=2, phrase_mass=True)
    assert m.whisper.calls[-1]["return_phrase_mass"] is True and r.matched is None and len(m.whisper.calls) == 2
    assert [mt["logmass"] for mt in r.matches] == [-0.5, -12.0]
    assert r.matches[0]["in_grammar"] == pytest.approx(math.exp(-0.5 / 4)) and r.matches[1]["in_grammar"] == pytest.approx(math.exp(-12.0 / 2))      # tokens + 1 steps
    assert r[1] == "400 401 402"
    # a threshold implies the mass; matched = the best match's share against it
    r = whisper.do_whisper(PCM, "tiny", models=m, phrases=PHRASES, phrase_threshold=0.5)
    assert m.whisper.calls[-1]["return_phrase_mass"] is True and r.matched is True and r[1] == "400 401 402"
    r = whisper.do_whisper(PCM, "tiny", models=m, phrases=PHRASES, phrase_threshold=0.95)
    assert r.matched is False and r[1] == "400 401 402"                          # no fallback asked: the phrase stays
    n = len(m.whisper.calls)
    r = whisper.do_whisper(PCM, "tiny", models=m, phrases=PHRASES, phrase_threshold=0.95, phrase_fallback=True, phrase_nbest=2)
    assert r.matched is False and r[1] == "900 901 902" and r.tokens == [900, 901, 902] and len(m.whisper.calls) == n + 2
    assert [mt["text"] for mt in r.matches] == ["400 401 402", "500"] and m.whisper.calls[-1].get("phrases") is None      # matches stay; the second decode is plain
    r = whisper.do_whisper(PCM, "tiny", models=m, phrases=PHRASES, phrase_threshold=0.5, phrase_fallback=True)
    assert r.matched is True and r[1] == "400 401 402" and len(m.whisper.calls) == n + 3      # matched: no second decode
    # threshold 1.0: only a mass of exactly 0 matches
    assert whisper.do_whisper(PCM, "tiny", models=m, phrases=PHRASES, phrase_threshold=1.0).matched is False
    m.whisper.mass = (0.0, -1.0)
    assert whisper.do_whisper(PCM, "tiny", models=m, phrases=PHRASES, phrase_threshold=1.0).matched is True
    m.whisper.mass = (float("nan"), -1.0)                                          # a NaN share is no match
    r = whisper.do_whisper(PCM, "tiny", models=m, phrases=PHRASES, phrase_threshold=0.01)
    assert r.matched is False and math.isnan(r.matches[0]["in_grammar"])
    m.whisper.mass = (NEG, -1.0)
    assert whisper.do_whisper(PCM, "tiny", models=m, phrases=PHRASES, phrase_mass=True).matches[0]["in_grammar"] == 0.0
    # the settings are the defaults
    m = _Models(phrase_threshold=0.95, phrase_fallback=True)
    r = whisper.do_whisper(PCM, "tiny", models=m, phrases=PHRASES)
    assert r.matched is False and r[1] == "900 901 902"
    assert whisper.do_whisper(PCM, "tiny", models=m, phrases=PHRASES, phrase_threshold=0.5).matched is True
    assert whisper.do_whisper(PCM, "tiny", models=m).matches is None               # they act on constrained requests only
    assert whisper.in_grammar(-3.0, 2) == pytest.approx(math.exp(-1.0)) and whisper.in_grammar(0.0, 5) == 1.0


def test_do_whisper_value_errors():
    from wis_hip import whisper
    m = _Models()
    for kw in (dict(phrase_threshold=1.5), dict(phrase_threshold=-0.1), dict(phrase_threshold=float("nan")), dict(phrase_threshold="high"),
               dict(phrase_fallback=True), dict(phrase_fallback=True, phrase_threshold=0.0)):
        with pytest.raises(ValueError) as e:
            whisper.do_whisper(PCM, "tiny", models=m, phrases=PHRASES, **kw)
        assert "phrase_" in str(e.value), (kw, str(e.value))
    for kw in (dict(phrase_mass=True), dict(phrase_threshold=0.5), dict(phrase_fallback=True)):      # without phrases
        with pytest.raises(ValueError) as e:
            whisper.do_whisper(PCM, "tiny", models=m, **kw)
        assert "needs phrases" in str(e.value)
    assert m.whisper.calls == []


def _wav(seconds):
    buf = io.BytesIO()
    with wave.open(buf, "wb") as w:
        w.setnchannels(1); w.setsampwidth(2); w.setframerate(16000)
        w.writeframes((np.sin(np.arange(int(16000 * seconds)) * 0.05) * 8000).astype("<i2").tobytes())
    return buf.getvalue()


def test_server_parameters_and_400s():
    import httpx
    from wis_hip.server import create_app
    models = _Models()
    app = create_app(models=models)
    wav = _wav(1.0)
    b = "pmBoundary7"
    body = (f"--{b}\r\nContent-Disposition: form-data; name=\"audio_file\"; filename=\"a.wav\"\r\nContent-Type: application/octet-stream\r\n\r\n").encode() + wav + f"\r\n--{b}--\r\n".encode()
    hdr = {"content-type": f"multipart/form-data; boundary={b}"}
    ph = "phrases=ids:400,401,402|ids:500&phrase_nbest=2"

    async def go():
        async with httpx.AsyncClient(transport=httpx.ASGITransport(app=app), base_url="http://wis") as c:
            for q, word in (("phrase_mass=maybe", "phrase_mass"), ("phrase_fallback=2", "phrase_fallback"), ("phrase_threshold=high", "phrase_threshold"),
                            ("phrase_threshold=1.5", "phrase_threshold"), ("phrase_threshold=-1", "phrase_threshold"), ("phrase_threshold=nan", "phrase_threshold"),
                            ("phrase_fallback=true", "phrase_fallback needs"), ("phrase_fallback=true&phrase_threshold=0", "phrase_fallback needs")):
                r = await c.post(f"/api/asr?model=tiny&{ph}&{q}", content=body, headers=hdr)
                assert r.status_code == 400 and word in r.json()["error"], (q, r.status_code, r.text)
            r = await c.post("/api/asr?model=tiny&phrase_mass=true", content=body, headers=hdr)      # without phrases
            assert r.status_code == 400 and "needs phrases" in r.json()["error"]
            r = await c.post(f"/api/asr?model=tiny&{ph}", content=body, headers=hdr)
            assert r.status_code == 200 and "matched" not in r.json() and set(r.json()["matches"][0]) == {"text", "score"}
            r = await c.post(f"/api/asr?model=tiny&{ph}&phrase_mass=true&phrase_threshold=&phrase_fallback=", content=body, headers=hdr)      # empty: the settings'
            j = r.json()
            assert r.status_code == 200 and "matched" not in j and [mt["logmass"] for mt in j["matches"]] == [-0.5, -12.0]
            assert j["matches"][0]["in_grammar"] == pytest.approx(math.exp(-0.125))
            r = await c.post(f"/api/asr?model=tiny&{ph}&phrase_threshold=0.2", content=body, headers=hdr)
            assert r.status_code == 200 and r.json()["matched"] is True and r.json()["text"] == "400 401 402"
            r = await c.post(f"/api/asr?model=tiny&{ph}&phrase_threshold=0.95&phrase_fallback=true", content=body, headers=hdr)
            j = r.json()
            assert r.status_code == 200 and j["matched"] is False and j["text"] == "900 901 902" and len(j["matches"]) == 2
            r = await c.post(f"/api/willow?model=tiny&{ph}&phrase_threshold=0.95&phrase_fallback=true", content=wav, headers={"x-audio-codec": "wav"})
            j = r.json()
            assert r.status_code == 200 and j["matched"] is False and j["text"] == "900 901 902" and j["matches"][1]["logmass"] == -12.0, r.text
            r = await c.post("/api/willow?model=tiny&phrase_threshold=2", content=wav, headers={"x-audio-codec": "wav"})
            assert r.status_code == 400 and "phrase_threshold" in r.json()["error"]
            models.whisper.mass = (NEG, float("nan"))                      # not finite: null in the JSON body
            r = await c.post(f"/api/asr?model=tiny&{ph}&phrase_threshold=0.2", content=body, headers=hdr)
            j = r.json()
            assert r.status_code == 200 and j["matched"] is False and j["matches"][0]["logmass"] is None and j["matches"][0]["in_grammar"] == 0.0
            assert j["matches"][1]["logmass"] is None and j["matches"][1]["in_grammar"] is None

    asyncio.run(go())
