"""-m gpu: Whisper timestamps on the GPU (ts_rules_kernel + logit_stats_kernel<true>) against the CPU statement of the rules
(tests/ts_ref.py) driving the oracle's search, and no_speech_prob against the oracle's logits at <|startoftranscript|>.

`wis_debug_search` with timestamps=1 runs the timestamp form of the sampling tail on caller-supplied logits tables built to hit every
rule; ids, finish step, score and beam ancestry must be IDENTICAL to ts_ref + WhisperRef.search.  A case is skipped - and counted - only
when the search's own decision margin or the timestamp decision's |logsumexp(timestamps) - max(text)| falls below 2e-4 (fp32 summation
order could then legitimately differ)."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from ts_ref import EOT, NO_TIMESTAMPS, TB, TsStepFn, generate_ts, grammar_errors

pytestmark = pytest.mark.gpu
V = 51865
WIS_E_STATE, WIS_E_UNSUPPORTED = -6, -7      # include/wis_hip.h
MARGIN = 2e-4           # wis_debug_search: the same fp32 logits on both sides
E2E_MARGIN = 0.02       # end to end: the engine's logits against the oracle's
PROMPT = [50258, 50259, 50359]


@pytest.fixture(scope="module")
def engine():
    from wis_hip import ctranslate2 as ct2, weights as W
    model = ct2.Whisper("unused", weights=W.synthetic_weights("tiny", seed=1234), arch=W.arch("tiny"), max_batch=16, max_beam=8)
    yield model
    model.close()


def _run_engine(model, table, B, beam, max_init=50, fixed_new=0):
    from wis_hip import _lib
    lib = _lib.load()
    steps = table.shape[0]
    o = _lib.GenOpts(0, beam, 0, 1.0, 1.0, 1, 1, fixed_new, 0)
    o.timestamps, o.max_initial_timestamp_index = 1, (-1 if max_init is None else max_init)
    ids = np.zeros((B, steps), np.int32); lens = np.zeros(B, np.int32); sc = np.zeros(B, np.float32)
    fin = np.zeros(B, np.int32); par = np.full((steps, B * beam), -1, np.int32)
    i32 = C.POINTER(C.c_int32)
    _lib.check(lib.wis_debug_search(model._replicas[0].handle, _lib.ptr(table), steps, B, C.byref(o), ids.ctypes.data_as(i32), lens.ctypes.data_as(i32),
                                    sc.ctypes.data_as(C.POINTER(C.c_float)), fin.ctypes.data_as(i32), par.ctypes.data_as(i32)))
    return [ids[b, :lens[b]].tolist() for b in range(B)], sc, fin, par


def _ts_table(rng, steps, B, beam, ts_shift):
    """N(0, 2^2) logits; the timestamp block shifted per (step, row) by ts_shift + U(-3, 3) (the decision goes both ways) and tilted
    towards low timestamps (the monotonicity mask and repeated timestamps matter); EOT climbs per utterance so searches end on it."""
    t = 2.0 * rng.standard_normal((steps, B * beam, V), dtype=np.float32)
    t[:, :, TB:] += (ts_shift + rng.uniform(-3.0, 3.0, size=(steps, B * beam, 1))).astype(np.float32)
    t[:, :, TB:] -= (0.004 * np.arange(V - TB, dtype=np.float32))[None, None, :]
    top = t[:, :, :TB].max(axis=2)
    ramp = rng.uniform(0.3, 1.2, size=B).astype(np.float32)
    for b in range(B):
        for j in range(beam):
            r = b * beam + j
            t[:, r, EOT] = top[:, r] - 7.0 + ramp[b] * np.arange(steps, dtype=np.float32) + 1.0 * rng.standard_normal(steps).astype(np.float32)
    return np.ascontiguousarray(t)


def _run_oracle(table, b, beam, max_init, fixed_new, stats):
    from oracle.whisper_ref import WhisperRef
    from wis_hip import weights as W
    tt = torch.from_numpy(table)

    def raw(step, last, origin):
        return tt[step, b * beam:(b + 1) * beam] if step > 0 else tt[0, b * beam].expand(beam, -1)
    fn = TsStepFn(raw, beam, W.SUPPRESS_IDS, W.SUPPRESS_IDS_BEGIN, True, fixed_new, max_init, stats)
    r = WhisperRef.search(fn, beam, V, EOT, table.shape[0], 1.0, 1.0)
    return r, fn


CASES = [  # (B, beam, ts_shift, max_init, fixed_new, steps)
    (3, 1, 2.0, 50, 0, 24), (2, 2, 1.0, 50, 0, 24), (3, 3, 1.5, 0, 0, 24), (2, 4, 0.5, None, 0, 20), (1, 5, 1.0, 50, 0, 24),
    (2, 5, 2.5, 3, 0, 24), (1, 6, 1.0, 50, 0, 20), (1, 7, 0.0, 50, 0, 16), (2, 8, 1.5, 50, 0, 16),
    (2, 1, 1.0, 50, 6, 10), (2, 5, 1.0, 50, 6, 10), (1, 8, 2.0, None, 4, 8),
]


def test_debug_search_timestamp_rules(engine):
    rng = np.random.default_rng(2024)
    stats = {"checked": 0, "skipped": 0}
    rules = {}
    for B, beam, shift, max_init, fixed_new, steps in CASES:
        table = _ts_table(rng, steps, B, beam, shift)
        ids, sc, fin, par = _run_engine(engine, table, B, beam, max_init, fixed_new)
        for b in range(B):
            r, fn = _run_oracle(table, b, beam, max_init, fixed_new, rules)
            if min(r["trace"]) < MARGIN or min(fn.margins) < MARGIN:
                stats["skipped"] += 1
                continue
            stats["checked"] += 1
            ctx = (B, beam, shift, max_init, fixed_new, b)
            assert ids[b] == r["ids"], (ctx, ids[b], r["ids"])
            assert fin[b] == r["finish_step"], (ctx, fin[b], r["finish_step"])
            if np.isfinite(r["score"]):
                assert abs(sc[b] - r["score"]) <= 2e-4 * max(1.0, abs(r["score"])), (ctx, sc[b], r["score"])
            for s, org in enumerate(r["origins"]):
                want = [b * beam + (0 if s == 0 else o) for o in org]
                assert par[s, b * beam:(b + 1) * beam].tolist() == want, (ctx, s)
            if not fixed_new:
                assert grammar_errors(ids[b], max_init) == [], (ctx, ids[b])
    print(f"\n[timestamps] debug-search: {stats['checked']} utterances checked, {stats['skipped']} skipped as near-ties; rule hits {rules}")
    assert stats["checked"] >= 0.7 * (stats["checked"] + stats["skipped"])
    for rule in ("after_pair", "open_segment", "monotonic", "monotonic_repeat_allowed", "initial_cap", "decision_timestamp", "decision_text"):
        assert rules.get(rule, 0) > 0, (rule, rules)


def _mel(golden_dir, name="3sec.flac"):
    from wis_hip import audio
    pcm, _ = audio.load_audio(os.path.join(golden_dir, "clips", name))
    return audio.log_mel_spectrogram(audio.pad_or_trim(pcm)).numpy()


@pytest.mark.parametrize("size,beam,fixed_new", [("tiny", 1, 0), ("tiny", 5, 0), ("tiny", 5, 8), ("base", 1, 10), ("base", 5, 0), ("large-v2", 5, 8)])
def test_engine_decodes_with_timestamps(golden_dir, size, beam, fixed_new):
    """The engine end to end with a timestamp prompt (no <|notimestamps|>): the oracle's decoder + the CPU rules + the oracle's search."""
    from oracle.whisper_ref import WhisperRef
    from wis_hip import ctranslate2 as ct2, weights as W
    from eot_ramp import with_eot_ramp
    w = W.synthetic_weights(size, seed=1234, emb_std=0.06, ln_jitter=0.1)
    if not fixed_new:
        w = with_eot_ramp(w, 8, 0.1)
    a = W.arch(size)
    mel = _mel(golden_dir)
    model = ct2.Whisper("unused", weights=w, arch=a, max_batch=1, max_beam=5)
    try:
        got = model.generate(ct2.StorageView.from_array(np.ascontiguousarray(mel[None])), [PROMPT], beam_size=beam, fixed_new_tokens=fixed_new,
                             max_length=80)[0]
    finally:
        model.close()
    ids = got.sequences_ids[0]
    assert grammar_errors(ids) == [], ids
    assert ids and TB <= ids[0] <= TB + 50 and NO_TIMESTAMPS not in ids, ids
    stamps = [t for t in ids if t >= TB]
    assert stamps == sorted(stamps), ids
    ref = WhisperRef(w, a["d_model"], a["n_layers"], a["n_heads"])
    r, fn = generate_ts(ref, mel, PROMPT, beam, W.SUPPRESS_IDS, W.SUPPRESS_IDS_BEGIN, fixed_new=fixed_new, max_new_tokens=40)
    # the engine's logits carry f16 weights and another summation order: a decision is forced only when it clears the engine-vs-oracle
    # logit error (the rule of smoke() and the other end-to-end tests).  Greedy: the ids up to the first step that does not are forced;
    # beam search: the whole result when every step does.  The grammar holds either way.
    step_m = [min(a, b) for a, b in zip(r["trace"], fn.margins)]
    first_tie = next((s for s, m in enumerate(step_m) if m <= E2E_MARGIN), len(step_m))
    whole = first_tie == len(step_m) and min(r["trace"]) > E2E_MARGIN
    n_cmp = len(r["ids"]) if whole else (first_tie if beam == 1 else 0)
    print(f"\n[timestamps] {size} beam {beam} fixed_new {fixed_new}: {ids}; {n_cmp} of {len(r['ids'])} ids forced and compared")
    assert ids[:n_cmp] == r["ids"][:n_cmp], (ids, r["ids"], n_cmp)
    if whole:
        assert abs(got.scores[0] - r["score"]) <= 2e-2, (got.scores, r["score"])


def test_no_speech_prob(golden_dir, engine):
    """B = 2: P(<|nospeech|>) at <|startoftranscript|> against the oracle's decode_logits([[SOT]]) softmax."""
    from oracle.whisper_ref import WhisperRef
    from wis_hip import _lib, ctranslate2 as ct2, weights as W
    w = W.synthetic_weights("tiny", seed=1234)
    a = W.arch("tiny")
    mels = np.ascontiguousarray(np.stack([_mel(golden_dir, "3sec.flac"), _mel(golden_dir, "10sec.flac")]))
    feats = ct2.StorageView.from_array(mels)
    ref = WhisperRef(w, a["d_model"], a["n_layers"], a["n_heads"])
    for prompt in (PROMPT + [NO_TIMESTAMPS], PROMPT):
        res = engine.generate(feats, [prompt] * 2, beam_size=2, fixed_new_tokens=3, return_no_speech_prob=True)
        for b in range(2):
            mem = ref.encode(mels[b:b + 1])
            lg = ref.decode_logits(np.array([[50258]]), mem)[0, -1]
            want = float(torch.softmax(torch.as_tensor(lg).double(), -1)[W.NO_SPEECH])
            assert abs(res[b].no_speech_prob - want) <= 1e-3, (b, res[b].no_speech_prob, want)
            assert res[b].no_speech_prob > 0.0
    # a call that did not ask leaves nothing to read
    engine.generate(feats, [PROMPT + [NO_TIMESTAMPS]] * 2, beam_size=2, fixed_new_tokens=3)
    out = np.zeros(2, np.float32)
    rc = _lib.load().wis_last_no_speech_prob(engine._replicas[0].handle, 2, out.ctypes.data_as(C.POINTER(C.c_float)))
    assert rc == WIS_E_STATE


def test_drafts_refuse_timestamps(engine):
    from wis_hip import _lib
    lib = _lib.load()
    o = _lib.GenOpts(0, 1, 0, 1.0, 1.0, 1, 1, 0, 0)
    o.timestamps = 1
    mel = np.zeros((80, 3000), np.float32)
    pr = np.asarray(PROMPT, np.int32); d = np.asarray([TB, 100], np.int32)
    ids = np.zeros(256, np.int32); n = np.zeros(1, np.int32); acc = C.c_int32(0)
    i32 = C.POINTER(C.c_int32)
    rc = lib.wis_generate_draft(engine._replicas[0].handle, _lib.ptr(mel), pr.ctypes.data_as(i32), 3, C.byref(o), d.ctypes.data_as(i32), 2,
                                ids.ctypes.data_as(i32), n.ctypes.data_as(i32), None, C.byref(acc))
    assert rc == WIS_E_UNSUPPORTED


def test_asr_endpoint_segments(golden_dir):
    """/api/asr?timestamps=true on tiny: segments are what segments_from_tokens makes of the ids the same decode returns."""
    import asyncio
    import httpx
    from wis_hip.server import create_app
    from wis_hip.settings import APISettings
    from wis_hip.whisper import WhisperModels, do_whisper, segments_from_tokens
    s = APISettings()
    s.whisper_model_path = "synthetic:{size}"
    s.fixed_new_tokens = 12
    s.beam_size = 1
    models = WhisperModels(s, device_index=[0])
    app = create_app(models=models)
    clip = os.path.join(golden_dir, "clips", "3sec.flac")
    direct = do_whisper(clip, "tiny", 1, models=models, timestamps=True)
    tok = models.tokenizer_for("tiny")
    assert direct.segments == segments_from_tokens(direct.tokens, tok, 0.0, min(direct[5] / 1000.0, 30.0))
    assert direct.tokens[0] >= TB and all(str(t) not in direct[1].split() for t in direct.tokens if t >= TB)
    data = open(clip, "rb").read()
    b = "gpuTsBoundary"
    body = (f"--{b}\r\nContent-Disposition: form-data; name=\"audio_file\"; filename=\"a.flac\"\r\n\r\n").encode() + data + f"\r\n--{b}--\r\n".encode()

    async def go():
        async with httpx.AsyncClient(transport=httpx.ASGITransport(app=app), base_url="http://wis", timeout=120) as c:
            r = await c.post("/api/asr?model=tiny&beam_size=1&timestamps=true", content=body, headers={"content-type": f"multipart/form-data; boundary={b}"})
            assert r.status_code == 200, r.text
            return r.json()
    j = asyncio.run(go())
    assert j["segments"] == direct.segments and j["text"] == direct[1]
    print(f"\n[timestamps] /api/asr segments: {j['segments']}")
