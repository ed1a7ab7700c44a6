"""-m gpu: the one-pass prefix route at model level - two handles on the same tiny seeded weights, prompt_prefill "windowed" and "one_pass".

(a) the prefix K / V of slot b * beam, read back per layer (wis_debug_self_kv), against a float64 restatement of the decoder (the oracle's decoder_step on
    float64 tensors, built as tests/enc_i8_ref.py decoder_logits builds it, with that module's encoder and cross K / V).  The windowed handle's error is
    measured first; the one-pass handle may be at most twice that - the two routes sum in different orders, neither is the truth.
(b) generate(fixed_new_tokens=6): identical ids, except where the oracle's search over the same prompt has a decision margin below MARGIN (a near-tie of the
    top two candidates): such a case is skipped.  With these seeds no case is (at most 1 in 12 may be).
(c) a P = 4 call: the same ids and the same captured graphs before and after wis_model_set_prefill(m, 1).
Fallbacks: where the route does not apply, the one-pass handle returns the windowed handle's ids and scores bit for bit."""
import ctypes as C
import os

import numpy as np
import pytest
import torch  # noqa: F401  (before libwis_hip.so: one HIP runtime per process)

import enc_i8_ref as E

pytestmark = pytest.mark.gpu
MARGIN = 0.02
SOT, PREV, NO_TIMESTAMPS = 50258, 50361, 50363


def _prompt(P, i):
    if P == 4:
        return [SOT, 50259, 50359, NO_TIMESTAMPS]
    return [PREV] + [int(t) for t in np.random.default_rng(100 * P + i).integers(0, 50257, P - 5)] + [SOT, 50259 + 7 * i, 50359, NO_TIMESTAMPS]


@pytest.fixture(scope="module")
def mel(golden_dir):
    return np.load(os.path.join(golden_dir, "logmel_3sec.npz"))["mel"].astype(np.float32)


@pytest.fixture(scope="module")
def rig(mel):
    from wis_hip import ctranslate2 as ct2, weights as W
    w, a = W.synthetic_weights("tiny", seed=1234, std=0.02, emb_std=0.06, ln_jitter=0.1), W.arch("tiny")
    made = {}

    def get(prefill="windowed", **kw):
        key = (prefill,) + tuple(sorted(kw.items()))
        if key not in made:
            made[key] = ct2.Whisper("unused", weights=w, arch=a, prompt_prefill=prefill, **{"max_batch": 8, "max_beam": 8, **kw})
        return made[key]
    get.w, get.arch = w, a
    yield get
    for m in made.values():
        m.close()


def _feats(mel, B):
    from wis_hip import ctranslate2 as ct2
    return ct2.StorageView.from_array(np.ascontiguousarray(np.repeat(mel[None], B, axis=0)))


def _pairs(res):
    return [(r.sequences_ids[0], r.scores[0]) for r in res]


_REF = {}      # the float64 references, computed once: "ckv" -> cross K / V, ("kv", prompt) -> per layer (K, V) [P][d]


def _ref_kv(rig, mel, prompt):
    from oracle.whisper_ref import WhisperRef
    w, a = rig.w, rig.arch
    if "ckv" not in _REF:
        _REF["ckv"] = E.cross_kv(w, a, E.encode(w, a, mel, quant=False), quant=False)
    key = ("kv", tuple(prompt))
    if key not in _REF:
        ref = WhisperRef(w, a["d_model"], a["n_layers"], a["n_heads"], n_vocab=a["n_vocab"])
        ref.w = {k: v.to(torch.float64) for k, v in ref.w.items() if k.startswith("decoder/")}
        tck = [(torch.from_numpy(np.ascontiguousarray(k, np.float64))[None], torch.from_numpy(np.ascontiguousarray(v, np.float64))[None]) for k, v in _REF["ckv"]]
        cache = [None] * ref.L
        ref.decoder_step(np.asarray([prompt]), 0, cache, tck)
        _REF[key] = [(k[0].numpy(), v[0].numpy()) for k, v in cache]
    return _REF[key]


def _kv_error(model, ref_kv, slot, Np):
    from wis_hip import _lib
    d, worst = ref_kv[0][0].shape[1], 0.0
    for layer, (k64, v64) in enumerate(ref_kv):
        k, v = np.empty((Np, d), np.float16), np.empty((Np, d), np.float16)
        _lib.check(_lib.load().wis_debug_self_kv(model._replicas[0].handle, layer, slot, Np, _lib.ptr(k), _lib.ptr(v)))
        worst = max(worst, np.abs(k - k64[:Np]).max(), np.abs(v - v64[:Np]).max())
    return worst


@pytest.mark.parametrize("beam", [1, 5])
@pytest.mark.parametrize("B", [1, 2])
@pytest.mark.parametrize("P", [17, 33, 228])
def test_one_pass_matches_windowed(rig, mel, P, B, beam):
    win, one = rig("windowed"), rig("one_pass")
    prompts = [_prompt(P, i) for i in range(B)]
    Np = P - 16
    res, err = {}, {}
    for name, model in (("windowed", win), ("one_pass", one)):
        res[name] = _pairs(model.generate(_feats(mel, B), prompts, beam_size=beam, fixed_new_tokens=6))
        err[name] = max(_kv_error(model, _ref_kv(rig, mel, prompts[b]), b * beam, Np) for b in range(B))
    print(f"P {P} B {B} beam {beam}: prefix K/V error against float64: windowed {err['windowed']:.3e}, one-pass {err['one_pass']:.3e}")
    assert err["one_pass"] <= 2 * err["windowed"], err
    for b in range(B):
        if res["one_pass"][b][0] != res["windowed"][b][0]:
            from oracle.whisper_ref import WhisperRef
            from wis_hip import weights as W
            ref = WhisperRef(rig.w, rig.arch["d_model"], rig.arch["n_layers"], rig.arch["n_heads"])
            _, _, trace = ref.generate(None, prompts[b], beam_size=beam, suppress_ids=W.SUPPRESS_IDS, suppress_begin=W.SUPPRESS_IDS_BEGIN,
                                       memory=ref.encode(mel[None])[0].numpy(), max_new_tokens=6, fixed_new=6, return_trace=True)
            if min(trace) <= MARGIN:
                pytest.skip(f"utterance {b}: the oracle's decision margin is {min(trace):.4f}: a near-tie")
            assert False, (b, res["one_pass"][b], res["windowed"][b])


def test_short_prompt_is_untouched(rig, mel):
    from wis_hip import _lib
    model = rig("windowed", max_batch=4)      # a handle of this test's own: its mode changes
    lib, h = _lib.load(), model._replicas[0].handle

    def call():
        n = C.c_int(0)
        out = _pairs(model.generate(_feats(mel, 2), [_prompt(4, 0)] * 2, beam_size=5, fixed_new_tokens=6))
        _lib.check(lib.wis_debug_graph_count(h, C.byref(n)))
        return out, n.value
    before = call()
    assert lib.wis_model_set_prefill(h, 2) != 0
    _lib.check(lib.wis_model_set_prefill(h, 1))
    assert call() == before
    _lib.check(lib.wis_model_set_prefill(h, 0))


@pytest.mark.parametrize("case", ["int8_float16", "cross_kv_int8", "ragged", "rows"])
def test_fallbacks_are_bit_identical(rig, mel, case):
    kw = {"int8_float16": {"compute_type": "int8_float16"}, "cross_kv_int8": {"cross_kv_compute_type": "int8"}}.get(case, {})
    win, one = rig("windowed", **kw), rig("one_pass", **kw)
    if case == "ragged":
        prompts, gen = [_prompt(40, 0), _prompt(33, 1)], {"ragged_prompts": True}
    elif case == "rows":
        prompts, gen = [_prompt(228, i) for i in range(2)], {}      # 2 x 212 prefix rows > 256
    else:
        prompts, gen = [_prompt(33, 0)], {}
    a = _pairs(win.generate(_feats(mel, len(prompts)), prompts, beam_size=5, fixed_new_tokens=6, **gen))
    b = _pairs(one.generate(_feats(mel, len(prompts)), prompts, beam_size=5, fixed_new_tokens=6, **gen))
    assert a == b
