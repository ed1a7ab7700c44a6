"""-m gpu: wis_align's one-pass route at model level - two handles on the same tiny seeded weights, align_forward "windowed" and "one_pass".

Reference: the oracle's teacher-forced decoder on float64 tensors over tests/enc_i8_ref.py's float64 encoder output, with the cross-attention queries (scaled by
1/8) and keys of the alignment heads taken where _mha receives them; align_ref turns them into the matrix, its DTW into the path, the float64 logits into
the text-token probabilities.  The windowed handle's maximum error is measured first; the one-pass handle may be at most twice that (the convention of
tests/test_gpu_prefill_model.py: the two routes sum in different orders and neither is the truth).  Both handles' DTW paths equal the reference path."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import align_ref as R
import enc_i8_ref as E

pytestmark = pytest.mark.gpu
P, WIDTH, FRAMES = 3, 7, 200
# text tokens per utterance: L = P + 1 + text_len rows each -> 16, 17, 257, 448 rows; an utterance boundary inside a 16-row block; three utterances, 292 rows
CASES = [(12,), (13,), (253,), (444,), (5, 40), (100, 120, 60)]
_i32 = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))
_f32 = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))


@pytest.fixture(scope="module")
def rig(golden_dir):
    from wis_hip import ctranslate2 as ct2, weights as W
    w, a = W.synthetic_weights("tiny", seed=77, emb_std=0.06, ln_jitter=0.1), W.arch("tiny")
    mel = np.load(os.path.join(golden_dir, "logmel_3sec.npz"))["mel"].astype(np.float32)
    made = {}

    def get(forward, **kw):
        key = (forward,) + tuple(sorted(kw.items()))
        if key not in made:
            made[key] = ct2.Whisper("unused", weights=w, arch=a, align_forward=forward, max_batch=3, max_beam=1, **kw)
        return made[key]
    get.w, get.arch, get.mels = w, a, [mel, np.ascontiguousarray(mel[:, ::-1])]      # utterance b hears mels[b % 2]
    yield get
    for m in made.values():
        m.close()


_REF = {}      # ("mem", i) -> float64 encoder output of mels[i]; (i, text) -> (matrix, path, probabilities)


def _ref(rig, i, text, st):
    from oracle.whisper_ref import WhisperRef
    w, a = rig.w, rig.arch
    if ("mem", i) not in _REF:
        _REF[("mem", i)] = torch.from_numpy(E.encode(w, a, rig.mels[i], quant=False))[None]
    key = (i, tuple(text))
    if key not in _REF:
        class Ref(WhisperRef):
            def _mha(self, q, k, v, mask=None):
                if mask is None:      # the cross-attention of a layer: q [1][rows][d], k [1][1500][d]
                    self.cross.append((q[0].numpy() * 0.125, k[0].numpy()))
                return super()._mha(q, k, v, mask)
        ref = Ref(w, a["d_model"], a["n_layers"], a["n_heads"], n_vocab=a["n_vocab"])
        ref.w = {k: v.to(torch.float64) for k, v in ref.w.items() if k.startswith("decoder/")}
        ref.cross = []
        n = len(text)
        lg = ref.decode_logits([[st.sot, st.lang_ids[0], st.transcribe, st.notimestamps] + list(text)], _REF[("mem", i)])[0].numpy()
        heads = [(l, h) for l in range(a["n_dec_layers"] // 2, a["n_dec_layers"]) for h in range(a["n_heads"])]
        q = np.stack([ref.cross[l][0][P:P + n + 1, 64 * h:64 * h + 64] for l, h in heads])
        K = np.stack([ref.cross[l][1][:, 64 * h:64 * h + 64] for l, h in heads])
        x = R.matrix(R.attention_weights(q, K)[:, :, :FRAMES // 2], WIDTH)
        lp = lg[P:P + n, :st.eot]
        pr = np.exp(lp - lp.max(-1, keepdims=True))
        _REF[key] = (x, R.dtw_fast(x), (pr / pr.sum(-1, keepdims=True))[np.arange(n), list(text)])
    return _REF[key]


def _texts(lens):
    rng = np.random.default_rng([len(lens), sum(lens)])
    return [rng.integers(0, 50000, size=n).astype(np.int32) for n in lens]


def _run(model, rig, texts, st):
    """(matrices, alignment results) of one call per entry point on the batch"""
    from wis_hip import _lib
    B, F = len(texts), FRAMES // 2
    mels = np.ascontiguousarray(np.stack([rig.mels[b % 2] for b in range(B)]))
    start = np.array([st.sot, st.lang_ids[0], st.transcribe], np.int32)
    flat, ln, nf = np.ascontiguousarray(np.concatenate(texts)), np.array([len(t) for t in texts], np.int32), np.full(B, FRAMES, np.int32)
    out = np.zeros(sum((len(t) + 1) * F for t in texts), np.float32)
    _lib.check(_lib.load().wis_debug_align_matrix(model._replicas[0].handle, _lib.ptr(mels), _lib.WIS_IN_MEL_HOST, B, _i32(start), P, _i32(flat), _i32(ln), _i32(nf), WIDTH, _f32(out)))
    mats, o = [], 0
    for t in texts:
        mats.append(out[o:o + (len(t) + 1) * F].reshape(len(t) + 1, F))
        o += (len(t) + 1) * F
    return mats, model.align(mels, start.tolist(), [t.tolist() for t in texts], [FRAMES] * B, median_filter_width=WIDTH)


@pytest.mark.parametrize("lens", CASES, ids=str)
def test_one_pass_against_float64_and_windowed(rig, lens):
    win, one = rig("windowed"), rig("one_pass")
    st, texts = win.special, _texts(lens)
    refs = [_ref(rig, b % 2, t, st) for b, t in enumerate(texts)]
    em, ep = {}, {}
    for name, model in (("windowed", win), ("one_pass", one)):
        mats, res = _run(model, rig, texts, st)
        em[name] = max(np.abs(m - r[0]).max() for m, r in zip(mats, refs))
        ep[name] = max(np.abs(np.asarray(a.text_token_probs, np.float64) - r[2]).max() for a, r in zip(res, refs))
        for b, (a, r) in enumerate(zip(res, refs)):
            assert len(a.text_token_probs) == lens[b]
            assert [p[0] for p in a.alignments] == r[1][0].tolist() and [p[1] for p in a.alignments] == r[1][1].tolist(), (name, b)
    print(f"text {lens}: matrix error against float64: windowed {em['windowed']:.3e}, one-pass {em['one_pass']:.3e}; "
          f"probabilities: windowed {ep['windowed']:.3e}, one-pass {ep['one_pass']:.3e}")
    assert em["one_pass"] <= 2 * em["windowed"] and ep["one_pass"] <= 2 * ep["windowed"], (em, ep)


def test_align_leaves_the_decoder_state_alone(rig):
    from wis_hip import _lib, ctranslate2 as ct2
    one = rig("one_pass")
    st = one.special
    feats = ct2.StorageView.from_array(np.ascontiguousarray(np.stack(rig.mels)))
    prompts = [[st.sot, st.lang_ids[0], st.transcribe, st.notimestamps]] * 2
    gen = lambda: [(r.sequences_ids[0], r.scores[0]) for r in one.generate(feats, prompts, beam_size=1, fixed_new_tokens=6)]
    before = gen()
    _run(one, rig, _texts((5, 40)), st)
    assert gen() == before
    assert _lib.load().wis_model_set_align_pass(one._replicas[0].handle, 2) == -1      # WIS_E_ARG, and the mode stays


def test_int8_decoder_weights_fall_back_bit_identically(rig):
    win, one = rig("windowed", compute_type="int8_float16"), rig("one_pass", compute_type="int8_float16")
    texts = _texts((5, 40))
    (ma, ra), (mb, rb) = _run(win, rig, texts, win.special), _run(one, rig, texts, win.special)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(ma, mb))
    assert [(r.alignments, r.text_token_probs) for r in ra] == [(r.alignments, r.text_token_probs) for r in rb]
