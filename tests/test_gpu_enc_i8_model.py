"""-m gpu: the int8 encoder (models.Whisper(encoder_compute_type="int8")) at model level, where tests/test_gpu_enc_i8.py stops.

* run_cross_kv's int8 route against float64: teacher-forced logits (wis_debug_logits on a memory block of the test's own, WIS_IN_ENC_HOST - the encoder
  is out of the picture) against the oracle's decoder in float64 behind enc_i8_ref.cross_kv.  e8 = the int8 engine against the int8-rule reference,
  e16 = the f16 engine on the same memory against the unquantised reference; asserted: e8 <= 2 e16.  The quantised integers are the same on both sides
  (the quantiser is bit-equal: test_gpu_enc_i8_shapes.py) and the int8 product is exact where the f16 one rounds, so int8 has no legitimate way to be
  worse; the factor 2 covers which f16 roundings of K / V fall the other way.  tests/test_enc_i8_cpu.py: wrong layer scales, a dropped activation
  scale or V under K's scales move these logits by 0.3 to 1.4 - five orders above the reference's own float32 noise.
* one encoder pass of five utterances, in which gemm_i8_pick takes all three tile forms; the widths 512, 768, 1024, 1280 (one layer each, seeded);
  clones.  Whole encoder, as in test_gpu_enc_i8.py: rel-L2 against enc_i8_ref.encode in float64 <= 4 max(s, e16).
Figures: profiles/enc_int8_tests.md."""
import ctypes as C
import zlib

import numpy as np
import pytest

from enc_i8_taps import rel, tiny_rig

pytestmark = pytest.mark.gpu
PROMPT = [50258, 50259, 50359, 50363]
TOKENS = PROMPT + [1000, 2000, 3000, 4000]
_f32p, _i32p = C.POINTER(C.c_float), C.POINTER(C.c_int32)


def _pick(M, N):
    """gemm_i8_pick (csrc/enc_kernels.hip) restated: 3 = 256 x 256, 2 = 64 x 128, 1 = 128 x 128"""
    if N % 256 == 0 and (N // 256) * -(-M // 256) >= 150:
        return 3
    return 2 if ((N // 128) * -(-M // 128) < 200 and M > 64) else 1


def _encode(lib, h, mels, d):
    from wis_hip import _lib
    out = np.zeros((mels.shape[0], 1500, d), np.float32)
    _lib.check(lib.wis_debug_encode(h, _lib.ptr(mels), _lib.WIS_IN_MEL_HOST, mels.shape[0], out.ctypes.data_as(_f32p)))
    return out


def _model(w, a, **kw):
    from wis_hip import ctranslate2 as ct2
    return ct2.Whisper("unused", weights=w, arch=a, max_beam=1, **kw)


def _logits(lib, h, mem, V):
    from wis_hip import _lib
    B, dec_in = mem.shape[0], np.ascontiguousarray(np.tile(np.asarray(TOKENS, np.int32), (mem.shape[0], 1)))
    out = np.zeros((B, len(TOKENS), V), np.float32)
    _lib.check(lib.wis_debug_logits(h, _lib.ptr(mem), _lib.WIS_IN_ENC_HOST, B, dec_in.ctypes.data_as(_i32p), len(TOKENS), out.ctypes.data_as(_f32p)))
    return out


def _generate(lib, h, mels, kind=0):
    """greedy, 4 fixed tokens -> (ids [B][4], scores [B])"""
    from wis_hip import _lib
    B = mels.shape[0]
    o = _lib.GenOpts(kind, 1, 0, 1.0, 1.0, 1, 1, 4, 0)
    prompt, ids, lens, sc = np.ascontiguousarray(np.tile(np.asarray(PROMPT, np.int32), (B, 1))), np.zeros((B, 224), np.int32), np.zeros(B, np.int32), np.zeros(B, np.float32)
    _lib.check(lib.wis_generate(h, _lib.ptr(mels), B, prompt.ctypes.data_as(_i32p), 4, C.byref(o), ids.ctypes.data_as(_i32p), lens.ctypes.data_as(_i32p), sc.ctypes.data_as(_f32p)))
    assert (lens == 4).all()
    return ids[:, :4].copy(), sc


@pytest.fixture(scope="module")
def tiny(golden_dir):
    import torch  # noqa: F401  (before libwis_hip.so: one HIP runtime per process)
    w, a, mels, refs = tiny_rig(golden_dir)
    models = {"int8": _model(w, a, max_batch=5, encoder_compute_type="int8"), "f16": _model(w, a, max_batch=5)}
    yield w, a, mels, refs, models
    for m in models.values():
        m.close()


@pytest.fixture(scope="module")
def ckv_refs(tiny, lib):
    """the memory block [3][1500][384] - the int8 engine's own encoder output for the two clips and the first again, one row of utterance 1 zeroed (scale 1
    by the rule) and one multiplied by 64 (a scale 64 times its neighbours') - and per utterance the float64 logits behind the int8-rule cross K/V and
    behind the unquantised one"""
    from enc_i8_ref import cross_kv, decoder_logits
    w, a, mels, _, models = tiny
    mem = _encode(lib, models["int8"]._replicas[0].handle, mels, a["d_model"])
    mem = np.ascontiguousarray(np.stack([mem[0], mem[1], mem[0]]))
    mem[1, 700], mem[1, 701] = 0, mem[1, 701] * 64
    assert np.array_equal(mem, mem.astype(np.float16).astype(np.float32))      # (f16 values: the engine's f32 -> f16 of the block changes nothing)
    two = [{q: decoder_logits(w, a, cross_kv(w, a, mem[b], quant=q), TOKENS) for q in (True, False)} for b in range(2)]
    return mem, [two[0], two[1], two[0]]


@pytest.mark.parametrize("B", [1, 3])
def test_cross_kv_int8_route_against_float64(tiny, ckv_refs, lib, B):
    """synthetic:tiny has four decoder layers (the layer strides of both images and of the scale vector matter); N = 3072, so B = 1 takes the 128 x 128
    form (72 tiles of 256 x 256 would be too few) and B = 3 the 256 x 256 one (12 x 18 = 216 tiles)"""
    w, a, _, _, models = tiny
    mem, refs = ckv_refs
    assert a["n_dec_layers"] == 4 and _pick(B * 1500, 4 * 2 * a["d_model"]) == (1 if B == 1 else 3)
    got8, got16 = (_logits(lib, models[k]._replicas[0].handle, np.ascontiguousarray(mem[:B]), a["n_vocab"]) for k in ("int8", "f16"))
    ref8, ref16 = (np.stack([refs[b][q] for b in range(B)]) for q in (True, False))
    e8, e16, cost = rel(got8, ref8), rel(got16, ref16), rel(got8, ref16)
    per = ", ".join(f"{rel(got8[b], ref8[b]):.3e} / {rel(got16[b], ref16[b]):.3e}" for b in range(B))
    print(f"cross K/V int8 route B {B}: e8 {e8:.3e}  e16 {e16:.3e}  int8 engine vs unquantised reference {cost:.3e}  (e8 / e16 per utterance: {per})")
    assert np.isfinite(got8).all() and e8 <= 2 * e16, (e8, e16)


def test_all_three_tile_forms_in_one_encoder_pass(tiny, lib):
    """five utterances, M = 7500: QKV (N = 1152) runs 128 x 128, FFN1 (N = 1536) 256 x 256, the attention output and FFN2 (N = 384) 64 x 128"""
    from wis_hip import ctranslate2 as ct2
    w, a, mels, refs, models = tiny
    d, order = a["d_model"], [0, 1, 0, 1, 0]
    assert [_pick(7500, n) for n in (3 * d, 4 * d, d)] == [1, 3, 2]
    x = np.ascontiguousarray(mels[order])
    got, f16 = models["int8"].encode(ct2.StorageView.from_array(x), to_cpu=True).array, models["f16"].encode(ct2.StorageView.from_array(x), to_cpu=True).array
    assert np.array_equal(got.view(np.uint32), _encode(lib, models["int8"]._replicas[0].handle, x, d).view(np.uint32)), "encode() is not one pass of five"
    for slot, i in enumerate(order):
        s, e16, e8 = rel(refs["q32"][i], refs["q64"][i]), rel(f16[slot], refs["f64"][i]), rel(got[slot], refs["q64"][i])
        print(f"encoder int8 B 5 slot {slot} (clip {i}): s {s:.3e}  e16 {e16:.3e}  int8 engine vs int8 reference {e8:.3e}  vs unquantised reference {rel(got[slot], refs['f64'][i]):.3e}")
        assert e8 <= 4 * max(s, e16), (slot, e8, s, e16)
    for same in ([0, 2, 4], [1, 3]):
        assert all(np.array_equal(got[same[0]].view(np.uint32), got[j].view(np.uint32)) for j in same[1:]), same
    kw = dict(beam_size=1, fixed_new_tokens=4)
    sv = ct2.StorageView.from_array(x)
    p, q = models["int8"].generate(sv, [PROMPT] * 5, **kw), models["int8"].generate(models["int8"].encode(sv), [PROMPT] * 5, **kw)
    assert [r.sequences_ids for r in p] == [r.sequences_ids for r in q] and [r.scores for r in p] == [r.scores for r in q]


def seeded_width(d, seed=1234, std=0.02, ln_jitter=0.1):
    """One encoder layer and one decoder layer of width d, drawn as wis_hip.weights.synthetic_weights draws its tensors (a stream per tensor name) -
    except the token embeddings, which no encoder test reads and which stay zero: a width costs about a second to make"""
    from wis_hip import weights as W
    out = {}
    for name, (shape, kind) in W.tensor_shapes(d, 1, n_dec_layers=1).items():
        rng = np.random.Generator(np.random.PCG64([seed, zlib.crc32(name.encode())]))
        if kind == "pos":
            out[name] = W.sinusoids(shape[0], shape[1])
            continue
        if kind == "emb":
            v = np.zeros(shape, np.float32)
        elif kind in ("g", "beta"):
            v = (1.0 if kind == "g" else 0.0) + ln_jitter * rng.standard_normal(shape, dtype=np.float32)
        else:
            v = rng.standard_normal(shape, dtype=np.float32) * np.float32(std)
            if kind == "bqkv":
                v[d:2 * d] = 0.0
            elif kind == "bkv":
                v[:d] = 0.0
        out[name] = v.astype(np.float16)
    return out


@pytest.fixture(scope="module", params=[512, 768, 1024, 1280])
def width(request, golden_dir):
    """(d, arch, mels, references by name, models).  The three references of a width (the int8 rule in float64 and in float32, the unquantised encoder
    in float64: some 250 GFLOP at d = 1280) are made once, and for the second (rolled) clip only where B = 2 runs (512 and 1280); measured with 16
    CPU threads: 1.1 s (768) to 3.8 s (1280, two clips) for the whole fixture, the two models included - no width needs its float32 run left out"""
    import torch  # noqa: F401
    from enc_i8_ref import encode
    from wis_hip import weights as W
    d = request.param
    mels = tiny_rig(golden_dir)[2][:2 if d in (512, 1280) else 1]
    w = seeded_width(d)
    a = W.arch_from_weights(w)
    assert (a["d_model"], a["n_heads"], a["n_enc_layers"], a["n_dec_layers"]) == (d, d // 64, 1, 1)
    refs = {k: [encode(w, a, m, quant=q, dtype=dt) for m in mels] for k, (q, dt) in
            {"q64": (True, np.float64), "q32": (True, np.float32), "f64": (False, np.float64)}.items()}
    models = {"int8": _model(w, a, max_batch=2, encoder_compute_type="int8"), "f16": _model(w, a, max_batch=2)}
    yield d, a, mels, refs, models
    for m in models.values():
        m.close()


def test_real_widths(width, lib):
    """d = 512 .. 1280 with encoder_weight_bits = 8: to_i8_mat at every width, layernorm_quant_kernel with two to five of its eight rounds live,
    quant_rows_kernel<10> on the FFN hidden rows (K = 4 d > 2048 from d = 768 on), FFN2 unsplit at K = 4 d.  d = 1280, one utterance: QKV and FFN1 on
    128 x 128, the attention output and FFN2 (K = 5120) on 64 x 128; two utterances: QKV and FFN1 on 256 x 256, FFN2 on 128 x 128 at K = 5120.
    The rule is test_gpu_enc_i8.py's, with s and e16 of the width and clip at hand"""
    d, a, mels, refs, models = width
    if d == 1280:
        assert [[_pick(B * 1500, n) for n in (3 * d, 4 * d, d)] for B in (1, 2)] == [[1, 1, 2], [3, 3, 1]]
    for B in range(1, len(mels) + 1):
        got, f16 = (_encode(lib, models[k]._replicas[0].handle, np.ascontiguousarray(mels[:B]), d) for k in ("int8", "f16"))
        for i in range(B):
            s, e16, e8 = rel(refs["q32"][i], refs["q64"][i]), rel(f16[i], refs["f64"][i]), rel(got[i], refs["q64"][i])
            print(f"encoder int8 d {d} B {B} utterance {i} (forms of QKV / FFN1 / FFN2 {[_pick(B * 1500, n) for n in (3 * d, 4 * d, d)]}): s {s:.3e}  e16 {e16:.3e}  "
                  f"int8 engine vs int8 reference {e8:.3e}  vs unquantised reference {rel(got[i], refs['f64'][i]):.3e}")
            assert np.isfinite(got[i]).all() and e8 <= 4 * max(s, e16), (d, B, i, e8, s, e16)


def test_clones_carry_the_int8_encoder(tiny, lib):
    """inter_threads = 2: replica 1 is wis_model_clone of replica 0 (the int8 matrices, their scales and the cross-K/V image are shared, the activation
    and memory quantisation buffers are the clone's own)"""
    w, a, mels, _, _ = tiny
    m = _model(w, a, max_batch=2, inter_threads=2, encoder_compute_type="int8")
    try:
        assert len(m._replicas) == 2
        h0, h1 = (r.handle for r in m._replicas)
        first = (_encode(lib, h0, mels, a["d_model"]), *_generate(lib, h0, mels))
        clone = (_encode(lib, h1, mels, a["d_model"]), *_generate(lib, h1, mels))
        again = (_encode(lib, h0, mels, a["d_model"]), *_generate(lib, h0, mels))
        for other in (clone, again):
            assert np.array_equal(first[0].view(np.uint32), other[0].view(np.uint32)) and np.array_equal(first[1], other[1])
            assert np.array_equal(first[2].view(np.uint32), other[2].view(np.uint32))
        assert np.isfinite(first[0]).all() and first[0].any()
    finally:
        m.close()
