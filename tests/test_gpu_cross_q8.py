"""-m gpu: the int8 cross K/V (cross_kv_compute_type="int8"; csrc/cross_q8.hip): quantiser bit for bit, attention against float64 under cross_q8_ref's bound
(dec_attn_ref's reference / n_acc_cross behind it), the engine's images, logits against the CPU oracle (oracle/whisper_ref.py's decoder in float64 through
enc_i8_ref.decoder_logits; the step route through wis_debug_logits_rows, wis_debug_logits' path at one row).  Figures: profiles/cross_kv_int8_ab.md."""
import ctypes as C

import numpy as np
import pytest

import cross_q8_ref as Q
import dec_attn_ref as D
from dec_attn_ref import k_image, ratios, vt_image, xf_index

pytestmark = pytest.mark.gpu
_f32p, _i32p = C.POINTER(C.c_float), C.POINTER(C.c_int32)
PROMPT = [50258, 50259, 50359, 50363]
TOKENS = PROMPT + [1000, 2000, 3000, 4000]
LOGITS_CAP = 0.004      # twice the rel-L2 measured on the GPU (profiles/cross_kv_int8_ab.md: 1.69e-3 step route, 1.81e-3 batched), one significant digit up
RS = [1, 5, 8, 16]


def _filled(n, dt):
    return np.full(n * np.dtype(dt).itemsize, 0x5A, np.uint8).view(dt)


@pytest.mark.parametrize("T", [1, 63, 64, 65, 1500])
@pytest.mark.parametrize("B,H", [(1, 1), (1, 3), (2, 1), (2, 3)])
def test_quantiser_bit_for_bit(lib, B, H, T):
    from wis_hip._lib import DevBuf, check
    L, d, Tpad, rng = 2, 64 * H, D.cdiv(T, 64) * 64, np.random.default_rng([B, H, T])
    K, V = (rng.standard_normal((L, B, T, d)) * np.exp(rng.uniform(-6, 6, (L, B, T, 1)))).astype(np.float16), rng.standard_normal((L, B, T, d)).astype(np.float16)
    den = (rng.integers(1, 0x400, (L, B, 64), dtype=np.uint16) | (rng.integers(0, 2, (L, B, 64), dtype=np.uint16) << 15)).view(np.float16)
    for X in (K, V):      # one key all zeros (scale 1), one with a single 65504, one of f16 denormals (later marks win where T < 3)
        X[:, :, 0 % T, :64], X[:, :, 2 % T, :64] = 0, den
        X[:, :, 1 % T, :64], X[:, :, 1 % T, 7] = 0, 65504
    kls, vls, qls, sls, G = B * H * 64 * T + 8, B * H * 64 * Tpad + 16, B * H * 64 * Tpad + 32, B * H * Tpad + 4, 16      # layer strides with slack, guard words
    kx, vt, *want = (_filled(L * n + G, t) for n, t in ((kls, np.float16), (vls, np.float16), (qls, np.int8), (qls, np.int8), (sls, np.float32), (sls, np.float32)))
    for l in range(L):
        kx[l * kls:l * kls + B * H * 64 * T], vt[l * vls:l * vls + B * H * 64 * Tpad] = k_image(K[l]).reshape(-1), vt_image(V[l], Tpad, D.PAT16).reshape(-1)
        for w, img, n in zip(want, Q.images(K[l], V[l], Tpad), (qls, qls, sls, sls)):
            w[l * n:l * n + img.size] = img.reshape(-1)
    din, dout = [DevBuf.from_numpy(a) for a in (kx, vt)], [DevBuf.from_numpy(_filled(w.size, w.dtype)) for w in want]
    check(lib.wis_op_cross_kv_quant(0, din[0].ptr, din[1].ptr, B, H, T, Tpad, L, kls, vls, *[o.ptr for o in dout], qls, qls, sls))
    for name, o, w in zip(("kq", "vq", "sk", "sv"), dout, want):      # images, scales, padding, stride slack and guard words in one comparison
        assert np.array_equal(o.to_numpy(np.uint8, (w.nbytes,)), w.view(np.uint8)), name


def _attn_problem(B, H, R, T, rng):
    """int8 K / V with scales 2^u, u in [-6, 2] per key (values sized so that scores stay O(5)), a zero key with scale 1, a PEAK key at chunk position 0,
    255 or 256 - one per case, by R, so every (T, B, H) sees all three; queries on dec_attn_ref's f16 grid with q_0 = 4 (the peak's lever, as in make_qkv)"""
    d, pk = 64 * H, min((0, 255, 256)[RS.index(R) % 3], T - 1)
    sk, sv = (np.exp2(rng.integers(-6, 3, (B, H, T))).astype(np.float32) for _ in range(2))
    Kq = np.clip(np.rint(rng.standard_normal((B, T, H, 64)) * 0.6 / sk.transpose(0, 2, 1)[..., None]), -127, 127).astype(np.int8)
    Vq = rng.integers(-127, 128, (B, T, H, 64)).astype(np.int8)
    Kq[..., 0], Kq[:, T // 3], Vq[:, T // 3], sk[..., T // 3], sv[..., T // 3] = 0, 0, 0, 1, 1
    Kq[:, pk, :, 0], sk[..., pk] = 96, 2.0 ** -5      # 96 * 2^-5 * q_0 = 12 = dec_attn_ref.PEAK
    q = np.concatenate([np.concatenate([D.make_control(1, R, rng, True)[0] for _ in range(H)], 1) for _ in range(B)], 0)      # [B R][d]
    q[:, ::64] = 4.0
    return q.astype(np.float32), Kq.reshape(B, T, d), sk, Vq.reshape(B, T, d), sv


@pytest.mark.parametrize("R", RS)
@pytest.mark.parametrize("B,H", [(1, 1), (2, 3)])
@pytest.mark.parametrize("T", [1, 33, 255, 256, 257, 1500])
def test_attention_against_float64(lib, T, B, H, R):
    from wis_hip._lib import DevBuf, check
    rng = np.random.default_rng([T, B, H, R])
    d, M, Tpad, GUARD = 64 * H, B * R, D.cdiv(T, 64) * 64, 64
    q16, Kq, sk, Vq, sv = _attn_problem(B, H, R, T, rng)
    imgs = [DevBuf.from_numpy(a) for a in Q.pack(Kq, sk, Vq, sv, Tpad)]
    forms = [(q16, None, None, None, None)]
    if R <= 8:
        ops = D.fold_operands(q16, rng)
        D.fold_query_check(q16, ops)
        forms += [(ops["q_one"], None, ops["stat"], ops["qcs"], ops["qb"]), (ops["q_a"], ops["q_b"], ops["stat"], ops["qcs"], ops["qb"])]
    refs = {(s, b, h): Q.reference(q16[b * R:b * R + R, 64 * h:64 * h + 64], Kq[b * (1 - s), :, 64 * h:64 * h + 64], sk[b * (1 - s), h],
                                   Vq[b * (1 - s), :, 64 * h:64 * h + 64], sv[b * (1 - s), h]) for s in range(min(B, 2)) for b in range(B) for h in range(H)}
    for fi, form in enumerate(forms):
        bufs = [None if a is None else DevBuf.from_numpy(np.ascontiguousarray(a, np.float32)) for a in form]
        for mb, shared in [(mb, s) for s in range(min(B, 2)) for mb in (0, D.cdiv(M, 16) + 1)]:      # kv_shared: every group reads utterance 0's K / V
            n = D.xf_elems(d, mb) if mb else M * d
            o = DevBuf.from_numpy(_filled(n + GUARD, np.uint16))
            check(lib.wis_op_dec_cross_attn_q8(0, *[b_.ptr if b_ else None for b_ in bufs], *[i.ptr for i in imgs], o.ptr, B, R, H, T, 6, mb, shared))
            raw = o.to_numpy(np.uint16, (n + GUARD,))
            assert (raw[n:] == 0x5A5A).all(), "guard words behind the output were written"
            idx = xf_index(np.arange(M)[:, None], np.arange(d)[None, :], mb) if mb else np.arange(n).reshape(M, d)
            rows = raw[idx].view(np.float16)
            assert not np.delete(raw[:n], idx.reshape(-1)).any(), "the fragment image outside rows [0, M) was written"
            for (s, b, h), (ref, unit) in refs.items():
                if s == shared:
                    r = ratios(rows[b * R:b * R + R, 64 * h:64 * h + 64], ref, unit).max()
                    assert r <= 2, (fi, mb, shared, b, h, float(r))


@pytest.fixture(scope="module")
def rig(golden_dir):
    import torch  # noqa: F401  (before libwis_hip.so: one HIP runtime per process)
    from enc_i8_taps import tiny_rig
    from wis_hip import ctranslate2 as ct2
    w, a, mels, _ = tiny_rig(golden_dir)
    models = {(ckv, enc): ct2.Whisper("unused", weights=w, arch=a, max_batch=5, max_beam=5, cross_kv_compute_type=ckv, encoder_compute_type=enc)
              for ckv in ("int8", "float16") for enc in ("float16", "int8")}
    rng = np.random.default_rng(7)
    mem = (rng.standard_normal((5, 1500, a["d_model"])) * np.exp(rng.uniform(-2, 2, (5, 1500, 1)))).astype(np.float16).astype(np.float32)
    yield w, a, mels, mem, models
    for m in models.values():
        m.close()


def _logits(lib, h, mem, V, R):
    from wis_hip import _lib
    B, dec_in = mem.shape[0], np.ascontiguousarray(np.tile(np.asarray(TOKENS, np.int32), (mem.shape[0], 1)))
    out = np.zeros((B, len(TOKENS), V), np.float32)
    _lib.check(lib.wis_debug_logits_rows(h, _lib.ptr(mem), _lib.WIS_IN_ENC_HOST, B, dec_in.ctypes.data_as(_i32p), len(TOKENS), R, out.ctypes.data_as(_f32p)))
    return out


def _f16_images(lib, h, l, b, H):
    from wis_hip import _lib
    kx, vt, flag = np.zeros((1, H, 8, 1500, 8), np.float16), np.zeros((1, H, 64, 1536), np.float16), C.c_int(-1)
    _lib.check(lib.wis_debug_cross_kv(h, l, b, _lib.ptr(kx), _lib.ptr(vt), None, None, None, None, C.byref(flag)))
    assert flag.value == 0
    return kx.transpose(0, 3, 1, 2, 4).reshape(1, 1500, 64 * H), vt[..., :1500].transpose(0, 3, 1, 2).reshape(1, 1500, 64 * H)


@pytest.mark.parametrize("enc", ["float16", "int8"])
@pytest.mark.parametrize("B", [1, 2])
def test_engine_builds_what_the_taps_build(rig, lib, B, enc):
    from wis_hip import _lib
    _, a, _, mem, models = rig
    H, flag, h8, h16 = a["n_heads"], C.c_int(), *(models[(c, enc)]._replicas[0].handle for c in ("int8", "float16"))
    for h in (h8, h16):
        _logits(lib, h, np.ascontiguousarray(mem[:B]), a["n_vocab"], 1)      # (runs run_cross_kv on the block)
    for l, b in np.ndindex(a.get("n_dec_layers", a["n_layers"]), B):
        got = [np.zeros((1, H, 4, 1536, 16), np.int8), np.zeros((1, H, 64, 1536), np.int8), np.zeros((1, H, 1536), np.float32), np.zeros((1, H, 1536), np.float32)]
        _lib.check(lib.wis_debug_cross_kv(h8, l, b, None, None, *[_lib.ptr(g) for g in got], C.byref(flag)))
        assert flag.value == 1
        for name, g, wnt in zip(("kq", "vq", "sk", "sv"), got, Q.images(*_f16_images(lib, h16, l, b, H), 1536)):
            assert np.array_equal(g, wnt), (name, l, b)


def test_an_ext_of_the_old_size_creates_an_f16_handle(rig, lib, monkeypatch):      # size 8 = the struct before cross_kv_bits: the 8 behind it is not read
    from wis_hip import _lib, ctranslate2 as ct2
    w, a, _, mem, _ = rig
    monkeypatch.setattr(ct2._lib, "ModelExt", type("Old", (_lib.ModelExt,), {"__init__": lambda self, size, enc, ckv, base=_lib.ModelExt: base.__init__(self, 8, enc, ckv)}))
    m = ct2.Whisper("unused", weights=w, arch=a, max_batch=1, max_beam=1, cross_kv_compute_type="int8")
    _logits(lib, m._replicas[0].handle, np.ascontiguousarray(mem[:1]), a["n_vocab"], 1)
    assert _f16_images(lib, m._replicas[0].handle, 0, 0, a["n_heads"])[0].any()      # (asserts is_int8 == 0 on the way)
    m.close()


@pytest.mark.parametrize("B,R", [(1, 1), (1, 8), (2, 8), (5, 8)])      # the step route at 1 and 8 rows per pass, the batched route at 16 and 40
def test_logits_against_the_cpu_oracle(rig, lib, B, R):
    from enc_i8_ref import cross_kv, decoder_logits
    from enc_i8_taps import rel
    w, a, _, mem, models = rig
    block = np.ascontiguousarray(mem[:B])
    want = np.stack([decoder_logits(w, a, cross_kv(w, a, block[b], quant=False, f16=False), TOKENS) for b in range(B)])
    assert rel(_logits(lib, models[("int8", "float16")]._replicas[0].handle, block, a["n_vocab"], R), want) <= LOGITS_CAP < 0.1


@pytest.mark.parametrize("beam", [1, 5])
@pytest.mark.parametrize("B", [1, 2])
def test_generate_is_deterministic_and_clones_match(rig, lib, B, beam):
    from wis_hip import _lib
    mels, parent, clone = rig[2], rig[4][("int8", "float16")]._replicas[0].handle, C.c_void_p()
    _lib.check(lib.wis_model_clone(parent, C.byref(clone)))
    runs = []
    for h in (parent, parent, clone):
        o, x = _lib.GenOpts(0, beam, 0, 1.0, 1.0, 1, 1, 6, 0), np.ascontiguousarray(mels[:B])
        prompt, ids, lens, sc = np.ascontiguousarray(np.tile(np.asarray(PROMPT, np.int32), (B, 1))), np.zeros((B, 224), np.int32), np.zeros(B, np.int32), np.zeros(B, np.float32)
        _lib.check(lib.wis_generate(h, _lib.ptr(x), B, prompt.ctypes.data_as(_i32p), 4, C.byref(o), ids.ctypes.data_as(_i32p), lens.ctypes.data_as(_i32p), sc.ctypes.data_as(_f32p)))
        runs.append((ids.copy(), lens.copy(), sc.view(np.uint32).copy()))
    lib.wis_model_destroy(clone)
    assert (runs[0][1] == 6).all() and all(np.array_equal(x, y) for r in runs[1:] for x, y in zip(runs[0], r)), "the second run or the clone differs"
