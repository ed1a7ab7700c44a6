"""-m gpu: the cross-K/V projection that writes the int8 images from its own epilogue (csrc/cross_q8.hip cross_kv_q8_fused_kernel, wis_op_enc_crosskv_q8).

Int8 operands: bit for bit against enc_i8_ref.cross_kv_from in float32 (the integer sum is exact, the f32 expression is the kernel's) + cross_q8_ref.images.
F16 operands: against P = float64(mem . W^T + bias), rounded to f16, + images.  The kernel's value is f16(P32), P32 the f32 MFMA sum plus the bias:
  ACC  every product reaches the result through at most d f32 additions (the chain's links in k order, a tree inside a link: never deeper than the
       sequential sum) and one more for the bias, each off by 2^-24 of a partial sum that sum |a_k w_k| + |bias| bounds: ACC = (d + 1) 2^-24 (sum |a w| + |b|).
       No margin factor on top: the sequential count already over-counts the tree.
  scale  the two absmax are f16 roundings (half an ulp each) of values at most the row's largest ACC apart: one f16 ulp of the larger + ACC; scale =
       absmax / 127 rounds once more in f32.  Zero rows and padding keys: exactly 1.
  value  q scale is within scale / 2 of f16(P32) (rint; |x inv| <= 127 (1 + 2^-22) never clips more), which is within half an f16 ulp of P32, itself within
       ACC of P: the issue's scale / 2 + one f16 ulp of the value + ACC leaves half an ulp for the f32 roundings of x * inv (127 2^-23 scale at most).
       Measured worst ratio to that bound: 0.999 - 1.000 on every case (rint's ties meet the scale / 2 term exactly; the rest is slack).
  bytes  at most 1 in 1000 differs from the reference's byte, and then by exactly 1 (an f16 rounding that fell on the other side); numpy's own float32
       GEMM is held to the same cap first, on the CPU."""
import ctypes as C

import numpy as np
import pytest

import cross_q8_ref as Q
from prep_ref import U16, U24

pytestmark = pytest.mark.gpu
GUARD = 64      # sentinel bytes in front of and behind every output
CASES = [(1500, B, H, L) for B in (1, 2) for H in (1, 6) for L in (1, 3)] + [(64, 1, 1, 1), (65, 1, 1, 1)]


def _problem(T, B, H, L):
    """mem f16 [B][T][d] with a scale per row and key 1 all zeros; W f16 [L 2d][d]; bias f32 [L 2d]: layer 0 has a zero bias on V head 0 (key 1's V row is
    all zeros: scale 1, zero bytes) and on K head 0 but for 40 in its LAST column (every key's absmax of that head sits there)"""
    d, rng = 64 * H, np.random.default_rng([T, B, H, L])
    mem = (rng.standard_normal((B, T, d)) * np.exp(rng.uniform(-2, 2, (B, T, 1)))).astype(np.float16)
    mem[:, 1] = 0
    W, bias = (rng.standard_normal((L * 2 * d, d)) / np.sqrt(d)).astype(np.float16), rng.standard_normal(L * 2 * d).astype(np.float32)
    bias[:64], bias[d:d + 64], bias[63] = 0, 0, 40
    return mem, W, bias


def _want(KV16, B, T, d, L, Tpad):      # f16 [B T][L 2d] -> the four images of all layers, layer after layer
    kv = KV16.reshape(B, T, L, 2, d)
    per = [Q.images(kv[:, :, l, 0], kv[:, :, l, 1], Tpad) for l in range(L)]
    return [np.stack([p[i] for p in per]) for i in range(4)]


def _run(lib, A, sa, W, sw, bias, B, T, Tpad, H, L):
    from wis_hip._lib import DevBuf, check
    n = L * B * H * Tpad
    outs = [DevBuf.from_numpy(np.full(2 * GUARD + nb, 0x5A, np.uint8)) for nb in (64 * n, 64 * n, 4 * n, 4 * n)]
    ins = [None if a is None else DevBuf.from_numpy(a) for a in (A, sa, W, sw, bias)]
    check(lib.wis_op_enc_crosskv_q8(0, *[i.ptr if i else None for i in ins], *[C.c_void_p(o.ptr.value + GUARD) for o in outs], B, T, Tpad, H, 64 * H, L))
    raw = [o.to_numpy(np.uint8, (o.nbytes,)) for o in outs]
    assert all((r[:GUARD] == 0x5A).all() and (r[-GUARD:] == 0x5A).all() for r in raw), "sentinel bytes around an output were written"
    kq, vq, sk, sv = (r[GUARD:-GUARD] for r in raw)
    return kq.view(np.int8).reshape(L, B, H, 4, Tpad, 16), vq.view(np.int8).reshape(L, B, H, 64, Tpad), sk.view(np.float32).reshape(L, B, H, Tpad), sv.view(np.float32).reshape(L, B, H, Tpad)


@pytest.mark.parametrize("T,B,H,L", CASES)
def test_int8_operands_bit_for_bit(lib, T, B, H, L):
    from enc_i8_ref import cross_kv_from
    from wis_hip.weights import quantize_rows
    d, Tpad = 64 * H, -(-T // 64) * 64
    mem, W, bias = _problem(T, B, H, L)
    (qa, sa), (qw, sw) = quantize_rows(mem.reshape(B * T, d)), quantize_rows(W)
    layers = [(qw[l * 2 * d:(l + 1) * 2 * d], sw[l * 2 * d:(l + 1) * 2 * d], bias[l * 2 * d:(l + 1) * 2 * d]) for l in range(L)]
    KV = np.concatenate([np.concatenate(kv, 1) for kv in cross_kv_from(qa, sa, layers, dtype=np.float32)], 1).astype(np.float16)
    want = _want(KV, B, T, d, L, Tpad)
    assert (want[3][0, :, 0, 1] == 1).all()      # key 1 of V head 0: the zero row
    for name, g, w in zip(("kq", "vq", "sk", "sv"), _run(lib, qa, sa, qw, sw, bias, B, T, Tpad, H, L), want):
        assert np.array_equal(g, w), name


def _byte_cap(got, want, who):
    diff = np.abs(got.astype(np.int16) - want.astype(np.int16))
    assert diff.max(initial=0) <= 1 and (diff != 0).mean() <= 1e-3, (who, int(diff.max()), float((diff != 0).mean()))
    return float((diff != 0).mean())


@pytest.mark.parametrize("T,B,H,L", CASES)
def test_f16_operands_against_float64(lib, T, B, H, L):
    d, Tpad, F = 64 * H, -(-T // 64) * 64, np.float64
    mem, W, bias = _problem(T, B, H, L)
    a = mem.reshape(B * T, d)
    P = a.astype(F) @ W.astype(F).T + bias.astype(F)
    acc = (d + 1) * U24 * (np.abs(a).astype(F) @ np.abs(W).astype(F).T + np.abs(bias))
    ulp = np.spacing(np.abs(P).astype(np.float16)).astype(F)
    want = _want(P.astype(np.float16), B, T, d, L, Tpad)
    mine = _want((a.astype(np.float32) @ W.astype(np.float32).T + bias).astype(np.float16), B, T, d, L, Tpad)      # numpy's float32 sum under the same cap
    for i in range(2):
        _byte_cap(mine[i], want[i], "float32 restatement")
    got = _run(lib, a, None, W, None, bias, B, T, Tpad, H, L)
    assert (want[3][0, :, 0, 1] == 1).all() and (got[3][0, :, 0, 1] == 1).all()
    p, arow = P.reshape(B, T, L, 2, H, 64), acc.reshape(B, T, L, 2, H, 64).max(-1)
    for i in (2, 3):      # scales: (one f16 ulp of the larger absmax + the row's ACC) / 127, and the f32 rounding of the quotient; zero rows and padding exact
        mx = np.maximum(got[i], want[i]).astype(F) * 127
        tol = np.spacing((mx * (1 + U16)).astype(np.float16)).astype(F) / 127 + 2 * U24 * mx
        tol[..., :T] += arow[:, :, :, i - 2].transpose(2, 0, 3, 1) / 127
        assert (np.abs(got[i].astype(F) - want[i]) <= np.where(want[i] == 1, 0, tol)).all(), ("sk", "sv")[i - 2]
    # values: undo the layouts (cross_q8_ref.pack) and hold q scale against P
    kq = got[0][..., :T, :].reshape(L, B, H, 4, T, 2, 8).transpose(1, 4, 0, 2, 5, 3, 6).reshape(B, T, L, H, 64)
    vq = got[1].reshape(L, B, H, 64, Tpad // 64, 4, 2, 8).transpose(1, 4, 6, 5, 7, 0, 2, 3).reshape(B, Tpad, L, H, 64)
    assert not got[0][..., T:, :].any() and not vq[:, T:].any(), "padding keys hold values"
    vq, worst = vq[:, :T], 0.0
    for q, s, c in ((kq, got[2], 0), (vq, got[3], 1)):
        sc = s[..., :T].transpose(1, 3, 0, 2)[..., None].astype(F)      # [B][T][L][H][1]
        ref, bound = p[:, :, :, c], sc / 2 + ulp.reshape(p.shape)[:, :, :, c] + acc.reshape(p.shape)[:, :, :, c]
        worst = max(worst, float((np.abs(q * sc - ref) / bound).max()))
    print(f"fused f16 T={T} B={B} H={H} L={L}: worst |q scale - P| / bound {worst:.3f}; bytes off by one: kq {_byte_cap(got[0], want[0], 'kq'):.2e} vq {_byte_cap(got[1], want[1], 'vq'):.2e}")
    assert worst <= 1


@pytest.mark.parametrize("H,L,B", [(6, 4, 1), (6, 4, 2), (4, 16, 2)])      # the ping-pong tile, the 128 x 128 tile, the 8-phase kernel (its own MFMA chain)
def test_f16_operands_repeat_the_two_launch_bits(lib, H, L, B):
    from wis_hip._lib import DevBuf, check
    T, Tpad, d = 1500, 1536, 64 * H
    mem, W, bias = _problem(T, B, H, L)
    kls, vls, n = B * T * d, B * d * Tpad, L * B * H * Tpad
    ins = [DevBuf.from_numpy(x) for x in (mem, W, bias)]
    kx, vt = DevBuf.from_numpy(np.zeros(L * kls, np.float16)), DevBuf.from_numpy(np.zeros(L * vls, np.float16))
    two = [DevBuf(nb) for nb in (64 * n, 64 * n, 4 * n, 4 * n)]
    check(lib.wis_op_enc_crosskv(0, *[i.ptr for i in ins], kx.ptr, vt.ptr, B, T, H, L, kls, vls))
    check(lib.wis_op_cross_kv_quant(0, kx.ptr, vt.ptr, B, H, T, Tpad, L, kls, vls, *[o.ptr for o in two], vls, vls, B * H * Tpad))
    for name, g, o in zip(("kq", "vq", "sk", "sv"), _run(lib, mem.reshape(B * T, d), None, W, None, bias, B, T, Tpad, H, L), two):
        assert np.array_equal(g.reshape(-1).view(np.uint8), o.to_numpy(np.uint8, (o.nbytes,))), name


@pytest.fixture(scope="module")
def rig(golden_dir):
    import torch  # noqa: F401  (before libwis_hip.so: one HIP runtime per process)
    from enc_i8_taps import tiny_rig
    from wis_hip import ctranslate2 as ct2
    w, a, _, _ = tiny_rig(golden_dir)
    models = {(ckv, enc): ct2.Whisper("unused", weights=w, arch=a, max_batch=5, max_beam=5, cross_kv_compute_type=ckv, encoder_compute_type=enc)
              for ckv in ("int8", "float16") for enc in ("float16", "int8")}
    rng = np.random.default_rng(7)
    yield w, a, (rng.standard_normal((2, 1500, a["d_model"])) * np.exp(rng.uniform(-2, 2, (2, 1500, 1)))).astype(np.float16), models
    for m in models.values():
        m.close()


@pytest.mark.parametrize("enc", ["float16", "int8"])
@pytest.mark.parametrize("B", [1, 2])
def test_engine_holds_the_tap_s_images_and_no_staging(rig, lib, B, enc):
    from enc_i8_ref import cross_kv_parts
    from wis_hip import _lib
    w, a, mem, models = rig
    H, d, L, T, Tpad, Bm = a["n_heads"], a["d_model"], a.get("n_dec_layers", a["n_layers"]), 1500, 1536, 5
    h8, h16 = (models[(c, enc)]._replicas[0].handle for c in ("int8", "float16"))
    block, dec_in, out = np.ascontiguousarray(mem[:B], np.float32), np.full((B, 1), 50258, np.int32), np.zeros((B, 1, a["n_vocab"]), np.float32)
    _lib.check(lib.wis_debug_logits_rows(h8, _lib.ptr(block), _lib.WIS_IN_ENC_HOST, B, dec_in.ctypes.data_as(C.POINTER(C.c_int32)), 1, 1, out.ctypes.data_as(C.POINTER(C.c_float))))
    qa, sa, layers = cross_kv_parts(w, a, mem[:B].reshape(B * T, d))
    if enc == "int8":
        ops = (qa, sa, np.concatenate([l[0] for l in layers]), np.concatenate([l[1] for l in layers]))
    else:
        ops = (mem[:B].reshape(B * T, d), None, np.concatenate([np.asarray(w[f"decoder/layer_{l}/attention/linear_1/weight"], np.float32) for l in range(L)]).astype(np.float16), None)
    tap = _run(lib, *ops, np.concatenate([l[2] for l in layers]), B, T, Tpad, H, L)
    flag = C.c_int()
    for l, b in np.ndindex(L, B):
        got = [np.zeros((H, 4, Tpad, 16), np.int8), np.zeros((H, 64, Tpad), np.int8), np.zeros((H, Tpad), np.float32), np.zeros((H, Tpad), np.float32)]
        _lib.check(lib.wis_debug_cross_kv(h8, l, b, None, None, *[_lib.ptr(g) for g in got], C.byref(flag)))
        for name, g, t in zip(("kq", "vq", "sk", "sv"), got, tap):
            assert flag.value == 1 and np.array_equal(g, t[l, b]), (name, l, b)
    # memory: the f16 images against the int8 images + scales, and no staging block (min(L, 4) layers of both f16 images at the parent) beside them
    f16_images = L * Bm * H * 64 * (T + Tpad) * 2
    saving, staging = f16_images - L * Bm * H * Tpad * (2 * 64 + 2 * 4), min(L, 4) * Bm * H * 64 * (T + Tpad) * 2
    assert abs((lib.wis_model_device_bytes(h16) - lib.wis_model_device_bytes(h8)) - saving) < 2 ** 20 < staging
