"""-m gpu: what run_encoder / run_cross_kv launch, one launch at a time, against float64 - element by element.

The taps (wis_op_mel_to_image, wis_op_enc_conv, wis_op_enc_qkv, wis_op_enc_crosskv, wis_op_gemm_splitk_ln) call the product's launch_gemm_* functions on the
GEMM descriptions the encoder itself builds; the shapes below are the smallest that reach every tile / kernel form gemm_pick_tile and launch_gemm_t choose
between (the kernel named beside each case is the one a kernel trace of this file showed: profiles/enc_ops_tests.md).

Every written output element obeys   |out - ref| <= c 2^-24 S + r,   S = |A| |W|^T + |bias| (+ |residual| / |positions|) in float64 on the same f16 operands,
r = 2^-10 |ref| for f16 outputs (one f16 rounding is 2^-11) and 0 for fp32 ones; behind a GELU the bound is taken on the pre-activation and multiplied by
GELU's Lipschitz constant 1.13.  c stands for the fp32 accumulation of the MFMA chain (+ the K-split sums, + the fp32 epilogue arithmetic): its worst case is
K; C_BOUND holds, per op, 4 x the largest ratio (|out - ref| - r) / (2^-24 S) seen on an MI355X over all cases, rounded up to a power of two (the figures:
profiles/enc_ops_tests.md).  Every element an op must not write keeps the bit pattern the buffer was filled with, and two runs agree to the bit."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -24
F16_R = 2.0 ** -10
GELU_LIP = 1.13
# per op: 4 x the worst observed ratio, rounded up to a power of two (profiles/enc_ops_tests.md); never more than K (asserted per case)
C_BOUND = {"qkv": 4, "crosskv": 4, "conv1": 1, "conv2": 8, "splitk_ln": 8}
PAT16, PAT32 = 0x5A5A, 0x5A5A5A5A      # f16 203.25 / f32 1.5e16: nothing these ops produce


def _pattern(n, dt):
    return np.full(n, PAT16 if dt == np.float16 else PAT32, np.uint16 if dt == np.float16 else np.uint32).view(dt)


def _is_pattern(a):
    return (a.view(np.uint16) == PAT16) if a.dtype == np.float16 else (a.view(np.uint32) == PAT32)


def _same_bits(a, b):
    return np.array_equal(a.view(np.uint8), b.view(np.uint8))


def _gelu(x):
    from scipy.special import erf
    return 0.5 * x * (1.0 + erf(x / np.sqrt(2.0)))


def _mm(a, b):
    """a [M][K] . b [N][K]^T in float64 (torch: the conftest keeps it to <= 16 threads)"""
    import torch
    return (torch.from_numpy(np.ascontiguousarray(a)) @ torch.from_numpy(np.ascontiguousarray(b)).T).numpy()


def _gemm_ref(A16, W16):
    """float64 product and magnitude sum of f16 (or f16-valued) operands"""
    A, W = A16.astype(np.float64), W16.astype(np.float64)
    return _mm(A, W), _mm(np.abs(A), np.abs(W))


def _relerr(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / (np.linalg.norm(b) + 1e-30))


def _check(tag, op, K, out, ref, unit, f16_out):
    """every element: |out - ref| <= C_BOUND[op] * unit + r; unit = 2^-24 S (times whatever the value passes through afterwards)"""
    c = C_BOUND[op]
    assert c <= K, (op, c, K)
    err = np.abs(out.astype(np.float64) - ref)
    r = F16_R * np.abs(ref) if f16_out else 0.0
    ratio = np.maximum(err - r, 0.0) / unit
    worst = float(ratio.max())
    i = np.unravel_index(int(ratio.argmax()), ratio.shape)
    e = _relerr(out, ref)
    print(f"{tag}: max (|out - ref| - r) / (2^-24 S) = {worst:.3f} at {tuple(int(x) for x in i)} (c = {c}, K = {K}); rel-L2 {e:.3e}")
    assert np.isfinite(out).all(), tag
    assert worst <= c, (tag, worst, c, i)
    assert e < (2e-3 if f16_out else 1e-4), (tag, e)
    return worst


def _swz(t):
    return (t & ~12) | ((t & 4) << 1) | ((t & 8) >> 1)


def _rand16(rng, shape, s):
    return (rng.standard_normal(shape) * s).astype(np.float16)


# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_mels", [80, 128])
def test_mel_to_image(lib, n_mels):
    from wis_hip._lib import DevBuf, check
    B, C = 2, 96 if n_mels == 80 else 128
    rng = np.random.default_rng(n_mels)
    mel = rng.standard_normal((B, n_mels, 3000)).astype(np.float32)
    d_mel = DevBuf.from_numpy(mel)
    outs = []
    for _ in range(2):
        d_img = DevBuf.from_numpy(_pattern(B * 3002 * C, np.float16))
        check(lib.wis_op_mel_to_image(0, d_mel.ptr, d_img.ptr, B, n_mels))
        outs.append(d_img.to_numpy(np.float16, (B, 3002, C)))
    img = outs[0]
    assert _same_bits(outs[0], outs[1])
    assert _is_pattern(img[:, 0]).all() and _is_pattern(img[:, 3001]).all()
    assert _same_bits(img[:, 1:3001, :n_mels], np.ascontiguousarray(mel.astype(np.float16).transpose(0, 2, 1)))
    assert (img[:, 1:3001, n_mels:].view(np.uint16) == 0).all()


def test_mel_to_image_other_bin_counts_are_refused(lib):
    from wis_hip._lib import DevBuf
    d_mel, d_img = DevBuf(64 * 3000 * 4), DevBuf(3002 * 128 * 2)
    assert lib.wis_op_mel_to_image(0, d_mel.ptr, d_img.ptr, 1, 64) == -7      # WIS_E_UNSUPPORTED


# ---------------------------------------------------------------------------------------
def _run_qkv(lib, xn, W, bias, B, T, H, vt_fill=None):
    from wis_hip._lib import DevBuf, check
    d, M, Tpad = 64 * H, B * T, (T + 63) // 64 * 64
    d_x, d_w, d_b = DevBuf.from_numpy(xn), DevBuf.from_numpy(W), DevBuf.from_numpy(bias)
    d_qk = DevBuf.from_numpy(_pattern(M * 2 * d, np.float16))
    d_vt = DevBuf.from_numpy(_pattern(B * H * 64 * Tpad, np.float16) if vt_fill is None else np.full(B * H * 64 * Tpad, vt_fill, np.float16))
    check(lib.wis_op_enc_qkv(0, d_x.ptr, d_w.ptr, d_b.ptr, d_qk.ptr, d_vt.ptr, B, T, H))
    return d_qk, d_vt, d_qk.to_numpy(np.float16, (M, 2 * d)), d_vt.to_numpy(np.float16, (B, H, 64, Tpad))


# every T is a multiple of 4 and ragged against every tile height; all but 64 and 1232 leave keys beyond T inside the last group of 16
@pytest.mark.parametrize("d,B,T", [
    (384, 1, 64),       # gemm_f16_kernel<EpiQKV, 128, 128>: one row tile (M <= 64 never takes the 64-row tile)
    (384, 1, 300),      # gemm_f16_kernel<EpiQKV, 64, 128>
    (384, 2, 1500),     # gemm_f16_kernel<EpiQKV, 128, 128>: 216 tiles, two utterances, the second starts inside a tile
    (1280, 2, 516),     # gemm_pp_kernel<EpiQKV>: 150 tiles of 256 x 128
    (1280, 1, 1500),    # gemm_pp_kernel<EpiQKV>: large at one utterance
    (1280, 3, 772),     # gemm_8p_kernel<EpiQKV, false> on [Q | K] + gemm_8p_kernel<EpiQKV, true> on V: 150 tiles of 256 x 256
    (1024, 4, 772),     # the same pair, medium's width (M >= 3073)
    (768, 4, 1028),     # ... small's (M >= 4097)
    (512, 5, 1232),     # ... base's (M >= 6145)
])
def test_enc_qkv(lib, d, B, T):
    H, M, Tpad = d // 64, B * T, (T + 63) // 64 * 64
    rng = np.random.default_rng(d * 13 + M)
    xn, W, bias = _rand16(rng, (M, d), 0.5), _rand16(rng, (3 * d, d), 0.1), rng.standard_normal(3 * d).astype(np.float32)
    Z, S = _gemm_ref(xn, W)
    Z += bias; S += np.abs(bias)
    _, _, qk, vt = _run_qkv(lib, xn, W, bias, B, T, H)
    _, _, qk2, vt2 = _run_qkv(lib, xn, W, bias, B, T, H)
    assert _same_bits(qk, qk2) and _same_bits(vt, vt2)
    tag = f"enc_qkv d{d} B{B} T{T}"
    w1 = _check(tag + " [Q|K]", "qkv", d, qk, Z[:, :2 * d], EPS * S[:, :2 * d], True)
    # V^T: key t of an utterance sits at _swz(t); the image positions that hold no key < T stay as they were
    tp = _swz(np.arange(T))
    untouched = np.ones(Tpad, bool); untouched[tp] = False
    assert _is_pattern(vt[..., untouched]).all(), tag + ": wrote V^T positions of keys >= T"
    v_out = vt[..., tp]                                                                   # [B][H][64][T], every key < T
    v_ref = Z[:, 2 * d:].reshape(B, T, H, 64).transpose(0, 2, 3, 1)
    v_S = S[:, 2 * d:].reshape(B, T, H, 64).transpose(0, 2, 3, 1)
    w2 = _check(tag + " V^T", "qkv", d, v_out, v_ref, EPS * v_S, True)
    print(f"RATIO qkv {tag} {max(w1, w2):.3f}")


def test_enc_qkv_refuses_rows_that_are_no_multiple_of_four(lib):
    from wis_hip._lib import DevBuf
    H, T = 6, 30
    d = 64 * H
    bufs = [DevBuf(T * d * 2), DevBuf(3 * d * d * 2), DevBuf(3 * d * 4), DevBuf(T * 2 * d * 2), DevBuf(H * 64 * 64 * 2)]
    assert lib.wis_op_enc_qkv(0, *[b.ptr for b in bufs], 1, T, H) == -1      # WIS_E_ARG


# ---------------------------------------------------------------------------------------
def _run_crosskv(lib, mem, W, bias, B, T, H, L, kx_ls, vt_ls, vt_fill=None):
    """the images live in buffers of L + 1 layer strides: the stride's slack behind EVERY layer, the last one included, must stay untouched"""
    from wis_hip._lib import DevBuf, check
    d_m, d_w, d_b = DevBuf.from_numpy(mem), DevBuf.from_numpy(W), DevBuf.from_numpy(bias)
    d_kx = DevBuf.from_numpy(_pattern((L + 1) * kx_ls, np.float16))
    d_vt = DevBuf.from_numpy(_pattern((L + 1) * vt_ls, np.float16) if vt_fill is None else np.full((L + 1) * vt_ls, vt_fill, np.float16))
    check(lib.wis_op_enc_crosskv(0, d_m.ptr, d_w.ptr, d_b.ptr, d_kx.ptr, d_vt.ptr, B, T, H, L, kx_ls, vt_ls))
    return d_kx, d_vt, d_kx.to_numpy(np.float16, (L + 1, kx_ls)), d_vt.to_numpy(np.float16, (L + 1, vt_ls))


@pytest.mark.parametrize("d,L,B,T,slack", [
    (1280, 4, 2, 388, 136),     # gemm_8p_kernel<EpiCrossKV, false> on every layer's K columns + <EpiCrossKV, true> on its V columns (periodic column split)
    (1280, 2, 2, 388, 136),     # gemm_pp_kernel<EpiCrossKV>
    (512, 6, 4, 388, 72),       # the 8-phase pair, base's width: six layers
    (384, 4, 8, 388, 72),       # gemm_f16_kernel<EpiCrossKV, 256, 256>: the column sets are not tile aligned, 256-wide tiles straddle K | V and layers
    (384, 4, 1, 1500, 8),       # gemm_pp_kernel<EpiCrossKV>: tiny at one utterance
    (384, 1, 1, 300, 0),        # gemm_f16_kernel<EpiCrossKV, 64, 128>
    (768, 2, 4, 836, 72),       # the 8-phase pair, small's width
])
def test_enc_crosskv(lib, d, L, B, T, slack):
    H, M, Tpad = d // 64, B * T, (T + 63) // 64 * 64
    kx_n, vt_n = B * T * d, B * d * Tpad
    kx_ls, vt_ls = kx_n + slack, vt_n + 2 * slack
    rng = np.random.default_rng(d * 7 + L * 1000 + M)
    mem, W = _rand16(rng, (M, d), 0.5), _rand16(rng, (L * 2 * d, d), 0.1)
    bias = (rng.standard_normal(L * 2 * d) + np.repeat(np.arange(L) * 0.5, 2 * d)).astype(np.float32)      # every layer's bias is its own
    Z, S = _gemm_ref(mem, W)
    Z += bias; S += np.abs(bias)
    _, _, kx, vt = _run_crosskv(lib, mem, W, bias, B, T, H, L, kx_ls, vt_ls)
    _, _, kx2, vt2 = _run_crosskv(lib, mem, W, bias, B, T, H, L, kx_ls, vt_ls)
    assert _same_bits(kx, kx2) and _same_bits(vt, vt2)
    tag = f"enc_crosskv d{d} L{L} B{B} T{T}"
    assert _is_pattern(kx[:L, kx_n:]).all() and _is_pattern(kx[L]).all(), tag + ": wrote outside the layers' K images"
    assert _is_pattern(vt[:L, vt_n:]).all() and _is_pattern(vt[L]).all(), tag + ": wrote outside the layers' V^T images"
    vimg = vt[:L, :vt_n].reshape(L, B, H, 64, Tpad)
    assert _is_pattern(vimg[..., T:]).all(), tag + ": wrote V^T positions of keys >= T"
    Zl, Sl = Z.reshape(B, T, L, 2, H, 64), S.reshape(B, T, L, 2, H, 64)
    # K image [B][H][8][T][8]: element (t, 8 g + j) of head h
    k_out = kx[:L, :kx_n].reshape(L, B, H, 8, T, 8)
    k_ref = Zl[:, :, :, 0].reshape(B, T, L, H, 8, 8).transpose(2, 0, 3, 4, 1, 5)
    k_S = Sl[:, :, :, 0].reshape(B, T, L, H, 8, 8).transpose(2, 0, 3, 4, 1, 5)
    w1 = _check(tag + " K image", "crosskv", d, k_out, k_ref, EPS * k_S, True)
    v_ref, v_S = Zl[:, :, :, 1].transpose(2, 0, 3, 4, 1), Sl[:, :, :, 1].transpose(2, 0, 3, 4, 1)      # [L][B][H][64][T]
    w2 = _check(tag + " V^T image", "crosskv", d, vimg[..., :T], v_ref, EPS * v_S, True)
    print(f"RATIO crosskv {tag} {max(w1, w2):.3f}")


def test_enc_crosskv_refuses_bad_rows_and_strides(lib):
    from wis_hip._lib import DevBuf
    H, T, L = 6, 32, 1
    d = 64 * H
    bufs = [DevBuf(T * d * 2), DevBuf(2 * d * d * 2), DevBuf(2 * d * 4), DevBuf(T * d * 2), DevBuf(d * 64 * 2)]
    ptrs = [b.ptr for b in bufs]
    assert lib.wis_op_enc_crosskv(0, *ptrs, 1, 30, H, L, 30 * d, 64 * d) == -1      # T % 4
    assert lib.wis_op_enc_crosskv(0, *ptrs, 1, T, H, L, T * d - 8, 64 * d) == -1      # a stride below the image
    assert lib.wis_op_enc_crosskv(0, *ptrs, 1, T, H, L, T * d, 64 * d + 4) == -1      # a stride that breaks the 16-byte stores


# ---------------------------------------------------------------------------------------
def _conv_rows(img, T, stride):
    """implicit im2col: output row t of an utterance = image rows stride t .. stride t + 2, [B*T][3 C] in float64"""
    B, _, C = img.shape
    out = np.empty((B, T, 3, C), np.float64)
    for k in range(3):
        out[:, :, k] = img[:, k:k + stride * T:stride][:, :T]
    return out.reshape(B * T, 3 * C)


@pytest.mark.parametrize("N,B,T,Cin,w_f16", [
    (384, 1, 3000, 80, 0),       # gemm_f16_kernel<EpiConv1, 64, 128>: tiny, f32 weights as the loader gets them
    (1280, 1, 3000, 80, 1),      # gemm_f16_kernel<EpiConv1, 128, 128>: large at one utterance
    (1280, 2, 1540, 80, 0),      # gemm_8pn_kernel<EpiConv1>: 125 tiles of 128 x 256; the second utterance starts inside a tile
    (1280, 3, 2476, 80, 1),      # gemm_8p_kernel<EpiConv1, false>: 150 tiles of 256 x 256
    (384, 2, 700, 128, 0),       # 128 mel bins: K = 384, no zero-weighted columns (64 x 128 tile)
])
def test_enc_conv1(lib, N, B, T, Cin, w_f16):
    from wis_hip._lib import DevBuf, check
    C = 96 if Cin == 80 else 128
    K = (3 * C + 63) // 64 * 64
    rng = np.random.default_rng(N + B * T + Cin)
    img = np.zeros((B, T + 2, C), np.float16)
    img[:, 1:T + 1, :Cin] = _rand16(rng, (B, T, Cin), 0.5)      # every utterance its own rows
    W = _rand16(rng, (N, Cin, 3), 0.1)
    bias = rng.standard_normal(N).astype(np.float32)
    Wp = np.zeros((N, 3, C), np.float64); Wp[:, :, :Cin] = W.astype(np.float64).transpose(0, 2, 1)
    A = _conv_rows(img, T, 1)
    Z, S = _mm(A, Wp.reshape(N, 3 * C)) + bias, _mm(np.abs(A), np.abs(Wp.reshape(N, 3 * C))) + np.abs(bias)
    d_w = DevBuf.from_numpy(W if w_f16 else W.astype(np.float32))
    d_b = DevBuf.from_numpy(bias)
    outs = []
    for tail in (0.0, 0.0, 60000.0):      # the 64 elements behind the image: the last row's zero-weighted columns read 32 of them at 80 bins
        d_img = DevBuf.from_numpy(np.concatenate([img.reshape(-1), np.full(64, tail, np.float16)]))
        d_out = DevBuf.from_numpy(_pattern(B * (T + 2) * N, np.float16))
        check(lib.wis_op_enc_conv(0, 1, d_img.ptr, d_w.ptr, w_f16, d_b.ptr, None, d_out.ptr, B, T, Cin, N))
        outs.append(d_out.to_numpy(np.float16, (B, T + 2, N)))
    tag = f"enc_conv1 N{N} B{B} T{T} Cin{Cin}"
    assert _same_bits(outs[0], outs[1]), tag + ": two runs differ"
    assert _same_bits(outs[0], outs[2]), tag + ": what lies behind the image reached the result"
    out = outs[0]
    assert _is_pattern(out[:, 0]).all() and _is_pattern(out[:, T + 1]).all(), tag + ": wrote a padding row"
    w = _check(tag, "conv1", K, out[:, 1:T + 1].reshape(B * T, N), _gelu(Z), GELU_LIP * EPS * S, True)
    print(f"RATIO conv1 {tag} {w:.3f}")


@pytest.mark.parametrize("N,B,T", [
    (1280, 1, 1500),     # gemm_f16_kernel<EpiConv2, 64, 128>: large at one utterance
    (1280, 2, 1300),     # gemm_f16_kernel<EpiConv2, 128, 128>
    (1280, 2, 1540),     # gemm_8pn_kernel<EpiConv2> (M >= 3073); m % T wraps inside a tile
    (1280, 3, 2476),     # gemm_8p_kernel<EpiConv2, false> (M >= 7425)
    (384, 2, 300),       # 64 x 128 tile at tiny's width, two utterances in one tile column
])
def test_enc_conv2(lib, N, B, T):
    from wis_hip._lib import DevBuf, check
    Cin, K = N, 3 * N
    rng = np.random.default_rng(N * 3 + B * T)
    img = np.zeros((B, 2 * T + 2, Cin), np.float16)
    img[:, 1:2 * T + 1] = _rand16(rng, (B, 2 * T, Cin), 0.5)
    W = _rand16(rng, (N, Cin, 3), 0.1)
    bias = rng.standard_normal(N).astype(np.float32)
    pos = rng.standard_normal((T, N)).astype(np.float32)      # a row of its own per t
    Wp = W.astype(np.float64).transpose(0, 2, 1).reshape(N, 3 * Cin)
    A = _conv_rows(img, T, 2)
    Z, S = _mm(A, Wp) + bias, _mm(np.abs(A), np.abs(Wp)) + np.abs(bias)
    del A
    posr = np.tile(pos.astype(np.float64), (B, 1))
    ref = _gelu(Z) + posr
    d_img, d_w, d_b, d_p = DevBuf.from_numpy(img), DevBuf.from_numpy(W), DevBuf.from_numpy(bias), DevBuf.from_numpy(pos)
    outs = []
    for _ in range(2):
        d_out = DevBuf.from_numpy(_pattern(B * T * N, np.float32))
        check(lib.wis_op_enc_conv(0, 2, d_img.ptr, d_w.ptr, 1, d_b.ptr, d_p.ptr, d_out.ptr, B, T, Cin, N))
        outs.append(d_out.to_numpy(np.float32, (B * T, N)))
    tag = f"enc_conv2 N{N} B{B} T{T}"
    assert _same_bits(outs[0], outs[1]), tag + ": two runs differ"
    w = _check(tag, "conv2", K, outs[0], ref, EPS * (GELU_LIP * S + np.abs(posr)), False)
    print(f"RATIO conv2 {tag} {w:.3f}")


def test_enc_conv_refuses_other_channel_counts(lib):
    from wis_hip._lib import DevBuf
    b = DevBuf(1 << 16)
    assert lib.wis_op_enc_conv(0, 1, b.ptr, b.ptr, 1, b.ptr, None, b.ptr, 1, 8, 64, 128) == -7      # conv1: 80 or 128 bins
    assert lib.wis_op_enc_conv(0, 2, b.ptr, b.ptr, 1, b.ptr, b.ptr, b.ptr, 1, 8, 96, 128) == -7      # conv2: K = 3 Cin in whole 64-deep k-tiles
    assert lib.wis_op_enc_conv(0, 3, b.ptr, b.ptr, 1, b.ptr, b.ptr, b.ptr, 1, 8, 128, 128) == -1


# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,N,K,splits,want,offset", [
    (1500, 1280, 5120, 0, 4, 0),      # gemm_pp_kernel<EpiPartial> x 4 slices + splitk_reduce_ln_kernel<4>: large's every layer at one utterance
    (1500, 1024, 4096, 0, 4, 0),      # the same, medium
    (3000, 768, 3072, 0, 2, 0),       # gemm_pp_kernel<EpiPartial> x 2 + splitk_reduce_ln_kernel<2>
    (1500, 384, 1536, 0, 4, 0),       # gemm_f16_kernel<EpiPartial, 128, 128> x 4 + <4>; 96 float4 per row: the second round of a wave is half masked
    (4500, 512, 2048, 0, 2, 0),       # gemm_pp_kernel<EpiPartial> x 2 + <2>, base at three utterances
    (1027, 1280, 5120, 2, 2, 0),      # gemm_f16_kernel<EpiPartial, 128, 128> x 2 + <2>; M % 4 = 3: the reduce's last workgroup has an idle wave
    (1027, 1280, 5120, 4, 4, 0),      # gemm_pp_kernel<EpiPartial> x 4 + <4>, the same rows
    (130, 512, 2048, 4, 4, 0),        # two row tiles of 128 x 128
    (130, 512, 2048, 4, 4, 200),      # residual rows at 200 +- 2.4: the statistics must not lose the variance
])
def test_gemm_splitk_layernorm(lib, M, N, K, splits, want, offset):
    from wis_hip._lib import DevBuf, check
    rng = np.random.default_rng(M * 3 + N + K + splits + offset)
    A, W, bias = _rand16(rng, (M, K), 0.5), _rand16(rng, (N, K), 0.1), rng.standard_normal(N).astype(np.float32)
    if offset:
        res = (offset + rng.integers(-16, 17, size=(M, N)) / 4.0).astype(np.float32)
        res[:, ::7] += 8.0
    else:
        res = rng.standard_normal((M, N)).astype(np.float32)
    g, b = (1 + 0.1 * rng.standard_normal(N)).astype(np.float32), (0.1 * rng.standard_normal(N)).astype(np.float32)
    Z, S = _gemm_ref(A, W)
    X = Z + bias + res
    S += np.abs(bias) + np.abs(res)
    mu = X.mean(1, keepdims=True)
    rstd = 1.0 / np.sqrt(((X - mu) ** 2).mean(1, keepdims=True) + 1e-5)      # two passes
    Y = (X - mu) * rstd * g + b
    d_a, d_w, d_b, d_g, d_e = [DevBuf.from_numpy(a) for a in (A, W, bias, g, b)]
    outs = []
    for _ in range(2):
        d_x, d_y = DevBuf.from_numpy(res), DevBuf.from_numpy(_pattern(M * N, np.float16))
        check(lib.wis_op_gemm_splitk_ln(0, d_a.ptr, d_w.ptr, d_b.ptr, d_x.ptr, d_g.ptr, d_e.ptr, d_y.ptr, M, N, K, splits))
        outs.append((d_x.to_numpy(np.float32, (M, N)), d_y.to_numpy(np.float16, (M, N))))
    tag = f"splitk_ln M{M} N{N} K{K} splits{splits or want} offset{offset}"
    assert _same_bits(outs[0][0], outs[1][0]) and _same_bits(outs[0][1], outs[1][1]), tag + ": two runs differ"
    if not splits:      # the encoder's own choice, modelled here: (N / 128) ceil(M / 128) tiles - none from 200 on, four ways up to 128, else two
        tiles = (N // 128) * ((M + 127) // 128)
        assert tiles < 200 and want == (4 if tiles <= 128 else 2)
    w1 = _check(tag + " X", "splitk_ln", K, outs[0][0], X, EPS * S, False)
    # first order: an error dx of a row element reaches y through rstd |gamma|
    w2 = _check(tag + " Y", "splitk_ln", K, outs[0][1], Y, EPS * S * rstd * np.abs(g), True)
    print(f"RATIO splitk_ln {tag} {max(w1, w2):.3f}")


def test_gemm_splitk_layernorm_choice_and_refusals(lib):
    """splits = 0 follows the encoder (4 / 2 / none by tile count); the fused reduction exists for 2 and 4 slices and N <= 2048"""
    from wis_hip._lib import DevBuf
    b = DevBuf(64 * 2304 * 4 * 4)
    args = [b.ptr] * 7
    assert lib.wis_op_gemm_splitk_ln(0, *args, 64, 256, 384, 3) == -1          # three slices: K % (3 x 64) == 0, no fused reduction for them
    assert lib.wis_op_gemm_splitk_ln(0, *args, 64, 256, 320, 2) == -7          # K is no whole number of 64-deep k-tiles per slice
    assert lib.wis_op_gemm_splitk_ln(0, *args, 64, 2176, 256, 2) == -1         # N > 2048
    assert lib.wis_op_gemm_splitk_ln(0, *args, 3200, 1024, 64, 0) == -7        # 200 tiles: the encoder does not split there


# ---------------------------------------------------------------------------------------
def _softmax(s):
    p = np.exp(s - s.max(-1, keepdims=True))
    return p / p.sum(-1, keepdims=True)


@pytest.mark.parametrize("d,B,T", [(384, 1, 200), (1280, 3, 772)])
def test_enc_qkv_feeds_enc_attention(lib, d, B, T):
    """the [Q | K] rows and the V^T image wis_op_enc_qkv writes are what wis_op_enc_attention reads: float64 attention computed from xn
    (the query rows of W and bias carry the 1/8, as the loader folds it), test_enc_attention's bar"""
    from wis_hip._lib import DevBuf, check
    H, M, Tpad = d // 64, B * T, (T + 63) // 64 * 64
    rng = np.random.default_rng(d + T)
    xn, W, bias = _rand16(rng, (M, d), 0.5), _rand16(rng, (3 * d, d), 0.1), rng.standard_normal(3 * d).astype(np.float32)
    W[:d] = (W[:d].astype(np.float32) * 0.125).astype(np.float16); bias[:d] *= 0.125      # exact: a power of two
    d_qk, d_vt, _, _ = _run_qkv(lib, xn, W, bias, B, T, H, vt_fill=0.0)      # the encoder's V^T buffer is zero where no key lives
    d_o = DevBuf(M * d * 2)
    check(lib.wis_op_enc_attention(0, d_qk.ptr, d_vt.ptr, d_o.ptr, B, T, Tpad, H))
    out = d_o.to_numpy(np.float16, (M, d))
    Z = (_mm(xn.astype(np.float64), W.astype(np.float64)) + bias).reshape(B, T, 3, H, 64)
    s = np.einsum("bqhd,bkhd->bhqk", Z[:, :, 0], Z[:, :, 1])
    ref = np.einsum("bhqk,bkhd->bqhd", _softmax(s), Z[:, :, 2]).reshape(M, d)
    e = _relerr(out, ref)
    print(f"enc_qkv -> enc_attention d{d} B{B} T{T}: rel err {e:.3e}, max abs {np.abs(out - ref).max():.3e}")
    assert e < 3e-3


def test_enc_crosskv_feeds_dec_cross_attn(lib):
    """the second layer's images of wis_op_enc_crosskv are what wis_op_dec_cross_attn reads: float64 attention from the encoder memory.  The queries
    are f16-representable (the kernel casts them) and scaled so that the scores spread like the decode attention tests' (sigma ~ 2.5); the bar is
    the encoder chain's relative one, since V here is twice the size of those tests' unit-variance rows"""
    from wis_hip._lib import DevBuf, check
    d, B, R, T, L = 1280, 2, 5, 1500, 2
    H, M, Tpad = d // 64, B * T, (T + 63) // 64 * 64
    kx_ls, vt_ls = B * T * d + 136, B * d * Tpad + 136
    rng = np.random.default_rng(77)
    mem, W = _rand16(rng, (M, d), 0.5), _rand16(rng, (L * 2 * d, d), 0.1)
    bias = (rng.standard_normal(L * 2 * d) + np.repeat(np.arange(L) * 0.5, 2 * d)).astype(np.float32)
    q = _rand16(rng, (B * R, d), 0.15).astype(np.float32)
    d_kx, d_vt, _, _ = _run_crosskv(lib, mem, W, bias, B, T, H, L, kx_ls, vt_ls, vt_fill=0.0)
    d_q, d_o = DevBuf.from_numpy(q), DevBuf(B * R * d * 2)
    l = 1
    check(lib.wis_op_dec_cross_attn(0, d_q.ptr, d_kx.ptr.value + l * kx_ls * 2, d_vt.ptr.value + l * vt_ls * 2, d_o.ptr, B, R, H, T, 6))
    out = d_o.to_numpy(np.float16, (B * R, d))
    Wl = W[l * 2 * d:(l + 1) * 2 * d].astype(np.float64)
    Z = (_mm(mem.astype(np.float64), Wl) + bias[l * 2 * d:(l + 1) * 2 * d]).reshape(B, T, 2, H, 64)
    s = np.einsum("brhd,bkhd->bhrk", q.astype(np.float64).reshape(B, R, H, 64), Z[:, :, 0])
    ref = np.einsum("bhrk,bkhd->brhd", _softmax(s), Z[:, :, 1]).reshape(B * R, d)
    e = _relerr(out, ref)
    print(f"enc_crosskv -> dec_cross_attn: rel err {e:.3e}, max abs {np.abs(out - ref).max():.3e}")
    assert e < 3e-3
