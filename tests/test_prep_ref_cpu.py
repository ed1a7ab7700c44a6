"""tests/prep_ref.py, the numpy specification of the load-time weight preparation, checked on the CPU: it agrees with the package's own quantiser
(wis_hip.weights.quantize_rows / quantize_folded), the folded projection it describes IS the projection behind a LayerNorm (float64 activations, up to the f16
rounding of W'), and the input families of tests/test_gpu_prep_ops.py tell it from each deliberately wrong variant: at least one word of an exact output, or at
least 4x the bound of a bounded one.  A family that cannot separate a variant is not claimed for it (SEPARATES below says which are, and why not the others)."""
import numpy as np
import pytest

import prep_ref as R

F, f32, f16 = np.float64, np.float32, np.float16
SHAPES = [(44, 384, 16), (1004, 128, 128)]      # (N, K, n_scale): ragged, query rows scaled by 1/8


@pytest.mark.parametrize("fam", R.FAMILIES + ("mixed",))
def test_quantiser_agrees_with_the_package(fam):
    from wis_hip.weights import quantize_folded, quantize_rows
    for N, K, _ in SHAPES:
        W, gamma, _, _ = R.make_case(fam, N, K, True)
        for Wst in (W, R.fold(W, gamma)):
            q, sc = R.quantise(Wst, N, 0, 1.0)
            q0, sc0 = quantize_rows(Wst)
            assert np.array_equal(q, q0) and np.array_equal(sc.view(np.uint32), sc0.view(np.uint32))
        q, sc = R.quantise(R.fold_f32(W, gamma), N, 0, 1.0)      # quantize_folded rounds the product to fp32 first: its own staging, not everywhere the device's
        deq = q.astype(f32) * sc[:, None]
        safe = np.where(gamma != 0, gamma, f32(1))
        assert np.array_equal(np.where(gamma[None, :] != 0, deq / safe[None, :], f32(0)).astype(f32), quantize_folded(W, gamma))


def test_folded_query_scale_only_moves_the_scale():
    """rows < n_scale: the same 8-bit values, the scale times 1/8 - the packer quantises the unscaled row"""
    W, _, _, _ = R.make_case("gauss", 44, 384, False)
    q0, s0 = R.quantise(W, 48, 0, 1.0)
    q1, s1 = R.quantise(W, 48, 16, 0.125)
    assert np.array_equal(q0, q1) and np.array_equal(s1[:16], s0[:16] * f32(0.125)) and np.array_equal(s1[16:], s0[16:])
    assert not q1[44:].any() and not s1[44:].any() and (R.pack8(q1).reshape(3, 12, 4, 16, 8)[2, :, :, 12:] == 128).all()


@pytest.mark.parametrize("N,K,n_scale", SHAPES)
@pytest.mark.parametrize("fam", ["gauss", "gamma_neg_zero", "beta10"])
def test_identity_of_the_folded_projection(fam, N, K, n_scale):
    """rs (W' x - mu c) + b' == W (LN(x) gamma + beta) + b: exactly (float64) with W' = W gamma unrounded, and within the f16 rounding of W' -
    rs sum_k |W'_k - W_k gamma_k| |x_k - mu|, each difference at most 2^-11 |W gamma| or half an f16 subnormal step - with the specification's W', c, b'"""
    W, gamma, beta, bias = R.make_case(fam, N, K, True)
    x = np.random.default_rng(N + K).standard_normal(K) * 3 + 1.5
    mu, rs = x.mean(), 1.0 / np.sqrt(x.var() + 1e-5)
    Wg = W.astype(F) * gamma.astype(F)
    want = W.astype(F) @ ((x - mu) * rs * gamma + beta) + bias
    exact = rs * (Wg @ x - mu * Wg.sum(1)) + (bias + W.astype(F) @ beta.astype(F))
    assert np.abs(exact - want).max() <= 1e-12 * (1 + np.abs(want).max())
    Wp = R.fold(W, gamma).astype(F)
    c, _, b, _ = R.fold_sums(W, gamma, beta, bias, 0, 1.0)
    got = rs * (Wp @ x - mu * c) + b
    bound = rs * ((R.U16 * np.abs(Wg) + 2.0 ** -25) @ np.abs(x - mu)) + 1e-6 * (1 + np.abs(want))      # (+ the fp32 products W * beta of the specification)
    assert (np.abs(got - want) <= bound).all()
    # the query rows: everything times 1/8
    c8, _, b8, _ = R.fold_sums(W, gamma, beta, bias, n_scale, 0.125)
    assert np.array_equal(c8[:n_scale], c[:n_scale] * 0.125) and np.allclose(b8[:n_scale] - bias[:n_scale], (b[:n_scale] - bias[:n_scale]) * 0.125, rtol=1e-12, atol=0)


# ---- right from wrong ---------------------------------------------------------------------------------------------------------------------------------------
def _separation(fam, N, K, n_scale):
    """variant -> True where the family's input separates it from the specification at this shape"""
    W, gamma, beta, bias = R.make_case(fam, N, K, True)
    Npad = -(-N // 16) * 16
    Wst = R.fold(W, gamma)
    out = {}
    c, cb, _, _ = R.fold_sums(W, gamma, beta, bias, n_scale, 0.125)
    cw = R.csum_unrounded(W, gamma, beta, bias, n_scale, 0.125)[0]
    out["csum_unrounded"] = bool((np.abs(cw - c) >= 4 * cb).any() and (cb > 0).any())
    q, sc = R.quantise(Wst, Npad, n_scale, 0.125)
    for name, fn in (("quant_trunc", R.quant_trunc), ("quant_128", R.quant_128)):
        qw, sw = fn(Wst, Npad, n_scale, 0.125)
        out[name] = bool((qw != q).any() or (sw.view(np.uint32) != sc.view(np.uint32)).any())
    out["csum8_from_f16"] = bool((R.csum8_from_f16(Wst, q, sc, n_scale, 0.125).view(np.uint32) != R.csum8(Wst, q, sc, n_scale, 0.125).view(np.uint32)).any())
    out["pack_scale_after_round"] = bool((R.pack_scale_after_round(Wst, Npad, 16, n_scale, 0.125).view(np.uint16) != R.pack(Wst, Npad, 16, n_scale, 0.125).view(np.uint16)).any())
    return out


ALL = R.FAMILIES + ("mixed",)
# which families are claimed for which variant.  Not claimed: `ties` and `clamp` for csum_unrounded - their gamma is a signed power of two, the fold does not
# round, and rounded and unrounded sums are the same numbers; `ties` for pack_scale_after_round - multiples of 2^-12 of at most eight bits: an eighth of them
# is a multiple of 2^-15 and still an f16 number, no second rounding happens.
SEPARATES = {
    "csum_unrounded": tuple(f for f in ALL if f not in ("ties", "clamp")),
    "quant_trunc": ALL,
    "quant_128": ALL,
    "csum8_from_f16": ALL,
    "pack_scale_after_round": tuple(f for f in ALL if f != "ties"),
}


@pytest.mark.parametrize("N,K,n_scale", SHAPES)
@pytest.mark.parametrize("fam", ALL)
def test_the_families_tell_right_from_wrong(fam, N, K, n_scale):
    sep = _separation(fam, N, K, n_scale)
    print(f"{fam} N{N} K{K}: " + " ".join(f"{k}={int(v)}" for k, v in sep.items()))
    for variant, fams in SEPARATES.items():
        if fam in fams:
            assert sep[variant], (variant, fam)


def test_ties_rows_round_half_even():
    """the tie rows: w / scale is exactly m / 2, and the specification goes to the even neighbour where half-away-from-zero would not"""
    W, _, _, _ = R.make_case("ties", 44, 384, False)
    q, sc = R.quantise(W, 48, 0, 1.0)
    assert (sc[:44] == f32(2.0 ** -(R.TIE_EXP - 1))).all()
    v = W.astype(F) / sc[:44, None]
    tie = np.abs(v - np.trunc(v)) == 0.5
    assert tie.mean() > 0.4 and (q[:44][tie] % 2 == 0).all()
    away = np.sign(v) * np.floor(np.abs(v) + 0.5)
    assert (q[:44][tie] != away[tie]).mean() > 0.4
    assert (np.abs(q[:44]).max(axis=1) == 127).all()


def test_image_index_map():
    """element (n, k) of the matrix sits at [n / rows][k / 32][(k / 8) % 4][n % rows][k % 8]; padding rows are zero / byte 128"""
    N, Npad, K = 44, 48, 64
    W = (np.arange(N * K).reshape(N, K) % 2048).astype(f16)
    for rows in (4, 8, 16):
        img = R.pack(W, Npad, rows, 0, 1.0).reshape(Npad // rows, K // 32, 4, rows, 8)
        for n, k in ((0, 0), (5, 9), (17, 40), (43, 63)):
            assert img[n // rows, k // 32, (k // 8) % 4, n % rows, k % 8] == W[n, k]
        assert not img.reshape(-1)[np.isin(np.arange(Npad).repeat(K).reshape(Npad, K), range(N, Npad)).reshape(Npad // rows, rows, K // 32, 4, 8).transpose(0, 2, 3, 1, 4).reshape(-1)].any()
        assert np.count_nonzero(img) == np.count_nonzero(W)
