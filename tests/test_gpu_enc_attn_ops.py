"""-m gpu: the two encoder kernels that are not GEMMs - self-attention (all four instantiations, through wis_op_enc_attention_ex) and
LayerNorm (both instantiations, through wis_op_layernorm) - against float64, element by element, at their edges.

Attention: the score patterns, the float64 reference and the bound are tests/enc_attn_ref.py (its docstring derives the bound;
tests/test_enc_attn_model_cpu.py shows on the CPU that a model of the lazy loop meets it with factor 1 and that every pattern reaches
the path it was built for).  Here every written element obeys |out - ref| <= 2 unit + 2^-10 |ref| and is finite; three launches agree
to the bit; V^T padding of 0x5A5A instead of zeros and f16 NaN rows behind the [Q | K] image change no bit; the output behind row B T
keeps its fill.  The lazy forms get Q as the engine delivers it (log2(e) / 8 folded in, one f16 rounding) and a base-2 reference; the
plain forms read the same f16 values with a base-e reference.

LayerNorm: e32[row] is the largest elementwise error against float64 of a numpy float32 two-pass restatement with pairwise sums (an order
the kernel does not use); every element obeys |out - ref| <= 4 e32[row] + 2^-10 |ref| (4: a wave tree against pairwise); where the
restatement of a row is exact the floor 2^-24 max|x - mu| rstd max|gamma| takes e32's place.

The figures of an MI355X run, the kernel each case ran and the mutations these tests catch: profiles/enc_attn_tests.md."""
import numpy as np
import pytest

import enc_attn_ref as R

pytestmark = pytest.mark.gpu

WIS_E_ARG, WIS_E_UNSUPPORTED = -1, -7      # include/wis_hip.h
PAT16 = 0x5A5A                             # f16 203.25: nothing these kernels produce from the inputs below
NAN16 = 0x7E00
GUARD = 4096
FORMS = [("plain", 0), ("lazy", 1), ("plain_split", 2), ("lazy_split", 3)]      # wis_op_enc_attention_ex: bit 0 lazy loop, bit 1 split-key pair
FACTOR = 2.0


def _same_bits(a, b):
    return np.array_equal(a.view(np.uint16), b.view(np.uint16))


_REF = {}


def _reference(pattern, B, T, H):
    """inputs and both references of a case, computed once"""
    key = (pattern, B, T, H)
    if key not in _REF:
        _REF.clear()      # (one case at a time: the parametrisation visits each key once)
        q, k, v = R.make_inputs(pattern, B, T, H)
        refs = {}
        for base2 in (False, True):
            ref, unit = np.empty((B, T, H, 64)), np.empty((B, T, H, 64))
            for b in range(B):
                for h in range(H):
                    ref[b, :, h], unit[b, :, h] = R.reference(q[b, :, h], k[b, :, h], v[b, :, h], base2)
            refs[base2] = (ref.reshape(B * T, H * 64), unit.reshape(B * T, H * 64))
        _REF[key] = (q, k, v, refs)
    return _REF[key]


def _attention_case(lib, pattern, B, T, H, extra_pad=0):
    from wis_hip._lib import DevBuf, check
    d = H * 64
    Tpad = (T + 63) // 64 * 64 + extra_pad
    q, k, v, refs = _reference(pattern, B, T, H)
    qk = R.qk_image(q, k)

    def qk_buf(guard_bits):      # 64 guard rows behind the image
        g = np.full((64, 2 * d), guard_bits, np.uint16).view(np.float16)
        return DevBuf.from_numpy(np.concatenate([qk, g], axis=0))

    d_qk0, d_qk1 = qk_buf(0), qk_buf(NAN16)
    d_vt0, d_vt1 = DevBuf.from_numpy(R.vt_image(v, Tpad, 0)), DevBuf.from_numpy(R.vt_image(v, Tpad, PAT16))
    fill = np.full(B * T * d + GUARD, PAT16, np.uint16)
    worst = {}
    for name, form in FORMS:
        if form & 2 and T < R.SPLIT_MIN_T:
            continue
        ref, unit = refs[bool(form & 1)]
        outs = []
        for d_qk, d_vt in ((d_qk0, d_vt0), (d_qk0, d_vt0), (d_qk0, d_vt0), (d_qk1, d_vt1)):
            d_o = DevBuf.from_numpy(fill)
            check(lib.wis_op_enc_attention_ex(0, d_qk.ptr, d_vt.ptr, d_o.ptr, B, T, Tpad, H, form))
            o = d_o.to_numpy(np.float16, (B * T * d + GUARD,))
            d_o.free()
            assert (o[B * T * d:].view(np.uint16) == PAT16).all(), (name, "output behind row B T overwritten")
            outs.append(o[:B * T * d].reshape(B * T, d))
        out = outs[0]
        ratio = R.ratios(out, ref, unit)
        w = float(ratio.max())
        i = np.unravel_index(int(ratio.argmax()), ratio.shape)
        worst[name] = w
        print(f"enc_attention {pattern} B{B} T{T} H{H} Tpad{Tpad} {name}: max (|out - ref| - r) / unit = {w:.3f} at {tuple(int(x) for x in i)}")
        assert np.isfinite(out).all(), (name, "non-finite output")
        assert w <= FACTOR, (name, w, i)
        assert _same_bits(outs[0], outs[1]) and _same_bits(outs[1], outs[2]), (name, "launches differ")
        assert _same_bits(outs[0], outs[3]), (name, "V^T padding / rows behind the [Q | K] image reached the output")
    for b_ in (d_qk0, d_qk1, d_vt0, d_vt1):
        b_.free()
    return worst


@pytest.mark.parametrize("T", R.T_LIST)
@pytest.mark.parametrize("pattern", R.PATTERNS)
def test_enc_attention_forms(lib, pattern, T):
    for B, H in ((1, 1), (2, 3)):
        _attention_case(lib, pattern, B, T, H)


@pytest.mark.parametrize("pattern", ["control", "tail", "up17"])
def test_enc_attention_wider_padding(lib, pattern):
    """Tpad one key tile beyond the last one the kernels read"""
    _attention_case(lib, pattern, 2, 200, 3, extra_pad=64)


def test_enc_attention_ex_refusals(lib):
    from wis_hip._lib import DevBuf
    B, T, H = 1, 192, 1
    d_qk, d_vt, d_o = DevBuf(T * 128 * 2), DevBuf(64 * 192 * 2), DevBuf(T * 64 * 2)
    for form in (2, 3):
        assert lib.wis_op_enc_attention_ex(0, d_qk.ptr, d_vt.ptr, d_o.ptr, B, T, 192, H, form) == WIS_E_ARG      # three key tiles
    assert lib.wis_op_enc_attention_ex(0, d_qk.ptr, d_vt.ptr, d_o.ptr, B, T, 192, H, 4) == WIS_E_ARG
    assert lib.wis_op_enc_attention_ex(0, d_qk.ptr, d_vt.ptr, d_o.ptr, B, T, 128, H, 1) == WIS_E_ARG              # Tpad < the key tiles


# ---------------------------------------------------------------------------------------
def _pairwise_sum32(a):
    """float32 row sums as a balanced binary tree over the zero-padded row"""
    n = 1 << max(0, int(a.shape[1] - 1).bit_length())
    a = np.concatenate([a, np.zeros((a.shape[0], n - a.shape[1]), np.float32)], axis=1)
    while n > 1:
        n //= 2
        a = a[:, :n] + a[:, n:]
    return a[:, 0]


KINDS = ["normal", "offset", "constant", "outlier", "zero", "tiny"]


def _ln_rows(rng, M, d, shift):
    x = np.empty((M, d), np.float32)
    kinds = [(i + shift) % len(KINDS) for i in range(M)]
    for i, kind in enumerate(kinds):
        if kind == 0:
            x[i] = rng.standard_normal(d) * 3 + 0.7
        elif kind == 1:
            x[i] = 1000.0 + rng.standard_normal(d)            # a common offset: a one-pass variance would cancel
        elif kind == 2:
            x[i] = 3.25                                       # constant: every partial sum is exact, so is the mean
        elif kind == 3:
            x[i] = rng.standard_normal(d) * 1e-3
            x[i, int(rng.integers(d))] = 1e4                  # one outlier
        elif kind == 4:
            x[i] = 0.0
        else:
            x[i] = rng.standard_normal(d) * 3e-3              # variance 9e-6, beside eps = 1e-5: the only kind that sees eps itself
    return x, kinds


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("affine", [True, False])
@pytest.mark.parametrize("M", [1, 3, 5, 130])
@pytest.mark.parametrize("d", [4, 260, 384, 512, 1028, 1280, 2048])
def test_layernorm_rows(lib, d, M, affine, kind):
    """every case launches every row kind (row i of launch `shift` is kind (i + shift) % 6; M < 6: six launches, so that every kind
    also sits in every row of the workgroup) and asserts the rows of ITS kind, so that a miss names the kind.

    The `offset` rows are what gave layernorm_kernel the second step of its mean: with the quotient of the plain sum alone (one to two
    ulp(1000) = 6e-5 off, where the pairwise restatement rounds correctly) 10 of their 56 cases stood at 4.7 ... 27.8 on an MI355X
    (profiles/enc_attn_tests.md)."""
    from wis_hip._lib import DevBuf, check
    rng = np.random.default_rng([d, M, int(affine)])      # (the same rows whatever `kind` is asserted)
    f32 = np.float32
    g = rng.standard_normal(d).astype(f32) if affine else np.ones(d, f32)
    be = rng.standard_normal(d).astype(f32) if affine else np.zeros(d, f32)
    d_g, d_b = (DevBuf.from_numpy(g), DevBuf.from_numpy(be)) if affine else (None, None)
    worst, seen = 0.0, 0
    for shift in range(len(KINDS) if M < len(KINDS) else 1):
        x, kinds = _ln_rows(rng, M, d, shift)
        mine = np.array([KINDS[j] == kind for j in kinds])
        if not mine.any():
            continue
        seen += int(mine.sum())
        x64 = x.astype(np.float64)
        mu, var = x64.mean(1, keepdims=True), x64.var(1, keepdims=True)
        rstd = 1.0 / np.sqrt(var + 1e-5)
        ref = (x64 - mu) * rstd * g + be
        mu32 = (_pairwise_sum32(x) / f32(d))[:, None]
        dev = x - mu32
        rstd32 = (f32(1) / np.sqrt(_pairwise_sum32(dev * dev) / f32(d) + f32(1e-5)))[:, None]
        y32 = dev * rstd32 * g + be
        assert y32.dtype == f32
        e32 = np.abs(y32.astype(np.float64) - ref).max(1)
        floor = 2.0 ** -24 * np.abs(x64 - mu).max(1) * rstd[:, 0] * np.abs(g).max()
        e32 = np.where(e32 == 0, floor, e32)
        d_x = DevBuf.from_numpy(x)
        d_y = DevBuf.from_numpy(np.full(M * d + GUARD, PAT16, np.uint16))
        check(lib.wis_op_layernorm(0, d_x.ptr, d_g.ptr if affine else None, d_b.ptr if affine else None, d_y.ptr, M, d))
        y = d_y.to_numpy(np.float16, (M * d + GUARD,))
        d_x.free(); d_y.free()
        assert (y[M * d:].view(np.uint16) == PAT16).all(), "output behind row M overwritten"
        out = y[:M * d].reshape(M, d)
        assert np.isfinite(out).all()
        if kind in ("constant", "zero"):      # exactly f16(beta) (0 without the affine part)
            for i in np.flatnonzero(mine):
                assert _same_bits(out[i], be.astype(np.float16)), (i, kind)
        err = np.abs(out.astype(np.float64) - ref)
        excess = np.maximum(err - 2.0 ** -10 * np.abs(ref), 0.0)
        with np.errstate(divide="ignore", invalid="ignore"):
            ratio = np.where(excess > 0, excess / e32[:, None], 0.0)[mine]
        w = float(ratio.max())
        worst = max(worst, w)
    assert seen > 0
    print(f"layernorm<{str(affine).lower()}> d{d} M{M} {kind}: max (|out - ref| - r) / e32 = {worst:.3f} over {seen} rows")
    assert worst <= 4.0, (kind, worst)


@pytest.mark.parametrize("d", [2052, 6])
def test_layernorm_refusals(lib, d):
    from wis_hip._lib import DevBuf
    d_x, d_y = DevBuf(4 * d * 4), DevBuf.from_numpy(np.full(4 * d, PAT16, np.uint16))
    assert lib.wis_op_layernorm(0, d_x.ptr, None, None, d_y.ptr, 4, d) == WIS_E_UNSUPPORTED
    assert (d_y.to_numpy(np.uint16, (4 * d,)) == PAT16).all()
