"""-m gpu: what the loader hands the decoder's step kernels - the LayerNorm fold, the f16 and 8-bit fragment images, the row scales, the column sums, the
cross-Q fold - through wis_op_prep_projection / wis_op_cq_fold (the product's own prep_projection and build_cq_fold on private memory), against the numpy
specification tests/prep_ref.py.  Exact outputs (folded staging, images, scales, 8-bit column sums) are compared word for word (f16 words with the sign of
a zero left open: prep_ref.words16 says why); the sums whose order belongs
to a kernel (column sums and bias of the fold, W'q bo, the product half of the cross-Q fold) against float64 sums of the same fp32 terms under the derived
bounds of prep_ref.py's docstring.  The fold's W' is the exact product w * gamma rounded to f16 once, as the compiled kernel and tests/test_gpu_dec_frag_ops.py
have it (prep_ref.fold; profiles/prep_tests.md has the figures against the twice-rounded formula).  Nothing skips: no comparison here has a near-tie to step around.

Shapes (N, K, n_scale): the smallest; two ragged ones (Npad > N); the QKV shapes of tiny and large with the folded 1/8 on the query rows; FFN2 at large's
width; the vocabulary projection, whose images are larger than the packers' 4096 x 256 grid (Npad = 51872 for 51865 and 51866).  Every shape as the
sixteen-row f16 image and as the 8-bit image, the first three also on eight- and four-row tiles; each with and without gamma / beta.

Inputs (prep_ref.make_case, seeded): Gaussian N(0, 0.05); one 30-sigma outlier per row; rows 0, N / 2, N - 1 zero; a gamma with negative entries and a stretch
of zeros; weights +-2^[-17, -13] (f16 subnormals after the 1/8, and often after the fold); a beta of magnitude 10; rows on exact .5 ties of the quantiser
(round-half-even shows); rows holding +absmax and -absmax.  Up to 1152 x 384 every family runs by itself and as `mixed` (row n of family n % 6 under the
negative / zero gamma and the large beta); the four larger shapes run `mixed` alone - a row is prepared independently of its neighbours, so what a larger
matrix adds is the addressing, and the file stays under a minute."""
import ctypes
import functools

import numpy as np
import pytest

import prep_ref as R

pytestmark = pytest.mark.gpu
F, f32, f16 = np.float64, np.float32, np.float16
GUARD = 512      # sentinel elements on either side of an output (the idiom of tests/test_gpu_gemv_nc5.py)
WIS_E_ARG = -1
SHAPES = [(16, 32, 0), (44, 384, 0), (1004, 128, 0), (1152, 384, 384), (3840, 1280, 1280), (1280, 5120, 0), (51865, 384, 0), (51866, 384, 0)]
FORMS = [(N, K, ns, w8, rows) for N, K, ns in SHAPES for w8, rows in ((0, 16), (1, 16))] + [(N, K, ns, 0, rows) for N, K, ns in SHAPES[:3] for rows in (8, 4)]
QS = 0.125


def _families(N, K):
    return R.FAMILIES + ("mixed",) if N * K <= 1152 * 384 else ("mixed",)


# ---- guarded device buffers ----------------------------------------------------------------------------------------------------------------------------------
def _pattern(dtype):
    return np.array([179], np.uint8)[0] if np.dtype(dtype) == np.uint8 else np.array([-77.0], dtype)[0]


class Out:
    """an output of n elements between two guards; `init` (optional) is what the body holds before the call"""
    def __init__(self, n, dtype, init=None):
        from wis_hip._lib import DevBuf
        self.n, self.dtype = int(n), np.dtype(dtype)
        self.host = np.full(self.n + 2 * GUARD, _pattern(dtype), dtype)
        if init is not None:
            self.host[GUARD:GUARD + self.n] = np.asarray(init, dtype).reshape(-1)
        self.buf = DevBuf.from_numpy(self.host)
        self.ptr = ctypes.c_void_p(self.buf.ptr.value + GUARD * self.dtype.itemsize)

    def read(self):
        """-> (body, guards intact)"""
        raw = self.buf.to_numpy(self.dtype, self.host.shape)
        bits = raw.view({1: np.uint8, 2: np.uint16, 4: np.uint32}[self.dtype.itemsize])
        s = np.array([_pattern(self.dtype)], self.dtype).view(bits.dtype)[0]
        return raw[GUARD:GUARD + self.n], bool((bits[:GUARD] == s).all() and (bits[GUARD + self.n:] == s).all())

    def untouched(self):
        return bool(np.array_equal(self.buf.to_numpy(self.dtype, self.host.shape).view(np.uint8), self.host.view(np.uint8)))


def _call(lib, W, gamma, beta, bias, N, Npad, K, n_scale, qscale, w8, rows, with_bias=True, with_csum=True):
    """-> (return code, dict of Out)"""
    from wis_hip._lib import DevBuf
    dW = DevBuf.from_numpy(W)
    dg, db = (DevBuf.from_numpy(gamma), DevBuf.from_numpy(beta)) if gamma is not None else (None, None)
    nimg = max(Npad, 1) * K
    o = dict(w=Out(N * K, f16), img=Out(nimg, np.uint8 if w8 else f16), bias=Out(N, f32, bias), csum=Out(max(Npad, N), f32))
    if w8:
        o["scale"] = Out(max(Npad, 1), f32)
    rc = lib.wis_op_prep_projection(0, dW.ptr, N, Npad, K, n_scale, qscale, dg.ptr if dg else None, db.ptr if db else None, o["bias"].ptr if with_bias else None,
                                    w8, rows, o["w"].ptr, o["img"].ptr, o["scale"].ptr if w8 else None, o["csum"].ptr if with_csum else None)
    return rc, o


def _unimage(img, Npad, K, rows):
    """the fragment order back to [Npad][K]"""
    return img.reshape(Npad // rows, K // 32, 4, rows, 8).transpose(0, 3, 1, 2, 4).reshape(Npad, K)


def _ratio(dev, ref, bound):
    """largest |dev - ref| / bound; where the bound is 0 (an all-zero row) the word must be the reference itself"""
    err = np.abs(dev.astype(F) - ref)
    z = bound == 0
    assert (err[z] == 0).all(), "a sum of zeros is not zero"
    return float((err[~z] / bound[~z]).max(initial=0.0))


def _bits(a):
    return a.view({1: np.uint8, 2: np.uint16, 4: np.uint32}[a.dtype.itemsize])


def _check(lib, fam, N, K, n_scale, w8, rows, ln):
    """one call, every assertion -> (ratio of c, ratio of the bias, scales off by one ulp)"""
    Npad = -(-N // 16) * 16 if rows == 16 else -(-N // rows) * rows
    W, gamma, beta, bias = R.make_case(fam, N, K, ln)
    rc, o = _call(lib, W, gamma, beta, bias, N, Npad, K, n_scale, QS, w8, rows)
    assert rc == 0, rc
    got = {}
    for k, v in o.items():
        got[k], ok = v.read()
        assert ok, f"a store outside the {k} output"
    Wst = R.fold(W, gamma) if ln else W
    assert np.array_equal(R.words16(got["w"]), R.words16(Wst.reshape(-1))), "the staging as the fold left it"
    ulp_off = 0
    rc_, rb_ = 0.0, 0.0
    if not w8:
        assert np.array_equal(R.words16(got["img"]), R.words16(R.pack(Wst, Npad, rows, n_scale, QS))), "f16 image"
        assert not _bits(_unimage(got["img"], Npad, K, rows)[N:]).any(), "padding rows of the f16 image are zero"
    else:
        q, sc = R.quantise(Wst, Npad, n_scale, QS)
        dsc = got["scale"][:Npad]
        assert not _bits(dsc[N:]).any(), "scales of the padding rows are 0"
        off = _bits(dsc) != _bits(sc)
        if off.any():      # a last-bit difference of the division: the scale to 1 ulp, the bytes exactly on the device's scale (profiles/prep_tests.md says if it happened)
            ulp_off = int(off.sum())
            assert (np.abs(_bits(dsc).astype(np.int64) - _bits(sc).astype(np.int64)) <= 1).all(), "a row scale off by more than one ulp"
            q, sc = R.quantise(Wst, Npad, n_scale, QS, scale=dsc)
        assert np.array_equal(got["img"], R.pack8(q)), "8-bit image"
        assert (_unimage(got["img"], Npad, K, 16)[N:] == 128).all(), "padding rows of the 8-bit image are 128"
    # column sums and bias
    cs = got["csum"][:Npad]
    if not ln:
        assert (_bits(cs) == R.SENTINEL).all(), "column sums written without a fold"
        assert np.array_equal(_bits(got["bias"]), _bits(bias)), "bias changed without a fold"
    else:
        assert (_bits(cs[N:]) == R.SENTINEL).all(), "column sums of the padding rows were written"
        assert not (_bits(cs[:N]) == R.SENTINEL).any()
        c, cb, b, bb = R.fold_sums(W, gamma, beta, bias, n_scale, QS)
        rb_ = _ratio(got["bias"], b, bb)
        assert rb_ <= 1.0, ("bias", rb_)
        if w8:
            assert np.array_equal(_bits(cs[:N]), _bits(R.csum8(Wst, q, sc, n_scale, QS))), "8-bit column sums"
        else:
            rc_ = _ratio(cs[:N], c, cb)
            assert rc_ <= 1.0, ("csum", rc_)
    return rc_, rb_, ulp_off


@pytest.mark.parametrize("ln", [0, 1])
@pytest.mark.parametrize("N,K,n_scale,w8,rows", FORMS)
def test_prep_projection(lib, N, K, n_scale, w8, rows, ln):
    for fam in _families(N, K):
        rc_, rb_, ulp = _check(lib, fam, N, K, n_scale, w8, rows, ln)
        print(f"prep N{N} K{K} ns{n_scale} {'w8' if w8 else 'f16 rows ' + str(rows)} ln{ln} {fam}: csum/bound {rc_:.3f} bias/bound {rb_:.3f} scales off by an ulp {ulp}")


def test_fold_without_an_image_is_refused_cleanly_and_refusals_write_nothing(lib):
    """what launch_pack_gemv / launch_pack_gemv8 / prep_projection refuse: WIS_E_ARG, and every output (the bias included: the fold ran on private memory) is as
    it was"""
    W, gamma, beta, bias = R.make_case("gauss", 44, 96, True)
    cases = [
        ("K % 32", dict(N=44, Npad=48, K=48, w8=0, rows=16)),
        ("K % 32, 8-bit", dict(N=44, Npad=48, K=48, w8=1, rows=16)),
        ("Npad % rows", dict(N=44, Npad=44, K=96, w8=0, rows=16)),
        ("Npad % 16, 8-bit", dict(N=44, Npad=44, K=96, w8=1, rows=16)),
        ("Npad < N", dict(N=44, Npad=32, K=96, w8=0, rows=16)),
        ("Npad < N, 8-bit", dict(N=44, Npad=32, K=96, w8=1, rows=16)),
        ("rows = 5", dict(N=44, Npad=45, K=96, w8=0, rows=5)),
        ("rows = 32", dict(N=44, Npad=64, K=96, w8=0, rows=32)),
        ("gamma without bias", dict(N=44, Npad=48, K=96, w8=0, rows=16, with_bias=False)),
        ("gamma without csum", dict(N=44, Npad=48, K=96, w8=0, rows=16, with_csum=False)),
    ]
    for name, kw in cases:
        K = kw["K"]
        for ln in ([1] if "gamma" in name else [0, 1]):
            rc, o = _call(lib, np.ascontiguousarray(W[:, :K]), gamma[:K] if ln else None, beta[:K] if ln else None, bias, kw["N"], kw["Npad"], K, 0, 1.0, kw["w8"], kw["rows"],
                          kw.get("with_bias", True), kw.get("with_csum", True))
            assert rc == WIS_E_ARG, (name, ln, rc)
            assert all(v.untouched() for v in o.values()), (name, ln)
    # ... and the same shapes with the fault removed pass
    rc, o = _call(lib, W, gamma, beta, bias, 44, 48, 96, 0, 1.0, 0, 16)
    assert rc == 0 and not o["img"].untouched()


# ---- the cross-Q fold ----------------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _cq_inputs(d, fam):
    Wq, gamma, beta, bq = R.make_case(fam, d, d, True, seed=1)
    Wo32 = (R.make_case(fam, d, d, False, seed=2)[0].astype(f32) * f32(1.37)).astype(f32)      # (not f16 numbers: the f32 form rounds on the way in)
    bo = np.random.default_rng([d, 3]).standard_normal(d).astype(f32)
    return Wq, gamma, beta, bq, Wo32, bo


def _cq_fold(lib, d, fam, wo_f16):
    from wis_hip._lib import DevBuf
    Wq, gamma, beta, bq, Wo32, bo = _cq_inputs(d, fam)
    Wo = Wo32.astype(f16) if wo_f16 else Wo32
    ins = [DevBuf.from_numpy(v) for v in (Wq, gamma, beta, bq, Wo, bo)]
    o = dict(fcat=Out(2 * d * d, f16), img=Out(2 * d * d, f16), b_cqo=Out(d, f32), qb=Out(d, f32), qcs=Out(d, f32))
    rc = lib.wis_op_cq_fold(0, ins[0].ptr, ins[1].ptr, ins[2].ptr, ins[3].ptr, ins[4].ptr, int(wo_f16), ins[5].ptr, d,
                            o["fcat"].ptr, o["img"].ptr, o["b_cqo"].ptr, o["qb"].ptr, o["qcs"].ptr)
    assert rc == 0, rc
    got = {}
    for k, v in o.items():
        got[k], ok = v.read()
        assert ok, f"a store outside the {k} output"
    return (Wq, gamma, beta, bq, Wo, bo), got


@pytest.mark.parametrize("wo_f16", [1, 0])
@pytest.mark.parametrize("fam", ["gauss", "outlier"])
@pytest.mark.parametrize("d", [384, 1280])
def test_cq_fold(lib, d, fam, wo_f16):
    (Wq, gamma, beta, bq, Wo, bo), got = _cq_fold(lib, d, fam, wo_f16)
    ref = R.cq_fold(Wq, gamma, beta, bq, Wo, bo)
    fcat = got["fcat"].reshape(d, 2 * d)
    assert np.array_equal(R.words16(fcat[:, :d]), R.words16(ref["wq"])), "the left half: W'q"
    rp = _ratio(fcat[:, d:], ref["P"], ref["P_bound"])
    assert np.array_equal(_bits(got["img"]), _bits(R.pack(fcat, d, 16, 0, 1.0))), "the image of the device's own [W'q | W'q Wo]"
    b, bb = R.b_cqo_ref(fcat, bo)
    r_b, r_qb, r_qcs = _ratio(got["b_cqo"], b, bb), _ratio(got["qb"], ref["qb"], ref["qb_bound"]), _ratio(got["qcs"], ref["qcs"], ref["qcs_bound"])
    print(f"cq_fold d{d} {fam} Wo {'f16' if wo_f16 else 'f32'}: product/bound {rp:.3f} b_cqo/bound {r_b:.3f} qb/bound {r_qb:.3f} qcs/bound {r_qcs:.3f}")
    assert rp <= 1.0 and r_b <= 1.0 and r_qb <= 1.0 and r_qcs <= 1.0, (rp, r_b, r_qb, r_qcs)


def test_cq_fold_is_what_the_out_cq_stage_runs_on(lib):
    """d = 384, five rows.  wis_op_gemv_out_cq builds its operands from the raw matrices with the same product code; its q_raw, qcs and qb must be, word for
    word, what the tap's outputs give: qcs / qb directly, q_raw as [f16(x0) | a] fcat^T + b_cqo through wis_op_gemv on the stand-alone sixteen-column kernel
    (which packs fcat into the very image the tap returned - asserted in test_cq_fold - and is word-equal to the fused kernel: tests/test_gpu_out_cq_kernel.py)"""
    from wis_hip._lib import DevBuf, check
    d, M = 384, 5
    (Wq, gamma, beta, bq, Wo, bo), got = _cq_fold(lib, d, "gauss", 1)
    rng = np.random.default_rng(384)
    a = rng.standard_normal((M, d)).astype(f16)
    x0 = (rng.standard_normal((M, d)) * 2 + 0.3).astype(f32)
    ins = [DevBuf.from_numpy(v) for v in (a, x0, Wo, bo, Wq, bq, gamma, beta)]
    outs = {k: DevBuf.from_numpy(np.full(n, 77.0, f32)) for k, n in (("x1", M * d), ("stat", M * (d // 16) * 2), ("q", M * d), ("qcs", d), ("qb", d))}
    check(lib.wis_op_gemv_out_cq(0, *[b.ptr for b in ins], outs["x1"].ptr, outs["stat"].ptr, outs["q"].ptr, None, outs["qcs"].ptr, outs["qb"].ptr, M, d, 0))
    q = outs["q"].to_numpy(f32, (M, d))
    assert np.array_equal(_bits(outs["qcs"].to_numpy(f32, (d,))), _bits(got["qcs"])) and np.array_equal(_bits(outs["qb"].to_numpy(f32, (d,))), _bits(got["qb"]))
    xcat = np.concatenate([x0.astype(f16), a], axis=1)
    dx, dWc, dbc, dy = DevBuf.from_numpy(xcat), DevBuf.from_numpy(got["fcat"]), DevBuf.from_numpy(got["b_cqo"]), DevBuf.from_numpy(np.full((M, d), 55.0, f32))
    check(lib.wis_op_gemv(0, dx.ptr, None, None, dWc.ptr, dbc.ptr, dy.ptr, M, d, 2 * d, 4))      # GV_OUT_F32
    q2 = dy.to_numpy(f32, (M, d))
    diff = _bits(q) != _bits(q2)
    print(f"cq_fold chained into the out+cq stage: {int(diff.sum())} of {diff.size} words differ")
    assert not diff.any()
