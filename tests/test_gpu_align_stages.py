"""-m gpu: the six alignment kernels (csrc/align.hip) stage by stage through wis_op_align_stage / wis_op_dtw_batch / wis_op_align_probs /
wis_op_align_capture (include/wis_hip.h), batched and ragged as wis_align calls them, element by element against tests/align_ref.py.

Scores + softmax, the norm, the chain and the token probabilities: ratio = |GPU - float64| / bound <= 2 for every element, the bound per
element from align_ref's derivation (its float32 models stay <= 1 on these very inputs: tests/test_align_model_cpu.py).  The norm is judged
against float64 from the very fp32 W it read - the caller's, or what stage 0 left on the GPU - so errors do not compound.  Median selection, head sum, DTW and capture are exact.
Every device buffer a kernel writes is pre-filled with a pattern and read back whole: nothing outside [b][row < N[b]][f < F[b]] may change.

test_norm_underflow_column_follows_the_fp32_model: weights about 1e-25 whose squared deviations underflow give std = 0 in fp32, so the column
is +-inf (0 / 0 = NaN where a weight equals the mean) - the value the fp32 model yields, which is what openai-whisper's own fp32
std_mean / divide gives on such a frame; float64 would return ordinary numbers there, so no float64 bound applies to that column."""
import ctypes as C

import numpy as np
import pytest

import align_ref as R

pytestmark = pytest.mark.gpu
WIS_E_ARG, WIS_E_UNSUPPORTED = -1, -7      # include/wis_hip.h


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype.itemsize == 4 else np.uint16)


def _ratio(err, bound):
    with np.errstate(all="ignore"):
        return float(np.max(np.abs(err) / bound, initial=0.0))


def _stage(lib, stage, c, W, *, T=None, acc=None, inp=None, ncap=None, width=None, hpc=None, expect=0):
    """one wis_op_align_stage call on case c -> (W, acc) as the device holds them afterwards"""
    from wis_hip import _lib
    T = T or c["T"]
    N, F = np.array(c["N"], np.int32), np.array(c["F"], np.int32)
    d_W = _lib.DevBuf.from_numpy(W)
    d_acc = _lib.DevBuf.from_numpy(acc) if acc is not None else None
    d_q = d_k = None
    koff, kb, ke = None, 0, 0
    if inp is not None:
        d_q, d_k = _lib.DevBuf.from_numpy(inp["q"]), _lib.DevBuf.from_numpy(inp["Kbuf"])
        koff, kb, ke = np.ascontiguousarray(inp["koff"], np.int64), int(inp["kbstride"]), inp["Kbuf"].size
    rc = lib.wis_op_align_stage(0, stage, d_q.ptr if d_q else None, d_k.ptr if d_k else None, ke, _lib.ptr(koff) if koff is not None else None, kb,
                                _lib.ptr(N), _lib.ptr(F), c["B"], c["nsel"], ncap or (inp["ncap"] if inp else max(c["N"])), max(c["N"]), max(c["F"]), T,
                                width or c.get("width", 7), c.get("hpc", 0) if hpc is None else hpc, d_W.ptr, W.size, d_acc.ptr if d_acc else None,
                                acc.size if acc is not None else 0)
    assert rc == expect, (rc, (lib.wis_last_error() or b"").decode())
    return d_W.to_numpy(np.float32, W.shape), (d_acc.to_numpy(np.float32, acc.shape) if acc is not None else None)


# ---- scores + softmax ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", R.SCORES_CASES, ids=R.case_id)
def test_scores_softmax(c, lib):
    inp = R.scores_inputs(c)
    T, B, nsel, nmax = c["T"], c["B"], c["nsel"], inp["nmax"]
    G = c["hpc"] or nsel
    W0 = R.sentinel(-(-nsel // G) * B * G * nmax * T)
    W1, _ = _stage(lib, 0, c, W0, inp=inp)
    per, inside = R.unpack_w(c, W1, G, T)
    assert np.array_equal(_bits(W1)[~inside], _bits(W0)[~inside]), "written outside [b][g][row < N[b]]"
    worst = 0.0
    for (b, s), got in per.items():
        F = c["F"][b]
        p, bound, _ = R.scores_bound(inp["q16"][b, s], inp["K16"][b, s])
        assert np.isfinite(got[:, :F]).all()
        worst = max(worst, _ratio(got[:, :F] - p[:, :F], bound[:, :F]))
    print(f"scores {R.case_id(c)}: ratio {worst:.3f}")
    assert worst <= 2.0


def test_stage_refuses_what_would_index_out_of_bounds(lib):
    c = dict(R.SCORES_CASES[4])
    inp = R.scores_inputs(c)
    W0 = R.sentinel(2 * c["B"] * 2 * inp["nmax"] * c["T"])
    for change in (dict(F=(1, 99, c["T"] + 1)), dict(ncap=inp["nmax"] - 1), dict(short_k=True), dict(koff=3)):
        cc, ii, ncap = dict(c), dict(inp), None
        if "F" in change:
            cc["F"] = change["F"]
        if "ncap" in change:
            ncap = change["ncap"]
        if "short_k" in change:
            ii["Kbuf"] = inp["Kbuf"][:-(c["T"] * 64 + 8)]      # (the spare slot may be the last one: cut into the one before it)
        if "koff" in change:
            ii["koff"] = inp["koff"] + change["koff"]
        W1, _ = _stage(lib, 0, cc, W0, inp=ii, ncap=ncap, expect=WIS_E_ARG)
        assert (lib.wis_last_error() or b"").decode().startswith("wis_op_align_stage:")
        assert np.array_equal(_bits(W1), _bits(W0))


# ---- norm ----------------------------------------------------------------------------------------------------------------------------
def _run_norm(lib, c, per):
    G = c.get("hpc", 0) or c["nsel"]
    W0 = R.pack_w(c, per, G, c["T"])
    W1, _ = _stage(lib, 1, c, W0)
    got, inside = R.unpack_w(c, W1, G, c["T"])
    before = R.unpack_w(c, W0, G, c["T"])[0]
    assert np.array_equal(_bits(W1)[~inside], _bits(W0)[~inside]), "written outside [b][g][row < N[b]]"
    for (b, s), g in got.items():
        assert np.array_equal(_bits(g[:, c["F"][b]:]), _bits(before[b, s][:, c["F"][b]:])), "written at frames >= F[b]"
    return {k: g[:, :c["F"][k[0]]] for k, g in got.items()}


@pytest.mark.parametrize("c", R.NORM_CASES, ids=R.case_id)
def test_norm(c, lib):
    per = R.norm_inputs(c)
    got = _run_norm(lib, c, per)
    worst, nx, n, other = 0.0, 0, 0, 0
    for (b, s), w in per.items():
        z, bound, ex = R.norm_bound(w)
        other += int((R.canon(got[b, s]) != R.canon(R.norm_model32(w))).sum())
        if c["N"][b] == 1:      # one token: every std is 0, 0 / 0
            assert np.isnan(got[b, s]).all()
            continue
        nx += int(ex.sum()); n += ex.size
        assert np.isfinite(got[b, s][:, ~ex]).all()
        worst = max(worst, _ratio((got[b, s] - z)[:, ~ex], bound[:, ~ex]))
    print(f"norm {R.case_id(c)}: ratio {worst:.3f}  excluded {nx} of {n} columns  words unlike the fp32 model's {other}")
    assert n > 0 and nx <= 0.01 * n and nx < n
    assert worst <= 2.0
    # the kernel's documented order (four row partitions, ((p0 + p1) + p2) + p3, two passes) in correctly rounded fp32 operations: the model's bits
    assert other == 0


@pytest.mark.parametrize("i", [1, 4])
def test_norm_of_the_gpus_own_softmax(i, lib):
    """stage 1 on the buffer stage 0 left (real attention weights: spread 20, most of the mass beyond the crop), judged against float64
    from those very fp32 weights"""
    c = R.SCORES_CASES[i]
    inp = R.scores_inputs(c)
    G = c["hpc"] or c["nsel"]
    W0 = R.sentinel(-(-c["nsel"] // G) * c["B"] * G * inp["nmax"] * c["T"])
    W1, _ = _stage(lib, 0, c, W0, inp=inp)
    W2, _ = _stage(lib, 1, c, W1)
    p, inside = R.unpack_w(c, W1, G, c["T"])
    z, _ = R.unpack_w(c, W2, G, c["T"])
    assert np.array_equal(_bits(W2)[~inside], _bits(W1)[~inside])
    worst, nx, n = 0.0, 0, 0
    for (b, s), w in p.items():
        F = c["F"][b]
        assert np.array_equal(_bits(z[b, s][:, F:]), _bits(w[:, F:])), "written at frames >= F[b]"
        if c["N"][b] == 1:
            assert np.isnan(z[b, s][:, :F]).all()
            continue
        ref, bound, ex = R.norm_bound(w[:, :F])
        assert (w[:, :F].astype(np.float64).std(0)[~ex] >= 2.0 ** -50).all()
        nx += int(ex.sum()); n += ex.size
        worst = max(worst, _ratio((z[b, s][:, :F] - ref)[:, ~ex], bound[:, ~ex]))
        assert np.array_equal(R.canon(z[b, s][:, :F]), R.canon(R.norm_model32(w[:, :F])))
    print(f"norm of stage 0's output, {R.case_id(c)}: ratio {worst:.3f}  excluded {nx} of {n} columns")
    assert n > 0 and nx <= 0.01 * n and worst <= 2.0


@pytest.mark.parametrize("N", [4, 8, 16])
def test_norm_equal_column_is_nan_alone(N, lib):
    c = R._case(130 + N, T=8, B=1, nsel=1, N=(N,), F=(8,))
    w = R.norm_inputs(c)[0, 0]
    w[:, 3] = np.float32(0.375)      # N equal values: the fp32 mean is exact, every deviation 0, std 0
    got = _run_norm(lib, c, {(0, 0): w})[0, 0]
    z, bound, ex = R.norm_bound(w)
    assert ex[3] and ex.sum() == 1
    assert np.isnan(got[:, 3]).all() and np.isfinite(np.delete(got, 3, axis=1)).all()
    assert _ratio((got - z)[:, ~ex], bound[:, ~ex]) <= 2.0


def test_norm_underflow_column_follows_the_fp32_model(lib):
    c = R._case(140, T=9, B=1, nsel=1, N=(6,), F=(9,))
    w = R.norm_inputs(c)[0, 0]
    w[:, 4] = (np.float32(1e-25) * (1.0 + np.array([0.0, 0.25, 0.5, 0.75, 0.125, 0.375]))).astype(np.float32)
    got = _run_norm(lib, c, {(0, 0): w})[0, 0]
    want = R.norm_model32(w)
    assert np.isinf(want[:, 4]).any() and not np.isfinite(want[:, 4]).any()
    assert np.array_equal(R.canon(got[:, 4]), R.canon(want[:, 4]))
    z, bound, ex = R.norm_bound(w)
    assert not ex.any()      # (float64 sees an ordinary column: the rule does not exclude it, the fp32 model speaks for it)
    keep = np.arange(9) != 4
    assert _ratio((got - z)[:, keep], bound[:, keep]) <= 2.0


# ---- median + head sum ---------------------------------------------------------------------------------------------------------------
def _run_median(lib, c, per):
    T, B, nsel, nmax = c["T"], c["B"], c["nsel"], max(c["N"])
    G = c["hpc"] or nsel
    W0 = R.pack_w(c, per, G, T)
    a0 = R.sentinel(B * nmax * T, -5000.0)
    W1, a1 = _stage(lib, 2, c, W0, acc=a0)
    assert np.array_equal(_bits(W1), _bits(W0)), "the median wrote to W"
    a0, a1 = a0.reshape(B, nmax, T), a1.reshape(B, nmax, T)
    written = np.zeros(a0.shape, bool)
    out = []
    for b in range(B):
        written[b, :c["N"][b], :c["F"][b]] = True
        out.append(a1[b, :c["N"][b], :c["F"][b]])
    assert np.array_equal(_bits(a1)[~written], _bits(a0)[~written]), "acc written outside [b][row < N[b]][f < F[b]]"
    return out, G


@pytest.mark.parametrize("c", R.MEDIAN_CASES, ids=R.case_id)
@pytest.mark.parametrize("planted", [False, True], ids=["ties", "nan_inf"])
def test_median_and_head_sum_exact(c, planted, lib):
    per = R.median_inputs(c, planted)
    got, G = _run_median(lib, c, per)
    for b in range(c["B"]):
        chunks = [np.stack([per[b, s] for s in range(g0, min(g0 + G, c["nsel"]))]) for g0 in range(0, c["nsel"], G)]
        want = R.median_sum_model32(chunks, c["width"], c["nsel"])
        assert np.array_equal(R.canon(got[b]), R.canon(want)), (b, np.argwhere(R.canon(got[b]) != R.canon(want))[:4])
    # one head alone: acc = -(0 + median) / 1, so the selection itself is compared with np.sort(...)[pad], bit for bit
    c1 = dict(c, nsel=1, hpc=0)
    sel, _ = _run_median(lib, c1, {(b, 0): per[b, 0] for b in range(c["B"])})
    for b in range(c["B"]):
        assert np.array_equal(R.canon(-sel[b]), R.canon(R.median_filter(per[b, 0], c["width"]) + np.float32(0)))


# ---- the chain -----------------------------------------------------------------------------------------------------------------------
def _chain(lib, c, inp, hpc):
    T, B, nsel, nmax = c["T"], c["B"], c["nsel"], max(c["N"])
    G = hpc or nsel
    a0 = R.sentinel(B * nmax * T, -5000.0)
    _, a1 = _stage(lib, 3, c, R.sentinel(B * G * nmax * T), inp=inp, acc=a0, hpc=hpc)
    a0, a1 = a0.reshape(B, nmax, T), a1.reshape(B, nmax, T)
    written = np.zeros(a0.shape, bool)
    for b in range(B):
        written[b, :c["N"][b], :c["F"][b]] = True
    assert np.array_equal(_bits(a1)[~written], _bits(a0)[~written]), "acc written outside [b][row < N[b]][f < F[b]]"
    return [a1[b, :c["N"][b], :c["F"][b]] for b in range(B)]


@pytest.mark.parametrize("hpc", [0, 1, 2])
def test_chain_ragged_batch(hpc, lib):
    from wis_hip import _lib
    c = R.CHAIN_CASE
    inp = R.scores_inputs(c)
    nsel, T = c["nsel"], c["T"]
    got = _chain(lib, c, inp, hpc)
    worst, nx, n = 0.0, 0, 0
    for b in range(c["B"]):
        q16 = np.stack([inp["q16"][b, s] for s in range(nsel)])
        K16 = np.stack([inp["K16"][b, s] for s in range(nsel)])
        ref, bound, excl, sb = R.chain_bound(q16, K16, c["F"][b], c["width"], -(-nsel // (hpc or nsel)))
        assert sb < 0.5
        nx += int(excl.sum()); n += excl.size
        assert np.isfinite(got[b][:, ~excl]).all()
        worst = max(worst, _ratio((got[b] - ref)[:, ~excl], bound[:, ~excl]))
        # the utterance alone, same chunking: the same bits (another nmax, ncap, no batch stride)
        c1 = dict(c, B=1, N=(c["N"][b],), F=(c["F"][b],))
        i1 = dict(inp, q=np.ascontiguousarray(inp["q"][b:b + 1, :, :c["N"][b] + 1]), Kbuf=inp["Kbuf"][b * inp["kbstride"]:(b + 1) * inp["kbstride"]],
                  ncap=c["N"][b] + 1, nmax=c["N"][b])
        alone = _chain(lib, c1, i1, hpc)[0]
        assert np.array_equal(_bits(alone), _bits(got[b])), f"utterance {b} differs from its own run"
        if hpc == 0:      # the older tap: dense q, K images back to back, ncap = n, the budget rule
            N, F = c["N"][b], c["F"][b]
            d_q = _lib.DevBuf.from_numpy(np.ascontiguousarray(inp["q"][b, :, :N]))
            d_k = _lib.DevBuf.from_numpy(np.stack([R.k_image(inp["K16"][b, s]) for s in range(nsel)]))
            d_o = _lib.DevBuf(N * F * 4)
            _lib.check(lib.wis_op_align_matrix(0, d_q.ptr, d_k.ptr, N, nsel, T, F, c["width"], d_o.ptr))
            assert np.array_equal(_bits(d_o.to_numpy(np.float32, (N, F))), _bits(got[b])), f"wis_op_align_matrix differs at utterance {b}"
    print(f"chain heads_per_chunk {hpc}: ratio {worst:.3f}  excluded {nx} of {n} columns")
    assert nx <= 0.01 * n and worst <= 2.0


# ---- DTW -----------------------------------------------------------------------------------------------------------------------------
def _dtw_batch(lib, tables, pitch, expect=0):
    from wis_hip import _lib
    B, G = len(tables), 8
    nmax, fmax = max(t.shape[0] for t in tables), max(t.shape[1] for t in tables)
    xb, cap = nmax * pitch, nmax + fmax + 2
    x = np.full(B * xb, np.nan, np.float32)      # what no table owns is NaN: a read outside a table poisons its path
    for b, t in enumerate(tables):
        x[b * xb:(b + 1) * xb].reshape(nmax, pitch)[:t.shape[0], :t.shape[1]] = t
    N, M = np.array([t.shape[0] for t in tables], np.int32), np.array([t.shape[1] for t in tables], np.int32)
    sent = np.full(B * cap + 2 * G, -77, np.int32)
    d_x, d_t, d_f, d_l = (_lib.DevBuf.from_numpy(a) for a in (x, sent, sent, np.full(B + 2 * G, -77, np.int32)))
    off = lambda d: C.c_void_p(d.ptr.value + 4 * G)
    rc = lib.wis_op_dtw_batch(0, d_x.ptr, x.size, xb, pitch, _lib.ptr(N), _lib.ptr(M), B, nmax, fmax, cap, off(d_t), off(d_f), off(d_l))
    assert rc == expect, (rc, (lib.wis_last_error() or b"").decode())
    t, f, l = d_t.to_numpy(np.int32, sent.shape), d_f.to_numpy(np.int32, sent.shape), d_l.to_numpy(np.int32, (B + 2 * G,))
    for a in (t, f, l):
        assert (a[:G] == -77).all() and (a[-G:] == -77).all(), "guard words overwritten"
    if expect:
        assert (t == -77).all() and (f == -77).all() and (l == -77).all()
        return None
    out = []
    for b in range(B):
        n = int(l[G + b])
        assert 1 <= n <= N[b] + M[b]      # (N + M: a path that non-finite costs send along both borders, as dtw_cpu's goes)
        tb, fb = t[G + b * cap:G + (b + 1) * cap], f[G + b * cap:G + (b + 1) * cap]
        assert (tb[n:] == -77).all() and (fb[n:] == -77).all(), "path slots beyond the length overwritten"
        out.append((tb[:n].astype(np.int64), fb[:n].astype(np.int64)))
    return out


def _check_dtw(tables, got):
    for x, (gt, gf) in zip(tables, got):
        with np.errstate(all="ignore"):
            rt, rf = R.dtw_fast(x)
            if x.size <= 2000:
                st, sf = R.dtw(x)
                assert np.array_equal(st, rt) and np.array_equal(sf, rf)
        assert np.array_equal(gt, rt) and np.array_equal(gf, rf), x.shape


def _tables(rng, shapes, quant=2):
    return [(np.round(rng.standard_normal(s) * quant) / quant).astype(np.float32) for s in shapes]


@pytest.mark.parametrize("pitch", ["fmax", "fmax+3", 1500])
def test_dtw_batch_ragged(pitch, lib):
    tables = _tables(np.random.default_rng(11), [(1, 1), (7, 33), (20, 5)])
    _check_dtw(tables, _dtw_batch(lib, tables, {"fmax": 33, "fmax+3": 36}.get(pitch, pitch)))


def test_dtw_batch_trace_word_edges(lib):
    tables = _tables(np.random.default_rng(12), [(5, M) for M in (14, 15, 16, 17, 31, 32, 33)])
    _check_dtw(tables, _dtw_batch(lib, tables, 36))
    tables = _tables(np.random.default_rng(13), [(M, 6) for M in (14, 15, 16, 17, 31, 32, 33)], quant=0.5)
    _check_dtw(tables, _dtw_batch(lib, tables, 6))


def test_dtw_batch_widest_and_refused(lib):
    tables = _tables(np.random.default_rng(14), [(511, 3), (3, 2)])
    _check_dtw(tables, _dtw_batch(lib, tables, 3))
    _dtw_batch(lib, _tables(np.random.default_rng(15), [(512, 3), (3, 2)]), 3, expect=WIS_E_UNSUPPORTED)


@pytest.mark.parametrize("kind", ["nan", "+inf", "-inf", "mixed"])
def test_dtw_batch_non_finite_tables(kind, lib):
    rng = np.random.default_rng(16)
    tables = _tables(rng, [(1, 1), (7, 33), (20, 5), (40, 45), (9, 17)])
    vals = {"nan": [np.nan], "+inf": [np.inf], "-inf": [-np.inf], "mixed": [np.nan, np.inf, -np.inf]}[kind]
    for t in tables[1:]:
        for _ in range(max(2, t.size // 12)):
            t[rng.integers(0, t.shape[0]), rng.integers(0, t.shape[1])] = vals[rng.integers(0, len(vals))]
    tables[0][0, 0] = vals[0]
    _check_dtw(tables, _dtw_batch(lib, tables, 48))


# ---- token probabilities ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("eot", R.PROBS_EOT)
def test_probs(eot, lib):
    from wis_hip import _lib
    lg, tg, dst = R.probs_inputs(eot)
    rows, vpad = lg.shape
    p0 = R.sentinel(12)
    d_l = _lib.DevBuf.from_numpy(lg)

    def run(tg, dst, expect=0):
        d_p = _lib.DevBuf.from_numpy(p0)
        rc = lib.wis_op_align_probs(0, d_l.ptr, rows, vpad, eot, _lib.ptr(tg), _lib.ptr(dst), d_p.ptr, 12)
        assert rc == expect, (rc, (lib.wis_last_error() or b"").decode())
        return d_p.to_numpy(np.float32, (12,))
    got = run(tg, dst)
    worst, used = 0.0, np.zeros(12, bool)
    for r in range(rows):
        if tg[r] < 0:
            continue
        used[dst[r]] = True
        p, bound, _ = R.probs_bound(lg[r], eot, tg[r])
        if np.isnan(p):
            assert np.isnan(got[dst[r]]), r
            continue
        worst = max(worst, abs(float(got[dst[r]]) - p) / bound)
    assert np.array_equal(_bits(got)[~used], _bits(p0)[~used]), "a slot without a target was written"
    print(f"probs eot {eot}: ratio {worst:.3f}")
    assert worst <= 2.0
    for bad_t, bad_d in ((vpad, int(dst[0])), (0, 12), (0, -1)):      # refused on the host, nothing written
        t2, d2 = tg.copy(), dst.copy()
        t2[0], d2[0] = bad_t, bad_d
        assert np.array_equal(_bits(run(t2, d2, WIS_E_ARG)), _bits(p0))


# ---- capture -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ub0,t0,P", [(0, 0, 4), (2, 16, 4), (0, 0, 20)])
def test_capture_exact(ub0, t0, P, lib):
    from wis_hip import _lib
    M, d, nsel, s0, n, ncap = 32, 128, 3, 1, 2, 20
    rng = np.random.default_rng(500 + ub0 + t0 + P)
    dq = rng.standard_normal((M, d)).astype(np.float32)
    special = np.array([1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11, 1.0 + 2.0 ** -11 + 2.0 ** -20, -(1.0 + 2.0 ** -11), 2.0 ** -24, 2.0 ** -25, 2.0 ** -25 * 1.001,
                        3 * 2.0 ** -25, 3e-6, -5e-8, 65504.0, 65519.0, 65520.0, -65520.0, 1e6, -7e4, 6.1e-5, 0.0], np.float32)
    dq[:, 3:3 + special.size] = special
    dq[:, 64 + 9:64 + 9 + special.size] = -special
    sel_head = np.array([1, 1, 0], np.int32)
    q0 = (-3.0 - (np.arange(8 * nsel * ncap * 64) % 13)).astype(np.float16).reshape(8, nsel, ncap, 64)      # (room behind the 4 utterances in use)
    d_dq, d_q = _lib.DevBuf.from_numpy(dq), _lib.DevBuf.from_numpy(q0)
    _lib.check(lib.wis_op_align_capture(0, d_dq.ptr, M, d, _lib.ptr(sel_head), s0, n, nsel, ub0, t0, P, ncap, d_q.ptr, q0.size))
    got = d_q.to_numpy(np.float16, q0.shape)
    want = R.capture_expected(dq, sel_head, s0, n, nsel, ub0, t0, P, ncap, q0)
    rows = [t0 + r % 16 - P for r in range(M)]
    assert any(i < 0 for i in rows) or any(i >= ncap for i in rows)
    assert (P < 20) == bool((_bits(want) != _bits(q0)).any())
    assert np.array_equal(_bits(got), _bits(want))
    rc = lib.wis_op_align_capture(0, d_dq.ptr, M, d, _lib.ptr(sel_head), s0, n, nsel, ub0, t0, P, ncap, d_q.ptr, (ub0 + 2) * nsel * ncap * 64 - 1)
    assert rc == WIS_E_ARG and np.array_equal(_bits(d_q.to_numpy(np.float16, q0.shape)), _bits(want))
