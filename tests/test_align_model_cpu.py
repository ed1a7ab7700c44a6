"""No GPU: the CPU twin of tests/test_gpu_align_stages.py.  The float32 numpy models of the alignment kernels (tests/align_ref.py: the kernels'
stated operation order) must stay within ONE times the per-element bounds of that module on the very inputs the GPU test uses (the GPU test
allows two), so the bounds are shown to hold for a correct fp32 implementation before any kernel runs; the exact models (median selection,
head sum) are checked against the float64 functions the older tests use; the share of columns that take no part is asserted per case."""
import numpy as np
import pytest

import align_ref as R


def _ratio(err, bound):
    with np.errstate(all="ignore"):
        return float(np.max(np.abs(err) / bound, initial=0.0))


@pytest.mark.parametrize("c", R.SCORES_CASES, ids=R.case_id)
def test_scores_model_meets_the_bound(c):
    inp = R.scores_inputs(c)
    worst, Emax = 0.0, 0.0
    for (b, s), q16 in inp["q16"].items():
        p, bound, (E, meas) = R.scores_bound(q16, inp["K16"][b, s])
        got, _ = R.scores_model32(q16, inp["K16"][b, s])
        F = c["F"][b]
        assert np.isfinite(got).all() and (bound > 0).all()
        if F < c["T"] and c["spread"]:      # the planted key lies beyond the crop and holds the row maximum
            assert (p[:, F:].argmax(-1) + F == p.argmax(-1)).all() and (c["spread"] < 20 or p[:, F:].sum(-1).min() > 0.5)
        worst = max(worst, _ratio(got[:, :F] - p[:, :F], bound[:, :F]))
        Emax = max(Emax, meas)
    print(f"scores {R.case_id(c)}: model ratio {worst:.3f}  numpy expf error {Emax / R.U:.3f} x 2^-24")
    assert worst <= 1.0


def _participating(c, excl_by_bs):
    """the exclusion rule's two assertions: at most 1 % of the case's columns (utterances of one token, whose every std is 0, have exact
    cases of their own and are not counted), and not all of them"""
    n = sum(e.size for (b, s), e in excl_by_bs.items() if c["N"][b] > 1)
    x = sum(int(e.sum()) for (b, s), e in excl_by_bs.items() if c["N"][b] > 1)
    assert n > 0 and x <= 0.01 * n and x < n, (x, n)
    return x / n


@pytest.mark.parametrize("c", R.NORM_CASES, ids=R.case_id)
def test_norm_model_meets_the_bound(c):
    per = R.norm_inputs(c)
    worst, excl = 0.0, {}
    for (b, s), w in per.items():
        got = R.norm_model32(w)
        z, bound, ex = R.norm_bound(w)
        excl[b, s] = ex
        if c["N"][b] == 1:
            assert ex.all() and np.isnan(got).all()
            continue
        sd = w.astype(np.float64).std(0)
        assert (sd[~ex] >= 2.0 ** -50).all()      # the squares of the deviations stay fp32 normals (one rounding is counted for them)
        worst = max(worst, _ratio((got - z)[:, ~ex], bound[:, ~ex]))
    share = _participating(c, excl)
    print(f"norm {R.case_id(c)}: model ratio {worst:.3f}  excluded {100 * share:.2f} %")
    assert worst <= 1.0


@pytest.mark.parametrize("i", [1, 4])
def test_norm_model_on_softmax_output_meets_the_bound(i):
    """the GPU test's stage 0 -> stage 1 case on the models: real attention weights, most of the mass beyond the crop"""
    c = R.SCORES_CASES[i]
    inp = R.scores_inputs(c)
    worst, excl = 0.0, {}
    for (b, s), q16 in inp["q16"].items():
        w = R.scores_model32(q16, inp["K16"][b, s])[0][:, :c["F"][b]]
        z, bound, ex = R.norm_bound(w)
        excl[b, s] = ex
        if c["N"][b] > 1:
            assert (w.astype(np.float64).std(0)[~ex] >= 2.0 ** -50).all()
            worst = max(worst, _ratio((R.norm_model32(w) - z)[:, ~ex], bound[:, ~ex]))
    _participating(c, excl)
    assert worst <= 1.0


def test_norm_bound_is_tight_where_std_is_ordinary_and_wide_where_it_is_small():
    rng = np.random.default_rng(5)
    w = rng.random((8, 2))
    w[:, 1] = 0.5 + w[:, 1] * 1e-6
    _, bound, ex = R.norm_bound(w.astype(np.float32))
    assert not ex.any() and bound[:, 0].max() < 16 * R.U * 3 and bound[:, 1].min() > 1e3 * bound[:, 0].max()


@pytest.mark.parametrize("N", [4, 8, 16])
def test_norm_model_equal_column_is_nan_alone(N):
    w = R.norm_inputs(R._case(130 + N, T=8, B=1, nsel=1, N=(N,), F=(8,)))[0, 0]
    w[:, 3] = np.float32(0.375)
    got, ref = R.norm_model32(w), R.norm_model32(np.delete(w, 3, axis=1))
    assert np.isnan(got[:, 3]).all() and np.array_equal(np.delete(got, 3, axis=1), ref) and np.isfinite(ref).all()


@pytest.mark.parametrize("c", R.MEDIAN_CASES, ids=R.case_id)
@pytest.mark.parametrize("planted", [False, True])
def test_median_model_is_nan_last_sort_selection(c, planted):
    per = R.median_inputs(c, planted)
    pad = c["width"] // 2
    for (b, s), w in per.items():
        got = R.median_select32(w, c["width"])
        want = R.median_filter(w, c["width"])      # np.sort of the reflect-padded windows, element pad
        assert got.dtype == np.float32 and np.array_equal(R.canon(got), R.canon(want))
        if planted and w.shape[1] >= 255:      # NaN beside finite values in the windows, and both kinds of result
            assert np.isnan(got).any() and np.isfinite(got).any()
    G = c["hpc"] or c["nsel"]
    for b in range(c["B"]):      # the head sum against float64 (its only roundings: nsel + chunks + 1 of them)
        chunks = [np.stack([per[b, s] for s in range(g0, min(g0 + G, c["nsel"]))]) for g0 in range(0, c["nsel"], G)]
        got = R.median_sum_model32(chunks, c["width"], c["nsel"]).astype(np.float64)
        m = np.array([R.median_filter(per[b, s].astype(np.float64), c["width"]) for s in range(c["nsel"])])
        with np.errstate(all="ignore"):
            want = -m.mean(0)
            ok = np.isfinite(want)
            assert np.array_equal(np.isnan(got), np.isnan(want))
            assert (np.abs(got - want)[ok] <= R.gamma(c["nsel"] + len(chunks) + 1) * np.abs(m).sum(0)[ok] / c["nsel"] + 1e-300).all()


@pytest.mark.parametrize("hpc", [0, 1, 2])
def test_chain_model_meets_the_bound(hpc):
    c = R.CHAIN_CASE
    inp = R.scores_inputs(c)
    G = hpc or c["nsel"]
    worst, nx, n = 0.0, 0, 0
    for b in range(c["B"]):
        q16 = np.stack([inp["q16"][b, s] for s in range(c["nsel"])])
        K16 = np.stack([inp["K16"][b, s] for s in range(c["nsel"])])
        ref, bound, excl, sb = R.chain_bound(q16, K16, c["F"][b], c["width"], -(-c["nsel"] // G))
        assert sb < 0.5      # the score error moves no participating column's std by half of it
        got = R.chain_model32(q16, K16, c["F"][b], c["width"], c["nsel"], G).astype(np.float64)
        worst = max(worst, _ratio((got - ref)[:, ~excl], bound[:, ~excl]))
        nx += int(excl.sum()); n += excl.size
    print(f"chain heads_per_chunk {hpc}: model ratio {worst:.3f}  excluded {nx} of {n} columns")
    assert nx <= 0.01 * n and worst <= 1.0


@pytest.mark.parametrize("eot", R.PROBS_EOT)
def test_probs_model_meets_the_bound(eot):
    lg, tg, dst = R.probs_inputs(eot)
    assert sorted(set(dst.tolist())) == sorted(dst.tolist()) and (lg[:, eot:] == 50.0).all()
    worst = 0.0
    for r in range(lg.shape[0]):
        if tg[r] < 0:
            continue
        p, bound, _ = R.probs_bound(lg[r], eot, tg[r])
        got = float(R.probs_model32(lg[r], eot, tg[r]))
        if np.isnan(p):
            assert r in (3, 5, 6) and np.isnan(got)
            continue
        assert 0.0 <= p <= 1.0
        worst = max(worst, abs(got - p) / bound)
    print(f"probs eot {eot}: model ratio {worst:.3f}")
    assert worst <= 1.0


def test_capture_reference_rounds_like_the_f16_cast():
    dq = np.array([[65504.0, 65519.9, 65520.0, -1e6, 2.0 ** -24, 2.0 ** -25, 2.0 ** -25 * 1.0001, 1.0 + 2.0 ** -11] * 8] * 16, np.float32)
    q0 = np.full((1, 1, 16, 64), -3.0, np.float16)
    out = R.capture_expected(dq, [0], 0, 1, 1, 0, 0, 4, 16, q0)
    assert (out[0, 0, 12:] == -3.0).all()
    row = out[0, 0, 0, :8].astype(np.float64)
    assert row[0] == 65504.0 and row[1] == 65504.0 and np.isposinf(row[2]) and np.isneginf(row[3])
    assert row[4] == 2.0 ** -24 and row[5] == 0.0 and row[6] == 2.0 ** -24 and row[7] == 1.0
