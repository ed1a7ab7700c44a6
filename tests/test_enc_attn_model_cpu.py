"""The numpy model of the lazy attention loop and the score patterns of tests/test_gpu_enc_attn_ops.py, checked without a GPU:
(a) the model (fp32 arithmetic, f16 P, the kernel's raise rule and split merge) stays within the bound of tests/enc_attn_ref.py with
    factor 1 on every pattern and length the GPU file uses - so the float64 reference and the bound themselves are sound, and the
    factor 2 the GPU gets is head-room, not a fit;
(b) every pattern reaches the path it was built for, counted as reference steps ("slow" tiles) per wave in the model - so that an edit
    of the patterns cannot silently turn the GPU cases into plain noise."""
import numpy as np
import pytest

import enc_attn_ref as R


def _case(pattern, T):
    q, k, v = R.make_inputs(pattern, 1, T, 1)
    return q[0, :, 0], k[0, :, 0], v[0, :, 0]


@pytest.mark.parametrize("T", R.T_LIST + [330])
@pytest.mark.parametrize("pattern", R.PATTERNS)
def test_model_within_bound(pattern, T):
    q, k, v = _case(pattern, T)
    ref, unit = R.reference(q, k, v, base2=True)
    assert np.isfinite(ref).all() and np.isfinite(unit).all()
    for split in (False, True)[:1 + (T >= R.SPLIT_MIN_T)]:
        out, _ = R.lazy_model(q, k, v, split)
        assert np.isfinite(out).all()
        worst = float(R.ratios(out, ref, unit).max())
        print(f"model {pattern} T{T} split{int(split)}: max (|out - ref| - r) / unit = {worst:.3f}")
        assert worst <= 1.0, (pattern, T, split, worst)


def test_reference_alone_passes():
    """the float64 reference rounded to f16 is inside r = 2^-10 |ref| everywhere (ratio 0), and base e differs from base 2"""
    q, k, v = _case("control", 200)
    ref2, unit2 = R.reference(q, k, v, base2=True)
    refe, _ = R.reference(q, k, v, base2=False)
    assert R.ratios(ref2.astype(np.float16), ref2, unit2).max() == 0.0
    assert R.ratios(refe.astype(np.float16), ref2, unit2).max() > 2.0


@pytest.mark.parametrize("T", [257, 321, 330, 520])
def test_patterns_reach_their_paths(T):
    nt = (T + 63) // 64
    slow = {p: R.lazy_model(*_case(p, T), False)[1] for p in R.PATTERNS}
    for p in R.PATTERNS:
        assert slow[p].shape == ((T + 31) // 32, nt) and slow[p][:, 0].all()      # the first tile always sets the reference
    assert slow["control"].mean() < 1 / 3                                   # the common path: no reference step
    for p in ("up17", "up40", "up200"):
        assert slow[p].all(), p                                             # every tile raises: one key of it overflows f16 already
    assert slow["up14"][:, :T // 64].all()                                  # every FULL tile raises, by its row sum alone (a tail of one key cannot)
    q, k, _ = _case("up14", T)
    s = q.astype(np.float64) @ k.astype(np.float64).T
    assert (s[:, 64:128].max(1) - s[:, :64].max(1)).max() < 16              # ... its weights stay inside f16 (< 2^16) on the fast path
    assert not slow["down12"][:, 1:].any()
    assert not slow["threshold"][:, 1].any() and slow["threshold"][:, 2].all()      # 32 x 2^9.96 < 2^15 == 32 x 2^10
    assert not slow["threshold"][:, 3:].any()
    # diverge: only the waves of queries 5 and 37 of each 128-query tile take the step in key tile 1
    d = slow["diverge"][:, 1]
    want = np.zeros_like(d)
    for qa in (5, 37):
        want[[(t0 + qa) // 32 for t0 in range(0, T, 128) if t0 + qa < T]] = True
    assert np.array_equal(d, want)
    last = nt - 1
    assert slow["tail"][:, last].all() and not slow["tail"][:, 1:last].any()     # + 20 at key T - 1
    nh = (nt + 1) // 2
    for p, tiles in (("split_up150", [nh]), ("split_mass_hi", [nh]), ("split_down150", []), ("split_mass_lo", [])):
        want = np.zeros(nt, bool)
        want[[0] + tiles] = True
        assert (slow[p] == want[None, :]).all(), p


def test_threshold_scores_are_exact():
    q, k, _ = _case("threshold", 321)
    s = q.astype(np.float64) @ k.astype(np.float64).T
    assert (s[:, :64] == 0).all() and (s[:, 128:192] == 10.0).all()
    assert (np.abs(s[:, 64:128] - 9.96) < 2e-3).all() and (s[:, 64:128] < 10).all()
    assert (s.astype(np.float32) == s).all()


def test_split_model_merges_distant_references():
    """the halves of the split_* patterns end on references 150 / 600 apart; the merged model still matches the unsplit one closely"""
    for p in ("split_up150", "split_down150", "split_mass_hi", "split_mass_lo"):
        q, k, v = _case(p, 321)
        a, _ = R.lazy_model(q, k, v, False)
        b, _ = R.lazy_model(q, k, v, True)
        assert np.abs(a.astype(np.float64) - b.astype(np.float64)).max() <= 2.0 ** -9 * np.abs(a.astype(np.float64)).max()
