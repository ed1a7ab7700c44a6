"""CPU twin of tests/test_gpu_dec_attn_edges.py: the numpy fp32 models of tests/dec_attn_ref.py (the plain self-attention loop at NB 2 / 4 / 8, the long
kernel's four-wave partials and merge, one cross-attention chunk plus the combine) meet the bound of that module with factor 1 on every pattern at the
shapes the GPU file uses, and every pattern reaches the path it was built for - read off the models' logs.  The fold forms' operands give the
intended f16 query whatever the fp32 order (the 1 / 16 ulp assertion)."""
import numpy as np
import pytest

import dec_attn_ref as D


def _check(out, ref, unit, what):
    assert np.isfinite(np.asarray(out, np.float64)).all(), what
    r = D.ratios(out, ref, unit)
    w = float(r.max())
    assert w <= 1.0, (what, w, np.unravel_index(int(r.argmax()), r.shape))
    return w


@pytest.mark.parametrize("ctx", [448, 64])
@pytest.mark.parametrize("nb", [2, 4, 8])
def test_self_model_meets_the_bound_and_patterns_reach_their_paths(nb, ctx):
    worst = {}
    for n in D.self_lens(nb, ctx):
        for pattern in D.PATTERNS:
            rng = np.random.default_rng([nb, ctx, n, D.PATTERNS.index(pattern)])
            q, k, v = D.problem(pattern, n, 8 * nb, 1, rng, False)
            junk = rng.standard_normal((max(ctx, 8 * nb) - n, 64)).astype(np.float16)      # what lies behind the history in the slot
            out, log = D.self_model(q[0], np.concatenate([k, junk]), np.concatenate([v, junk]), n, nb)
            ref, unit = D.reference(q, k, v, D.n_acc_self(n, nb))
            worst[pattern] = max(worst.get(pattern, 0.0), _check(out[None], ref, unit, (pattern, nb, n)))
            passes = D.cdiv(n, 8 * nb)
            assert log["passes"] == passes
            if passes >= 2:
                if pattern in ("up20", "up150"):      # (up3: a step the noise can undo - rescales by factors near 1, not in every pass)
                    assert log["rescales"] == passes - 1, (pattern, n, log)
                if pattern in ("up150", "far150_last", "far600_last"):      # the earlier partials are rescaled to exact zeros
                    assert log["alphas"][-1] == 0.0, (pattern, n, log)
                if pattern.startswith("down") or (pattern.startswith("far") and pattern.endswith("_first")):
                    assert log["rescales"] == 0, (pattern, n, log)
                if pattern in ("down150", "far150_first", "far600_first"):
                    assert log["zero_weights"] >= n - 8 * nb, (pattern, n, log)
                if pattern == "tail" and n % (8 * nb):
                    assert log["clamped"] == passes * 8 * nb - n and log["rescales"] >= 1, (pattern, n, log)
    print(f"self model nb{nb} ctx{ctx}: " + " ".join(f"{p}={w:.3f}" for p, w in worst.items()))


@pytest.mark.parametrize("plen", D.PLENS)
def test_long_model_meets_the_bound_and_patterns_reach_their_paths(plen):
    worst = {}
    sufs = D.SUFFIXES
    for pattern in D.PATTERNS:
        rng = np.random.default_rng([plen, D.PATTERNS.index(pattern)])
        q, kp, vp, own = D.long_problem(pattern, plen, sufs, rng)
        ctx = 448
        junk = rng.standard_normal((ctx, 64)).astype(np.float16)
        kps, vps = np.concatenate([kp, junk])[:ctx], np.concatenate([vp, junk])[:ctx]
        maxlast = plen + max(sufs) - 1
        for j, s in enumerate(sufs):
            ko, vo = own[j]
            kos = np.concatenate([junk[:plen], ko, junk])[:ctx]      # the row's own slot: its positions plen .. last, anything elsewhere
            vos = np.concatenate([junk[:plen], vo, junk])[:ctx]
            last = plen + s - 1
            out, log = D.long_model(q[j], kps, vps, kos, vos, plen, last, maxlast)
            ref, unit = D.reference(q[j:j + 1], np.concatenate([kp, ko]), np.concatenate([vp, vo]), D.n_acc_long(plen + s, plen))
            worst[pattern] = max(worst.get(pattern, 0.0), _check(out[None], ref, unit, (pattern, plen, s)))
            assert log["suffix_passes"] == D.cdiv(max(sufs), 32)
            # waves without a valid position: wave w holds prefix positions 8 w .. 8 w + 7 (mod 32) and suffix positions plen + 8 w ..
            empty = sum(1 for w in range(4) if plen <= 8 * w and s <= 8 * w)
            assert log["empty_waves"] == empty, (pattern, plen, s, log)
            if plen <= 8 and s <= 8:
                assert log["empty_waves"] >= 1
            if pattern in ("far150_first", "far600_first") and plen >= 33:      # block 0 is spread over all four waves: later blocks weigh 0
                assert log["zero_weights"] > 0, (pattern, plen, s, log)
            if pattern in ("far150_last", "far600_last", "one") and plen + s > 32 and s < 25:
                # the mass sits in at most three waves' positions: the merge weight of another wave is an exact 0
                assert log["zero_merge"] >= 1, (pattern, plen, s, log)
            if pattern == "tail" and s % 32:
                assert log["clamped"] > 0
    print(f"long model plen{plen}: " + " ".join(f"{p}={w:.3f}" for p, w in worst.items()))


@pytest.mark.parametrize("T,CL", [(1500, 256), (1536, 256), (449, 256), (1500, 128)])
def test_cross_model_meets_the_bound_and_patterns_reach_their_paths(T, CL):
    worst = {}
    R = 5
    C = D.cdiv(T, CL)
    for pattern in D.CROSS_PATTERNS:
        rng = np.random.default_rng([T, CL, D.CROSS_PATTERNS.index(pattern)])
        q, k, v = D.problem(pattern, T, CL, R, rng, True)
        assert np.array_equal(q.astype(np.float16).astype(np.float32), q)
        out, log = D.cross_model(q, k, v, CL)
        ref, unit = D.reference(q, k, v, D.n_acc_cross(T, CL), chunk=CL)
        worst[pattern] = max(worst.get(pattern, 0.0), _check(out, ref, unit, (pattern, T, CL)))
        assert log["masked"] == C * CL - T
        if pattern in ("up150", "down150") or pattern.startswith("far"):
            assert log["zero_combine"] == R * (C - 1), (pattern, log)      # every chunk but the one that holds the mass: weight exactly 0
        if pattern in ("tail", "head", "edge_last", "edge_first") or pattern.startswith("edge_k"):
            assert log["denormal_p"] > 0, (pattern, log)                  # the marked key's neighbours: f16 denormals about the chunk maximum
        if pattern == "one":
            assert log["zero_p"] == R * (min(CL, T - (T // 2) // CL * CL) - 1), (pattern, log)
    print(f"cross model T{T} CL{CL}: " + " ".join(f"{p}={w:.3f}" for p, w in worst.items()))


@pytest.mark.parametrize("H,M", [(6, 5), (6, 8), (20, 50), (32, 10)])
def test_fold_operands_give_the_intended_query(H, M):
    d = 64 * H
    rng = np.random.default_rng([H, M])
    q16 = np.empty((M, d), np.float32)
    zero = np.zeros(d, bool)
    for h in range(H):
        pattern = D.CROSS_PATTERNS[h % len(D.CROSS_PATTERNS)]
        q16[:, 64 * h:64 * h + 64] = D.problem(pattern, 64, 32, M, rng, True)[0]
        zero[64 * h:64 * h + 64] = pattern == "flat"
    ops = D.fold_operands(q16, rng, zero)
    w = D.fold_query_check(q16, ops)
    if d <= 1280:
        w = max(w, D.fold_query_check(q16, ops, from_rows=True))
    print(f"fold operands H{H} M{M}: finished query within {w:.4f} f16 ulp of the intended one")
    assert w <= 1 / 16


@pytest.mark.parametrize("pattern", ["control", "tail", "flat"])
def test_models_meet_the_bound_where_the_f16_output_is_a_denormal(pattern):
    """V scaled by 2^-16: every output lies on the f16 denormal grid, whose rounding (2^-25, absolute) is a term of `unit` of its own - without it the
    self-attention model stands above 1 here, as the TREE kernel's `tail` case did on the GPU (dec_attn_ref.py's docstring)"""
    rng = np.random.default_rng([7, D.PATTERNS.index(pattern)])
    small = lambda v: (v.astype(np.float32) * np.float32(2.0 ** -16)).astype(np.float16)
    n, nb = 76, 8
    q, k, v = D.problem(pattern, n, 8 * nb, 4, rng, False)
    v = small(v)
    pad = np.zeros((64, 64), np.float16)
    for r in range(4):
        out, _ = D.self_model(q[r], np.concatenate([k, pad]), np.concatenate([v, pad]), n, nb)
        ref, unit = D.reference(q[r:r + 1], k, v, D.n_acc_self(n, nb))
        assert (np.abs(ref) < 2.0 ** -14).all()
        _check(out[None], ref, unit, (pattern, "self", r))
    q, k, v = D.problem(pattern, 449, 256, 5, rng, True)
    v = small(v)
    out, _ = D.cross_model(q, k, v, 256)
    ref, unit = D.reference(q, k, v, D.n_acc_cross(449, 256), chunk=256)
    _check(out, ref, unit, (pattern, "cross"))
