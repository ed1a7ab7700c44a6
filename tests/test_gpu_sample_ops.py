"""-m gpu: what runs behind the logits, op by op - the two kernels that permute the self-attention cache in place (kv_reorder_kernel,
kv_gather_kernel), bit-exact against a numpy gather, and the three softmax readers (no_speech_kernel, lang_probs_kernel, logit_stats_kernel +
greedy_pick_kernel) against float64.  Through the wis_op_* taps of csrc/taps.hip, which call the product's launch functions.

Tolerances of the softmax readers.  No bar is fixed in advance: per case the error of a plain numpy fp32 RESTATEMENT of the kernel's reduction
against float64 is measured on the same inputs - per-256-strided partial sums and a tree for no_speech (expf there is an accurate exponential:
np.exp in fp32), per-64 for lang_probs, per sub-chunk (max, sum) pairs merged over the 64 sub-chunks for the greedy pick; the last two kernels
use __expf, which is exp2 of the fp32 product log2(e) x (clang's __clang_hip_math.h), restated as such - and the bar is 4 x that error, with a floor
of a few fp32 ulps of the result.  The measurement never uses the kernel's output.  Every test prints (restatement error, bar, kernel error);
profiles/sample_ops_tests.md holds the figures of one run.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
EOT = 50257
ULP = 2.0 ** -23               # fp32: spacing of the numbers in [1, 2)
VS_INTS, VS_NWIN, VS_BASE, VS_PATH, VS_PATH_W = 32 + 8 * 32, 2, 16, 32, 32      # kernels.hpp DRAFT_VS_*: the verification state's layout
WIS_E_ARG = -1


def _biteq(a, b):
    """bit equality (NaN payloads and signed zeros included)"""
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))


def _i32(a):
    return np.ascontiguousarray(np.asarray(a, np.int32))


def _random_f16_bits(rng, shape):
    """every f16 bit pattern is fair game: NaN payloads, infinities, denormals, both zeros"""
    a = rng.integers(0, 1 << 16, size=shape, dtype=np.uint16)
    a.reshape(-1)[:8] = [0x7E00, 0x7C01, 0xFFFF, 0xFC00, 0x7C00, 0x8000, 0x0001, 0x7DFF]
    return a


# ---- kv_reorder ---------------------------------------------------------------------------------------------------------------------------
def _parent_tables(rng, B, beam):
    """name -> parent i32 [B * beam] (absolute slots of the row's own utterance)"""
    base = np.repeat(np.arange(B) * beam, beam)
    rel = {"identity": np.tile(np.arange(beam), B),
           "rotation": np.tile((np.arange(beam) + 1) % beam, B),                                   # one k-cycle
           "swap": np.tile(np.array([1, 0] + list(range(2, beam))), B),                            # a swap plus fixed points
           "fan_out": np.tile(np.full(beam, beam - 1), B),                                         # every slot from one slot
           "random": rng.integers(0, beam, size=B * beam)}                                         # with repeats
    return {k: _i32(base + v) for k, v in rel.items()}


def _reorder(lib, old_k, old_v, parent, step_u, done, B, beam, P, ctx, d):
    from wis_hip._lib import DevBuf, check
    L, slots = old_k.shape[0], old_k.shape[1]
    dk, dv = DevBuf.from_numpy(old_k), DevBuf.from_numpy(old_v)
    dp, ds, dd = DevBuf.from_numpy(_i32(parent)), DevBuf.from_numpy(_i32(step_u)), DevBuf.from_numpy(_i32(done))
    check(lib.wis_op_kv_reorder(0, dk.ptr, dv.ptr, slots * ctx * d, L, dp.ptr, ds.ptr, dd.ptr, B, beam, P, ctx, d))
    return dk.to_numpy(np.uint16, old_k.shape), dv.to_numpy(np.uint16, old_v.shape)


def _reorder_ref(old, parent, step_u, done, B, beam, P):
    new = old.copy()
    for b in range(B):
        if done[b]:
            continue
        npos = P - 1 + step_u[b]
        for j in range(beam):
            new[:, b * beam + j, :npos] = old[:, parent[b * beam + j], :npos]
    return new


# d / 8 = 48, 160, 16, 288 sixteen-byte chunks per row: below a block of 256 threads, below a wave, above a block; all but the third shape hold more
# than 8 positions, so the 8 position slices of the grid wrap
@pytest.mark.parametrize("L,B,beam,d,ctx,P,step", [(2, 1, 5, 384, 64, 3, 7), (2, 3, 8, 1280, 64, 4, 20), (1, 2, 2, 128, 32, 1, 1), (2, 2, 5, 2304, 48, 3, 12)])
def test_kv_reorder_is_the_gather_by_parent(lib, L, B, beam, d, ctx, P, step):
    rng = np.random.default_rng([L, B, beam, d])
    slots = B * beam + 2                       # two slots behind the batch: never touched
    old_k, old_v = _random_f16_bits(rng, (L, slots, ctx, d)), _random_f16_bits(rng, (L, slots, ctx, d))
    step_u = [max(1, step - 3 * b) for b in range(B)]                  # every utterance at a step of its own
    for name, parent in _parent_tables(rng, B, beam).items():
        for done in ([0] * B,) if B == 1 else ([0] * B, [0] * (B - 1) + [1], [1] + [0] * (B - 1)):
            new_k, new_v = _reorder(lib, old_k, old_v, parent, step_u, done, B, beam, P, ctx, d)
            for what, old, new in (("K", old_k, new_k), ("V", old_v, new_v)):
                exp = _reorder_ref(old, parent, step_u, done, B, beam, P)
                assert _biteq(new, exp), (name, done, what, np.argwhere(new != exp)[:4].tolist())
                # (spelled out: positions at or above P - 1 + step_u[b], finished utterances and the slots behind the batch keep their bytes)
                for b in range(B):
                    npos = P - 1 + step_u[b] if not done[b] else 0
                    assert _biteq(new[:, b * beam:(b + 1) * beam, npos:], old[:, b * beam:(b + 1) * beam, npos:]), (name, done, what, b)
                assert _biteq(new[:, B * beam:], old[:, B * beam:])
                if name == "identity":
                    assert _biteq(new, old)
    print(f"kv_reorder L{L} B{B} beam{beam} d{d}: 5 parent tables x {1 if B == 1 else 3} done patterns bit-identical to the numpy gather")


def test_kv_reorder_beam_1_moves_nothing(lib):
    rng = np.random.default_rng(1)
    old_k, old_v = _random_f16_bits(rng, (2, 3, 32, 128)), _random_f16_bits(rng, (2, 3, 32, 128))
    new_k, new_v = _reorder(lib, old_k, old_v, [1, 0, 0], [5, 5, 5], [0, 0, 0], 3, 1, 2, 32, 128)      # (a parent table that WOULD move rows)
    assert _biteq(new_k, old_k) and _biteq(new_v, old_v)


# ---- kv_gather ----------------------------------------------------------------------------------------------------------------------------
def _gather(lib, old_k, old_v, vs, done, beam, w0, ctx, d):
    from wis_hip._lib import DevBuf, check
    L, slots = old_k.shape[0], old_k.shape[1]
    dk, dv, dvs, dd = DevBuf.from_numpy(old_k), DevBuf.from_numpy(old_v), DevBuf.from_numpy(_i32(vs)), DevBuf.from_numpy(_i32([done]))
    check(lib.wis_op_kv_gather(0, dk.ptr, dv.ptr, slots * ctx * d, L, dvs.ptr, dd.ptr, beam, w0, ctx, d))
    return dk.to_numpy(np.uint16, old_k.shape), dv.to_numpy(np.uint16, old_v.shape)


@pytest.mark.parametrize("d", [384, 1280])
@pytest.mark.parametrize("beam", [2, 5, 8])
def test_kv_gather_is_the_gather_by_path(lib, beam, d):
    L, ctx = 2, 64
    rng = np.random.default_rng([beam, d])
    slots = beam + 1
    old_k, old_v = _random_f16_bits(rng, (L, slots, ctx, d)), _random_f16_bits(rng, (L, slots, ctx, d))
    n = 0
    for w0 in (3, 10):
        for nwin in (1, 7, min(32, ctx - w0)):
            base = rng.integers(0, beam, size=beam)                                  # random with repeats
            path = np.stack([rng.permutation(beam) if u % 2 else rng.integers(0, beam, size=beam) for u in range(nwin)], axis=1)      # [beam][nwin]: permutations
            path[:, 0] = (np.arange(beam) + 1) % beam                                # (cycles that differ from step to step) and tables with repeats
            vs = np.full(VS_INTS, beam, np.int32)                                    # (entries beyond nwin / beam name the spare slot: never to be used)
            vs[0], vs[VS_NWIN] = 0, nwin
            vs[VS_BASE:VS_BASE + beam] = base
            for j in range(beam):
                vs[VS_PATH + VS_PATH_W * j:VS_PATH + VS_PATH_W * j + nwin] = path[j]
            for done in (0, 2):                                                      # 2 = parked: the window's steps still stand
                new_k, new_v = _gather(lib, old_k, old_v, vs, done, beam, w0, ctx, d)
                for what, old, new in (("K", old_k, new_k), ("V", old_v, new_v)):
                    exp = old.copy()
                    for j in range(beam):
                        exp[:, j, :w0] = old[:, base[j], :w0]
                        for u in range(nwin):
                            exp[:, j, w0 + u] = old[:, path[j, u], w0 + u]
                    assert _biteq(new, exp), (w0, nwin, done, what, np.argwhere(new != exp)[:4].tolist())
                    assert _biteq(new[:, :, w0 + nwin:], old[:, :, w0 + nwin:]) and _biteq(new[:, beam:], old[:, beam:])
                n += 1
            vs0 = vs.copy(); vs0[VS_NWIN] = 0
            for v, done in ((vs, 1), (vs0, 0)):                                      # finished inside the window / nothing replayed: nothing is written
                new_k, new_v = _gather(lib, old_k, old_v, v, done, beam, w0, ctx, d)
                assert _biteq(new_k, old_k) and _biteq(new_v, old_v), (w0, nwin, done)
    print(f"kv_gather beam{beam} d{d}: {n} windows bit-identical to the numpy gather; done = 1 and an empty window write nothing")


# ---- fp32 restatements --------------------------------------------------------------------------------------------------------------------
def _tree(a):
    """sum of the last axis (a power of two) by halving, in the array's precision"""
    while a.shape[-1] > 1:
        h = a.shape[-1] // 2
        a = a[..., :h] + a[..., h:]
    return a[..., 0]


def _fast_exp(x):
    """__expf: exp2 of the fp32 product log2(e) x"""
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        return np.exp2((np.float32(1.4426950408889634) * x.astype(np.float32)).astype(np.float32)).astype(np.float32)


def _softmax64(x):
    x = x.astype(np.float64)
    e = np.exp(x - x.max())
    return e / e.sum()


def _report(what, ref_err, bar, got_err):
    print(f"{what}: fp32 restatement vs float64 {ref_err:.3e}, bar {bar:.3e}, kernel vs float64 {got_err:.3e}")


def _extreme_rows(rng, n, width):
    """rows [n][width]: N(0, 3^2); all equal; one value at +80 over N(0, 1); everything near -80; rest N(0, 3^2)"""
    x = (3.0 * rng.standard_normal((n, width))).astype(np.float32)
    kinds = ["normal"] * n
    for r, k in zip(range(n), ("normal", "equal", "max80", "near-80")):
        kinds[r] = k
        if k == "equal":
            x[r] = np.float32(1.625)
        elif k == "max80":
            x[r] = rng.standard_normal(width).astype(np.float32); x[r, int(rng.integers(0, width))] = np.float32(80.0)
        elif k == "near-80":
            x[r] = (-80.0 + 0.25 * rng.standard_normal(width)).astype(np.float32)
    return x, kinds


# ---- no_speech ----------------------------------------------------------------------------------------------------------------------------
def _no_speech_f32(row, ns):
    """no_speech_kernel in numpy fp32: thread t sums exp(row[i] - max) over i = t, t + 256, ..; four wave sums; (w0 + w1) + (w2 + w3)"""
    V = row.shape[0]
    mx = row.max()
    pad = np.full((-V) % 256, -np.inf, np.float32)
    e = np.exp(np.concatenate([row, pad]).reshape(-1, 256) - mx).astype(np.float32)
    part = np.add.reduce(e, axis=0, dtype=np.float32)                 # row after row: thread t's running sum
    w = _tree(part.reshape(4, 64))
    s = np.float32(np.float32(w[0] + w[1]) + np.float32(w[2] + w[3]))
    return np.float32(np.exp(np.float32(row[ns] - mx))) / s


@pytest.mark.parametrize("r0", [0, 2])
@pytest.mark.parametrize("V", [51865, 51866])
def test_no_speech_against_float64(lib, V, r0):
    from wis_hip._lib import DevBuf, check
    B, rs = 3, 4
    ld = (V + 31) // 32 * 32
    rng = np.random.default_rng([V, r0])
    worst = (0.0, 0.0, 0.0)
    for case in range(2):
        rows, kinds = _extreme_rows(rng, 5, V)
        rows = rows[[0, 1, 2]] if case == 0 else rows[[3, 4, 0]]
        kinds = kinds[:3] if case == 0 else [kinds[3], "ns-is-max", kinds[0]]
        for ns in (0, V // 2 + 7, V - 1):
            x = rows.copy()
            if case == 1:
                x[1, ns] = x[1].max() + np.float32(2.5)               # <|nospeech|> itself is the row's maximum
            # the rows of the other prompt positions hold other logits, the padding columns a value that would swamp the sum
            buf = (3.0 * rng.standard_normal((B * rs, ld)) + 4.0).astype(np.float32)
            buf[:, V:] = np.float32(1e4)
            buf[np.arange(B) * rs + r0, :V] = x
            d_l, d_o = DevBuf.from_numpy(buf), DevBuf.from_numpy(np.full(B, -1.0, np.float32))
            check(lib.wis_op_no_speech(0, d_l.ptr, ld, B, rs, r0, V, ns, d_o.ptr))
            got = d_o.to_numpy(np.float32, (B,))
            for b in range(B):
                p64 = _softmax64(x[b])[ns]
                ref_err = abs(float(_no_speech_f32(x[b], ns)) - p64) / p64
                bar = max(4 * ref_err, 4 * ULP)
                err = abs(float(got[b]) - p64) / p64
                if err / bar >= worst[2] / max(worst[1], 1e-300):
                    worst = (ref_err, bar, err)
                assert np.isfinite(got[b]) and err <= bar, (kinds[b], ns, got[b], p64, ref_err, err, bar)
                if kinds[b] == "equal":
                    assert abs(got[b] * V - 1.0) <= 4 * ULP
    _report(f"no_speech V{V} r0 {r0} (relative error of the probability, the case nearest its bar)", *worst)


def test_no_speech_refuses_a_token_outside_the_vocabulary(lib):
    from wis_hip._lib import DevBuf
    V = 51865
    d_l, d_o = DevBuf(4 * 51872 * 4), DevBuf(16)
    for ns in (-1, V, V + 3):
        assert lib.wis_op_no_speech(0, d_l.ptr, 51872, 1, 4, 0, V, ns, d_o.ptr) == WIS_E_ARG


# ---- lang_probs ---------------------------------------------------------------------------------------------------------------------------
def _lang_probs_f32(row, ids):
    """lang_probs_kernel in numpy fp32: lane l takes ids l, l + 64, ..; wave maximum; wave sum of __expf; __expf / sum"""
    n = len(ids)
    v = row[ids]
    mx = v.max()
    e = _fast_exp(np.concatenate([v, np.full((-n) % 64, -np.inf, np.float32)]).reshape(-1, 64) - mx)
    s = _tree(np.add.reduce(e, axis=0, dtype=np.float32))
    return (_fast_exp(v - mx) / s).astype(np.float32)


@pytest.mark.parametrize("B", [1, 5])
@pytest.mark.parametrize("n_lang", [1, 63, 64, 65, 99, 100])
def test_lang_probs_against_float64(lib, n_lang, B):
    from wis_hip._lib import DevBuf, check
    V = 51866
    ld = (V + 31) // 32 * 32
    rng = np.random.default_rng([n_lang, B])
    ids = np.concatenate([[0, V - 1], rng.choice(np.arange(1, V - 1), size=n_lang, replace=False)])[:n_lang] if n_lang > 1 else np.array([V - 1])
    ids = _i32(ids[rng.permutation(n_lang)])                          # scattered over the row, ids 0 and V - 1 among them, in no order
    x, kinds = _extreme_rows(rng, B, n_lang)
    buf = (3.0 * rng.standard_normal((B, ld)) + 90.0).astype(np.float32)      # every other column of the row is larger than the listed ones
    for b in range(B):
        buf[b, ids] = x[b]
    d_l, d_i, d_p = DevBuf.from_numpy(buf), DevBuf.from_numpy(ids), DevBuf.from_numpy(np.full(B * n_lang + 8, -1.0, np.float32))
    check(lib.wis_op_lang_probs(0, d_l.ptr, ld, d_i.ptr, n_lang, d_p.ptr, B))
    out = d_p.to_numpy(np.float32, (B * n_lang + 8,))
    assert (out[B * n_lang:] == -1.0).all()
    got = out[:B * n_lang].reshape(B, n_lang)
    worst = (0.0, 0.0, 0.0)
    for b in range(B):
        p64 = _softmax64(x[b])
        p32 = _lang_probs_f32(buf[b], ids)
        # error of the probability vector in units of its largest entry (entries below ~1e-38 of it have no fp32 representation to speak of), and
        # the relative error of every entry the fast exponential can still represent as a normal number
        big = p64 >= 1e-36
        ref_err = max(np.abs(p32 - p64).max() / p64.max(), (np.abs(p32 - p64)[big] / p64[big]).max())
        err = max(np.abs(got[b] - p64).max() / p64.max(), (np.abs(got[b] - p64)[big] / p64[big]).max())
        bar = max(4 * ref_err, 4 * ULP)
        if err / bar >= worst[2] / max(worst[1], 1e-300):
            worst = (ref_err, bar, err)
        assert np.isfinite(got[b]).all() and err <= bar, (kinds[b], ref_err, err, bar)
        assert abs(float(got[b].astype(np.float64).sum()) - 1.0) <= bar, (kinds[b], got[b].sum(), bar)
        if kinds[b] == "equal":
            assert np.abs(got[b] * n_lang - 1.0).max() <= 4 * ULP
    _report(f"lang_probs n_lang {n_lang} B{B} (the row nearest its bar)", *worst)


# ---- greedy rows: logit_stats_kernel + greedy_pick_kernel ----------------------------------------------------------------------------------
def _greedy_f32(x32, V):
    """logit_stats_kernel + greedy_pick_kernel in numpy fp32 on the masked row x32: 64 sub-chunks of SL = ceil(V / 64) ids; in a sub-chunk lane l holds
    ids lo + l + 64 i (i < 16), its maximum, the lane's sum of __expf(v - max) over i, a wave sum; then M = max of the maxima, S = wave sum of
    sum x __expf(max - M), lse = M + log(S); the pick is the best (value - lse, lower id first) of the sub-chunks' winners"""
    SL = -(-V // 64)
    lo = np.arange(64)[:, None, None] * SL
    idx = lo + np.arange(64)[None, None, :] + 64 * np.arange(16)[None, :, None]               # [sub][i][lane]
    ok = (idx < np.minimum(lo + SL, V)) & (np.arange(16)[None, :, None] * 64 + np.arange(64)[None, None, :] < SL)
    vals = np.where(ok, x32[np.minimum(idx, V - 1)], np.float32(-np.inf)).astype(np.float32)
    smx = vals.reshape(64, -1).max(axis=1)
    with np.errstate(invalid="ignore"):
        e = np.where(np.isfinite(smx)[:, None, None], _fast_exp(vals - smx[:, None, None]), np.float32(0))
    ssm = _tree(np.add.reduce(e, axis=1, dtype=np.float32))
    M = smx.max()
    S = _tree(np.where(np.isfinite(smx), ssm * _fast_exp(smx - M), np.float32(0)).astype(np.float32))
    lse = np.float32(M + np.log(S, dtype=np.float32))
    tok = int(np.flatnonzero(x32 == M)[0])
    return tok, np.float32(M - lse)


def _greedy_inputs(rng, n_rows, V, pad):
    """logits f32 [n_rows][pad]: N(0, 2^2) with a clear maximum (+14) per row where picks go wrong: id 0, id V - 1, both sides of a sub-chunk boundary,
    two equal maxima in different sub-chunks (the lower id wins), a suppressed id above the maximum (masked), EOT / 220 above it (masked at step 0 only)"""
    SL = -(-V // 64)
    x = (2.0 * rng.standard_normal((n_rows, pad))).astype(np.float32)
    x[:, V:] = np.float32(1e4)                                        # padding columns: never read
    for r in range(n_rows):
        c = int(rng.integers(1, 64)) * SL
        kind = r % 7
        if kind == 0: x[r, 0] = 14.0
        elif kind == 1: x[r, V - 1] = 14.0
        elif kind == 2: x[r, c - 1] = 14.0; x[r, c] = 13.5
        elif kind == 3: x[r, c] = 14.0; x[r, c - 1] = 13.5
        elif kind == 4:
            a, b = sorted(rng.choice(64, size=2, replace=False).tolist())
            x[r, a * SL + 700] = 14.0; x[r, b * SL + 3] = 14.0        # equal maxima, the lower id in the HIGHER lane
        elif kind == 5: x[r, 50258] = 20.0; x[r, int(rng.integers(1000, 50000)) | 1024] = 14.0      # <|startoftranscript|> is suppressed
        else: x[r, EOT] = 16.0; x[r, 220] = 15.0; x[r, 30000 + r] = 14.0
    return x


def _run_greedy(lib, logits, V, pad, bias_all, bias_begin, step_u, B, beam, lr_b, lr_j, lr_off, rowmap):
    from wis_hip._lib import DevBuf, check
    n = B * beam
    d_l, d_bb, d_s = DevBuf.from_numpy(logits), DevBuf.from_numpy(bias_begin), DevBuf.from_numpy(_i32(step_u))
    d_ba = DevBuf.from_numpy(bias_all) if bias_all is not None else None
    d_rm = DevBuf.from_numpy(_i32(rowmap)) if rowmap is not None else None
    d_t, d_p = DevBuf.from_numpy(np.full(n + 4, -7, np.int32)), DevBuf.from_numpy(np.full(n + 4, -7.0, np.float32))
    check(lib.wis_op_greedy_rows(0, d_l.ptr, V, pad, EOT, d_ba.ptr if d_ba else None, d_bb.ptr, d_s.ptr, B, beam, lr_b, lr_j, lr_off,
                                 d_rm.ptr if d_rm else None, d_t.ptr, d_p.ptr))
    tok, lp = d_t.to_numpy(np.int32, (n + 4,)), d_p.to_numpy(np.float32, (n + 4,))
    assert (tok[n:] == -7).all() and (lp[n:] == -7.0).all()
    return tok[:n], lp[:n]


# (rows, form): "tf" = the teacher-forced rows of a draft verification, row b reads logits row b + f at its own step; "map" = B x beam rows,
# row (b, j) reads logits row b * beam + rowmap[j] + 2 (the replay of a verified beam window), steps per utterance
@pytest.mark.parametrize("V", [51865, 51866])
@pytest.mark.parametrize("rows,form,f", [(1, "tf", 0), (7, "tf", 3), (40, "tf", 0), (40, "tf", 3), (1, "map", 0), (7, "map", 0), (40, "map", 0)])
@pytest.mark.parametrize("with_bias_all", [False, True])
def test_greedy_rows_against_float64(lib, V, rows, form, f, with_bias_all):
    from wis_hip import weights as W
    pad = (V + 31) // 32 * 32
    rng = np.random.default_rng([V, rows, f, int(with_bias_all), form == "map"])
    sup = W.SUPPRESS_IDS if V == W.N_VOCAB else W.special_tokens(V).default_suppress_ids()
    bias_all = None
    if with_bias_all:
        bias_all = np.zeros(pad, np.float32); bias_all[sup] = -np.inf
        bias_all[[5, 4000, V - 3]] = [-2.5, 0.75, -1.125]            # (finite entries are added like any other)
    bias_begin = np.zeros(pad, np.float32); bias_begin[[220, EOT]] = -np.inf
    if form == "tf":
        B, beam, lr_b, lr_j, lr_off, rowmap = rows, 1, 1, 0, f, None
        n_log = rows + f + 1
        step_u = [0 if b % 3 == 0 else int(rng.integers(1, 30)) for b in range(B)]
        src = [b + f for b in range(rows)]
    else:
        B, beam = {1: (1, 1), 7: (1, 7), 40: (5, 8)}[rows]
        lr_b, lr_j, lr_off, rowmap = beam, 1, 2, rng.permutation(beam)
        n_log = rows + 3
        step_u = [0 if b % 2 == 0 else int(rng.integers(1, 30)) for b in range(B)]
        src = [b * beam + int(rowmap[j]) + 2 for b in range(B) for j in range(beam)]
    logits = _greedy_inputs(rng, n_log, V, pad)
    tok, lp = _run_greedy(lib, logits, V, pad, bias_all, bias_begin, step_u, B, beam, lr_b, lr_j, lr_off, rowmap)
    worst = (0.0, 0.0, 0.0)
    for m in range(rows):
        first = step_u[m // beam] == 0
        raw = logits[src[m], :V]
        x32 = raw + bias_all[:V] if with_bias_all else raw.copy()
        x32 = (x32 + bias_begin[:V]).astype(np.float32) if first else x32.astype(np.float32)
        x64 = raw.astype(np.float64) + (bias_all[:V] if with_bias_all else 0.0) + (bias_begin[:V] if first else 0.0)
        mx = x64.max()
        lse64 = mx + np.log(np.exp(x64 - mx).sum())
        tok64 = int(np.flatnonzero(x64 == mx)[0])                    # the lowest id among equal maxima
        lp64 = mx - lse64
        tok32, lp32 = _greedy_f32(x32, V)
        assert tok32 == tok64
        ref_err = abs(float(lp32) - lp64)
        # floor: lp = v - lse is a difference of fp32 numbers of the size of the logit, so a few ulps of THAT size (and of lp itself)
        bar = max(4 * ref_err, 4 * float(np.spacing(np.float32(max(abs(mx), abs(lse64), abs(lp64))))))
        err = abs(float(lp[m]) - lp64)
        if err / bar >= worst[2] / max(worst[1], 1e-300):
            worst = (ref_err, bar, err)
        assert tok[m] == tok64, (m, src[m], step_u[m // beam], int(tok[m]), tok64)
        assert err <= bar, (m, float(lp[m]), lp64, ref_err, err, bar)
    _report(f"greedy rows V{V} {rows} rows {form} f{f} bias_all {with_bias_all} (absolute error of the log-probability, the row nearest its bar)", *worst)
