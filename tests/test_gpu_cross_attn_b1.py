"""-m gpu: the one-utterance decode step's cross-attention launch (csrc/dec_kernels.hip, launch_dec_cross_attn: granule form, `small` grid) through
wis_op_dec_cross_attn_stat, against the float64 reference and the bound of tests/dec_attn_ref.py with the factor tests/test_gpu_dec_attn_edges.py uses for
these kernels (its _cross_case is the case runner here: every written element within the bound and finite, three launches of a call and repeated calls
agree to the bit, nothing written behind the rows, poisoned padding never reaches the output, the fragment-image form holds the same bits).

Routes.  At d = 1280 (H = 20) a `small` granule-form call runs dec_cross_attn_b1_kernel, the kernel of its own of the large models' one-utterance step; at
every other width (H = 6, d = 384; H = 12, d = 768) it runs dec_cross_attn_rs_kernel<SPIN, NT, 2>.  B = 2 moves the combiner (the last chunk's workgroup
of each head) to other places of the grid and keeps the grid small (2 x 20 x 6 = 240 workgroups <= 256).

No test can see which kernel ran: test_patterns_reached only restates the launch's conditions through tests/test_gpu_dec_attn_edges.py's cross_kernel, which
names the rs instantiation of those conditions (for H = 20 too, where the launch goes on to dec_cross_attn_b1_kernel); the route itself is shown by the kernel
trace in profiles/cross_attn_b1_ab.md, section 5.  WIS_CA_RS=0 or WIS_CA_SPIN=0 in the environment move every case here off the new kernel without a word.

Shapes.  T = 512 (two full 256-key chunks), T = 449 (two chunks, 193 keys in the last) and T = 1500 (six chunks, 220 keys in the last) with R in
{1, 5, 8}.  T = 257 in two 256-key chunks - one key in the last - is NOT in the grid: launch_dec_cross_attn derives the chunk length from T and the chunk
count (257 keys in 2 chunks are 160-key chunks, which it rejects; no chunk count gives 256), so no caller can reach that shape - test_t257_is_rejected
holds the library to that - and T = 449 is the shortest two-chunk sequence the 256-key form takes.  The heads of a call run the score patterns of
dec_attn_ref.CROSS_PATTERNS in turn; at H = 20 these include `flat` (a row whose scores are all equal: q = 0) and `one` (one key 600 above all others: every
other exponential underflows in f32), and test_patterns_reached says so.  test_one_key_dominates_by_60 has inputs of its own: one key about 60 above the
rest, where e^-60 is an ordinary f32 number whose f16 P is 0, in the first, a middle and the ragged last chunk.  test_kv_shared runs the new kernel's
kv_shared bit (both row groups read utterance 0's K / V, which differ from utterance 1's in memory).

test_b1_equals_rs_word_for_word compares the two kernels word for word: the same per-head problems (queries, K, V, column sums, bias) in heads 0-11 of an
H = 12 call (d = 768: dec_cross_attn_rs_kernel<SPIN, NT, 2>) and of an H = 20 call (d = 1280: dec_cross_attn_b1_kernel), with row partials that give both
widths the same LayerNorm statistics exactly (every 16-column tile: sum 0, M2 4 -> mean 0, variance 0.25 at either width: 768 x 0.25 x fl(1 / 768) and
1280 x 0.25 x fl(1 / 1280) both round to 0.25), so the folded query of a head is the same f16 words in both calls and so must the output be."""
import numpy as np
import pytest

import dec_attn_ref as D
import test_gpu_dec_attn_edges as E

pytestmark = pytest.mark.gpu

SHAPES = [(512, 2), (449, 2), (1500, 6)]      # (T, chunks): 256-key chunks each


def test_patterns_reached():
    first20 = D.CROSS_PATTERNS[:20]
    assert "flat" in first20 and "one" in first20
    for T, chunks in SHAPES:
        for H, name in ((20, "dec_cross_attn_rs_kernel<SPIN, NT, 2>"), (6, "dec_cross_attn_rs_kernel<SPIN, NT, 2>")):
            for B in (1, 2):
                # (cross_kernel names the rs instantiation whose conditions the launch takes; at d = 1280 that launch goes to dec_cross_attn_b1_kernel)
                assert E.cross_kernel("stat", B, 5, H, T, chunks) == (name, 256)


@pytest.mark.parametrize("B", [1, 2])
@pytest.mark.parametrize("H", [6, 20])
@pytest.mark.parametrize("R", [1, 5, 8])
@pytest.mark.parametrize("T,chunks", SHAPES)
def test_cross_attn_b1_edges(lib, T, chunks, R, H, B):
    E._cross_case(lib, "stat", B, R, H, T, chunks)


@pytest.mark.parametrize("R", [1, 5])
@pytest.mark.parametrize("T,chunks", [(512, 2), (449, 2)])
def test_b1_equals_rs_word_for_word(lib, T, chunks, R):
    from wis_hip._lib import DevBuf, check
    rng = np.random.default_rng([T, R, 77])
    Tpad = D.cdiv(T, 64) * 64
    outs = {}
    H0 = 12
    q = rng.standard_normal((R, 64 * 20)).astype(np.float32)
    K = (rng.standard_normal((1, T, 64 * 20)) * 0.5).astype(np.float16)
    V = rng.standard_normal((1, T, 64 * 20)).astype(np.float16)
    qcs = rng.standard_normal(64 * 20).astype(np.float32)
    qb = (rng.standard_normal(64 * 20) * 0.25).astype(np.float32)
    for H in (H0, 20):      # H = 12: dec_cross_attn_rs_kernel<SPIN, NT, 2>; H = 20: dec_cross_attn_b1_kernel
        d = 64 * H
        stat = np.zeros((R, d // 16, 2), np.float32)
        stat[..., 1] = 4.0
        host = [q[:, :d], None, stat, qcs[:d], qb[:d]]
        bufs = [None if a is None else DevBuf.from_numpy(np.ascontiguousarray(a, np.float32)) for a in host]
        kx = DevBuf.from_numpy(E._guarded(D.k_image(K[:, :, :d]), 0))
        vt = DevBuf.from_numpy(E._guarded(D.vt_image(V[:, :, :d], Tpad, 0), 0))
        runs = []
        for _ in range(2):
            o = E._Out(R, d, 0)
            check(lib.wis_op_dec_cross_attn_stat(0, *[b.ptr if b else None for b in bufs], kx.ptr, vt.ptr, o.buf.ptr, 1, R, H, T, chunks, 0, 0, 0))
            runs.append(o.rows())
        for b in bufs + [kx, vt]:
            if b:
                b.free()
        assert E._same(runs[0], runs[1]), f"H = {H}: two calls differ"
        assert np.isfinite(runs[0].astype(np.float64)).all()
        outs[H] = runs[0]
    assert E._same(outs[H0], outs[20][:, :64 * H0]), "dec_cross_attn_b1_kernel and dec_cross_attn_rs_kernel<SPIN, NT, 2> differ in heads 0-11"


@pytest.mark.parametrize("T,chunks", [(1500, 6), (449, 2)])
def test_kv_shared(lib, T, chunks):
    """B = 2, H = 20 (dec_cross_attn_b1_kernel: kv_shared travels in bit 7 of its packed shape argument); H = 6 the rs kernel's flag beside it"""
    E._cross_case(lib, "stat", 2, 5, 20, T, chunks, kv_shared=1)
    E._cross_case(lib, "stat", 2, 5, 6, T, chunks, kv_shared=1)


def test_t257_is_rejected(lib):
    """257 keys in 2 chunks: 160-key chunks, which launch_dec_cross_attn does not run (and no chunk count makes them 256)"""
    from wis_hip._lib import DevBuf
    B, R, H, T, chunks = 1, 5, 6, 257, 2
    assert D.cdiv(D.cdiv(T, chunks), 32) * 32 == 160 and all(D.cdiv(D.cdiv(T, c), 32) * 32 != 256 for c in range(1, 17))
    d, Tpad = 64 * H, D.cdiv(T, 64) * 64
    rng = np.random.default_rng(257)
    q16 = rng.standard_normal((R, d)).astype(np.float16).astype(np.float32)
    ops = D.fold_operands(q16, rng, None)
    K = rng.standard_normal((B, T, d)).astype(np.float16)
    bufs = [DevBuf.from_numpy(np.ascontiguousarray(ops[k], np.float32)) for k in ("q_one", "stat", "qcs", "qb")]
    kx, vt = DevBuf.from_numpy(E._guarded(D.k_image(K), 0)), DevBuf.from_numpy(E._guarded(D.vt_image(K, Tpad, 0), 0))
    o = E._Out(R, d, 0)
    rc = lib.wis_op_dec_cross_attn_stat(0, bufs[0].ptr, None, bufs[1].ptr, bufs[2].ptr, bufs[3].ptr, kx.ptr, vt.ptr, o.buf.ptr, B, R, H, T, chunks, 0, 0, 0)
    rows = o.rows()
    for b in bufs + [kx, vt]:
        b.free()
    assert rc != 0, "257 keys in 2 chunks accepted"
    assert (E._bits(rows) == D.PAT16).all(), "a rejected call wrote output"


@pytest.mark.parametrize("B", [1, 2])
def test_one_key_dominates_by_60(lib, B):
    """every (utterance, head): key t* scores 60 +- 2 above every other key (q . k = 8 x 7.5 there, |noise| small elsewhere); t* runs through the first key,
    the K waves' seam (127 | 128), a middle chunk and the last key of the ragged last chunk.  Bound and factor as in every case of these files."""
    from wis_hip._lib import DevBuf, check
    R, H, T, chunks, CL = 5, 20, 1500, 6, 256
    d, M, Tpad = 64 * H, B * R, D.cdiv(T, 64) * 64
    rng = np.random.default_rng([60, B])
    places = [0, 127, 128, 255, 256, 700, 1279, 1280, 1499]
    q16 = (rng.integers(1, 5, (M, d)) * rng.choice([-1, 1], (M, d)) / 32.0).astype(np.float32)      # (no exact zeros: the fold cannot produce one)
    K = (rng.integers(-4, 5, (B, T, d)) / 32.0).astype(np.float16)
    V = rng.standard_normal((B, T, d)).astype(np.float16)
    want = []
    for b in range(B):
        for h in range(H):
            sl = slice(64 * h, 64 * h + 64)
            ts = places[(h + 3 * b) % len(places)]
            q16[b * R:b * R + R, 64 * h] = 8.0
            K[b, :, 64 * h] = 0.0
            K[b, ts, 64 * h] = 7.5
            q, k, v = q16[b * R:b * R + R, sl], K[b, :, sl], V[b, :, sl]
            s = q.astype(np.float64) @ k.astype(np.float64).T
            gap = s[:, ts] - np.delete(s, ts, axis=1).max(1)
            assert (gap > 58).all() and (gap < 62).all(), (gap.min(), gap.max())
            want.append((slice(b * R, b * R + R), sl) + D.reference(q, k, v, D.n_acc_cross(T, CL), chunk=CL))
    ops = D.fold_operands(q16, rng, None)
    D.fold_query_check(q16, ops, from_rows=False)
    bufs = [DevBuf.from_numpy(np.ascontiguousarray(ops[k], np.float32)) for k in ("q_one", "stat", "qcs", "qb")]
    kx, vt = DevBuf.from_numpy(E._guarded(D.k_image(K), 0)), DevBuf.from_numpy(E._guarded(D.vt_image(V, Tpad, 0), 0))
    runs = []
    for _ in range(2):
        o = E._Out(M, d, 0)
        check(lib.wis_op_dec_cross_attn_stat(0, bufs[0].ptr, None, bufs[1].ptr, bufs[2].ptr, bufs[3].ptr, kx.ptr, vt.ptr, o.buf.ptr, B, R, H, T, chunks, 0, 0, 0))
        runs.append(o.rows())
    for b in bufs + [kx, vt]:
        b.free()
    assert E._same(runs[0], runs[1]), "two calls differ"
    worst = 0.0
    for rows, sl, ref, unit in want:
        out = runs[0][rows, sl]
        assert np.isfinite(out.astype(np.float64)).all()
        worst = max(worst, float(np.nan_to_num(D.ratios(out, ref, unit), nan=np.inf).max()))
    print(f"\nEDGES|cross|dec_cross_attn_b1_kernel|gap60|stat B{B} R{R} H{H} T{T}/{chunks}|{worst:.4f}")
    assert worst <= E.FACTOR, worst
