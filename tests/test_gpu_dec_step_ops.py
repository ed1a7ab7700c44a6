"""-m gpu: op-level parity of the kernels the DECODE STEP launches, in the forms it launches them, against float64 numpy on exactly the
values the kernels read (f16 arrays cast up, fp32 inputs as given).  The taps (include/wis_hip.h: wis_op_dec_cross_attn_stat,
wis_op_dec_self_attn_ex, wis_op_gemv_qkv, wis_op_gemv_out_cq) add arguments and the loader's preparation only; which instantiation runs is
decided by the product's launch_* functions (dec_kernels.hip), so every case below names the kernel those rules give it:

  cross-attention, query folded from row partials (launch_dec_cross_attn, xres_is_stat = 1; T = 1500 in 6 chunks of 256 keys unless noted)
    H  6, B 1              dec_cross_attn_rs_kernel<SPIN, NT, 2>       36 workgroups: "small" (<= 256), granule hand-off
    H  6, B 1, no_spin     dec_cross_attn_rs_kernel<-, NT, 2>          the ticket form of the same grid
    H  6, B 8              dec_cross_attn_rs_kernel<SPIN, -, 2>        288 workgroups: not small
    H  6, B 8, no_spin     dec_cross_attn_rs_kernel<-, -, 2>
    H 20, B 1              rs<SPIN, NT>                                the headline grid, 120 workgroups
    H 20, B 8              rs<SPIN, ->                                 960 workgroups
    H 16, B 3              rs<SPIN, ->                                 d = 1024
    H 20, B 10             rs<-, ->                                    B H = 200 > CA_SPIN_MAX_BH = 192: no granule buffers, the ticket form
    H 32, B 1              dec_cross_attn_kernel<4, 6, FOLD 3, SPIN>   d = 2048 > the rs kernel's 1280; 192 workgroups: small, V up front
    H 32, B 2              dec_cross_attn_kernel<4, 6, FOLD 4, SPIN>   384 workgroups: the operands staged through LDS
    H 20, B 1, 12 chunks   dec_cross_attn_kernel<2, 16, FOLD 2, ->     128-key chunks: neither the rs kernel nor the hand-off
    the H = 6 grids also at T = 1536 (no ragged chunk) and 449 in 2 chunks; T = 1345 in 6 chunks (a last chunk of 65 keys) is UNSUPPORTED by design:
    V^T is read unconditionally up to chunks x 256 keys, so launch_dec_cross_attn asks for chunks x 256 <= Tpad = T rounded up to 64, which
    leaves every last chunk more than 192 keys - the test asserts that answer
  cross-attention, plain form at R = 16 (the > 8-rows batched route and draft verification): dec_cross_attn_kernel<4, 6, FOLD 0, ->, kv_shared 0 / 1
  self-attention: dec_self_attn_kernel<false, 2 | 4 | 8> at the history lengths StepGraph::nb_for (generate.hip) gives each, both sides of every
    boundary, plus one length past the first pass of the two short forms (the kernel's contract: any nb is right for any length);
    dec_self_attn_kernel<true, 8> by ancestor table
  QKV projection with the scatter epilogue (GV_LN | GV_QKV): gemv_kernel<1, 1, SC, RM> at M <= 8 (launch_gemv), gemv_frag_kernel above (launch_gemv_frag)
  fused out-projection + cross-Q: gemv_dual_kernel<3, 6 | 4, 8 | 6, 12 | 8, 16 | 10, 20> (d = 384 .. 1280) at M <= 8, gemv_frag3_kernel above

Every bound is one the suite already has (test_gpu_dec_attn.py, test_gpu_ops.py test_gemv) or is derived where it is used."""
import functools

import numpy as np
import pytest

from test_gpu_dec_attn import _cross_layouts, _softmax

pytestmark = pytest.mark.gpu

F = np.float64
WIS_E_UNSUPPORTED = -7      # include/wis_hip.h


def xf_index(m, k, MB):
    """kernels.hpp xf_index: element (row m, column k) of an activation fragment image of MB 16-row blocks."""
    m, k = np.asarray(m, np.int64), np.asarray(k, np.int64)
    return (((k >> 5) * MB + (m >> 4)) * 64 + (m & 15) + 16 * ((k >> 3) & 3)) * 8 + (k & 7)


def _from_xf(img, M, d, MB):
    """rows [M][d] out of a fragment image; everything else in the image must still be the tap's zero fill."""
    idx = xf_index(np.arange(M)[:, None], np.arange(d)[None, :], MB)
    rest = np.ones(img.size, bool)
    rest[idx.reshape(-1)] = False
    assert not img[rest].view(np.uint16).any(), "a store outside the rows' places in the fragment image"
    return img[idx]


def _relerr(a, b):
    a, b = np.asarray(a, F), np.asarray(b, F)
    return float(np.linalg.norm(a - b) / (np.linalg.norm(b) + 1e-30))


def _partials(x):
    """per-16-column (sum x, sum (x - tile mean)^2) of fp32 rows, computed in float64 and stored as fp32 [M][d/16][2]."""
    t = x.astype(F).reshape(x.shape[0], -1, 16)
    s = t.sum(-1)
    m2 = ((t - s[..., None] / 16) ** 2).sum(-1)
    return np.stack([s, m2], -1)


def _merge(stat):
    """mean / rstd of the rows from fp32 partials, merged in float64."""
    s, m2 = stat[..., 0].astype(F), stat[..., 1].astype(F)
    d = 16 * s.shape[1]
    mu = s.sum(1, keepdims=True) / d
    var = (m2 + 16 * (s / 16 - mu) ** 2).sum(1, keepdims=True) / d
    return mu, 1.0 / np.sqrt(var + 1e-5)


@functools.lru_cache(maxsize=2)
def _kv(H, B, T):
    """K / V of B utterances (every utterance different), natural f16 [B][T][d] + the kernel's layouts on the device; shared by the cases of a grid."""
    from wis_hip import _lib
    d, Tpad = 64 * H, (T + 63) // 64 * 64
    rng = np.random.default_rng(1000 * H + 10 * B + T)
    K = (rng.standard_normal((B, T, d), dtype=np.float32) * 0.6).astype(np.float16)
    V = rng.standard_normal((B, T, d), dtype=np.float32).astype(np.float16)
    for b in range(B):      # a few dominant keys per (utterance, head): the chunk maxima differ by a lot (the partial combine)
        for h in range(H):
            K[b, (37 * h + 411 * b) % T, 64 * h:64 * h + 64] *= 4
    kx, vt = _cross_layouts(K, V, T, Tpad)
    return K, V, _lib.DevBuf.from_numpy(kx), _lib.DevBuf.from_numpy(vt)


def _attend(q, K, V, B, R, shared=False):
    """softmax(q K^T) V per (utterance, head) in float64; shared: every row group reads utterance 0."""
    d = q.shape[1]
    exp = np.zeros((B * R, d))
    for b in range(B):
        kb = 0 if shared else b
        for h in range(d // 64):
            sl = slice(64 * h, 64 * h + 64)
            s = q[b * R:(b + 1) * R, sl] @ K[kb, :, sl].astype(F).T
            exp[b * R:(b + 1) * R, sl] = _softmax(s) @ V[kb, :, sl].astype(F)
    return exp


def _cross_call(lib, q, q2, stat, qcs, qb, d_kx, d_vt, B, R, H, T, chunks, out_mb, kv_shared, no_spin):
    """three calls (nine launches on fresh tickets / epochs each): bit-identical; returns the rows as float64 [B*R][d]."""
    from wis_hip import _lib
    d, M = 64 * H, B * R
    bufs = [None if a is None else _lib.DevBuf.from_numpy(a) for a in (q, q2, stat, qcs, qb)]
    n = (d // 32) * out_mb * 64 * 8 if out_mb else M * d
    d_out = _lib.DevBuf.from_numpy(np.full(n, 77.0, np.float16))
    outs = []
    for rep in range(3):
        _lib.check(lib.wis_op_dec_cross_attn_stat(0, *[b.ptr if b else None for b in bufs], d_kx.ptr, d_vt.ptr, d_out.ptr, B, R, H, T, chunks, out_mb, kv_shared, no_spin))
        outs.append(d_out.to_numpy(np.float16, (n,)))
    assert np.array_equal(outs[0].view(np.uint16), outs[1].view(np.uint16)) and np.array_equal(outs[1].view(np.uint16), outs[2].view(np.uint16))
    rows = _from_xf(outs[0], M, d, out_mb) if out_mb else outs[0].reshape(M, d)
    return rows.astype(F)


def _cross_stat_case(lib, H, B, R, T, chunks, no_spin, offset=0.0):
    d, M = 64 * H, B * R
    K, V, d_kx, d_vt = _kv(H, B, T)
    rng = np.random.default_rng(17 * H + 5 * B + R + T + chunks + int(offset))
    if offset:      # multiples of 1/4: the partials below are exact in fp32, so the merge alone is tested
        x = (offset + rng.integers(-16, 17, size=(M, d)) / 4.0).astype(np.float32)
        x[:, ::5] += 6.0
    else:
        x = (rng.standard_normal((M, d)) * 2.4 + 0.7).astype(np.float32)
    stat = _partials(x).astype(np.float32)
    if offset:
        assert np.array_equal(stat.astype(F), _partials(x))
    mu, rs = _merge(stat)
    qcs = rng.standard_normal(d).astype(np.float32)
    qb = (0.1 * rng.standard_normal(d)).astype(np.float32)
    q_want = rng.standard_normal((M, d)) * 0.5
    q_raw = (q_want - qb) / rs + mu * qcs
    # one half alone (the dual launch leaves all of q_raw in q), and two halves of comparable size (the batched fold)
    q_one = q_raw.astype(np.float32)
    q_a = (0.5 * q_raw + q_raw.std() * rng.standard_normal((M, d))).astype(np.float32)
    q_b = (q_raw - q_a.astype(F)).astype(np.float32)
    worst = 0.0
    if (T, chunks) == (1345, 6):      # six 256-key chunks reach past Tpad = 1408 (this file's header): the launcher has to refuse, not read past V^T
        from wis_hip import _lib
        with pytest.raises(_lib.WisError) as e:
            _cross_call(lib, q_a, q_b, stat, qcs, qb, d_kx, d_vt, B, R, H, T, chunks, 0, 0, no_spin)
        assert e.value.code == WIS_E_UNSUPPORTED
        return worst
    for qa, q2 in ((q_one, None), (q_a, q_b)):
        qsum = qa.astype(F) + (q2.astype(F) if q2 is not None else 0.0)
        exp = _attend(rs * (qsum - mu * qcs.astype(F)) + qb.astype(F), K, V, B, R)
        for out_mb in (0, (M + 15) // 16):
            got = _cross_call(lib, qa, q2, stat, qcs, qb, d_kx, d_vt, B, R, H, T, chunks, out_mb, 0, no_spin)
            err = np.abs(got - exp).max()
            print(f"cross-attn from partials H={H} B={B} R={R} T={T}/{chunks} no_spin={no_spin} offset={offset} q2={q2 is not None} out_mb={out_mb}: max abs err {err:.2e}")
            worst = max(worst, err)
            # test_dec_cross_attn_folded_query_vs_fp64's bound, same reasoning: the plain tap's 3e-3 + the f16 cast of the finished query
            assert err <= 5e-3, (H, B, R, T, chunks, no_spin, offset, q2 is not None, out_mb, err)
    return worst


_RS = [1, 3, 5, 8]
_STAT_CASES = (
    [(6, B, R, T, ch, ns) for B in (1, 8) for (T, ch) in ((1500, 6), (1345, 6), (1536, 6), (449, 2)) for ns in (0, 1) for R in _RS]
    + [(20, B, R, 1500, 6, 0) for B in (1, 8) for R in _RS]
    + [(16, 3, 5, 1500, 6, 0), (20, 10, 5, 1500, 6, 0), (32, 1, 5, 1500, 6, 0), (32, 2, 5, 1500, 6, 0), (20, 1, 5, 1500, 12, 0)])


@pytest.mark.parametrize("H,B,R,T,chunks,no_spin", _STAT_CASES)
def test_cross_attn_from_partials_vs_fp64(H, B, R, T, chunks, no_spin, lib):
    """q = rs (q_raw [+ q2] - mu qcs) + qb with mu / rs merged from the row partials, then softmax(q K^T) V: every form the step launches
    (the table in this file's header), with one and with two halves of q_raw, row-major and into the fragment image."""
    _cross_stat_case(lib, H, B, R, T, chunks, no_spin)


@pytest.mark.parametrize("B", [1, 3])
def test_cross_attn_from_partials_rows_with_a_large_common_offset(B, lib):
    """rows at 1000 +- 2.4 (test_dec_cross_attn_folded_query_vs_fp64's rows, for the from-partials forms that ship): a merge that took
    sum(M2) + sum(16 m_t^2) - d mu^2 in fp32 would lose the variance; the kernels merge about the first tile's mean."""
    _cross_stat_case(lib, 20, B, 5, 1500, 6, 0, offset=1000.0)


@pytest.mark.parametrize("kv_shared", [0, 1])
@pytest.mark.parametrize("B", [2, 5])
def test_cross_attn_plain_16_rows_shared_kv_vs_fp64(B, kv_shared, lib):
    """R = 16 rows per group, finished query (FOLD 0, ticket form): the > 8-rows batched route (kv_shared 0) and draft verification (kv_shared 1:
    every group reads utterance 0's K / V - the groups b > 0 have DIFFERENT K / V in memory here, so a kernel that ignored the flag is caught)."""
    H, R, T = 20, 16, 1500
    d = 64 * H
    K, V, d_kx, d_vt = _kv(H, B, T)
    rng = np.random.default_rng(3 + B + kv_shared)
    q = (rng.standard_normal((B * R, d)) * 0.5).astype(np.float16).astype(np.float32)      # f16-representable: the kernel casts q
    exp = _attend(q.astype(F), K, V, B, R, shared=bool(kv_shared))
    for out_mb in (0, B):
        got = _cross_call(lib, q, None, None, None, None, d_kx, d_vt, B, R, H, T, 6, out_mb, kv_shared, 0)
        err = np.abs(got - exp).max()
        print(f"plain cross-attn R=16 B={B} kv_shared={kv_shared} out_mb={out_mb}: max abs err {err:.2e}")
        assert err <= 3e-3, (B, kv_shared, out_mb, err)      # test_dec_cross_attn_vs_fp64's bound


def test_cross_attn_unsupported_chunking_is_an_error(lib):
    """7 chunks of T = 1500 would be 224-key chunks: launch_dec_cross_attn has 128- and 256-key chunks only and must say so."""
    from wis_hip import _lib
    K, V, d_kx, d_vt = _kv(6, 1, 1500)
    q = np.zeros((5, 384), np.float32)
    with pytest.raises(_lib.WisError) as e:
        _cross_call(lib, q, None, None, None, None, d_kx, d_vt, 1, 5, 6, 1500, 7, 0, 0, 0)
    assert e.value.code == WIS_E_UNSUPPORTED


# ---------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=2)
def _cache(H, slots, ctx=448):
    from wis_hip import _lib
    rng = np.random.default_rng(100 * H + slots)
    kc = (rng.standard_normal((slots, ctx, 64 * H), dtype=np.float32) * 0.5).astype(np.float16)
    vc = rng.standard_normal((slots, ctx, 64 * H), dtype=np.float32).astype(np.float16)
    return kc, vc, _lib.DevBuf.from_numpy(kc), _lib.DevBuf.from_numpy(vc)


def _self_call(lib, q, pos, d_kc, d_vc, M, H, ctx, rpu, sstride, rmul, nb, out_mb, anc=None, w0=0, aw=0, base=None):
    from wis_hip import _lib
    d = 64 * H
    d_q, d_pos = _lib.DevBuf.from_numpy(q), _lib.DevBuf.from_numpy(pos)
    d_anc = _lib.DevBuf.from_numpy(anc) if anc is not None else None
    d_base = _lib.DevBuf.from_numpy(base) if base is not None else None
    n = (d // 32) * out_mb * 64 * 8 if out_mb else M * d
    d_out = _lib.DevBuf.from_numpy(np.full(n, 77.0, np.float16))
    _lib.check(lib.wis_op_dec_self_attn_ex(0, d_q.ptr, d_kc.ptr, d_vc.ptr, d_pos.ptr, d_out.ptr, M, H, ctx, rpu, sstride, rmul, nb, out_mb,
                                           d_anc.ptr if d_anc else None, w0, aw, d_base.ptr if d_base else None))
    img = d_out.to_numpy(np.float16, (n,))
    return (_from_xf(img, M, d, out_mb) if out_mb else img.reshape(M, d)).astype(F)


# (nb, history length): what StepGraph::nb_for assigns - 2 up to 16 cached positions, 4 up to 32, 8 beyond - on both sides of each boundary;
# (2, 17) and (4, 33): the second pass of the short forms' loop
_SELF_LENS = [(2, 1), (2, 15), (2, 16), (4, 17), (4, 31), (4, 32), (8, 33), (8, 64), (8, 65), (8, 447), (2, 17), (4, 33)]


@pytest.mark.parametrize("H", [20, 16])
@pytest.mark.parametrize("rows,rpu,sstride,rmul", [(1, 1, 1, 0), (5, 5, 5, 1), (16, 8, 8, 1), (4, 4, 5, 0)])
def test_self_attn_step_forms_vs_fp64(H, rows, rpu, sstride, rmul, lib):
    """test_dec_self_attn_vs_fp64's rows and reference for the forms it does not reach: nb = 2 / 4 and the fragment-image output."""
    d, ctx = 64 * H, 448
    kc, vc, d_kc, d_vc = _cache(H, 2 * max(sstride, rpu) + 2)
    rng = np.random.default_rng(200 * H + rows)
    for nb, hist in _SELF_LENS:
        q = (rng.standard_normal((rows, d)) * 0.4).astype(np.float32)
        if rmul:        # decode rows: every row in its own slot, lengths hist, hist - 1, hist - 2
            pos = np.array([max(0, hist - 1 - (r % 3)) for r in range(rows)], np.int32)
        else:           # prefill rows: the utterance's rows at consecutive positions ending at hist - 1, in its first slot
            pos = np.array([max(0, hist - rpu + (r % rpu)) for r in range(rows)], np.int32)
        exp = np.zeros((rows, d))
        for m in range(rows):
            ls = (m // rpu) * sstride + (m % rpu) * rmul
            n = int(pos[m]) + 1
            for h in range(H):
                sl = slice(64 * h, 64 * h + 64)
                s = kc[ls, :n, sl].astype(F) @ q[m, sl].astype(F)
                exp[m, sl] = _softmax(s[None])[0] @ vc[ls, :n, sl].astype(F)
        for out_mb in (0, (rows + 15) // 16):
            got = _self_call(lib, q, pos, d_kc, d_vc, rows, H, ctx, rpu, sstride, rmul, nb, out_mb)
            err = np.abs(got - exp).max()
            print(f"self-attn H={H} rows={rows} nb={nb} hist={hist} out_mb={out_mb}: max abs err {err:.2e}")
            assert err <= 2e-3, (H, rows, nb, hist, out_mb, err)      # test_dec_self_attn_vs_fp64's bound


@pytest.mark.parametrize("H", [6, 20])
@pytest.mark.parametrize("M", [16, 32])
def test_self_attn_tree_form_vs_fp64(H, M, lib):
    """The TREE form (dec_kernels.hip, the comment above dec_self_attn_kernel): the rows are nodes of a beam tree; row m's history is a path - positions
    < w0 in slot base[m] (no base table: in the slot of its window-step-0 ancestor, anc[m][0]), position w0 + t in slot anc[m][t], the slot of its
    ancestor at window step t.  A row at depth t sits at position w0 + t (its own K / V row is the last of its path); table entries behind a row's
    depth are never used and point at some other valid slot here."""
    d, ctx, slots = 64 * H, 448, 8
    kc, vc, d_kc, d_vc = _cache(H, slots)
    for aw in (1, 5, 32):
        for w0 in (3, 70):
            for with_base in (False, True):
                rng = np.random.default_rng(H + 7 * M + 31 * aw + w0 + with_base)
                per = max(1, M // aw)
                depth = np.minimum(np.arange(M) // per, aw - 1)
                own = rng.integers(0, slots, size=M)
                anc = rng.integers(0, slots, size=(M, aw)).astype(np.int32)
                for m in range(M):      # rows are in depth order: a parent's path is complete when its child copies it
                    t = int(depth[m])
                    if t:
                        parent = int(rng.choice(np.nonzero(depth == t - 1)[0]))
                        anc[m, :t] = anc[parent, :t]
                    anc[m, t] = own[m]
                base = rng.integers(0, slots, size=M).astype(np.int32) if with_base else None
                pos = (w0 + depth).astype(np.int32)
                q = (rng.standard_normal((M, d)) * 0.4).astype(np.float32)
                exp = np.zeros((M, d))
                for m in range(M):
                    n = int(pos[m]) + 1
                    sl_of = np.array([(base[m] if with_base else anc[m, 0]) if p < w0 else anc[m, p - w0] for p in range(n)])
                    kk, vv = kc[sl_of, np.arange(n)].astype(F), vc[sl_of, np.arange(n)].astype(F)
                    for h in range(H):
                        sl = slice(64 * h, 64 * h + 64)
                        exp[m, sl] = _softmax((kk[:, sl] @ q[m, sl].astype(F))[None])[0] @ vv[:, sl]
                for out_mb in (0, M // 16):
                    got = _self_call(lib, q, pos, d_kc, d_vc, M, H, ctx, 16, 0, 0, 8, out_mb, anc, w0, aw, base)
                    err = np.abs(got - exp).max()
                    print(f"tree self-attn H={H} M={M} aw={aw} w0={w0} base={with_base} out_mb={out_mb}: max abs err {err:.2e}")
                    assert err <= 2e-3, (H, M, aw, w0, with_base, out_mb, err)


# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [384, 1280])
@pytest.mark.parametrize("M", [1, 5, 8, 16, 40])
def test_gemv_qkv_scatter_vs_fp64(M, d, lib):
    """q, k, v = split(LN(x) W^T + b), q scaled by 1/8 (the loader folds 1/sqrt(64) into the query rows), in float64 on the folded matrix
    f16(W o gamma) as test_gemv_layernorm_rows_with_a_large_common_offset has it; k / v rows land at (slot[m], pos[m]) and NOTHING else of the caches changes."""
    from wis_hip._lib import DevBuf, check
    ctx = 448 if M <= 8 else 96
    rng = np.random.default_rng(13 * M + d)
    x = (rng.standard_normal((M, d)) * 2 + 0.3).astype(np.float32)
    W = (rng.standard_normal((3 * d, d)) * 0.05).astype(np.float16)
    bias = rng.standard_normal(3 * d).astype(np.float32)
    g = (1 + 0.1 * rng.standard_normal(d)).astype(np.float32); be = (0.1 * rng.standard_normal(d)).astype(np.float32)
    slot = (2 * rng.permutation(M) + 1).astype(np.int32)      # a permutation with gaps: the even slots stay untouched
    nslots = 2 * M + 2
    # distinct positions per row, the first and the last of the cache among them (one row: the last)
    pos = np.concatenate([[ctx - 1], [0], 1 + rng.permutation(ctx - 2)])[:M].astype(np.int32)
    rng.shuffle(pos)
    assert len(set(pos.tolist())) == M and pos.max() == ctx - 1 and (M == 1 or pos.min() == 0)
    x64 = x.astype(F)
    mu = x64.mean(1, keepdims=True); var = x64.var(1, keepdims=True)
    Wg = (W.astype(np.float32) * g).astype(np.float16).astype(F)
    ref = ((x64 - mu) / np.sqrt(var + 1e-5)) @ Wg.T + W.astype(F) @ be.astype(F) + bias
    ref[:, :d] *= 0.125
    sent_k = (np.arange(nslots * ctx * d, dtype=np.uint32) * 2654435761 >> 13).astype(np.uint16).reshape(nslots, ctx, d)
    sent_v = ~sent_k
    d_kc, d_vc = DevBuf.from_numpy(sent_k), DevBuf.from_numpy(sent_v)
    d_q = DevBuf.from_numpy(np.full((M, d), 77.0, np.float32))
    bufs = [DevBuf.from_numpy(a) for a in (x, g, be, W, bias, slot, pos)]
    check(lib.wis_op_gemv_qkv(0, *[b.ptr for b in bufs], d_q.ptr, d_kc.ptr, d_vc.ptr, M, d, ctx))
    q = d_q.to_numpy(np.float32, (M, d))
    gk, gv = d_kc.to_numpy(np.uint16, (nslots, ctx, d)), d_vc.to_numpy(np.uint16, (nslots, ctx, d))
    for name, got, want, tol in (("q", q, ref[:, :d], 1e-3), ("k", gk[slot, pos].view(np.float16), ref[:, d:2 * d], 2e-3), ("v", gv[slot, pos].view(np.float16), ref[:, 2 * d:], 2e-3)):
        e = _relerr(got, want)
        worst = float(np.abs(got.astype(F) - want).max())
        print(f"gemv QKV M{M} d{d} {name}: rel err {e:.3e} max abs {worst:.3e}")
        assert e < tol, (name, e)                                   # test_gemv: 1e-3 for f32, 2e-3 for f16 outputs
        assert worst < 0.05 * (1 + float(np.abs(want).max())), (name, worst)
    for name, got, sent in (("K", gk, sent_k), ("V", gv, sent_v)):
        got = got.copy()
        got[slot, pos] = sent[slot, pos]
        assert np.array_equal(got, sent), f"{name} cache changed outside the rows' (slot, pos)"


# ---------------------------------------------------------------------------------------
def _out_cq_inputs(M, d, exact):
    rng = np.random.default_rng(29 * M + d + exact)
    a = rng.standard_normal((M, d)).astype(np.float16)
    Wq = (rng.standard_normal((d, d)) * 0.05).astype(np.float16); bq = rng.standard_normal(d).astype(np.float32)
    g = (1 + 0.1 * rng.standard_normal(d)).astype(np.float32); be = (0.1 * rng.standard_normal(d)).astype(np.float32)
    if exact:       # x1 = x0: rows of multiples of 1/4 near 200 - every intermediate of the partials is representable in fp32
        x0 = (200.0 + rng.integers(-16, 17, size=(M, d)) / 4.0).astype(np.float32)
        x0[:, ::7] += 8.0
        Wo = np.zeros((d, d), np.float16); bo = np.zeros(d, np.float32)
    else:
        x0 = (rng.standard_normal((M, d)) * 2 + 0.3).astype(np.float32)
        Wo = (rng.standard_normal((d, d)) * 0.05).astype(np.float16); bo = rng.standard_normal(d).astype(np.float32)
    return a, x0, Wo, bo, Wq, bq, g, be


def _out_cq_case(lib, M, d, force_frag, exact):
    from wis_hip._lib import DevBuf, check
    a, x0, Wo, bo, Wq, bq, g, be = _out_cq_inputs(M, d, exact)
    frag = M > 8 or force_frag
    ins = [DevBuf.from_numpy(v) for v in (a, x0, Wo, bo, Wq, bq, g, be)]
    nt = d // 16
    outs = {k: DevBuf.from_numpy(np.full(n, 77.0, np.float32)) for k, n in (("x1", M * d), ("stat", M * nt * 2), ("q", M * d), ("q2", M * d), ("qcs", d), ("qb", d))}
    check(lib.wis_op_gemv_out_cq(0, *[b.ptr for b in ins], outs["x1"].ptr, outs["stat"].ptr, outs["q"].ptr, outs["q2"].ptr if frag else None,
                                 outs["qcs"].ptr, outs["qb"].ptr, M, d, int(force_frag)))
    x1 = outs["x1"].to_numpy(np.float32, (M, d)); stat = outs["stat"].to_numpy(np.float32, (M, nt, 2))
    q = outs["q"].to_numpy(np.float32, (M, d)); q2 = outs["q2"].to_numpy(np.float32, (M, d)) if frag else None
    qcs = outs["qcs"].to_numpy(np.float32, (d,)); qb = outs["qb"].to_numpy(np.float32, (d,))
    tag = f"out+cq M{M} d{d} {'frag3' if frag else 'dual'}{' exact' if exact else ''}"
    # x1 = x0 + a Wo^T + bo: test_gemv's bounds for an f32 output
    x1_ref = x0.astype(F) + a.astype(F) @ Wo.astype(F).T + bo
    e = _relerr(x1, x1_ref); worst = float(np.abs(x1 - x1_ref).max())
    print(f"{tag} x1: rel err {e:.3e} max abs {worst:.3e}")
    assert e < 1e-3 and worst < 0.05 * (1 + float(np.abs(x1_ref).max())), (e, worst)
    # the row partials against float64 partials of the kernel's OWN x1 (the partial arithmetic apart from the GEMM's error)
    pref = _partials(x1)
    ds = float(np.abs(stat[..., 0] - pref[..., 0]).max()); dm = np.abs(stat[..., 1] - pref[..., 1])
    print(f"{tag} partials: sums off by {ds:.3e}, M2 by {float((dm / pref[..., 1].max(1, keepdims=True)).max()):.3e} of the row's largest")
    if exact:
        assert np.array_equal(x1, x0) and np.array_equal(stat.astype(F), pref)
    else:
        assert ds <= 16 * 2.0 ** -23 * float(np.abs(x1).max())
        assert (dm <= 1e-5 * pref[..., 1].max(1, keepdims=True)).all()
    # the query, finished in float64 with the statistics of the REFERENCE x1, against LN(x1_ref) Wq^T + bq (times the folded 1/8)
    mu = x1_ref.mean(1, keepdims=True); rs = 1.0 / np.sqrt(x1_ref.var(1, keepdims=True) + 1e-5)
    q_ref = (((x1_ref - mu) * rs * g + be) @ Wq.astype(F).T + bq) * 0.125
    q_fin = rs * (q.astype(F) + (q2.astype(F) if frag else 0.0) - mu * qcs.astype(F)) + qb.astype(F)
    e = _relerr(q_fin, q_ref); worst = float(np.abs(q_fin - q_ref).max())
    print(f"{tag} q: rel err {e:.3e} max abs {worst:.3e}")
    if not exact:       # (rows at 200 +- 2.4: q_raw carries mu c ~ 200 |c| in fp32 - its own test is the chain below)
        assert e < 1e-3 and worst < 0.05 * (1 + float(np.abs(q_ref).max())), (e, worst)
    return x1_ref, q_ref, stat, q, q2, qcs, qb


@pytest.mark.parametrize("d", [384, 512, 768, 1024, 1280])
@pytest.mark.parametrize("M", [1, 4, 5, 8])
def test_fused_out_cq_dual_vs_fp64(M, d, lib):
    """launch_gemv_dual (the one-utterance step): gemv_dual_kernel<d / 128, d / 64>.
    The q bound is test_gemv's 1e-3 for a LayerNorm-fused f32 output.  It was set for one f16 matrix, here the right half is the PRODUCT W'q Wo
    rounded to f16 and x0 is read as f16: the specified arithmetic (those rounded operands on these inputs, in float64 numpy on the CPU) is
    2.0e-4 .. 2.6e-4 rel-L2 from the reference over d = 384 .. 1280 and M = 1 .. 40 - four times inside the bound, which therefore stands."""
    _out_cq_case(lib, M, d, False, False)


@pytest.mark.parametrize("d", [384, 1280])
@pytest.mark.parametrize("M", [16, 40, 80])
def test_fused_out_cq_frag3_vs_fp64(M, d, lib):
    """launch_gemv_frag3 (the batched step): gemv_frag3_kernel<1 | 3 | 5 row blocks>, M = 40: a ragged last row block; the two halves of q_raw come
    out of the two k-step halves (wks / wk0) of the packed [W'q | W'q Wo].  Bounds as in the dual form."""
    _out_cq_case(lib, M, d, False, False)


@pytest.mark.parametrize("M,d,force_frag", [(5, 384, 0), (5, 1280, 0), (40, 384, 0), (40, 1280, 0), (5, 1280, 1)])
def test_fused_out_cq_partials_are_exact_on_representable_rows(M, d, force_frag, lib):
    """Wo = 0, bo = 0 and x0 of multiples of 1/4 near 200: x1 = x0 bit for bit, and both partials exactly the float64 ones."""
    _out_cq_case(lib, M, d, bool(force_frag), True)


@pytest.mark.parametrize("M,d", [(5, 384), (5, 1280), (8, 1024), (16, 384), (40, 1280), (80, 1280)])
def test_fused_out_cq_feeds_cross_attention(M, d, lib):
    """producer -> consumer of one layer without a model: the tap's q, q2, partials, column sums and bias go straight into
    wis_op_dec_cross_attn_stat (one utterance of M rows; above 8 rows M / 8 utterances of 8, into the fragment image as the batched step does)
    against the float64 layer LN -> cross-Q -> attention from x1_ref.  5e-3 as above: the q error (< 1e-3 relative) sits below the f16 cast."""
    H, T = d // 64, 1500
    B, R = (1, M) if M <= 8 else (M // 8, 8)
    x1_ref, q_ref, stat, q, q2, qcs, qb = _out_cq_case(lib, M, d, False, False)
    K, V, d_kx, d_vt = _kv(H, B, T)
    exp = _attend(q_ref, K, V, B, R)
    got = _cross_call(lib, q, q2, stat, qcs, qb, d_kx, d_vt, B, R, H, T, 6, 0 if M <= 8 else (M + 15) // 16, 0, 0)
    err = np.abs(got - exp).max()
    print(f"out+cq -> cross-attn M{M} d{d}: max abs err {err:.2e}")
    assert err <= 5e-3, (M, d, err)
