"""-m gpu: the decoder's attention kernels (csrc/dec_kernels.hip) element by element at their edges - the twin of tests/test_gpu_enc_attn_ops.py.

dec_self_attn_kernel<false, 2 | 4 | 8> and <true, 8> through wis_op_dec_self_attn_ex, dec_self_attn_long_kernel through wis_op_dec_self_attn_long, every
shipped form of dec_cross_attn_kernel / dec_cross_attn_rs_kernel through wis_op_dec_cross_attn_stat, wis_op_dec_cross_attn and
wis_op_dec_cross_attn_folded.  The score patterns, the float64 reference and the bound are tests/dec_attn_ref.py (its docstring derives the bound;
tests/test_dec_attn_model_cpu.py shows on the CPU that numpy models of the loops meet it with factor 1 and that every pattern reaches its path).

Every case asserts: every written element obeys |out - ref| <= 2 unit + 2^-10 |ref| and is finite; three launches agree to the bit; the output buffer,
pre-filled with 0x5A5A, keeps that fill behind its last row, and the fragment-image form (out_mb > 0) holds the same bits in the rows' places and the
tap's zero fill everywhere else; a second run on poisoned memory gives the same bits.  Poison is f16 NaN in every cache element no row may read
(self-attention: positions behind a row's length, slots no row owns, (slot, position) pairs on no row's path), and for cross-attention 0x5A5A in V^T's
padding [T, Tpad) with a NaN block behind the K image and behind the V^T image.

Self-attention packs one (pattern, history length) per row or utterance of a launch, cross-attention one pattern per (utterance, head): the problems of
a grid are independent, so one launch carries many.  Every line printed as `EDGES|family|kernel|pattern|shape|ratio` is the worst
(|out - ref| - 2^-10 |ref|) / unit of that pattern in that case, `LAUNCHES|kernel|n` the launches the case made (to set against a kernel trace); profiles/dec_attn_tests.md holds the figures of an MI355X run, the kernel each case
ran and the mutations these tests catch."""
import functools

import numpy as np
import pytest

import dec_attn_ref as D

pytestmark = pytest.mark.gpu

GUARD = 4096
FACTOR = 2.0
F = np.float64
CA_SPIN_MAX_BH = 192      # csrc/kernels.hpp


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint16)


def _same(a, b):
    return np.array_equal(_bits(a), _bits(b))


def _nan16(shape):
    return np.full(shape, D.NAN16, np.uint16).view(np.float16)


class _Out:
    """an output buffer pre-filled with 0x5A5A, GUARD elements longer than the kernel may write"""

    def __init__(self, M, d, out_mb):
        from wis_hip._lib import DevBuf
        self.M, self.d, self.mb = M, d, out_mb
        self.n = D.xf_elems(d, out_mb) if out_mb else M * d
        self.buf = DevBuf.from_numpy(np.full(self.n + GUARD, D.PAT16, np.uint16))

    def rows(self):
        o = self.buf.to_numpy(np.float16, (self.n + GUARD,))
        self.buf.free()
        assert (_bits(o[self.n:]) == D.PAT16).all(), "output behind the last row overwritten"
        if not self.mb:
            return o[:self.n].reshape(self.M, self.d)
        img = o[:self.n]
        idx = D.xf_index(np.arange(self.M)[:, None], np.arange(self.d)[None, :], self.mb)
        rest = np.ones(self.n, bool)
        rest[idx.reshape(-1)] = False
        assert not _bits(img[rest]).any(), "a store outside the rows' places in the fragment image"
        return img[idx]


class _Report:
    """worst ratio per pattern of one case; prints every figure, then asserts"""

    def __init__(self, family, kernel, shape):
        self.head, self.shape, self.worst, self.bad = f"EDGES|{family}|{kernel}", shape, {}, []
        self.kernel, self.launches = kernel, 0

    def add(self, pattern, out, ref, unit, what):
        if not np.isfinite(np.asarray(out, F)).all():
            self.bad.append((what, pattern, "non-finite"))
        r = D.ratios(out, ref, unit)
        w = float(np.nan_to_num(r, nan=np.inf).max())
        self.worst[pattern] = max(self.worst.get(pattern, 0.0), w)
        if not w <= FACTOR:
            self.bad.append((what, pattern, w, tuple(int(i) for i in np.unravel_index(int(np.nan_to_num(r, nan=np.inf).argmax()), r.shape))))

    def check(self, cond, what):
        if not cond:
            self.bad.append(what)

    def done(self):
        print(f"\nLAUNCHES|{self.kernel}|{self.launches}")
        for p, w in self.worst.items():
            print(f"{self.head}|{p}|{self.shape}|{w:.4f}")
        assert not self.bad, self.bad[:8]


def _batches(items, n):
    return [items[i:i + n] for i in range(0, len(items), n)]


# =======================================================================================
# dec_self_attn_kernel<false, NB>
def _self_launches(lib, rep, q, pos, caches, M, H, ctx, rpu, sstride, rmul, nb, anc=None, w0=0, aw=0, base=None):
    """three launches on the clean cache, one on the poisoned one, one into the fragment image: all the same bits; -> rows f16 [M][d]"""
    from wis_hip._lib import DevBuf, check
    d = 64 * H
    small = [DevBuf.from_numpy(a) if a is not None else None for a in (q, pos, anc, base)]
    d_q, d_pos, d_anc, d_base = small
    outs = []
    for (d_kc, d_vc), mb in ((caches[0], 0), (caches[0], 0), (caches[0], 0), (caches[1], 0), (caches[0], (M + 15) // 16)):
        o = _Out(M, d, mb)
        check(lib.wis_op_dec_self_attn_ex(0, d_q.ptr, d_kc.ptr, d_vc.ptr, d_pos.ptr, o.buf.ptr, M, H, ctx, rpu, sstride, rmul, nb, mb,
                                          d_anc.ptr if d_anc else None, w0, aw, d_base.ptr if d_base else None))
        outs.append(o.rows())
        rep.launches += 1
    for b in small:
        if b is not None:
            b.free()
    rep.check(_same(outs[0], outs[1]) and _same(outs[1], outs[2]), "launches differ")
    rep.check(_same(outs[0], outs[3]), "cache contents no row may read reached the output")
    rep.check(_same(outs[0], outs[4]), "the fragment-image form differs from the row-major one")
    return outs[0]


def _upload_caches(kc, vc, readable):
    """(clean, poisoned) device caches: poisoned = f16 NaN wherever `readable` [slots][ctx] is False, K and V both"""
    from wis_hip._lib import DevBuf
    kp, vp = kc.copy(), vc.copy()
    kp[~readable], vp[~readable] = _nan16(()), _nan16(())
    return (DevBuf.from_numpy(kc), DevBuf.from_numpy(vc)), (DevBuf.from_numpy(kp), DevBuf.from_numpy(vp))


def _free_caches(caches):
    for pair in caches:
        for b in pair:
            b.free()


@pytest.mark.parametrize("mode", ["decode", "prefill"])
@pytest.mark.parametrize("ctx", [448, 64])
@pytest.mark.parametrize("nb", [2, 4, 8])
def test_self_attn_plain_edges(lib, nb, ctx, mode):
    """decode: 16 rows, each in its own slot (rmul = 1) with its own (pattern, length); prefill: 4 utterances of 4 rows at consecutive positions in the
    utterance's first slot (rmul = 0), one (pattern, length) per utterance; one slot (every second one) is owned by no row."""
    rep = _Report("self", f"dec_self_attn_kernel<false, {nb}>", f"ctx{ctx} {mode}")
    combos = [(p, n) for n in D.self_lens(nb, ctx) for p in D.PATTERNS]
    for H in (1, 3):
        d = 64 * H
        for batch in _batches(combos, 16 if mode == "decode" else 4):
            rng = np.random.default_rng([nb, ctx, H, mode == "decode", D.PATTERNS.index(batch[0][0]), batch[0][1]])
            if mode == "decode":
                M, rpu, sstride, rmul, slots = len(batch), len(batch), len(batch) + 1, 1, len(batch) + 1
                groups = [(g, [g], [n - 1]) for g, (_, n) in enumerate(batch)]                                  # (slot, rows, positions)
            else:
                M, rpu, sstride, rmul, slots = 4 * len(batch), 4, 2, 0, 2 * len(batch)
                groups = [(2 * g, list(range(4 * g, 4 * g + 4)), [max(0, n - 4 + r) for r in range(4)]) for g, (_, n) in enumerate(batch)]
            kc = (rng.standard_normal((slots, ctx, d)) * 0.5).astype(np.float16)
            vc = rng.standard_normal((slots, ctx, d)).astype(np.float16)
            readable = np.zeros((slots, ctx), bool)
            q, pos = np.zeros((M, d), np.float32), np.zeros(M, np.int32)
            want = []
            for (pattern, n), (slot, rows, ps) in zip(batch, groups):
                readable[slot, :n] = True
                pos[rows] = ps
                for h in range(H):
                    sl = slice(64 * h, 64 * h + 64)
                    qq, kk, vv = D.problem(pattern, n, 8 * nb, len(rows), rng, False)
                    q[rows, sl], kc[slot, :n, sl], vc[slot, :n, sl] = qq, kk, vv
                    for i, (m, p) in enumerate(zip(rows, ps)):
                        want.append((pattern, m, sl, D.reference(qq[i:i + 1], kk[:p + 1], vv[:p + 1], D.n_acc_self(p + 1, nb))))
            caches = _upload_caches(kc, vc, readable)
            out = _self_launches(lib, rep, q, pos, caches, M, H, ctx, rpu, sstride, rmul, nb)
            _free_caches(caches)
            for pattern, m, sl, (ref, unit) in want:
                rep.add(pattern, out[m:m + 1, sl], ref, unit, (H, m, int(pos[m]) + 1))
    rep.done()


# =======================================================================================
# dec_self_attn_kernel<true, 8>: the rows are nodes of a beam tree (test_self_attn_tree_form_vs_fp64's ancestor tables)
def _tree_levels(pattern, w0, aw, ctx):
    """levels by POSITION (every slot holds them: whichever ancestor a path takes, the structure is the same; the noise dims and V differ per slot, so a
    wrong slot is still a wrong answer).  Blocks are the pre-window part [0, w0) and window steps of w0 positions - or the kernel's 64-position pass where
    the pre-window part is longer - so up / down / far / edge straddle the window boundary (w0 = 3) or the pass boundary (w0 = 70); `tail` rises by
    PEAK per window step, so that EVERY row's largest score is its own last position, in the slot of the beam that produced it."""
    n = w0 + aw
    if pattern == "control":
        return None
    if pattern == "tail":
        lv = np.where(np.arange(n) >= w0, D.PEAK * (np.arange(n) - w0 + 1), 0.0)
    else:
        lv = D.levels(pattern, n, 64 if w0 > 64 else w0)
    return np.concatenate([lv, np.zeros(ctx - n)])


@pytest.mark.parametrize("with_base", [False, True])
@pytest.mark.parametrize("w0", [3, 70])
@pytest.mark.parametrize("aw", [1, 5, 32])
def test_self_attn_tree_edges(lib, aw, w0, with_base):
    M, ctx, slots = 16, 448, 8
    rep = _Report("self", "dec_self_attn_kernel<true, 8>", f"aw{aw} w0 {w0} base{int(with_base)}")
    for H in (1, 3):
        d = 64 * H
        for pattern in D.PATTERNS:
            rng = np.random.default_rng([aw, w0, with_base, H, D.PATTERNS.index(pattern)])
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
            lv = _tree_levels(pattern, w0, aw, ctx)
            kc, vc = np.empty((slots, ctx, d), np.float16), np.empty((slots, ctx, d), np.float16)
            q = np.empty((M, d), np.float32)
            for h in range(H):
                sl = slice(64 * h, 64 * h + 64)
                for s in range(slots):
                    qq, kc[s, :, sl], vc[s, :, sl] = D.make_control(ctx, M, rng, False) if lv is None else D.make_qkv(pattern, lv, M, rng, False)
                q[:, sl] = qq
            readable = np.zeros((slots, ctx), bool)
            paths = []
            for m in range(M):
                n = int(pos[m]) + 1
                sl_of = np.array([(base[m] if with_base else anc[m, 0]) if p < w0 else anc[m, p - w0] for p in range(n)])
                readable[sl_of, np.arange(n)] = True
                paths.append(sl_of)
            caches = _upload_caches(kc, vc, readable)
            out = _self_launches(lib, rep, q, pos, caches, M, H, ctx, 16, 0, 0, 8, anc, w0, aw, base)
            _free_caches(caches)
            for m in range(M):
                n = len(paths[m])
                kk, vv = kc[paths[m], np.arange(n)], vc[paths[m], np.arange(n)]
                for h in range(H):
                    sl = slice(64 * h, 64 * h + 64)
                    ref, unit = D.reference(q[m:m + 1, sl], kk[:, sl], vv[:, sl], D.n_acc_self(n, 8))
                    rep.add(pattern, out[m:m + 1, sl], ref, unit, (H, m, n))
    rep.done()


# =======================================================================================
# dec_self_attn_long_kernel
def _sufs(k, i):
    """generated lengths of the k rows of utterance number i: mixed within the utterance, every length of D.SUFFIXES in turn"""
    S = D.SUFFIXES
    return [S[(i + 2 * j) % len(S)] for j in range(k)] if k < 8 else [S[(i + j) % len(S)] for j in range(k)]


@pytest.mark.parametrize("k", [1, 3, 8])
@pytest.mark.parametrize("plen", D.PLENS)
def test_self_attn_long_edges(lib, plen, k):
    """B utterances of k rows: the prompt's plen positions in the utterance's first slot, row j's generated positions behind them in slot b k + j.
    Poisoned: prefix-slot positions >= plen (but row 0's own), own-slot positions outside [plen, pos], one slot behind the last utterance's."""
    from wis_hip._lib import DevBuf, check
    ctx = 448
    rep = _Report("long", "dec_self_attn_long_kernel", f"plen{plen} k{k}")
    for B, H in ((1, 1), (2, 3)):
        d, M = 64 * H, B * k
        for bi, batch in enumerate(_batches(D.PATTERNS, B)):
            batch = (batch * B)[:B]
            rng = np.random.default_rng([plen, k, B, bi])
            slots = M + 1
            kc = (rng.standard_normal((slots, ctx, d)) * 0.5).astype(np.float16)
            vc = rng.standard_normal((slots, ctx, d)).astype(np.float16)
            readable = np.zeros((slots, ctx), bool)
            q, pos = np.zeros((M, d), np.float32), np.zeros(M, np.int32)
            want = []
            for b, pattern in enumerate(batch):
                sufs = _sufs(k, B * bi + b + plen)
                readable[b * k, :plen] = True
                for j, s in enumerate(sufs):
                    pos[b * k + j] = plen + s - 1
                    readable[b * k + j, plen:plen + s] = True
                for h in range(H):
                    sl = slice(64 * h, 64 * h + 64)
                    qq, kp, vp, own = D.long_problem(pattern, plen, sufs, rng)
                    q[b * k:b * k + k, sl] = qq
                    kc[b * k, :plen, sl], vc[b * k, :plen, sl] = kp, vp
                    for j, s in enumerate(sufs):
                        kc[b * k + j, plen:plen + s, sl], vc[b * k + j, plen:plen + s, sl] = own[j]
                        ref = D.reference(qq[j:j + 1], np.concatenate([kp, own[j][0]]), np.concatenate([vp, own[j][1]]), D.n_acc_long(plen + s, plen))
                        want.append((pattern, b * k + j, sl, ref))
            caches = _upload_caches(kc, vc, readable)
            d_q, d_pos, d_plen = DevBuf.from_numpy(q), DevBuf.from_numpy(pos), DevBuf.from_numpy(np.full(B, plen, np.int32))
            outs = []
            for (d_kc, d_vc), mb in ((caches[0], 0), (caches[0], 0), (caches[0], 0), (caches[1], 0), (caches[0], (M + 15) // 16)):
                o = _Out(M, d, mb)
                check(lib.wis_op_dec_self_attn_long(0, d_q.ptr, d_kc.ptr, d_vc.ptr, d_pos.ptr, d_plen.ptr, o.buf.ptr, B, k, H, ctx, mb))
                outs.append(o.rows())
                rep.launches += 1
            _free_caches(caches)
            for b_ in (d_q, d_pos, d_plen):
                b_.free()
            rep.check(_same(outs[0], outs[1]) and _same(outs[1], outs[2]), "launches differ")
            rep.check(_same(outs[0], outs[3]), "cache contents no row may read reached the output")
            rep.check(_same(outs[0], outs[4]), "the fragment-image form differs from the row-major one")
            for pattern, m, sl, (ref, unit) in want:
                rep.add(pattern, outs[0][m:m + 1, sl], ref, unit, (B, H, m, int(pos[m]) + 1))
    rep.done()


# =======================================================================================
# cross-attention
def cross_kernel(tap, B, R, H, T, chunks, no_spin=0):
    """the instantiation launch_dec_cross_attn (dec_kernels.hip) gives a call of a tap (`stat`: the fold from row partials, `folded`: the fold from the
    rows, `plain`: the finished query), restated from its rules; the taps hand it granule buffers iff B H <= CA_SPIN_MAX_BH and not no_spin"""
    d = 64 * H
    CL = D.cdiv(D.cdiv(T, chunks), 32) * 32
    used = D.cdiv(T, CL)
    assert CL in (128, 256) and CL * chunks <= D.cdiv(T, 64) * 64
    spin = B * H <= CA_SPIN_MAX_BH and not no_spin and CL == 256 and 2 <= used <= 6 and R <= 8
    s = "SPIN" if spin else "-"
    if tap == "stat":
        small = B * H * used <= 256
        if CL == 256 and used <= 6 and R <= 8 and d <= 1280:
            return f"dec_cross_attn_rs_kernel<{s}, {'NT' if small else '-'}, 2>", CL
        if CL == 128:
            return "dec_cross_attn_kernel<2, 16, 2, ->", CL
        if used > 6:
            return "dec_cross_attn_kernel<4, 16, 2, ->", CL
        return f"dec_cross_attn_kernel<4, 6, {3 if small else (4 if R <= 8 else 2)}, {s}>", CL
    fold = 1 if tap == "folded" else 0
    if CL == 128:
        return f"dec_cross_attn_kernel<2, 16, {fold}, ->", CL
    return f"dec_cross_attn_kernel<4, {6 if used <= 6 else 16}, {fold}, {s}>", CL


@functools.lru_cache(maxsize=200)
def _cross_problem(pattern, T, CL, R, variant):
    """one (utterance, head): inputs and reference, computed once and shared by every form that runs it"""
    rng = np.random.default_rng([D.CROSS_PATTERNS.index(pattern), T, CL, R, variant])
    q, k, v = D.problem(pattern, T, CL, R, rng, True)
    ref, unit = D.reference(q, k, v, D.n_acc_cross(T, CL), chunk=CL)
    for a in (q, k, v, ref, unit):
        a.setflags(write=False)
    return q, k, v, ref, unit


def _guarded(img, bits):
    return np.concatenate([_bits(img).reshape(-1), np.full(GUARD, bits, np.uint16)])


def _cross_case(lib, tap, B, R, H, T, chunks, no_spin=0, kv_shared=0, expect=None):
    from wis_hip._lib import DevBuf, check
    kernel, CL = cross_kernel(tap, B, R, H, T, chunks, no_spin)
    if expect is not None:
        assert kernel == expect, (kernel, expect)
    d, M, Tpad = 64 * H, B * R, D.cdiv(T, 64) * 64
    NP = len(D.CROSS_PATTERNS)
    rep = _Report("cross", kernel, f"{tap} B{B} R{R} H{H} T{T}/{chunks}" + (" no_spin" if no_spin else "") + (" kv_shared" if kv_shared else ""))
    # utterance 0 decides where `flat` sits (below), so on narrow grids its heads go through all the patterns in turn, launch by launch
    for offset in range(0, NP, H) if H <= 8 else [0]:
        # utterance 0: the patterns in turn; the others five further on - but a head that is `flat` anywhere is flat everywhere (q = 0 needs
        # zero column sums and bias in the fold forms, which the utterances share)
        pat = [[D.CROSS_PATTERNS[(h + offset) % NP] for h in range(H)]]
        for b in range(1, B):
            other = [D.CROSS_PATTERNS[(h + 5 * b + offset) % NP] for h in range(H)]
            pat.append([p0 if "flat" in (p0, p) else p for p0, p in zip(pat[0], other)])
        K, V = np.empty((B, T, d), np.float16), np.empty((B, T, d), np.float16)
        q16 = np.empty((M, d), np.float32)
        want = []
        for b in range(B):
            for h in range(H):
                sl = slice(64 * h, 64 * h + 64)
                kvb = 0 if kv_shared else b      # kv_shared: every row group reads utterance 0's K / V (the others hold different data)
                K[b, :, sl], V[b, :, sl] = _cross_problem(pat[b][h], T, CL, R, b % 3)[1:3]
                q, k, v, ref, unit = _cross_problem(pat[kvb][h], T, CL, R, kvb % 3)
                if kv_shared and b:             # the group's own queries against utterance 0's keys: its own reference
                    q = _cross_problem(pat[b][h], T, CL, R, b % 3)[0]
                    ref, unit = D.reference(q, k, v, D.n_acc_cross(T, CL), chunk=CL)
                q16[b * R:b * R + R, sl] = q
                want.append((pat[kvb][h], slice(b * R, b * R + R), sl, ref, unit))
        kx = D.k_image(K)
        images = [(DevBuf.from_numpy(_guarded(kx, 0)), DevBuf.from_numpy(_guarded(D.vt_image(V, Tpad, 0), 0))),
                  (DevBuf.from_numpy(_guarded(kx, D.NAN16)), DevBuf.from_numpy(_guarded(D.vt_image(V, Tpad, D.PAT16), D.NAN16)))]
        rng = np.random.default_rng([B, R, H, T, chunks, offset])
        if tap == "plain":
            forms = [(q16, None, None, None, None)]
        else:
            zero = np.repeat(np.array([p == "flat" for p in pat[0]]), 64)
            ops = D.fold_operands(q16, rng, zero)
            D.fold_query_check(q16, ops, from_rows=tap == "folded")
            if tap == "folded":
                forms = [(ops["q_one"], None, ops["x"], ops["qcs"], ops["qb"])]
            else:
                forms = [(ops["q_one"], None, ops["stat"], ops["qcs"], ops["qb"]), (ops["q_a"], ops["q_b"], ops["stat"], ops["qcs"], ops["qb"])]
        outs = []
        for q, q2, xs, qcs, qb in forms:
            bufs = [None if a is None else DevBuf.from_numpy(np.ascontiguousarray(a, np.float32)) for a in (q, q2, xs, qcs, qb)]
            ptr = [b_.ptr if b_ else None for b_ in bufs]
            for (d_kx, d_vt), mb in ((images[0], 0), (images[0], 0), (images[0], 0), (images[1], 0), (images[0], (M + 15) // 16)):
                o = _Out(M, d, mb)
                if tap == "stat" or (tap == "plain" and (R > 8 or kv_shared or mb)):
                    check(lib.wis_op_dec_cross_attn_stat(0, *ptr, d_kx.ptr, d_vt.ptr, o.buf.ptr, B, R, H, T, chunks, mb, kv_shared, no_spin))
                elif tap == "plain":
                    check(lib.wis_op_dec_cross_attn(0, ptr[0], d_kx.ptr, d_vt.ptr, o.buf.ptr, B, R, H, T, chunks))
                elif mb:
                    continue      # (wis_op_dec_cross_attn_folded writes rows only)
                else:
                    check(lib.wis_op_dec_cross_attn_folded(0, ptr[0], ptr[2], ptr[3], ptr[4], d_kx.ptr, d_vt.ptr, o.buf.ptr, B, R, H, T, chunks))
                outs.append(o.rows())
                rep.launches += 3      # (the cross-attention taps launch three times: the granule form's epochs advance)
            for b_ in bufs:
                if b_:
                    b_.free()
        for pair in images:
            for b_ in pair:
                b_.free()
        rep.check(_same(outs[0], outs[1]) and _same(outs[1], outs[2]), "launches differ")
        rep.check(_same(outs[0], outs[3]), "V^T padding / memory behind the K or V^T image reached the output")
        rep.check(all(_same(outs[0], o) for o in outs[4:]), "the fragment-image form or the two-halves query differs from the first run")
        for pattern, rows, sl, ref, unit in want:
            rep.add(pattern, outs[0][rows, sl], ref, unit, (rows.start // R, sl.start // 64))
    rep.done()


_SMALL = [      # (tap, B, H, no_spin, the kernel at T = 1500 in 6 chunks)
    ("stat", 1, 6, 0, "dec_cross_attn_rs_kernel<SPIN, NT, 2>"),
    ("stat", 1, 6, 1, "dec_cross_attn_rs_kernel<-, NT, 2>"),
    ("stat", 8, 6, 0, "dec_cross_attn_rs_kernel<SPIN, -, 2>"),
    ("stat", 8, 6, 1, "dec_cross_attn_rs_kernel<-, -, 2>"),
    ("plain", 1, 6, 0, "dec_cross_attn_kernel<4, 6, 0, SPIN>"),
    ("folded", 1, 6, 0, "dec_cross_attn_kernel<4, 6, 1, SPIN>"),
]


@pytest.mark.parametrize("tap,B,H,no_spin,kernel", _SMALL, ids=[f"{c[0]}-B{c[1]}-{'ticket' if c[3] else 'granule'}" for c in _SMALL])
@pytest.mark.parametrize("R", [1, 5, 8])
@pytest.mark.parametrize("T,chunks", [(1500, 6), (1536, 6), (449, 2)])
def test_cross_attn_small_grid_edges(lib, T, chunks, R, tap, B, H, no_spin, kernel):
    """the H = 6 grids in every form, at a ragged last chunk of 220 keys (T 1500), none (1536) and two chunks with 193 keys in the last (449);
    at T = 449 the 8-utterance grid is `small` too (96 workgroups), so it runs the NT form: the case is named by what cross_kernel says"""
    _cross_case(lib, tap, B, R, H, T, chunks, no_spin, expect=kernel if T != 449 else None)


_LARGE = [      # (B, H, R, T, chunks, kernel)
    (10, 20, 5, 1500, 6, "dec_cross_attn_rs_kernel<-, -, 2>"),        # B H = 200 > 192: no granule buffers
    (1, 32, 5, 1500, 6, "dec_cross_attn_kernel<4, 6, 3, SPIN>"),       # d = 2048: beyond the rs kernel; 192 workgroups: small
    (1, 32, 8, 449, 2, "dec_cross_attn_kernel<4, 6, 3, SPIN>"),
    (2, 32, 5, 1500, 6, "dec_cross_attn_kernel<4, 6, 4, SPIN>"),       # 384 workgroups: the operands through LDS
    (2, 32, 1, 1536, 6, "dec_cross_attn_kernel<4, 6, 4, SPIN>"),
    (1, 6, 5, 1500, 12, "dec_cross_attn_kernel<2, 16, 2, ->"),         # 128-key chunks, the last one of 92 keys
    (1, 6, 8, 1536, 12, "dec_cross_attn_kernel<2, 16, 2, ->"),
    (2, 6, 1, 1500, 12, "dec_cross_attn_kernel<2, 16, 2, ->"),
]


@pytest.mark.parametrize("B,H,R,T,chunks,kernel", _LARGE)
def test_cross_attn_from_partials_other_forms_edges(lib, B, H, R, T, chunks, kernel):
    _cross_case(lib, "stat", B, R, H, T, chunks, expect=kernel)


@pytest.mark.parametrize("kv_shared", [0, 1])
@pytest.mark.parametrize("T,chunks", [(1500, 6), (449, 2)])
def test_cross_attn_plain_16_rows_edges(lib, T, chunks, kv_shared):
    """R = 16, the finished query, the ticket form; kv_shared: both row groups read utterance 0, whose K / V differ from utterance 1's in memory"""
    _cross_case(lib, "plain", 2, 16, 6, T, chunks, kv_shared=kv_shared, expect="dec_cross_attn_kernel<4, 6, 0, ->")
