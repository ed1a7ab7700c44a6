"""The tail of the LayerNorm-folded projections of the one-utterance decode step (dec_kernels.hip gemv_body MODE 1: row statistics reduced behind the MFMA
loop, published through LDS, finalised in the epilogue), word for word against a float32 model of the kernel's own arithmetic (tests/ln_tail_ref.py), through
the wis_op_gemv (flags 8 | 4: LayerNorm fold, fp32 output) and wis_op_gemv_qkv taps.  One-hot weights, gamma = 1 and beta = 0 make the MFMA part exact, so
every output word is determined by the order of the float32 sums - a reduction tree other than wave_sum's changes words, and the tests below assert that
their inputs do tell trees apart.  The test passes unchanged on the build in front of the change that reduces the 2 RM statistics together (it ran there
first): that is what makes it a same-bits test.

Which kernel runs (launch_gemv's own predicate: two n-tiles per workgroup at K = 1280, 4 or 5 rows, N % 32 == 0, N >= 4096, no residual / QKV epilogue):
  K =  384, N =   44   gemv_kernel<1, 1,  3, RM, false>         3 workgroups, the last with columns past N; 96 float4 columns: waves 0 and 1 hold partials (wave 1 half), nothing at tid + 256
  K = 1280, N =   48   gemv_kernel<1, 1, 10, RM, false>         3 workgroups; wave 0 alone owns the second column set (tid + 256 < 320)
  K = 1280, N = 4096   gemv_kernel<1, 1, 20, 5, false, 2>       M = 4, 5: the two-tile (FFN1 / vocabulary) instantiation, 128 workgroups
                       gemv_kernel<1, 1, 10, RM, false>         M = 3, 6: one tile, 256 workgroups, at the same N
  QKV, d = 384 / 1280  gemv_kernel<1, 1, 3 / 10, RM, false>     N = 3 d, the scatter epilogue: q fp32, K / V rows as f16 at (slot, pos)
RM = 3, 5, 8 for M <= 3, <= 5, <= 8: rows M .. RM - 1 are clamped duplicates of row M - 1."""
import ctypes
import functools

import numpy as np
import pytest

import ln_tail_ref as R

GV_OUT_F32, GV_LN = 4, 8
GUARD = 256


def _draw(model, M, K):
    """rows that tell the trees apart.  Pairing the rows (0, 2), (1, 3) re-associates ONE addition per wave, and whether that moves a rounding is a coin
    toss per row; so the rows are drawn again (the model alone decides, nothing of the code under test) until both other trees change an output word."""
    for seed in range(M + K, M + K + 64000, 1000):
        x = R.rows(R.KINDS[:M], K, seed=seed)
        ref = model(x)
        wrong = tuple(model(x, tree=t) for t in ("rows02", "sequential"))
        if all((w.view(np.uint32) != ref.view(np.uint32)).any() for w in wrong):
            return x, ref, wrong
    raise AssertionError("no draw told the trees apart")


@functools.lru_cache(maxsize=None)
def _case(M, N, K):
    """inputs, computed once and shared: x [M][K], the hot columns, bias, the model's output and the two wrong-tree outputs"""
    rng = np.random.default_rng(1000 * M + N + K)
    kn = rng.integers(0, K, N)
    kn[:4] = [0, K - 1, K // 2, 1]
    bias = rng.standard_normal(N).astype(np.float32)
    W = np.zeros((N, K), np.float16)
    W[np.arange(N), kn] = 1.0
    x, ref, wrong = _draw(lambda x, **kw: R.model(x, kn, bias, **kw), M, K)
    for a in (x, kn, bias, W, ref) + wrong:
        a.setflags(write=False)
    return x, kn, bias, W, ref, wrong


GEMV_SHAPES = [(M, 44, 384) for M in range(1, 9)] + [(M, 48, 1280) for M in range(1, 9)] + [(M, 4096, 1280) for M in (3, 4, 5, 6)]


@pytest.mark.parametrize("M,N,K", [s for s in GEMV_SHAPES if s[1] < 4096] + [(5, 4096, 1280)])
def test_inputs_tell_trees_apart(M, N, K):
    """pure numpy: the model with the rows paired (0, 2), (1, 3) and with a sequential sum differs from the true model in at least one output word"""
    _, _, _, _, ref, wrong = _case(M, N, K)
    for w in wrong:
        assert (w.view(np.uint32) != ref.view(np.uint32)).any()
    assert np.isfinite(ref).all()


def test_model_matches_float64_layernorm():
    """the model is a LayerNorm: against float64 on the same rows, within what the float32 single-pass statistics allow"""
    x, kn, bias, _, ref, _ = _case(5, 48, 1280)
    x64 = x.astype(np.float64)
    want = (x.astype(np.float16).astype(np.float64)[:, kn] - x64.mean(1, keepdims=True)) / np.sqrt(x64.var(1, keepdims=True) + 1e-5) + bias
    # (row 1 is constant: 0 / sqrt(1e-5) apart from the f16 rounding of the operand, which the variance of 0 magnifies by 316)
    assert np.abs(ref - want)[[0, 2, 3, 4]].max() < 2e-2
    assert np.abs(ref - want)[1].max() < 316 * 2.0 ** -11 * 8


@pytest.mark.gpu
@pytest.mark.parametrize("M,N,K", GEMV_SHAPES)
def test_gemv_ln_words(lib, M, N, K):
    from wis_hip._lib import DevBuf, check
    x, kn, bias, W, ref, wrong = _case(M, N, K)
    for w in wrong:
        assert (w.view(np.uint32) != ref.view(np.uint32)).any()
    host = np.full(M * N + 2 * GUARD, -77.0, np.float32)
    ones, zeros = np.ones(K, np.float32), np.zeros(K, np.float32)
    dx, dg, db, dW, dbias, dy = (DevBuf.from_numpy(a) for a in (x, ones, zeros, W, bias, host))
    check(lib.wis_op_gemv(0, dx.ptr, dg.ptr, db.ptr, dW.ptr, dbias.ptr, ctypes.c_void_p(dy.ptr.value + 4 * GUARD), M, N, K, GV_LN | GV_OUT_F32))
    raw = dy.to_numpy(np.float32, host.shape)
    got = raw[GUARD:GUARD + M * N].reshape(M, N)
    nd = int((got.view(np.uint32) != ref.view(np.uint32)).sum())
    print(f"gemv LN tail M{M} N{N} K{K}: {nd} of {M * N} words differ from the float32 model; max |diff| {float(np.abs(got - ref).max()):.3e}")
    assert (raw[:GUARD] == -77.0).all() and (raw[GUARD + M * N:] == -77.0).all(), "a store outside the M x N output"
    assert np.array_equal(got.view(np.uint32), ref.view(np.uint32))


@functools.lru_cache(maxsize=None)
def _qkv_case(M, d):
    rng = np.random.default_rng(77 * M + d)
    N = 3 * d
    kn = rng.integers(0, d, N)
    kn[[0, d, 2 * d]] = 0; kn[[1, d + 1, 2 * d + 1]] = d - 1
    bias = rng.standard_normal(N).astype(np.float32)
    W = np.zeros((N, d), np.float16)
    W[np.arange(N), kn] = 1.0
    b2 = bias.copy(); b2[:d] *= np.float32(0.125)      # the loader scales the query part of the bias with the query rows
    x, ref, wrong = _draw(lambda x, **kw: R.model(x, kn, b2, qscale_rows=d, **kw), M, d)
    for a in (x, bias, W, ref) + wrong:
        a.setflags(write=False)
    return x, bias, W, ref, wrong


def _at(buf, byte_off):
    return ctypes.c_void_p(buf.ptr.value + int(byte_off))


@pytest.mark.gpu
@pytest.mark.parametrize("M,d", [(M, 384) for M in (1, 3, 4, 8)] + [(M, 1280) for M in (2, 5, 6, 8)])
def test_qkv_ln_words(lib, M, d):
    """q: all words; K / V: the f16 rows at (slot, pos).  The slots are not the row indices, the last one lies beyond 2^31 BYTES into either cache at d = 384
    and beyond 2^31 ELEMENTS at d = 1280 (the address arithmetic has to be 64-bit), positions include the first and the last of a slot.  The caches are
    allocated, not filled: a window of sentinel rows goes around every row the launch writes (the positions on either side, wrapping into the neighbouring
    slot) and must come back unchanged."""
    from wis_hip._lib import DevBuf, check, load, ptr
    x, bias, W, ref, wrong = _qkv_case(M, d)
    for w in wrong:
        assert (w.view(np.uint32) != ref.view(np.uint32)).any()
    ctx = 448
    rng = np.random.default_rng(5 * M + d)
    need = (2 ** 31 if d == 384 else 2 ** 32) // (ctx * d * 2) + 2      # first slot whose rows start past the mark
    # (every other slot at the most: the windows of two rows never meet)
    slot = np.sort(rng.choice(np.arange(1, need - 1, 2), M - 1, replace=False)).astype(np.int64) if M > 1 else np.zeros(0, np.int64)
    slot = np.concatenate([slot, [need]])
    rng.shuffle(slot)
    assert (slot != np.arange(M)).any() and int(slot.max()) * ctx * d * 2 > (2 ** 31 if d == 384 else 2 ** 32)
    pos = np.concatenate([[ctx - 1], [0], 1 + rng.permutation(ctx - 2)])[:M]
    rng.shuffle(pos)
    nslots = int(slot.max()) + 1
    rowb = d * 2
    caches = [DevBuf(nslots * ctx * rowb + rowb), DevBuf(nslots * ctx * rowb + rowb)]      # (one spare row behind the last slot: the window of its last position)
    sent = ((np.arange(3 * d, dtype=np.uint32) * 2654435761 >> 13) & 0x7FFF).astype(np.uint16)
    L = load()
    first = [max(int(s) * ctx + int(p) - 1, 0) for s, p in zip(slot, pos)]      # first row of each window
    for c in caches:
        for f in first:
            check(L.wis_dev_h2d(0, _at(c, f * rowb), ptr(sent), sent.nbytes))
    d_q = DevBuf.from_numpy(np.full(M * d + 2 * GUARD, -77.0, np.float32))
    ones, zeros = np.ones(d, np.float32), np.zeros(d, np.float32)
    bufs = [DevBuf.from_numpy(a) for a in (x, ones, zeros, W, bias, slot.astype(np.int32), pos.astype(np.int32))]
    check(lib.wis_op_gemv_qkv(0, *[b.ptr for b in bufs], _at(d_q, 4 * GUARD), caches[0].ptr, caches[1].ptr, M, d, ctx))
    rawq = d_q.to_numpy(np.float32, (M * d + 2 * GUARD,))
    q = rawq[GUARD:GUARD + M * d].reshape(M, d)
    print(f"QKV LN tail M{M} d{d}: q {int((q.view(np.uint32) != ref[:, :d].view(np.uint32)).sum())} of {M * d} words differ from the float32 model")
    assert (rawq[:GUARD] == -77.0).all() and (rawq[GUARD + M * d:] == -77.0).all()
    assert np.array_equal(q.view(np.uint32), ref[:, :d].view(np.uint32))
    for name, c, want in (("K", caches[0], ref[:, d:2 * d]), ("V", caches[1], ref[:, 2 * d:])):
        want16 = want.astype(np.float16).view(np.uint16)
        for m, f in enumerate(first):
            win = np.empty(3 * d, np.uint16)
            check(L.wis_dev_d2h(0, ptr(win), _at(c, f * rowb), win.nbytes))
            at = int(slot[m]) * ctx + int(pos[m]) - f      # the written row's place in the window (0 where the window starts at the cache's first row)
            exp = sent.copy(); exp[at * d:(at + 1) * d] = want16[m]
            nd = int((win[at * d:(at + 1) * d] != want16[m]).sum())
            print(f"  {name} row {m} (slot {int(slot[m])}, pos {int(pos[m])}): {nd} of {d} words differ")
            assert np.array_equal(win, exp), f"{name} row {m}: the row at (slot, pos) or a sentinel row next to it"
