"""float32 model of the LayerNorm-folded skinny GEMM of the decode step (dec_kernels.hip gemv_body MODE 1), operation for operation, for weights that make
the MFMA part exact: W one-hot per output row (a single 1.0 at column k_n; the QKV tap's packer scales the query rows by 1/8, a power of two), gamma = 1,
beta = 0.  Then the accumulator of output n is exactly f32(f16(x[m][k_n])) (times 1/8 on a query row), the folded column sum exactly 1 (or 1/8), the folded
bias the bias, and what is left is float32 arithmetic in a known order:

  shift     c = x[r][0]
  partials  thread tid of 256 owns float4 columns tid and tid + 256 (where they exist), and with a, b, c, e = the four values minus the shift
            sa = 0; sa += (a + b) + (c + e) per column     sb = 0; sb += (a a + b b) + (c c + e e) per column
  tree      the balanced pairwise tree over the 256 threads in natural order: wave_sum's tree over the 64 lanes of a wave (xor 1, xor 2, the other quad,
            the other half row, (row 0 + row 1) + (row 2 + row 3)), then (w0 + w1) + (w2 + w3) in the epilogue
  final     A = S1 * f32(1 / K), B = S2 * f32(1 / K), mu = c + A, rs = 1 / sqrt(max(B - A A, 0) + 1e-5) with correctly rounded division and square root
            y = rs * (s - mu * cs) + bias, nothing contracted

`tree` selects the reduction order: "pairwise" is the kernel's; "rows02" pairs the 16-lane rows (0, 2), (1, 3) (what closing the rows with the half swap
first computes) and "sequential" adds the 256 partials in index order - the two other trees the tests use to show that the inputs tell trees apart."""
import numpy as np

f32 = np.float32


def thread_partials(x):
    """x f32 [K] -> (sa, sb) f32 [256]: what each thread of the workgroup holds in front of the reduction"""
    K = x.shape[0]
    assert K % 4 == 0 and K // 4 <= 512
    c = x[0]
    sa, sb = np.zeros(256, f32), np.zeros(256, f32)
    x4 = x.reshape(K // 4, 4)
    for j in range(2):
        n = min(max(K // 4 - 256 * j, 0), 256)
        if n == 0:
            continue
        v = x4[256 * j:256 * j + n] - c
        a, b, cc, e = v[:, 0], v[:, 1], v[:, 2], v[:, 3]
        sa[:n] = sa[:n] + ((a + b) + (cc + e))
        sb[:n] = sb[:n] + ((a * a + b * b) + (cc * cc + e * e))
    return sa, sb


def reduce256(v, tree="pairwise"):
    v = np.asarray(v, f32)
    assert v.shape == (256,)
    if tree == "sequential":
        s = f32(0)
        for t in v:
            s = f32(s + t)
        return s
    w = v.reshape(4, 4, 16)      # [wave][row][lane of the row]
    while w.shape[-1] > 1:       # inside a 16-lane row: adjacent pairs, four times
        w = w[..., 0::2] + w[..., 1::2]
    w = w[..., 0]                # [wave][row]
    if tree == "pairwise":
        w = (w[:, 0] + w[:, 1]) + (w[:, 2] + w[:, 3])
    elif tree == "rows02":
        w = (w[:, 0] + w[:, 2]) + (w[:, 1] + w[:, 3])
    else:
        raise ValueError(tree)
    return f32((w[0] + w[1]) + (w[2] + w[3]))


def row_stats(x, tree="pairwise"):
    """-> (mu, rs) of one raw row, as the epilogue computes them"""
    K = x.shape[0]
    sa, sb = thread_partials(x)
    invK = f32(1.0) / f32(K)
    A = f32(reduce256(sa, tree) * invK)
    B = f32(reduce256(sb, tree) * invK)
    mu = f32(x[0] + A)
    var = np.maximum(f32(B - f32(A * A)), f32(0))
    rs = f32(1.0) / np.sqrt(f32(var + f32(1e-5)), dtype=f32)
    return mu, f32(rs)


def model(x, kn, bias, qscale_rows=0, tree="pairwise"):
    """x f32 [M][K], kn int [N] (the hot column of each output row), bias f32 [N] (as the kernel adds it) -> y f32 [M][N].  Output rows n < qscale_rows
    carry the folded query scale: accumulator and column sum times 1/8."""
    x = np.ascontiguousarray(x, f32)
    M, K = x.shape
    N = kn.shape[0]
    sc = np.where(np.arange(N) < qscale_rows, f32(0.125), f32(1.0)).astype(f32)
    y = np.empty((M, N), f32)
    with np.errstate(over="ignore", invalid="ignore"):
        for m in range(M):
            mu, rs = row_stats(x[m], tree)
            s = x[m, kn].astype(np.float16).astype(f32) * sc      # exact: one product per output, a power-of-two scale
            y[m] = rs * (s - mu * sc) + bias
    return y


def rows(kinds, K, seed):
    """the three kinds of rows of the tests: 'r' random about a common offset of 200 (sigma 2.4), 'c' constant (variance 0), 'm' 1e4 and 1e-4 magnitudes
    mixed, signs random"""
    rng = np.random.default_rng(seed)
    out = np.empty((len(kinds), K), f32)
    for i, k in enumerate(kinds):
        if k == "r":
            out[i] = (200.0 + 2.4 * rng.standard_normal(K)).astype(f32)
        elif k == "c":
            out[i] = f32(3.25 * (i + 1))
        elif k == "m":
            mag = np.where(rng.random(K) < 0.5, 1e4, 1e-4) * (1 + 0.25 * rng.random(K))
            out[i] = (mag * rng.choice([-1.0, 1.0], K)).astype(f32)
        else:
            raise ValueError(k)
    return out


KINDS = "rcmrmcrm"      # row i of a test's input; row 0 is random, so every input set tells the trees apart
