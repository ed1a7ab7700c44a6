"""wave_sums<N> (csrc/common.hpp: N sums of a wave through one interleaved tree, the rows closed with gfx950's row swaps) against wave_sum, word for word,
through the wis_op_wave_sums tap: one wave runs wave_sum per value and wave_sums on the same registers in the same launch and returns both, every lane's
word.  N = 6, 10, 16: the 2 RM statistics of the three row-register forms of the LayerNorm-folded skinny GEMM (dec_kernels.hip gemv_body MODE 1).

The tree is the contract - xor 1, xor 2, the other quad, the other half row, then (row 0 + row 1) + (row 2 + row 3) - and float addition is not associative,
so the inputs are chosen to make any other tree change the word: twelve decades of magnitude inside one wave.  The numpy model of that tree is checked
against both outputs, and against the (r0 + r2) + (r1 + r3) closing it must differ on the wide-range inputs."""
import numpy as np
import pytest

f32 = np.float32


def tree(x, closing="01_23"):
    """x f32 [N][64] -> [N]: the balanced pairwise tree in lane order, rows closed as given"""
    with np.errstate(over="ignore", invalid="ignore"):
        w = np.asarray(x, f32).reshape(-1, 4, 16)
        while w.shape[-1] > 1:
            w = w[..., 0::2] + w[..., 1::2]
        w = w[..., 0]
        return (w[:, 0] + w[:, 1]) + (w[:, 2] + w[:, 3]) if closing == "01_23" else (w[:, 0] + w[:, 2]) + (w[:, 1] + w[:, 3])


def inputs(N):
    """name -> f32 [N][64]"""
    rng = np.random.default_rng(N)
    out = {}
    # normals over twelve decades of magnitude in one wave, signs mixed
    out["decades"] = (rng.standard_normal((N, 64)) * 10.0 ** rng.uniform(-6, 6, (N, 64))).astype(f32)
    out["equal"] = np.repeat(rng.standard_normal((N, 1)).astype(f32), 64, axis=1)
    den = (rng.integers(1, 1 << 23, (N, 64), dtype=np.uint32) | (rng.integers(0, 2, (N, 64), dtype=np.uint32) << 31)).view(f32)
    out["denormals"] = den
    big = (rng.standard_normal((N, 64)) * 1e-3).astype(f32)
    big[np.arange(N), rng.integers(0, 64, N)] = f32(3e38)
    out["one_3e38"] = big
    z = np.zeros((N, 64), f32)
    z.view(np.uint32)[rng.random((N, 64)) < 0.5] = 0x80000000
    z[0] = f32(-0.0)      # all lanes -0: the sum is -0
    out["signed_zeros"] = z
    inf = rng.standard_normal((N, 64)).astype(f32)
    inf[np.arange(N), rng.integers(0, 64, N)] = np.inf
    out["inf_lane"] = inf
    nan = rng.standard_normal((N, 64)).astype(f32)
    nan[np.arange(N), rng.integers(0, 64, N)] = np.nan
    out["nan_lane"] = nan
    return out


@pytest.mark.parametrize("N", [6, 10, 16])
def test_inputs_tell_closings_apart(N):
    """pure numpy: on the wide-range inputs the (r0 + r2) + (r1 + r3) closing gives another word for at least one value"""
    x = inputs(N)["decades"]
    assert (tree(x).view(np.uint32) != tree(x, "02_13").view(np.uint32)).any()


@pytest.mark.gpu
@pytest.mark.parametrize("N", [6, 10, 16])
def test_wave_sums_words(lib, N):
    from wis_hip._lib import DevBuf, check
    for name, x in inputs(N).items():
        dx = DevBuf.from_numpy(x)
        d_old, d_new = DevBuf.from_numpy(np.full((N, 64), 77.0, f32)), DevBuf.from_numpy(np.full((N, 64), -77.0, f32))
        check(lib.wis_op_wave_sums(0, dx.ptr, N, d_old.ptr, d_new.ptr))
        old, new = d_old.to_numpy(np.uint32, (N, 64)), d_new.to_numpy(np.uint32, (N, 64))
        want = tree(x).view(np.uint32)
        print(f"wave_sums N{N} {name}: {int((old != new).sum())} of {N * 64} words differ from wave_sum, {int((new[:, 0] != want).sum())} of {N} from the numpy tree")
        assert (old == old[:, :1]).all(), "wave_sum is wave-uniform"
        assert np.array_equal(new, old), name      # bit patterns: NaNs compare too
        if name != "nan_lane":                    # (which quiet NaN an addition returns is the hardware's choice; the two helpers agree on it above)
            assert np.array_equal(new[:, 0], want), name


@pytest.mark.gpu
def test_wave_sums_rejects_other_counts(lib):
    from wis_hip._lib import DevBuf
    d = DevBuf(16 * 64 * 4)
    for N in (0, 5, 8, 17):
        assert lib.wis_op_wave_sums(0, d.ptr, N, d.ptr, d.ptr) != 0
