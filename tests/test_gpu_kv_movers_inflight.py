"""-m gpu: the two in-place cache movers (dec_kernels.hip kv_reorder_kernel, its FROM form and kv_gather_kernel), exact against a numpy gather through
wis_op_kv_reorder, wis_op_kv_reorder_from and wis_op_kv_gather, on the cases a form with every slot's request in flight at once has to get right.
Such a form (eight unconditional loads per thread - a slot that keeps its row, or one beyond the beam, asks for a stand-in chunk and drops it - one
wait, then the stores) was measured and did not ship (profiles/out_cq_kernel_ab.txt); the cases hold for the guarded loads the
kernels keep, and stay for whoever tries again:

a slot that continues itself must keep its bytes whatever sits in its register; a beam smaller than eight must never read or write a slot beyond its
own (slots = beam + 1: the spare slot's bytes are checked, and nothing lies behind it); a cycle must see every parent chunk before any row is
overwritten; positions at or above the history stay.  History lengths 1 .. 3 are fewer than the 8 position slices of the grid: most workgroups have
nothing to do.  Every f16 bit pattern is fair game (NaN payloads, both zeros): the comparison is on the raw words."""
import numpy as np
import pytest

from test_gpu_sample_ops import VS_BASE, VS_INTS, VS_NWIN, VS_PATH, VS_PATH_W, _biteq, _gather, _i32, _random_f16_bits, _reorder

pytestmark = pytest.mark.gpu
L, CTX = 2, 16


def _tables(beam):
    """name -> parent slot per beam (one utterance, slots 0 .. beam - 1)"""
    cyc = (np.arange(beam) + 1) % beam                       # one cycle through every slot: the in-place hazard
    mixed = np.arange(beam); mixed[-1] = 0                   # all continue themselves but the last: the stand-in chunk is slot 0's, in beam - 1 registers
    return {"cycle": cyc, "self": np.arange(beam), "parent0": np.zeros(beam, np.int64), "mixed": mixed}


def _want(old, parent, lo, hi):
    new = old.copy()
    for j, p in enumerate(parent):
        new[:, j, lo:hi] = old[:, p, lo:hi]
    return new


@pytest.fixture(scope="module")
def caches():
    """(beam, d) -> K, V u16 [L][beam + 1][CTX][d], made once and never written"""
    made = {}

    def get(beam, d):
        if (beam, d) not in made:
            rng = np.random.default_rng([beam, d, 77])
            made[beam, d] = tuple(_random_f16_bits(rng, (L, beam + 1, CTX, d)) for _ in range(2))
            for a in made[beam, d]:
                a.setflags(write=False)
        return made[beam, d]
    return get


@pytest.mark.parametrize("d", [384, 1280])
@pytest.mark.parametrize("beam", [2, 5, 8])
def test_kv_reorder_every_slot_in_flight(lib, caches, beam, d):
    old_k, old_v = caches(beam, d)
    for name, parent in _tables(beam).items():
        for npos in (1, 2, 3):                               # P = 1: step_u positions of history, less the one the step counted already
            for done in (0, 1):
                new_k, new_v = _reorder(lib, old_k, old_v, parent, [npos], [done], 1, beam, 1, CTX, d)
                for what, old, new in (("K", old_k, new_k), ("V", old_v, new_v)):
                    want = old if done else _want(old, parent, 0, npos)
                    assert _biteq(new, want), (name, npos, done, what, np.argwhere(new != want)[:4].tolist())
                    if name == "self":
                        assert _biteq(new, old)


@pytest.mark.parametrize("d", [384, 1280])
@pytest.mark.parametrize("beam", [2, 5, 8])
def test_kv_reorder_from_every_slot_in_flight(lib, caches, beam, d):
    from wis_hip._lib import DevBuf, check
    old_k, old_v = caches(beam, d)
    plen = 7                                                 # the prompt's positions 0 .. 6 never move
    for name, parent in _tables(beam).items():
        for n in (1, 2, 3):                                  # positions [plen, plen + n) move: step_u = n + 1
            for done in (0, 1):
                dk, dv = DevBuf.from_numpy(old_k), DevBuf.from_numpy(old_v)
                ctl = [DevBuf.from_numpy(_i32(a)) for a in (parent, [n + 1], [done], [plen])]
                check(lib.wis_op_kv_reorder_from(0, dk.ptr, dv.ptr, (beam + 1) * CTX * d, L, *[c.ptr for c in ctl], 1, beam, CTX, d))
                for what, old, new in (("K", old_k, dk.to_numpy(np.uint16, old_k.shape)), ("V", old_v, dv.to_numpy(np.uint16, old_v.shape))):
                    want = old if done else _want(old, parent, plen, plen + n)
                    assert _biteq(new, want), (name, n, done, what, np.argwhere(new != want)[:4].tolist())


@pytest.mark.parametrize("d", [384, 1280])
@pytest.mark.parametrize("beam", [2, 5, 8])
def test_kv_gather_every_slot_in_flight(lib, caches, beam, d):
    """positions before the window by the `base` table, the window's by one table per step: every pairing of the four tables, so a position where
    every slot keeps its row (skipped whole) stands next to one where all move"""
    old_k, old_v = caches(beam, d)
    tabs = _tables(beam)
    for bname, base in tabs.items():
        for pname, step_tab in tabs.items():
            for w0, nwin in ((1, 1), (1, 2), (2, 1)):        # one to three history positions
                vs = np.full(VS_INTS, beam, np.int32)        # (entries beyond nwin / beam name the spare slot: never to be used)
                vs[0], vs[VS_NWIN] = 0, nwin
                vs[VS_BASE:VS_BASE + beam] = base
                path = np.stack([step_tab if u == 0 else tabs["cycle"] for u in range(nwin)], axis=1)      # [beam][nwin]
                for j in range(beam):
                    vs[VS_PATH + VS_PATH_W * j:VS_PATH + VS_PATH_W * j + nwin] = path[j]
                for done in (0, 1, 2):                       # 1: finished inside the window, nothing moves; 2: parked, the window's steps stand
                    new_k, new_v = _gather(lib, old_k, old_v, vs, done, beam, w0, CTX, d)
                    for what, old, new in (("K", old_k, new_k), ("V", old_v, new_v)):
                        want = old.copy()
                        if done != 1:
                            want = _want(want, base, 0, w0)
                            for u in range(nwin):
                                want[:, :beam, w0 + u] = old[:, path[:, u], w0 + u]
                        assert _biteq(new, want), (bname, pname, w0, nwin, done, what, np.argwhere(new != want)[:4].tolist())
