"""The integer arithmetic of the fused solver's work-item decode (csrc/cfs_fused.hip: rcp31, rcp_div and the range selection of the
shifted-pose loop), restated in numpy and compared with `//` and with the chain of range tests it replaced.  rcp_div(e, rcp31(d)) is
umulhi(2 e, floor(2^31 / d) + 1); it must equal e // d whenever e * d < 2^31, d = 1 included.  launch_fused_tier refuses plans
outside that range, and an item index is below nj * lin_w * nseg <= 20 480 (a tile's base distances fit 160 KB of LDS)."""
import numpy as np
import pytest


def rcp31(d):
    return (0x80000000 // d) + 1


def rcp_div(e, rc):
    return ((((e.astype(np.uint64) << np.uint64(1)) & np.uint64(0xffffffff)) * np.uint64(rc)) >> np.uint64(32)).astype(np.int64)


def test_rcp_div_is_floor_division_over_the_whole_range():
    e_all = np.arange(0, 4 * 20480, dtype=np.int64)
    for d in list(range(1, 2049)) + [4095, 4096, 5000, 8191, 10240, 16384, 20480]:
        e = e_all[e_all * d < 2**31]
        np.testing.assert_array_equal(rcp_div(e, rcp31(d)), e // d, err_msg=f"d = {d}")
    for d in (1, 2, 3, 7, 255):                            # up to the bound itself
        e = np.arange(max(0, (2**31 - 1) // d - 100000), (2**31 - 1) // d + 1, dtype=np.int64)
        np.testing.assert_array_equal(rcp_div(e, rcp31(d)), e // d, err_msg=f"d = {d}, e at the bound")


@pytest.mark.parametrize("nj", [2, 3, 4, 5, 6])
def test_range_selection_equals_the_chain_of_range_tests(nj):
    rng = np.random.default_rng(nj)
    for _ in range(200):
        cnt = rng.integers(0, 224, nj) * (rng.random(nj) < 0.7)             # empty ranges included
        offs = np.concatenate([[0], np.cumsum(cnt * 2 * np.arange(1, nj + 1))])
        e = np.arange(offs[-1])
        k_old, ent_old, v_old = np.ones_like(e), np.zeros_like(e), np.ones_like(e)
        for kk in range(1, nj + 1):                                          # before: e in [offs[kk-1], offs[kk])
            m = (e >= offs[kk - 1]) & (e < offs[kk])
            r = e - offs[kk - 1]
            k_old[m], ent_old[m] = kk, r[m] // (2 * kk)
            v_old[m] = r[m] - ent_old[m] * 2 * kk + 1
        k1, lo, rc = np.ones_like(e), np.zeros_like(e), np.full(e.shape, 0x80000001, dtype=np.uint64)
        for kk in range(2, nj + 1):                                          # now: the last range that starts at or before e
            m = e >= offs[kk - 1]
            k1[m], lo[m], rc[m] = kk, offs[kk - 1], (0x100000000 // (2 * kk)) + 1
        r = e - lo
        ent = ((r.astype(np.uint64) * rc) >> np.uint64(32)).astype(np.int64)
        np.testing.assert_array_equal(k1, k_old)
        np.testing.assert_array_equal(ent, ent_old)
        np.testing.assert_array_equal(r - ent * 2 * k1 + 1, v_old)
