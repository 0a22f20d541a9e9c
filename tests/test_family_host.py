"""The host numerics of a problem family (csrc/cfs_family.cpp), without a GPU: tests/native/family_check.cpp is built with g++, the
way oracle/Makefile uses gcc, and run as a child process on the recorded cases of tests/golden/family_host_*.

1. Bit for bit what cfs_api.hip computed before the numerics moved out of it (tests/family_cases.py makes the cases,
   tests/tools/record_family_host.py says how they were recorded).  g++ and the library's own host compiler agree in every bit of
   every case here, so the program is built with g++.
2. Properties of the same numbers, each against a bound the code or the project already states.
"""
import json
import os
import shutil
import subprocess
from fractions import Fraction

import numpy as np
import pytest

from motionplanning_5d_m_amd import sysinfo
import family_cases as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
with open(os.path.join(GOLDEN, "family_host_refusals.json")) as _f:
    REFUSALS = json.load(_f)
RECORDED = sorted(f[len("family_host_"):-len("_in.npy")] for f in os.listdir(GOLDEN) if f.startswith("family_host_") and f.endswith("_in.npy"))


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    cxx = shutil.which("g++")
    assert cxx, "g++ is needed to build tests/native/family_check.cpp"
    exe = str(tmp_path_factory.mktemp("family") / "family_check")
    subprocess.run([cxx, "-O3", "-std=c++17", "-Wall", "-Wextra", "-o", exe, os.path.join(ROOT, "tests", "native", "family_check.cpp"),
                    os.path.join(ROOT, "motionplanning_5d_m_amd", "csrc", "cfs_family.cpp")], check=True)
    return exe


def _case(name):
    a = np.load(os.path.join(GOLDEN, f"family_host_{name}_in.npy"))
    return R.OPS[int(a[0])], a[1:]


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def test_every_case_of_the_recorder_is_recorded():
    assert RECORDED == sorted(R.cases())


@pytest.mark.parametrize("name", RECORDED)
def test_recorded_numbers_bit_for_bit(program, name):
    op, data = _case(name)
    got, refused = R.run(program, op, data)
    if name.startswith("refuse_"):
        assert refused == REFUSALS[name] and got.size == 0
        return
    want = np.load(os.path.join(GOLDEN, f"family_host_{name}.npy"))
    assert refused is None and got.shape == want.shape
    assert np.array_equal(_bits(got), _bits(want)), np.flatnonzero(_bits(got) != _bits(want))[:8]


def test_the_cases_are_what_their_names_say():
    for case in (1, 2, 3):
        nj, H, dt = R.SHAPES[case]
        _, a = _case(f"create_{case}_cfs")
        assert (a[0], a[1], a[3]) == (nj, H, dt) and a[4] == 1 and a[5] == 1
        QQ = a[6:6 + (H * nj) ** 2].reshape(H * nj, H * nj, order="F")
        assert np.array_equal(QQ, QQ.T) == (case != 2)
    w = _case("weights_2_alpha")[1]
    assert w[4] != 0 and w[5] != w[6]                                   # q_cross, w_stage != w_terminal
    Rblk = w[8 + 18:8 + 27].reshape(3, 3, order="F")
    assert not np.array_equal(Rblk, Rblk.T)
    _, a = _case("cost_2_dense")
    Qaug = a[3:].reshape(24, 24, order="F")
    assert not np.array_equal(Qaug, Qaug.T) and np.count_nonzero(Qaug) > 500


# ---- poses ------------------------------------------------------------------------------------------------------------------
def _poses_out(name):
    g = np.load(os.path.join(GOLDEN, f"family_host_{name}.npy"))
    inv, frame, itv, turn = g[:36].reshape(3, 3, 4), g[36:40], g[40:40 + 72].reshape(3, 24), g[112:]
    return inv, frame, itv, turn


def test_identity_pose_inverts_to_the_identity_with_plus_zero():
    inv, frame, itv, turn = _poses_out("poses_identity")
    want = np.hstack([np.eye(3), np.zeros((3, 1))])
    for k in range(3):
        assert np.array_equal(_bits(inv[k]), _bits(want))               # +0 translation, not -0
    assert np.all(itv[:, 0] == 0) and np.all(itv[:, 23] == 0) and list(turn) == [-1, 0]
    assert np.array_equal(frame[:3], (np.array([0.1, -0.2, 0.0]) + np.array([0.5, 0.3, 0.4])) / 2.0)    # centre of the box of family_cases


def test_turned_pose_inverse_and_interval():
    _, a = _case("poses_turn")
    T = a[-36:].reshape(3, 3, 4)
    inv, frame, itv, turn = _poses_out("poses_turn")
    for k in range(3):
        M = np.vstack([T[k], [0, 0, 0, 1]]) @ np.vstack([inv[k], [0, 0, 0, 1]])
        assert np.abs(M - np.eye(4)).max() < 1e-15 * 8
    assert list(itv[:, 0]) == [0, 1, 1] and list(turn) == [-1, 0]
    assert abs(itv[1, 4] - 0.3) < 1e-15 and abs(itv[2, 4] - 0.2) < 1e-14      # theta of 0 -> 0.3 and of 0.3 -> 0.5 about one axis
    assert np.abs(itv[1, 1:4] - np.array([1, 2, 3]) / np.sqrt(14)).max() < 1e-15 * 8


def test_equal_consecutive_poses_are_held_and_a_quarter_turn_is_reported():
    _, _, itv, turn = _poses_out("poses_held")
    assert list(itv[:, 0]) == [0, 0, 1] and itv[1, 23] == 0 and list(turn) == [-1, 0]
    _, _, itv, turn = _poses_out("poses_quarter")
    assert list(turn) == [0, 1] and itv[1, 0] == 0


# ---- lambda_max_upper -------------------------------------------------------------------------------------------------------
def _sym_matrices():
    out = []
    for case in (1, 2, 3):
        QQ = R.sys_info(case).QQ
        out.append(0.5 * (QQ + QQ.T))
    out.append(np.eye(5))
    return out


@pytest.mark.parametrize("k", range(4))
def test_lambda_max_upper_brackets_the_largest_eigenvalue(program, k):
    """numpy's largest eigenvalue <= bound <= that x n^(1/32) x 1.001, the function's own comment.  Rounding allowance: the
    five squarings of an n x n matrix, the norms and exp / log each lose a few ulp, and the 32nd root divides the relative error of the
    powers by 32: 64 ulp covers them with room, and is 1.4e-14 against the 1e-3 the 1.001 factor adds on purpose."""
    A = _sym_matrices()[k]
    n = A.shape[0]
    got, refused = R.run(program, "lmax", np.concatenate([[n], R.f_order(A)]))
    assert refused is None
    lam = np.linalg.eigvalsh(A).max()
    ulp = 64 * np.finfo(float).eps
    assert lam * (1 - ulp) <= got[0] <= lam * n ** (1 / 32) * 1.001 * (1 + ulp), (lam, got[0])


# ---- spd_inverse ------------------------------------------------------------------------------------------------------------
def _exact_inverse(A):
    n = A.shape[0]
    M = [[Fraction(float(A[i, j])) for j in range(n)] + [Fraction(int(i == j)) for j in range(n)] for i in range(n)]
    for c in range(n):
        p = next(r for r in range(c, n) if M[r][c] != 0)
        M[c], M[p] = M[p], M[c]
        M[c] = [v / M[c][c] for v in M[c]]
        for r in range(n):
            if r != c and M[r][c] != 0:
                M[r] = [a - M[r][c] * b for a, b in zip(M[r], M[c])]
    return [[M[i][n + j] for j in range(n)] for i in range(n)]


@pytest.mark.parametrize("k", range(4))
def test_spd_inverse_is_symmetric_and_no_worse_than_numpy(program, k):
    """It accumulates in 80-bit and rounds once per entry: against the exact inverse (fractions.Fraction) its largest entry error is
    at most that of numpy.linalg.inv on the same matrix; where numpy's error is 0, one ulp of that entry is allowed."""
    A = _sym_matrices()[k]
    n = A.shape[0]
    assert n <= 12
    got, refused = R.run(program, "inv", np.concatenate([[n], R.f_order(A)]))
    assert refused is None
    inv = got.reshape(n, n, order="F")
    assert np.array_equal(_bits(inv), _bits(inv.T))
    exact = _exact_inverse(A)
    ref = np.linalg.inv(A)
    err = lambda M: max(abs(Fraction(float(M[i, j])) - exact[i][j]) for i in range(n) for j in range(n))   # noqa: E731
    e_got, e_np = err(inv), err(ref)
    print(f"n={n}: spd_inverse {float(e_got):.3e}  numpy {float(e_np):.3e}")
    if e_np == 0:
        assert all(abs(Fraction(float(inv[i, j])) - exact[i][j]) <= Fraction(float(np.spacing(abs(float(exact[i][j]))))) for i in range(n) for j in range(n))
    else:
        assert e_got <= e_np


# ---- QQ, alpha and the state-cost terms against the Python builder -------------------------------------------------------------
@pytest.mark.parametrize("case", [1, 2, 3])
def test_weights_against_build_sys_info(case):
    """tolerances of CFSBatch._weights_match (QQ, alpha) and of tests/test_gpu_batch.py (ff, caug)"""
    nj, H, dt = R.SHAPES[case]
    nn = H * nj
    s = R.sys_info(case)
    g = np.load(os.path.join(GOLDEN, f"family_host_weights_{case}_alpha.npy"))
    QQ, alpha = g[:nn * nn].reshape(nn, nn, order="F"), g[nn * nn + 36]
    F1, F2 = (g[nn * nn + 37 + k * nn * nj:][:nn * nj].reshape(nn, nj, order="F") for k in (0, 1))
    Cq = g[nn * nn + 37 + 2 * nn * nj:].reshape(2 * nj, 2 * nj, order="F")
    assert np.abs(QQ - s.QQ).max() <= 1e-12 * np.abs(s.QQ).max()
    assert abs(alpha - s.alpha) <= 1e-9 * abs(s.alpha)
    x0 = 0.3 + 0.1 * np.arange(nj)
    xg = -0.2 + 0.15 * np.arange(nj)
    ff, caug = sysinfo.cost_terms(s.Aaug, s.Baug, s.Qaug_state, np.concatenate([x0, np.zeros(nj)]), xg, H, nj)
    np.testing.assert_allclose(F1 @ x0 - F2 @ xg, ff, rtol=1e-11, atol=1e-9)
    z = np.concatenate([x0, xg])
    np.testing.assert_allclose(z @ Cq @ z, caug, rtol=1e-11, atol=1e-9)
    # the terms of the weights are the terms of the Qaug they assemble, bit for bit
    c = np.load(os.path.join(GOLDEN, f"family_host_cost_{case}.npy"))
    assert np.array_equal(_bits(c), _bits(g[nn * nn + 37:]))
