"""The fused solver's whole-CU tier (w1) and its variants against the references.

launch_fused sends every solve whose shape fits half a CU to w2m (CFS) or w2s (PSGCFS), so the suite's default solves reach w1
only at the very largest shapes, in the default variant, on the 256-row kernels.  Every handle here is therefore built twice: with
the default tier and with debug_options(tier_w1=True), on shapes that test_tier_query.py proves run a half-CU tier by default
(tier_shapes.py) -- and one shape that is w1 with no flag at all.  w1 differs from the half-CU tiers where a solver goes wrong: 64
register-resident inverse-Gram columns (24 / 16 there), hence where PRow's tail path begins; the split of Y between LDS and global
memory and so y_combine's summation order; the linearisation tile width; the register budget; its own LDS plan.

The bars are those of the tests whose checks are repeated here (test_gpu_first_iteration.py, test_gpu_chaos.py, test_gpu_parity.py,
test_gpu_jacobian.py and the variant files); DESIGN.md's "Tiers" bullet records what these tests print.  Measured on an MI355X:
the linearisations of w1 and of the default tier are bit-identical on all three batches; u of the QP piece on w1 is within 3.6e-11 of
the oracle's (no arbitration needed), KKT residuals below 2.1e-11; un-kinked steps of whole solves within 3.9e-9 (bar 1e-8).
"""
import concurrent.futures as cf
import copy
from types import SimpleNamespace

import numpy as np
import pytest

import soft_reference as S
import test_gpu_jacobian as TJ
import test_gpu_limits as TL
import test_gpu_moving as TM
import test_gpu_soft as TS
from helpers import (KINK, ONE_STEP_TOL, check_one_step_at_a_time, device_lambda_to_rows, kkt_certificate, oracle_obs,
                     truth_on_active_set)
from motionplanning_5d_m_amd import workloads
from motionplanning_5d_m_amd.solvers import fused_tier
from test_gpu_first_iteration import _dense_qp
from test_gpu_limits import c3_256, c3_ref  # noqa: F401  (fixtures of the limits tests, for their bodies run on w1)
from test_gpu_moving import c3m  # noqa: F401
from tier_shapes import BATCH_SHAPES, DEFAULT_W1_NJ_H, DEFAULT_W1_NOBS, SINGLE_SHAPES

pytestmark = pytest.mark.gpu

TOL_RAD = 1e-7            # test_gpu_parity.py's
FIELDS = ("u", "x_", "cost_all", "e_cost_all", "e_u_all", "iter_O", "total_iter", "status")
S96_SEED, S160_SEED, S256_SEED, W1D_SEED = 3, 20260118, 2, 20260119
W1 = dict(tier_w1=True)


# ---- the batches ------------------------------------------------------------------------------------------------------------------
def oracle_dist_fn(O):
    """workloads.config3's obstacle rejection through the oracle: the batches are the same on every machine"""
    orobot = O.robotproperty2("M200i")
    return lambda rb, th, ob: np.array([[O.dist_arm(orobot, t, np.stack([o[:3], o[3:]], axis=1))[0] for o in ob] for t in th])


def make_s96(pkg, B=16, H=16, seed=S96_SEED):
    """M200i, 5 joints, H 16, two line obstacles across the sweep (build_sys_info with test_other_joint_counts' weights); starts and
    goals jittered by U(-0.1, 0.1) rad"""
    robot = pkg.robotproperty2("M200i")
    x0 = np.array([0.7825, 0.0284, 0.2172, 0.1444, -1.1779])
    xg = x0 * np.array([-1.0, 1, 1, 1, 1])
    s = pkg.build_sys_info(robot, 5, H, x0, xg, pkg.line_reference(x0, xg, H), Qp=np.diag([10.0, 10, 1, 1, 1]), Qv=np.diag([10.0, 10, 1, 1, 1]),
                           Rblk=np.eye(5) * 2, cR=50.0, lim=np.ones(5), max_input_blk=np.ones(5), epsilon_O=0.1, MAX_O_ITER=12)
    rng = np.random.default_rng(seed)
    x0b, xgb = x0 + rng.uniform(-0.1, 0.1, (B, 5)), xg + rng.uniform(-0.1, 0.1, (B, 5))
    noise = 0.1 * rng.standard_normal((B, 12, H * 5))
    x_init, xR1, ff, caug = workloads._batch_terms(s, x0b, xgb)
    ob = [pkg.cylinder((3700, 8500, 1), (3700, 8500, 1200), 0.15, 0.2), pkg.cylinder((3600, 8900, 1), (3600, 8900, 700), 0.15, 0.2)]
    obs = np.ascontiguousarray(np.broadcast_to(pkg.obs_to_array(ob), (B, 2, 6)))
    return s, SimpleNamespace(B=B, nobs=2, x0=x0b, xg=xgb, x_init=x_init, xR1=xR1, ff=ff, caug=caug, obs=obs, noise=noise,
                              margin_cfs=np.full(2, 0.12), margin_psg=np.full(2, 0.08))    # (oracle, CFS: 14 of 16 converge, 2 end QP_INFEASIBLE)


def make_shape(pkg, O, route_wp, tag):
    if tag == "s96":
        return make_s96(pkg)
    if tag == "s160":
        return workloads.config3(oracle_dist_fn(O), B=48, nobs=3, seed=S160_SEED)
    if tag == "s256":
        return workloads.config4(route_wp, B=32, seed=S256_SEED)
    assert tag in ("w1d CFS", "w1d PSGCFS")              # the 160-row shapes that are w1 by default: config 3 with more obstacles
    return workloads.config3(oracle_dist_fn(O), B=8, nobs=DEFAULT_W1_NOBS[tag[4:]], seed=W1D_SEED)


@pytest.fixture(scope="module")
def shapes(gpu, O, route_wp):
    cache = {}

    def get(tag):
        if tag not in cache:
            s, bt = make_shape(gpu, O, route_wp, tag)
            if tag in BATCH_SHAPES:
                assert (s.njoint, s.H, bt.nobs, bt.obs.shape[1]) == BATCH_SHAPES[tag][:3] + (bt.nobs,)      # the table test_tier_query.py proves half-CU
            cache[tag] = (s, bt)
        return cache[tag]
    return get


def _handle(gpu, s, bt, mode, tier, n=None, **kw):
    margin = bt.margin_cfs if mode == "CFS" else bt.margin_psg
    h = gpu.CFSBatch(s, bt.nobs, margin, mode=mode, max_batch=bt.B if n is None else n, **kw)
    if tier == "w1":
        h.debug_options(**W1)
    return h


def _solve(gpu, s, bt, mode, tier, idx=None, dbg=None, log=False, **kw):
    idx = np.arange(bt.B) if idx is None else np.asarray(idx)
    h = _handle(gpu, s, bt, mode, "default", n=len(idx), **kw)
    h.debug_options(**dict(W1 if tier == "w1" else {}, **(dbg or {})))
    if log:
        h.log_u(True)
    nz = bt.noise[idx] if (mode == "PSGCFS" and bt.noise is not None) else None
    r = h.solve(bt.x_init[idx], bt.xR1[idx], bt.ff[idx], bt.caug[idx], bt.obs[idx], noise=nz)
    r.ulog = h.read_u_log(len(idx)) if log else None
    h.close()
    return r


def _same(a, b, fields=FIELDS, msg=""):
    for f in fields:
        np.testing.assert_array_equal(getattr(a, f), getattr(b, f), err_msg=f"{msg} {f}")


def _oracle_linearisation(O, s, bt, mode):
    margin = bt.margin_cfs if mode == "CFS" else bt.margin_psg
    robot = O.robotproperty2("M200i")
    B, H, nn = bt.B, s.H, s.H * 5
    dist, lid, grad = np.zeros((B, bt.nobs, H)), np.zeros((B, bt.nobs, H), np.int32), np.zeros((B, bt.nobs, H, 5))
    for b in range(B):
        s2 = SimpleNamespace(**vars(s))
        s2.xR1, s2.robot = bt.xR1[b], robot
        _, _, dist[b], lid[b], grad[b] = O.get_con("M200i", s2, oracle_obs(bt, b, margin), bt.x_init[b], np.zeros(nn), mode=mode, dense=False)
    return dist, lid, grad


BATCH_CASES = [(t, m) for t, v in BATCH_SHAPES.items() for m in v[3]]


# ---- a. the linearisation piece ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("jacobian", ["fd_literal", "analytic"])
@pytest.mark.parametrize("tag", list(BATCH_SHAPES))
def test_linearisation_on_w1(gpu, O, shapes, tag, jacobian):
    s, bt = shapes(tag)
    H, nj = s.H, 5
    o_dist, o_lid, o_grad = _oracle_linearisation(O, s, bt, "CFS")
    for mode in BATCH_SHAPES[tag][3]:                     # the Hessian is a template argument: each solver has its own kernel
        h = _handle(gpu, s, bt, mode, "w1", jacobian=jacobian)
        dist, lid, grad = h.linearize(bt.x_init, bt.obs)
        h.debug_options(no_prune=True, **W1)
        dist_u, lid_u, grad_u = h.linearize(bt.x_init, bt.obs)
        h.close()
        np.testing.assert_array_equal(dist, dist_u)       # pruned == unpruned, bit for bit
        np.testing.assert_array_equal(grad, grad_u)
        np.testing.assert_array_equal(lid, lid_u)
        assert np.abs(dist - o_dist).max() < 1e-14
        np.testing.assert_array_equal(lid, o_lid)
        if jacobian == "fd_literal":
            assert np.abs(grad - o_grad).max() < 2e-9
        else:                                             # cfs_dist_arm_grad's numbers (checked against derivest there), bit for bit
            th = bt.x_init.reshape(bt.B, H, 2 * nj)[:, :, :nj]
            for b in range(bt.B):
                d1, l1, g1 = gpu.dist_arm(s.robot, th[b], bt.obs[b], want_grad=True)
                np.testing.assert_array_equal(dist[b], d1.T)
                np.testing.assert_array_equal(lid[b], l1.T)
                np.testing.assert_array_equal(grad[b], g1.transpose(1, 0, 2))
        hd = _handle(gpu, s, bt, mode, "default", jacobian=jacobian)
        dd, ld, gd = hd.linearize(bt.x_init, bt.obs)
        hd.close()
        np.testing.assert_array_equal(lid, ld)
        print(f"[{tag} {mode} {jacobian}] w1 against the default tier: dist {'bit-identical' if np.array_equal(dist, dd) else f'max diff {np.abs(dist - dd).max():.1e}'}, "
              f"grad {'bit-identical' if np.array_equal(grad, gd) else f'max diff {np.abs(grad - gd).max():.1e}'}; "
              f"w1 against the oracle: dist {np.abs(dist - o_dist).max():.1e}" + (f", grad {np.abs(grad - o_grad).max():.1e}" if jacobian == "fd_literal" else ""))


# ---- b. the QP piece --------------------------------------------------------------------------------------------------------------
def _lin(s, bt, mode):
    return bt.ff if mode == "CFS" else -s.alpha * (bt.ff + 10.0 * bt.noise[:, 0] / 2.0)      # PSGCFS_FANUC.m:109 at u = 0, iter_O = 1


def _against_oracle(O, G, g0, A, rhs, u_dev, tag):
    """u of one QP against the oracle's; beyond 1e-9 the extended-precision solution on the oracle's active set arbitrates.
    Returns (relative error against the oracle, oracle status, number of active rows of the oracle)"""
    xo, lo, _, sto, _ = O.qp_solve(G, g0, A, rhs)
    if sto:
        return None, sto, 0
    sc = max(np.abs(xo).max(), 1e-300)
    rel = np.abs(u_dev - xo).max() / sc
    if rel > 1e-9:
        xt, lt = truth_on_active_set(G, g0, A, rhs, np.nonzero(lo > 0)[0])
        assert lt.min() > -1e-9 * max(lt.max(), 1.0) and (rhs - A @ xt).min() > -1e-9       # the oracle's active set is optimal
        sc = np.abs(xt).max()
        e_dev, e_orc = np.abs(u_dev - xt).max() / sc, np.abs(xo - xt).max() / sc
        assert e_dev <= max(1e-9, 4.0 * e_orc), (tag, e_dev, e_orc)
    return rel, 0, int((lo > 0).sum())


def _kkt(s, bt, mode, h, lin, u, lam, x_, rows=None):
    """KKT residuals of device answers from the device's own multipliers, on the rows the same handle builds"""
    nn, H = s.H * 5, s.H
    n = u.shape[0]
    A, rhs = h.get_con(x_, np.zeros((n, nn)), bt.xR1[:n] if rows is None else bt.xR1[rows], bt.obs[:n] if rows is None else bt.obs[rows])
    if mode == "CFS":
        eye = np.broadcast_to(np.eye(nn), (n, nn, nn))
        A = np.concatenate([A, eye, -eye], axis=1)
        rhs = np.concatenate([rhs, np.broadcast_to(s.MAX_input, (n, nn)), np.broadcast_to(s.MAX_input, (n, nn))], axis=1)
    Gm = 0.5 * (s.QQ + s.QQ.T) if mode == "CFS" else np.eye(nn)
    g0 = lin if mode == "CFS" else -lin
    return np.array(kkt_certificate(Gm, g0, A, rhs, u, device_lambda_to_rows(lam, bt.nobs, H, 5, mode == "CFS")))


@pytest.mark.parametrize("tag,mode", BATCH_CASES)
def test_qp_piece_on_w1(gpu, O, shapes, tag, mode):
    s, bt = shapes(tag)
    B, nn = bt.B, s.H * 5
    margin = bt.margin_cfs if mode == "CFS" else bt.margin_psg
    noise = bt.noise if (mode == "PSGCFS" and bt.noise is not None) else None
    s1 = copy.copy(s)
    s1.MAX_O_ITER = 1
    h1, hd = _handle(gpu, s1, bt, mode, "w1"), _handle(gpu, s1, bt, mode, "default")
    lin, z = _lin(s, bt, mode), np.zeros((B, nn))

    # the piece == a whole w1 solve with MAX_O_ITER = 1, bit for bit (own linearisation)
    dist, _, grad = h1.linearize(bt.x_init, bt.obs)
    u_qp, lam, it, st = h1.qp(lin, z, bt.xR1, dist, grad)
    whole = h1.solve(bt.x_init, bt.xR1, bt.ff, bt.caug, bt.obs, noise=noise)
    solved = st == 0
    assert np.array_equal(solved, whole.status == 1) and np.array_equal(st == 2, whole.status == 2) and not (st == 3).any()
    np.testing.assert_array_equal(u_qp[solved], whole.u[solved])
    np.testing.assert_array_equal(it, whole.total_iter)

    # both tiers and the oracle on the oracle's linearisation: the same split, u to 1e-9 (or arbitrated)
    o_dist, _, o_grad = _oracle_linearisation(O, s, bt, mode)
    u1, _, _, st1 = h1.qp(lin, z, bt.xR1, o_dist, o_grad)
    ud, _, _, std = hd.qp(lin, z, bt.xR1, o_dist, o_grad)
    np.testing.assert_array_equal(st1, std)
    assert set(np.unique(st1)) <= {0, 2}
    rel = np.zeros(B)
    for b in range(B):
        r, sto, _ = _against_oracle(O, *_dense_qp(s, bt, mode, b, O, margin), u1[b], (tag, mode, b))
        assert (sto == 0) == (st1[b] == 0) and (sto == 2) == (st1[b] == 2), (b, sto, st1[b])
        rel[b] = r or 0.0
    assert np.array_equal(st1 == 0, solved)
    tiers = "bit-identical" if np.array_equal(u1[solved], ud[solved]) else f"max rel diff {(np.abs(u1 - ud).max(axis=1)[solved] / np.abs(ud).max(axis=1)[solved]).max():.1e}"

    # KKT certificate of the w1 answers from w1's own multipliers
    cert = _kkt(s, bt, mode, h1, lin, u_qp, lam, bt.x_init)[:, solved]
    print(f"[{tag} {mode} w1] solved {solved.sum()}/{B}; rel u err vs oracle: median {np.median(rel[solved]):.1e} max {rel[solved].max():.1e} "
          f"({int((rel > 1e-9).sum())} arbitrated); w1 against the default tier: {tiers}; KKT: stationarity {cert[0].max():.1e} "
          f"primal {cert[1].max():.1e} dual {cert[2].max():.1e} complementarity {cert[3].max():.1e}")
    assert solved.any()
    assert cert.max() <= 1e-9
    h1.close()
    hd.close()


# ---- c. QPs with many active rows: PRow's register / tail boundary (64 columns on w1, 24 on w2m) ---------------------------------
# CFS QPs of problem MANY_B of s160 (the oracle's linearisation at x_init) with ff scaled by the factor: (factor, active rows of the
# oracle's optimum, input bounds among them), chosen on the CPU with O.qp_solve.  Scaling ff binds few input bounds here (at most 35
# of the 300 on any problem of the batch, up to a factor of 3000): the velocity limits bind first, so the active rows counted are of
# all kinds, which is what PRow's boundary sees.  The smallest multiplier of each optimum is > 8e-7 of the largest: the counts are
# not a matter of rounding.
MANY_B = 20
MANY_ACTIVE = [(140.0, 63, 5), (350.0, 65, 5), (2000.0, 106, 11)]


@pytest.mark.parametrize("tier", ["default", "w1"])
def test_qp_piece_with_many_active_rows(gpu, O, shapes, tier):
    s, bt = shapes("s160")
    b, nn, n = MANY_B, s.H * 5, len(MANY_ACTIVE)
    counts = [c for _, c, _ in MANY_ACTIVE]
    assert any(60 <= c <= 63 for c in counts) and any(65 <= c <= 70 for c in counts) and any(c > 100 for c in counts)
    o_dist, _, o_grad = _oracle_linearisation(O, s, bt, "CFS")
    G, _, A, rhs = _dense_qp(s, bt, "CFS", b, O, bt.margin_cfs)
    lin = np.stack([f * bt.ff[b] for f, _, _ in MANY_ACTIVE])
    rep = lambda a: np.ascontiguousarray(np.broadcast_to(a[b], (n,) + a[b].shape))   # noqa: E731
    h = _handle(gpu, s, bt, "CFS", tier, n=n)
    u, lam, it, st = h.qp(lin, np.zeros((n, nn)), rep(bt.xR1), rep(o_dist), rep(o_grad))
    assert (st == 0).all(), st
    for k, (f, count, bounds) in enumerate(MANY_ACTIVE):
        rel, sto, act = _against_oracle(O, G, lin[k], A, rhs, u[k], (tier, f))
        assert sto == 0 and act == count, (f, sto, act)
        dev_act = int((lam[k] > 0).sum())
        print(f"[s160 CFS {tier}] ff x {f:g}: oracle {count} active rows ({bounds} input bounds), device {dev_act} in {int(it[k])} steps, "
              f"rel u err {rel:.1e}")
    # the certificate needs the rows of the oracle's linearisation: they are the dense QP's
    lam_rows = device_lambda_to_rows(lam, bt.nobs, s.H, 5, True)
    cert = np.array(kkt_certificate(G, lin, np.broadcast_to(A, (n,) + A.shape), np.broadcast_to(rhs, (n,) + rhs.shape), u, lam_rows))
    print(f"[s160 CFS {tier}] KKT: stationarity {cert[0].max():.1e} primal {cert[1].max():.1e} dual {cert[2].max():.1e} complementarity {cert[3].max():.1e}")
    assert cert.max() <= 1e-9
    h.close()


# ---- d. whole solves, one outer iteration at a time ---------------------------------------------------------------------------------
@pytest.mark.parametrize("tag,mode", BATCH_CASES)
def test_whole_solves_on_w1_one_step_at_a_time(gpu, O, shapes, tag, mode):
    """Every problem of the batch.  The seeds were chosen on the CPU so that the oracle's own iterates (O.optimizer(...,
    history=True)) leave at least 0.6 of the steps un-kinked.  Share found, oracle's iterates: s96 0.87 (CFS) / 0.90 (PSGCFS),
    s160 0.81 / 0.99, s256 0.60 (config 4's routes kink often: 0.52-0.60 over 26 seeds, seed 2 is the best of them).  The device's
    own steps must be un-kinked to 0.6 as well where the oracle's share leaves room, and to the checker's 0.4 on s256."""
    s, bt = shapes(tag)
    r = check_one_step_at_a_time(gpu, O, s, bt, mode, np.arange(bt.B), tag, tier_w1=True, min_unkinked=0.4 if tag == "s256" else 0.6)
    assert r["problems"] == bt.B and r["steps"] >= bt.B


# ---- e. the variants' reference comparisons on w1 -------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["CFS", "PSGCFS"])
def test_soft_qp_on_w1_one_step_at_a_time(gpu, O, c3, mode):
    TS.check_infeasible_problems_one_step_at_a_time(gpu, O, c3, mode, "w1", n=48)


def test_limits_get_con_and_qp_on_w1(gpu, O, c3_256):  # noqa: F811
    TL.check_get_con_and_qp(gpu, O, c3_256, "w1")


@pytest.mark.parametrize("mode,tol", [("CFS", 1e-7), ("PSGCFS", 1e-5)])
def test_limits_whole_solves_on_w1(gpu, c3_256, c3_ref, mode, tol):  # noqa: F811
    TL.check_whole_solves(gpu, c3_256, c3_ref, mode, tol, "w1")


def test_moving_linearize_and_get_con_on_w1(gpu, O, c3m):  # noqa: F811
    TM.check_linearize_and_get_con(gpu, O, c3m, "w1")


@pytest.mark.parametrize("mode,tol", [("CFS", 1e-7), ("PSGCFS", 1e-5)])
def test_moving_whole_solves_on_w1(gpu, O, c3m, mode, tol):  # noqa: F811
    TM.check_whole_solves(gpu, O, c3m, mode, tol, "w1")


@pytest.mark.parametrize("mode", ["CFS", "PSGCFS"])
def test_analytic_every_iteration_on_w1(gpu, O, c3, mode):
    TJ.check_every_iteration(gpu, O, c3, mode, "w1", idx=np.arange(48))


MU = 1e6
SOFT_STEP_TOL = 1e-7      # test_gpu_soft.py's bar for softened steps


@pytest.mark.parametrize("tier", ["default", "w1"])
def test_analytic_soften_limits_combined_one_step_at_a_time(gpu, O, shapes, tier):
    """analytic Jacobian + soft QP + joint limits in one handle (the asl kernels), CFS on s160: every logged iterate is one oracle QP
    (hard when the oracle solves it, otherwise the soft one: soft_reference.py) on the rows cfs_get_con of the same handle builds at
    the device's previous iterate -- collision rows from the analytic gradient, position rows last."""
    s, bt = shapes("s160")
    H, nj, nn, B = s.H, 5, s.H * 5, bt.B
    lim = workloads.CONFIG3_CELL_LIMITS
    h = _handle(gpu, s, bt, "CFS", tier, jacobian="analytic", on_infeasible="soften", soft_weight=MU, joint_limits=lim)
    h.log_u(True)
    got = h.solve(bt.x_init, bt.xR1, bt.ff, bt.caug, bt.obs)
    ulog = h.read_u_log(B)
    col = S.collision_rows(bt.nobs, H, nj)
    rng = np.random.default_rng(11)
    jobs = [(b, k, ulog[b, k - 2] if k >= 2 else np.zeros(nn), ulog[b, k - 1], 1e-12 * rng.standard_normal(nn))
            for b in range(B) for k in range(1, int(got.iter_O[b]))]

    def rows(b, k, u_prev):                               # (the handle is used from one thread: the device rows are gathered first)
        x_ = bt.x_init[b] if k == 1 else O.rollout(H, nj, s.robot.delta_t, bt.xR1[b], u_prev)
        A, rhs = h.get_con(x_[None], u_prev[None], bt.xR1[b][None], bt.obs[b][None])
        keep = np.isfinite(rhs[0])                        # the cell leaves joints 2 and 5 free: no row for an infinite bound
        return SimpleNamespace(G=s.QQ, g0=bt.ff[b], A=np.vstack([A[0][keep], np.eye(nn), -np.eye(nn)]),
                               b=np.concatenate([rhs[0][keep], s.MAX_input, s.MAX_input]), col=col, box=s.MAX_input)
    qs = [(rows(b, k, up), rows(b, k, up + kick) if k >= 2 else None) for b, k, up, _, kick in jobs]
    h.close()

    def one(a):
        (b, k, _, u_k, _), (q, q2) = jobs[a], qs[a]
        want, soft, viol, st, _ = S.oracle_soft_step(O, q, MU)
        w2, soft2, _, st2, _ = S.oracle_soft_step(O, q2, MU) if q2 is not None else (want, soft, 0, st, 0)
        sc = max(np.abs(u_k).max(), 1e-300)
        err = np.abs(u_k - want).max() / sc if st == 0 else np.inf
        sens = np.abs(w2 - want).max() / sc if (st == 0 and st2 == 0 and soft == soft2) else np.inf
        return err, sens, soft, abs(got.viol_all[b, k - 1] - viol), (got.viol_all[b, k - 1] > 0) == soft

    with cf.ThreadPoolExecutor(16) as ex:
        res = list(ex.map(one, range(len(jobs))))
    err, sens, soft = np.array([r[0] for r in res]), np.array([r[1] for r in res]), np.array([r[2] for r in res])
    dviol = np.array([r[3] for r in res])
    kink = ~(sens <= KINK)
    tol = np.where(soft, SOFT_STEP_TOL, ONE_STEP_TOL)
    print(f"[s160 CFS asl {tier}] {len(jobs)} outer iterations of {B} problems, {int(soft.sum())} softened, {int(kink.sum())} kinked; un-kinked: "
          f"max err {err[~kink].max():.1e}, max |viol - oracle| {dviol[~kink].max():.1e} m; status {np.bincount(got.status, minlength=5)}")
    assert len(jobs) >= B and soft.any()
    assert (~kink).sum() >= 0.6 * len(jobs)
    assert (err[~kink] <= tol[~kink]).all(), [(jobs[a][0], jobs[a][1], err[a]) for a in np.nonzero(~kink & ~(err <= tol))[0]]
    assert (dviol[~kink] <= 1e-9).all()
    assert all(r[4] for r, kk in zip(res, kink) if not kk)                                   # softened exactly where the oracle softens
    assert (err[kink] <= np.maximum(tol[kink], 1e3 * sens[kink])).mean() >= 0.98 if kink.any() else True


# ---- f. bit-for-bit invariants within w1 ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["CFS", "PSGCFS"])
def test_bitwise_invariants_on_w1(gpu, shapes, mode):
    s, bt = shapes("s160")
    base = _solve(gpu, s, bt, mode, "w1", log=False)
    _same(base, _solve(gpu, s, bt, mode, "w1", log=True), msg="u log")                       # logging u changes nothing
    cert_off = _solve(gpu, s, bt, mode, "w1", dbg=dict(no_certificate=True))
    _same(base, cert_off, fields=("status", "iter_O", "u", "x_", "cost_all", "e_u_all"), msg="certificate")    # test_gpu_shortcuts.py's
    assert (base.total_iter <= cert_off.total_iter).all()
    _same(base, _solve(gpu, s, bt, mode, "w1", joint_limits=TL.FAR5), msg="inactive limits")
    _same(base, _solve(gpu, s, bt, mode, "w1", joint_limits=TL.INF5), msg="infinite limits")
    rows = SimpleNamespace(**vars(bt))
    rows.obs = TM._const_rows(bt.obs, s.H)
    _same(base, _solve(gpu, s, rows, mode, "w1", obstacles="per_waypoint"), msg="constant per-waypoint rows")
    half = bt.B // 2                                       # a problem's answer does not depend on the batch it was solved in
    for idx in (np.arange(half), np.arange(half, bt.B)):
        part = _solve(gpu, s, bt, mode, "w1", idx=idx)
        for f in FIELDS:
            np.testing.assert_array_equal(getattr(part, f), getattr(base, f)[idx], err_msg=f"batch split {f}")
    assert (base.status == 2).any() and (base.status <= 1).any()     # both outcomes took part (the certificate ran)


# ---- g. the other joint counts ---------------------------------------------------------------------------------------------------------
def _single(mod, rid, nj, H):
    """(sys_info, obs cell) built by mod = the package or the oracle"""
    robot = mod.robotproperty2(rid)
    if rid == "2L":                                       # test_two_link_arm_long_horizon's problem at main_2L's horizon
        x0, xg = np.zeros(2), np.array([np.pi / 2, 0.0])
        kw = dict(Qp=np.diag([10.0, 1.0]), Qv=np.diag([10.0, 1.0]), Rblk=np.diag([5.0, 4.0]), cR=0.1, lim=np.ones(2), max_input_blk=np.ones(2) * 0.25,
                  epsilon_O=1e-6, MAX_O_ITER=30)
        x_init = np.tile(np.concatenate([x0, np.zeros(2)]), H)
        c = np.array([0.3, 0.3, 0.0])
        ob = [dict(shape="circle", l=np.stack([c, c], axis=1), D=0.05, epsilon=0.05)]
    else:                                                 # test_other_joint_counts' problem
        x0 = np.array([0.7825, 0.0284, 0.2172, 0.1444, -1.1779, 0.3])[:nj]
        xg = x0 * np.array([-1.0, 1, 1, 1, 1, 1])[:nj]
        kw = dict(Qp=np.diag([10.0, 10, 1, 1, 1, 1][:nj]), Qv=np.diag([10.0, 10, 1, 1, 1, 1][:nj]), Rblk=np.eye(nj) * 2, cR=50.0, lim=np.ones(nj),
                  max_input_blk=np.ones(nj), epsilon_O=0.1, MAX_O_ITER=12)
        x_init = mod.line_reference(x0, xg, H)
        ob = [dict(shape="cylinder", l=np.array([[3.7, 3.7], [8.5, 8.5], [0.001, 1.2]]), D=0.15, epsilon=0.2)]
    return mod.build_sys_info(robot, nj, H, x0, xg, x_init, **kw), ob


SINGLE_CASES = [(rid, nj, H, mode, tier) for (rid, nj, H), inst in SINGLE_SHAPES.items() for mode in ("CFS", "PSGCFS")
                for tier in (("default", "w1") if inst in (3160, 4160, 6160) else ("w1",))]


@pytest.mark.parametrize("rid,nj,H,mode,tier", SINGLE_CASES)
def test_other_joint_counts_on_w1(gpu, O, rid, nj, H, mode, tier):
    """(the instantiations 3160, 4160 and 6160 are launched by no other test: those run in the default tier as well)"""
    (s, ob), (t, _) = _single(gpu, rid, nj, H), _single(O, rid, nj, H)
    noise = np.random.default_rng(nj).standard_normal((s.MAX_O_ITER, H * nj)) * 0.1 if mode == "PSGCFS" else None
    slv = (gpu.CFS_FANUC if mode == "CFS" else gpu.PSGCFS_FANUC)(ob, s, rid)
    if tier == "w1":
        slv._batch.debug_options(**W1)
    got = slv.optimizer(noise=noise)
    want = O.optimizer(rid, t, [dict(l=ob[0]["l"], D=ob[0]["D"], epsilon=ob[0]["epsilon"])], mode, noise=noise)
    err = np.abs(got.x_ - want.x_).max()
    print(f"[{rid} nj {nj} H {H} {mode} {tier}] status {got.status} iter_O {got.iter_O}; linf(x_ - oracle) {err:.1e} rad")
    assert got.status == want.status and got.iter_O == want.iter_O
    assert err < (TOL_RAD if mode == "CFS" else 1e-5)
    np.testing.assert_allclose(got.eval.cost_all, want.cost_all, rtol=1e-8 if mode == "CFS" else 1e-6)


# ---- h. a 160-row shape that is w1 with no flag --------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["CFS", "PSGCFS"])
def test_default_w1_shape_one_step_at_a_time(gpu, O, shapes, mode):
    (nj, H), nobs = DEFAULT_W1_NJ_H, DEFAULT_W1_NOBS[mode]
    assert fused_tier(nj, H, nobs, mode) == 0 and nj * H <= 160         # w1, with no debug flag
    s, bt = shapes("w1d " + mode)
    assert (s.H, bt.nobs, bt.B) == (H, nobs, 8)
    # (un-kinked share of the oracle's own iterates: 0.75 for CFS with 25 obstacles, 0.97 for PSGCFS with 13)
    check_one_step_at_a_time(gpu, O, s, bt, mode, np.arange(bt.B), f"nobs {nobs}, default w1", tier_w1=False, min_unkinked=0.6)
