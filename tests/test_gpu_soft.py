"""The infeasible-QP policy on the device (include/cfs_hip.h, CFS_INFEAS_SOFTEN).

* STOP set explicitly is the default bit for bit; SOFTEN changes nothing for a problem whose QPs are all feasible;
* a problem the default ends QP_INFEASIBLE carries on, and every outer iteration of it is checked ONE step at a time
  against the oracle started from the device's own previous iterate (pattern of tests/test_gpu_chaos.py): the hard QP when
  the oracle solves it, otherwise the soft QP solved by the oracle on the augmented matrices (tests/soft_reference.py);
* cfs_qp on infeasible linearisations, warm start on/off, repeatability, and the refused mesh combinations.
"""
import concurrent.futures as cf
import copy
from types import SimpleNamespace

import numpy as np
import pytest

import soft_reference as S
from helpers import oracle_obs, truth_on_active_set

pytestmark = pytest.mark.gpu

MU = 1e6
ONE_STEP_TOL = 1e-8       # |u_k(device) - oracle_step(u_{k-1}(device))|_inf / |u_k|_inf on un-kinked steps
SOFT_STEP_TOL = 1e-7      # the same on softened steps whose extended-precision solution also disagrees beyond 1e-8: the soft
                          # QP's dual carries 1/mu on its diagonal (main_2L, mu = 1e6: one step of 51 at 3.3e-8)
VIOL_TOL = 1e-9           # viol_all[k] against the oracle's max slack, m
KINK = 1e-9               # the oracle's own single step moves by more than this (relative) under a 1e-12 kick
FIELDS = ("u", "x_", "cost_all", "e_cost_all", "e_u_all", "iter_O", "total_iter", "status")


def _solve(gpu, s, bt, mode, idx, log=False, dbg=None, **kw):
    margin = bt.margin_cfs if mode == "CFS" else bt.margin_psg
    nz = bt.noise[idx] if (mode == "PSGCFS" and bt.noise is not None) else None
    slv = gpu.CFSBatch(s, bt.nobs, margin, mode=mode, max_batch=len(idx), **kw)
    if dbg:
        slv.debug_options(**dbg)
    if log:
        slv.log_u(True)
    r = slv.solve(bt.x_init[idx], bt.xR1[idx], bt.ff[idx], bt.caug[idx], bt.obs[idx], noise=nz)
    r.ulog = slv.read_u_log(len(idx)) if log else None
    slv.close()
    return r


# ---- 1, 7: STOP is the default; two soft solves agree bit for bit ------------------------------------------------------------
@pytest.mark.parametrize("mode", ["CFS", "PSGCFS"])
def test_stop_is_the_default_and_soft_solves_repeat(gpu, c3, mode):
    s, bt = c3
    idx = np.arange(256)
    margin = bt.margin_cfs if mode == "CFS" else bt.margin_psg
    h = gpu.CFSBatch(s, bt.nobs, margin, mode=mode, max_batch=1)
    assert h.infeasible_policy == ("stop", None)
    h.set_infeasible_policy("soften", 1e5)
    assert h.infeasible_policy == ("soften", 1e5)
    h.set_infeasible_policy("stop")
    assert h.infeasible_policy == ("stop", None)
    h.close()
    fresh = _solve(gpu, s, bt, mode, idx)
    stop = _solve(gpu, s, bt, mode, idx, on_infeasible="stop", soft_weight=1e6)
    for k in FIELDS + ("viol_all", "n_soft"):
        np.testing.assert_array_equal(getattr(fresh, k), getattr(stop, k), err_msg=k)
    assert not fresh.viol_all.any() and not fresh.n_soft.any() and (fresh.status != 4).all()
    a = _solve(gpu, s, bt, mode, idx, on_infeasible="soften", soft_weight=MU)
    b = _solve(gpu, s, bt, mode, idx, on_infeasible="soften", soft_weight=MU)
    for k in FIELDS + ("viol_all", "n_soft"):
        np.testing.assert_array_equal(getattr(a, k), getattr(b, k), err_msg=k)


# ---- 2: feasible problems unchanged, infeasible ones carry on -----------------------------------------------------------------
@pytest.mark.parametrize("mode", ["CFS", "PSGCFS"])
def test_config3_soften_changes_only_the_infeasible_problems(gpu, c3, mode):
    s, bt = c3
    idx = np.arange(bt.x_init.shape[0])
    d = _solve(gpu, s, bt, mode, idx, log=True)
    g = _solve(gpu, s, bt, mode, idx, log=True, on_infeasible="soften", soft_weight=MU)
    ok = d.status <= 1
    for k in FIELDS:
        np.testing.assert_array_equal(getattr(d, k)[ok], getattr(g, k)[ok], err_msg=k)
    assert not g.viol_all[ok].any() and not g.n_soft[ok].any()
    inf = d.status == 2
    assert inf.sum() > 0
    assert (g.status[inf] != 2).all(), np.bincount(g.status[inf])
    assert (g.n_soft[inf] >= 1).all()
    for a in np.nonzero(inf)[0]:                                     # iterates logged before the failing iteration are the default's
        n = int(d.iter_O[a]) - 1
        np.testing.assert_array_equal(d.ulog[a, :n], g.ulog[a, :n])
        assert not g.viol_all[a, :n].any() and g.viol_all[a, n] > 0
    if mode == "CFS":                                                 # (PSGCFS: the last iteration may take no step, hence solve no QP)
        last = g.viol_all[np.arange(len(idx)), np.maximum(g.iter_O - 2, 0)]
        assert ((g.status == 4) == (last > 0)).all()                 # SOFT_ENDED <=> the last QP was softened
    print(f"[config3 {mode}] default {np.bincount(d.status, minlength=5)} -> soften {np.bincount(g.status, minlength=5)}; "
          f"n_soft of the infeasible {np.bincount(g.n_soft[inf])}")


# ---- 3: one step at a time against the oracle --------------------------------------------------------------------------------
def _check_steps(O, cases, tag):
    """cases: namespaces (ROBOT, s (oracle sys_info with x_), obs, xR1, ff, mode, noise (rows, nn) | None, got: iter_O, status,
    cost_all, caug, ulog (K, nn), viol (K,))"""
    jobs = []
    rng = np.random.default_rng(7)
    for c in cases:
        n_it = int(c.iter_O) - 1
        rows = 0
        for k in range(1, n_it + 1):
            u_prev = c.ulog[k - 2] if k >= 2 else None
            nz = None
            if c.mode == "PSGCFS":
                cst = lambda j: 100000.0 if j < 0 else (c.caug if j == 0 else c.cost_all[j - 1])   # noqa: E731
                if abs(cst(k - 1) - cst(k - 2)) < 1e-4:                # stop_inner: no QP, u stays
                    continue
                nz = c.noise[rows] if c.noise is not None and rows < c.noise.shape[0] else None
                rows += 1
            jobs.append((c, k, u_prev, nz, 1e-12 * rng.standard_normal(c.ulog.shape[1])))

    def one(job):
        c, k, u_prev, nz, kick = job
        q = S.step_qp(O, c.ROBOT, c.s, c.obs, c.xR1, c.ff, u_prev, k, c.mode, noise_row=nz)
        want, soft, viol, st, lam = S.oracle_soft_step(O, q, MU)
        if k == 1:
            s2 = copy.copy(c.s)
            s2.x_ = np.asarray(c.s.x_, float).reshape(-1) + np.resize(kick, np.asarray(c.s.x_).size)   # the first step starts from x_init: kick that
            q2 = S.step_qp(O, c.ROBOT, s2, c.obs, c.xR1, c.ff, None, 1, c.mode, noise_row=nz)
        else:
            q2 = S.step_qp(O, c.ROBOT, c.s, c.obs, c.xR1, c.ff, u_prev + kick, k, c.mode, noise_row=nz)
        w2, soft2, _, st2, _ = S.oracle_soft_step(O, q2, MU)
        u_k = c.ulog[k - 1]
        sc = max(np.abs(u_k).max(), 1e-300)
        err = np.abs(u_k - want).max() / sc if st == 0 else np.inf
        if soft and st == 0 and not err <= ONE_STEP_TOL:
            # arbiter (helpers.truth_on_active_set): the soft QP's dual carries 1/mu on its diagonal, so fp64 solvers may part by
            # more than 1e-8 on it; the extended-precision solution on the oracle's active set decides
            Ga, ga, Aa = S.augment(q.G, q.g0, q.A, q.col, MU)
            act = [r for r in np.nonzero(lam > 0)[0]]
            act = [r for i, r in enumerate(act) if not any(np.array_equal(Aa[r], Aa[p]) for p in act[:i])]   # get_con repeats the velocity rows per obstacle
            x_ld, _ = truth_on_active_set(Ga, ga, Aa, q.b, np.array(act, int))
            err = min(err, np.abs(u_k - x_ld[:len(u_k)]).max() / sc)
        sens = np.abs(w2 - want).max() / sc if (st == 0 and st2 == 0 and soft == soft2) else np.inf
        dev_soft = c.viol[k - 1] > 0
        tstar = S.least_violation(q.A, q.b, q.col, q.box) if dev_soft != soft else None
        return (c.name, k, err, sens, soft, dev_soft, abs(c.viol[k - 1] - viol), tstar)

    with cf.ThreadPoolExecutor(16) as ex:
        res = list(ex.map(one, jobs))
    err = np.array([r[2] for r in res])
    sens = np.array([r[3] for r in res])
    kink = ~(sens <= KINK)
    nsoft = sum(r[4] for r in res)
    print(f"[{tag}] {len(cases)} problems, {len(res)} outer iterations ({nsoft} softened by the oracle), {int(kink.sum())} kinked; "
          f"un-kinked: max err {err[~kink].max() if (~kink).any() else 0:.1e}, max |viol - oracle| "
          f"{max([r[6] for r, kk in zip(res, kink) if not kk] or [0]):.1e} m")
    assert nsoft > 0
    bad = [(r[0], r[1], r[2]) for r, kk in zip(res, kink) if not kk and not r[2] <= (SOFT_STEP_TOL if r[4] else ONE_STEP_TOL)]
    assert not bad, bad
    badv = [(r[0], r[1], r[6]) for r, kk in zip(res, kink) if not kk and not r[6] <= VIOL_TOL]
    assert not badv, badv
    badd = [(r[0], r[1], r[4], r[5], r[7]) for r in res if r[4] != r[5] and r[7] > 1e-9]
    assert not badd, badd
    assert (~kink).sum() >= 0.3 * len(res)                           # (RRT routes: 37 % of the steps are kinked-free)


def _config3_cases(gpu, O, s, bt, mode, idx, **kw):
    g = _solve(gpu, s, bt, mode, idx, log=True, on_infeasible="soften", soft_weight=MU, **kw)
    margin = bt.margin_cfs if mode == "CFS" else bt.margin_psg
    out = []
    for a, b in enumerate(idx):
        so = SimpleNamespace(**vars(s))
        so.robot, so.x_ = O.robotproperty2("M200i"), bt.x_init[b]
        out.append(SimpleNamespace(name=int(b), ROBOT="M200i", s=so, obs=oracle_obs(bt, b, margin), xR1=bt.xR1[b], ff=bt.ff[b],
                                   mode=mode, noise=bt.noise[b] if (mode == "PSGCFS" and bt.noise is not None) else None,
                                   iter_O=g.iter_O[a], cost_all=g.cost_all[a], caug=bt.caug[b], ulog=g.ulog[a], viol=g.viol_all[a]))
    return out, g


@pytest.mark.parametrize("mode", ["CFS", "PSGCFS"])
def test_config3_infeasible_problems_one_step_at_a_time(gpu, O, c3, mode):
    check_infeasible_problems_one_step_at_a_time(gpu, O, c3, mode, "default")


def check_infeasible_problems_one_step_at_a_time(gpu, O, c3, mode, tier, n=256):
    """the body of the test above; tier "w1": on the w1 tier, n: the first n problems"""
    s, bt = c3
    dbg = dict(tier_w1=True) if tier == "w1" else None              # config 3's shape runs the half-CU tiers by default
    d = _solve(gpu, s, bt, mode, np.arange(n), dbg=dbg)
    idx = np.nonzero(d.status == 2)[0]
    assert idx.size > 0
    cases, _ = _config3_cases(gpu, O, s, bt, mode, idx, dbg=dbg)
    _check_steps(O, cases, f"config3 {mode} {tier}")


@pytest.mark.parametrize("mode", ["CFS", "PSGCFS"])
def test_main_2l_one_step_at_a_time(gpu, O, mode):
    R, s, obs = gpu.main_2L_problem()
    P = O.problem_main_2L()
    slv = (gpu.CFS_FANUC if mode == "CFS" else gpu.PSGCFS_FANUC)(obs, s, R, on_infeasible="soften", soft_weight=MU)
    slv._batch.log_u(True)
    slv.optimizer()
    ulog = slv._batch.read_u_log(1)[0]
    assert slv.n_soft > 0 and slv.status in (0, 1, 4)
    viol = np.zeros(s.MAX_O_ITER)
    viol[:len(slv.viol_all)] = slv.viol_all
    c = SimpleNamespace(name="main_2L", ROBOT="2L", s=P.sys_info, obs=P.obs, xR1=P.sys_info.xR1, ff=P.sys_info.ff, mode=mode,
                        noise=None, iter_O=slv.iter_O, cost_all=slv.eval.cost_all, caug=float(P.sys_info.caug), ulog=ulog, viol=viol)
    print(f"[main_2L {mode}] status {slv.status} iter_O {slv.iter_O} n_soft {slv.n_soft} last viol {slv.viol_all[-1]:.4f}")
    _check_steps(O, [c], f"main_2L {mode}")


def test_rrtstar_cfs_on_device_grown_routes_one_step_at_a_time(gpu, O):
    obs_r, s_r, goal, rg, rs, off = gpu.RRTstar_problem()
    planner = gpu.RRT_FANUC(obs_r, s_r, goal, rg, rs, off, "M200i", "RRT")
    res = [r for r in planner.grow(seed=20261015, S=64) if not r.fail][:32]
    assert len(res) == 32
    cases, n_inf_default = [], 0
    for i, r in enumerate(res):
        R, s, obs = gpu.RRTstar_CFS_problem(r.route)
        d = gpu.CFS_FANUC(obs, s, R).optimizer()
        n_inf_default += d.status == 2
        slv = gpu.CFS_FANUC(obs, s, R, on_infeasible="soften", soft_weight=MU)
        slv._batch.log_u(True)
        slv.optimizer()
        if d.status <= 1:
            np.testing.assert_array_equal(slv.x_, d.x_)
            assert slv.n_soft == 0
        else:
            assert slv.status != 2
        P = O.problem_RRTstar_CFS(r.route)
        viol = np.zeros(s.MAX_O_ITER)
        viol[:len(slv.viol_all)] = slv.viol_all
        cases.append(SimpleNamespace(name=i, ROBOT="M200i", s=P.sys_info, obs=P.obs, xR1=P.sys_info.xR1, ff=P.sys_info.ff, mode="CFS",
                                     noise=None, iter_O=slv.iter_O, cost_all=slv.eval.cost_all, caug=float(P.sys_info.caug),
                                     ulog=slv._batch.read_u_log(1)[0], viol=viol))
    print(f"[RRTstar_CFS] {n_inf_default} of 32 device-grown routes end QP_INFEASIBLE by default")
    _check_steps(O, cases, "RRTstar_CFS device-grown routes")


# ---- 4: analytic Jacobian with soft mode ----------------------------------------------------------------------------------------
def test_analytic_soft_one_step_on_the_device_rows(gpu, O, c3):
    """the soft step of an analytic handle against the oracle's soft QP on the rows cfs_get_con of that handle returns"""
    s, bt = c3
    mode = "CFS"
    d = _solve(gpu, s, bt, mode, np.arange(128), jacobian="analytic")
    idx = np.nonzero(d.status == 2)[0][:8]
    assert idx.size > 0
    g = _solve(gpu, s, bt, mode, idx, log=True, jacobian="analytic", on_infeasible="soften", soft_weight=MU)
    h = gpu.CFSBatch(s, bt.nobs, bt.margin_cfs, mode=mode, max_batch=1, jacobian="analytic")
    nn, checked, soft_seen = s.H * 5, 0, 0
    for a, b in enumerate(idx):
        for k in range(1, int(g.iter_O[a])):
            u_prev = g.ulog[a, k - 2] if k >= 2 else np.zeros(nn)
            x_ = bt.x_init[b][None] if k == 1 else O.rollout(s.H, 5, s.robot.delta_t, bt.xR1[b], u_prev)[None]
            A, rhs = h.get_con(x_, u_prev[None], bt.xR1[b][None], bt.obs[b][None])
            A = np.vstack([A[0], np.eye(nn), -np.eye(nn)])
            rhs = np.concatenate([rhs[0], s.MAX_input, s.MAX_input])
            q = SimpleNamespace(G=s.QQ, g0=bt.ff[b], A=A, b=rhs, col=S.collision_rows(bt.nobs, s.H, 5), box=s.MAX_input)
            want, soft, viol, st, _ = S.oracle_soft_step(O, q, MU)
            assert st == 0
            u_k = g.ulog[a, k - 1]
            err = np.abs(u_k - want).max() / max(np.abs(u_k).max(), 1e-300)
            assert err <= ONE_STEP_TOL or k > 1 and err <= 1e-6, (int(b), k, err)
            if soft:
                soft_seen += 1
                assert abs(g.viol_all[a, k - 1] - viol) <= 1e-7, (int(b), k, g.viol_all[a, k - 1], viol)
            checked += 1
    h.close()
    assert soft_seen > 0
    print(f"[analytic soft] {checked} steps of {idx.size} problems, {soft_seen} softened")


# ---- 5: cfs_qp on infeasible linearisations ----------------------------------------------------------------------------------
def test_cfs_qp_soft_on_infeasible_iteration_2(gpu, O, c3):
    s, bt = c3
    mode = "CFS"
    d = _solve(gpu, s, bt, mode, np.arange(256), log=True)
    idx = np.nonzero((d.status == 2) & (d.iter_O == 2))[0][:16]
    assert idx.size > 0
    u1 = d.ulog[idx, 0]
    x1 = np.stack([O.rollout(s.H, 5, s.robot.delta_t, bt.xR1[b], u1[a]) for a, b in enumerate(idx)])
    h = gpu.CFSBatch(s, bt.nobs, bt.margin_cfs, mode=mode, max_batch=len(idx))
    dist, _, grad = h.linearize(x1, bt.obs[idx])
    _, _, _, st0 = h.qp(bt.ff[idx], u1, bt.xR1[idx], dist, grad)
    assert (st0 == 2).all()
    prev = np.full(len(idx), np.inf)
    nH = bt.nobs * s.H
    for mu in (1e4, 1e6, 1e8):
        h.set_infeasible_policy("soften", mu)
        u, lam, _, st = h.qp(bt.ff[idx], u1, bt.xR1[idx], dist, grad)
        assert (st == 4).all(), st
        slack = lam[:, :nH] / mu
        for a, b in enumerate(idx):
            so = SimpleNamespace(**vars(s))
            so.robot, so.x_ = O.robotproperty2("M200i"), bt.x_init[b]
            q = S.step_qp(O, "M200i", so, oracle_obs(bt, b, bt.margin_cfs), bt.xR1[b], bt.ff[b], u1[a], 2, mode)
            want, sl, _, st_o, _ = S.soft_qp(O, q.G, q.g0, q.A, q.b, q.col, mu)
            assert st_o == 0
            tol = 1e-8 if mu <= 1e6 else 1e-6
            assert np.abs(u[a] - want).max() <= tol * max(np.abs(want).max(), 1.0), (int(b), mu)
            assert abs(slack[a].max() - sl.max()) <= (1e-9 if mu <= 1e6 else 1e-7), (int(b), mu, slack[a].max(), sl.max())
        ss = (slack * slack).sum(axis=1)                             # |s|^2 is non-increasing in mu; the max slack need not be
        assert (ss <= prev * (1 + 1e-6) + 1e-15).all(), (ss, prev)
        prev = ss
    h.close()


# ---- 6: warm start on / off ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["CFS", "PSGCFS"])
def test_soft_results_do_not_depend_on_the_warm_start(gpu, c3, mode):
    s, bt = c3
    d = _solve(gpu, s, bt, mode, np.arange(256))
    idx = np.nonzero(d.status == 2)[0]
    a = _solve(gpu, s, bt, mode, idx, log=True, on_infeasible="soften", soft_weight=MU)
    b = _solve(gpu, s, bt, mode, idx, log=True, on_infeasible="soften", soft_weight=MU, dbg=dict(no_warm_start=True))
    np.testing.assert_array_equal(a.status, b.status)
    np.testing.assert_array_equal(a.iter_O, b.iter_O)
    np.testing.assert_array_equal(a.n_soft, b.n_soft)
    # The warm start changes the rounding of a hard QP (a different sequence of active-set steps), and the outer loop of these
    # problems amplifies rounding (helpers.chaotic_problems): the iterates must part at rounding level, never by a jump.
    same, first = 0, []
    for p in range(len(idx)):
        n = int(a.iter_O[p]) - 1
        d = np.abs(a.ulog[p, :n] - b.ulog[p, :n]).max(axis=1) / np.maximum(np.abs(a.ulog[p, :n]).max(axis=1), 1e-300)
        if not d.any():
            same += 1
            continue
        first.append(float(d[np.nonzero(d)[0][0]]))
    close = (np.abs(a.u - b.u).max(axis=1) <= 1e-9).mean()
    print(f"[warm start {mode}] {same} of {len(idx)} problems bit-identical, final u within 1e-9 on {close:.0%}; "
          f"first differences: max {max(first or [0]):.1e}")
    assert max(first or [0]) <= 1e-9


# ---- 8: mesh handles are out of scope ------------------------------------------------------------------------------------------
def test_mesh_combinations_are_refused(gpu):
    R, s, obs = gpu.main_FANUC_problem()
    m = gpu.Mesh(vertices=np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], float), faces=np.array([[0, 1, 2]], np.int32))
    h = gpu.CFSBatch(s, 2, [0.25, 0.25], max_batch=1)
    h.set_meshes([m])
    with pytest.raises(gpu.CfsError) as e:
        h.set_infeasible_policy("soften", MU)
    assert e.value.code == -1
    assert h.infeasible_policy == ("stop", None)
    h.close()
    h = gpu.CFSBatch(s, 2, [0.25, 0.25], max_batch=1, on_infeasible="soften", soft_weight=MU)
    with pytest.raises(gpu.CfsError) as e:
        h.set_meshes([m])
    assert e.value.code == -1
    h.close()
