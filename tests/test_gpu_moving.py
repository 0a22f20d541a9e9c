"""Per-waypoint (moving) obstacles on the device (include/cfs_hip.h, CFS_OBS_PER_WAYPOINT):
constant rows are bit for bit the static handle; moving rows match the test-side reference (tests/moving_reference.py) piece by
piece and solve by solve; the solver keeps clear of where the obstacle IS at each waypoint; the refused combinations."""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest

import moving_reference as MR
from motionplanning_5d_m_amd import _lib, workloads

pytestmark = pytest.mark.gpu
FIELDS = ("u", "x_", "cost_all", "e_cost_all", "e_u_all", "iter_O", "total_iter", "status")
MU = 1e5


def _dist_fn(gpu):
    return lambda rb, th, ob: gpu.dist_arm(rb, th, ob)[0]


def _tier(h, tier):
    """tier "w1": the handle's fused kernels run on the w1 tier (config 3's shape runs the half-CU tiers by default)"""
    if tier == "w1":
        h.debug_options(tier_w1=True)
    return h


def _const_rows(obs, H):
    return np.ascontiguousarray(np.broadcast_to(obs[:, None], (obs.shape[0], H) + obs.shape[1:]))


@pytest.fixture(scope="module")
def c3_256(gpu):
    return workloads.config3(_dist_fn(gpu), B=256)


@pytest.fixture(scope="module")
def c3m(gpu):
    return workloads.config3_moving(_dist_fn(gpu), B=256, seed=20260115)


# ---- 1. constant rows are the static handle, bit for bit --------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["CFS", "PSGCFS"])
@pytest.mark.parametrize("jacobian", ["fd_literal", "analytic"])
@pytest.mark.parametrize("policy", ["stop", "soften"])
def test_constant_rows_are_bitwise_the_static_handle(gpu, c3_256, mode, jacobian, policy):
    import torch
    s, bt = c3_256
    margin = bt.margin_cfs if mode == "CFS" else bt.margin_psg
    kw = dict(mode=mode, max_batch=bt.B, jacobian=jacobian, on_infeasible=policy, soft_weight=MU if policy == "soften" else None)
    nz = bt.noise if mode == "PSGCFS" else None
    st = gpu.CFSBatch(s, bt.nobs, margin, **kw)
    mv = gpu.CFSBatch(s, bt.nobs, margin, obstacles="per_waypoint", **kw)
    assert st.obstacle_motion == "static" and mv.obstacle_motion == "per_waypoint"
    rows = _const_rows(bt.obs, s.H)
    want = st.solve(bt.x_init, bt.xR1, bt.ff, bt.caug, bt.obs, noise=nz)
    got = mv.solve(bt.x_init, bt.xR1, bt.ff, bt.caug, rows, noise=nz)
    for f in FIELDS + ("viol_all", "n_soft"):
        np.testing.assert_array_equal(getattr(got, f), getattr(want, f), err_msg=f)
    dev = torch.device("cuda:0")
    t = lambda a: torch.tensor(np.ascontiguousarray(a), dtype=torch.float64, device=dev)  # noqa: E731
    out = mv.solve_device(t(bt.x_init), t(bt.xR1), t(bt.ff), t(bt.caug), t(rows), noise=None if nz is None else t(nz))
    torch.cuda.synchronize()
    for f in FIELDS:
        np.testing.assert_array_equal(getattr(out, f).cpu().numpy(), getattr(got, f), err_msg="solve_device " + f)
    st.close()
    mv.close()


# ---- 2. pieces against the reference's per-waypoint get_con ------------------------------------------------------------------
def test_linearize_and_get_con_match_the_reference(gpu, O, c3m):
    check_linearize_and_get_con(gpu, O, c3m, "default")


def check_linearize_and_get_con(gpu, O, c3m, tier):
    """the body of the test below; tier "w1": on the w1 tier"""
    s, bt = c3m
    H, nj, n = s.H, 5, 4
    h = _tier(gpu.CFSBatch(s, bt.nobs, bt.margin_cfs, max_batch=n, obstacles="per_waypoint"), tier)
    dist, lid, grad = h.linearize(bt.x_init[:n], bt.obs[:n])
    u = np.sin(np.arange(H * nj))[None] * 0.05 * np.ones((n, 1))
    x_u = np.stack([O.rollout(H, nj, s.robot.delta_t, bt.xR1[b], u[b]) for b in range(n)])
    A0, b0 = h.get_con(bt.x_init[:n], np.zeros((n, H * nj)), bt.xR1[:n], bt.obs[:n])
    A1, b1 = h.get_con(x_u, u, bt.xR1[:n], bt.obs[:n])
    for b in range(n):
        s2 = SimpleNamespace(**vars(s))
        s2.xR1, s2.robot = bt.xR1[b], O.robotproperty2("M200i")
        Ar, br, dr, lr, gr = MR.get_con_moving(O, "M200i", s2, bt.obs[b], bt.margin_cfs, bt.x_init[b], np.zeros(H * nj), "CFS")
        np.testing.assert_allclose(dist[b], dr, rtol=0, atol=1e-14)
        np.testing.assert_array_equal(lid[b], lr)
        np.testing.assert_allclose(grad[b], gr, rtol=0, atol=2e-9)
        np.testing.assert_allclose(A0[b], Ar, rtol=0, atol=5e-9)
        np.testing.assert_allclose(b0[b], br, rtol=0, atol=1e-13)
        Ar, br, *_ = MR.get_con_moving(O, "M200i", s2, bt.obs[b], bt.margin_cfs, x_u[b], u[b], "CFS")
        np.testing.assert_allclose(A1[b], Ar, rtol=0, atol=5e-9)
        np.testing.assert_allclose(b1[b], br, rtol=0, atol=5e-9)
    # a static handle given the rows of waypoint 1 only disagrees wherever the obstacles have moved
    hs = _tier(gpu.CFSBatch(s, bt.nobs, bt.margin_cfs, max_batch=n), tier)
    ds, _, _ = hs.linearize(bt.x_init[:n], np.ascontiguousarray(bt.obs[:n, 0]))
    np.testing.assert_array_equal(ds[:, :, 0], dist[:, :, 0])
    assert np.abs(ds[:, :, -1] - dist[:, :, -1]).max() > 1e-3
    h.close()
    hs.close()


# ---- 3. whole solves against the reference -------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode,tol", [("CFS", 1e-7), ("PSGCFS", 1e-5)])
def test_whole_solves_match_the_reference(gpu, O, c3m, mode, tol):
    check_whole_solves(gpu, O, c3m, mode, tol, "default")


def check_whole_solves(gpu, O, c3m, mode, tol, tier):
    """the body of the test below; tier "w1": on the w1 tier"""
    s, bt = c3m
    idx = list(range(16))
    margin = bt.margin_cfs if mode == "CFS" else bt.margin_psg
    h = _tier(gpu.CFSBatch(s, bt.nobs, margin, mode=mode, max_batch=len(idx), obstacles="per_waypoint"), tier)
    got = h.solve(bt.x_init[idx], bt.xR1[idx], bt.ff[idx], bt.caug[idx], bt.obs[idx],
                  noise=bt.noise[idx] if mode == "PSGCFS" else None)
    want = MR.batch_moving(O, s, bt, mode, idx)
    chaotic, moved = MR.chaotic_moving(O, s, bt, mode, idx, want)
    print(f"{mode}: excluded as chaotic (reference moves > 1e-6 under a 1e-12 kick): {[idx[k] for k in np.nonzero(chaotic)[0]]}")
    checked = 0
    for k, b in enumerate(idx):
        if chaotic[k]:
            continue
        assert (int(got.status[k]), int(got.iter_O[k])) == (want[k].status, want[k].iter_O), b
        assert np.abs(got.x_[k] - want[k].x_).max() < tol, b
        checked += 1
    assert checked >= len(idx) // 2
    h.close()


# ---- 4. what the feature is for: clearance from where the obstacle is at each waypoint ---------------------------------------
def _clearance(gpu, robot, x_, rows):
    """min over obstacles of dist_arm at every waypoint: x_ (H*10,), rows (H, nobs, 6) -> (H,)"""
    th = x_.reshape(-1, 10)[:, :5]
    d = gpu.dist_arm(robot, th, rows.reshape(-1, 6))[0]                  # (H, H*nobs)
    H, nobs = rows.shape[:2]
    return np.array([d[i, i * nobs:(i + 1) * nobs].min() for i in range(H)])


def test_main_fanuc_crossing_obstacle(gpu):
    R, s, obs = gpu.main_FANUC_problem()
    H, dt, eps = s.H, s.robot.delta_t, 0.25
    rb = s.robot
    away = np.array([rb.base[0] + 8.0, rb.base[1] - 8.0, 0.001, rb.base[0] + 8.0, rb.base[1] - 8.0, 1.5])
    free = gpu.CFS_FANUC([dict(l=np.stack([away[:3], away[3:]], axis=1), epsilon=eps, D=0.2)], s, R).optimizer()
    assert free.status == 0
    m = H // 2
    pos = gpu.dist_arm(rb, free.x_.reshape(H, 10)[m - 1, :5][None], away[None], want_pos=True)[2][0]   # (nj, 2, 3)
    c = 0.5 * (pos[-1, 0] + pos[-1, 1])                                   # middle of the last link at waypoint m
    target = np.array([c[0], c[1], 0.001, c[0], c[1], 1.5])
    out = (c[:2] - rb.base[:2]) / np.linalg.norm(c[:2] - rb.base[:2])     # radially outward through it
    converged = 0
    # the axis comes in at constant speed from `far` (waypoint 1: the static solve's t = 0 row), reaches the last link at waypoint
    # m, then goes back the way it came or stays there; approach distances 1.5 and 3 m
    for reach, back in ((1.5, True), (1.5, False), (3.0, True), (3.0, False)):
        far = target + reach * np.array([out[0], out[1], 0.0, out[0], out[1], 0.0])
        v = (far - target) / ((m - 1) * dt)
        rows = np.stack([target + (abs(i + 1 - m) if back else max(m - i - 1, 0)) * dt * v for i in range(H)])[:, None]   # (H, 1, 6)
        np.testing.assert_allclose(rows[0, 0], far, atol=1e-12)
        l3 = np.stack([rows[:, 0, :3].T, rows[:, 0, 3:].T], axis=1)                      # (3, 2, H)
        snap = gpu.CFS_FANUC([dict(l=l3[:, :, 0], epsilon=eps, D=0.2)], s, R).optimizer()   # the t = 0 snapshot
        snap_clear = _clearance(gpu, rb, snap.x_, rows).min()
        assert snap.status == 0 and snap_clear < 1e-3                    # converges, but through the moving obstacle
        # the dodge takes more outer iterations than main_FANUC.m's 20 (with 20 every variant ends MAX_ITER 1.5-2 cm short)
        s100 = SimpleNamespace(**vars(s))
        s100.MAX_O_ITER = 100
        mv = gpu.CFS_FANUC([dict(l=l3, epsilon=eps, D=0.2)], s100, R)
        assert mv._batch.obstacle_motion == "per_waypoint"
        mv.optimizer()
        clear = _clearance(gpu, rb, mv.x_, rows).min()
        print(f"crossing obstacle (reach {reach} m, {'back' if back else 'stays'}): per-waypoint status {mv.status} iter_O "
              f"{mv.iter_O}, min clearance {clear:.4f} m (t = 0 snapshot: {snap_clear:.4f} m)")
        assert mv.status in (0, 1) and clear > snap_clear + 0.2
        if mv.status == 0:   # a converged plan keeps the margin at every waypoint, up to what the linearisation leaves (0.24 mm here)
            assert clear >= eps - 1e-3
            converged += 1
    assert converged >= 1


def test_config3_moving_converged_solves_keep_clear(gpu, c3m):
    s, bt = c3m
    h = gpu.CFSBatch(s, bt.nobs, bt.margin_cfs, mode="CFS", max_batch=bt.B, obstacles="per_waypoint")
    r = h.solve(bt.x_init, bt.xR1, bt.ff, bt.caug, bt.obs)
    conv = np.nonzero(r.status == 0)[0]
    assert conv.size >= bt.B // 2
    th = r.x_.reshape(bt.B, s.H, 10)[:, :, :5]
    worst = np.inf
    for i in range(s.H):                                                  # every problem against its own rows of waypoint i
        d = gpu.dist_arm(s.robot, th[conv, i], bt.obs[conv, i].reshape(-1, 6))[0]        # (n, n*nobs)
        for k in range(conv.size):
            worst = min(worst, d[k, k * bt.nobs:(k + 1) * bt.nobs].min())
    print(f"config3_moving CFS: {conv.size} of {bt.B} converged, worst clearance {worst:.5f} m (margin 0.25)")
    assert worst >= 0.25 - 2e-2, worst             # the bound test_gpu_plan.py applies to converged static solves
    h.close()


# ---- 5. refused on the device side ----------------------------------------------------------------------------------------------
def test_refused_combinations(gpu):
    R, s, obs = gpu.main_FANUC_problem()
    lib = gpu.lib()
    m = gpu.Mesh(vertices=np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], float), faces=np.array([[0, 1, 2]], np.int32))
    h = gpu.CFSBatch(s, 2, [0.25, 0.25], max_batch=1)
    h.set_meshes([m])
    with pytest.raises(gpu.CfsError) as e:
        h.set_obstacle_motion("per_waypoint")                           # meshes stay static
    assert e.value.code == -1 and h.obstacle_motion == "static"
    h.close()
    h = gpu.CFSBatch(s, 2, [0.25, 0.25], max_batch=1, obstacles="per_waypoint")
    with pytest.raises(ValueError):
        h.set_meshes([m])
    arr = (C.c_void_p * 1)(m._h)
    assert lib.cfs_problem_set_meshes(h._h, 1, arr) == -1
    assert lib.cfs_problem_set_obstacle_motion(h._h, 2) == -1 and lib.cfs_problem_set_obstacle_motion(h._h, -1) == -1
    assert h.obstacle_motion == "per_waypoint"
    z = lambda *sh: np.zeros(sh)  # noqa: E731
    with pytest.raises(ValueError):
        h.chomp(s.x_[None], z(1, 10), s.ff[None], z(1), z(1, 2, 6), z(1, s.H * 5), [0.2, 0.2], [0.25, 0.25])
    x_init, xR1, ff, caug, ob, u0 = s.x_[None].copy(), z(1, 10), s.ff[None].copy(), z(1), z(1, 2, 6), z(1, s.H * 5)
    D, ep = np.array([0.2, 0.2]), np.array([0.25, 0.25])
    i = _lib.cfs_batch_in()
    i.B = 1
    i.x_init, i.xR1, i.ff, i.caug, i.obs = [a.ctypes.data_as(C.c_void_p) for a in (x_init, xR1, ff, caug, ob)]
    r = [z(1, 150), z(1, 300), z(1, 20), z(1, 20), z(1, 20), np.zeros(1, np.int32), np.zeros(1, np.int32), np.zeros(1, np.int32)]
    o = _lib.cfs_batch_out(*[a.ctypes.data_as(C.c_void_p) for a in r])
    assert lib.cfs_chomp_batch(h._h, C.byref(i), u0.ctypes.data_as(C.c_void_p), D.ctypes.data_as(C.c_void_p),
                               ep.ctypes.data_as(C.c_void_p), C.byref(o)) == -1
    h.set_obstacle_motion("static")
    assert h.obstacle_motion == "static"
    h.close()


def test_largest_shape_is_solved_or_refused_at_set_time(gpu):
    """H = 64 x nobs = 32 (two-link arm: the five-joint arm's static plan is refused at creation already)"""
    R, s2, obs = gpu.main_2L_problem()
    s = gpu.build_sys_info(s2.robot, 2, 64, np.zeros(2), np.array([np.pi / 2, 0.0]), np.tile(np.zeros(4), 64),
                           Qp=np.diag([10.0, 1.0]), Qv=np.diag([10.0, 1.0]), Rblk=np.diag([5.0, 4.0]), cR=0.1, lim=np.array([0.1, 0.2]),
                           max_input_blk=np.ones(2) * 0.5 * s2.robot.delta_t, epsilon_O=1e-6, MAX_O_ITER=5)
    nobs = 32
    rng = np.random.default_rng(4)
    rad, ang = rng.uniform(0.8, 1.5, nobs), rng.uniform(0, 2 * np.pi, nobs)
    cen = np.stack([rad * np.cos(ang), rad * np.sin(ang)], axis=1)
    ob = np.concatenate([cen, np.zeros((nobs, 1)), cen, np.zeros((nobs, 1))], axis=1)[None]
    st = gpu.CFSBatch(s, nobs, [0.05] * nobs, max_batch=1)
    mv = gpu.CFSBatch(s, nobs, [0.05] * nobs, max_batch=1)
    try:
        mv.set_obstacle_motion("per_waypoint")
    except gpu.CfsError as e:
        assert e.code == -1 and mv.obstacle_motion == "static"
        return
    xR1 = np.zeros((1, 4))
    want = st.solve(s.x_[None], xR1, s.ff[None], np.array([s.caug]), ob)
    got = mv.solve(s.x_[None], xR1, s.ff[None], np.array([s.caug]), _const_rows(ob, 64))
    for f in FIELDS:
        np.testing.assert_array_equal(getattr(got, f), getattr(want, f), err_msg=f)
