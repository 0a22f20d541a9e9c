"""The clearance audit with moving meshes on the device (include/cfs_hip.h, cfs_clearance_mesh_motion*):
parity with the test-side reference (tests/clearance_motion_reference.py, which tests/test_clearance_motion_reference.py checks on
the CPU), dist_wp against the linearisation's own distances, dist_path against the one triangle it names, identity / constant poses
and a static handle against cfs_clearance_mesh, nesting and soundness of the bound, independence of the batch, of the query variants,
of the mesh order and of the stream, the table cache, the refusals, a six-joint robot, and what the feature is for: a plan that
keeps its margin at every waypoint and loses 8 cm of it in between.

Shapes: main_FANUC (M200i) at H = 12, B = 3, the 148-triangle post and ball (moving) and a far box (held still) next to the line
obstacle; S = 4 (49 samples: one partly filled wavefront) and 16 (193: four wavefronts, the last partly filled)."""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest

import clearance_mesh_cases as MC
import clearance_motion_reference as CM
import clearance_reference as CR
import mesh_motion_reference as M
from test_gpu_clearance_mesh import _one_triangle
from test_gpu_mesh_motion import _Cell

pytestmark = pytest.mark.gpu
ROBOT = "M200i"
DIST = ("dist_wp", "dist_path", "dist_lower")
OUT = DIST + ("t_path", "link_path")
ALL = OUT + ("tri_path",)
LINE_ROW = np.concatenate([M.LINE[:, 0], M.LINE[:, 1]])[None]
H12, OFF, DY, ANG = M.CASES.cfs12
POSES = {"vertical": M.poses_z(H12, DY, ANG), "general-axis": M.poses_general(H12, DY, ANG)}
EYE = M.identity_poses(H12)


@pytest.fixture(scope="module")
def cells(gpu):
    """per solver: the handle (line, post and ball, far box; B = 3) and, per pose schedule, the device's own plans on the posed handle"""
    out = {}
    for mode in ("CFS", "PSGCFS"):
        c = _Cell(gpu, M.fanuc(gpu, H12), mode, [M.post_and_ball(gpu.mesh, OFF), M.far_box(gpu.mesh)], B=3)
        c.tris = [M.post_and_ball(gpu.mesh, OFF), M.far_box(gpu.mesh)]
        c.plans = {}
        for name, P in POSES.items():
            c.h.set_mesh_motion([P, EYE])
            c.plans[name] = c.solve()
        out[mode] = c
    yield out
    for c in out.values():
        c.close()


def _posed(cells, mode, name):
    c = cells[mode]
    c.h.set_mesh_motion([POSES[name], EYE])
    return c, c.plans[name]


def _audit(c, r, S, entry="clearance_mesh_motion", sl=slice(None)):
    return getattr(c.h, entry)(r.x_[sl], r.u[sl], c.xR1[sl], c.obs[sl], substeps=S)


def _reference(O, c, r, b, poses, S, tris=None, H=H12):
    return CM.audit(O, O.robotproperty2(ROBOT), H, 5, c.s.robot.delta_t, r.x_[b], r.u[b], c.xR1[b], LINE_ROW, tris or c.tris, poses, S)


def _parity(got, b, want, label):
    """1e-10 m on the three distances of every column, equal link and time wherever the runner-up sample is 1e-9 m above the
    minimum; no sample of the reference is near the surrogate's switch, so no pair is left out.  Returns the largest deviation."""
    assert np.abs(want.D).min() > 2e-4
    dev = max(float(np.abs(getattr(got, k)[b] - getattr(want, k)).max()) for k in DIST)
    sure = want.gap > 1e-9
    print(f"{label}: max deviation {dev:.3e} m, {int(sure.sum())} of {sure.size} columns with a clear arg-min, mover dist_wp "
          f"{got.dist_wp[b, 1]:.7f} dist_path {got.dist_path[b, 1]:.7f} dist_lower {got.dist_lower[b, 1]:.7f}")
    for k in DIST:
        assert np.abs(getattr(got, k)[b] - getattr(want, k)).max() <= 1e-10, k
    assert (got.link_path[b][sure] == want.link_path[sure]).all()
    assert (got.t_path[b][sure] == want.t_path[sure]).all()
    return dev


def _same(a, b, keys=ALL + ("short_by",), msg=""):
    for k in keys:
        np.testing.assert_array_equal(getattr(a, k), getattr(b, k), err_msg=f"{msg} {k}")


@pytest.mark.parametrize("S", [4, 16])
@pytest.mark.parametrize("name", list(POSES))
@pytest.mark.parametrize("mode", ["CFS", "PSGCFS"])
def test_parity_with_the_reference(gpu, O, cells, mode, name, S):
    """every problem of the batch, every column.  The bound is asserted for plans that ended with status 0 / 1 (its premise is a
    solved problem; the CFS plan against the general-axis schedule ends QP_INFEASIBLE), parity for all."""
    c, r = _posed(cells, mode, name)
    got = _audit(c, r, S)
    for b in range(3):
        want = _reference(O, c, r, b, [POSES[name], EYE], S)
        _parity(got, b, want, f"{mode} {name} S={S} problem {b} status {r.status[b]}")
        assert want.v_mesh[0, 1:].min() > 0.03 and not want.v_mesh[1].any()       # the post moves, the box stands
        assert (got.dist_path[b] <= got.dist_wp[b]).all()
        if r.status[b] <= 1:
            assert (got.dist_lower[b] <= got.dist_path[b]).all()
    np.testing.assert_array_equal(got.short_by, (c.h.margin[None] - got.dist_path).max(axis=1))
    assert (got.tri_path[:, 0] == -1).all() and (got.tri_path[:, 1] >= 0).all() and (got.tri_path[:, 1] < 148).all()


@pytest.mark.parametrize("name", list(POSES))
@pytest.mark.parametrize("mode", ["CFS", "PSGCFS"])
def test_dist_wp_is_measured_where_the_linearisation_measures_it(cells, mode, name):
    """1e-12 m between dist_wp of the mesh columns and the smallest of the H distances the posed handle's linearisation (the rows
    get_con is built from) returns at the same x_: sample k = S uses the stored inverse pose of its waypoint, unchanged"""
    c, r = _posed(cells, mode, name)
    got = _audit(c, r, 4)
    dist = c.h.linearize(r.x_, c.obs)[0]                # (B, nobs, H)
    dev = np.abs(dist[:, 1:].min(axis=2) - got.dist_wp[:, 1:]).max()
    print(f"{mode} {name}: dist_wp against the linearisation {dev:.3e} m")
    assert dev <= 1e-12


@pytest.mark.parametrize("name", list(POSES))
@pytest.mark.parametrize("mode", ["CFS", "PSGCFS"])
def test_dist_path_is_the_distance_to_the_triangle_it_names(gpu, cells, mode, name):
    """1e-12 m between dist_path and cfs_mesh_segment_distance of link link_path against the ONE triangle tri_path, the link
    placed in the mesh's frame by the inverse of the interpolated pose at t_path"""
    c, r = _posed(cells, mode, name)
    S, dt = 16, c.s.robot.delta_t
    got = _audit(c, r, S)
    itvs = CM.intervals(c.tris[0], POSES[name], dt)
    between = 0
    for b in range(3):
        g = int(round(got.t_path[b, 1] / dt * S))
        i, k = (0, 0) if g == 0 else ((g - 1) // S, (g - 1) % S + 1)
        between += 0 < k < S and i > 0                  # strictly between two waypoints, at an interpolated pose
        assert (got.dist_path[b, 1] == got.dist_wp[b, 1]) if k == S else (got.dist_path[b, 1] < got.dist_wp[b, 1])
        T = CM.sample_pose(itvs, i, k, S)
        TH, _ = CR.samples(H12, 5, dt, r.x_[b], r.u[b], c.xR1[b], np.zeros((1, 6)), S)
        pos = gpu.dist_arm(c.s.robot, MC.pose_of(TH, S, dt, got.t_path[b, 1])[None], np.zeros((1, 6)), want_pos=True)[2]
        ends = pos[0, got.link_path[b, 1] - 1].reshape(2, 3)
        seg = ((ends - T[:, 3]) @ T[:, :3]).reshape(1, 6)                  # R'(w - t) of both ends
        d = _one_triangle(gpu, c.tris[0][got.tri_path[b, 1]], seg)
        assert abs(d - got.dist_path[b, 1]) <= 1e-12, (b, d, got.dist_path[b, 1])
    print(f"{mode} {name}: {between} of 3 path minima at an interpolated pose")


@pytest.mark.parametrize("mode", ["CFS", "PSGCFS"])
def test_identity_poses_and_a_static_handle_are_the_static_audit_bit_for_bit(cells, mode):
    c, r = _posed(cells, mode, "vertical")
    moving = _audit(c, r, 16)
    c.h.set_mesh_motion(None)
    want = _audit(c, r, 16, "clearance_mesh")
    _same(_audit(c, r, 16), want, msg="static handle")                      # the new entry on a static handle
    c.h.set_mesh_motion([EYE, np.eye(4)])
    _same(_audit(c, r, 16), want, msg="identity poses")
    _same(_audit(c, r, 5), (c.h.set_mesh_motion(None), _audit(c, r, 5, "clearance_mesh"))[1], msg="identity, S = 5")
    assert np.abs(moving.dist_path[:, 1] - want.dist_path[:, 1]).max() > 1e-3       # and the motion matters


def test_a_constant_general_pose_is_the_static_audit_of_the_transformed_mesh(gpu, cells):
    """the hierarchy differs (it is built from other vertices), the answer does not: 1e-10 m; the held intervals add no speed"""
    c, r = _posed(cells, "CFS", "general-axis")
    T = POSES["general-axis"][H12 // 2]
    c.h.set_mesh_motion([T, np.eye(4)])
    got = _audit(c, r, 16)
    other = _Cell(gpu, c.s, "CFS", [M.transform(c.tris[0], T), c.tris[1]], B=3)
    want = other.h.clearance_mesh(r.x_, r.u, c.xR1, c.obs, substeps=16)
    dev = max(float(np.abs(getattr(got, k) - getattr(want, k)).max()) for k in DIST)
    print(f"constant pose against the transformed mesh: {dev:.3e} m")
    assert dev <= 1e-10
    np.testing.assert_array_equal(got.dist_wp[:, 0], want.dist_wp[:, 0])
    other.close()


@pytest.mark.parametrize("name", list(POSES))
@pytest.mark.parametrize("mode", ["CFS", "PSGCFS"])
def test_grids_nest_and_the_bound_is_sound(cells, mode, name):
    c, r = _posed(cells, mode, name)
    a16, a64 = _audit(c, r, 16), _audit(c, r, 64)
    assert (a64.dist_path <= a16.dist_path).all() and (a16.dist_path <= a16.dist_wp).all()
    np.testing.assert_array_equal(a64.dist_wp, a16.dist_wp)
    ok = r.status <= 1
    assert ok.any() or (mode, name) == ("CFS", "general-axis")
    assert (a16.dist_lower <= a64.dist_path)[ok].all() and (a64.dist_lower <= a64.dist_path)[ok].all()


def test_results_do_not_depend_on_the_batch_the_query_variant_or_the_call(cells):
    c, r = _posed(cells, "PSGCFS", "general-axis")
    want = _audit(c, r, 16)
    _same(_audit(c, r, 16), want, msg="second call")
    for b in range(3):
        got = _audit(c, r, 16, sl=slice(b, b + 1))
        for k in ALL + ("short_by",):
            np.testing.assert_array_equal(getattr(got, k), getattr(want, k)[b:b + 1], err_msg=f"problem {b} alone {k}")
    for S in (5, 16):
        res = {}
        for variant, flags in (("cold", dict(clear_no_bound=True)), ("bound", {}), ("seed", dict(clear_no_bound=True, clear_seed=True)),
                               ("both", dict(clear_seed=True))):
            c.h.debug_options(**flags)
            res[variant] = _audit(c, r, S)
        c.h.debug_options()
        for variant in ("bound", "seed", "both"):
            _same(res[variant], res["cold"], keys=OUT, msg=f"S={S} {variant}")
        np.testing.assert_array_equal(res["bound"].tri_path, res["cold"].tri_path)


def test_two_meshes_in_either_order_and_new_poses_after_an_audit(gpu, cells):
    """the columns follow the meshes; and set_mesh_motion between two audits of the same S invalidates the pose table"""
    c, r = _posed(cells, "CFS", "vertical")
    a = _audit(c, r, 16)
    swapped = _Cell(gpu, c.s, "CFS", [c.tris[1], c.tris[0]], B=3)
    swapped.h.set_mesh_motion([EYE, POSES["vertical"]])
    perm = [0, 2, 1]
    b = swapped.h.clearance_mesh_motion(r.x_, r.u, c.xR1, c.obs, substeps=16)
    for k in ALL:
        np.testing.assert_array_equal(getattr(a, k), getattr(b, k)[:, perm], err_msg=k)
    c.h.set_mesh_motion([POSES["general-axis"], EYE])                      # other poses, the same S: the table is rebuilt
    a2 = _audit(c, r, 16)
    assert np.abs(a2.dist_path[:, 1] - a.dist_path[:, 1]).max() > 1e-4
    swapped.h.set_mesh_motion([EYE, POSES["general-axis"]])
    b2 = swapped.h.clearance_mesh_motion(r.x_, r.u, c.xR1, c.obs, substeps=16)
    for k in ALL:
        np.testing.assert_array_equal(getattr(a2, k), getattr(b2, k)[:, perm], err_msg=f"new poses {k}")
    c.h.set_mesh_motion([POSES["vertical"], EYE])                          # and back: the first table's results again
    _same(_audit(c, r, 16), a, msg="back to the first poses")
    swapped.close()


def test_device_entry_behind_a_solve_on_one_stream(cells):
    """a solve and the audit of its outputs enqueued on a non-default stream with no host sync in between"""
    import torch
    c, r = _posed(cells, "CFS", "vertical")
    want = _audit(c, r, 16)                             # the workspace and the table exist: the device entry only enqueues
    dev = torch.device("cuda:0")
    t = lambda a: torch.tensor(np.ascontiguousarray(a), dtype=torch.float64, device=dev)  # noqa: E731
    args = [t(a) for a in (c.x_init, c.xR1, c.ff, c.caug, c.obs)]
    torch.cuda.synchronize()
    st = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(st):
        out = c.h.solve_device(*args, stream=st.cuda_stream)
        aud = c.h.clearance_mesh_motion_device(out.x_, out.u, args[1], args[4], substeps=16, stream=st.cuda_stream)
    st.synchronize()
    np.testing.assert_array_equal(out.x_.cpu().numpy(), r.x_)
    for k in ALL + ("short_by",):
        np.testing.assert_array_equal(getattr(aud, k).cpu().numpy(), getattr(want, k), err_msg=k)


def test_refusals_write_nothing(gpu, cells):
    c, r = _posed(cells, "CFS", "vertical")
    lib, n = gpu.lib(), 2
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    x_, u, x1, ob = (np.ascontiguousarray(a[:n]) for a in (r.x_, r.u, c.xR1, c.obs))
    o = [np.full((n, 3), -7.0) for _ in range(4)] + [np.full((n, 3), -7, np.int32) for _ in range(2)]
    base = [x_, u, x1, ob] + o
    call = lambda h, B, S, arrs, fn="cfs_clearance_mesh_motion": getattr(lib, fn)(h._h, B, S, *[None if a is None else p(a) for a in arrs])  # noqa: E731
    assert call(c.h, 0, 16, base) == -1 and call(c.h, 4, 16, base) == -1
    assert call(c.h, n, 0, base) == -1 and call(c.h, n, 65, base) == -1 and b"substeps" in lib.cfs_last_error()
    for i in range(len(base)):
        assert call(c.h, n, 16, base[:i] + [None] + base[i + 1:]) == -1
    assert call(c.h, n, 4, base, "cfs_clearance_mesh") == -1 and b"mesh motion" in lib.cfs_last_error()   # the static audit still refuses
    bare = gpu.CFSBatch(c.s, 3, [M.EPS_MARGIN] * 3, mode="CFS", max_batch=3)          # no meshes
    assert call(bare, n, 16, base) == -1 and b"mesh obstacles" in lib.cfs_last_error()
    with pytest.raises(ValueError, match="mesh"):
        bare.clearance_mesh_motion(x_, u, x1, ob)
    bare.close()
    jump = POSES["vertical"].copy()
    jump[7:] = M.pose_about([0, 0, 1], [M.C_POST[0], M.C_POST[1], 0.0], 1.6, [0, 0, 0]) @ jump[7:]   # 1.65 rad between waypoints 7 and 8
    c.h.set_mesh_motion([jump, EYE])                    # the solvers take it: only the audit interpolates
    assert c.solve().status.shape == (3,)
    assert call(c.h, n, 16, base) == -1
    msg = lib.cfs_last_error()
    assert b"quarter turn" in msg and b"mesh 0" in msg and b"waypoints 7 and 8" in msg
    with pytest.raises(gpu.CfsError, match="quarter turn"):
        _audit(c, r, 16)
    assert all((a == -7).all() for a in o)
    jump[7:] = POSES["vertical"][7:]
    jump[7:] = M.pose_about([0, 0, 1], [M.C_POST[0], M.C_POST[1], 0.0], 1.4, [0, 0, 0]) @ jump[7:]   # 1.45 rad: inside the quarter turn
    c.h.set_mesh_motion([jump, EYE])
    assert call(c.h, n, 16, base) == 0 and all((a != -7).all() for a in o)


def test_a_six_joint_robot_against_a_turning_box(gpu, O):
    """M16iB with 6 joints, H = 20, S = 3 (61 samples), a 48-triangle box that travels and turns about a skew axis through a point
    off its centre: other joint counts and a tiny hierarchy take other paths.  The audit needs a rollout, not a solution"""
    nj, H, S = 6, 20, 3
    robot, orobot = gpu.robotproperty2("M16iB"), O.robotproperty2("M16iB")
    rng = np.random.default_rng(5)
    x0 = np.array([0.4, 0.3, 0.2, 0.1, -1.2, 0.3])
    u = rng.uniform(-0.06, 0.06, (H, nj))
    xR1 = np.concatenate([x0, rng.uniform(-0.05, 0.05, nj)])
    x_ = O.rollout(H, nj, orobot.delta_t, xR1, u.reshape(-1))
    th = x_.reshape(H, 2 * nj)[:, :nj]
    ends = np.asarray(O.arm_pos(orobot, th[H // 2]))
    ctr = ends[nj - 1, 1] + np.array([0.3, 0.3, 0.3])
    tri = gpu.mesh.box_mesh(ctr - 0.1, ctr + 0.1, n=2)
    assert tri.shape[0] == 48
    P = np.stack([M.pose_about([1, 2, 3], ctr + [0.1, 0.0, 0.05], 0.8 * (i + 1) / H, [0.0, -0.15 * (i + 1) / H, 0.05 * (i + 1) / H])
                  for i in range(H)])
    s = gpu.build_sys_info(robot, nj, H, x0, th[-1], x_, Qp=np.eye(nj), Qv=np.eye(nj), Rblk=np.eye(nj) * 2, cR=50.0, lim=np.ones(nj),
                           max_input_blk=np.ones(nj), epsilon_O=0.05, MAX_O_ITER=1)
    mesh = gpu.Mesh(tri=tri)
    h = gpu.CFSBatch(s, 1, [0.1], mode="CFS", max_batch=1)
    h.set_meshes([mesh])
    h.set_mesh_motion([P])
    got = h.clearance_mesh_motion(x_[None], u.reshape(1, -1), xR1[None], np.zeros((1, 1, 6)), substeps=S)
    want = CM.audit(O, orobot, H, nj, orobot.delta_t, x_, u.reshape(-1), xR1, np.zeros((0, 6)), [tri], [P], S)
    assert np.abs(want.D).min() > 2e-4
    dev = max(float(np.abs(getattr(got, k)[0] - getattr(want, k)).max()) for k in DIST)
    print(f"M16iB nj=6 H=20 S=3: max deviation {dev:.3e} m, dist_path {got.dist_path[0, 0]:.7f} gap {want.gap[0]:.3e}")
    assert dev <= 1e-10
    if want.gap[0] > 1e-9:
        assert got.link_path[0, 0] == want.link_path[0] and got.t_path[0, 0] == want.t_path[0]
    assert 0 <= got.tri_path[0, 0] < 48 and want.v_mesh[0, 0] == 0.0 and want.v_mesh[0, 1:].min() > 0.0   # moving in every interval but the held first
    h.close(), mesh.close()


def test_the_plan_keeps_its_margin_at_the_waypoints_and_the_audit_finds_it_short(gpu, O):
    """what the audit is for: PSGCFS, H = 30, planned on the posed handle.  The reference's audit of the same plan is the yardstick
    (1e-10 m); the plan reads its margin D = 0.2 at the waypoints to the linearisation's 1e-3, and the audit finds it more than
    5 cm short of it (measured 0.1201329 m, at t = 0: the start pose, which no collision row covers, against the mesh held at
    pose 1 over the first interval)"""
    H, off, dy, ang = M.CASES.psg
    tri, P = M.post_and_ball(gpu.mesh, off), M.poses_z(H, dy, ang)
    c = _Cell(gpu, M.fanuc(gpu, H), "PSGCFS", [tri])
    c.h.set_mesh_motion([P])
    r = c.solve()
    assert r.status[0] == 1
    got = _audit(c, r, 16)
    want = _reference(O, c, r, 0, [P], 16, tris=[tri], H=H)
    _parity(got, 0, want, "PSGCFS H=30 on the posed handle")
    assert got.dist_wp[0, 1] > M.D_MARGIN - 1e-3 and got.dist_path[0, 1] < M.D_MARGIN - 0.05
    assert abs(got.short_by[0] - (M.D_MARGIN - got.dist_path[0].min())) < 1e-15 and got.short_by[0] > 0.05
    assert 0.0 < got.dist_lower[0, 1] <= got.dist_path[0, 1]
    c.close()


def test_audit_mesh_motion_leaves_the_solve_untouched(gpu):
    """audit_mesh_motion=S changes nothing the solve returns and attaches the handle's own audit of the returned plan"""
    R, s, obs = gpu.main_FANUC_problem()
    tri, P = M.post_and_ball(gpu.mesh, 0.05), M.poses_z(s.H, -0.3, 0.6)
    mesh = gpu.Mesh(tri=tri)
    cell = obs + [dict(mesh=mesh, D=0.2, epsilon=0.25, pose=P)]
    a = gpu.CFS_FANUC(cell, s, R).optimizer()
    b = gpu.CFS_FANUC(cell, s, R, audit_mesh_motion=8).optimizer()
    assert a.clearance_mesh_motion is None and b.clearance_mesh is None and b.clearance is None
    for f in ("u", "x_", "iter_O", "total_iter", "status"):
        np.testing.assert_array_equal(getattr(a, f), getattr(b, f), err_msg=f)
    m8 = b.clearance_mesh_motion
    assert m8.dist_path.shape == (len(cell),) and isinstance(m8.short_by, float) and (m8.dist_path <= m8.dist_wp).all()
    want = b._batch.clearance_mesh_motion(b.x_[None], b.u[None], *[b._args()[i] for i in (0, 3)], substeps=8)
    for k in ALL:
        np.testing.assert_array_equal(getattr(m8, k), getattr(want, k)[0], err_msg=k)
    with pytest.raises(ValueError, match="audit_mesh"):
        gpu.CFS_FANUC(cell, s, R, audit_mesh=8)
    mesh.close()
