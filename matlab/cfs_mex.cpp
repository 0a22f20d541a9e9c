// cfs_mex.cpp -- MEX gateway over include/cfs_hip.h.
// Build on a machine with MATLAB + ROCm:  mex -I../include cfs_mex.cpp -L../motionplanning_5d_m_amd -lcfs_hip
// (not compiled in the build image: no MATLAB, no mex.h; the C ABI underneath is what the test suite exercises).
//
//   [u, x_, cost_all, e_cost_all, e_u_all, iter_O, total_iter, status] = cfs_mex('solve', mode, obs, sys_info, ROBOT, noise)
//        mode 0 = CFS_FANUC.optimizer (Lib/CFS_FANUC.m:62-79), 1 = PSGCFS_FANUC.optimizer (Lib/PSGCFS_FANUC.m:65-82);
//        obs = the reference's obs cell (obs{j}.l 3x2, .epsilon, .D; obs{j}.mesh = handle for a mesh obstacle, last in the cell);
//        noise = nn x rows matrix of normrnd(0,0.1) draws consumed one column per PSG step (PSGCFS_FANUC.m:109), or []
//   [Ainq, binq] = cfs_mex('get_con', mode, obs, sys_info, ROBOT, x_, u)   % self.get_con() (Lib/CFS_FANUC.m:101-135): dense, reference row order
//   [dist_path, dist_lower, dist_wp, t_path, link_path] = cfs_mex('clearance', mode, obs, sys_info, ROBOT, x_, u, substeps)
//        audit of a solved trajectory (x_, u as 'solve' returns them) between its waypoints, nobs x 1 each: the smallest distance over
//        substeps (default 16, 1..64) samples per interval, a certified lower bound over continuous time, the smallest distance at
//        the waypoints, and when / on which link the path minimum occurs (cfs_clearance, include/cfs_hip.h); no mesh obstacles
//   [dist_path, dist_lower, dist_wp, t_path, link_path, tri_path] = cfs_mex('clearance_mesh', mode, obs, sys_info, ROBOT, x_, u, substeps)
//        the same for an obs cell with at least one mesh obstacle (cfs_clearance_mesh): every column, and per mesh column the closest
//        triangle of the mesh's list at the path minimum (1-based; 0 in line columns)
//   [dist_path, dist_lower, dist_wp, t_path, link_path, tri_path] = cfs_mex('clearance_mesh_motion', mode, obs, sys_info, ROBOT, x_, u, substeps)
//        the same where mesh entries carry obs{j}.pose (cfs_clearance_mesh_motion): the meshes are placed by the interpolated pose
//        between the waypoints and dist_lower carries their surface speed; 'clearance_mesh' itself keeps refusing the field
//   [u, x_, cost_all, e_cost_all, e_u_all, iter_O] = cfs_mex('chomp', obs_, sys_info, ROBOT, uref)   % CHOMP_FANUC.optimizer (Lib/CHOMP_FANUC.m:54-69);
//        obs_ = the reference's cell: obs_{1}.num_obs followed by the obstacles (M16iB/CHOMP.m:26-29)
//   [d, linkid, grad] = cfs_mex('dist_arm', theta, obs_l, robot, ROBOT)  % dist_arm_3D_200i_2 / dist_arm_3D_Heu_2 / dist_arm_2L(theta, base, obs_l, robot)
//        theta = njoint x N (one pose per column), obs_l = 3x2 obstacle axis (or 6 x nobs, one [l(:,1); l(:,2)] per column): the
//        geometry kernel RRT_FANUC.feasible (Lib/RRT_FANUC.m:146-181) and get_con (Lib/CFS_FANUC.m:115) call; d, linkid = nobs x N;
//        grad (when asked for) = njoint x (nobs*N), column (n-1)*nobs+j = the analytic d(d(j,n))/d(theta(:,n)) (cfs_dist_arm_grad)
//   'solve' and 'get_con' honour an optional sys_info.jacobian = 'fd_literal' (default, num_jac.m) | 'analytic' (include/cfs_hip.h)
//   'solve' and 'get_con' honour an optional sys_info.joint_limits = njoint x 2 [lo, hi] (rad, bounds on x_; cfs_problem_set_joint_limits):
//   every QP keeps the waypoints inside, and get_con returns 2*H*njoint more rows (+pos (i,c), then -pos (i,c))
//   'solve' and 'get_con' accept moving obstacles: obs{j}.l may be 3x2xH (page i = the axis at waypoint i); any such entry makes
//   the handle CFS_OBS_PER_WAYPOINT and the 3x2 entries are held over the horizon (include/cfs_hip.h, moving obstacles)
//   [route, all_nodes, total_dis, all_ee, fail, node_num] = cfs_mex('rrt', obs, sys_info, goal, region_g, region_s, sample_off, ROBOT, SOLVER, U)
//        obs may end with mesh obstacles (obs{j}.mesh, obs{j}.D), received as 'clearance_mesh' receives them: cfs_rrt_grow_mesh
//        RRT_FANUC(obs, sys_info, goal, region_g, region_s, sample_off, ROBOT, SOLVER).find_route() (Lib/RRT_FANUC.m:48-91) grown on the GPU;
//        U = rand(ndraw, S): MATLAB's own rand, consumed per tree exactly as find_route consumes it (one per proposal + nstate for a random
//        sample); S > 1 grows S seeds at once (s_Parallel_rrt.m:16's parfor) and the outputs become cells
//   [theta, status, err_pos, clearance, selected, n_ok, err_axis] = cfs_mex('ik', obs, robot, ROBOT, target_pos, target_axis, theta_ref, opts)
//        goal configurations for Cartesian targets (cfs_ik_solve, include/cfs_hip.h "inverse kinematics"): target_pos 3 x T, target_axis
//        3 x T or [] (position only), theta_ref njoint x T (njoint = its rows); obs = line obstacles (.l, .D; may be {}), a mesh obstacle
//        is refused; opts (optional struct): lo, hi (default robot.thetamax(1:njoint,:)), tool, tool_axis (default robot.cap{njoint}.p(:,1)
//        and the unit vector towards p(:,2)), weight, restarts (64), max_iter (100), tol_pos (1e-6), tol_axis (1e-6), seed (0).
//        theta njoint x T (NaN columns where status ~= 0), the others 1 x T; selected is 1-based (0: none)
//   [theta, status, err_pos, clearance, selected, n_ok, err_axis] = cfs_mex('ik_mesh', obs, robot, ROBOT, target_pos, target_axis, theta_ref, opts)
//        'ik' in a cell that ends with mesh obstacles (obs{j}.mesh, obs{j}.D), received as 'rrt' receives them: cfs_ik_solve_mesh.  A
//        converged restart is also rejected when a link axis comes closer to mesh j than max(D_j, 1e-4); clearance counts the meshes
//   [theta, status, path, clearance, selected, n_ok, n_done] = cfs_mex('cart_path', obs, robot, ROBOT, start, start_state, target_pos, target_axis, theta_ref, opts)
//        straight tool lines from IK candidates (cfs_cart_path, include/cfs_hip.h "Cartesian paths"): start njoint x R x T (or njoint x
//        (R*T), candidate r of target t in column (t-1)*R + r), start_state R x T or [] (every start is used), target_pos 3 x T,
//        target_axis 3 x T or [] (position only), theta_ref njoint x T; obs = line obstacles (.l, .D; may be {}), a mesh obstacle is
//        refused; opts (optional struct): lo, hi, tool, tool_axis, weight, tol_pos, tol_axis as for 'ik', steps (16), max_iter (20),
//        max_joint_step (0.2).  theta njoint x T (the winner's start; NaN columns where status ~= 0), path njoint x ((steps+1)*T)
//        (reshape(path, njoint, steps+1, T)), the others 1 x T; selected is 1-based (0: none)
//   [theta, status, path, clearance, selected, n_ok, n_done] = cfs_mex('cart_path_mesh', obs, robot, ROBOT, start, start_state, target_pos, target_axis, theta_ref, opts)
//        'cart_path' in a cell that ends with mesh obstacles (obs{j}.mesh, obs{j}.D), received as 'ik_mesh' receives them:
//        cfs_cart_path_mesh.  A line also ends at the first configuration whose link axes come closer to mesh j than max(D_j, 1e-4);
//        clearance counts the meshes
//   [theta, status, path, clearance, selected, n_ok, n_done] = cfs_mex('cart_follow', obs, robot, ROBOT, start, start_state, path_pos, path_axis, theta_ref, opts)
//        polylines of tool poses from IK candidates (cfs_cart_follow, include/cfs_hip.h "Tool paths"): the arguments, options and
//        outputs of 'cart_path', parsed by the same code, with path_pos 3 x M x T (or 3 x (M*T)) and path_axis the same shape or [] in
//        the place of the target; opts.steps (16) is the number of sub-steps per segment, so a path has N = (M-1)*steps + 1 <= 257 rows
//        and path is njoint x (N*T) (reshape(path, njoint, N, T)).  Row 1 of a path is a pose to reach, not the start: theta is the start
//   [theta, status, path, clearance, selected, n_ok, n_done] = cfs_mex('cart_follow_mesh', obs, robot, ROBOT, start, start_state, path_pos, path_axis, theta_ref, opts)
//        'cart_follow' in a cell that ends with mesh obstacles, received as 'cart_path_mesh' receives them: cfs_cart_follow_mesh
//   [time, sdot, duration, status, selected, group_status] = cfs_mex('path_time', robot, ROBOT, paths, dims, state, vmax, amax, opts)
//        a clock on joint paths (cfs_path_time, include/cfs_hip.h "Path timing"): paths njoint x N x R x G -- reshape(path, njoint, N, 1, T)
//        of 'cart_follow' / 'cart_path', or their candidates --, dims = [N R G] (a 4-D array arrives as njoint x (N*R*G)), state R x G
//        or [] (a path is timed only where its entry is 0), vmax / amax njoint x 1 (rad/s, rad/s^2).  opts: feed (m/s; default Inf: no
//        cap), tool (3 x 1; default the end effector), curve_share (default 0.5), stop_every (default 0: rest at the two ends only; k >= 2:
//        also at every row that is a multiple of k, counted from 0).  time and sdot are N x (R*G) (reshape(time, N, R, G)), duration and
//        status R x G (0 timed | 1 not timed | 2 numeric | 3 stalled | 4 repeated row; NaN rows where not 0), selected 1 x G (1-based, 0
//        without a timed path), group_status 1 x G
//   [clear_lower, chord_upper, state_out, status, clear_path, s_path, link_path, obs_path, clear_rows, chord_err] = ...
//        cfs_mex('path_audit', obs, robot, ROBOT, paths, dims, state, opts)
//        what joint paths do between their rows (cfs_path_audit, include/cfs_hip.h "Tool-path audit"): paths, dims = [N R G] and state as
//        for 'path_time', with N >= 2; obs the cell of line obstacles (mesh obstacles are not audited).  opts: substeps (default 8),
//        min_clearance (m; default -Inf: no test), max_chord (m; default Inf: no test), tool (3 x 1; default the end effector).  Every
//        output is R x G: the certified clearance and chord deviation, state_out (state, else 3 non-finite | 6 clear_lower <
//        min_clearance | 7 chord_upper > max_chord | 0: goes into 'path_time' as its state), status (0 audited | 1 not audited | 2
//        non-finite; NaN where not 0), the sampled clearance with its place (s_path counts rows from 0; link_path 1-based; obs_path
//        1-based, 0 without obstacles or where not audited), the clearance at the rows and the sampled chord deviation
//   Cost_b = cfs_mex('cost_b', sys_info, ROBOT)                    % EVAL.get_Cost_b (Lib/EVAL.m:75-78, main_FANUC.m:131-132)
//   h = cfs_mex('mesh_load_stl', path, scale, map_from_stl)        % Lib/functions/MapFromSTL.m
//   [dis, points] = cfs_mex('mesh_segment_distance', h, seg6)      % point2surface_dis (M200i/dist_arm_surf_200i.m:21)
//   cfs_mex('mesh_destroy', h)
#include "mex.h"
#include "cfs_hip.h"
#include <cmath>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

static double field_scalar(const mxArray *s, const char *name)
{
    const mxArray *f = mxGetField(s, 0, name);
    if (!f) mexErrMsgIdAndTxt("cfs:field", "sys_info.%s is missing", name);
    return mxGetScalar(f);
}
static double *field_ptr(const mxArray *s, const char *name, bool required = true)
{
    const mxArray *f = mxGetField(s, 0, name);
    if (!f) { if (required) mexErrMsgIdAndTxt("cfs:field", "sys_info.%s is missing", name); return nullptr; }
    return mxGetPr(f);
}
static void check(int rc) { if (rc != CFS_SUCCESS) mexErrMsgIdAndTxt("cfs:abi", "%s", cfs_last_error()); }
static cfs_mesh *mesh_of(const mxArray *h) { return reinterpret_cast<cfs_mesh *>(static_cast<uintptr_t>(*static_cast<uint64_t *>(mxGetData(h)))); }

static void fill_robot(const mxArray *robot, const char *ROBOT, int nj, cfs_robot &r)
{
    memset(&r, 0, sizeof r);
    r.kind = !strcmp(ROBOT, "M200i") ? CFS_ROBOT_M200I : (!strcmp(ROBOT, "2L") ? CFS_ROBOT_2L : CFS_ROBOT_M16IB);   // CFS_FANUC.m:49-54
    const mxArray *DH = mxGetField(robot, 0, "DH"), *cap = mxGetField(robot, 0, "cap"), *T = mxGetField(robot, 0, "T");
    r.nlink = r.kind == CFS_ROBOT_2L ? nj : (int)mxGetM(DH);
    if (DH) memcpy(r.DH, mxGetPr(DH), sizeof(double) * 4 * r.nlink);                 // nlink x 4, column-major as MATLAB holds it
    memcpy(r.base, mxGetPr(mxGetField(robot, 0, "base")), sizeof(double) * 3);
    for (int i = 0; i < r.nlink && i < (int)mxGetNumberOfElements(cap); ++i)          // robot.cap{i}.p is 3x2 = [p1 p2]
        memcpy(r.cap + 6 * i, mxGetPr(mxGetField(mxGetCell(cap, i), 0, "p")), sizeof(double) * 6);
    if (T) memcpy(r.T, mxGetPr(T), sizeof(double) * 9);                              // 2L: robot.T (robotproperty2.m:117-119)
    r.delta_t = mxGetScalar(mxGetField(robot, 0, "delta_t"));
}

// the problem-family handle of one MATLAB object: obs cell (first = index of the first obstacle in it) + sys_info + ROBOT
struct Family {
    cfs_problem *p = nullptr;
    cfs_problem_desc d;
    std::vector<double> margin, obs6, Dv, epsv;
    ~Family() { if (p) cfs_problem_destroy(p); }
};
// moving (solve, get_con): obs{j}.l may be 3x2xH; obs6 is then H x nobs x 6 and the handle CFS_OBS_PER_WAYPOINT
static void make_family(Family &f, int mode, const mxArray *obs, int first, int nobs, const mxArray *S, const char *ROBOT, bool need_both = false,
                        bool moving = false)
{
    cfs_problem_desc &d = f.d;
    memset(&d, 0, sizeof d);
    d.mode = mode;
    d.H = (int)field_scalar(S, "H");
    d.njoint = (int)field_scalar(S, "njoint");
    d.nobs = nobs;
    fill_robot(mxGetField(S, 0, "robot"), ROBOT, d.njoint, d.robot);
    d.QQ = field_ptr(S, "QQ"); d.Aaug = field_ptr(S, "Aaug"); d.Baug = field_ptr(S, "Baug"); d.lim = field_ptr(S, "lim");
    d.MAX_input = field_ptr(S, "MAX_input", mode == CFS_MODE_CFS);
    d.epsilon_O = field_scalar(S, "epsilon_O");
    d.MAX_O_ITER = (int)field_scalar(S, "MAX_O_ITER");
    d.alpha = mxGetField(S, 0, "alpha") ? field_scalar(S, "alpha") : 0.0;
    d.max_batch = 1;
    const size_t H = (size_t)d.H;
    bool per_wp = false;                                   // some obs{j}.l is 3x2xH
    if (moving && H > 1)
        for (int j = 0; j < nobs; ++j) {
            const mxArray *o = mxGetCell(obs, first + j);
            const mxArray *fl = o ? mxGetField(o, 0, "l") : nullptr;
            if (fl && !mxGetField(o, 0, "mesh") && mxGetNumberOfElements(fl) == 6 * H) per_wp = true;
        }
    const size_t nrow = per_wp ? H : 1;                    // obstacle rows per obstacle
    f.margin.assign(nobs, 0.0); f.obs6.assign(6 * (size_t)nobs * nrow, 0.0); f.Dv.assign(nobs, 0.0); f.epsv.assign(nobs, 0.0);
    std::vector<const cfs_mesh *> meshes;
    std::vector<double> poses;                             // nmesh x H x 12, row-major [R | t] per waypoint (cfs_problem_set_mesh_motion)
    bool posed = false;                                    // some mesh entry carries .pose
    for (int j = 0; j < nobs; ++j) {
        const mxArray *o = mxGetCell(obs, first + j);
        if (!o) mexErrMsgIdAndTxt("cfs:obs", "obs{%d} is empty", first + j + 1);
        // the margin field the mode reads must exist (CFS_FANUC.m:117 reads .epsilon, PSGCFS_FANUC.m:158 reads .D); the other one is
        // optional (0) -- a cell written for one solver need not carry the other solver's field
        const mxArray *fD = mxGetField(o, 0, "D"), *fE = mxGetField(o, 0, "epsilon");
        if (!(mode == CFS_MODE_CFS ? fE : fD))
            mexErrMsgIdAndTxt("cfs:obs", "obs{%d}.%s is missing", first + j + 1, mode == CFS_MODE_CFS ? "epsilon" : "D");
        if (need_both && !(fD && fE)) mexErrMsgIdAndTxt("cfs:obs", "obs_{%d} needs both .D and .epsilon (Lib/CHOMP_FANUC.m:95-96)", first + j + 1);
        f.Dv[j] = fD ? mxGetScalar(fD) : 0.0;
        f.epsv[j] = fE ? mxGetScalar(fE) : 0.0;
        f.margin[j] = mode == CFS_MODE_CFS ? f.epsv[j] : f.Dv[j];
        const mxArray *mh = mxGetField(o, 0, "mesh");
        if (mh) {
            meshes.push_back(mesh_of(mh));
            // optional obs{j}.pose: 3x4xH or 4x4xH (page i = the mesh's pose at waypoint i), or one 3x4 / 4x4 held over the horizon;
            // a mesh entry without it is held still (identity)
            const size_t at = poses.size();
            poses.resize(at + 12 * H, 0.0);
            for (size_t i = 0; i < H; ++i) poses[at + 12 * i] = poses[at + 12 * i + 5] = poses[at + 12 * i + 10] = 1.0;
            if (const mxArray *fp = mxGetField(o, 0, "pose")) {
                if (!moving) mexErrMsgIdAndTxt("cfs:obs", "obs{%d}.pose: only 'solve' and 'get_con' place a mesh per waypoint", first + j + 1);
                const size_t rows = mxGetM(fp), ne = mxGetNumberOfElements(fp);
                if (mxIsChar(fp) || (rows != 3 && rows != 4) || (ne != 4 * rows && ne != 4 * rows * H))
                    mexErrMsgIdAndTxt("cfs:obs", "obs{%d}.pose must be 3x4xH or 4x4xH (or one 3x4 / 4x4)", first + j + 1);
                for (size_t i = 0; i < H; ++i) {
                    const double *pg = mxGetPr(fp) + (ne == 4 * rows ? 0 : 4 * rows * i);   // column-major page
                    for (size_t r = 0; r < 3; ++r)
                        for (size_t c = 0; c < 4; ++c) poses[at + 12 * i + 4 * r + c] = pg[c * rows + r];
                    if (rows == 4 && !(pg[3] == 0.0 && pg[7] == 0.0 && pg[11] == 0.0 && pg[15] == 1.0))
                        mexErrMsgIdAndTxt("cfs:obs", "obs{%d}.pose: the last row of a 4x4 pose must be [0 0 0 1]", first + j + 1);
                }
                posed = true;
            }
        }
        else if (!meshes.empty()) mexErrMsgTxt("mesh obstacles must come last in the obs cell");
        else {
            const mxArray *fl = mxGetField(o, 0, "l");
            const size_t ne = fl ? mxGetNumberOfElements(fl) : 0;
            if (ne != 6 && !(per_wp && ne == 6 * H))
                mexErrMsgIdAndTxt("cfs:obs", moving ? "obs{%d}.l must be 3x2 or 3x2xH" : "obs{%d}.l must be 3x2", first + j + 1);
            for (size_t i = 0; i < nrow; ++i)                                        // row [i][j] = [l(:,1,i); l(:,2,i)]
                memcpy(&f.obs6[6 * (i * (size_t)nobs + j)], mxGetPr(fl) + (ne == 6 ? 0 : 6 * i), sizeof(double) * 6);
        }
    }
    if (per_wp && !meshes.empty()) mexErrMsgTxt("mesh obstacles are static: they cannot share an obs cell with 3x2xH axes");
    d.margin = f.margin.data();
    check(cfs_problem_create(&d, &f.p));
    if (per_wp) check(cfs_problem_set_obstacle_motion(f.p, CFS_OBS_PER_WAYPOINT));
    if (!meshes.empty()) check(cfs_problem_set_meshes(f.p, (int)meshes.size(), meshes.data()));
    if (posed) check(cfs_problem_set_mesh_motion(f.p, poses.data()));   // rigidity is the library's check
    // optional sys_info.jacobian = 'fd_literal' (num_jac.m, the default) | 'analytic' (cfs_problem_set_jacobian)
    if (const mxArray *fj = mxGetField(S, 0, "jacobian")) {
        if (!mxIsChar(fj)) mexErrMsgIdAndTxt("cfs:field", "sys_info.jacobian must be 'fd_literal' or 'analytic'");
        const std::string jm = mxArrayToString(fj);
        if (jm == "analytic") check(cfs_problem_set_jacobian(f.p, CFS_JAC_ANALYTIC));
        else if (jm != "fd_literal") mexErrMsgIdAndTxt("cfs:field", "sys_info.jacobian must be 'fd_literal' or 'analytic'");
    }
    // optional sys_info.joint_limits = njoint x 2 [lo, hi] (cfs_problem_set_joint_limits; CHOMP_FANUC has no QP to hold them)
    if (const mxArray *fl = need_both ? nullptr : mxGetField(S, 0, "joint_limits")) {
        if (mxIsChar(fl) || (int)mxGetM(fl) != d.njoint || mxGetN(fl) != 2)
            mexErrMsgIdAndTxt("cfs:field", "sys_info.joint_limits must be an njoint x 2 double matrix [lo, hi]");
        const double *jl = mxGetPr(fl);                    // column-major: lo = column 1, hi = column 2
        check(cfs_problem_set_joint_limits(f.p, jl, jl + d.njoint));
    }
}

static void solve(int nlhs, mxArray *plhs[], int nrhs, const mxArray *prhs[])
{
    if (nrhs < 5) mexErrMsgTxt("cfs_mex('solve', mode, obs, sys_info, ROBOT [, noise])");
    const int mode = (int)mxGetScalar(prhs[1]);
    const mxArray *S = prhs[3];
    const std::string ROBOT = mxArrayToString(prhs[4]);
    Family f;
    make_family(f, mode, prhs[2], 0, (int)mxGetNumberOfElements(prhs[2]), S, ROBOT.c_str(), false, true);
    const cfs_problem_desc &d = f.d;
    const int nn = d.H * d.njoint, nx = d.H * 2 * d.njoint, K = d.MAX_O_ITER;
    double caug = field_scalar(S, "caug");
    cfs_batch_in in;
    memset(&in, 0, sizeof in);
    in.B = 1;
    in.x_init = field_ptr(S, "x_"); in.xR1 = field_ptr(S, "xR"); in.ff = field_ptr(S, "ff"); in.caug = &caug; in.obs = f.obs6.data();
    if (nrhs > 5 && !mxIsEmpty(prhs[5])) { in.noise = mxGetPr(prhs[5]); in.noise_rows = (int)mxGetN(prhs[5]); }   // nn x rows, one column per draw
    mxArray *o_u = mxCreateDoubleMatrix(nn, 1, mxREAL), *o_x = mxCreateDoubleMatrix(nx, 1, mxREAL);
    mxArray *o_c = mxCreateDoubleMatrix(K, 1, mxREAL), *o_ec = mxCreateDoubleMatrix(K, 1, mxREAL), *o_eu = mxCreateDoubleMatrix(K, 1, mxREAL);
    int iter_O = 1, total_iter = 0, status = 0;
    cfs_batch_out out;
    out.u = mxGetPr(o_u); out.x_ = mxGetPr(o_x); out.cost_all = mxGetPr(o_c); out.e_cost_all = mxGetPr(o_ec); out.e_u_all = mxGetPr(o_eu);
    out.iter_O = &iter_O; out.total_iter = &total_iter; out.status = &status;
    check(cfs_solve_batch(f.p, &in, &out));
    mxArray *outs[8] = {o_u, o_x, o_c, o_ec, o_eu, mxCreateDoubleScalar(iter_O), mxCreateDoubleScalar(total_iter), mxCreateDoubleScalar(status)};
    for (int k = 0; k < 8; ++k) { if (k < nlhs || k == 0) plhs[k] = outs[k]; else mxDestroyArray(outs[k]); }
}

// self.get_con(): dense self.Ainq / self.binq at the object's current (x_, u)  (Lib/CFS_FANUC.m:101-135, PSGCFS_FANUC.m:145-184)
static void get_con(int nlhs, mxArray *plhs[], int nrhs, const mxArray *prhs[])
{
    if (nrhs < 7) mexErrMsgTxt("[Ainq, binq] = cfs_mex('get_con', mode, obs, sys_info, ROBOT, x_, u)");
    const int mode = (int)mxGetScalar(prhs[1]);
    const std::string ROBOT = mxArrayToString(prhs[4]);
    Family f;
    make_family(f, mode, prhs[2], 0, (int)mxGetNumberOfElements(prhs[2]), prhs[3], ROBOT.c_str(), false, true);
    int on = 0;
    check(cfs_problem_get_joint_limits(f.p, &on, nullptr, nullptr));
    const int nn = f.d.H * f.d.njoint, rows = f.d.nobs * f.d.H * (1 + 2 * f.d.njoint) + (on ? 2 * nn : 0);
    mxArray *A = mxCreateDoubleMatrix(rows, nn, mxREAL), *b = mxCreateDoubleMatrix(rows, 1, mxREAL);
    check(cfs_get_con(f.p, 1, mxGetPr(prhs[5]), mxGetPr(prhs[6]), field_ptr(prhs[3], "xR"), f.obs6.data(), mxGetPr(A), mxGetPr(b)));
    plhs[0] = A;
    if (nlhs > 1) plhs[1] = b; else mxDestroyArray(b);
}

// clearance of a solved trajectory along the motion between its waypoints (cfs_clearance; the reference has no counterpart: its
// collision rows, Lib/CFS_FANUC.m:110-120, are written at the waypoints only)
static void clearance(int nlhs, mxArray *plhs[], int nrhs, const mxArray *prhs[])
{
    if (nrhs < 7) mexErrMsgTxt("[dist_path, dist_lower, dist_wp, t_path, link_path] = cfs_mex('clearance', mode, obs, sys_info, ROBOT, x_, u [, substeps])");
    const int mode = (int)mxGetScalar(prhs[1]);
    const std::string ROBOT = mxArrayToString(prhs[4]);
    Family f;
    make_family(f, mode, prhs[2], 0, (int)mxGetNumberOfElements(prhs[2]), prhs[3], ROBOT.c_str(), false, true);
    const int nobs = f.d.nobs, S = nrhs > 7 ? (int)mxGetScalar(prhs[7]) : 16;
    mxArray *o[5];
    for (int k = 0; k < 5; ++k) o[k] = mxCreateDoubleMatrix(nobs, 1, mxREAL);
    std::vector<int> link(nobs, 0);
    check(cfs_clearance(f.p, 1, S, mxGetPr(prhs[5]), mxGetPr(prhs[6]), field_ptr(prhs[3], "xR"), f.obs6.data(), mxGetPr(o[2]), mxGetPr(o[0]),
                        mxGetPr(o[1]), mxGetPr(o[3]), link.data()));
    for (int j = 0; j < nobs; ++j) mxGetPr(o[4])[j] = link[j];
    for (int k = 0; k < 5; ++k) { if (k < nlhs || k == 0) plhs[k] = o[k]; else mxDestroyArray(o[k]); }
}

// the same for an obs cell with mesh obstacles (cfs_clearance_mesh): every column, lines first; tri_path is 1-based like MATLAB's
// triangle lists (0 in the line columns)
static void clearance_mesh(int nlhs, mxArray *plhs[], int nrhs, const mxArray *prhs[])
{
    if (nrhs < 7) mexErrMsgTxt("[dist_path, dist_lower, dist_wp, t_path, link_path, tri_path] = cfs_mex('clearance_mesh', mode, obs, sys_info, ROBOT, x_, u [, substeps])");
    const int mode = (int)mxGetScalar(prhs[1]);
    const std::string ROBOT = mxArrayToString(prhs[4]);
    Family f;
    make_family(f, mode, prhs[2], 0, (int)mxGetNumberOfElements(prhs[2]), prhs[3], ROBOT.c_str());   // static rows: a handle with meshes has no others
    const int nobs = f.d.nobs, S = nrhs > 7 ? (int)mxGetScalar(prhs[7]) : 16;
    mxArray *o[6];
    for (int k = 0; k < 6; ++k) o[k] = mxCreateDoubleMatrix(nobs, 1, mxREAL);
    std::vector<int> link(nobs, 0), tri(nobs, -1);
    check(cfs_clearance_mesh(f.p, 1, S, mxGetPr(prhs[5]), mxGetPr(prhs[6]), field_ptr(prhs[3], "xR"), f.obs6.data(), mxGetPr(o[2]), mxGetPr(o[0]),
                             mxGetPr(o[1]), mxGetPr(o[3]), link.data(), tri.data()));
    for (int j = 0; j < nobs; ++j) { mxGetPr(o[4])[j] = link[j]; mxGetPr(o[5])[j] = tri[j] + 1; }
    for (int k = 0; k < 6; ++k) { if (k < nlhs || k == 0) plhs[k] = o[k]; else mxDestroyArray(o[k]); }
}

// the same for an obs cell whose meshes may carry obs{j}.pose (cfs_clearance_mesh_motion): between two waypoints a mesh is placed
// by the interpolated pose and its surface speed enters dist_lower; a cell without poses gives 'clearance_mesh's results
static void clearance_mesh_motion(int nlhs, mxArray *plhs[], int nrhs, const mxArray *prhs[])
{
    if (nrhs < 7) mexErrMsgTxt("[dist_path, dist_lower, dist_wp, t_path, link_path, tri_path] = cfs_mex('clearance_mesh_motion', mode, obs, sys_info, ROBOT, x_, u [, substeps])");
    const int mode = (int)mxGetScalar(prhs[1]);
    const std::string ROBOT = mxArrayToString(prhs[4]);
    Family f;
    make_family(f, mode, prhs[2], 0, (int)mxGetNumberOfElements(prhs[2]), prhs[3], ROBOT.c_str(), false, true);
    const int nobs = f.d.nobs, S = nrhs > 7 ? (int)mxGetScalar(prhs[7]) : 16;
    mxArray *o[6];
    for (int k = 0; k < 6; ++k) o[k] = mxCreateDoubleMatrix(nobs, 1, mxREAL);
    std::vector<int> link(nobs, 0), tri(nobs, -1);
    check(cfs_clearance_mesh_motion(f.p, 1, S, mxGetPr(prhs[5]), mxGetPr(prhs[6]), field_ptr(prhs[3], "xR"), f.obs6.data(), mxGetPr(o[2]),
                                    mxGetPr(o[0]), mxGetPr(o[1]), mxGetPr(o[3]), link.data(), tri.data()));
    for (int j = 0; j < nobs; ++j) { mxGetPr(o[4])[j] = link[j]; mxGetPr(o[5])[j] = tri[j] + 1; }
    for (int k = 0; k < 6; ++k) { if (k < nlhs || k == 0) plhs[k] = o[k]; else mxDestroyArray(o[k]); }
}

// CHOMP_FANUC(obs_, sys_info, uref, ROBOT).optimizer()  (Lib/CHOMP_FANUC.m:34-69; Lib/functions/s_Solver.m:12-21)
static void chomp(int nlhs, mxArray *plhs[], int nrhs, const mxArray *prhs[])
{
    if (nrhs < 5) mexErrMsgTxt("cfs_mex('chomp', obs_, sys_info, ROBOT, uref)");
    const mxArray *S = prhs[2];
    const std::string ROBOT = mxArrayToString(prhs[3]);
    const int nobs = (int)mxGetScalar(mxGetField(mxGetCell(prhs[1], 0), 0, "num_obs"));    // obs_{1}.num_obs (M16iB/CHOMP.m:26)
    Family f;
    make_family(f, CFS_MODE_CFS, prhs[1], 1, nobs, S, ROBOT.c_str(), true);
    const int nn = f.d.H * f.d.njoint, nx = f.d.H * 2 * f.d.njoint, K = f.d.MAX_O_ITER;
    double caug = field_scalar(S, "caug");
    cfs_batch_in in;
    memset(&in, 0, sizeof in);
    in.B = 1;
    in.x_init = field_ptr(S, "x_"); in.xR1 = field_ptr(S, "xR"); in.ff = field_ptr(S, "ff"); in.caug = &caug; in.obs = f.obs6.data();
    mxArray *o_u = mxCreateDoubleMatrix(nn, 1, mxREAL), *o_x = mxCreateDoubleMatrix(nx, 1, mxREAL);
    mxArray *o_c = mxCreateDoubleMatrix(K, 1, mxREAL), *o_ec = mxCreateDoubleMatrix(K, 1, mxREAL), *o_eu = mxCreateDoubleMatrix(K, 1, mxREAL);
    int iter_O = 1;
    cfs_batch_out out;
    memset(&out, 0, sizeof out);
    out.u = mxGetPr(o_u); out.x_ = mxGetPr(o_x); out.cost_all = mxGetPr(o_c); out.e_cost_all = mxGetPr(o_ec); out.e_u_all = mxGetPr(o_eu);
    out.iter_O = &iter_O;
    check(cfs_chomp_batch(f.p, &in, mxGetPr(prhs[4]), f.Dv.data(), f.epsv.data(), &out));
    mxArray *outs[6] = {o_u, o_x, o_c, o_ec, o_eu, mxCreateDoubleScalar(iter_O)};
    for (int k = 0; k < 6; ++k) { if (k < nlhs || k == 0) plhs[k] = outs[k]; else mxDestroyArray(outs[k]); }
}

// [d, linkid] = dist_arm_*(theta, base, obs_l, robot) for N poses x nobs obstacle axes: the primitive under RRT_FANUC.feasible
// (Lib/RRT_FANUC.m:146-181) and get_con (Lib/CFS_FANUC.m:115); matlab/dist_arm_3D_200i_2.m is the one-line shim over it
static void dist_arm(int nlhs, mxArray *plhs[], int nrhs, const mxArray *prhs[])
{
    if (nrhs < 5) mexErrMsgTxt("[d, linkid] = cfs_mex('dist_arm', theta, obs_l, robot, ROBOT)");
    const std::string ROBOT = mxArrayToString(prhs[4]);
    const int nj = (int)mxGetM(prhs[1]), N = (int)mxGetN(prhs[1]);
    if (mxGetNumberOfElements(prhs[2]) % 6) mexErrMsgTxt("obs_l must be 3x2 (or 6 x nobs)");
    const int nobs = (int)(mxGetNumberOfElements(prhs[2]) / 6);
    cfs_robot r;
    fill_robot(prhs[3], ROBOT.c_str(), nj, r);
    std::vector<double> d((size_t)N * nobs);
    std::vector<int> lid((size_t)N * nobs);
    mxArray *og = nullptr;
    if (nlhs > 2) {   // grad = d(d)/d(theta), njoint x nobs x N: the analytic gradient (cfs_dist_arm_grad; N x nobs x njoint row-major)
        og = mxCreateDoubleMatrix(nj, (size_t)nobs * N, mxREAL);
        check(cfs_dist_arm_grad(&r, nj, N, mxGetPr(prhs[1]), nobs, mxGetPr(prhs[2]), d.data(), lid.data(), mxGetPr(og)));
    } else
        check(cfs_dist_arm(&r, nj, N, mxGetPr(prhs[1]), nobs, mxGetPr(prhs[2]), d.data(), lid.data(), nullptr));   // theta njoint x N column-major = N x njoint row-major
    mxArray *od = mxCreateDoubleMatrix(nobs, N, mxREAL), *ol = mxCreateDoubleMatrix(nobs, N, mxREAL);
    for (size_t k = 0; k < d.size(); ++k) { mxGetPr(od)[k] = d[k]; mxGetPr(ol)[k] = lid[k]; }               // N x nobs row-major = nobs x N column-major
    plhs[0] = od;
    if (nlhs > 1) plhs[1] = ol; else mxDestroyArray(ol);
    if (og) plhs[2] = og;
}

// RRT_FANUC.find_route for S = size(U,2) seeds (Lib/RRT_FANUC.m:63-91; Lib/functions/s_Parallel_rrt.m:16-25)
static void rrt(int nlhs, mxArray *plhs[], int nrhs, const mxArray *prhs[])
{
    if (nrhs < 10) mexErrMsgTxt("cfs_mex('rrt', obs, sys_info, goal, region_g, region_s, sample_off, ROBOT, SOLVER, U)");
    const mxArray *obs = prhs[1], *S_ = prhs[2];
    const std::string ROBOT = mxArrayToString(prhs[7]), SOLVER = mxArrayToString(prhs[8]);
    cfs_rrt_desc d;
    memset(&d, 0, sizeof d);
    d.nstate = (int)field_scalar(S_, "nstate");
    fill_robot(mxGetField(S_, 0, "robot"), ROBOT.c_str(), d.nstate, d.robot);
    d.solver = SOLVER == "RRT*" ? CFS_RRT_STAR : CFS_RRT;
    d.max_iter = 400; d.bi = 0.5; d.rewire = 0.2;                                   // class property defaults (Lib/RRT_FANUC.m:37-38, :135)
    d.x0 = field_ptr(S_, "x0"); d.goal_th = field_ptr(S_, "goal_th"); d.ratial = field_ptr(S_, "ratial");
    d.goal = mxGetPr(prhs[3]); d.region_g = mxGetPr(prhs[4]); d.region_s = mxGetPr(prhs[5]); d.sample_off = mxGetPr(prhs[6]);
    // line obstacles (.l, .D) first, then mesh obstacles (.mesh = a handle of cfs_mex('mesh_create' ...), .D): cfs_rrt_grow_mesh
    const int ncell = (int)mxGetNumberOfElements(obs);
    std::vector<double> obs6, D, D_mesh;
    std::vector<const cfs_mesh *> meshes;
    for (int j = 0; j < ncell; ++j) {
        const mxArray *o = mxGetCell(obs, j), *fD = o ? mxGetField(o, 0, "D") : nullptr, *mh = o ? mxGetField(o, 0, "mesh") : nullptr;
        if (mh) {
            if (!fD) mexErrMsgIdAndTxt("cfs:obs", "obs{%d} needs .mesh and .D", j + 1);
            if (mxGetField(o, 0, "pose")) mexErrMsgIdAndTxt("cfs:obs", "obs{%d}.pose: a moving mesh needs a time axis ('solve', 'get_con')", j + 1);
            meshes.push_back(mesh_of(mh));
            D_mesh.push_back(mxGetScalar(fD));
            continue;
        }
        if (!meshes.empty()) mexErrMsgTxt("mesh obstacles must come last in the obs cell");
        const mxArray *fl = o ? mxGetField(o, 0, "l") : nullptr;
        if (!fl || !fD || mxGetNumberOfElements(fl) != 6) mexErrMsgIdAndTxt("cfs:obs", "obs{%d} needs .l (3x2) and .D", j + 1);
        obs6.insert(obs6.end(), mxGetPr(fl), mxGetPr(fl) + 6);
        D.push_back(mxGetScalar(fD));
    }
    d.nobs = (int)D.size(); d.obs = obs6.data(); d.D = D.data();
    const int ndraw = (int)mxGetM(prhs[9]), S = (int)mxGetN(prhs[9]);
    d.uniforms = mxGetPr(prhs[9]); d.ndraw = ndraw;                                 // ndraw x S column-major = S x ndraw row-major
    const size_t N = (size_t)d.max_iter + 1, nj = d.nstate;
    std::vector<int> node_num(S), fail(S), route_len(S), parent(S * N);
    std::vector<double> nodes(S * N * nj), total_dis(S * N), all_ee((size_t)S * d.max_iter * 3), route(S * N * nj);
    cfs_rrt_out o;
    memset(&o, 0, sizeof o);
    o.node_num = node_num.data(); o.fail = fail.data(); o.route_len = route_len.data(); o.parent = parent.data();
    o.nodes = nodes.data(); o.total_dis = total_dis.data(); o.all_ee = all_ee.data(); o.route = route.data();
    if (meshes.empty()) check(cfs_rrt_grow(&d, S, &o));
    else check(cfs_rrt_grow_mesh(&d, (int)meshes.size(), meshes.data(), D_mesh.data(), 0, S, &o));
    mxArray *outs[6];
    for (int k = 0; k < 4; ++k) outs[k] = S > 1 ? mxCreateCellMatrix(1, S) : nullptr;
    outs[4] = mxCreateDoubleMatrix(1, S, mxREAL); outs[5] = mxCreateDoubleMatrix(1, S, mxREAL);
    for (int t = 0; t < S; ++t) {
        const int n = node_num[t], L = route_len[t];
        mxArray *r = mxCreateDoubleMatrix(nj, L, mxREAL), *an = mxCreateDoubleMatrix(nj + 1, n, mxREAL);
        mxArray *td = mxCreateDoubleMatrix(1, n, mxREAL), *ee = mxCreateDoubleMatrix(3, n > 0 ? n - 1 : 0, mxREAL);
        memcpy(mxGetPr(r), &route[(size_t)t * N * nj], sizeof(double) * nj * L);      // rows of `route` are MATLAB's columns
        for (int i = 0; i < n; ++i) {
            mxGetPr(an)[(size_t)i * (nj + 1)] = parent[(size_t)t * N + i];            // all_nodes = [parent; node] (Lib/RRT_FANUC.m:66, :185)
            memcpy(mxGetPr(an) + (size_t)i * (nj + 1) + 1, &nodes[((size_t)t * N + i) * nj], sizeof(double) * nj);
            mxGetPr(td)[i] = total_dis[(size_t)t * N + i];
        }
        if (n > 1) memcpy(mxGetPr(ee), &all_ee[(size_t)t * d.max_iter * 3], sizeof(double) * 3 * (n - 1));
        mxArray *one[4] = {r, an, td, ee};
        for (int k = 0; k < 4; ++k) { if (S > 1) mxSetCell(outs[k], t, one[k]); else outs[k] = one[k]; }
        mxGetPr(outs[4])[t] = fail[t]; mxGetPr(outs[5])[t] = n;
    }
    for (int k = 0; k < 6; ++k) { if (k < nlhs || k == 0) plhs[k] = outs[k]; else mxDestroyArray(outs[k]); }
}

// goal configurations for Cartesian targets (cfs_ik_solve; the reference's drivers type xg in, main_FANUC.m:30, RRTstar_CFS.m:43)
static void ik(int nlhs, mxArray *plhs[], int nrhs, const mxArray *prhs[])
{
    if (nrhs < 7) mexErrMsgTxt("[theta, status, err_pos, clearance, selected, n_ok, err_axis] = cfs_mex('ik', obs, robot, ROBOT, target_pos, target_axis, theta_ref [, opts])");
    const mxArray *obs = prhs[1], *robot = prhs[2], *opts = nrhs > 7 ? prhs[7] : nullptr;
    const std::string ROBOT = mxArrayToString(prhs[3]);
    const int nj = (int)mxGetM(prhs[6]), T = (int)mxGetN(prhs[4]);
    if (mxGetM(prhs[4]) != 3 || (int)mxGetN(prhs[6]) != T) mexErrMsgTxt("target_pos must be 3 x T and theta_ref njoint x T");
    const bool use_axis = !mxIsEmpty(prhs[5]);
    if (use_axis && (mxGetM(prhs[5]) != 3 || (int)mxGetN(prhs[5]) != T)) mexErrMsgTxt("target_axis must be 3 x T or []");
    cfs_ik_desc d;
    memset(&d, 0, sizeof d);
    fill_robot(robot, ROBOT.c_str(), nj, d.robot);
    d.njoint = nj; d.use_axis = use_axis ? 1 : 0;
    auto opt = [&](const char *name) -> const mxArray * { const mxArray *f = opts ? mxGetField(opts, 0, name) : nullptr; return f && !mxIsEmpty(f) ? f : nullptr; };
    auto num = [&](const char *name, double dflt) { const mxArray *f = opt(name); return f ? mxGetScalar(f) : dflt; };
    // joint ranges: opts.lo / opts.hi, else robot.thetamax(1:njoint,:) (nlink x 2 column-major)
    std::vector<double> lo(nj), hi(nj);
    const mxArray *tm = mxGetField(robot, 0, "thetamax");
    for (int c = 0; c < nj; ++c) {
        if (opt("lo") && opt("hi")) { lo[c] = mxGetPr(opt("lo"))[c]; hi[c] = mxGetPr(opt("hi"))[c]; }
        else if (tm && (int)mxGetM(tm) >= nj) { lo[c] = mxGetPr(tm)[c]; hi[c] = mxGetPr(tm)[mxGetM(tm) + c]; }
        else mexErrMsgTxt("joint ranges: give opts.lo and opts.hi, or robot.thetamax");
    }
    d.lo = lo.data(); d.hi = hi.data();
    d.weight = opt("weight") ? mxGetPr(opt("weight")) : nullptr;
    // tool: opts.tool / opts.tool_axis, else the end effector of Lib/RRT_FANUC.m:186 and the axis of its capsule
    const double *cp = d.robot.cap + 6 * (nj - 1);
    double ax[3] = {cp[3] - cp[0], cp[4] - cp[1], cp[5] - cp[2]};
    if (ax[0] == 0.0 && ax[1] == 0.0 && ax[2] == 0.0) ax[2] = 1.0;
    for (int q = 0; q < 3; ++q) {
        d.tool[q] = opt("tool") ? mxGetPr(opt("tool"))[q] : cp[q];
        d.tool_axis[q] = opt("tool_axis") ? mxGetPr(opt("tool_axis"))[q] : ax[q];
    }
    d.restarts = (int)num("restarts", 64); d.max_iter = (int)num("max_iter", 100);
    d.tol_pos = num("tol_pos", 1e-6); d.tol_axis = num("tol_axis", 1e-6);
    d.seed = (unsigned long long)num("seed", 0);
    std::vector<double> obs6, D;
    const int ncell = (int)mxGetNumberOfElements(obs);
    for (int j = 0; j < ncell; ++j) {
        const mxArray *o = mxGetCell(obs, j), *fl = o ? mxGetField(o, 0, "l") : nullptr, *fD = o ? mxGetField(o, 0, "D") : nullptr;
        if (o && mxGetField(o, 0, "mesh")) mexErrMsgTxt("'ik' reads line obstacles only: mesh obstacles are not supported");
        if (!fl || !fD || mxGetNumberOfElements(fl) != 6) mexErrMsgIdAndTxt("cfs:obs", "obs{%d} needs .l (3x2) and .D", j + 1);
        obs6.insert(obs6.end(), mxGetPr(fl), mxGetPr(fl) + 6);
        D.push_back(mxGetScalar(fD));
    }
    d.nobs = (int)D.size(); d.obs = obs6.data(); d.D = D.data();
    mxArray *o_th = mxCreateDoubleMatrix(nj, T, mxREAL);                              // T x njoint row-major = njoint x T column-major
    mxArray *o_d[3] = {mxCreateDoubleMatrix(1, T, mxREAL), mxCreateDoubleMatrix(1, T, mxREAL), mxCreateDoubleMatrix(1, T, mxREAL)};
    std::vector<int> status(T), selected(T), n_ok(T);
    cfs_ik_out o;
    memset(&o, 0, sizeof o);
    o.theta = mxGetPr(o_th); o.status = status.data(); o.selected = selected.data(); o.n_ok = n_ok.data();
    o.err_pos = mxGetPr(o_d[0]); o.clearance = mxGetPr(o_d[1]); o.err_axis = mxGetPr(o_d[2]);
    check(cfs_ik_solve(&d, T, mxGetPr(prhs[4]), use_axis ? mxGetPr(prhs[5]) : nullptr, mxGetPr(prhs[6]), &o));
    mxArray *o_i[3] = {mxCreateDoubleMatrix(1, T, mxREAL), mxCreateDoubleMatrix(1, T, mxREAL), mxCreateDoubleMatrix(1, T, mxREAL)};
    for (int t = 0; t < T; ++t) { mxGetPr(o_i[0])[t] = status[t]; mxGetPr(o_i[1])[t] = selected[t] + 1; mxGetPr(o_i[2])[t] = n_ok[t]; }
    mxArray *outs[7] = {o_th, o_i[0], o_d[0], o_d[1], o_i[1], o_i[2], o_d[2]};
    for (int k = 0; k < 7; ++k) { if (k < nlhs || k == 0) plhs[k] = outs[k]; else mxDestroyArray(outs[k]); }
}

// 'ik' in a cell that ends with mesh obstacles (cfs_ik_solve_mesh): the same arguments and outputs, the obs cell as 'rrt' takes it
static void ik_mesh(int nlhs, mxArray *plhs[], int nrhs, const mxArray *prhs[])
{
    if (nrhs < 7) mexErrMsgTxt("[theta, status, err_pos, clearance, selected, n_ok, err_axis] = cfs_mex('ik_mesh', obs, robot, ROBOT, target_pos, target_axis, theta_ref [, opts])");
    const mxArray *obs = prhs[1], *robot = prhs[2], *opts = nrhs > 7 ? prhs[7] : nullptr;
    const std::string ROBOT = mxArrayToString(prhs[3]);
    const int nj = (int)mxGetM(prhs[6]), T = (int)mxGetN(prhs[4]);
    if (mxGetM(prhs[4]) != 3 || (int)mxGetN(prhs[6]) != T) mexErrMsgTxt("target_pos must be 3 x T and theta_ref njoint x T");
    const bool use_axis = !mxIsEmpty(prhs[5]);
    if (use_axis && (mxGetM(prhs[5]) != 3 || (int)mxGetN(prhs[5]) != T)) mexErrMsgTxt("target_axis must be 3 x T or []");
    cfs_ik_desc d;
    memset(&d, 0, sizeof d);
    fill_robot(robot, ROBOT.c_str(), nj, d.robot);
    d.njoint = nj; d.use_axis = use_axis ? 1 : 0;
    auto opt = [&](const char *name) -> const mxArray * { const mxArray *f = opts ? mxGetField(opts, 0, name) : nullptr; return f && !mxIsEmpty(f) ? f : nullptr; };
    auto num = [&](const char *name, double dflt) { const mxArray *f = opt(name); return f ? mxGetScalar(f) : dflt; };
    // joint ranges: opts.lo / opts.hi, else robot.thetamax(1:njoint,:) (nlink x 2 column-major)
    std::vector<double> lo(nj), hi(nj);
    const mxArray *tm = mxGetField(robot, 0, "thetamax");
    for (int c = 0; c < nj; ++c) {
        if (opt("lo") && opt("hi")) { lo[c] = mxGetPr(opt("lo"))[c]; hi[c] = mxGetPr(opt("hi"))[c]; }
        else if (tm && (int)mxGetM(tm) >= nj) { lo[c] = mxGetPr(tm)[c]; hi[c] = mxGetPr(tm)[mxGetM(tm) + c]; }
        else mexErrMsgTxt("joint ranges: give opts.lo and opts.hi, or robot.thetamax");
    }
    d.lo = lo.data(); d.hi = hi.data();
    d.weight = opt("weight") ? mxGetPr(opt("weight")) : nullptr;
    // tool: opts.tool / opts.tool_axis, else the end effector of Lib/RRT_FANUC.m:186 and the axis of its capsule
    const double *cp = d.robot.cap + 6 * (nj - 1);
    double ax[3] = {cp[3] - cp[0], cp[4] - cp[1], cp[5] - cp[2]};
    if (ax[0] == 0.0 && ax[1] == 0.0 && ax[2] == 0.0) ax[2] = 1.0;
    for (int q = 0; q < 3; ++q) {
        d.tool[q] = opt("tool") ? mxGetPr(opt("tool"))[q] : cp[q];
        d.tool_axis[q] = opt("tool_axis") ? mxGetPr(opt("tool_axis"))[q] : ax[q];
    }
    d.restarts = (int)num("restarts", 64); d.max_iter = (int)num("max_iter", 100);
    d.tol_pos = num("tol_pos", 1e-6); d.tol_axis = num("tol_axis", 1e-6);
    d.seed = (unsigned long long)num("seed", 0);
    // line obstacles (.l, .D) first, then mesh obstacles (.mesh = a handle of cfs_mex('mesh_load_stl' ...), .D), as in 'rrt'
    std::vector<double> obs6, D, D_mesh;
    std::vector<const cfs_mesh *> meshes;
    const int ncell = (int)mxGetNumberOfElements(obs);
    for (int j = 0; j < ncell; ++j) {
        const mxArray *o = mxGetCell(obs, j), *fl = o ? mxGetField(o, 0, "l") : nullptr, *fD = o ? mxGetField(o, 0, "D") : nullptr;
        const mxArray *mh = o ? mxGetField(o, 0, "mesh") : nullptr;
        if (mh) {
            if (!fD) mexErrMsgIdAndTxt("cfs:obs", "obs{%d} needs .mesh and .D", j + 1);
            if (mxGetField(o, 0, "pose")) mexErrMsgIdAndTxt("cfs:obs", "obs{%d}.pose: a moving mesh needs a time axis ('solve', 'get_con')", j + 1);
            meshes.push_back(mesh_of(mh));
            D_mesh.push_back(mxGetScalar(fD));
            continue;
        }
        if (!meshes.empty()) mexErrMsgTxt("mesh obstacles must come last in the obs cell");
        if (!fl || !fD || mxGetNumberOfElements(fl) != 6) mexErrMsgIdAndTxt("cfs:obs", "obs{%d} needs .l (3x2) and .D", j + 1);
        obs6.insert(obs6.end(), mxGetPr(fl), mxGetPr(fl) + 6);
        D.push_back(mxGetScalar(fD));
    }
    if (meshes.empty()) mexErrMsgTxt("'ik_mesh' needs at least one mesh obstacle at the end of the obs cell: use 'ik' for line obstacles only");
    d.nobs = (int)D.size(); d.obs = obs6.data(); d.D = D.data();
    mxArray *o_th = mxCreateDoubleMatrix(nj, T, mxREAL);                              // T x njoint row-major = njoint x T column-major
    mxArray *o_d[3] = {mxCreateDoubleMatrix(1, T, mxREAL), mxCreateDoubleMatrix(1, T, mxREAL), mxCreateDoubleMatrix(1, T, mxREAL)};
    std::vector<int> status(T), selected(T), n_ok(T);
    cfs_ik_out o;
    memset(&o, 0, sizeof o);
    o.theta = mxGetPr(o_th); o.status = status.data(); o.selected = selected.data(); o.n_ok = n_ok.data();
    o.err_pos = mxGetPr(o_d[0]); o.clearance = mxGetPr(o_d[1]); o.err_axis = mxGetPr(o_d[2]);
    check(cfs_ik_solve_mesh(&d, (int)meshes.size(), meshes.data(), D_mesh.data(), 0, T, mxGetPr(prhs[4]), use_axis ? mxGetPr(prhs[5]) : nullptr,
                            mxGetPr(prhs[6]), &o));
    mxArray *o_i[3] = {mxCreateDoubleMatrix(1, T, mxREAL), mxCreateDoubleMatrix(1, T, mxREAL), mxCreateDoubleMatrix(1, T, mxREAL)};
    for (int t = 0; t < T; ++t) { mxGetPr(o_i[0])[t] = status[t]; mxGetPr(o_i[1])[t] = selected[t] + 1; mxGetPr(o_i[2])[t] = n_ok[t]; }
    mxArray *outs[7] = {o_th, o_i[0], o_d[0], o_d[1], o_i[1], o_i[2], o_d[2]};
    for (int k = 0; k < 7; ++k) { if (k < nlhs || k == 0) plhs[k] = outs[k]; else mxDestroyArray(outs[k]); }
}

// Cost_b = EVAL(sys_info).get_Cost_b()  (Lib/EVAL.m:75-78)
// straight tool lines from IK candidates (cfs_cart_path): the approach move of a pick, which the reference's drivers do not have.
// follow: the verb 'cart_follow' (cfs_cart_follow), polylines of tool poses through the same arguments
static void cart_path(int nlhs, mxArray *plhs[], int nrhs, const mxArray *prhs[], bool follow = false)
{
    if (nrhs < 9) mexErrMsgTxt("[theta, status, path, clearance, selected, n_ok, n_done] = cfs_mex('cart_path', obs, robot, ROBOT, start, start_state, target_pos, target_axis, theta_ref [, opts])");
    const mxArray *obs = prhs[1], *robot = prhs[2], *opts = nrhs > 9 ? prhs[9] : nullptr;
    const std::string ROBOT = mxArrayToString(prhs[3]);
    // follow: target_pos / target_axis are the polylines path_pos / path_axis, 3 x M x T (mxGetN of it is M*T), and T is theta_ref's
    const int nj = (int)mxGetM(prhs[8]), T = (int)mxGetN(follow ? prhs[8] : prhs[6]);
    const int M = T > 0 ? (int)(mxGetN(prhs[6]) / T) : 0;
    if (mxGetM(prhs[6]) != 3 || (int)mxGetN(prhs[8]) != T || T < 1 || (int)mxGetN(prhs[6]) != M * T || (follow && M < 2))
        mexErrMsgTxt(follow ? "path_pos must be 3 x M x T with M >= 2 and theta_ref njoint x T" : "target_pos must be 3 x T and theta_ref njoint x T");
    const bool use_axis = !mxIsEmpty(prhs[7]);
    if (use_axis && (mxGetM(prhs[7]) != 3 || (int)mxGetN(prhs[7]) != M * T))
        mexErrMsgTxt(follow ? "path_axis must be 3 x M x T or []" : "target_axis must be 3 x T or []");
    const int R = (int)(mxGetN(prhs[4]) / T);                                         // mxGetN of njoint x R x T is R*T
    if ((int)mxGetM(prhs[4]) != nj || R < 1 || (int)mxGetN(prhs[4]) != R * T) mexErrMsgTxt("start must be njoint x R x T");
    std::vector<int> state;
    if (!mxIsEmpty(prhs[5])) {
        if ((int)mxGetNumberOfElements(prhs[5]) != R * T) mexErrMsgTxt("start_state must be R x T or []");
        state.resize((size_t)R * T);
        for (int e = 0; e < R * T; ++e) state[e] = (int)mxGetPr(prhs[5])[e];
    }
    cfs_cart_desc d;
    memset(&d, 0, sizeof d);
    fill_robot(robot, ROBOT.c_str(), nj, d.robot);
    d.njoint = nj; d.use_axis = use_axis ? 1 : 0;
    auto opt = [&](const char *name) -> const mxArray * { const mxArray *f = opts ? mxGetField(opts, 0, name) : nullptr; return f && !mxIsEmpty(f) ? f : nullptr; };
    auto num = [&](const char *name, double dflt) { const mxArray *f = opt(name); return f ? mxGetScalar(f) : dflt; };
    std::vector<double> lo(nj), hi(nj);
    const mxArray *tm = mxGetField(robot, 0, "thetamax");
    for (int c = 0; c < nj; ++c) {
        if (opt("lo") && opt("hi")) { lo[c] = mxGetPr(opt("lo"))[c]; hi[c] = mxGetPr(opt("hi"))[c]; }
        else if (tm && (int)mxGetM(tm) >= nj) { lo[c] = mxGetPr(tm)[c]; hi[c] = mxGetPr(tm)[mxGetM(tm) + c]; }
        else mexErrMsgTxt("joint ranges: give opts.lo and opts.hi, or robot.thetamax");
    }
    d.lo = lo.data(); d.hi = hi.data();
    d.weight = opt("weight") ? mxGetPr(opt("weight")) : nullptr;
    const double *cp = d.robot.cap + 6 * (nj - 1);
    double ax[3] = {cp[3] - cp[0], cp[4] - cp[1], cp[5] - cp[2]};
    if (ax[0] == 0.0 && ax[1] == 0.0 && ax[2] == 0.0) ax[2] = 1.0;
    for (int q = 0; q < 3; ++q) {
        d.tool[q] = opt("tool") ? mxGetPr(opt("tool"))[q] : cp[q];
        d.tool_axis[q] = opt("tool_axis") ? mxGetPr(opt("tool_axis"))[q] : ax[q];
    }
    d.candidates = R; d.steps = (int)num("steps", 16); d.max_iter = (int)num("max_iter", 20);
    d.max_joint_step = num("max_joint_step", 0.2);
    d.tol_pos = num("tol_pos", 1e-6); d.tol_axis = num("tol_axis", 1e-6);
    if (d.steps < 1 || d.steps > 256) mexErrMsgTxt("opts.steps must be in 1..256");
    if (follow && (M - 1) * d.steps > 256) mexErrMsgTxt("(M-1)*opts.steps must be at most 256: the rows of a path after row 0");
    const int rows = (follow ? (M - 1) * d.steps : d.steps) + 1;                       // of a path
    std::vector<double> obs6, D;
    const int ncell = (int)mxGetNumberOfElements(obs);
    for (int j = 0; j < ncell; ++j) {
        const mxArray *o = mxGetCell(obs, j), *fl = o ? mxGetField(o, 0, "l") : nullptr, *fD = o ? mxGetField(o, 0, "D") : nullptr;
        if (o && mxGetField(o, 0, "mesh"))
            mexErrMsgTxt(follow ? "'cart_follow' reads line obstacles only: use 'cart_follow_mesh' for a cell that ends with mesh obstacles"
                                : "'cart_path' reads line obstacles only: mesh obstacles are not supported");
        if (!fl || !fD || mxGetNumberOfElements(fl) != 6) mexErrMsgIdAndTxt("cfs:obs", "obs{%d} needs .l (3x2) and .D", j + 1);
        obs6.insert(obs6.end(), mxGetPr(fl), mxGetPr(fl) + 6);
        D.push_back(mxGetScalar(fD));
    }
    d.nobs = (int)D.size(); d.obs = obs6.data(); d.D = D.data();
    mxArray *o_th = mxCreateDoubleMatrix(nj, T, mxREAL);                              // T x njoint row-major = njoint x T column-major
    mxArray *o_path = mxCreateDoubleMatrix(nj, (size_t)rows * T, mxREAL);             // T x rows x njoint row-major
    mxArray *o_cl = mxCreateDoubleMatrix(1, T, mxREAL);
    std::vector<int> status(T), selected(T), n_ok(T), n_done(T);
    cfs_cart_out o;
    memset(&o, 0, sizeof o);
    o.theta = mxGetPr(o_th); o.status = status.data(); o.path = mxGetPr(o_path); o.selected = selected.data(); o.n_ok = n_ok.data();
    o.n_done = n_done.data(); o.clearance = mxGetPr(o_cl);
    if (follow)
        check(cfs_cart_follow(&d, T, M, mxGetPr(prhs[4]), state.empty() ? nullptr : state.data(), mxGetPr(prhs[6]),
                              use_axis ? mxGetPr(prhs[7]) : nullptr, mxGetPr(prhs[8]), &o));
    else
        check(cfs_cart_path(&d, T, mxGetPr(prhs[4]), state.empty() ? nullptr : state.data(), mxGetPr(prhs[6]), use_axis ? mxGetPr(prhs[7]) : nullptr,
                            mxGetPr(prhs[8]), &o));
    mxArray *o_i[4] = {mxCreateDoubleMatrix(1, T, mxREAL), mxCreateDoubleMatrix(1, T, mxREAL), mxCreateDoubleMatrix(1, T, mxREAL),
                       mxCreateDoubleMatrix(1, T, mxREAL)};
    for (int t = 0; t < T; ++t) {
        mxGetPr(o_i[0])[t] = status[t]; mxGetPr(o_i[1])[t] = selected[t] + 1; mxGetPr(o_i[2])[t] = n_ok[t]; mxGetPr(o_i[3])[t] = n_done[t];
    }
    mxArray *outs[7] = {o_th, o_i[0], o_path, o_cl, o_i[1], o_i[2], o_i[3]};
    for (int k = 0; k < 7; ++k) { if (k < nlhs || k == 0) plhs[k] = outs[k]; else mxDestroyArray(outs[k]); }
}

// 'cart_path' in a cell that ends with mesh obstacles (cfs_cart_path_mesh): the same arguments and outputs, the obs cell as 'rrt' takes it
// follow: the verb 'cart_follow_mesh' (cfs_cart_follow_mesh)
static void cart_path_mesh(int nlhs, mxArray *plhs[], int nrhs, const mxArray *prhs[], bool follow = false)
{
    if (nrhs < 9) mexErrMsgTxt("[theta, status, path, clearance, selected, n_ok, n_done] = cfs_mex('cart_path_mesh', obs, robot, ROBOT, start, start_state, target_pos, target_axis, theta_ref [, opts])");
    const mxArray *obs = prhs[1], *robot = prhs[2], *opts = nrhs > 9 ? prhs[9] : nullptr;
    const std::string ROBOT = mxArrayToString(prhs[3]);
    // follow: target_pos / target_axis are the polylines path_pos / path_axis, 3 x M x T (mxGetN of it is M*T), and T is theta_ref's
    const int nj = (int)mxGetM(prhs[8]), T = (int)mxGetN(follow ? prhs[8] : prhs[6]);
    const int M = T > 0 ? (int)(mxGetN(prhs[6]) / T) : 0;
    if (mxGetM(prhs[6]) != 3 || (int)mxGetN(prhs[8]) != T || T < 1 || (int)mxGetN(prhs[6]) != M * T || (follow && M < 2))
        mexErrMsgTxt(follow ? "path_pos must be 3 x M x T with M >= 2 and theta_ref njoint x T" : "target_pos must be 3 x T and theta_ref njoint x T");
    const bool use_axis = !mxIsEmpty(prhs[7]);
    if (use_axis && (mxGetM(prhs[7]) != 3 || (int)mxGetN(prhs[7]) != M * T))
        mexErrMsgTxt(follow ? "path_axis must be 3 x M x T or []" : "target_axis must be 3 x T or []");
    const int R = (int)(mxGetN(prhs[4]) / T);                                         // mxGetN of njoint x R x T is R*T
    if ((int)mxGetM(prhs[4]) != nj || R < 1 || (int)mxGetN(prhs[4]) != R * T) mexErrMsgTxt("start must be njoint x R x T");
    std::vector<int> state;
    if (!mxIsEmpty(prhs[5])) {
        if ((int)mxGetNumberOfElements(prhs[5]) != R * T) mexErrMsgTxt("start_state must be R x T or []");
        state.resize((size_t)R * T);
        for (int e = 0; e < R * T; ++e) state[e] = (int)mxGetPr(prhs[5])[e];
    }
    cfs_cart_desc d;
    memset(&d, 0, sizeof d);
    fill_robot(robot, ROBOT.c_str(), nj, d.robot);
    d.njoint = nj; d.use_axis = use_axis ? 1 : 0;
    auto opt = [&](const char *name) -> const mxArray * { const mxArray *f = opts ? mxGetField(opts, 0, name) : nullptr; return f && !mxIsEmpty(f) ? f : nullptr; };
    auto num = [&](const char *name, double dflt) { const mxArray *f = opt(name); return f ? mxGetScalar(f) : dflt; };
    std::vector<double> lo(nj), hi(nj);
    const mxArray *tm = mxGetField(robot, 0, "thetamax");
    for (int c = 0; c < nj; ++c) {
        if (opt("lo") && opt("hi")) { lo[c] = mxGetPr(opt("lo"))[c]; hi[c] = mxGetPr(opt("hi"))[c]; }
        else if (tm && (int)mxGetM(tm) >= nj) { lo[c] = mxGetPr(tm)[c]; hi[c] = mxGetPr(tm)[mxGetM(tm) + c]; }
        else mexErrMsgTxt("joint ranges: give opts.lo and opts.hi, or robot.thetamax");
    }
    d.lo = lo.data(); d.hi = hi.data();
    d.weight = opt("weight") ? mxGetPr(opt("weight")) : nullptr;
    const double *cp = d.robot.cap + 6 * (nj - 1);
    double ax[3] = {cp[3] - cp[0], cp[4] - cp[1], cp[5] - cp[2]};
    if (ax[0] == 0.0 && ax[1] == 0.0 && ax[2] == 0.0) ax[2] = 1.0;
    for (int q = 0; q < 3; ++q) {
        d.tool[q] = opt("tool") ? mxGetPr(opt("tool"))[q] : cp[q];
        d.tool_axis[q] = opt("tool_axis") ? mxGetPr(opt("tool_axis"))[q] : ax[q];
    }
    d.candidates = R; d.steps = (int)num("steps", 16); d.max_iter = (int)num("max_iter", 20);
    d.max_joint_step = num("max_joint_step", 0.2);
    d.tol_pos = num("tol_pos", 1e-6); d.tol_axis = num("tol_axis", 1e-6);
    if (d.steps < 1 || d.steps > 256) mexErrMsgTxt("opts.steps must be in 1..256");
    if (follow && (M - 1) * d.steps > 256) mexErrMsgTxt("(M-1)*opts.steps must be at most 256: the rows of a path after row 0");
    const int rows = (follow ? (M - 1) * d.steps : d.steps) + 1;                       // of a path
    // line obstacles (.l, .D) first, then mesh obstacles (.mesh = a handle of cfs_mex('mesh_load_stl' ...), .D), as in 'rrt'
    std::vector<double> obs6, D, D_mesh;
    std::vector<const cfs_mesh *> meshes;
    const int ncell = (int)mxGetNumberOfElements(obs);
    for (int j = 0; j < ncell; ++j) {
        const mxArray *o = mxGetCell(obs, j), *fl = o ? mxGetField(o, 0, "l") : nullptr, *fD = o ? mxGetField(o, 0, "D") : nullptr;
        const mxArray *mh = o ? mxGetField(o, 0, "mesh") : nullptr;
        if (mh) {
            if (!fD) mexErrMsgIdAndTxt("cfs:obs", "obs{%d} needs .mesh and .D", j + 1);
            if (mxGetField(o, 0, "pose")) mexErrMsgIdAndTxt("cfs:obs", "obs{%d}.pose: a moving mesh needs a time axis ('solve', 'get_con')", j + 1);
            meshes.push_back(mesh_of(mh));
            D_mesh.push_back(mxGetScalar(fD));
            continue;
        }
        if (!meshes.empty()) mexErrMsgTxt("mesh obstacles must come last in the obs cell");
        if (!fl || !fD || mxGetNumberOfElements(fl) != 6) mexErrMsgIdAndTxt("cfs:obs", "obs{%d} needs .l (3x2) and .D", j + 1);
        obs6.insert(obs6.end(), mxGetPr(fl), mxGetPr(fl) + 6);
        D.push_back(mxGetScalar(fD));
    }
    if (meshes.empty())
        mexErrMsgTxt(follow ? "'cart_follow_mesh' needs at least one mesh obstacle at the end of the obs cell: use 'cart_follow' for line obstacles only"
                            : "'cart_path_mesh' needs at least one mesh obstacle at the end of the obs cell: use 'cart_path' for line obstacles only");
    d.nobs = (int)D.size(); d.obs = obs6.data(); d.D = D.data();
    mxArray *o_th = mxCreateDoubleMatrix(nj, T, mxREAL);                              // T x njoint row-major = njoint x T column-major
    mxArray *o_path = mxCreateDoubleMatrix(nj, (size_t)rows * T, mxREAL);             // T x rows x njoint row-major
    mxArray *o_cl = mxCreateDoubleMatrix(1, T, mxREAL);
    std::vector<int> status(T), selected(T), n_ok(T), n_done(T);
    cfs_cart_out o;
    memset(&o, 0, sizeof o);
    o.theta = mxGetPr(o_th); o.status = status.data(); o.path = mxGetPr(o_path); o.selected = selected.data(); o.n_ok = n_ok.data();
    o.n_done = n_done.data(); o.clearance = mxGetPr(o_cl);
    if (follow)
        check(cfs_cart_follow_mesh(&d, (int)meshes.size(), meshes.data(), D_mesh.data(), 0, T, M, mxGetPr(prhs[4]),
                                   state.empty() ? nullptr : state.data(), mxGetPr(prhs[6]), use_axis ? mxGetPr(prhs[7]) : nullptr,
                                   mxGetPr(prhs[8]), &o));
    else
        check(cfs_cart_path_mesh(&d, (int)meshes.size(), meshes.data(), D_mesh.data(), 0, T, mxGetPr(prhs[4]), state.empty() ? nullptr : state.data(),
                                 mxGetPr(prhs[6]), use_axis ? mxGetPr(prhs[7]) : nullptr, mxGetPr(prhs[8]), &o));
    mxArray *o_i[4] = {mxCreateDoubleMatrix(1, T, mxREAL), mxCreateDoubleMatrix(1, T, mxREAL), mxCreateDoubleMatrix(1, T, mxREAL),
                       mxCreateDoubleMatrix(1, T, mxREAL)};
    for (int t = 0; t < T; ++t) {
        mxGetPr(o_i[0])[t] = status[t]; mxGetPr(o_i[1])[t] = selected[t] + 1; mxGetPr(o_i[2])[t] = n_ok[t]; mxGetPr(o_i[3])[t] = n_done[t];
    }
    mxArray *outs[7] = {o_th, o_i[0], o_path, o_cl, o_i[1], o_i[2], o_i[3]};
    for (int k = 0; k < 7; ++k) { if (k < nlhs || k == 0) plhs[k] = outs[k]; else mxDestroyArray(outs[k]); }
}

// a clock on joint paths (cfs_path_time): options through the same two lambdas as the other tool verbs
static void path_time(int nlhs, mxArray *plhs[], int nrhs, const mxArray *prhs[])
{
    if (nrhs < 8) mexErrMsgTxt("[time, sdot, duration, status, selected, group_status] = cfs_mex('path_time', robot, ROBOT, paths, dims, state, vmax, amax [, opts])");
    const mxArray *robot = prhs[1], *opts = nrhs > 8 ? prhs[8] : nullptr;
    const std::string ROBOT = mxArrayToString(prhs[2]);
    if (mxGetNumberOfElements(prhs[4]) != 3) mexErrMsgTxt("dims must be [N R G]");
    for (int q = 0; q < 3; ++q) {                                                     // whole numbers that an int holds, before any cast
        const double v = mxGetPr(prhs[4])[q];
        if (!(v >= 1.0 && v <= 1e6) || v != std::floor(v)) mexErrMsgTxt("dims must be three whole numbers [N R G], each in 1..1e6");
    }
    const int nj = (int)mxGetM(prhs[3]), N = (int)mxGetPr(prhs[4])[0], R = (int)mxGetPr(prhs[4])[1], G = (int)mxGetPr(prhs[4])[2];
    if (nj < 2 || nj > 6) mexErrMsgTxt("paths must have 2..6 rows (njoint)");
    if ((double)R * G > 2147483647.0 || mxGetNumberOfElements(prhs[3]) != (size_t)nj * N * R * G)
        mexErrMsgTxt("paths must be njoint x N x R x G with dims = [N R G]");
    if ((int)mxGetNumberOfElements(prhs[6]) != nj || (int)mxGetNumberOfElements(prhs[7]) != nj) mexErrMsgTxt("vmax and amax must be njoint x 1");
    std::vector<int> state;
    if (!mxIsEmpty(prhs[5])) {
        if ((int)mxGetNumberOfElements(prhs[5]) != R * G) mexErrMsgTxt("state must be R x G or []");
        state.resize((size_t)R * G);
        for (int e = 0; e < R * G; ++e) state[e] = (int)mxGetPr(prhs[5])[e];
    }
    cfs_time_desc d;
    memset(&d, 0, sizeof d);
    fill_robot(robot, ROBOT.c_str(), nj, d.robot);
    d.njoint = nj;
    auto opt = [&](const char *name) -> const mxArray * { const mxArray *f = opts ? mxGetField(opts, 0, name) : nullptr; return f && !mxIsEmpty(f) ? f : nullptr; };
    auto num = [&](const char *name, double dflt) { const mxArray *f = opt(name); return f ? mxGetScalar(f) : dflt; };
    const double *cp = d.robot.cap + 6 * (nj - 1);
    for (int q = 0; q < 3; ++q) d.tool[q] = opt("tool") ? mxGetPr(opt("tool"))[q] : cp[q];
    d.vmax = mxGetPr(prhs[6]); d.amax = mxGetPr(prhs[7]);
    d.feed = num("feed", HUGE_VAL); d.curve_share = num("curve_share", 0.5); d.stop_every = (int)num("stop_every", 0);
    const size_t np = (size_t)R * G;
    mxArray *o_t = mxCreateDoubleMatrix(N, np, mxREAL), *o_s = mxCreateDoubleMatrix(N, np, mxREAL);   // G x R x N row-major = N x (R*G) column-major
    mxArray *o_d = mxCreateDoubleMatrix(R, G, mxREAL);
    std::vector<int> status(np), selected(G), gstatus(G);
    cfs_time_out o;
    memset(&o, 0, sizeof o);
    o.time = mxGetPr(o_t); o.sdot = mxGetPr(o_s); o.duration = mxGetPr(o_d); o.status = status.data(); o.selected = selected.data();
    o.group_status = gstatus.data();
    check(cfs_path_time(&d, G, R, N, mxGetPr(prhs[3]), state.empty() ? nullptr : state.data(), &o));
    mxArray *o_st = mxCreateDoubleMatrix(R, G, mxREAL), *o_sel = mxCreateDoubleMatrix(1, G, mxREAL), *o_gs = mxCreateDoubleMatrix(1, G, mxREAL);
    for (size_t e = 0; e < np; ++e) mxGetPr(o_st)[e] = status[e];
    for (int g = 0; g < G; ++g) { mxGetPr(o_sel)[g] = selected[g] + 1; mxGetPr(o_gs)[g] = gstatus[g]; }
    mxArray *outs[6] = {o_t, o_s, o_d, o_st, o_sel, o_gs};
    for (int k = 0; k < 6; ++k) { if (k < nlhs || k == 0) plhs[k] = outs[k]; else mxDestroyArray(outs[k]); }
}

// what joint paths do between their rows (cfs_path_audit): dims and state as 'path_time' reads them, the obs cell as 'ik' reads it
static void path_audit(int nlhs, mxArray *plhs[], int nrhs, const mxArray *prhs[])
{
    if (nrhs < 7) mexErrMsgTxt("[clear_lower, chord_upper, state_out, status, clear_path, s_path, link_path, obs_path, clear_rows, chord_err] = cfs_mex('path_audit', obs, robot, ROBOT, paths, dims, state [, opts])");
    const mxArray *obs = prhs[1], *robot = prhs[2], *opts = nrhs > 7 ? prhs[7] : nullptr;
    const std::string ROBOT = mxArrayToString(prhs[3]);
    if (mxGetNumberOfElements(prhs[5]) != 3) mexErrMsgTxt("dims must be [N R G]");
    for (int q = 0; q < 3; ++q) {                                                     // whole numbers that an int holds, before any cast
        const double v = mxGetPr(prhs[5])[q];
        if (!(v >= 1.0 && v <= 1e6) || v != std::floor(v)) mexErrMsgTxt("dims must be three whole numbers [N R G], each in 1..1e6");
    }
    const int nj = (int)mxGetM(prhs[4]), N = (int)mxGetPr(prhs[5])[0], R = (int)mxGetPr(prhs[5])[1], G = (int)mxGetPr(prhs[5])[2];
    if (nj < 2 || nj > 6) mexErrMsgTxt("paths must have 2..6 rows (njoint)");
    if ((double)R * G > 2147483647.0 || mxGetNumberOfElements(prhs[4]) != (size_t)nj * N * R * G)
        mexErrMsgTxt("paths must be njoint x N x R x G with dims = [N R G]");
    std::vector<int> state;
    if (!mxIsEmpty(prhs[6])) {
        if ((int)mxGetNumberOfElements(prhs[6]) != R * G) mexErrMsgTxt("state must be R x G or []");
        state.resize((size_t)R * G);
        for (int e = 0; e < R * G; ++e) state[e] = (int)mxGetPr(prhs[6])[e];
    }
    cfs_audit_desc d;
    memset(&d, 0, sizeof d);
    fill_robot(robot, ROBOT.c_str(), nj, d.robot);
    d.njoint = nj;
    auto opt = [&](const char *name) -> const mxArray * { const mxArray *f = opts ? mxGetField(opts, 0, name) : nullptr; return f && !mxIsEmpty(f) ? f : nullptr; };
    auto num = [&](const char *name, double dflt) { const mxArray *f = opt(name); return f ? mxGetScalar(f) : dflt; };
    const double *cp = d.robot.cap + 6 * (nj - 1);
    for (int q = 0; q < 3; ++q) d.tool[q] = opt("tool") ? mxGetPr(opt("tool"))[q] : cp[q];
    d.substeps = (int)num("substeps", 8); d.min_clearance = num("min_clearance", -HUGE_VAL); d.max_chord = num("max_chord", HUGE_VAL);
    std::vector<double> obs6, D;
    const int ncell = (int)mxGetNumberOfElements(obs);
    for (int j = 0; j < ncell; ++j) {
        const mxArray *o = mxGetCell(obs, j), *fl = o ? mxGetField(o, 0, "l") : nullptr, *fD = o ? mxGetField(o, 0, "D") : nullptr;
        if (o && mxGetField(o, 0, "mesh")) mexErrMsgTxt("'path_audit' reads line obstacles only: meshes are not audited");
        if (!fl || !fD || mxGetNumberOfElements(fl) != 6) mexErrMsgIdAndTxt("cfs:obs", "obs{%d} needs .l (3x2) and .D", j + 1);
        obs6.insert(obs6.end(), mxGetPr(fl), mxGetPr(fl) + 6);
        D.push_back(mxGetScalar(fD));
    }
    d.nobs = (int)D.size(); d.obs = d.nobs ? obs6.data() : nullptr; d.D = d.nobs ? D.data() : nullptr;
    const size_t np = (size_t)R * G;
    mxArray *o_f[6];                                                                  // G x R row-major = R x G column-major
    for (int k = 0; k < 6; ++k) o_f[k] = mxCreateDoubleMatrix(R, G, mxREAL);
    std::vector<int> link(np), ob(np), status(np), sout(np);
    cfs_audit_out o;
    memset(&o, 0, sizeof o);
    o.clear_lower = mxGetPr(o_f[0]); o.chord_upper = mxGetPr(o_f[1]); o.clear_path = mxGetPr(o_f[2]); o.s_path = mxGetPr(o_f[3]);
    o.clear_rows = mxGetPr(o_f[4]); o.chord_err = mxGetPr(o_f[5]);
    o.link_path = link.data(); o.obs_path = ob.data(); o.status = status.data(); o.state_out = sout.data();
    check(cfs_path_audit(&d, G, R, N, mxGetPr(prhs[4]), state.empty() ? nullptr : state.data(), &o));
    mxArray *o_i[4];
    for (int k = 0; k < 4; ++k) o_i[k] = mxCreateDoubleMatrix(R, G, mxREAL);
    for (size_t e = 0; e < np; ++e) {
        mxGetPr(o_i[0])[e] = sout[e]; mxGetPr(o_i[1])[e] = status[e]; mxGetPr(o_i[2])[e] = link[e] > 0 ? link[e] : 0;
        mxGetPr(o_i[3])[e] = ob[e] + 1;                                              // both 1-based; 0 without obstacles or where not audited
    }
    mxArray *outs[10] = {o_f[0], o_f[1], o_i[0], o_i[1], o_f[2], o_f[3], o_i[2], o_i[3], o_f[4], o_f[5]};
    for (int k = 0; k < 10; ++k) { if (k < nlhs || k == 0) plhs[k] = outs[k]; else mxDestroyArray(outs[k]); }
}

static void cost_b(mxArray *plhs[], int nrhs, const mxArray *prhs[])
{
    if (nrhs < 3) mexErrMsgTxt("Cost_b = cfs_mex('cost_b', sys_info, ROBOT)");
    const mxArray *S = prhs[1];
    const std::string ROBOT = mxArrayToString(prhs[2]);
    Family f;
    cfs_problem_desc &d = f.d;
    memset(&d, 0, sizeof d);
    d.mode = CFS_MODE_CFS;
    d.H = (int)field_scalar(S, "H"); d.njoint = (int)field_scalar(S, "njoint"); d.nobs = 1;
    fill_robot(mxGetField(S, 0, "robot"), ROBOT.c_str(), d.njoint, d.robot);
    d.QQ = field_ptr(S, "QQ"); d.lim = field_ptr(S, "lim"); d.MAX_input = field_ptr(S, "MAX_input");
    d.epsilon_O = field_scalar(S, "epsilon_O"); d.MAX_O_ITER = (int)field_scalar(S, "MAX_O_ITER"); d.max_batch = 1;
    const double zero = 0.0;
    d.margin = &zero;
    check(cfs_problem_create(&d, &f.p));
    double caug = field_scalar(S, "caug"), cost = 0.0;
    check(cfs_cost_b(f.p, 1, field_ptr(S, "ff"), &caug, &cost, nullptr));
    plhs[0] = mxCreateDoubleScalar(cost);
}

void mexFunction(int nlhs, mxArray *plhs[], int nrhs, const mxArray *prhs[])
{
    if (nrhs < 1 || !mxIsChar(prhs[0])) mexErrMsgTxt("cfs_mex(command, ...)");
    const std::string cmd = mxArrayToString(prhs[0]);
    if (cmd == "solve") {
        solve(nlhs, plhs, nrhs, prhs);
    } else if (cmd == "get_con") {
        get_con(nlhs, plhs, nrhs, prhs);
    } else if (cmd == "clearance") {
        clearance(nlhs, plhs, nrhs, prhs);
    } else if (cmd == "clearance_mesh") {
        clearance_mesh(nlhs, plhs, nrhs, prhs);
    } else if (cmd == "clearance_mesh_motion") {
        clearance_mesh_motion(nlhs, plhs, nrhs, prhs);
    } else if (cmd == "chomp") {
        chomp(nlhs, plhs, nrhs, prhs);
    } else if (cmd == "dist_arm") {
        dist_arm(nlhs, plhs, nrhs, prhs);
    } else if (cmd == "rrt") {
        rrt(nlhs, plhs, nrhs, prhs);
    } else if (cmd == "ik") {
        ik(nlhs, plhs, nrhs, prhs);
    } else if (cmd == "ik_mesh") {
        ik_mesh(nlhs, plhs, nrhs, prhs);
    } else if (cmd == "cart_path") {
        cart_path(nlhs, plhs, nrhs, prhs);
    } else if (cmd == "cart_path_mesh") {
        cart_path_mesh(nlhs, plhs, nrhs, prhs);
    } else if (cmd == "cart_follow") {
        cart_path(nlhs, plhs, nrhs, prhs, true);
    } else if (cmd == "cart_follow_mesh") {
        cart_path_mesh(nlhs, plhs, nrhs, prhs, true);
    } else if (cmd == "path_time") {
        path_time(nlhs, plhs, nrhs, prhs);
    } else if (cmd == "path_audit") {
        path_audit(nlhs, plhs, nrhs, prhs);
    } else if (cmd == "cost_b") {
        cost_b(plhs, nrhs, prhs);
    } else if (cmd == "mesh_load_stl") {
        cfs_mesh *m = nullptr;
        check(cfs_mesh_load_stl(mxArrayToString(prhs[1]), nrhs > 2 ? mxGetScalar(prhs[2]) : 1.0, nrhs > 3 && mxGetScalar(prhs[3]) != 0, &m));
        plhs[0] = mxCreateNumericMatrix(1, 1, mxUINT64_CLASS, mxREAL);
        *static_cast<uint64_t *>(mxGetData(plhs[0])) = static_cast<uint64_t>(reinterpret_cast<uintptr_t>(m));
    } else if (cmd == "mesh_segment_distance") {
        const int n = (int)(mxGetNumberOfElements(prhs[2]) / 6);
        plhs[0] = mxCreateDoubleMatrix(n, 1, mxREAL);
        mxArray *pts = mxCreateDoubleMatrix(6, n, mxREAL);
        check(cfs_mesh_segment_distance(mesh_of(prhs[1]), n, mxGetPr(prhs[2]), mxGetPr(plhs[0]), mxGetPr(pts), nullptr));
        if (nlhs > 1) plhs[1] = pts; else mxDestroyArray(pts);
    } else if (cmd == "mesh_destroy") {
        cfs_mesh_destroy(mesh_of(prhs[1]));
    } else {
        mexErrMsgIdAndTxt("cfs:cmd", "unknown command %s", cmd.c_str());
    }
}
