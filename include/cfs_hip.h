/*
 * cfs_hip.h -- C ABI of libcfs_hip.so: the MI355X (gfx950) Convex-Feasible-Set inner loop.
 *
 * This is the drop-in boundary for the reference's hot path.  The reference
 * (JessicaLeu-code/MotionPlanning_5D_m) is MATLAB with no FFI of its own; the entry points
 * below are what a MEX gateway for that path binds (see INTEGRATION.md and matlab/cfs_mex.cpp).
 * Each entry point cites the reference interface it replaces (paths relative to the
 * reference root).
 *
 * Conventions
 *   - all floating point is IEEE fp64; all matrices are COLUMN-MAJOR exactly as MATLAB hands
 *     them (mxGetPr); a leading batch dimension B, where present, is the slowest one;
 *   - plain pointers and sizes only; the caller owns every buffer; the library owns only the
 *     opaque cfs_problem handle (device copies of the problem-family constants and workspace);
 *   - functions return CFS_SUCCESS (0) or a negative cfs_error; they never abort; the text of
 *     the last error of the calling thread is available from cfs_last_error();
 *   - entry points with the suffix _device take DEVICE pointers and a hipStream_t (passed as
 *     void*); they enqueue work and return without synchronising; the others take HOST
 *     pointers, copy in/out and synchronise;
 *   - there is no CPU fallback anywhere: without a HIP device every compute entry point
 *     returns CFS_ERR_NO_DEVICE.
 */
#ifndef CFS_HIP_H
#define CFS_HIP_H

#ifdef __cplusplus
extern "C" {
#endif

#define CFS_ABI_VERSION 1
#define CFS_MAX_LINKS 8   /* rows of robot.DH / entries of robot.cap the library accepts */
#define CFS_MAX_OBS 32    /* obstacles per problem                                       */
#define CFS_MAX_H 64      /* horizon (waypoints), one wavefront lane per waypoint         */

/* error codes (return values) */
typedef enum cfs_error {
    CFS_SUCCESS = 0,
    CFS_ERR_INVALID_ARG = -1,
    CFS_ERR_NO_DEVICE = -2,
    CFS_ERR_HIP = -3,          /* a HIP runtime call failed, see cfs_last_error()           */
    CFS_ERR_NOT_SPD = -4,      /* QQ (symmetrised) is not positive definite                  */
    CFS_ERR_DYNAMICS = -5,     /* sys_info.Aaug/Baug are not the double integrator of robot.A/B */
    CFS_ERR_ALLOC = -6
} cfs_error;

/* per-problem status written by the solvers; the reference has no error convention
 * (quadprog's exitflag is ignored, Lib/CFS_FANUC.m:85) -- an infeasible QP there crashes at
 * Lib/CFS_FANUC.m:92; here it is reported. */
typedef enum cfs_status {
    CFS_OK_CONVERGED = 0,  /* "Converged at stepN"  (Lib/EVAL.m:65-67) */
    CFS_OK_MAXITER = 1,    /* "MAX_ITER"            (Lib/EVAL.m:69-72) */
    CFS_QP_INFEASIBLE = 2, /* the linearised constraints of some outer iteration are infeasible */
    CFS_NUMERIC = 3,       /* the active-set solver gave up (iteration cap / breakdown)      */
    CFS_SOFT_ENDED = 4     /* CFS_INFEAS_SOFTEN handles only: the outer loop ended (stop test or MAX_O_ITER) on a softened
                              QP; x_ violates the linearised clearance by viol_all[last] (cfs_soft_results) */
} cfs_status;

/* which dist_arm_* the class constructor selects (Lib/CFS_FANUC.m:49-54) */
typedef enum cfs_robot_kind {
    CFS_ROBOT_M16IB = 0, /* Lib/M16iB/dist_arm_3D_Heu_2.m : DH chain (Lib/functions/CapPos.m)            */
    CFS_ROBOT_M200I = 1, /* Lib/200i/dist_arm_3D_200i_2.m : DH chain with theta(2) - pi/2 (:11)           */
    CFS_ROBOT_2L = 2     /* Lib/2L/dist_arm_2L.m + Lib/2L/CapPos2.m : planar Rz chain with robot.T        */
} cfs_robot_kind;

typedef enum cfs_mode {
    CFS_MODE_CFS = 0,    /* Lib/CFS_FANUC.m    : QP with QQ, ff, bounds +-MAX_input, margin obs{j}.epsilon */
    CFS_MODE_PSGCFS = 1  /* Lib/PSGCFS_FANUC.m : noisy gradient step + projection QP, margin obs{j}.D      */
} cfs_mode;

/* robot = the fields of robotproperty2(id) (Lib/functions/robotproperty2.m:1-153) the path reads */
typedef struct cfs_robot {
    int kind;                       /* cfs_robot_kind                                           */
    int nlink;                      /* size(robot.DH,1)                                          */
    double DH[CFS_MAX_LINKS * 4];   /* robot.DH, nlink x 4 COLUMN-MAJOR: DH[i + c*nlink]         */
    double base[3];                 /* robot.base                                                */
    double cap[CFS_MAX_LINKS * 6];  /* robot.cap{i+1}.p, 3x2 column-major each: cap[i*6 + k*3+r] */
    double T[9];                    /* 2L only: robot.T, 3x3 column-major                        */
    double delta_t;                 /* robot.delta_t                                             */
} cfs_robot;

/* problem family = everything in sys_info that does not change across the batch
 * (main_FANUC.m:106-127): consumed by cfs_problem_create. */
typedef struct cfs_problem_desc {
    cfs_robot robot;        /* sys_info.robot                                                  */
    int mode;               /* cfs_mode                                                        */
    int H;                  /* sys_info.H       (<= CFS_MAX_H)                                 */
    int njoint;             /* sys_info.njoint  (= sys_info.nu; nstate = 2*njoint)             */
    int nobs;               /* size(obs,2)      (<= CFS_MAX_OBS)                               */
    const double *QQ;       /* sys_info.QQ, nn x nn, nn = H*njoint                             */
    const double *Aaug;     /* sys_info.Aaug, (H*nstate) x nstate; may be NULL (then implied)  */
    const double *Baug;     /* sys_info.Baug, (H*nstate) x nn;     may be NULL (then implied)  */
    const double *lim;      /* sys_info.lim, njoint                                            */
    const double *MAX_input;/* sys_info.MAX_input, nn (CFS mode; ignored for PSGCFS)           */
    const double *margin;   /* nobs: obs{j}.epsilon (CFS, CFS_FANUC.m:117) / obs{j}.D (PSGCFS_FANUC.m:158) */
    double epsilon_O;       /* sys_info.epsilon_O                                              */
    int MAX_O_ITER;         /* sys_info.MAX_O_ITER                                             */
    double alpha;           /* sys_info.alpha (PSGCFS step, main_FANUC.m:120); CFS mode does not read it */
    int max_batch;          /* capacity B_max of the handle's device workspace                 */
} cfs_problem_desc;

typedef struct cfs_problem cfs_problem; /* opaque */

/* per-batch inputs: what differs between the B problems (start/goal/obstacles/seeds) */
typedef struct cfs_batch_in {
    int B;
    const double *x_init; /* B x (H*nstate): sys_info.x_  (stacked [theta;omega] of waypoints 1..H) */
    const double *xR1;    /* B x nstate    : sys_info.xR(:,1)                                       */
    const double *ff;     /* B x nn        : sys_info.ff                                            */
    const double *caug;   /* B             : sys_info.caug                                          */
    const double *obs;    /* B x nobs x 6  : [obs{j}.l(:,1); obs{j}.l(:,2)]  (B x H x nobs x 6 on a
                             CFS_OBS_PER_WAYPOINT handle: cfs_problem_set_obstacle_motion)          */
    const double *noise;  /* PSGCFS: B x noise_rows x nn draws of normrnd(0,0.1) (PSGCFS_FANUC.m:109),
                             one row consumed per PSG step; NULL = zeros                            */
    int noise_rows;
} cfs_batch_in;

/* per-batch outputs: what the callers read back (main_FANUC.m:144-162, RRTstar_CFS.m:197-203) */
typedef struct cfs_batch_out {
    double *u;           /* B x nn          : self.u                                   */
    double *x_;          /* B x (H*nstate)  : self.x_                                  */
    double *cost_all;    /* B x MAX_O_ITER  : self.eval.cost_all   (first iter_O-1 entries valid) */
    double *e_cost_all;  /* B x MAX_O_ITER  : self.eval.e_cost_all                     */
    double *e_u_all;     /* B x MAX_O_ITER  : self.eval.e_u_all                        */
    int *iter_O;         /* B : self.iter_O (reference convention: iterations run = iter_O-1) */
    int *total_iter;     /* B : self.total_iter (sum of active-set steps; stands in for quadprog's output.iterations) */
    int *status;         /* B : cfs_status                                             */
} cfs_batch_out;

/* ---- library ------------------------------------------------------------------------------ */
int cfs_abi_version(void);
const char *cfs_last_error(void);
int cfs_device_count(void);                 /* number of HIP devices (0 without a GPU)  */
int cfs_set_device(int device);             /* device used by subsequently created handles */

/* ---- problem family handle ------------------------------------------------------------------
 * replaces: the constructors CFS_FANUC(obs,sys_info,ROBOT) (Lib/CFS_FANUC.m:40-59) and
 * PSGCFS_FANUC(obs,sys_info,ROBOT) (Lib/PSGCFS_FANUC.m:43-62) plus the once-per-solve setup
 * quadprog does internally (factorising QQ).  Host pointers.  Validates Aaug/Baug against
 * the double integrator of robot.A/robot.B (robotproperty2.m:136-139) when they are given. */
int cfs_problem_create(const cfs_problem_desc *desc, cfs_problem **out);
void cfs_problem_destroy(cfs_problem *p);

/* The same from the WEIGHTS of the drivers' cost instead of the assembled matrices (row f2 of the scope table): the library
 * builds Aaug/Baug (double integrator of robot.A/robot.B), Q = [Qp q_cross*I; q_cross*I Qv], Qaug = blkdiag(w_stage*Q, ...,
 * w_terminal*Q), R = kron(I_H, Rblk), R = R + R', QQ = Baug'*Qaug*Baug + cR*R exactly as main_FANUC.m:64-97 (RRTstar_CFS.m:
 * 124-157, main_2L.m:69-93) do, the state-cost terms cfs_set_state_cost would otherwise be given (so cfs_build_terms_device
 * works at once), and, when desc->alpha == 0, alpha = 1/max(svd(QQ)) (main_FANUC.m:120).  desc->QQ / Aaug / Baug are ignored.
 * Neither QQ nor Qaug crosses the boundary; cfs_problem_family reads back what was built.  Because the structure of QQ is
 * known, QQ*u inside the solver (get_cost, Lib/EVAL.m:51-53; dcostArm_f, Lib/PSGCFS_FANUC.m:131-133) is evaluated through
 * Baug and the 2nj x 2nj blocks instead of the dense nn x nn matrix. */
typedef struct cfs_cost_weights {
    const double *Qp;   /* njoint x njoint column-major: Q(1:nj,1:nj)           (main_FANUC.m:66-70)   */
    const double *Qv;   /* njoint x njoint:              Q(nj+1:2nj,nj+1:2nj)   (main_FANUC.m:73-77)   */
    double q_cross;     /* Q(1:nj,nj+1:2nj) = Q(nj+1:2nj,1:nj) = q_cross*eye    (0.1, main_FANUC.m:71-72) */
    double w_stage;     /* Qaug block of waypoints 1..H-1 = Q*w_stage           (0.1, main_FANUC.m:81) */
    double w_terminal;  /* Qaug block of waypoint H      = Q*w_terminal         (10000, main_FANUC.m:83) */
    const double *Rblk; /* njoint x njoint column-major                         (main_FANUC.m:90-94)   */
    double cR;          /* QQ = Baug'*Qaug*Baug + R.*cR                         (50 | 10 | 0.1, :97)   */
} cfs_cost_weights;
int cfs_problem_create_from_weights(const cfs_problem_desc *desc, const cfs_cost_weights *w, cfs_problem **out);
/* what the handle was built with: QQ (nn x nn column-major, HOST pointer, may be NULL) and alpha (may be NULL) */
int cfs_problem_family(const cfs_problem *p, double *QQ, double *alpha);

/* ---- whole solve -----------------------------------------------------------------------------
 * replaces: self.optimizer() (Lib/CFS_FANUC.m:62-79, Lib/PSGCFS_FANUC.m:65-82) for B problems.
 * Host pointers; copies in, runs all outer iterations on the device, copies out, synchronises. */
int cfs_solve_batch(cfs_problem *p, const cfs_batch_in *in, const cfs_batch_out *out);

/* Same with DEVICE pointers on `stream` (hipStream_t as void*), no synchronisation.
 * in->B <= max_batch.  This is the entry bench.py times (inputs resident in HBM). */
int cfs_solve_batch_device(cfs_problem *p, const cfs_batch_in *in, const cfs_batch_out *out, void *stream);

/* Launch order of the fused solver: workgroup w solves problem order[w].  The added batch dimension has no counterpart in
 * the reference; a launch lasts as long as its longest problem plus the time that problem waited for a free compute unit.
 *   order = NULL, n = 0  automatic (default): problems whose initial trajectory violates the most (waypoint, obstacle)
 *                        clearances first, counted by a pre-pass on the solve's stream when B exceeds the device's compute units
 *   order = NULL, n < 0  identity (blockIdx order)
 *   order != NULL        HOST pointer, a permutation of 0..n-1, used by the next solves with B = n (a replanning loop may pass
 *                        the previous solve's total_iter, sorted); synchronises the device
 * Results do not depend on the order. */
int cfs_set_launch_order(cfs_problem *p, const int *order, int n);

/* ---- per-problem setup on the device (row f2 of the scope table) ---------------------------------------
 * replaces, for B (start, goal) pairs at once: the straight-line reference of main_FANUC.m:38-49
 * (x_ = joint-space line, zero velocities, waypoint 0 dropped), xR(:,1) = [x0; 0] and the cost terms
 * ff = ((Aaug*xR(:,1)-gaug)'*Qaug*Baug)' and caug = (Aaug*xR(:,1)-gaug)'*Qaug*(Aaug*xR(:,1)-gaug) with
 * gaug = kron(ones(H,1),[xg;0])  (main_FANUC.m:98-103).
 * cfs_set_state_cost: Qaug = the drivers' state-cost matrix (H*nstate x H*nstate, column-major, HOST pointer;
 * main_FANUC.m:79-84), given once per handle.  cfs_build_terms_device: x0, xg: B x njoint (DEVICE);
 * outputs (DEVICE): x_init B x H*nstate, xR1 B x nstate, ff B x nn, caug B; enqueued on `stream`. */
int cfs_set_state_cost(cfs_problem *p, const double *Qaug);
int cfs_build_terms_device(cfs_problem *p, int B, const double *x0, const double *xg,
                           double *x_init, double *xR1, double *ff, double *caug, void *stream);
/* The same from B RRT routes (RRTstar_CFS.m:94-110): routes is B x nwp x njoint (DEVICE; per problem the 5 x nwp route_wp as
 * MATLAB stores it); x_init = cubicpolytraj(route, (0:nwp-1)*delta_t, linspace(0,(nwp-1)*delta_t,H+1)) with zero waypoint
 * velocities (its default), waypoint 0 dropped, zero velocities; x0 / xg = the route's ends. */
int cfs_build_terms_from_routes_device(cfs_problem *p, int B, const double *routes, int nwp,
                                       double *x_init, double *xR1, double *ff, double *caug, void *stream);
/* The same for routes of DIFFERENT lengths, as cfs_rrt_grow_device leaves them: routes is B x nwp_stride x njoint, route b
 * has nwp[b] >= 2 rows (nwp: DEVICE int array; a route of a single row -- a start inside the goal region -- is treated as
 * start = goal).  RRTstar_CFS.m:96-100 resamples size(self.route,2) waypoints to horizon+1 samples whatever the length. */
int cfs_build_terms_from_ragged_routes_device(cfs_problem *p, int B, const double *routes, int nwp_stride, const int *nwp,
                                              double *x_init, double *xR1, double *ff, double *caug, void *stream);

/* ---- baseline cost ---------------------------------------------------------------------------
 * replaces: Cost_b = EVAL(sys_info).get_Cost_b() (Lib/EVAL.m:75-78, called at main_FANUC.m:131-132) for B problems of the
 * handle's family: u_b = quadprog(Qaug, paug) without constraints = -H^{-1} ff (H = QQ symmetrised, as quadprog does),
 * cost_b = get_cost(u_b) = 0.5*u_b'*QQ*u_b + ff'*u_b + caug (Lib/EVAL.m:51-53).  HOST pointers.  ff: B x nn; caug: B;
 * cost_b: B; u_b: B x nn (may be NULL).  Works for handles of either mode (the family's QQ is the same). */
int cfs_cost_b(cfs_problem *p, int B, const double *ff, const double *caug, double *cost_b, double *u_b);
/* replaces: cost = self.eval.get_cost(u) (Lib/EVAL.m:51-53) for B given u (B x nn): 0.5*u'*QQ*u + ff'*u + caug.  HOST pointers. */
int cfs_get_cost(cfs_problem *p, int B, const double *u, const double *ff, const double *caug, double *cost);

/* ---- measurement ------------------------------------------------------------------------------
 * When enabled, cfs_solve_batch_device brackets each kernel launch with hipEvents recorded on the
 * caller's stream (the reference has only tic/toc around the solver calls, main_FANUC.m:140-152).
 * cfs_profile_read synchronises on those events and returns, accumulated since the last read: the
 * milliseconds spent in the fused solve kernel (the event pair sits directly around its launch, after
 * the launch-order pre-pass; for handles with mesh obstacles it spans the loop of per-iteration
 * launches) and in the MFMA batched product, and the number of solves. */
int cfs_profile_enable(cfs_problem *p, int on);
int cfs_profile_read(cfs_problem *p, double *solve_kernel_ms, double *gemm_kernel_ms, int *solves);

/* ---- pieces of the path (host pointers; for callers that drive the outer loop themselves and
 *      for kernel-level parity tests) ------------------------------------------------------- */

/* [d,linkid] = dist_arm_all(theta,base,obs{j}.l,robot) (Lib/CFS_FANUC.m:115 ->
 * Lib/200i/dist_arm_3D_200i_2.m:1-30 | Lib/M16iB/dist_arm_3D_Heu_2.m | Lib/2L/dist_arm_2L.m)
 * for N configurations x nobs obstacles.  theta: N x njoint; obs: nobs x 6;
 * d: N x nobs; linkid: N x nobs (1-based); pos (optional): N x njoint x 6 capsule end points
 * [pos{i}.p(:,1); pos{i}.p(:,2)] (Lib/functions/CapPos.m:18-20). */
int cfs_dist_arm(const cfs_robot *robot, int njoint, int N, const double *theta, int nobs, const double *obs,
                 double *d, int *linkid, double *pos);

/* cfs_dist_arm with the analytic gradient (the CFS_JAC_ANALYTIC contract below) for the same N configurations x nobs
 * obstacles: extends [d,linkid] = dist_arm_all(theta,base,obs{j}.l,robot) (Lib/CFS_FANUC.m:115) by
 * grad = d/dtheta d, the exact derivative in place of Diff = num_jac(f,theta)' (Lib/CFS_FANUC.m:112-118,
 * Lib/functions/num_jac.m:1-17).  d and linkid are bit for bit cfs_dist_arm's; grad: N x nobs x njoint
 * (all of d, linkid, grad required).  The same device code as the solver's analytic linearisation. */
int cfs_dist_arm_grad(const cfs_robot *robot, int njoint, int N, const double *theta, int nobs, const double *obs,
                      double *d, int *linkid, double *grad);

/* the distance/Jacobian half of get_con (Lib/CFS_FANUC.m:110-121): for every (problem, obstacle,
 * waypoint) the distance, closest link and Diff = num_jac(f,theta)' (Lib/functions/num_jac.m:1-17,
 * literal scheme).  x_: B x (H*nstate); obs: B x nobs x 6 (B x H x nobs x 6 per waypoint);
 * dist: B x nobs x H; linkid: B x nobs x H; grad: B x nobs x H x njoint. */
int cfs_linearize(cfs_problem *p, int B, const double *x_, const double *obs, double *dist, int *linkid, double *grad);

/* self.get_con() with the reference's public dense outputs self.Ainq / self.binq
 * (Lib/CFS_FANUC.m:101-135): rows = nobs*H*(1+2*njoint) in the reference's row order.  On a handle with joint limits
 * (cfs_problem_set_joint_limits) rows = nobs*H*(1+2*njoint) + 2*H*njoint: the reference's rows, then +pos (i, c) for every
 * waypoint i and joint c (Bpos row (i, c) <= hi_c - theta0_c - (i+1)*delta_t*v0_c), then -pos (i, c) (-Bpos row (i, c) <=
 * theta0_c + (i+1)*delta_t*v0_c - lo_c), theta0 / v0 = xR1(1:njoint) / xR1(njoint+1:end); an infinite bound gives an infinite binq.
 * x_: B x (H*nstate); u: B x nn; xR1: B x nstate; obs: B x nobs x 6 (B x H x nobs x 6 per waypoint);
 * Ainq: B x (rows x nn column-major); binq: B x rows. */
int cfs_get_con(cfs_problem *p, int B, const double *x_, const double *u, const double *xR1, const double *obs,
                double *Ainq, double *binq);

/* one QP of the path for B problems on given linearisation data (dist/grad as returned by
 * cfs_linearize at u_lin): CFS mode  = quadprog(QQ,ff,Ainq,binq,[],[],-MAX_input,MAX_input)
 * (Lib/CFS_FANUC.m:85); PSGCFS mode = quadprog(I,-u_,Ainq,binq) (Lib/PSGCFS_FANUC.m:117-120) with
 * u_ passed in `lin`.  lin: B x nn (CFS: ff; PSGCFS: u_); u_lin: B x nn; xR1: B x nstate.
 * Outputs u: B x nn; lambda (optional): B x (nobs*H + 4*nn) multipliers ordered
 * [collision (j,i) | vel+ (i,c) | vel- (i,c) | bound+ | bound-] (with joint limits B x (nobs*H + 6*nn): then | pos+ (i,c) |
 * pos- (i,c)]); qp_iter, status: B. */
int cfs_qp(cfs_problem *p, int B, const double *lin, const double *u_lin, const double *xR1,
           const double *dist, const double *grad, double *u, double *lambda, int *qp_iter, int *status);

/* ---- Jacobian mode -------------------------------------------------------
 * How the solver linearises the line obstacles: Diff in get_con (Lib/CFS_FANUC.m:112-118).
 *   CFS_JAC_FD_LITERAL (default): num_jac (Lib/functions/num_jac.m:1-17) literally -- central differences with
 *     eps = 1e-5 and the perturbed xp never restored, evaluated at 2*njoint+1 poses; parity with the reference.
 *   CFS_JAC_ANALYTIC: for each (problem, obstacle, waypoint) the exact derivative with respect to theta of the branch of
 *     dist_arm_* active at the base pose: the first-minimum link, distLinSeg (Lib/functions/distLinSeg.m:23-91)
 *     differentiated through the branch taken (point / parallel / general, clamp then recompute: a clamped parameter
 *     contributes nothing) and through the near-zero surrogate dis = -|c - p1e| (dist_arm_3D_200i_2.m:22-24; 0 for a
 *     zero-length link).  Equal to the gradient of dist_arm wherever that is differentiable, the one-sided derivative
 *     of the winning branch at kinks.  The distances and closest links are unchanged (bit for bit the literal mode's
 *     base-pose values); the iterates differ from the literal mode's by the O(eps) of num_jac and what the outer loop
 *     makes of it.  Mesh obstacles keep their own linearisation (cfs_problem_set_meshes) in either mode; CHOMP
 *     (cfs_chomp_batch) is not affected.
 * The mode applies to every later solve and piece (cfs_linearize, cfs_get_con, cfs_qp) of the handle; a handle serves one
 * stream at a time, so set it between solves.  NULL handle or unknown mode: CFS_ERR_INVALID_ARG, nothing else happens. */
typedef enum cfs_jacobian_mode { CFS_JAC_FD_LITERAL = 0, CFS_JAC_ANALYTIC = 1 } cfs_jacobian_mode;
int cfs_problem_set_jacobian(cfs_problem *p, int mode);
int cfs_problem_get_jacobian(const cfs_problem *p, int *mode);

/* ---- infeasible-QP policy -----------------------------------------------------------------------
 * What an outer iteration does when its linearised QP is proven infeasible.  The reference ignores quadprog's exitflag and
 * carries on from whatever iterate interior-point-convex returns (Lib/CFS_FANUC.m:85-92, Lib/PSGCFS_FANUC.m:116-127).
 *   CFS_INFEAS_STOP (default): status CFS_QP_INFEASIBLE, the solve of that problem ends (bit for bit the behaviour without
 *     a policy).
 *   CFS_INFEAS_SOFTEN: the same outer iteration solves the soft-constraint QP in its place,
 *       min 1/2 u'Gu + g'u + (weight/2) sum_r s_r^2   s.t.  a_r'u - s_r <= b_r (collision rows), velocity and input rows hard,
 *     with G, g the hard QP's own terms (QQ, ff for CFS; I, -u_ for the PSGCFS projection), and continues from its u exactly
 *     as from a hard one (rollout, get_cost without the penalty, store_result, stop test).  Only a QP that is proven
 *     infeasible is softened; a feasible one is solved as with STOP, bit for bit.  The soft QP is strictly convex, its slacks
 *     are s_r = lambda_r / weight >= 0.  Should it be infeasible too (the velocity and input rows alone are; never with
 *     v0 = 0), the status is CFS_QP_INFEASIBLE.  A problem whose outer loop ends on a softened QP reports CFS_SOFT_ENDED;
 *     one whose last QP was hard reports CFS_OK_CONVERGED / CFS_OK_MAXITER as usual.
 *     weight: cost units per m^2 of slack, finite and > 0.  Between 1e4 and 1e6 recommended: the max slack is then within
 *     1e-3 m of the least violation possible; above ~1e8 the soft QP's dual becomes nearly singular (its complementarity
 *     residual grows with the weight) and the outer loop may stall at MAX_O_ITER.
 * cfs_qp on a SOFTEN handle runs the same two stages: status 0 for a hard solution, CFS_SOFT_ENDED for a soft one, 2 when
 * even the soft QP is infeasible; lambda holds the multipliers of the QP that produced u (slacks: lambda / weight).
 * The policy applies to later solves and pieces of the handle (set it between solves).  NULL handle, unknown policy or a weight
 * that is not finite and > 0 (with either policy; STOP does not use it): CFS_ERR_INVALID_ARG, nothing changes.  Mesh obstacles are not supported in soft mode: SOFTEN on
 * a handle with meshes, or cfs_problem_set_meshes (nmesh > 0) on a SOFTEN handle, gives CFS_ERR_INVALID_ARG.  CHOMP is not
 * affected. */
typedef enum cfs_infeasible_policy { CFS_INFEAS_STOP = 0, CFS_INFEAS_SOFTEN = 1 } cfs_infeasible_policy;
int cfs_problem_set_infeasible_policy(cfs_problem *p, int policy, double weight);
/* policy and weight as last set (CFS_INFEAS_STOP and 0 on a handle where the policy was never set) */
int cfs_problem_get_infeasible_policy(const cfs_problem *p, int *policy, double *weight);
/* Results of the handle's last whole solve (cfs_solve_batch or cfs_solve_batch_device; synchronises the device), host pointers:
 * viol_all: B x MAX_O_ITER, the largest slack max_r s_r of each outer iteration's QP (0 for a hard QP and after the last
 * iteration); n_soft: B, the number of softened outer iterations.  All zero after a solve with STOP.  Either may be NULL. */
int cfs_soft_results(cfs_problem *p, int B, double *viol_all, int *n_soft);

/* ---- moving obstacles ----------------------------------------------------------------------------
 * Obstacles given per waypoint: a predicted path of a person's forearm, a part on a conveyor, another arm.  Collision row (j, i)
 * of get_con (Lib/CFS_FANUC.m:110-120, Lib/PSGCFS_FANUC.m:152-160) depends only on waypoint i's pose and on obstacle j, so only
 * the obstacle that the linearisation reads for waypoint i changes; the QP, the infeasibility certificate, the warm start, the
 * soft QP, the rollout, the costs and the stop tests are those of a static handle.
 *   CFS_OBS_STATIC (default): every obs array the handle reads is B x nobs x 6, one axis per obstacle for the whole horizon.
 *   CFS_OBS_PER_WAYPOINT: every obs array that cfs_solve_batch, cfs_solve_batch_device, cfs_linearize and cfs_get_con read is
 *     B x H x nobs x 6; row [b][i][j] is obstacle j's [l(:,1); l(:,2)] at waypoint i+1, i.e. row i of x_, at time (i+1)*delta_t.
 *     Margins stay per obstacle.  With the same row at every waypoint, every result is bit for bit the static handle's.  The
 *     automatic launch order measures waypoint i against row i.
 * CFS_ERR_INVALID_ARG, nothing changes: NULL handle; unknown motion; PER_WAYPOINT on a handle with meshes (nmesh > 0: meshes move by
 * cfs_problem_set_mesh_motion, next to static lines); PER_WAYPOINT for a shape whose per-waypoint linearisation tiles (nobs*6 more doubles of LDS per waypoint) do not fit
 * every tier of the fused solver that the static shape fits (checked here, not at launch).  On a PER_WAYPOINT handle
 * cfs_problem_set_meshes with nmesh > 0 and cfs_chomp_batch give CFS_ERR_INVALID_ARG.  Not affected: cfs_qp (it reads no
 * obstacles), cfs_dist_arm*, RRT, cfs_select_best_device, the cfs_build_terms* entry points.  Set it between solves. */
typedef enum cfs_obstacle_motion { CFS_OBS_STATIC = 0, CFS_OBS_PER_WAYPOINT = 1 } cfs_obstacle_motion;
int cfs_problem_set_obstacle_motion(cfs_problem *p, int motion);
int cfs_problem_get_obstacle_motion(const cfs_problem *p, int *motion);

/* ---- joint position limits ---------------------------------------------------------------------------
 * The reference bounds velocities (Lib/CFS_FANUC.m:126-129, Lib/PSGCFS_FANUC.m:175-178) and, in CFS mode, inputs, never positions,
 * although robotproperty2.m defines robot.thetamax.  With limits set, every QP of the handle (whole solves, cfs_qp, cfs_get_con) has
 * two more hard rows per waypoint i and joint c:  lo_c <= theta0_c + (i+1)*delta_t*v0_c + (Bpos u)[i,c] <= hi_c,  i.e. row i of x_
 * as the solver computes it (no DH offset is applied: the bounds are on x_ itself).  The rows are hard in the soft QP of
 * CFS_INFEAS_SOFTEN too (they never get a slack and never enter viol_all).  A QP whose limits cannot be met (a start outside them by
 * more than the velocity rows let one step cover) ends the problem with CFS_QP_INFEASIBLE under either policy.  lo / hi: njoint
 * values each; either side may be infinite (a row that can never become active).  lo == hi == NULL clears the limits (the default:
 * every result is then the unlimited handle's).  With rows that never bind, every result is bit for bit the unlimited handle's.
 * CFS_ERR_INVALID_ARG, nothing changes: NULL handle; one of lo / hi NULL; a NaN; lo[c] >= hi[c]; a shape whose LDS plan with the
 * position rows does not fit every tier of the fused solver that the plan without them fits (checked here, not at launch).  On a
 * handle with limits cfs_chomp_batch gives CFS_ERR_INVALID_ARG (CHOMP_FANUC has no QP).  Mesh handles (cfs_problem_set_meshes) run
 * the same QP and get the rows too.  Set them between solves.
 * get: *on = 1 with limits, 0 without; lo / hi (njoint each, either may be NULL) receive them, -inf / +inf without limits. */
int cfs_problem_set_joint_limits(cfs_problem *p, const double *lo, const double *hi);
int cfs_problem_get_joint_limits(const cfs_problem *p, int *on, double *lo, double *hi);

/* ---- mesh obstacles -----------------------------------------------------
 * The reference measures the arm against a surface with `[dis, points] = point2surface_dis(pos{i}.p, obs)`
 * (M200i/dist_arm_surf_200i.m:21, Lib/functions/dist_arm_surface.m:43) and loads its maps with stlread
 * (Lib/functions/MapFromSTL.m:1-11), but contains neither function.  The contract here is the build's own:
 * dis = min over the triangles of the Euclidean distance between the link axis and the triangle (0 when they
 * intersect); points = [closest point on the link axis ; closest point on the mesh]; equal distances resolve
 * to the smaller parameter along the axis.  A cfs_mesh owns the device copy of the triangles and of a bounding
 * volume hierarchy; it lives on the device selected with cfs_set_device at creation. */
typedef struct cfs_mesh cfs_mesh; /* opaque */

/* vertices: nv x 3 (x, y, z per row); triangles: nt x 3 vertex indices (0-based); HOST pointers */
int cfs_mesh_create(const double *vertices, int nv, const int *triangles, int nt, cfs_mesh **out);
/* binary STL file.  map_from_stl != 0 applies Lib/functions/MapFromSTL.m:6-10 (every axis shifted to start at 0,
 * y -= 100, then (x, y, z) <- (z, x, y)); every coordinate is finally multiplied by `scale` (the maps are in mm). */
int cfs_mesh_load_stl(const char *path, double scale, int map_from_stl, cfs_mesh **out);
/* any output may be NULL; bbox6 = [min xyz, max xyz] */
int cfs_mesh_info(const cfs_mesh *m, int *ntri, int *nnodes, int *depth, double *bbox6);
void cfs_mesh_destroy(cfs_mesh *m);

/* point2surface_dis for n segments (HOST pointers): segs n x 6 = [p(:,1); p(:,2)]; dis n;
 * points n x 6 (may be NULL); tri n = index of the closest triangle in the caller's list (may be NULL).
 * The geometry is evaluated WITHOUT FMA contraction (as cfs_rrt_grow_mesh evaluates it; cfs_dist_arm_mesh, the solvers, the
 * clearance audits, cfs_ik_solve_mesh and cfs_cart_path_mesh contract): it rounds like the CPU statement of the contract, so
 * that distances equal in exact arithmetic (a segment in the surface, parallel to a wall or to an edge) resolve to the same
 * point there and here.  A distance may differ in its last bits from cfs_dist_arm_mesh's for the same link axis. */
int cfs_mesh_segment_distance(const cfs_mesh *m, int n, const double *segs, double *dis, double *points, int *tri);

/* dist_arm_surf_200i (M200i/dist_arm_surf_200i.m:1-29) for N poses (HOST pointers): theta N x njoint;
 * d N; linkid N (1-based, may be NULL); points N x 6 of the closest link (may be NULL).  Same near-zero
 * surrogate (:22-24) and first-minimum rule (:25-28) as cfs_dist_arm. */
int cfs_dist_arm_mesh(const cfs_robot *robot, int njoint, int N, const double *theta, const cfs_mesh *m,
                      double *d, int *linkid, double *points);

/* From now on the LAST nmesh of the handle's nobs obstacles are these meshes (their entries of cfs_batch_in.obs are
 * ignored; margin[] still applies per obstacle): every later solve measures the arm against them with the contract
 * above, rows ordered as get_con orders obstacles (Lib/CFS_FANUC.m:111).  nmesh = 0 restores line obstacles only.
 * The meshes must outlive the solves. */
int cfs_problem_set_meshes(cfs_problem *p, int nmesh, const cfs_mesh *const *meshes);

/* ---- moving meshes ------------------------------------------------------------------------------------
 * A rigid pose per waypoint for every mesh of the handle: a carrier on a conveyor, a part on a belt.  Collision row (j, i) of
 * get_con depends on waypoint i's pose and on obstacle j only (see "moving obstacles"), so mesh row (j, i) of cfs_solve_batch,
 * cfs_solve_batch_device, cfs_linearize and cfs_get_con becomes the mesh contract's distance between waypoint i's link axes and
 * mesh j placed by pose [j][i]; the near-zero surrogate and the first minimum over the links are unchanged, and the Jacobian stays
 * the literal num_jac, taken on that same distance.  The QP, the certificate, the rollout, the costs and the stop tests are those
 * of a static handle.
 * poses: HOST, nmesh x H x 12.  Entry [j][i] is the row-major 3x4 matrix [R | t] that places mesh j (vertices as given to
 * cfs_mesh_create / cfs_mesh_load_stl) in the world at waypoint i+1 (row i of x_, time (i+1)*delta_t):
 * x_world = R x_mesh + t.  NULL: the meshes are static again.
 * Evaluation: no hierarchy is rebuilt.  The distance from a link axis to a mesh placed by [R | t] equals the distance from the
 * inverse-transformed axis to the mesh as stored; the library inverts each pose on the host in double (R', -R't), keeps
 * nmesh x H x 12 on the device, and the linearisation kernels measure transformed end points against the stored mesh.  With
 * identity poses the transform is exact (x*1 + y*0 + z*0 + 0), so every result is bit for bit the static handle's.
 * The poses belong to the handle and are shared by every problem of a batch, as the meshes are; every call of
 * cfs_problem_set_meshes resets the handle to static.  Line obstacles of such a handle are static (meshes stay refused on a
 * CFS_OBS_PER_WAYPOINT handle), and meshes stay refused with CFS_INFEAS_SOFTEN and in cfs_chomp_batch.  cfs_clearance_mesh and
 * cfs_clearance_mesh_device give CFS_ERR_INVALID_ARG on a handle with mesh motion: their certified bound assumes v_obs = 0 in the
 * mesh columns; cfs_clearance_mesh_motion audits such a handle, with pose interpolation and a surface-speed term in its bound.
 * CFS_ERR_INVALID_ARG, nothing changes: NULL handle; a handle without meshes (nmesh == 0); a pose that is not finite; a pose with
 * max|RR' - I| > 1e-9 or det R <= 0 (scaling or mirroring would break the isometry every bound of the traversal relies on).
 * Synchronises the device; set it between solves. */
int cfs_problem_set_mesh_motion(cfs_problem *p, const double *poses);

/* ---- CHOMP_FANUC ----------------------------------------------------------
 * self = CHOMP_FANUC(obs_, sys_info, uref, ROBOT); self = self.optimizer()  (Lib/CHOMP_FANUC.m:34-69) for B problems of
 * the handle's family (robot, H, QQ, alpha, epsilon_O, MAX_O_ITER; create it in CFS mode).  HOST pointers.
 * in: x_init, xR1, ff, caug, obs as for cfs_solve_batch (noise unused); u0: B x nn = uref; D, epsilon: nobs =
 * obs_{j+1}.D / .epsilon.  out: u, x_, cost_all / e_cost_all / e_u_all (B x MAX_O_ITER), iter_O; total_iter (0) and
 * status may be NULL.  The update is the reference's, literally (step 3*alpha, gradient rows Baug((i-1)*njoint+1:
 * i*njoint,:), dm_f without the M200i joint offset, derivest derivatives): see csrc/cfs_chomp.hip for the list. */
int cfs_chomp_batch(cfs_problem *p, const cfs_batch_in *in, const double *u0, const double *D, const double *epsilon,
                    const cfs_batch_out *out);

/* ---- RRT / RRT* tree growth ---------------------------------------------------------
 * replaces: RRT_FANUC(obs, sys_info, goal, region_g, region_s, sample_off, ROBOT, SOLVER).find_route() (Lib/RRT_FANUC.m:48-91)
 * for S independent trees at once -- the seeds Lib/functions/s_Parallel_rrt.m:14-28 spreads over a parfor pool.  One wavefront
 * grows one tree entirely on the device (nearest neighbour under the `ratial`-weighted norm, 0.1-rad extension, capsule
 * feasibility against every obstacle with the same FK + distLinSeg + near-zero surrogate as the CFS path, RRT* re-parenting
 * within `rewire` of the sample, goal test, failure at node_num > MAX_ITER, route back-tracking); the reference's quirks are
 * kept (csrc/cfs_rrt.hip lists them).  MATLAB's rand stream cannot be reproduced: pass the uniforms (S x ndraw, consumed as
 * the reference consumes rand: one per proposal, nstate more when the sample is random) or NULL + a seed for the library's
 * counter-based generator (u = splitmix64 finaliser of seed + tree*0x9E3779B97F4A7C15 + (counter+1)*0xBF58476D1CE4E5B9,
 * top 53 bits * 2^-53). */
typedef enum cfs_rrt_solver { CFS_RRT = 0, CFS_RRT_STAR = 1 } cfs_rrt_solver;   /* SOLVER 'RRT' | 'RRT*' (Lib/RRT_FANUC.m:70-84) */
typedef struct cfs_rrt_desc {
    cfs_robot robot;          /* sys_info.robot (+ ROBOT: robot.kind decides the theta(2) - pi/2 offset, :158-160)   */
    int nstate;               /* sys_info.nstate = joints of the tree (2..6)                                         */
    int solver;               /* cfs_rrt_solver                                                                      */
    int max_iter;             /* MAX_ITER (400, :37); <= 1000                                                        */
    double bi;                /* goal bias threshold (0.5, :38): pp < bi -> random sample, else goal_th              */
    double rewire;            /* RRT* re-parenting radius around the sample (0.2, :135)                              */
    int per_tree;             /* 0: x0 / goal / goal_th are nstate vectors shared by all trees; 1: S x nstate         */
    const double *x0;         /* sys_info.x0                                                                         */
    const double *goal;       /* goal (centre of the goal region, :195-197)                                          */
    const double *goal_th;    /* sys_info.goal_th (the biased sample, :113)                                          */
    const double *region_g, *region_s, *sample_off, *ratial;   /* nstate each (:108-111, :117, :195-197)             */
    int nobs;
    const double *obs;        /* nobs x 6: [obs{j}.l(:,1); obs{j}.l(:,2)]                                            */
    const double *D;          /* nobs: obs{j}.D (:174)                                                               */
    const double *uniforms;   /* S x ndraw draws of rand, or NULL                                                    */
    int ndraw;
    unsigned long long seed;  /* generator mode (uniforms == NULL)                                                   */
    long long max_draws;      /* generator mode: uniforms a tree may consume before it gives up (fail = 2)           */
} cfs_rrt_desc;
typedef struct cfs_rrt_out {
    int *node_num;            /* S : self.node_num                                                                    */
    int *fail;                /* S : 0 route found | 1 node_num > MAX_ITER ("Failed to find path.", :201-205) | 2 the uniforms
                                     ran out while sampling | 3 RRT* re-parenting closed a cycle (the reference would never return) */
    int *parent;              /* S x (max_iter+1) : self.all_nodes(1,:) (1-based, -1 for the root)                    */
    double *nodes;            /* S x (max_iter+1) x nstate : self.all_nodes(2:end,:)' (one node per row)              */
    double *total_dis;        /* S x (max_iter+1) : self.total_dis                                                    */
    double *all_ee;           /* S x max_iter x 3 : self.all_ee' (may be NULL)                                        */
    int *route_len;           /* S : size(self.route,2)                                                               */
    double *route;            /* S x (max_iter+1) x nstate : self.route' (first route_len rows), start to goal       */
    long long *draws_used;    /* S : uniforms consumed (may be NULL)                                                  */
    long long *proposals;     /* S : getRandNode calls (may be NULL)                                                  */
} cfs_rrt_out;
/* HOST pointers in the descriptor and in `out`; copies in, grows, copies out, synchronises */
int cfs_rrt_grow(const cfs_rrt_desc *d, int S, const cfs_rrt_out *out);
/* DEVICE pointers (every array of the descriptor and of `out`; the descriptor struct itself is host memory), enqueued on
 * `stream`; routes can go straight into cfs_build_terms_from_ragged_routes_device */
int cfs_rrt_grow_device(const cfs_rrt_desc *d, int S, const cfs_rrt_out *out, void *stream);

/* The same trees in a cell that also holds mesh obstacles.  feasible() (Lib/RRT_FANUC.m:146-181) is extended
 * the way M200i/dist_arm_surf_200i.m:21-24 extends dist_arm: the line obstacles of the descriptor are tested first, as above; then,
 * for every mesh j and link i, dis = the mesh distance of the link axis under the mesh contract ("mesh obstacles" above), if
 * |dis| < 1e-4 then dis = -|points(:,1) - p(:,2)|, and the node is rejected if dis < D_mesh[j].  Equivalently: mesh j rejects the
 * node exactly when some triangle lies closer than max(D_mesh[j], 1e-4) to some link axis; the hierarchy is walked as a threshold
 * query that may stop at the first such triangle, and the decision does not depend on the traversal order.  Everything else (draws
 * per proposal, nearest node, extension, addNode, arrangeNode, goal test, failure codes, route, all_ee) is cfs_rrt_grow's;
 * nmesh = 0 gives exactly what cfs_rrt_grow* gives.  The geometry is evaluated without FMA contraction, like the tree arithmetic,
 * so a proposal within rounding of its threshold may be decided differently from a cfs_dist_arm_mesh call.
 * meshes: nmesh handles created on the current device (cfs_set_device); they must outlive the launch.  D_mesh: HOST, nmesh
 * margins, finite and > 0.  d->nobs + nmesh <= CFS_MAX_OBS.  CFS_ERR_INVALID_ARG, with nothing launched, for any violation of
 * these, for unknown flags, for a MAX_ITER whose tree no longer fits into 64 KB of LDS next to the mesh scratch, and for every
 * argument cfs_rrt_grow refuses.
 * flags: 0, or a developer switch like the CFS_DBG_CLEAR_* ones below (RRT has no handle to carry them; results are bit-identical
 * under every value): */
#define CFS_RRT_MESH_PER_LANE 1        /* variant A: one (mesh, link) pair per lane, private threshold query (the correctness baseline)     */
#define CFS_RRT_MESH_WAVE 2            /* variant B: one wave-cooperative traversal over a shared frontier in LDS (the default: 2.7-3.7x A) */
#define CFS_RRT_MESH_SMALL_FRONTIER 4  /* variant B with a frontier of 8 entries: its overflow path (decided by variant A) under test        */
int cfs_rrt_grow_mesh(const cfs_rrt_desc *d, int nmesh, const cfs_mesh *const *meshes, const double *D_mesh, int flags, int S,
                      const cfs_rrt_out *out);
int cfs_rrt_grow_mesh_device(const cfs_rrt_desc *d, int nmesh, const cfs_mesh *const *meshes, const double *D_mesh /* HOST, nmesh */,
                             int flags, int S, const cfs_rrt_out *out, void *stream);

/* ---- best of K smoothed routes per slot ---------------------------------------------------------
 * The reference grows num_seed RRT seeds, keeps the route with the FEWEST NODES, first seed on ties
 * (Lib/functions/s_Parallel_rrt.m:27-28: [~, I] = min(routeL)), and runs one CFS on it (RRTstar_CFS.m:94-196).  Here all K
 * routes of a slot are smoothed in one solve over S*K problems, stored slot-major (candidate s*K + k), and this entry keeps
 * per slot the best SMOOTHED result instead: route length predicts neither the final cost nor whether the linearised QPs
 * stay feasible, so ranking after the solve keeps every slot that any of its seeds can solve (the reference's pick is one
 * of the K candidates, so the kept cost is never above it when that pick solves).  With n = iter_O - 1 (outer iterations
 * run), the final cost is cost_all[n-1] (eval.cost_new) and the final violation viol_all[n-1]:
 *   1. only candidates with route_ok[s*K+k] != 0 are eligible;
 *   2. class A = status 0 or 1: the lowest final cost wins;
 *   3. if class A is empty, class B = status 4 (CFS_SOFT_ENDED): the lowest final violation wins, then the lowest final cost;
 *   4. if both are empty but some route was found: the found-route candidate with the lowest k, its status (2 or 3) as it
 *      is, has_solution = 0;
 *   5. if no route was found: selected = -1, has_solution = 0, and the slot's rows of `best` / best_viol_all are untouched;
 *   6. ties go to the lowest k; a NaN final cost or violation, or n outside 1..MAX_O_ITER, makes a candidate ineligible
 *      for class A / B (it can still be the candidate of rule 4).
 * has_solution = 1 exactly when the winner comes from class A or B.  When cand_viol_all is NULL (allowed on STOP handles
 * only) a status-4 candidate's violation counts as 0.
 * The winner's rows are gathered into slot-major outputs: u, x_, cost_all, e_cost_all, e_u_all, viol_all (when
 * best_viol_all is given), iter_O, total_iter, status.  One wavefront per slot, no atomics: the result is deterministic and
 * depends on the slot's own K candidates only, not on S or on launch order.
 * DEVICE pointers, enqueued on `stream`:  route_ok S*K;  cand: S*K rows (cfs_batch_out of the solve, all 8 arrays);
 * cand_viol_all: S*K x MAX_O_ITER (viol_all of cfs_soft_results; required on a CFS_INFEAS_SOFTEN handle, may be NULL on a
 * STOP one);  best: S rows (all 8 arrays), must not overlap cand;  best_viol_all: S x MAX_O_ITER or NULL (needs cand_viol_all);
 * selected, has_solution: S.  CFS_ERR_INVALID_ARG for K outside 1..64, S < 1, a NULL handle, a NULL required array, or
 * S*K > max_batch of the handle. */
int cfs_select_best_device(cfs_problem *p, int S, int K, const int *route_ok, const cfs_batch_out *cand,
                           const double *cand_viol_all, const cfs_batch_out *best, double *best_viol_all, int *selected,
                           int *has_solution, void *stream);

/* ---- clearance audit between the waypoints ---------------------------------------------------------
 * Every collision row of get_con is written at a waypoint (Lib/CFS_FANUC.m:110-120, Lib/PSGCFS_FANUC.m:152-160); between two
 * waypoints the arm follows the double integrator of robotproperty2.m:136-139, and nothing in the reference -- nor any status
 * of the solvers -- says how close that motion comes to an obstacle.  This entry measures it for B trajectories of the handle's
 * family, S = substeps samples per interval (1..64):
 *   interval i = 0..H-1 starts at state i-1 (xR1 for i = 0, row i-1 of x_ otherwise), has acceleration u[i] and lasts delta_t;
 *   sample k = 0..S is the pose theta = theta_s + tau*v_s + tau^2/2*u_i at tau = k*delta_t/S, except that sample k = S is row i
 *   of x_ itself (the waypoint values are cfs_dist_arm's on x_).  x_ must be the rollout of (xR1, u), as every solver returns it.
 *   At every sample: dist_arm (the FK, distLinSeg, near-zero surrogate and first-minimum link of cfs_dist_arm) against every
 *   line obstacle.  obs: B x nobs x 6; on a CFS_OBS_PER_WAYPOINT handle B x H x nobs x 6, and inside interval i >= 1 the two end
 *   points of an obstacle are interpolated linearly between row i-1 (tau = 0) and row i (tau = delta_t); in interval 0 the
 *   obstacle is held at row 0 (the handle has no row for t = 0).
 * Outputs per (problem, obstacle), B x nobs each, all required:
 *   dist_wp     min over the H waypoints;
 *   dist_path   min over all H*(S+1) samples (<= dist_wp);
 *   t_path, link_path   where the first such minimum occurs (lowest interval, then lowest k): seconds from the start,
 *               (i + k/S)*delta_t, and the closest link (1-based);
 *   dist_lower  min over all sub-intervals [k, k+1] of (d_k + d_{k+1})/2 - L*delta_t/(2*S), where L bounds |d/dtau distance| on
 *               the sub-interval: L = max over links k of sum_{m<=k} w_m*rho[m][k] + v_obs, w_m the larger |v_m| at the two ends
 *               (the velocity is linear in tau), rho[m][k] = sum_{j=m..k} len_j + c_k with len_j = hypot(a_j, d_j) of DH row j
 *               (2L: the length of link j's translation) and c_k the larger norm of capsule k's end points in its link frame,
 *               v_obs the larger end-point displacement of the obstacle over the interval divided by delta_t (0 when static or
 *               held).  GUARANTEE: if dist_lower[b][j] > 0, obstacle j stays at least that far from every capsule axis of
 *               problem b for all t in [0, H*delta_t] (a positive bound also rules out the near-zero surrogate, the only
 *               discontinuity of dist_arm).  dist_path - dist_lower <= max L * delta_t/(2*S): the bound tightens as 1/S.
 * Deterministic (no atomics); a problem's results depend on neither B nor its position in the batch.  Independent of mode,
 * Jacobian mode, infeasible-QP policy and joint limits; reads no state of the handle that a solve writes and changes none.
 * CFS_ERR_INVALID_ARG, nothing written: NULL handle or array, B outside 1..max_batch, substeps outside 1..64, a handle with mesh
 * obstacles (cfs_problem_set_meshes with nmesh > 0: meshes are not audited).
 * cfs_clearance_device: DEVICE pointers, enqueued on `stream`, no synchronisation.  cfs_clearance: HOST pointers, synchronises. */
int cfs_clearance_device(cfs_problem *p, int B, int substeps, const double *x_, const double *u, const double *xR1, const double *obs,
                         double *dist_wp, double *dist_path, double *dist_lower, double *t_path, int *link_path, void *stream);
int cfs_clearance(cfs_problem *p, int B, int substeps, const double *x_, const double *u, const double *xR1, const double *obs,
                  double *dist_wp, double *dist_path, double *dist_lower, double *t_path, int *link_path);

/* ---- clearance audit with mesh obstacles -----------------------------------------------------------------
 * The audit above for a handle whose last nmesh >= 1 obstacles are meshes (cfs_problem_set_meshes) and do not move (a handle with
 * cfs_problem_set_mesh_motion is refused; its line obstacles are static in any case).  Time
 * line, samples, first-minimum rule, t_path and link_path are the contract above word for word; all outputs are B x nobs in the
 * handle's obstacle order (line obstacles first, the last nmesh columns are the meshes).  obs: B x nobs x 6, the rows of the mesh
 * obstacles are not read (as in every solve of such a handle).
 *   line columns   bit for bit what cfs_clearance returns on a line-only handle of the same robot, H, delta_t and rows;
 *   mesh columns   the distance at a sample is cfs_dist_arm_mesh's: the same FK, the mesh contract above (exact minimum over the
 *                  triangles, ties to the smaller axis parameter), the near-zero surrogate of dist_arm_surf_200i.m:22-24, first
 *                  minimum over the links;
 *   dist_lower     the same formula with v_obs = 0 in the mesh columns.  The GUARANTEE carries over unchanged: the distance from
 *                  a segment to a fixed closed set (a union of triangles) is 1-Lipschitz in the segment's end points, and that is
 *                  the only property of the obstacle the bound uses; a faceted surface changes which triangle is closest between
 *                  two samples, not how fast the distance can change;
 *   tri_path       B x nobs: the index, in the caller's triangle list (cfs_mesh_create / the STL's order), of a closest triangle
 *                  of link link_path at the dist_path sample; -1 in line columns.  Where several triangles are equally close (a
 *                  shared edge or vertex) any one of them may be reported; the distances do not depend on which.
 * dist_wp, dist_path and dist_lower do not depend on the order in which a hierarchy is traversed.  Deterministic (no atomics); a
 * problem's results depend on neither B nor its position in the batch.  Reads the handle's constants and meshes only, changes
 * nothing, independent of mode, Jacobian mode, infeasible-QP policy and joint limits.  The first audit of a handle, and the first
 * with more substeps than any before, allocates the per-sample workspace (max_batch x nmesh x (H*substeps + 1) records) and
 * synchronises the device once; later audits enqueue only.
 * CFS_ERR_INVALID_ARG, nothing written: NULL handle or array, B outside 1..max_batch, substeps outside 1..64, a handle without
 * meshes (use cfs_clearance).  cfs_clearance and cfs_clearance_device keep refusing handles with meshes.
 * cfs_clearance_mesh_device: DEVICE pointers, enqueued on `stream`, no synchronisation.  cfs_clearance_mesh: HOST pointers,
 * synchronises. */
int cfs_clearance_mesh_device(cfs_problem *p, int B, int substeps, const double *x_, const double *u, const double *xR1,
                              const double *obs, double *dist_wp, double *dist_path, double *dist_lower, double *t_path,
                              int *link_path, int *tri_path, void *stream);
int cfs_clearance_mesh(cfs_problem *p, int B, int substeps, const double *x_, const double *u, const double *xR1, const double *obs,
                       double *dist_wp, double *dist_path, double *dist_lower, double *t_path, int *link_path, int *tri_path);

/* ---- clearance audit with moving meshes -------------------------------------------------------------------
 * The audit above for a handle whose meshes move (cfs_problem_set_mesh_motion).  Arguments, outputs, column order, time line,
 * samples, first-minimum rule, t_path, link_path and tri_path are those of cfs_clearance_mesh word for word; what is new is where
 * a mesh stands at a sample between two waypoints, and the term its motion adds to the bound.
 *   static handle   meshes and no motion: the static path runs, every result is bit for bit cfs_clearance_mesh's.
 *   moving handle   pose [j][i] belongs to waypoint i+1 (row i of x_).  Interval 0 has no earlier pose: pose [j][0] is held over
 *                   it (as the line audit holds row 0 there).  In interval i >= 1 the sample at k = S uses the stored inverse pose
 *                   [j][i] exactly as the linearisation reads it, so dist_wp is measured where get_con measures it.  If poses
 *                   i-1 and i are bitwise equal, the stored pose [j][i] is used over the whole interval and the mesh speed is 0:
 *                   constant or identity poses give bit for bit the static audit.
 *   interpolation   otherwise, at s = k/S mesh j is placed by p -> R(s)(p - c_j) + c_w(s).  c_j = (min + max)/2 of the bounding
 *                   box of mesh j's stored vertices.  R(s) = Rod(a, s*theta) R_{i-1}, the rotation about the unit axis a by the
 *                   angle s*theta applied after pose i-1's, with a and theta from R_rel = R_i R_{i-1}': w = vee(R_rel - R_rel')/2,
 *                   theta = atan2(|w|, (tr R_rel - 1)/2), a = w/|w| (a pure translation has theta = 0 and R(s) = R_{i-1}).
 *                   c_w(s) is the straight line from R_{i-1} c_j + t_{i-1} to R_i c_j + t_i.  No hierarchy is rebuilt: the link
 *                   ends go into the stored frame by the inverse, w -> c_j + R(s)'(w - c_w(s)); the near-zero surrogate and the
 *                   closest point live in the mesh's frame (an isometry keeps every distance).
 *   dist_lower      the formula of cfs_clearance with L = L_arm + v_mesh[j][i] on the sub-intervals of interval i,
 *                   v_mesh[j][i] = (theta*r_j + |c_w(1) - c_w(0)|)/delta_t, r_j = max over the stored vertices of |v - c_j|;
 *                   0 in interval 0 and in held intervals.  No surface point moves faster than that under the interpolation
 *                   above; the distance is a minimum over pairs of points, each Lipschitz with the sum of the two speeds, so the
 *                   GUARANTEE of cfs_clearance holds for the interpolated motion.
 *   line columns    the lines of such a handle are static: bit for bit cfs_clearance's.
 * The inverse transforms of the H*substeps + 1 distinct samples of every mesh do not depend on the problem: a small kernel writes
 * them once into a table on the handle, rebuilt only when substeps or the poses change.  Deterministic (no atomics); a problem's
 * results depend on neither B nor its position in the batch.
 * CFS_ERR_INVALID_ARG, nothing written: everything cfs_clearance_mesh refuses other than the motion itself (NULL handle or array,
 * B outside 1..max_batch, substeps outside 1..64, a handle without meshes); a mesh whose poses at two consecutive waypoints
 * differ by more than a quarter turn (tr R_rel < 1, theta > pi/2: towards pi the axis taken from the skew part loses accuracy and
 * theta*r_j certifies nothing; the message names the mesh and the waypoint).  cfs_clearance_mesh and cfs_clearance_mesh_device
 * keep refusing a handle with mesh motion.
 * cfs_clearance_mesh_motion_device: DEVICE pointers, enqueued on `stream`, no synchronisation once the workspace and the table
 * exist.  cfs_clearance_mesh_motion: HOST pointers, synchronises. */
int cfs_clearance_mesh_motion_device(cfs_problem *p, int B, int substeps, const double *x_, const double *u, const double *xR1,
                                     const double *obs, double *dist_wp, double *dist_path, double *dist_lower, double *t_path,
                                     int *link_path, int *tri_path, void *stream);
int cfs_clearance_mesh_motion(cfs_problem *p, int B, int substeps, const double *x_, const double *u, const double *xR1,
                              const double *obs, double *dist_wp, double *dist_path, double *dist_lower, double *t_path,
                              int *link_path, int *tri_path);

/* ---- inverse kinematics -------------------------------------------------------------------------------
 * Every entry point above that takes a goal takes a joint vector, as the reference's drivers type it in (xg, main_FANUC.m:30,
 * RRTstar_CFS.m:43).  This entry finds, for T Cartesian targets at once, the configuration inside the joint limits that reaches the
 * target, passes RRT's feasible() against the line obstacles, and is nearest to a reference configuration.  No handle.
 *   pose(theta)  FK of the chain cfs_dist_arm runs for robot.kind (theta(2) - pi/2 for M200i), then
 *                pos = M_njoint * tool + base (as link_ends adds it) and dir = R_njoint * tool_axis; tool_axis is normalised on entry.
 *                tool = robot.cap{njoint}.p(:,1) gives the reference's end effector all_ee (Lib/RRT_FANUC.m:186).
 *   residual     r = [pos - target_pos] (3 rows, use_axis = 0) or [pos - target_pos; dir - target_axis] (6 rows, use_axis = 1;
 *                every target_axis row is normalised on entry); F = r'r; e_pos / e_axis = the 2-norms of the two halves (e_axis = 0
 *                when use_axis = 0).
 *   Jacobian     analytic: column c = [w_c x (pos - q_c); w_c x dir] with (w_c, q_c) the axis of joint c and a point on it.
 * One wavefront per target, one lane per restart k = 0..restarts-1.  Restart 0 starts at theta_ref clamped into [lo, hi]; restart
 * k >= 1 at theta_c = lo_c + u*(hi_c - lo_c), u = the RRT generator above with tree = k and counter = c (the joint), so every target
 * of a call, wherever it stands in the batch, tries the same starts.  Then, with lambda = 1e-2 and it = 0, the restart repeats:
 *   1. F not finite (NaN or inf): state 3, end;
 *   2. e_pos <= tol_pos and (use_axis = 0 or e_axis <= tol_axis): converged, end;
 *   3. it == max_iter: state 1, end;
 *   4. delta = -(J'J + lambda*I)^-1 J'r by Cholesky (a pivot that is not finite and > 0: state 3, end);
 *   5. s = max_c |delta_c|; if s > 0.5 (rad): delta = delta*(0.5/s);
 *   6. trial_c = theta_c + delta_c, set to lo_c if below it and to hi_c if above it;
 *   7. if F(trial) < F (false for a NaN): theta = trial, lambda = max(lambda/10, 1e-9); else lambda = min(10*lambda, 1e9);
 *   8. it = it + 1.
 * A converged restart is inside the limits by construction.  Its clearance is min_j (d_j - D_j), d_j = min over the links of
 * seg_seg_dist (distLinSeg with the near-zero surrogate: cfs_dist_arm's d), +inf when nobs = 0; it collides exactly when feasible()
 * (Lib/RRT_FANUC.m:146-181) rejects it: some link's distance to obstacle j is < D_j, i.e. clearance < 0.
 * States of a restart (cand_status): 0 converged and free | 1 max_iter reached | 2 converged but in collision | 3 numeric.
 * Per target: among the restarts in state 0 the one with the smallest sum_c weight_c*((theta_c - theta_ref_c)^2) wins (plain IEEE
 * products and sums in joint order, so a host can restate the cost to the last bit), ties to the lowest restart (a wave reduction
 * on (cost, lane), no atomics).  status: 0 solved | 1 no restart converged | 2 every converged restart
 * collides.  selected = the winning restart or -1; n_ok = restarts in state 0; theta, err_pos, err_axis, clearance = the winner's
 * (rows of targets with status != 0 hold NaN, selected = -1).  cand_theta (T x restarts x njoint: where each restart ended),
 * cand_status, cand_iter (T x restarts: `it` when it ended).  A target's results depend on neither T nor its position in the batch.
 * CFS_ERR_INVALID_ARG, nothing written: a NULL descriptor, out, out->theta or out->status; a robot / njoint cfs_dist_arm refuses or
 * njoint < 2; use_axis not 0 / 1; restarts outside 1..64; max_iter outside 1..1000; nobs outside 0..CFS_MAX_OBS; tolerances, tool,
 * lo, hi, weight that are not finite, lo >= hi, weight <= 0, tol <= 0; a tool_axis that is not finite or (use_axis = 1) zero;
 * T < 1; NULL target_pos or theta_ref; use_axis = 1 with a NULL target_axis; nobs > 0 with NULL obs or D; and, in cfs_ik_solve,
 * whose arrays the host can read: a non-finite target_pos, target_axis, theta_ref, obs or D, a zero target_axis row.
 * cfs_ik_solve: HOST pointers throughout, synchronises.  cfs_ik_solve_device: lo, hi, weight stay HOST pointers (njoint values, read
 * at the call); obs, D, target_pos, target_axis, theta_ref and every array of `out` are DEVICE pointers; enqueued on `stream`, no
 * synchronisation.  A non-finite value in a device array ends the restarts that read it in state 3. */
typedef struct cfs_ik_desc {
    cfs_robot robot;
    int njoint;                 /* 2..6: the chain of cfs_dist_arm for robot.kind                                        */
    double tool[3];             /* a point in the frame of link njoint                                                   */
    double tool_axis[3];        /* a direction in the same frame (normalised on entry)                                   */
    int use_axis;               /* 0: position only (3 rows) | 1: position + direction (6 rows)                          */
    const double *lo, *hi;      /* njoint each, finite, lo < hi                                                          */
    const double *weight;       /* njoint, > 0, or NULL = ones: the norm of "nearest to theta_ref"                       */
    int restarts;               /* 1..64, one lane each                                                                  */
    int max_iter;               /* 1..1000                                                                               */
    double tol_pos, tol_axis;   /* metres / norm of the direction difference; finite, > 0                                */
    int nobs;                   /* 0..CFS_MAX_OBS line obstacles                                                         */
    const double *obs;          /* nobs x 6: [obs{j}.l(:,1); obs{j}.l(:,2)]                                              */
    const double *D;            /* nobs: obs{j}.D (Lib/RRT_FANUC.m:174)                                                  */
    unsigned long long seed;
} cfs_ik_desc;
typedef struct cfs_ik_out {
    double *theta;              /* T x njoint                                                                            */
    int *status;                /* T                                                                                     */
    int *selected, *n_ok;       /* T (may be NULL)                                                                       */
    double *err_pos, *err_axis, *clearance;   /* T (may be NULL)                                                         */
    double *cand_theta;         /* T x restarts x njoint (may be NULL)                                                   */
    int *cand_status, *cand_iter;             /* T x restarts (may be NULL)                                              */
} cfs_ik_out;
/* target_pos: T x 3; target_axis: T x 3 (read when use_axis = 1; may be NULL otherwise); theta_ref: T x njoint */
int cfs_ik_solve(const cfs_ik_desc *d, int T, const double *target_pos, const double *target_axis, const double *theta_ref,
                 const cfs_ik_out *out);
int cfs_ik_solve_device(const cfs_ik_desc *d, int T, const double *target_pos, const double *target_axis, const double *theta_ref,
                        const cfs_ik_out *out, void *stream);
/* The same inverse kinematics in a cell that also holds mesh obstacles.  The contract is "inverse kinematics"
 * above word for word, with these changes.  After the line test, a restart that converged and passed the lines is tested against the
 * meshes with exactly the decision of cfs_rrt_grow_mesh: it takes state 2 when some triangle of some mesh j lies strictly closer
 * than thr_j = max(D_mesh[j], 1e-4) to some link axis, and stays in state 0 otherwise (an existence test: the traversal order does
 * not matter).  State 2 therefore means "converged but in collision with a line obstacle or a mesh", and status 2 "every converged
 * restart collides with a line obstacle or a mesh".  Every converged restart is tested, so n_ok and cand_status keep their meaning.
 * clearance = min(line clearance, min_j (dm_j - D_mesh[j])), dm_j = the exact mesh distance (the mesh contract above) of the nearest
 * link axis of the winner; the winner is free, so dm_j >= thr_j and the near-zero surrogate cannot apply.  cand_theta and cand_iter
 * do not depend on the meshes: starts, steps 1-8, the line test, the cost and the selection are cfs_ik_solve's.  A target's results
 * depend on neither T nor its position in the batch; there are no atomics on the normal path.
 * The geometry is evaluated WITH FMA contraction, as cfs_dist_arm_mesh evaluates it and cfs_rrt_grow_mesh does not: a pose within
 * rounding of a threshold may be decided differently here than by cfs_rrt_grow_mesh; the clearance agrees with cfs_dist_arm_mesh.
 * meshes: nmesh >= 1 handles created on the current device (cfs_set_device); they must outlive the launch.  D_mesh: HOST in both
 * entries, nmesh margins, finite and > 0.  CFS_ERR_INVALID_ARG, with nothing written, for everything cfs_ik_solve (cfs_ik_solve_mesh)
 * or cfs_ik_solve_device (cfs_ik_solve_mesh_device) refuses; nmesh < 1; d->nobs + nmesh > CFS_MAX_OBS; NULL meshes, a NULL entry or
 * NULL D_mesh; a D_mesh that is not finite and > 0; a mesh of another device; unknown flag bits; both variant bits set (or
 * CFS_IK_MESH_PER_LANE with CFS_IK_MESH_SMALL_FRONTIER).  flags: 0 (the default variant), or a developer switch with the value and
 * the meaning of RRT's (results are bit-identical under every value): */
#define CFS_IK_MESH_PER_LANE 1        /* variant A: one (mesh, link) pair per lane, private threshold query                              */
#define CFS_IK_MESH_WAVE 2            /* variant B: one wave-cooperative traversal over a shared frontier in LDS (the default)           */
#define CFS_IK_MESH_SMALL_FRONTIER 4  /* variant B with a frontier of 8 entries: its overflow path (decided by variant A) under test      */
int cfs_ik_solve_mesh(const cfs_ik_desc *d, int nmesh, const cfs_mesh *const *meshes, const double *D_mesh, int flags, int T,
                      const double *target_pos, const double *target_axis, const double *theta_ref, const cfs_ik_out *out);
int cfs_ik_solve_mesh_device(const cfs_ik_desc *d, int nmesh, const cfs_mesh *const *meshes, const double *D_mesh /* HOST, nmesh */,
                             int flags, int T, const double *target_pos, const double *target_axis, const double *theta_ref,
                             const cfs_ik_out *out, void *stream);
/* pose(theta) and its Jacobian for N configurations, the device functions the solver runs (HOST pointers, like cfs_dist_arm).
 * theta: N x njoint; pos, dir: N x 3; jac: N x 6 x njoint (rows 0-2 d pos / d theta, rows 3-5 d dir / d theta; may be NULL).
 * tool_axis must be finite and not zero.  With tool = robot.cap{njoint}.p(:,1), pos is cfs_dist_arm's pos of that end point. */
int cfs_tool_pose(const cfs_robot *robot, int njoint, const double *tool, const double *tool_axis, int N, const double *theta,
                  double *pos, double *dir, double *jac);

/* ---- Cartesian paths ----------------------------------------------------------------------------------
 * "inverse kinematics" above orients the tool at a goal; this entry moves it there along a straight line.  For T targets at once,
 * and for up to 64 start configurations per target (the candidates: cfs_ik_out.cand_theta with cand_status is accepted as it is),
 * it traces the straight tool line from every start's own pose to the target in K steps and keeps, per target, the start nearest
 * to a reference configuration whose line completes inside the joint limits, without a joint jump and free of the line obstacles.
 * No handle.  pose, residual, Jacobian, steps 1-8, the collision rule (clearance < 0) and the cost are those of "inverse kinematics",
 * word for word; fields of cfs_cart_desc that cfs_ik_desc also has keep their meaning.
 * One wavefront per target, one lane per candidate r = 0..candidates-1, start_r = start[t][r]:
 *   - no start: a coordinate of start_r is not finite or lies outside [lo, hi], or start_state is given and start_state[t][r] != 0:
 *     state 5, end;
 *   - (p0, a0) = pose(start_r); theta_0 = start_r; if theta_0 collides: state 2 with 0 steps done, end;
 *   - for k = 1..K, with s = k/K (K = steps):
 *       p_k = p0 + s*(target_pos - p0);  use_axis = 1: a_k = b/|b|, b = (1-s)*a0 + s*target_axis (every target_axis row is normalised
 *       on entry); |b| <= 1e-6 (or not finite): state 3, end;
 *       steps 1-8 of "inverse kinematics" towards (p_k, a_k), starting at theta_{k-1} with lambda = 1e-2 and it = 0; convergence is
 *       tested before every step, so a point that is already on the line costs 0 iterations;
 *       step 3 (it == max_iter): state 1, end;  step 1 or 4 failing: state 3, end;
 *       otherwise theta_k = the converged configuration; max_c |theta_k,c - theta_{k-1},c| > max_joint_step: state 4, end;
 *       otherwise theta_k collides: state 2, end;  otherwise step k is done;
 *   - step K done: state 0.
 * States of a candidate (cand_status): 0 complete | 1 a step did not converge | 2 collision | 3 numeric | 4 joint jump | 5 no start.
 * Per target: among the candidates in state 0 the one with the smallest sum_c weight_c*((start_c - theta_ref_c)^2) wins -- the cost
 * of "inverse kinematics" on the START, plain IEEE products and sums in joint order --, ties to the lowest candidate (a wave
 * reduction on (cost, lane), no atomics; a cost that is not finite puts the candidate in state 3).  status: 0 solved | 1 some
 * candidate had a start but none completed | 2 no candidate had a start.
 * theta = the winner's start; path = the winner's theta_0..theta_K; selected = the winner or -1; n_ok = candidates in state 0;
 * n_done = the largest number of steps any candidate completed; clearance = the minimum of min_j (d_j - D_j) over the winner's K+1
 * configurations (+inf when nobs = 0).  Rows of targets with status != 0 hold NaN in theta, path and clearance, and selected = -1.
 * cand_done = steps the candidate completed; cand_iter = its iterations summed over the steps; cand_end = the last configuration it
 * reached or tried (theta_K; where the failing step's iteration ended; the theta_k that jumped or collides; NaN in state 5);
 * cand_path = its accepted configurations theta_0..theta_cand_done and NaN in every later row (every row is NaN in state 5 and for
 * a start that collides).  A target's results depend on neither T nor its position in the batch.
 * The collision rule is evaluated at the K+1 configurations, not between them.
 * CFS_ERR_INVALID_ARG, nothing written: everything cfs_ik_solve refuses about the shared fields (a NULL descriptor, out, out->theta
 * or out->status; a robot / njoint cfs_dist_arm refuses or njoint < 2; use_axis not 0 / 1; max_iter outside 1..1000; nobs outside
 * 0..CFS_MAX_OBS; tolerances, tool, lo, hi, weight that are not finite, lo >= hi, weight <= 0, tol <= 0; a tool_axis that is not
 * finite or (use_axis = 1) zero; T < 1; NULL target_pos or theta_ref; use_axis = 1 with a NULL target_axis; nobs > 0 with NULL obs or
 * D); candidates outside 1..64; steps outside 1..256; a max_joint_step that is not finite and > 0; a NULL start; in cfs_cart_path,
 * whose arrays the host can read: a non-finite target_pos, target_axis, theta_ref, obs or D, a zero target_axis row (start is NOT
 * checked: a bad start is state 5); in cfs_cart_path_device: out->path without out->cand_path (path is gathered from cand_path, the
 * launch's workspace, and the device entry allocates nothing; cfs_cart_path stages one itself).
 * cfs_cart_path: HOST pointers throughout, synchronises.  cfs_cart_path_device: lo, hi, weight stay HOST pointers; obs, D, start,
 * start_state, target_pos, target_axis, theta_ref and every array of `out` are DEVICE pointers; enqueued on `stream`, no
 * synchronisation.  A non-finite value in a device array ends the candidates that read it in state 3 (start: state 5). */
typedef struct cfs_cart_desc {
    cfs_robot robot;
    int njoint;                 /* 2..6: the chain of cfs_dist_arm for robot.kind                                        */
    double tool[3];             /* a point in the frame of link njoint                                                   */
    double tool_axis[3];        /* a direction in the same frame (normalised on entry)                                   */
    int use_axis;               /* 0: position only (3 rows) | 1: position + direction (6 rows)                          */
    const double *lo, *hi;      /* njoint each, finite, lo < hi                                                          */
    const double *weight;       /* njoint, > 0, or NULL = ones: the norm of "nearest to theta_ref"                       */
    int candidates;             /* R, 1..64, one lane each                                                               */
    int steps;                  /* K, 1..256 line points after the start                                                 */
    int max_iter;               /* 1..1000, per step                                                                     */
    double max_joint_step;      /* rad, finite, > 0: the largest move of a joint between two line points                 */
    double tol_pos, tol_axis;   /* metres / norm of the direction difference; finite, > 0                                */
    int nobs;                   /* 0..CFS_MAX_OBS line obstacles                                                         */
    const double *obs;          /* nobs x 6: [obs{j}.l(:,1); obs{j}.l(:,2)]                                              */
    const double *D;            /* nobs: obs{j}.D (Lib/RRT_FANUC.m:174)                                                  */
} cfs_cart_desc;
typedef struct cfs_cart_out {
    double *theta;              /* T x njoint                                                                            */
    int *status;                /* T                                                                                     */
    double *path;               /* T x (steps+1) x njoint (may be NULL)                                                  */
    int *selected, *n_ok, *n_done;            /* T (may be NULL)                                                         */
    double *clearance;          /* T (may be NULL)                                                                       */
    int *cand_status, *cand_done, *cand_iter; /* T x candidates (may be NULL)                                            */
    double *cand_end;           /* T x candidates x njoint (may be NULL)                                                 */
    double *cand_path;          /* T x candidates x (steps+1) x njoint (may be NULL)                                     */
} cfs_cart_out;
/* start: T x candidates x njoint; start_state: T x candidates or NULL (= every start is used); target_pos: T x 3; target_axis: T x 3
 * (read when use_axis = 1; may be NULL otherwise); theta_ref: T x njoint */
int cfs_cart_path(const cfs_cart_desc *d, int T, const double *start, const int *start_state, const double *target_pos,
                  const double *target_axis, const double *theta_ref, const cfs_cart_out *out);
int cfs_cart_path_device(const cfs_cart_desc *d, int T, const double *start, const int *start_state, const double *target_pos,
                         const double *target_axis, const double *theta_ref, const cfs_cart_out *out, void *stream);

/* ---- Cartesian paths against mesh obstacles ---------------------------------------------------------------
 * "Cartesian paths" above in a cell that also holds mesh obstacles.  (nmesh, meshes, D_mesh, flags) is the table of cfs_ik_solve_mesh*,
 * with its rules: nmesh >= 1 handles created on the current device that outlive the launch, D_mesh HOST memory in both entries, nmesh
 * margins, finite and > 0, d->nobs + nmesh <= CFS_MAX_OBS, flags 0 or CFS_IK_MESH_PER_LANE / CFS_IK_MESH_WAVE / CFS_IK_MESH_SMALL_FRONTIER
 * with IK's values and meaning (results are bit-identical under every value).  cfs_cart_desc and cfs_cart_out are unchanged.
 * The result is defined from the line-only call, so the trace itself never depends on the meshes.  Let (st_L, done_L, iter_L, end_L,
 * path_L) be what cfs_cart_path gives a candidate on the same inputs; rows 0..nrow_L-1 of path_L are its accepted configurations.
 *   1. Row k of path_L is mesh-rejected when some triangle of some mesh j lies strictly closer than thr_j = max(D_mesh[j], 1e-4) to
 *      some link axis of that configuration: exactly the decision of cfs_ik_solve_mesh and cfs_rrt_grow_mesh, an existence test that
 *      does not depend on the traversal order.
 *   2. Let m be the smallest mesh-rejected row among the accepted rows.  If there is none, the candidate's outputs are the line-only
 *      ones, bit for bit.
 *   3. Otherwise cand_status = 2, cand_done = max(m-1, 0), cand_end = row m of path_L (the colliding configuration, as for a line
 *      collision), and rows >= m of cand_path are NaN (m = 0: every row, as for a start that collides with a line).
 *   4. cand_iter = iter_L always.
 *      For state, cand_done, cand_end and cand_path this equals testing the meshes right after the line test at every booked step: the
 *      first event in step order decides (a line-only joint jump at step j with a mesh hit at m < j is state 2).  A candidate the
 *      meshes reject early still traces its whole line.
 *   5. Selection, status, n_ok and n_done follow the rules of "Cartesian paths" on the new states: the smallest cost of the START among
 *      the candidates in state 0, ties to the lowest candidate, the cost taken to the last bit as cfs_cart_path computes it.
 *   6. clearance of a target with a winner = the minimum over the winner's K+1 configurations of min(line clearance, min_j (dm_j -
 *      D_mesh[j])), dm_j = the exact, unbounded mesh distance of the nearest link axis (the functions of cfs_dist_arm_mesh, evaluated
 *      WITH FMA contraction as there); NaN without a winner.  A threshold decision within rounding may differ from cfs_rrt_grow_mesh's.
 * CFS_ERR_INVALID_ARG, nothing written: everything cfs_cart_path (cfs_cart_path_mesh) or cfs_cart_path_device
 * (cfs_cart_path_mesh_device) refuses, and everything cfs_ik_solve_mesh* refuses about the mesh table; in cfs_cart_path_mesh_device
 * also a NULL out->cand_path, with or without out->path: it is the workspace between the three launches (the trace, the mesh walk, the
 * selection) and the device entry allocates nothing; cfs_cart_path_mesh stages one itself.  Pointers are HOST / DEVICE as in
 * cfs_cart_path / cfs_cart_path_device; the device entry enqueues on `stream` and synchronises nothing.  A target's results depend
 * on neither T nor its position in the batch; there are no atomics on the normal path. */
int cfs_cart_path_mesh(const cfs_cart_desc *d, int nmesh, const cfs_mesh *const *meshes, const double *D_mesh, int flags, int T,
                       const double *start, const int *start_state, const double *target_pos, const double *target_axis,
                       const double *theta_ref, const cfs_cart_out *out);
int cfs_cart_path_mesh_device(const cfs_cart_desc *d, int nmesh, const cfs_mesh *const *meshes, const double *D_mesh /* HOST, nmesh */,
                              int flags, int T, const double *start, const int *start_state, const double *target_pos,
                              const double *target_axis, const double *theta_ref, const cfs_cart_out *out, void *stream);

/* ---- Tool paths --------------------------------------------------------------------------------------------
 * "Cartesian paths" above moves the tool along one straight line; these entries move it along a polyline of M tool poses (a chain of
 * straight moves: a bead, a seam, "down - across - up").  For T targets at once, and for up to 64 start configurations per target (the
 * candidates: cfs_ik_out.cand_theta with cand_status of an inverse-kinematics call at the first pose is accepted as it is), they follow
 * the target's whole polyline from every start and keep, per target, the start nearest to a reference configuration whose path
 * completes inside the joint limits, without a joint jump and free of the line obstacles.  No handle.  cfs_cart_desc and cfs_cart_out
 * are unchanged, with these meanings: d->steps = K is the number of sub-steps per segment, npts = M the number of poses of the
 * polyline; a path has N = (M-1)*K + 1 rows, and every "steps+1" in cfs_cart_out reads N.  path_pos: T x M x 3, the points P_0..P_{M-1}
 * of every target; path_axis: T x M x 3, the tool directions A_0..A_{M-1}, read when use_axis = 1 (may be NULL otherwise); every row
 * is normalised where it is read, as target_axis is above.
 * The contract is "Cartesian paths" word for word -- pose, residual, Jacobian, steps 1-8, the collision rule (clearance < 0) and the
 * cost are those of "inverse kinematics" --, with these changes.
 *   Rows.  Row 0 is (P_0, A_0).  Row n >= 1 lies on segment i = (n-1) div K, with k = n - i*K and s = k/K: its point is
 *     p_n = P_i + s*(P_{i+1} - P_i), its axis (use_axis = 1) a_n = b/|b|, b = (1-s)*A_i + s*A_{i+1}; |b| <= 1e-6 (or not finite):
 *     state 3, end.  Two consecutive axes that are opposite therefore end a candidate at the middle of that segment (or, for odd K,
 *     not at all: no row lies there).  A segment of length zero is followed like any other.
 *   No start (state 5): as in cfs_cart_path.
 *   Every row n = 0..N-1, row 0 included: steps 1-8 of "inverse kinematics" towards (p_n, a_n), with lambda = 1e-2 and it = 0,
 *     starting at the configuration before it, theta_{n-1} (for row 0: the start).  Convergence is tested before every step, so a start
 *     that solves (P_0, A_0) costs 0 iterations and row 0 of its path is then the start, bit for bit.
 *     step 3 (it == max_iter): state 1, end;  step 1 or 4 failing: state 3, end;
 *     otherwise theta_n = the converged configuration; max_c |theta_n,c - theta_{n-1},c| > max_joint_step: state 4, end -- ROW 0 IS
 *     TESTED AGAINST THE START, so a start far from the first pose is a joint jump;
 *     otherwise theta_n collides: state 2, end;  otherwise row n is accepted.
 *   Row N-1 accepted: state 0.
 * States of a candidate: those of cfs_cart_path (0 complete | 1 a row did not converge | 2 collision | 3 numeric | 4 joint jump | 5 no
 * start).  cand_done, cand_end, cand_iter and cand_path keep cfs_cart_path's conventions exactly, with K replaced by N-1: cand_done =
 * the index of the last accepted row, 0 when none was accepted; cand_iter = the iterations summed over the rows, row 0's included;
 * cand_end = the last configuration reached or tried (NaN in state 5); cand_path = the accepted configurations theta_0..theta_cand_done
 * and NaN in every later row (every row when none was accepted).
 * The cost, the selection, theta (the winner's START, not row 0 of its path), status, selected, n_ok, n_done, path and clearance (the
 * minimum over the winner's N configurations) are cfs_cart_path's.  The collision rule is evaluated at the N configurations, not
 * between them.  A target's results depend on neither T nor its position in the batch.
 * cfs_cart_follow_mesh*: rules 1-6 of "Cartesian paths against mesh obstacles" applied to the line-only answer of cfs_cart_follow on
 * the same inputs, with K+1 read as N; the mesh table, its flags and its refusals are those of cfs_cart_path_mesh*.
 * CFS_ERR_INVALID_ARG, nothing written: everything cfs_cart_path* / cfs_cart_path_mesh* refuse about the shared fields (path_pos in
 * the place of target_pos, path_axis in the place of target_axis), including, in the device entries, out->path without out->cand_path
 * (cfs_cart_follow_device) and a NULL out->cand_path (cfs_cart_follow_mesh_device); npts outside 2..257; (npts-1)*steps > 256; a NULL
 * path_pos; use_axis = 1 with a NULL path_axis; in the host entries, whose arrays the host can read: a non-finite path_pos or
 * path_axis, a zero path_axis row (start is NOT checked: a bad start is state 5).
 * cfs_cart_follow / cfs_cart_follow_mesh: HOST pointers throughout, synchronise.  The _device entries: lo, hi, weight (and D_mesh) stay
 * HOST pointers; obs, D, start, start_state, path_pos, path_axis, theta_ref and every array of `out` are DEVICE pointers; enqueued on
 * `stream`, no synchronisation.  A non-finite value in a device array ends the candidates that read it in state 3 (start: state 5). */
/* start: T x candidates x njoint; start_state: T x candidates or NULL; path_pos, path_axis: T x npts x 3; theta_ref: T x njoint */
int cfs_cart_follow(const cfs_cart_desc *d, int T, int npts, const double *start, const int *start_state, const double *path_pos,
                    const double *path_axis, const double *theta_ref, const cfs_cart_out *out);
int cfs_cart_follow_device(const cfs_cart_desc *d, int T, int npts, const double *start, const int *start_state, const double *path_pos,
                           const double *path_axis, const double *theta_ref, const cfs_cart_out *out, void *stream);
int cfs_cart_follow_mesh(const cfs_cart_desc *d, int nmesh, const cfs_mesh *const *meshes, const double *D_mesh, int flags, int T, int npts,
                         const double *start, const int *start_state, const double *path_pos, const double *path_axis,
                         const double *theta_ref, const cfs_cart_out *out);
int cfs_cart_follow_mesh_device(const cfs_cart_desc *d, int nmesh, const cfs_mesh *const *meshes, const double *D_mesh /* HOST, nmesh */,
                                int flags, int T, int npts, const double *start, const int *start_state, const double *path_pos,
                                const double *path_axis, const double *theta_ref, const cfs_cart_out *out, void *stream);

/* ---- Path timing ---------------------------------------------------------------------------------------------
 * The entries above return joint rows with no clock on them.  These put one on: for G groups of R paths of N rows each (cfs_cart_out's
 * cand_path with cand_status is accepted as it is, G = T, R = candidates; `path` is the case R = 1) they compute, per path, the fastest
 * pass through its rows that keeps every joint inside its speed and acceleration limits and the tool point under a feed rate, at rest
 * at both ends (and at the stop rows), and per group the path that completes soonest.  No handle.
 * Definition, per path with rows q_0..q_{N-1}, one unit of the path parameter s per row.  All arithmetic is IEEE double in the order
 * written, no fused multiply-add; min / max over joints run in joint order (they are exact, so the order does not matter).
 *   d_n = q_{n+1} - q_n (n = 0..N-2);  kappa_n = d_n - d_{n-1} at interior rows, 0 at rows 0 and N-1;
 *   m_{n,c} = max(|d_{n-1,c}|, |d_{n,c}|), the one neighbour that exists at the two ends;
 *   l_n = |p_{n+1} - p_n| = sqrt((dx*dx + dy*dy) + dz*dz), p_n the tool point of row n ("inverse kinematics": pose(theta), `tool`);
 *   e_n = max(l_{n-1}, l_n), the one neighbour at the two ends.
 *   b_n = (ds/dt)^2 at row n.  On segment n the path acceleration u_n = (b_{n+1} - b_n)/2 is constant and the joint acceleration is
 *   taken as kappa_{n,c}*b_n + d_{n,c}*u_n.
 *   cap_n = min( min_c (vmax_c / m_{n,c})^2,  min_c (curve_share*amax_c) / |kappa_{n,c}|,  (feed / e_n)^2 ), a term with a zero
 *     denominator (and the feed term with feed = +inf) left out; cap_n = 0 at rows 0 and N-1 and, with stop_every = k >= 2, at every
 *     row n with n mod k == 0.
 *   ubar_n (segment n) = min_c (amax_c - |kappa_{n,c}|*cap_n) / |d_{n,c}|; a joint with kappa_{n,c} = 0 contributes amax_c/|d_{n,c}|
 *     (no product), a joint with d_{n,c} = 0 nothing.  ubar_n >= (1 - curve_share)*amax_c/|d_{n,c}| > 0, so
 *     |kappa*b_n + d*u_n| <= amax holds for every b_n <= cap_n, |u_n| <= ubar_n: curve_share splits a joint's acceleration between
 *     following the curve and changing speed, which makes the profile conservative against the true limits, never beyond them.
 *   backward: K_{N-1} = cap_{N-1}, K_n = min(cap_n, K_{n+1} + 2*ubar_n);  forward: b_0 = K_0, b_{n+1} = min(K_{n+1}, b_n + 2*ubar_n):
 *     the pointwise largest profile of that constraint set.
 *   sdot_n = sqrt(b_n);  time_0 = 0, time_{n+1} = time_n + 2/(sdot_n + sdot_{n+1}) (exact for constant u);  duration = time_{N-1}.
 * status of a path, the first that applies: 1 not timed (state given and its entry != 0) | 2 numeric: a row holds a non-finite value |
 * 4 repeated row: some d_n is zero in every joint (a polyline segment of length zero produces such bit-equal rows: the caller drops
 * them before timing) | 3 stalled: two consecutive rows with b = 0 (a stop row next to an end or to another stop row) | 2 the duration
 * is not finite | 0 timed.  time, sdot and duration of a path with status != 0 hold NaN.
 * Per group: selected = the status-0 path with the smallest duration, the lowest index on a tie, -1 without one; group_status = 0 with
 * a selected path, else 1.  A path's results depend on neither G, R nor its position in the batch.
 * CFS_ERR_INVALID_ARG, nothing written: a NULL descriptor; the robot / njoint refusals of cfs_ik_solve (njoint 2..6); G < 1; R outside
 * 1..64; N outside 3..257; stop_every 1 or negative; NULL vmax / amax or an entry that is not finite and > 0; feed that is NaN or
 * <= 0 (+inf: no cap, no forward kinematics runs, robot geometry and tool are not used); with a finite feed a non-finite tool;
 * curve_share outside (0, 1); NULL paths, out, out->duration or out->status; out->time without out->sdot (sdot is the workspace between
 * the two passes); in cfs_path_time_device a NULL out->sdot (nothing is allocated there; cfs_path_time stages its own).
 * cfs_path_time: HOST pointers throughout, synchronises; values of `paths` are not refused (status 2).  cfs_path_time_device: vmax and
 * amax stay HOST pointers; paths, state and every array of `out` are DEVICE pointers; enqueued on `stream`, nothing allocated, no
 * synchronisation.
 * Measured: a change of 1e-12 rad in every entry of every row changes no status and moves a time stamp by at
 * most 1.5e-9 s on paths of 2 to 60 s (the CPU restatement, three robots, stops none and every 4 rows); the device equals the
 * restatement bit for bit without a feed and within 3.4e-14 s with one.  One MI355X, M200i, cfs_path_time_device on outputs allocated
 * once: 1 024 x 64 paths of 17 rows 0.085 ms (0.143 ms with a feed), of 257 rows 1.73 ms (2.37 ms); 1 024 x 1 paths 0.060 ms
 * (0.124 ms) and 0.83 ms (1.75 ms). */
typedef struct cfs_time_desc {
    cfs_robot robot;
    int njoint;            /* 2..6 */
    double tool[3];        /* tool point in the frame of link njoint (read with a finite feed) */
    const double *vmax;    /* njoint, rad/s, finite and > 0 */
    const double *amax;    /* njoint, rad/s^2, finite and > 0 */
    double feed;           /* m/s, > 0; +inf: no cap on the tool point's speed */
    double curve_share;    /* in (0, 1): the share of amax that following the curve may use */
    int stop_every;        /* 0: rest at the two ends only; k >= 2: also at every row that is a multiple of k */
} cfs_time_desc;

typedef struct cfs_time_out {
    double *time;          /* G x R x N, may be NULL */
    double *sdot;          /* G x R x N, may be NULL in cfs_path_time only */
    double *duration;      /* G x R */
    int *status;           /* G x R */
    int *selected;         /* G, may be NULL */
    int *group_status;     /* G, may be NULL */
} cfs_time_out;

/* paths: G x R x N x njoint; state: G x R or NULL */
int cfs_path_time(const cfs_time_desc *d, int G, int R, int N, const double *paths, const int *state, const cfs_time_out *out);
int cfs_path_time_device(const cfs_time_desc *d, int G, int R, int N, const double *paths, const int *state, const cfs_time_out *out,
                         void *stream);

/* ---- Tool-path audit -------------------------------------------------------------------------------------------
 * "Cartesian paths" and "Tool paths" evaluate their collision rule at the N rows of a path; a controller moves the joints linearly
 * between the rows ("Path timing" assumes the same).  These entries measure that motion: for G groups of R paths of N rows each
 * (cfs_cart_out's cand_path with cand_status is accepted as it is, G = T, R = candidates; `path` is the case R = 1) they return, per
 * path, the clearance from the line obstacles and the deviation of the tool point from the chord, each sampled and each with a bound
 * that holds between the samples.  No handle.
 * Motion.  On segment n = 0..N-2 the motion is theta(sigma) = q_n + sigma*d_n, d_n = q_{n+1} - q_n, sigma in [0, 1].  The samples are
 *   sigma_k = k/S, k = 0..S, S = d->substeps.  The sample sigma = 1 is row n+1 itself, read from the path and not recomputed.
 * Clearance at a sample: min_j (d_j - D_j), d_j = cfs_dist_arm's distance to obstacle j with its near-zero surrogate: the clearance of
 *   "inverse kinematics", the number cfs_cart_out.clearance reports.  +inf when nobs = 0.  A NaN sticks.
 * Per path (all G x R):
 *   clear_rows   the minimum over the N rows.  For the winner of cfs_cart_path / cfs_cart_follow this is its `clearance`: the same
 *                expression of the same device functions, in a kernel compiled on its own, so NOT promised bit for bit; the two agree
 *                to the parity tolerance below (on the shapes tested they are equal).
 *   clear_path   the minimum over all (N-1)*S + 1 samples.
 *   s_path, link_path, obs_path   where the first such minimum lies (lowest n, then lowest k): the path parameter n + k/S; the obstacle
 *                j (0-based) with the smallest d_j - D_j there, the lowest on a tie; the link (1-based) closest to that obstacle,
 *                cfs_dist_arm's first minimum.  With nobs = 0: s_path = 0, link_path = obs_path = -1.
 *   clear_lower  the minimum over all sub-intervals [sigma_k, sigma_{k+1}] of every segment of (c_k + c_{k+1})/2 - L_n/(2S), c the
 *                clearance at the two ends, L_n = max over links k of sum_{m<=k} |d_{n,m}|*rho[m][k], rho the matrix of "clearance
 *                audit between the waypoints" (the reach of capsule k about the axis of joint m).
 *                Guarantee: if clear_lower > 0, every capsule axis stays at least D_j + clear_lower away from every obstacle j for
 *                all sigma of all segments; a positive bound also rules out the near-zero surrogate.  Nothing is claimed for a bound
 *                that is not positive.  clear_path - clear_lower <= max_n L_n/(2S).
 *   chord_err    the maximum over all samples of e = |p(theta(sigma_k)) - ((1-sigma_k)*p_n + sigma_k*p_{n+1})|, p the tool point of
 *                "inverse kinematics" (pose(theta), `tool`), p_n and p_{n+1} the tool points of the two rows: the distance from the
 *                point a linear Cartesian move commands at the same fraction, which bounds the distance to the chord from above.
 *                e = 0 at the rows.
 *   chord_upper  the maximum over the same sub-intervals of max(e_k, e_{k+1}) + A_n/(8*S*S),
 *                A_n = sum_m sum_l |d_{n,m}|*|d_{n,l}|*rt[max(m,l)], rt[m] = sum_{j=m..njoint-1} len_j + |tool|, len_j the length of
 *                the translation of link j as rho takes it.  A_n bounds |d^2 p / d sigma^2| on the segment; the second term is the
 *                error of linear interpolation over a sub-interval of length 1/S.
 *                Guarantee: the tool point never leaves the same-fraction chord point by more than chord_upper.
 *   status       the first that applies: 1 not audited (state given and its entry != 0) | 2 a row holds a non-finite value | 0 audited.
 *                Every floating-point output of a path with status != 0 holds NaN, link_path and obs_path hold -1.
 *   state_out    the input state where it is non-zero; else 3 where status = 2; else 6 where clear_lower < min_clearance; else 7
 *                where chord_upper > max_chord; else 0 (a NaN bound fails a threshold that is on).  6 and 7 extend the candidate
 *                states 0..5 of cfs_cart_out.cand_status, so state_out goes into cfs_path_time's `state` as it is and the soonest
 *                path is then chosen among those that pass.  With both thresholds off (-inf, +inf) state_out equals state on
 *                finite paths.
 * No atomics: the result is deterministic, and a path's results depend on neither G, R nor its position in the batch.
 * CFS_ERR_INVALID_ARG, nothing written: a NULL descriptor; the robot / njoint refusals of cfs_ik_solve (njoint 2..6); G < 1; R outside
 * 1..64; N outside 2..257 (a line traced with steps = 1 has two rows); substeps outside 1..64; nobs outside 0..CFS_MAX_OBS; nobs > 0
 * with a NULL obs or D; a non-finite tool; min_clearance NaN or +inf; max_chord NaN or <= 0; NULL paths, out or out->status; in
 * cfs_path_audit, whose arrays the host can read, a non-finite obs or D (values of `paths` are not refused: status 2).
 * cfs_path_audit: HOST pointers throughout, synchronises.  cfs_path_audit_device: obs, D, paths, state and every array of `out` are
 * DEVICE pointers; enqueued on `stream`, nothing allocated, no synchronisation.
 * Parity: the device is compared with a CPU restatement within max(1000 x the movement of the restatement's
 * own outputs under a change of 1e-12 rad in every entry of every row, 1e-10); status, state_out, link_path and obs_path are equal.
 * Measured: one MI355X, M200i, two line obstacles, 1 024 x 64 paths of 17 rows: 1.91 ms per launch at S = 4,
 * 2.36 ms at S = 8, 3.25 ms at S = 16. */
typedef struct cfs_audit_desc {
    cfs_robot robot;
    int njoint;             /* 2..6 */
    double tool[3];         /* tool point in the frame of link njoint */
    int nobs;               /* 0..CFS_MAX_OBS line obstacles */
    const double *obs;      /* nobs x 6, rows [l(:,1); l(:,2)] */
    const double *D;        /* nobs margins */
    int substeps;           /* S, 1..64 */
    double min_clearance;   /* finite, or -inf: no test */
    double max_chord;       /* > 0, or +inf: no test */
} cfs_audit_desc;

typedef struct cfs_audit_out {  /* G x R each; every array but status may be NULL */
    double *clear_rows;
    double *clear_path;
    double *s_path;
    double *clear_lower;
    double *chord_err;
    double *chord_upper;
    int *link_path;
    int *obs_path;
    int *status;
    int *state_out;
} cfs_audit_out;

/* paths: G x R x N x njoint; state: G x R or NULL */
int cfs_path_audit(const cfs_audit_desc *d, int G, int R, int N, const double *paths, const int *state, const cfs_audit_out *out);
int cfs_path_audit_device(const cfs_audit_desc *d, int G, int R, int N, const double *paths, const int *state, const cfs_audit_out *out,
                          void *stream);

/* ---- developer / test entry points -------------------------------------------------------------------
 * No caller of the path needs these; they exist so that every shortcut the solver takes can be switched off and compared
 * under pytest (tests/test_gpu_shortcuts.py), and for the cycle-stamp / step-trace probes under tools/.  All state is per
 * handle: nothing is read from the environment, nothing is process-wide.  Results with and without each switch are the
 * same optimum of the same strictly convex QPs; what the tests assert bit for bit, and what to a tolerance, is stated there. */
/* value 1 is retired (it was CFS_DBG_GATHER_ROLLOUTS): do not reuse it */
#define CFS_DBG_NO_REFINE 2         /* no iterative refinement of the step directions                                                  */
#define CFS_DBG_NO_WARM_START 8     /* every QP starts from the empty active set                                                       */
#define CFS_DBG_NO_CERTIFICATE 16   /* CFS_FANUC: no step-free infeasibility certificate (infeasible QPs are proven by the dual steps)  */
#define CFS_DBG_NO_PRUNE 32         /* num_jac evaluates every link at every evaluation point (no candidate pruning)                    */
#define CFS_DBG_NO_AUTO_ORDER 64    /* no automatic launch order                                                                       */
#define CFS_DBG_TIER_W1 128         /* one workgroup per compute unit (64 register-resident columns of the inverse Gram matrix)         */
#define CFS_DBG_CLEAR_NO_BOUND 256  /* cfs_clearance_mesh*: every link's hierarchy query starts unbounded (not from the running minimum)   */
#define CFS_DBG_CLEAR_SEED 512      /* cfs_clearance_mesh*: waypoint poses first, sub-samples seeded with their winning triangles       */
/* mask: OR of CFS_DBG_*; warm_max: largest previous active set a warm start takes (0 = default: 24 rows for CFS_FANUC, the
 * register-resident columns for PSGCFS_FANUC; <= 64); polish_tol: relative drift of an active row at the optimum that
 * triggers the projection (<= 0 = default 1e-11).  Applies to the following solves / pieces of this handle. */
int cfs_debug_set_options(cfs_problem *p, int mask, int warm_max, double polish_tol);
/* which tier of the fused solver a solve of this shape runs (no handle, no device touched): *tier = 0 w1 (one workgroup per compute
 * unit), 1 w2m (two per unit, CFS_FANUC), 2 w2s (two per unit, PSGCFS_FANUC); force_w1 != 0: as under CFS_DBG_TIER_W1.
 * per_waypoint / limits != 0: a CFS_OBS_PER_WAYPOINT handle / one with joint limits, which run the tier of the plain static shape
 * or are refused.  CFS_ERR_INVALID_ARG, *tier unwritten, for a NULL tier, njoint outside 2..6, H outside 1..CFS_MAX_H, nobs outside
 * 1..CFS_MAX_OBS, an unknown mode, or a shape whose handle would be refused for the on-chip budget. */
int cfs_debug_fused_tier(int njoint, int H, int nobs, int mode, int per_waypoint, int limits, int force_w1, int *tier);
/* cycle stamps: B > 0, out == NULL: enable for the next solves of <= B problems; out != NULL: read 12 accumulators per
 * problem (HOST pointer, synchronises); B <= 0, out == NULL: off */
int cfs_debug_stamps(cfs_problem *p, int B, unsigned long long *out);
/* trace of the active-set steps of problem b: 8 doubles per step, at most cap steps; cap <= 0: off.
 * cfs_debug_trace_read: out = (cap+1)*8 doubles (HOST), out[0] = number of records */
int cfs_debug_trace_begin(cfs_problem *p, int b, int cap);
int cfs_debug_trace_read(cfs_problem *p, double *out);
/* the launch-order pre-pass alone (cfs_set_launch_order, automatic order), for B in 1..max_batch whatever the device's compute
 * units: key[b] = (waypoint, line obstacle) pairs of x_init[b] whose clearance is below the obstacle's margin, order = the problems
 * by descending key, ties by index, exactly as a solve of these inputs would compute them.  HOST pointers: x_init B x (H*nstate);
 * obs B x nobs x 6 (B x H x nobs x 6 per waypoint); key, order: B each, either may be NULL, not both.  A handle without a line
 * obstacle gives zero keys and the identity order.  Synchronises the device. */
int cfs_debug_launch_order(cfs_problem *p, int B, const double *x_init, const double *obs, int *key, int *order);
/* log of u after every outer iteration (either solver; the solve itself is unchanged): on != 0 allocates
 * max_batch x MAX_O_ITER x nn doubles; cfs_debug_read_u_log copies the first B problems to `out` (HOST) */
int cfs_debug_log_u(cfs_problem *p, int on);
int cfs_debug_read_u_log(cfs_problem *p, int B, double *out);
/* cfs_rrt_grow_mesh*, variant B: proposals of the current device, since the last reset, whose frontier overflowed its capacity and
 * that variant A decided instead (one counter per device and process; HOST pointer, may be NULL; synchronises the device).
 * With CFS_RRT_MESH_SMALL_FRONTIER it shows that the overflow path ran. */
int cfs_debug_rrt_frontier_overflows(unsigned long long *count, int reset);
/* cfs_ik_solve_mesh*, variant B: the same counter for candidate poses (restarts) whose frontier overflowed */
int cfs_debug_ik_frontier_overflows(unsigned long long *count, int reset);
/* cfs_cart_path_mesh*, variant B: the same counter for the poses (rows of a traced line) that variant A decided for it */
int cfs_debug_cart_frontier_overflows(unsigned long long *count, int reset);
/* cfs_mesh_segment_distance, arguments and outputs alike, evaluated WITH FMA contraction: the build of the hierarchy traversal
 * and of the exact geometry that cfs_dist_arm_mesh, the solvers' linearisation, the clearance audits, cfs_ik_solve_mesh and
 * cfs_cart_path_mesh run, made reachable for arbitrary segments (tests/test_gpu_mesh_geometry.py) */
int cfs_debug_mesh_segment_distance_contracted(const cfs_mesh *m, int n, const double *segs, double *dis, double *points, int *tri);

#ifdef __cplusplus
}
#endif
#endif /* CFS_HIP_H */
