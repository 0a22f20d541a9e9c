// cfs_problem.h -- the problem-family handle (device constants + workspace of cfs_problem_create).  Private to the translation units of
// libcfs_hip.so that own an entry point taking a handle; not installed, not part of the C ABI.
#pragma once
#include "cfs_host.h"

// State of the handle that is reset as a whole: resetting one is assigning a fresh one (the buffers free what they held).
struct MeshSet {                          // cfs_problem_set_meshes: the meshes and the workspace of their linearisation
    DevBuf<DevMesh> meshes_d;
    std::vector<DevMesh> meshes_h;        // host copy of meshes_d (the stored triangles give c_j and r_j)
    std::vector<double> mesh_frame;       // nmesh x 4: (c_j, r_j), filled by the first cfs_problem_set_mesh_motion after set_meshes
    DevBuf<double> st_cost, m_ends, m_base, m_shift, m_upper, m_pd, m_pnd;
    DevBuf<int> st_done, m_tri, m_near, m_pi;
};
struct MeshMotion {                       // cfs_problem_set_mesh_motion, and what cfs_clearance_mesh_motion* keeps of it
    DevBuf<double> mesh_pose;             // nmesh x H x 12 inverse poses (null: the meshes are static)
    DevBuf<double> mesh_itv;              // per (mesh, interval), CLEAR_ITV doubles each
    DevBuf<double> cmm_pose, cmm_v;       // the pose table of the last audit, kept per (sub-steps, motion generation): rebuilt only when either changes
    int cmm_S = 0, cmm_cap = 0, cmm_gen = -1;
    int turn_mesh = -1, turn_wp = 0;      // first (mesh, waypoint) whose pose is more than a quarter turn from the one before; -1: none
};
struct ClearMeshWork {                    // cfs_clearance_mesh*: per-sample workspace for S sub-steps (grown by the first audit that needs more) and rho on the device
    DevBuf<double> cm_d, cm_L, cm_rho;
    DevBuf<int> cm_lk, cm_tri, cm_seed;
    int S = 0;
};

struct cfs_problem {
    cfs_problem_desc d;
    int device;
    int nn, ns, nx;
    double lmax_vel, lmax_H;
    DevRobot hrobot;
    DevBuf<DevRobot> rb;
    DevBuf<double> QQ, Hinv, Hq, M1n, M2n, lim, maxin, margin;
    DevBuf<double> F1, F2, Cq;   // per-problem cost terms from (x0, xg), set by cfs_set_state_cost
    DevBuf<DevCost> cost;        // structure of QQ (handles created from the cost weights)
    std::vector<double> QQ_host; // what cfs_problem_family hands back
    // workspace (max_batch problems)
    DevBuf<double> x0, qu, dist, grad, Yg, Pt, u_hist, qu_hist;
    DevBuf<int> noise_row, linkid, pool_flag;
    bool pool_dirty = false;   // a solve of this handle failed to enqueue: clear the spill-pool flags before the next one
    int pool_n = 1;            // slots of the spill pool (Yg / Pt): one per workgroup that can be resident at once, never more than max_batch
    DevBuf<int> order, okey;   // launch order of the fused solver, automatic: violation count of the initial trajectory -> rank
    DevBuf<int> order_user;    // the caller's permutation (cfs_set_launch_order); a solve of another batch size falls back to the automatic order
    int n_cu = 256;            // compute units of the handle's device: a batch of at most n_cu problems starts all at once
    int order_mode = 0, order_n = 0;   // 0 automatic, 1 given (order_n entries), 2 identity
    // mesh obstacles (cfs_problem_set_meshes): the last nmesh of the nobs obstacles
    int nmesh = 0;
    MeshSet mesh;
    MeshMotion mm;
    int motion_gen = 0;                   // counts every change of the poses, across resets of mm: the pose table of mm.cmm_gen is rebuilt when they differ
    ClearMeshWork cm;
    // developer / test switches (cfs_debug_*, include/cfs_hip.h): per handle, no process-wide state
    int dbg_mask = 0, dbg_warm_max = 0;
    double dbg_polish_tol = 1e-11;        // = the constraint scan's own feasibility tolerance
    DevBuf<unsigned long long> stamps;    // 12 cycle accumulators per problem
    int stamps_B = 0;
    DevBuf<double> trace;                 // 8 doubles per active-set step of problem trace_b
    int trace_b = -1, trace_cap = 0;
    DevBuf<double> u_log;                 // max_batch x MAX_O_ITER x nn: u after every outer iteration (both solvers)
    int jac = CFS_JAC_FD_LITERAL;         // cfs_problem_set_jacobian: which linearisation every later launch of this handle runs
    int infeas = CFS_INFEAS_STOP;         // cfs_problem_set_infeasible_policy
    int motion = CFS_OBS_STATIC;          // cfs_problem_set_obstacle_motion: obs arrays are B x nobs x 6 | B x H x nobs x 6
    bool limited = false;                 // cfs_problem_set_joint_limits: position rows in every QP (the LIM kernels); lim[nj, 3nj) = [lo; hi]
    std::vector<double> jlim;             // [lo; hi] as set (2 nj; empty: no limits)
    double rho[CFS_MAX_LINKS * CFS_MAX_LINKS];   // cfs_clearance*: reach of capsule k about the axis of joint m (cfs_clear_build_rho)
    double soft_weight = 0.0;             // mu of CFS_INFEAS_SOFTEN (0: never set)
    DevBuf<double> soft_viol;             // max_batch x MAX_O_ITER: viol_all of the last whole solve (allocated with SOFTEN)
    DevBuf<int> soft_n;                   // max_batch: n_soft of the last whole solve
    bool prof = false;
    std::vector<hipEvent_t> ev;   // 4 per profiled solve: gemm start/stop, fused start/stop
    std::vector<hipEvent_t> ev_free;   // recycled events: none is created inside a timed region once the pool is warm
    void reset_mesh_motion() { mm = MeshMotion{}; ++motion_gen; }   // the handle's meshes are static again
    ~cfs_problem()                        // the caller has selected `device`; the buffers free themselves
    {
        for (hipEvent_t e : ev) (void)hipEventDestroy(e);
        for (hipEvent_t e : ev_free) (void)hipEventDestroy(e);
    }
};

inline bool cfs_moving(const cfs_problem *p) { return p->motion == CFS_OBS_PER_WAYPOINT; }
// obstacle rows per problem in every obs array the handle reads: nobs (static) | H x nobs (per waypoint)
inline size_t cfs_obs_rows(const cfs_problem *p) { return (size_t)p->d.nobs * (cfs_moving(p) ? (size_t)p->d.H : 1); }
inline int cfs_check_batch(const cfs_problem *p, int B)
{
    if (!p) return cfs_fail(CFS_ERR_INVALID_ARG, "NULL handle");
    if (B < 1 || B > p->d.max_batch) return cfs_fail(CFS_ERR_INVALID_ARG, "B=%d outside 1..max_batch=%d", B, p->d.max_batch);
    return CFS_SUCCESS;
}

// ---- clearance audits (cfs_clear.hip, cfs_clear_mesh.hip): the arrays of one call, host or device ----------------------------------
struct ClearArrays {
    const double *x_, *u, *xR1, *obs;
    double *dist_wp, *dist_path, *dist_lower, *t_path;
    int *link_path, *tri_path;                           // tri_path: the mesh audit only
};
// what all six entries refuse, in one order; mesh: the handle must have meshes (otherwise: must have none) and tri_path is an output;
// motion (cfs_clearance_mesh_motion*, with mesh): mesh motion is admitted, unless two consecutive poses are over a quarter turn apart
int cfs_check_clearance(const cfs_problem *p, int B, int substeps, const ClearArrays &a, bool mesh, bool motion = false);
// cfs_clearance's kernel on the first nline obstacle rows and output columns of the handle
hipError_t cfs_launch_clearance_lines(const cfs_problem *p, int B, int substeps, int nline, const ClearArrays &a, hipStream_t s);
// the host-array entry of every audit: stages the arrays, calls the _device entry on the NULL stream, copies back
int cfs_clearance_host(cfs_problem *p, int B, int substeps, const ClearArrays &h, bool mesh, bool motion = false);
