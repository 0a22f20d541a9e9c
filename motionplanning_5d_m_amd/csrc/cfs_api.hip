// cfs_api.hip -- host side of libcfs_hip.so: the C ABI declared in include/cfs_hip.h.
// Owns the problem-family handle (device constants + workspace) and enqueues the kernels of one
// solve on a caller-supplied stream without any host round trip inside the outer loop.
#include "cfs_problem.h"
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <cstdlib>
#include <new>
#include <vector>

namespace {

thread_local char g_err[512] = "";
int g_device = 0;

int have_device()
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

}  // namespace

int cfs_fail(int code, const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof g_err, fmt, ap);
    va_end(ap);
    return code;
}
int cfs_current_device() { return g_device; }
int cfs_use_device(int device)
{
    if (have_device() == 0) return cfs_fail(CFS_ERR_NO_DEVICE, "no HIP device visible");
    CFS_HIPCHK(hipSetDevice(device));
    return CFS_SUCCESS;
}
int cfs_frontier_overflows(const void *symbol, unsigned long long *count, int reset)
{
    if (!count && !reset) return cfs_fail(CFS_ERR_INVALID_ARG, "nothing to do: count is NULL and reset is 0");
    int rc = cfs_use_device(g_device);
    if (rc) return rc;
    CFS_HIPCHK(hipDeviceSynchronize());
    if (count) CFS_HIPCHK(hipMemcpyFromSymbol(count, symbol, sizeof *count));
    if (reset) {
        const unsigned long long zero = 0ull;
        CFS_HIPCHK(hipMemcpyToSymbol(symbol, &zero, sizeof zero));
    }
    return CFS_SUCCESS;
}
void cfs_build_dev_robot(const cfs_robot &r, DevRobot &d)
{
    memset(&d, 0, sizeof d);
    d.kind = r.kind;
    d.nlink = r.nlink;
    for (int i = 0; i < r.nlink && i < CFS_MAX_LINKS; ++i) {
        d.dh_d[i] = r.DH[i + 1 * r.nlink];
        d.dh_a[i] = r.DH[i + 2 * r.nlink];
        const double al = r.DH[i + 3 * r.nlink];
        d.ca[i] = cos(al);
        d.sa[i] = sin(al);
        d.th_off[i] = 0.0;
        for (int e = 0; e < 6; ++e) d.cap[i * 6 + e] = r.cap[i * 6 + e];
    }
    if (r.kind == CFS_ROBOT_M200I) d.th_off[1] = M_PI / 2;   // dist_arm_3D_200i_2.m:11
    for (int e = 0; e < 3; ++e) d.base[e] = r.base[e];
    if (r.kind == CFS_ROBOT_2L)
        for (int i = 0; i + 1 < 3 && i < CFS_MAX_LINKS; ++i)   // link i uses robot.T(:,i+2) (1-based), CapPos2.m:25
            for (int e = 0; e < 3; ++e) d.t2l[i * 3 + e] = r.T[(i + 1) * 3 + e];
    // every point of the arm stays within `reach` of every joint axis; an evaluation point of num_jac moves each joint
    // by at most eps/2, so no link-obstacle distance changes by more than nlink*eps/2*reach (the segment distance is
    // 1-Lipschitz in the end points).  The pruning margin of the linearisation is a generous multiple of that.
    double reach = 0.0, capmax = 0.0;
    for (int i = 0; i < r.nlink && i < CFS_MAX_LINKS; ++i) {
        reach += (r.kind == CFS_ROBOT_2L) ? sqrt(d.t2l[i * 3] * d.t2l[i * 3] + d.t2l[i * 3 + 1] * d.t2l[i * 3 + 1] + d.t2l[i * 3 + 2] * d.t2l[i * 3 + 2])
                                          : fabs(d.dh_a[i]) + fabs(d.dh_d[i]);
        for (int k = 0; k < 2; ++k) {
            const double *c = d.cap + i * 6 + k * 3;
            capmax = std::max(capmax, sqrt(c[0] * c[0] + c[1] * c[1] + c[2] * c[2]));
        }
    }
    d.shift_bound = r.nlink * (1e-5 / 2) * (reach + capmax);
    d.prune_tol = 1e-3 + 8.0 * d.shift_bound;
}
int cfs_check_robot(const cfs_robot *r, int nj)
{
    if (!r) return cfs_fail(CFS_ERR_INVALID_ARG, "robot is NULL");
    if (r->kind < CFS_ROBOT_M16IB || r->kind > CFS_ROBOT_2L) return cfs_fail(CFS_ERR_INVALID_ARG, "unknown robot kind %d", r->kind);
    if (r->nlink < 1 || r->nlink > CFS_MAX_LINKS) return cfs_fail(CFS_ERR_INVALID_ARG, "robot.nlink %d outside 1..%d", r->nlink, CFS_MAX_LINKS);
    if (nj < 1 || nj > 6 || nj > r->nlink) return cfs_fail(CFS_ERR_INVALID_ARG, "njoint %d unsupported (1..6, <= nlink)", nj);
    if (r->kind == CFS_ROBOT_2L && nj > 2) return cfs_fail(CFS_ERR_INVALID_ARG, "the 2L model has 2 joints");
    return CFS_SUCCESS;
}

// Tier of the fused kernel (cfs_device.h).  Two problems per CU win whenever they fit: measured on config 3, PSGCFS
// 3.6 -> 2.3 ms per solve with w2s, CFS 5.8 -> 5.6 ms with w2m (its infeasibility proofs run active sets of ~100 rows).
// w2s is compiled for the identity Hessian only (PSGCFS), w2m for QQ only (CFS), w1 for both; force_w1: CFS_DBG_TIER_W1.
bool fused_fits(int nj, int H, int nobs) { return fused_fits_tier<FUSED_W1>(nj, H, nobs); }
// The tier is chosen by the plain static plan for every kind of handle: cfs_problem_set_obstacle_motion and cfs_problem_set_joint_limits
// admit a handle only when its plan (move: per-waypoint obstacle rows in the tiles; lim: position rows) fits every tier the plain plan
// fits, so its solves run the same tier and, with constant rows / limits that never bind, the same arithmetic as the plain handle's.
static bool fused_keeps_tier(int nj, int H, int nobs, int mode, bool move, bool lim)
{
    if (!fused_fits_tier<FUSED_W1>(nj, H, nobs, move, lim)) return false;
    if (mode == CFS_MODE_PSGCFS) return fused_fits_tier<FUSED_W2S>(nj, H, nobs, move, lim) == fused_fits_tier<FUSED_W2S>(nj, H, nobs);
    return fused_fits_tier<FUSED_W2M>(nj, H, nobs, move, lim) == fused_fits_tier<FUSED_W2M>(nj, H, nobs);
}
// the four switches of a handle -> the template arguments of its kernels
template <class F> static hipError_t for_bool(bool b, F &&f) { return b ? f(std::true_type{}) : f(std::false_type{}); }
template <FusedTier T>
static hipError_t launch_tier(int nj, const FusedParams &p, hipStream_t s, bool analytic, const SoftParams *soft, bool move, bool lim)
{
    return for_bool(analytic, [&](auto J) { return for_bool(soft != nullptr, [&](auto S) { return for_bool(move, [&](auto M) { return for_bool(lim, [&](auto L) {
        return launch_fused_tier<T, decltype(J)::value, decltype(S)::value, decltype(M)::value, decltype(L)::value>(nj, p, s, soft);
    }); }); }); });
}
// the one rule: read by launch_fused and by cfs_debug_fused_tier
static FusedTier fused_tier(int nj, int H, int nobs, int mode, bool force_w1)
{
    const bool ident = mode == CFS_MODE_PSGCFS;
    if (!force_w1 && ident && fused_fits_tier<FUSED_W2S>(nj, H, nobs)) return FUSED_W2S;
    if (!force_w1 && !ident && fused_fits_tier<FUSED_W2M>(nj, H, nobs)) return FUSED_W2M;
    return FUSED_W1;
}
hipError_t launch_fused(int nj, FusedParams p, hipStream_t s, bool force_w1, bool analytic, const SoftParams *soft, bool move, bool lim)
{
    switch (fused_tier(nj, p.H, p.nobs, p.mode, force_w1)) {
    case FUSED_W2S: return launch_tier<FUSED_W2S>(nj, p, s, analytic, soft, move, lim);
    case FUSED_W2M: return launch_tier<FUSED_W2M>(nj, p, s, analytic, soft, move, lim);
    default: return launch_tier<FUSED_W1>(nj, p, s, analytic, soft, move, lim);
    }
}

extern "C" {

int cfs_abi_version(void) { return CFS_ABI_VERSION; }
const char *cfs_last_error(void) { return g_err; }
int cfs_device_count(void) { return have_device(); }

int cfs_set_device(int device)
{
    const int n = have_device();
    if (n == 0) return cfs_fail(CFS_ERR_NO_DEVICE, "no HIP device visible");
    if (device < 0 || device >= n) return cfs_fail(CFS_ERR_INVALID_ARG, "device %d out of range (0..%d)", device, n - 1);
    g_device = device;
    return CFS_SUCCESS;
}

static size_t pt_stride(int nn) { return nn > 160 ? (size_t)256 * 256 : (nn > 96 ? (size_t)160 * 160 : (size_t)96 * 96); }   // QB*QB >= (QB-PR)*QB in every tier


int cfs_problem_create(const cfs_problem_desc *desc, cfs_problem **out)
{
    if (!desc || !out) return cfs_fail(CFS_ERR_INVALID_ARG, "NULL argument");
    *out = nullptr;
    const int nj = desc->njoint, H = desc->H;
    int rc = cfs_check_robot(&desc->robot, nj);
    if (rc) return rc;
    if (nj < 2) return cfs_fail(CFS_ERR_INVALID_ARG, "njoint %d unsupported (2..6)", nj);
    if (H < 1 || H > CFS_MAX_H) return cfs_fail(CFS_ERR_INVALID_ARG, "H %d outside 1..%d", H, CFS_MAX_H);
    if (desc->nobs < 1 || desc->nobs > CFS_MAX_OBS) return cfs_fail(CFS_ERR_INVALID_ARG, "nobs %d outside 1..%d", desc->nobs, CFS_MAX_OBS);
    if (desc->mode != CFS_MODE_CFS && desc->mode != CFS_MODE_PSGCFS) return cfs_fail(CFS_ERR_INVALID_ARG, "unknown mode %d", desc->mode);
    if (!desc->QQ || !desc->lim || !desc->margin) return cfs_fail(CFS_ERR_INVALID_ARG, "QQ/lim/margin must be given");
    if (desc->mode == CFS_MODE_CFS && !desc->MAX_input) return cfs_fail(CFS_ERR_INVALID_ARG, "MAX_input must be given in CFS mode");
    if (desc->max_batch < 1) return cfs_fail(CFS_ERR_INVALID_ARG, "max_batch must be >= 1");
    if (!fused_fits(nj, H, desc->nobs))
        return cfs_fail(CFS_ERR_INVALID_ARG, "H=%d x nobs=%d x njoint=%d exceeds the 160 KB on-chip budget of one problem (nobs*H*njoint*8 B of gradients must fit next to the solver state)", H, desc->nobs, nj);
    if (desc->MAX_O_ITER < 0) return cfs_fail(CFS_ERR_INVALID_ARG, "MAX_O_ITER must be >= 0");
    const double dt = desc->robot.delta_t;
    if (!(dt > 0)) return cfs_fail(CFS_ERR_INVALID_ARG, "robot.delta_t must be positive");
    const int nn = H * nj, ns = 2 * nj, nx = H * ns;

    if (FamilyRefusal r = check_double_integrator(nj, H, dt, desc->Aaug, desc->Baug)) return cfs_fail(r.code, "%s", r.text);
    if (have_device() == 0) return cfs_fail(CFS_ERR_NO_DEVICE, "no HIP device visible");
    FamilyMatrices fm;                       // H^{-1}, the QP's Hessian inverse, H^{-1}Bpos', H^{-1}Bvel' and the two eigenvalue bounds (cfs_family.cpp)
    if (FamilyRefusal r = family_matrices(nj, H, dt, desc->mode, desc->QQ, fm)) return cfs_fail(r.code, "%s", r.text);
    cfs_problem *p = new (std::nothrow) cfs_problem();
    if (!p) return cfs_fail(CFS_ERR_ALLOC, "out of host memory");
    p->d = *desc;
    p->QQ_host.assign(desc->QQ, desc->QQ + (size_t)nn * nn);
    p->d.QQ = p->d.Aaug = p->d.Baug = p->d.lim = p->d.MAX_input = p->d.margin = nullptr;
    p->device = g_device;
    if (hipDeviceGetAttribute(&p->n_cu, hipDeviceAttributeMultiprocessorCount, g_device) != hipSuccess || p->n_cu < 1) p->n_cu = 256;
    p->nn = nn; p->ns = ns; p->nx = nx; p->lmax_vel = fm.lmax_vel; p->lmax_H = fm.lmax_H;
    cfs_build_dev_robot(desc->robot, p->hrobot);
    cfs_clear_build_rho(p->hrobot, nj, p->rho);
    const size_t Bm = (size_t)desc->max_batch;
    // spill pool (rows of Y beyond LDS, columns of P beyond the registers): one slot per workgroup that can be resident at once (two per
    // compute unit), not one per problem of the batch -- config 4: 512 slots instead of 4 096 (0.4 GB instead of 3.4 GB per handle)
    p->pool_n = (int)std::min<size_t>(Bm, (size_t)2 * p->n_cu);
    const size_t Pn = (size_t)p->pool_n;
    hipError_t e = hipSetDevice(p->device);
    auto up = [&](auto &buf, const auto *src, size_t count) { if (e == hipSuccess) e = buf.upload(src, count); };
    auto room = [&](auto &buf, size_t count) { if (e == hipSuccess) e = buf.alloc(count); };
    up(p->rb, &p->hrobot, 1); up(p->QQ, desc->QQ, (size_t)nn * nn); up(p->Hinv, fm.Hinv.data(), (size_t)nn * nn);
    up(p->M1n, fm.M1n.data(), (size_t)nn * nn); up(p->M2n, fm.M2n.data(), (size_t)nn * nn); up(p->Hq, fm.Hq.data(), (size_t)nn * nn);
    room(p->Pt, Pn * pt_stride(nn));
    room(p->lim, 3 * (size_t)nj);            // [lim | lo | hi]: the last two are written by cfs_problem_set_joint_limits
    if (e == hipSuccess) e = hipMemcpy(p->lim.p, desc->lim, nj * sizeof(double), hipMemcpyHostToDevice);
    if (desc->mode == CFS_MODE_CFS) up(p->maxin, desc->MAX_input, nn);
    else if (e == hipSuccess) e = p->maxin.zeros(nn);
    up(p->margin, desc->margin, desc->nobs);
    room(p->x0, Bm * nn); room(p->qu, Bm * nn); room(p->dist, Bm * desc->nobs * H); room(p->grad, Bm * desc->nobs * H * nj);
    room(p->Yg, Pn * nn * nn);
    if (e == hipSuccess) e = p->pool_flag.zeros(Pn * 16);
    if (desc->mode == CFS_MODE_CFS) { room(p->u_hist, Bm * (size_t)desc->MAX_O_ITER * nn); room(p->qu_hist, Bm * (size_t)desc->MAX_O_ITER * nn); }
    room(p->noise_row, Bm); room(p->linkid, Bm * desc->nobs * H); room(p->order, Bm); room(p->okey, Bm); room(p->order_user, Bm);
    if (e != hipSuccess) {
        delete p;                            // its device was selected above
        return cfs_fail(CFS_ERR_HIP, "device setup failed: %s", hipGetErrorString(e));
    }
    *out = p;
    return CFS_SUCCESS;
}

void cfs_problem_destroy(cfs_problem *p)
{
    if (!p) return;
    (void)hipSetDevice(p->device);
    delete p;
}

int cfs_problem_family(const cfs_problem *p, double *QQ, double *alpha)
{
    if (!p) return cfs_fail(CFS_ERR_INVALID_ARG, "NULL handle");
    if (QQ) memcpy(QQ, p->QQ_host.data(), p->QQ_host.size() * sizeof(double));
    if (alpha) *alpha = p->d.alpha;
    return CFS_SUCCESS;
}

int cfs_problem_create_from_weights(const cfs_problem_desc *desc, const cfs_cost_weights *w, cfs_problem **out)
{
    if (!desc || !w || !out) return cfs_fail(CFS_ERR_INVALID_ARG, "NULL argument");
    *out = nullptr;
    if (!w->Qp || !w->Qv || !w->Rblk) return cfs_fail(CFS_ERR_INVALID_ARG, "Qp/Qv/Rblk must be given");
    const int nj = desc->njoint, H = desc->H;
    if (nj < 2 || nj > 6 || H < 1 || H > CFS_MAX_H) return cfs_fail(CFS_ERR_INVALID_ARG, "njoint %d / H %d unsupported", nj, H);
    const double dt = desc->robot.delta_t;
    if (!(dt > 0)) return cfs_fail(CFS_ERR_INVALID_ARG, "robot.delta_t must be positive");
    WeightFamily wf;                         // Qaug, QQ, cR*(Rblk + Rblk') and alpha = 1/max(svd(QQ)) when the caller left it 0 (cfs_family.cpp)
    family_from_weights(nj, H, dt, w, desc->alpha == 0.0 && desc->mode == CFS_MODE_PSGCFS, wf);
    DevCost hc;
    memset(&hc, 0, sizeof hc);
    for (int c = 0; c < nj; ++c)
        for (int r = 0; r < nj; ++r) {
            hc.Qp[r + c * nj] = w->Qp[r + c * nj];
            hc.Qv[r + c * nj] = w->Qv[r + c * nj];
        }
    memcpy(hc.Rs, wf.Rs, sizeof hc.Rs);
    hc.qc = w->q_cross; hc.ws = w->w_stage; hc.wt = w->w_terminal;
    cfs_problem_desc d2 = *desc;
    d2.QQ = wf.QQ.data();
    d2.Aaug = d2.Baug = nullptr;                           // implied: the double integrator
    if (d2.alpha == 0.0 && d2.mode == CFS_MODE_PSGCFS) d2.alpha = wf.alpha;   // main_FANUC.m:120
    cfs_problem *p = nullptr;
    int rc = cfs_problem_create(&d2, &p);
    if (rc) return rc;
    rc = cfs_set_state_cost(p, wf.Qaug.data());
    if (rc == CFS_SUCCESS) {
        const hipError_t e = p->cost.upload(&hc, 1);
        if (e != hipSuccess) rc = cfs_fail(CFS_ERR_HIP, "device setup failed: %s", hipGetErrorString(e));
    }
    if (rc) { cfs_problem_destroy(p); return rc; }
    *out = p;
    return CFS_SUCCESS;
}

// family-level fields of the fused kernel's parameter block (everything that does not change across a batch)
static void fill_fused_family(const cfs_problem *p, FusedParams &fp, int B)
{
    memset(&fp, 0, sizeof fp);
    fp.rb = p->rb.p; fp.kind = p->d.robot.kind; fp.B = B; fp.H = p->d.H; fp.nobs = p->d.nobs; fp.mode = p->d.mode;
    fp.has_bounds = p->d.mode == CFS_MODE_CFS; fp.max_o_iter = p->d.MAX_O_ITER;
    fp.dt = p->d.robot.delta_t; fp.alpha = p->d.alpha; fp.epsilon_O = p->d.epsilon_O; fp.lmax_vel = p->lmax_vel; fp.lmax_H = p->lmax_H;
    fp.M1 = p->M1n.p; fp.M2 = p->M2n.p; fp.M3 = p->Hq.p; fp.QQ = p->QQ.p; fp.cost = p->cost.p;
    fp.lim = p->lim.p; fp.maxin = p->maxin.p; fp.margin = p->margin.p;
    fp.x0 = p->x0.p;
    fp.Yg = p->Yg.p; fp.Pt = p->Pt.p; fp.pt_stride = pt_stride(p->nn); fp.pool_flag = p->pool_flag.p; fp.pool_n = p->pool_n;
    // kernel switch word: bit 1 = no refinement, bit 3 = no warm start, bit 4 = no step-free certificate
    fp.opt = p->dbg_mask & (CFS_DBG_NO_REFINE | CFS_DBG_NO_WARM_START | CFS_DBG_NO_CERTIFICATE);
    fp.polish_tol = p->dbg_polish_tol;
    fp.warm_max = p->dbg_warm_max;
    fp.no_prune = (p->dbg_mask & CFS_DBG_NO_PRUNE) ? 1 : 0;
    fp.dbg = p->trace.p; fp.dbg_b = p->trace_b; fp.dbg_cap = p->trace_cap;
    fp.stamps = (p->stamps.p && B <= p->stamps_B) ? p->stamps.p : nullptr;
    fp.u_log = p->u_log.p;
}
static bool force_w1(const cfs_problem *p) { return (p->dbg_mask & CFS_DBG_TIER_W1) != 0; }
static bool analytic(const cfs_problem *p) { return p->jac == CFS_JAC_ANALYTIC; }
static bool limited(const cfs_problem *p) { return p->limited; }
// the soft kernels' parameters for a SOFTEN handle (null: STOP, the default kernels); whole: record viol_all / n_soft
static const SoftParams *soft_params(const cfs_problem *p, SoftParams &sp, bool whole)
{
    if (p->infeas != CFS_INFEAS_SOFTEN) return nullptr;
    sp.inv_weight = 1.0 / p->soft_weight;
    sp.viol = whole ? p->soft_viol.p : nullptr;
    sp.n_soft = whole ? p->soft_n.p : nullptr;
    return &sp;
}

int cfs_set_launch_order(cfs_problem *p, const int *order, int n)
{
    if (!p) return cfs_fail(CFS_ERR_INVALID_ARG, "NULL argument");
    if (!order) { p->order_mode = n < 0 ? 2 : 0; p->order_n = 0; return CFS_SUCCESS; }
    if (n < 1 || n > p->d.max_batch) return cfs_fail(CFS_ERR_INVALID_ARG, "n=%d outside 1..max_batch=%d", n, p->d.max_batch);
    std::vector<char> seen((size_t)n, 0);
    for (int i = 0; i < n; ++i) {
        if (order[i] < 0 || order[i] >= n || seen[order[i]]) return cfs_fail(CFS_ERR_INVALID_ARG, "order is not a permutation of 0..%d (entry %d)", n - 1, i);
        seen[order[i]] = 1;
    }
    CFS_HIPCHK(hipSetDevice(p->device));
    CFS_HIPCHK(hipDeviceSynchronize());      // a solve in flight may still be reading the previous order
    CFS_HIPCHK(hipMemcpy(p->order_user.p, order, (size_t)n * sizeof(int), hipMemcpyHostToDevice));
    p->order_mode = 1; p->order_n = n;
    return CFS_SUCCESS;
}

static int enqueue_solve(cfs_problem *p, const cfs_batch_in *in, const cfs_batch_out *out, hipStream_t s, hipEvent_t *e4);

// the launch-order pre-pass of B problems of this handle (x_init, obs: DEVICE): the line obstacles are the first nobs - nmesh of
// every row of `obs`, a per-waypoint handle has one row per waypoint; read by enqueue_solve and by cfs_debug_launch_order
static OrderParams order_params(const cfs_problem *p, int B, const double *x_init, const double *obs)
{
    OrderParams op;
    op.rb = p->rb.p; op.B = B; op.H = p->d.H; op.nj = p->d.njoint; op.nobs = p->d.nobs - p->nmesh; op.obs_stride = p->d.nobs;
    op.wp_stride = cfs_moving(p) ? p->d.nobs : 0;
    op.x_init = x_init; op.obs = obs; op.margin = p->margin.p; op.key = p->okey.p; op.order = p->order.p;
    return op;
}

// the handle's part of the mesh linearisation's parameter block (the caller sets x_, status_done and seed_prev)
static LinMeshParams lin_mesh_params(const cfs_problem *p, int B)
{
    LinMeshParams lm;
    lm.rb = p->rb.p; lm.B = B; lm.H = p->d.H; lm.nmesh = p->nmesh; lm.meshes = p->mesh.meshes_d.p;
    lm.mesh_pose = p->mm.mesh_pose.p;
    lm.dist = p->dist.p; lm.grad = p->grad.p;
    lm.ends = p->mesh.m_ends.p; lm.base_d = p->mesh.m_base.p; lm.upper_d = p->mesh.m_upper.p; lm.base_t = p->mesh.m_tri.p; lm.shift_d = p->mesh.m_shift.p;
    lm.near = p->mesh.m_near.p; lm.piece_d = p->mesh.m_pd.p; lm.piece_i = p->mesh.m_pi.p; lm.piece_nd = p->mesh.m_pnd.p;
    return lm;
}

int cfs_solve_batch_device(cfs_problem *p, const cfs_batch_in *in, const cfs_batch_out *out, void *stream)
{
    if (!p || !in || !out) return cfs_fail(CFS_ERR_INVALID_ARG, "NULL argument");
    const int B = in->B;
    if (int rc = cfs_check_batch(p, B)) return rc;
    if (!in->x_init || !in->xR1 || !in->ff || !in->caug || !in->obs) return cfs_fail(CFS_ERR_INVALID_ARG, "NULL input array");
    if (!out->u || !out->x_ || !out->cost_all || !out->e_cost_all || !out->e_u_all || !out->iter_O || !out->total_iter || !out->status)
        return cfs_fail(CFS_ERR_INVALID_ARG, "NULL output array");
    CFS_HIPCHK(hipSetDevice(p->device));
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);

    hipEvent_t e4[4] = {nullptr, nullptr, nullptr, nullptr};
    int rc = CFS_SUCCESS;
    if (p->prof)
        for (int k = 0; k < 4 && rc == CFS_SUCCESS; ++k) {
            if (!p->ev_free.empty()) { e4[k] = p->ev_free.back(); p->ev_free.pop_back(); }
            else if (hipEventCreate(&e4[k]) != hipSuccess) { e4[k] = nullptr; rc = cfs_fail(CFS_ERR_HIP, "hipEventCreate failed"); }
        }
    if (rc == CFS_SUCCESS) {
        rc = enqueue_solve(p, in, out, s, e4);
        if (rc != CFS_SUCCESS) p->pool_dirty = true;
    }
    if (p->prof)                         // recorded events are read by cfs_profile_read; after an error they go back to the pool
        for (int k = 0; k < 4; ++k)
            if (e4[k]) (rc == CFS_SUCCESS ? p->ev : p->ev_free).push_back(e4[k]);
    return rc;
}

static int enqueue_solve(cfs_problem *p, const cfs_batch_in *in, const cfs_batch_out *out, hipStream_t s, hipEvent_t *e4)
{
    const int B = in->B, nj = p->d.njoint, nn = p->nn, K = p->d.MAX_O_ITER;
    // Every workgroup gives its spill slot back on every exit path, so the flags are all clear after a solve that ran.  They are
    // cleared at creation and again after a solve whose enqueue failed half way -- not per solve: with the chip held by another
    // solve's fused workgroups even a memset node waits ~0.08 ms for a slot on this stream.
    if (p->pool_dirty) {
        CFS_HIPCHK(hipMemsetAsync(p->pool_flag.p, 0, (size_t)p->pool_n * 16 * sizeof(int), s));
        p->pool_dirty = false;
    }
    if (p->prof) CFS_HIPCHK(hipEventRecord(e4[0], s));
    if (p->d.mode == CFS_MODE_CFS) {     // unconstrained minimiser -H^{-1} ff (MFMA), constant over the outer loop
        GemvParams g;
        g.B = B; g.nn = nn; g.M = p->Hinv.p; g.X = in->ff; g.Y = p->x0.p; g.scale = -1.0;
        launch_batched_gemv(g, s);
    }
    if (p->prof) CFS_HIPCHK(hipEventRecord(e4[1], s));
    FusedParams fp;
    fill_fused_family(p, fp, B);
    fp.noise_rows = in->noise ? in->noise_rows : 0;
    fp.x_init = in->x_init; fp.xR1 = in->xR1; fp.ff = in->ff; fp.caug = in->caug; fp.obs = in->obs; fp.noise = in->noise;
    fp.u = out->u; fp.x_ = out->x_; fp.cost_all = out->cost_all; fp.e_cost_all = out->e_cost_all; fp.e_u_all = out->e_u_all;
    fp.iter_O = out->iter_O; fp.total_iter = out->total_iter; fp.status = out->status;
    fp.u_hist = (p->d.mode == CFS_MODE_CFS && K > 0) ? p->u_hist.p : nullptr;
    // Launch order.  Workgroups are dispatched in blockIdx order and a launch ends with its longest problem, so problems
    // that will run long active sets should not wait for a free compute unit behind short ones.  Automatic: a pre-pass
    // counts the clearances the initial trajectory violates (two small kernels on the same stream, ~10 us) -- only when the
    // batch cannot start all at once anyway.
    const int nline = p->d.nobs - p->nmesh;
    if (p->order_mode == 1 && p->order_n == B) fp.order = p->order_user.p;
    else if (p->order_mode != 2 && !(p->dbg_mask & CFS_DBG_NO_AUTO_ORDER) && B > p->n_cu && nline > 0) {   // also when a given order is for another batch size
        launch_order(order_params(p, B, in->x_init, in->obs), s);
        fp.order = p->order.p;
    }
    SoftParams sp;
    const SoftParams *soft = soft_params(p, sp, true);
    if (p->soft_viol.p) {                // viol_all / n_soft of this solve (zero beyond each problem's last iteration; all zero under STOP)
        CFS_HIPCHK(hipMemsetAsync(p->soft_viol.p, 0, (size_t)B * std::max(K, 1) * sizeof(double), s));
        CFS_HIPCHK(hipMemsetAsync(p->soft_n.p, 0, (size_t)B * sizeof(int), s));
    }
    if (p->prof) CFS_HIPCHK(hipEventRecord(e4[2], s));   // after the launch-order pre-pass: [e4[2], e4[3]] brackets the fused kernel alone (mesh handles: the loop of launches)
    if (p->nmesh == 0) {
        CFS_HIPCHK(launch_fused(nj, fp, s, force_w1(p), analytic(p), soft, cfs_moving(p), limited(p)));
    } else {
        // Mesh obstacles are linearised by their own kernel (hierarchy traversals do not fit the fused kernel's register
        // budget), which needs the current iterate: one outer iteration per launch, state carried through HBM.  Every
        // launch is enqueued up front; finished problems return at once, so there is still no host round trip.
        LinMeshParams lm = lin_mesh_params(p, B);
        fp.nmesh = p->nmesh; fp.ext_dist = p->dist.p; fp.ext_grad = p->grad.p; fp.max_launch_iters = 1;
        fp.st_qu = p->qu.p; fp.st_cost = p->mesh.st_cost.p; fp.st_noise = p->noise_row.p; fp.st_done = p->mesh.st_done.p;
        for (int it = 0; it < std::max(K, 1); ++it) {
            lm.x_ = it == 0 ? in->x_init : out->x_;
            lm.status_done = it == 0 ? nullptr : p->mesh.st_done.p;
            lm.seed_prev = it > 0;
            CFS_HIPCHK(launch_linearize_mesh(nj, lm, s));
            fp.resume = it > 0;
            CFS_HIPCHK(launch_fused(nj, fp, s, force_w1(p), analytic(p), nullptr, false, limited(p)));
        }
    }
    if (p->prof) CFS_HIPCHK(hipEventRecord(e4[3], s));
    if (fp.u_hist) {                     // CFS cost history: QQ * (all logged u) on the matrix cores, then the dots
        if (p->u_hist.n) {
            GemvParams g;
            g.B = B * K; g.nn = nn; g.M = p->QQ.p; g.X = p->u_hist.p; g.Y = p->qu_hist.p; g.scale = 1.0;
            launch_batched_gemv(g, s);
            CostHistParams ch;
            ch.B = B; ch.nn = nn; ch.max_o_iter = K; ch.u_hist = p->u_hist.p; ch.qu_hist = p->qu_hist.p;
            ch.ff = in->ff; ch.caug = in->caug; ch.iter_O = out->iter_O; ch.cost_all = out->cost_all; ch.e_cost_all = out->e_cost_all;
            launch_cost_history(ch, s);
        }
    }
    CFS_HIPCHK(hipGetLastError());
    return CFS_SUCCESS;
}

int cfs_solve_batch(cfs_problem *p, const cfs_batch_in *in, const cfs_batch_out *out)
{
    if (!p || !in || !out) return cfs_fail(CFS_ERR_INVALID_ARG, "NULL argument");
    const int B = in->B;
    if (int rc = cfs_check_batch(p, B)) return rc;
    if (!in->x_init || !in->xR1 || !in->ff || !in->caug || !in->obs) return cfs_fail(CFS_ERR_INVALID_ARG, "NULL input array");
    CFS_HIPCHK(hipSetDevice(p->device));
    const size_t nn = p->nn, nx = p->nx, ns = p->ns, K = p->d.MAX_O_ITER;
    Stage st;
    cfs_batch_in din = *in;
    din.x_init = st.up(in->x_init, B * nx);
    din.xR1 = st.up(in->xR1, B * ns);
    din.ff = st.up(in->ff, B * nn);
    din.caug = st.up(in->caug, B);
    din.obs = st.up(in->obs, B * cfs_obs_rows(p) * 6);
    din.noise = in->noise ? st.up(in->noise, (size_t)B * in->noise_rows * nn) : nullptr;
    cfs_batch_out dout;
    dout.u = st.out<double>(B * nn);
    dout.x_ = st.out<double>(B * nx);
    dout.cost_all = st.zeros<double>(B * K);
    dout.e_cost_all = st.zeros<double>(B * K);
    dout.e_u_all = st.zeros<double>(B * K);
    dout.iter_O = st.out<int>(B);
    dout.total_iter = st.out<int>(B);
    dout.status = st.out<int>(B);
    if (st.err != hipSuccess) return st.result("staging");
    int rc = cfs_solve_batch_device(p, &din, &dout, nullptr);
    if (rc) return rc;
    CFS_HIPCHK(hipStreamSynchronize(nullptr));
    st.down(out->u, dout.u, B * nn);
    st.down(out->x_, dout.x_, B * nx);
    st.down(out->cost_all, dout.cost_all, B * K);
    st.down(out->e_cost_all, dout.e_cost_all, B * K);
    st.down(out->e_u_all, dout.e_u_all, B * K);
    st.down(out->iter_O, dout.iter_O, B);
    st.down(out->total_iter, dout.total_iter, B);
    st.down(out->status, dout.status, B);
    return st.result("copy back");
}

// ---- EVAL.get_Cost_b (Lib/EVAL.m:75-78; main_FANUC.m:131-132) ----------------------------------------------------------
// u_b = quadprog(Qaug, paug) with no constraints = -H^{-1} ff (H = QQ symmetrised, as quadprog does), cost = get_cost(u_b):
// two products on the matrix cores (the first is the one every CFS solve starts with) and one dot per problem.
int cfs_cost_b(cfs_problem *p, int B, const double *ff, const double *caug, double *cost_b, double *u_b)
{
    if (!p || !ff || !caug || !cost_b) return cfs_fail(CFS_ERR_INVALID_ARG, "NULL argument");
    if (int rc = cfs_check_batch(p, B)) return rc;
    CFS_HIPCHK(hipSetDevice(p->device));
    const size_t nn = p->nn;
    Stage st;
    const double *d_ff = st.up(ff, B * nn), *d_caug = st.up(caug, (size_t)B);
    double *d_cost = st.out<double>((size_t)B);
    if (st.err != hipSuccess) return st.result("staging");
    GemvParams g;
    g.B = B; g.nn = (int)nn; g.M = p->Hinv.p; g.X = d_ff; g.Y = p->x0.p; g.scale = -1.0;
    launch_batched_gemv(g, nullptr);
    g.M = p->QQ.p; g.X = p->x0.p; g.Y = p->qu.p; g.scale = 1.0;
    launch_batched_gemv(g, nullptr);
    CostHistParams ch;
    memset(&ch, 0, sizeof ch);
    ch.B = B; ch.nn = (int)nn; ch.max_o_iter = 1; ch.u_hist = p->x0.p; ch.qu_hist = p->qu.p; ch.ff = d_ff; ch.caug = d_caug;
    ch.iter_O = nullptr; ch.cost_all = d_cost; ch.e_cost_all = nullptr;      // iter_O == NULL: one logged iterate per problem
    launch_cost_history(ch, nullptr);
    CFS_HIPCHK(hipGetLastError());
    CFS_HIPCHK(hipStreamSynchronize(nullptr));
    st.down(cost_b, d_cost, (size_t)B);
    if (u_b) st.down(u_b, p->x0.p, B * nn);
    return st.result("copy back");
}

// cost = self.eval.get_cost(u) (Lib/EVAL.m:51-53) for B given u: QQ*u on the matrix cores, one dot per problem
int cfs_get_cost(cfs_problem *p, int B, const double *u, const double *ff, const double *caug, double *cost)
{
    if (!p || !u || !ff || !caug || !cost) return cfs_fail(CFS_ERR_INVALID_ARG, "NULL argument");
    if (int rc = cfs_check_batch(p, B)) return rc;
    CFS_HIPCHK(hipSetDevice(p->device));
    const size_t nn = p->nn;
    Stage st;
    const double *d_u = st.up(u, B * nn), *d_ff = st.up(ff, B * nn), *d_caug = st.up(caug, (size_t)B);
    double *d_cost = st.out<double>((size_t)B);
    if (st.err != hipSuccess) return st.result("staging");
    GemvParams g;
    g.B = B; g.nn = (int)nn; g.M = p->QQ.p; g.X = d_u; g.Y = p->qu.p; g.scale = 1.0;
    launch_batched_gemv(g, nullptr);
    CostHistParams ch;
    memset(&ch, 0, sizeof ch);
    ch.B = B; ch.nn = (int)nn; ch.max_o_iter = 1; ch.u_hist = d_u; ch.qu_hist = p->qu.p; ch.ff = d_ff; ch.caug = d_caug; ch.cost_all = d_cost;
    launch_cost_history(ch, nullptr);
    CFS_HIPCHK(hipGetLastError());
    CFS_HIPCHK(hipStreamSynchronize(nullptr));
    st.down(cost, d_cost, (size_t)B);
    return st.result("copy back");
}

// ---- developer / test entry points (declared in include/cfs_hip.h; per handle) --------------------------------------------
int cfs_debug_set_options(cfs_problem *p, int mask, int warm_max, double polish_tol)
{
    if (!p) return cfs_fail(CFS_ERR_INVALID_ARG, "NULL handle");
    const int known = CFS_DBG_NO_REFINE | CFS_DBG_NO_WARM_START | CFS_DBG_NO_CERTIFICATE | CFS_DBG_NO_PRUNE | CFS_DBG_NO_AUTO_ORDER |
                      CFS_DBG_TIER_W1 | CFS_DBG_CLEAR_NO_BOUND | CFS_DBG_CLEAR_SEED;
    if (mask & ~known) return cfs_fail(CFS_ERR_INVALID_ARG, "unknown option bits 0x%x", mask & ~known);
    if (warm_max < 0 || warm_max > 64) return cfs_fail(CFS_ERR_INVALID_ARG, "warm_max %d outside 0..64", warm_max);
    p->dbg_mask = mask; p->dbg_warm_max = warm_max;
    p->dbg_polish_tol = polish_tol > 0.0 ? polish_tol : 1e-11;
    return CFS_SUCCESS;
}

int cfs_debug_fused_tier(int njoint, int H, int nobs, int mode, int per_waypoint, int limits, int force_w1, int *tier)
{
    if (!tier) return cfs_fail(CFS_ERR_INVALID_ARG, "NULL argument");
    if (njoint < 2 || njoint > 6) return cfs_fail(CFS_ERR_INVALID_ARG, "njoint %d unsupported (2..6)", njoint);
    if (H < 1 || H > CFS_MAX_H) return cfs_fail(CFS_ERR_INVALID_ARG, "H %d outside 1..%d", H, CFS_MAX_H);
    if (nobs < 1 || nobs > CFS_MAX_OBS) return cfs_fail(CFS_ERR_INVALID_ARG, "nobs %d outside 1..%d", nobs, CFS_MAX_OBS);
    if (mode != CFS_MODE_CFS && mode != CFS_MODE_PSGCFS) return cfs_fail(CFS_ERR_INVALID_ARG, "unknown mode %d", mode);
    if (!fused_fits(njoint, H, nobs))
        return cfs_fail(CFS_ERR_INVALID_ARG, "H=%d x nobs=%d x njoint=%d exceeds the 160 KB on-chip budget of one problem", H, nobs, njoint);
    // the admission rules of cfs_problem_set_obstacle_motion and cfs_problem_set_joint_limits, in either order of the two calls
    if (per_waypoint && !fused_keeps_tier(njoint, H, nobs, mode, true, limits != 0))
        return cfs_fail(CFS_ERR_INVALID_ARG, "per-waypoint obstacles: H=%d x nobs=%d x njoint=%d exceeds the on-chip budget of this shape's tier", H, nobs, njoint);
    if (limits && !fused_keeps_tier(njoint, H, nobs, mode, per_waypoint != 0, true))
        return cfs_fail(CFS_ERR_INVALID_ARG, "joint limits: H=%d x nobs=%d x njoint=%d exceeds the on-chip budget of this shape's tier", H, nobs, njoint);
    *tier = (int)fused_tier(njoint, H, nobs, mode, force_w1 != 0);
    return CFS_SUCCESS;
}

int cfs_debug_stamps(cfs_problem *p, int B, unsigned long long *out)
{
    if (!p) return cfs_fail(CFS_ERR_INVALID_ARG, "NULL handle");
    CFS_HIPCHK(hipSetDevice(p->device));
    if (out) {
        if (!p->stamps.p) return cfs_fail(CFS_ERR_INVALID_ARG, "stamps are not enabled");
        CFS_HIPCHK(hipDeviceSynchronize());
        CFS_HIPCHK(hipMemcpy(out, p->stamps.p, (size_t)p->stamps_B * 12 * 8, hipMemcpyDeviceToHost));
        return CFS_SUCCESS;
    }
    CFS_HIPCHK(hipDeviceSynchronize());
    p->stamps.release(); p->stamps_B = 0;
    if (B <= 0) return CFS_SUCCESS;
    if (B > p->d.max_batch) return cfs_fail(CFS_ERR_INVALID_ARG, "B=%d exceeds max_batch=%d", B, p->d.max_batch);
    CFS_HIPCHK(p->stamps.zeros((size_t)B * 12));
    p->stamps_B = B;
    return CFS_SUCCESS;
}

int cfs_debug_trace_begin(cfs_problem *p, int b, int cap)
{
    if (!p) return cfs_fail(CFS_ERR_INVALID_ARG, "NULL handle");
    CFS_HIPCHK(hipSetDevice(p->device));
    CFS_HIPCHK(hipDeviceSynchronize());
    p->trace.release(); p->trace_b = -1; p->trace_cap = 0;
    if (cap <= 0) return CFS_SUCCESS;
    CFS_HIPCHK(p->trace.zeros((size_t)(cap + 1) * 8));
    p->trace_b = b; p->trace_cap = cap;
    return CFS_SUCCESS;
}

int cfs_debug_trace_read(cfs_problem *p, double *out)
{
    if (!p || !out) return cfs_fail(CFS_ERR_INVALID_ARG, "NULL argument");
    if (!p->trace.p) return cfs_fail(CFS_ERR_INVALID_ARG, "no trace was begun");
    CFS_HIPCHK(hipSetDevice(p->device));
    CFS_HIPCHK(hipDeviceSynchronize());
    CFS_HIPCHK(hipMemcpy(out, p->trace.p, (size_t)(p->trace_cap + 1) * 8 * sizeof(double), hipMemcpyDeviceToHost));
    return CFS_SUCCESS;
}

int cfs_debug_launch_order(cfs_problem *p, int B, const double *x_init, const double *obs, int *key, int *order)
{
    if (!p || !x_init || !obs || (!key && !order)) return cfs_fail(CFS_ERR_INVALID_ARG, "NULL argument");
    if (int rc = cfs_check_batch(p, B)) return rc;
    if (p->d.nobs - p->nmesh == 0) {         // no line obstacle: nothing to count, and a solve launches no pre-pass
        for (int b = 0; b < B; ++b) {
            if (key) key[b] = 0;
            if (order) order[b] = b;
        }
        return CFS_SUCCESS;
    }
    CFS_HIPCHK(hipSetDevice(p->device));
    CFS_HIPCHK(hipDeviceSynchronize());      // a solve in flight may still be reading okey / order
    Stage st;
    const double *d_x = st.up(x_init, (size_t)B * p->nx), *d_obs = st.up(obs, (size_t)B * cfs_obs_rows(p) * 6);
    if (st.err != hipSuccess) return st.result("staging");
    launch_order(order_params(p, B, d_x, d_obs), nullptr);
    CFS_HIPCHK(hipGetLastError());
    CFS_HIPCHK(hipStreamSynchronize(nullptr));
    st.down(key, p->okey.p, (size_t)B); st.down(order, p->order.p, (size_t)B);
    return st.result("copy back");
}

int cfs_debug_log_u(cfs_problem *p, int on)
{
    if (!p) return cfs_fail(CFS_ERR_INVALID_ARG, "NULL handle");
    CFS_HIPCHK(hipSetDevice(p->device));
    CFS_HIPCHK(hipDeviceSynchronize());
    p->u_log.release();
    if (!on || p->d.MAX_O_ITER < 1) return CFS_SUCCESS;
    const size_t n = (size_t)p->d.max_batch * p->d.MAX_O_ITER * p->nn;
    CFS_HIPCHK(p->u_log.zeros(n));
    return CFS_SUCCESS;
}

int cfs_debug_read_u_log(cfs_problem *p, int B, double *out)
{
    if (!p || !out) return cfs_fail(CFS_ERR_INVALID_ARG, "NULL argument");
    if (!p->u_log.p) return cfs_fail(CFS_ERR_INVALID_ARG, "the u log is not enabled");
    if (int rc = cfs_check_batch(p, B)) return rc;
    CFS_HIPCHK(hipSetDevice(p->device));
    CFS_HIPCHK(hipDeviceSynchronize());
    CFS_HIPCHK(hipMemcpy(out, p->u_log.p, (size_t)B * p->d.MAX_O_ITER * p->nn * sizeof(double), hipMemcpyDeviceToHost));
    return CFS_SUCCESS;
}

int cfs_set_state_cost(cfs_problem *p, const double *Qaug)
{
    if (!p || !Qaug) return cfs_fail(CFS_ERR_INVALID_ARG, "NULL argument");
    CFS_HIPCHK(hipSetDevice(p->device));
    std::vector<double> F1, F2, Cq;
    state_cost_terms(p->d.njoint, p->d.H, p->d.robot.delta_t, Qaug, F1, F2, Cq);
    CFS_HIPCHK(p->F1.upload(F1.data(), F1.size())); CFS_HIPCHK(p->F2.upload(F2.data(), F2.size())); CFS_HIPCHK(p->Cq.upload(Cq.data(), Cq.size()));
    return CFS_SUCCESS;
}

// x0 / xg (route == NULL), or routes of nwp rows (nwp_b == NULL), or ragged routes (nwp_b[b] of nwp_stride rows each)
static int build_terms(cfs_problem *p, int B, const double *x0, const double *xg, const double *route, int nwp, const int *nwp_b, int nwp_stride,
                       double *x_init, double *xR1, double *ff, double *caug, void *stream)
{
    if (!p->F1.p) return cfs_fail(CFS_ERR_INVALID_ARG, "call cfs_set_state_cost first");
    CFS_HIPCHK(hipSetDevice(p->device));
    TermsParams t;
    t.B = B; t.H = p->d.H; t.nj = p->d.njoint; t.F1 = p->F1.p; t.F2 = p->F2.p; t.Cq = p->Cq.p;
    t.x0 = x0; t.xg = xg; t.route = route; t.nwp = nwp; t.nwp_b = nwp_b; t.nwp_stride = nwp_stride; t.dt = p->d.robot.delta_t;
    t.x_init = x_init; t.xR1 = xR1; t.ff = ff; t.caug = caug;
    launch_build_terms(t, reinterpret_cast<hipStream_t>(stream));
    CFS_HIPCHK(hipGetLastError());
    return CFS_SUCCESS;
}

int cfs_build_terms_device(cfs_problem *p, int B, const double *x0, const double *xg,
                           double *x_init, double *xR1, double *ff, double *caug, void *stream)
{
    if (!p || !x0 || !xg || !x_init || !xR1 || !ff || !caug) return cfs_fail(CFS_ERR_INVALID_ARG, "NULL argument");
    if (B < 1) return cfs_fail(CFS_ERR_INVALID_ARG, "B must be >= 1");
    return build_terms(p, B, x0, xg, nullptr, 0, nullptr, 0, x_init, xR1, ff, caug, stream);
}

int cfs_build_terms_from_routes_device(cfs_problem *p, int B, const double *routes, int nwp,
                                       double *x_init, double *xR1, double *ff, double *caug, void *stream)
{
    if (!p || !routes || !x_init || !xR1 || !ff || !caug) return cfs_fail(CFS_ERR_INVALID_ARG, "NULL argument");
    if (B < 1 || nwp < 2) return cfs_fail(CFS_ERR_INVALID_ARG, "B >= 1 and at least two route waypoints are needed");
    return build_terms(p, B, nullptr, nullptr, routes, nwp, nullptr, 0, x_init, xR1, ff, caug, stream);
}

int cfs_build_terms_from_ragged_routes_device(cfs_problem *p, int B, const double *routes, int nwp_stride, const int *nwp,
                                              double *x_init, double *xR1, double *ff, double *caug, void *stream)
{
    if (!p || !routes || !nwp || !x_init || !xR1 || !ff || !caug) return cfs_fail(CFS_ERR_INVALID_ARG, "NULL argument");
    if (B < 1 || nwp_stride < 1) return cfs_fail(CFS_ERR_INVALID_ARG, "B >= 1 and nwp_stride >= 1 are needed");
    return build_terms(p, B, nullptr, nullptr, routes, nwp_stride, nwp, nwp_stride, x_init, xR1, ff, caug, stream);
}

int cfs_chomp_batch(cfs_problem *p, const cfs_batch_in *in, const double *u0, const double *D, const double *epsilon,
                    const cfs_batch_out *out)
{
    if (!p || !in || !out || !u0 || !D || !epsilon) return cfs_fail(CFS_ERR_INVALID_ARG, "NULL argument");
    const int B = in->B;
    if (int rc = cfs_check_batch(p, B)) return rc;
    if (!in->x_init || !in->xR1 || !in->ff || !in->caug || !in->obs) return cfs_fail(CFS_ERR_INVALID_ARG, "NULL input array");
    if (!out->u || !out->x_ || !out->cost_all || !out->e_cost_all || !out->e_u_all || !out->iter_O) return cfs_fail(CFS_ERR_INVALID_ARG, "NULL output array");
    if (p->nmesh > 0) return cfs_fail(CFS_ERR_INVALID_ARG, "CHOMP_FANUC measures line obstacles only (Lib/CHOMP_FANUC.m:119)");
    if (cfs_moving(p)) return cfs_fail(CFS_ERR_INVALID_ARG, "CHOMP_FANUC takes static obstacles only (the handle is CFS_OBS_PER_WAYPOINT)");
    if (limited(p)) return cfs_fail(CFS_ERR_INVALID_ARG, "CHOMP_FANUC has no QP to hold joint limits (the handle has them: clear them first)");
    if (!chomp_fits(p->d.njoint, p->d.H, p->d.nobs)) return cfs_fail(CFS_ERR_INVALID_ARG, "H x nobs too large for the CHOMP kernel's 64 KB of LDS");
    CFS_HIPCHK(hipSetDevice(p->device));
    const size_t nn = p->nn, nx = p->nx, ns = p->ns, K = p->d.MAX_O_ITER, nobs = p->d.nobs;
    Stage st;
    ChompParams c;
    memset(&c, 0, sizeof c);
    c.rb = p->rb.p; c.B = B; c.H = p->d.H; c.nobs = p->d.nobs; c.max_o_iter = p->d.MAX_O_ITER;
    c.dt = p->d.robot.delta_t; c.alpha = p->d.alpha; c.epsilon_O = p->d.epsilon_O; c.QQ = p->QQ.p;
    c.x_init = st.up(in->x_init, B * nx); c.xR1 = st.up(in->xR1, B * ns); c.ff = st.up(in->ff, B * nn); c.caug = st.up(in->caug, B);
    c.obs = st.up(in->obs, B * nobs * 6); c.u0 = st.up(u0, B * nn); c.D = st.up(D, nobs); c.eps = st.up(epsilon, nobs);
    c.u = st.out<double>(B * nn); c.x_ = st.out<double>(B * nx);
    const size_t nlog = B * std::max<size_t>(K, 1);
    c.cost_all = st.zeros<double>(nlog); c.e_cost_all = st.zeros<double>(nlog); c.e_u_all = st.zeros<double>(nlog);
    c.iter_O = st.out<int>(B); c.total_iter = st.out<int>(B); c.status = st.out<int>(B);
    if (st.err != hipSuccess) return st.result("staging");
    chomp_derivest_tables(c);
    CFS_HIPCHK(launch_chomp(p->d.njoint, c, nullptr));
    CFS_HIPCHK(hipStreamSynchronize(nullptr));
    st.down(out->u, c.u, B * nn); st.down(out->x_, c.x_, B * nx);
    st.down(out->cost_all, c.cost_all, B * K); st.down(out->e_cost_all, c.e_cost_all, B * K); st.down(out->e_u_all, c.e_u_all, B * K);
    st.down(out->iter_O, c.iter_O, B); st.down(out->total_iter, c.total_iter, B); st.down(out->status, c.status, B);
    return st.result("copy back");
}

int cfs_problem_set_meshes(cfs_problem *p, int nmesh, const cfs_mesh *const *meshes)
{
    if (!p) return cfs_fail(CFS_ERR_INVALID_ARG, "NULL handle");
    if (nmesh < 0 || nmesh > p->d.nobs) return cfs_fail(CFS_ERR_INVALID_ARG, "nmesh %d outside 0..nobs=%d", nmesh, p->d.nobs);
    if (nmesh > 0 && !meshes) return cfs_fail(CFS_ERR_INVALID_ARG, "meshes is NULL");
    if (nmesh > 0 && p->infeas == CFS_INFEAS_SOFTEN) return cfs_fail(CFS_ERR_INVALID_ARG, "mesh obstacles are not supported with CFS_INFEAS_SOFTEN");
    if (nmesh > 0 && cfs_moving(p)) return cfs_fail(CFS_ERR_INVALID_ARG, "mesh obstacles are static: not supported on a CFS_OBS_PER_WAYPOINT handle");
    CFS_HIPCHK(hipSetDevice(p->device));
    std::vector<DevMesh> v(nmesh);
    for (int i = 0; i < nmesh; ++i) {
        if (!meshes[i]) return cfs_fail(CFS_ERR_INVALID_ARG, "meshes[%d] is NULL", i);
        if (meshes[i]->device != p->device) return cfs_fail(CFS_ERR_INVALID_ARG, "meshes[%d] lives on device %d, the problem on %d", i, meshes[i]->device, p->device);
        v[i] = meshes[i]->view();
    }
    p->mesh = MeshSet{}; p->reset_mesh_motion(); p->cm = ClearMeshWork{};   // the old set goes before the new one is allocated; the meshes are static again
    p->nmesh = 0;
    if (nmesh > 0) {
        size_t we, wb, ws, wn, wpd, wpi, wpn;
        linearize_mesh_workspace(p->d.njoint, nmesh, &we, &wb, &ws, &wn, &wpd, &wpi, &wpn);
        const size_t bh = (size_t)p->d.max_batch * p->d.H;
        CFS_HIPCHK(p->mesh.m_ends.alloc(bh * we)); CFS_HIPCHK(p->mesh.m_base.alloc(bh * wb)); CFS_HIPCHK(p->mesh.m_upper.alloc(bh * wb)); CFS_HIPCHK(p->mesh.m_tri.alloc(bh * wb)); CFS_HIPCHK(p->mesh.m_shift.alloc(bh * ws)); CFS_HIPCHK(p->mesh.m_near.alloc(bh * wn));
        CFS_HIPCHK(p->mesh.m_pd.alloc(bh * wpd)); CFS_HIPCHK(p->mesh.m_pi.alloc(bh * wpi)); CFS_HIPCHK(p->mesh.m_pnd.alloc(bh * wpn));
        CFS_HIPCHK(p->mesh.st_cost.alloc(2 * (size_t)p->d.max_batch));
        CFS_HIPCHK(p->mesh.st_done.alloc(p->d.max_batch));
        CFS_HIPCHK(p->mesh.meshes_d.upload(v.data(), nmesh));
        p->mesh.meshes_h = v;
        p->nmesh = nmesh;
    }
    return CFS_SUCCESS;
}

int cfs_problem_set_mesh_motion(cfs_problem *p, const double *poses)
{
    if (!p) return cfs_fail(CFS_ERR_INVALID_ARG, "NULL handle");
    if (p->nmesh < 1) return cfs_fail(CFS_ERR_INVALID_ARG, "mesh motion needs a handle with mesh obstacles (cfs_problem_set_meshes)");
    CFS_HIPCHK(hipSetDevice(p->device));
    if (!poses) {
        CFS_HIPCHK(hipDeviceSynchronize());  // a solve in flight may still be reading the poses
        p->reset_mesh_motion();
        return CFS_SUCCESS;
    }
    // [R | t] -> [R' | -R't]; only rigid motions are admitted (cfs_family.cpp)
    const size_t n = (size_t)p->nmesh * p->d.H;
    std::vector<double> inv;
    if (FamilyRefusal r = invert_mesh_poses(p->nmesh, p->d.H, poses, inv)) return cfs_fail(r.code, "%s", r.text);
    CFS_HIPCHK(hipDeviceSynchronize());
    // what the audit between the waypoints needs per (mesh, interval) (cfs_clearance_mesh_motion, cfs_family.h CLEAR_ITV)
    std::vector<double> itv(n * CLEAR_ITV, 0.0);
    int turn_mesh = -1, turn_wp = 0;
    if (p->mesh.mesh_frame.empty()) {             // c_j and r_j of the stored vertices, once per cfs_problem_set_meshes
        std::vector<double> frame(4 * (size_t)p->nmesh);
        for (int jm = 0; jm < p->nmesh; ++jm) {
            const DevMesh &m = p->mesh.meshes_h[jm];
            std::vector<double> tri(9 * (size_t)m.nt);
            CFS_HIPCHK(hipMemcpy(tri.data(), m.tri, tri.size() * sizeof(double), hipMemcpyDeviceToHost));
            mesh_frame(tri.data(), m.nt, frame.data() + 4 * jm);
        }
        p->mesh.mesh_frame = frame;
    }
    for (int jm = 0; jm < p->nmesh; ++jm)
        mesh_motion_intervals(poses + (size_t)jm * p->d.H * 12, p->d.H, p->d.robot.delta_t, p->mesh.mesh_frame.data() + 4 * jm,
                              itv.data() + (size_t)jm * p->d.H * CLEAR_ITV, jm, turn_mesh, turn_wp);
    if (!p->mm.mesh_pose.p) {
        hipError_t e = p->mm.mesh_pose.alloc(n * 12);
        if (e == hipSuccess) e = p->mm.mesh_itv.alloc(n * CLEAR_ITV);
        if (e != hipSuccess) { p->reset_mesh_motion(); return cfs_fail(CFS_ERR_HIP, "mesh poses: %s", hipGetErrorString(e)); }
    }
    CFS_HIPCHK(hipMemcpy(p->mm.mesh_pose.p, inv.data(), n * 12 * sizeof(double), hipMemcpyHostToDevice));
    CFS_HIPCHK(hipMemcpy(p->mm.mesh_itv.p, itv.data(), itv.size() * sizeof(double), hipMemcpyHostToDevice));
    p->mm.turn_mesh = turn_mesh; p->mm.turn_wp = turn_wp;
    ++p->motion_gen;                         // the audit's pose table belongs to the poses before
    return CFS_SUCCESS;
}

int cfs_profile_enable(cfs_problem *p, int on)
{
    if (!p) return cfs_fail(CFS_ERR_INVALID_ARG, "NULL handle");
    p->prof = on != 0;
    return CFS_SUCCESS;
}

int cfs_profile_read(cfs_problem *p, double *solve_kernel_ms, double *gemm_kernel_ms, int *solves)
{
    if (!p) return cfs_fail(CFS_ERR_INVALID_ARG, "NULL handle");
    CFS_HIPCHK(hipSetDevice(p->device));
    double fused = 0.0, gemm = 0.0;
    const int n = (int)(p->ev.size() / 4);
    for (int k = 0; k < n; ++k) {
        float ms = 0.f;
        CFS_HIPCHK(hipEventSynchronize(p->ev[4 * k + 3]));
        CFS_HIPCHK(hipEventElapsedTime(&ms, p->ev[4 * k + 0], p->ev[4 * k + 1]));
        gemm += ms;
        CFS_HIPCHK(hipEventElapsedTime(&ms, p->ev[4 * k + 2], p->ev[4 * k + 3]));
        fused += ms;
    }
    for (hipEvent_t e : p->ev) p->ev_free.push_back(e);
    p->ev.clear();
    if (solve_kernel_ms) *solve_kernel_ms = fused;
    if (gemm_kernel_ms) *gemm_kernel_ms = gemm;
    if (solves) *solves = n;
    return CFS_SUCCESS;
}

int cfs_problem_set_jacobian(cfs_problem *p, int mode)
{
    if (!p) return cfs_fail(CFS_ERR_INVALID_ARG, "NULL handle");
    if (mode != CFS_JAC_FD_LITERAL && mode != CFS_JAC_ANALYTIC) return cfs_fail(CFS_ERR_INVALID_ARG, "unknown jacobian mode %d", mode);
    p->jac = mode;
    return CFS_SUCCESS;
}

int cfs_problem_get_jacobian(const cfs_problem *p, int *mode)
{
    if (!p || !mode) return cfs_fail(CFS_ERR_INVALID_ARG, "NULL argument");
    *mode = p->jac;
    return CFS_SUCCESS;
}

int cfs_problem_set_infeasible_policy(cfs_problem *p, int policy, double weight)
{
    if (!p) return cfs_fail(CFS_ERR_INVALID_ARG, "NULL handle");
    if (policy != CFS_INFEAS_STOP && policy != CFS_INFEAS_SOFTEN) return cfs_fail(CFS_ERR_INVALID_ARG, "unknown infeasible-QP policy %d", policy);
    if (!std::isfinite(weight) || !(weight > 0.0)) return cfs_fail(CFS_ERR_INVALID_ARG, "soft weight %g is not finite and > 0", weight);
    if (policy == CFS_INFEAS_SOFTEN && p->nmesh > 0) return cfs_fail(CFS_ERR_INVALID_ARG, "mesh obstacles are not supported with CFS_INFEAS_SOFTEN");
    if (policy == CFS_INFEAS_SOFTEN && !p->soft_viol.p) {   // handle-owned result buffers, from the first SOFTEN on
        CFS_HIPCHK(hipSetDevice(p->device));
        const size_t nv = (size_t)p->d.max_batch * std::max(p->d.MAX_O_ITER, 1);
        hipError_t e = p->soft_viol.zeros(nv);
        if (e == hipSuccess) e = p->soft_n.zeros(p->d.max_batch);
        if (e != hipSuccess) { p->soft_viol.release(); p->soft_n.release(); return cfs_fail(CFS_ERR_HIP, "soft result buffers: %s", hipGetErrorString(e)); }
    }
    p->soft_weight = weight;
    p->infeas = policy;
    return CFS_SUCCESS;
}

int cfs_problem_set_obstacle_motion(cfs_problem *p, int motion)
{
    if (!p) return cfs_fail(CFS_ERR_INVALID_ARG, "NULL handle");
    if (motion != CFS_OBS_STATIC && motion != CFS_OBS_PER_WAYPOINT) return cfs_fail(CFS_ERR_INVALID_ARG, "unknown obstacle motion %d", motion);
    if (motion == CFS_OBS_PER_WAYPOINT) {
        if (p->nmesh > 0) return cfs_fail(CFS_ERR_INVALID_ARG, "mesh obstacles are static: CFS_OBS_PER_WAYPOINT needs a handle without meshes");
        if (!fused_keeps_tier(p->d.njoint, p->d.H, p->d.nobs, p->d.mode, true, limited(p)))
            return cfs_fail(CFS_ERR_INVALID_ARG, "H=%d x nobs=%d x njoint=%d: the per-waypoint obstacle rows of a linearisation tile do not fit the "
                        "on-chip budget of the static plan's tier", p->d.H, p->d.nobs, p->d.njoint);
    }
    p->motion = motion;
    return CFS_SUCCESS;
}

int cfs_problem_set_joint_limits(cfs_problem *p, const double *lo, const double *hi)
{
    if (!p) return cfs_fail(CFS_ERR_INVALID_ARG, "NULL handle");
    if (!lo && !hi) { p->limited = false; p->jlim.clear(); return CFS_SUCCESS; }
    if (!lo || !hi) return cfs_fail(CFS_ERR_INVALID_ARG, "lo and hi are both given or both NULL");
    const int nj = p->d.njoint;
    for (int c = 0; c < nj; ++c) {
        if (std::isnan(lo[c]) || std::isnan(hi[c])) return cfs_fail(CFS_ERR_INVALID_ARG, "joint %d: NaN limit", c);
        if (!(lo[c] < hi[c])) return cfs_fail(CFS_ERR_INVALID_ARG, "joint %d: lo %g >= hi %g", c, lo[c], hi[c]);
    }
    if (!fused_keeps_tier(nj, p->d.H, p->d.nobs, p->d.mode, cfs_moving(p), true))
        return cfs_fail(CFS_ERR_INVALID_ARG, "H=%d x nobs=%d x njoint=%d: the LDS plan with joint limits does not fit every tier of the fused solver "
                    "that the plan without them fits", p->d.H, p->d.nobs, nj);
    std::vector<double> v(lo, lo + nj);
    v.insert(v.end(), hi, hi + nj);
    CFS_HIPCHK(hipSetDevice(p->device));
    CFS_HIPCHK(hipDeviceSynchronize());      // a solve in flight may still be reading the previous limits
    CFS_HIPCHK(hipMemcpy(p->lim.p + nj, v.data(), 2 * (size_t)nj * sizeof(double), hipMemcpyHostToDevice));
    p->jlim = v;
    p->limited = true;
    return CFS_SUCCESS;
}

int cfs_problem_get_joint_limits(const cfs_problem *p, int *on, double *lo, double *hi)
{
    if (!p || !on) return cfs_fail(CFS_ERR_INVALID_ARG, "NULL argument");
    const int nj = p->d.njoint;
    *on = p->limited ? 1 : 0;
    for (int c = 0; c < nj; ++c) {
        if (lo) lo[c] = p->limited ? p->jlim[c] : -INFINITY;
        if (hi) hi[c] = p->limited ? p->jlim[nj + c] : INFINITY;
    }
    return CFS_SUCCESS;
}

int cfs_problem_get_obstacle_motion(const cfs_problem *p, int *motion)
{
    if (!p || !motion) return cfs_fail(CFS_ERR_INVALID_ARG, "NULL argument");
    *motion = p->motion;
    return CFS_SUCCESS;
}

int cfs_problem_get_infeasible_policy(const cfs_problem *p, int *policy, double *weight)
{
    if (!p || !policy || !weight) return cfs_fail(CFS_ERR_INVALID_ARG, "NULL argument");
    *policy = p->infeas;
    *weight = p->soft_weight;
    return CFS_SUCCESS;
}

int cfs_soft_results(cfs_problem *p, int B, double *viol_all, int *n_soft)
{
    if (!p) return cfs_fail(CFS_ERR_INVALID_ARG, "NULL handle");
    if (int rc = cfs_check_batch(p, B)) return rc;
    const size_t nv = (size_t)B * p->d.MAX_O_ITER;
    if (!p->soft_viol.p) {               // never softened: nothing was
        if (viol_all) memset(viol_all, 0, nv * sizeof(double));
        if (n_soft) memset(n_soft, 0, (size_t)B * sizeof(int));
        return CFS_SUCCESS;
    }
    CFS_HIPCHK(hipSetDevice(p->device));
    CFS_HIPCHK(hipDeviceSynchronize());      // the last solve may have been enqueued on any stream
    if (viol_all && nv) CFS_HIPCHK(hipMemcpy(viol_all, p->soft_viol.p, nv * sizeof(double), hipMemcpyDeviceToHost));
    if (n_soft) CFS_HIPCHK(hipMemcpy(n_soft, p->soft_n.p, (size_t)B * sizeof(int), hipMemcpyDeviceToHost));
    return CFS_SUCCESS;
}

// The pieces below run the SAME kernel as the whole solve (cfs_solve_fused_kernel, FusedParams::piece), so that the
// kernel-level parity tests certify the code that is benchmarked.

// stage what the fused kernel's constructor reads; arrays the piece does not use are zero-filled
struct PieceBuffers {
    double *x_, *xR1, *ff, *caug, *obs;
};
static int stage_piece(cfs_problem *p, Stage &st, int B, const double *x_, const double *xR1, const double *obs, PieceBuffers &pb)
{
    auto in = [&](const double *h, size_t n) { return h ? st.up(h, n) : st.zeros<double>(n); };
    pb.x_ = in(x_, (size_t)B * p->nx);
    pb.xR1 = in(xR1, (size_t)B * p->ns);
    pb.ff = st.zeros<double>((size_t)B * p->nn);
    pb.caug = st.zeros<double>((size_t)B);
    pb.obs = in(obs, (size_t)B * cfs_obs_rows(p) * 6);
    return st.result("staging");
}

// linearisation of B trajectories into p->dist / p->grad (B x nobs x H [x nj]) and, optionally, linkid
static int linearize_piece(cfs_problem *p, int B, const PieceBuffers &pb, double *d_dist, double *d_grad, int *d_linkid)
{
    const int nj = p->d.njoint;
    FusedParams fp;
    fill_fused_family(p, fp, B);
    fp.x_init = pb.x_; fp.xR1 = pb.xR1; fp.ff = pb.ff; fp.caug = pb.caug; fp.obs = pb.obs;
    fp.piece = 1;
    fp.dump_dist = d_dist; fp.dump_grad = d_grad; fp.dump_linkid = d_linkid;
    if (d_linkid) CFS_HIPCHK(hipMemsetAsync(d_linkid, 0, (size_t)B * p->d.nobs * p->d.H * sizeof(int), nullptr));
    if (p->nmesh > 0) {          // rows of the mesh obstacles come from the hierarchy kernels, as in the whole solve
        LinMeshParams lm = lin_mesh_params(p, B);
        lm.x_ = pb.x_; lm.status_done = nullptr; lm.seed_prev = 0;
        CFS_HIPCHK(launch_linearize_mesh(nj, lm, nullptr));
        fp.nmesh = p->nmesh; fp.ext_dist = p->dist.p; fp.ext_grad = p->grad.p;
    }
    SoftParams sp;
    CFS_HIPCHK(launch_fused(nj, fp, nullptr, force_w1(p), analytic(p), soft_params(p, sp, false), cfs_moving(p), limited(p)));
    return CFS_SUCCESS;
}

int cfs_linearize(cfs_problem *p, int B, const double *x_, const double *obs, double *dist, int *linkid, double *grad)
{
    int rc = cfs_check_batch(p, B);
    if (rc) return rc;
    if (!x_ || !obs || !dist || !grad) return cfs_fail(CFS_ERR_INVALID_ARG, "NULL array");
    CFS_HIPCHK(hipSetDevice(p->device));
    const size_t nobs = p->d.nobs, H = p->d.H, nj = p->d.njoint;
    Stage st;
    PieceBuffers pb;
    rc = stage_piece(p, st, B, x_, nullptr, obs, pb);
    if (rc) return rc;
    double *d_dist = st.out<double>((size_t)B * nobs * H);
    double *d_grad = st.out<double>((size_t)B * nobs * H * nj);
    if (st.err != hipSuccess) return st.result("staging");
    rc = linearize_piece(p, B, pb, d_dist, d_grad, p->linkid.p);
    if (rc) return rc;
    CFS_HIPCHK(hipStreamSynchronize(nullptr));
    st.down(dist, d_dist, (size_t)B * nobs * H);
    st.down(linkid, p->linkid.p, (size_t)B * nobs * H);
    st.down(grad, d_grad, (size_t)B * nobs * H * nj);
    return st.result("copy back");
}

int cfs_get_con(cfs_problem *p, int B, const double *x_, const double *u, const double *xR1, const double *obs,
                double *Ainq, double *binq)
{
    int rc = cfs_check_batch(p, B);
    if (rc) return rc;
    if (!x_ || !u || !xR1 || !obs || !Ainq || !binq) return cfs_fail(CFS_ERR_INVALID_ARG, "NULL array");
    CFS_HIPCHK(hipSetDevice(p->device));
    const size_t nobs = p->d.nobs, H = p->d.H, nj = p->d.njoint, nn = p->nn;
    const size_t rows = nobs * H * (1 + 2 * nj) + (limited(p) ? 2 * nn : 0);   // limited: + pos+ (i, c), pos- (i, c)
    Stage st;
    PieceBuffers pb;
    rc = stage_piece(p, st, B, x_, xR1, obs, pb);
    if (rc) return rc;
    DenseConParams dc;
    dc.B = B; dc.H = p->d.H; dc.nj = p->d.njoint; dc.nobs = p->d.nobs; dc.dt = p->d.robot.delta_t;
    double *d_dist = st.out<double>((size_t)B * nobs * H);
    double *d_grad = st.out<double>((size_t)B * nobs * H * nj);
    dc.dist = d_dist; dc.grad = d_grad;
    dc.u = st.up(u, (size_t)B * nn);
    dc.xR1 = pb.xR1;
    dc.lim = p->lim.p; dc.margin = p->margin.p;
    dc.plim = limited(p) ? p->lim.p + nj : nullptr;
    dc.Ainq = st.out<double>((size_t)B * rows * nn);
    dc.binq = st.out<double>((size_t)B * rows);
    if (st.err != hipSuccess) return st.result("staging");
    rc = linearize_piece(p, B, pb, d_dist, d_grad, nullptr);
    if (rc) return rc;
    launch_dense_con(dc, nullptr);
    CFS_HIPCHK(hipGetLastError());
    CFS_HIPCHK(hipStreamSynchronize(nullptr));
    st.down(Ainq, dc.Ainq, (size_t)B * rows * nn);
    st.down(binq, dc.binq, (size_t)B * rows);
    return st.result("copy back");
}

int cfs_qp(cfs_problem *p, int B, const double *lin, const double *u_lin, const double *xR1,
           const double *dist, const double *grad, double *u, double *lambda, int *qp_iter, int *status)
{
    int rc = cfs_check_batch(p, B);
    if (rc) return rc;
    if (!lin || !u_lin || !xR1 || !dist || !grad || !u) return cfs_fail(CFS_ERR_INVALID_ARG, "NULL array");
    CFS_HIPCHK(hipSetDevice(p->device));
    const size_t nobs = p->d.nobs, H = p->d.H, nj = p->d.njoint, nn = p->nn;
    const size_t nlam = nobs * H + (limited(p) ? 6 : 4) * nn;   // [collision | vel+ | vel- | bound+ | bound- (| pos+ | pos-)]
    Stage st;
    PieceBuffers pb;
    rc = stage_piece(p, st, B, nullptr, xR1, nullptr, pb);
    if (rc) return rc;
    double *d_lin = st.up(lin, (size_t)B * nn);
    double *d_u = st.up(u_lin, (size_t)B * nn);
    double *d_dist = st.up(dist, (size_t)B * nobs * H);
    double *d_grad = st.up(grad, (size_t)B * nobs * H * nj);
    double *d_lam = lambda ? st.out<double>((size_t)B * nlam) : nullptr;
    int *d_it = st.out<int>((size_t)B), *d_st = st.out<int>((size_t)B);
    if (st.err != hipSuccess) return st.result("staging");
    FusedParams fp;
    fill_fused_family(p, fp, B);
    fp.x_init = pb.x_; fp.xR1 = pb.xR1; fp.ff = pb.ff; fp.caug = pb.caug; fp.obs = pb.obs;
    fp.piece = 2;
    fp.nmesh = p->d.nobs; fp.ext_dist = d_dist; fp.ext_grad = d_grad;     // every row of the linearisation is given
    fp.u = d_u; fp.total_iter = d_it; fp.status = d_st; fp.dump_lambda = d_lam;
    if (p->d.mode == CFS_MODE_CFS) {      // start point: the unconstrained minimiser -H^{-1} ff (CFS) | u_ itself (projection)
        GemvParams g;
        g.B = B; g.nn = (int)nn; g.M = p->Hinv.p; g.X = d_lin; g.Y = p->x0.p; g.scale = -1.0;
        launch_batched_gemv(g, nullptr);
        fp.x0 = p->x0.p;
    } else fp.x0 = d_lin;
    SoftParams sp;
    CFS_HIPCHK(launch_fused(p->d.njoint, fp, nullptr, force_w1(p), analytic(p), soft_params(p, sp, false), false, limited(p)));
    CFS_HIPCHK(hipGetLastError());
    CFS_HIPCHK(hipStreamSynchronize(nullptr));
    st.down(u, d_u, (size_t)B * nn);
    if (lambda) st.down(lambda, d_lam, (size_t)B * nlam);
    st.down(qp_iter, d_it, (size_t)B);
    st.down(status, d_st, (size_t)B);
    return st.result("copy back");
}

}  // extern "C"
