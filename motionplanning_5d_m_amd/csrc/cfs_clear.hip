// cfs_clear.hip -- clearance audit of B trajectories along the motion between the waypoints (cfs_clearance_device).
//
// Reference behaviour restated (not translated): get_con writes its collision rows at the H waypoints only
// (Lib/CFS_FANUC.m:110-120, Lib/PSGCFS_FANUC.m:152-160); between them the arm follows the double integrator of
// robotproperty2.m:136-139, theta(tau) = theta_s + tau v_s + tau^2/2 u_i.  Nothing in the reference measures that motion; this
// kernel does, with the dist_arm of cfs_geom_dev.h (same FK, seg_seg_dist, near-zero surrogate, first-minimum link), and adds a
// lower bound of the distance over continuous time (include/cfs_hip.h, cfs_clearance_device).
//
// Time line.  Sample S of interval i and sample 0 of interval i+1 are the same pose (row i of x_) against the same obstacle
// rows, so the H*(S+1) samples of the contract are G = H*S + 1 distinct ones, g = 0 (xR1) and g = i*S + k (k = 1..S); the
// first minimum over g is the contract's (lowest interval, then lowest k).  Sub-interval g joins samples g and g + 1.
//
// MI355X mapping: one workgroup of P = 256 | 128 | 64 threads per problem (the largest whose LDS plan leaves room for two
// workgroups per compute unit), the problem's x_, u, xR1, obstacle rows, their speeds and rho staged in LDS.  The time line is
// walked in passes of P samples that overlap by one:
//   phase A  one lane per sample: the pose, then link by link (one transform in registers) the distance to every obstacle,
//            min / first-minimum link kept in LDS at [obstacle][lane] (consecutive lanes, consecutive words: no bank
//            conflict); the lane also bounds the arm's share of |d/dtau distance| on the sub-interval that starts at its sample;
//   phase B  one lane per (obstacle, part of the pass): a sequential scan of its part -- neighbouring samples are neighbouring
//            words -- updates the lane's running minima (waypoints, all samples with their first arg-min, sub-interval bounds).
// The parts of an obstacle meet once, after the last pass, in LDS; ties go to the lowest g.  No atomics: every output is a
// minimum over values that do not depend on P, on B or on the launch, so neither does the result.
#include "cfs_clear_dev.h"
#include "cfs_geom_dev.h"
#include "cfs_problem.h"
#include <algorithm>
#include <cmath>
#include <cstring>

namespace {

constexpr int CLEAR_MAX_P = 256;

struct ClearPlan {               // LDS layout: offsets in doubles, then (from the end of the doubles) in ints
    int P;
    size_t rb, rho, x, u, x1, obs, vobs, L, d, rwp, rpath, rlow, n_double, lk, rg, rlk, bytes;
};

ClearPlan clear_plan(int P, int H, int nj, int nobs, bool move)
{
    ClearPlan q;
    size_t o = 0;
    q.P = P;
    q.rb = o; o += sizeof(DevRobot) / 8;
    q.rho = o; o += CFS_MAX_LINKS * CFS_MAX_LINKS;
    q.x = o; o += (size_t)H * 2 * nj;
    q.u = o; o += (size_t)H * nj;
    q.x1 = o; o += 2 * (size_t)nj;
    q.obs = o; o += (size_t)(move ? H : 1) * nobs * 6;
    q.vobs = o; o += move ? (size_t)H * nobs : 0;
    q.L = o; o += P;
    q.d = o; o += (size_t)nobs * P;
    q.rwp = o; o += P;
    q.rpath = o; o += P;
    q.rlow = o; o += P;
    q.n_double = o;
    size_t i = 0;
    q.lk = i; i += (size_t)nobs * P;
    q.rg = i; i += P;
    q.rlk = i; i += P;
    q.bytes = o * 8 + i * 4;
    return q;
}

__device__ __forceinline__ double norm3(double x, double y, double z) { return sqrt(x * x + y * y + z * z); }

__global__ __launch_bounds__(CLEAR_MAX_P) void cfs_clearance_kernel(ClearParams C, ClearPlan Q)
{
    extern __shared__ __attribute__((aligned(16))) double lds[];
    const int P = blockDim.x, t = threadIdx.x, b = blockIdx.x;
    const int H = C.H, nj = C.nj, ns = 2 * nj, nn = H * nj, nobs = C.nobs, S = C.S;
    const bool move = C.move != 0;
    double *s_rb = lds + Q.rb, *s_rho = lds + Q.rho, *s_x = lds + Q.x, *s_u = lds + Q.u, *s_x1 = lds + Q.x1;
    double *s_obs = lds + Q.obs, *s_vobs = lds + Q.vobs, *s_L = lds + Q.L, *s_d = lds + Q.d;
    double *r_wp = lds + Q.rwp, *r_path = lds + Q.rpath, *r_low = lds + Q.rlow;
    int *ibase = reinterpret_cast<int *>(lds + Q.n_double);
    int *s_lk = ibase + Q.lk, *r_g = ibase + Q.rg, *r_lk = ibase + Q.rlk;

    // ---- stage the problem ----
    {
        const double *src = reinterpret_cast<const double *>(C.rb);
        for (int e = t; e < (int)(sizeof(DevRobot) / 8); e += P) s_rb[e] = src[e];
        for (int e = t; e < CFS_MAX_LINKS * CFS_MAX_LINKS; e += P) s_rho[e] = C.rho[e];
        for (int e = t; e < H * ns; e += P) s_x[e] = C.x_[(size_t)b * H * ns + e];
        for (int e = t; e < nn; e += P) s_u[e] = C.u[(size_t)b * nn + e];
        for (int e = t; e < ns; e += P) s_x1[e] = C.xR1[(size_t)b * ns + e];
        const int no = (move ? H : 1) * nobs * 6;
        for (int e = t; e < no; e += P) s_obs[e] = C.obs[(size_t)b * C.obs_stride * 6 + e];
    }
    __syncthreads();
    const DevRobot *rb = reinterpret_cast<const DevRobot *>(s_rb);
    if (move)                    // speed of obstacle j in interval i: the larger end-point displacement between rows i-1 and i over
        for (int e = t; e < H * nobs; e += P) {      // delta_t; 0 in interval 0, where the obstacle is held at row 0
            const int i = e / nobs;
            double v = 0.0;
            if (i > 0) {
                const double *a = s_obs + (size_t)(e - nobs) * 6, *c = s_obs + (size_t)e * 6;
                v = fmax(norm3(c[0] - a[0], c[1] - a[1], c[2] - a[2]), norm3(c[3] - a[3], c[4] - a[4], c[5] - a[5])) / C.dt;
            }
            s_vobs[e] = v;
        }

    const int G = H * S + 1;                         // samples of the time line (>= 2); sub-intervals: G - 1
    // phase B's lane: obstacle jB, part pB of the pass; a part is `chunk` samples
    const int nparts = P / nobs, chunk = (P + nparts - 1) / nparts;
    const int jB = t % nobs, pB = t / nobs;
    const bool scan = pB < nparts;
    double a_wp = INFINITY, a_path = INFINITY, a_low = INFINITY;
    int a_g = 0, a_lk = 0;

    for (int g0 = 0; g0 < G - 1; g0 += P - 1) {
        __syncthreads();                             // the previous pass's scan is over (first pass: s_vobs is written)
        // ---- phase A: sample g = g0 + t ----
        const int g = g0 + t;
        if (g < G) {
            int i, k;                                                                       // g = i*S + k, k = 1..S (g = 0: k = 0)
            clear_sample_ik(g, S, i, k);
            const double *oa = s_obs, *ob = s_obs;                                          // obstacle rows: a + wo (b - a)
            double wo = 0.0;
            if (move) {
                if (i == 0 || k == S) oa = ob = s_obs + (size_t)i * nobs * 6;
                else { oa = s_obs + (size_t)(i - 1) * nobs * 6; ob = s_obs + (size_t)i * nobs * 6; wo = (double)k / (double)S; }
            }
            for (int j = 0; j < nobs; ++j) { s_d[j * P + t] = INFINITY; s_lk[j * P + t] = 0; }
            // one link: its transform from the parent's (none for link 0), then its distance to every obstacle
            double M[12];
            auto link = [&](int kk, const double *par) {
                const double th = clear_sample_theta(s_x, s_u, s_x1, nj, S, C.dt, i, k, kk);
                double sn, cs, Mn[12], e6[6];
                sincos(th - rb->th_off[kk], &sn, &cs);
                fk_step(rb, kk, sn, cs, par, Mn);
#pragma unroll
                for (int q = 0; q < 12; ++q) M[q] = Mn[q];
                link_ends(rb, kk, M, e6);
                for (int j = 0; j < nobs; ++j) {
                    double o6[6];
#pragma unroll
                    for (int q = 0; q < 6; ++q) { const double a = oa[j * 6 + q]; o6[q] = a + wo * (ob[j * 6 + q] - a); }
                    const double dis = seg_seg_dist(e6, o6);
                    if (dis < s_d[j * P + t]) { s_d[j * P + t] = dis; s_lk[j * P + t] = kk + 1; }   // first minimum wins
                }
            };
            link(0, nullptr);
            for (int kk = 1; kk < nj; ++kk) link(kk, M);
            // arm's share of |d/dtau distance| on sub-interval [g, g+1] (cfs_clear_dev.h)
            s_L[t] = g < G - 1 ? clear_arm_speed(s_x, s_u, s_x1, s_rho, nj, S, C.dt, g) : 0.0;
        }
        __syncthreads();
        // ---- phase B: obstacle jB, samples [pB*chunk, (pB+1)*chunk) of the pass ----
        if (scan) {
            const int s1 = min(min((pB + 1) * chunk, P), G - g0);
            for (int s = pB * chunk; s < s1; ++s) {
                const int gg = g0 + s;
                const double d0 = s_d[jB * P + s];
                if (d0 < a_path) { a_path = d0; a_g = gg; a_lk = s_lk[jB * P + s]; }
                if (gg > 0 && gg % S == 0) a_wp = fmin(a_wp, d0);
                if (s + 1 < P && gg + 1 < G) {       // sub-interval gg: its other end is in this pass
                    const double vo = move ? s_vobs[(gg / S) * nobs + jB] : 0.0;
                    const double low = (d0 + s_d[jB * P + s + 1]) / 2.0 - (s_L[s] + vo) * C.dt / (2.0 * (double)S);
                    a_low = fmin(a_low, low);
                }
            }
        }
    }
    // ---- the parts of an obstacle meet: lowest distance, then lowest g ----
    if (scan) { r_wp[t] = a_wp; r_path[t] = a_path; r_low[t] = a_low; r_g[t] = a_g; r_lk[t] = a_lk; }
    __syncthreads();
    if (t < nobs) {
        double m_wp = INFINITY, m_path = INFINITY, m_low = INFINITY;
        int m_g = 0, m_lk = 0;
        for (int pp = 0; pp < nparts; ++pp) {
            const int e = pp * nobs + t;
            m_wp = fmin(m_wp, r_wp[e]);
            m_low = fmin(m_low, r_low[e]);
            if (r_path[e] < m_path || (r_path[e] == m_path && r_g[e] < m_g)) { m_path = r_path[e]; m_g = r_g[e]; m_lk = r_lk[e]; }
        }
        const int i = m_g == 0 ? 0 : (m_g - 1) / S, k = m_g == 0 ? 0 : (m_g - 1) % S + 1;
        const size_t o = (size_t)b * C.out_stride + t;
        C.dist_wp[o] = m_wp;
        C.dist_path[o] = m_path;
        C.dist_lower[o] = m_low;
        C.t_path[o] = ((double)i + (double)k / (double)S) * C.dt;
        C.link_path[o] = m_lk;
    }
}

}  // namespace

// rho[m*CFS_MAX_LINKS + k], m <= k < nj: no point of capsule k is farther than this from the axis of joint m -- the lengths of
// the link translations between them (DH: hypot(a_j, d_j); 2L: |robot.T(:, j+1)|) plus the farther end of capsule k in its frame
void cfs_clear_build_rho(const DevRobot &rb, int nj, double *rho)
{
    for (int e = 0; e < CFS_MAX_LINKS * CFS_MAX_LINKS; ++e) rho[e] = 0.0;
    for (int k = 0; k < nj && k < CFS_MAX_LINKS; ++k) {
        const double *c = rb.cap + k * 6;
        const double ck = std::max(sqrt(c[0] * c[0] + c[1] * c[1] + c[2] * c[2]), sqrt(c[3] * c[3] + c[4] * c[4] + c[5] * c[5]));
        double len = 0.0;
        for (int m = k; m >= 0; --m) {
            const double *tl = rb.t2l + m * 3;
            len += rb.kind == CFS_ROBOT_2L ? sqrt(tl[0] * tl[0] + tl[1] * tl[1] + tl[2] * tl[2]) : hypot(rb.dh_a[m], rb.dh_d[m]);
            rho[m * CFS_MAX_LINKS + k] = len + ck;
        }
    }
}

hipError_t launch_clearance(const ClearParams &p, hipStream_t s)
{
    // the largest workgroup whose plan leaves room for two per compute unit; the smallest one always fits (CFS_MAX_H waypoints of
    // CFS_MAX_OBS moving obstacles: 152 KB)
    ClearPlan q = clear_plan(64, p.H, p.nj, p.nobs, p.move != 0);
    for (int P = CLEAR_MAX_P; P > 64; P /= 2) {
        const ClearPlan c = clear_plan(P, p.H, p.nj, p.nobs, p.move != 0);
        if (c.bytes <= 80 * 1024) { q = c; break; }
    }
    if (q.bytes > 160 * 1024) return hipErrorInvalidValue;
    if (q.bytes > 64 * 1024) {                       // dynamic LDS beyond the default limit
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(cfs_clearance_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(cfs_clearance_kernel, dim3(p.B), dim3(q.P), q.bytes, s, p, q);
    return hipGetLastError();
}

// ---- C ABI (include/cfs_hip.h, "clearance audit") ---------------------------------------------------------------------------
// Reads the family constants of the handle (robot, H, nobs, delta_t, obstacle motion) and nothing a solve writes.
int cfs_check_clearance(const cfs_problem *p, int B, int substeps, const ClearArrays &a, bool mesh, bool motion)
{
    int rc = cfs_check_batch(p, B);
    if (rc) return rc;
    if (substeps < 1 || substeps > 64) return cfs_fail(CFS_ERR_INVALID_ARG, "substeps=%d outside 1..64", substeps);
    if (!a.x_ || !a.u || !a.xR1 || !a.obs || !a.dist_wp || !a.dist_path || !a.dist_lower || !a.t_path || !a.link_path || (mesh && !a.tri_path))
        return cfs_fail(CFS_ERR_INVALID_ARG, "NULL array");
    if (mesh && p->nmesh < 1)
        return cfs_fail(CFS_ERR_INVALID_ARG, "%s needs a handle with mesh obstacles (cfs_problem_set_meshes): use cfs_clearance",
                        motion ? "cfs_clearance_mesh_motion" : "cfs_clearance_mesh");
    if (mesh && motion && p->mm.mesh_pose.p && p->mm.turn_mesh >= 0)
        return cfs_fail(CFS_ERR_INVALID_ARG, "the poses of mesh %d at waypoints %d and %d are more than a quarter turn apart: the audit does not interpolate them",
                        p->mm.turn_mesh, p->mm.turn_wp, p->mm.turn_wp + 1);
    if (mesh && !motion && p->mm.mesh_pose.p) return cfs_fail(CFS_ERR_INVALID_ARG, "cfs_clearance_mesh audits static meshes (its bound takes v_obs = 0 in the mesh columns): this handle has mesh motion");
    if (!mesh && p->nmesh > 0) return cfs_fail(CFS_ERR_INVALID_ARG, "the clearance audit measures line obstacles only: this handle has %d mesh obstacles", p->nmesh);
    return CFS_SUCCESS;
}

hipError_t cfs_launch_clearance_lines(const cfs_problem *p, int B, int substeps, int nline, const ClearArrays &a, hipStream_t s)
{
    ClearParams cp;
    cp.rb = p->rb.p; cp.B = B; cp.H = p->d.H; cp.nj = p->d.njoint; cp.nobs = nline; cp.S = substeps;
    cp.move = cfs_moving(p) ? 1 : 0; cp.dt = p->d.robot.delta_t;             // a handle with meshes is static
    cp.x_ = a.x_; cp.u = a.u; cp.xR1 = a.xR1; cp.obs = a.obs;
    cp.dist_wp = a.dist_wp; cp.dist_path = a.dist_path; cp.dist_lower = a.dist_lower; cp.t_path = a.t_path; cp.link_path = a.link_path;
    cp.obs_stride = (int)cfs_obs_rows(p); cp.out_stride = p->d.nobs;
    memcpy(cp.rho, p->rho, sizeof cp.rho);
    return launch_clearance(cp, s);
}

int cfs_clearance_host(cfs_problem *p, int B, int substeps, const ClearArrays &h, bool mesh, bool motion)
{
    int rc = cfs_check_clearance(p, B, substeps, h, mesh, motion);
    if (rc) return rc;
    CFS_HIPCHK(hipSetDevice(p->device));
    const size_t nB = B, n = nB * p->d.nobs;
    Stage st;
    const ClearArrays a{st.up(h.x_, nB * p->nx), st.up(h.u, nB * p->nn), st.up(h.xR1, nB * p->ns), st.up(h.obs, nB * cfs_obs_rows(p) * 6),
                        st.out<double>(n), st.out<double>(n), st.out<double>(n), st.out<double>(n), st.out<int>(n), mesh ? st.out<int>(n) : nullptr};
    if (st.err != hipSuccess) return st.result("staging");
    rc = motion ? cfs_clearance_mesh_motion_device(p, B, substeps, a.x_, a.u, a.xR1, a.obs, a.dist_wp, a.dist_path, a.dist_lower, a.t_path, a.link_path, a.tri_path, nullptr)
       : mesh ? cfs_clearance_mesh_device(p, B, substeps, a.x_, a.u, a.xR1, a.obs, a.dist_wp, a.dist_path, a.dist_lower, a.t_path, a.link_path, a.tri_path, nullptr)
              : cfs_clearance_device(p, B, substeps, a.x_, a.u, a.xR1, a.obs, a.dist_wp, a.dist_path, a.dist_lower, a.t_path, a.link_path, nullptr);
    if (rc) return rc;
    CFS_HIPCHK(hipStreamSynchronize(nullptr));
    st.down(h.dist_wp, a.dist_wp, n); st.down(h.dist_path, a.dist_path, n); st.down(h.dist_lower, a.dist_lower, n); st.down(h.t_path, a.t_path, n);
    st.down(h.link_path, a.link_path, n); st.down(h.tri_path, a.tri_path, n);
    return st.result("copy back");
}

extern "C" int cfs_clearance_device(cfs_problem *p, int B, int substeps, const double *x_, const double *u, const double *xR1, const double *obs,
                                    double *dist_wp, double *dist_path, double *dist_lower, double *t_path, int *link_path, void *stream)
{
    const ClearArrays a{x_, u, xR1, obs, dist_wp, dist_path, dist_lower, t_path, link_path, nullptr};
    int rc = cfs_check_clearance(p, B, substeps, a, false);
    if (rc) return rc;
    CFS_HIPCHK(hipSetDevice(p->device));
    CFS_HIPCHK(cfs_launch_clearance_lines(p, B, substeps, p->d.nobs, a, reinterpret_cast<hipStream_t>(stream)));
    return CFS_SUCCESS;
}

extern "C" int cfs_clearance(cfs_problem *p, int B, int substeps, const double *x_, const double *u, const double *xR1, const double *obs,
                             double *dist_wp, double *dist_path, double *dist_lower, double *t_path, int *link_path)
{
    return cfs_clearance_host(p, B, substeps, ClearArrays{x_, u, xR1, obs, dist_wp, dist_path, dist_lower, t_path, link_path, nullptr}, false);
}
