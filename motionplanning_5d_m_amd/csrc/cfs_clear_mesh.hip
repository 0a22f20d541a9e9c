// cfs_clear_mesh.hip -- clearance audit against mesh obstacles along the motion between the waypoints (cfs_clearance_mesh_device).
//
// The contract is cfs_clear.hip's (time line, samples, first minimum, t_path, link_path, lower bound) with the distance of
// cfs_dist_arm_mesh: same FK, the exact segment-triangle minimum over the hierarchy (cfs_mesh_dev.h), the near-zero surrogate of
// dist_arm_surf_200i.m:22-24, first-minimum link.  A static mesh does not move, so the bound's v_obs is 0: the distance from a segment
// to a fixed closed set is 1-Lipschitz in the segment's end points, which is all the argument of DESIGN.md section 17 uses.  A mesh
// with a pose per waypoint (cfs_clearance_mesh_motion_device) is measured through the POSED instantiations further down.
//
// MI355X mapping.  A sample costs nj * nmesh hierarchy traversals of unequal length -- three orders of
// magnitude more than a line sample -- so a problem is spread over ceil(G / 64) workgroups instead of one, and the per-sample
// results travel through a workspace in HBM (B x nmesh x G distances, links, triangles; B x G arm speeds):
//   sample kernel  one lane per sample, a wavefront per workgroup: the 64 lanes hold consecutive samples of one problem, poses that
//                  differ by one sub-step, so their traversals take nearly the same path (little divergence, shared L2 lines).  The
//                  lane walks the links in order (one transform in registers) and queries every mesh per link; its private
//                  (node, bound) stack is strided in LDS as in cfs_mesh_seg_kernel (64 x 20 x 8 B = 10 KB per workgroup).
//   scan kernel    one workgroup per (problem, mesh): lanes stride over the samples (consecutive words), keep the waypoint minimum,
//                  the path minimum with its first arg-min and the sub-interval bounds, and meet once in LDS; ties go to the lowest g.
// No atomics; every output is a minimum over per-sample values that depend on the sample alone, so neither B nor the position in the
// batch nor the launch shape changes a bit.
//
// Time coherence, two independent switches (ClearMeshParams::opt; both leave every distance bit-identical to cold, unbounded queries
// because mesh_query returns the lexicographic minimum (distance, axis parameter) over a rigorously pruned set whatever it starts from):
//   bound  link k's query starts from the incumbent max(running minimum of links < k, 1e-4): a link with nothing closer can neither
//          become the (first) minimum nor reach the surrogate -- the argument of the solver's candidate pruning;
//   seed   the H + 1 waypoint poses are queried first, then every sub-sample's query tests the winning triangle of its interval's
//          start before it descends (seed_tri of mesh_query).
#include "cfs_clear_dev.h"
#include "cfs_mesh_dev.h"
#include "cfs_problem.h"

namespace {

constexpr int CM_THREADS = 64;                       // sample kernel: one wavefront of consecutive samples
constexpr int CM_SCAN = 256;

// which samples a launch of the sample kernel covers
enum { CM_ALL = 0, CM_WAYPOINTS = 1, CM_BETWEEN = 2 };

// Moving meshes (cfs_clearance_mesh_motion*).  Where mesh jm stands at sample g does not depend on the problem,
// so the inverse transform of every (mesh, sample) is written once per (sub-steps, poses) by this kernel, one lane each, and the sample
// kernel's POSED instantiations only apply it.  A waypoint sample (k = S), interval 0 and a held interval copy the 12 stored doubles
// the linearisation reads (cfs_mesh.hip, mesh_link_ends): dist_wp is measured where get_con measures it, and constant poses give the
// static audit's bits.  Otherwise, at s = k/S: R(s) = Rod(a, s*theta) R_{i-1}, c_w(s) on the straight line, and the row-major record
// [R(s)' | c_j - R(s)'c_w(s)] maps a world point into the frame the mesh is stored in.
__global__ __launch_bounds__(CM_THREADS) void cfs_clear_mesh_pose_kernel(int nmesh, int H, int S, const double *itv, const double *inv,
                                                                         double *out_pose, double *out_v)
{
    const int G = H * S + 1, e = blockIdx.x * CM_THREADS + threadIdx.x;
    if (e >= nmesh * G) return;
    const int jm = e / G, g = e % G;
    int i, k;
    clear_sample_ik(g, S, i, k);
    const double *q = itv + ((size_t)jm * H + i) * CLEAR_ITV;
    double *o = out_pose + (size_t)e * 12;
    if (g < H) out_v[(size_t)jm * H + g] = itv[((size_t)jm * H + g) * CLEAR_ITV + 23];
    if (k == S || q[0] == 0.0) {                     // g = 0 is interval 0, which is held
        const double *src = inv + ((size_t)jm * H + i) * 12;
        for (int r = 0; r < 12; ++r) o[r] = src[r];
        return;
    }
    const double s = (double)k / (double)S;
    double sn, cs;
    sincos(s * q[4], &sn, &cs);
    const double ax = q[1], ay = q[2], az = q[3], c1 = 1.0 - cs;
    const double Q[9] = {cs + c1 * ax * ax, c1 * ax * ay - sn * az, c1 * ax * az + sn * ay,       // Rodrigues: I + sin K + (1 - cos) K^2
                         c1 * ay * ax + sn * az, cs + c1 * ay * ay, c1 * ay * az - sn * ax,
                         c1 * az * ax - sn * ay, c1 * az * ay + sn * ax, cs + c1 * az * az};
    double R[9], cw[3];
    for (int r = 0; r < 3; ++r) {
        for (int c = 0; c < 3; ++c) R[3 * r + c] = Q[3 * r] * q[5 + c] + Q[3 * r + 1] * q[8 + c] + Q[3 * r + 2] * q[11 + c];
        cw[r] = q[14 + r] + s * (q[17 + r] - q[14 + r]);
    }
    for (int r = 0; r < 3; ++r) {                    // row r of R': column r of R
        o[4 * r] = R[r]; o[4 * r + 1] = R[3 + r]; o[4 * r + 2] = R[6 + r];
        o[4 * r + 3] = q[20 + r] - (R[r] * cw[0] + R[3 + r] * cw[1] + R[6 + r] * cw[2]);
    }
}

// POSED: the link ends go through table row (mesh, sample) before the query; the surrogate's closest point and the link's far end both
// live in the mesh's frame.  The static instantiations keep the statements they always had.
template <bool BOUND, bool POSED>
__global__ __launch_bounds__(CM_THREADS) void cfs_clear_mesh_sample_kernel(ClearMeshParams C, int phase)
{
    __shared__ int s_stack[MESH_STACK * CM_THREADS];
    __shared__ float s_lbs[MESH_STACK * CM_THREADS];
    const int t = threadIdx.x, b = blockIdx.y;
    const int H = C.H, nj = C.nj, ns = 2 * nj, S = C.S, nmesh = C.nmesh, G = H * S + 1;
    const int e = blockIdx.x * CM_THREADS + t;
    int g;                                           // this lane's sample
    if (phase == CM_ALL) g = e;
    else if (phase == CM_WAYPOINTS) g = e <= H ? e * S : G;
    else g = e < H * (S - 1) ? (e / (S - 1)) * S + e % (S - 1) + 1 : G;
    if (g >= G) return;
    const double *x = C.x_ + (size_t)b * H * ns, *u = C.u + (size_t)b * H * nj, *x1 = C.xR1 + (size_t)b * ns;
    const DevRobot *rb = C.rb;
    int i, k;
    clear_sample_ik(g, S, i, k);
    // workspace rows of this sample: [b][mesh][g]; seeds [b][waypoint 0..H][link][mesh] (hierarchy order, -1: none)
    double *w_d = C.ws_d + (size_t)b * nmesh * G + g;
    int *w_lk = C.ws_lk + (size_t)b * nmesh * G + g, *w_tri = C.ws_tri + (size_t)b * nmesh * G + g;
    const bool seeded = phase == CM_BETWEEN, seeding = phase == CM_WAYPOINTS;
    // a sub-sample g = i*S + k, 0 < k < S, starts from waypoint pose i (g = 0 is pose 0, g = i*S is pose i)
    int *w_seed = C.ws_seed + ((size_t)b * (H + 1) + (seeding ? g / S : i)) * nj * nmesh;
    for (int jm = 0; jm < nmesh; ++jm) { w_d[(size_t)jm * G] = INFINITY; w_lk[(size_t)jm * G] = 0; w_tri[(size_t)jm * G] = -1; }
    double M[12];
    // one link: its transform from the parent's (none for link 0), then its distance to every mesh
    auto link = [&](int kk, const double *par) {
        const double th = clear_sample_theta(x, u, x1, nj, S, C.dt, i, k, kk);
        double sn, cs, Mn[12], e6[6];
        sincos(th - rb->th_off[kk], &sn, &cs);
        fk_step(rb, kk, sn, cs, par, Mn);
#pragma unroll
        for (int q = 0; q < 12; ++q) M[q] = Mn[q];
        link_ends(rb, kk, M, e6);
        for (int jm = 0; jm < nmesh; ++jm) {
            const double cur = w_d[(size_t)jm * G];
            const int seed = seeded ? w_seed[kk * nmesh + jm] : -1;
            Best bq;
            double m6[POSED ? 6 : 1];
            const double *a6 = e6;                   // the link's ends in the frame mesh jm is stored in
            if constexpr (POSED) {
                const double *T = C.pose + ((size_t)jm * G + g) * 12;
#pragma unroll
                for (int r = 0; r < 3; ++r) {
                    const double t0 = T[4 * r], t1 = T[4 * r + 1], t2 = T[4 * r + 2], t3 = T[4 * r + 3];
                    m6[r] = t0 * e6[0] + t1 * e6[1] + t2 * e6[2] + t3;
                    m6[3 + r] = t0 * e6[3] + t1 * e6[4] + t2 * e6[5] + t3;
                }
                a6 = m6;
            }
            mesh_query<CM_THREADS, false>(C.meshes[jm], a6, a6 + 3, seed, s_stack + t, s_lbs + t, bq, nullptr,
                                          BOUND ? fmax(cur, 0.0001) : INFINITY);
            if (seeding) w_seed[kk * nmesh + jm] = bq.tri;
            if (bq.tri < 0) continue;                // nothing closer than the bound: not the minimum
            const double dis = with_surrogate(bq, a6);
            if (dis < cur) {                         // first minimum wins
                w_d[(size_t)jm * G] = dis; w_lk[(size_t)jm * G] = kk + 1; w_tri[(size_t)jm * G] = C.meshes[jm].orig[bq.tri];
            }
        }
    };
    link(0, nullptr);
#pragma unroll 1
    for (int kk = 1; kk < nj; ++kk) link(kk, M);
    if (g < G - 1) C.ws_L[(size_t)b * G + g] = clear_arm_speed(x, u, x1, C.rho, nj, S, C.dt, g);
}

// POSED: L of sub-interval g carries the surface speed of mesh jm in its interval g / S (0 where the mesh is held: L + 0 is L)
template <bool POSED>
__global__ __launch_bounds__(CM_SCAN) void cfs_clear_mesh_scan_kernel(ClearMeshParams C)
{
    __shared__ double r_wp[CM_SCAN], r_path[CM_SCAN], r_low[CM_SCAN];
    __shared__ int r_g[CM_SCAN];
    const int t = threadIdx.x, jm = blockIdx.x, b = blockIdx.y;
    const int S = C.S, G = C.H * S + 1, nline = C.nobs - C.nmesh;
    const double *d = C.ws_d + ((size_t)b * C.nmesh + jm) * G, *L = C.ws_L + (size_t)b * G;
    double a_wp = INFINITY, a_path = INFINITY, a_low = INFINITY;
    int a_g = 0;
    for (int g = t; g < G; g += CM_SCAN) {           // g rises: a strict < keeps the lane's lowest arg-min
        const double d0 = d[g];
        if (d0 < a_path) { a_path = d0; a_g = g; }
        if (g > 0 && g % S == 0) a_wp = fmin(a_wp, d0);
        if constexpr (POSED) {
            if (g + 1 < G) a_low = fmin(a_low, (d0 + d[g + 1]) / 2.0 - (L[g] + C.v_mesh[(size_t)jm * C.H + g / S]) * C.dt / (2.0 * (double)S));
        } else {
            if (g + 1 < G) a_low = fmin(a_low, (d0 + d[g + 1]) / 2.0 - L[g] * C.dt / (2.0 * (double)S));   // v_obs = 0
        }
    }
    r_wp[t] = a_wp; r_path[t] = a_path; r_low[t] = a_low; r_g[t] = a_g;
    __syncthreads();
    if (t == 0) {                                    // the lanes meet: lowest distance, then lowest g
        double m_wp = INFINITY, m_path = INFINITY, m_low = INFINITY;
        int m_g = 0;
        for (int q = 0; q < CM_SCAN; ++q) {
            m_wp = fmin(m_wp, r_wp[q]);
            m_low = fmin(m_low, r_low[q]);
            if (r_path[q] < m_path || (r_path[q] == m_path && r_g[q] < m_g)) { m_path = r_path[q]; m_g = r_g[q]; }
        }
        int i, k;
        clear_sample_ik(m_g, S, i, k);
        const size_t o = (size_t)b * C.nobs + nline + jm, w = ((size_t)b * C.nmesh + jm) * G + m_g;
        C.dist_wp[o] = m_wp;
        C.dist_path[o] = m_path;
        C.dist_lower[o] = m_low;
        C.t_path[o] = ((double)i + (double)k / (double)S) * C.dt;
        C.link_path[o] = C.ws_lk[w];
        C.tri_path[o] = C.ws_tri[w];
    }
    if (jm == 0)                                     // line columns have no triangle
        for (int j = t; j < nline; j += CM_SCAN) C.tri_path[(size_t)b * C.nobs + j] = -1;
}

template <bool BOUND, bool POSED>
void launch_samples(const ClearMeshParams &p, int phase, int n, hipStream_t s)
{
    if (n <= 0) return;
    hipLaunchKernelGGL((cfs_clear_mesh_sample_kernel<BOUND, POSED>), dim3((n + CM_THREADS - 1) / CM_THREADS, p.B), dim3(CM_THREADS), 0, s, p, phase);
}

template <bool POSED>
hipError_t launch_clearance_mesh_as(const ClearMeshParams &p, hipStream_t s)
{
    const int G = p.H * p.S + 1;
    const bool bound = (p.opt & CLEAR_MESH_BOUND) != 0;
    auto samples = [&](int phase, int n) { if (bound) launch_samples<true, POSED>(p, phase, n, s); else launch_samples<false, POSED>(p, phase, n, s); };
    if (p.opt & CLEAR_MESH_SEED) {
        samples(CM_WAYPOINTS, p.H + 1);
        samples(CM_BETWEEN, p.H * (p.S - 1));
    } else {
        samples(CM_ALL, G);
    }
    hipLaunchKernelGGL(cfs_clear_mesh_scan_kernel<POSED>, dim3(p.nmesh, p.B), dim3(CM_SCAN), 0, s, p);
    return hipGetLastError();
}

// the workspace of an audit with `substeps` sub-steps (grown by the first audit that needs more) and the launch, shared by the static
// and the moving entry; pose / v_mesh: the pose table of a moving handle, null for static meshes
int clearance_mesh_enqueue(cfs_problem *p, int B, int substeps, const ClearArrays &a, const double *pose, const double *v_mesh, hipStream_t s)
{
    const int nline = p->d.nobs - p->nmesh;
    if (substeps > p->cm.S) {                        // grow the workspace (the old one is freed first, which waits for whatever still reads it)
        const size_t G = (size_t)p->d.H * substeps + 1, mb = (size_t)p->d.max_batch;
        p->cm = ClearMeshWork{};
        CFS_HIPCHK(p->cm.cm_d.alloc(mb * G * p->nmesh)); CFS_HIPCHK(p->cm.cm_L.alloc(mb * G));
        CFS_HIPCHK(p->cm.cm_lk.alloc(mb * G * p->nmesh)); CFS_HIPCHK(p->cm.cm_tri.alloc(mb * G * p->nmesh));
        CFS_HIPCHK(p->cm.cm_seed.alloc(mb * (size_t)(p->d.H + 1) * p->d.njoint * p->nmesh));
        CFS_HIPCHK(p->cm.cm_rho.upload(p->rho, CFS_MAX_LINKS * CFS_MAX_LINKS));
        p->cm.S = substeps;
    }
    if (nline > 0) CFS_HIPCHK(cfs_launch_clearance_lines(p, B, substeps, nline, a, s));   // the line columns: cfs_clearance's kernel
    ClearMeshParams cm;
    cm.rb = p->rb.p; cm.B = B; cm.H = p->d.H; cm.nj = p->d.njoint; cm.nobs = p->d.nobs; cm.nmesh = p->nmesh; cm.S = substeps;
    cm.opt = ((p->dbg_mask & CFS_DBG_CLEAR_NO_BOUND) ? 0 : CLEAR_MESH_BOUND) | ((p->dbg_mask & CFS_DBG_CLEAR_SEED) ? CLEAR_MESH_SEED : 0);
    cm.dt = p->d.robot.delta_t;
    cm.meshes = p->mesh.meshes_d.p;
    cm.x_ = a.x_; cm.u = a.u; cm.xR1 = a.xR1;
    cm.dist_wp = a.dist_wp; cm.dist_path = a.dist_path; cm.dist_lower = a.dist_lower; cm.t_path = a.t_path;
    cm.link_path = a.link_path; cm.tri_path = a.tri_path;
    cm.ws_d = p->cm.cm_d.p; cm.ws_L = p->cm.cm_L.p; cm.ws_lk = p->cm.cm_lk.p; cm.ws_tri = p->cm.cm_tri.p; cm.ws_seed = p->cm.cm_seed.p;
    cm.rho = p->cm.cm_rho.p;
    cm.pose = pose; cm.v_mesh = v_mesh;
    CFS_HIPCHK(launch_clearance_mesh(cm, s));
    return CFS_SUCCESS;
}

}  // namespace

hipError_t launch_clearance_mesh(const ClearMeshParams &p, hipStream_t s)
{
    return p.pose ? launch_clearance_mesh_as<true>(p, s) : launch_clearance_mesh_as<false>(p, s);
}

hipError_t launch_clear_mesh_poses(int nmesh, int H, int S, const double *itv, const double *inv, double *out_pose, double *out_v, hipStream_t s)
{
    const int n = nmesh * (H * S + 1);
    hipLaunchKernelGGL(cfs_clear_mesh_pose_kernel, dim3((n + CM_THREADS - 1) / CM_THREADS), dim3(CM_THREADS), 0, s, nmesh, H, S, itv, inv, out_pose, out_v);
    return hipGetLastError();
}

// ---- C ABI (include/cfs_hip.h, "clearance audit against mesh obstacles") ------------------------------------------------------
extern "C" int cfs_clearance_mesh_device(cfs_problem *p, int B, int substeps, const double *x_, const double *u, const double *xR1,
                                         const double *obs, double *dist_wp, double *dist_path, double *dist_lower, double *t_path,
                                         int *link_path, int *tri_path, void *stream)
{
    const ClearArrays a{x_, u, xR1, obs, dist_wp, dist_path, dist_lower, t_path, link_path, tri_path};
    int rc = cfs_check_clearance(p, B, substeps, a, true);
    if (rc) return rc;
    CFS_HIPCHK(hipSetDevice(p->device));
    return clearance_mesh_enqueue(p, B, substeps, a, nullptr, nullptr, reinterpret_cast<hipStream_t>(stream));
}

extern "C" int cfs_clearance_mesh(cfs_problem *p, int B, int substeps, const double *x_, const double *u, const double *xR1, const double *obs,
                                  double *dist_wp, double *dist_path, double *dist_lower, double *t_path, int *link_path, int *tri_path)
{
    return cfs_clearance_host(p, B, substeps, ClearArrays{x_, u, xR1, obs, dist_wp, dist_path, dist_lower, t_path, link_path, tri_path}, true);
}

// ---- C ABI (include/cfs_hip.h, "clearance audit with moving meshes") -----------------------------------------------------------
extern "C" int cfs_clearance_mesh_motion_device(cfs_problem *p, int B, int substeps, const double *x_, const double *u, const double *xR1,
                                                const double *obs, double *dist_wp, double *dist_path, double *dist_lower, double *t_path,
                                                int *link_path, int *tri_path, void *stream)
{
    const ClearArrays a{x_, u, xR1, obs, dist_wp, dist_path, dist_lower, t_path, link_path, tri_path};
    int rc = cfs_check_clearance(p, B, substeps, a, true, true);
    if (rc) return rc;
    CFS_HIPCHK(hipSetDevice(p->device));
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (!p->mm.mesh_pose.p) return clearance_mesh_enqueue(p, B, substeps, a, nullptr, nullptr, s);   // static meshes: the static path
    if (substeps > p->mm.cmm_cap) {                     // grow the table (alloc frees the old one first, which waits for whatever still reads it)
        p->mm.cmm_cap = 0; p->mm.cmm_gen = -1;
        CFS_HIPCHK(p->mm.cmm_pose.alloc((size_t)p->nmesh * ((size_t)p->d.H * substeps + 1) * 12));
        CFS_HIPCHK(p->mm.cmm_v.alloc((size_t)p->nmesh * p->d.H));
        p->mm.cmm_cap = substeps;
    }
    if (p->mm.cmm_S != substeps || p->mm.cmm_gen != p->motion_gen) {   // the table of another S or of other poses: rebuild it, ahead of the audit on its stream
        CFS_HIPCHK(launch_clear_mesh_poses(p->nmesh, p->d.H, substeps, p->mm.mesh_itv.p, p->mm.mesh_pose.p, p->mm.cmm_pose.p, p->mm.cmm_v.p, s));
        p->mm.cmm_S = substeps; p->mm.cmm_gen = p->motion_gen;
    }
    return clearance_mesh_enqueue(p, B, substeps, a, p->mm.cmm_pose.p, p->mm.cmm_v.p, s);
}

extern "C" int cfs_clearance_mesh_motion(cfs_problem *p, int B, int substeps, const double *x_, const double *u, const double *xR1,
                                         const double *obs, double *dist_wp, double *dist_path, double *dist_lower, double *t_path,
                                         int *link_path, int *tri_path)
{
    return cfs_clearance_host(p, B, substeps, ClearArrays{x_, u, xR1, obs, dist_wp, dist_path, dist_lower, t_path, link_path, tri_path}, true, true);
}
