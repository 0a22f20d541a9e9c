// cfs_cart.hip -- batched tool paths from IK candidates: straight lines (include/cfs_hip.h, "Cartesian paths") and
// polylines of tool poses ("Tool paths"; section 27), traced by one kernel, cfs_cart_kernel<NJ, POLY>.
//
// The reference has no Cartesian moves: its drivers plan between joint vectors.  A pick ends with a straight tool move from a
// pre-grasp pose into the grasp (a controller's LIN move); this unit asks, for every configuration inverse kinematics found for the
// pre-grasp, whether that move exists inside the joint ranges, without a joint flip and free of the line obstacles, and keeps per
// target the candidate nearest to a reference configuration whose line completes.  A glue bead or a weld seam is a chain of such moves:
// a polyline of tool poses per target, asked the same question as a whole.
//
// MI355X mapping: cfs_ik_kernel's.  One 64-lane wavefront owns one target, one lane one candidate; four targets per 256-thread
// workgroup; the robot, the obstacle rows and their margins are staged once per workgroup in LDS behind the only block barrier.  A
// lane's path is a sequential chain (step k starts where step k-1 ended) and lanes need different iteration counts per step, so the
// kernel is ONE loop whose pass is one damped least-squares iteration of the lane's current step (cfs_ik_dev.h: the contract's steps
// 1-8 literally); finishing a step (joint jump, collision, the next line point, lambda and `it` reset) is bookkeeping at the head of
// the same pass.  A wave therefore runs max over its lanes of the lanes' totals, not the sum over the steps of per-step maxima; the
// arithmetic of a lane is that of the nested form (for every step: restart from theta_{k-1}).  Lanes that have ended idle under the
// EXEC mask until a ballot says that none is running; the selection is IK's wave argmin on (cost, lane) by xor shuffles.  No atomics,
// no block barrier after the staging, no host round trip.  Everything is fp64; every loop over joints is unrolled at compile time.
// The start load, the pass and the epilogue are one text for both kinds of path; `if constexpr (POLY)` stands only where they differ.  A
// line's row 0 is the start itself and the lane holds the start's pose, the line's origin, for the whole run.  A polyline's row 0 is a
// pose to reach like every later row and is jump-tested against the start; the head of a pass reads the two poses of the lane's segment
// from the target's table (follow_row) and nothing of the path is held.  The outputs have one convention, K = rows - 1.
//
// Mesh obstacles (cfs_cart_path_mesh*).  The trace does not depend on collisions, so the meshes are tested BEHIND
// it on the same stream, in two more launches that read what it left in cand_path (the workspace between the launches):
//   cfs_cart_mesh_kernel<NJ, MESH>   one wavefront per (target, candidate), one wavefront per workgroup.  For the candidate's accepted
//                                    rows in ascending order: lane-uniform FK (ik_clearance<NJ, true> hands out the link ends, into LDS), then
//                                    the threshold test of cfs_mesh_hit_dev.h with the whole wave on that one pose (variant A, or
//                                    variant B with variant A deciding a pose whose frontier overflows).  The first hit ends the walk
//                                    and rewrites the candidate's outputs: state 2, done = max(m-1, 0), end = row m, rows >= m NaN.
//   cfs_cart_select_kernel<NJ>       one wavefront per target, one lane per candidate.  A candidate is complete when all K+1 rows of
//                                    its cand_path are numbers (accepted rows are a prefix and hold no NaN), so the states are read
//                                    off cand_path alone and the optional cand_status / cand_done need not exist.  Cost of the start,
//                                    the xor-shuffle argmin, then the winner's clearance: the (row, mesh, link) triples strided over
//                                    the lanes, one exact unbounded mesh_query each, a wave min with the line clearance of the rows.
// They run behind either instantiation of the trace.  The trace itself holds no mesh walk: at 256 VGPR + 249 AGPR for the line with
// NJ = 5 a hierarchy walk inside its pass would put the iteration in scratch.
//
// What the kernels here share with cfs_ik.hip is called, not restated: ik_stage, ik_converged, ik_cost, ik_argmin
// (cfs_ik_dev.h), mesh_hit, mesh_pair_clearance, mesh_wave_min (cfs_mesh_hit_dev.h) and the descriptor checks of cfs_tool_host.h.
#include "cfs_mesh_hit_dev.h"
#include "cfs_ik_dev.h"
#include "cfs_tool_host.h"

namespace {

constexpr int WV = 64;
constexpr int CART_WAVES = 4;                                 // targets per workgroup
constexpr int CART_MAX_STEPS = 256;
constexpr double CART_AXIS_MIN = 1e-6;                        // |(1-s)*a0 + s*target_axis| at or below this: the interpolated axis is undefined

struct CartParams {
    DevRobot rb;                                              // by value, as in IkParams: no device allocation in the _device entry
    int T, R, K, nobs, use_axis, max_iter;
    double tool[3], axis[3];                                  // axis normalised on the host
    double lo[6], hi[6], w[6];
    double tol_pos, tol_axis, max_joint_step;
    const double *obs, *D;                                    // nobs x 6, nobs
    const double *start;                                      // T x R x NJ
    const int *start_state;                                   // T x R or null
    const double *target_pos, *target_axis, *theta_ref;       // T x 3, T x 3 (use_axis), T x NJ
    double *theta;                                            // T x NJ
    int *status;                                              // T
    double *path;                                             // T x (K+1) x NJ
    int *selected, *n_ok, *n_done;                            // T
    double *clearance;                                        // T
    int *cand_status, *cand_done, *cand_iter;                 // T x R
    double *cand_end, *cand_path;                             // T x R x NJ, T x R x (K+1) x NJ
};

// (p_n, a_n) of row n >= 1 of a polyline, on segment i with ksub sub-steps: both poses of the segment are read from the target's table
// here, where they are needed, and not held (the table is the wave's, so lanes on the same segment read the same addresses).  False:
// the interpolated axis is undefined.
__device__ __forceinline__ bool follow_row(const double *pos, const double *axs, int n, int i, int ksub, bool use_axis, double *pk, double *ak)
{
    const double s = (double)(n - i * ksub) / (double)ksub;
#pragma unroll
    for (int q = 0; q < 3; ++q) pk[q] = pos[i * 3 + q] + s * (pos[i * 3 + 3 + q] - pos[i * 3 + q]);
    if (!use_axis) return true;
    double u[3], v[3], b[3];
#pragma unroll
    for (int q = 0; q < 3; ++q) { u[q] = axs[i * 3 + q]; v[q] = axs[i * 3 + 3 + q]; }
    const double un = sqrt(u[0] * u[0] + u[1] * u[1] + u[2] * u[2]), vn = sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
#pragma unroll
    for (int q = 0; q < 3; ++q) b[q] = (1.0 - s) * (u[q] / un) + s * (v[q] / vn);
    const double bn = sqrt(b[0] * b[0] + b[1] * b[1] + b[2] * b[2]);
    if (!(bn > CART_AXIS_MIN)) return false;
    ak[0] = b[0] / bn; ak[1] = b[1] / bn; ak[2] = b[2] / bn;
    return true;
}

// the start's own pose, a line's origin: the line instantiation holds it for the whole run, the polyline's has none
template <bool POLY> struct CartOrigin { double p[3] = {0.0, 0.0, 0.0}, a[3] = {0.0, 0.0, 0.0}; };
template <> struct CartOrigin<true> {};

// The trace of both entries.  A path has P.K + 1 rows; a lane keeps the pose (pk, ak) of the row it works on and the number of rows it
// has written.  POLY false, the straight line of cfs_cart_path*: P.target_pos / P.target_axis are T x 3, row 0 is the start itself
// (its residual is zero, so the first pass books it) and the lane holds the start's pose, the line's origin o, for the whole run;
// ksub is not read.  POLY true, the polyline of cfs_cart_follow*: they are the tables (T x M x 3), ksub the sub-steps of a segment,
// row 0 a pose to reach like every later row (jump-tested against the start), and nothing of the path is held: the lane keeps its segment.
template <int NJ, bool POLY>
__global__ __launch_bounds__(WV * CART_WAVES) void cfs_cart_kernel(const CartParams P, const int ksub)
{
    __shared__ __attribute__((aligned(16))) double s_rb[sizeof(DevRobot) / 8];
    __shared__ double s_obs[CFS_MAX_OBS * 6];
    __shared__ double s_D[CFS_MAX_OBS];
    // the only block barrier is in there: whole waves may leave after it
    const DevRobot *rb = ik_stage<WV * CART_WAVES>(P.rb, s_rb, P.nobs, P.obs, P.D, s_obs, s_D);
    const int lane = threadIdx.x % WV, t = blockIdx.x * CART_WAVES + threadIdx.x / WV;
    if (t >= P.T) return;
    const bool use_axis = P.use_axis != 0;
    const bool active = lane < P.R;                           // lanes >= candidates never run and enter the reductions with neutral values
    const size_t row = (size_t)t * P.R + (active ? lane : 0);
    const size_t prow = row * (size_t)(P.K + 1);              // the candidate's first row of cand_path
    size_t tab = (size_t)t * 3;                               // the target's row of target_pos / target_axis,
    if constexpr (POLY) tab *= (size_t)(P.K / ksub + 1);      // or its first row of the two tables

    double th[NJ];
    int st = 5;                                               // -1: running
    if (active) {
        bool ok = !P.start_state || P.start_state[row] == 0;
#pragma unroll
        for (int c = 0; c < NJ; ++c) {
            th[c] = P.start[row * NJ + c];
            ok = ok && th[c] >= P.lo[c] && th[c] <= P.hi[c];  // false for a NaN and for +-inf
        }
        if (ok) st = -1;
    }
    if (st != -1) {
#pragma unroll
        for (int c = 0; c < NJ; ++c) th[c] = __builtin_nan("");
    }

    double pk[3] = {0.0, 0.0, 0.0}, ak[3] = {0.0, 0.0, 0.0}, prev[NJ], r[6], F = 0.0, A[NJ * NJ], g[NJ];
    [[maybe_unused]] CartOrigin<POLY> o;
    double lam = IK_LAMBDA0, cmin = INFINITY;
    int it = 0, itsum = 0, seg = 0, nrow = 0;                 // nrow: rows of cand_path written = the row the lane works on; seg: POLY
#pragma unroll
    for (int q = 0; q < 6; ++q) r[q] = 0.0;
#pragma unroll
    for (int c = 0; c < NJ; ++c) { prev[c] = th[c]; g[c] = 0.0; }
#pragma unroll
    for (int q = 0; q < NJ * NJ; ++q) A[q] = 0.0;
    if constexpr (!POLY) {
        // row 0 is the start itself: its pose is its own, so its residual is zero and the first pass books it (collision test, row 0
        // of the path; the jump test against itself passes) like every later row
        if (st < 0) {
            double tw[NJ * 6];
            ik_pose<NJ>(rb, P.tool, P.axis, th, o.p, o.a, tw);
        }
#pragma unroll
        for (int q = 0; q < 3; ++q) { pk[q] = o.p[q]; ak[q] = o.a[q]; }
    } else if (st < 0) {
        // row 0 is (P_0, A_0 normalised): set up from the start like any later row from the row before it
#pragma unroll
        for (int q = 0; q < 3; ++q) pk[q] = P.target_pos[tab + q];
        if (use_axis) {
#pragma unroll
            for (int q = 0; q < 3; ++q) ak[q] = P.target_axis[tab + q];
            const double an = sqrt(ak[0] * ak[0] + ak[1] * ak[1] + ak[2] * ak[2]);
            ak[0] /= an; ak[1] /= an; ak[2] /= an;            // a zero or non-finite row: NaN, which step 1 turns into state 3
        }
        double p[3], a[3], tw[NJ * 6];
        ik_pose<NJ>(rb, P.tool, P.axis, th, p, a, tw);
        ik_residual(p, a, pk, ak, use_axis, r, &F);
        ik_normal<NJ>(tw, p, a, r, use_axis, A, g);
    }

    for (;;) {
        // ---- head of the pass: a row whose pose is reached is booked and the next one set up --------------------------------
        if (st < 0) {
            if (!(F < INFINITY)) st = 3;                                                        // step 1
            else if (ik_converged(r, use_axis, P.tol_pos, P.tol_axis)) {                        // step 2: theta_n = th
                double s = 0.0;
#pragma unroll
                for (int c = 0; c < NJ; ++c) s = fabs(th[c] - prev[c]) > s ? fabs(th[c] - prev[c]) : s;
                if (s > P.max_joint_step) st = 4;                                               // row 0: against the start (a line's: itself)
                if (st < 0) {
                    const double c = ik_clearance<NJ>(rb, th, P.nobs, s_obs, s_D);
                    if (!(c >= 0.0)) st = 2;
                    else if (c < cmin) cmin = c;
                }
                if (st < 0) {
                    if (P.cand_path) {
#pragma unroll
                        for (int c = 0; c < NJ; ++c) P.cand_path[(prow + nrow) * NJ + c] = th[c];
                    }
                    if (nrow == P.K) { st = 0; ++nrow; }
                    else {
                        ++nrow;
                        // the poses are read again at every row rather than held: twelve registers the iteration needs
                        if constexpr (!POLY) {
                            const double s = (double)nrow / (double)P.K;
#pragma unroll
                            for (int q = 0; q < 3; ++q) pk[q] = o.p[q] + s * (P.target_pos[tab + q] - o.p[q]);
                            if (use_axis) {
                                double ta[3], b[3];
#pragma unroll
                                for (int q = 0; q < 3; ++q) ta[q] = P.target_axis[tab + q];
                                const double tn = sqrt(ta[0] * ta[0] + ta[1] * ta[1] + ta[2] * ta[2]);
#pragma unroll
                                for (int q = 0; q < 3; ++q) b[q] = (1.0 - s) * o.a[q] + s * (ta[q] / tn);
                                const double n = sqrt(b[0] * b[0] + b[1] * b[1] + b[2] * b[2]);
                                if (!(n > CART_AXIS_MIN)) st = 3;
                                else { ak[0] = b[0] / n; ak[1] = b[1] / n; ak[2] = b[2] / n; }
                            }
                        } else {
                            if (nrow - seg * ksub > ksub) ++seg;                                // row nrow lies on segment (nrow-1) div ksub
                            if (!follow_row(P.target_pos + tab, P.target_axis + tab, nrow, seg, ksub, use_axis, pk, ak)) st = 3;
                        }
                        if (st < 0) {                                                           // the restart of row nrow from theta_{nrow-1}
                            double p[3], a[3], tw[NJ * 6];
#pragma unroll
                            for (int c = 0; c < NJ; ++c) prev[c] = th[c];
                            ik_pose<NJ>(rb, P.tool, P.axis, th, p, a, tw);
                            ik_residual(p, a, pk, ak, use_axis, r, &F);
                            ik_normal<NJ>(tw, p, a, r, use_axis, A, g);
                            lam = IK_LAMBDA0;
                            it = 0;
                        }
                    }
                }
            }
        }
        if (__ballot(st < 0) == 0ull) break;
        // ---- one iteration of the current row (a row set up above is tested before it iterates) -----------------------------
        if (st < 0) {
            if (!(F < INFINITY)) st = 3;                                                        // step 1
            else if (ik_converged(r, use_axis, P.tol_pos, P.tol_axis)) {}                       // step 2: the next pass books it
            else if (it >= P.max_iter) st = 1;                                                  // step 3
            else {                                                                              // cfs_ik_kernel's steps 4-8, statement for statement
                double delta[NJ], trial[NJ];
                if (!ik_solve_step<NJ>(A, g, lam, delta)) st = 3;                               // step 4
                else {
                    double s = 0.0;
#pragma unroll
                    for (int c = 0; c < NJ; ++c) s = fabs(delta[c]) > s ? fabs(delta[c]) : s;
                    const double sc = s > IK_STEP_CAP ? IK_STEP_CAP / s : 1.0;                  // step 5
#pragma unroll
                    for (int c = 0; c < NJ; ++c) {
                        const double x = th[c] + (s > IK_STEP_CAP ? delta[c] * sc : delta[c]);
                        trial[c] = x < P.lo[c] ? P.lo[c] : (x > P.hi[c] ? P.hi[c] : x);        // step 6
                    }
                    double p2[3], a2[3], tw2[NJ * 6], r2[6], F2;
                    ik_pose<NJ>(rb, P.tool, P.axis, trial, p2, a2, tw2);
                    ik_residual(p2, a2, pk, ak, use_axis, r2, &F2);
                    if (F2 < F) {                                                               // step 7
#pragma unroll
                        for (int c = 0; c < NJ; ++c) th[c] = trial[c];
#pragma unroll
                        for (int q = 0; q < 6; ++q) r[q] = r2[q];
                        F = F2;
                        ik_normal<NJ>(tw2, p2, a2, r2, use_axis, A, g);
                        lam = lam / 10.0 > IK_LAMBDA_MIN ? lam / 10.0 : IK_LAMBDA_MIN;
                    } else {
                        lam = lam * 10.0 < IK_LAMBDA_MAX ? lam * 10.0 : IK_LAMBDA_MAX;
                    }
                    ++it; ++itsum;                                                              // step 8
                }
            }
        }
    }

    // ---- cost of the START, candidate outputs, selection -------------------------------------------------------------------
    const double nan = __builtin_nan("");
    double cost = INFINITY;
    if (st == 0) {
        const double s = ik_cost<NJ>(P.w, P.start + row * NJ, P.theta_ref + (size_t)t * NJ);
        if (s < INFINITY) cost = s; else st = 3;
    }
    int md = nrow > 1 ? nrow - 1 : 0;                         // the last accepted row
    if (active) {
        if (P.cand_status) P.cand_status[row] = st;
        if (P.cand_done) P.cand_done[row] = md;
        if (P.cand_iter) P.cand_iter[row] = itsum;
        if (P.cand_end) {
#pragma unroll
            for (int c = 0; c < NJ; ++c) P.cand_end[row * NJ + c] = th[c];
        }
        if (P.cand_path) {
            for (size_t e = (prow + nrow) * NJ; e < (prow + P.K + 1) * NJ; ++e) P.cand_path[e] = nan;
        }
    }
    const int n_ok = __popcll(__ballot(st == 0));
    const bool any_start = __ballot(st != 5) != 0ull;
    const int bl = ik_argmin<true>(cost, lane, &md);
    const bool ok = n_ok > 0;
    if (ok ? lane == bl : lane == 0) {
#pragma unroll
        for (int c = 0; c < NJ; ++c) P.theta[(size_t)t * NJ + c] = ok ? P.start[row * NJ + c] : nan;
        P.status[t] = ok ? 0 : (any_start ? 1 : 2);
        if (P.selected) P.selected[t] = ok ? lane : -1;
        if (P.n_ok) P.n_ok[t] = n_ok;
        if (P.n_done) P.n_done[t] = md;
        if (P.clearance) P.clearance[t] = ok ? cmin : nan;
    }
    if (P.path) {
        // the winner's rows of cand_path (the launch's workspace), copied by the whole wave: the fence makes the winner's stores
        // visible to the other lanes of its wave
        const size_t n = (size_t)(P.K + 1) * NJ;
        double *dst = P.path + (size_t)t * n;
        if (ok) {
            __threadfence();
            const double *src = P.cand_path + ((size_t)t * P.R + bl) * n;
            for (size_t e = lane; e < n; e += WV) dst[e] = src[e];
        } else {
            for (size_t e = lane; e < n; e += WV) dst[e] = nan;
        }
    }
}

// ksub == 0: the straight line of cfs_cart_path; otherwise the polyline with ksub sub-steps per segment
hipError_t launch_cart(int nj, const CartParams &p, int ksub, hipStream_t s)
{
    return cfs_for_nj(nj, [&](auto N) {
        constexpr int NJ = decltype(N)::value;
        const dim3 grid((p.T + CART_WAVES - 1) / CART_WAVES), block(WV * CART_WAVES);
        if (ksub) hipLaunchKernelGGL((cfs_cart_kernel<NJ, true>), grid, block, 0, s, p, ksub);
        else hipLaunchKernelGGL((cfs_cart_kernel<NJ, false>), grid, block, 0, s, p, ksub);
        return hipGetLastError();
    });
}

// ---- mesh obstacles behind the trace -----------------------------------------------------------------------------------------
// dynamic LDS of a mesh wave: the private stacks of variant A and of the exact queries (MESH_STACK*64 ints + as many floats = 10 KB),
// then variant B's frontier (RRT_FRONTIER_CAP pairs + as many nodes = 4 KB)
constexpr int CART_STACK_WORDS = 2 * MESH_STACK * WV, CART_FRONTIER_WORDS = 2 * RRT_FRONTIER_CAP;

struct CartMeshArgs {
    CartParams P;
    ToolMeshArgs M;                                           // the mesh table of a cfs_cart_path_mesh* call
};

// poses of variant B whose frontier overflowed and that variant A decided (cfs_debug_cart_frontier_overflows): one vector atomic by
// lane 0 per such pose, none on the normal path
__device__ unsigned long long g_cart_frontier_overflows = 0ull;

// one wavefront = one workgroup = one (target, candidate); everything below is wave-uniform
template <int NJ, int MESH>
__global__ __launch_bounds__(WV) void cfs_cart_mesh_kernel(const CartMeshArgs A_)
{
    const CartParams &P = A_.P;
    __shared__ __attribute__((aligned(16))) double s_rb[sizeof(DevRobot) / 8];
    __shared__ double s_ends[NJ * 6];                         // the pose's link ends: wave-uniform, so they need no registers
    extern __shared__ __attribute__((aligned(16))) int s_mesh[];
    const DevRobot *rb = ik_stage<WV>(P.rb, s_rb);
    const int lane = threadIdx.x;
    const size_t row = blockIdx.x;                            // t * R + r; the grid is exactly T * R
    const size_t prow = row * (size_t)(P.K + 1);
    int *s_stack = s_mesh;
    float *s_lbs = reinterpret_cast<float *>(s_stack + MESH_STACK * WV);
    int *s_fpair = s_mesh + CART_STACK_WORDS, *s_fnode = s_fpair + RRT_FRONTIER_CAP;
    const RrtMeshArgs &MA = A_.M.MA;

    for (int k = 0; k <= P.K; ++k) {
        double th[NJ];
        double *ends = s_ends;
#pragma unroll
        for (int c = 0; c < NJ; ++c) th[c] = P.cand_path[(prow + k) * NJ + c];     // one address for the wave
        if (th[0] != th[0]) return;                           // the accepted rows are a prefix: nothing after the first NaN row
        ik_clearance<NJ, true>(rb, th, 0, nullptr, nullptr, ends);                 // every lane stores the same values and reads its own
        if (!mesh_hit<NJ, MESH>(MA, ends, lane, s_stack, s_lbs, s_fpair, s_fnode, &g_cart_frontier_overflows)) continue;
        // row k is the first mesh-rejected row: state 2, as for a line collision at step k
        if (lane == 0) {
            if (P.cand_status) P.cand_status[row] = 2;
            if (P.cand_done) P.cand_done[row] = k > 0 ? k - 1 : 0;
            if (P.cand_end) {
#pragma unroll
                for (int c = 0; c < NJ; ++c) P.cand_end[row * NJ + c] = th[c];
            }
        }
        const double nan = __builtin_nan("");
        for (size_t e = (prow + k) * NJ + lane; e < (prow + P.K + 1) * NJ; e += WV) P.cand_path[e] = nan;
        return;
    }
}

template <int NJ>
__global__ __launch_bounds__(WV) void cfs_cart_select_kernel(const CartMeshArgs A_)
{
    const CartParams &P = A_.P;
    __shared__ __attribute__((aligned(16))) double s_rb[sizeof(DevRobot) / 8];
    __shared__ double s_obs[CFS_MAX_OBS * 6];
    __shared__ double s_D[CFS_MAX_OBS];
    extern __shared__ __attribute__((aligned(16))) int s_mesh[];
    const DevRobot *rb = ik_stage<WV>(P.rb, s_rb, P.nobs, P.obs, P.D, s_obs, s_D);
    const int lane = threadIdx.x, t = blockIdx.x;
    const bool active = lane < P.R;
    const size_t row = (size_t)t * P.R + (active ? lane : 0);
    const size_t prow = row * (size_t)(P.K + 1);
    const double nan = __builtin_nan("");

    // the candidate's state, read off its inputs and its rows of cand_path: no start (the trace's test) | accepted rows
    bool has_start = false;
    int nrow = 0;
    double cost = INFINITY;
    if (active) {
        has_start = !P.start_state || P.start_state[row] == 0;
#pragma unroll
        for (int c = 0; c < NJ; ++c) {
            const double v = P.start[row * NJ + c];
            has_start = has_start && v >= P.lo[c] && v <= P.hi[c];
        }
        if (has_start) {
            for (int k = 0; k <= P.K; ++k) {
                const double v = P.cand_path[(prow + k) * NJ];
                if (v != v) break;
                ++nrow;
            }
        }
        if (nrow == P.K + 1) {
            const double s = ik_cost<NJ>(P.w, P.start + row * NJ, P.theta_ref + (size_t)t * NJ);      // cfs_cart_kernel's cost
            if (s < INFINITY) cost = s;
        }
    }
    const bool good = cost < INFINITY;
    const int n_ok = __popcll(__ballot(good));
    const bool any_start = __ballot(has_start) != 0ull;
    int md = nrow > 1 ? nrow - 1 : 0;
    const int bl = ik_argmin<true>(cost, lane, &md);
    const bool ok = n_ok > 0;
    const size_t n = (size_t)(P.K + 1) * NJ;
    const double *src = P.cand_path + ((size_t)t * P.R + (ok ? bl : 0)) * n;

    // the winner's clearance: triple = (row, mesh, link), one exact unbounded query each; the lane that holds a row's first triple
    // also takes the row's line clearance
    double mm = INFINITY;
    if (ok && P.clearance) {
        int *s_stack = s_mesh;
        float *s_lbs = reinterpret_cast<float *>(s_stack + MESH_STACK * WV);
        const RrtMeshArgs &MA = A_.M.MA;
        const int per = MA.nmesh * NJ, ntrip = (P.K + 1) * per;
        for (int q = lane; q < ntrip; q += WV) {
            const int k = q / per, pr = q - k * per;
            double th[NJ], ends[NJ * 6];
#pragma unroll
            for (int c = 0; c < NJ; ++c) th[c] = src[(size_t)k * NJ + c];
            const double cl = ik_clearance<NJ, true>(rb, th, pr == 0 ? P.nobs : 0, s_obs, s_D, ends);
            if (cl < mm) mm = cl;
            const double v = mesh_pair_clearance<NJ>(MA, A_.M.D, ends, pr, s_stack + lane, s_lbs + lane);
            if (v < mm) mm = v;
        }
        mm = mesh_wave_min(mm);
    }
    if (lane == 0) {
#pragma unroll
        for (int c = 0; c < NJ; ++c) P.theta[(size_t)t * NJ + c] = ok ? P.start[((size_t)t * P.R + bl) * NJ + c] : nan;
        P.status[t] = ok ? 0 : (any_start ? 1 : 2);
        if (P.selected) P.selected[t] = ok ? bl : -1;
        if (P.n_ok) P.n_ok[t] = n_ok;
        if (P.n_done) P.n_done[t] = md;
        if (P.clearance) P.clearance[t] = ok ? mm : nan;
    }
    if (P.path) {
        double *dst = P.path + (size_t)t * n;
        for (size_t e = lane; e < n; e += WV) dst[e] = ok ? src[e] : nan;
    }
}

size_t cart_mesh_lds_bytes(int variant) { return (size_t)(CART_STACK_WORDS + (variant == RRT_MESH_WAVE ? CART_FRONTIER_WORDS : 0)) * 4; }

// the two launches behind the trace
hipError_t launch_cart_mesh(int nj, int variant, const CartMeshArgs &a, hipStream_t s)
{
    if (variant != RRT_MESH_PER_LANE && variant != RRT_MESH_WAVE) return hipErrorInvalidValue;
    return cfs_for_nj(nj, [&](auto N) {
        constexpr int NJ = decltype(N)::value;
        const dim3 grid((unsigned)((size_t)a.P.T * a.P.R));
        if (variant == RRT_MESH_PER_LANE)
            hipLaunchKernelGGL((cfs_cart_mesh_kernel<NJ, RRT_MESH_PER_LANE>), grid, dim3(WV), cart_mesh_lds_bytes(variant), s, a);
        else
            hipLaunchKernelGGL((cfs_cart_mesh_kernel<NJ, RRT_MESH_WAVE>), grid, dim3(WV), cart_mesh_lds_bytes(variant), s, a);
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(cfs_cart_select_kernel<NJ>, dim3(a.P.T), dim3(WV), cart_mesh_lds_bytes(RRT_MESH_PER_LANE), s, a);
        return hipGetLastError();
    });
}

// ---- C ABI (include/cfs_hip.h, "Cartesian paths", "Tool paths") -------------------------------------------------------------------
// Every entry comes through the functions below.  `npts` is the optional path table: nullptr for the straight line of cfs_cart_path*
// (target_pos / target_axis are T x 3), else the number M of poses of cfs_cart_follow*'s polylines (they are the T x M x 3 tables
// path_pos / path_axis, and a path has (M-1)*steps + 1 rows).
const char *cart_pos_name(const int *npts) { return npts ? "path_pos" : "target_pos"; }
const char *cart_axis_name(const int *npts) { return npts ? "path_axis" : "target_axis"; }

// everything of a call that is host memory in both entries (cfs_tool_host.h); fills the by-value part of the kernel's parameter block
int check_cart(const cfs_cart_desc *d, const int *npts, int T, const double *start, const double *target_pos, const double *target_axis,
               const double *theta_ref, const cfs_cart_out *out, CartParams &P)
{
    int rc = check_tool_head(d);
    if (rc) return rc;
    if (d->candidates < 1 || d->candidates > WV) return cfs_fail(CFS_ERR_INVALID_ARG, "candidates %d outside 1..%d", d->candidates, WV);
    if (d->steps < 1 || d->steps > CART_MAX_STEPS) return cfs_fail(CFS_ERR_INVALID_ARG, "steps %d outside 1..%d", d->steps, CART_MAX_STEPS);
    if (npts && (*npts < 2 || *npts > CART_MAX_STEPS + 1)) return cfs_fail(CFS_ERR_INVALID_ARG, "npts %d outside 2..%d", *npts, CART_MAX_STEPS + 1);
    if (npts && (*npts - 1) * d->steps > CART_MAX_STEPS)
        return cfs_fail(CFS_ERR_INVALID_ARG, "(npts-1)*steps = %d: a path has at most %d rows after row 0", (*npts - 1) * d->steps, CART_MAX_STEPS);
    if ((rc = check_tool_max_iter(d->max_iter))) return rc;
    if (!(std::isfinite(d->max_joint_step) && d->max_joint_step > 0.0)) return cfs_fail(CFS_ERR_INVALID_ARG, "max_joint_step must be finite and > 0");
    if ((rc = check_tool_fields(d, T))) return rc;
    if (!start || !target_pos || !theta_ref) return cfs_fail(CFS_ERR_INVALID_ARG, "NULL start / %s / theta_ref", cart_pos_name(npts));
    if ((rc = check_tool_io(d, target_axis, out, cart_axis_name(npts)))) return rc;
    fill_tool_params(d, T, P);
    P.R = d->candidates; P.K = npts ? (*npts - 1) * d->steps : d->steps; P.max_joint_step = d->max_joint_step;
    return CFS_SUCCESS;
}

void cart_point(CartParams &P, const double *obs, const double *D, const double *start, const int *start_state, const double *target_pos,
                const double *target_axis, const double *theta_ref, const cfs_cart_out *o)
{
    P.obs = obs; P.D = D; P.start = start; P.start_state = start_state;
    P.target_pos = target_pos; P.target_axis = target_axis; P.theta_ref = theta_ref;
    P.theta = o->theta; P.status = o->status; P.path = o->path; P.selected = o->selected; P.n_ok = o->n_ok; P.n_done = o->n_done;
    P.clearance = o->clearance; P.cand_status = o->cand_status; P.cand_done = o->cand_done; P.cand_iter = o->cand_iter;
    P.cand_end = o->cand_end; P.cand_path = o->cand_path;
}

// the trace, then (mc given) the mesh walk and the selection over it, all on stream s.  The trace's own selection would only be
// overwritten, so it is not asked for: its optional target outputs are withheld from the first launch.
hipError_t launch_cart_all(int nj, int variant, CartMeshArgs &a, int ksub, bool mesh, hipStream_t s)
{
    if (!mesh) return launch_cart(nj, a.P, ksub, s);
    CartParams first = a.P;
    first.path = nullptr; first.selected = nullptr; first.n_ok = nullptr; first.n_done = nullptr; first.clearance = nullptr;
    const hipError_t e = launch_cart(nj, first, ksub, s);
    return e != hipSuccess ? e : launch_cart_mesh(nj, variant, a, s);
}

// mc == nullptr: the line-only call
int cart_device(const cfs_cart_desc *d, const MeshCall *mc, const int *npts, int T, const double *start, const int *start_state, const double *target_pos,
                const double *target_axis, const double *theta_ref, const cfs_cart_out *out, void *stream)
{
    static_assert(sizeof(CartParams) <= 4096, "the parameter block travels as a kernel argument");
    static_assert(sizeof(CartMeshArgs) <= 4096, "the parameter block and the mesh table travel as a kernel argument");
    CartMeshArgs A;
    int rc = check_cart(d, npts, T, start, target_pos, target_axis, theta_ref, out, A.P);
    if (rc) return rc;
    int variant = RRT_MESH_NONE;
    if (mc) {
        rc = check_mesh_call(d->nobs, *mc, CART_MESH_DEFAULT, A.M, variant);
        if (rc) return rc;
        if (!out->cand_path)
            return cfs_fail(CFS_ERR_INVALID_ARG, "%s: out->cand_path must be given, the workspace between the launches (nothing is allocated here)",
                            npts ? "cfs_cart_follow_mesh_device" : "cfs_cart_path_mesh_device");
    } else if (out->path && !out->cand_path)
        return cfs_fail(CFS_ERR_INVALID_ARG, "%s: out->path needs out->cand_path, the launch's workspace (nothing is allocated here)",
                        npts ? "cfs_cart_follow_device" : "cfs_cart_path_device");
    rc = cfs_use_device(cfs_current_device());
    if (rc) return rc;
    cart_point(A.P, d->obs, d->D, start, start_state, target_pos, target_axis, theta_ref, out);
    const hipError_t e = launch_cart_all(d->njoint, variant, A, npts ? d->steps : 0, mc != nullptr, reinterpret_cast<hipStream_t>(stream));
    if (e != hipSuccess) return cfs_fail(CFS_ERR_HIP, "Cartesian path launch failed: %s", hipGetErrorString(e));
    return CFS_SUCCESS;
}

int cart_host(const cfs_cart_desc *d, const MeshCall *mc, const int *npts, int T, const double *start, const int *start_state, const double *target_pos,
              const double *target_axis, const double *theta_ref, const cfs_cart_out *out)
{
    CartMeshArgs A;
    CartParams &P = A.P;
    int rc = check_cart(d, npts, T, start, target_pos, target_axis, theta_ref, out, P);
    if (rc) return rc;
    int variant = RRT_MESH_NONE;
    if (mc) {   // refuse before anything is staged on the device
        rc = check_mesh_call(d->nobs, *mc, CART_MESH_DEFAULT, A.M, variant);
        if (rc) return rc;
    }
    const size_t nj = d->njoint, R = d->candidates, K1 = (size_t)P.K + 1, nobs = d->nobs, nT = T, M = npts ? *npts : 1;
    rc = check_tool_arrays(d, T, target_pos, target_axis, theta_ref, M, cart_pos_name(npts), cart_axis_name(npts));
    if (rc) return rc;
    rc = cfs_use_device(cfs_current_device());
    if (rc) return rc;
    Stage st;
    cfs_cart_out o;
    memset(&o, 0, sizeof o);
    const double *obs_d = st.up(d->obs, nobs * 6), *D_d = st.up(d->D, nobs), *s_d = st.up(start, nT * R * nj);
    const int *ss_d = start_state ? st.up(start_state, nT * R) : nullptr;
    const double *tp_d = st.up(target_pos, nT * M * 3);
    const double *ta_d = d->use_axis ? st.up(target_axis, nT * M * 3) : nullptr;
    const double *tr_d = st.up(theta_ref, nT * nj);
    o.theta = st.out<double>(nT * nj); o.status = st.out<int>(nT);
    if (out->path) o.path = st.out<double>(nT * K1 * nj);
    if (out->selected) o.selected = st.out<int>(nT);
    if (out->n_ok) o.n_ok = st.out<int>(nT);
    if (out->n_done) o.n_done = st.out<int>(nT);
    if (out->clearance) o.clearance = st.out<double>(nT);
    if (out->cand_status) o.cand_status = st.out<int>(nT * R);
    if (out->cand_done) o.cand_done = st.out<int>(nT * R);
    if (out->cand_iter) o.cand_iter = st.out<int>(nT * R);
    if (out->cand_end) o.cand_end = st.out<double>(nT * R * nj);
    if (out->cand_path || out->path || mc) o.cand_path = st.out<double>(nT * R * K1 * nj);     // also the workspace behind `path` and between the launches
    if (st.err == hipSuccess) {
        cart_point(P, obs_d, D_d, s_d, ss_d, tp_d, ta_d, tr_d, &o);
        st.err = launch_cart_all(d->njoint, variant, A, npts ? d->steps : 0, mc != nullptr, nullptr);
        if (st.err == hipSuccess) st.err = hipStreamSynchronize(nullptr);
    }
    st.down(out->theta, o.theta, nT * nj); st.down(out->status, o.status, nT); st.down(out->path, o.path, nT * K1 * nj);
    st.down(out->selected, o.selected, nT); st.down(out->n_ok, o.n_ok, nT); st.down(out->n_done, o.n_done, nT);
    st.down(out->clearance, o.clearance, nT);
    st.down(out->cand_status, o.cand_status, nT * R); st.down(out->cand_done, o.cand_done, nT * R); st.down(out->cand_iter, o.cand_iter, nT * R);
    st.down(out->cand_end, o.cand_end, nT * R * nj); st.down(out->cand_path, o.cand_path, nT * R * K1 * nj);
    return st.result("Cartesian path staging or launch");
}
}  // namespace

extern "C" int cfs_cart_path_device(const cfs_cart_desc *d, int T, const double *start, const int *start_state, const double *target_pos,
                                    const double *target_axis, const double *theta_ref, const cfs_cart_out *out, void *stream)
{
    return cart_device(d, nullptr, nullptr, T, start, start_state, target_pos, target_axis, theta_ref, out, stream);
}

extern "C" int cfs_cart_path(const cfs_cart_desc *d, int T, const double *start, const int *start_state, const double *target_pos,
                             const double *target_axis, const double *theta_ref, const cfs_cart_out *out)
{
    return cart_host(d, nullptr, nullptr, T, start, start_state, target_pos, target_axis, theta_ref, out);
}

extern "C" int cfs_cart_path_mesh_device(const cfs_cart_desc *d, int nmesh, const cfs_mesh *const *meshes, const double *D_mesh, int flags, int T,
                                         const double *start, const int *start_state, const double *target_pos, const double *target_axis,
                                         const double *theta_ref, const cfs_cart_out *out, void *stream)
{
    const MeshCall mc{nmesh, meshes, D_mesh, flags};
    return cart_device(d, &mc, nullptr, T, start, start_state, target_pos, target_axis, theta_ref, out, stream);
}

extern "C" int cfs_cart_path_mesh(const cfs_cart_desc *d, int nmesh, const cfs_mesh *const *meshes, const double *D_mesh, int flags, int T,
                                  const double *start, const int *start_state, const double *target_pos, const double *target_axis,
                                  const double *theta_ref, const cfs_cart_out *out)
{
    const MeshCall mc{nmesh, meshes, D_mesh, flags};
    return cart_host(d, &mc, nullptr, T, start, start_state, target_pos, target_axis, theta_ref, out);
}

// ---- tool paths (include/cfs_hip.h, "Tool paths"): the same two functions with the path table ---------------------------------------
extern "C" int cfs_cart_follow_device(const cfs_cart_desc *d, int T, int npts, const double *start, const int *start_state, const double *path_pos,
                                      const double *path_axis, const double *theta_ref, const cfs_cart_out *out, void *stream)
{
    return cart_device(d, nullptr, &npts, T, start, start_state, path_pos, path_axis, theta_ref, out, stream);
}

extern "C" int cfs_cart_follow(const cfs_cart_desc *d, int T, int npts, const double *start, const int *start_state, const double *path_pos,
                               const double *path_axis, const double *theta_ref, const cfs_cart_out *out)
{
    return cart_host(d, nullptr, &npts, T, start, start_state, path_pos, path_axis, theta_ref, out);
}

extern "C" int cfs_cart_follow_mesh_device(const cfs_cart_desc *d, int nmesh, const cfs_mesh *const *meshes, const double *D_mesh, int flags, int T,
                                           int npts, const double *start, const int *start_state, const double *path_pos, const double *path_axis,
                                           const double *theta_ref, const cfs_cart_out *out, void *stream)
{
    const MeshCall mc{nmesh, meshes, D_mesh, flags};
    return cart_device(d, &mc, &npts, T, start, start_state, path_pos, path_axis, theta_ref, out, stream);
}

extern "C" int cfs_cart_follow_mesh(const cfs_cart_desc *d, int nmesh, const cfs_mesh *const *meshes, const double *D_mesh, int flags, int T, int npts,
                                    const double *start, const int *start_state, const double *path_pos, const double *path_axis,
                                    const double *theta_ref, const cfs_cart_out *out)
{
    const MeshCall mc{nmesh, meshes, D_mesh, flags};
    return cart_host(d, &mc, &npts, T, start, start_state, path_pos, path_axis, theta_ref, out);
}

extern "C" int cfs_debug_cart_frontier_overflows(unsigned long long *count, int reset)
{
    return cfs_frontier_overflows(&g_cart_frontier_overflows, count, reset);
}
