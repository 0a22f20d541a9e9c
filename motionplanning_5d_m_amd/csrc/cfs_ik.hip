// cfs_ik.hip -- batched collision-aware inverse kinematics (include/cfs_hip.h, "inverse kinematics").
//
// The reference has no inverse kinematics: its drivers type the goal in as a joint vector (xg, main_FANUC.m:30, RRTstar_CFS.m:43).
// What it does define is used as it is: the chain of CapPos.m:13-20 / CapPos2.m:19-28 (fk_step), the end effector
// all_ee = pos{nstate}.p(:,1) (Lib/RRT_FANUC.m:186), feasible() (Lib/RRT_FANUC.m:146-181) and the joint ranges robot.thetamax.
//
// MI355X mapping.  One 64-lane wavefront owns one target, one lane one restart of a damped least-squares (Levenberg-Marquardt)
// iteration, the contract's steps 1-8 literally.  A lane keeps theta, the 3x4 chain, the 6 x NJ Jacobian, the NJ x NJ normal
// matrix and its Cholesky factor in registers (every loop over joints is unrolled at compile time: NJ is a template parameter);
// the robot, the obstacle rows and their margins are staged once per workgroup (4 waves = 4 targets) in LDS.  Restarts of one
// target end at different iterations: a lane that has ended idles under the EXEC mask until a ballot says that none is running,
// so every lane reaches the selection, a wave argmin on (cost, lane) by xor shuffles.  No atomics, no block barrier after the
// staging, no host round trip.  Everything is fp64.  The staging, the convergence test, the cost and the argmin are
// cfs_ik_dev.h's (ik_stage, ik_converged, ik_cost, ik_argmin), the same functions cfs_cart.hip runs; the mesh decision and the winner's
// mesh clearance are cfs_mesh_hit_dev.h's (mesh_hit, mesh_pair_clearance); the checks of the descriptor are cfs_tool_host.h's.
//
// Mesh obstacles (cfs_ik_solve_mesh*).  cfs_ik_kernel<NJ, MESH> with MESH != RRT_MESH_NONE puts the decision of
// cfs_rrt_grow_mesh between the line test and the cost: a restart that converged and passed the lines takes state 2 when some
// triangle of some mesh j lies strictly closer than thr_j = max(D_mesh[j], 1e-4) to some link axis.  A lane holds one candidate
// pose, but the traversals of cfs_mesh_hit_dev.h want a whole wave on ONE pose, so the wave serialises its candidates:
// mask = ballot(st == 0); the lowest lane's NJ x 6 link ends (ik_clearance hands them out) are broadcast by v_readlane, the wave
// runs the threshold test on them (variant A: one (mesh, link) pair per lane; variant B: the shared frontier in LDS, variant A
// deciding a pose whose frontier overflows), that lane takes state 2 on a hit, and the mask loses its lowest bit.  All of it is
// wave-uniform.  After the selection the winner's link ends are broadcast once more and lanes p < nmesh*NJ run one exact unbounded
// query each; a wave min gives the mesh part of the clearance.  The mesh code is compiled out of the line-only instantiation
// (MESH == RRT_MESH_NONE), which keeps its code, its registers and its bits.  This translation unit contracts into FMAs, as
// cfs_mesh.hip does and cfs_rrt.hip does not: a pose within rounding of a threshold may be decided differently here than by
// cfs_rrt_grow_mesh; the clearance agrees with cfs_dist_arm_mesh (the same functions under the same flags).
#include "cfs_mesh_hit_dev.h"
#include "cfs_ik_dev.h"
#include "cfs_tool_host.h"

namespace {

constexpr int WV = 64;
constexpr int IK_WAVES = 4;                                   // targets per workgroup
// mesh kernels, dynamic LDS per wave: the private stacks of variant A and of the winner's exact query (MESH_STACK*64 ints + as many
// floats = 10 KB), then variant B's frontier (RRT_FRONTIER_CAP pairs + as many nodes = 4 KB)
constexpr int IK_STACK_WORDS = 2 * MESH_STACK * WV, IK_FRONTIER_WORDS = 2 * RRT_FRONTIER_CAP;

struct IkParams {
    DevRobot rb;                                              // by value, as in RrtParams: no device allocation in the _device entry
    int T, R, nobs, use_axis, max_iter;
    double tool[3], axis[3];                                  // axis normalised on the host
    double lo[6], hi[6], w[6];
    double tol_pos, tol_axis;
    unsigned long long seed;
    const double *obs, *D;                                    // nobs x 6, nobs
    const double *target_pos, *target_axis, *theta_ref;       // T x 3, T x 3 (use_axis), T x NJ
    double *theta;                                            // T x NJ
    int *status, *selected, *n_ok;                            // T
    double *err_pos, *err_axis, *clearance;                   // T
    double *cand_theta;                                       // T x R x NJ
    int *cand_status, *cand_iter;                             // T x R
};

template <int MESH> struct IkArgs { IkParams P; ToolMeshArgs M; };          // M: the mesh table of a cfs_ik_solve_mesh* call
template <> struct IkArgs<RRT_MESH_NONE> { IkParams P; };

// candidates of variant B whose frontier overflowed and that variant A decided (cfs_debug_ik_frontier_overflows): one vector atomic
// by lane 0 per such candidate, none on the normal path
__device__ unsigned long long g_ik_frontier_overflows = 0ull;

struct PoseParams {
    DevRobot rb;
    int N;
    double tool[3], axis[3];
    const double *theta;                                      // N x NJ
    double *pos, *dir, *jac;                                  // N x 3, N x 3, N x 6 x NJ (may be null)
};

// the RRT generator (include/cfs_hip.h, "RRT / RRT*") with tree = restart, counter = joint
__device__ __forceinline__ double ik_uniform(unsigned long long seed, int restart, int joint)
{
    unsigned long long z = seed + (unsigned long long)restart * 0x9E3779B97F4A7C15ull + ((unsigned long long)joint + 1ull) * 0xBF58476D1CE4E5B9ull;
    z ^= z >> 30; z *= 0xBF58476D1CE4E5B9ull;
    z ^= z >> 27; z *= 0x94D049BB133111EBull;
    z ^= z >> 31;
    return (double)(z >> 11) * 0x1.0p-53;
}

// MESH: RRT_MESH_NONE (the line-only kernel: the mesh code is compiled out) | RRT_MESH_PER_LANE | RRT_MESH_WAVE
template <int NJ, int MESH>
__global__ __launch_bounds__(WV * IK_WAVES) void cfs_ik_kernel(const IkArgs<MESH> A_)
{
    const IkParams &P = A_.P;
    __shared__ __attribute__((aligned(16))) double s_rb[sizeof(DevRobot) / 8];
    __shared__ double s_obs[CFS_MAX_OBS * 6];
    __shared__ double s_D[CFS_MAX_OBS];
    // the only block barrier is in there: whole waves may leave after it
    const DevRobot *rb = ik_stage<WV * IK_WAVES>(P.rb, s_rb, P.nobs, P.obs, P.D, s_obs, s_D);
    const int lane = threadIdx.x % WV, t = blockIdx.x * IK_WAVES + threadIdx.x / WV;
    if (t >= P.T) return;
    const bool use_axis = P.use_axis != 0;
    const bool active = lane < P.R;                           // lanes >= restarts idle and enter the reductions with neutral values

    double tp[3], ta[3] = {0.0, 0.0, 0.0}, tref[NJ], th[NJ];
#pragma unroll
    for (int q = 0; q < 3; ++q) tp[q] = P.target_pos[(size_t)t * 3 + q];
    if (use_axis) {
#pragma unroll
        for (int q = 0; q < 3; ++q) ta[q] = P.target_axis[(size_t)t * 3 + q];
        const double n = sqrt(ta[0] * ta[0] + ta[1] * ta[1] + ta[2] * ta[2]);
        ta[0] = ta[0] / n; ta[1] = ta[1] / n; ta[2] = ta[2] / n;
    }
#pragma unroll
    for (int c = 0; c < NJ; ++c) {
        tref[c] = P.theta_ref[(size_t)t * NJ + c];
        const double x = lane == 0 ? tref[c] : P.lo[c] + ik_uniform(P.seed, lane, c) * (P.hi[c] - P.lo[c]);
        th[c] = x < P.lo[c] ? P.lo[c] : (x > P.hi[c] ? P.hi[c] : x);          // a NaN passes: state 3 below
    }

    double p[3], a[3], tw[NJ * 6], r[6], F = 0.0, A[NJ * NJ], g[NJ], lam = IK_LAMBDA0;
    int st = active ? -1 : 1, it = 0;                         // -1: running
#pragma unroll
    for (int q = 0; q < 6; ++q) r[q] = 0.0;
    if (active) {
        ik_pose<NJ>(rb, P.tool, P.axis, th, p, a, tw);
        ik_residual(p, a, tp, ta, use_axis, r, &F);
        ik_normal<NJ>(tw, p, a, r, use_axis, A, g);
    }
    for (;;) {
        if (st < 0) {
            if (!(F < INFINITY)) st = 3;                                                        // step 1
            else if (ik_converged(r, use_axis, P.tol_pos, P.tol_axis)) st = 0;                  // step 2
            else if (it >= P.max_iter) st = 1;                                                  // step 3
        }
        if (__ballot(st < 0) == 0ull) break;
        if (st < 0) {
            // steps 4-8 stand here and in cfs_cart_kernel, statement for statement: as a shared function they cost both NJ = 5 kernels 2 %
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
                ik_residual(p2, a2, tp, ta, use_axis, r2, &F2);
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
                ++it;                                                                       // step 8
            }
        }
    }

    // ---- collision, cost, selection ---------------------------------------------------------------------------------------
    double ep, ea, clear = INFINITY, cost = INFINITY;
    ik_errors(r, &ep, &ea);
    [[maybe_unused]] double ends[MESH == RRT_MESH_NONE ? 1 : NJ * 6];          // the candidate's link ends (mesh kernels only)
    if constexpr (MESH == RRT_MESH_NONE) {
        if (st == 0) {
            clear = ik_clearance<NJ>(rb, th, P.nobs, s_obs, s_D);
            if (!(clear >= 0.0)) st = 2;
        }
    } else {
        // the wave's slice of the dynamic LDS (launch_ik_mesh sizes it)
        extern __shared__ __attribute__((aligned(16))) int s_mesh[];
        const int wave = threadIdx.x / WV;
        int *s_stack = s_mesh + wave * IK_STACK_WORDS;
        float *s_lbs = reinterpret_cast<float *>(s_stack + MESH_STACK * WV);
        int *s_fpair = s_mesh + IK_WAVES * IK_STACK_WORDS + wave * IK_FRONTIER_WORDS, *s_fnode = s_fpair + RRT_FRONTIER_CAP;
        const RrtMeshArgs &MA = A_.M.MA;
        for (int q = 0; q < NJ * 6; ++q) ends[q] = 0.0;
        if (st == 0) {
            clear = ik_clearance<NJ, true>(rb, th, P.nobs, s_obs, s_D, ends);
            if (!(clear >= 0.0)) st = 2;
        }
        // every converged restart that passed the lines, lowest lane first: the whole wave on that one pose
        unsigned long long todo = __ballot(st == 0);
        while (todo != 0ull) {
            const int l = __ffsll((long long)todo) - 1;
            todo &= todo - 1ull;
            double pe[NJ * 6];
#pragma unroll
            for (int q = 0; q < NJ * 6; ++q) pe[q] = ik_bcast(ends[q], l);
            const bool hit = mesh_hit<NJ, MESH>(MA, pe, lane, s_stack, s_lbs, s_fpair, s_fnode, &g_ik_frontier_overflows);
            if (hit && lane == l) st = 2;
        }
    }
    if (st == 0) {
        const double s = ik_cost<NJ>(P.w, th, tref);
        if (s < INFINITY) cost = s; else st = 3;
    }
    if (active) {
        const size_t row = (size_t)t * P.R + lane;
        if (P.cand_theta) {
#pragma unroll
            for (int c = 0; c < NJ; ++c) P.cand_theta[row * NJ + c] = th[c];
        }
        if (P.cand_status) P.cand_status[row] = st;
        if (P.cand_iter) P.cand_iter[row] = it;
    }
    const int n_ok = __popcll(__ballot(st == 0));
    const bool any_hit = __ballot(st == 2) != 0ull;
    const int bl = ik_argmin(cost, lane);
    if constexpr (MESH != RRT_MESH_NONE) {
        // the winner's clearance: one exact, unbounded query per (mesh, link) pair, min_j (dm_j - D_mesh[j]) by a wave min
        if (n_ok > 0) {
            extern __shared__ __attribute__((aligned(16))) int s_mesh[];
            int *s_stack = s_mesh + (threadIdx.x / WV) * IK_STACK_WORDS;
            float *s_lbs = reinterpret_cast<float *>(s_stack + MESH_STACK * WV);
            const RrtMeshArgs &MA = A_.M.MA;
            double pe[NJ * 6];
#pragma unroll
            for (int q = 0; q < NJ * 6; ++q) pe[q] = ik_bcast(ends[q], bl);
            double mm = INFINITY;
            for (int pr = lane; pr < MA.nmesh * NJ; pr += WV) {
                const double v = mesh_pair_clearance<NJ>(MA, A_.M.D, pe, pr, s_stack + lane, s_lbs + lane);
                if (v < mm) mm = v;
            }
            mm = mesh_wave_min(mm);
            if (mm < clear) clear = mm;                       // only the winner's `clear` is written
        }
    }
    const double nan = __builtin_nan("");
    if (n_ok > 0 ? lane == bl : lane == 0) {
        const bool ok = n_ok > 0;
#pragma unroll
        for (int c = 0; c < NJ; ++c) P.theta[(size_t)t * NJ + c] = ok ? th[c] : nan;
        P.status[t] = ok ? 0 : (any_hit ? 2 : 1);
        if (P.selected) P.selected[t] = ok ? lane : -1;
        if (P.n_ok) P.n_ok[t] = n_ok;
        if (P.err_pos) P.err_pos[t] = ok ? ep : nan;
        if (P.err_axis) P.err_axis[t] = ok ? ea : nan;
        if (P.clearance) P.clearance[t] = ok ? clear : nan;
    }
}

// cfs_tool_pose: one thread per configuration, the solver's own device functions
template <int NJ>
__global__ __launch_bounds__(256) void cfs_tool_pose_kernel(const PoseParams P)
{
    __shared__ __attribute__((aligned(16))) double s_rb[sizeof(DevRobot) / 8];
    const DevRobot *rb = ik_stage<256>(P.rb, s_rb);
    const int n = blockIdx.x * 256 + threadIdx.x;
    if (n >= P.N) return;
    double th[NJ], p[3], a[3], tw[NJ * 6];
#pragma unroll
    for (int c = 0; c < NJ; ++c) th[c] = P.theta[(size_t)n * NJ + c];
    ik_pose<NJ>(rb, P.tool, P.axis, th, p, a, tw);
#pragma unroll
    for (int q = 0; q < 3; ++q) { P.pos[(size_t)n * 3 + q] = p[q]; P.dir[(size_t)n * 3 + q] = a[q]; }
    if (P.jac) {
#pragma unroll
        for (int c = 0; c < NJ; ++c) {
            double j6[6];
            ik_jac_col(tw + c * 6, p, a, j6);
#pragma unroll
            for (int q = 0; q < 6; ++q) P.jac[((size_t)n * 6 + q) * NJ + c] = j6[q];
        }
    }
}

template <int NJ, int MESH> hipError_t launch_ik_kernel(size_t lds, const IkArgs<MESH> &a, hipStream_t s)
{
    hipLaunchKernelGGL((cfs_ik_kernel<NJ, MESH>), dim3((a.P.T + IK_WAVES - 1) / IK_WAVES), dim3(WV * IK_WAVES), lds, s, a);
    return hipGetLastError();
}

hipError_t launch_ik(int nj, const IkParams &p, hipStream_t s)
{
    return cfs_for_nj(nj, [&](auto N) { return launch_ik_kernel<decltype(N)::value, RRT_MESH_NONE>(0, {p}, s); });
}

size_t ik_mesh_lds_bytes(int variant)
{
    return (size_t)IK_WAVES * (IK_STACK_WORDS + (variant == RRT_MESH_WAVE ? IK_FRONTIER_WORDS : 0)) * 4;
}

hipError_t launch_ik_mesh(int nj, int variant, const IkParams &p, const ToolMeshArgs &m, hipStream_t s)
{
    if (variant != RRT_MESH_PER_LANE && variant != RRT_MESH_WAVE) return hipErrorInvalidValue;
    const size_t lds = ik_mesh_lds_bytes(variant);
    return cfs_for_nj(nj, [&](auto N) {
        constexpr int NJ = decltype(N)::value;
        return variant == RRT_MESH_PER_LANE ? launch_ik_kernel<NJ, RRT_MESH_PER_LANE>(lds, {p, m}, s) : launch_ik_kernel<NJ, RRT_MESH_WAVE>(lds, {p, m}, s);
    });
}

hipError_t launch_tool_pose(int nj, const PoseParams &p, hipStream_t s)
{
    return cfs_for_nj(nj, [&](auto N) {
        hipLaunchKernelGGL(cfs_tool_pose_kernel<decltype(N)::value>, dim3((p.N + 255) / 256), dim3(256), 0, s, p);
        return hipGetLastError();
    });
}

// ---- C ABI (include/cfs_hip.h, "inverse kinematics") ----------------------------------------------------------------------------
// everything of a call that is host memory in both entries (cfs_tool_host.h); fills the by-value part of the kernel's parameter block
int check_ik(const cfs_ik_desc *d, int T, const double *target_pos, const double *target_axis, const double *theta_ref, const cfs_ik_out *out,
             IkParams &P)
{
    int rc = check_tool_head(d);
    if (rc) return rc;
    if (d->restarts < 1 || d->restarts > WV) return cfs_fail(CFS_ERR_INVALID_ARG, "restarts %d outside 1..%d", d->restarts, WV);
    if ((rc = check_tool_max_iter(d->max_iter)) || (rc = check_tool_fields(d, T))) return rc;
    if (!target_pos || !theta_ref) return cfs_fail(CFS_ERR_INVALID_ARG, "NULL target_pos / theta_ref");
    if ((rc = check_tool_io(d, target_axis, out))) return rc;
    fill_tool_params(d, T, P);
    P.R = d->restarts; P.seed = d->seed;
    return CFS_SUCCESS;
}

void ik_point(IkParams &P, const double *obs, const double *D, const double *target_pos, const double *target_axis, const double *theta_ref,
              const cfs_ik_out *o)
{
    P.obs = obs; P.D = D; P.target_pos = target_pos; P.target_axis = target_axis; P.theta_ref = theta_ref;
    P.theta = o->theta; P.status = o->status; P.selected = o->selected; P.n_ok = o->n_ok;
    P.err_pos = o->err_pos; P.err_axis = o->err_axis; P.clearance = o->clearance;
    P.cand_theta = o->cand_theta; P.cand_status = o->cand_status; P.cand_iter = o->cand_iter;
}

// mc == nullptr: the line-only call
int ik_device(const cfs_ik_desc *d, const MeshCall *mc, int T, const double *target_pos, const double *target_axis, const double *theta_ref,
              const cfs_ik_out *out, void *stream)
{
    static_assert(sizeof(IkParams) <= 4096, "the parameter block travels as a kernel argument");
    static_assert(sizeof(IkArgs<RRT_MESH_WAVE>) <= 4096, "the parameter block and the mesh table travel as a kernel argument");
    IkParams P;
    int rc = check_ik(d, T, target_pos, target_axis, theta_ref, out, P);
    if (rc) return rc;
    ToolMeshArgs M;
    int variant = RRT_MESH_NONE;
    if (mc) {
        rc = check_mesh_call(d->nobs, *mc, IK_MESH_DEFAULT, M, variant);
        if (rc) return rc;
    }
    rc = cfs_use_device(cfs_current_device());
    if (rc) return rc;
    ik_point(P, d->obs, d->D, target_pos, target_axis, theta_ref, out);
    hipError_t e = mc ? launch_ik_mesh(d->njoint, variant, P, M, reinterpret_cast<hipStream_t>(stream))
                      : launch_ik(d->njoint, P, reinterpret_cast<hipStream_t>(stream));
    if (e != hipSuccess) return cfs_fail(CFS_ERR_HIP, "IK launch failed: %s", hipGetErrorString(e));
    return CFS_SUCCESS;
}

int ik_host(const cfs_ik_desc *d, const MeshCall *mc, int T, const double *target_pos, const double *target_axis, const double *theta_ref,
            const cfs_ik_out *out)
{
    IkParams P;
    int rc = check_ik(d, T, target_pos, target_axis, theta_ref, out, P);
    if (rc) return rc;
    ToolMeshArgs M;
    int variant = RRT_MESH_NONE;
    if (mc) {   // refuse before anything is staged on the device
        rc = check_mesh_call(d->nobs, *mc, IK_MESH_DEFAULT, M, variant);
        if (rc) return rc;
    }
    rc = check_tool_arrays(d, T, target_pos, target_axis, theta_ref);
    if (rc) return rc;
    rc = cfs_use_device(cfs_current_device());
    if (rc) return rc;
    const size_t nT = T, nj = d->njoint, R = d->restarts, nobs = d->nobs;
    Stage st;
    cfs_ik_out o;
    memset(&o, 0, sizeof o);
    const double *obs_d = st.up(d->obs, nobs * 6), *D_d = st.up(d->D, nobs), *tp_d = st.up(target_pos, nT * 3);
    const double *ta_d = d->use_axis ? st.up(target_axis, nT * 3) : nullptr;
    const double *tr_d = st.up(theta_ref, nT * nj);
    o.theta = st.out<double>(nT * nj); o.status = st.out<int>(nT);
    if (out->selected) o.selected = st.out<int>(nT);
    if (out->n_ok) o.n_ok = st.out<int>(nT);
    if (out->err_pos) o.err_pos = st.out<double>(nT);
    if (out->err_axis) o.err_axis = st.out<double>(nT);
    if (out->clearance) o.clearance = st.out<double>(nT);
    if (out->cand_theta) o.cand_theta = st.out<double>(nT * R * nj);
    if (out->cand_status) o.cand_status = st.out<int>(nT * R);
    if (out->cand_iter) o.cand_iter = st.out<int>(nT * R);
    if (st.err == hipSuccess) {
        ik_point(P, obs_d, D_d, tp_d, ta_d, tr_d, &o);
        st.err = mc ? launch_ik_mesh(d->njoint, variant, P, M, nullptr) : launch_ik(d->njoint, P, nullptr);
        if (st.err == hipSuccess) st.err = hipStreamSynchronize(nullptr);
    }
    st.down(out->theta, o.theta, nT * nj); st.down(out->status, o.status, nT);
    st.down(out->selected, o.selected, nT); st.down(out->n_ok, o.n_ok, nT);
    st.down(out->err_pos, o.err_pos, nT); st.down(out->err_axis, o.err_axis, nT); st.down(out->clearance, o.clearance, nT);
    st.down(out->cand_theta, o.cand_theta, nT * R * nj); st.down(out->cand_status, o.cand_status, nT * R); st.down(out->cand_iter, o.cand_iter, nT * R);
    return st.result("IK staging or launch");
}
}  // namespace

extern "C" int cfs_ik_solve_device(const cfs_ik_desc *d, int T, const double *target_pos, const double *target_axis, const double *theta_ref,
                                   const cfs_ik_out *out, void *stream)
{
    return ik_device(d, nullptr, T, target_pos, target_axis, theta_ref, out, stream);
}

extern "C" int cfs_ik_solve(const cfs_ik_desc *d, int T, const double *target_pos, const double *target_axis, const double *theta_ref,
                            const cfs_ik_out *out)
{
    return ik_host(d, nullptr, T, target_pos, target_axis, theta_ref, out);
}

extern "C" int cfs_ik_solve_mesh_device(const cfs_ik_desc *d, int nmesh, const cfs_mesh *const *meshes, const double *D_mesh, int flags, int T,
                                        const double *target_pos, const double *target_axis, const double *theta_ref, const cfs_ik_out *out,
                                        void *stream)
{
    const MeshCall mc{nmesh, meshes, D_mesh, flags};
    return ik_device(d, &mc, T, target_pos, target_axis, theta_ref, out, stream);
}

extern "C" int cfs_ik_solve_mesh(const cfs_ik_desc *d, int nmesh, const cfs_mesh *const *meshes, const double *D_mesh, int flags, int T,
                                 const double *target_pos, const double *target_axis, const double *theta_ref, const cfs_ik_out *out)
{
    const MeshCall mc{nmesh, meshes, D_mesh, flags};
    return ik_host(d, &mc, T, target_pos, target_axis, theta_ref, out);
}

extern "C" int cfs_debug_ik_frontier_overflows(unsigned long long *count, int reset)
{
    return cfs_frontier_overflows(&g_ik_frontier_overflows, count, reset);
}

extern "C" int cfs_tool_pose(const cfs_robot *robot, int njoint, const double *tool, const double *tool_axis, int N, const double *theta,
                             double *pos, double *dir, double *jac)
{
    int rc = cfs_check_robot(robot, njoint);
    if (rc) return rc;
    if (njoint < 2) return cfs_fail(CFS_ERR_INVALID_ARG, "njoint %d unsupported (2..6)", njoint);
    if (N < 0 || !tool || !tool_axis || !theta || !pos || !dir) return cfs_fail(CFS_ERR_INVALID_ARG, "bad argument");
    if (!finite3(tool) || !finite3(tool_axis)) return cfs_fail(CFS_ERR_INVALID_ARG, "tool / tool_axis must be finite");
    const double an = std::sqrt(tool_axis[0] * tool_axis[0] + tool_axis[1] * tool_axis[1] + tool_axis[2] * tool_axis[2]);
    if (!(an > 0.0)) return cfs_fail(CFS_ERR_INVALID_ARG, "tool_axis is zero");
    if (N == 0) return CFS_SUCCESS;
    rc = cfs_use_device(cfs_current_device());
    if (rc) return rc;
    PoseParams P;
    memset(&P, 0, sizeof P);
    cfs_build_dev_robot(*robot, P.rb);
    P.N = N;
    for (int q = 0; q < 3; ++q) { P.tool[q] = tool[q]; P.axis[q] = tool_axis[q] / an; }
    const size_t nj = njoint, n = N;
    Stage st;
    P.theta = st.up(theta, n * nj); P.pos = st.out<double>(n * 3); P.dir = st.out<double>(n * 3);
    if (jac) P.jac = st.out<double>(n * 6 * nj);
    if (st.err == hipSuccess) st.err = launch_tool_pose(njoint, P, nullptr);
    if (st.err == hipSuccess) st.err = hipStreamSynchronize(nullptr);
    st.down(pos, P.pos, n * 3); st.down(dir, P.dir, n * 3); st.down(jac, P.jac, n * 6 * nj);
    return st.result("cfs_tool_pose");
}
