// cfs_audit.hip -- audit of joint paths between their rows: sampled and certified clearance against line obstacles, sampled and
// certified deviation of the tool point from the chord (include/cfs_hip.h, "Tool-path audit").
//
// The Cartesian paths, the tool paths and the path timing treat a path as N rows; a controller moves the joints linearly between
// them.  This unit measures that motion on G x R paths at once: (N-1)*S + 1 samples per path, each one forward kinematics plus
// nobs * NJ segment pairs, then ordered reductions over the samples and over the sub-intervals between neighbouring samples.
//
// MI355X mapping.  cfs_path_audit_kernel<NJ>: one wavefront (a workgroup of 64) per path; a path that is not audited leaves after
// one load.  The robot, the obstacle rows with their margins and the path's rows are staged in LDS (ik_stage, then the rows, whose
// finiteness is tested on the way: at most 257 x 6 doubles, the dynamic part of the LDS plan).  Phase 1, lanes stride over the rows:
// clearance and tool point of every row into LDS -- the tool points are the chord's ends, the clearances are clear_rows and the
// samples sigma = 0 | 1, which are therefore read and never recomputed.  Phase 2, the time line g = n*S + k in passes of 64 samples
// that overlap by one: lane t holds sample g0 + t (a row: from LDS; otherwise one ik_clearance and one ik_pose at q_n + (k/S) d_n)
// and takes sample g0 + t + 1 from its neighbour with one shuffle, so a sub-interval reads both its ends once and no sample
// value goes through memory; the overlap recomputes one sample in 64.  Every lane keeps running extrema, the minimum of the
// clearance with its sample index; the lanes meet once, in xor shuffles on (value, index), so the first minimum is exact.  The
// closest link and obstacle are found once per path, at the minimal sample, by all lanes alike.  No atomics, no workspace, no
// dynamically indexed private array.
// Compiled with the flags of cfs_cart.o and cfs_ik.o (contraction as the compiler chooses): the clearances are ik_clearance's as
// those units evaluate it, and nothing in the contract is promised to the last bit against a CPU restatement.
#include "cfs_ik_dev.h"
#include "cfs_tool_host.h"
#include <climits>

namespace {

constexpr int AUDIT_MAX_ROWS = 257, AUDIT_MAX_PATHS = 64, AUDIT_MAX_SUB = 64;
constexpr int AUDIT_FIXED = (int)(sizeof(DevRobot) / 8) + CFS_MAX_OBS * 7;   // doubles of LDS in front of the rows

struct AuditParams {
    DevRobot rb;                                              // by value: no device allocation in the _device entry
    int total, N, S, nobs;                                    // total = G*R
    double tool[3], min_clearance, max_chord;
    double rho[CFS_MAX_LINKS * CFS_MAX_LINKS];                // cfs_clear_build_rho
    double rt[CFS_MAX_LINKS];                                 // reach of the tool point about the axis of joint m
    const double *obs, *D;                                    // nobs x 6, nobs
    const double *paths;                                      // total x N x NJ
    const int *state;                                         // total or null
    double *clear_rows, *clear_path, *s_path, *clear_lower, *chord_err, *chord_upper;   // total each, may be null
    int *link_path, *obs_path, *state_out;                    // total each, may be null
    int *status;                                              // total
};

// min / max in which a NaN sticks
__device__ __forceinline__ double audit_min(double a, double v) { return (v < a || v != v) ? v : a; }
__device__ __forceinline__ double audit_max(double a, double v) { return (v > a || v != v) ? v : a; }

__device__ __forceinline__ double audit_wave_min(double v)
{
#pragma unroll
    for (int m = 1; m < IK_WV; m <<= 1) v = audit_min(v, __shfl_xor(v, m, IK_WV));
    return v;
}

__device__ __forceinline__ double audit_wave_max(double v)
{
#pragma unroll
    for (int m = 1; m < IK_WV; m <<= 1) v = audit_max(v, __shfl_xor(v, m, IK_WV));
    return v;
}

template <int NJ>
__device__ __forceinline__ void audit_point(const DevRobot *rb, const AuditParams &P, const double *q, double *p)
{
    const double zero[3] = {0.0, 0.0, 0.0};
    double a[3], tw[NJ * 6];                                  // direction and twists are not used: dead code after inlining
    ik_pose<NJ>(rb, P.tool, zero, q, p, a, tw);
}

// the configuration of sample g = n*S + k: row n itself at k = 0, else q_n + (k/S) (q_{n+1} - q_n)
template <int NJ>
__device__ __forceinline__ void audit_theta(const double *rows, int S, int g, double *th, double *sigma)
{
    const int n = g / S, k = g - n * S;
    const double sg = (double)k / (double)S;
    const double *q0 = rows + n * NJ, *q1 = rows + (k == 0 ? n : n + 1) * NJ;   // k = 0 on the last row: no row behind it is read
#pragma unroll
    for (int c = 0; c < NJ; ++c) th[c] = k == 0 ? q0[c] : q0[c] + sg * (q1[c] - q0[c]);
    *sigma = sg;
}

template <int NJ>
__global__ __launch_bounds__(IK_WV) void cfs_path_audit_kernel(const AuditParams P)
{
    extern __shared__ __attribute__((aligned(16))) double lds[];
    const int lane = threadIdx.x, i = blockIdx.x, N = P.N, S = P.S, nobs = P.nobs;
    const double nan = __builtin_nan("");
    const int st_in = P.state ? P.state[i] : 0;               // uniform over the workgroup
    int status = st_in != 0 ? 1 : 0;
    double *s_rb = lds, *s_obs = s_rb + sizeof(DevRobot) / 8, *s_D = s_obs + CFS_MAX_OBS * 6;
    double *s_rows = lds + AUDIT_FIXED, *s_pt = s_rows + N * NJ, *s_c = s_pt + N * 3;

    double o_rows = nan, o_path = nan, o_s = nan, o_low = nan, o_err = nan, o_up = nan;
    int o_link = -1, o_obs = -1;
    if (status == 0) {                                        // uniform: the barriers below are reached by all 64 lanes or by none
        const double *path = P.paths + (size_t)i * N * NJ;
        bool bad = false;
        for (int e = lane; e < N * NJ; e += IK_WV) {
            const double v = path[e];
            s_rows[e] = v;
            bad = bad || !(fabs(v) < INFINITY);
        }
        const DevRobot *rb = ik_stage<IK_WV>(P.rb, s_rb, nobs, P.obs, P.D, s_obs, s_D);   // the barrier covers the rows too
        if (__syncthreads_or(bad ? 1 : 0)) status = 2;
        if (status == 0) {
            // ---- phase 1: the rows ----
            double c_rows = INFINITY;
            for (int r = lane; r < N; r += IK_WV) {
                double th[NJ], p[3];
#pragma unroll
                for (int c = 0; c < NJ; ++c) th[c] = s_rows[r * NJ + c];
                const double cl = ik_clearance<NJ>(rb, th, nobs, s_obs, s_D);
                audit_point<NJ>(rb, P, th, p);
                s_c[r] = cl;
                s_pt[r * 3 + 0] = p[0]; s_pt[r * 3 + 1] = p[1]; s_pt[r * 3 + 2] = p[2];
                c_rows = audit_min(c_rows, cl);
            }
            __syncthreads();
            // ---- phase 2: the samples, in passes of 63 sub-intervals ----
            const int GS = (N - 1) * S + 1;                   // samples; sub-intervals: GS - 1 >= 1
            double a_path = INFINITY, a_low = INFINITY, a_err = 0.0, a_up = 0.0;
            int a_g = INT_MAX;
            for (int g0 = 0; g0 < GS - 1; g0 += IK_WV - 1) {
                const int g = g0 + lane;
                double cl = INFINITY, er = 0.0;
                if (g < GS) {
                    const int n = g / S, k = g - n * S;
                    if (k == 0) {
                        cl = s_c[n];
                    } else {
                        double th[NJ], p[3], sg;
                        audit_theta<NJ>(s_rows, S, g, th, &sg);
                        cl = ik_clearance<NJ>(rb, th, nobs, s_obs, s_D);
                        audit_point<NJ>(rb, P, th, p);
                        const double *pa = s_pt + n * 3, *pb = pa + 3;
                        const double ex = p[0] - ((1.0 - sg) * pa[0] + sg * pb[0]), ey = p[1] - ((1.0 - sg) * pa[1] + sg * pb[1]),
                                     ez = p[2] - ((1.0 - sg) * pa[2] + sg * pb[2]);
                        er = sqrt((ex * ex + ey * ey) + ez * ez);
                    }
                    // the first sample of a pass behind the first is the last of the pass before it: met twice, with one index
                    if (a_g == INT_MAX || (cl != cl ? !(a_path != a_path) : cl < a_path)) { a_path = cl; a_g = g; }
                    a_err = audit_max(a_err, er);
                }
                const double cl1 = __shfl_down(cl, 1, IK_WV), er1 = __shfl_down(er, 1, IK_WV);
                if (lane < IK_WV - 1 && g < GS - 1) {         // sub-interval g, on segment n = g div S
                    const double *q0 = s_rows + (g / S) * NJ, *q1 = q0 + NJ;
                    double ad[NJ], L = 0.0, A = 0.0;
#pragma unroll
                    for (int c = 0; c < NJ; ++c) ad[c] = fabs(q1[c] - q0[c]);
#pragma unroll
                    for (int kk = 0; kk < NJ; ++kk) {
                        double sum = 0.0;
#pragma unroll
                        for (int m = 0; m <= kk; ++m) sum += ad[m] * P.rho[m * CFS_MAX_LINKS + kk];
                        L = fmax(L, sum);
                    }
#pragma unroll
                    for (int m = 0; m < NJ; ++m)
#pragma unroll
                        for (int l = 0; l < NJ; ++l) A += ad[m] * ad[l] * P.rt[m > l ? m : l];
                    a_low = audit_min(a_low, (cl + cl1) / 2.0 - L / (2.0 * (double)S));
                    a_up = audit_max(a_up, audit_max(er, er1) + A / (8.0 * (double)S * (double)S));
                }
            }
            // ---- the lanes meet: NaN first, then the lowest value, then the lowest sample ----
            o_rows = audit_wave_min(c_rows);
            o_low = audit_wave_min(a_low);
            o_err = audit_wave_max(a_err);
            o_up = audit_wave_max(a_up);
            double key = a_path != a_path ? -INFINITY : a_path;
            bool isn = a_path != a_path;
#pragma unroll
            for (int m = 1; m < IK_WV; m <<= 1) {
                const double ok = __shfl_xor(key, m, IK_WV);
                const int og = __shfl_xor(a_g, m, IK_WV);
                const bool on = __shfl_xor(isn ? 1 : 0, m, IK_WV) != 0;
                const bool take = on != isn ? on : (ok < key || (ok == key && og < a_g));
                if (take) { key = ok; a_g = og; isn = on; }
            }
            o_path = isn ? nan : key;
            {
                const int n = a_g / S, k = a_g - n * S;
                o_s = (double)n + (double)k / (double)S;
            }
            if (nobs > 0) {                                   // the closest obstacle and its first closest link at sample a_g
                double th[NJ], sg, ends[NJ * 6], best = INFINITY;
                audit_theta<NJ>(s_rows, S, a_g, th, &sg);
                (void)ik_clearance<NJ, true>(rb, th, 0, s_obs, s_D, ends);
                o_obs = 0; o_link = 1;
                for (int j = 0; j < nobs; ++j) {
                    double o6[6], d = INFINITY;
                    int lk = 1;
#pragma unroll
                    for (int q = 0; q < 6; ++q) o6[q] = s_obs[j * 6 + q];
#pragma unroll
                    for (int kk = 0; kk < NJ; ++kk) {
                        const double dis = seg_seg_dist(ends + kk * 6, o6);
                        if (dis < d) { d = dis; lk = kk + 1; }
                    }
                    const double mg = d - s_D[j];
                    if (mg < best) { best = mg; o_obs = j; o_link = lk; }
                }
            }
        }
    }
    if (lane != 0) return;
    int so = st_in;
    if (so == 0) {
        if (status == 2) so = 3;
        else if (o_low < P.min_clearance || (o_low != o_low && P.min_clearance > -INFINITY)) so = 6;
        else if (o_up > P.max_chord || (o_up != o_up && P.max_chord < INFINITY)) so = 7;
    }
    if (P.clear_rows) P.clear_rows[i] = o_rows;
    if (P.clear_path) P.clear_path[i] = o_path;
    if (P.s_path) P.s_path[i] = o_s;
    if (P.clear_lower) P.clear_lower[i] = o_low;
    if (P.chord_err) P.chord_err[i] = o_err;
    if (P.chord_upper) P.chord_upper[i] = o_up;
    if (P.link_path) P.link_path[i] = o_link;
    if (P.obs_path) P.obs_path[i] = o_obs;
    if (P.state_out) P.state_out[i] = so;
    P.status[i] = status;
}

size_t audit_lds_bytes(int N, int nj) { return ((size_t)AUDIT_FIXED + (size_t)N * (nj + 4)) * 8; }

hipError_t launch_audit(int nj, const AuditParams &p, hipStream_t s)
{
    return cfs_for_nj(nj, [&](auto NJc) {
        constexpr int NJ = decltype(NJc)::value;
        hipLaunchKernelGGL((cfs_path_audit_kernel<NJ>), dim3(p.total), dim3(IK_WV), audit_lds_bytes(p.N, NJ), s, p);
        return hipGetLastError();
    });
}

// every refusal; then the by-value part of the parameter block (pointers are set by the caller)
int check_audit(const cfs_audit_desc *d, int G, int R, int N, const double *paths, const cfs_audit_out *out, AuditParams &P)
{
    int rc = check_tool_chain(d);
    if (rc) return rc;
    if (G < 1) return cfs_fail(CFS_ERR_INVALID_ARG, "at least one group is needed");
    if (R < 1 || R > AUDIT_MAX_PATHS) return cfs_fail(CFS_ERR_INVALID_ARG, "R %d outside 1..%d", R, AUDIT_MAX_PATHS);
    if ((long long)G * R > INT_MAX) return cfs_fail(CFS_ERR_INVALID_ARG, "G * R exceeds %d paths", INT_MAX);
    if (N < 2 || N > AUDIT_MAX_ROWS) return cfs_fail(CFS_ERR_INVALID_ARG, "N %d outside 2..%d", N, AUDIT_MAX_ROWS);
    if (d->substeps < 1 || d->substeps > AUDIT_MAX_SUB) return cfs_fail(CFS_ERR_INVALID_ARG, "substeps=%d outside 1..%d", d->substeps, AUDIT_MAX_SUB);
    if (d->nobs < 0 || d->nobs > CFS_MAX_OBS) return cfs_fail(CFS_ERR_INVALID_ARG, "nobs %d outside 0..%d", d->nobs, CFS_MAX_OBS);
    if (d->nobs > 0 && (!d->obs || !d->D)) return cfs_fail(CFS_ERR_INVALID_ARG, "obs / D must be given");
    if (!finite3(d->tool)) return cfs_fail(CFS_ERR_INVALID_ARG, "tool must be finite");
    if (d->min_clearance != d->min_clearance || d->min_clearance == INFINITY)
        return cfs_fail(CFS_ERR_INVALID_ARG, "min_clearance must be finite (-inf: no test)");
    if (!(d->max_chord > 0.0)) return cfs_fail(CFS_ERR_INVALID_ARG, "max_chord must be > 0 (+inf: no test)");
    if (!paths) return cfs_fail(CFS_ERR_INVALID_ARG, "paths must be given");
    if (!out || !out->status) return cfs_fail(CFS_ERR_INVALID_ARG, "out and out->status must be given");
    memset(&P, 0, sizeof P);
    cfs_build_dev_robot(d->robot, P.rb);
    P.total = G * R; P.N = N; P.S = d->substeps; P.nobs = d->nobs;
    P.min_clearance = d->min_clearance; P.max_chord = d->max_chord;
    const int nj = d->njoint;
    cfs_clear_build_rho(P.rb, nj, P.rho);
    const double tl = std::sqrt(d->tool[0] * d->tool[0] + d->tool[1] * d->tool[1] + d->tool[2] * d->tool[2]);
    double len = 0.0;                                         // the link translations from joint m to the last link, as in rho
    for (int m = nj - 1; m >= 0; --m) {
        const double *t = P.rb.t2l + m * 3;
        len += P.rb.kind == CFS_ROBOT_2L ? std::sqrt(t[0] * t[0] + t[1] * t[1] + t[2] * t[2]) : std::hypot(P.rb.dh_a[m], P.rb.dh_d[m]);
        P.rt[m] = len + tl;
    }
    for (int q = 0; q < 3; ++q) P.tool[q] = d->tool[q];
    return CFS_SUCCESS;
}

void audit_point_to(AuditParams &P, const double *obs, const double *D, const double *paths, const int *state, const cfs_audit_out *o)
{
    P.obs = obs; P.D = D; P.paths = paths; P.state = state;
    P.clear_rows = o->clear_rows; P.clear_path = o->clear_path; P.s_path = o->s_path; P.clear_lower = o->clear_lower;
    P.chord_err = o->chord_err; P.chord_upper = o->chord_upper; P.link_path = o->link_path; P.obs_path = o->obs_path;
    P.status = o->status; P.state_out = o->state_out;
}
}  // namespace

extern "C" int cfs_path_audit_device(const cfs_audit_desc *d, int G, int R, int N, const double *paths, const int *state,
                                     const cfs_audit_out *out, void *stream)
{
    static_assert(sizeof(AuditParams) <= 4096, "the parameter block travels as a kernel argument");
    static_assert((AUDIT_FIXED + AUDIT_MAX_ROWS * (CFS_MAX_LINKS + 4)) * 8 <= 64 * 1024, "the LDS plan fits the default limit");
    AuditParams P;
    int rc = check_audit(d, G, R, N, paths, out, P);
    if (rc) return rc;
    rc = cfs_use_device(cfs_current_device());
    if (rc) return rc;
    audit_point_to(P, d->obs, d->D, paths, state, out);
    const hipError_t e = launch_audit(d->njoint, P, reinterpret_cast<hipStream_t>(stream));
    if (e != hipSuccess) return cfs_fail(CFS_ERR_HIP, "path audit launch failed: %s", hipGetErrorString(e));
    return CFS_SUCCESS;
}

extern "C" int cfs_path_audit(const cfs_audit_desc *d, int G, int R, int N, const double *paths, const int *state, const cfs_audit_out *out)
{
    AuditParams P;
    int rc = check_audit(d, G, R, N, paths, out, P);
    if (rc) return rc;
    if (d->nobs && (!all_finite(d->obs, (size_t)d->nobs * 6) || !all_finite(d->D, d->nobs)))
        return cfs_fail(CFS_ERR_INVALID_ARG, "obs / D must be finite");
    rc = cfs_use_device(cfs_current_device());
    if (rc) return rc;
    const size_t np = (size_t)G * R, nobs = d->nobs;
    Stage st;
    cfs_audit_out o;
    memset(&o, 0, sizeof o);
    const double *paths_d = st.up(paths, np * N * d->njoint);
    const int *state_d = state ? st.up(state, np) : nullptr;
    const double *obs_d = nobs ? st.up(d->obs, nobs * 6) : nullptr, *D_d = nobs ? st.up(d->D, nobs) : nullptr;
    if (out->clear_rows) o.clear_rows = st.out<double>(np);
    if (out->clear_path) o.clear_path = st.out<double>(np);
    if (out->s_path) o.s_path = st.out<double>(np);
    if (out->clear_lower) o.clear_lower = st.out<double>(np);
    if (out->chord_err) o.chord_err = st.out<double>(np);
    if (out->chord_upper) o.chord_upper = st.out<double>(np);
    if (out->link_path) o.link_path = st.out<int>(np);
    if (out->obs_path) o.obs_path = st.out<int>(np);
    if (out->state_out) o.state_out = st.out<int>(np);
    o.status = st.out<int>(np);
    if (st.err == hipSuccess) {
        audit_point_to(P, obs_d, D_d, paths_d, state_d, &o);
        st.err = launch_audit(d->njoint, P, nullptr);
        if (st.err == hipSuccess) st.err = hipStreamSynchronize(nullptr);
    }
    st.down(out->clear_rows, o.clear_rows, np); st.down(out->clear_path, o.clear_path, np); st.down(out->s_path, o.s_path, np);
    st.down(out->clear_lower, o.clear_lower, np); st.down(out->chord_err, o.chord_err, np); st.down(out->chord_upper, o.chord_upper, np);
    st.down(out->link_path, o.link_path, np); st.down(out->obs_path, o.obs_path, np); st.down(out->state_out, o.state_out, np);
    st.down(out->status, o.status, np);
    return st.result("path audit staging or launch");
}
