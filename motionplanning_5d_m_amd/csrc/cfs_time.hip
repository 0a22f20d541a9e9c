// cfs_time.hip -- batched timing of joint paths under speed, acceleration and feed limits (include/cfs_hip.h, "Path timing"; DESIGN.md
// section 28).
//
// IK, the Cartesian paths and the tool paths return joint rows without a clock.  This unit puts one on G x R paths of N rows at once:
// per path the pointwise largest (ds/dt)^2 profile of the contract's constraint set (a backward and a forward pass over the rows), per
// group the path that completes soonest.
//
// MI355X mapping.  cfs_path_time_kernel<NJ, FEED>: one lane per path over the flat G*R index, 256 lanes per workgroup, so R = 1 (timing
// the winners) wastes no lanes.  A path is a sequential recurrence over its rows and paths are independent, so there is nothing for
// lanes to share but the robot, staged once per workgroup in LDS (ik_stage) for the forward kinematics of the feed cap.  The backward
// pass walks the rows from the last to the first holding a window of two rows (configuration, tool point, segment), one load of a row
// and one ik_pose per step, and leaves K_n in the path's sdot row; the forward pass walks back up, recomputes the segment's tangential
// budget from the same window with the same instructions (so it is the backward pass's value to the last bit), and overwrites
// sdot.  The two passes are one loop with a direction: with ik_pose inlined once per pass and again in front of each, the 5-joint
// kernel kept 36 B of scratch per lane; with one site it keeps none.  No LDS array, no dynamically indexed private array, no atomics.
// A lane's rows are N*NJ doubles from its neighbour's: its loads and stores do not coalesce across the wave, consecutive rows of one
// lane share cache lines instead (DESIGN.md section 28 has the measured cost).  cfs_path_time_select_kernel: one wavefront per group,
// one lane per path, ik_argmin on (duration, lane).
// The arithmetic of the contract is IEEE double in the order written: this object is compiled with -ffp-contract=off (Makefile).
#include "cfs_ik_dev.h"
#include "cfs_tool_host.h"
#include <climits>

namespace {

constexpr int TIME_WG = 256;                                  // paths per workgroup
constexpr int TIME_SEL_WAVES = 4;                             // groups per workgroup of the selection
constexpr int TIME_MAX_ROWS = 257, TIME_MAX_PATHS = 64;

struct TimeParams {
    DevRobot rb;                                              // by value: no device allocation in the _device entry
    int total, G, R, N, stop_every;                           // total = G*R
    double tool[3], vmax[6], amax[6], feed, gam;
    const double *paths;                                      // total x N x NJ
    const int *state;                                         // total or null
    double *time, *sdot;                                      // total x N (time may be null)
    double *duration;                                         // total
    int *status;                                              // total
    int *selected, *group_status;                             // G, may be null
};

// cap_n and, with a segment behind the row (hc), ubar_n.  dp / dc: the segments before and after the row (hp / hc: they exist);
// lp / lc: the tool point's way over them (FEED); stop: the row is one the path rests at.
template <int NJ, bool FEED>
__device__ __forceinline__ void time_row(const TimeParams &P, const double *dp, const double *dc, bool hp, bool hc, double lp, double lc, bool stop,
                                         double *cap_out, double *ub_out)
{
    const bool inner = hp && hc;
    double cap = INFINITY, ak[NJ];
#pragma unroll
    for (int c = 0; c < NJ; ++c) {
        const double a = hp ? fabs(dp[c]) : 0.0, b = hc ? fabs(dc[c]) : 0.0;
        const double m = a > b ? a : b;
        if (m > 0.0) {
            const double t = P.vmax[c] / m, t2 = t * t;
            cap = t2 < cap ? t2 : cap;
        }
        ak[c] = inner ? fabs(dc[c] - dp[c]) : 0.0;
        if (ak[c] > 0.0) {
            const double t = (P.gam * P.amax[c]) / ak[c];
            cap = t < cap ? t : cap;
        }
    }
    if constexpr (FEED) {
        const double a = hp ? lp : 0.0, b = hc ? lc : 0.0;
        const double e = a > b ? a : b;
        if (e > 0.0) {
            const double t = P.feed / e, t2 = t * t;
            cap = t2 < cap ? t2 : cap;
        }
    }
    if (stop) cap = 0.0;
    double ub = INFINITY;
    if (hc) {
#pragma unroll
        for (int c = 0; c < NJ; ++c) {
            const double ad = fabs(dc[c]);
            if (ad > 0.0) {
                const double num = ak[c] > 0.0 ? P.amax[c] - ak[c] * cap : P.amax[c];
                const double t = num / ad;
                ub = t < ub ? t : ub;
            }
        }
    }
    *cap_out = cap;
    *ub_out = ub;
}

template <int NJ>
__device__ __forceinline__ void time_point(const DevRobot *rb, const TimeParams &P, const double *q, double *p)
{
    const double zero[3] = {0.0, 0.0, 0.0};
    double a[3], tw[NJ * 6];                                  // direction and twists are not used: dead code after inlining
    ik_pose<NJ>(rb, P.tool, zero, q, p, a, tw);
}

__device__ __forceinline__ double time_dist(const double *a, const double *b)
{
    const double dx = a[0] - b[0], dy = a[1] - b[1], dz = a[2] - b[2];
    return sqrt((dx * dx + dy * dy) + dz * dz);
}

template <int NJ, bool FEED>
__global__ __launch_bounds__(TIME_WG) void cfs_path_time_kernel(const TimeParams P)
{
    __shared__ __attribute__((aligned(16))) double s_rb[sizeof(DevRobot) / 8];
    const DevRobot *rb = nullptr;
    if constexpr (FEED) rb = ik_stage<TIME_WG>(P.rb, s_rb);   // the only block barrier: lanes may leave after it; no feed reads no robot
    const int i = blockIdx.x * TIME_WG + threadIdx.x;
    if (i >= P.total) return;
    const int N = P.N, k = P.stop_every;
    const double *path = P.paths + (size_t)i * N * NJ;
    double *sd = P.sdot + (size_t)i * N, *tm = P.time ? P.time + (size_t)i * N : nullptr;
    const double nan = __builtin_nan("");

    int st = (P.state && P.state[i] != 0) ? 1 : 0;
    double dur = nan;
    if (st == 0) {
        bool fin = true, rep = false, stall = false;
        double Knext = 0.0, b = 0.0, s = 0.0, t = 0.0;
        // pass 0 walks the rows N-1 .. 0 and leaves K_n in sdot[n]; pass 1 walks 0 .. N-1 and overwrites it with sqrt(b_n).  Both are
        // this one loop: visit j loads the next row in walking order (none at j == N) and closes the row visited before it, whose two
        // segments are then known.  One load of a row and one ik_pose per visit.
        for (int pass = 0; pass < 2 && st == 0; ++pass) {
            const bool fwd = pass != 0;
            double qm[NJ], pm[3] = {0.0, 0.0, 0.0}, dold[NJ], lold = 0.0;   // the row to close; the segment walked before it
#pragma unroll
            for (int c = 0; c < NJ; ++c) { qm[c] = 0.0; dold[c] = 0.0; }
            for (int j = 0; j <= N; ++j) {
                const bool hn = j < N, ho = j > 1;            // a segment towards the new row / the older segment exists
                double qx[NJ], px[3] = {0.0, 0.0, 0.0}, dnew[NJ], lnew = 0.0;
#pragma unroll
                for (int c = 0; c < NJ; ++c) { qx[c] = 0.0; dnew[c] = 0.0; }
                if (hn) {
                    const int r = fwd ? j : N - 1 - j;
                    bool good = true, zero = j > 0;
#pragma unroll
                    for (int c = 0; c < NJ; ++c) {
                        qx[c] = path[(size_t)r * NJ + c];
                        good = good && fabs(qx[c]) < INFINITY;
                        if (j > 0) dnew[c] = fwd ? qx[c] - qm[c] : qm[c] - qx[c];   // q_{n+1} - q_n in either direction
                        zero = zero && dnew[c] == 0.0;
                    }
                    if (!fwd) { fin = fin && good; rep = rep || zero; }   // both are final when the backward walk ends
                    if constexpr (FEED) {
                        time_point<NJ>(rb, P, qx, px);
                        if (j > 0) lnew = time_dist(px, pm);
                    }
                }
                if (j > 0) {
                    const int m = fwd ? j - 1 : N - j;        // the row to close, in path order: dp before it, dc behind it
                    double dp[NJ], dc[NJ];
#pragma unroll
                    for (int c = 0; c < NJ; ++c) { dp[c] = fwd ? dold[c] : dnew[c]; dc[c] = fwd ? dnew[c] : dold[c]; }
                    const bool hp = fwd ? ho : hn, hc = fwd ? hn : ho;
                    const double lp = fwd ? lold : lnew, lc = fwd ? lnew : lold;
                    const bool stop = !hp || !hc || (k >= 2 && m % k == 0);
                    double cap, ub;
                    time_row<NJ, FEED>(P, dp, dc, hp, hc, lp, lc, stop, &cap, &ub);
                    if (!fwd) {
                        double K = cap;
                        if (hc) {
                            const double up = Knext + 2.0 * ub;
                            K = up < cap ? up : cap;
                        }
                        sd[m] = K;
                        Knext = K;
                    } else {
                        if (hc) {
                            const double Kx = sd[m + 1], up = b + 2.0 * ub;
                            const double bx = up < Kx ? up : Kx;
                            const double s1 = sqrt(bx);
                            stall = stall || (b == 0.0 && bx == 0.0);
                            sd[m] = s;
                            if (tm) tm[m] = t;
                            t = t + 2.0 / (s + s1);
                            b = bx;
                            s = s1;
                        } else {
                            sd[m] = s;
                            if (tm) tm[m] = t;
                        }
                    }
                }
#pragma unroll
                for (int c = 0; c < NJ; ++c) { qm[c] = qx[c]; dold[c] = dnew[c]; }
#pragma unroll
                for (int q = 0; q < 3; ++q) pm[q] = px[q];
                lold = lnew;
            }
            if (!fwd) {
                if (!fin) st = 2;
                else if (rep) st = 4;
                else { b = sd[0]; s = sqrt(b); }
            } else {
                if (stall) st = 3;
                else if (!(fabs(t) < INFINITY)) st = 2;
                else dur = t;
            }
        }
    }
    if (st != 0) {
        for (int n = 0; n < N; ++n) {
            sd[n] = nan;
            if (tm) tm[n] = nan;
        }
    }
    P.duration[i] = dur;
    P.status[i] = st;
}

__global__ __launch_bounds__(IK_WV * TIME_SEL_WAVES) void cfs_path_time_select_kernel(const TimeParams P)
{
    const int lane = threadIdx.x % IK_WV, g = blockIdx.x * TIME_SEL_WAVES + threadIdx.x / IK_WV;
    if (g >= P.G) return;
    double cost = INFINITY;
    if (lane < P.R) {
        const size_t e = (size_t)g * P.R + lane;
        if (P.status[e] == 0) cost = P.duration[e];
    }
    const int bl = ik_argmin(cost, lane);
    const bool ok = ik_bcast(cost, bl) < INFINITY;
    if (lane == 0) {
        if (P.selected) P.selected[g] = ok ? bl : -1;
        if (P.group_status) P.group_status[g] = ok ? 0 : 1;
    }
}

// the timing, then (either group output given) the selection over what it wrote, on stream s
hipError_t launch_time(int nj, const TimeParams &p, hipStream_t s)
{
    hipError_t e = cfs_for_nj(nj, [&](auto N) {
        const dim3 grid((p.total + TIME_WG - 1) / TIME_WG), block(TIME_WG);
        if (p.feed < INFINITY) hipLaunchKernelGGL((cfs_path_time_kernel<decltype(N)::value, true>), grid, block, 0, s, p);
        else hipLaunchKernelGGL((cfs_path_time_kernel<decltype(N)::value, false>), grid, block, 0, s, p);
        return hipGetLastError();
    });
    if (e != hipSuccess || (!p.selected && !p.group_status)) return e;
    hipLaunchKernelGGL(cfs_path_time_select_kernel, dim3((p.G + TIME_SEL_WAVES - 1) / TIME_SEL_WAVES), dim3(IK_WV * TIME_SEL_WAVES), 0, s, p);
    return hipGetLastError();
}

// every refusal; then the by-value part of the parameter block (pointers are set by the caller).  need_sdot: the _device entry
int check_time(const cfs_time_desc *d, int G, int R, int N, const double *paths, const cfs_time_out *out, bool need_sdot, TimeParams &P)
{
    int rc = check_tool_chain(d);
    if (rc) return rc;
    if (G < 1) return cfs_fail(CFS_ERR_INVALID_ARG, "at least one group is needed");
    if (R < 1 || R > TIME_MAX_PATHS) return cfs_fail(CFS_ERR_INVALID_ARG, "R %d outside 1..%d", R, TIME_MAX_PATHS);
    if ((long long)G * R > INT_MAX) return cfs_fail(CFS_ERR_INVALID_ARG, "G * R exceeds %d paths", INT_MAX);
    if (N < 3 || N > TIME_MAX_ROWS) return cfs_fail(CFS_ERR_INVALID_ARG, "N %d outside 3..%d", N, TIME_MAX_ROWS);
    if (d->stop_every < 0 || d->stop_every == 1) return cfs_fail(CFS_ERR_INVALID_ARG, "stop_every must be 0 or >= 2, not %d", d->stop_every);
    if (!d->vmax || !d->amax) return cfs_fail(CFS_ERR_INVALID_ARG, "vmax / amax must be given");
    for (int c = 0; c < d->njoint; ++c)
        if (!(std::isfinite(d->vmax[c]) && d->vmax[c] > 0.0 && std::isfinite(d->amax[c]) && d->amax[c] > 0.0))
            return cfs_fail(CFS_ERR_INVALID_ARG, "vmax[%d] / amax[%d] must be finite and > 0", c, c);
    if (!(d->feed > 0.0)) return cfs_fail(CFS_ERR_INVALID_ARG, "feed must be > 0 (+inf: no cap)");
    if (std::isfinite(d->feed) && !finite3(d->tool)) return cfs_fail(CFS_ERR_INVALID_ARG, "tool must be finite");
    if (!(d->curve_share > 0.0 && d->curve_share < 1.0)) return cfs_fail(CFS_ERR_INVALID_ARG, "curve_share must lie in (0, 1)");
    if (!paths) return cfs_fail(CFS_ERR_INVALID_ARG, "paths must be given");
    if (!out || !out->duration || !out->status) return cfs_fail(CFS_ERR_INVALID_ARG, "out, out->duration and out->status must be given");
    if (out->time && !out->sdot) return cfs_fail(CFS_ERR_INVALID_ARG, "out->time needs out->sdot, the workspace between the two passes");
    if (need_sdot && !out->sdot)
        return cfs_fail(CFS_ERR_INVALID_ARG,
                        "cfs_path_time_device: out->sdot must be given, the workspace between the two passes (nothing is allocated here)");
    memset(&P, 0, sizeof P);
    cfs_build_dev_robot(d->robot, P.rb);
    P.total = G * R; P.G = G; P.R = R; P.N = N; P.stop_every = d->stop_every;
    P.feed = d->feed; P.gam = d->curve_share;
    for (int q = 0; q < 3; ++q) P.tool[q] = std::isfinite(d->feed) ? d->tool[q] : 0.0;
    for (int c = 0; c < d->njoint; ++c) { P.vmax[c] = d->vmax[c]; P.amax[c] = d->amax[c]; }
    return CFS_SUCCESS;
}

void time_point_to(TimeParams &P, const double *paths, const int *state, const cfs_time_out *o)
{
    P.paths = paths; P.state = state;
    P.time = o->time; P.sdot = o->sdot; P.duration = o->duration; P.status = o->status; P.selected = o->selected; P.group_status = o->group_status;
}
}  // namespace

extern "C" int cfs_path_time_device(const cfs_time_desc *d, int G, int R, int N, const double *paths, const int *state, const cfs_time_out *out,
                                    void *stream)
{
    static_assert(sizeof(TimeParams) <= 4096, "the parameter block travels as a kernel argument");
    TimeParams P;
    int rc = check_time(d, G, R, N, paths, out, true, P);
    if (rc) return rc;
    rc = cfs_use_device(cfs_current_device());
    if (rc) return rc;
    time_point_to(P, paths, state, out);
    const hipError_t e = launch_time(d->njoint, P, reinterpret_cast<hipStream_t>(stream));
    if (e != hipSuccess) return cfs_fail(CFS_ERR_HIP, "path timing launch failed: %s", hipGetErrorString(e));
    return CFS_SUCCESS;
}

extern "C" int cfs_path_time(const cfs_time_desc *d, int G, int R, int N, const double *paths, const int *state, const cfs_time_out *out)
{
    TimeParams P;
    int rc = check_time(d, G, R, N, paths, out, false, P);
    if (rc) return rc;
    rc = cfs_use_device(cfs_current_device());
    if (rc) return rc;
    const size_t np = (size_t)G * R, nr = np * N, nG = G;
    Stage st;
    cfs_time_out o;
    memset(&o, 0, sizeof o);
    const double *paths_d = st.up(paths, nr * d->njoint);
    const int *state_d = state ? st.up(state, np) : nullptr;
    if (out->time) o.time = st.out<double>(nr);
    o.sdot = st.out<double>(nr);                              // also the workspace between the passes
    o.duration = st.out<double>(np); o.status = st.out<int>(np);
    if (out->selected) o.selected = st.out<int>(nG);
    if (out->group_status) o.group_status = st.out<int>(nG);
    if (st.err == hipSuccess) {
        time_point_to(P, paths_d, state_d, &o);
        st.err = launch_time(d->njoint, P, nullptr);
        if (st.err == hipSuccess) st.err = hipStreamSynchronize(nullptr);
    }
    st.down(out->time, o.time, nr); st.down(out->sdot, o.sdot, nr); st.down(out->duration, o.duration, np); st.down(out->status, o.status, np);
    st.down(out->selected, o.selected, nG); st.down(out->group_status, o.group_status, nG);
    return st.result("path timing staging or launch");
}
