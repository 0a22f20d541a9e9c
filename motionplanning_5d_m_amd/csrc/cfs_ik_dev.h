// cfs_ik_dev.h -- device functions of the inverse-kinematics iteration (include/cfs_hip.h, "inverse kinematics"), shared by cfs_ik.hip
// and cfs_cart.hip: the leaves (pose, residual, analytic Jacobian, the damped step, the line-obstacle clearance) and what the kernels
// of both units do with them -- the workgroup staging (ik_stage), the convergence test (ik_converged), the cost
// (ik_cost) and the wave argmin of the selection (ik_argmin).  Steps 4-8 of the iteration stand in the two kernels themselves,
// cfs_ik_kernel and cfs_cart_kernel: as a function here they moved the register allocation of the NJ = 5 instantiations and cost them
// 2 %.  Every loop over
// joints is unrolled at compile time: NJ is a template parameter.
#pragma once
#include "cfs_geom_dev.h"
#include <cmath>

namespace {

constexpr int IK_WV = 64;                                     // lanes of a wavefront: one restart or candidate each
constexpr double IK_LAMBDA0 = 1e-2, IK_LAMBDA_MIN = 1e-9, IK_LAMBDA_MAX = 1e9, IK_STEP_CAP = 0.5;

// The robot and, with s_obs given, the nobs obstacle rows and their margins into the workgroup's LDS, by all WG threads, and the
// block barrier behind it; returns the staged robot.
template <int WG>
__device__ __forceinline__ const DevRobot *ik_stage(const DevRobot &rb, double *s_rb, int nobs = 0, const double *obs = nullptr,
                                                    const double *D = nullptr, double *s_obs = nullptr, double *s_D = nullptr)
{
    const double *src = reinterpret_cast<const double *>(&rb);
    for (int e = threadIdx.x; e < (int)(sizeof(DevRobot) / 8); e += WG) s_rb[e] = src[e];
    if (s_obs) {
        for (int e = threadIdx.x; e < nobs * 6; e += WG) s_obs[e] = obs[e];
        for (int e = threadIdx.x; e < nobs; e += WG) s_D[e] = D[e];
    }
    __syncthreads();
    return reinterpret_cast<const DevRobot *>(s_rb);
}

// lane l's value in every lane (l is wave-uniform): two v_readlane
__device__ __forceinline__ double ik_bcast(double v, int l)
{
    const long long b = __double_as_longlong(v);
    const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(b & 0xffffffffll), l);
    const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)((unsigned long long)b >> 32), l);
    return __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
}

// pose(theta): tool point (link_ends' expression, base added) and tool direction in the world frame, and the twist of every joint
template <int NJ>
__device__ __forceinline__ void ik_pose(const DevRobot *rb, const double *tool, const double *axis, const double *th, double *p, double *a,
                                        double *tw)
{
    double M[12], Mn[12];
#pragma unroll
    for (int k = 0; k < NJ; ++k) {
        joint_twist(rb, k, k == 0 ? nullptr : M, tw + k * 6);
        double sn, cs;
        sincos(th[k] - rb->th_off[k], &sn, &cs);
        fk_step(rb, k, sn, cs, k == 0 ? nullptr : M, Mn);
#pragma unroll
        for (int q = 0; q < 12; ++q) M[q] = Mn[q];
    }
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        p[r] = (M[r * 4 + 0] * tool[0] + M[r * 4 + 1] * tool[1] + M[r * 4 + 2] * tool[2]) + M[r * 4 + 3] + rb->base[r];
        a[r] = M[r * 4 + 0] * axis[0] + M[r * 4 + 1] * axis[1] + M[r * 4 + 2] * axis[2];
    }
}

// column c of the Jacobian: [w x (p - q); w x a]
__device__ __forceinline__ void ik_jac_col(const double *tw6, const double *p, const double *a, double *j6)
{
    const double wx = tw6[0], wy = tw6[1], wz = tw6[2];
    const double rx = p[0] - tw6[3], ry = p[1] - tw6[4], rz = p[2] - tw6[5];
    j6[0] = wy * rz - wz * ry; j6[1] = wz * rx - wx * rz; j6[2] = wx * ry - wy * rx;
    j6[3] = wy * a[2] - wz * a[1]; j6[4] = wz * a[0] - wx * a[2]; j6[5] = wx * a[1] - wy * a[0];
}

// A = J'J (full symmetric, row-major) and g = J'r over the first M rows (3 | 6)
template <int NJ>
__device__ __forceinline__ void ik_normal(const double *tw, const double *p, const double *a, const double *r, bool use_axis, double *A, double *g)
{
    double J[NJ * 6];
#pragma unroll
    for (int c = 0; c < NJ; ++c) {
        ik_jac_col(tw + c * 6, p, a, J + c * 6);
        if (!use_axis) { J[c * 6 + 3] = 0.0; J[c * 6 + 4] = 0.0; J[c * 6 + 5] = 0.0; }
    }
#pragma unroll
    for (int c = 0; c < NJ; ++c) {
        double s = 0.0;
#pragma unroll
        for (int q = 0; q < 6; ++q) s += J[c * 6 + q] * r[q];
        g[c] = s;
#pragma unroll
        for (int e = 0; e <= c; ++e) {
            double v = 0.0;
#pragma unroll
            for (int q = 0; q < 6; ++q) v += J[c * 6 + q] * J[e * 6 + q];
            A[c * NJ + e] = v; A[e * NJ + c] = v;
        }
    }
}

// delta = -(A + lam I)^-1 g by Cholesky; false when a pivot is not finite and > 0
template <int NJ>
__device__ __forceinline__ bool ik_solve_step(const double *A, const double *g, double lam, double *delta)
{
    double L[NJ * NJ];
    bool ok = true;
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        double s = A[j * NJ + j] + lam;
#pragma unroll
        for (int k = 0; k < j; ++k) s -= L[j * NJ + k] * L[j * NJ + k];
        ok = ok && (s > 0.0) && (s < INFINITY);
        const double dj = sqrt(s);
        L[j * NJ + j] = dj;
#pragma unroll
        for (int i = j + 1; i < NJ; ++i) {
            double t = A[i * NJ + j];
#pragma unroll
            for (int k = 0; k < j; ++k) t -= L[i * NJ + k] * L[j * NJ + k];
            L[i * NJ + j] = t / dj;
        }
    }
    double y[NJ];
#pragma unroll
    for (int i = 0; i < NJ; ++i) {
        double t = -g[i];
#pragma unroll
        for (int k = 0; k < i; ++k) t -= L[i * NJ + k] * y[k];
        y[i] = t / L[i * NJ + i];
    }
#pragma unroll
    for (int i = NJ - 1; i >= 0; --i) {
        double t = y[i];
#pragma unroll
        for (int k = i + 1; k < NJ; ++k) t -= L[k * NJ + i] * delta[k];
        delta[i] = t / L[i * NJ + i];
    }
    return ok;
}

__device__ __forceinline__ void ik_residual(const double *p, const double *a, const double *tp, const double *ta, bool use_axis, double *r,
                                            double *F)
{
    r[0] = p[0] - tp[0]; r[1] = p[1] - tp[1]; r[2] = p[2] - tp[2];
    r[3] = use_axis ? a[0] - ta[0] : 0.0; r[4] = use_axis ? a[1] - ta[1] : 0.0; r[5] = use_axis ? a[2] - ta[2] : 0.0;
    *F = (r[0] * r[0] + r[1] * r[1] + r[2] * r[2]) + (r[3] * r[3] + r[4] * r[4] + r[5] * r[5]);
}

// the position and the axis error of a residual
__device__ __forceinline__ void ik_errors(const double *r, double *ep, double *ea)
{
    *ep = sqrt(r[0] * r[0] + r[1] * r[1] + r[2] * r[2]);
    *ea = sqrt(r[3] * r[3] + r[4] * r[4] + r[5] * r[5]);
}

// step 2: the pose is reached.  Both comparisons are made before they are combined: with `&&` / `||` the compiler moves the second
// norm into a branch of its own, and the line instantiation of cfs_cart_kernel<6, *>, the kernels with scratch, then takes 16 B per
// lane more of it.
__device__ __forceinline__ bool ik_converged(const double *r, bool use_axis, double tol_pos, double tol_axis)
{
    double ep, ea;
    ik_errors(r, &ep, &ea);
    const bool bp = ep <= tol_pos, ba = ea <= tol_axis;
    return bp & (!use_axis | ba);
}

// sum_c w[c] * (a[c] - b[c])^2 in joint order, no FMA: the contract's cost to the last bit
template <int NJ>
__device__ __forceinline__ double ik_cost(const double *w, const double *a, const double *b)
{
    double s = 0.0;
#pragma unroll
    for (int c = 0; c < NJ; ++c) {
        const double dlt = a[c] - b[c];
        s = __dadd_rn(s, __dmul_rn(w[c], __dmul_rn(dlt, dlt)));
    }
    return s;
}

// the selection: the lane of the wave's smallest cost, the lowest such lane on a tie, by xor shuffles; every lane returns it.
// WITH_MAX: the wave's maximum of *vmax rides in the same loop.
template <bool WITH_MAX = false>
__device__ __forceinline__ int ik_argmin(double bc, int lane, [[maybe_unused]] int *vmax = nullptr)
{
    int bl = lane;
#pragma unroll
    for (int m = 1; m < IK_WV; m <<= 1) {
        const double oc = __shfl_xor(bc, m, IK_WV);
        const int ol = __shfl_xor(bl, m, IK_WV);
        if constexpr (WITH_MAX) {
            const int ov = __shfl_xor(*vmax, m, IK_WV);
            if (ov > *vmax) *vmax = ov;
        }
        if (oc < bc || (oc == bc && ol < bl)) { bc = oc; bl = ol; }
    }
    return bl;
}

// min_j (d_j - D_j), d_j = cfs_dist_arm's distance to obstacle j; +inf without obstacles.  ENDS: the NJ x 6 link ends go to ends_out
template <int NJ, bool ENDS = false>
__device__ __forceinline__ double ik_clearance(const DevRobot *rb, const double *th, int nobs, const double *obs, const double *D,
                                               double *ends_out = nullptr)
{
    double ends_loc[NJ * 6], M[12], Mn[12];
    double *ends = ENDS ? ends_out : ends_loc;
#pragma unroll
    for (int k = 0; k < NJ; ++k) {
        double sn, cs;
        sincos(th[k] - rb->th_off[k], &sn, &cs);
        fk_step(rb, k, sn, cs, k == 0 ? nullptr : M, Mn);
#pragma unroll
        for (int q = 0; q < 12; ++q) M[q] = Mn[q];
        link_ends(rb, k, M, ends + k * 6);
    }
    double c = INFINITY;
    for (int j = 0; j < nobs; ++j) {
        double o6[6];
#pragma unroll
        for (int q = 0; q < 6; ++q) o6[q] = obs[j * 6 + q];
        double d = INFINITY;
#pragma unroll
        for (int k = 0; k < NJ; ++k) {
            const double dis = seg_seg_dist(ends + k * 6, o6);
            if (dis < d) d = dis;
        }
        const double m = d - D[j];
        if (m < c || m != m) c = m;                           // a NaN sticks: the restart then counts as colliding
    }
    return c;
}

}  // namespace
