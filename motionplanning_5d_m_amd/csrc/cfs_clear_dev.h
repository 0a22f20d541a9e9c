// cfs_clear_dev.h -- the time line of the clearance audit, shared by its two kernels (cfs_clear.hip: line obstacles;
// cfs_clear_mesh.hip: mesh obstacles).  Sample g of the G = H*S + 1 distinct ones is g = 0 (xR1) or g = i*S + k, k = 1..S; the arm
// follows theta(tau) = theta_s + tau v_s + tau^2/2 u_i inside interval i (robotproperty2.m:136-139) and stands at row i of x_ itself
// at k = S.  x: H x 2nj, u: H x nj, x1: 2nj, in LDS or in HBM.
#pragma once
#include "cfs_device.h"

// interval and sub-step of sample g
__device__ __forceinline__ void clear_sample_ik(int g, int S, int &i, int &k)
{
    i = g == 0 ? 0 : (g - 1) / S;
    k = g == 0 ? 0 : (g - 1) % S + 1;
}

// joint kk at sample (i, k)
__device__ __forceinline__ double clear_sample_theta(const double *x, const double *u, const double *x1, int nj, int S, double dt, int i, int k, int kk)
{
    const int ns = 2 * nj;
    const double *xs = i == 0 ? x1 : x + (size_t)(i - 1) * ns;                      // state the interval starts from
    const double tau = (double)k * dt / (double)S;
    if (k == S) return x[(size_t)i * ns + kk];                                      // the waypoint itself: row i of x_
    if (k == 0) return xs[kk];
    return xs[kk] + tau * xs[nj + kk] + tau * tau / 2.0 * u[i * nj + kk];
}

// arm's share of |d/dtau distance| on sub-interval [g, g+1], g < G - 1: no point of link kk moves faster than
// sum_{m<=kk} |v_m| rho[m][kk], and |v_m| is largest at an end of the sub-interval (v is linear in tau)
__device__ __forceinline__ double clear_arm_speed(const double *x, const double *u, const double *x1, const double *rho, int nj, int S, double dt, int g)
{
    const int ns = 2 * nj;
    const int i2 = g / S, k2 = g % S;
    const double *x2 = i2 == 0 ? x1 : x + (size_t)(i2 - 1) * ns;
    const double t0 = (double)k2 * dt / (double)S, t1 = (double)(k2 + 1) * dt / (double)S;
    double L = 0.0;
    for (int kk = 0; kk < nj; ++kk) {
        double sum = 0.0;
        for (int m = 0; m <= kk; ++m) {
            const double v0 = x2[nj + m], uu = u[i2 * nj + m];
            sum += fmax(fabs(v0 + t0 * uu), fabs(v0 + t1 * uu)) * rho[m * CFS_MAX_LINKS + kk];
        }
        L = fmax(L, sum);
    }
    return L;
}
