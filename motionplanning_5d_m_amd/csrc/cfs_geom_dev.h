// cfs_geom_dev.h -- device functions shared by the linearisation kernels: forward kinematics of one
// link (Lib/functions/CapPos.m:13-20, Lib/2L/CapPos2.m:19-28), Lumelsky segment-segment distance
// (Lib/functions/distLinSeg.m:23-91) with the near-zero surrogate of dist_arm_3D_200i_2.m:22-24.
#pragma once
#include "cfs_device.h"

constexpr double FD_EPS = 1e-5;  // num_jac.m:6

__host__ __device__ constexpr int nvt(int nj) { return nj * (nj + 2); }   // sum_{k=1..nj} (2k+1)
__device__ __forceinline__ int kvoff(int k1) { return k1 * k1 - 1; }      // offset of link k1 (1-based)

// one homogeneous link transform A_k(angle) appended to parent (3x4 row-major), CapPos.m:13-17
__device__ __forceinline__ void fk_step(const DevRobot *rb, int k, double st, double ct,
                                        const double *par, double *out)
{
    double R[12];
    if (rb->kind == CFS_ROBOT_2L) {           // CapPos2.m:19-25
        R[0] = ct;  R[1] = -st; R[2] = 0.0;  R[3] = rb->t2l[k * 3 + 0];
        R[4] = st;  R[5] = ct;  R[6] = 0.0;  R[7] = rb->t2l[k * 3 + 1];
        R[8] = 0.0; R[9] = 0.0; R[10] = 1.0; R[11] = rb->t2l[k * 3 + 2];
    } else {
        const double ca = rb->ca[k], sa = rb->sa[k], a = rb->dh_a[k], d = rb->dh_d[k];
        R[0] = ct;  R[1] = -st * ca; R[2] = st * sa;   R[3] = a * ct;
        R[4] = st;  R[5] = ct * ca;  R[6] = -ct * sa;  R[7] = a * st;
        R[8] = 0.0; R[9] = sa;       R[10] = ca;       R[11] = d;
    }
    if (par == nullptr) {                      // M{1} = eye(4)
#pragma unroll
        for (int e = 0; e < 12; ++e) out[e] = R[e];
        return;
    }
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        const double p0 = par[r * 4 + 0], p1 = par[r * 4 + 1], p2 = par[r * 4 + 2], p3 = par[r * 4 + 3];
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            double s = p0 * R[c] + p1 * R[4 + c] + p2 * R[8 + c];
            if (c == 3) s += p3;
            out[r * 4 + c] = s;
        }
    }
}

// capsule axis end points in the world frame, CapPos.m:18-20
__device__ __forceinline__ void link_ends(const DevRobot *rb, int k, const double *M, double *e6)
{
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
        const double *p = rb->cap + k * 6 + kk * 3;
#pragma unroll
        for (int r = 0; r < 3; ++r)
            e6[kk * 3 + r] = (M[r * 4 + 0] * p[0] + M[r * 4 + 1] * p[1] + M[r * 4 + 2] * p[2]) + M[r * 4 + 3] + rb->base[r];
    }
}

// a/b without the IEEE special-case scaffolding (v_div_scale/fmas/fixup): v_rcp_f64 seed, two Newton
// steps, one residual correction.  Result within 1 ulp of the correctly rounded quotient for the finite,
// well-scaled operands of this routine (lengths and dot products of link / obstacle axes in metres).
#ifndef CFS_FAST_DIV
#define CFS_FAST_DIV 1
#endif
__device__ __forceinline__ double fdiv(double a, double b)
{
#if !CFS_FAST_DIV
    return a / b;
#endif
    double r = __builtin_amdgcn_rcp(b);
    r = fma(fma(-b, r, 1.0), r, r);
    r = fma(fma(-b, r, 1.0), r, r);
    const double q = a * r;
    return fma(fma(-b, q, a), r, q);
}

__device__ __forceinline__ double fixbound(double x) { return x < 0.0 ? 0.0 : (x > 1.0 ? 1.0 : x); }

// distLinSeg.m:23-91 followed by the near-zero surrogate of dist_arm_3D_200i_2.m:22-24.
// a6 = link axis [p1s;p1e], o6 = obstacle axis [p2s;p2e].
__device__ __forceinline__ double seg_seg_dist(const double *a6, const double *o6)
{
    const double d1x = a6[3] - a6[0], d1y = a6[4] - a6[1], d1z = a6[5] - a6[2];
    const double d2x = o6[3] - o6[0], d2y = o6[4] - o6[1], d2z = o6[5] - o6[2];
    const double d12x = o6[0] - a6[0], d12y = o6[1] - a6[1], d12z = o6[2] - a6[2];
    const double D1 = d1x * d1x + d1y * d1y + d1z * d1z;
    const double D2 = d2x * d2x + d2y * d2y + d2z * d2z;
    const double S1 = d1x * d12x + d1y * d12y + d1z * d12z;
    const double S2 = d2x * d12x + d2y * d12y + d2z * d12z;
    const double R = d1x * d2x + d1y * d2y + d1z * d2z;
    const double den = D1 * D2 - R * R;
    double t, u;
    if (D1 == 0.0 || D2 == 0.0) {
        if (D1 != 0.0) { u = 0.0; t = fixbound(fdiv(S1, D1)); }
        else if (D2 != 0.0) { t = 0.0; u = fixbound(fdiv(-S2, D2)); }
        else { t = 0.0; u = 0.0; }
    } else if (den == 0.0) {
        t = 0.0;
        u = fdiv(-S2, D2);
        const double uf = fixbound(u);
        if (uf != u) { t = fixbound(fdiv(uf * R + S1, D1)); u = uf; }
    } else {
        t = fixbound(fdiv(S1 * D2 - S2 * R, den));
        u = fdiv(t * R - S2, D2);
        const double uf = fixbound(u);
        if (uf != u) { t = fixbound(fdiv(uf * R + S1, D1)); u = uf; }
    }
    const double ex = d1x * t - d2x * u - d12x, ey = d1y * t - d2y * u - d12y, ez = d1z * t - d2z * u - d12z;
    double dis = sqrt(ex * ex + ey * ey + ez * ez);
    if (fabs(dis) < 0.0001) {
        const double qx = (a6[0] + d1x * t) - a6[3], qy = (a6[1] + d1y * t) - a6[4], qz = (a6[2] + d1z * t) - a6[5];
        dis = -sqrt(qx * qx + qy * qy + qz * qz);
    }
    return dis;
}


// ---- analytic Jacobian (cfs_problem_set_jacobian(CFS_JAC_ANALYTIC), cfs_dist_arm_grad) ----------------------------------
// The exact derivative of the branch of dist_arm_* that is active at the base pose: the winning link's seg_seg_dist,
// differentiated in forward mode through the branch of distLinSeg.m that was taken (a clamped parameter is a constant) and
// through the near-zero surrogate.  One kinematic chain per pose; the literal scheme of num_jac.m evaluates 2*nj+1 of them.
// Both callers (cfs_geom.hip, cfs_fused.hip) use these functions with contraction fixed per expression, so the gradient of
// the handle-free entry point and the solver's are the same numbers bit for bit.

// Twist of joint k (axis and a point on it, world frame), read off fk_step.  DH: dA/dθ = G·A with G the generator of a
// rotation about z through the origin, so with M_k = M_{k-1}·A_k every point x of links >= k moves as x' = ω × (x - q),
// ω = M_{k-1}·z, q = origin of M_{k-1}.  2L: A = Tr(t)·Rz(θ), dA/dθ = Tr(t)·G·Tr(-t)·A: the axis passes through M_{k-1}·t.
// q carries rb->base as link_ends' points do.  tw6 = [ω; q].
__device__ __forceinline__ void joint_twist(const DevRobot *rb, int k, const double *par, double *tw6)
{
#pragma clang fp contract(on)
    double t0 = 0.0, t1 = 0.0, t2 = 0.0;
    if (rb->kind == CFS_ROBOT_2L) { t0 = rb->t2l[k * 3 + 0]; t1 = rb->t2l[k * 3 + 1]; t2 = rb->t2l[k * 3 + 2]; }
    if (par == nullptr) {
        tw6[0] = 0.0; tw6[1] = 0.0; tw6[2] = 1.0;
        tw6[3] = t0 + rb->base[0]; tw6[4] = t1 + rb->base[1]; tw6[5] = t2 + rb->base[2];
        return;
    }
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        tw6[r] = par[r * 4 + 2];
        tw6[3 + r] = (par[r * 4 + 0] * t0 + par[r * 4 + 1] * t1 + par[r * 4 + 2] * t2) + par[r * 4 + 3] + rb->base[r];
    }
}

// base pose of one configuration from the sin / cos of its joint angles (sc: [nj][2], the joint offset already subtracted):
// capsule end points of every link (ends: [nj][6], the numbers link_ends gives) and the twist of every joint (tw: [nj][6])
__device__ __forceinline__ void arm_chain(const DevRobot *rb, int nj, const double *sc, double *ends, double *tw)
{
    double M[12], Mn[12];
    for (int k = 0; k < nj; ++k) {
        joint_twist(rb, k, k == 0 ? nullptr : M, tw + k * 6);
        fk_step(rb, k, sc[2 * k], sc[2 * k + 1], k == 0 ? nullptr : M, Mn);
#pragma unroll
        for (int q = 0; q < 12; ++q) M[q] = Mn[q];
        link_ends(rb, k, M, ends + k * 6);
    }
}

// seg_seg_dist with what its derivative needs: the same branches as seg_seg_dist, decided by the same arithmetic, and how t
// and u depend on the end points in the branch taken (tm / um, 0: constant -- fixed at 0 or clamped)
//   tm 1: t = S1/D1   2: t = (u R + S1)/D1 (u clamped)   3: t = (S1 D2 - S2 R)/den
//   um 1: u = -S2/D2  2: u = (t R - S2)/D2
struct SegTan {
    double d1x, d1y, d1z, d2x, d2y, d2z, d12x, d12y, d12z, D1, D2, S2, R, den, t, u, ex, ey, ez, dis, qx, qy, qz, qn;
    int tm, um;
    bool sur;     // the near-zero surrogate dis = -|p1s + d1 t - p1e| (dist_arm_3D_200i_2.m:22-24)
};
__device__ __forceinline__ SegTan seg_seg_prep(const double *a6, const double *o6)
{
#pragma clang fp contract(on)
    SegTan s;
    s.d1x = a6[3] - a6[0]; s.d1y = a6[4] - a6[1]; s.d1z = a6[5] - a6[2];
    s.d2x = o6[3] - o6[0]; s.d2y = o6[4] - o6[1]; s.d2z = o6[5] - o6[2];
    s.d12x = o6[0] - a6[0]; s.d12y = o6[1] - a6[1]; s.d12z = o6[2] - a6[2];
    const double D1 = s.d1x * s.d1x + s.d1y * s.d1y + s.d1z * s.d1z;
    const double D2 = s.d2x * s.d2x + s.d2y * s.d2y + s.d2z * s.d2z;
    const double S1 = s.d1x * s.d12x + s.d1y * s.d12y + s.d1z * s.d12z;
    const double S2 = s.d2x * s.d12x + s.d2y * s.d12y + s.d2z * s.d12z;
    const double R = s.d1x * s.d2x + s.d1y * s.d2y + s.d1z * s.d2z;
    const double den = D1 * D2 - R * R;
    int tm = 0, um = 0;
    double t, u;
    if (D1 == 0.0 || D2 == 0.0) {
        if (D1 != 0.0) { u = 0.0; const double tq = fdiv(S1, D1); t = fixbound(tq); tm = t == tq ? 1 : 0; }
        else if (D2 != 0.0) { t = 0.0; const double uq = fdiv(-S2, D2); u = fixbound(uq); um = u == uq ? 1 : 0; }
        else { t = 0.0; u = 0.0; }
    } else if (den == 0.0) {
        t = 0.0;
        u = fdiv(-S2, D2);
        um = 1;
        const double uf = fixbound(u);
        if (uf != u) { const double tq = fdiv(uf * R + S1, D1); t = fixbound(tq); tm = t == tq ? 2 : 0; u = uf; um = 0; }
    } else {
        const double tq = fdiv(S1 * D2 - S2 * R, den);
        t = fixbound(tq);
        tm = t == tq ? 3 : 0;
        u = fdiv(t * R - S2, D2);
        um = 2;
        const double uf = fixbound(u);
        if (uf != u) { const double tq2 = fdiv(uf * R + S1, D1); t = fixbound(tq2); tm = t == tq2 ? 2 : 0; u = uf; um = 0; }
    }
    s.D1 = D1; s.D2 = D2; s.S2 = S2; s.R = R; s.den = den; s.t = t; s.u = u; s.tm = tm; s.um = um;
    s.ex = s.d1x * t - s.d2x * u - s.d12x; s.ey = s.d1y * t - s.d2y * u - s.d12y; s.ez = s.d1z * t - s.d2z * u - s.d12z;
    s.dis = sqrt(s.ex * s.ex + s.ey * s.ey + s.ez * s.ez);
    s.sur = fabs(s.dis) < 0.0001;
    s.qx = s.qy = s.qz = s.qn = 0.0;
    if (s.sur) {
        s.qx = (a6[0] + s.d1x * t) - a6[3]; s.qy = (a6[1] + s.d1y * t) - a6[4]; s.qz = (a6[2] + s.d1z * t) - a6[5];
        s.qn = sqrt(s.qx * s.qx + s.qy * s.qy + s.qz * s.qz);
        s.dis = -s.qn;
    }
    return s;
}

// directional derivative of the distance for a tangent g6 = [p1s'; p1e'] of the link end points (the obstacle is fixed)
__device__ __forceinline__ double seg_seg_dir(const SegTan &s, const double *g)
{
#pragma clang fp contract(on)
    const double g1x = g[3] - g[0], g1y = g[4] - g[1], g1z = g[5] - g[2];   // (p1e - p1s)'
    const double g12x = -g[0], g12y = -g[1], g12z = -g[2];                  // (p2s - p1s)'
    const double D1p = 2.0 * (s.d1x * g1x + s.d1y * g1y + s.d1z * g1z);
    const double S1p = (g1x * s.d12x + g1y * s.d12y + g1z * s.d12z) + (s.d1x * g12x + s.d1y * g12y + s.d1z * g12z);
    const double S2p = s.d2x * g12x + s.d2y * g12y + s.d2z * g12z;
    const double Rp = g1x * s.d2x + g1y * s.d2y + g1z * s.d2z;
    const double t = s.t, u = s.u;
    double tp = 0.0, up = 0.0;
    if (s.tm == 1) tp = fdiv(S1p - t * D1p, s.D1);
    else if (s.tm == 2) tp = fdiv((u * Rp + S1p) - t * D1p, s.D1);
    else if (s.tm == 3) tp = fdiv(((S1p * s.D2 - S2p * s.R) - s.S2 * Rp) - t * (D1p * s.D2 - 2.0 * s.R * Rp), s.den);
    if (s.um == 1) up = fdiv(-S2p, s.D2);
    else if (s.um == 2) up = fdiv((tp * s.R + t * Rp) - S2p, s.D2);
    if (!s.sur) {
        const double epx = (g1x * t + s.d1x * tp) - s.d2x * up - g12x;
        const double epy = (g1y * t + s.d1y * tp) - s.d2y * up - g12y;
        const double epz = (g1z * t + s.d1z * tp) - s.d2z * up - g12z;
        return fdiv(s.ex * epx + s.ey * epy + s.ez * epz, s.dis);
    }
    if (!(s.qn > 0.0)) return 0.0;        // the surrogate of a zero-length link: gradient 0
    const double qpx = (g[0] + g1x * t + s.d1x * tp) - g[3];
    const double qpy = (g[1] + g1y * t + s.d1y * tp) - g[4];
    const double qpz = (g[2] + g1z * t + s.d1z * tp) - g[5];
    return -fdiv(s.qx * qpx + s.qy * qpy + s.qz * qpz, s.qn);
}

// d/dθ_m of dist_arm at the base pose, m = 0..nj-1: the winning link k (0-based) with end points e6 moves with joints
// 0..k only (x' = ω_m × (x - q_m), joint_twist); the other entries are 0.  g: nj entries (any address space).
__device__ __forceinline__ void winner_grad(const double *e6, const double *tw, int k, int nj, const double *o6, double *g)
{
#pragma clang fp contract(on)
    const SegTan s = seg_seg_prep(e6, o6);
    for (int m = 0; m < nj; ++m) {
        double v = 0.0;
        if (m <= k) {
            const double *w = tw + m * 6;
            double g6[6];
#pragma unroll
            for (int p = 0; p < 2; ++p) {
                const double rx = e6[p * 3 + 0] - w[3], ry = e6[p * 3 + 1] - w[4], rz = e6[p * 3 + 2] - w[5];
                g6[p * 3 + 0] = w[1] * rz - w[2] * ry;
                g6[p * 3 + 1] = w[2] * rx - w[0] * rz;
                g6[p * 3 + 2] = w[0] * ry - w[1] * rx;
            }
            v = seg_seg_dir(s, g6);
        }
        g[m] = v;
    }
}
