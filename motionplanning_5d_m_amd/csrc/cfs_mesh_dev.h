// cfs_mesh_dev.h -- device side of the mesh obstacles shared by the translation units that query a hierarchy (cfs_mesh.hip: distance
// entry points and the linearisation; cfs_clear_mesh.hip: the clearance audit): the exact segment-triangle distance, the rigorous
// segment-box lower bound and the nearest-first traversal.  Contract: cfs_mesh.hip's head comment.
#pragma once
#include "cfs_geom_dev.h"
#include "cfs_host.h"
#include <cmath>

namespace {

constexpr int MESH_THREADS = 128;
constexpr int MESH_STACK = 20;              // >= depth of the balanced hierarchy + 2 (checked at build time)
#ifndef CFS_LEAF_TRIS
#define CFS_LEAF_TRIS 2
#endif
constexpr int LEAF_TRIS = CFS_LEAF_TRIS;

// ---- device geometry -------------------------------------------------------------------------------
__device__ __forceinline__ double dot3(const double *a, const double *b) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }
__device__ __forceinline__ void sub3(const double *a, const double *b, double *c) { c[0] = a[0] - b[0]; c[1] = a[1] - b[1]; c[2] = a[2] - b[2]; }
__device__ __forceinline__ void cross3(const double *a, const double *b, double *c)
{
    c[0] = a[1] * b[2] - a[2] * b[1];
    c[1] = a[2] * b[0] - a[0] * b[2];
    c[2] = a[0] * b[1] - a[1] * b[0];
}
__device__ __forceinline__ double clamp01(double x) { return x < 0.0 ? 0.0 : (x > 1.0 ? 1.0 : x); }

// Lib/functions/distLinSeg.m:23-91 with both outputs: distance, parameter t on the first segment, closest points
__device__ double seg_seg_full(const double *p1s, const double *p1e, const double *p2s, const double *p2e, double *t_out, double *pts)
{
    double d1[3], d2[3], d12[3];
    sub3(p1e, p1s, d1); sub3(p2e, p2s, d2); sub3(p2s, p1s, d12);
    const double D1 = dot3(d1, d1), D2 = dot3(d2, d2), S1 = dot3(d1, d12), S2 = dot3(d2, d12), R = dot3(d1, d2);
    const double den = D1 * D2 - R * R;
    double t, u;
    if (D1 == 0.0 || D2 == 0.0) {
        if (D1 != 0.0) { u = 0.0; t = clamp01(S1 / D1); }
        else if (D2 != 0.0) { t = 0.0; u = clamp01(-S2 / D2); }
        else { t = 0.0; u = 0.0; }
    } else if (den == 0.0) {
        t = 0.0;
        u = -S2 / D2;
        const double uf = clamp01(u);
        if (uf != u) { t = clamp01((uf * R + S1) / D1); u = uf; }
    } else {
        t = clamp01((S1 * D2 - S2 * R) / den);
        u = (t * R - S2) / D2;
        const double uf = clamp01(u);
        if (uf != u) { t = clamp01((uf * R + S1) / D1); u = uf; }
    }
    double e[3];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        e[r] = d1[r] * t - d2[r] * u - d12[r];
        pts[r] = p1s[r] + d1[r] * t;
        pts[3 + r] = p2s[r] + d2[r] * u;
    }
    *t_out = t;
    return sqrt(dot3(e, e));
}

// closest point of triangle ABC to P (Voronoi regions; Ericson, Real-Time Collision Detection 5.1.5)
__device__ void closest_pt_triangle(const double *P, const double *A, const double *B, const double *C, double *Q)
{
    double ab[3], ac[3], ap[3], bp[3], cp[3];
    sub3(B, A, ab); sub3(C, A, ac); sub3(P, A, ap);
    const double d1 = dot3(ab, ap), d2 = dot3(ac, ap);
    if (d1 <= 0.0 && d2 <= 0.0) { Q[0] = A[0]; Q[1] = A[1]; Q[2] = A[2]; return; }
    sub3(P, B, bp);
    const double d3 = dot3(ab, bp), d4 = dot3(ac, bp);
    if (d3 >= 0.0 && d4 <= d3) { Q[0] = B[0]; Q[1] = B[1]; Q[2] = B[2]; return; }
    const double vc = d1 * d4 - d3 * d2;
    if (vc <= 0.0 && d1 >= 0.0 && d3 <= 0.0) {
        const double v = d1 / (d1 - d3);
#pragma unroll
        for (int r = 0; r < 3; ++r) Q[r] = A[r] + v * ab[r];
        return;
    }
    sub3(P, C, cp);
    const double d5 = dot3(ab, cp), d6 = dot3(ac, cp);
    if (d6 >= 0.0 && d5 <= d6) { Q[0] = C[0]; Q[1] = C[1]; Q[2] = C[2]; return; }
    const double vb = d5 * d2 - d1 * d6;
    if (vb <= 0.0 && d2 >= 0.0 && d6 <= 0.0) {
        const double w = d2 / (d2 - d6);
#pragma unroll
        for (int r = 0; r < 3; ++r) Q[r] = A[r] + w * ac[r];
        return;
    }
    const double va = d3 * d6 - d5 * d4;
    if (va <= 0.0 && (d4 - d3) >= 0.0 && (d5 - d6) >= 0.0) {
        const double w = (d4 - d3) / ((d4 - d3) + (d5 - d6));
#pragma unroll
        for (int r = 0; r < 3; ++r) Q[r] = B[r] + w * (C[r] - B[r]);
        return;
    }
    const double denom = 1.0 / (va + vb + vc);
    const double v = vb * denom, w = vc * denom;
#pragma unroll
    for (int r = 0; r < 3; ++r) Q[r] = A[r] + ab[r] * v + ac[r] * w;
}

struct Best {                  // incumbent of one query
    double d, t;
    double pts[6];
    int tri;
};
__device__ __forceinline__ void take(Best &b, double dis, double t, const double *pl, const double *pm, int tri)
{
    if (dis < b.d || (dis == b.d && t < b.t)) {
        b.d = dis; b.t = t; b.tri = tri;
#pragma unroll
        for (int r = 0; r < 3; ++r) { b.pts[r] = pl[r]; b.pts[3 + r] = pm[r]; }
    }
}

// segment P0P1 against triangle T (9 doubles)
__device__ void seg_tri_update(const double *P0, const double *P1, const double *T, int tri, Best &b)
{
    const double *A = T, *B = T + 3, *C = T + 6;
    double d[3], ab[3], ac[3], n[3], e0[3], e1[3];
    sub3(P1, P0, d);
    const double D = dot3(d, d);
    sub3(B, A, ab); sub3(C, A, ac);
    cross3(ab, ac, n);
    if (dot3(n, n) > 0.0) {                                  // proper triangle: does the segment pierce it?
        sub3(P0, A, e0); sub3(P1, A, e1);
        const double s0 = dot3(n, e0), s1 = dot3(n, e1);
        if (s0 * s1 <= 0.0 && s0 != s1) {
            const double t = s0 / (s0 - s1);
            double X[3], xa[3], xb[3], xc[3], bc[3], ca[3], c0[3], c1[3], c2[3];
#pragma unroll
            for (int r = 0; r < 3; ++r) X[r] = P0[r] + t * d[r];
            sub3(X, A, xa); sub3(X, B, xb); sub3(X, C, xc);
            sub3(C, B, bc); sub3(A, C, ca);
            cross3(ab, xa, c0); cross3(bc, xb, c1); cross3(ca, xc, c2);
            if (dot3(n, c0) >= 0.0 && dot3(n, c1) >= 0.0 && dot3(n, c2) >= 0.0) { take(b, 0.0, t, X, X, tri); return; }
        }
    }
    {
        double Q[3], e[3];
        closest_pt_triangle(P0, A, B, C, Q);
        sub3(P0, Q, e);
        take(b, sqrt(dot3(e, e)), 0.0, P0, Q, tri);
        closest_pt_triangle(P1, A, B, C, Q);
        sub3(P1, Q, e);
        take(b, sqrt(dot3(e, e)), D == 0.0 ? 0.0 : 1.0, P1, Q, tri);
    }
#pragma unroll 1
    for (int k = 0; k < 3; ++k) {
        const double *ea = T + 3 * k, *eb = T + 3 * ((k + 1) % 3);
        double p6[6], tt;
        const double dis = seg_seg_full(P0, P1, ea, eb, &tt, p6);
        double tpar = 0.0;
        if (D != 0.0) { double e[3]; sub3(p6, P0, e); tpar = dot3(e, d) / D; }
        take(b, dis, tpar, p6, p6 + 3, tri);
    }
}

// Rigorous lower bound of dist(segment, box), normally the distance itself.  f(t) = dist^2(P0 + t d, box) is convex and
// piecewise quadratic: on the piece where the set of violated slabs is fixed it is sum_r (e_r + t d_r)^2.  Starting from
// the middle, minimise the current piece and move there; when the minimiser lies in its own piece it is the global one
// (convexity).  That takes 2-3 rounds; a point that sits exactly on a slab boundary can make the pattern alternate, and
// then the bound falls back to a cover of the segment by LB_BALLS balls (radius |d| / (2 LB_BALLS)) plus the box-box
// distance -- any lower bound of a cover is a lower bound of the segment.
#ifndef CFS_LB_BALLS
#define CFS_LB_BALLS 4
#endif
__device__ double node_lower_bound(const double *P0, const double *P1, const double *blo, const double *bhi)
{
    double d[3];
    sub3(P1, P0, d);
    const double len2 = dot3(d, d);
    if (len2 > 0.0) {
        double t = 0.5;
#pragma unroll 1
        for (int it = 0; it < 5; ++it) {
            double A = 0.0, B = 0.0, C = 0.0;
            int pat = 0;
#pragma unroll
            for (int r = 0; r < 3; ++r) {
                const double p = P0[r] + t * d[r];
                if (p < blo[r]) { const double e = P0[r] - blo[r]; A += d[r] * d[r]; B += e * d[r]; C += e * e; pat |= 1 << (2 * r); }
                else if (p > bhi[r]) { const double e = P0[r] - bhi[r]; A += d[r] * d[r]; B += e * d[r]; C += e * e; pat |= 2 << (2 * r); }
            }
            if (pat == 0) return 0.0;                            // the point is inside the box
            const double tn = A > 0.0 ? fmin(1.0, fmax(0.0, -B / A)) : t;
            int pat2 = 0;
#pragma unroll
            for (int r = 0; r < 3; ++r) {
                const double p = P0[r] + tn * d[r];
                if (p < blo[r]) pat2 |= 1 << (2 * r);
                else if (p > bhi[r]) pat2 |= 2 << (2 * r);
            }
            if (pat2 == pat) {                                   // the minimiser of this piece lies in this piece: global minimum
                double v = 0.0;                                  // sum of squares at tn, term by term: no cancellation when the
#pragma unroll                                                   // segment touches the box (A tn^2 + 2 B tn + C would lose it)
                for (int r = 0; r < 3; ++r) {
                    const double p = P0[r] + tn * d[r];
                    const double g = fmax(0.0, fmax(blo[r] - p, p - bhi[r]));
                    v += g * g;
                }
                return sqrt(v) * (1.0 - 1e-12) - 1e-13 * (1.0 + sqrt(C));   // shaved: stays a lower bound under rounding
            }
            t = tn;
        }
    }
    constexpr int NB = CFS_LB_BALLS;
    double bb = 0.0;
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        const double lo = fmin(P0[r], P1[r]), hi = fmax(P0[r], P1[r]);
        const double g = fmax(0.0, fmax(blo[r] - hi, lo - bhi[r]));
        bb += g * g;
    }
    bb = sqrt(bb);
    if (len2 == 0.0) return bb * (1.0 - 1e-14);              // a point: the box-box bound is the exact point-box distance
    const double rad = sqrt(len2) * (0.5 / NB);
    double sp2 = INFINITY;
#pragma unroll
    for (int i = 0; i < NB; ++i) {
        const double f = (2 * i + 1) * (0.5 / NB);
        double g2 = 0.0;
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            const double c = P0[r] + f * d[r];
            const double g = fmax(0.0, fmax(blo[r] - c, c - bhi[r]));
            g2 += g * g;
        }
        sp2 = fmin(sp2, g2);
    }
    const double sp = sqrt(sp2);
    // the balls' bound loses a few ulp in rad and the square root: shave it so that it stays a lower bound
    const double spb = (sp - rad) - 1e-12 * (sp + rad);
    return fmax(bb * (1.0 - 1e-14), fmax(0.0, spb));
}

// Triangles whose distance is within `margin` of the minimum, gathered while a query runs (LDS, strided like the stack).
// A pose shifted by less than margin/2 has its closest triangle among them, so the shifted poses of num_jac need no traversal.
constexpr int NEAR_CAP = 12;
struct NearList {
    int *idx;            // [NEAR_CAP] strided
    float *dd;           // [NEAR_CAP] strided, distances rounded DOWN (an entry is never dropped wrongly, at worst kept needlessly)
    double margin;
    int n;
    bool over;           // more than NEAR_CAP triangles tie within the margin: the caller falls back to traversals
};
template <int STRIDE>
__device__ __forceinline__ void near_compact(NearList &nl, double best)
{
    int w = 0;
    for (int i = 0; i < nl.n; ++i)
        if ((double)nl.dd[i * STRIDE] <= best + nl.margin) { nl.idx[w * STRIDE] = nl.idx[i * STRIDE]; nl.dd[w * STRIDE] = nl.dd[i * STRIDE]; ++w; }
    nl.n = w;
}

// nearest-first traversal; the thread's private stack (node, lower bound) lives in LDS, strided by STRIDE
// `bound`: only triangles closer than this matter to the caller (b.tri stays -1 when there is none)
template <int STRIDE, bool COLLECT>
__device__ void mesh_query(const DevMesh &m, const double *P0, const double *P1, int seed_tri, int *stack, float *lbs, Best &b, NearList *nl,
                           double bound = INFINITY)
{
    b.d = bound; b.t = INFINITY; b.tri = -1;
#pragma unroll
    for (int r = 0; r < 6; ++r) b.pts[r] = 0.0;
    if (m.nt == 0) return;
    if (seed_tri >= 0) seg_tri_update(P0, P1, m.tri + 9 * (size_t)seed_tri, seed_tri, b);   // incumbent from a nearby query
    int sp = 0;
    int cur = 0;                                            // the root is always an inner node (upload_mesh)
    const double slack = COLLECT ? nl->margin : 0.0;        // with a collector, everything within the margin must be visited
    for (;;) {
        if (cur < 0) {                                      // leaf
            const int code = -(cur + 1), first = code >> 3, count = code & 7;
            for (int k = first; k < first + count; ++k) {
                if (k == seed_tri) continue;
                if (COLLECT) {
                    Best tb;
                    tb.d = INFINITY; tb.t = INFINITY; tb.tri = -1;
                    seg_tri_update(P0, P1, m.tri + 9 * (size_t)k, k, tb);
                    take(b, tb.d, tb.t, tb.pts, tb.pts + 3, k);
                    if (!nl->over && tb.d <= b.d + nl->margin) {
                        if (nl->n == NEAR_CAP) near_compact<STRIDE>(*nl, b.d);
                        if (nl->n == NEAR_CAP) nl->over = true;
                        else { nl->idx[nl->n * STRIDE] = k; nl->dd[nl->n * STRIDE] = __double2float_rd(tb.d); ++nl->n; }
                    }
                } else {
                    seg_tri_update(P0, P1, m.tri + 9 * (size_t)k, k, b);
                }
            }
            cur = 0x7fffffff;
        } else {
            const BvhNode nd = m.nodes[cur];                // one load: both children's boxes
            const double ll = node_lower_bound(P0, P1, nd.lo[0], nd.hi[0]);
            const double lr = node_lower_bound(P0, P1, nd.lo[1], nd.hi[1]);
            const int nearc = ll <= lr ? nd.child[0] : nd.child[1], farc = ll <= lr ? nd.child[1] : nd.child[0];
            const double ln = fmin(ll, lr), lf = fmax(ll, lr);
            cur = 0x7fffffff;
            if (ln <= b.d + slack) {
                cur = nearc;
                if (lf <= b.d + slack && sp < MESH_STACK) { stack[sp * STRIDE] = farc; lbs[sp * STRIDE] = __double2float_rd(lf); ++sp; }
            }
        }
        while (cur == 0x7fffffff) {
            if (sp == 0) { if (COLLECT) near_compact<STRIDE>(*nl, b.d); return; }
            --sp;
            if ((double)lbs[sp * STRIDE] <= b.d + slack) cur = stack[sp * STRIDE];   // the incumbent may have improved since the push
        }
    }
}

__device__ __forceinline__ double with_surrogate(const Best &bq, const double *a6)
{
    double dis = bq.d;
    if (fabs(dis) < 0.0001) {                                // dist_arm_surf_200i.m:22-24
        const double qx = bq.pts[0] - a6[3], qy = bq.pts[1] - a6[4], qz = bq.pts[2] - a6[5];
        dis = -sqrt(qx * qx + qy * qy + qz * qz);
    }
    return dis;
}

}  // namespace
