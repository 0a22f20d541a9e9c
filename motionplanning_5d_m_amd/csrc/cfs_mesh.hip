// cfs_mesh.hip -- mesh obstacles: binary-STL loader, BVH, segment-to-mesh distance
// (the `point2surface_dis` the reference calls but does not contain: M200i/dist_arm_surf_200i.m:21,
// Lib/functions/dist_arm_surface.m:43), dist_arm over a mesh, and the linearisation (distance + literal
// num_jac gradient) of mesh obstacles that feeds the fused solver.
//
// Contract (the build's own, DESIGN.md "Mesh obstacles"): dis = min over triangles of the Euclidean distance
// between the link axis and the triangle (0 when they intersect); points = [closest point on the axis; closest
// point on the mesh]; equal distances resolve to the smaller parameter along the axis, so the answer does not
// depend on the traversal order.  The hierarchy only prunes: a node is skipped when a rigorous lower bound of
// its distance exceeds the incumbent.
#include "cfs_mesh_dev.h"
#include "cfs_host.h"
#include "cfs_mesh_query_dev.h"
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <numeric>

namespace {

// ---- device geometry, the traversal (mesh_query) and the near-zero surrogate: cfs_mesh_dev.h ----------------------

// ---- kernels ------------------------------------------------------------------------------------------
// point2surface_dis (cfs_mesh_seg_kernel): cfs_mesh_query_dev.h.  The public entry is cfs_mesh_query.hip's build of it (no FMA
// contraction); this unit's build is cfs_debug_mesh_segment_distance_contracted
// dist_arm over a mesh (M200i/dist_arm_surf_200i.m:1-29): one thread per (pose, link), min over links in LDS
struct ArmMeshParams { const DevRobot *rb; DevMesh m; int N, nj; const double *theta; double *d; int *linkid; double *pts; };

__global__ __launch_bounds__(MESH_THREADS) void cfs_dist_arm_mesh_kernel(ArmMeshParams P)
{
    __shared__ int s_stack[MESH_STACK * MESH_THREADS];
    __shared__ float s_lbs[MESH_STACK * MESH_THREADS];
    __shared__ double s_dis[MESH_THREADS];
    __shared__ double s_pts[MESH_THREADS * 6];
    const int nj = P.nj, per = MESH_THREADS / nj;           // poses per workgroup
    const int lp = threadIdx.x / nj, k = threadIdx.x - lp * nj;
    const int pose = blockIdx.x * per + lp;
    const bool live = lp < per && pose < P.N;
    double dis = INFINITY;
    if (live) {
        const DevRobot *rb = P.rb;
        double M[12], Mn[12], e6[6];
        for (int k1 = 0; k1 <= k; ++k1) {                    // CapPos.m:13-20 up to this thread's link
            double sn, cs;
            sincos(P.theta[(size_t)pose * nj + k1] - rb->th_off[k1], &sn, &cs);
            fk_step(rb, k1, sn, cs, k1 == 0 ? nullptr : M, Mn);
            for (int q = 0; q < 12; ++q) M[q] = Mn[q];
        }
        link_ends(rb, k, M, e6);
        Best b;
        mesh_query<MESH_THREADS, false>(P.m, e6, e6 + 3, -1, s_stack + threadIdx.x, s_lbs + threadIdx.x, b, nullptr);
        dis = b.d;
        if (fabs(dis) < 0.0001) {                            // dist_arm_surf_200i.m:22-24
            const double qx = b.pts[0] - e6[3], qy = b.pts[1] - e6[4], qz = b.pts[2] - e6[5];
            dis = -sqrt(qx * qx + qy * qy + qz * qz);
        }
        for (int r = 0; r < 6; ++r) s_pts[threadIdx.x * 6 + r] = b.pts[r];
    }
    s_dis[threadIdx.x] = dis;
    __syncthreads();
    if (live && k == 0) {
        double d = INFINITY;
        int id = 0;
        for (int i = 0; i < nj; ++i) { const double v = s_dis[lp * nj + i]; if (v < d) { d = v; id = i + 1; } }   // :25-28, first minimum wins
        P.d[pose] = d;
        if (P.linkid) P.linkid[pose] = id;
        if (P.pts && id > 0)
            for (int r = 0; r < 6; ++r) P.pts[(size_t)pose * 6 + r] = s_pts[(lp * nj + id - 1) * 6 + r];
    }
}

// Linearisation against mesh obstacles: the same scheme as cfs_fused.hip (link variants, base distances, pruned
// candidates, minima per evaluation point of num_jac), the distance being a hierarchy query.  Four kernels, every one
// with a thread per item, so that the expensive cold traversals of the base pose fill the machine:
//   fk     (b, waypoint, evaluation point) -> end points of every link variant
//   upper  (b, waypoint, link, mesh)       -> greedy upper bound of the base-pose distance (one descent)
//   base   (b, waypoint, link, mesh, piece)-> distance + winning triangle at the base pose per quarter of the link axis, for what can matter
//   reduce (b, waypoint, link, mesh)       -> the link's minimum over its pieces, surrogate, merged near-tie list
//   shift  (b, waypoint, mesh, variant)    -> distance at the shifted poses of the links that can be the minimum there,
//                                             started from the base pose's triangle (their traversals prune almost everything)
//   fd     (b, waypoint, mesh)             -> minima per evaluation point, distance and literal num_jac gradient
template <int NJ>
__global__ __launch_bounds__(MESH_THREADS) void mesh_fk_kernel(LinMeshParams P)
{
    constexpr int NS = 2 * NJ, NVT = nvt(NJ), NE = 2 * NJ + 1;
    const int e = blockIdx.x * MESH_THREADS + threadIdx.x;
    if (e >= P.B * P.H * NE) return;
    const int ev = e % NE, wp = (e / NE) % P.H, b = e / (NE * P.H);
    if (P.status_done && P.status_done[b] != 0) return;
    const DevRobot *rb = P.rb;
    double M[12], Mn[12], e6[6];
#pragma unroll
    for (int k1 = 1; k1 <= NJ; ++k1) {
        // evaluation point ev has joint m at +eps/2 if ev == 2m-1 and at -eps/2 if ev >= 2m (num_jac.m:8-14: xp is never restored)
        double x = P.x_[((size_t)b * P.H + wp) * NS + k1 - 1];
        if (ev == 2 * k1 - 1) x = x + FD_EPS / 2;            // num_jac.m:11
        else if (ev >= 2 * k1) x = x - FD_EPS / 2;           // num_jac.m:13
        x = x - rb->th_off[k1 - 1];                          // same joint offset as dist_arm_3D_200i_2.m:11
        double sn, cs;
        sincos(x, &sn, &cs);
        fk_step(rb, k1 - 1, sn, cs, k1 == 1 ? nullptr : M, Mn);
#pragma unroll
        for (int q = 0; q < 12; ++q) M[q] = Mn[q];
        if (ev <= 2 * k1) {                                  // link k1 at evaluation point ev is variant min(ev, 2 k1): stored by its owner
            link_ends(rb, k1 - 1, M, e6);
            double *dst = P.ends + (((size_t)b * P.H + wp) * NVT + kvoff(k1) + ev) * 6;
#pragma unroll
            for (int q = 0; q < 6; ++q) dst[q] = e6[q];
        }
    }
}

// one descent to the nearest leaf, no backtracking: an upper bound of the distance for ~2 log2(nt) box bounds
__device__ double mesh_greedy_upper(const DevMesh &m, const double *P0, const double *P1)
{
    if (m.nt == 0) return INFINITY;
    int cur = 0;
    for (;;) {
        if (cur < 0) {
            const int code = -(cur + 1), first = code >> 3, count = code & 7;
            Best b;
            b.d = INFINITY; b.t = INFINITY; b.tri = -1;
            for (int k = first; k < first + count; ++k) seg_tri_update(P0, P1, m.tri + 9 * (size_t)k, k, b);
            return b.d;
        }
        const BvhNode nd = m.nodes[cur];
        cur = node_lower_bound(P0, P1, nd.lo[0], nd.hi[0]) <= node_lower_bound(P0, P1, nd.lo[1], nd.hi[1]) ? nd.child[0] : nd.child[1];
    }
}

// End points of link variant `var` at (b, wp), in the frame mesh jm is stored in.  A static handle (mesh_pose null) reads them as
// mesh_fk_kernel wrote them.  With mesh motion (cfs_problem_set_mesh_motion) both go through the inverse pose of (mesh, waypoint):
// a rigid map, so every distance, bound and near-tie margin downstream holds unchanged, and equal end points (a point link) stay
// equal.  POSED is the launch's: a static handle runs the instantiations without the transform, its code is what it always was.
template <int NVT, bool POSED>
__device__ __forceinline__ void mesh_link_ends(const LinMeshParams &P, int b, int wp, int var, int jm, double *a6)
{
    const double *src = P.ends + (((size_t)b * P.H + wp) * NVT + var) * 6;
#pragma unroll
    for (int q = 0; q < 6; ++q) a6[q] = src[q];
    if constexpr (POSED) {
        const double *T = P.mesh_pose + ((size_t)jm * P.H + wp) * 12;   // row-major [R' | -R't]
        double t[12];
#pragma unroll
        for (int q = 0; q < 12; ++q) t[q] = T[q];
#pragma unroll
        for (int e = 0; e < 6; e += 3) {
            const double x = a6[e], y = a6[e + 1], z = a6[e + 2];
#pragma unroll
            for (int r = 0; r < 3; ++r) a6[e + r] = t[4 * r] * x + t[4 * r + 1] * y + t[4 * r + 2] * z + t[4 * r + 3];
        }
    }
}

template <int NJ, bool POSED>
__global__ __launch_bounds__(MESH_THREADS, 2) void mesh_upper_kernel(LinMeshParams P)
{
    constexpr int NVT = nvt(NJ);
    const int e = blockIdx.x * MESH_THREADS + threadIdx.x;
    if (e >= P.B * P.H * NJ * P.nmesh) return;
    const int wp = e % P.H, b = (e / P.H) % P.B, jm = (e / (P.H * P.B)) % P.nmesh, k0 = e / (P.H * P.B * P.nmesh);
    if (P.status_done && P.status_done[b] != 0) return;
    double a6[6];
    mesh_link_ends<NVT, POSED>(P, b, wp, kvoff(k0 + 1), jm, a6);
    const size_t o = (((size_t)b * P.H + wp) * NJ + k0) * P.nmesh + jm;
    double up = mesh_greedy_upper(P.meshes[jm], a6, a6 + 3);
    if (P.seed_prev) {
        const int tp = P.base_t[o];
        if (tp >= 0 && tp < P.meshes[jm].nt) {
            Best bp;
            bp.d = INFINITY; bp.t = INFINITY; bp.tri = -1;
            seg_tri_update(a6, a6 + 3, P.meshes[jm].tri + 9 * (size_t)tp, tp, bp);
            up = fmin(up, bp.d);
        }
    }
    P.upper_d[o] = up;
}

// A link axis is queried in MESH_PIECES equal pieces: the pieces far from the surface die at the root against the common
// bound, and the others have short verification sets.  dist(link, T) = min over the pieces of dist(piece, T).
#ifndef CFS_MESH_PIECES
#define CFS_MESH_PIECES 4
#endif
constexpr int MESH_PIECES = CFS_MESH_PIECES;
constexpr int PIECE_D = 5;                                   // per piece: raw distance, parameter along the whole axis, closest point on the axis
constexpr int PIECE_I = 2 + NEAR_CAP;                        // winning triangle, near count (-1: overflow), near triangles

// ---- wave-cooperative query: one wavefront works on ONE query at a time, 64 hierarchy nodes or 64 triangles per round, so no
// lane waits for another lane's longer traversal.  Same semantics as mesh_query<.., true> (lexicographic minimum, near list).
#ifndef CFS_CO_QPW
#define CFS_CO_QPW 16
#endif
constexpr int CO_FR = 768, CO_TR = 320, CO_QPW = CFS_CO_QPW;   // frontier / triangle buffer of a wavefront; queries set up per wavefront
static_assert(64 + 128 * LEAF_TRIS <= CO_TR, "a round of 64 nodes can emit 128 leaves");
struct CoopLds {
    int fr[CO_FR];
    int tr[CO_TR];
    double cb[128 * 6];      // boxes (lo, hi) of the children a round could not rule out cheaply, compacted
    int cc[128];             // their child codes
    int ni[NEAR_CAP];
    float nd[NEAR_CAP];
};
__device__ __forceinline__ double wmin64(double v)
{
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v = fmin(v, __shfl_xor(v, m, 64));
    return v;
}
__device__ __forceinline__ int prefix_of(unsigned long long mask, int lane) { return __popcll(mask & ((1ull << lane) - 1ull)); }

// false: a buffer would overflow (the caller repeats the query sequentially)
__device__ bool mesh_query_coop(const DevMesh &m, const double *P0, const double *P1, CoopLds &L, int lane, double bound, double margin,
                                Best &b, int &near_n, bool &near_over)
{
    b.d = bound; b.t = INFINITY; b.tri = -1;
#pragma unroll
    for (int r = 0; r < 6; ++r) b.pts[r] = 0.0;
    near_n = 0; near_over = false;
    if (m.nt == 0) return true;
    int nf = m.ncut, nt = m.ncut_tri;                           // start at the cut (<= 64 inner nodes, <= 254 triangles), not at the root
    if (lane < nf) L.fr[lane] = m.cut[lane];
    for (int k = lane; k < nt; k += 64) L.tr[k] = m.cut_tri[k];
    __syncthreads();
    while (nf > 0 || nt > 0) {
        if (nf > 0 && nt < 64) {
            // expand up to 64 inner nodes from the end of the frontier (depth first in blocks of 64)
            if (nf + 64 > CO_FR) return false;
            const int take = min(nf, 64);
            nf -= take;
            const bool act = lane < take;
            const int ref = act ? L.fr[nf + lane] : 0;
            __syncthreads();
            // Two passes.  Most children of a round are far away: the box-box distance between the segment's bounding box and
            // the child's (a lower bound of the true distance, ~20 flops) rules them out.  An inner child that passes is
            // opened; a leaf that passes is compacted through LDS, so the exact segment-box bound (2-5 Newton rounds,
            // divergent) runs once over dense lanes and only where it saves triangle tests.
            const double lim = b.d + margin, lim2 = lim * lim * (1.0 + 1e-13);
            int nc = 0;
            {
                BvhNode nd;
                if (act) nd = m.nodes[ref];
#pragma unroll
                for (int c = 0; c < 2; ++c) {
                    bool cand = false;
                    if (act) {
                        double g2 = 0.0;
#pragma unroll
                        for (int r = 0; r < 3; ++r) {
                            const double lo = fmin(P0[r], P1[r]), hi = fmax(P0[r], P1[r]);
                            const double g = fmax(0.0, fmax(nd.lo[c][r] - hi, lo - nd.hi[c][r]));
                            g2 += g * g;
                        }
                        cand = !(g2 * (1.0 - 1e-13) > lim2);      // an empty child has lo = +inf: g2 = inf, never a candidate
                    }
                    const bool inner = cand && nd.child[c] >= 0;
                    const unsigned long long mi = __ballot(inner);
                    if (inner) L.fr[nf + prefix_of(mi, lane)] = nd.child[c];
                    nf += __popcll(mi);
                    const bool leafc = cand && nd.child[c] < 0 && ((-(nd.child[c] + 1)) & 7) > 0;
                    const unsigned long long mk = __ballot(leafc);
                    if (leafc) {
                        const int sl = nc + prefix_of(mk, lane);
#pragma unroll
                        for (int r = 0; r < 3; ++r) { L.cb[sl * 6 + r] = nd.lo[c][r]; L.cb[sl * 6 + 3 + r] = nd.hi[c][r]; }
                        L.cc[sl] = nd.child[c];
                    }
                    nc += __popcll(mk);
                }
            }
            __syncthreads();
            for (int base = 0; base < nc; base += 64) {
                const int sl = base + lane;
                const bool has_c = sl < nc;
                double lcx = INFINITY;
                int chx = 0;
                if (has_c) {
                    double blo[3], bhi[3];
#pragma unroll
                    for (int r = 0; r < 3; ++r) { blo[r] = L.cb[sl * 6 + r]; bhi[r] = L.cb[sl * 6 + 3 + r]; }
                    chx = L.cc[sl];
                    // measured per solve, exact bound everywhere / nowhere / leaves only: config 5 9.6 / 8.3 / 8.7 ms, one
                    // 5 120-triangle sphere 116 / 122 / 110 ms, posts + beam 17.3 / 15.9 / 16.3 ms
                    lcx = node_lower_bound(P0, P1, blo, bhi);
                }
                const bool q = has_c && lcx <= lim;
                const int code = -(chx + 1), first = code >> 3, cnt = q ? (code & 7) : 0;
#pragma unroll
                for (int k = 0; k < LEAF_TRIS; ++k) {
                    const bool has = k < cnt;
                    const unsigned long long mt = __ballot(has);
                    if (has) L.tr[nt + prefix_of(mt, lane)] = first + k;
                    nt += __popcll(mt);
                }
            }
            __syncthreads();
        } else {
            // test up to 64 triangles, one per lane
            const int take = min(nt, 64);
            nt -= take;
            const int k = lane < take ? L.tr[nt + lane] : -1;
            __syncthreads();
            Best tb;
            tb.d = INFINITY; tb.t = INFINITY; tb.tri = -1;
#pragma unroll
            for (int r = 0; r < 6; ++r) tb.pts[r] = 0.0;
            if (k >= 0) seg_tri_update(P0, P1, m.tri + 9 * (size_t)k, k, tb);
            const double dmin = wmin64(tb.d);
            const double tmin = wmin64(tb.d == dmin ? tb.t : INFINITY);
            if (dmin < b.d || (dmin == b.d && tmin < b.t)) {
                const unsigned long long win = __ballot(tb.d == dmin && tb.t == tmin);
                const int wl = (int)__builtin_ctzll(win);
                b.d = dmin; b.t = tmin; b.tri = __shfl(tb.tri, wl, 64);
#pragma unroll
                for (int r = 0; r < 6; ++r) b.pts[r] = __shfl(tb.pts[r], wl, 64);
            }
            if (!near_over) {
                const bool nr = k >= 0 && tb.d <= b.d + margin;
                const unsigned long long mn = __ballot(nr);
                const int add = __popcll(mn);
                if (near_n + add > NEAR_CAP) {                // compact what is there against the current minimum first
                    const bool keep = lane < near_n && (double)L.nd[lane] <= b.d + margin;
                    const int ki = lane < near_n ? L.ni[lane] : 0;
                    const float kd = lane < near_n ? L.nd[lane] : 0.0f;
                    const unsigned long long mkp = __ballot(keep);
                    __syncthreads();
                    if (keep) { L.ni[prefix_of(mkp, lane)] = ki; L.nd[prefix_of(mkp, lane)] = kd; }
                    near_n = __popcll(mkp);
                    __syncthreads();
                }
                if (near_n + add > NEAR_CAP) near_over = true;
                else {
                    if (nr) { L.ni[near_n + prefix_of(mn, lane)] = k; L.nd[near_n + prefix_of(mn, lane)] = __double2float_rd(tb.d); }
                    near_n += add;
                }
                __syncthreads();
            }
        }
    }
    if (!near_over) {                                          // final filter against the final minimum
        const bool keep = lane < near_n && (double)L.nd[lane] <= b.d + margin;
        const int ki = lane < near_n ? L.ni[lane] : 0;
        const float kd = lane < near_n ? L.nd[lane] : 0.0f;
        const unsigned long long mkp = __ballot(keep);
        __syncthreads();
        if (keep) { L.ni[prefix_of(mkp, lane)] = ki; L.nd[prefix_of(mkp, lane)] = kd; }
        near_n = __popcll(mkp);
        __syncthreads();
    }
    return true;
}

template <int NJ, bool POSED>
__global__ __launch_bounds__(64) void mesh_base_kernel(LinMeshParams P)
{
    constexpr int NVT = nvt(NJ);
    __shared__ CoopLds L;
    const int lane = threadIdx.x;
    const int total = P.B * P.H * NJ * P.nmesh * MESH_PIECES;
    // Stage 1, a query per lane: set it up and test it against the root's two boxes.  Most pieces of most links have nothing
    // within their bound and end here.  Piece and link index fastest: every wavefront gets its share of the few that survive
    // (stage 2 takes them one after the other).
    const int e = blockIdx.x * CO_QPW + lane;
    bool live = lane < CO_QPW && e < total;
    int jm = 0, pc = 0;
    size_t o = 0;
    bool point = false;
    double s6[6] = {0, 0, 0, 0, 0, 0}, bound = 0.0;
    const double margin = 4.0 * P.rb->shift_bound;              // twice what the argument needs (see NearList)
    if (live) {
        pc = e % MESH_PIECES;
        const int k0 = (e / MESH_PIECES) % NJ;
        jm = (e / (MESH_PIECES * NJ)) % P.nmesh;
        const int wp = (e / (MESH_PIECES * NJ * P.nmesh)) % P.H, b = e / (MESH_PIECES * NJ * P.nmesh * P.H);
        live = !(P.status_done && P.status_done[b] != 0);
        o = (((size_t)b * P.H + wp) * NJ + k0) * P.nmesh + jm;
        if (live) {
            double a6[6], d[3];
            mesh_link_ends<NVT, POSED>(P, b, wp, kvoff(k0 + 1), jm, a6);
            sub3(a6 + 3, a6, d);
            point = dot3(d, d) == 0.0;                           // M200i links 1 and 3 are points: one "piece"
#pragma unroll
            for (int r = 0; r < 3; ++r) {
                s6[r] = point || pc == 0 ? a6[r] : a6[r] + ((double)pc / MESH_PIECES) * d[r];
                s6[3 + r] = point || pc == MESH_PIECES - 1 ? a6[3 + r] : a6[r] + ((double)(pc + 1) / MESH_PIECES) * d[r];
            }
            // Only the minimum over the links and the links within prune_tol of it matter (see mesh_shift_kernel), and the
            // minimum is at most the smallest greedy upper bound: a piece with nothing closer than `bound` is out.
            double umin = INFINITY;
#pragma unroll
            for (int kk = 0; kk < NJ; ++kk) umin = fmin(umin, P.upper_d[(((size_t)b * P.H + wp) * NJ + kk) * P.nmesh + jm]);
            bound = (fmax(umin, 0.0001) + P.rb->prune_tol) * (1.0 + 1e-12) + margin;
            double *rec = P.piece_d + (o * MESH_PIECES + pc) * PIECE_D;
            int *reci = P.piece_i + (o * MESH_PIECES + pc) * PIECE_I;
            rec[0] = INFINITY; rec[1] = INFINITY; rec[2] = rec[3] = rec[4] = 0.0; reci[0] = -1; reci[1] = 0;   // "nothing within the bound"
            bool go = !(point && pc > 0) && P.meshes[jm].nt > 0;
            if (go) {                                            // box of the piece against the boxes of the root's children (cheap; the
                const BvhNode nd = P.meshes[jm].nodes[0];        // cut round of stage 2 is cheap too for what slips through)
                const double lim = bound + margin, lim2 = lim * lim * (1.0 + 1e-13);
                double g2min = INFINITY;
#pragma unroll
                for (int c = 0; c < 2; ++c) {
                    double g2 = 0.0;
#pragma unroll
                    for (int r = 0; r < 3; ++r) {
                        const double lo = fmin(s6[r], s6[3 + r]), hi = fmax(s6[r], s6[3 + r]);
                        const double g = fmax(0.0, fmax(nd.lo[c][r] - hi, lo - nd.hi[c][r]));
                        g2 += g * g;
                    }
                    g2min = fmin(g2min, g2);
                }
                go = !(g2min * (1.0 - 1e-13) > lim2);
            }
            live = go;
        }
    }
    // Stage 2, the survivors one at a time, the whole wavefront on each.
    unsigned long long todo = __ballot(live);
    while (todo) {
        const int src = (int)__builtin_ctzll(todo);
        todo &= todo - 1;
        double q6[6];
#pragma unroll
        for (int r = 0; r < 6; ++r) q6[r] = __shfl(s6[r], src, 64);
        const double qbound = __shfl(bound, src, 64);
        const int qjm = __shfl(jm, src, 64), qpc = __shfl(pc, src, 64);
        const bool qpoint = __shfl((int)point, src, 64) != 0;
        const unsigned long long qo = __shfl((unsigned long long)o, src, 64);
        double *rec = P.piece_d + (qo * MESH_PIECES + qpc) * PIECE_D;
        int *reci = P.piece_i + (qo * MESH_PIECES + qpc) * PIECE_I;
        double *recn = P.piece_nd + (qo * MESH_PIECES + qpc) * NEAR_CAP;
        Best bq;
        int near_n;
        bool near_over;
        __syncthreads();
        if (!mesh_query_coop(P.meshes[qjm], q6, q6 + 3, L, lane, qbound, margin, bq, near_n, near_over)) {
            // a buffer was about to overflow: lane 0 repeats the query with the sequential traversal (its stack in the same LDS)
            __syncthreads();
            NearList nl;
            nl.idx = L.ni; nl.dd = L.nd; nl.n = 0; nl.over = false; nl.margin = margin;
            if (lane == 0) mesh_query<1, true>(P.meshes[qjm], q6, q6 + 3, -1, L.fr, reinterpret_cast<float *>(L.tr), bq, &nl, qbound);
            __syncthreads();
            bq.d = __shfl(bq.d, 0, 64); bq.t = __shfl(bq.t, 0, 64); bq.tri = __shfl(bq.tri, 0, 64);
#pragma unroll
            for (int r = 0; r < 6; ++r) bq.pts[r] = __shfl(bq.pts[r], 0, 64);
            near_n = __shfl(nl.n, 0, 64);
            near_over = __shfl((int)nl.over, 0, 64) != 0;
        }
        if (bq.tri >= 0) {
            if (lane == 0) {
                rec[0] = bq.d;
                rec[1] = qpoint ? 0.0 : ((double)qpc + bq.t) / MESH_PIECES;
                rec[2] = bq.pts[0]; rec[3] = bq.pts[1]; rec[4] = bq.pts[2];
                reci[0] = bq.tri;
                reci[1] = near_over ? -1 : near_n;
            }
            if (!near_over && lane < near_n) { reci[2 + lane] = L.ni[lane]; recn[lane] = (double)L.nd[lane]; }
        }
        __syncthreads();
    }
}

// pieces -> link: lexicographic minimum (distance, parameter), surrogate, and the union of the pieces' near lists
template <int NJ, bool POSED>
__global__ __launch_bounds__(MESH_THREADS) void mesh_reduce_kernel(LinMeshParams P)
{
    constexpr int NVT = nvt(NJ);
    const int e = blockIdx.x * MESH_THREADS + threadIdx.x;
    if (e >= P.B * P.H * NJ * P.nmesh) return;
    const int jm = e % P.nmesh, k0 = (e / P.nmesh) % NJ, wp = (e / (P.nmesh * NJ)) % P.H, b = e / (P.nmesh * NJ * P.H);
    if (P.status_done && P.status_done[b] != 0) return;
    const size_t o = (((size_t)b * P.H + wp) * NJ + k0) * P.nmesh + jm;
    Best bq;
    bq.d = INFINITY; bq.t = INFINITY; bq.tri = -1;
    for (int pc = 0; pc < MESH_PIECES; ++pc) {
        const double *rec = P.piece_d + (o * MESH_PIECES + pc) * PIECE_D;
        const int tri = P.piece_i[(o * MESH_PIECES + pc) * PIECE_I];
        if (tri >= 0) take(bq, rec[0], rec[1], rec + 2, rec + 2, tri);
    }
    int *near = P.near + o * (NEAR_CAP + 1);
    if (bq.tri < 0) { P.base_d[o] = INFINITY; P.base_t[o] = -1; near[0] = 0; return; }   // farther than the bound: never the minimum, never a candidate
    double t6[6];                                            // the closest point is in the mesh's frame: so must the link end be
    const double *a6 = P.ends + (((size_t)b * P.H + wp) * NVT + kvoff(k0 + 1)) * 6;
    if constexpr (POSED) { mesh_link_ends<NVT, true>(P, b, wp, kvoff(k0 + 1), jm, t6); a6 = t6; }
    P.base_d[o] = with_surrogate(bq, a6);
    P.base_t[o] = bq.tri;
    const double lim = bq.d + 4.0 * P.rb->shift_bound;
    int n = 0;
    bool over = false;
    for (int pc = 0; pc < MESH_PIECES && !over; ++pc) {
        const int *reci = P.piece_i + (o * MESH_PIECES + pc) * PIECE_I;
        const double *recn = P.piece_nd + (o * MESH_PIECES + pc) * NEAR_CAP;
        if (reci[0] < 0) continue;
        // a piece whose own minimum is beyond the limit contributes nothing, whatever its list says
        if (P.piece_d[(o * MESH_PIECES + pc) * PIECE_D] > lim) continue;
        if (reci[1] < 0) { over = true; break; }
        for (int i = 0; i < reci[1]; ++i) {
            if (recn[i] > lim) continue;
            bool dup = false;
            for (int w = 0; w < n; ++w) dup = dup || near[1 + w] == reci[2 + i];
            if (dup) continue;
            if (n == NEAR_CAP) { over = true; break; }
            near[1 + n++] = reci[2 + i];
        }
    }
    near[0] = over ? -1 : n;                                 // < 0: too many ties, the shifted poses traverse instead
}

template <int NJ, bool POSED>
__global__ __launch_bounds__(MESH_THREADS, 2) void mesh_shift_kernel(LinMeshParams P)
{
    constexpr int NVT = nvt(NJ), NSV = NVT - NJ;
    __shared__ int s_stack[MESH_STACK * MESH_THREADS];
    __shared__ float s_lbs[MESH_STACK * MESH_THREADS];
    const int e = blockIdx.x * MESH_THREADS + threadIdx.x;
    if (e >= P.B * P.H * P.nmesh * NSV) return;
    const int wp = e % P.H, b = (e / P.H) % P.B, jm = (e / (P.H * P.B)) % P.nmesh, sv = e / (P.H * P.B * P.nmesh);   // variant slowest (see base)
    if (P.status_done && P.status_done[b] != 0) return;
    int k1 = 1, v = 1;                                       // sv enumerates (link k1, variant v = 1..2 k1)
    {
        int acc = 0;
#pragma unroll
        for (int kk = 1; kk <= NJ; ++kk) { if (sv >= acc && sv < acc + 2 * kk) { k1 = kk; v = sv - acc + 1; } acc += 2 * kk; }
    }
    const size_t bo = (((size_t)b * P.H + wp) * NJ) * P.nmesh + jm;
    double m0 = INFINITY;
#pragma unroll
    for (int k0 = 0; k0 < NJ; ++k0) m0 = fmin(m0, P.base_d[bo + (size_t)k0 * P.nmesh]);
    // a link farther than prune_tol above max(min, 1e-4) cannot be the minimum nor reach the surrogate at a shifted pose
    const double thr = fmax(m0, 0.0001) + P.rb->prune_tol;
    double out = INFINITY;
    if (P.base_d[bo + (size_t)(k1 - 1) * P.nmesh] < thr) {
        double a6[6];
        mesh_link_ends<NVT, POSED>(P, b, wp, kvoff(k1) + v, jm, a6);
        Best bq;
        const size_t ob = bo + (size_t)(k1 - 1) * P.nmesh;
        const int *near = P.near + ob * (NEAR_CAP + 1);
        const int nn_ = near[0];
        if (nn_ >= 0) {                                      // the pose moved by < margin/2: its closest triangle is on the list
            const DevMesh &m = P.meshes[jm];
            bq.d = INFINITY; bq.t = INFINITY; bq.tri = -1;
            for (int i = 0; i < nn_; ++i) { const int k = near[1 + i]; seg_tri_update(a6, a6 + 3, m.tri + 9 * (size_t)k, k, bq); }
        } else {
            mesh_query<MESH_THREADS, false>(P.meshes[jm], a6, a6 + 3, P.base_t[ob], s_stack + threadIdx.x, s_lbs + threadIdx.x, bq, nullptr);
        }
        out = with_surrogate(bq, a6);
    }
    P.shift_d[(((size_t)b * P.H + wp) * P.nmesh + jm) * NSV + sv] = out;   // +inf: not a candidate
}

template <int NJ>
__global__ __launch_bounds__(MESH_THREADS) void mesh_fd_kernel(LinMeshParams P)
{
    constexpr int NVT = nvt(NJ), NSV = NVT - NJ, NE = 2 * NJ + 1;
    const int e = blockIdx.x * MESH_THREADS + threadIdx.x;
    if (e >= P.B * P.H * P.nmesh) return;
    const int jm = e % P.nmesh, wp = (e / P.nmesh) % P.H, b = e / (P.nmesh * P.H);
    if (P.status_done && P.status_done[b] != 0) return;
    const size_t bo = (((size_t)b * P.H + wp) * NJ) * P.nmesh + jm;
    const double *sh = P.shift_d + (((size_t)b * P.H + wp) * P.nmesh + jm) * NSV;
    double dev[NE];
    dev[0] = INFINITY;
#pragma unroll
    for (int k0 = 0; k0 < NJ; ++k0) dev[0] = fmin(dev[0], P.base_d[bo + (size_t)k0 * P.nmesh]);
#pragma unroll
    for (int ev = 1; ev < NE; ++ev) {
        double d = INFINITY;
#pragma unroll
        for (int k1 = 1; k1 <= NJ; ++k1) {
            const double dis = sh[k1 * (k1 - 1) + min(ev, 2 * k1) - 1];   // variants of link k1 start at sum_{k<k1} 2k = k1 (k1-1)
            if (dis < d) d = dis;
        }
        dev[ev] = d;
    }
    const size_t o = ((size_t)b * P.nmesh + jm) * P.H + wp;
    P.dist[o] = dev[0];
#pragma unroll
    for (int m = 0; m < NJ; ++m) P.grad[o * NJ + m] = (dev[2 * m + 1] - dev[2 * m + 2]) / FD_EPS;   // num_jac.m:14
}

// ---- host: hierarchy ------------------------------------------------------------------------------------
struct Builder {
    const double *tri;             // nt x 9, caller order
    std::vector<int> order;        // permutation being built
    std::vector<double> cen;       // nt x 3 centroids
    std::vector<BvhNode> nodes;
    int depth = 0;

    // builds the subtree of triangles [first, first + count); returns its reference (inner node index, or leaf code < 0) and box
    int build(int first, int count, int level, double *lo, double *hi)
    {
        depth = std::max(depth, level);
        double clo[3] = {INFINITY, INFINITY, INFINITY}, chi[3] = {-INFINITY, -INFINITY, -INFINITY};
        for (int r = 0; r < 3; ++r) { lo[r] = INFINITY; hi[r] = -INFINITY; }
        for (int i = first; i < first + count; ++i) {
            const double *T = tri + 9 * (size_t)order[i];
            for (int v = 0; v < 3; ++v)
                for (int r = 0; r < 3; ++r) { lo[r] = std::min(lo[r], T[3 * v + r]); hi[r] = std::max(hi[r], T[3 * v + r]); }
            for (int r = 0; r < 3; ++r) { clo[r] = std::min(clo[r], cen[3 * (size_t)order[i] + r]); chi[r] = std::max(chi[r], cen[3 * (size_t)order[i] + r]); }
        }
        if (count <= LEAF_TRIS) return -(first * 8 + count) - 1;
        const int id = (int)nodes.size();
        nodes.emplace_back();
        int ax = 0;
        for (int r = 1; r < 3; ++r) if (chi[r] - clo[r] > chi[ax] - clo[ax]) ax = r;
        const int mid = first + count / 2;                    // median split: balanced, depth <= ceil(log2(nt)) + 1
        std::nth_element(order.begin() + first, order.begin() + mid, order.begin() + first + count,
                         [&](int a, int c) { const double ca = cen[3 * (size_t)a + ax], cc = cen[3 * (size_t)c + ax]; return ca < cc || (ca == cc && a < c); });
        BvhNode nd;
        memset(&nd, 0, sizeof nd);
        nd.child[0] = build(first, mid - first, level + 1, nd.lo[0], nd.hi[0]);
        nd.child[1] = build(mid, first + count - mid, level + 1, nd.lo[1], nd.hi[1]);
        nodes[id] = nd;
        return id;
    }
};

int upload_mesh(const std::vector<double> &tri9, cfs_mesh **out)
{
    const int nt = (int)(tri9.size() / 9);
    for (double v : tri9) if (!std::isfinite(v)) return cfs_fail(CFS_ERR_INVALID_ARG, "mesh has a non-finite coordinate");
    Builder bd;
    bd.tri = tri9.data();
    bd.order.resize(nt);
    std::iota(bd.order.begin(), bd.order.end(), 0);
    bd.cen.resize(3 * (size_t)nt);
    for (int i = 0; i < nt; ++i)
        for (int r = 0; r < 3; ++r) bd.cen[3 * (size_t)i + r] = (tri9[9 * (size_t)i + r] + tri9[9 * (size_t)i + 3 + r] + tri9[9 * (size_t)i + 6 + r]) / 3.0;
    bd.nodes.reserve(2 * (size_t)nt / LEAF_TRIS + 8);
    double rlo[3], rhi[3];
    if (nt > (1 << 27)) return cfs_fail(CFS_ERR_INVALID_ARG, "mesh too large (%d triangles)", nt);
    const int root = bd.build(0, nt, 1, rlo, rhi);
    if (root < 0) {                                          // a mesh that is one leaf: give it an inner root with an empty second child
        BvhNode nd;
        memset(&nd, 0, sizeof nd);
        for (int r = 0; r < 3; ++r) { nd.lo[0][r] = rlo[r]; nd.hi[0][r] = rhi[r]; nd.lo[1][r] = INFINITY; nd.hi[1][r] = -INFINITY; }
        nd.child[0] = root; nd.child[1] = -1;                // -1 = leaf code of zero triangles
        bd.nodes.push_back(nd);
    }
    if (bd.depth + 2 > MESH_STACK) return cfs_fail(CFS_ERR_INVALID_ARG, "mesh hierarchy too deep (%d levels)", bd.depth);
    std::vector<double> tri_o(9 * (size_t)nt);
    for (int i = 0; i < nt; ++i) memcpy(&tri_o[9 * (size_t)i], &tri9[9 * (size_t)bd.order[i]], 72);
    cfs_mesh *m = new (std::nothrow) cfs_mesh();
    if (!m) return cfs_fail(CFS_ERR_ALLOC, "out of host memory");
    m->device = cfs_current_device();
    m->nt = nt; m->nnodes = (int)bd.nodes.size(); m->depth = bd.depth;
    for (int r = 0; r < 3; ++r) { m->bbox[r] = rlo[r]; m->bbox[3 + r] = rhi[r]; }
    hipError_t e = hipSetDevice(m->device);
    if (e == hipSuccess) e = m->nodes.upload(bd.nodes.data(), bd.nodes.size());
    if (e == hipSuccess) e = m->tri.upload(tri_o.data(), tri_o.size());
    if (e == hipSuccess) e = m->orig.upload(bd.order.data(), (size_t)nt);
    // the cut a cooperative traversal starts from: open the hierarchy level by level while the inner nodes fit a wavefront
    std::vector<int> cut{0}, cut_tri;
    while (!cut.empty() && cut.size() <= 32) {
        std::vector<int> next;
        for (int id : cut)
            for (int c = 0; c < 2; ++c) {
                const int ch = bd.nodes[id].child[c];
                if (ch >= 0) next.push_back(ch);
                else { const int code = -(ch + 1); for (int k = 0; k < (code & 7); ++k) cut_tri.push_back((code >> 3) + k); }
            }
        cut.swap(next);
    }
    m->ncut = (int)cut.size(); m->ncut_tri = (int)cut_tri.size();
    cut.insert(cut.end(), cut_tri.begin(), cut_tri.end());
    if (e == hipSuccess) e = m->cut.upload(cut.data(), cut.size());
    if (e != hipSuccess) {
        const int rc = cfs_fail(cfs_device_count() > 0 ? CFS_ERR_HIP : CFS_ERR_NO_DEVICE, "mesh upload failed: %s", hipGetErrorString(e));
        cfs_mesh_destroy(m);
        return rc;
    }
    *out = m;
    return CFS_SUCCESS;
}

}  // namespace

template <int NJ, bool POSED>
static hipError_t launch_linearize_mesh_nj(const LinMeshParams &p, hipStream_t s)
{
    constexpr int NVT = nvt(NJ), NE = 2 * NJ + 1;
    const dim3 block(MESH_THREADS);
    auto blocks = [](size_t n) { return dim3((unsigned)((n + MESH_THREADS - 1) / MESH_THREADS)); };
    const size_t bh = (size_t)p.B * p.H;
    hipLaunchKernelGGL(mesh_fk_kernel<NJ>, blocks(bh * NE), block, 0, s, p);
    hipLaunchKernelGGL((mesh_upper_kernel<NJ, POSED>), blocks(bh * NJ * p.nmesh), block, 0, s, p);
    hipLaunchKernelGGL((mesh_base_kernel<NJ, POSED>), dim3((unsigned)((bh * NJ * p.nmesh * MESH_PIECES + CO_QPW - 1) / CO_QPW)), dim3(64), 0, s, p);
    hipLaunchKernelGGL((mesh_reduce_kernel<NJ, POSED>), blocks(bh * NJ * p.nmesh), block, 0, s, p);
    hipLaunchKernelGGL((mesh_shift_kernel<NJ, POSED>), blocks(bh * p.nmesh * (NVT - NJ)), block, 0, s, p);
    hipLaunchKernelGGL(mesh_fd_kernel<NJ>, blocks(bh * p.nmesh), block, 0, s, p);
    return hipGetLastError();
}

hipError_t launch_linearize_mesh(int nj, const LinMeshParams &p, hipStream_t s)
{
    if (p.mesh_pose) return cfs_for_nj(nj, [&](auto N) { return launch_linearize_mesh_nj<decltype(N)::value, true>(p, s); });
    return cfs_for_nj(nj, [&](auto N) { return launch_linearize_mesh_nj<decltype(N)::value, false>(p, s); });
}

// doubles / ints of workspace per (problem, waypoint) the pipeline needs
void linearize_mesh_workspace(int nj, int nmesh, size_t *ends, size_t *base, size_t *shift, size_t *near, size_t *piece_d, size_t *piece_i,
                              size_t *piece_nd)
{
    *ends = (size_t)nvt(nj) * 6;
    *base = (size_t)nj * nmesh;
    *shift = (size_t)nmesh * (nvt(nj) - nj);
    *near = (size_t)nj * nmesh * (NEAR_CAP + 1);
    *piece_d = (size_t)nj * nmesh * MESH_PIECES * PIECE_D;
    *piece_i = (size_t)nj * nmesh * MESH_PIECES * PIECE_I;
    *piece_nd = (size_t)nj * nmesh * MESH_PIECES * NEAR_CAP;
}

extern "C" {

int cfs_mesh_create(const double *vertices, int nv, const int *triangles, int nt, cfs_mesh **out)
{
    if (!out) return cfs_fail(CFS_ERR_INVALID_ARG, "out is NULL");
    *out = nullptr;
    if (!vertices || !triangles || nv < 3 || nt < 1) return cfs_fail(CFS_ERR_INVALID_ARG, "a mesh needs vertices and at least one triangle");
    if (cfs_device_count() <= 0) return cfs_fail(CFS_ERR_NO_DEVICE, "no HIP device visible");
    std::vector<double> tri9(9 * (size_t)nt);
    for (int i = 0; i < nt; ++i)
        for (int v = 0; v < 3; ++v) {
            const int id = triangles[3 * (size_t)i + v];
            if (id < 0 || id >= nv) return cfs_fail(CFS_ERR_INVALID_ARG, "triangle %d refers to vertex %d of %d", i, id, nv);
            for (int r = 0; r < 3; ++r) tri9[9 * (size_t)i + 3 * v + r] = vertices[3 * (size_t)id + r];
        }
    return upload_mesh(tri9, out);
}

// binary STL (80-byte header, uint32 count, 50-byte records); map_from_stl applies Lib/functions/MapFromSTL.m:6-10
// (shift every axis to start at 0, y -= 100, then (x, y, z) <- (z, x, y)) before the uniform `scale`
int cfs_mesh_load_stl(const char *path, double scale, int map_from_stl, cfs_mesh **out)
{
    if (!out) return cfs_fail(CFS_ERR_INVALID_ARG, "out is NULL");
    *out = nullptr;
    if (!path) return cfs_fail(CFS_ERR_INVALID_ARG, "path is NULL");
    if (!(scale > 0)) return cfs_fail(CFS_ERR_INVALID_ARG, "scale must be positive");
    FILE *f = fopen(path, "rb");
    if (!f) return cfs_fail(CFS_ERR_INVALID_ARG, "cannot open %s", path);
    unsigned char head[84];
    if (fread(head, 1, 84, f) != 84) { fclose(f); return cfs_fail(CFS_ERR_INVALID_ARG, "%s: shorter than an STL header", path); }
    unsigned int nt;
    memcpy(&nt, head + 80, 4);
    fseek(f, 0, SEEK_END);
    const long sz = ftell(f);
    if (nt < 1 || sz != 84 + 50 * (long)nt) { fclose(f); return cfs_fail(CFS_ERR_INVALID_ARG, "%s: not a binary STL (%u triangles, %ld bytes)", path, nt, sz); }
    fseek(f, 84, SEEK_SET);
    std::vector<unsigned char> rec(50 * (size_t)nt);
    const size_t got = fread(rec.data(), 50, nt, f);
    fclose(f);
    if (got != nt) return cfs_fail(CFS_ERR_INVALID_ARG, "%s: truncated", path);
    std::vector<double> tri9(9 * (size_t)nt);
    for (size_t i = 0; i < nt; ++i) {
        float v[9];
        memcpy(v, rec.data() + 50 * i + 12, 36);
        for (int r = 0; r < 9; ++r) tri9[9 * i + r] = (double)v[r];
    }
    if (map_from_stl) {
        double mn[3] = {INFINITY, INFINITY, INFINITY};
        for (size_t i = 0; i < 3 * (size_t)nt; ++i)
            for (int r = 0; r < 3; ++r) mn[r] = std::min(mn[r], tri9[3 * i + r]);
        for (size_t i = 0; i < 3 * (size_t)nt; ++i) {
            const double x = tri9[3 * i] - mn[0], y = (tri9[3 * i + 1] - mn[1]) - 100.0, z = tri9[3 * i + 2] - mn[2];
            tri9[3 * i] = z; tri9[3 * i + 1] = x; tri9[3 * i + 2] = y;
        }
    }
    for (double &v : tri9) v *= scale;
    if (cfs_device_count() <= 0) return cfs_fail(CFS_ERR_NO_DEVICE, "no HIP device visible");
    return upload_mesh(tri9, out);
}

int cfs_mesh_info(const cfs_mesh *m, int *ntri, int *nnodes, int *depth, double *bbox6)
{
    if (!m) return cfs_fail(CFS_ERR_INVALID_ARG, "mesh is NULL");
    if (ntri) *ntri = m->nt;
    if (nnodes) *nnodes = m->nnodes;
    if (depth) *depth = m->depth;
    if (bbox6) memcpy(bbox6, m->bbox, sizeof m->bbox);
    return CFS_SUCCESS;
}

void cfs_mesh_destroy(cfs_mesh *m)
{
    if (!m) return;
    delete m;
}

// cfs_mesh_segment_distance in this unit's arithmetic (FMA contraction on, as in every kernel below and in the clearance, IK
// and Cartesian units): the hierarchy and the exact geometry of cfs_mesh_dev.h as the solvers run them, for arbitrary segments
int cfs_debug_mesh_segment_distance_contracted(const cfs_mesh *m, int n, const double *segs, double *dis, double *points, int *tri)
{
    return mesh_segment_query(m, n, segs, dis, points, tri, "cfs_debug_mesh_segment_distance_contracted");
}

// dist_arm_surf_200i for N poses (host arrays): d[N], linkid[N] (1-based, may be NULL), points[N x 6] (may be NULL)
int cfs_dist_arm_mesh(const cfs_robot *robot, int njoint, int N, const double *theta, const cfs_mesh *m,
                      double *d, int *linkid, double *points)
{
    if (!robot || !theta || !m || !d || N < 1) return cfs_fail(CFS_ERR_INVALID_ARG, "robot/theta/mesh/d must be given, N >= 1");
    int rc = cfs_check_robot(robot, njoint);
    if (rc) return rc;
    CFS_HIPCHK(hipSetDevice(m->device));
    DevRobot hr;
    cfs_build_dev_robot(*robot, hr);
    const size_t n = N;
    Stage st;
    ArmMeshParams q{st.up(&hr, 1), m->view(), N, njoint, st.up(theta, n * njoint), st.out<double>(n), st.out<int>(n), st.out<double>(n * 6)};
    if (st.err == hipSuccess) {
        const int per = MESH_THREADS / njoint;
        hipLaunchKernelGGL(cfs_dist_arm_mesh_kernel, dim3((N + per - 1) / per), dim3(MESH_THREADS), 0, nullptr, q);
        st.err = hipGetLastError();
    }
    st.down(d, q.d, n); st.down(linkid, q.linkid, n); st.down(points, q.pts, n * 6);
    return st.result("cfs_dist_arm_mesh");
}

}  // extern "C"
