// cfs_mesh_hit_dev.h -- the threshold test of link axes against mesh hierarchies, shared by the translation units that ask the
// existence question of DESIGN.md section 19 with a whole wavefront (cfs_rrt.hip: a proposal; cfs_ik.hip: a converged restart;
// cfs_cart.hip: a row of a traced line): does SOME triangle of SOME mesh j lie strictly closer than thr_j to SOME link axis?
// mesh_hit is what the units call; mesh_pair_clearance and mesh_wave_min measure a winner's clearance.  Two variants with the same decision:
//   A (mesh_hit_per_lane)  lane p < nmesh*NJ owns one (mesh, link) pair and runs mesh_query<64, false>(bound = thr_j); the vote
//                          is a ballot of b.tri >= 0.  Private stacks in LDS (MESH_STACK*64*8 B = 10 KB).
//   B (mesh_hit_wave)      one frontier of (pair, inner node) entries in LDS shared by the wave: each round the lanes take up to
//                          64 entries from its end, each lane bounds both children of its node, inner children that survive are
//                          appended by ballot + prefix count, the triangles of surviving leaves are tested exactly, and a
//                          ballot ends the test on the first hit.  A pose whose frontier would overflow its capacity is to be
//                          decided by variant A (same decision by construction).
// Both are called by all 64 lanes of a wave with the SAME pose in `ends` (wave-uniform control flow).  The arithmetic is
// cfs_mesh_dev.h's; whether it contracts into FMAs is the including translation unit's flag (cfs_rrt.o: off; cfs_ik.o: on), so a
// pose within rounding of a threshold may be decided differently by two translation units.
#pragma once
#include "cfs_mesh_dev.h"

namespace {

constexpr int MESH_HIT_WV = 64;

// link k's axis out of the FK result, without dynamic indexing of the register array
template <int NJ>
__device__ __forceinline__ void pick_link(const double *ends, int k, double *a6)
{
#pragma unroll
    for (int kk = 0; kk < NJ; ++kk)
        if (kk == k) {
#pragma unroll
            for (int q = 0; q < 6; ++q) a6[q] = ends[kk * 6 + q];
        }
}

// variant A: one (mesh, link) pair per lane, threshold query with a private stack
template <int NJ>
__device__ __forceinline__ bool mesh_hit_per_lane(const RrtMeshArgs &MA, const double *ends, int lane, int *stack, float *lbs)
{
    constexpr int WV = MESH_HIT_WV;
    bool hit = false;
    const int npair = MA.nmesh * NJ;
    for (int p = lane; p < npair; p += WV) {
        const int j = p / NJ, k = p - j * NJ;
        double a6[6];
        pick_link<NJ>(ends, k, a6);
        const DevMesh m{MA.m[j].nodes, MA.m[j].tri, nullptr, 0, MA.m[j].nt, nullptr, nullptr, 0, 0};
        Best b;
        mesh_query<WV, false>(m, a6, a6 + 3, -1, stack + lane, lbs + lane, b, nullptr, MA.m[j].thr);
        hit = hit || (b.tri >= 0 && b.d < MA.m[j].thr);       // take() also accepts a tie with the bound: the rule is strict (dis < D)
    }
    return __ballot(hit) != 0ull;
}

// variant B: wave-cooperative threshold traversal.  1: some triangle is below its threshold; 0: none; -1: the frontier overflowed
template <int NJ>
__device__ __forceinline__ int mesh_hit_wave(const RrtMeshArgs &MA, const double *ends, int lane, int *f_pair, int *f_node)
{
    constexpr int WV = MESH_HIT_WV;
    const int npair = MA.nmesh * NJ, cap = MA.cap;
    if (npair > cap) return -1;
    for (int p = lane; p < npair; p += WV) { f_pair[p] = p; f_node[p] = 0; }      // the root is always an inner node (upload_mesh)
    int count = npair;
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    while (count > 0) {
        const int n = count < WV ? count : WV;                // from the end: depth first in blocks of 64, the frontier stays short
        count -= n;
        const bool live = lane < n;
        int p = 0, node = 0;
        if (live) { p = f_pair[count + lane]; node = f_node[count + lane]; }
        __builtin_amdgcn_wave_barrier();
        bool hit = false, push0 = false, push1 = false;
        int c0 = 0, c1 = 0;
        if (live) {
            const int j = p / NJ, k = p - j * NJ;
            double a6[6];
            pick_link<NJ>(ends, k, a6);
            const double thr = MA.m[j].thr;
            const double *tri = MA.m[j].tri;
            if (MA.m[j].nt > 0) {
                const BvhNode nd = MA.m[j].nodes[node];       // one load: both children's boxes
                const double l0 = node_lower_bound(a6, a6 + 3, nd.lo[0], nd.hi[0]);
                const double l1 = node_lower_bound(a6, a6 + 3, nd.lo[1], nd.hi[1]);
                c0 = nd.child[0]; c1 = nd.child[1];
                const bool s0 = l0 < thr, s1 = l1 < thr;      // an empty child's bound is +inf or NaN: never below
                push0 = s0 && c0 >= 0; push1 = s1 && c1 >= 0;
                const int leaf0 = (s0 && c0 < 0) ? c0 : 0, leaf1 = (s1 && c1 < 0) ? c1 : 0;
#pragma unroll 1
                for (int it = 0; it < 2; ++it) {
                    const int lf = it == 0 ? leaf0 : leaf1;
                    if (lf < 0) {
                        const int code = -(lf + 1), first = code >> 3, cnt = code & 7;
                        Best b;
                        b.d = thr; b.t = INFINITY; b.tri = -1;
                        for (int q = first; q < first + cnt; ++q) seg_tri_update(a6, a6 + 3, tri + 9 * (size_t)q, q, b);
                        hit = hit || (b.tri >= 0 && b.d < thr);       // strict, as in variant A
                    }
                }
            }
        }
        if (__ballot(hit) != 0ull) return 1;
        const unsigned long long below = (1ull << lane) - 1ull;
        const unsigned long long m0 = __ballot(push0);
        if (push0) { const int pos = count + __popcll(m0 & below); if (pos < cap) { f_pair[pos] = p; f_node[pos] = c0; } }
        count += __popcll(m0);
        const unsigned long long m1 = __ballot(push1);
        if (push1) { const int pos = count + __popcll(m1 & below); if (pos < cap) { f_pair[pos] = p; f_node[pos] = c1; } }
        count += __popcll(m1);
        if (count > cap) return -1;
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    }
    return 0;
}

// The decision under the unit's variant MESH (RRT_MESH_PER_LANE | RRT_MESH_WAVE): variant B, and a pose whose frontier overflows is
// counted in *overflows (the unit's cfs_debug_*_frontier_overflows counter: one vector atomic by lane 0, none on the normal path)
// and decided by variant A.
template <int NJ, int MESH>
__device__ __forceinline__ bool mesh_hit(const RrtMeshArgs &MA, const double *ends, int lane, int *stack, float *lbs, int *f_pair, int *f_node,
                                         unsigned long long *overflows)
{
    if constexpr (MESH == RRT_MESH_PER_LANE) {
        return mesh_hit_per_lane<NJ>(MA, ends, lane, stack, lbs);
    } else {
        const int h = mesh_hit_wave<NJ>(MA, ends, lane, f_pair, f_node);
        if (h < 0 && lane == 0) atomicAdd(overflows, 1ull);
        return h < 0 ? mesh_hit_per_lane<NJ>(MA, ends, lane, stack, lbs) : h != 0;
    }
}

// The clearance of one (mesh, link) pair pr = j * NJ + k of the pose in `ends`: one exact, unbounded query, dm_j - D[j] (subtracting
// D_j is monotone, so a minimum over the links may be taken after it).  stack / lbs: the lane's own slots.
template <int NJ>
__device__ __forceinline__ double mesh_pair_clearance(const RrtMeshArgs &MA, const double *D, const double *ends, int pr, int *stack, float *lbs)
{
    const int j = pr / NJ, k = pr - j * NJ;
    double a6[6];
    pick_link<NJ>(ends, k, a6);
    const DevMesh m{MA.m[j].nodes, MA.m[j].tri, nullptr, 0, MA.m[j].nt, nullptr, nullptr, 0, 0};
    Best b;
    mesh_query<MESH_HIT_WV, false>(m, a6, a6 + 3, -1, stack, lbs, b, nullptr);
    return b.d - D[j];
}

// the wave's minimum in every lane
__device__ __forceinline__ double mesh_wave_min(double v)
{
#pragma unroll
    for (int m = 1; m < MESH_HIT_WV; m <<= 1) {
        const double o = __shfl_xor(v, m, MESH_HIT_WV);
        if (o < v) v = o;
    }
    return v;
}

}  // namespace
