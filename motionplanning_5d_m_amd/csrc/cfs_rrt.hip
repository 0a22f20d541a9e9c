// cfs_rrt.hip -- RRT / RRT* tree growth in joint space, one wavefront per tree, whole trees on the device (row f1).
//
// Reference behaviour restated (not translated): Lib/RRT_FANUC.m
//   find_route   :63-91    tree = [x0]; until goal_reached: getNode, addNode, [arrangeNode for RRT*]; back-track the route
//   getRandNode  :106-131  pp = rand; pp < bi: sample = (rand(nstate,1)-0.5).*region_s*2 + sample_off, else sample = goal_th;
//                          nearest node under the `ratial`-weighted 2-norm (first minimum wins, strict <, :124);
//                          newNode = near + (sample-near)*0.1/norm(near-sample)  (UNWEIGHTED norm)
//   feasible     :146-181  FK (theta(2) - pi/2 for M200i) + distLinSeg of every link against every obstacle axis, near-zero
//                          surrogate, reject if any distance < obs{j}.D; getNode :95-103 keeps sampling until feasible
//   addNode      :184-190  edge cost = total_dis(parent) + toNode_dis(parent): the parent -> SAMPLE distance (quirk kept)
//   arrangeNode  :134-142  RRT*: nodes within 0.2 of the SAMPLE are re-parented to the new node when that is cheaper; costs
//                          of their descendants are not propagated (quirk kept)
//   goal_reached :193-207  all(goal - region_g < newNode) & all(newNode < goal + region_g); fail when node_num > MAX_ITER
// and Lib/functions/s_Parallel_rrt.m:14-28 (independent seeds; here any number of trees per launch instead of parfor's 6).
//
// MI355X mapping.  A tree is a strictly sequential chain of proposals; trees are independent.  One 64-lane wavefront owns one
// tree for its whole life: the tree (nodes, parents, costs, the per-proposal distances) lives in LDS (<= 28 KB at
// MAX_ITER = 400: several trees per CU), the nearest-neighbour search is a wave argmin over the nodes (lane i takes nodes
// i, i + 64, ...), the feasibility test runs one (obstacle, link) pair per lane on the shared forward-kinematics result, RRT*'s
// re-parenting is one lane per node.  All control flow is wave-uniform (decisions come from ballots / wave reductions), there
// is no block barrier and no host round trip; >= 1024 trees per launch fill the chip.
// Random numbers: MATLAB's rand stream cannot be reproduced, so the caller either passes the uniforms (S x ndraw, consumed
// exactly as the reference consumes rand: one per proposal + nstate more when the sample is random) or a seed for the
// counter-based generator below (splitmix64 of (seed, tree, counter): reproducible on any host in integer arithmetic).
//
// This translation unit is compiled with -ffp-contract=off (Makefile): tree arithmetic (weighted norms, the 0.1-rad extension,
// cost sums) is then plain IEEE mul / add / div / sqrt in the order written here, so that parents, nodes, costs and routes are
// BIT-identical to the CPU restatement (oracle/rrt_oracle.py); only sin / cos differ from libm by <= 1 ulp (all_ee: 1e-14).
//
// Mesh obstacles (cfs_rrt_grow_mesh*).  feasible() is extended the way M200i/dist_arm_surf_200i.m:21-24
// extends dist_arm: after the line obstacles, for every mesh j and link i, dis = mesh distance of the link axis (contract:
// cfs_mesh.hip's head comment), |dis| < 1e-4 -> dis = -|points(:,1) - p(:,2)|, reject if dis < D_j.  The surrogate is negative and
// D_j > 0, so mesh j rejects the node exactly when SOME triangle lies closer than thr_j = max(D_j, 1e-4) to SOME link axis: an
// existence question (cfs_mesh_hit_dev.h holds the two traversals; cfs_ik.hip asks it too).  The traversal prunes a hierarchy node whose rigorous lower bound is not below thr_j and may stop at the
// first triangle below it; the decision does not depend on the order.  The mesh test runs only when the lines have passed (the
// same decision, fewer traversals).  Two variants, bit-identical trees:
//   A (RRT_MESH_PER_LANE)  lane p < nmesh*NJ owns one (mesh, link) pair and runs mesh_query<64, false>(bound = thr_j); the vote
//                          is a ballot of b.tri >= 0.  Private stacks in LDS (MESH_STACK*64*8 B = 10 KB).
//   B (RRT_MESH_WAVE)      one frontier of (pair, inner node) entries in LDS shared by the wave: each round the lanes take up to
//                          64 entries from its end, each lane bounds both children of its node, inner children that survive are
//                          appended by ballot + prefix count, the triangles of surviving leaves are tested exactly, and a
//                          ballot ends the test on the first hit.  A proposal whose frontier would overflow its capacity is
//                          decided by variant A (same decision by construction).
// Exact distances and lower bounds are cfs_mesh_dev.h's functions.  They are compiled here WITHOUT FMA contraction (the flag
// above covers the whole translation unit), so a distance may differ in its last bits from cfs_dist_arm_mesh, whose translation
// unit contracts: a proposal within rounding of its threshold may be decided differently from a cfs_dist_arm_mesh call.
// The line-only kernel (cfs_rrt_kernel) keeps its code path: the mesh code is compiled out of it.
#include "cfs_mesh_hit_dev.h"
#include "cfs_geom_dev.h"
#include "cfs_host.h"
#include <cmath>
#include <cstring>

namespace {

constexpr int WV = 64;

__device__ __forceinline__ double rrt_uniform(const RrtParams &P, int tree, unsigned long long counter)
{
    if (P.uniforms) return P.uniforms[(size_t)tree * P.ndraw + counter];
    unsigned long long z = P.seed + (unsigned long long)tree * 0x9E3779B97F4A7C15ull + (counter + 1ull) * 0xBF58476D1CE4E5B9ull;
    z ^= z >> 30; z *= 0xBF58476D1CE4E5B9ull;
    z ^= z >> 27; z *= 0x94D049BB133111EBull;
    z ^= z >> 31;
    return (double)(z >> 11) * 0x1.0p-53;
}

// proposals of variant B whose frontier overflowed and that variant A decided (cfs_debug_rrt_frontier_overflows): one vector atomic
// by lane 0 per such proposal, none on the normal path
__device__ unsigned long long g_rrt_frontier_overflows = 0ull;

// kernel arguments: the mesh table exists only in the mesh kernels' parameter block
template <int MESH> struct RrtArgs { RrtParams P; RrtMeshArgs MA; };
template <> struct RrtArgs<RRT_MESH_NONE> { RrtParams P; };

// MESH: RRT_MESH_NONE (the line-only kernel: the mesh code is compiled out) | RRT_MESH_PER_LANE | RRT_MESH_WAVE

template <int NJ, int MESH>
__global__ __launch_bounds__(WV) void cfs_rrt_kernel(const RrtArgs<MESH> A)
{
    const RrtParams &P = A.P;
    extern __shared__ __attribute__((aligned(16))) double lds[];
    const int t = blockIdx.x, lane = threadIdx.x;
    const int NMAX = P.max_iter + 1;                          // node_num may reach MAX_ITER + 1 before the failure test fires (:201)
    double *s_nodes = lds;                                    // [NMAX][NJ]
    double *s_tot = s_nodes + (size_t)NMAX * NJ;              // total_dis
    double *s_to = s_tot + NMAX;                              // toNode_dis of the current proposal
    int *s_par = reinterpret_cast<int *>(s_to + NMAX);        // parent (1-based, -1 for the root), all_nodes(1,:)
    int *s_stack = nullptr, *s_fpair = nullptr, *s_fnode = nullptr;   // mesh scratch behind the tree (rrt_mesh_lds_bytes)
    float *s_lbs = nullptr;
    if constexpr (MESH != RRT_MESH_NONE) {
        s_stack = s_par + ((NMAX + 1) & ~1);
        s_lbs = reinterpret_cast<float *>(s_stack + MESH_STACK * WV);
        if constexpr (MESH == RRT_MESH_WAVE) { s_fpair = s_stack + 2 * MESH_STACK * WV; s_fnode = s_fpair + RRT_FRONTIER_CAP; }
    }
    const DevRobot *rb = &P.rb;                               // robot constants travel in the kernel's parameter block (scalar loads)
    const double *x0 = P.x0 + (P.per_tree ? (size_t)t * NJ : 0), *goal = P.goal + (P.per_tree ? (size_t)t * NJ : 0);
    const double *goal_th = P.goal_th + (P.per_tree ? (size_t)t * NJ : 0);

    double newNode[NJ];
#pragma unroll
    for (int c = 0; c < NJ; ++c) newNode[c] = x0[c];
    if (lane < NJ) s_nodes[lane] = x0[lane];
    if (lane == 0) { s_tot[0] = 0.0; s_par[0] = -1; }
    int node_num = 1, parent = 1, fail = 0;
    unsigned long long cursor = 0, proposals = 0;
    const unsigned long long draw_cap = P.uniforms ? (unsigned long long)P.ndraw : (unsigned long long)P.max_draws;

    auto reached = [&]() {                                    // goal_reached (:193-199): both vector tests must hold for every joint
        bool in = true;
#pragma unroll
        for (int c = 0; c < NJ; ++c) in = in && ((goal[c] - P.region_g[c]) < newNode[c]) && (newNode[c] < (goal[c] + P.region_g[c]));
        return in;
    };
    bool done = reached();
    if (node_num > P.max_iter) { fail = 1; done = true; }
    __builtin_amdgcn_wave_barrier();

    while (!done) {
        // ---- getNode (:95-103): propose until feasible -------------------------------------------------------------------
        double e_first[3] = {0.0, 0.0, 0.0};
        for (;;) {
            if (cursor + 1ull + (unsigned long long)NJ > draw_cap) { fail = 2; break; }      // the random stream is exhausted: every wave gets here
            ++proposals;
            // getRandNode (:106-114)
            const double pp = rrt_uniform(P, t, cursor++);
            double sample[NJ];
            if (pp < P.bi) {
#pragma unroll
                for (int c = 0; c < NJ; ++c) sample[c] = (rrt_uniform(P, t, cursor + c) - 0.5) * P.region_s[c] * 2.0 + P.sample_off[c];
                cursor += NJ;
            } else {
#pragma unroll
                for (int c = 0; c < NJ; ++c) sample[c] = goal_th[c];
            }
            // nearest node under the weighted norm (:116-127): lane i scans nodes i, i + 64, ... in increasing order
            double best = INFINITY;
            int bidx = 0x7fffffff;
            for (int i = lane; i < node_num; i += WV) {
                double s2 = 0.0;
#pragma unroll
                for (int c = 0; c < NJ; ++c) { const double w = (s_nodes[i * NJ + c] - sample[c]) * P.ratial[c]; s2 += w * w; }
                const double dis = sqrt(s2);
                s_to[i] = dis;
                if (dis < best) { best = dis; bidx = i; }
            }
            // wave argmin, first minimum wins (:124 replaces only on a strictly smaller distance): smaller distance, then smaller index
#pragma unroll
            for (int m = 1; m < WV; m <<= 1) {
                const double ob = __shfl_xor(best, m, WV);
                const int oi = __shfl_xor(bidx, m, WV);
                if (ob < best || (ob == best && oi < bidx)) { best = ob; bidx = oi; }
            }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");      // s_to is read across lanes below
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            // the reference starts from node 1 and `dis_ < dis` is false for NaN: a NaN first distance keeps node 1, NaN elsewhere
            // never wins (NaN arises only after a zero-length extension, sample == nearest node)
            if (bidx == 0x7fffffff || s_to[0] != s_to[0]) bidx = 0;
            parent = bidx + 1;
            double near[NJ], n2 = 0.0;
#pragma unroll
            for (int c = 0; c < NJ; ++c) { near[c] = s_nodes[bidx * NJ + c]; const double w = near[c] - sample[c]; n2 += w * w; }
            const double nrm = sqrt(n2);
#pragma unroll
            for (int c = 0; c < NJ; ++c) newNode[c] = near[c] + (sample[c] - near[c]) * 0.1 / nrm;      // :129, left to right
            // feasible (:146-181): FK once per lane (uniform work), one (obstacle, link) pair per lane
            double ends[NJ * 6], M[12], Mn[12];
#pragma unroll
            for (int k = 0; k < NJ; ++k) {
                double sn, cs;
                sincos(newNode[k] - rb->th_off[k], &sn, &cs);
                fk_step(rb, k, sn, cs, k == 0 ? nullptr : M, Mn);
#pragma unroll
                for (int q = 0; q < 12; ++q) M[q] = Mn[q];
                link_ends(rb, k, M, ends + k * 6);
            }
            bool hit = false;
            for (int p = lane; p < P.nobs * NJ; p += WV) {
                const int j = p / NJ, k = p - j * NJ;
                double o6[6], a6[6];
#pragma unroll
                for (int q = 0; q < 6; ++q) o6[q] = P.obs[j * 6 + q];
#pragma unroll
                for (int kk = 0; kk < NJ; ++kk)
                    if (kk == k) {
#pragma unroll
                        for (int q = 0; q < 6; ++q) a6[q] = ends[kk * 6 + q];
                    }
                const double dis = seg_seg_dist(a6, o6);
                hit = hit || (dis < P.D[j]);
            }
            bool infeasible = __ballot(hit) != 0ull;
            if constexpr (MESH != RRT_MESH_NONE) {
                if (!infeasible) infeasible = mesh_hit<NJ, MESH>(A.MA, ends, lane, s_stack, s_lbs, s_fpair, s_fnode, &g_rrt_frontier_overflows);
            }
            e_first[0] = ends[(NJ - 1) * 6]; e_first[1] = ends[(NJ - 1) * 6 + 1]; e_first[2] = ends[(NJ - 1) * 6 + 2];   // pos{nstate}.p(:,1) (:186)
            if (!infeasible) break;
        }
        if (fail) break;
        // ---- addNode (:184-190) ------------------------------------------------------------------------------------------
        const int nn_ = node_num;                             // 0-based index of the new node
        if (nn_ >= NMAX) { fail = 1; break; }                // cannot happen: the failure test below fires first
        const double tot_new = s_tot[parent - 1] + s_to[parent - 1];
        __builtin_amdgcn_wave_barrier();
        if (lane < NJ) s_nodes[nn_ * NJ + lane] = newNode[lane];
        if (lane == 0) {
            s_par[nn_] = parent; s_tot[nn_] = tot_new;
            if (P.all_ee) { double *ee = P.all_ee + ((size_t)t * P.max_iter + (nn_ - 1)) * 3; ee[0] = e_first[0]; ee[1] = e_first[1]; ee[2] = e_first[2]; }
        }
        node_num = nn_ + 1;
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        // ---- arrangeNode (:134-142), RRT* only: toNode_dis has one entry per node that existed at the proposal ----------------
        if (P.solver == 1) {
            for (int i = lane; i < nn_; i += WV) {
                const double td = s_to[i];
                if (td < P.rewire) {
                    const double via = tot_new + td;
                    if (s_tot[i] > via) { s_par[i] = node_num; s_tot[i] = via; }
                }
            }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        }
        // ---- goal_reached (:193-207) -------------------------------------------------------------------------------------
        done = reached();
        if (node_num > P.max_iter) { fail = 1; done = true; }
    }

    // ---- results: the tree, then the route by back-tracking (:85-90) --------------------------------------------------------
    __builtin_amdgcn_wave_barrier();
    for (int e = lane; e < node_num * NJ; e += WV) P.nodes[(size_t)t * NMAX * NJ + e] = s_nodes[e];
    for (int i = lane; i < node_num; i += WV) { P.parent[(size_t)t * NMAX + i] = s_par[i]; P.total_dis[(size_t)t * NMAX + i] = s_tot[i]; }
    // route = [ancestors ..., newNode]; `parent` is the parent chosen by the LAST proposal (for a tree of one node: none)
    int len = 1, p = node_num > 1 ? parent : -1;
    while (p != -1 && len <= node_num) { ++len; p = s_par[p - 1]; }          // length first (uniform); a re-parenting cycle ends at node_num + 1
    if (p != -1) { fail = fail ? fail : 3; len = 1; }                        // RRT* may close a cycle (the reference would never return): report
    if (lane == 0) {
        double *rt = P.route + (size_t)t * NMAX * NJ;
        int pos = len - 1;
#pragma unroll
        for (int c = 0; c < NJ; ++c) rt[pos * NJ + c] = newNode[c];
        p = (node_num > 1 && len > 1) ? parent : -1;
        while (p != -1 && pos > 0) {
            --pos;
            for (int c = 0; c < NJ; ++c) rt[pos * NJ + c] = s_nodes[(p - 1) * NJ + c];
            p = s_par[p - 1];
        }
        P.node_num[t] = node_num; P.fail[t] = fail; P.route_len[t] = len;
        if (P.draws_used) P.draws_used[t] = (long long)cursor;
        if (P.proposals) P.proposals[t] = (long long)proposals;
    }
}

}  // namespace

size_t rrt_lds_bytes(int nj, int max_iter)
{
    const size_t NMAX = (size_t)max_iter + 1;
    return NMAX * nj * 8 + NMAX * 8 * 2 + ((NMAX * 4 + 7) & ~(size_t)7);
}

size_t rrt_mesh_lds_bytes(int nj, int max_iter, int variant)
{
    size_t b = rrt_lds_bytes(nj, max_iter);
    if (variant != RRT_MESH_NONE) b += (size_t)MESH_STACK * WV * 8;                  // variant A's stacks (B falls back to A)
    if (variant == RRT_MESH_WAVE) b += (size_t)RRT_FRONTIER_CAP * 8;                 // variant B's frontier
    return b;
}

namespace {
template <int NJ, int MESH> hipError_t launch_rrt_kernel(size_t lds, const RrtArgs<MESH> &a, hipStream_t s)
{
    if (lds > 64 * 1024) return hipErrorInvalidValue;
    hipLaunchKernelGGL((cfs_rrt_kernel<NJ, MESH>), dim3(a.P.S), dim3(WV), lds, s, a);
    return hipGetLastError();
}
}  // namespace

hipError_t launch_rrt_mesh(int nj, int variant, const RrtParams &p, const RrtMeshArgs &ma, hipStream_t s)
{
    if (variant != RRT_MESH_PER_LANE && variant != RRT_MESH_WAVE) return hipErrorInvalidValue;
    const size_t lds = rrt_mesh_lds_bytes(nj, p.max_iter, variant);
    return cfs_for_nj(nj, [&](auto N) {
        constexpr int NJ = decltype(N)::value;
        return variant == RRT_MESH_PER_LANE ? launch_rrt_kernel<NJ, RRT_MESH_PER_LANE>(lds, {p, ma}, s) : launch_rrt_kernel<NJ, RRT_MESH_WAVE>(lds, {p, ma}, s);
    });
}

hipError_t launch_rrt(int nj, const RrtParams &p, hipStream_t s)
{
    return cfs_for_nj(nj, [&](auto N) { return launch_rrt_kernel<decltype(N)::value, RRT_MESH_NONE>(rrt_lds_bytes(nj, p.max_iter), {p}, s); });
}

static_assert(CFS_RRT_MESH_PER_LANE == CFS_IK_MESH_PER_LANE && CFS_RRT_MESH_WAVE == CFS_IK_MESH_WAVE && CFS_RRT_MESH_SMALL_FRONTIER == CFS_IK_MESH_SMALL_FRONTIER,
              "cfs_check_mesh_table reads the flags of both families");
int cfs_check_mesh_table(int nobs, int nmesh, const cfs_mesh *const *meshes, const double *D_mesh, int flags, int min_nmesh, int default_variant,
                         RrtMeshArgs &ma, int &variant)
{
    variant = RRT_MESH_NONE;
    memset(&ma, 0, sizeof ma);
    if (nmesh < min_nmesh || nobs + nmesh > CFS_MAX_OBS)
        return cfs_fail(CFS_ERR_INVALID_ARG, "nobs %d + nmesh %d outside %d..%d", nobs, nmesh, min_nmesh, CFS_MAX_OBS);
    if (flags & ~(CFS_RRT_MESH_PER_LANE | CFS_RRT_MESH_WAVE | CFS_RRT_MESH_SMALL_FRONTIER)) return cfs_fail(CFS_ERR_INVALID_ARG, "unknown flags 0x%x", flags);
    if ((flags & CFS_RRT_MESH_PER_LANE) && (flags & (CFS_RRT_MESH_WAVE | CFS_RRT_MESH_SMALL_FRONTIER)))
        return cfs_fail(CFS_ERR_INVALID_ARG, "CFS_RRT_MESH_PER_LANE excludes the other flags");
    if (nmesh == 0) return CFS_SUCCESS;
    if (!meshes || !D_mesh) return cfs_fail(CFS_ERR_INVALID_ARG, "meshes / D_mesh must be given");
    for (int j = 0; j < nmesh; ++j) {
        if (!meshes[j]) return cfs_fail(CFS_ERR_INVALID_ARG, "mesh %d is NULL", j);
        if (!std::isfinite(D_mesh[j]) || !(D_mesh[j] > 0.0)) return cfs_fail(CFS_ERR_INVALID_ARG, "D_mesh[%d] must be finite and > 0", j);
    }
    for (int j = 0; j < nmesh; ++j) {
        if (meshes[j]->device != cfs_current_device())
            return cfs_fail(CFS_ERR_INVALID_ARG, "mesh %d lives on device %d, the current device is %d", j, meshes[j]->device, cfs_current_device());
        ma.m[j].nodes = meshes[j]->nodes.p; ma.m[j].tri = meshes[j]->tri.p; ma.m[j].nt = meshes[j]->nt;
        ma.m[j].thr = D_mesh[j] > 0.0001 ? D_mesh[j] : 0.0001;                         // dist_arm_surf_200i.m:22-24 folded into the threshold
    }
    ma.nmesh = nmesh;
    variant = (flags & CFS_RRT_MESH_PER_LANE) ? RRT_MESH_PER_LANE : (flags & (CFS_RRT_MESH_WAVE | CFS_RRT_MESH_SMALL_FRONTIER)) ? RRT_MESH_WAVE : default_variant;
    ma.cap = (flags & CFS_RRT_MESH_SMALL_FRONTIER) ? RRT_FRONTIER_SMALL : RRT_FRONTIER_CAP;
    return CFS_SUCCESS;
}

// ---- C ABI (include/cfs_hip.h, "RRT / RRT*") -----------------------------------------------------------------------------------
namespace {
int check_rrt(const cfs_rrt_desc *d, int S)
{
    if (!d) return cfs_fail(CFS_ERR_INVALID_ARG, "NULL descriptor");
    int rc = cfs_check_robot(&d->robot, d->nstate);
    if (rc) return rc;
    if (d->nstate < 2) return cfs_fail(CFS_ERR_INVALID_ARG, "nstate %d unsupported (2..6)", d->nstate);
    if (S < 1) return cfs_fail(CFS_ERR_INVALID_ARG, "at least one tree is needed");
    if (d->solver != CFS_RRT && d->solver != CFS_RRT_STAR) return cfs_fail(CFS_ERR_INVALID_ARG, "unknown solver %d", d->solver);
    if (d->max_iter < 1 || rrt_lds_bytes(d->nstate, d->max_iter) > 64 * 1024) return cfs_fail(CFS_ERR_INVALID_ARG, "MAX_ITER %d outside 1..%d", d->max_iter, 1000);
    if (d->nobs < 0 || d->nobs > CFS_MAX_OBS) return cfs_fail(CFS_ERR_INVALID_ARG, "nobs %d outside 0..%d", d->nobs, CFS_MAX_OBS);
    if (!d->x0 || !d->goal || !d->goal_th || !d->region_g || !d->region_s || !d->sample_off || !d->ratial) return cfs_fail(CFS_ERR_INVALID_ARG, "NULL array in the descriptor");
    if (d->nobs > 0 && (!d->obs || !d->D)) return cfs_fail(CFS_ERR_INVALID_ARG, "obs / D must be given");
    if (!d->uniforms && d->max_draws < 1) return cfs_fail(CFS_ERR_INVALID_ARG, "max_draws must be >= 1 in generator mode");
    if (d->uniforms && d->ndraw < 1) return cfs_fail(CFS_ERR_INVALID_ARG, "ndraw must be >= 1");
    return CFS_SUCCESS;
}

// cfs_check_mesh_table, then what only the tree kernels need: the tree and the variant's mesh scratch share the 64 KB of LDS
int check_rrt_mesh(const cfs_rrt_desc *d, int nmesh, const cfs_mesh *const *meshes, const double *D_mesh, int flags, RrtMeshArgs &ma, int &variant)
{
    int rc = cfs_check_mesh_table(d->nobs, nmesh, meshes, D_mesh, flags, 0, RRT_MESH_DEFAULT, ma, variant);
    if (rc) return rc;
    if (rrt_mesh_lds_bytes(d->nstate, d->max_iter, variant) > 64 * 1024)
        return cfs_fail(CFS_ERR_INVALID_ARG, "MAX_ITER %d does not fit next to the mesh scratch (%zu B of LDS, limit 65536)", d->max_iter,
                        rrt_mesh_lds_bytes(d->nstate, d->max_iter, variant));
    return CFS_SUCCESS;
}

bool out_complete(const cfs_rrt_out *out)
{
    return out && out->node_num && out->fail && out->parent && out->nodes && out->total_dis && out->route_len && out->route;
}

int grow_device(const cfs_rrt_desc *d, int nmesh, const cfs_mesh *const *meshes, const double *D_mesh, int flags, int S, const cfs_rrt_out *out, void *stream)
{
    int rc = check_rrt(d, S);
    if (rc) return rc;
    RrtMeshArgs ma;
    int variant;
    rc = check_rrt_mesh(d, nmesh, meshes, D_mesh, flags, ma, variant);
    if (rc) return rc;
    if (!out_complete(out)) return cfs_fail(CFS_ERR_INVALID_ARG, "NULL output array");
    rc = cfs_use_device(cfs_current_device());
    if (rc) return rc;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    RrtParams P;
    memset(&P, 0, sizeof P);
    cfs_build_dev_robot(d->robot, P.rb);
    P.S = S; P.nobs = d->nobs; P.solver = d->solver; P.max_iter = d->max_iter; P.per_tree = d->per_tree;
    P.bi = d->bi; P.rewire = d->rewire;
    P.x0 = d->x0; P.goal = d->goal; P.goal_th = d->goal_th; P.region_g = d->region_g; P.region_s = d->region_s; P.sample_off = d->sample_off; P.ratial = d->ratial;
    P.obs = d->obs; P.D = d->D; P.uniforms = d->uniforms; P.ndraw = d->ndraw; P.seed = d->seed; P.max_draws = d->max_draws;
    P.node_num = out->node_num; P.fail = out->fail; P.parent = out->parent; P.route_len = out->route_len;
    P.nodes = out->nodes; P.total_dis = out->total_dis; P.all_ee = out->all_ee; P.route = out->route;
    P.draws_used = out->draws_used; P.proposals = out->proposals;
    hipError_t e = variant == RRT_MESH_NONE ? launch_rrt(d->nstate, P, s) : launch_rrt_mesh(d->nstate, variant, P, ma, s);
    if (e != hipSuccess) return cfs_fail(CFS_ERR_HIP, "RRT launch failed: %s", hipGetErrorString(e));
    return CFS_SUCCESS;
}

int grow_host(const cfs_rrt_desc *d, int nmesh, const cfs_mesh *const *meshes, const double *D_mesh, int flags, int S, const cfs_rrt_out *out)
{
    int rc = check_rrt(d, S);
    if (rc) return rc;
    {   // refuse before anything is staged on the device; grow_device checks again and keeps the table (host work only, no launch)
        RrtMeshArgs ma;
        int variant;
        rc = check_rrt_mesh(d, nmesh, meshes, D_mesh, flags, ma, variant);
        if (rc) return rc;
    }
    if (!out_complete(out)) return cfs_fail(CFS_ERR_INVALID_ARG, "NULL output array");
    rc = cfs_use_device(cfs_current_device());
    if (rc) return rc;
    const size_t nj = d->nstate, N = (size_t)d->max_iter + 1, per = d->per_tree ? (size_t)S : 1, nS = S, nee = nS * d->max_iter * 3;
    Stage st;
    cfs_rrt_desc dd = *d;
    dd.x0 = st.up(d->x0, per * nj); dd.goal = st.up(d->goal, per * nj); dd.goal_th = st.up(d->goal_th, per * nj);
    dd.region_g = st.up(d->region_g, nj); dd.region_s = st.up(d->region_s, nj); dd.sample_off = st.up(d->sample_off, nj); dd.ratial = st.up(d->ratial, nj);
    dd.obs = st.up(d->obs, (size_t)d->nobs * 6); dd.D = st.up(d->D, (size_t)d->nobs);
    if (d->uniforms) dd.uniforms = st.up(d->uniforms, nS * d->ndraw);
    cfs_rrt_out o;
    memset(&o, 0, sizeof o);
    o.node_num = st.out<int>(nS); o.fail = st.out<int>(nS); o.route_len = st.out<int>(nS);
    o.parent = st.zeros<int>(nS * N); o.nodes = st.zeros<double>(nS * N * nj); o.total_dis = st.zeros<double>(nS * N);
    o.route = st.zeros<double>(nS * N * nj);
    if (out->all_ee) o.all_ee = st.zeros<double>(nee);
    if (out->draws_used) o.draws_used = st.out<long long>(nS);
    if (out->proposals) o.proposals = st.out<long long>(nS);
    if (st.err != hipSuccess) return st.result("RRT staging");
    rc = grow_device(&dd, nmesh, meshes, D_mesh, flags, S, &o, nullptr);
    if (rc) return rc;
    CFS_HIPCHK(hipStreamSynchronize(nullptr));
    st.down(out->node_num, o.node_num, nS); st.down(out->fail, o.fail, nS); st.down(out->route_len, o.route_len, nS);
    st.down(out->parent, o.parent, nS * N); st.down(out->nodes, o.nodes, nS * N * nj); st.down(out->total_dis, o.total_dis, nS * N);
    st.down(out->route, o.route, nS * N * nj);
    st.down(out->all_ee, o.all_ee, nee); st.down(out->draws_used, o.draws_used, nS); st.down(out->proposals, o.proposals, nS);
    return st.result("RRT staging");
}
}  // namespace

extern "C" int cfs_rrt_grow_device(const cfs_rrt_desc *d, int S, const cfs_rrt_out *out, void *stream)
{
    return grow_device(d, 0, nullptr, nullptr, 0, S, out, stream);
}

extern "C" int cfs_rrt_grow(const cfs_rrt_desc *d, int S, const cfs_rrt_out *out)
{
    return grow_host(d, 0, nullptr, nullptr, 0, S, out);
}

extern "C" int cfs_rrt_grow_mesh_device(const cfs_rrt_desc *d, int nmesh, const cfs_mesh *const *meshes, const double *D_mesh, int flags, int S,
                                        const cfs_rrt_out *out, void *stream)
{
    return grow_device(d, nmesh, meshes, D_mesh, flags, S, out, stream);
}

extern "C" int cfs_rrt_grow_mesh(const cfs_rrt_desc *d, int nmesh, const cfs_mesh *const *meshes, const double *D_mesh, int flags, int S,
                                 const cfs_rrt_out *out)
{
    return grow_host(d, nmesh, meshes, D_mesh, flags, S, out);
}

extern "C" int cfs_debug_rrt_frontier_overflows(unsigned long long *count, int reset)
{
    return cfs_frontier_overflows(&g_rrt_frontier_overflows, count, reset);
}
