// cfs_plan.hip -- per-slot choice of the best of K smoothed RRT routes (cfs_select_best_device).
//
// Reference behaviour restated (not translated): s_Parallel_rrt.m:27-28 keeps the route with the fewest nodes of its seeds
// and RRTstar_CFS.m:94-196 smooths that one route.  Here all K routes of a slot have been smoothed in one solve; this kernel
// picks one per slot by the rule of include/cfs_hip.h (cfs_select_best_device) and gathers its results.
//
// MI355X mapping: one wavefront per slot, four slots per 256-thread workgroup.  Lane k < K ranks candidate s*K + k by the key
// (class, primary, secondary, k); a butterfly of __shfl_xor leaves the lexicographic minimum on every lane.  The key is a total
// order (k is unique within a slot), so every lane ends with the same winner whatever the order of the exchanges: the result
// depends on the slot's own K candidates alone, not on S, the launch or the other slots.  The wavefront then copies the
// winner's rows with lane-strided loads and stores.  No atomics, no LDS.
#include "cfs_problem.h"

namespace {

constexpr int PLAN_WAVES = 4;   // slots per workgroup

struct SelectParams {
    int S, K, nn, nx, mk;                  // slots, candidates per slot, row lengths of u / x_ / the per-iteration logs
    const int *route_ok;                   // S*K
    cfs_batch_out cand, best;              // S*K rows in, S rows out
    const double *cand_viol;               // S*K x mk, or null (then the violation of every candidate counts as 0)
    double *best_viol;                     // S x mk, or null (nothing gathered)
    int *selected, *has_solution;          // S
};

// class of a candidate: 0 status 0/1 (A), 1 status 4 (B), 2 route found otherwise, 3 not eligible (no route / lane >= K)
struct Key {
    int cls;
    double p1, p2;
    int k;
};

__device__ __forceinline__ bool key_less(const Key &a, const Key &b)
{
    if (a.cls != b.cls) return a.cls < b.cls;
    if (a.p1 != b.p1) return a.p1 < b.p1;
    if (a.p2 != b.p2) return a.p2 < b.p2;
    return a.k < b.k;
}

__device__ __forceinline__ Key candidate_key(const SelectParams &P, int s, int k)
{
    Key key{3, 0.0, 0.0, k};
    if (k >= P.K) return key;
    const size_t c = (size_t)s * P.K + k;
    if (P.route_ok[c] == 0) return key;
    key.cls = 2;
    const int st = P.cand.status[c];
    const int n = P.cand.iter_O[c] - 1;                          // outer iterations run (reference convention)
    if ((st != CFS_OK_CONVERGED && st != CFS_OK_MAXITER && st != CFS_SOFT_ENDED) || n < 1 || n > P.mk) return key;
    const double cost = P.cand.cost_all[c * P.mk + (n - 1)];     // eval.cost_new
    if (st == CFS_SOFT_ENDED) {
        const double viol = P.cand_viol ? P.cand_viol[c * P.mk + (n - 1)] : 0.0;
        if (isnan(cost) || isnan(viol)) return key;
        key.cls = 1; key.p1 = viol; key.p2 = cost;
    } else {
        if (isnan(cost)) return key;
        key.cls = 0; key.p1 = cost;
    }
    return key;
}

__device__ __forceinline__ void copy_row(const double *src, double *dst, int n, int lane)
{
    for (int e = lane; e < n; e += CFS_WAVE) dst[e] = src[e];
}

__global__ __launch_bounds__(CFS_WAVE * PLAN_WAVES) void cfs_select_best_kernel(SelectParams P)
{
    const int lane = threadIdx.x % CFS_WAVE;
    const int s = blockIdx.x * PLAN_WAVES + threadIdx.x / CFS_WAVE;
    if (s >= P.S) return;                                        // a whole wavefront leaves: no shuffle is left half-joined
    Key m = candidate_key(P, s, lane);
    for (int off = CFS_WAVE / 2; off > 0; off >>= 1) {
        Key o;
        o.cls = __shfl_xor(m.cls, off);
        o.p1 = __shfl_xor(m.p1, off);
        o.p2 = __shfl_xor(m.p2, off);
        o.k = __shfl_xor(m.k, off);
        if (key_less(o, m)) m = o;
    }
    if (m.cls == 3) {                                            // no seed of the slot found a route: its rows stay as they are
        if (lane == 0) { P.selected[s] = -1; P.has_solution[s] = 0; }
        return;
    }
    const size_t c = (size_t)s * P.K + m.k;
    copy_row(P.cand.u + c * P.nn, P.best.u + (size_t)s * P.nn, P.nn, lane);
    copy_row(P.cand.x_ + c * P.nx, P.best.x_ + (size_t)s * P.nx, P.nx, lane);
    copy_row(P.cand.cost_all + c * P.mk, P.best.cost_all + (size_t)s * P.mk, P.mk, lane);
    copy_row(P.cand.e_cost_all + c * P.mk, P.best.e_cost_all + (size_t)s * P.mk, P.mk, lane);
    copy_row(P.cand.e_u_all + c * P.mk, P.best.e_u_all + (size_t)s * P.mk, P.mk, lane);
    if (P.best_viol) copy_row(P.cand_viol + c * P.mk, P.best_viol + (size_t)s * P.mk, P.mk, lane);
    if (lane == 0) {
        P.best.iter_O[s] = P.cand.iter_O[c];
        P.best.total_iter[s] = P.cand.total_iter[c];
        P.best.status[s] = P.cand.status[c];
        P.selected[s] = m.k;
        P.has_solution[s] = m.cls <= 1 ? 1 : 0;
    }
}

bool out_complete(const cfs_batch_out *o)
{
    return o->u && o->x_ && o->cost_all && o->e_cost_all && o->e_u_all && o->iter_O && o->total_iter && o->status;
}

}  // namespace

extern "C" int cfs_select_best_device(cfs_problem *p, int S, int K, const int *route_ok, const cfs_batch_out *cand,
                                      const double *cand_viol_all, const cfs_batch_out *best, double *best_viol_all, int *selected,
                                      int *has_solution, void *stream)
{
    if (K < 1 || K > CFS_WAVE) return cfs_fail(CFS_ERR_INVALID_ARG, "K=%d outside 1..%d", K, CFS_WAVE);
    if (S < 1) return cfs_fail(CFS_ERR_INVALID_ARG, "S=%d: at least one slot is needed", S);
    if (!p) return cfs_fail(CFS_ERR_INVALID_ARG, "NULL handle");
    if (!route_ok || !cand || !best || !selected || !has_solution) return cfs_fail(CFS_ERR_INVALID_ARG, "NULL argument");
    if (!out_complete(cand) || !out_complete(best)) return cfs_fail(CFS_ERR_INVALID_ARG, "NULL array in cand or best");
    if (!cand_viol_all && best_viol_all) return cfs_fail(CFS_ERR_INVALID_ARG, "best_viol_all needs cand_viol_all");
    if ((long long)S * K > p->d.max_batch)
        return cfs_fail(CFS_ERR_INVALID_ARG, "S*K=%lld exceeds max_batch=%d", (long long)S * K, p->d.max_batch);
    if (p->infeas == CFS_INFEAS_SOFTEN && !cand_viol_all)
        return cfs_fail(CFS_ERR_INVALID_ARG, "cand_viol_all is required on a CFS_INFEAS_SOFTEN handle");
    CFS_HIPCHK(hipSetDevice(p->device));
    SelectParams P;
    P.S = S; P.K = K; P.nn = p->nn; P.nx = p->nx; P.mk = p->d.MAX_O_ITER;
    P.route_ok = route_ok; P.cand = *cand; P.best = *best;
    P.cand_viol = cand_viol_all; P.best_viol = best_viol_all;
    P.selected = selected; P.has_solution = has_solution;
    const int blocks = (S + PLAN_WAVES - 1) / PLAN_WAVES;
    hipLaunchKernelGGL(cfs_select_best_kernel, dim3(blocks), dim3(CFS_WAVE * PLAN_WAVES), 0,
                       reinterpret_cast<hipStream_t>(stream), P);
    CFS_HIPCHK(hipGetLastError());
    return CFS_SUCCESS;
}
