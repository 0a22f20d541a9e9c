// cfs_mesh_query_dev.h -- point2surface_dis for host arrays: the kernel (a thread per segment, one hierarchy traversal each) and
// its launch.  Included by two units that differ in how they round: cfs_mesh_query.hip (no FMA contraction: the public
// cfs_mesh_segment_distance) and cfs_mesh.hip (contracted like the linearisation, dist_arm, clearance, IK and Cartesian units:
// cfs_debug_mesh_segment_distance_contracted, the entry through which the tests feed arbitrary segments to that build of
// cfs_mesh_dev.h).  Everything here is internal to the including unit.
#pragma once
#include "cfs_mesh_dev.h"
#include "cfs_host.h"

namespace {

struct SegQueryParams { DevMesh m; int n; const double *segs; double *dis, *pts; int *tri; };

__global__ __launch_bounds__(MESH_THREADS) void cfs_mesh_seg_kernel(SegQueryParams P)
{
    __shared__ int s_stack[MESH_STACK * MESH_THREADS];
    __shared__ float s_lbs[MESH_STACK * MESH_THREADS];
    const int i = blockIdx.x * MESH_THREADS + threadIdx.x;
    if (i >= P.n) return;
    double seg[6];
#pragma unroll
    for (int r = 0; r < 6; ++r) seg[r] = P.segs[(size_t)i * 6 + r];
    Best b;
    mesh_query<MESH_THREADS, false>(P.m, seg, seg + 3, -1, s_stack + threadIdx.x, s_lbs + threadIdx.x, b, nullptr);
    P.dis[i] = b.d;
    if (P.pts)
#pragma unroll
        for (int r = 0; r < 6; ++r) P.pts[(size_t)i * 6 + r] = b.pts[r];
    if (P.tri) P.tri[i] = b.tri >= 0 ? P.m.orig[b.tri] : -1;
}

// dis[n], points[n x 6] (may be NULL), tri[n] (may be NULL); `what` names the entry point in error messages
int mesh_segment_query(const cfs_mesh *m, int n, const double *segs, double *dis, double *points, int *tri, const char *what)
{
    if (!m || !segs || !dis || n < 1) return cfs_fail(CFS_ERR_INVALID_ARG, "mesh/segs/dis must be given, n >= 1");
    CFS_HIPCHK(hipSetDevice(m->device));
    const size_t nn = n;
    Stage st;
    SegQueryParams q{m->view(), n, st.up(segs, nn * 6), st.out<double>(nn), st.out<double>(nn * 6), st.out<int>(nn)};
    if (st.err == hipSuccess) {
        hipLaunchKernelGGL(cfs_mesh_seg_kernel, dim3((n + MESH_THREADS - 1) / MESH_THREADS), dim3(MESH_THREADS), 0, nullptr, q);
        st.err = hipGetLastError();
    }
    st.down(dis, q.dis, nn); st.down(points, q.pts, nn * 6); st.down(tri, q.tri, nn);
    return st.result(what);
}

}  // namespace
