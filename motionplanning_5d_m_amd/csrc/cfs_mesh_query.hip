// cfs_mesh_query.hip -- point2surface_dis (cfs_mesh_segment_distance), the public segment-to-mesh query, in a unit of its own
// because it is built WITHOUT FMA contraction (Makefile), like cfs_rrt.hip: plain IEEE arithmetic in the order written, so that
// it rounds like the CPU statement of the contract (oracle/mesh_oracle.c).  That matters where the contract's tie rule decides:
// for a segment in the surface, or parallel to a wall or an edge, a continuum of axis points is at the minimum distance, the
// candidates differ in their last bits only, and contracted arithmetic orders them otherwise than the oracle does -- the two then
// report closest pairs a whole segment apart (tests/test_gpu_mesh_geometry.py).  The linearisation and dist_arm over a mesh
// (cfs_mesh.hip) stay contracted: they are the hot path, and only their distances are compared; the same kernel in that build is
// cfs_debug_mesh_segment_distance_contracted.  Contract and hierarchy: cfs_mesh.hip's head comment, cfs_mesh_dev.h.
#include "cfs_mesh_query_dev.h"

extern "C" {

// point2surface_dis for n segments (host arrays): dis[n], points[n x 6] (may be NULL), tri[n] (may be NULL)
int cfs_mesh_segment_distance(const cfs_mesh *m, int n, const double *segs, double *dis, double *points, int *tri)
{
    return mesh_segment_query(m, n, segs, dis, points, tri, "cfs_mesh_segment_distance");
}

}  // extern "C"
