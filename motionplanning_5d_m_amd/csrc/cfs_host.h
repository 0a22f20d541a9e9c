// cfs_host.h -- host-side helpers shared by the translation units of libcfs_hip.so (not part of the C ABI).
#pragma once
#include "cfs_device.h"
#include "cfs_family.h"                                  // CLEAR_ITV, the record cfs_clear_mesh.hip reads
#include <type_traits>
#include <vector>

int cfs_fail(int code, const char *fmt, ...);            // records the message of cfs_last_error(), returns code
int cfs_current_device();                                // device chosen with cfs_set_device
int cfs_use_device(int device);                          // CFS_ERR_NO_DEVICE unless a device is visible, then hipSetDevice(device)
int cfs_check_robot(const cfs_robot *r, int nj);         // CFS_SUCCESS or an error code (message recorded)
void cfs_build_dev_robot(const cfs_robot &r, DevRobot &d);
// reads and / or zeroes a __device__ unsigned long long counter (its address) of the current device: cfs_debug_*_frontier_overflows
int cfs_frontier_overflows(const void *symbol, unsigned long long *count, int reset);

#define CFS_HIPCHK(call)                                                                                     \
    do {                                                                                                     \
        hipError_t e_ = (call);                                                                              \
        if (e_ != hipSuccess) return cfs_fail(CFS_ERR_HIP, "%s failed: %s", #call, hipGetErrorString(e_));   \
    } while (0)

// f(std::integral_constant<int, NJ>{}) for the runtime joint count nj = 2..6: how every launcher picks its kernel instantiation
template <class F> hipError_t cfs_for_nj(int nj, F &&f)
{
    switch (nj) {
    case 2: return f(std::integral_constant<int, 2>{});
    case 3: return f(std::integral_constant<int, 3>{});
    case 4: return f(std::integral_constant<int, 4>{});
    case 5: return f(std::integral_constant<int, 5>{});
    case 6: return f(std::integral_constant<int, 6>{});
    default: return hipErrorInvalidValue;
    }
}

// a device array that a handle owns: freed by release(), by the next alloc() and by the destructor; movable, not copyable
template <class T>
struct DevBuf {
    T *p = nullptr;
    size_t n = 0;
    DevBuf() = default;
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    DevBuf(DevBuf &&o) noexcept : p(o.p), n(o.n) { o.p = nullptr; o.n = 0; }
    DevBuf &operator=(DevBuf &&o) noexcept
    {
        if (this != &o) { release(); p = o.p; n = o.n; o.p = nullptr; o.n = 0; }
        return *this;
    }
    ~DevBuf() { release(); }
    hipError_t alloc(size_t count)                       // the old block goes first (hipFree waits for whatever still reads it)
    {
        release();
        n = count;
        return hipMalloc(reinterpret_cast<void **>(&p), (count ? count : 1) * sizeof(T));
    }
    hipError_t upload(const T *h, size_t count)          // alloc + copy of count elements from the host
    {
        hipError_t e = alloc(count);
        if (e == hipSuccess && count) e = hipMemcpy(p, h, count * sizeof(T), hipMemcpyHostToDevice);
        return e;
    }
    hipError_t zeros(size_t count)                       // alloc + zero fill
    {
        hipError_t e = alloc(count);
        if (e == hipSuccess && count) e = hipMemset(p, 0, count * sizeof(T));
        return e;
    }
    void release() { if (p) (void)hipFree(p); p = nullptr; n = 0; }
};

// device staging of host arrays for the host-pointer entry points: the first error sticks and turns every later call into a no-op,
// the destructor frees what was allocated
struct Stage {
    std::vector<void *> ptrs;
    hipError_t err = hipSuccess;
    template <class T> T *up(const T *h, size_t n)       // n elements (room for one when n is 0); h == nullptr: left uninitialised
    {
        if (err != hipSuccess) return nullptr;
        void *d = nullptr;
        err = hipMalloc(&d, (n ? n : 1) * sizeof(T));
        if (err != hipSuccess) return nullptr;
        ptrs.push_back(d);
        if (h && n) err = hipMemcpy(d, h, n * sizeof(T), hipMemcpyHostToDevice);
        return static_cast<T *>(d);
    }
    template <class T> T *out(size_t n) { return up<T>(nullptr, n); }
    template <class T> T *zeros(size_t n)
    {
        T *d = out<T>(n);
        if (d && n) err = hipMemset(d, 0, n * sizeof(T));
        return d;
    }
    template <class T> void down(T *h, const T *d, size_t n)   // h == nullptr (an optional output): nothing to do
    {
        if (err == hipSuccess && h && n) err = hipMemcpy(h, d, n * sizeof(T), hipMemcpyDeviceToHost);
    }
    int result(const char *what) const                   // CFS_SUCCESS, or CFS_ERR_HIP with "<what> failed: <HIP's message>"
    {
        return err == hipSuccess ? CFS_SUCCESS : cfs_fail(CFS_ERR_HIP, "%s failed: %s", what, hipGetErrorString(err));
    }
    ~Stage() { for (void *q : ptrs) (void)hipFree(q); }
};

// ---- mesh obstacles (cfs_mesh.hip) --------------------------------------------------------------
struct BvhNode {                 // 128 B = one L2 line: an inner node carries the boxes of BOTH children, so a level costs one
    double lo[2][3], hi[2][3];   // dependent load; an empty child has lo = +inf, hi = -inf (its lower bound is +inf)
    int child[2];                // >= 0: inner node index; < 0: leaf, -(first * 8 + count) - 1, triangles [first, first + count) in BVH order
    int pad[2];
};
struct DevMesh {                 // device view of one mesh
    const BvhNode *nodes;
    const double *tri;           // nt x 9 (A, B, C), in BVH order
    const int *orig;             // BVH order -> index in the caller's triangle list
    int nnodes, nt;
    // where a wave-cooperative traversal starts: the hierarchy cut open to <= 64 inner nodes (a wavefront's width), plus the
    // triangles of the leaves met on the way -- the 1, 2, 4, ... lane rounds near the root are one dependent load each
    const int *cut, *cut_tri;
    int ncut, ncut_tri;
};
struct cfs_mesh {
    int device = 0, nt = 0, nnodes = 0, depth = 0;
    double bbox[6] = {0, 0, 0, 0, 0, 0};
    DevBuf<BvhNode> nodes;
    DevBuf<double> tri;
    DevBuf<int> orig;
    DevBuf<int> cut;             // ncut node indices, then ncut_tri triangle indices
    int ncut = 0, ncut_tri = 0;
    DevMesh view() const { return DevMesh{nodes.p, tri.p, orig.p, nnodes, nt, cut.p, cut.p + ncut, ncut, ncut_tri}; }
};

struct LinMeshParams {           // distance + literal finite-difference Jacobian against mesh obstacles
    const DevRobot *rb;
    int B, H, nmesh;
    const DevMesh *meshes;       // device array [nmesh]
    const double *x_;            // B x (H*2*NJ)
    const int *status_done;     // B, may be null: problems whose entry is non-zero have finished and are skipped
    int seed_prev;               // base_t holds the winning triangles of the previous outer iteration of the same problems: their
                                 // distance to the moved link is one more upper bound (the trajectory moves little between iterations)
    double *dist;                // B x nmesh x H
    double *grad;                // B x nmesh x H x NJ
    // workspace per (problem, waypoint), sizes from linearize_mesh_workspace
    double *ends;                // [NVT][6]          end points of every link variant
    double *upper_d;             // [NJ][nmesh]       greedy upper bound of the base-pose distance
    double *base_d;              // [NJ][nmesh]       base-pose distance (surrogate applied; +inf: farther than any link that matters)
    int *base_t;                 // [NJ][nmesh]       base-pose winning triangle (hierarchy order)
    double *shift_d;             // [nmesh][NVT-NJ]   shifted-pose distances of the candidate links, +inf otherwise
    int *near;                   // [NJ][nmesh][1+cap] count (-1: overflow) + triangles within the shift margin of the base minimum
    double *piece_d, *piece_nd;  // per piece of a link axis: record / near-list distances (sizes from linearize_mesh_workspace)
    int *piece_i;
    const double *mesh_pose;     // nmesh x H x 12, may be null (static meshes): the INVERSE of each waypoint's pose [R | t] of a mesh,
                                 // row-major [R' | -R't]; the kernels measure link ends mapped by it against the mesh as stored
};
hipError_t launch_linearize_mesh(int nj, const LinMeshParams &p, hipStream_t s);
void linearize_mesh_workspace(int nj, int nmesh, size_t *ends, size_t *base, size_t *shift, size_t *near, size_t *piece_d, size_t *piece_i,
                              size_t *piece_nd);

// ---- clearance audit against mesh obstacles (cfs_clear_mesh.hip) ---------------------------------------
enum { CLEAR_MESH_BOUND = 1, CLEAR_MESH_SEED = 2 };      // ClearMeshParams::opt
struct ClearMeshParams {
    const DevRobot *rb;
    int B, H, nj, nobs, nmesh, S;                        // nobs: all obstacles of the handle (output stride); the meshes are the last nmesh
    int opt;                                             // CLEAR_MESH_*: how the queries use the time coherence (same results either way)
    double dt;
    const DevMesh *meshes;                               // device array [nmesh]
    const double *x_, *u, *xR1;                          // B x H*2nj, B x H*nj, B x 2nj
    double *dist_wp, *dist_path, *dist_lower, *t_path;   // B x nobs each: columns nobs - nmesh .. nobs - 1 are written
    int *link_path, *tri_path;                           // B x nobs; tri_path: every column (-1 in the line columns)
    // workspace of the handle, G = H*S + 1 samples per problem
    double *ws_d, *ws_L;                                 // B x nmesh x G per-sample distance; B x G arm's share of the Lipschitz bound
    int *ws_lk, *ws_tri, *ws_seed;                       // B x nmesh x G closest link / triangle; B x (H+1) x nj x nmesh waypoint winners
    const double *rho;                                   // device, CFS_MAX_LINKS^2 (cfs_clear_build_rho)
    // moving meshes (cfs_clearance_mesh_motion*), both null for static meshes: the table launch_clear_mesh_poses writes
    const double *pose;                                  // nmesh x G x 12: row-major [R' | c_j - R'c_w] of (mesh, sample), world -> stored frame
    const double *v_mesh;                                // nmesh x H: bound of the surface speed of a mesh in an interval
};
hipError_t launch_clearance_mesh(const ClearMeshParams &p, hipStream_t s);
// writes the pose table of S sub-steps: out_pose nmesh x (H*S + 1) x 12, out_v nmesh x H; inv: the stored inverse poses, nmesh x H x 12
hipError_t launch_clear_mesh_poses(int nmesh, int H, int S, const double *itv, const double *inv, double *out_pose, double *out_v, hipStream_t s);

// ---- CHOMP_FANUC (cfs_chomp.hip) -----------------------------------------------------------------------
struct ChompParams {
    const DevRobot *rb;
    int B, H, nobs, max_o_iter;
    double dt, alpha, epsilon_O;
    const double *QQ;                                    // nn x nn column-major
    const double *x_init, *xR1, *ff, *caug, *obs, *u0;   // per problem: H*ns, ns, nn, 1, nobs*6, nn
    const double *D, *eps;                               // nobs: obs{j}.D, obs{j}.epsilon
    double *u, *x_, *cost_all, *e_cost_all, *e_u_all;
    int *iter_O, *total_iter, *status;
    double delta[26], fdarule[2], rmat[12], pinv[12], cov_scale;   // derivest's constant tables (chomp_derivest_tables)
};
hipError_t launch_chomp(int nj, const ChompParams &p, hipStream_t s);
void chomp_derivest_tables(ChompParams &p);
bool chomp_fits(int nj, int H, int nobs);

// ---- RRT / RRT* tree growth (cfs_rrt.hip) ---------------------------------------------------------------------
struct RrtParams {
    DevRobot rb;                                         // by value: no device allocation, no synchronisation in the _device entry
    int S, nobs, solver, max_iter, per_tree;             // trees; obstacles; 0 RRT | 1 RRT*; MAX_ITER; 1: x0 / goal / goal_th are S x nstate
    double bi, rewire;                                   // goal bias threshold (0.5, RRT_FANUC.m:38), re-parenting radius (0.2, :135)
    const double *x0, *goal, *goal_th;                   // nstate (or S x nstate)
    const double *region_g, *region_s, *sample_off, *ratial;   // nstate
    const double *obs, *D;                               // nobs x 6, nobs
    const double *uniforms;                              // S x ndraw or null (then the counter-based generator with `seed`)
    int ndraw;
    unsigned long long seed;
    long long max_draws;                                 // generator mode: uniforms a tree may consume before it gives up (fail = 2)
    int *node_num, *fail, *parent, *route_len;           // S, S, S x (max_iter+1), S
    double *nodes, *total_dis, *all_ee, *route;          // S x (max_iter+1) x nstate, S x (max_iter+1), S x max_iter x 3 (may be null), S x (max_iter+1) x nstate
    long long *draws_used, *proposals;                   // S (may be null)
};
hipError_t launch_rrt(int nj, const RrtParams &p, hipStream_t s);
size_t rrt_lds_bytes(int nj, int max_iter);
// mesh obstacles of the feasibility test (cfs_rrt_grow_mesh*): by value as well, a second kernel argument of the mesh kernels only
enum { RRT_MESH_NONE = 0, RRT_MESH_PER_LANE = 1, RRT_MESH_WAVE = 2 };   // variant A | variant B
constexpr int RRT_MESH_DEFAULT = RRT_MESH_WAVE;          // flags == 0: the variant the measurement of DESIGN.md section 19 names
constexpr int RRT_FRONTIER_CAP = 512;                    // variant B: (pair, node) entries of the wave's frontier
constexpr int RRT_FRONTIER_SMALL = 8;                    // CFS_RRT_MESH_SMALL_FRONTIER: forces the overflow path under test
struct RrtMeshEntry {
    const BvhNode *nodes;
    const double *tri;                                   // nt x 9, hierarchy order
    double thr;                                          // max(D_j, 1e-4): a triangle closer than this rejects the node
    int nt, pad;
};
struct RrtMeshArgs {
    int nmesh, cap;                                      // cap: variant B's frontier capacity (<= RRT_FRONTIER_CAP)
    RrtMeshEntry m[CFS_MAX_OBS];
};
hipError_t launch_rrt_mesh(int nj, int variant, const RrtParams &p, const RrtMeshArgs &ma, hipStream_t s);
size_t rrt_mesh_lds_bytes(int nj, int max_iter, int variant);      // rrt_lds_bytes + the variant's mesh scratch
// The mesh table of a cfs_rrt_grow_mesh* / cfs_ik_solve_mesh* call -> kernel argument + variant (RRT_MESH_NONE when nmesh is 0); host
// work only, nothing is launched or allocated.  min_nmesh: 0 (RRT) | 1 (IK).  The device of a mesh is compared last, so that every
// other refusal is the same with and without a device.
int cfs_check_mesh_table(int nobs, int nmesh, const cfs_mesh *const *meshes, const double *D_mesh, int flags, int min_nmesh, int default_variant,
                         RrtMeshArgs &ma, int &variant);
// cfs_ik_solve_mesh* (cfs_ik.hip) runs the same two variants on its candidates; flags == 0: the variant the measurement of DESIGN.md
// section 21 names
constexpr int IK_MESH_DEFAULT = RRT_MESH_WAVE;
// cfs_cart_path_mesh* (cfs_cart.hip) runs them on the rows of a traced line; flags == 0: variant B on the strength of DESIGN.md section
// 19, as section 21 does (section 24 says which measurement is owed)
constexpr int CART_MESH_DEFAULT = RRT_MESH_WAVE;
