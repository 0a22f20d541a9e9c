// cfs_tool_host.h -- what the entries of cfs_ik.hip and cfs_cart.hip share on the host (not part of the C ABI): the checks of the
// descriptor fields that cfs_ik_desc and cfs_cart_desc have in common, with one set of messages, and the mesh table of a *_mesh* call.
// cfs_time.hip takes the check of the chain (check_tool_chain) and the array helpers from here.
// The order of the refusals is observable through cfs_last_error(): a unit calls check_tool_head, makes its own refusals (restarts |
// candidates, steps), then check_tool_max_iter, its own again (max_joint_step), check_tool_fields, its own pointer check,
// check_tool_io, and fill_tool_params last.
#pragma once
#include "cfs_host.h"
#include <cmath>
#include <cstring>

inline bool finite3(const double *v) { return std::isfinite(v[0]) && std::isfinite(v[1]) && std::isfinite(v[2]); }
inline bool all_finite(const double *v, size_t n)
{
    for (size_t i = 0; i < n; ++i)
        if (!std::isfinite(v[i])) return false;
    return true;
}

// the meshes of a cfs_ik_solve_mesh* / cfs_cart_path_mesh* call, and what its kernels take of them: RRT's table (thresholds, frontier
// capacity), then the margins for the winner's clearance
struct MeshCall { int nmesh; const cfs_mesh *const *meshes; const double *D_mesh; int flags; };
struct ToolMeshArgs {
    RrtMeshArgs MA;
    double D[CFS_MAX_OBS];
};
inline int check_mesh_call(int nobs, const MeshCall &c, int default_variant, ToolMeshArgs &m, int &variant)
{
    memset(&m, 0, sizeof m);
    int rc = cfs_check_mesh_table(nobs, c.nmesh, c.meshes, c.D_mesh, c.flags, 1, default_variant, m.MA, variant);
    if (rc) return rc;
    for (int j = 0; j < c.nmesh; ++j) m.D[j] = c.D_mesh[j];
    return CFS_SUCCESS;
}

// the robot and the joint count of a descriptor (cfs_time_desc has these and no tool direction)
template <class Desc> int check_tool_chain(const Desc *d)
{
    if (!d) return cfs_fail(CFS_ERR_INVALID_ARG, "NULL descriptor");
    int rc = cfs_check_robot(&d->robot, d->njoint);
    if (rc) return rc;
    if (d->njoint < 2) return cfs_fail(CFS_ERR_INVALID_ARG, "njoint %d unsupported (2..6)", d->njoint);
    return CFS_SUCCESS;
}

// Desc: cfs_ik_desc | cfs_cart_desc
template <class Desc> int check_tool_head(const Desc *d)
{
    int rc = check_tool_chain(d);
    if (rc) return rc;
    if (d->use_axis != 0 && d->use_axis != 1) return cfs_fail(CFS_ERR_INVALID_ARG, "use_axis must be 0 or 1, not %d", d->use_axis);
    return CFS_SUCCESS;
}

inline int check_tool_max_iter(int max_iter)
{
    return max_iter < 1 || max_iter > 1000 ? cfs_fail(CFS_ERR_INVALID_ARG, "max_iter %d outside 1..1000", max_iter) : (int)CFS_SUCCESS;
}

// obstacles, tolerances, tool point and axis, joint ranges and weights, the number of targets
template <class Desc> int check_tool_fields(const Desc *d, int T)
{
    if (d->nobs < 0 || d->nobs > CFS_MAX_OBS) return cfs_fail(CFS_ERR_INVALID_ARG, "nobs %d outside 0..%d", d->nobs, CFS_MAX_OBS);
    if (d->nobs > 0 && (!d->obs || !d->D)) return cfs_fail(CFS_ERR_INVALID_ARG, "obs / D must be given");
    if (!(std::isfinite(d->tol_pos) && d->tol_pos > 0.0 && std::isfinite(d->tol_axis) && d->tol_axis > 0.0))
        return cfs_fail(CFS_ERR_INVALID_ARG, "tol_pos / tol_axis must be finite and > 0");
    if (!finite3(d->tool) || !finite3(d->tool_axis)) return cfs_fail(CFS_ERR_INVALID_ARG, "tool / tool_axis must be finite");
    if (d->use_axis && !(d->tool_axis[0] * d->tool_axis[0] + d->tool_axis[1] * d->tool_axis[1] + d->tool_axis[2] * d->tool_axis[2] > 0.0))
        return cfs_fail(CFS_ERR_INVALID_ARG, "tool_axis is zero");
    if (!d->lo || !d->hi) return cfs_fail(CFS_ERR_INVALID_ARG, "lo / hi must be given");
    for (int c = 0; c < d->njoint; ++c) {
        if (!std::isfinite(d->lo[c]) || !std::isfinite(d->hi[c]) || !(d->lo[c] < d->hi[c]))
            return cfs_fail(CFS_ERR_INVALID_ARG, "joint %d: lo / hi must be finite with lo < hi", c);
        if (d->weight && !(std::isfinite(d->weight[c]) && d->weight[c] > 0.0)) return cfs_fail(CFS_ERR_INVALID_ARG, "weight[%d] must be finite and > 0", c);
    }
    if (T < 1) return cfs_fail(CFS_ERR_INVALID_ARG, "at least one target is needed");
    return CFS_SUCCESS;
}

// Out: cfs_ik_out | cfs_cart_out
template <class Desc, class Out> int check_tool_io(const Desc *d, const double *target_axis, const Out *out, const char *axis_name = "target_axis")
{
    if (d->use_axis && !target_axis) return cfs_fail(CFS_ERR_INVALID_ARG, "use_axis = 1 needs %s", axis_name);
    if (!out || !out->theta || !out->status) return cfs_fail(CFS_ERR_INVALID_ARG, "out, out->theta and out->status must be given");
    return CFS_SUCCESS;
}

// the by-value part of the kernel's parameter block (IkParams | CartParams) that both have: everything else of P is zeroed
template <class Desc, class Params> void fill_tool_params(const Desc *d, int T, Params &P)
{
    memset(&P, 0, sizeof P);
    cfs_build_dev_robot(d->robot, P.rb);
    P.T = T; P.nobs = d->nobs; P.use_axis = d->use_axis; P.max_iter = d->max_iter;
    const double an = std::sqrt(d->tool_axis[0] * d->tool_axis[0] + d->tool_axis[1] * d->tool_axis[1] + d->tool_axis[2] * d->tool_axis[2]);
    for (int q = 0; q < 3; ++q) { P.tool[q] = d->tool[q]; P.axis[q] = an > 0.0 ? d->tool_axis[q] / an : 0.0; }
    for (int c = 0; c < d->njoint; ++c) { P.lo[c] = d->lo[c]; P.hi[c] = d->hi[c]; P.w[c] = d->weight ? d->weight[c] : 1.0; }
    P.tol_pos = d->tol_pos; P.tol_axis = d->tol_axis;
}

// the values of the host arrays of such a call (the host-pointer entries only: a _device entry cannot read its inputs).  npts poses per
// target (cfs_cart_follow*'s tables; 1 elsewhere), named in the messages as the entry names them
template <class Desc>
int check_tool_arrays(const Desc *d, int T, const double *target_pos, const double *target_axis, const double *theta_ref, size_t npts = 1,
                      const char *pos_name = "target_pos", const char *axis_name = "target_axis")
{
    const size_t nT = T, nj = d->njoint, nobs = d->nobs;
    if (!all_finite(target_pos, nT * npts * 3) || !all_finite(theta_ref, nT * nj))
        return cfs_fail(CFS_ERR_INVALID_ARG, "%s / theta_ref must be finite", pos_name);
    if (nobs && (!all_finite(d->obs, nobs * 6) || !all_finite(d->D, nobs))) return cfs_fail(CFS_ERR_INVALID_ARG, "obs / D must be finite");
    if (d->use_axis) {
        if (!all_finite(target_axis, nT * npts * 3)) return cfs_fail(CFS_ERR_INVALID_ARG, "%s must be finite", axis_name);
        for (size_t t = 0; t < nT * npts; ++t) {
            const double *v = target_axis + t * 3;
            if (!(v[0] * v[0] + v[1] * v[1] + v[2] * v[2] > 0.0)) return cfs_fail(CFS_ERR_INVALID_ARG, "%s row %d is zero", axis_name, (int)t);
        }
    }
    return CFS_SUCCESS;
}
