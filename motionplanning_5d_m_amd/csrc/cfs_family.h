// cfs_family.h -- host numerics of a problem family: everything cfs_api.hip derives on the CPU from a descriptor, cost weights or
// mesh poses before it touches the device.  Plain arrays and std::vector, no HIP header: the unit compiles and runs without a GPU
// (tests/native/family_check.cpp).  Written in long double where the comments of cfs_family.cpp say why.
#pragma once
#include "../../include/cfs_hip.h"
#include <vector>

// One record per (mesh, interval) of a handle with mesh motion, derived on the host in double (cfs_problem_set_mesh_motion):
// [0] 1: the interval is interpolated, 0: the stored pose of its waypoint is held over it (interval 0, bitwise equal poses);
// [1..3] axis a, [4] theta, [5..13] R_{i-1} row-major, [14..16] c_w(0), [17..19] c_w(1), [20..22] c_j, [23] v_mesh
constexpr int CLEAR_ITV = 24;

// what an entry point refuses: code == CFS_SUCCESS, or a cfs_error and the text the caller hands to cfs_fail
struct FamilyRefusal {
    int code = CFS_SUCCESS;
    char text[256] = "";
    explicit operator bool() const { return code != CFS_SUCCESS; }
};

std::vector<double> symmetrise(int nn, const double *QQ);
bool spd_inverse(int n, const double *Asym, std::vector<double> &inv, std::vector<long double> &Li);
double lambda_max_upper(int nn, std::vector<double> G);
double sym_lambda_max(int n, std::vector<double> A);

// sys_info.Aaug / Baug (either may be null) against the double integrator of robot.A / robot.B
FamilyRefusal check_double_integrator(int nj, int H, double dt, const double *Aaug, const double *Baug);

struct FamilyMatrices {
    std::vector<double> Hinv, Hq, M1n, M2n;   // nn x nn column-major each
    double lmax_vel = 0.0, lmax_H = 1.0;
};
FamilyRefusal family_matrices(int nj, int H, double dt, int mode, const double *QQ, FamilyMatrices &f);

struct WeightFamily {
    std::vector<double> Qaug, QQ;             // nx x nx, nn x nn column-major
    double Rs[36];                            // nj x nj column-major: cR*(Rblk + Rblk')
    double alpha = 0.0;                       // 1/max(svd(QQ)) when asked for, 0 otherwise
};
void family_from_weights(int nj, int H, double dt, const cfs_cost_weights *w, bool want_alpha, WeightFamily &f);

// F1 (nn x nj), F2 (nn x nj), Cq (2nj x 2nj) of cfs_set_state_cost
void state_cost_terms(int nj, int H, double dt, const double *Qaug, std::vector<double> &F1, std::vector<double> &F2, std::vector<double> &Cq);

// poses: nmesh x H x 12 row-major [R | t]  ->  inv: their inverses [R' | -R't]
FamilyRefusal invert_mesh_poses(int nmesh, int H, const double *poses, std::vector<double> &inv);
// f[0..2] = c_j (centre of the bounding box), f[3] = r_j (largest vertex distance from it) of the nt stored triangles (nt x 9)
void mesh_frame(const double *tri, int nt, double *f);
void mesh_motion_intervals(const double *T, int H, double dt, const double *frame, double *itv, int jm, int &turn_mesh, int &turn_wp);
