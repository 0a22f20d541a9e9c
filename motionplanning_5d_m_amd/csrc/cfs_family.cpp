// cfs_family.cpp -- host numerics of a problem family (cfs_family.h): the linear algebra behind cfs_problem_create,
// cfs_problem_create_from_weights, cfs_set_state_cost and cfs_problem_set_mesh_motion.  No HIP, no device.
#include "cfs_family.h"
#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>

namespace {

FamilyRefusal refuse(int code, const char *fmt, ...)
{
    FamilyRefusal r;
    r.code = code;
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(r.text, sizeof r.text, fmt, ap);
    va_end(ap);
    return r;
}

}  // namespace

// lambda_max(G) <= ||G^(2^k)||_inf^(1/2^k) for symmetric G: five squarings are within n^(1/32) of it (+ margin for fp64 rounding)
double lambda_max_upper(int nn, std::vector<double> G)
{
    std::vector<double> T2((size_t)nn * nn);
    double logscale = 0.0;
    for (int it = 0; it < 5; ++it) {
        double nrm = 0.0;
        for (int i = 0; i < nn; ++i) { double s = 0.0; for (int j = 0; j < nn; ++j) s += fabs(G[i + (size_t)j * nn]); if (s > nrm) nrm = s; }
        if (!(nrm > 0.0)) return 0.0;
        for (auto &v : G) v /= nrm;
        logscale = 2.0 * (logscale + log(nrm));
        for (int i = 0; i < nn; ++i)
            for (int j = 0; j < nn; ++j) { double s = 0.0; for (int k = 0; k < nn; ++k) s += G[i + (size_t)k * nn] * G[k + (size_t)j * nn]; T2[i + (size_t)j * nn] = s; }
        G.swap(T2);
    }
    double nrm = 0.0;
    for (int i = 0; i < nn; ++i) { double s = 0.0; for (int j = 0; j < nn; ++j) s += fabs(G[i + (size_t)j * nn]); if (s > nrm) nrm = s; }
    return exp((logscale + log(nrm)) / 32.0) * 1.001;
}

// (QQ + QQ') / 2: quadprog symmetrises its Hessian silently
std::vector<double> symmetrise(int nn, const double *QQ)
{
    std::vector<double> sym((size_t)nn * nn);
    for (int j = 0; j < nn; ++j)
        for (int i = 0; i < nn; ++i) sym[i + (size_t)j * nn] = 0.5 * (QQ[i + (size_t)j * nn] + QQ[j + (size_t)i * nn]);
    return sym;
}

// symmetric positive definite inverse in extended precision (once per problem family)
bool spd_inverse(int n, const double *Asym, std::vector<double> &inv, std::vector<long double> &Li)
{
    std::vector<long double> L((size_t)n * n, 0.0L);
    Li.assign((size_t)n * n, 0.0L);
    for (int j = 0; j < n; ++j) {
        long double s = Asym[j + (size_t)j * n];
        for (int k = 0; k < j; ++k) s -= L[j + (size_t)k * n] * L[j + (size_t)k * n];
        if (!(s > 0)) return false;
        const long double ljj = sqrtl(s);
        L[j + (size_t)j * n] = ljj;
        for (int i = j + 1; i < n; ++i) {
            long double t = Asym[i + (size_t)j * n];
            for (int k = 0; k < j; ++k) t -= L[i + (size_t)k * n] * L[j + (size_t)k * n];
            L[i + (size_t)j * n] = t / ljj;
        }
    }
    for (int j = 0; j < n; ++j) {          // Li = L^{-1}, lower
        Li[j + (size_t)j * n] = 1.0L / L[j + (size_t)j * n];
        for (int i = j + 1; i < n; ++i) {
            long double s = 0.0L;
            for (int k = j; k < i; ++k) s -= L[i + (size_t)k * n] * Li[k + (size_t)j * n];
            Li[i + (size_t)j * n] = s / L[i + (size_t)i * n];
        }
    }
    inv.assign((size_t)n * n, 0.0);
    for (int i = 0; i < n; ++i)
        for (int j = 0; j <= i; ++j) {     // A^{-1} = Li' Li
            long double s = 0.0L;
            for (int k = i; k < n; ++k) s += Li[k + (size_t)i * n] * Li[k + (size_t)j * n];
            inv[i + (size_t)j * n] = inv[j + (size_t)i * n] = (double)s;
        }
    return true;
}

// largest eigenvalue of a symmetric matrix by cyclic Jacobi rotations (once per family, n <= 384)
double sym_lambda_max(int n, std::vector<double> A)
{
    for (int sweep = 0; sweep < 60; ++sweep) {
        double off = 0.0, dia = 0.0;
        for (int j = 0; j < n; ++j)
            for (int i = 0; i < n; ++i) (i == j ? dia : off) += A[i + (size_t)j * n] * A[i + (size_t)j * n];
        if (off <= 1e-30 * dia) break;
        for (int p_ = 0; p_ < n - 1; ++p_)
            for (int q_ = p_ + 1; q_ < n; ++q_) {
                const double apq = A[p_ + (size_t)q_ * n];
                if (apq == 0.0) continue;
                const double theta = (A[q_ + (size_t)q_ * n] - A[p_ + (size_t)p_ * n]) / (2.0 * apq);
                const double t = (theta >= 0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
                const double c = 1.0 / sqrt(t * t + 1.0), sn = t * c;
                for (int k = 0; k < n; ++k) {               // columns p, q
                    const double akp = A[k + (size_t)p_ * n], akq = A[k + (size_t)q_ * n];
                    A[k + (size_t)p_ * n] = c * akp - sn * akq;
                    A[k + (size_t)q_ * n] = sn * akp + c * akq;
                }
                for (int k = 0; k < n; ++k) {               // rows p, q
                    const double apk = A[p_ + (size_t)k * n], aqk = A[q_ + (size_t)k * n];
                    A[p_ + (size_t)k * n] = c * apk - sn * aqk;
                    A[q_ + (size_t)k * n] = sn * apk + c * aqk;
                }
            }
    }
    double m = A[0];
    for (int i = 1; i < n; ++i) m = std::max(m, A[i + (size_t)i * n]);
    return m;
}

// sys_info.Aaug / Baug must be the double integrator of robot.A / robot.B
// (robotproperty2.m:136-139, main_FANUC.m:79-86): the kernels roll out with prefix sums.
FamilyRefusal check_double_integrator(int nj, int H, double dt, const double *Aaug, const double *Baug)
{
    const int ns = 2 * nj, nx = H * ns;
    if (Baug) {
        for (int i = 0; i < H; ++i)
            for (int k = 0; k < H; ++k)
                for (int r = 0; r < ns; ++r)
                    for (int c = 0; c < nj; ++c) {
                        double want = 0.0;
                        if (k <= i && (r % nj) == c) want = r < nj ? ((double)(i - k) + 0.5) * dt * dt : dt;
                        const double got = Baug[(i * ns + r) + (size_t)(k * nj + c) * nx];
                        if (fabs(got - want) > 1e-12 * (1.0 + fabs(want)))
                            return refuse(CFS_ERR_DYNAMICS, "Baug(%d,%d)=%.17g, double integrator expects %.17g", i * ns + r + 1, k * nj + c + 1, got, want);
                    }
    }
    if (Aaug) {
        for (int i = 0; i < H; ++i)
            for (int r = 0; r < ns; ++r)
                for (int c = 0; c < ns; ++c) {
                    double want = (r == c) ? 1.0 : 0.0;
                    if (r < nj && c == r + nj) want = (double)(i + 1) * dt;
                    const double got = Aaug[(i * ns + r) + (size_t)c * nx];
                    if (fabs(got - want) > 1e-12 * (1.0 + fabs(want)))
                        return refuse(CFS_ERR_DYNAMICS, "Aaug(%d,%d)=%.17g, double integrator expects %.17g", i * ns + r + 1, c + 1, got, want);
                }
    }
    return FamilyRefusal{};
}

FamilyRefusal family_matrices(int nj, int H, double dt, int mode, const double *QQ, FamilyMatrices &f)
{
    const int nn = H * nj;
    // H^{-1} of the QP Hessian: QQ symmetrised (quadprog does so silently) for CFS, identity for the
    // PSGCFS projection (PSGCFS_FANUC.m:117)
    std::vector<double> &Hinv = f.Hinv;
    std::vector<long double> Li;            // L^{-1} (lower), H = L L'
    const std::vector<double> sym = symmetrise(nn, QQ);
    if (!spd_inverse(nn, sym.data(), Hinv, Li)) return refuse(CFS_ERR_NOT_SPD, "QQ is not positive definite");
    std::vector<double> &Hq = f.Hq;   // Hessian inverse used by the QP
    if (mode == CFS_MODE_CFS) Hq = Hinv;
    else {
        Hq.assign((size_t)nn * nn, 0.0);
        for (int i = 0; i < nn; ++i) Hq[i + (size_t)i * nn] = 1.0;
    }
    // Family matrices H^{-1}Bpos', H^{-1}Bvel' (columns = constraint position (i, c), natural row order): extended-precision
    // sums over the entries of the ONE rounded matrix Hq, on purpose.  Every product n_a'H^{-1}n_p the kernel forms is then
    // exactly symmetric in (a, p) -- the QP is solved for a Hessian inverse that differs from the true one by 1 ulp per entry,
    // which is harmless -- whereas columns taken from a more accurate solve L^{-T}(L^{-1}Bpos') disagree with the rounded Hq
    // columns of the bound rows by eps*cond(H) ~ 1e-10: the step refinement then never reaches its residual target and runs
    // all its passes (measured: CFS mode 30 % slower, same answers).
    std::vector<double> &M1n = f.M1n, &M2n = f.M2n;
    M1n.assign((size_t)nn * nn, 0.0); M2n.assign((size_t)nn * nn, 0.0);
    {
        std::vector<long double> a1(nn), a2(nn);
        for (int c = 0; c < nj; ++c)
            for (int i = 0; i < H; ++i) {
                for (int r = 0; r < nn; ++r) {
                    long double s1 = 0.0L, s2 = 0.0L;
                    for (int k = 0; k <= i; ++k) {
                        const long double h = Hq[r + (size_t)(k * nj + c) * nn];
                        s1 += ((long double)(i - k) + 0.5L) * (long double)dt * (long double)dt * h;
                        s2 += (long double)dt * h;
                    }
                    a1[r] = s1; a2[r] = s2;
                }
                const int col = i * nj + c;
                for (int r = 0; r < nn; ++r) { M1n[r + (size_t)col * nn] = (double)a1[r]; M2n[r + (size_t)col * nn] = (double)a2[r]; }
            }
    }

    // rigorous upper bounds of lambda_max(H) and of lambda_max(G), G = D'HD/dt^2 (D = first difference along the waypoints, so
    // that u = D s/dt for s = Bvel u), H = the QP Hessian (QQ symmetrised | I): the early infeasibility test of the fused kernel
    double lmax_vel = 0.0, lmax_H = 1.0;
    {
        const std::vector<double> &Hs = mode == CFS_MODE_CFS ? sym : Hq;   // Hq is the identity for PSGCFS
        std::vector<double> G;
        auto Dt = [&](std::vector<double> &M, bool left) {     // M <- D'M (left) or M D (right): row/col k minus row/col k+nj
            for (int o = 0; o < nn; ++o)
                for (int k = 0; k + nj < nn; ++k) {
                    if (left) M[k + (size_t)o * nn] -= M[(k + nj) + (size_t)o * nn];
                    else M[o + (size_t)k * nn] -= M[o + (size_t)(k + nj) * nn];
                }
        };
        G = Hs; Dt(G, true); Dt(G, false);
        for (auto &v : G) v /= (double)(dt * dt);
        lmax_vel = lambda_max_upper(nn, G);
        if (mode == CFS_MODE_CFS) lmax_H = lambda_max_upper(nn, Hs);   // not 1/alpha: alpha is the caller's PSGCFS step
    }
    f.lmax_vel = lmax_vel; f.lmax_H = lmax_H;
    return FamilyRefusal{};
}

void family_from_weights(int nj, int H, double dt, const cfs_cost_weights *w, bool want_alpha, WeightFamily &f)
{
    const int ns = 2 * nj, nn = H * nj, nx = H * ns;
    // Q = [Qp qc*I; qc*I Qv] (main_FANUC.m:65-77), Qaug = blkdiag(Q*w_stage, ..., Q*w_terminal) (:81-84)
    std::vector<double> Q((size_t)ns * ns, 0.0);
    std::vector<double> &Qaug = f.Qaug, &QQ = f.QQ;
    Qaug.assign((size_t)nx * nx, 0.0);
    for (int c = 0; c < nj; ++c)
        for (int r = 0; r < nj; ++r) {
            Q[r + (size_t)c * ns] = w->Qp[r + c * nj];
            Q[(nj + r) + (size_t)(nj + c) * ns] = w->Qv[r + c * nj];
            if (r == c) { Q[r + (size_t)(nj + c) * ns] = w->q_cross; Q[(nj + r) + (size_t)c * ns] = w->q_cross; }
        }
    for (int i = 0; i < H; ++i) {
        const double wi = i == H - 1 ? w->w_terminal : w->w_stage;
        for (int c = 0; c < ns; ++c)
            for (int r = 0; r < ns; ++r) Qaug[(i * ns + r) + (size_t)(i * ns + c) * nx] = Q[r + (size_t)c * ns] * wi;
    }
    // T = Qaug*Baug (block rows), QQ = Baug'*T + cR*(R + R')  (:96-97); Baug(i,k) = [((i-k)+1/2) dt^2 I; dt I] for k <= i
    std::vector<double> T((size_t)nx * nn, 0.0);
    QQ.assign((size_t)nn * nn, 0.0);
    for (int k = 0; k < H; ++k)
        for (int c = 0; c < nj; ++c) {
            const int col = k * nj + c;
            for (int i = k; i < H; ++i) {
                const double bp = ((double)(i - k) + 0.5) * dt * dt, bv = dt;
                for (int r = 0; r < ns; ++r)
                    T[(i * ns + r) + (size_t)col * nx] = Qaug[(i * ns + r) + (size_t)(i * ns + c) * nx] * bp + Qaug[(i * ns + r) + (size_t)(i * ns + nj + c) * nx] * bv;
            }
        }
    for (int col = 0; col < nn; ++col)
        for (int k = 0; k < H; ++k)
            for (int c = 0; c < nj; ++c) {
                double sacc = 0.0;
                for (int i = k; i < H; ++i)
                    sacc += (((double)(i - k) + 0.5) * dt * dt) * T[(i * ns + c) + (size_t)col * nx] + dt * T[(i * ns + nj + c) + (size_t)col * nx];
                QQ[(k * nj + c) + (size_t)col * nn] = sacc;
            }
    memset(f.Rs, 0, sizeof f.Rs);
    for (int c = 0; c < nj; ++c)
        for (int r = 0; r < nj; ++r) f.Rs[r + c * nj] = (w->Rblk[r + c * nj] + w->Rblk[c + r * nj]) * w->cR;
    for (int i = 0; i < H; ++i)
        for (int c = 0; c < nj; ++c)
            for (int r = 0; r < nj; ++r) QQ[(i * nj + r) + (size_t)(i * nj + c) * nn] += f.Rs[r + c * nj];
    f.alpha = 0.0;
    if (want_alpha) {   // alpha = 1/max(svd(QQ))  (main_FANUC.m:120)
        f.alpha = 1.0 / sym_lambda_max(nn, symmetrise(nn, QQ.data()));
    }
}

void state_cost_terms(int nj, int H, double dt, const double *Qaug, std::vector<double> &F1, std::vector<double> &F2, std::vector<double> &Cq)
{
    const int ns = 2 * nj, nn = H * nj, nx = H * ns;
    // E = [Aaug(:,1:nj), -G] (nx x 2nj): state error per unit of x0 / xg;  QE = Qaug*E;  F = Baug'*QE;  Cq = E'*QE
    std::vector<long double> E((size_t)nx * 2 * nj, 0.0L), QE((size_t)nx * 2 * nj, 0.0L);
    for (int i = 0; i < H; ++i)
        for (int c = 0; c < nj; ++c) {
            E[(i * ns + c) + (size_t)c * nx] = 1.0L;                      // A^i(1:nj,1:nj) = I  (x0 has zero velocity)
            E[(i * ns + c) + (size_t)(nj + c) * nx] = -1.0L;              // -gaug
        }
    for (int col = 0; col < 2 * nj; ++col)
        for (int r = 0; r < nx; ++r) {
            long double s = 0.0L;
            for (int k = 0; k < nx; ++k) s += (long double)Qaug[r + (size_t)k * nx] * E[k + (size_t)col * nx];
            QE[r + (size_t)col * nx] = s;
        }
    F1.assign((size_t)nn * nj, 0.0); F2.assign((size_t)nn * nj, 0.0); Cq.assign((size_t)4 * nj * nj, 0.0);
    for (int col = 0; col < 2 * nj; ++col) {
        for (int k = 0; k < H; ++k)
            for (int c = 0; c < nj; ++c) {                              // row (k,c) of Baug': sum over waypoints i >= k
                long double s = 0.0L;
                for (int i = k; i < H; ++i)
                    s += ((long double)(i - k) + 0.5L) * dt * dt * QE[(i * ns + c) + (size_t)col * nx] + (long double)dt * QE[(i * ns + nj + c) + (size_t)col * nx];
                if (col < nj) F1[(k * nj + c) + (size_t)col * nn] = (double)s;
                else F2[(k * nj + c) + (size_t)(col - nj) * nn] = (double)(-s);   // ff = F1*x0 - F2*xg
            }
        for (int r = 0; r < 2 * nj; ++r) {
            long double s = 0.0L;
            for (int k = 0; k < nx; ++k) s += E[k + (size_t)r * nx] * QE[k + (size_t)col * nx];
            Cq[r + (size_t)col * 2 * nj] = (double)s;
        }
    }
}

// [R | t] -> [R' | -R't] in double: the kernels map link ends into the frame each mesh is stored in.  Only a rigid motion keeps
// the distances (and with them every bound, pruning radius and near-tie margin) of the stored mesh valid.
FamilyRefusal invert_mesh_poses(int nmesh, int H, const double *poses, std::vector<double> &inv)
{
    const size_t n = (size_t)nmesh * H;
    inv.assign(n * 12, 0.0);
    for (size_t e = 0; e < n; ++e) {
        const double *T = poses + e * 12;
        const int jm = (int)(e / H), wp = (int)(e % H);
        for (int q = 0; q < 12; ++q)
            if (!std::isfinite(T[q])) return refuse(CFS_ERR_INVALID_ARG, "pose of mesh %d at waypoint %d is not finite", jm, wp + 1);
        double dev = 0.0;
        for (int r = 0; r < 3; ++r)
            for (int c = 0; c < 3; ++c) {
                const double g = T[4 * r] * T[4 * c] + T[4 * r + 1] * T[4 * c + 1] + T[4 * r + 2] * T[4 * c + 2];
                dev = std::max(dev, std::fabs(g - (r == c ? 1.0 : 0.0)));
            }
        const double det = T[0] * (T[5] * T[10] - T[6] * T[9]) - T[1] * (T[4] * T[10] - T[6] * T[8]) + T[2] * (T[4] * T[9] - T[5] * T[8]);
        if (dev > 1e-9 || !(det > 0.0))
            return refuse(CFS_ERR_INVALID_ARG, "pose of mesh %d at waypoint %d is not a rigid motion (max|RR' - I| = %.3g, det R = %.3g)",
                          jm, wp + 1, dev, det);
        double *o = inv.data() + e * 12;
        for (int r = 0; r < 3; ++r) {
            for (int c = 0; c < 3; ++c) o[4 * r + c] = T[4 * c + r];
            o[4 * r + 3] = 0.0 - (T[r] * T[3] + T[4 + r] * T[7] + T[8 + r] * T[11]);   // 0 - x: +0 for the identity
        }
    }
    return FamilyRefusal{};
}

void mesh_frame(const double *tri, int nt, double *f)
{
    double r2 = 0.0;
    for (int r = 0; r < 3; ++r) {
        double lo = INFINITY, hi = -INFINITY;
        for (size_t v = 0; v < 3 * (size_t)nt; ++v) { lo = std::min(lo, tri[3 * v + r]); hi = std::max(hi, tri[3 * v + r]); }
        f[r] = (lo + hi) / 2.0;
    }
    for (size_t v = 0; v < 3 * (size_t)nt; ++v) {
        const double x = tri[3 * v] - f[0], y = tri[3 * v + 1] - f[1], z = tri[3 * v + 2] - f[2];
        r2 = std::max(r2, x * x + y * y + z * z);
    }
    f[3] = std::sqrt(r2);
}

// The H interval records (CLEAR_ITV doubles each, cfs_family.h) of one mesh for the audit between the waypoints, in double: T is its
// H x 12 poses, frame = (c_j, r_j).  Interval i joins poses i-1 and i; interval 0 and an interval whose two poses are bitwise equal are
// held.  The first interval that turns by more than a quarter (tr R_rel < 1) is reported in (turn_mesh, turn_wp): the audit refuses it.
void mesh_motion_intervals(const double *T, int H, double dt, const double *frame, double *itv, int jm, int &turn_mesh, int &turn_wp)
{
    for (int i = 0; i < H; ++i) {
        double *q = itv + (size_t)i * CLEAR_ITV;
        const double *T1 = T + (size_t)i * 12, *T0 = T + (size_t)(i > 0 ? i - 1 : 0) * 12;
        for (int r = 0; r < 3; ++r) q[20 + r] = frame[r];
        if (i == 0 || memcmp(T0, T1, 12 * sizeof(double)) == 0) continue;      // held: q[0] = 0, v_mesh = 0
        double Rr[9], c0[3], c1[3];
        for (int r = 0; r < 3; ++r)
            for (int c = 0; c < 3; ++c) Rr[3 * r + c] = T1[4 * r] * T0[4 * c] + T1[4 * r + 1] * T0[4 * c + 1] + T1[4 * r + 2] * T0[4 * c + 2];
        const double tr = Rr[0] + Rr[4] + Rr[8];
        if (tr < 1.0) {
            if (turn_mesh < 0) { turn_mesh = jm; turn_wp = i; }
            continue;
        }
        const double w[3] = {(Rr[7] - Rr[5]) / 2.0, (Rr[2] - Rr[6]) / 2.0, (Rr[3] - Rr[1]) / 2.0};
        const double nw = std::sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2]), theta = std::atan2(nw, (tr - 1.0) / 2.0);
        for (int r = 0; r < 3; ++r) {
            c0[r] = T0[4 * r] * frame[0] + T0[4 * r + 1] * frame[1] + T0[4 * r + 2] * frame[2] + T0[4 * r + 3];
            c1[r] = T1[4 * r] * frame[0] + T1[4 * r + 1] * frame[1] + T1[4 * r + 2] * frame[2] + T1[4 * r + 3];
        }
        const double dx = c1[0] - c0[0], dy = c1[1] - c0[1], dz = c1[2] - c0[2];
        q[0] = 1.0;
        for (int r = 0; r < 3; ++r) {
            q[1 + r] = nw > 0.0 ? w[r] / nw : 0.0;
            for (int c = 0; c < 3; ++c) q[5 + 3 * r + c] = T0[4 * r + c];
            q[14 + r] = c0[r]; q[17 + r] = c1[r];
        }
        q[4] = theta;
        q[23] = (theta * frame[3] + std::sqrt(dx * dx + dy * dy + dz * dz)) / dt;
    }
}
