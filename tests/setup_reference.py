"""Plain np.longdouble references of the kernels that prepare a batch and evaluate its cost (TEST INFRASTRUCTURE ONLY): the batched
product and cost (cfs_get_cost, cfs_cost_b, the cost history of a CFS solve), the terms builder (line reference, cubic route
resampling, ff, caug, xR1), the dense constraint writer and the launch-order pre-pass.  Written from include/cfs_hip.h and the
kernels' comments; every function restates one operation with no tiling, no batching tricks and no shared code with the product.
The bounds that go with them (gamma, the componentwise absolute sums) are here too, so that the CPU test of this file and the GPU
tests use the same ones."""
import numpy as np

LD = np.longdouble
EPS = float(np.finfo(np.float64).eps)          # 2^-52; one rounding is at most EPS/2 relative


def ld(a):
    return np.asarray(a, dtype=LD)


def gamma(m):
    """Higham's gamma_m with unit roundoff EPS: the relative bound of m stacked fp64 roundings, taken generously (EPS, not EPS/2)"""
    return m * EPS / (1.0 - m * EPS)


# ---- cost -----------------------------------------------------------------------------------------------------------------------
def gemv_cost(QQ, u, ff, caug):
    """get_cost(u) = 0.5 u'QQ u + ff'u + caug (Lib/EVAL.m:51-53) for u (B, nn), ff (B, nn), caug (B,): longdouble (B,)"""
    QQ, u, ff, caug = ld(QQ), np.atleast_2d(ld(u)), np.atleast_2d(ld(ff)), ld(caug).reshape(-1)
    qu = u @ QQ.T                                # row b = QQ u_b
    return LD(0.5) * (u * qu).sum(axis=1) + (ff * u).sum(axis=1) + caug


def gemv_cost_abs(QQ, u, ff, caug):
    """0.5 |u|'|QQ||u| + |ff|'|u| + |caug|: what the rounding of get_cost scales with"""
    QQ, u, ff, caug = np.abs(ld(QQ)), np.abs(np.atleast_2d(ld(u))), np.abs(np.atleast_2d(ld(ff))), np.abs(ld(caug).reshape(-1))
    return LD(0.5) * (u * (u @ QQ.T)).sum(axis=1) + (ff * u).sum(axis=1) + caug


def solve_ld(Hs, rhs):
    """Hs x = rhs in longdouble for a symmetric positive definite Hs (Cholesky, plain loops over columns); rhs (nn,) or (nn, B)"""
    A, n = ld(Hs).copy(), Hs.shape[0]
    L = np.zeros((n, n), LD)
    for j in range(n):
        d = A[j, j] - (L[j, :j] * L[j, :j]).sum()
        assert d > 0
        L[j, j] = np.sqrt(d)
        L[j + 1:, j] = (A[j + 1:, j] - L[j + 1:, :j] @ L[j, :j]) / L[j, j]
    x = ld(rhs).copy()
    for j in range(n):
        x[j] = (x[j] - L[j, :j] @ x[:j]) / L[j, j]
    for j in range(n - 1, -1, -1):
        x[j] = (x[j] - L[j + 1:, j] @ x[j + 1:]) / L[j, j]
    return x


# ---- terms builder ----------------------------------------------------------------------------------------------------------------
def line_terms(x0, xg, H):
    """main_FANUC.m:38-49: (x_init (H, 2nj), xR1 (2nj,)): waypoint n = 1..H of linspace(x0, xg, H+1), the last one xg itself, zero
    velocities; xR1 = [x0; 0]"""
    x0, xg = ld(x0), ld(xg)
    nj = x0.size
    x = np.zeros((H, 2 * nj), LD)
    for i in range(H):
        x[i, :nj] = xg if i == H - 1 else x0 + LD(i + 1) * (xg - x0) / LD(H)
    return x, np.concatenate([x0, np.zeros(nj, LD)])


def route_position(n, nwp, H):
    """sample n of linspace(0, (nwp-1) dt, H+1) in units of dt, exactly: (segment k, numerator of tau over H).  At a knot tau is 0
    (1 only at the route's end)."""
    num = n * (nwp - 1)
    k = min(num // H, nwp - 2)
    return k, num - k * H


def route_terms(route, nwp, dt, H):
    """RRTstar_CFS.m:94-100: cubicpolytraj(route, (0:nwp-1) dt, linspace(0, (nwp-1) dt, H+1)) with zero waypoint velocities, sample 0
    dropped.  route: (>= nwp, nj), rows from nwp on are not read.  Returns (x_init (H, 2nj), xR1 (2nj,), seg (H, nj)): seg is the
    largest |r_k+1 - r_k| over the segments that may be named for the sample (two at a knot, where the value is the knot itself
    whichever is named).  nwp = 1: the node at every waypoint.  dt cancels: the sample times are exact multiples of dt / H."""
    del dt
    r = ld(route)
    nj = r.shape[1]
    x, seg = np.zeros((H, 2 * nj), LD), np.zeros((H, nj), LD)
    xR1 = np.concatenate([r[0], np.zeros(nj, LD)])
    if nwp < 2:
        x[:, :nj] = r[0]
        return x, xR1, seg
    for i in range(H):
        k, num = route_position(i + 1, nwp, H)
        tau = LD(num) / LD(H)
        x[i, :nj] = r[k] + (3 * tau * tau - 2 * tau * tau * tau) * (r[k + 1] - r[k])
        seg[i] = np.abs(r[k + 1] - r[k])
        if num == 0 and k > 0:
            seg[i] = np.maximum(seg[i], np.abs(r[k] - r[k - 1]))
        if num == H and k + 2 < nwp:
            seg[i] = np.maximum(seg[i], np.abs(r[k + 2] - r[k + 1]))
    return x, xR1, seg


def cost_terms_ld(Aaug, Baug, Qaug, xR1, xg):
    """main_FANUC.m:98-103 for one problem: ff = Baug' Qaug (Aaug xR1 - gaug), caug = (Aaug xR1 - gaug)' Qaug (Aaug xR1 - gaug),
    gaug = kron(ones(H, 1), [xg; 0]); and the componentwise absolute sums S = |Baug'| |Qaug| (|Aaug| |xR1| + |gaug|) (nn,) and
    Sc = (|Aaug| |xR1| + |gaug|)' |Qaug| (|Aaug| |xR1| + |gaug|).  Returns (ff, caug, S, Sc)."""
    A, Bm, Q, x1, xg = ld(Aaug), ld(Baug), ld(Qaug), ld(xR1), ld(xg)
    nj = xg.size
    H = A.shape[0] // (2 * nj)
    gaug = np.tile(np.concatenate([xg, np.zeros(nj, LD)]), H)
    e = A @ x1 - gaug
    a = np.abs(A) @ np.abs(x1) + np.abs(gaug)
    Qe, Qa = Q @ e, np.abs(Q) @ a
    return Bm.T @ Qe, e @ Qe, np.abs(Bm).T @ Qa, a @ Qa


# ---- dense constraint writer ---------------------------------------------------------------------------------------------------------
def dense_con(dist, grad, margin, lim, plim, xR1, u, dt, H, nj, nobs):
    """self.Ainq / self.binq of one problem from its linearisation, in the row order of Lib/CFS_FANUC.m:119-129: for obstacle j, for
    waypoint i: the collision row [-Diff' Bpos_i | (d - margin_j) - Diff' Bpos_i u], then nj rows [Bvel_i | lim - v0], then nj rows
    [-Bvel_i | lim + v0]; Bpos_i = [(i - k + 1/2) dt^2 I for k <= i], Bvel_i = [dt I for k <= i].  plim = (lo, hi) appends H nj rows
    [Bpos (i, c) | hi_c - theta0_c - (i+1) dt v0_c], then H nj rows [-Bpos (i, c) | theta0_c + (i+1) dt v0_c - lo_c].
    dist (nobs, H), grad (nobs, H, nj).  Returns (A (rows, nn), b (rows,), babs (rows,)): babs is the sum of the absolute values of
    the terms of b."""
    dist, grad, margin, lim, x1, u, dt = ld(dist), ld(grad), ld(margin), ld(lim), ld(xR1), ld(u), LD(dt)
    nn, per = H * nj, 1 + 2 * nj
    rref = nobs * H * per
    rows = rref + (0 if plim is None else 2 * nn)
    A, b, babs = np.zeros((rows, nn), LD), np.zeros(rows, LD), np.zeros(rows, LD)
    v0 = x1[nj:]
    for j in range(nobs):
        for i in range(H):
            r = (j * H + i) * per
            for k in range(i + 1):
                coef = (LD(i - k) + LD(0.5)) * dt * dt
                A[r, k * nj:(k + 1) * nj] = -grad[j, i] * coef
                for c in range(nj):
                    A[r + 1 + c, k * nj + c] = dt
                    A[r + 1 + nj + c, k * nj + c] = -dt
            b[r] = (dist[j, i] - margin[j]) + A[r] @ u
            babs[r] = abs(dist[j, i]) + abs(margin[j]) + np.abs(A[r]) @ np.abs(u)
            b[r + 1:r + 1 + nj], b[r + 1 + nj:r + per] = lim - v0, lim + v0
            babs[r + 1:r + 1 + nj] = babs[r + 1 + nj:r + per] = np.abs(lim) + np.abs(v0)
    if plim is not None:
        lo, hi = ld(plim[0]), ld(plim[1])
        for i in range(H):
            pos = x1[:nj] + LD(i + 1) * dt * v0
            pabs = np.abs(x1[:nj]) + np.abs(LD(i + 1) * dt * v0)
            for c in range(nj):
                q = rref + i * nj + c
                for k in range(i + 1):
                    coef = (LD(i - k) + LD(0.5)) * dt * dt
                    A[q, k * nj + c], A[q + nn, k * nj + c] = coef, -coef
                b[q], b[q + nn] = hi[c] - pos[c], pos[c] - lo[c]
                babs[q], babs[q + nn] = np.abs(hi[c]) + pabs[c], np.abs(lo[c]) + pabs[c]
    return A, b, babs


# ---- launch-order pre-pass ---------------------------------------------------------------------------------------------------------
def order_keys(dists, margin):
    """key[b] = number of (waypoint, line obstacle) pairs with distance below the obstacle's margin; dists (B, H, nline)"""
    return (np.asarray(dists) < np.asarray(margin)[None, None, :]).sum(axis=(1, 2)).astype(np.int32)


def stable_rank(keys):
    """the problems by descending key, ties by index"""
    keys = [int(k) for k in keys]
    return np.array(sorted(range(len(keys)), key=lambda b: (-keys[b], b)), dtype=np.int32)
