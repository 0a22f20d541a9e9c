"""CPU restatement of the path-timing contract of include/cfs_hip.h ("Path timing"), TEST INFRASTRUCTURE ONLY.

Written from the header's text alone: the caps and the tangential budgets vectorised over the rows of one path, the backward and the
forward pass as two scalar loops, the statuses in the header's order, the selection.  The tool points of the feed cap are an input
(N, 3): the caller takes them from whatever forward kinematics it trusts (ik_reference.Arm on the CPU, cfs_tool_pose on the device).
numpy's +, -, *, / and sqrt on float64 are IEEE operations without contraction, the arithmetic the header prescribes.
"""
import math
from types import SimpleNamespace

import numpy as np

INF = math.inf


def stop_rows(N, stop_every):
    s = np.zeros(N, bool)
    s[0] = s[N - 1] = True
    if stop_every >= 2:
        s[::stop_every] = True
    return s


def terms(q, vmax, amax, feed=INF, points=None, gamma=0.5, stop_every=0):
    """d (N-1, nj), kappa (N, nj), m (N, nj), e (N,) or None, cap (N,), ubar (N-1,) of one path of finite rows"""
    q, vmax, amax = np.asarray(q, float), np.asarray(vmax, float), np.asarray(amax, float)
    N = q.shape[0]
    d = q[1:] - q[:-1]
    ad = np.abs(d)
    m = np.empty_like(q)
    m[0], m[N - 1] = ad[0], ad[N - 2]
    m[1:-1] = np.maximum(ad[:-1], ad[1:])
    kap = np.zeros_like(q)
    kap[1:-1] = d[1:] - d[:-1]
    ak = np.abs(kap)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        t = vmax[None, :] / m
        cap = np.where(m > 0, t * t, INF).min(axis=1)
        cap = np.minimum(cap, np.where(ak > 0, (gamma * amax)[None, :] / ak, INF).min(axis=1))
        e = None
        if feed < INF:
            dp = points[1:] - points[:-1]
            l = np.sqrt((dp[:, 0] * dp[:, 0] + dp[:, 1] * dp[:, 1]) + dp[:, 2] * dp[:, 2])
            e = np.empty(N)
            e[0], e[N - 1] = l[0], l[N - 2]
            e[1:-1] = np.maximum(l[:-1], l[1:])
            t = feed / e
            cap = np.minimum(cap, np.where(e > 0, t * t, INF))
        cap[stop_rows(N, stop_every)] = 0.0
        num = np.where(ak[:-1] > 0, amax[None, :] - ak[:-1] * cap[:-1, None], amax[None, :])
        ub = np.where(ad > 0, num / ad, INF).min(axis=1)
    return SimpleNamespace(d=d, kappa=kap, m=m, e=e, cap=cap, ubar=ub)


def time_path(q, vmax, amax, feed=INF, points=None, gamma=0.5, stop_every=0, state=0):
    """One path: namespace of status, duration, time (N,), sdot (N,), b (N,) and, when the passes ran, the terms() as .terms"""
    q = np.asarray(q, float)
    N = q.shape[0]
    nan = np.full(N, np.nan)
    out = SimpleNamespace(status=0, duration=np.nan, time=nan, sdot=nan.copy(), b=nan.copy(), terms=None)
    if state != 0:
        out.status = 1
        return out
    if not np.isfinite(q).all():
        out.status = 2
        return out
    if (q[1:] == q[:-1]).all(axis=1).any():
        out.status = 4
        return out
    T = terms(q, vmax, amax, feed, points, gamma, stop_every)
    cap, ub = T.cap, T.ubar
    K = np.empty(N)
    K[N - 1] = cap[N - 1]
    for n in range(N - 2, -1, -1):
        K[n] = min(cap[n], K[n + 1] + 2.0 * ub[n])
    b = np.empty(N)
    b[0] = K[0]
    for n in range(N - 1):
        b[n + 1] = min(K[n + 1], b[n] + 2.0 * ub[n])
    out.terms = T
    if ((b[:-1] == 0) & (b[1:] == 0)).any():
        out.status = 3
        return out
    s = np.sqrt(b)
    t = np.empty(N)
    t[0] = 0.0
    for n in range(N - 1):
        t[n + 1] = t[n] + 2.0 / (s[n] + s[n + 1])
    if not np.isfinite(t[N - 1]):
        out.status = 2
        return out
    out.time, out.sdot, out.b, out.duration = t, s, b, t[N - 1]
    return out


def select(duration, status):
    """(selected (G,), group_status (G,)) of duration / status (G, R): first argmin over the status-0 paths"""
    cost = np.where(status == 0, duration, INF)
    sel = np.where((status == 0).any(axis=1), cost.argmin(axis=1), -1).astype(np.int32)
    return sel, (sel < 0).astype(np.int32)


def time_paths(paths, vmax, amax, feed=INF, points=None, gamma=0.5, stop_every=0, state=None):
    """paths (G, R, N, nj), points (G, R, N, 3) | None, state (G, R) | None -> namespace of time, sdot (G, R, N), duration, status
    (G, R), selected, group_status (G,)"""
    paths = np.asarray(paths, float)
    G, R, N, _ = paths.shape
    r = SimpleNamespace(time=np.full((G, R, N), np.nan), sdot=np.full((G, R, N), np.nan), duration=np.full((G, R), np.nan),
                        status=np.zeros((G, R), np.int32))
    for g in range(G):
        for j in range(R):
            o = time_path(paths[g, j], vmax, amax, feed, None if points is None else points[g, j], gamma, stop_every,
                          0 if state is None else int(state[g, j]))
            r.time[g, j], r.sdot[g, j], r.duration[g, j], r.status[g, j] = o.time, o.sdot, o.duration, o.status
    r.selected, r.group_status = select(r.duration, r.status)
    return r


# ---- the properties a timed path has, checked on any (sdot, time) of it: the restatement's or the device's -----------------------
def limit_ratios(q, sdot, vmax, amax, feed=INF, points=None):
    """the largest of |kappa*b_n + d*u_n| / amax over segments and joints, of m*sdot / vmax and of e*sdot / feed over rows, b = sdot^2"""
    T = terms(q, vmax, amax, feed, points)
    b = sdot * sdot
    u = (b[1:] - b[:-1]) / 2.0
    acc = np.abs(T.kappa[:-1] * b[:-1, None] + T.d * u[:, None]) / np.asarray(amax, float)[None, :]
    vel = T.m * sdot[:, None] / np.asarray(vmax, float)[None, :]
    fd = 0.0 if T.e is None else float((T.e * sdot / feed).max())
    return float(acc.max()), float(vel.max()), fd


def slack(q, sdot, vmax, amax, feed=INF, points=None, gamma=0.5, stop_every=0, b=None):
    """per row the smallest relative distance of b_n = sdot_n^2 to cap_n, b_{n-1} + 2*ubar_{n-1} and b_{n+1} + 2*ubar_n (0 where it
    equals one of them): a profile with a row above 0 could be raised there.  b: the exact b_n where the caller has them"""
    T = terms(q, vmax, amax, feed, points, gamma, stop_every)
    b = sdot * sdot if b is None else b
    N = b.shape[0]
    cand = np.full((3, N), INF)
    cand[0] = T.cap
    cand[1, 1:] = b[:-1] + 2.0 * T.ubar
    cand[2, :-1] = b[1:] + 2.0 * T.ubar
    with np.errstate(invalid="ignore", divide="ignore"):
        rel = np.abs(cand - b[None, :]) / np.where(b > 0, b, 1.0)[None, :]
    return np.nanmin(np.where(np.isfinite(cand), rel, INF), axis=0)


def smooth_paths(lim, G, R, N, seed, wave=0.2):
    """(G, R, N, nj) smooth joint curves: a straight move between two configurations inside the middle of the joint ranges plus a
    sine term whose rows differ by at most `wave` rad"""
    lim = np.asarray(lim, float)
    nj = lim.shape[0]
    rng = np.random.default_rng(seed)
    mid, half = 0.5 * (lim[:, 0] + lim[:, 1]), 0.5 * (lim[:, 1] - lim[:, 0]) * 0.5
    a = mid + (2 * rng.random((G, R, 1, nj)) - 1) * half
    z = mid + (2 * rng.random((G, R, 1, nj)) - 1) * half
    s = np.linspace(0.0, 1.0, N)[None, None, :, None]
    cycles = rng.integers(1, 4, (G, R, 1, nj))
    amp = wave * rng.random((G, R, 1, nj)) * (N - 1) / (2 * np.pi * cycles)      # |d/dn| of the sine term <= wave
    amp = np.minimum(amp, 0.3)
    return a + (z - a) * s + amp * np.sin(2 * np.pi * cycles * s + 2 * np.pi * rng.random((G, R, 1, nj)))


# ---- the parity inputs: what the device is compared with, and how far a 1e-12 rad change of every row moves the answer -------------
PARITY = dict(G=3, R=7, N=17, seed=11, vmax=1.0, amax=2.0, feed=0.1, gamma=0.5, kick=1e-12)
_parity_cache = {}


def points_of(arm, paths):
    """tool points (..., 3) of configurations (..., nj) by arm.pose (ik_reference.Arm)"""
    flat = paths.reshape(-1, paths.shape[-1])
    return np.array([arm.pose(th)[0] for th in flat]).reshape(paths.shape[:-1] + (3,))


def parity_case(arm, lim, stop_every=0):
    """(paths, points, {with feed?: (reference, movement, tolerance)}): the reference of the parity paths with and without the feed,
    the largest movement of a time stamp or an sdot when every row is moved by kick * (+-1 per entry), and max(1000 * movement,
    1e-10).  No status may change under the move (asserted here)."""
    key = (arm.robot.name, arm.nj, stop_every)
    if key in _parity_cache:
        return _parity_cache[key]
    P = PARITY
    nj = arm.nj
    paths = smooth_paths(lim, P["G"], P["R"], P["N"], P["seed"])
    sign = np.where(np.random.default_rng(P["seed"] + 1).random(paths.shape) < 0.5, -1.0, 1.0)
    moved = paths + P["kick"] * sign
    pts, pts_moved = points_of(arm, paths), points_of(arm, moved)
    vmax, amax = np.full(nj, P["vmax"]), np.full(nj, P["amax"])
    out = {}
    for with_feed in (False, True):
        feed = P["feed"] if with_feed else INF
        ref = time_paths(paths, vmax, amax, feed, pts, P["gamma"], stop_every)
        per = time_paths(moved, vmax, amax, feed, pts_moved, P["gamma"], stop_every)
        assert (ref.status == per.status).all() and (ref.status == 0).all()
        movement = float(max(np.abs(per.time - ref.time).max(), np.abs(per.sdot - ref.sdot).max()))
        out[with_feed] = (ref, movement, max(1000.0 * movement, 1e-10))
    _parity_cache[key] = (paths, pts, out)
    return _parity_cache[key]
