"""CPU restatement of the tool-path audit of include/cfs_hip.h ("Tool-path audit"), TEST INFRASTRUCTURE ONLY.

Written from the header's text alone, without the device's shortcuts: every segment has its own S+1 samples (row n+1 is met twice, as
sample S of segment n and as sample 0 of segment n+1, and is not merged), the configuration of a sample is q_n + (k/S) d_n for k < S
and row n+1 itself for k = S.  The clearance is the oracle's dist_arm (near-zero surrogate, first-minimum link) through
clearance_reference._dist_all, the tool point is ik_reference.Arm.pose, rho is clearance_reference.rho_matrix and rt is restated here.
Also the property checkers that the CPU and the GPU suite both run, on the restatement's outputs and on the device's.
"""
import math
from types import SimpleNamespace

import numpy as np

import clearance_reference as CR
from oracle import oracle as O

INF = math.inf
FLOATS = ("clear_rows", "clear_path", "s_path", "clear_lower", "chord_err", "chord_upper")
INTS = ("link_path", "obs_path", "status", "state_out")


def rt_vector(robot, nj, tool):
    """rt[m] = sum_{j=m..nj-1} len_j + |tool|, len_j the translation of link j as rho_matrix takes it"""
    ln = [float(np.sqrt((robot.T[:, j + 1] ** 2).sum())) if robot.name == "2L" else math.hypot(robot.DH[j, 2], robot.DH[j, 1]) for j in range(nj)]
    return np.array([sum(ln[m:]) for m in range(nj)]) + float(np.linalg.norm(tool))


def segment_bounds(robot, nj, tool, q):
    """L_n and A_n of every segment of the path q (N, nj)"""
    rho, rt = CR.rho_matrix(robot, nj), rt_vector(robot, nj, tool)
    ad = np.abs(q[1:] - q[:-1])
    L = np.array([max(float(a[:k + 1] @ rho[:k + 1, k]) for k in range(nj)) for a in ad])
    mx = np.maximum.outer(np.arange(nj), np.arange(nj))
    A = np.array([float((np.outer(a, a) * rt[mx]).sum()) for a in ad])
    return L, A


def samples(q, S):
    """configurations (N-1, S+1, nj) and fractions (S+1,) of the samples of path q"""
    N, nj = q.shape
    sig = np.arange(S + 1) / S
    TH = np.empty((N - 1, S + 1, nj))
    for n in range(N - 1):
        d = q[n + 1] - q[n]
        for k in range(S):
            TH[n, k] = q[n] + sig[k] * d
        TH[n, S] = q[n + 1]
    return TH, sig


def measure(arm, q, obs, D, S):
    """clearance c (N-1, S+1), its obstacle and link, the chord deviation e (N-1, S+1) and the least raw distance dmin (N-1, S+1)
    at every sample of path q"""
    N, nj = q.shape
    TH, sig = samples(q, S)
    flat = TH.reshape(-1, nj)
    nobs = len(D)
    if nobs:
        d, lk = CR._dist_all(O, arm.robot, flat, np.broadcast_to(np.asarray(obs, float), (flat.shape[0], nobs, 6)))
        m = d - np.asarray(D, float)[None, :]
        ob = m.argmin(axis=1)                                 # first minimum over the obstacles
        c, lk, dmin = m.min(axis=1), lk[np.arange(flat.shape[0]), ob], d.min(axis=1)
    else:
        c, ob, lk, dmin = np.full(flat.shape[0], INF), np.full(flat.shape[0], -1), np.full(flat.shape[0], -1), np.full(flat.shape[0], INF)
    p = np.array([arm.pose(th)[0] for th in flat]).reshape(N - 1, S + 1, 3)
    pa, pb = p[:, :1], p[:, -1:]
    chordpt = (1.0 - sig)[None, :, None] * pa + sig[None, :, None] * pb
    e = np.sqrt(((p - chordpt) ** 2).sum(axis=2))
    return c.reshape(N - 1, S + 1), ob.reshape(N - 1, S + 1), lk.reshape(N - 1, S + 1), e, dmin.reshape(N - 1, S + 1)


def audit_path(arm, q, obs, D, S, state=0, min_clearance=-INF, max_chord=INF):
    """One path: the header's outputs, and for the tests gap (how far above the minimum the lowest sample at ANOTHER path parameter
    is), L_max and A_max"""
    q = np.asarray(q, float)
    N, nj = q.shape
    out = SimpleNamespace(**{k: np.nan for k in FLOATS}, link_path=-1, obs_path=-1, status=0, state_out=int(state), gap=np.nan, L_max=np.nan,
                          A_max=np.nan)
    if state != 0:
        out.status = 1
        return out
    if not np.isfinite(q).all():
        out.status, out.state_out = 2, 3
        return out
    c, ob, lk, e, _ = measure(arm, q, obs, D, S)
    L, A = segment_bounds(arm.robot, nj, arm.tool, q)
    out.clear_rows = float(min(c[:, 0].min(), c[-1, S]))
    flat = c.reshape(-1)
    first = int(flat.argmin())                                # lowest n, then lowest k
    n, k = divmod(first, S + 1)
    out.clear_path, out.s_path = float(flat[first]), n + k / S
    out.link_path, out.obs_path = int(lk[n, k]), int(ob[n, k])
    s_all = (np.arange(N - 1)[:, None] + np.arange(S + 1)[None, :] / S).reshape(-1)
    other = flat[s_all != out.s_path]
    out.gap = float(other.min() - flat[first]) if other.size and flat[first] < INF else INF
    out.clear_lower = float(((c[:, :-1] + c[:, 1:]) / 2.0 - (L / (2.0 * S))[:, None]).min())
    out.chord_err = float(e.max())
    out.chord_upper = float((np.maximum(e[:, :-1], e[:, 1:]) + (A / (8.0 * S * S))[:, None]).max())
    out.L_max, out.A_max = float(L.max()), float(A.max())
    if out.clear_lower < min_clearance:
        out.state_out = 6
    elif out.chord_upper > max_chord:
        out.state_out = 7
    return out


def audit_paths(arm, paths, obs, D, S, state=None, min_clearance=-INF, max_chord=INF, idx=None):
    """paths (P, N, nj), state (P,) | None -> namespace of (len(idx),) arrays (idx: the paths to audit, default all)"""
    idx = range(len(paths)) if idx is None else idx
    rs = [audit_path(arm, paths[i], obs, D, S, 0 if state is None else int(state[i]), min_clearance, max_chord) for i in idx]
    return SimpleNamespace(**{k: np.array([getattr(r, k) for r in rs]) for k in FLOATS + INTS + ("gap", "L_max", "A_max")})


def dense(arm, q, obs, D, S, factor=16):
    """(the least clearance, the largest chord deviation, the least raw distance) on a grid `factor` times as dense: the stand-in for
    continuous sigma in the soundness tests.  The chord deviation refers to the segment's own end points, so it is the same quantity."""
    c, _, _, e, dmin = measure(arm, np.asarray(q, float), obs, D, S * factor)
    return float(c.min()), float(e.max()), float(dmin.min())


# ---- the properties an audited path has, checked on any outputs of it: the restatement's or the device's -------------------------
def check_conventions(r, state, finite_rows):
    """status, the NaN / -1 rows and what of state_out does not depend on the thresholds.  r: arrays of one shape; state: the input
    state or None; finite_rows: bool array, the path has finite rows only"""
    state = np.zeros(r.status.shape, np.int32) if state is None else np.asarray(state)
    want = np.where(state != 0, 1, np.where(finite_rows, 0, 2))
    np.testing.assert_array_equal(r.status, want)
    off = want != 0
    for k in FLOATS:
        v = getattr(r, k)
        assert np.isnan(v[off]).all(), k
        assert not np.isnan(v[~off]).any(), k
    assert (r.link_path[off] == -1).all() and (r.obs_path[off] == -1).all()
    np.testing.assert_array_equal(r.state_out[state != 0], state[state != 0])
    assert (r.state_out[want == 2] == 3).all()
    assert np.isin(r.state_out[want == 0], (0, 6, 7)).all()


def check_state_out(r, min_clearance=-INF, max_chord=INF):
    """state_out of the audited paths from the path's own bounds, in the header's order"""
    ok = r.status == 0
    want = np.where(r.clear_lower[ok] < min_clearance, 6, np.where(r.chord_upper[ok] > max_chord, 7, 0))
    np.testing.assert_array_equal(r.state_out[ok], want)


def check_path(robot, nj, tool, q, S, nobs, r, eps=1e-12):
    """one audited path's outputs r (scalars) against each other and against L_n, A_n of its rows"""
    N = q.shape[0]
    L, A = segment_bounds(robot, nj, tool, q)
    assert r.clear_path <= r.clear_rows
    assert 0.0 <= r.s_path <= N - 1 and abs(r.s_path * S - round(r.s_path * S)) <= 1e-9
    if nobs:
        assert 1 <= r.link_path <= nj and 0 <= r.obs_path < nobs
        assert r.clear_path - r.clear_lower <= L.max() / (2.0 * S) + eps
    else:
        assert r.clear_rows == INF and r.clear_path == INF and r.clear_lower == INF
        assert r.s_path == 0.0 and r.link_path == -1 and r.obs_path == -1
    assert 0.0 <= r.chord_err <= r.chord_upper
    assert r.chord_upper - r.chord_err <= A.max() / (8.0 * S * S) + eps
    if S == 1:                                                # e = 0 at the rows: the bound is the interpolation remainder alone
        assert r.chord_err == 0.0 and abs(r.chord_upper - A.max() / 8.0) <= eps


def check_sound(arm, q, obs, D, S, r, eps=1e-12):
    """the two guarantees against a 16 times denser sampling of the same motion"""
    cmin, emax, dmin = dense(arm, q, obs, D, S)
    if r.clear_lower > 0:
        assert cmin >= r.clear_lower - eps, (cmin, r.clear_lower)
    if len(D) and dmin >= 1e-4:
        assert r.clear_lower <= cmin + eps, (cmin, r.clear_lower)   # no surrogate on the way: the distance is Lipschitz with L_n
    assert r.chord_upper >= emax - eps, (emax, r.chord_upper)
    return cmin, emax


def pick(r, i):
    """the scalars of path i of a namespace of arrays"""
    return SimpleNamespace(**{k: (v.reshape(-1)[i] if isinstance(v, np.ndarray) else v) for k, v in vars(r).items()})


# ---- inputs ---------------------------------------------------------------------------------------------------------------------------
def post_scene(arm, q0=0.2, step=0.3, half=0.05, D=0.01):
    """the fixed scene: rows q_0 = q0*1 and q_0 + step*e_1, a vertical post of +-half through the tool point at sigma = 0.5"""
    a = np.full(arm.nj, q0)
    b = a.copy()
    b[0] += step
    mid = arm.pose(a + 0.5 * (b - a))[0]
    obs = np.concatenate([mid - [0, 0, half], mid + [0, 0, half]])[None, :]
    return np.stack([a, b]), obs, np.array([D])


def two_obstacles(arm, lim):
    """two line obstacles near the tool points of the middle of the joint ranges: close enough to the parity paths to matter"""
    mid = 0.5 * (np.asarray(lim, float)[:, 0] + np.asarray(lim, float)[:, 1])
    p = arm.pose(mid)[0]
    r = max(float(np.linalg.norm(p - arm.base)), 0.2)
    a = np.concatenate([p + r * np.array([0.35, -0.5, -0.2]), p + r * np.array([0.35, 0.5, 0.3])])
    b = np.concatenate([p + r * np.array([-0.6, 0.4, 0.5]), p + r * np.array([-0.4, 0.5, -0.5])])
    return np.stack([a, b]), np.array([0.02, 0.03])


# ---- the parity inputs: what the device is compared with, and how far a 1e-12 rad change of every row moves the answer -------------
PARITY = dict(G=3, R=7, N=17, S=4, seed=23, kick=1e-12)
_parity_cache = {}


def smooth_paths(lim, G, R, N, seed, wave=0.2):
    import path_time_reference as PT
    return PT.smooth_paths(lim, G, R, N, seed, wave)


def parity_inputs(lim, G, R, N, seed):
    """paths (G, R, N, nj) in path_time_reference.smooth_paths' style, state (G, R) with every fifth path not to be audited, and one
    NaN row (path 1, where the batch has that many)"""
    paths = smooth_paths(lim, G, R, N, seed)
    state = np.zeros(G * R, np.int32)
    state[4::5] = 3
    if G * R >= 2:
        paths.reshape(G * R, N, -1)[1, N // 2, -1] = np.nan
    return paths, state.reshape(G, R)


def _separating(values, fallback):
    """a threshold no value lies within a factor 2 of: the geometric middle of the widest gap (in ratio) between neighbouring positive
    values when that gap is wider than a factor 4.5, else `fallback`"""
    v = np.sort(values[values > 0])
    if v.size >= 2:
        ratio = v[1:] / v[:-1]
        i = int(ratio.argmax())
        if ratio[i] > 4.5:
            return float(math.sqrt(v[i] * v[i + 1]))
    return fallback(v)


def parity_case(arm, lim):
    """(paths, state, obs, D, min_clearance, max_chord, reference, movement per float output, tolerance per float output) of the parity
    paths.  The thresholds are chosen on the restatement alone so that every state_out decision is robust: min_clearance inside the
    widest gap of the positive clear_lower values (else a quarter of the least: every positive bound passes), max_chord inside the
    widest gap of the chord_upper values of the paths that pass it (else four times the largest: all pass).  The movement is the
    largest change of an output when every row is moved by kick * (+-1 per entry), the tolerance max(1000 * movement, 1e-10).  No
    integer output may change under the move (asserted here)."""
    key = (arm.robot.name, arm.nj)
    if key in _parity_cache:
        return _parity_cache[key]
    P = PARITY
    paths, state = parity_inputs(lim, P["G"], P["R"], P["N"], P["seed"])
    obs, D = two_obstacles(arm, lim)
    flat, st = paths.reshape(-1, P["N"], arm.nj), state.reshape(-1)
    sign = np.where(np.random.default_rng(P["seed"] + 1).random(flat.shape) < 0.5, -1.0, 1.0)
    free = audit_paths(arm, flat, obs, D, P["S"], st)
    ok = free.status == 0
    min_clearance = _separating(free.clear_lower[ok], lambda v: float(v[0]) / 4.0 if v.size else 1e-3)
    passing = ok & ~(free.clear_lower < min_clearance)
    max_chord = _separating(free.chord_upper[passing], lambda v: float(v[-1]) * 4.0 if v.size else 1.0)
    ref = audit_paths(arm, flat, obs, D, P["S"], st, min_clearance, max_chord)
    per = audit_paths(arm, flat + P["kick"] * sign, obs, D, P["S"], st, min_clearance, max_chord)
    for k in INTS:
        np.testing.assert_array_equal(getattr(ref, k), getattr(per, k), err_msg=k)
    movement = {k: float(np.abs(getattr(per, k)[ok] - getattr(ref, k)[ok]).max()) for k in FLOATS}
    tol = {k: max(1000.0 * v, 1e-10) for k, v in movement.items()}
    _parity_cache[key] = (paths, state, obs, D, min_clearance, max_chord, ref, movement, tol)
    return _parity_cache[key]
