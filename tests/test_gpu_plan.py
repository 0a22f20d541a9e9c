"""RRTCFSPlanner and cfs_select_best_device on the MI355X.

1. the selection rule in isolation, on synthetic candidates, against a numpy restatement (bit-identical gathers);
2. select="shortest" is the hand composition grow_device -> shortest route per slot -> ragged builder -> solve_device;
3. select="best" returns candidate `selected` of the real S*K solve, and that candidate is the rule's choice;
4. best is never worse than shortest on the same trees, and solves strictly more slots;
5. plausibility of the kept trajectories (cost band of M200i/test.xlsx, clearance, velocity limits);
6. the SOFTEN policy;
7. rounds, never-found slots and determinism."""
import zlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SEED = 20261015
CLASS_A, SOFT = (0, 1), 4


def rule(route_ok, status, iter_O, cost_all, viol_all, K):
    """include/cfs_hip.h, cfs_select_best_device, restated: (selected, has_solution) per slot."""
    S, MK = route_ok.size // K, cost_all.shape[1]
    sel, has = np.full(S, -1, np.int32), np.zeros(S, np.int32)
    for s in range(S):
        A, B, F = [], [], []
        for k in range(K):
            c = s * K + k
            if not route_ok[c]:
                continue
            F.append(k)
            n = int(iter_O[c]) - 1
            if not 1 <= n <= MK:
                continue
            cost = cost_all[c, n - 1]
            v = viol_all[c, n - 1] if viol_all is not None else 0.0
            if status[c] in CLASS_A and not np.isnan(cost):
                A.append((cost, k))
            elif status[c] == SOFT and not (np.isnan(cost) or np.isnan(v)):
                B.append((v, cost, k))
        if A:
            sel[s], has[s] = min(A)[-1], 1
        elif B:
            sel[s], has[s] = min(B)[-1], 1
        elif F:
            sel[s] = F[0]
    return sel, has


def _np(ns, keys=("u", "x_", "cost_all", "e_cost_all", "e_u_all", "iter_O", "total_iter", "status")):
    return {k: getattr(ns, k).cpu().numpy() for k in keys}


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.tobytes() == b.tobytes()


@pytest.fixture(scope="module")
def problem(gpu):
    return gpu.RRTstar_problem()


@pytest.fixture(scope="module")
def dev():
    import torch
    return torch.device("cuda", 0)


def _pairs(problem, S):
    """RRTstar_CFS.m's start and goal for each of S slots (one shared pair would be one slot)"""
    _, s_r, g, *_ = problem
    return np.tile(s_r.x0, (S, 1)), np.tile(g, (S, 1))


def _planner(gpu, problem, **kw):
    pobs, s, g, region_g, region_s, off = problem
    return gpu.RRTCFSPlanner(pobs, s, region_g, region_s, off, **kw)


# ---- 1. the rule in isolation ---------------------------------------------------------------------------------------------------
def _synthetic(rng, S, K, MK, nn, nx, case):
    SK = S * K
    route_ok = (rng.random(SK) < 0.8).astype(np.int32)
    status = rng.choice([0, 1, 2, 3, 4], SK).astype(np.int32)
    iter_O = rng.integers(2, MK + 2, SK).astype(np.int32)
    cost = rng.choice([1.0, 2.0, 3.0, 2.0], (SK, MK)) * 1e5                   # few distinct values: ties are common
    viol = rng.choice([0.0, 1e-3, 2e-3], (SK, MK))
    if case == "all_A":
        status[:] = rng.choice([0, 1], SK)
        route_ok[:] = 1
    elif case == "ties":
        status[:], route_ok[:], cost[:] = 0, 1, 2.5e5
    elif case == "nan":
        cost[rng.random((SK, MK)) < 0.4] = np.nan
        viol[rng.random((SK, MK)) < 0.3] = np.nan
    elif case == "only_soft":
        status[:] = 4
    elif case == "mixed_234":
        status[:] = rng.choice([2, 3, 4], SK)
    elif case == "no_route":
        route_ok[:] = 0
        route_ok[rng.random(SK) < 0.1] = 1
    elif case == "bad_iter":
        iter_O[:] = rng.choice([0, 1, MK + 1, MK + 2], SK)
    arrs = dict(u=rng.standard_normal((SK, nn)), x_=rng.standard_normal((SK, nx)), cost_all=cost, e_cost_all=rng.random((SK, MK)),
                e_u_all=rng.random((SK, MK)), iter_O=iter_O, total_iter=rng.integers(0, 999, SK).astype(np.int32), status=status)
    return route_ok, arrs, viol


@pytest.mark.parametrize("S,K,case,soft", [
    (12, 6, "all_A", False), (12, 6, "ties", False), (12, 6, "nan", True), (12, 6, "only_soft", True), (12, 6, "mixed_234", True),
    (12, 6, "no_route", True), (12, 6, "bad_iter", True), (37, 1, "random", True), (5, 64, "random", True), (7, 6, "random", True),
    (9, 6, "only_soft", False), (3, 64, "nan", False)])
def test_rule_in_isolation(gpu, problem, dev, S, K, case, soft):
    import torch
    from motionplanning_5d_m_amd.plan import select_best_device
    kw = dict(on_infeasible="soften", soft_weight=1e4) if soft else {}
    pl = _planner(gpu, problem, num_seed=K, max_slots=S, **kw)
    cfs = pl.cfs
    MK, nn, nx = cfs.K, cfs.nn, cfs.nx
    rng = np.random.default_rng(zlib.crc32(repr((S, K, case, soft)).encode()))
    route_ok, arrs, viol = _synthetic(rng, S, K, MK, nn, nx, case)
    t = lambda a: torch.tensor(a, device=dev)  # noqa: E731
    cand = type("O", (), {k: t(v) for k, v in arrs.items()})
    best = cfs.alloc_outputs(S, dev)
    for k in arrs:
        getattr(best, k).fill_(-7)                                                    # rows of a no-route slot stay as they are
    bviol = torch.full((S, MK), -7.0, dtype=torch.float64, device=dev) if soft else None
    sel, has = torch.full((S,), 99, dtype=torch.int32, device=dev), torch.full((S,), 99, dtype=torch.int32, device=dev)
    select_best_device(cfs, S, K, t(route_ok), cand, best, sel, has, t(viol) if soft else None, bviol)
    torch.cuda.synchronize()
    want_sel, want_has = rule(route_ok, arrs["status"], arrs["iter_O"], arrs["cost_all"], viol if soft else None, K)
    got_sel, got_has = sel.cpu().numpy(), has.cpu().numpy()
    np.testing.assert_array_equal(got_sel, want_sel)
    np.testing.assert_array_equal(got_has, want_has)
    got = _np(best)
    for s in range(S):
        for k, a in arrs.items():
            want = a[s * K + want_sel[s]] if want_sel[s] >= 0 else np.full_like(a[0], -7)
            assert _same_bits(got[k][s], want), (case, s, k)
        if soft:
            want = viol[s * K + want_sel[s]] if want_sel[s] >= 0 else np.full(MK, -7.0)
            assert _same_bits(bviol[s].cpu().numpy(), want)
    if case == "ties":
        assert (want_sel == 0).all()
    if case == "no_route":
        assert (want_sel == -1).any()
    pl.close()


def test_select_validates_against_the_handle(gpu, problem, dev):
    import torch
    from motionplanning_5d_m_amd.plan import select_best_device
    pl = _planner(gpu, problem, num_seed=6, max_slots=2, on_infeasible="soften", soft_weight=1e4)
    cand = pl.cfs.alloc_outputs(12, dev)
    best = pl.cfs.alloc_outputs(3, dev)
    i = torch.zeros(12, dtype=torch.int32, device=dev)
    v = torch.zeros(12, pl.cfs.K, dtype=torch.float64, device=dev)
    with pytest.raises(gpu.CfsError) as e:                                                 # S*K = 18 > max_batch = 12
        select_best_device(pl.cfs, 3, 6, i, cand, best, i, i, v, None)
    assert e.value.code == -1 and "max_batch" in str(e.value)
    with pytest.raises(gpu.CfsError) as e:                                                 # SOFTEN needs cand_viol_all
        select_best_device(pl.cfs, 2, 6, i, cand, best, i, i, None, None)
    assert e.value.code == -1
    pl.close()


# ---- 2. shortest = the hand composition -------------------------------------------------------------------------------------------
def test_shortest_is_the_hand_composition(gpu, problem, dev):
    import torch
    pobs, s_r, g, *_ = problem
    S, K, seed = 48, 6, SEED + 2
    pl = _planner(gpu, problem, num_seed=K, max_slots=S, select="shortest")
    r = pl.plan(*_pairs(problem, S), seed)
    torch.cuda.synchronize()
    # by hand (tests/tools/rrt_bench.py's per-slot rule): round 0 of every slot is tree s*K + k of one launch
    x0 = torch.tensor(np.broadcast_to(s_r.x0, (S * K, 5)).copy(), device=dev)
    gg = torch.tensor(np.broadcast_to(g, (S * K, 5)).copy(), device=dev)
    tr = pl.rrt.grow_device(S * K, seed, dev, x0=x0, goal=gg)
    INF = torch.iinfo(torch.int32).max
    ln = torch.where(tr.fail == 0, tr.route_len, torch.full_like(tr.route_len, INF)).view(S, K)
    best_len, kpick = ln.min(dim=1)
    pick = torch.arange(S, device=dev) * K + kpick
    ref = gpu.CFSBatch(pl.sys_cfs, len(pobs), [o["epsilon"] for o in pobs], max_batch=S)
    terms = ref.build_terms_from_ragged_routes_device(tr.route[pick].contiguous(), tr.route_len[pick].contiguous())
    obs = pl._obs[:S].contiguous()
    want = _np(ref.solve_device(*terms, obs))
    torch.cuda.synchronize()
    rounds, sel = r.rounds.cpu().numpy(), r.selected.cpu().numpy()
    one = rounds == 1
    assert one.sum() >= S // 2
    np.testing.assert_array_equal(one, (best_len < INF).cpu().numpy())
    np.testing.assert_array_equal(sel[one], kpick.cpu().numpy()[one])
    got = _np(r)
    for k in want:
        assert _same_bits(got[k][one], want[k][one]), k
    L = tr.route_len[pick].cpu().numpy()
    np.testing.assert_array_equal(r.route_len.cpu().numpy()[one], L[one])
    st = got["status"][one]
    np.testing.assert_array_equal(r.has_solution.cpu().numpy()[one], np.isin(st, CLASS_A).astype(np.int32))
    ref.close()
    pl.close()


# ---- 3-5. best on RRTstar_problem, S = 256, K = 6, STOP ------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ab256(gpu, problem):
    import torch
    pobs, s_r, g, *_ = problem
    out = {}
    for sel in ("best", "shortest"):
        pl = _planner(gpu, problem, num_seed=6, max_slots=256, select=sel)
        out[sel] = pl.plan(*_pairs(problem, 256), SEED, want_candidates=True)
        torch.cuda.synchronize()
        pl.close()
    return out


def test_best_returns_the_rules_candidate(ab256):
    r = ab256["best"]
    c = r.candidates
    K = 6
    cand = _np(c)
    ok = c.route_ok.cpu().numpy()
    want_sel, want_has = rule(ok, cand["status"], cand["iter_O"], cand["cost_all"], None, K)
    sel = r.selected.cpu().numpy()
    np.testing.assert_array_equal(sel, want_sel)
    np.testing.assert_array_equal(r.has_solution.cpu().numpy(), want_has)
    got = _np(r)
    for s in np.nonzero(sel >= 0)[0]:
        for k in got:
            assert _same_bits(got[k][s], cand[k][s * K + sel[s]]), (s, k)
    assert (sel >= 0).all()                                    # 50 rounds of 6 seeds: every slot finds a route


def test_best_is_never_worse_than_shortest(ab256):
    b, s = ab256["best"], ab256["shortest"]
    K = 6
    np.testing.assert_array_equal(b.rounds.cpu().numpy(), s.rounds.cpu().numpy())   # the same trees
    cand = _np(b.candidates)
    sh = _np(s)
    ks = s.selected.cpu().numpy()
    rows = np.arange(ks.size) * K + ks
    for k in sh:                                               # a problem's result does not depend on its batch position
        assert _same_bits(sh[k], cand[k][rows]), k
    s_ok = np.isin(sh["status"], CLASS_A)
    bst = b.status.cpu().numpy()
    b_ok = np.isin(bst, CLASS_A)
    assert b_ok[s_ok].all()
    bc, sc = b.cost.cpu().numpy(), s.cost.cpu().numpy()
    assert (bc[s_ok] <= sc[s_ok]).all()
    print(f"[plan S=256 K=6 STOP] solved (status 0/1): shortest {s_ok.mean():.3f}, best {b_ok.mean():.3f}")
    assert b_ok.mean() > s_ok.mean()


def test_best_is_plausible(gpu, ab256, problem):
    b = ab256["best"]
    pobs = problem[0]
    st, cost, x = b.status.cpu().numpy(), b.cost.cpu().numpy(), b.x_.cpu().numpy()
    ok = st == 0
    assert ok.sum() >= 10
    med = float(np.median(cost[ok]))
    print(f"[plan S=256] status-0 slots {ok.sum()}, median final cost {med:.4g}")
    assert 1.5e5 <= med <= 4e5                                 # M200i/test.xlsx rows 5-19
    from motionplanning_5d_m_amd.solvers import obs_to_array
    th = x[ok].reshape(-1, 40, 10)
    d, _ = gpu.dist_arm(gpu.robotproperty2("M200i"), th[:, :, :5].reshape(-1, 5), obs_to_array(pobs))
    margin = np.array([o["epsilon"] for o in pobs])
    assert (d >= margin[None] - 2e-2).all(), float((d - margin[None]).min())
    assert np.abs(th[:, :, 5:]).max() <= 1.0 + 1e-6            # lim = ones(5)


# ---- 6. SOFTEN ------------------------------------------------------------------------------------------------------------------
def test_soften(gpu, problem):
    import torch
    pobs, s_r, g, *_ = problem
    S, K = 64, 6
    pl = _planner(gpu, problem, num_seed=K, max_slots=S, on_infeasible="soften", soft_weight=1e4)
    r = pl.plan(*_pairs(problem, S), SEED + 6, want_candidates=True)
    torch.cuda.synchronize()
    st, sel = r.status.cpu().numpy(), r.selected.cpu().numpy()
    found = sel >= 0
    assert found.all()
    assert np.isin(st[found], (0, 1, 4)).all(), np.bincount(st[found] + 1)
    cst = r.candidates.status.cpu().numpy().reshape(S, K)
    cok = r.candidates.route_ok.cpu().numpy().reshape(S, K) != 0
    anyA = (np.isin(cst, CLASS_A) & cok).any(axis=1)
    assert not (anyA & (st == 4)).any()
    np.testing.assert_array_equal(r.has_solution.cpu().numpy(), np.isin(st, (0, 1, 4)).astype(np.int32))
    cv = r.candidates.viol_all.cpu().numpy()
    bv = r.viol_all.cpu().numpy()
    for s in range(S):
        assert _same_bits(bv[s], cv[s * K + sel[s]])
    want_sel, _ = rule(cok.reshape(-1).astype(np.int32), r.candidates.status.cpu().numpy(), r.candidates.iter_O.cpu().numpy(),
                       r.candidates.cost_all.cpu().numpy(), cv, K)
    np.testing.assert_array_equal(sel, want_sel)
    print(f"[plan S=64 SOFTEN 1e4] status 0/1 {np.isin(st, CLASS_A).mean():.3f}, 0/1/4 {np.isin(st, (0, 1, 4)).mean():.3f}")
    pl.close()


# ---- 7. rounds, never-found slots, determinism -------------------------------------------------------------------------------------
def test_rounds_regrow_only_open_slots(gpu, problem, dev):
    import torch
    from motionplanning_5d_m_amd.plan import ROUND_SEED_STRIDE
    pobs, s_r, g, *_ = problem
    S, seed = 16, SEED + 7
    pl = _planner(gpu, problem, num_seed=1, max_slots=S)
    r = pl.plan(*_pairs(problem, S), seed)
    torch.cuda.synchronize()
    rounds, sel = r.rounds.cpu().numpy(), r.selected.cpu().numpy()
    assert (rounds >= 2).any() and (sel == 0).all()
    x0 = torch.tensor(np.broadcast_to(s_r.x0, (S, 5)).copy(), device=dev)
    gg = torch.tensor(np.broadcast_to(g, (S, 5)).copy(), device=dev)
    t0 = pl.rrt.grow_device(S, seed, dev, x0=x0, goal=gg)
    f0 = t0.fail.cpu().numpy()
    np.testing.assert_array_equal(rounds >= 2, f0 != 0)                 # exactly the slots whose round-0 seed failed
    open1 = np.nonzero(f0 != 0)[0]
    t1 = pl.rrt.grow_device(open1.size, seed + ROUND_SEED_STRIDE, dev, x0=x0[:open1.size].contiguous(), goal=gg[:open1.size].contiguous())
    f1 = t1.fail.cpu().numpy()
    two = open1[f1 == 0]                                                # done in round 2: the compacted launch's trees
    assert (rounds[two] == 2).all()
    L = t1.route_len.cpu().numpy()[f1 == 0]
    np.testing.assert_array_equal(r.route_len.cpu().numpy()[two], L)
    got, want = r.route.cpu().numpy()[two], t1.route.cpu().numpy()[f1 == 0]
    for i in range(two.size):
        assert _same_bits(got[i, :L[i]], want[i, :L[i]])
    pl.close()


def test_never_found_and_determinism(gpu, problem):
    import torch
    pobs, s_r, g, *_ = problem
    pl = _planner(gpu, problem, num_seed=6, max_slots=8)
    r = pl.plan(*_pairs(problem, 8), SEED, max_rounds=2, max_draws=1)        # every tree runs out of uniforms at once
    torch.cuda.synchronize()
    assert (r.selected.cpu().numpy() == -1).all() and (r.rounds.cpu().numpy() == 2).all()
    assert (r.has_solution.cpu().numpy() == 0).all() and (r.status.cpu().numpy() == -1).all()
    assert (r.route_len.cpu().numpy() == 0).all() and np.isnan(r.cost.cpu().numpy()).all()
    x0 = np.tile(s_r.x0, (8, 1)) + 0.01 * np.arange(8)[:, None]
    a = pl.plan(x0, g, SEED + 3)
    b = pl.plan(x0, g, SEED + 3)
    torch.cuda.synchronize()
    for k in ("u", "x_", "cost_all", "e_cost_all", "e_u_all", "iter_O", "total_iter", "status", "selected", "has_solution",
              "route", "route_len", "rounds", "cost"):
        assert _same_bits(getattr(a, k).cpu().numpy(), getattr(b, k).cpu().numpy()), k
    pl.close()
