"""Developer aid (GPU): writes the recordings tests/test_gpu_lin_decode.py compares against -- tests/golden/lin_decode_*.npy -- with
whatever library is given (default libcfs_hip.so; a file next to it).  They are recorded with a library built from the commit
BEFORE the work-item decode of the linearisation changed (runtime divisions, the five-way range chain).
usage: python tests/tools/record_lin_decode.py [libname.so] [outdir]

`<case>_in.npy` holds the inputs (designed here with the CPU oracle: link positions, per-link distances) and, per problem, how many
(waypoint, obstacle) pairs have two candidate links, how many are on the near-zero surrogate, and how many links have no
candidate at all; `<case>_<mode>_<tier>.npy` the outputs of tests/lin_decode_cases.run."""
import os
import sys
import zlib

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))
import numpy as np

from motionplanning_5d_m_amd import _lib
LIBNAME = next((a for a in sys.argv[1:] if a.endswith(".so")), "libcfs_hip.so")
_lib.LIB_PATH = os.path.join(os.path.dirname(_lib.LIB_PATH), LIBNAME)          # before the first lib() call
OUT = next((a for a in sys.argv[1:] if not a.endswith(".so")), os.path.join(os.path.dirname(HERE), "golden"))
import motionplanning_5d_m_amd as pkg
from motionplanning_5d_m_amd import workloads
from oracle import oracle as O
import lin_decode_cases as L

O.build()


def design(case):
    rid, nj, H, nobs, kw, _ = L.CASES[case]
    moving = kw.get("obstacles") == "per_waypoint"
    s, x0, xg = L.family(pkg, case)
    rng = np.random.default_rng(zlib.crc32(case.encode()))
    x0b, xgb = x0 + rng.uniform(-0.1, 0.1, (L.B, nj)), xg + rng.uniform(-0.1, 0.1, (L.B, nj))
    x_init, xR1, ff, caug = workloads._batch_terms(s, x0b, xgb)
    orobot = O.robotproperty2(rid)
    pos = np.array([[O.arm_pos(orobot, x_init[b].reshape(H, 2 * nj)[i, :nj]) for i in range(H)] for b in range(L.B)])   # (B, H, link, end, xyz)
    if rid == "2L":
        c = np.array([0.3, 0.3, 0.0]) + np.concatenate([rng.uniform(-0.05, 0.05, (L.B, 2)), np.zeros((L.B, 1))], axis=1)
        obs = np.concatenate([c, c], axis=1)[:, None, :]
        obs[0, 0] = np.tile(0.5 * (pos[0, H // 3, 1, 0] + pos[0, H // 3, 1, 1]), 2)        # a point on link 2: the surrogate
    else:
        base = np.asarray(pkg.robotproperty2(rid).base, float).reshape(-1)
        rad, ang, z2 = rng.uniform(0.3, 1.2, (L.B, nobs)), rng.uniform(0.0, 2 * np.pi, (L.B, nobs)), rng.uniform(0.6, 1.5, (L.B, nobs))
        rad[L.B // 2:] = 0.8 + rad[L.B // 2:] / 3                                              # the second half of the batch: obstacles that hang
        cx, cy = base[0] + rad * np.cos(ang), base[1] + rad * np.sin(ang)                    # far out and high, where the lower links never are
        obs = np.stack([cx, cy, np.full_like(cx, 0.001), cx, cy, z2], axis=2)
        obs[L.B // 2:, :, 2], obs[L.B // 2:, :, 5] = 0.9, 0.9 + z2[L.B // 2:]
        mid = 0.5 * (pos[0, H // 3, nj - 2, 0] + pos[0, H // 3, nj - 2, 1])
        obs[0, 0] = np.tile(mid, 2)                                                          # a point on a link: the surrogate
        obs[1, nobs - 1] = np.concatenate([mid - [0.0, 0.0, 0.2], mid + [0.0, 0.0, 0.2]]) + np.tile(pos[1, H // 2, nj - 2, 0] - mid, 2)   # a segment through a link of problem 1
        jt = pos[2, H // 2, nj - 1, 0]                                                       # near the joint two links share
        obs[2, 0] = np.tile(jt + 0.04 * (jt - pos[2, H // 2, nj - 2, 0]) / np.linalg.norm(jt - pos[2, H // 2, nj - 2, 0]) + [0.0, 0.03, 0.0], 2)
    if moving:                                                                               # constant horizontal velocity; the rows above hold at their waypoint
        vel = np.concatenate([rng.uniform(-0.01, 0.01, (L.B, nobs, 2)), np.zeros((L.B, nobs, 1))], axis=2)
        step = np.arange(H)[None, :, None, None] - np.array([H // 3, H // 2, H // 2] + [0] * (L.B - 3))[:, None, None, None]
        obs = obs[:, None] + step * np.tile(vel, (1, 1, 2))[:, None]
    rec = np.zeros(L.B, dtype=L.in_dtype(case))
    rec["x_init"], rec["xR1"], rec["ff"], rec["caug"], rec["obs"] = x_init, xR1, ff, caug, obs
    rec["noise"] = 0.1 * rng.standard_normal((L.B, 12, H * nj))
    for b in range(L.B):
        near = np.zeros(nj, bool)
        for i in range(H):
            for j in range(nobs):
                o = obs[b, i, j] if moving else obs[b, j]
                d = np.array([O.dist_lin_seg(pos[b, i, k, 0], pos[b, i, k, 1], o[:3], o[3:])[0] for k in range(nj)])
                m0 = max(d.min(), 1e-4)
                rec["two_candidates"][b] += (d < m0 + 1e-3).sum() >= 2      # prune_tol is at least 1 mm
                rec["surrogate"][b] += d.min() < 1e-4
                near |= d < m0 + 0.005                                      # ... and below 5 mm (1 mm + 8 x links x 5e-6 rad x the reach)
        rec["idle_links"][b] = nj - near.sum()
    return rec


if __name__ == "__main__":
    os.makedirs(OUT, exist_ok=True)
    for case in L.CASES:
        rec = design(case)
        # what the obstacles are designed for: without these the recordings do not reach the edges of the decode
        assert rec["two_candidates"].sum() > 0, f"{case}: no (waypoint, obstacle) pair with two candidate links"
        assert rec["surrogate"].sum() > 0, f"{case}: no pair on the near-zero surrogate"
        assert rec["idle_links"].sum() > 0, f"{case}: no link without candidates"
        np.save(os.path.join(OUT, f"lin_decode_{case}_in.npy"), rec)
        print(f"{case} ({LIBNAME}): pairs with two candidate links {rec['two_candidates'].tolist()}, on the surrogate {rec['surrogate'].tolist()}, "
              f"links without candidates {rec['idle_links'].tolist()}")
        for mode, tier in L.CASES[case][5]:
            out = L.run(pkg, case, mode, tier, rec)
            assert (out["dist"] < 0).any(), f"{case} {mode} {tier}: the device saw no pair on the surrogate"
            np.save(os.path.join(OUT, f"lin_decode_{case}_{mode}_{tier}.npy"), out)
            print(f"  {mode} {tier}: status {out['status'].tolist()}, iter_O {out['iter_O'].tolist()}, total_iter {out['total_iter'].tolist()}, "
                  f"min dist {out['dist'].min():.3e}, links closest {np.bincount(out['linkid'].ravel(), minlength=7).tolist()}")
