"""The problems helpers.chaotic_problems sets aside are NOT left unchecked: every outer iteration of every one of them is
compared with ONE iteration of the oracle started from the DEVICE's own previous iterate.

Why this closes the gap.  On a chaotic problem the end-to-end comparison is meaningless -- the oracle itself moves by
> 1e-6 rad under a 1e-12 kick of x_init -- but that amplification builds up over the 5-20 outer iterations.  With the
device's iterate u_{k-1} as the starting point only ONE iteration's amplification is in play, so a solver defect that shows
up at iteration >= 2 (where warm starts, the certificate and the drift projection first run) cannot hide behind the chaos:
u_k(device) must equal oracle_step(u_{k-1}(device)) to 1e-8 of |u_k| (1e-9 at the first iteration) wherever the oracle's own
single step is not itself kinked.  "Kinked" is again decided by the ORACLE alone: its single step moves by more than 1e-9 of |u_k| when u_{k-1} is
kicked by N(0, 1e-12^2) (a min-over-links switch, a clamp of distLinSeg or the near-zero surrogate of
dist_arm_3D_200i_2.m:22-24 crossed inside the finite-difference stencil: amplification > 1e3 in ONE iteration -- these steps
are what makes the problem chaotic, 8-50 % of its iterations).  On a kinked step the device must still be as close to the
oracle as the oracle is to its kicked self (within 1e3 x that move).  Measured (MI355X, round 3): un-kinked steps max 2.7e-9 /
1.3e-9 / 4.7e-9 (config 3 CFS / PSGCFS / config-4 shape), first iterations 5.5e-11 / 0 / 6.8e-10.

The checker is helpers.check_one_step_at_a_time (an index list of problems, optionally forced to the w1 tier).  The u log comes from cfs_debug_log_u (both solvers; the solve itself is unchanged: asserted bit for bit).
"""
import numpy as np
import pytest

from helpers import check_one_step_at_a_time

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("mode", ["CFS", "PSGCFS"])
def test_config3_chaotic_problems_one_step_at_a_time(gpu, O, c3, c3_oracle, mode):
    s, bt = c3
    _, chaotic, _ = c3_oracle(mode)
    check_one_step_at_a_time(gpu, O, s, bt, mode, np.nonzero(chaotic)[0], "config3 chaotic")


def test_config4_chaotic_problems_one_step_at_a_time(gpu, O, c4, c4_oracle):
    s, bt = c4
    _, chaotic, _ = c4_oracle("CFS")
    check_one_step_at_a_time(gpu, O, s, bt, "CFS", np.nonzero(chaotic)[0], "config4 shape chaotic")
