"""Problem shapes for GPU tests that force the fused solver's w1 tier (debug_options(tier_w1=True)): test_tier_query.py proves on
the CPU that each of them runs a half-CU tier by default, so that forcing w1 there really changes the kernel; test_gpu_tiers.py
asserts that the handles it builds have exactly these shapes.  Data only."""

# tag -> (nj, H, nobs, solvers run)
BATCH_SHAPES = {
    "s96": (5, 16, 2, ("CFS", "PSGCFS")),       # nn = 80: the 96-row kernels
    "s160": (5, 30, 3, ("CFS", "PSGCFS")),      # nn = 150: the 160-row kernels (config 3 with 3 obstacles)
    "s256": (5, 40, 2, ("CFS",)),               # nn = 200: the 256-row kernels (config 4's shape)
}

# single problems on the other instantiations: (robot, nj, H) -> nj * 1000 + rows of the kernel; one obstacle each
SINGLE_SHAPES = {
    ("M200i", 3, 24): 3096,
    ("M200i", 3, 40): 3160,
    ("M200i", 4, 40): 4160,
    ("M200i", 6, 20): 6160,
    ("2L", 2, 40): 2096,
    ("M200i", 6, 40): 6256,
}

# nj 5, H 30 (config 3's shape, nn = 150, the 160-row kernels): the smallest obstacle count at which the shape no longer fits half a
# CU, per solver -- solved on w1 with no debug flag (found with the query and pinned by test_tier_query.py)
DEFAULT_W1_NJ_H = (5, 30)
DEFAULT_W1_NOBS = {"CFS": 25, "PSGCFS": 13}


def instantiation(nj, H):
    nn = nj * H
    return nj * 1000 + (96 if nn <= 96 else (160 if nn <= 160 else 256))
