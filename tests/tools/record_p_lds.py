"""Developer aid (GPU): writes the recordings tests/test_gpu_p_lds.py compares against -- tests/golden/p_lds_*.npy -- with whatever
library is given (default libcfs_hip.so; a file next to it).  They are recorded with a build whose `w2s` tier keeps the first
columns of P in registers (W2S_FLAGS without -DCFS_P_LDS=1, e.g. tools/build_variant.sh regs "" "" "-DCFS_PR=16 -DCFS_TU=4").
usage: python tests/tools/record_p_lds.py [libname.so] [outdir]"""
import os
import sys

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
import test_gpu_p_lds as T

os.makedirs(OUT, exist_ok=True)
s, bt = workloads.config3(lambda rb, th, ob: pkg.dist_arm(rb, th, ob)[0], B=1024)
got = T.solve_psgcfs(pkg, s, bt.nobs, bt.margin_psg, bt.x_init, bt.xR1, bt.ff, bt.caug, bt.obs, bt.noise)
np.save(os.path.join(OUT, "p_lds_config3_counts.npy"), T.pack_counts(got))
np.save(os.path.join(OUT, "p_lds_config3_every8th.npy"), T.pack_full(got)[::8])
print(f"config3 ({LIBNAME}): status {np.bincount(got.status, minlength=4).tolist()}, total_iter sum {int(got.total_iter.sum())}, max {int(got.total_iter.max())}, "
      f">= 100 steps: {int((got.total_iter >= 100).sum())}")
for name in ("2l_h40", "m16ib_h20"):
    s, margin, *args = T.small_case(pkg, name)
    got = T.solve_psgcfs(pkg, s, len(margin), margin, *args)
    np.save(os.path.join(OUT, f"p_lds_{name}.npy"), T.pack_full(got))
    print(f"{name} ({LIBNAME}): status {got.status.tolist()}, iter_O {got.iter_O.tolist()}, total_iter {got.total_iter.tolist()}")
