"""Makes tests/golden/reference_maps.tar.xz: the reference's three binary STL maps and the transformed map it stores, as DATA.

    python tests/golden/make_reference_maps.py <reference checkout>

Members, bit for bit as the reference holds them:
  assembly line_Assem1.STL, material_traveller.STL, table.STL   map/*.STL (27 396 / 12 620 / 2 156 triangles, millimetres)
  environment_v.npy                                             map/environment.mat:envir.v (82 188 x 3 float64, mm): the
                                                                reference's own MapFromSTL.m output for the assembly line
The other fields of environment.mat (faces, normals, colours) are not used by any test and are left out.  The archive is
written reproducibly (sorted members, zero mtimes and owners), so re-running the script gives the same bytes.
"""
import io
import os
import sys
import tarfile

import numpy as np
import scipy.io

STLS = ("assembly line_Assem1.STL", "material_traveller.STL", "table.STL")


def main(ref):
    members = {name: open(os.path.join(ref, "map", name), "rb").read() for name in STLS}
    env = scipy.io.loadmat(os.path.join(ref, "map", "environment.mat"))["envir"]["v"][0, 0]
    buf = io.BytesIO()
    np.save(buf, np.ascontiguousarray(env, dtype=np.float64))
    members["environment_v.npy"] = buf.getvalue()
    out = os.path.join(os.path.dirname(os.path.abspath(__file__)), "reference_maps.tar.xz")
    with tarfile.open(out, "w:xz", preset=9, format=tarfile.GNU_FORMAT) as tf:
        for name in sorted(members):
            info = tarfile.TarInfo(name)
            info.size, info.mtime, info.mode = len(members[name]), 0, 0o644
            tf.addfile(info, io.BytesIO(members[name]))
    print(out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main(sys.argv[1])
