"""The MATLAB side of inverse kinematics against mesh obstacles, checked the way tests/test_mex_shim_ik.py checks 'ik' (no MATLAB
here): the gateway compiles against the ABI header through the stub mex.h; 'ik_mesh' takes mesh handles at the end of the cell as
'rrt' does, calls cfs_ik_solve_mesh, is dispatched and documented."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_gateway_with_the_ik_mesh_command_is_valid_cpp():
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "tests", "stubs"),
                        "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "matlab", "cfs_mex.cpp")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_ik_mesh_command_calls_the_mesh_entry_and_is_dispatched():
    src = open(os.path.join(ROOT, "matlab", "cfs_mex.cpp")).read()
    m = re.search(r"static void ik_mesh\(.*?\n}\n", src, re.S)
    assert m
    body = m.group(0)
    hdr = open(os.path.join(ROOT, "include", "cfs_hip.h")).read()
    assert "int cfs_ik_solve_mesh(" in hdr and "int cfs_ik_solve_mesh_device(" in hdr and "int cfs_debug_ik_frontier_overflows(" in hdr
    for f in ("njoint", "use_axis", "lo", "hi", "weight", "restarts", "max_iter", "tol_pos", "tol_axis", "nobs", "obs", "D", "seed", "tool", "tool_axis"):
        assert re.search(rf"d\.{f}\b", body), f                                        # every field of the descriptor is set
    assert re.search(r"check\(cfs_ik_solve_mesh\(&d, \(int\)meshes\.size\(\), meshes\.data\(\), D_mesh\.data\(\), 0, T,", body)
    assert "meshes.push_back(mesh_of(mh))" in body and "mesh obstacles must come last in the obs cell" in body      # as 'rrt' takes them
    assert "cfs_ik_solve(" not in body and "selected[t] + 1" in body
    assert re.search(r'cmd == "ik_mesh"\) \{\s*ik_mesh\(nlhs, plhs, nrhs, prhs\);', src)
    assert "cfs_mex('ik_mesh', obs, robot, ROBOT, target_pos, target_axis, theta_ref, opts)" in src   # documented in the header comment
    # 'ik' keeps its refusal
    ik = re.search(r"static void ik\(.*?\n}\n", src, re.S).group(0)
    assert "mesh obstacles are not supported" in ik and "cfs_ik_solve_mesh" not in ik
