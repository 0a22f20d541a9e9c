"""The MATLAB side of Cartesian paths against mesh obstacles, checked the way tests/test_mex_shim_ik_mesh.py checks 'ik_mesh' (no MATLAB
here): the gateway compiles against the ABI header through the stub mex.h; 'cart_path_mesh' fills the descriptor the header declares,
takes mesh handles at the end of the cell as 'ik_mesh' does, calls cfs_cart_path_mesh, is dispatched and documented; 'cart_path' keeps
its refusal and its text."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_gateway_with_the_cart_path_mesh_command_is_valid_cpp():
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "tests", "stubs"),
                        "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "matlab", "cfs_mex.cpp")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_cart_path_mesh_command_calls_the_mesh_entry_and_is_dispatched():
    src = open(os.path.join(ROOT, "matlab", "cfs_mex.cpp")).read()
    m = re.search(r"static void cart_path_mesh\(.*?\n}\n", src, re.S)
    assert m
    body = m.group(0)
    hdr = open(os.path.join(ROOT, "include", "cfs_hip.h")).read()
    assert "int cfs_cart_path_mesh(" in hdr and "int cfs_cart_path_mesh_device(" in hdr and "int cfs_debug_cart_frontier_overflows(" in hdr
    for f in ("njoint", "use_axis", "lo", "hi", "weight", "candidates", "steps", "max_iter", "max_joint_step", "tol_pos", "tol_axis", "nobs", "obs",
              "D", "tool", "tool_axis"):
        assert re.search(rf"d\.{f}\b", body), f                                        # every field of the descriptor is set
    for f in ("theta", "status", "path", "selected", "n_ok", "n_done", "clearance"):
        assert re.search(rf"o\.{f} =", body), f
    assert re.search(r"check\(cfs_cart_path_mesh\(&d, \(int\)meshes\.size\(\), meshes\.data\(\), D_mesh\.data\(\), 0, T, mxGetPr\(prhs\[4\]\), "
                     r"state\.empty\(\) \? nullptr : state\.data\(\),\s*mxGetPr\(prhs\[6\]\), use_axis \? mxGetPr\(prhs\[7\]\) : nullptr, "
                     r"mxGetPr\(prhs\[8\]\), &o\)\);", body)
    assert "meshes.push_back(mesh_of(mh))" in body and "mesh obstacles must come last in the obs cell" in body      # as 'ik_mesh' takes them
    assert "d.nobs = (int)D.size()" in body                                            # the descriptor carries the line obstacles only
    assert "cfs_cart_path(" not in body and "selected[t] + 1" in body
    assert "needs at least one mesh obstacle" in body
    assert re.search(r'cmd == "cart_path_mesh"\) \{\s*cart_path_mesh\(nlhs, plhs, nrhs, prhs\);', src)
    assert "cfs_mex('cart_path_mesh', obs, robot, ROBOT, start, start_state, target_pos, target_axis, theta_ref, opts)" in src
    # 'cart_path' keeps its refusal and its text
    line = re.search(r"static void cart_path\(.*?\n}\n", src, re.S).group(0)
    assert "'cart_path' reads line obstacles only: mesh obstacles are not supported" in line and "cfs_cart_path_mesh" not in line
