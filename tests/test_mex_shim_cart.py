"""The MATLAB side of Cartesian paths, checked the way tests/test_mex_shim_ik.py checks 'ik' (no MATLAB here): the 'cart_path'
command compiles against the ABI header through the stub mex.h, fills the descriptor the header declares, refuses mesh obstacles
and is dispatched."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _cart_command():
    src = open(os.path.join(ROOT, "matlab", "cfs_mex.cpp")).read()
    m = re.search(r"static void cart_path\(.*?\n}\n", src, re.S)
    assert m
    return src, m.group(0)


def test_gateway_with_the_cart_path_command_is_valid_cpp():
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "tests", "stubs"),
                        "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "matlab", "cfs_mex.cpp")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_cart_path_command_fills_the_descriptor_and_is_dispatched():
    src, body = _cart_command()
    hdr = open(os.path.join(ROOT, "include", "cfs_hip.h")).read()
    assert "int cfs_cart_path(" in hdr and "int cfs_cart_path_device(" in hdr
    fields = re.search(r"typedef struct cfs_cart_desc \{(.*?)\} cfs_cart_desc;", hdr, re.S).group(1)
    for f in ("njoint", "use_axis", "lo", "hi", "weight", "candidates", "steps", "max_iter", "max_joint_step", "tol_pos", "tol_axis", "nobs", "obs",
              "D", "tool", "tool_axis"):
        assert re.search(rf"\b{f}\b", fields), f
        assert re.search(rf"d\.{f}\b", body), f                                        # every field of the descriptor is set
    outs = re.search(r"typedef struct cfs_cart_out \{(.*?)\} cfs_cart_out;", hdr, re.S).group(1)
    for f in ("theta", "status", "path", "selected", "n_ok", "n_done", "clearance"):
        assert re.search(rf"\b{f}\b", outs), f
        assert re.search(rf"o\.{f} =", body), f
    assert "fill_robot(robot, ROBOT.c_str(), nj, d.robot)" in body
    assert re.search(r"check\(cfs_cart_path\(&d, T, mxGetPr\(prhs\[4\]\), state\.empty\(\) \? nullptr : state\.data\(\), mxGetPr\(prhs\[6\]\), "
                     r"use_axis \? mxGetPr\(prhs\[7\]\) : nullptr,\s*mxGetPr\(prhs\[8\]\), &o\)\);", body)
    assert "mesh obstacles are not supported" in body and 'mxGetField(robot, 0, "thetamax")' in body
    assert "selected[t] + 1" in body                                                   # 1-based, like MATLAB's indices
    assert re.search(r'cmd == "cart_path"\) \{\s*cart_path\(nlhs, plhs, nrhs, prhs\);', src)
    assert "cfs_mex('cart_path', obs, robot, ROBOT, start, start_state, target_pos, target_axis, theta_ref, opts)" in src
