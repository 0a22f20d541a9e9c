"""The MATLAB side of inverse kinematics, checked the way tests/test_mex_shim.py checks the gateway (no MATLAB here): the 'ik'
command compiles against the ABI header through the stub mex.h, fills the descriptor the header declares, refuses mesh obstacles
and is dispatched."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _ik_command():
    src = open(os.path.join(ROOT, "matlab", "cfs_mex.cpp")).read()
    m = re.search(r"static void ik\(.*?\n}\n", src, re.S)
    assert m
    return src, m.group(0)


def test_gateway_with_the_ik_command_is_valid_cpp():
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "tests", "stubs"),
                        "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "matlab", "cfs_mex.cpp")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_ik_command_fills_the_descriptor_and_is_dispatched():
    src, body = _ik_command()
    hdr = open(os.path.join(ROOT, "include", "cfs_hip.h")).read()
    assert "int cfs_ik_solve(" in hdr and "int cfs_ik_solve_device(" in hdr and "int cfs_tool_pose(" in hdr
    fields = re.search(r"typedef struct cfs_ik_desc \{(.*?)\} cfs_ik_desc;", hdr, re.S).group(1)
    for f in ("njoint", "use_axis", "lo", "hi", "weight", "restarts", "max_iter", "tol_pos", "tol_axis", "nobs", "obs", "D", "seed", "tool", "tool_axis"):
        assert re.search(rf"\b{f}\b", fields), f
        assert re.search(rf"d\.{f}\b", body), f                                        # every field of the descriptor is set
    assert "fill_robot(robot, ROBOT.c_str(), nj, d.robot)" in body
    assert re.search(r"check\(cfs_ik_solve\(&d, T, mxGetPr\(prhs\[4\]\), use_axis \? mxGetPr\(prhs\[5\]\) : nullptr, mxGetPr\(prhs\[6\]\), &o\)\);", body)
    assert "mesh obstacles are not supported" in body and 'mxGetField(robot, 0, "thetamax")' in body
    assert "selected[t] + 1" in body                                                   # 1-based, like MATLAB's indices
    assert re.search(r'cmd == "ik"\) \{\s*ik\(nlhs, plhs, nrhs, prhs\);', src)
    assert "cfs_mex('ik', obs, robot, ROBOT, target_pos, target_axis, theta_ref, opts)" in src   # documented in the header comment
