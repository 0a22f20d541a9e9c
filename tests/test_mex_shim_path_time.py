"""The MATLAB side of path timing, checked the way tests/test_mex_shim_cart_follow.py checks its verbs (no MATLAB here): the gateway
compiles against the ABI header through the stub mex.h; 'path_time' is dispatched to one function that reads the shape of the 4-D
paths from dims, fills cfs_time_desc from the arguments and the options and calls cfs_path_time; the verb is documented."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _src():
    return open(os.path.join(ROOT, "matlab", "cfs_mex.cpp")).read()


def _body(src, name):
    m = re.search(rf"static void {name}\(.*?\n}}\n", src, re.S)
    assert m
    return m.group(0)


def test_gateway_with_the_path_time_command_is_valid_cpp():
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "tests", "stubs"),
                        "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "matlab", "cfs_mex.cpp")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_the_verb_is_dispatched_and_fills_the_descriptor():
    src = _src()
    hdr = open(os.path.join(ROOT, "include", "cfs_hip.h")).read()
    assert "int cfs_path_time(" in hdr
    assert re.search(r'cmd == "path_time"\) \{\s*path_time\(nlhs, plhs, nrhs, prhs\);', src)
    body = _body(src, "path_time")
    assert src.count("cfs_time_desc d;") == 1 and "cfs_time_desc d;" in body
    # paths is njoint x N x R x G: its shape comes from dims, and the element count is checked against it
    assert "N = (int)mxGetPr(prhs[4])[0], R = (int)mxGetPr(prhs[4])[1], G = (int)mxGetPr(prhs[4])[2]" in body
    assert "mxGetNumberOfElements(prhs[3]) != (size_t)nj * N * R * G" in body
    # dims is checked as doubles (whole, in range; a NaN fails the comparison) in front of the casts, njoint before the robot's capsule is read
    check, cast, cap = body.index("v != std::floor(v)"), body.index("N = (int)mxGetPr(prhs[4])[0]"), body.index("d.robot.cap + 6 * (nj - 1)")
    assert "!(v >= 1.0 && v <= 1e6)" in body and check < cast < body.index("nj < 2 || nj > 6") < cap
    assert "(int)mxGetNumberOfElements(prhs[5]) != R * G" in body and "state.empty() ? nullptr : state.data()" in body
    assert "(int)mxGetNumberOfElements(prhs[6]) != nj || (int)mxGetNumberOfElements(prhs[7]) != nj" in body
    for field in ("d.njoint = nj", "d.vmax = mxGetPr(prhs[6])", "d.amax = mxGetPr(prhs[7])", 'd.feed = num("feed", HUGE_VAL)',
                  'd.curve_share = num("curve_share", 0.5)', 'd.stop_every = (int)num("stop_every", 0)', "fill_robot(robot, ROBOT.c_str(), nj, d.robot)"):
        assert field in body, field
    assert re.search(r"check\(cfs_path_time\(&d, G, R, N, mxGetPr\(prhs\[3\]\), state\.empty\(\) \? nullptr : state\.data\(\), &o\)\);", body)
    # G x R x N row-major is N x (R*G) column-major; selected goes out 1-based
    assert "mxCreateDoubleMatrix(N, np, mxREAL)" in body and "mxCreateDoubleMatrix(R, G, mxREAL)" in body and "selected[g] + 1" in body
    for k in ("o.time", "o.sdot", "o.duration", "o.status", "o.selected", "o.group_status"):
        assert k + " = " in body, k


def test_the_verb_is_documented():
    src = _src()
    assert "cfs_mex('path_time', robot, ROBOT, paths, dims, state, vmax, amax, opts)" in src
    readme = open(os.path.join(ROOT, "matlab", "README.md")).read()
    assert "'path_time'" in readme and "njoint x N x R x G" in readme and "reshape(time, N, R, G)" in readme
