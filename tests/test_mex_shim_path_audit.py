"""The MATLAB side of the tool-path audit, checked the way tests/test_mex_shim_path_time.py checks its verb (no MATLAB here): the
gateway compiles against the ABI header through the stub mex.h; 'path_audit' is dispatched to one function that reads the shape of the
4-D paths from dims, the obs cell as 'ik' reads it, fills cfs_audit_desc from the arguments and the options and calls cfs_path_audit;
the verb is documented."""
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


def test_gateway_with_the_path_audit_command_is_valid_cpp():
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "tests", "stubs"),
                        "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "matlab", "cfs_mex.cpp")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_the_verb_is_dispatched_and_fills_the_descriptor():
    src = _src()
    hdr = open(os.path.join(ROOT, "include", "cfs_hip.h")).read()
    assert "int cfs_path_audit(" in hdr
    assert re.search(r'cmd == "path_audit"\) \{\s*path_audit\(nlhs, plhs, nrhs, prhs\);', src)
    body = _body(src, "path_audit")
    assert src.count("cfs_audit_desc d;") == 1 and "cfs_audit_desc d;" in body
    # paths is njoint x N x R x G: its shape comes from dims, and the element count is checked against it
    assert "N = (int)mxGetPr(prhs[5])[0], R = (int)mxGetPr(prhs[5])[1], G = (int)mxGetPr(prhs[5])[2]" in body
    assert "mxGetNumberOfElements(prhs[4]) != (size_t)nj * N * R * G" in body
    # dims is checked as doubles (whole, in range; a NaN fails the comparison) in front of the casts, njoint before the robot's capsule is read
    check, cast, cap = body.index("v != std::floor(v)"), body.index("N = (int)mxGetPr(prhs[5])[0]"), body.index("d.robot.cap + 6 * (nj - 1)")
    assert "!(v >= 1.0 && v <= 1e6)" in body and check < cast < body.index("nj < 2 || nj > 6") < cap
    assert "(int)mxGetNumberOfElements(prhs[6]) != R * G" in body and "state.empty() ? nullptr : state.data()" in body
    # line obstacles only, and no pointer to an empty list
    assert 'mxGetField(o, 0, "mesh")' in body and "meshes are not audited" in body
    assert "d.obs = d.nobs ? obs6.data() : nullptr" in body and "d.D = d.nobs ? D.data() : nullptr" in body
    for field in ("d.njoint = nj", 'd.substeps = (int)num("substeps", 8)', 'd.min_clearance = num("min_clearance", -HUGE_VAL)',
                  'd.max_chord = num("max_chord", HUGE_VAL)', "fill_robot(robot, ROBOT.c_str(), nj, d.robot)"):
        assert field in body, field
    assert re.search(r"check\(cfs_path_audit\(&d, G, R, N, mxGetPr\(prhs\[4\]\), state\.empty\(\) \? nullptr : state\.data\(\), &o\)\);", body)
    # G x R row-major is R x G column-major; the obstacle goes out 1-based
    assert "mxCreateDoubleMatrix(R, G, mxREAL)" in body and "ob[e] + 1" in body
    for k in ("clear_rows", "clear_path", "s_path", "clear_lower", "chord_err", "chord_upper", "link_path", "obs_path", "status", "state_out"):
        assert f"o.{k} = " in body, k


def test_the_verb_is_documented():
    src = _src()
    assert "cfs_mex('path_audit', obs, robot, ROBOT, paths, dims, state, opts)" in src
    readme = open(os.path.join(ROOT, "matlab", "README.md")).read()
    assert "'path_audit'" in readme and "njoint x N x R x G" in readme and "state_out" in readme
