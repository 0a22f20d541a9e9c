"""The MATLAB side of tool paths, checked the way tests/test_mex_shim_cart.py checks 'cart_path' (no MATLAB here): the gateway
compiles against the ABI header through the stub mex.h; 'cart_follow' and 'cart_follow_mesh' are dispatched to the functions of
'cart_path' and 'cart_path_mesh' -- one parsing of the arguments for each pair of verbs, not a copy --, which call cfs_cart_follow /
cfs_cart_follow_mesh with the number of poses read off path_pos; the verbs are documented."""
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


def test_gateway_with_the_cart_follow_commands_is_valid_cpp():
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "tests", "stubs"),
                        "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "matlab", "cfs_mex.cpp")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_the_two_verbs_share_the_parsing_of_cart_path_and_are_dispatched():
    src = _src()
    hdr = open(os.path.join(ROOT, "include", "cfs_hip.h")).read()
    assert "int cfs_cart_follow(" in hdr and "int cfs_cart_follow_mesh(" in hdr
    # dispatched to the existing functions with the flag: no third and fourth copy of the parsing
    assert re.search(r'cmd == "cart_follow"\) \{\s*cart_path\(nlhs, plhs, nrhs, prhs, true\);', src)
    assert re.search(r'cmd == "cart_follow_mesh"\) \{\s*cart_path_mesh\(nlhs, plhs, nrhs, prhs, true\);', src)
    assert "static void cart_follow" not in src and src.count("cfs_cart_desc d;") == 2
    line, mesh = _body(src, "cart_path"), _body(src, "cart_path_mesh")
    for body in (line, mesh):
        assert "bool follow = false)" in body.split("\n")[0]
        # T is theta_ref's, M = the poses of path_pos; both tables are checked against M*T
        assert "T = (int)mxGetN(follow ? prhs[8] : prhs[6])" in body and "M = T > 0 ? (int)(mxGetN(prhs[6]) / T) : 0" in body
        assert "(int)mxGetN(prhs[6]) != M * T" in body and "(int)mxGetN(prhs[7]) != M * T" in body and "follow && M < 2" in body
        assert "(M - 1) * d.steps > 256" in body
        assert "rows = (follow ? (M - 1) * d.steps : d.steps) + 1" in body and "mxCreateDoubleMatrix(nj, (size_t)rows * T, mxREAL)" in body
    assert re.search(r"if \(follow\)\s*check\(cfs_cart_follow\(&d, T, M, mxGetPr\(prhs\[4\]\), state\.empty\(\) \? nullptr : state\.data\(\), "
                     r"mxGetPr\(prhs\[6\]\),\s*use_axis \? mxGetPr\(prhs\[7\]\) : nullptr, mxGetPr\(prhs\[8\]\), &o\)\);\s*else\s*check\(cfs_cart_path\(", line)
    assert re.search(r"if \(follow\)\s*check\(cfs_cart_follow_mesh\(&d, \(int\)meshes\.size\(\), meshes\.data\(\), D_mesh\.data\(\), 0, T, M, "
                     r"mxGetPr\(prhs\[4\]\),\s*state\.empty\(\) \? nullptr : state\.data\(\), mxGetPr\(prhs\[6\]\), use_axis \? mxGetPr\(prhs\[7\]\) : nullptr,\s*"
                     r"mxGetPr\(prhs\[8\]\), &o\)\);\s*else\s*check\(cfs_cart_path_mesh\(", mesh)
    assert "cfs_cart_follow_mesh" not in line and "cfs_cart_follow(" not in mesh
    assert "'cart_follow' reads line obstacles only" in line and "'cart_follow_mesh' needs at least one mesh obstacle" in mesh
    assert "a moving mesh needs a time axis" in mesh                                   # a mesh entry with a pose stays refused


def test_the_verbs_are_documented():
    src = _src()
    assert "cfs_mex('cart_follow', obs, robot, ROBOT, start, start_state, path_pos, path_axis, theta_ref, opts)" in src
    assert "cfs_mex('cart_follow_mesh', obs, robot, ROBOT, start, start_state, path_pos, path_axis, theta_ref, opts)" in src
    readme = open(os.path.join(ROOT, "matlab", "README.md")).read()
    assert "'cart_follow'" in readme and "'cart_follow_mesh'" in readme and "(M-1)*steps + 1" in readme
