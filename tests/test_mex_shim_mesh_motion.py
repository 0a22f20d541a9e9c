"""The MATLAB side of moving meshes, checked the way tests/test_mex_shim_rrt_mesh.py checks the gateway (no MATLAB here): the
gateway compiles against the ABI header, make_family reads obs{j}.pose into the row-major nmesh x H x 12 array of
cfs_problem_set_mesh_motion for 'solve' and 'get_con' only, and the commands without a time axis refuse the field."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _src():
    return open(os.path.join(ROOT, "matlab", "cfs_mex.cpp")).read()


def _body(src, name):
    m = re.search(r"static void %s\(.*?\n}\n" % name, src, re.S)
    assert m, name
    return m.group(0)


def test_gateway_with_mesh_poses_is_valid_cpp():
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "tests", "stubs"),
                        "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "matlab", "cfs_mex.cpp")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_make_family_packs_the_poses_and_sets_them_after_the_meshes():
    src = _src()
    hdr = open(os.path.join(ROOT, "include", "cfs_hip.h")).read()
    assert "int cfs_problem_set_mesh_motion(cfs_problem *p, const double *poses);" in hdr
    body = _body(src, "make_family")
    assert 'mxGetField(o, 0, "pose")' in body
    assert "poses[at + 12 * i + 4 * r + c] = pg[c * rows + r]" in body                 # column-major page -> row-major [R | t]
    assert "poses[at + 12 * i] = poses[at + 12 * i + 5] = poses[at + 12 * i + 10] = 1.0" in body     # no pose: held still
    assert "ne != 4 * rows && ne != 4 * rows * H" in body                              # one matrix, or a page per waypoint
    assert "pg[15] == 1.0" in body                                                     # a 4x4 page ends in [0 0 0 1]
    assert "if (!moving) mexErrMsgIdAndTxt" in body                                    # only 'solve' and 'get_con' pass moving = true
    i_meshes = body.index("check(cfs_problem_set_meshes(")
    i_motion = body.index("if (posed) check(cfs_problem_set_mesh_motion(f.p, poses.data()));")
    assert i_meshes < i_motion                                                         # set_meshes resets the motion: order matters


def test_only_solve_and_get_con_place_meshes_per_waypoint():
    src = _src()
    for name in ("solve", "get_con"):
        assert re.search(r"make_family\(f, mode, prhs\[2\], 0, [^;]*, false, true\);", _body(src, name)), name
    assert not re.search(r"make_family\([^;]*true\);", _body(src, "clearance_mesh"))   # static rows: .pose is refused there
    for name in ("rrt", "ik_mesh", "cart_path_mesh"):
        assert 'if (mxGetField(o, 0, "pose")) mexErrMsgIdAndTxt' in _body(src, name), name


def test_readme_describes_the_field():
    txt = open(os.path.join(ROOT, "matlab", "README.md")).read()
    assert "obs{j}.pose" in txt and "3x4xH or 4x4xH" in txt and "cfs_problem_set_mesh_motion" in txt
