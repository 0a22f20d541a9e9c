"""The MATLAB side of RRT in a cell with mesh obstacles, checked the way tests/test_mex_shim.py checks the gateway (no MATLAB
here): the 'rrt' command compiles against the ABI header, routes an obs cell with mesh handles to cfs_rrt_grow_mesh and one without
to cfs_rrt_grow, refuses a mesh before a line obstacle, and the classdef passes its cell through untouched."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _rrt_command():
    src = open(os.path.join(ROOT, "matlab", "cfs_mex.cpp")).read()
    m = re.search(r"static void rrt\(.*?\n}\n", src, re.S)
    assert m
    return src, m.group(0)


def test_gateway_with_the_mesh_rrt_command_is_valid_cpp():
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "tests", "stubs"),
                        "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "matlab", "cfs_mex.cpp")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_rrt_command_routes_mesh_cells_to_the_mesh_entry():
    src, body = _rrt_command()
    hdr = open(os.path.join(ROOT, "include", "cfs_hip.h")).read()
    assert "cfs_rrt_grow_mesh(" in hdr and "cfs_rrt_grow_mesh_device(" in hdr
    assert re.search(r"if \(meshes\.empty\(\)\) check\(cfs_rrt_grow\(&d, S, &o\)\);", body)
    assert re.search(r"check\(cfs_rrt_grow_mesh\(&d, \(int\)meshes\.size\(\), meshes\.data\(\), D_mesh\.data\(\), 0, S, &o\)\);", body)
    assert 'mxGetField(o, 0, "mesh")' in body and "mesh_of(mh)" in body               # handles arrive as for 'clearance_mesh'
    assert "mesh obstacles must come last in the obs cell" in body
    assert "d.nobs = (int)D.size()" in body                                            # the descriptor carries the line obstacles only


def test_classdef_passes_the_obs_cell_through():
    txt = open(os.path.join(ROOT, "matlab", "RRT_FANUC.m")).read()
    assert "cfs_mex('rrt', self.obs, self.sys_info" in txt and "cfs_rrt_grow_mesh" in txt
