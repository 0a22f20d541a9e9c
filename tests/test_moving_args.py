"""Per-waypoint obstacles at the Python surface, without a device: obs cells with 3x2xH axes, their arrays, and the
combinations that are refused before anything reaches the library (CPU)."""
import numpy as np
import pytest

import motionplanning_5d_m_amd as pkg
from motionplanning_5d_m_amd import solvers


def _moving_cell(H):
    a = np.array([[3.806, 3.606], [8.413, 8.413], [0.001, 1.038]])
    l3 = a[:, :, None] + np.linspace(0.0, 0.3, H)[None, None, :] * np.array([1.0, 0.0, 0.0])[:, None, None]
    return [dict(l=l3, epsilon=0.25, D=0.2), dict(l=a + 0.5, epsilon=0.25, D=0.2)]


def test_obs_traj_to_array_layout_and_broadcast():
    H = 7
    obs = _moving_cell(H)
    arr = pkg.obs_traj_to_array(obs, H)
    assert arr.shape == (H, 2, 6) and arr.flags.c_contiguous and arr.dtype == np.float64
    for i in range(H):
        np.testing.assert_array_equal(arr[i, 0], np.concatenate([obs[0]["l"][:, 0, i], obs[0]["l"][:, 1, i]]))
        np.testing.assert_array_equal(arr[i, 1], pkg.obs_to_array([obs[1]])[0])     # the 3x2 entry is held over the horizon
    assert arr[0, 0, 0] != arr[-1, 0, 0]
    assert solvers.obs_moving(obs) and not solvers.obs_moving([obs[1]])
    static = pkg.obs_traj_to_array([obs[1]], H)                                      # a static cell as rows: constant
    assert (static == static[:1]).all()


@pytest.mark.parametrize("shape", [(3, 2, 6), (3, 2, 8), (2, 2, 7), (3, 3)])
def test_obs_traj_to_array_rejects_wrong_shapes(shape):
    with pytest.raises(ValueError):
        pkg.obs_traj_to_array([dict(l=np.zeros(shape), epsilon=0.25, D=0.2)], 7)


def test_refused_before_the_device():
    R, s, obs = pkg.main_FANUC_problem()
    with pytest.raises(ValueError):
        pkg.CFSBatch(s, 1, [0.25], obstacles="moving")                # unknown motion
    with pytest.raises(ValueError):
        pkg.CFSBatch(s, 1, [0.25], obstacles=1)
    cell = _moving_cell(s.H)
    with pytest.raises(ValueError):                                     # a 3x2xH axis whose page count is not H
        pkg.CFS_FANUC([dict(cell[0], l=cell[0]["l"][:, :, :-1])], s, R)
    with pytest.raises(ValueError):                                     # meshes are static: not in a moving cell
        pkg.PSGCFS_FANUC(cell + [dict(mesh=object(), epsilon=0.25, D=0.2)], s, R)
    with pytest.raises(ValueError):                                     # CHOMP takes static obstacles only
        pkg.CHOMP_FANUC([dict(num_obs=2)] + cell, s, np.zeros(s.H * 5), R)


def test_per_waypoint_shape_checks_of_the_batch_handle():
    """the shape rule of CFSBatch._check_obs, on a stand-in whose motion is per waypoint (no device needed)"""
    class Stub:
        H, nobs, obstacle_motion = 5, 3, "per_waypoint"
        _check_obs = pkg.CFSBatch._check_obs
    st = Stub()
    st._check_obs(np.zeros((2, 5, 3, 6)), 2)
    for bad in [(2, 3, 6), (2, 5, 3, 5), (2, 4, 3, 6), (1, 5, 3, 6)]:
        with pytest.raises(ValueError):
            st._check_obs(np.zeros(bad), 2)
    Stub.obstacle_motion = "static"
    st._check_obs(np.zeros((2, 3, 6)), 2)
    with pytest.raises(AssertionError):
        st._check_obs(np.zeros((2, 5, 3, 6)), 2)
