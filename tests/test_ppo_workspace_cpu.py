"""The workspace sizes of the PPO update and the returns, pinned (no GPU needed).

The launchers carve their workspaces with the same descriptions the size functions use
(csrc/bg_ppo_fused.hip Gw2Space / Gw1Space / PlanSpace; csrc/bg_returns.hip), so the sizes
must stay what they were, byte for byte.  The literals below were printed by the library
built from the commit before the host-layer refactor (loaded through BGX_LIB), not by the
code under test."""
import ctypes
import os

import pytest

M = [0, 1, 31, 32, 33, 2048, 2**21]
SIZES = {
    "bgx_ppo_gw2_workspace": [8454144, 8718336, 8718336, 8718336, 8718336, 8982528, 549519360],
    "bgx_ppo_gw1_workspace": [3784704, 3784704, 3784704, 3784704, 3784704, 7340032, 62390272],
    "bgx_ppo_plan_workspace": [68, 204, 204, 204, 204, 340, 278596],
    "bgx_episode_stats_workspace": [0, 48, 48, 48, 48, 384, 393216],
    "bgx_selfplay_gae_workspace": [0, 16, 16, 16, 16, 128, 131072],
}


@pytest.fixture(scope="module")
def lib():
    import bgx._lib as L
    if not os.path.exists(L.LIB_PATH):
        pytest.skip("libbgx.so not built")
    return L.load()


@pytest.mark.parametrize("fn", sorted(SIZES))
def test_workspace_sizes(lib, fn):
    import bgx._lib as L
    f = getattr(lib, fn)
    assert (f.restype, f.argtypes) == (ctypes.c_int64, [ctypes.c_int32])
    assert [f(m) for m in M] == SIZES[fn]
    assert f(-1) == L.BGX_EINVAL
