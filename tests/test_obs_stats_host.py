"""Running observation statistics of the device-resident env (include/rsb.h: rsb_env_observe_normalized & co.), CPU tier: the C-ABI declares,
exports and prototypes the new entry points, the facade and the gym module carry the surface RaisimGymVecEnv calls, and a C++ program written
against the facade's new methods compiles with g++.  tests/test_gpu_obs_stats.py runs all of it on the GPU."""
import os
import subprocess

import pytest

from common import ROOT

NEW_ENTRY_POINTS = ("rsb_env_observe_normalized", "rsb_env_obs_stats_update", "rsb_env_obs_normalize", "rsb_env_get_obs_stats",
                    "rsb_env_set_obs_stats", "rsb_env_obs_stats_device")
BIN = os.path.join(ROOT, "tests", "cpp", "_build", "obs_stats_facade_test")
URDF = os.path.join(ROOT, "raisimlib_amd", "rsc", "anymal_c_like.urdf")


@pytest.fixture(scope="module")
def gym_module(built_lib):
    from raisimlib_amd.gym import build_env_module, load_env_module
    build_env_module(os.path.join(ROOT, "tests", "cpp", "anymal_env"), name="rsg_anymal")
    return load_env_module("rsg_anymal")


def compile_obs_stats_facade():
    os.makedirs(os.path.dirname(BIN), exist_ok=True)
    lib = os.path.join(ROOT, "raisimlib_amd", "lib")
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-pthread", "-I", os.path.join(ROOT, "include"), "-o", BIN,
                    os.path.join(ROOT, "tests", "cpp", "obs_stats_facade_test.cpp"), "-L", lib, "-lrsb", f"-Wl,-rpath,{lib}"], check=True)


def test_new_entry_points_are_declared_exported_and_prototyped(built_lib):
    from raisimlib_amd import _capi
    from test_capi_abi import header_functions
    declared = header_functions()
    for name in NEW_ENTRY_POINTS:
        assert name in declared, name
        assert hasattr(built_lib, name), name
        assert name in _capi.PROTOTYPES, name


def test_new_entry_points_refuse_a_null_world(built_lib):
    """no world, no device work: every new call returns RSB_E_INVALID (a CPU box can run this)"""
    import ctypes as C
    L = built_lib
    assert L.rsb_env_observe_normalized(None, None, 1, 0.0, 0) != 0
    assert L.rsb_env_obs_stats_update(None, None, 1, 0, 0) != 0
    assert L.rsb_env_obs_normalize(None, None, None, 1, 0.0, 0) != 0
    assert L.rsb_env_get_obs_stats(None, None, None, None) != 0
    assert L.rsb_env_set_obs_stats(None, None, None, 1.0) != 0
    m, s = C.c_void_p(0), C.c_void_p(0)
    assert L.rsb_env_obs_stats_device(None, C.byref(m), C.byref(s)) != 0


def test_device_env_binds_what_raisim_gym_vec_env_calls(gym_module):
    """DeviceRaisimGymEnv has every method of RaisimGymEnv that test_gym_module.py lists (upstream's raisim_gym surface), statistics included"""
    for meth in ("init", "reset", "observe", "step", "setSeed", "close", "isTerminalState", "setSimulationTimeStep", "setControlTimeStep",
                 "getObDim", "getActionDim", "getNumOfEnvs", "turnOnVisualization", "turnOffVisualization", "curriculumUpdate",
                 "getObStatistics", "setObStatistics"):
        assert hasattr(gym_module.DeviceRaisimGymEnv, meth), meth
    for meth in ("observeDevice", "stepDevice", "updateObStatistics"):
        assert hasattr(gym_module.DeviceRaisimGymEnv, meth), meth


def test_vec_env_config_has_the_normaliser_switches(gym_module):
    cfg = gym_module.VecEnvConfig()
    assert cfg.normalize_observation is False and cfg.obs_clip == 0.0      # defaults keep the raw observations (upstream normalises by default)
    cfg.normalize_observation, cfg.obs_clip = True, 10.0
    assert cfg.normalize_observation is True and cfg.obs_clip == 10.0


def test_python_vec_env_has_the_statistics_surface(built_lib):
    import inspect
    from raisimlib_amd.vecenv import VecEnv
    for meth in ("update_obs_statistics", "obs_statistics", "set_obs_statistics", "obs_statistics_device", "normalize_obs"):
        assert callable(getattr(VecEnv, meth, None)), meth
    sig = inspect.signature(VecEnv.observe).parameters
    assert sig["normalized"].default is False and sig["update_statistics"].default is False
    assert inspect.signature(VecEnv.rollout_mlp).parameters["live_ob_stats"].default is False


def test_obs_stats_facade_compiles_with_gxx(built_lib):
    compile_obs_stats_facade()
    if built_lib.rsb_device_count() > 0:
        pytest.skip("a GPU is visible: covered by the gpu test")
    r = subprocess.run([BIN, URDF], capture_output=True, text=True)
    assert r.returncode == 1 and "no HIP device" in r.stdout
