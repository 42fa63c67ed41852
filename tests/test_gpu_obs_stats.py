"""Running observation statistics of the device-resident env on the GPU (include/rsb.h: rsb_env_observe_normalized, rsb_env_obs_stats_update,
rsb_env_obs_normalize, rsb_env_get_obs_stats / rsb_env_set_obs_stats, rsb_env_obs_stats_device).  The arithmetic is the template path's
updateObservationStatisticsAndNormalize (include/raisim/VectorizedEnvironment.hpp), restated here in numpy fp64; the statistics are deterministic
(no atomics), a block of batches folds to the bits of one-batch updates, and an actor network in the closed loop reads the live statistics."""
import os
import subprocess

import numpy as np
import pytest

from common import ROOT
from raisimlib_amd import workload

pytestmark = pytest.mark.gpu

RSC = os.path.join(ROOT, "raisimlib_amd", "rsc")
CFG = ("num_envs: {n}\nnum_threads: 8   # ignored\nsimulation_dt: 0.0025\ncontrol_dt: 0.01\nrender: false\naction_std: 0.3\n"
       "reward:\n  forwardVel:\n    coeff: 0.3\n  torque:\n    coeff: -4e-5\n")
GC_INIT = [0, 0, 0.57, 1.0, 0.0, 0.0, 0.0, 0.03, 0.4, -0.8, -0.03, 0.4, -0.8, 0.03, -0.4, 0.8, -0.03, -0.4, 0.8]


@pytest.fixture(scope="module")
def gm(built_lib):
    from raisimlib_amd.gym import build_env_module, load_env_module
    build_env_module(os.path.join(ROOT, "tests", "cpp", "anymal_env"), name="rsg_anymal")
    return load_env_module("rsg_anymal")


def ref_update(mean, var, count, ob):
    """the template path's update in fp64: batch mean and population variance over the envs, merged with Chan's formula"""
    x = np.asarray(ob, np.float64).reshape(-1, ob.shape[-1])
    n = x.shape[0]
    bm, bv = x.mean(0), x.var(0)
    tot = count + n
    d = mean - bm
    return mean * (count / tot) + bm * (n / tot), (var * count + bv * n + d * d * (count * n / tot)) / tot, tot


def random_actions(n, steps, seed):
    import torch
    g = torch.Generator(device="cpu").manual_seed(seed)
    return [((torch.rand((n, 12), generator=g) * 2 - 1) * (3.0 if k % 7 == 6 else 1.0)).to("cuda:0") for k in range(steps)]


def stats_run(anymal, n, steps, seed=3):
    """`steps` control steps with random actions; after each: the raw observation (rsb_env_observe), then the normalised one with update"""
    import torch
    env = workload.closed_loop_env(anymal, n)
    raw, norm, stats = [], [], []
    for a in random_actions(n, steps, seed):
        env.step(a)
        r = env.observe(torch.empty((n, env.num_obs), device="cuda:0"))
        o = env.observe(torch.empty((n, env.num_obs), device="cuda:0"), normalized=True, update_statistics=True)
        raw.append(r.cpu().numpy()); norm.append(o.cpu().numpy()); stats.append(env.obs_statistics())
    return env, raw, norm, stats


@pytest.mark.parametrize("n", [4096, 1000])
def test_statistics_and_normalisation_match_an_fp64_restatement(built_lib, anymal, n):
    env, raw, norm, stats = stats_run(anymal, n, 24)
    D = env.num_obs
    mean, var, count = np.zeros(D), np.ones(D), 1e-4
    for k in range(len(raw)):
        mean, var, count = ref_update(mean, var, count, raw[k])
        m, v, c = stats[k]
        assert c == pytest.approx(count, rel=1e-12), k
        np.testing.assert_allclose(m, mean, rtol=1e-5, atol=1e-12, err_msg=f"mean after step {k}")
        np.testing.assert_allclose(v, var, rtol=1e-5, atol=1e-12, err_msg=f"var after step {k}")
        want = (raw[k].astype(np.float64) - mean) / np.sqrt(var + 1e-8)
        ok = var > 1e-6
        assert ok.sum() > D // 2, k
        err = np.abs(norm[k] - want)[:, ok].max()
        assert err < 1e-4, (k, err)
    assert np.abs(np.stack(norm)[-1]).max() > 1.0       # (a live run: the statistics are not trivially the identity)
    env.close()


def test_template_path_parity(gm):
    """RaisimGymEnv(normalizeObservation=True) beside DeviceRaisimGymEnv(normalize_observation=True), the same actions, observe(True) after every
    step: after 25 steps the statistics agree and the counts are equal.  (The two paths' raw observations agree to 1e-4 - test_gym_module.py -,
    so the tolerance carries that bound besides rtol 1e-4.)"""
    n = 64
    tpl = gm.RaisimGymEnv(RSC, CFG.format(n=n), True)
    cfg = gm.VecEnvConfig()
    cfg.num_envs, cfg.gc_init, cfg.normalize_observation = n, GC_INIT, True
    dev = gm.DeviceRaisimGymEnv(os.path.join(RSC, "anymal_c_like.urdf"), cfg)
    dev.init()
    tpl.reset()
    rng = np.random.default_rng(0)
    o1, o2 = np.zeros((n, 34), np.float32), np.zeros((n, 34), np.float32)
    r1, r2, d1, d2 = np.zeros(n, np.float32), np.zeros(n, np.float32), np.zeros(n, bool), np.zeros(n, bool)
    for it in range(25):
        a = (rng.uniform(-1, 1, (n, 12)) * (4.0 if it % 6 == 5 else 1.0)).astype(np.float32)
        tpl.step(a, r1, d1)
        dev.step(a, r2, d2)
        tpl.observe(o1, True)
        dev.observe(o2, True)
        assert np.array_equal(d1, d2)
    m1, v1, m2, v2 = (np.zeros(34, np.float32) for _ in range(4))
    c1, c2 = tpl.getObStatistics(m1, v1), dev.getObStatistics(m2, v2)
    assert c1 == c2
    assert np.all(np.abs(m2 - m1) <= 1e-4 * np.abs(m1) + 1e-4)
    assert np.all(np.abs(v2 - v1) <= 1e-4 * v1 + 2e-4 * np.sqrt(v1))
    assert np.isfinite(o2).all() and np.abs(o2).max() > 1.0


def test_deterministic_batched_and_round_trips(built_lib, anymal):
    import torch
    n, K = 1000, 12
    # (a) two identical runs: bit-identical statistics and normalised observations
    runs = [stats_run(anymal, n, 6, seed=11) for _ in range(2)]
    for k in range(6):
        assert np.array_equal(runs[0][2][k], runs[1][2][k]), k
        for a, b in zip(runs[0][3][k], runs[1][3][k]):
            assert np.array_equal(np.asarray(a), np.asarray(b)), k
    for r in runs:
        r[0].close()
    # (b) a rollout block [K + 1, N, D] in one call == K + 1 one-batch calls, bit for bit
    env = workload.closed_loop_env(anymal, n)
    layers = [(torch.from_numpy(W).to("cuda:0"), torch.from_numpy(b).to("cuda:0")) for W, b in workload.closed_loop_mlp(env.num_obs, env.num_acts, hidden=(64, 32), out_scale=0.3)]
    ro = {"ob": torch.zeros((K + 1, n, env.num_obs), device="cuda:0")}
    env.rollout_mlp(K, layers, rollout=ro)
    m0 = (np.linspace(-1, 1, env.num_obs) * 0.3).astype(np.float32)
    v0 = np.linspace(0.2, 3.0, env.num_obs).astype(np.float32)
    probe = torch.randn((n, env.num_obs), generator=torch.Generator(device="cpu").manual_seed(5)).to("cuda:0") * 3
    out = {}
    for mode in ("block", "single"):
        env.set_obs_statistics(m0, v0, 100.0)
        if mode == "block":
            env.update_obs_statistics(ro["ob"])
        else:
            for k in range(K + 1):
                env.update_obs_statistics(ro["ob"][k])
        out[mode] = (*env.obs_statistics(), env.normalize_obs(probe).cpu().numpy())
    for a, b in zip(out["block"], out["single"]):
        assert np.array_equal(np.asarray(a), np.asarray(b))
    assert out["block"][2] == 100.0 + (K + 1) * n
    # (c) update=False leaves the statistics alone; the normalised observation is the raw one through rsb_env_obs_normalize
    before = env.obs_statistics()
    raw = env.observe(torch.empty((n, env.num_obs), device="cuda:0"))
    o = env.observe(torch.empty((n, env.num_obs), device="cuda:0"), normalized=True, update_statistics=False)
    after = env.obs_statistics()
    for a, b in zip(before, after):
        assert np.array_equal(np.asarray(a), np.asarray(b))
    assert torch.equal(o, env.normalize_obs(raw))
    clipped = env.observe(torch.empty((n, env.num_obs), device="cuda:0"), normalized=True, clip=0.5)
    assert torch.equal(clipped, torch.clamp(o, -0.5, 0.5))
    host = env.normalize_obs(raw.cpu().numpy())        # the host path: staged through the library, same kernel
    assert np.array_equal(host, o.cpu().numpy())
    # (d) set -> get round-trips exactly
    m1 = np.random.default_rng(1).normal(size=env.num_obs).astype(np.float32)
    v1 = np.random.default_rng(2).uniform(0.01, 5, size=env.num_obs).astype(np.float32)
    env.set_obs_statistics(m1, v1, 12345.678)
    m, v, c = env.obs_statistics()
    assert np.array_equal(m, m1) and np.array_equal(v, v1) and c == 12345.678
    env.close()


def test_closed_loop_reads_the_live_statistics(built_lib, anymal):
    """rollout_mlp(live_ob_stats=True): the actions are a torch forward pass over clamp((ob - mean) * rsqrt(var + eps), +-clip) of the rollout's raw
    observations with the statistics as of the launch; lock-step, pipelined and resident give the same bits; an update between two rollouts is
    seen by the second."""
    import torch
    n, K1, K = 1000, 8, 20
    dev = torch.device("cuda:0")
    mlp = [(torch.from_numpy(W).to(dev), torch.from_numpy(b).to(dev)) for W, b in workload.closed_loop_mlp(34, 12, hidden=(64, 32), out_scale=0.3)]

    def forward(ob, mean, var, clip):
        x = torch.clamp((ob.double() - torch.from_numpy(mean).to(dev).double()) * torch.rsqrt(torch.from_numpy(var).to(dev) + 1e-8).double(), -clip, clip)
        for i, (W, b) in enumerate(mlp):
            x = x @ W.double().t() + b.double()
            if i + 1 < len(mlp):
                x = torch.tanh(x)
        return torch.clamp(x, -3.0, 3.0)

    out = {}
    for mode in ("lockstep", "pipelined", "resident"):
        env = workload.closed_loop_env(anymal, n)
        if mode == "pipelined":
            assert env.world.set_step_pipelining(True)
        if mode == "resident":
            env.world.set_step_residency(True)
            assert env.world.residency_status(2)
        ro0 = {"ob": torch.zeros((K1 + 1, n, 34), device=dev)}
        env.rollout_mlp(K1, mlp, activation="tanh", clip=3.0, rollout=ro0)          # raw statistics-free warm-up run
        env.update_obs_statistics(ro0["ob"])
        runs = []
        for r in range(2):
            ro = {"ob": torch.zeros((K + 1, n, 34), device=dev), "act": torch.zeros((K, n, 12), device=dev),
                  "reward": torch.zeros((K, n), device=dev), "done": torch.zeros((K, n), dtype=torch.uint8, device=dev)}
            stats = env.obs_statistics()
            env.rollout_mlp(K, mlp, activation="tanh", clip=3.0, ob_clip=5.0, rollout=ro, live_ob_stats=True)
            env.update_obs_statistics(ro["ob"])          # folded after the run: the next run sees it
            env.world.step_pipeline_join()
            runs.append((ro, stats))
        with pytest.raises(ValueError):
            env.rollout_mlp(1, mlp, ob_mean=torch.zeros(34, device=dev), ob_var=torch.ones(34, device=dev), live_ob_stats=True)
        out[mode] = (runs, env.obs_statistics())
        env.close()
    for mode in ("pipelined", "resident"):
        for (ra, sa), (rb, sb) in zip(out["lockstep"][0], out[mode][0]):
            for key in ra:
                assert torch.equal(ra[key], rb[key]), (mode, key)
        for a, b in zip(out["lockstep"][1], out[mode][1]):
            assert np.array_equal(np.asarray(a), np.asarray(b)), mode
    (ro1, s1), (ro2, s2) = out["lockstep"][0]
    assert s2[2] == s1[2] + (K + 1) * n and not np.array_equal(s1[0], s2[0])
    for ro, (m, v, _) in ((ro1, s1), (ro2, s2)):
        err = (ro["act"].double() - forward(ro["ob"][:K], m, v, 5.0)).abs().max().item()
        assert err < 2e-5, err
    stale = (ro2["act"].double() - forward(ro2["ob"][:K], s1[0], s1[1], 5.0)).abs().max().item()
    assert stale > 1e-4, stale            # the second run did not use the first run's statistics


def test_upstream_runner_over_the_device_env(gm, tmp_path):
    """RaisimGymVecEnv(DeviceRaisimGymEnv(cfg with normalisation)): construct, reset, step, observe(True), save_scaling, load_scaling"""
    from raisimlib_amd.gym import RaisimGymVecEnv
    n = 128
    cfg = gm.VecEnvConfig()
    cfg.num_envs, cfg.gc_init, cfg.normalize_observation, cfg.obs_clip = n, GC_INIT, True, 10.0
    impl = gm.DeviceRaisimGymEnv(os.path.join(RSC, "anymal_c_like.urdf"), cfg)
    impl.init()
    env = RaisimGymVecEnv(impl)
    env.reset()
    rng = np.random.default_rng(4)
    for _ in range(5):
        env.step(rng.uniform(-1, 1, (n, 12)).astype(np.float32))
        ob = env.observe(True)
        assert ob.shape == (n, 34) and np.isfinite(ob).all() and np.abs(ob).max() <= 10.0
    env.save_scaling(str(tmp_path), "3")
    assert env.count == pytest.approx(1e-4 + 5 * n)
    saved_mean, saved_var = env.mean.copy(), env.var.copy()
    env.wrapper.setObStatistics(np.zeros(34, np.float32), np.ones(34, np.float32), 1.0)
    env.load_scaling(str(tmp_path), 3, count=2e5)
    m, v = np.zeros(34, np.float32), np.zeros(34, np.float32)
    c = env.wrapper.getObStatistics(m, v)
    assert np.array_equal(m, saved_mean) and np.array_equal(v, saved_var) and c == 2e5
    ob = env.observe(False)
    assert np.isfinite(ob).all()
    term = np.zeros(n, bool)
    env.wrapper.isTerminalState(term)
    env.wrapper.setSimulationTimeStep(0.0025); env.wrapper.setControlTimeStep(0.01)      # (reconfigures the task: the statistics stay)
    env.wrapper.getObStatistics(m, v)
    assert np.array_equal(m, saved_mean)
    env.close()


def test_obs_stats_facade_runs_on_gpu(built_lib):
    from test_obs_stats_host import BIN, URDF, compile_obs_stats_facade
    compile_obs_stats_facade()
    r = subprocess.run([BIN, URDF], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "obs_stats_facade_test OK" in r.stdout
