"""Times the batched frame-acceleration queries (rsb_get_frame_accelerations, rsb_get_frame_jacobian_rates, rsb_imu_observe;
csrc/rsb_frame_accel.hip) at N = 4096, ANYmal-like and Atlas-like, with the feet and with every body as frames, torch CUDA tensors in and out
(RSB_DEVICE: nothing synchronises), through the C-ABI with the pointers made once.  Device-event time around 200 calls after 20 warm-up calls, median
of 7 such windows.  Yardsticks, in the same process: rsb_get_frame_kinematics with velocities (the same walk without accelerations),
rsb_get_frame_jacobians (for the rates), and one lock-step rsb_control_step of the same world.
Each model runs in a child process of its own under a time limit, and the tool stops at the first failure.
Writes profiles/frame_accel_bench.txt (--out PATH to write elsewhere).  There is no pass / fail threshold.  A tool, not part of bench.py."""
import ctypes as C
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N, CALLS, WARM, WINDOWS = 4096, 200, 20, 7
CASES = (("ANYmal-like", 2), ("Atlas-like", 5))
LIMIT = 240      # seconds per model


def timed(fn):
    """median over WINDOWS windows of the device-event time of CALLS calls, in microseconds per call"""
    import numpy as np
    import torch
    for _ in range(WARM):
        fn()
    per = []
    for _ in range(WINDOWS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(CALLS):
            fn()
        e1.record()
        e1.synchronize()
        per.append(e0.elapsed_time(e1) * 1e3 / CALLS)
    return float(np.median(per))


def case(name, config):
    import numpy as np
    import torch

    import bench
    from raisimlib_amd import BatchedWorld, _capi, workload
    dev = torch.device("cuda:0")
    r = bench.Recipe(config, -1.0)
    model = r.model
    w = BatchedWorld(model, N)
    w.set_stream(torch.cuda.current_stream().cuda_stream)
    r.setup_world(w, N, 0)
    gc0, gv0 = r.initial_state(N, 0)
    w.set_state(gc0, gv0)
    w.set_pd_target(None, np.zeros((N, model.nv), np.float32))
    feet = np.asarray(r.feet, np.int32)
    bank = torch.from_numpy(np.stack([r.targets(N, k, 0).astype(np.float32) for k in range(16)])).to(dev)
    g0, v0 = torch.from_numpy(gc0.astype(np.float32)).to(dev), torch.from_numpy(gv0.astype(np.float32)).to(dev)
    obs = torch.zeros((N, w.obs_dim(len(feet))), dtype=torch.float32, device=dev)
    step = w.control_step_plan(workload.SUBSTEPS, obs.data_ptr(), feet, feet, g0.data_ptr(), v0.data_ptr(), N)
    k = [0]

    def control_step():
        step(bank[k[0] % 16].data_ptr())
        k[0] += 1
    t_step = timed(control_step)      # (also brings the world into the benchmark's stationary mix of states)
    nv, nb, b = model.nv, model.nb, model.blob
    L, h, D = w.L, w.handle, _capi.RSB_DEVICE
    gen = torch.Generator(device=dev); gen.manual_seed(1)
    udot = torch.randn((N, nv), dtype=torch.float32, device=dev, generator=gen)
    p = lambda t: C.c_void_p(t.data_ptr())
    ck = _capi.check
    pct = lambda t: f"{100 * t / t_step:5.1f} % of a control step"
    lines = [f"{name}: N = {N}, {nb} bodies, nv = {nv}, tree depth {b.depth}",
             f"  rsb_control_step (lock-step, {workload.SUBSTEPS} sub-steps)                    {t_step:9.1f} us"]
    sets = (("the feet", [(int(b.col_body[s]), tuple(float(x) for x in b.col_pos[s])) for s in feet]), ("every body", [(i, (0.0, 0.0, 0.0)) for i in range(nb)]))
    for label, frames in sets:
        arr, F = w._frames(frames)
        a3 = [torch.empty((N, F, 3), dtype=torch.float32, device=dev) for _ in range(2)]
        j = [torch.empty((N, F, 3, nv), dtype=torch.float32, device=dev) for _ in range(2)]
        imu = torch.empty((N, F, 6), dtype=torch.float32, device=dev)
        pu, pl, pa, pjl, pjr, pi = p(udot), p(a3[0]), p(a3[1]), p(j[0]), p(j[1]), p(imu)
        t_kin = timed(lambda: ck(L.rsb_get_frame_kinematics(h, arr, F, None, None, pl, pa, D), "rsb_get_frame_kinematics"))
        t_acc = timed(lambda: ck(L.rsb_get_frame_accelerations(h, arr, F, pu, 0, pl, pa, D), "rsb_get_frame_accelerations"))
        t_bias = timed(lambda: ck(L.rsb_get_frame_accelerations(h, arr, F, None, 0, pl, None, D), "rsb_get_frame_accelerations"))
        t_imu = timed(lambda: ck(L.rsb_imu_observe(h, arr, F, pu, pi, 0, D), "rsb_imu_observe"))
        t_jac = timed(lambda: ck(L.rsb_get_frame_jacobians(h, arr, F, pjl, pjr, D), "rsb_get_frame_jacobians"))
        t_rate = timed(lambda: ck(L.rsb_get_frame_jacobian_rates(h, arr, F, pjl, pjr, D), "rsb_get_frame_jacobian_rates"))
        t_py = timed(lambda: w.imu_observe(frames, udot, out=imu))
        lines += [f"  {label}, F = {F}:",
                  f"    rsb_get_frame_kinematics, lin_vel + ang_vel (yardstick)       {t_kin:9.1f} us = {pct(t_kin)}",
                  f"    rsb_get_frame_accelerations, lin + ang, with udot             {t_acc:9.1f} us = {pct(t_acc)}",
                  f"    rsb_get_frame_accelerations, lin, udot = NULL (the bias)      {t_bias:9.1f} us = {pct(t_bias)}",
                  f"    rsb_imu_observe, with udot                                    {t_imu:9.1f} us = {pct(t_imu)}",
                  f"    rsb_get_frame_jacobians, lin + rot (yardstick)                {t_jac:9.1f} us = {pct(t_jac)}   ({2 * N * F * 3 * nv * 4 / 1e6:.1f} MB written)",
                  f"    rsb_get_frame_jacobian_rates, lin + rot                       {t_rate:9.1f} us = {pct(t_rate)}",
                  f"    BatchedWorld.imu_observe(frames, udot, out=..)                {t_py:9.1f} us   (the gap to the C-ABI line is host time of the Python mirror)"]
    w.close()
    print("\n".join(lines), flush=True)


def main():
    if "--case" in sys.argv:      # the child: one model
        i = int(sys.argv[sys.argv.index("--case") + 1])
        case(*CASES[i])
        return 0
    out = os.path.join(ROOT, "profiles", "frame_accel_bench.txt")
    if "--out" in sys.argv:
        out = sys.argv[sys.argv.index("--out") + 1]
    text = ["command: python tools/bench_frame_accel.py",
            f"device-event time per call: {CALLS} calls after {WARM} warm-up calls, median of {WINDOWS} windows; torch CUDA tensors (RSB_DEVICE), the world on torch's stream;",
            "the C-ABI with the pointers made once unless a line says otherwise", ""]
    for i in range(len(CASES)):
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--case", str(i)], capture_output=True, text=True, timeout=LIMIT)
        if r.returncode != 0:
            print(r.stdout + r.stderr)
            print(f"bench_frame_accel: {CASES[i][0]} failed with status {r.returncode}; stopping, nothing written")
            return 1
        print(r.stdout, end="")
        text += [r.stdout.rstrip(), ""]
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        f.write("\n".join(text))
    return 0


if __name__ == "__main__":
    sys.exit(main())
