"""Times the batched frame queries (rsb_get_frame_kinematics, rsb_get_frame_jacobians, rsb_add_external_wrench; csrc/rsb_frames.hip) at N = 4096:
ANYmal-like with 5 frames (base + the four feet) and Atlas-like with every body, torch CUDA tensors in and out (RSB_DEVICE: nothing synchronises).
Device-event time around 200 calls after 20 warm-up calls, median of 7 such windows.  For scale, in the same process: the lock-step
rsb_control_step of the same world (what a control step costs), and - from a child process built with g++ from tools/bench_frames_host.cpp - the
facade's per-env host loop over the same frames for the same 4096 envs (what the same information cost before these entry points existed).
Writes profiles/r09_frames_timing.txt (--out PATH to write elsewhere).  A tool, not part of bench.py."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

import bench
from raisimlib_amd import BatchedWorld, workload

N, CALLS, WARM, WINDOWS = 4096, 200, 20, 7
dev = torch.device("cuda:0")


def timed(fn):
    """median over WINDOWS windows of the device-event time of CALLS calls, in microseconds per call"""
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


def host_loop(urdf, bodies):
    exe = os.path.join(ROOT, "tools", "_build", "bench_frames_host")
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    lib = os.path.join(ROOT, "raisimlib_amd", "lib")
    subprocess.run(["g++", "-std=c++17", "-O2", "-pthread", "-I", os.path.join(ROOT, "include"), "-o", exe, os.path.join(ROOT, "tools", "bench_frames_host.cpp"),
                    "-L", lib, "-lrsb", f"-Wl,-rpath,{lib}"], check=True)
    out = subprocess.run([exe, urdf, str(N), *[str(b) for b in bodies]], check=True, capture_output=True, text=True, timeout=600).stdout.split()
    return float(out[1]), float(out[3])


def case(name, config, urdf, frames, bodies_for_host):
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
    F = len(frames)
    kin = {n: torch.empty(s, dtype=torch.float32, device=dev) for n, s in dict(pos=(N, F, 3), rot=(N, F, 3, 3), lin_vel=(N, F, 3), ang_vel=(N, F, 3)).items()}
    jac = {n: torch.empty((N, F, 3, model.nv), dtype=torch.float32, device=dev) for n in ("lin", "rot")}
    force, torque = torch.randn((N, 3), device=dev), torch.randn((N, 3), device=dev)
    t_kin = timed(lambda: w.frame_kinematics(frames, out=kin))
    t_pos = timed(lambda: w.frame_kinematics(frames, out={"pos": kin["pos"]}))
    t_jac = timed(lambda: w.frame_jacobians(frames, out=jac))
    t_wr = timed(lambda: w.add_external_wrench(frames[-1], force, torque))
    w.set_generalized_force(np.zeros((N, model.nv), np.float32))
    w.close()
    t_host, t_batched_host = host_loop(urdf, bodies_for_host)
    kb = N * (model.nq + model.nv) * 4 / 1e3, N * F * 18 * 4 / 1e3
    lines = [f"{name}: N = {N}, {F} frames, nv = {model.nv}, tree depth {model.blob.depth}",
             f"  rsb_control_step (lock-step, {workload.SUBSTEPS} sub-steps)     {t_step:9.1f} us",
             f"  rsb_get_frame_kinematics (pos, rot, lin_vel, ang_vel) {t_kin:9.1f} us = {100 * t_kin / t_step:5.1f} % of a control step   (reads {kb[0]:.0f} kB, writes {kb[1]:.0f} kB)",
             f"  rsb_get_frame_kinematics (pos only)                   {t_pos:9.1f} us = {100 * t_pos / t_step:5.1f} %",
             f"  rsb_get_frame_jacobians (J_lin, J_rot)                {t_jac:9.1f} us = {100 * t_jac / t_step:5.1f} %   (writes {N * F * 6 * model.nv * 4 / 1e6:.1f} MB)",
             f"  rsb_add_external_wrench (force + torque, one frame)   {t_wr:9.1f} us = {100 * t_wr / t_step:5.1f} %",
             f"  per-env host loop over the same frames (4 accessors)  {t_host:9.1f} ms   (the batched call with RSB_HOST outputs, copies included: {t_batched_host:.2f} ms)"]
    print("\n".join(lines), flush=True)
    return lines


def main():
    out = os.path.join(ROOT, "profiles", "r09_frames_timing.txt")
    if "--out" in sys.argv:
        out = sys.argv[sys.argv.index("--out") + 1]
    rsc = os.path.join(ROOT, "raisimlib_amd", "rsc")
    a = bench.Recipe(2, -1.0).model
    feet = sorted(a.collision_indices("_foot"))[:4]
    frames_a = [(0, (0.0, 0.0, 0.0))] + [(int(a.blob.col_body[s]), tuple(float(x) for x in a.blob.col_pos[s])) for s in feet]
    t = bench.Recipe(5, -1.0).model
    frames_t = [(b, (0.0, 0.0, 0.0)) for b in range(t.nb)]
    text = [f"command: python tools/bench_frames.py {' '.join(sys.argv[1:])}".rstrip(),
            f"device-event time per call: {CALLS} calls after {WARM} warm-up calls, median of {WINDOWS} windows; torch CUDA tensors (RSB_DEVICE), the world on torch's stream", ""]
    text += case("ANYmal-like, base + four feet", 2, os.path.join(rsc, "anymal_c_like.urdf"), frames_a, [f[0] for f in frames_a]) + [""]
    text += case("Atlas-like, every body", 5, os.path.join(rsc, "atlas_like.urdf"), frames_t, [f[0] for f in frames_t])
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        f.write("\n".join(text) + "\n")


if __name__ == "__main__":
    main()
