"""Times the sensor-mounted ray scan (rsb_ray_scan; csrc/rsb_ray_scan.hip) at N = 4096 ANYmal-like envs, one frame on the base, a 32 x 24 pinhole
pattern pitched down by 0.5 rad, max_dist 10 m, torch CUDA tensors in and out (RSB_DEVICE: nothing synchronises):
  on the ground plane of bench.py's config 2 and on the shared 128 x 128 height map of its config 3;
  terrain only (flags 0) and with the robot's collision shapes (RSB_RAY_BODIES);
  against what a caller had to do before this entry point for the terrain-only image: rsb_get_frame_kinematics (pos, rot) into torch tensors,
  the pattern rotated in torch, rsb_ray_test - three passes over [N, P, 3] tensors (its largest difference from the fused scan is printed);
  and, for scale, the lock-step rsb_control_step of the same world.
Device-event time around 200 calls after 20 warm-up calls, median of 7 such windows.  Writes profiles/ray_scan_bench.txt (--out PATH to write
elsewhere).  A tool, not part of bench.py."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

import bench
from raisimlib_amd import BatchedWorld, depth_camera_rays, workload

N, CALLS, WARM, WINDOWS = 4096, 200, 20, 7
W, H, HFOV, PITCH, MAX_DIST = 32, 24, 1.5, 0.5, 10.0
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


class Composed:
    """the terrain-only image from the entry points that existed before: frame kinematics, a rotation in torch, rsb_ray_test"""

    def __init__(self, w, frame, dirs):
        self.w, self.frame, self.dirs = w, [frame], torch.from_numpy(dirs).to(dev)
        P = dirs.shape[0]
        self.kin = {"pos": torch.empty((N, 1, 3), dtype=torch.float32, device=dev), "rot": torch.empty((N, 1, 3, 3), dtype=torch.float32, device=dev)}
        self.dist = torch.empty((N, P), dtype=torch.float32, device=dev)
        self.P = P

    def __call__(self):
        self.w.frame_kinematics(self.frame, out=self.kin)
        o = self.kin["pos"].expand(N, self.P, 3).contiguous()
        d = torch.matmul(self.dirs, self.kin["rot"][:, 0].transpose(1, 2)).contiguous()      # [N, P, 3]: R dirs[k]
        self.w.ray_test(o, d, MAX_DIST, out=self.dist)
        return self.dist


def main():
    out = os.path.join(ROOT, "profiles", "ray_scan_bench.txt")
    if "--out" in sys.argv:
        out = sys.argv[sys.argv.index("--out") + 1]
    c, s = np.cos(PITCH), np.sin(PITCH)
    dirs = (depth_camera_rays(W, H, HFOV).astype(np.float64) @ np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]]).T).astype(np.float32)
    P = dirs.shape[0]
    frame = (0, (0.35, 0.0, 0.1))      # at the front of the base, outside its collision spheres
    lines = []
    for config, terrain in ((2, "ground plane (config 2)"), (3, "shared 128 x 128 height map (config 3)")):
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
        tdirs = torch.from_numpy(dirs).to(dev)
        img = torch.empty((N, 1, P), dtype=torch.float32, device=dev)
        hit = torch.empty((N, 1, P), dtype=torch.int32, device=dev)
        t_terrain = timed(lambda: w.ray_scan([frame], tdirs, MAX_DIST, bodies=False, out=img))
        plain = img.clone()
        composed = Composed(w, frame, dirs)
        t_composed = timed(composed)
        both = (plain[:, 0] >= 0) & (composed() >= 0)
        diff = float((composed() - plain[:, 0]).abs()[both].max())
        flips = int(((plain[:, 0] >= 0) != (composed() >= 0)).sum())
        t_bodies = timed(lambda: w.ray_scan([frame], tdirs, MAX_DIST, bodies=True, out=img))
        t_depth = timed(lambda: w.ray_scan([frame], tdirs, MAX_DIST, bodies=True, planar=True, miss_max=True, out={"out": img, "hit": hit}))
        on_robot, on_ground = float((hit >= 0).float().mean()), float((hit == -2).float().mean())
        lines += [f"ANYmal-like, N = {N}, one frame on the base, {W} x {H} pattern (P = {P}), max_dist {MAX_DIST:g} m, {terrain}",
                  f"  rsb_control_step (lock-step, {workload.SUBSTEPS} sub-steps)                      {t_step:9.1f} us",
                  f"  rsb_ray_scan, terrain only (flags 0)                          {t_terrain:9.1f} us = {100 * t_terrain / t_step:5.1f} % of a control step   (writes {N * P * 4 / 1e6:.1f} MB)",
                  f"    composed: rsb_get_frame_kinematics + rotation in torch + rsb_ray_test {t_composed:9.1f} us = {t_composed / t_terrain:5.2f} x the fused call"
                  f"   (max |difference| where both hit {diff:.2e}, {flips} of {N * P} rays hit in one and miss in the other)",
                  f"  rsb_ray_scan, RSB_RAY_BODIES                                  {t_bodies:9.1f} us = {t_bodies / t_terrain:5.2f} x terrain only",
                  f"  rsb_ray_scan, BODIES | PLANAR | MISS_MAX, ranges and hit codes {t_depth:9.1f} us   ({100 * on_robot:.1f} % of the rays stop at the robot, {100 * on_ground:.1f} % at the terrain)",
                  f"  the fused terrain-only scan is {'NOT slower' if t_terrain <= t_composed else 'SLOWER'} than the composition", ""]
        w.close()
    print("\n".join(lines), flush=True)
    text = [f"command: python tools/bench_ray_scan.py {' '.join(sys.argv[1:])}".rstrip(),
            f"device-event time per call: {CALLS} calls after {WARM} warm-up calls, median of {WINDOWS} windows; torch CUDA tensors (RSB_DEVICE), the world on torch's stream", ""]
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        f.write("\n".join(text + lines) + "\n")


if __name__ == "__main__":
    main()
