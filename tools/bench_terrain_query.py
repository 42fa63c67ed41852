"""Times the batched terrain queries (rsb_get_terrain_height, rsb_height_scan, rsb_ray_test; csrc/rsb_terrain_query.hip) at N = 4096 on the shared
128 x 128 height map of bench.py's config 3, torch CUDA tensors in and out (RSB_DEVICE: nothing synchronises):
  the fused height scan for a 17 x 11 pattern under the base and for 4 feet x 9 points;
  the same two results composed from what existed before these entry points: rsb_get_frame_kinematics (pos, rot) into torch tensors and the
  triangle lookup written in torch below (its largest difference from the fused scan is printed with it);
  rsb_get_terrain_height at P = 187, rsb_ray_test at R = 64 downward-forward rays;
  and, for scale, the lock-step rsb_control_step of the same world.
Device-event time around 200 calls after 20 warm-up calls, median of 7 such windows.  Writes profiles/r10_terrain_query_bench.txt (--out PATH to
write elsewhere).  A tool, not part of bench.py."""
import os
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


def grid(nx, ny, hx, hy):
    gx, gy = np.meshgrid(np.linspace(-hx, hx, nx), np.linspace(-hy, hy, ny), indexing="ij")
    return np.stack([gx.ravel(), gy.ravel()], axis=-1).astype(np.float32)


class TorchScan:
    """the scan composed in torch: frame positions and rotations from rsb_get_frame_kinematics, then the collider's triangulation"""

    def __init__(self, w, frames, pattern, heights, size):
        self.w, self.frames, self.pat = w, frames, torch.from_numpy(pattern).to(dev)
        self.H = torch.from_numpy(np.ascontiguousarray(heights, np.float32)).to(dev).reshape(-1)
        self.ys, self.xs = heights.shape
        self.x0 = self.y0 = -0.5 * size
        self.inv_dx, self.inv_dy = (self.xs - 1) / size, (self.ys - 1) / size
        F = len(frames)
        self.kin = {"pos": torch.empty((N, F, 3), dtype=torch.float32, device=dev), "rot": torch.empty((N, F, 3, 3), dtype=torch.float32, device=dev)}

    def __call__(self):
        self.w.frame_kinematics(self.frames, out=self.kin)
        p, R = self.kin["pos"], self.kin["rot"]
        hy = torch.hypot(R[..., 0, 0], R[..., 1, 0]).clamp_min(1e-6)
        c, s = (R[..., 0, 0] / hy)[..., None], (R[..., 1, 0] / hy)[..., None]
        x = p[..., 0:1] + c * self.pat[:, 0] - s * self.pat[:, 1]
        y = p[..., 1:2] + s * self.pat[:, 0] + c * self.pat[:, 1]
        gx = ((x - self.x0) * self.inv_dx).clamp(0, self.xs - 1)
        gy = ((y - self.y0) * self.inv_dy).clamp(0, self.ys - 1)
        ix, iy = gx.floor().clamp_max(self.xs - 2), gy.floor().clamp_max(self.ys - 2)
        fx, fy = gx - ix, gy - iy
        base = iy.long() * self.xs + ix.long()
        h00, h10, h01, h11 = self.H[base], self.H[base + 1], self.H[base + self.xs], self.H[base + self.xs + 1]
        lower = fx >= fy
        sx, sy = torch.where(lower, h10 - h00, h11 - h01), torch.where(lower, h11 - h10, h01 - h00)
        return p[..., 2:3] - (h00 + sx * fx + sy * fy)


def main():
    out = os.path.join(ROOT, "profiles", "r10_terrain_query_bench.txt")
    if "--out" in sys.argv:
        out = sys.argv[sys.argv.index("--out") + 1]
    r = bench.Recipe(3, -1.0)
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
    maps, _ = r.terrain(N, 0)
    size = workload.HEIGHTMAP_SIZE
    base = [(0, (0.0, 0.0, 0.0))]
    foot_frames = [(int(model.blob.col_body[s]), tuple(float(x) for x in model.blob.col_pos[s])) for s in sorted(model.collision_indices("_foot"))[:4]]
    cases = [("base, 17 x 11 pattern (P = 187)", base, grid(17, 11, 0.8, 0.5)), ("4 feet x 9 points (3 x 3, P = 9)", foot_frames, grid(3, 3, 0.1, 0.1))]
    lines = [f"ANYmal-like on the shared 128 x 128 height map of config 3: N = {N}",
             f"  rsb_control_step (lock-step, {workload.SUBSTEPS} sub-steps)            {t_step:9.1f} us"]
    for name, frames, pattern in cases:
        F, P = len(frames), pattern.shape[0]
        tp = torch.from_numpy(pattern).to(dev)
        fused = torch.empty((N, F, P), dtype=torch.float32, device=dev)
        t_fused = timed(lambda: w.height_scan(frames, tp, out=fused))
        composed = TorchScan(w, frames, pattern, maps[0], size)
        t_torch = timed(composed)
        diff = float((composed() - fused).abs().max())
        lines += [f"  rsb_height_scan, {name:34s} {t_fused:9.1f} us = {100 * t_fused / t_step:5.1f} % of a control step   (writes {N * F * P * 4 / 1e3:.0f} kB)",
                  f"    composed: rsb_get_frame_kinematics + lookup in torch     {t_torch:9.1f} us = {t_torch / t_fused:5.1f} x the fused call   (max |difference| {diff:.2e})"]
    P, R = 187, 64
    rng = np.random.default_rng(1)
    xy = torch.from_numpy(rng.uniform(-0.5 * size, 0.5 * size, (N, P, 2)).astype(np.float32)).to(dev)
    th, tn = torch.empty((N, P), dtype=torch.float32, device=dev), torch.empty((N, P, 3), dtype=torch.float32, device=dev)
    t_h = timed(lambda: w.terrain_height(xy, out={"height": th}))
    t_hn = timed(lambda: w.terrain_height(xy, out={"height": th, "normal": tn}))
    org = np.zeros((N, R, 3), np.float32)
    org[..., :2] = gc0[:, None, :2]
    org[..., 2] = 0.9
    ang = np.linspace(-0.6, 0.6, 8)[None, :, None] + rng.uniform(-np.pi, np.pi, (N, 1, 1))
    pitch = np.linspace(-1.2, -0.15, 8)[None, None, :]
    dirs = np.stack([np.cos(ang) * np.cos(pitch), np.sin(ang) * np.cos(pitch), np.broadcast_to(np.sin(pitch), (N, 8, 8))], axis=-1).reshape(N, R, 3).astype(np.float32)
    to, td, tt = torch.from_numpy(org).to(dev), torch.from_numpy(dirs).to(dev), torch.empty((N, R), dtype=torch.float32, device=dev)
    t_ray = timed(lambda: w.ray_test(to, td, 10.0, out=tt))
    hit = float((tt >= 0).float().mean())
    lines += [f"  rsb_get_terrain_height, P = {P} (height)                   {t_h:9.1f} us = {100 * t_h / t_step:5.1f} %",
              f"  rsb_get_terrain_height, P = {P} (height + normal)          {t_hn:9.1f} us = {100 * t_hn / t_step:5.1f} %",
              f"  rsb_ray_test, R = {R} downward-forward rays, max_dist 10 m  {t_ray:9.1f} us = {100 * t_ray / t_step:5.1f} %   ({100 * hit:.0f} % of the rays hit)"]
    w.close()
    print("\n".join(lines), flush=True)
    text = [f"command: python tools/bench_terrain_query.py {' '.join(sys.argv[1:])}".rstrip(),
            f"device-event time per call: {CALLS} calls after {WARM} warm-up calls, median of {WINDOWS} windows; torch CUDA tensors (RSB_DEVICE), the world on torch's stream", ""]
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        f.write("\n".join(text + lines) + "\n")


if __name__ == "__main__":
    main()
