"""Times the batched whole-body queries (rsb_get_centroidal, rsb_get_centroidal_momentum_matrix; csrc/rsb_centroidal.hip) at N = 4096, ANYmal-like and
Atlas-like, torch CUDA tensors out (RSB_DEVICE: nothing synchronises).  Device-event time around 200 calls after 20 warm-up calls, median of 7 such
windows.  For scale, in the same process: the lock-step rsb_control_step of the same world (what a control step costs), and the composition a user
would have written in torch before these entry points existed - rsb_integrate1, rsb_get_mass_matrix into a [N, nv, nv] tensor, rsb_get_field(GV), and
the six base rows of M times gv (the momentum about the base origin; the centre of mass and the energies are not even in it).
Writes profiles/r11_centroidal_bench.txt (--out PATH to write elsewhere).  There is no pass / fail threshold.  A tool, not part of bench.py."""
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

import bench
from raisimlib_amd import BatchedWorld, _capi, workload

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


def case(name, config):
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
    nv = model.nv
    out = {n: torch.empty((N, 3), dtype=torch.float32, device=dev) for n in ("com", "com_vel", "lin_mom", "ang_mom")}
    out.update({n: torch.empty((N,), dtype=torch.float32, device=dev) for n in ("kinetic", "potential")})
    A = torch.empty((N, 6, nv), dtype=torch.float32, device=dev)
    t_all = timed(lambda: w.centroidal(out=out))
    t_com = timed(lambda: w.centroidal(out={"com": out["com"]}))
    t_mat = timed(lambda: w.centroidal_momentum_matrix(out=A))
    # the same calls through the C-ABI with the pointers made once: without the Python mirror's per-tensor argument checks, which bound the enqueue rate
    L, h = w.L, w.handle
    ptr = [C.c_void_p(out[n].data_ptr()) for n in ("com", "com_vel", "lin_mom", "ang_mom", "kinetic", "potential")]
    pA = C.c_void_p(A.data_ptr())
    c_all = timed(lambda: L.rsb_get_centroidal(h, *ptr, _capi.RSB_DEVICE))
    c_com = timed(lambda: L.rsb_get_centroidal(h, ptr[0], None, None, None, None, None, _capi.RSB_DEVICE))
    c_mat = timed(lambda: L.rsb_get_centroidal_momentum_matrix(h, pA, _capi.RSB_DEVICE))
    M = torch.empty((N, nv, nv), dtype=torch.float32, device=dev)
    gv = torch.empty((N, nv), dtype=torch.float32, device=dev)
    pM, pv = C.c_void_p(M.data_ptr()), C.c_void_p(gv.data_ptr())

    def torch_composition():
        _capi.check(L.rsb_integrate1(h), "rsb_integrate1")
        _capi.check(L.rsb_get_mass_matrix(h, pM, _capi.RSB_DEVICE), "rsb_get_mass_matrix")
        _capi.check(L.rsb_get_field(h, _capi.RSB_F_GV, pv, _capi.RSB_DEVICE), "rsb_get_field")
        return torch.bmm(M[:, :6, :], gv[:, :, None])
    t_torch = timed(torch_composition)
    w.close()
    kb = N * (model.nq + nv) * 4 / 1e3
    lines = [f"{name}: N = {N}, {model.nb} bodies, nv = {nv}, tree depth {model.blob.depth}, {256 // model.nb} envs per workgroup",
             f"  rsb_control_step (lock-step, {workload.SUBSTEPS} sub-steps)            {t_step:9.1f} us",
             f"  rsb_get_centroidal (all six outputs)                  {t_all:9.1f} us = {100 * t_all / t_step:5.1f} % of a control step   (reads {kb:.0f} kB, writes {N * 14 * 4 / 1e3:.0f} kB)",
             f"  rsb_get_centroidal (com only)                         {t_com:9.1f} us = {100 * t_com / t_step:5.1f} %",
             f"  rsb_get_centroidal_momentum_matrix                    {t_mat:9.1f} us = {100 * t_mat / t_step:5.1f} %   (writes {N * 6 * nv * 4 / 1e6:.1f} MB)",
             f"  the same three through the C-ABI, pointers made once   {c_all:9.1f} us / {c_com:.1f} us / {c_mat:.1f} us   (the gap to the lines above is host time of the Python mirror: a window of back-to-back calls measures the slower of enqueue and device)",
             f"  torch: integrate1 + mass matrix + gv + M[:, :6] @ gv  {t_torch:9.1f} us = {100 * t_torch / t_step:5.1f} %   (momentum about the base origin only; {N * nv * nv * 4 / 1e6:.1f} MB of M)"]
    print("\n".join(lines), flush=True)
    return lines


def main():
    out = os.path.join(ROOT, "profiles", "r11_centroidal_bench.txt")
    if "--out" in sys.argv:
        out = sys.argv[sys.argv.index("--out") + 1]
    text = [f"command: python tools/bench_centroidal.py {' '.join(sys.argv[1:])}".rstrip(),
            f"device-event time per call: {CALLS} calls after {WARM} warm-up calls, median of {WINDOWS} windows; torch CUDA tensors (RSB_DEVICE), the world on torch's stream", ""]
    text += case("ANYmal-like", 2) + [""]
    text += case("Atlas-like", 5)
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        f.write("\n".join(text) + "\n")


if __name__ == "__main__":
    main()
