"""Times the batched dynamics queries (rsb_inverse_dynamics, rsb_forward_dynamics; csrc/rsb_dynamics.hip) at N = 4096, ANYmal-like and Atlas-like,
torch CUDA tensors in and out (RSB_DEVICE: nothing synchronises), through the C-ABI with the pointers made once.  Device-event time around 200 calls
after 20 warm-up calls, median of 7 such windows.  Timed: tau alone with udot = NULL; tau with udot; all three outputs with the contact list; forward
dynamics.  Yardsticks, in the same process: one lock-step rsb_control_step of the same world; what a user had to write before - rsb_integrate1 +
rsb_get_nonlinearities (h alone), + rsb_get_mass_matrix and M @ udot + h in torch (inverse dynamics), torch.linalg.solve(M, tau - h) (forward dynamics).
Each model runs in a child process of its own under a time limit, and the tool stops at the first failure.
Writes profiles/r12_dynamics_bench.txt (--out PATH to write elsewhere).  There is no pass / fail threshold.  A tool, not part of bench.py."""
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
    t_step = timed(control_step)      # (also brings the world into the benchmark's stationary mix of states, with contacts)
    nv, nb = model.nv, model.nb
    L, h, D = w.L, w.handle, _capi.RSB_DEVICE
    gen = torch.Generator(device=dev); gen.manual_seed(1)
    udot = torch.randn((N, nv), dtype=torch.float32, device=dev, generator=gen)
    tin = torch.randn((N, nv), dtype=torch.float32, device=dev, generator=gen)
    tau, acc = torch.empty_like(udot), torch.empty_like(udot)
    jf, jt = (torch.empty((N, nb, 3), dtype=torch.float32, device=dev) for _ in range(2))
    p = lambda t: C.c_void_p(t.data_ptr())
    pu, pi, pt, pa, pf, pn = p(udot), p(tin), p(tau), p(acc), p(jf), p(jt)
    ck = _capi.check
    t_h = timed(lambda: ck(L.rsb_inverse_dynamics(h, None, None, 0, None, None, 0, pt, None, None, D), "rsb_inverse_dynamics"))
    t_id = timed(lambda: ck(L.rsb_inverse_dynamics(h, pu, None, 0, None, None, 0, pt, None, None, D), "rsb_inverse_dynamics"))
    t_all = timed(lambda: ck(L.rsb_inverse_dynamics(h, pu, None, 0, None, None, _capi.RSB_DYN_CONTACTS, pt, pf, pn, D), "rsb_inverse_dynamics"))
    t_fd = timed(lambda: ck(L.rsb_forward_dynamics(h, pi, None, 0, None, None, 0, pa, D), "rsb_forward_dynamics"))
    t_py = timed(lambda: w.inverse_dynamics(udot, out={"tau": tau}))
    M = torch.empty((N, nv, nv), dtype=torch.float32, device=dev)
    hh = torch.empty((N, nv), dtype=torch.float32, device=dev)
    pM, ph = p(M), p(hh)

    def old_h():
        ck(L.rsb_integrate1(h), "rsb_integrate1")
        ck(L.rsb_get_nonlinearities(h, ph, D), "rsb_get_nonlinearities")

    def old_id():
        old_h()
        ck(L.rsb_get_mass_matrix(h, pM, D), "rsb_get_mass_matrix")
        return torch.baddbmm(hh[:, :, None], M, udot[:, :, None])

    def old_fd():
        old_h()
        ck(L.rsb_get_mass_matrix(h, pM, D), "rsb_get_mass_matrix")
        return torch.linalg.solve(M, tin - hh)
    t_oh, t_oid, t_ofd = timed(old_h), timed(old_id), timed(old_fd)
    w.close()
    pct = lambda t: f"{100 * t / t_step:5.1f} % of a control step"
    lines = [f"{name}: N = {N}, {nb} bodies, nv = {nv}, tree depth {model.blob.depth}, {256 // nb} envs per workgroup",
             f"  rsb_control_step (lock-step, {workload.SUBSTEPS} sub-steps)                    {t_step:9.1f} us",
             f"  rsb_inverse_dynamics, tau, udot = NULL (= h)                  {t_h:9.1f} us = {pct(t_h)}",
             f"  rsb_inverse_dynamics, tau, with udot                          {t_id:9.1f} us = {pct(t_id)}",
             f"  rsb_inverse_dynamics, tau + joint wrenches, with contacts     {t_all:9.1f} us = {pct(t_all)}",
             f"  rsb_forward_dynamics                                          {t_fd:9.1f} us = {pct(t_fd)}",
             f"  BatchedWorld.inverse_dynamics(udot, out={{'tau': ..}})           {t_py:9.1f} us   (the gap to the C-ABI line is host time of the Python mirror)",
             f"  before: rsb_integrate1 + rsb_get_nonlinearities               {t_oh:9.1f} us = {pct(t_oh)}",
             f"  before: ... + rsb_get_mass_matrix, M @ udot + h in torch      {t_oid:9.1f} us = {pct(t_oid)}   ({N * nv * nv * 4 / 1e6:.1f} MB of M)",
             f"  before: ... + torch.linalg.solve(M, tau - h)                  {t_ofd:9.1f} us = {pct(t_ofd)}"]
    print("\n".join(lines), flush=True)


def main():
    if "--case" in sys.argv:      # the child: one model
        i = int(sys.argv[sys.argv.index("--case") + 1])
        case(*CASES[i])
        return 0
    out = os.path.join(ROOT, "profiles", "r12_dynamics_bench.txt")
    if "--out" in sys.argv:
        out = sys.argv[sys.argv.index("--out") + 1]
    text = ["command: python tools/bench_dynamics.py",
            f"device-event time per call: {CALLS} calls after {WARM} warm-up calls, median of {WINDOWS} windows; torch CUDA tensors (RSB_DEVICE), the world on torch's stream;",
            "the C-ABI with the pointers made once unless a line says otherwise", ""]
    for i in range(len(CASES)):
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--case", str(i)], capture_output=True, text=True, timeout=LIMIT)
        if r.returncode != 0:
            print(r.stdout + r.stderr)
            print(f"bench_dynamics: {CASES[i][0]} failed with status {r.returncode}; stopping, nothing written")
            return 1
        print(r.stdout, end="")
        text += [r.stdout.rstrip(), ""]
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        f.write("\n".join(text))
    return 0


if __name__ == "__main__":
    sys.exit(main())
