"""Times the batched dynamics derivatives (rsb_inverse_dynamics_derivatives, rsb_forward_dynamics_derivatives; csrc/rsb_dynamics_derivatives.hip) at
N = 4096, ANYmal-like and Atlas-like, torch CUDA tensors in and out (RSB_DEVICE: nothing synchronises), through the C-ABI with the pointers made once.
Device-event time around 20 calls after 3 warm-up calls, median of 5 such windows.  Timed: each matrix of the inverse form alone and the three
together; the forward form with dudot_dq + dudot_dv, and with all four outputs.  Yardsticks, in the same process: rsb_inverse_dynamics and
rsb_forward_dynamics themselves, and what a user had to write before for ONE matrix, dtau_dq - 2 nv central-difference evaluations through
rsb_set_state + rsb_inverse_dynamics and the state restored afterwards, with the 2 nv perturbed configurations (quaternion products included) made
once outside the timed region and the differences left untaken: the floor of that route.
Each model runs in a child process of its own under a time limit, and the tool stops at the first failure.
Writes profiles/dynamics_derivatives_bench.txt (--out PATH to write elsewhere).  There is no pass / fail threshold.  A tool, not part of bench.py."""
import ctypes as C
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N, CALLS, WARM, WINDOWS = 4096, 20, 3, 5
CASES = (("ANYmal-like", 2), ("Atlas-like", 5))
LIMIT = 240      # seconds per model
EPS = 1e-3


def timed(fn, calls=CALLS):
    """median over WINDOWS windows of the device-event time of `calls` calls, in microseconds per call"""
    import numpy as np
    import torch
    for _ in range(WARM):
        fn()
    per = []
    for _ in range(WINDOWS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(calls):
            fn()
        e1.record()
        e1.synchronize()
        per.append(e0.elapsed_time(e1) * 1e3 / calls)
    return float(np.median(per))


def perturbed(gc, nv):
    """the 2 nv configurations gc (+) (+-EPS e_j) under the retraction of rsb.h, [2 nv, N, nq]"""
    import torch
    out = []
    for j in range(nv):
        for s in (EPS, -EPS):
            q = gc.clone()
            if j < 3:
                q[:, j] += s
            elif j < 6:
                a = torch.zeros(4, dtype=gc.dtype, device=gc.device)
                a[0], a[1 + j - 3] = float(torch.cos(torch.tensor(s / 2))), float(torch.sin(torch.tensor(s / 2)))
                b = gc[:, 3:7]
                q[:, 3] = a[0] * b[:, 0] - (a[1:] * b[:, 1:]).sum(1)
                q[:, 4:7] = a[0] * b[:, 1:] + b[:, :1] * a[1:] + torch.linalg.cross(a[1:].expand_as(b[:, 1:]), b[:, 1:])
            else:
                q[:, 7 + j - 6] += s
            out.append(q)
    return torch.stack(out)


def case(name, config):
    import numpy as np
    import torch

    import bench
    from raisimlib_amd import BatchedWorld, _capi
    dev = torch.device("cuda:0")
    r = bench.Recipe(config, -1.0)
    model = r.model
    w = BatchedWorld(model, N)
    w.set_stream(torch.cuda.current_stream().cuda_stream)
    r.setup_world(w, N, 0)
    gc0, gv0 = r.initial_state(N, 0)
    w.set_state(gc0, gv0)
    nv, nb = model.nv, model.nb
    L, h, D = w.L, w.handle, _capi.RSB_DEVICE
    gen = torch.Generator(device=dev); gen.manual_seed(1)
    udot = torch.randn((N, nv), dtype=torch.float32, device=dev, generator=gen)
    tin = torch.randn((N, nv), dtype=torch.float32, device=dev, generator=gen)
    tau, acc = torch.empty_like(udot), torch.empty_like(udot)
    A, B, Cm = (torch.empty((N, nv, nv), dtype=torch.float32, device=dev) for _ in range(3))
    p = lambda t: C.c_void_p(t.data_ptr())
    pu, pi, pt, pa, pA, pB, pC = p(udot), p(tin), p(tau), p(acc), p(A), p(B), p(Cm)
    ck = _capi.check
    ID, FD = L.rsb_inverse_dynamics_derivatives, L.rsb_forward_dynamics_derivatives
    who_i, who_f = "rsb_inverse_dynamics_derivatives", "rsb_forward_dynamics_derivatives"
    t_id = timed(lambda: ck(L.rsb_inverse_dynamics(h, pu, None, 0, None, None, 0, pt, None, None, D), "rsb_inverse_dynamics"))
    t_fd = timed(lambda: ck(L.rsb_forward_dynamics(h, pi, None, 0, None, None, 0, pa, D), "rsb_forward_dynamics"))
    t_q = timed(lambda: ck(ID(h, pu, None, 0, None, None, 0, pA, None, None, D), who_i))
    t_v = timed(lambda: ck(ID(h, pu, None, 0, None, None, 0, None, pB, None, D), who_i))
    t_a = timed(lambda: ck(ID(h, pu, None, 0, None, None, 0, None, None, pC, D), who_i))
    t_3 = timed(lambda: ck(ID(h, pu, None, 0, None, None, 0, pA, pB, pC, D), who_i))
    t_f2 = timed(lambda: ck(FD(h, pi, None, 0, None, None, 0, None, pA, pB, None, D), who_f))
    t_f4 = timed(lambda: ck(FD(h, pi, None, 0, None, None, 0, pa, pA, pB, pC, D), who_f))
    g0 = torch.from_numpy(np.ascontiguousarray(gc0, np.float32)).to(dev)
    v0 = torch.from_numpy(np.ascontiguousarray(gv0, np.float32)).to(dev)
    bank = perturbed(g0, nv)
    cols = torch.empty((2 * nv, N, nv), dtype=torch.float32, device=dev)
    pg, pv = p(g0), p(v0)
    pq = [C.c_void_p(bank[k].data_ptr()) for k in range(2 * nv)]
    pc = [C.c_void_p(cols[k].data_ptr()) for k in range(2 * nv)]

    def differences():
        for k in range(2 * nv):
            ck(L.rsb_set_state(h, pq[k], pv, None, D), "rsb_set_state")
            ck(L.rsb_inverse_dynamics(h, pu, None, 0, None, None, 0, pc[k], None, None, D), "rsb_inverse_dynamics")
        ck(L.rsb_set_state(h, pg, pv, None, D), "rsb_set_state")
    t_old = timed(differences, calls=3)
    w.close()
    lines = [f"{name}: N = {N}, {nb} bodies, nv = {nv}, tree depth {model.blob.depth}, {256 // nb} envs per workgroup, {N * nv * nv * 4 / 1e6:.1f} MB per matrix",
             f"  rsb_inverse_dynamics, tau, with udot                                  {t_id:10.1f} us",
             f"  rsb_forward_dynamics                                                  {t_fd:10.1f} us",
             f"  rsb_inverse_dynamics_derivatives, dtau_dq alone                       {t_q:10.1f} us",
             f"  rsb_inverse_dynamics_derivatives, dtau_dv alone                       {t_v:10.1f} us",
             f"  rsb_inverse_dynamics_derivatives, dtau_dudot alone                    {t_a:10.1f} us",
             f"  rsb_inverse_dynamics_derivatives, all three                           {t_3:10.1f} us",
             f"  rsb_forward_dynamics_derivatives, dudot_dq + dudot_dv                 {t_f2:10.1f} us",
             f"  rsb_forward_dynamics_derivatives, udot + all three                    {t_f4:10.1f} us",
             f"  before: dtau_dq by {2 * nv} x (rsb_set_state + rsb_inverse_dynamics) + restore  {t_old:10.1f} us = {t_old / t_q:.2f} x dtau_dq alone"]
    print("\n".join(lines), flush=True)


def main():
    if "--case" in sys.argv:      # the child: one model
        i = int(sys.argv[sys.argv.index("--case") + 1])
        case(*CASES[i])
        return 0
    out = os.path.join(ROOT, "profiles", "dynamics_derivatives_bench.txt")
    if "--out" in sys.argv:
        out = sys.argv[sys.argv.index("--out") + 1]
    text = ["command: python tools/bench_dynamics_derivatives.py",
            f"device-event time per call: {CALLS} calls after {WARM} warm-up calls, median of {WINDOWS} windows (the difference route: 3 calls per window);",
            "torch CUDA tensors (RSB_DEVICE), the world on torch's stream; the C-ABI with the pointers made once", ""]
    for i in range(len(CASES)):
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--case", str(i)], capture_output=True, text=True, timeout=LIMIT)
        if r.returncode != 0:
            print(r.stdout + r.stderr)
            print(f"bench_dynamics_derivatives: {CASES[i][0]} failed with status {r.returncode}; stopping, nothing written")
            return 1
        print(r.stdout, end="")
        text += [r.stdout.rstrip(), ""]
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        f.write("\n".join(text))
    return 0


if __name__ == "__main__":
    sys.exit(main())
