"""Times the batched held-frame queries (rsb_constrained_forward_dynamics, rsb_frame_impulse; csrc/rsb_constrained.hip) at N = 4096, ANYmal-like and
Atlas-like, torch CUDA tensors in and out (RSB_DEVICE: nothing synchronises), through the C-ABI with the pointers made once.  Device-event time around
200 calls after 20 warm-up calls, median of 7 such windows.  Timed: both queries for the four feet (the humanoid: hands and feet) with linear rows
(m = 12) and with RSB_DELASSUS_ANGULAR (m = 24; damping 1e-4: dependent on the quadruped).  Next to them, in the same process, the route a user has without them:
rsb_forward_dynamics + rsb_get_frame_accelerations + rsb_get_frame_delassus, then in torch the damping, torch.linalg.cholesky_ex, torch.cholesky_solve
and a bmm for JMinv^T lambda.  If torch's batched Cholesky does not run on the machine the file says so and reports the three library calls alone.
Each model runs in a child process of its own under a time limit, and the tool stops at the first failure.
Writes profiles/constrained_bench.txt (--out PATH to write elsewhere).  There is no pass / fail threshold.  A tool, not part of bench.py."""
import ctypes as C
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bench_inverse_mass import CALLS, N, WARM, WINDOWS, timed      # noqa: E402  (the same windows as the sibling tool)

CASES = (("ANYmal-like", 2), ("Atlas-like", 5))
LIMIT = 240      # seconds per model
DAMPING = 1e-4


def case(name, config):
    import torch

    import bench
    from raisimlib_amd import BatchedWorld, _capi
    dev = torch.device("cuda:0")
    r = bench.Recipe(config, -1.0)
    model = r.model
    blob = model.blob
    w = BatchedWorld(model, N)
    w.set_stream(torch.cuda.current_stream().cuda_stream)
    r.setup_world(w, N, 0)
    gc0, gv0 = r.initial_state(N, 0)
    w.set_state(gc0, gv0)
    nv, nb = model.nv, model.nb
    L, h, D = w.L, w.handle, _capi.RSB_DEVICE
    feet = [(int(blob.col_body[s]), tuple(float(x) for x in blob.col_pos[s])) for s in list(r.feet)[:4]]
    if len({b for b, _ in feet}) < 4:      # (the humanoid's foot primitives share two bodies: its hands and feet instead, the last four bodies without children)
        leaves = [i for i in range(nb) if i not in set(blob.parent[:nb])]
        feet = [(i, (0.0, 0.0, -0.05)) for i in leaves[-4:]]
    fr, F = w._frames(feet)
    gen = torch.Generator(device=dev); gen.manual_seed(1)
    new = lambda *shape, dtype=torch.float32: torch.empty(shape, dtype=dtype, device=dev)
    tau = torch.randn((N, nv), dtype=torch.float32, device=dev, generator=gen)
    p = lambda t: C.c_void_p(t.data_ptr())
    ck = _capi.check
    lines = [f"{name}: N = {N}, {nb} bodies, nv = {nv}, four frames"]
    for flags, kk, damping in ((0, 3, 0.0), (_capi.RSB_DELASSUS_ANGULAR, 6, DAMPING)):
        m = kk * F
        udot, lam, st, dgv = new(N, nv), new(N, m), new(N, dtype=torch.int32), new(N, nv)
        uf, lin, ang, G, JM = new(N, nv), new(N, F, 3), new(N, F, 3), new(N, m, m), new(N, m, nv)
        t_c = timed(lambda: ck(L.rsb_constrained_forward_dynamics(h, p(tau), fr, F, flags, None, damping, p(udot), p(lam), p(st), D), "rsb_constrained_forward_dynamics"))
        solved = int((st == 0).sum().item())
        t_i = timed(lambda: ck(L.rsb_frame_impulse(h, fr, F, flags, None, None, damping, p(dgv), p(lam), p(st), D), "rsb_frame_impulse"))

        def library_calls():
            ck(L.rsb_forward_dynamics(h, p(tau), None, 0, None, None, 0, p(uf), D), "rsb_forward_dynamics")
            ck(L.rsb_get_frame_accelerations(h, fr, F, p(uf), 0, p(lin), p(ang) if kk == 6 else None, D), "rsb_get_frame_accelerations")
            ck(L.rsb_get_frame_delassus(h, fr, F, flags, None, p(G), p(JM), D), "rsb_get_frame_delassus")

        def torch_route():
            library_calls()
            a = torch.cat([lin, ang], dim=2).reshape(N, m, 1) if kk == 6 else lin.reshape(N, m, 1)
            rho = damping * torch.diagonal(G, dim1=1, dim2=2).amax(dim=1)
            A = G + rho[:, None, None] * torch.eye(m, device=dev)
            Lc, info = torch.linalg.cholesky_ex(A)
            x = torch.cholesky_solve(-a, Lc)
            return uf + torch.bmm(JM.transpose(1, 2), x).squeeze(2), info      # (the caller still has to look at info: a synchronisation)
        t_l = timed(library_calls)
        try:
            got, _ = torch_route()
            torch.cuda.synchronize()
            t_t = timed(torch_route)
            ck(L.rsb_constrained_forward_dynamics(h, p(tau), fr, F, flags, None, damping, p(udot), p(lam), p(st), D), "rsb_constrained_forward_dynamics")
            diff = float((got - udot).abs().max().item())
            route = f"{t_t:9.1f} us ({t_t / t_c:4.1f} x; max |udot - the query's| {diff:.1e})"
        except Exception as e:      # torch's batched Cholesky is not available here
            route = f"torch.linalg.cholesky_ex did not run on this machine ({type(e).__name__}); the three library calls alone: {t_l:9.1f} us"
        lines += [f"  m = {m:2d} ({'angular, damping 1e-4' if kk == 6 else 'linear, no damping'}): {solved} of {N} envs solved",
                  f"    rsb_constrained_forward_dynamics (udot, lambda, status)      {t_c:9.1f} us",
                  f"    rsb_frame_impulse (dgv, lambda, status)                      {t_i:9.1f} us",
                  f"    rsb_forward_dynamics + rsb_get_frame_accelerations + rsb_get_frame_delassus alone {t_l:9.1f} us",
                  f"    ... + torch: damping, cholesky_ex, cholesky_solve, bmm       {route}"]
    w.close()
    print("\n".join(lines), flush=True)


def main():
    if "--case" in sys.argv:      # the child: one model
        i = int(sys.argv[sys.argv.index("--case") + 1])
        case(*CASES[i])
        return 0
    out = os.path.join(ROOT, "profiles", "constrained_bench.txt")
    if "--out" in sys.argv:
        out = sys.argv[sys.argv.index("--out") + 1]
    text = ["command: python tools/bench_constrained.py",
            f"device-event time per call: {CALLS} calls after {WARM} warm-up calls, median of {WINDOWS} windows; torch CUDA tensors (RSB_DEVICE), the world on torch's stream;",
            "the C-ABI with the pointers made once; a query is four kernels: aba_kernel (or none), frame_accel_kernel (frame_kinematics_kernel), delassus_kernel, held_solve_kernel", ""]
    for i in range(len(CASES)):
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--case", str(i)], capture_output=True, text=True, timeout=LIMIT)
        if r.returncode != 0:
            print(r.stdout + r.stderr)
            print(f"bench_constrained: {CASES[i][0]} failed with status {r.returncode}; stopping, nothing written")
            return 1
        print(r.stdout, end="")
        text += [r.stdout.rstrip(), ""]
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        f.write("\n".join(text))
    return 0


if __name__ == "__main__":
    sys.exit(main())
