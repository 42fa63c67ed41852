"""Times batched inverse kinematics (rsb_inverse_kinematics; csrc/rsb_ik.hip) at N = 4096, ANYmal-like (the four feet) and Atlas-like (hands and
feet), torch CUDA tensors in and out (RSB_DEVICE: nothing synchronises), through the C-ABI with the pointers made once.  Device-event time around 200
calls after 20 warm-up calls, median of 7 such windows (tools/bench_inverse_mass.timed).  The targets are the frames' places at joint angles up to
0.2 rad away from the start, the base held, max_iter 30, damping 1e-3, max_step 0.5, tolerances 1e-4: position rows (m = 12), and position and
orientation rows (m = 24).  Next to the position rows, in the same process, the composition a caller has today, for the number of steps K the
slowest env of the call took: per step rsb_set_state (the iterate has to be resident), rsb_get_frame_kinematics, rsb_get_frame_jacobians, then in
torch the rows, J J^T + rho I, torch.linalg.cholesky_ex, torch.cholesky_solve, J^T y, the clip and the update.  If torch's batched Cholesky does not
run on the machine the file says so and reports the library calls of the K steps alone.  Each model runs in a child process of its own under a time
limit, and the tool stops at the first failure.
Writes profiles/ik_bench.txt (--out PATH to write elsewhere).  There is no pass / fail threshold.  A tool, not part of bench.py."""
import ctypes as C
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bench_inverse_mass import CALLS, N, WARM, WINDOWS, timed      # noqa: E402  (the same windows as the sibling tools)

CASES = (("ANYmal-like", 2), ("Atlas-like", 5))
LIMIT = 400      # seconds per model
MAX_ITER, DAMPING, POS_TOL, ROT_TOL, MAX_STEP = 30, 1e-3, 1e-4, 1e-4, 0.5


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
    nv, nq, nb = model.nv, model.nq, model.nb
    L, h, D = w.L, w.handle, _capi.RSB_DEVICE
    feet = [(int(blob.col_body[s]), tuple(float(x) for x in blob.col_pos[s])) for s in list(r.feet)[:4]]
    if len({b for b, _ in feet}) < 4:      # (the humanoid's foot primitives share two bodies: its hands and feet instead, the last four bodies without children)
        leaves = [i for i in range(nb) if i not in set(blob.parent[:nb])]
        feet = [(i, (0.0, 0.0, -0.05)) for i in leaves[-4:]]
    fr, F = w._frames(feet)
    gen = torch.Generator(device=dev); gen.manual_seed(1)
    new = lambda *shape, dtype=torch.float32: torch.empty(shape, dtype=dtype, device=dev)
    p = lambda t: C.c_void_p(t.data_ptr())
    ck = _capi.check
    q0 = torch.from_numpy(gc0.astype("float32")).to(dev).contiguous()
    u0 = torch.from_numpy(gv0.astype("float32")).to(dev).contiguous()
    moved = q0.clone()
    moved[:, 7:] += 0.4 * torch.rand((N, nq - 7), device=dev, generator=gen) - 0.2
    tpos, trot = new(N, F, 3), new(N, F, 9)
    ck(L.rsb_set_state(h, p(moved), p(u0), None, D), "rsb_set_state")
    ck(L.rsb_get_frame_kinematics(h, fr, F, p(tpos), p(trot), None, None, D), "rsb_get_frame_kinematics")
    ck(L.rsb_set_state(h, p(q0), p(u0), None, D), "rsb_set_state")
    opt = _capi.IkOptions(MAX_ITER, DAMPING, POS_TOL, ROT_TOL, MAX_STEP)
    gc, err, its, st = new(N, nq), new(N, 2), new(N, dtype=torch.int32), new(N, dtype=torch.int32)
    lines = [f"{name}: N = {N}, {nb} bodies, nv = {nv}, four frames, the base held"]
    for flags, kk in ((0, 3), (_capi.RSB_IK_ANGULAR, 6)):
        m = kk * F
        call = lambda: ck(L.rsb_inverse_kinematics(h, fr, F, flags, p(tpos), p(trot) if kk == 6 else None, None, None, C.byref(opt), p(gc), p(err), p(its), p(st), D),
                          "rsb_inverse_kinematics")
        t_k = timed(call)
        torch.cuda.synchronize()
        K, mean_k, conv = int(its.max().item()), float(its.float().mean().item()), int((st == 0).sum().item())
        lines += [f"  m = {m:2d} ({'position and orientation' if kk == 6 else 'position'} rows): {conv} of {N} envs converged, steps: mean {mean_k:.2f}, most {K}",
                  f"    rsb_inverse_kinematics (gc, error, iterations, status)        {t_k:9.1f} us"]
        if kk == 6:
            continue
        q, pos, Jl = q0.clone(), new(N, F, 3), new(N, m, nv)
        eye = torch.eye(m, device=dev)

        def library_calls():
            ck(L.rsb_set_state(h, p(q), None, None, D), "rsb_set_state")
            ck(L.rsb_get_frame_kinematics(h, fr, F, p(pos), None, None, None, D), "rsb_get_frame_kinematics")
            ck(L.rsb_get_frame_jacobians(h, fr, F, p(Jl), None, D), "rsb_get_frame_jacobians")

        def library_only():
            for _ in range(K):
                library_calls()

        def torch_route():
            q.copy_(q0)
            for _ in range(K):
                library_calls()
                e = (tpos - pos).reshape(N, m, 1)
                J = Jl[:, :, 6:]
                A = torch.bmm(J, J.transpose(1, 2))
                rho = DAMPING * torch.diagonal(A, dim1=1, dim2=2).amax(dim=1)
                Lc, info = torch.linalg.cholesky_ex(A + rho[:, None, None] * eye)
                dq = torch.bmm(J.transpose(1, 2), torch.cholesky_solve(e, Lc)).squeeze(2)
                s = dq.abs().amax(dim=1, keepdim=True)
                q[:, 7:] += dq * torch.where(s > MAX_STEP, MAX_STEP / s, torch.ones_like(s))
            return q      # (no per-env stop: converged envs keep stepping; looking at info or at the rows would be a synchronisation)
        t_l = timed(library_only)
        try:
            got = torch_route().clone()
            torch.cuda.synchronize()
            t_t = timed(torch_route)
            call()
            diff = float((got - gc).abs().max().item())
            route = f"{t_t:9.1f} us ({t_t / t_k:4.1f} x; max |gc - the query's| {diff:.1e})"
        except Exception as e:      # torch's batched Cholesky is not available here
            route = f"torch.linalg.cholesky_ex did not run on this machine ({type(e).__name__}); the library calls alone: {t_l:9.1f} us"
        ck(L.rsb_set_state(h, p(q0), None, None, D), "rsb_set_state")
        lines += [f"    {K} x (rsb_set_state + rsb_get_frame_kinematics + rsb_get_frame_jacobians) alone {t_l:9.1f} us",
                  f"    ... + torch per step: rows, J J^T + rho I, cholesky_ex, cholesky_solve, J^T y, clip, update   {route}"]
    w.close()
    print("\n".join(lines), flush=True)


def main():
    if "--case" in sys.argv:      # the child: one model
        i = int(sys.argv[sys.argv.index("--case") + 1])
        case(*CASES[i])
        return 0
    out = os.path.join(ROOT, "profiles", "ik_bench.txt")
    if "--out" in sys.argv:
        out = sys.argv[sys.argv.index("--out") + 1]
    text = ["command: python tools/bench_ik.py",
            f"device-event time per call: {CALLS} calls after {WARM} warm-up calls, median of {WINDOWS} windows; torch CUDA tensors (RSB_DEVICE), the world on torch's stream;",
            f"the C-ABI with the pointers made once; a query is one kernel, ik_kernel; max_iter {MAX_ITER}, damping {DAMPING}, max_step {MAX_STEP}, tolerances {POS_TOL}", ""]
    for i in range(len(CASES)):
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--case", str(i)], capture_output=True, text=True, timeout=LIMIT)
        if r.returncode != 0:
            print(r.stdout + r.stderr)
            print(f"bench_ik: {CASES[i][0]} failed with status {r.returncode}; stopping, nothing written")
            return 1
        print(r.stdout, end="")
        text += [r.stdout.rstrip(), ""]
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        f.write("\n".join(text))
    return 0


if __name__ == "__main__":
    sys.exit(main())
