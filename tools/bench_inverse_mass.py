"""Times the batched inverse-mass queries (rsb_apply_inverse_mass, rsb_get_frame_delassus; csrc/rsb_inverse_mass.hip) at N = 4096, ANYmal-like and
Atlas-like, torch CUDA tensors in and out (RSB_DEVICE: nothing synchronises), through the C-ABI with the pointers made once.  Device-event time around
200 calls after 20 warm-up calls, median of 7 such windows.  Timed: the solve with R = 1, R = 12 and R = nv right-hand sides; the Delassus matrix of
the four feet (12 x 12, G alone and G + JMinv) and of four frames with RSB_DELASSUS_ANGULAR (24 x 24).  Yardsticks, in the same process: one
rsb_forward_dynamics; what a user had to write before - rsb_integrate1 + rsb_get_inverse_mass_matrix (the dense [N, nv, nv] slow path), then
torch.bmm for the solve, or rsb_get_frame_jacobians and two torch.bmm for J M^-1 J^T.
Each model runs in a child process of its own under a time limit, and the tool stops at the first failure.
Writes profiles/inverse_mass_bench.txt (--out PATH to write elsewhere).  There is no pass / fail threshold.  A tool, not part of bench.py."""
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
    feet += [(nb - 1 - k, (0.0, 0.0, 0.0)) for k in range(4 - len(feet))]
    fr, F = w._frames(feet)
    gen = torch.Generator(device=dev); gen.manual_seed(1)
    new = lambda *shape: torch.empty(shape, dtype=torch.float32, device=dev)
    B = {R: torch.randn((N, R, nv), dtype=torch.float32, device=dev, generator=gen) for R in (1, 12, nv)}
    X = {R: torch.empty_like(b) for R, b in B.items()}
    tin, acc = torch.randn((N, nv), dtype=torch.float32, device=dev, generator=gen), new(N, nv)
    G3, JM3, G6, JM6 = new(N, 12, 12), new(N, 12, nv), new(N, 24, 24), new(N, 24, nv)
    p = lambda t: C.c_void_p(t.data_ptr())
    ck = _capi.check
    t_fd = timed(lambda: ck(L.rsb_forward_dynamics(h, p(tin), None, 0, None, None, 0, p(acc), D), "rsb_forward_dynamics"))
    t_x = {R: timed(lambda R=R: ck(L.rsb_apply_inverse_mass(h, p(B[R]), R, None, p(X[R]), D), "rsb_apply_inverse_mass")) for R in B}
    t_g = timed(lambda: ck(L.rsb_get_frame_delassus(h, fr, F, 0, None, p(G3), None, D), "rsb_get_frame_delassus"))
    t_gj = timed(lambda: ck(L.rsb_get_frame_delassus(h, fr, F, 0, None, p(G3), p(JM3), D), "rsb_get_frame_delassus"))
    t_g6 = timed(lambda: ck(L.rsb_get_frame_delassus(h, fr, F, _capi.RSB_DELASSUS_ANGULAR, None, p(G6), p(JM6), D), "rsb_get_frame_delassus"))
    t_py = timed(lambda: w.frame_delassus(feet, out={"G": G3}))
    Mi, Jl = new(N, nv, nv), new(N, F, 3, nv)

    def old_minv():
        ck(L.rsb_integrate1(h), "rsb_integrate1")
        ck(L.rsb_get_inverse_mass_matrix(h, p(Mi), D), "rsb_get_inverse_mass_matrix")

    def old_solve(R):
        old_minv()
        return torch.bmm(B[R], Mi)      # (M^-1 is symmetric)

    def old_delassus():
        old_minv()
        ck(L.rsb_get_frame_jacobians(h, fr, F, p(Jl), None, D), "rsb_get_frame_jacobians")
        J = Jl.view(N, 3 * F, nv)
        JM = torch.bmm(J, Mi)
        return torch.bmm(JM, J.transpose(1, 2))
    t_om = timed(old_minv)
    t_os = {R: timed(lambda R=R: old_solve(R)) for R in B}
    t_od = timed(old_delassus)
    w.close()
    rel = lambda t: f"{t / t_fd:5.2f} x rsb_forward_dynamics"
    lines = [f"{name}: N = {N}, {nb} bodies, nv = {nv}, tree depth {blob.depth}, {256 // nb} envs per workgroup",
             f"  rsb_forward_dynamics (one right-hand side, re-factors)        {t_fd:9.1f} us"]
    lines += [f"  rsb_apply_inverse_mass, R = {R:2d}                               {t_x[R]:9.1f} us = {rel(t_x[R])}   before: {t_os[R]:9.1f} us ({t_os[R] / t_x[R]:5.1f} x)" for R in B]
    lines += [f"  rsb_get_frame_delassus, four feet, G 12 x 12                  {t_g:9.1f} us = {rel(t_g)}   before: {t_od:9.1f} us ({t_od / t_g:5.1f} x)",
              f"  rsb_get_frame_delassus, four feet, G + JMinv                  {t_gj:9.1f} us = {rel(t_gj)}",
              f"  rsb_get_frame_delassus, four frames, angular, G 24 x 24 + JMinv {t_g6:7.1f} us = {rel(t_g6)}",
              f"  BatchedWorld.frame_delassus(feet, out={{'G': ..}})               {t_py:9.1f} us   (the gap to the C-ABI line is host time of the Python mirror)",
              f"  before: rsb_integrate1 + rsb_get_inverse_mass_matrix alone    {t_om:9.1f} us   ({N * nv * nv * 4 / 1e6:.1f} MB of M^-1)",
              "  (before: ... then torch.bmm(B, M^-1) for a solve; rsb_get_frame_jacobians, torch.bmm(J, M^-1), torch.bmm(., J^T) for G)"]
    print("\n".join(lines), flush=True)


def main():
    if "--case" in sys.argv:      # the child: one model
        i = int(sys.argv[sys.argv.index("--case") + 1])
        case(*CASES[i])
        return 0
    out = os.path.join(ROOT, "profiles", "inverse_mass_bench.txt")
    if "--out" in sys.argv:
        out = sys.argv[sys.argv.index("--out") + 1]
    text = ["command: python tools/bench_inverse_mass.py",
            f"device-event time per call: {CALLS} calls after {WARM} warm-up calls, median of {WINDOWS} windows; torch CUDA tensors (RSB_DEVICE), the world on torch's stream;",
            "the C-ABI with the pointers made once unless a line says otherwise; one column per pass over the tree (2 (depth - 1) barriers per column, + 1 for G)", ""]
    for i in range(len(CASES)):
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--case", str(i)], capture_output=True, text=True, timeout=LIMIT)
        if r.returncode != 0:
            print(r.stdout + r.stderr)
            print(f"bench_inverse_mass: {CASES[i][0]} failed with status {r.returncode}; stopping, nothing written")
            return 1
        print(r.stdout, end="")
        text += [r.stdout.rstrip(), ""]
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        f.write("\n".join(text))
    return 0


if __name__ == "__main__":
    sys.exit(main())
