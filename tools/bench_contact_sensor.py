"""Times the batched contact sensors (rsb_get_body_contact_wrenches, rsb_contact_observe, rsb_contact_timers; csrc/rsb_contact_sensor.hip) at
N = 4096, ANYmal-like and Atlas-like, with the feet and with every body as frames, torch CUDA tensors in and out (RSB_DEVICE: nothing synchronises),
through the C-ABI with the pointers made once.  Device-event time around 200 calls after 20 warm-up calls, median of 7 such windows.  Yardsticks, in
the same process: one lock-step rsb_control_step of the same world, rsb_get_frame_kinematics with velocities (the same walk), and the composition the
sensors replace: rsb_get_frame_kinematics for the frame points plus a torch reduction over the resident contact list (rsb_device_ptr(RSB_F_CONTACTS)
viewed as [N, kmax, 12]) giving force, torque, normal force and contact flag per frame.
Each model runs in a child process of its own under a time limit, and the tool stops at the first failure.
Writes profiles/contact_sensor_bench.txt (--out PATH to write elsewhere).  There is no pass / fail threshold.  A tool, not part of bench.py."""
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


class Raw:
    """a device buffer the world owns, for torch.as_tensor"""
    def __init__(self, ptr, shape, typestr):
        self.__cuda_array_interface__ = dict(shape=shape, typestr=typestr, data=(int(ptr), False), version=2)


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
    t_step = timed(control_step)      # (also brings the world into the benchmark's stationary mix of states and contacts)
    nv, nb, b, kmax = model.nv, model.nb, model.blob, w.max_contacts()
    L, h, D = w.L, w.handle, _capi.RSB_DEVICE
    inv_dt = float(np.float32(1.0 / w.get_time_step()))
    con = torch.as_tensor(Raw(w.device_ptr(_capi.RSB_F_CONTACTS), (N, kmax, 12), "<f4"), device=dev)
    cnt = torch.as_tensor(Raw(w.device_ptr(_capi.RSB_F_CONTACT_COUNT), (N,), "<i4"), device=dev)
    slot = torch.arange(kmax, device=dev)
    p = lambda t: C.c_void_p(t.data_ptr())
    ck = _capi.check
    pct = lambda t: f"{100 * t / t_step:5.1f} % of a control step"
    torch.cuda.synchronize()
    lines = [f"{name}: N = {N}, {nb} bodies, nv = {nv}, kmax = {kmax}, {float(cnt.float().mean()):.2f} contacts per env",
             f"  rsb_control_step (lock-step, {workload.SUBSTEPS} sub-steps)                    {t_step:9.1f} us"]
    sets = (("the feet", [(int(b.col_body[s]), tuple(float(x) for x in b.col_pos[s])) for s in feet]), ("every body", [(i, (0.0, 0.0, 0.0)) for i in range(nb)]))
    for label, frames in sets:
        arr, F = w._frames(frames)
        a3 = [torch.empty((N, F, 3), dtype=torch.float32, device=dev) for _ in range(3)]
        count = torch.empty((N, F), dtype=torch.int32, device=dev)
        rows = torch.empty((N, F, 6), dtype=torch.float32, device=dev)
        air, ctime, td = (torch.zeros((N, F), dtype=torch.float32, device=dev) for _ in range(3))
        bodies = torch.tensor([f[0] for f in frames], dtype=torch.int32, device=dev)
        pf, pt, pp, pc, pr = p(a3[0]), p(a3[1]), p(a3[2]), p(count), p(rows)

        def composition():
            ck(L.rsb_get_frame_kinematics(h, arr, F, pp, None, None, None, D), "rsb_get_frame_kinematics")
            own = (con[:, None, :, 10].view(torch.int32) == bodies[None, :, None]) & (slot[None, :] < cnt[:, None])[:, None, :]      # [N, F, kmax]
            f = con[:, :, 6:9] * inv_dt
            force = torch.einsum("nfk,nkc->nfc", own.float(), f)
            lever = con[:, None, :, 0:3] - a3[2][:, :, None, :]
            torque = (torch.cross(lever, f[:, None].expand_as(lever), dim=-1) * own[..., None]).sum(2)
            normal = torch.einsum("nfk,nk->nf", own.float(), (con[:, :, 6:9] * con[:, :, 3:6]).sum(-1) * inv_dt)
            return force, torque, normal, normal > 1.0
        t_kin = timed(lambda: ck(L.rsb_get_frame_kinematics(h, arr, F, None, None, pf, pt, D), "rsb_get_frame_kinematics"))
        t_wr = timed(lambda: ck(L.rsb_get_body_contact_wrenches(h, arr, F, 0, pf, pt, pc, D), "rsb_get_body_contact_wrenches"))
        t_f = timed(lambda: ck(L.rsb_get_body_contact_wrenches(h, arr, F, 0, pf, None, None, D), "rsb_get_body_contact_wrenches"))
        t_obs = timed(lambda: ck(L.rsb_contact_observe(h, arr, F, _capi.RSB_CONTACT_LOCAL, 1.0, pr, 0, D), "rsb_contact_observe"))
        t_tim = timed(lambda: ck(L.rsb_contact_timers(h, arr, F, 0, 1.0, 0.01, None, p(air), p(ctime), p(td), D), "rsb_contact_timers"))
        t_cmp = timed(composition)
        t_py = timed(lambda: w.contact_observe(frames, out=rows))
        lines += [f"  {label}, F = {F}:",
                  f"    rsb_get_frame_kinematics, lin_vel + ang_vel (yardstick)       {t_kin:9.1f} us = {pct(t_kin)}",
                  f"    rsb_get_body_contact_wrenches, force + torque + count         {t_wr:9.1f} us = {pct(t_wr)}",
                  f"    rsb_get_body_contact_wrenches, force alone                    {t_f:9.1f} us = {pct(t_f)}",
                  f"    rsb_contact_observe, RSB_CONTACT_LOCAL                        {t_obs:9.1f} us = {pct(t_obs)}",
                  f"    rsb_contact_timers, both timers + touchdown                   {t_tim:9.1f} us = {pct(t_tim)}",
                  f"    frame kinematics + torch reduction over the list (replaced)   {t_cmp:9.1f} us = {pct(t_cmp)}",
                  f"    BatchedWorld.contact_observe(frames, out=..)                  {t_py:9.1f} us   (the gap to the C-ABI line is host time of the Python mirror)"]
    w.close()
    print("\n".join(lines), flush=True)


def main():
    if "--case" in sys.argv:      # the child: one model
        i = int(sys.argv[sys.argv.index("--case") + 1])
        case(*CASES[i])
        return 0
    out = os.path.join(ROOT, "profiles", "contact_sensor_bench.txt")
    if "--out" in sys.argv:
        out = sys.argv[sys.argv.index("--out") + 1]
    text = ["command: python tools/bench_contact_sensor.py",
            f"device-event time per call: {CALLS} calls after {WARM} warm-up calls, median of {WINDOWS} windows; torch CUDA tensors (RSB_DEVICE), the world on torch's stream;",
            "the C-ABI with the pointers made once unless a line says otherwise", ""]
    for i in range(len(CASES)):
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--case", str(i)], capture_output=True, text=True, timeout=LIMIT)
        if r.returncode != 0:
            print(r.stdout + r.stderr)
            print(f"bench_contact_sensor: {CASES[i][0]} failed with status {r.returncode}; stopping, nothing written")
            return 1
        print(r.stdout, end="")
        text += [r.stdout.rstrip(), ""]
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        f.write("\n".join(text))
    return 0


if __name__ == "__main__":
    sys.exit(main())
