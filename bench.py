#!/usr/bin/env python3
"""bench.py — env-steps/s of the batched World::integrate() hot path on N MI355X (BASELINE.json metric).

One "step" = one control step of the vectorised env = 4 x integrate() (dt = 0.0025) for 4096 envs per GPU, i.e. 16384
env-steps per GPU per step, run as ONE fused kernel launch through the C-ABI (rsb_control_step).  Per step, inside the
timed region, every rank also
  - reads the control step's PD targets (nominal + uniform noise, per-env seeded) in place,
  - applies rsg_anymal's termination rule on device (any non-foot contact -> reset that env),
  - writes the (q, u, foot contact force) observation block and, for N>1, all-gathers it over RCCL/xGMI.
State is resident in HBM when the timed region starts.  Envs are sharded 4096 per rank (weak scaling); the only
collective is the obs all-gather.

--config 2 (default, BASELINE.json configs[1], the configuration `metric` is quoted on): ANYmal-C-like envs on flat ground;
--config 3: the same robots on a shared 128 x 128 height map; --config 5: Atlas-like humanoid, kmax 16.

The regime is fixed by the bench, not by --steps / --warmup: PREROLL untimed control steps run first (the population of
standing / falling / freshly reset robots is stationary after ~100 control steps), then --warmup, then the timed region.

A plain single-GPU run (no --full) does only what `value` needs: set-up, pre-roll, --warmup control steps through the leg `value`
reports (one resident launch of max(1, --warmup) steps), ONE timed bracket of exactly --steps control steps of that leg, the outputs of its
last control step if --dump-outputs DIR is given (DIR/obs.npy, done.npy, gc.npy, gv.npy), and the JSON line.  Everything below -
the other legs, brackets of 7 repeats, the sampling pass, `roofline`, the CPU baseline, `secondary`, `closed_loop`,
`boundary_template_path` - runs with --full.  A run with several ranks (or --force-collective) without --full keeps its legs (lock-step
first, pipelined, resident; one bracket each) and drops the sampling pass, the trailing lock-step leg and the CPU leg.

With --full, after the timed region a sampling pass of SAMPLE_LAUNCHES more control steps of the same sequence is run with every
launch bracketed by HIP events on the launch stream (inside the library), so the kernel duration behind `roofline` never
rests on a handful of brackets; the few brackets taken inside the timed region (every EVENT_STRIDE-th launch) are reported
next to it.  The same pass counts resets per step and the env-age distribution (config.workload).

Output: ONE JSON line on rank 0; with --full it carries `roofline` (HBM; SURVEY.md §8d algorithmic bytes per env-step x env-steps per launch
over the step kernel's mean launch duration) and `cpu_baseline` (the in-repo fp64 oracle, OpenMP over envs on the host
cores, started from the GPU population's state at the start of the timed region; rank 0, N=1 only).

What else the default single-GPU --full line carries (round 4-5):
  value / lockstep      the timed region with consecutive control steps pipelined on the device (rsb_set_step_pipelining) and, same bracket,
                        with every launch waiting for the one before it; roofline.frac_throughput / frac_kernel_duration say which time each
                        fraction divides by; below 64 steps every launch of the timed region is bracketed (stride 1)
  closed_loop           the same workload with a POLICY IN THE LOOP (rsb_closed_loop_run_*: an action stage between every two steps, handed over
                        env block by env block): the linear reference stage and, under `mlp`, an actor network 34-128-128-12; pipelined and lock-step
  secondary             configs 3 and 5 with the same --steps / --warmup;  boundary_template_path: the pybind gym module over Environment.hpp
N > 1 (--gpus N): leg 1 = lock-step + in-line all-gather (must succeed), leg 2 = pipelined + gather on a side stream (under a guard); `value_leg`,
`pipelined_leg_error` and the `rccl` block (rank count, device ids) say what ran.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

ENVS_PER_GPU = 4096
HBM_PEAK_GBS = 8000.0             # MI355X_MICROARCH.md: 8.0 TB/s spec (6.29 TB/s measured copy peak)
TARGET_BANK = 128                 # distinct pre-generated PD-target sets cycled through (per-env seeded, control step k -> set k % 128)
EVENT_STRIDE = 8                  # inside the timed region every 8th launch is bracketed by HIP events (a bracket costs ~7 us of stream time)
PREROLL = 200                     # untimed control steps before --warmup: the workload is the stationary population, whatever --warmup is
SAMPLE_LAUNCHES = 256             # control steps of the post-timing sampling pass (every launch bracketed; long enough that its mean and the timed region's agree)
# SURVEY.md §8d contract numbers: unfused state traffic per env-step, fp32
BYTES_PER_ENV_STEP = {2: 456.0, 3: 520.0, 5: 1080.0}


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=100)
    ap.add_argument("--config", type=int, default=2, choices=(2, 3, 5),
                    help="BASELINE.json configs: 2 = ANYmal flat (headline), 3 = ANYmal on a 128x128 height map, 5 = Atlas-like")
    ap.add_argument("--envs-per-gpu", type=int, default=ENVS_PER_GPU)
    ap.add_argument("--atlas-regime", choices=("standing", "collapsing"), default="standing",
                    help="config 5: 'standing' = gains that hold the humanoid up (SURVEY.md 8d: standing PD, multi-contact feet); "
                         "'collapsing' = the kp 200 / kd 5 workload of rounds 1-2 (every env falls within 0.6 s and is reset)")
    ap.add_argument("--per-env-maps", action="store_true", help="config 3 variant: one 128x128 height map per env (SURVEY.md 8d: 'to stress gathers')")
    ap.add_argument("--preroll", type=int, default=PREROLL, help="diagnostic: untimed control steps before --warmup")
    ap.add_argument("--max-iter", type=int, default=0, help="contact-solver iteration cap (0 = library default)")
    ap.add_argument("--lanes-per-env", type=int, default=0)
    ap.add_argument("--hm-contacts", type=int, default=1, choices=(1, 2), help="diagnostic (config 3): contacts per primitive against the height map (rsb_set_heightmap_contacts; 2 = the second-flank kernel class)")
    ap.add_argument("--hm-angle", type=float, default=45.0, help="diagnostic (--hm-contacts 2): least angle in degrees between the two contact normals")
    ap.add_argument("--integration", default="semi_implicit", choices=("semi_implicit", "euler", "trapezoid"), help="diagnostic: rsb_set_integration_scheme (non-default schemes run in their own kernel class)")
    ap.add_argument("--slip-rule", default="energy", choices=("energy", "coulomb"), help="diagnostic: rsb_set_slip_rule (coulomb = the classical law, a kernel class of its own)")
    ap.add_argument("--anderson", type=int, default=-1, help="diagnostic: first sweep of the Anderson step in multi-contact envs of kmax > 8 worlds (library default 2; 0 = off)")
    ap.add_argument("--no-reset", action="store_true", help="disable the non-foot-contact termination rule")
    ap.add_argument("--no-cpu", action="store_true", help="skip the CPU baseline leg (--full)")
    ap.add_argument("--cpu-seconds", type=float, default=12.0)
    ap.add_argument("--stall-window", type=int, default=-1, help="diagnostic: solver stagnation window (library default 4)")
    ap.add_argument("--freeze-after", type=int, default=-1, help="diagnostic: sweeps before friction directions lag (default 6)")
    ap.add_argument("--settle-tol", type=float, default=-1.0, help="diagnostic: settled-direction tolerance in rad (library default 0 = off)")
    ap.add_argument("--no-self-collision", action="store_true", help="diagnostic: switch the self-collision sweep off (RaiSim's default, and this library's, is on)")
    ap.add_argument("--early-termination", action="store_true",
                    help="NOT the headline workload: envs stop integrating at the sub-step of their first non-foot contact")
    ap.add_argument("--overlap-collective", action="store_true",
                    help="double-buffer the obs block and overlap the all-gather of step k with the kernel of step k+1 "
                         "(default: in line on the launch stream; the overlap could not be tried on >1 GPU here)")
    ap.add_argument("--no-kernel-events", action="store_true",
                    help="diagnostic: no HIP-event brackets anywhere (roofline fields become null)")
    ap.add_argument("--target-amplitude", type=float, default=-1.0,
                    help="diagnostic: amplitude (rad) of the uniform PD-target noise (config 2/3: 0.3; config 5 collapsing: 0.1; "
                         "config 5 standing has two amplitude classes: use --target-scale there)")
    ap.add_argument("--target-scale", type=float, default=1.0,
                    help="diagnostic (config 5 standing): scale on the per-class noise amplitudes 0.03 rad (legs, back) / 0.1 rad (arms, neck)")
    ap.add_argument("--force-collective", action="store_true",
                    help="diagnostic: run the obs all-gather (RCCL) even with one rank, to see its per-step cost")
    ap.add_argument("--obs-exchange", choices=("rccl", "peer"), default="rccl",
                    help="how the per-control-step obs block reaches the other ranks: 'rccl' = all-gather (default until a multi-GPU box has "
                         "measured both), 'peer' = peer-mapped buffers written by the step kernel's epilogue (rsb_obs_peer_*: no collective, no copy kernel)")
    ap.add_argument("--peer-no-wait", action="store_true", help="diagnostic (--obs-exchange peer): rows and flags are written, nobody waits for them")
    ap.add_argument("--lockstep", action="store_true",
                    help="no pipelining of consecutive control steps (rsb_set_step_pipelining off): every launch waits for the slowest wave of the one "
                         "before it - what a caller gets that consumes every step's output before it issues the next one.  The default line reports "
                         "this number as `lockstep` next to the pipelined `value`")
    ap.add_argument("--no-secondary", action="store_true",
                    help="headline only: skip the `secondary` block (configs 3 and 5 with the same --steps / --warmup) and `boundary_template_path` "
                         "that the default single-GPU --full run of config 2 appends")
    ap.add_argument("--repeats", type=int, default=None,
                    help="every timed leg is R fresh brackets of exactly --steps steps, back to back; `value` = the MEDIAN bracket, value_repeats / value_min / "
                         "value_max beside it (VERDICT r05 #2: a 1.7 ms region measured once is not a measurement).  Default 7 with --full, else 1: "
                         "a plain run times exactly --steps steps (--closed-loop-only: 7)")
    ap.add_argument("--full", action="store_true",
                    help="everything the benchmark measures besides the headline: the other legs (pipelined, lock-step) with 7 brackets each, the sampling "
                         "pass behind `roofline`, the CPU baseline, and on the default single-GPU line `secondary`, `closed_loop` and `boundary_template_path`.  "
                         "Without it a single-rank run sets up, warms up, times the --steps steps of the leg `value` reports and prints the line; a run with several "
                         "ranks (or --force-collective) keeps its legs, one bracket each, and drops the sampling pass, the trailing lock-step leg and the CPU leg")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the timed leg computed in its last control step as DIR/<name>.npy (float32): obs (the "
                         "observation block), done (termination flags), gc / gv (generalized coordinates / velocities); a seeded sample of envs above 64 MB; with several ranks, rank 0's envs")
    ap.add_argument("--specialization", default="compile", choices=("compile", "cached", "off"),
                    help="specialised code objects of the step kernel (rsb_set_specialization; csrc/step_spec.h): compile = a key build() did not prebuild is compiled during "
                         "warm-up (~3 s, never inside a timed region); cached = prebuilt objects only; off = the ahead-of-time kernel classes (rounds 1-5)")
    ap.add_argument("--no-resident", action="store_true",
                    help="no resident leg (rsb_set_step_residency: --steps control steps in ONE launch of the step kernel): `value` is then the pipelined leg's, as in round 5")
    ap.add_argument("--closed-loop-only", action="store_true", help="diagnostic: only the `closed_loop` block (policy in the loop, include/rsb_pipeline.h), as its own JSON line")
    ap.add_argument("--stage-grid", type=int, default=0, help="diagnostic (closed loop): workgroups of the action stage (library default 256)")
    ap.add_argument("--share-device", action="store_true",
                    help="N > 1 on a ONE-GPU box: every rank uses cuda:0 (VERDICT r05 #4: the legs of an N > 1 run with real kernels and real processes - "
                         "lock-step + in-line gather, pipelined + side-stream gather, resident + one gather per launch - before a multi-GPU node runs them). "
                         "RCCL refuses two ranks on one device: use --backend gloo.  Not a measurement: the ranks share the chip")
    ap.add_argument("--backend", default="nccl", choices=("nccl", "gloo"), help="torch.distributed backend of the obs all-gather (nccl = RCCL; gloo: --share-device runs)")
    ap.add_argument("--dry-run-fail-leg", type=int, default=-1, help="test hook (--dry-run-ranks): the second leg raises on this rank")
    ap.add_argument("--dry-run-ranks", action="store_true",
                    help="plumbing check without GPUs: the ranks rendezvous on gloo, all-gather a host obs block per step and "
                         "print the contract line with dry_run=true (no device world, no physics; value is not a measurement)")
    return ap.parse_args()


def _free_port():
    import socket
    with socket.socket(socket.AF_INET, socket.SOCK_STREAM) as sk:
        sk.bind(("127.0.0.1", 0))
        return sk.getsockname()[1]


def spawn_ranks(args):
    """`python bench.py --gpus N` without a launcher: re-exec this script N times, one rank per GPU (what
    `python -m torch.distributed.run --nproc-per-node N bench.py --gpus N` would do), forward rank 0's stdout (the one JSON
    line) and every rank's stderr, and fail if any rank fails.  Returns the exit code."""
    import subprocess
    n = args.gpus
    if not args.dry_run_ranks:
        import torch
        have = torch.cuda.device_count()
        if have < (1 if args.share_device else n):
            print(f"bench.py: --gpus {n} needs {n} visible GPUs, this node shows {have} (no CPU or single-GPU fallback for N>1)",
                  file=sys.stderr)
            return 2
    port = int(os.environ.get("MASTER_PORT", "0")) or _free_port()
    procs = []
    for r in range(n):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(n), LOCAL_WORLD_SIZE=str(n),
                   MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"))
        out = None if r == 0 else subprocess.DEVNULL          # rank 0 owns stdout: exactly one JSON line reaches the caller
        procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__), *sys.argv[1:]], env=env, stdout=out))
    rc = 0
    try:
        pending = set(range(n))
        while pending:
            for r in list(pending):
                code = procs[r].poll()
                if code is None:
                    continue
                pending.discard(r)
                if code != 0 and rc == 0:
                    rc = code
                    print(f"bench.py: rank {r} exited with code {code}; stopping the other ranks", file=sys.stderr)
                    for q in pending:
                        procs[q].terminate()
            time.sleep(0.05)
    finally:
        for pr in procs:
            if pr.poll() is None:
                pr.kill()
    return rc


def dry_run_ranks(args, rank, world_size):
    """The N>1 plumbing on CPU (gloo): rendezvous, env-shard bookkeeping, the communicator check (`rccl`), and the SAME two-leg order the device
    path runs (two_legs): first the in-line all-gather per "step" through the ObsGatherer the device path uses, then - under the guard - the
    double-buffered leg that stands for the pipelined steps + side-stream gather; barrier-bracketed timing with the MAX over ranks, ONE JSON line
    on rank 0.  --dry-run-fail-leg R makes the second leg raise on rank R: the line must then be the first leg's.  No physics."""
    import torch
    import torch.distributed as dist
    from raisimlib_amd.dist import ObsGatherer, env_range
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", "29500")
    dist.init_process_group("gloo", rank=rank, world_size=world_size)
    n, obs_dim = args.envs_per_gpu, 49
    lo, hi = env_range(rank, n)
    ones = torch.ones(1, dtype=torch.float64)
    dist.all_reduce(ones)
    allr = [torch.zeros(2, dtype=torch.int64) for _ in range(world_size)]
    dist.all_gather(allr, torch.tensor([rank, int(os.environ.get("LOCAL_RANK", rank))], dtype=torch.int64))
    rccl_info = {"backend": dist.get_backend(), "rccl_ranks": dist.get_world_size(), "allreduce_of_ones": float(ones.item()),
                 "by_rank": [{"rank": int(r[0]), "local_rank": int(r[1])} for r in allr]}
    rows = torch.arange(lo, hi, dtype=torch.float32)[:, None].expand(n, obs_dim)
    state = {"k": 0}

    def leg(overlap, fail):
        gath = ObsGatherer(n, obs_dim, torch.device("cpu"), overlap=overlap, force=args.force_collective)

        def step(k):
            gath.acquire(k)
            gath.local(k).copy_(rows + float(k))          # stands for the step kernel writing this rank's obs block
            gath.gather(k)
        for _ in range(args.warmup):
            step(state["k"]); state["k"] += 1
        gath.drain()
        dist.barrier()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            step(state["k"]); state["k"] += 1
        gath.drain()
        if fail:
            raise RuntimeError("injected failure of the second leg (--dry-run-fail-leg)")
        dist.barrier()
        mine = time.perf_counter() - t0
        t = torch.tensor([mine], dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        per_rank = [torch.zeros(1, dtype=torch.float64) for _ in range(world_size)]
        dist.all_gather(per_rank, torch.tensor([mine], dtype=torch.float64))
        last = gath.gathered(state["k"] - 1)
        want = torch.arange(0, world_size * n, dtype=torch.float32) + float(state["k"] - 1)
        ok = bool(torch.equal(last[:, 0], want)) if gath.active else True
        return {"elapsed": float(t.item()), "ms_by_rank": [float(x.item()) / args.steps * 1e3 for x in per_rank], "ok": ok, "obs_all_gather": gath.describe()}

    def all_agree(ok):
        f = torch.tensor([1.0 if ok else 0.0], dtype=torch.float64)
        if ok or args.dry_run_fail_leg < 0:
            dist.all_reduce(f, op=dist.ReduceOp.MIN)
        else:
            # (the rank that raised left the leg's collectives early: it catches up with the barrier and the two reductions the others are in)
            dist.barrier(); dist.all_reduce(torch.zeros(1, dtype=torch.float64), op=dist.ReduceOp.MAX)
            dist.all_gather([torch.zeros(1, dtype=torch.float64) for _ in range(world_size)], torch.zeros(1, dtype=torch.float64))
            dist.all_reduce(f, op=dist.ReduceOp.MIN)
        return float(f.item()) == 1.0

    two = world_size > 1
    legs = two_legs((lambda: leg(False, False)) if two else None, lambda: leg(args.overlap_collective or two, rank == args.dry_run_fail_leg), all_agree)
    use = legs[legs["use"]]
    ok = use["ok"] and (legs["first"] is None or legs["first"]["ok"])
    dist.destroy_process_group()
    if rank == 0:
        elapsed = use["elapsed"]
        print(json.dumps({
            "metric": "env-steps/sec (DRY RUN: rank plumbing only, no physics)", "value": world_size * n * 4 * args.steps / elapsed,
            "unit": "env-steps/s", "n_gpus": world_size, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": elapsed / args.steps * 1e3, "ms_per_step_by_rank": use["ms_by_rank"],
            "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "f32", "data": "synthetic", "dry_run": True,
            "value_leg": ("second (stands for: pipelined steps + gather on a side stream)" if legs["use"] == "second" else "first (stands for: lock-step + in-line all-gather)"),
            "pipelined_leg_error": legs["error"], "rccl": rccl_info,
            "lockstep": ({"value": world_size * n * 4 * args.steps / legs["first"]["elapsed"], "ms_per_step": legs["first"]["elapsed"] / args.steps * 1e3, "ran_first": True,
                          "obs_all_gather": legs["first"]["obs_all_gather"]} if legs["first"] else None),
            "config": {"workload": "dry run of the rank plumbing on gloo", "envs_per_gpu": n, "parallelism": f"env-shard x{world_size}",
                       "obs_all_gather": use["obs_all_gather"], "gathered_rows_correct": ok}}), flush=True)
    return 0 if ok else 1


class Recipe:
    """Everything that defines one BASELINE.json configuration: model, terrain, gains, initial state, targets."""

    def __init__(self, config, amplitude, atlas_regime="standing", per_env_maps=False, target_scale=1.0):
        from raisimlib_amd import Model, rsc_path, workload
        self.config = config
        self.wl = workload
        self.per_env_maps = bool(per_env_maps) and config == 3
        # solver settings of envs with redundant contact sets (rsb_set_solver_multi_contact: depth, light passes, freeze_after,
        # stall_window).  Library default depth 3; the humanoid's feet also stand on two spheres of one edge, so config 5 uses
        # depth 2 (tests/test_oracle_solver_heuristics.py pins exactly this setting on both config-5 populations)
        self.multi_contact = (2 if config == 5 else 3, False, 0, 16)
        # Anderson acceleration of the sweep in those envs (rsb_set_solver_anderson: first sweep, clip; kmax > 8 worlds only = config 5):
        # the library default, spelled out so that world and oracle are set from one place (--anderson 0 switches it off for an A/B)
        self.anderson = (2, 20.0)
        self.atlas_regime = atlas_regime
        self._terrain = {}
        if config == 5:
            self.model = Model(urdf_path=rsc_path("atlas_like.urdf"))
            self.kmax = 16
            b = self.model.blob
            self.joint_names = [b.joint_name[i].value.decode() for i in range(b.nb)]
            self.feet = self.model.collision_indices("_foot_0") + self.model.collision_indices("_foot_1") + \
                self.model.collision_indices("_foot_2") + self.model.collision_indices("_foot_3")
            self.feet = sorted(self.feet)
            head = ("configs[4]: 4096 Atlas-like humanoids (synthetic stand-in URDF, 31 bodies / 36 DoF, 18 collision spheres, "
                    "kmax 16) per GPU, flat ground, ")
            if atlas_regime == "standing":
                if amplitude >= 0:
                    raise SystemExit("config 5 (standing) has two noise amplitude classes: scale them with --target-scale (--target-amplitude is in rad and means one amplitude)")
                self.amp = float(target_scale)                           # scale of the per-class noise amplitudes
                self.kp, self.kd = workload.atlas_standing_gains(self.joint_names)
                a0, a1 = (self.amp * x for x in workload.ATLAS_STAND_AMP)
                self.name = head + ("STANDING regime: implicit PD kp 3000 / kd 60 on legs and back, kp 300 / kd 10 on arms and neck, targets = zero "
                                    f"pose + U(-{a0:g},{a0:g}) rad (legs, back) / U(-{a1:g},{a1:g}) rad (arms, neck) per control step, per-env seed 77+i")
            else:
                self.amp = amplitude if amplitude >= 0 else 0.1
                self.kp, self.kd = workload.atlas_gains(self.model.nv)
                self.name = head + ("COLLAPSING regime (rounds 1-2; kp 200 cannot hold 164 kg up): implicit PD kp=200 kd=5, targets = zero pose + "
                                    f"U(-{self.amp:g},{self.amp:g}) rad per control step, per-env seed 77+i")
            self.metric = "env-steps/sec, 4096 Atlas-like humanoid envs flat terrain dt=0.0025"
        else:
            self.model = Model(urdf_path=rsc_path("anymal_c_like.urdf"))
            self.kmax = 8
            self.amp = amplitude if amplitude >= 0 else 0.3
            self.kp, self.kd = workload.anymal_gains(self.model.nv)
            self.feet = self.model.collision_indices("_foot")
            if config == 2:
                terrain = "flat ground"
            elif self.per_env_maps:
                terrain = ("ONE 128x128 height map PER ENV (12.8 m x 12.8 m, smoothed uniform noise, +-0.1 m, seed 7+i; 256 MB of maps per GPU), "
                           "base xy spread over +-6 m of it (per-env seeded)")
            else:
                terrain = ("shared 128x128 height map over 12.8 m x 12.8 m (smoothed uniform noise, +-0.1 m, seed 7), base xy spread over "
                           "+-6 m of it (per-env seeded)")
            self.name = (f"configs[{config - 1}]: 4096 ANYmal-C-like (synthetic stand-in URDF) envs per GPU, {terrain}, PD kp=50 kd=0.2, "
                         f"targets = nominal + U(-{self.amp:g},{self.amp:g}) rad per control step, per-env seed 1234+i")
            self.metric = "env-steps/sec, 4096 ANYmal-C envs flat terrain dt=0.0025" if config == 2 else \
                "env-steps/sec, 4096 ANYmal-C envs on a 128x128 raisim::HeightMap dt=0.0025"

    def terrain(self, n, env_offset):
        """config 3: (maps [n_maps, 128, 128], env -> map [n]) of the envs [env_offset, env_offset + n)"""
        key = (n, env_offset)
        if key not in self._terrain:
            wl = self.wl
            if self.per_env_maps:
                self._terrain[key] = (wl.env_heightmaps(n, 128, 128, amplitude=0.1, seed0=7, env_offset=env_offset), np.arange(n, dtype=np.int32))
            else:
                self._terrain[key] = (wl.smoothed_heightmap(128, 128, amplitude=0.1, seed=7)[None], np.zeros(n, np.int32))
        return self._terrain[key]

    def initial_state(self, n, env_offset):
        wl = self.wl
        if self.config == 5:
            return wl.atlas_initial_state(n, self.model.nq, self.model.nv)
        if self.config == 3:
            maps, env_map = self.terrain(n, env_offset)
            return wl.anymal_initial_state_on_maps(n, maps, env_map, wl.HEIGHTMAP_SIZE, env_offset=env_offset)
        return wl.anymal_initial_state(n, env_offset=env_offset)

    def targets(self, n, k, env_offset):
        if self.config == 5:
            if self.atlas_regime == "standing":
                return self.wl.atlas_standing_targets(n, k, self.joint_names, env_offset=env_offset, scale=self.amp)
            return self.wl.atlas_targets(n, k, self.model.nq, env_offset=env_offset, amplitude=self.amp)
        return self.wl.anymal_targets(n, k, env_offset=env_offset, amplitude=self.amp)

    def setup_world(self, world, n, env_offset):
        wl = self.wl
        if self.kmax != 8:
            world.set_max_contacts(self.kmax)
        world.set_time_step(wl.DT)
        world.set_pd_gains(self.kp, self.kd)
        world.set_solver_multi_contact(*self.multi_contact)
        world.set_solver_anderson(*self.anderson)
        if self.config == 3:
            maps, env_map = self.terrain(n, env_offset)
            if self.per_env_maps:
                world.add_height_maps(maps, wl.HEIGHTMAP_SIZE, wl.HEIGHTMAP_SIZE, 0.0, 0.0, env_map)
            else:
                world.add_height_map(128, 128, wl.HEIGHTMAP_SIZE, wl.HEIGHTMAP_SIZE, 0.0, 0.0, maps[0])

    def setup_oracle(self, orc, n, env_offset):
        orc.p.kmax = self.kmax
        orc.p.multi_depth, orc.p.multi_light, orc.p.multi_freeze_after, orc.p.multi_stall_window = (int(x) for x in self.multi_contact)
        orc.p.anderson, orc.p.anderson_clip = int(self.anderson[0]), float(self.anderson[1])
        if self.config == 3:
            wl = self.wl
            maps, env_map = self.terrain(n, env_offset)
            if self.per_env_maps:
                orc.set_heightmaps(maps, wl.HEIGHTMAP_SIZE, wl.HEIGHTMAP_SIZE, 0.0, 0.0, env_map)
            else:
                orc.set_heightmap(128, 128, wl.HEIGHTMAP_SIZE, wl.HEIGHTMAP_SIZE, 0.0, 0.0, maps[0])


def recorded_traffic(config, n_envs, substeps, resident=False):
    """HBM bytes per launch of the step kernel from the newest committed PMC pass of this configuration
    (profiles/rNN_pmc_traffic*.json: rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE in separate passes over this same command,
    tools/collect_profiles.sh).  The counters cannot be collected from inside this process, so the committed measurement
    is reported - only when it was taken on this workload - together with its provenance; otherwise null."""
    import glob
    pat = "r*_pmc_traffic.json" if config == 2 else f"r*_pmc_traffic_config{config}.json"
    if resident:        # (the resident class's passes record HBM bytes per CONTROL STEP of a launch: hbm_bytes_per_control_step)
        pat = "r*_pmc_traffic_resident.json" if config == 2 else f"r*_pmc_traffic_resident_config{config}.json"
    files = sorted(glob.glob(os.path.join(ROOT, "profiles", pat)))
    if not files or n_envs != ENVS_PER_GPU or substeps != 4:
        return None, None, None
    try:
        rec = json.load(open(files[-1]))
        val = rec.get("hbm_bytes_per_control_step") if resident else rec.get("hbm_bytes_per_launch", rec.get("hbm_bytes_per_launch_raw"))
        return float(val), os.path.relpath(files[-1], ROOT) + " (" + rec.get("note", "FETCH_SIZE+WRITE_SIZE per launch") + ")", rec
    except Exception:
        return None, None, None


def cpu_baseline(recipe, max_iter, reset, budget_s, q0, u0, gc_reset, gv_reset, step0, self_collision=True):
    """Time the fp64 oracle (OpenMP over envs) on a bounded sample of the same workload: it starts from the state the GPU
    population had at the start of the timed region (so both legs see the same stationary mix of standing, falling and
    freshly reset robots) and continues the same target sequence.

    The container's visible core count can exceed its CPU quota, so the leg first probes a few thread counts for
    ~1 s each and then spends the budget at the fastest one; `cores` reports the threads actually used.
    """
    from oracle.pyoracle import Oracle  # the CPU baseline leg is one of the three allowed oracle users
    from raisimlib_amd import workload
    model = recipe.model
    orc = Oracle(model.blob)
    recipe.setup_oracle(orc, q0.shape[0], 0)
    orc.p.self_collision = int(self_collision)
    if max_iter > 0:
        orc.p.max_iter = max_iter
    n = q0.shape[0]
    kp, kd = recipe.kp.astype(np.float64), recipe.kd.astype(np.float64)
    dtg = np.zeros((n, model.nv))
    feet_set = np.zeros(model.ncol, bool)
    feet_set[recipe.feet] = True
    state = {"q": q0.astype(np.float64), "u": u0.astype(np.float64), "cs": step0}
    warm = orc.new_warm_state(n)      # the solver warm state the device keeps per env (cleared on reset, as there)

    def control_step(threads):
        pt = recipe.targets(n, state["cs"] % TARGET_BANK, 0).astype(np.float32).astype(np.float64)
        t0 = time.perf_counter()
        r = orc.step_batch(state["q"], state["u"], workload.SUBSTEPS, kp, kd, pt, dtg, nthreads=threads,
                           want_contacts=reset, lam_warm=warm)
        dt_ = time.perf_counter() - t0
        q, u = r["q"], r["u"]
        if reset:
            con, ncs = r["contacts"], r["n_contacts"]
            valid = np.arange(con.shape[1])[None, :] < ncs[:, None]
            term = (valid & ~(feet_set[con["collision"] & 0xffff] & (con["collision"] < 0x10000))).any(axis=1)   # (a self-collision entry carries flag bits: never a foot on the ground)
            term = term | (r["flags"] & 2).astype(bool)
            q[term], u[term] = gc_reset[term], gv_reset[term]
            warm[term] = 0.0
        state["q"], state["u"] = q, u
        state["cs"] += 1
        return dt_

    def run(threads, seconds):
        spent, steps = 0.0, 0
        while spent < seconds:
            spent += control_step(threads)
            steps += n * workload.SUBSTEPS
        return steps / spent, spent, steps

    hw = orc.max_threads()
    for _ in range(3):     # untimed: build the solver warm state the GPU population already has
        control_step(0)
    try:
        hw = min(hw, len(os.sched_getaffinity(0)))
    except AttributeError:
        pass
    cands = sorted({1, min(8, hw), min(16, hw), min(32, hw), min(64, hw), hw})
    probe = {t: run(t, 1.0)[0] for t in cands}
    best = max(probe, key=probe.get)
    rate, spent, steps = run(best, max(budget_s - len(cands), 2.0))
    return {"value": rate, "unit": "env-steps/s", "cores": int(best), "kind": "port",
            "single_thread": probe[1],
            "sample": f"{n} envs, {steps} env-steps of the same workload in {spent:.1f} s, started from the GPU population's state at "
                      f"the start of the timed region (control step {step0}) after 3 untimed control steps, fp64 oracle, OpenMP "
                      f"schedule(static) over envs; thread-count probe {{threads: env-steps/s}} = "
                      + json.dumps({str(k): round(v) for k, v in probe.items()})}


def cpu_quota():
    """CPUs the container may use per scheduling period (cgroup v2 cpu.max / v1 cfs quota); None when unlimited or unknown."""
    try:
        q, per = open("/sys/fs/cgroup/cpu.max").read().split()[:2]
        return None if q == "max" else max(1, int(int(q) / int(per)))
    except Exception:
        pass
    try:
        q = int(open("/sys/fs/cgroup/cpu/cpu.cfs_quota_us").read())
        per = int(open("/sys/fs/cgroup/cpu/cpu.cfs_period_us").read())
        return None if q <= 0 else max(1, q // per)
    except Exception:
        return None


def template_path(n, steps, threads=0):
    """The headline workload through the reference's own boundary: RaisimGymVecEnv -> the raisim_gym-style pybind11 module
    -> VectorizedEnvironment<ENVIRONMENT> over the UNMODIFIED rsg_anymal-style tests/cpp/anymal_env/Environment.hpp, numpy buffers in place.
    The n step() bodies run as fibers on `threads` host threads (default: the box's cores, at most 32); their integrate() calls are
    recorded and flushed as one fused launch + one rsb_view_exchange per control step (include/raisim/World.hpp)."""
    from raisimlib_amd.gym import RaisimGymVecEnv, build_env_module, load_env_module
    try:
        cores = len(os.sched_getaffinity(0))
    except AttributeError:
        cores = os.cpu_count() or 1
    # more actively waiting threads than the container's CPU quota get the whole group throttled: 32 threads on a 16-CPU quota measured
    # 32-39 M over bursts shorter than one 100-ms cgroup period and 20-22 M SUSTAINED, 16 threads 26-30 M sustained (profiles/r04_ab_log.txt, call V)
    threads = threads or max(1, min(32, cores, cpu_quota() or cores))
    rsc = os.path.join(ROOT, "raisimlib_amd", "rsc")
    cfg = (f"num_envs: {n}\nnum_threads: {threads}\nsimulation_dt: 0.0025\ncontrol_dt: 0.01\nrender: false\naction_std: 0.3\n"
           "reward:\n  forwardVel:\n    coeff: 0.3\n  torque:\n    coeff: -4e-5\n")
    build_env_module(os.path.join(ROOT, "tests", "cpp", "anymal_env"), name="rsg_anymal")
    mod = load_env_module("rsg_anymal")
    rng = np.random.default_rng(0)
    acts = [rng.uniform(-1, 1, (n, 12)).astype(np.float32) for _ in range(8)]
    env = RaisimGymVecEnv(mod.RaisimGymEnv(rsc, cfg, False), normalize_ob=False)
    env.reset()
    for k in range(10):
        env.step(acts[k % 8]); env.observe(False)
    l0 = env.wrapper.viewLaunches()
    t0 = time.perf_counter()
    for k in range(steps):
        env.step(acts[k % 8]); env.observe(False)
    dt = time.perf_counter() - t0
    res = {"env_steps_per_s": n * 4 * steps / dt, "ms_per_control_step": dt / steps * 1e3, "control_steps_timed": steps, "host_threads": threads, "cpu_quota": cpu_quota(),
           "kernel_launches_per_control_step": (env.wrapper.viewLaunches() - l0) / steps,
           "what": "RaisimGymVecEnv.step + observe (numpy buffers, host round trip included) over N unmodified Environment.hpp objects: "
                   "setPdTarget, 4 x World::integrate(), state / contact / generalized-force reads, reward, termination, reset per env"}
    env.close()
    return res


def closed_loop_leg(args, dev, n):
    """The headline workload with a POLICY IN THE LOOP (include/rsb_pipeline.h): config 2 as the device-resident vectorised env
    (action -> PD targets nominal + 0.3 * action, 4 x integrate(), reward / termination / reset / next observation in the step's epilogue) and the
    in-repo reference stage between two steps: action = W ob + noise[k], W a fixed 12 x 34 matrix, noise[k] the open-loop benchmark's own target draw
    of control step k - every step's targets depend on the step before.  Step k + 1's workgroup b starts when the stage has published block b's
    actions computed from step k's observation of block b: the steps still overlap.  Timed like the headline (same --steps, barrier-free single
    GPU: synchronise, enqueue ONE run of --steps steps, join, synchronise), pipelined and in lock-step from the same pre-rolled population."""
    import torch
    from raisimlib_amd import Model, rsc_path, workload
    model = Model(urdf_path=rsc_path("anymal_c_like.urdf"))
    stream = torch.cuda.Stream(device=dev)
    res = {"what": "rsb_closed_loop_run_linear: K control steps of the vectorised env with the reference action stage (fixed linear policy, 12 x 34, + the open-loop "
                   "benchmark's target noise) between every two steps.  `resident` (round 6, rsb_set_step_residency): the run is ONE launch of the step kernel, the "
                   "env block's own wave evaluates the stage between two control steps; `pipelined`: a launch per step + a persistent stage kernel, handed over env "
                   "block by env block; `lockstep`: pass, step, pass, ... on one stream.  All three bit-identical (tests/test_gpu_resident.py, test_gpu_closed_loop.py); "
                   "each value = the median of `repeats` brackets of --steps steps",
           "policy": {"W": f"U(-{workload.CLOSED_LOOP_W_SCALE:g}, {workload.CLOSED_LOOP_W_SCALE:g}) seeded, [12, 34]", "noise": "config 2's target draws, period 128", "action_std": 0.3}}
    with torch.cuda.stream(stream):
        env = workload.closed_loop_env(model, n, device=dev.index or 0, stream=stream.cuda_stream)
        W = torch.from_numpy(workload.closed_loop_policy(env.num_obs, env.num_acts)).to(dev)
        noise = torch.from_numpy(workload.closed_loop_noise(n, TARGET_BANK)).to(dev)
        w = env.world
        if args.stage_grid:
            env.set_stage_grid(args.stage_grid)
        mlp = [(torch.from_numpy(Wl).to(dev), torch.from_numpy(bl).to(dev)) for Wl, bl in workload.closed_loop_mlp(env.num_obs, env.num_acts)]
        ob_mean, ob_var = torch.zeros(env.num_obs, device=dev), torch.ones(env.num_obs, device=dev)
        res["mlp"] = {"what": "rsb_closed_loop_run_mlp: the same run with an ACTOR NETWORK as the action stage - raisimGymTorch's default architecture (MLP 34 -> 128 -> 128 "
                              "-> 12, LeakyReLU [RECALL]), observation normalisation (clamp((ob - mean) / sqrt(var + eps), +-10), frozen statistics), fp32, evaluated per env block "
                              "by the stage's waves (lane = unit, no LDS, <= 96 registers: a stage wave shares its SIMD with a step wave)",
                      "policy": {"layers": "34-128-128-12, hidden U(+-1/sqrt(fan_in)), output U(+-%g), zero biases, seeded" % workload.CLOSED_LOOP_W_SCALE,
                                 "activation": "leaky_relu(0.01)", "noise": "config 2's target draws, period 128", "action_std": 0.3}}
        runners = {"linear": lambda K, ro=None: env.rollout_linear(K, W, noise=noise, rollout=ro),
                   "mlp": lambda K, ro=None: env.rollout_mlp(K, mlp, activation="leaky_relu", ob_mean=ob_mean, ob_var=ob_var, noise=noise, rollout=ro)}
        for kind, run in runners.items():
            dst = res if kind == "linear" else res["mlp"]
            for mode in ("resident", "pipelined", "lockstep"):
                w.set_step_residency(mode == "resident")
                if mode == "resident" and (args.no_resident or not w.residency_status(1 if kind == "linear" else 2)):
                    dst["resident"] = None
                    continue
                on = w.set_step_pipelining(mode == "pipelined")
                if mode == "pipelined" and not on:
                    dst["pipelined"] = None
                    continue
                env.reset()
                w.synchronize()
                # (env.reset() also restarts the world's closed-loop step counter, which selects the noise slice: all modes run the same sequence)
                run(args.preroll + args.warmup)
                w.step_pipeline_join()
                torch.cuda.synchronize()
                # R fresh brackets of --steps steps each, back to back; the median bracket is the mode's value
                reps, t_enq = [], 0.0
                for _ in range(max(1, args.repeats)):
                    t0 = time.perf_counter()
                    run(args.steps)
                    t_enq = time.perf_counter() - t0
                    w.step_pipeline_join()
                    torch.cuda.synchronize()
                    reps.append(time.perf_counter() - t0)
                dt = float(np.median(reps))
                vals = [n * workload.SUBSTEPS * args.steps / x for x in reps]
                K2 = 64
                ro = {"done": torch.zeros((K2, n), dtype=torch.uint8, device=dev)}
                run(K2, ro)
                w.step_pipeline_join()
                cnt, _ = w.get_contacts()
                q, _ = w.get_state()
                dst[mode] = {"value": n * workload.SUBSTEPS * args.steps / dt, "unit": "env-steps/s", "ms_per_step": dt / args.steps * 1e3, "steps": args.steps,
                             "value_repeats": vals, "value_min": min(vals), "value_max": max(vals), "repeats": len(vals), "spread_rel": (max(vals) - min(vals)) / float(np.median(vals)),
                             "resident_launches": w.residency_launches(),
                             "host_enqueue_ms_per_step": t_enq / args.steps * 1e3,
                             "resets_per_control_step_mean": float(ro["done"].sum().item()) / K2, "contacts_per_env": float(cnt.mean()),
                             "solver_iters_mean": float(w.get_solver_iterations().mean()), "base_height_mean": float(q[:, 2].mean())}
        w.set_step_residency(False)
        faults, code = w.step_pipeline_fault()
        launches, joins = w.step_pipelining_stats()
        res["pipeline"] = {"pipelined_launches": launches, "joins": joins, "faults": faults, "last_fault_code": code, "streams_overlap": bool(w.pipeline_overlaps)}
        env.close()
    return res


def two_legs(first, second, all_agree):
    """The order of an N > 1 bench run (also what --dry-run-ranks exercises on CPU): `first` - the combination that has run
    before, or None when there is only one leg - must succeed; `second` runs under a guard.  A second leg that raised on ANY rank (all_agree:
    MIN over the ranks) does not count anywhere: every rank then reports the first leg.  Returns {"use": "first" | "second", "first": result |
    None, "second": result | None, "error": message | None}; with no first leg a failure of the second one is re-raised."""
    r1 = first() if first is not None else None
    r2, err = None, None
    try:
        r2 = second()
    except Exception as e:
        if r1 is None:
            raise
        err = f"{type(e).__name__}: {e}"
    ok = all_agree(err is None)
    if not ok and err is None:
        err = "the leg raised on another rank"
    if r1 is None:
        return {"use": "second", "first": None, "second": r2, "error": None}
    return {"use": "second" if ok else "first", "first": r1, "second": r2 if ok else None, "error": err}


def measure(args, rank, local_rank, world_size, dev, coll):
    """One configuration end to end on this rank: world, pre-roll, warm-up, the timed region (barrier + synchronise on both sides, MAX
    over ranks), the sampling pass behind `roofline`, the CPU leg.  Returns the contract dictionary on rank 0, None elsewhere."""
    import torch
    import torch.distributed as dist

    from raisimlib_amd import BatchedWorld, workload
    out = None
    N = args.envs_per_gpu
    # did the communicator come up with every rank, each on a GPU of its own?  (the driver's scaling run reads this: VERDICT r04 #2)
    rccl_info = None
    if world_size > 1 or coll:
        ones = torch.ones(1, dtype=torch.float64, device=dev)
        dist.all_reduce(ones)
        props = torch.cuda.get_device_properties(local_rank)
        mine = torch.tensor([rank, local_rank, torch.cuda.current_device(), int(getattr(props, "pci_bus_id", -1)), int(getattr(props, "multi_processor_count", 0))],
                            dtype=torch.int64, device=dev)
        allr = torch.zeros(5 * world_size, dtype=torch.int64, device=dev)
        dist.all_gather_into_tensor(allr, mine)
        rows = allr.view(world_size, 5).cpu().tolist()
        rccl_info = {"backend": dist.get_backend(), "rccl_ranks": dist.get_world_size(), "allreduce_of_ones": float(ones.item()),
                     "by_rank": [{"rank": r[0], "local_rank": r[1], "device": r[2], "pci_bus_id": r[3], "compute_units": r[4]} for r in rows],
                     "distinct_devices": len({(r[2], r[3]) for r in rows})}
    recipe = Recipe(args.config, args.target_amplitude, args.atlas_regime, args.per_env_maps, args.target_scale)
    if args.anderson >= 0:
        recipe.anderson = (args.anderson, recipe.anderson[1])
    model, feet = recipe.model, recipe.feet
    world = BatchedWorld(model, N, device=local_rank)
    stream = torch.cuda.Stream(device=dev)       # everything below (kernels, copies, events, collectives) is ordered on it
    torch.cuda.set_stream(stream)
    world.set_stream(stream.cuda_stream)
    recipe.setup_world(world, N, rank * N)
    if args.max_iter > 0:
        world.set_contact_solver_param(1.0, 1.0, 1.0, args.max_iter, 1e-5)
    if (args.hm_contacts != 1 or args.integration != "semi_implicit" or args.slip_rule != "energy") and not args.no_cpu:
        raise SystemExit("--hm-contacts / --integration / --slip-rule are diagnostics of the device path: run them with --no-cpu (the CPU leg measures the default rules)")
    if args.slip_rule != "energy":
        world.set_slip_rule(args.slip_rule)
    if args.hm_contacts != 1:
        world.set_heightmap_contacts(args.hm_contacts, args.hm_angle)
    if args.integration != "semi_implicit":
        world.set_integration_scheme(args.integration)
    if args.lanes_per_env:
        world.set_lanes_per_env(args.lanes_per_env)
    if args.early_termination:
        world.set_early_termination(True)
    if args.no_self_collision:
        world.set_self_collision(False)
    if args.stall_window >= 0:
        world.set_solver_stagnation_exit(args.stall_window, 0.5)
    if args.freeze_after >= 0 or args.settle_tol >= 0:
        world.set_solver_friction_lag(args.freeze_after if args.freeze_after >= 0 else 6, True,
                                      args.settle_tol if args.settle_tol >= 0 else 0.0)

    # per-rank env shard: rank r owns global envs [r*N, (r+1)*N); every random number is a function of the global index
    off = rank * N
    gc0, gv0 = recipe.initial_state(N, off)
    gc0_d = torch.from_numpy(gc0.astype(np.float32)).to(dev)
    gv0_d = torch.from_numpy(gv0.astype(np.float32)).to(dev)
    world.set_state(gc0, gv0)
    world.set_pd_target(None, np.zeros((N, model.nv), np.float32))
    bank_all = torch.from_numpy(np.stack([recipe.targets(N, k, off).astype(np.float32) for k in range(TARGET_BANK)])).to(dev)      # [128, N, nq]: the resident launch reads slice k % 128 itself
    bank = [bank_all[k] for k in range(TARGET_BANK)]
    obs_dim = world.obs_dim(len(feet))
    # obs block of this rank and the gathered block of all ranks (raisimlib_amd/dist.py); with --overlap-collective
    # double-buffered, so that the all-gather of control step k (RCCL, its own stream) overlaps the kernel of step k+1
    from raisimlib_amd.dist import ObsGatherer, PeerObsGatherer
    # consecutive control steps overlap on the device (rsb_set_step_pipelining) unless --lockstep; the peer-mapped exchange has no pipelined twin
    pipelined = not args.lockstep and args.obs_exchange != "peer"
    if args.obs_exchange == "peer":
        gath = PeerObsGatherer(world, np.asarray(feet, np.int32), force=args.force_collective, no_wait=args.peer_no_wait)
    else:
        gath = ObsGatherer(N, obs_dim, dev, overlap=args.overlap_collective, force=args.force_collective, pipeline_world=world if pipelined else None)
    obs_b, nbuf = gath.local_bufs, gath.nbuf
    feet_idx = np.asarray(feet, np.int32)
    reset = not args.no_reset
    done_d = torch.zeros(N, dtype=torch.uint8, device=dev)         # done flags of the fused control step (rsb_set_done_output)
    age_d = torch.zeros(N, dtype=torch.int32, device=dev)          # control steps since each env's last reset
    if reset:
        world.set_done_output(done_d.data_ptr())

    # one foreign call per control step (rsb_control_step); the step kernel's launches are bracketed by HIP events inside
    # the library (ring of event pairs on the launch stream, read back after the fact, no per-launch synchronisation)
    step_fns = [world.control_step_plan(workload.SUBSTEPS, o.data_ptr() if o is not None else 0, feet_idx, feet_idx if reset else None,
                                        gc0_d.data_ptr() if reset else 0, gv0_d.data_ptr() if reset else 0, N) for o in obs_b]
    bank_ptr = [b.data_ptr() for b in bank]

    def control_step(k):
        gath.acquire(k)                     # the gather that still reads this buffer (stream-side wait, the host runs on)
        step_fns[gath.slot(k)](bank_ptr[k % TARGET_BANK])
        gath.gather(k)

    drain = gath.drain

    def track_ages():                       # untimed passes only: age += 1, reset envs start again at 0
        world.get_stream()                  # (torch's kernels read the step's done flags on the borrowed stream: joins a pipelined step first)
        age_d.add_(1).mul_(1 - done_d.to(torch.int32))

    # ---- untimed: pre-roll into the stationary regime, then the caller's warm-up
    if pipelined and not world.set_step_pipelining(True):
        # RSB_STEP_PIPELINING=0, or a profiler that serialises dispatches (rocprofv3 --pmc): the library keeps the steps in lock-step
        pipelined = False
        if gath.pipe is not None:
            gath = ObsGatherer(N, obs_dim, dev, overlap=args.overlap_collective, force=args.force_collective)
            obs_b, nbuf = gath.local_bufs, gath.nbuf
            step_fns = [world.control_step_plan(workload.SUBSTEPS, o.data_ptr() if o is not None else 0, feet_idx, feet_idx if reset else None,
                                                gc0_d.data_ptr() if reset else 0, gv0_d.data_ptr() if reset else 0, N) for o in obs_b]
            drain = gath.drain
    # a plain run (no --full, one rank) times only the leg `value` reports: the resident leg where the world has a resident launch, else the per-step leg.
    # Its --warmup control steps then run through that leg (a resident launch of --warmup steps), after the pre-roll
    resident_wanted = not (args.no_resident or args.lockstep or args.obs_exchange == "peer" or args.early_termination or args.overlap_collective)
    lean = not args.full and not coll
    lean_resident = lean and resident_wanted and world.residency_status(0)
    kstep = 0
    for _ in range(args.preroll + (0 if lean_resident else args.warmup)):
        control_step(kstep)
        if reset:
            track_ages()
        kstep += 1
    drain()
    torch.cuda.synchronize()
    q_start, u_start = world.get_state()    # the population the timed region starts from (the CPU leg starts from it too)
    step_start = kstep

    # ---- the timed region(s).  N = 1: the pipelined steps (or lock-step with --lockstep).  N > 1: the combination that HAS run
    # before goes first - lock-step control steps + the all-gather in line on the launch stream (tests/test_distributed_gloo.py, rounds 1-3's
    # bench path) -, then the pipelined steps + gather on a side stream, which no hardware has run with N > 1 before the driver's scaling run,
    # under a guard (two_legs): if that leg raises on any rank, `value` is the first leg's.
    R = max(1, args.repeats)

    def per_step(step_fn):
        return lambda k0, n: [step_fn(k) for k in range(k0, k0 + n)]

    def timed(run_fn, drain_fn, k0):
        if coll:
            dist.barrier()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        err = None
        try:
            run_fn(k0, args.steps)
            drain_fn()
        except Exception as e:      # (kept until this rank has been through the collectives below: the other ranks are in them)
            err = e
        t_enq = time.perf_counter() - t0       # host side done; the GPU may still be working
        if coll:
            dist.barrier()
        torch.cuda.synchronize()
        el = time.perf_counter() - t0
        try:
            world.step_pipeline_join()           # (a pipeline fault surfaces HERE as RsbError: the library has replayed the steps in lock-step by then)
        except Exception as e:
            err = err or e
        t = torch.tensor([el], dtype=torch.float64, device=dev)
        by_rank = [el / args.steps * 1e3]
        if coll:
            every = torch.zeros(world_size, dtype=torch.float64, device=dev)
            dist.all_gather_into_tensor(every, t)
            by_rank = [float(x) / args.steps * 1e3 for x in every.cpu()]
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
        if err is not None:
            raise err
        return {"elapsed": float(t.item()), "ms_by_rank": by_rank, "t_enqueued": t_enq}

    def repeated(run_fn, drain_fn):
        """R fresh brackets of exactly --steps steps each, back to back (same sequence continued); the MEDIAN bracket is the leg's result, every
        bracket's time is kept beside it"""
        nonlocal kstep
        res = []
        for _ in range(R):
            res.append(timed(run_fn, drain_fn, kstep))
            kstep += args.steps
        order = sorted(range(R), key=lambda i: res[i]["elapsed"])
        pick = dict(res[order[(R - 1) // 2]])
        pick["repeats_elapsed"] = [r["elapsed"] for r in res]
        return pick

    def spread(r, scale):
        """value_repeats / min / max of a leg from its brackets' times (scale = env-steps per bracket)"""
        v = [scale / e for e in r["repeats_elapsed"]]
        return {"value_repeats": v, "value_min": min(v), "value_max": max(v), "repeats": len(v), "spread_rel": (max(v) - min(v)) / float(np.median(v))}

    def start_brackets():
        if args.no_kernel_events or not args.full:
            return 0
        stride = EVENT_STRIDE if args.steps >= 64 else 1      # (>= 16 brackets at the driver's --steps 20; a bracket costs ~7 us of stream time, stated in the line)
        n = R * ((args.steps + stride - 1) // stride)
        world.enable_timing(max(n, 2))
        world.set_timing_stride(stride)
        return n

    def leg_lockstep_inline():
        nonlocal kstep
        world.set_step_pipelining(False)
        g2 = ObsGatherer(N, obs_dim, dev, overlap=False, force=args.force_collective)
        fns2 = [world.control_step_plan(workload.SUBSTEPS, o.data_ptr() if o is not None else 0, feet_idx, feet_idx if reset else None,
                                        gc0_d.data_ptr() if reset else 0, gv0_d.data_ptr() if reset else 0, N) for o in g2.local_bufs]

        def step_inline(k):
            g2.acquire(k)
            fns2[g2.slot(k)](bank_ptr[k % TARGET_BANK])
            g2.gather(k)
        for _ in range(max(5, args.warmup // 4)):
            step_inline(kstep)
            kstep += 1
        g2.drain()
        r = repeated(per_step(step_inline), g2.drain)
        if args.dump_outputs:
            snap["first"] = last_step_outputs(world, g2.local(kstep - 1), done_d if reset else None)
        if g2.active:      # this rank's slice of the gathered block of the last step = its own block
            r["gathered_rows_of_this_rank_correct"] = bool(torch.equal(g2.gathered(kstep - 1)[rank * N:(rank + 1) * N], g2.local(kstep - 1)))
        r["obs_all_gather"] = g2.describe()
        return r

    n_in = 0

    def leg_primary():
        nonlocal kstep, n_in, q_start, u_start, step_start
        if lockstep_first_wanted:      # back into the pipelined regime before its timed region
            world.set_step_pipelining(True)
            for _ in range(max(5, args.warmup // 4)):
                control_step(kstep)
                kstep += 1
            drain()
            torch.cuda.synchronize()
            q_start, u_start = world.get_state()
            step_start = kstep
        n_in = start_brackets()
        r = repeated(per_step(control_step), drain)
        if args.dump_outputs:
            snap["second"] = last_step_outputs(world, gath.local_bufs[gath.slot(kstep - 1)], done_d if reset else None)
        if gath.active and hasattr(gath, "gathered"):      # this rank's slice of the gathered block of the last step = its own block
            torch.cuda.synchronize()
            r["gathered_rows_of_this_rank_correct"] = bool(torch.equal(gath.gathered(kstep - 1)[rank * N:(rank + 1) * N], gath.local(kstep - 1)))
        return r

    # ---- the RESIDENT leg (round 6; rsb_set_step_residency): the timed region's --steps control steps are ONE launch of the step kernel - an env block's
    # state stays in LDS, a wave's time is a sum over the control steps (the slowest-wave tail of every launch averages out), nothing is handed over between
    # launches.  Same sequence, same outputs per control step (obs block, done flags, resets); N > 1: the obs blocks of the launch's control steps are
    # all-gathered ONCE behind it ([steps, N, obs] per rank - one larger collective instead of --steps small ones).  Bit-identical to the lock-step
    # steps (tests/test_gpu_resident.py).  Runs under the same guard as the pipelined leg when N > 1.
    res_state = {"launch_ms": np.zeros(0), "gather": None}
    snap = {}           # --dump-outputs: the last control step's outputs of each leg, taken right after its timed brackets

    def leg_resident():
        nonlocal kstep
        world.set_step_residency(True)
        if not world.residency_status(0):
            raise RuntimeError("no resident kernel class for this configuration")
        if coll:
            obs_r = torch.empty((args.steps, N, obs_dim), dtype=torch.float32, device=dev)
            obs_all = torch.empty((world_size, args.steps, N, obs_dim), dtype=torch.float32, device=dev)
            stride_r = N * obs_dim
        else:
            obs_r, obs_all, stride_r = obs_b[0], None, 0
        fn = world.control_steps_plan(workload.SUBSTEPS, bank_all.data_ptr(), TARGET_BANK, obs_r.data_ptr(), stride_r, feet_idx, feet_idx if reset else None,
                                      gc0_d.data_ptr() if reset else 0, gv0_d.data_ptr() if reset else 0, N)

        def run(k0, n):
            fn(n, k0)
            if coll:
                world.get_stream()
                dist.all_gather_into_tensor(obs_all.view(world_size * args.steps * N, obs_dim), obs_r.view(args.steps * N, obs_dim))
        # untimed: two launches of the same length (the population is already stationary); a plain run: one launch of --warmup steps (at least one
        # step, so that the resident class's first-launch cost - code-object load, a compile on a cache miss - never lands in the timed bracket)
        for n_warm in ([max(1, args.warmup)] if lean else [args.steps, args.steps]):
            run(kstep, n_warm)
            kstep += n_warm
        torch.cuda.synchronize()
        events = args.full and not args.no_kernel_events
        if events:
            world.enable_timing(max(R, 2))
            world.set_timing_stride(1)
        l0 = world.residency_launches()
        r = repeated(run, lambda: None)
        assert world.residency_launches() - l0 == R, "the resident leg did not run resident launches"
        if events:
            res_state["launch_ms"] = world.read_kernel_ms(R).astype(np.float64)
            world.enable_timing(0)
        if coll:
            r["gathered_rows_of_this_rank_correct"] = bool(torch.equal(obs_all[rank], obs_r))
            res_state["gather"] = {"collective": "all_gather_into_tensor (RCCL) ONCE per resident launch", "bytes_per_rank": int(obs_r.numel() * 4),
                                   "block": [args.steps, N, obs_dim], "issued_on": "the launch stream, behind the launch"}
        if args.dump_outputs:
            snap["resident"] = last_step_outputs(world, obs_r[args.steps - 1] if coll else obs_r, done_d if reset else None)
        world.set_step_residency(False)
        return r

    # (RSB_BENCH_TWO_LEGS=1 with --force-collective: the N > 1 order of legs on ONE rank - the only way this path meets a GPU before the driver's scaling run)
    forced_two_legs = bool(os.environ.get("RSB_BENCH_TWO_LEGS")) and coll
    lockstep_first_wanted = (world_size > 1 or forced_two_legs) and pipelined

    def all_agree(ok):
        if not coll:
            return ok
        f = torch.tensor([1.0 if ok else 0.0], dtype=torch.float64, device=dev)
        dist.all_reduce(f, op=dist.ReduceOp.MIN)
        return float(f.item()) == 1.0

    def rows_ok_everywhere(r):
        """gathered_rows_of_this_rank_correct of a leg -> also ..._on_all_ranks (MIN over the ranks: rank 0 prints the line)"""
        if r is not None and coll and r.get("gathered_rows_of_this_rank_correct") is not None:
            r["gathered_rows_correct_on_all_ranks"] = all_agree(bool(r["gathered_rows_of_this_rank_correct"]))

    def spec_block():
        spec_mode, spec_n, gen_n = world.specialization_status()
        return {"mode": ("off", "cached", "compile")[spec_mode], "step_launches_specialized": spec_n, "step_launches_generic": gen_n,
                "what": "specialised code objects of the step kernel (raisimlib_amd/csrc/step_spec.h): the SAME kernel class compiled with the model's dimensions and the world's "
                        "switches as compile-time constants; results bit-identical to the ahead-of-time class (tests/test_gpu_spec.py); counts are this world's launches of all legs"}

    workload_text = (recipe.name + ", dt=0.0025, 4 sub-steps per control step fused in one launch"
                     + (", non-foot contact -> reset (rsg_anymal rule)" if reset else ", no resets")
                     + (", EARLY TERMINATION at the sub-step of the first non-foot contact (not upstream's rule)" if args.early_termination else "")
                     + ", obs (q,u,foot force) written each control step"
                     + f"; stationary regime: {args.preroll} untimed pre-roll control steps before --warmup")

    def state_at_end():
        iters = world.get_solver_iterations()
        counts, _ = world.get_contacts()
        q_end, _ = world.get_state()
        return {"solver_iters_mean": float(iters.mean()), "solver_iters_max": int(iters.max()),
                "contacts_per_env": float(counts.mean()), "base_height_mean": float(q_end[:, 2].mean())}

    if lean:
        # ---- a plain run: the leg `value` reports and nothing else (the other legs, the sampling pass behind `roofline` and the CPU leg: --full)
        leg = leg_resident() if lean_resident else leg_primary()
        total_env_steps = N * workload.SUBSTEPS * args.steps
        out = {
            "metric": recipe.metric,
            "value": total_env_steps / leg["elapsed"], "unit": "env-steps/s", "n_gpus": 1, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": leg["elapsed"] / args.steps * 1e3, "ms_per_step_by_rank": leg["ms_by_rank"], "higher_is_better": True, "scaling": "weak",
            **spread(leg, total_env_steps),
            "value_is": "the MEDIAN of `repeats` fresh brackets of exactly --steps control steps each (barrier + synchronise on both sides, MAX over ranks), back to back",
            "value_leg": "resident" if lean_resident else "pipelined" if pipelined else "lockstep",
            "resident_leg_error": None if lean_resident or not resident_wanted else "RuntimeError: no resident kernel class for this configuration",
            "specialization": spec_block(),
            "vs_baseline": None, "dtype": "f32", "data": "synthetic", "full": False,
            "config": {"workload": workload_text, "workload_version": 3,
                       "regime_name": (args.atlas_regime if args.config == 5 else "reset-on-non-foot-contact" if reset else "no-reset"),
                       "preroll_control_steps": args.preroll, "envs_per_gpu": N, "substeps_per_step": workload.SUBSTEPS,
                       "lanes_per_env": world.lanes_per_env(), "parallelism": "env-shard x1",
                       "warmup": (f"{max(1, args.warmup)} control steps in one resident launch after the pre-roll" if lean_resident else
                                  f"{args.warmup} control steps after the pre-roll")},
            "build": {"source_hash": world.L.rsb_source_hash().decode(), "library": os.path.relpath(os.path.realpath(__import__("raisimlib_amd")._capi.LIB_PATH), ROOT)},
            "host_enqueue_ms_per_step": leg["t_enqueued"] / args.steps * 1e3,
            "state_at_end": state_at_end(),
        }
        if args.dump_outputs:
            out["outputs"] = dump_outputs(args.dump_outputs, snap["resident" if lean_resident else "second"])
        world.close()
        return out

    legs = two_legs(leg_lockstep_inline if lockstep_first_wanted else None, leg_primary, all_agree)
    lockstep_first = legs["first"]
    value_leg, pipelined_leg_error = ("pipelined" if pipelined else "lockstep"), legs["error"]
    if legs["use"] == "second":
        elapsed, ms_by_rank, t_enqueued = legs["second"]["elapsed"], legs["second"]["ms_by_rank"], legs["second"]["t_enqueued"]
    else:       # the pipelined leg raised (here or on another rank): the line is the first leg's
        elapsed, ms_by_rank, t_enqueued = lockstep_first["elapsed"], lockstep_first["ms_by_rank"], lockstep_first["t_enqueued"]
        value_leg = "lockstep + in-line all-gather (the pipelined leg raised: see pipelined_leg_error)"
        try:
            world.set_step_pipelining(False)
        except Exception:
            pass
        pipelined = False
        n_in = 0
    kernel_ms_in = world.read_kernel_ms(n_in).astype(np.float64) if n_in else np.zeros(0)
    if n_in:
        world.enable_timing(0)
    primary_leg = legs["second"] if legs["use"] == "second" else lockstep_first
    rows_ok_everywhere(lockstep_first)
    rows_ok_everywhere(legs["second"])

    # ---- the resident leg, under a guard (N > 1: every rank agrees whether it counts; a leg that raised anywhere counts nowhere)
    res_leg, resident_leg_error = None, None
    if resident_wanted:
        try:
            res_leg = leg_resident()
        except Exception as e:
            resident_leg_error = f"{type(e).__name__}: {e}"
            try:
                world.set_step_residency(False)
            except Exception:
                pass
        if not all_agree(resident_leg_error is None):
            res_leg = None
            resident_leg_error = resident_leg_error or "the leg raised on another rank"
        rows_ok_everywhere(res_leg)

    # ---- sampling pass (untimed, same sequence continued; --full): every launch bracketed; resets and env ages recorded
    kernel_ms_s = np.zeros(0)
    resets = []
    sampled = SAMPLE_LAUNCHES if args.full else 0
    if sampled and not args.no_kernel_events:
        world.enable_timing(SAMPLE_LAUNCHES)
        world.set_timing_stride(1)
    for _ in range(sampled):
        control_step(kstep)
        if reset:
            track_ages()                    # (joins: the sampling pass's launches do not overlap, their brackets are the kernel's own duration)
            resets.append(done_d.sum())
        else:
            world.get_stream()
        kstep += 1
    drain()
    torch.cuda.synchronize()
    bracket_overhead_ms = None
    if sampled and not args.no_kernel_events:
        kernel_ms_s = world.read_kernel_ms(SAMPLE_LAUNCHES).astype(np.float64)
        world.enable_timing(0)
        # what an event pair measures with nothing in between, on the same stream: subtracted from the brackets
        evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(64)]
        for e0, e1 in evs:
            e0.record(stream)
            e1.record(stream)
        torch.cuda.synchronize()
        bracket_overhead_ms = float(np.median([e0.elapsed_time(e1) for e0, e1 in evs]))

    # ---- the same workload with every launch waiting for the one before it (rsb_set_step_pipelining off; --full): same bracket, same number of steps
    lockstep, lockstep_leg = None, lockstep_first
    if lockstep_first is not None:
        lockstep = lockstep_first["elapsed"]
    elif pipelined and args.full:
        world.set_step_pipelining(False)
        for _ in range(max(5, args.warmup // 4)):
            control_step(kstep)
            kstep += 1
        drain()
        lockstep_leg = repeated(per_step(control_step), drain)
        lockstep = lockstep_leg["elapsed"]
        world.set_step_pipelining(True)
    pipe_launches, pipe_joins = world.step_pipelining_stats()      # (also sets world.pipeline_overlaps: the probe found two streams on different hardware queues)
    env_steps_per_step = N * workload.SUBSTEPS
    total_env_steps = world_size * env_steps_per_step * args.steps
    value = total_env_steps / elapsed
    # what `value` is: the resident leg when it ran (on every rank), else the pipelined leg, else lock-step
    primary_value, primary_name = value, value_leg
    resident_value = total_env_steps / res_leg["elapsed"] if res_leg is not None else None
    # N = 1: the resident leg when it ran.  N > 1: the FASTER of the legs that succeeded on every rank (elapsed is the MAX over ranks, so all ranks agree):
    # the resident leg's one all-gather of [steps, N, obs] per launch sits behind the launch, the pipelined leg hides its per-step gathers on a side stream
    value_is_resident = res_leg is not None and (world_size == 1 or res_leg["elapsed"] <= elapsed)
    if value_is_resident:
        value = resident_value
        value_leg = "resident"
    spec_info = spec_block()
    iters = world.get_solver_iterations()
    counts, _ = world.get_contacts()
    q_end, _ = world.get_state()
    ages = age_d.cpu().numpy()
    resets = [float(r.item()) for r in resets]

    if rank == 0:
        bytes_per_env_step = BYTES_PER_ENV_STEP[args.config]
        roof = {"bound": "hbm", "achieved": None, "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": None, "traffic": None}
        if len(kernel_ms_s):
            raw = float(kernel_ms_s.mean())
            kmean_ms = raw - bracket_overhead_ms
            standalone_ms = kmean_ms
            eff_ms = elapsed / args.steps * 1e3
            if pipelined and len(kernel_ms_in):
                # two launches are in flight: a launch takes start -> end what the TIMED REGION's brackets say (waiting for SIMDs and for its
                # predecessors' envs included; rocprofv3's kernel durations of the same command are this number), and one completes every
                # ms_per_step.  The chip's rate is bytes per launch over that interval; bytes over one launch's duration is kept beside it
                raw = float(kernel_ms_in.mean())
                kmean_ms = raw - bracket_overhead_ms
                achieved = bytes_per_env_step * env_steps_per_step / (eff_ms * 1e-3) / 1e9
            else:
                achieved = bytes_per_env_step * env_steps_per_step / (kmean_ms * 1e-3) / 1e9
            traffic, traffic_src, pmc = recorded_traffic(args.config, N, workload.SUBSTEPS) if reset and not args.max_iter else (None, None, None)
            # what actually bounds the kernel: issue slots of the one wave each SIMD holds (recorded SQ_INSTS_VALU x 4 cycles
            # over the measured launch time at the 2.4 GHz shader clock), reported next to the HBM roofline
            valu = None
            if pmc and pmc.get("counters", {}).get("SQ_INSTS_VALU"):
                waves = -(-N * world.lanes_per_env() // 64)
                per_wave = pmc["counters"]["SQ_INSTS_VALU"] / waves
                cyc = (eff_ms if pipelined and len(kernel_ms_in) else kmean_ms) * 1e-3 * 2.4e9    # cycles a SIMD spends per wave and launch
                valu = {"valu_inst_per_wave_per_launch": per_wave,
                        "issue_slot_frac": per_wave * 4.0 / cyc,
                        "valu_pipe_frac": per_wave * 2.0 / cyc,
                        "note": "one wave per SIMD.  issue_slot_frac: (VALU instructions x 4 cycles) / launch cycles - the rate a LONE wave can issue at "
                                "(profiles/r02_ubench_lone_wave_latency.txt); valu_pipe_frac: the same at 2 cycles per wave64 instruction - what the "
                                "SIMD-32 pipe can take from SEVERAL co-resident waves (MI355X_MICROARCH.md; profiles/r04_ubench_two_waves.txt: two waves "
                                "per SIMD run dependent FMA chains and the sweep-loop mix at 0.8-1.0x the lone wave's time EACH).  Recorded PMC pass, measured launch time"}
            alg_bytes = bytes_per_env_step * env_steps_per_step
            fused_bytes = bytes_per_env_step * N          # with the sub-steps fused in one launch the state crosses HBM once per CONTROL step
            bw_thr = alg_bytes / (eff_ms * 1e-3) / 1e9          # over the interval between two launches' completions (= ms_per_step: what the chip sustains)
            bw_dur = alg_bytes / (kmean_ms * 1e-3) / 1e9        # over ONE launch's start -> end (pipelined launches overlap: this is the smaller number)
            if valu is not None:
                valu["recorded"] = True       # SQ_INSTS_VALU comes from the committed PMC pass named in traffic_source, not from this run
            roof = {"bound": "hbm", "achieved": achieved, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                    "frac": achieved / HBM_PEAK_GBS,
                    # both fractions under explicit names.  `frac` (the contract field) = frac_throughput when launches are
                    # pipelined, = frac_kernel_duration in lock-step (the two coincide there up to the launch gap)
                    "frac_throughput": bw_thr / HBM_PEAK_GBS, "frac_kernel_duration": bw_dur / HBM_PEAK_GBS,
                    "traffic": traffic, "traffic_source": traffic_src, "traffic_recorded": traffic is not None,
                    "fused_algorithmic_bytes_per_launch": fused_bytes,
                    "traffic_over_fused_algorithmic_bytes": (traffic / fused_bytes) if traffic else None,
                    "traffic_over_algorithmic_bytes": (traffic / alg_bytes) if traffic else None,
                    "kernel": "rsb_step_kernel", "kernel_ms_mean": kmean_ms,
                    "kernel_ms_p50": float(np.median(kernel_ms_s)) - bracket_overhead_ms,
                    "kernel_ms_max": float(kernel_ms_s.max()) - bracket_overhead_ms,
                    "kernel_launches_timed": int(len(kernel_ms_s)),
                    "kernel_ms_mean_bracket_raw": raw, "event_pair_overhead_ms": bracket_overhead_ms,
                    "timed_region_brackets": {"n": int(len(kernel_ms_in)), "stride": (EVENT_STRIDE if args.steps >= 64 else 1),
                                              "kernel_ms_mean": (float(kernel_ms_in.mean()) - bracket_overhead_ms) if len(kernel_ms_in) else None},
                    "method": f"HIP event pairs recorded by the library on the launch stream around each of {len(kernel_ms_s)} launches of a "
                              "sampling pass that continues the timed region's sequence; an empty event pair on the same stream is subtracted",
                    "algorithmic_bytes_per_env_step": bytes_per_env_step,
                    "algorithmic_bytes_per_launch": bytes_per_env_step * env_steps_per_step, "valu_issue": valu}
            if pipelined and len(kernel_ms_in):
                roof.update({"effective_ms_per_launch": eff_ms, "launches_in_flight": kmean_ms / eff_ms,
                             "achieved_over_one_launch_duration": bytes_per_env_step * env_steps_per_step / (kmean_ms * 1e-3) / 1e9,
                             "kernel_ms_standalone": standalone_ms,
                             "kernel_ms_p50": float(np.median(kernel_ms_in)) - bracket_overhead_ms, "kernel_ms_max": float(kernel_ms_in.max()) - bracket_overhead_ms,
                             "kernel_launches_timed": int(len(kernel_ms_in)),
                             "method": f"pipelined control steps: kernel_ms_* = start -> end of {len(kernel_ms_in)} launches of the TIMED REGION (every {EVENT_STRIDE}th; HIP event "
                                       "pairs recorded by the library on the launch's stream, an empty pair subtracted; rocprofv3 --kernel-trace reports the same "
                                       "durations) - two launches overlap, so `achieved` = algorithmic bytes per launch / effective_ms_per_launch (= ms_per_step), "
                                       "the rate the chip sustains; achieved_over_one_launch_duration divides by kernel_ms_mean instead; kernel_ms_standalone = a "
                                       "pipelined launch with nothing else in flight (sampling pass: joined after every step)"})
        if value_is_resident and len(res_state["launch_ms"]) and roof.get("achieved") is not None:
            # `value` is the resident leg: the dominant kernel is the resident class of rsb_step_kernel, ONE launch = --steps control steps.  Algorithmic bytes
            # per launch = SURVEY 8d's contract figure x env-steps per launch (the unfused 456 B / env-step - never the fused figure silently); duration = the
            # launch's own start -> end (HIP event pair recorded by the library on the launch stream, one per repeat).  Nothing overlaps it: throughput and
            # kernel-duration fractions coincide up to the launch gap.
            lms = res_state["launch_ms"] - bracket_overhead_ms
            alg_launch = bytes_per_env_step * env_steps_per_step * args.steps
            ach = alg_launch / (float(lms.mean()) * 1e-3) / 1e9
            t_res, t_src, _ = recorded_traffic(args.config, N, workload.SUBSTEPS, resident=True) if reset and not args.max_iter else (None, None, None)
            traffic_launch = t_res * args.steps if t_res else None      # (recorded per CONTROL STEP of a resident launch)
            fused_launch = bytes_per_env_step * N * args.steps
            roof = {"bound": "hbm", "achieved": ach, "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": ach / HBM_PEAK_GBS,
                    "frac_throughput": alg_launch / res_leg["elapsed"] / 1e9 / HBM_PEAK_GBS, "frac_kernel_duration": ach / HBM_PEAK_GBS,
                    "traffic": traffic_launch, "traffic_source": t_src, "traffic_recorded": traffic_launch is not None,
                    "fused_algorithmic_bytes_per_launch": fused_launch,
                    "traffic_over_fused_algorithmic_bytes": (traffic_launch / fused_launch) if traffic_launch else None,
                    "traffic_over_algorithmic_bytes": (traffic_launch / alg_launch) if traffic_launch else None,
                    "kernel": "rsb_step_kernel (resident class: --steps control steps per launch)", "control_steps_per_launch": args.steps,
                    "kernel_ms_mean": float(lms.mean()), "kernel_ms_p50": float(np.median(lms)), "kernel_ms_max": float(lms.max()), "kernel_launches_timed": int(len(lms)),
                    "kernel_ms_per_control_step": float(lms.mean()) / args.steps, "event_pair_overhead_ms": bracket_overhead_ms,
                    "method": f"HIP event pair recorded by the library on the launch stream around each of the {len(lms)} resident launches of the timed brackets "
                              "(one launch = one bracket = --steps control steps); an empty event pair on the same stream is subtracted",
                    "algorithmic_bytes_per_env_step": bytes_per_env_step, "algorithmic_bytes_per_launch": alg_launch,
                    "valu_issue": roof.get("valu_issue"),
                    "control_step_launches": roof}      # the per-control-step launches of the pipelined / lock-step legs, as round 5 reported them
        age_pct = [int(x) for x in np.percentile(ages, [10, 50, 90, 99])] if reset else None
        out = {
            "metric": recipe.metric,
            "value": value, "unit": "env-steps/s", "n_gpus": world_size, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": (res_leg if value_is_resident else primary_leg)["elapsed"] / args.steps * 1e3,
            "ms_per_step_by_rank": (res_leg if value_is_resident else primary_leg)["ms_by_rank"], "higher_is_better": True, "scaling": "weak",
            **spread(res_leg if value_is_resident else primary_leg, total_env_steps),
            "value_is": "the MEDIAN of `repeats` fresh brackets of exactly --steps control steps each (barrier + synchronise on both sides, MAX over ranks), back to back",
            "value_leg": value_leg, "pipelined_leg_error": pipelined_leg_error, "resident_leg_error": resident_leg_error,
            "specialization": spec_info,
            "resident": ({"value": resident_value, "unit": "env-steps/s", "ms_per_step": res_leg["elapsed"] / args.steps * 1e3, "steps": args.steps, **spread(res_leg, total_env_steps),
                          "launches_per_bracket": 1, "obs_all_gather": res_state["gather"], "gathered_rows_of_this_rank_correct": res_leg.get("gathered_rows_of_this_rank_correct"),
                          "gathered_rows_correct_on_all_ranks": res_leg.get("gathered_rows_correct_on_all_ranks"),
                          "what": "rsb_control_steps with rsb_set_step_residency: the bracket's --steps control steps are ONE launch of the step kernel's resident class - env blocks "
                                  "stay in LDS, terminated envs restart in LDS, obs block / done flags go to HBM per control step, state / warm / contact records after the "
                                  "last one; bit-identical to the lock-step steps (tests/test_gpu_resident.py)"} if res_leg is not None else None),
            "pipelined": ({"value": primary_value, "unit": "env-steps/s", "ms_per_step": elapsed / args.steps * 1e3, "steps": args.steps, **spread(primary_leg, total_env_steps),
                           "leg": primary_name, "gathered_rows_of_this_rank_correct": primary_leg.get("gathered_rows_of_this_rank_correct"),
                           "gathered_rows_correct_on_all_ranks": primary_leg.get("gathered_rows_correct_on_all_ranks"), "what": "round 5's `value`: one launch per control step, consecutive launches overlapping on the device (rsb_set_step_pipelining)"}
                          if res_leg is not None else None),
            "vs_baseline": None, "dtype": "f32", "data": "synthetic", "full": args.full,
            "config": {
                "workload": workload_text,
                # the workload definitions behind the metric strings changed in round 3 (config 3: bases spread over +-6 m of the map instead
                # of its centre; config 5: the STANDING regime is the default, rounds 1-2 measured what is now --atlas-regime collapsing):
                # lines are comparable only at equal workload_version (and regime_name for config 5)
                "workload_version": 3, "regime_name": (args.atlas_regime if args.config == 5 else "reset-on-non-foot-contact" if reset else "no-reset"),
                "preroll_control_steps": args.preroll,
                "regime": {"resets_per_control_step_mean": float(np.mean(resets)) if resets else None,
                           "env_age_control_steps_p10_p50_p90_p99": age_pct,
                           "sampled_over_control_steps": sampled},
                "envs_per_gpu": N, "substeps_per_step": workload.SUBSTEPS,
                "contact_solver": {"max_iter": args.max_iter or 150, "threshold_rel": 1e-5, "alpha": [1.0, 1.0, 1.0],
                                   "sweep": "grouped (block Jacobi across limbs, Gauss-Seidel within a limb)",
                                   "friction_directions_lag_after_sweeps": args.freeze_after if args.freeze_after >= 0 else 6,
                                   "stagnation_exit": {"window": args.stall_window if args.stall_window >= 0 else 4, "factor": 0.5},
                                   "multi_contact_envs": {"min_contacts_on_one_limb": recipe.multi_contact[0], "light_passes": bool(recipe.multi_contact[1]),
                                                          "friction_directions_lag_after_sweeps": recipe.multi_contact[2], "stagnation_window": recipe.multi_contact[3],
                                                          "anderson_depth1": ({"first_sweep": recipe.anderson[0], "clip": recipe.anderson[1]} if recipe.kmax > 8 and recipe.anderson[0] > 0 else None)},
                                   "warm_start": True},
                "self_collision": {"enabled": not args.no_self_collision, "candidate_pairs": int(len(world.self_collision_pairs()))},
                "lanes_per_env": world.lanes_per_env(), "parallelism": f"env-shard x{world_size}",
                "step_pipelining": ("on: consecutive control-step launches overlap at workgroup granularity (rsb_set_step_pipelining; results bit-identical to "
                                    "lock-step, tests/test_gpu_pipeline.py); `lockstep` = the same steps with every launch waiting for the one before it"
                                    if pipelined else "off (--lockstep)" if args.lockstep else "off (the peer-mapped exchange has no pipelined kernel class)"
                                    if args.obs_exchange == "peer" else "off (RSB_STEP_PIPELINING=0 or a dispatch-serialising profiler in the environment)"),
                "step_pipelining_stats": ({"pipelined_launches": pipe_launches, "joins": pipe_joins, "streams_overlap": bool(world.pipeline_overlaps)} if pipelined else None),
                "obs_all_gather": gath.describe(),
            },
            "roofline": roof,
            "rccl": rccl_info,
            "lockstep": ({"value": total_env_steps / lockstep, "unit": "env-steps/s", "ms_per_step": lockstep / args.steps * 1e3, "steps": args.steps, **spread(lockstep_leg, total_env_steps),
                          "ran_first": lockstep_first is not None, "obs_all_gather": (lockstep_first or {}).get("obs_all_gather"),
                          "gathered_rows_of_this_rank_correct": (lockstep_first or {}).get("gathered_rows_of_this_rank_correct"),
                          "gathered_rows_correct_on_all_ranks": (lockstep_first or {}).get("gathered_rows_correct_on_all_ranks"),
                          "what": "rsb_set_step_pipelining off, same bracket: every launch waits for the slowest wave of the one before it (what a caller "
                                  "gets that consumes each step's output before issuing the next step, e.g. a policy in the loop)"} if lockstep else None),
            "build": {"source_hash": world.L.rsb_source_hash().decode(), "library": os.path.relpath(os.path.realpath(__import__("raisimlib_amd")._capi.LIB_PATH), ROOT)},
            "host_enqueue_ms_per_step": (res_leg["t_enqueued"] if value_is_resident else t_enqueued) / args.steps * 1e3,
            "state_at_end": {"solver_iters_mean": float(iters.mean()), "solver_iters_max": int(iters.max()),
                             "contacts_per_env": float(counts.mean()), "base_height_mean": float(q_end[:, 2].mean())},
        }
        if world_size == 1 and not args.no_cpu and args.full:
            # the CPU leg runs AFTER every GPU leg of the run (main): 16 busy threads exhaust the box's CPU quota, and a throttled host thread
            # cannot feed a 2 ms timed region (measured: the secondary configurations lost up to 30 % at --steps 20 behind a CPU leg)
            cpu_seconds, max_iter, nsc = args.cpu_seconds, args.max_iter, not args.no_self_collision
            gcf = gc0.astype(np.float32).astype(np.float64)
            out["_cpu_leg"] = lambda: cpu_baseline(recipe, max_iter, reset, cpu_seconds, q_start, u_start, gcf, gv0, step_start, self_collision=nsc)
        if args.dump_outputs:       # the leg `value` reports, right after its timed brackets
            out["outputs"] = dump_outputs(args.dump_outputs, snap["resident" if value_is_resident else legs["use"]])
    world.close()
    return out


DUMP_BYTES_MAX = 64 << 20          # --dump-outputs: at most this many bytes in all; above it, the same seeded sample of envs from every array
DUMP_SEED = 20240229


def last_step_outputs(world, obs, done):
    """What a caller of the timed leg receives from its last control step, as host float32 arrays of one row per env: the observation block
    (device buffer `obs`, None where the exchange keeps no local block), the termination flags (device buffer `done`, None without resets) and the
    state the world holds after the step."""
    import torch
    world.get_stream()                  # (joins a pipelined step before torch reads the buffers it writes)
    torch.cuda.synchronize()
    gc, gv = world.get_state()
    out = {"gc": gc, "gv": gv}
    if obs is not None:
        out["obs"] = obs.float().cpu().numpy()
    if done is not None:
        out["done"] = done.cpu().numpy().astype(np.float32)
    return {k: np.ascontiguousarray(v, dtype=np.float32) for k, v in out.items()}


def dump_outputs(dirname, arrays):
    """--dump-outputs: one DIR/<name>.npy per array (rows = envs).  Above DUMP_BYTES_MAX the same seeded sample of rows is kept from every array
    and its env indices are written beside them (env_index.npy).  Returns {name: shape} as written."""
    os.makedirs(dirname, exist_ok=True)
    n = next(iter(arrays.values())).shape[0]
    row_bytes = sum(a.nbytes // max(a.shape[0], 1) for a in arrays.values())
    if n * row_bytes > DUMP_BYTES_MAX:
        keep = max(1, DUMP_BYTES_MAX // (row_bytes + 8))
        idx = np.sort(np.random.default_rng(DUMP_SEED).choice(n, size=keep, replace=False))
        arrays = {k: v[idx] for k, v in arrays.items()}
        arrays["env_index"] = idx.astype(np.float64)
    for k, v in arrays.items():
        np.save(os.path.join(dirname, k + ".npy"), v)
    return {k: list(v.shape) for k, v in arrays.items()}


def finish_cpu_leg(o):
    leg = o.pop("_cpu_leg", None) if o else None
    if leg is not None:
        o["cpu_baseline"] = leg()


def main():
    args = parse()
    if args.repeats is None:       # (a plain run times exactly --steps steps; the diagnostic --closed-loop-only keeps its seven brackets per leg)
        args.repeats = 7 if args.full or args.closed_loop_only else 1
    if "WORLD_SIZE" not in os.environ and args.gpus > 1:
        # started without a launcher: this process becomes the launcher of --gpus ranks (one per GPU)
        sys.exit(spawn_ranks(args))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world_size = int(os.environ.get("WORLD_SIZE", "1"))
    if world_size != args.gpus and rank == 0:
        print(f"bench.py: --gpus {args.gpus} but the launcher started {world_size} rank(s); the launcher's count is used", file=sys.stderr)
    if args.dry_run_ranks:
        sys.exit(dry_run_ranks(args, rank, world_size))
    os.environ.setdefault("RSB_SPECIALIZE", {"compile": "compile", "cached": "1", "off": "0"}[args.specialization])   # every world of this process (the library reads it at rsb_create)
    os.environ.setdefault("HIP_FORCE_DEV_KERNARG", "1")   # kernel arguments in device memory (this image's default; see rsb_world.hip)
    # the closed loop runs three streams that must overlap (two step streams + the action stage's) beside the caller's: HIP's default of 4 hardware queues
    # can alias them (action-stage waits then time out, pipeline fault code 6), also where the environment names that default explicitly
    if int(os.environ.get("GPU_MAX_HW_QUEUES") or 0) < 8:
        os.environ["GPU_MAX_HW_QUEUES"] = "8"
    import torch
    import torch.distributed as dist

    from raisimlib_amd import BatchedWorld, workload

    if args.share_device:
        local_rank = 0          # every rank on cuda:0
    if torch.cuda.device_count() <= local_rank:
        raise SystemExit(f"bench.py: rank {rank} needs GPU {local_rank}, this node shows {torch.cuda.device_count()} (no CPU fallback)")
    coll = world_size > 1 or args.force_collective     # the obs all-gather is part of the step
    if coll:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29500")
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    if coll:
        if args.backend == "nccl":
            dist.init_process_group("nccl", rank=rank, world_size=world_size, device_id=dev)
        else:
            dist.init_process_group("gloo", rank=rank, world_size=world_size)

    if args.closed_loop_only:
        print(json.dumps({"closed_loop": closed_loop_leg(args, dev, args.envs_per_gpu)}), flush=True)
        return
    out = measure(args, rank, local_rank, world_size, dev, coll)
    default_run = (args.full and world_size == 1 and args.config == 2 and not args.no_secondary and not args.no_cpu and args.envs_per_gpu == ENVS_PER_GPU
                   and not (args.early_termination or args.no_reset or args.max_iter or args.lanes_per_env or args.no_self_collision or args.force_collective or args.lockstep))
    if rank == 0 and default_run:
        # what the driver's default run also records: the other single-GPU configurations of BASELINE.json with
        # the same --steps / --warmup, and the headline workload through the reference's own boundary
        import copy
        out["secondary"] = {}
        second = {}
        for cfg in (3, 5):          # the GPU legs first, ...
            a2 = copy.copy(args)
            a2.config, a2.cpu_seconds = cfg, min(args.cpu_seconds, 7.0)
            a2.dump_outputs = None      # (DIR holds the headline's outputs only)
            try:
                second[cfg] = measure(a2, rank, local_rank, world_size, dev, coll)
            except Exception as e:      # a secondary line must never take the headline down
                out["secondary"][f"config{cfg}"] = {"error": f"{type(e).__name__}: {e}"}
        # ... the headline workload with a policy in the loop (closed-loop pipeline, include/rsb_pipeline.h) ...
        try:
            out["closed_loop"] = closed_loop_leg(args, dev, args.envs_per_gpu)
        except Exception as e:
            out["closed_loop"] = {"error": f"{type(e).__name__}: {e}"}
        # ... then the headline workload through the reference's own boundary (host threads + GPU; two attempts, both reported: 32 actively
        # waiting threads on a 16-CPU quota are sometimes throttled as a group for a whole attempt, profiles/r04_ab_log.txt) ...
        try:
            # (SUSTAINED: >= 600 control steps = several 100-ms cgroup periods per attempt, whatever --steps says)
            tries = sorted((template_path(args.envs_per_gpu, max(args.steps // 4, 600)) for _ in range(3)), key=lambda t_: t_["env_steps_per_s"])
            best = tries[1]         # the MEDIAN of three attempts, all three listed
            best["attempts_env_steps_per_s"] = [t_["env_steps_per_s"] for t_ in tries]
            best["value_is"] = "median of 3 attempts"
            out["boundary_template_path"] = best
        except Exception as e:
            out["boundary_template_path"] = {"error": f"{type(e).__name__}: {e}"}
        finish_cpu_leg(out)         # ... then the CPU legs
        for cfg, o2 in second.items():
            try:
                finish_cpu_leg(o2)
                r2, c2 = o2["roofline"], o2.get("cpu_baseline") or {}
                out["secondary"][f"config{cfg}"] = {
                    "metric": o2["metric"], "value": o2["value"], "unit": o2["unit"], "steps": o2["steps"], "warmup": o2["warmup"], "ms_per_step": o2["ms_per_step"],
                    "lockstep_value": (o2.get("lockstep") or {}).get("value"), "kernel_ms_mean": r2.get("kernel_ms_mean"), "roofline": {k: r2.get(k) for k in ("bound", "achieved", "peak", "unit", "frac", "traffic", "algorithmic_bytes_per_launch")},
                    "cpu_baseline": {k: c2.get(k) for k in ("value", "unit", "cores", "kind", "sample")} if c2 else None,
                    "workload": o2["config"]["workload"], "regime": o2["config"]["regime"], "state_at_end": o2["state_at_end"]}
            except Exception as e:      # a secondary line must never take the headline down
                out["secondary"][f"config{cfg}"] = {"error": f"{type(e).__name__}: {e}"}
    finish_cpu_leg(out)
    if coll:
        dist.destroy_process_group()
    if rank == 0:
        try:    # RCCL writes its version banner through C stdio; flush it so that the JSON line is the last line
            import ctypes
            ctypes.CDLL(None).fflush(None)
        except Exception:
            pass
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
