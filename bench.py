#!/usr/bin/env python3
"""Headline benchmark: Gram entries/s of the signature-PDE-kernel hot path on MI355X.

    python bench.py [--gpus N] [--steps K] [--warmup W] [--config c3|c2|c4|c4mini|c5] [--scaling weak|strong]
                    [--dump-outputs DIR] [--full]
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 \
           --master-port P bench.py --gpus N --steps K --warmup W

Either launch works: started as plain `python bench.py --gpus N` (no WORLD_SIZE in the environment) with N > 1, the script
re-executes itself under torch.distributed.run with N ranks on 127.0.0.1 and a free port, one rank per GPU (LOCAL_RANK ->
device), and rank 0's JSON line comes out of the same stdout.

A "step" is one pass of the hot path over one batch of synthetic paths already resident in HBM:
  * gram configs (c2, c3, c4mini, c5): one SigKernel.compute_Gram call (static kernel -> increments -> PDE solve);
  * c4 (BASELINE configs[3]): one compute_mmd(X, Y).backward() -- three Gram matrices and two adjoint-PDE Grams.
The default is BASELINE.json configs[2], the headline: batch 512 x 512, len 128, dim 8, LinearKernel, dyadic 1, fp64.

N > 1 runs the PRODUCT's sharding, SigKernel(process_group=WORLD) (sigkernel_amd/distributed.py): the rows of X are
split over the ranks, every rank solves its block with no data-path collective, and one RCCL all-gather assembles the
full matrix on every rank.  --scaling weak (default for gram configs): X has N x rows_per_gpu rows; --scaling strong
(default and only choice for c4, the config BASELINE names for 8 GPUs): the batch is fixed and divided.

A plain run does only what the headline needs: set up, W warm-up steps, the K timed steps, the outputs of the last step
(--dump-outputs DIR: DIR/<name>.npy, see dump_outputs) and rank 0's JSON line with the contract fields (metric, value, unit,
higher_is_better, dtype, ms_per_step) and the config.  Everything else is measured only with --full:

With N > 1 (or --force-dist) the line's `configs` holds BASELINE configs[3] (the config BASELINE.json names for 8 GPUs) and configs[4]
STRONG-scaled under the same process group (dist_configs), beside the other scaling of the headline config and the per-step time in the
collectives; at N = 1 without it, `configs` holds c2, two training-sized MMD steps, c5, c4.

With --full, rank 0's JSON line also carries
  roofline     : the kernel that dominates the step against the ceiling that binds it (fp64 vector issue for the fused
                 kernels, with the HBM-equivalent rate of the increments they never materialise as a second figure;
                 HBM for the streaming solver), from HIP-event timings of its launches on the launch stream
  adjoint      : forward-with-edges + adjoint at the same shape (HIP events), against 3 (M-1)(N-1) s bytes per entry
  cpu_baseline : the CPU oracle (C restatement of the reference's Cython solver) on this box's host cores, on a bounded
                 sample of the same workload: all threads (value) and one thread (the reference is single-threaded)
  parity       : 64 random entries of the timed output and sampled gradient rows re-computed by the oracle
"""
import argparse
import json
import os
import sys
import time



def _cpu_quota_threads():
    """Hardware threads this process may really use: those visible, capped by the container's cgroup CPU quota (cgroup v2 cpu.max)."""
    n = min(os.cpu_count() or 1, len(os.sched_getaffinity(0)))
    try:
        q, per = open("/sys/fs/cgroup/cpu.max").read().split()[:2]
        if q != "max":
            n = min(n, max(1, int(-(-float(q) // float(per)))))
    except Exception:      # noqa: BLE001
        pass
    return max(1, n)


# The GPU boxes show 256 hardware threads under a 16-CPU cgroup quota.  Every OpenMP runtime in the process (torch's intra-op pool,
# numpy's BLAS, the oracle's libgomp) would start 256 threads that spin at their barriers, burn the quota and get the WHOLE process
# throttled -- measured: the parity / baseline phases of this script took 12 s in one run and 340 s in the next.  So, BEFORE torch and
# numpy are imported: as many threads as the quota allows, sleeping when idle, not pinned (the host is shared with other boxes).
# (N ranks on one node share the quota)
_QUOTA_THREADS = max(1, _cpu_quota_threads() // max(1, int(os.environ.get("LOCAL_WORLD_SIZE", os.environ.get("WORLD_SIZE", "1")))))
os.environ.setdefault("OMP_NUM_THREADS", str(_QUOTA_THREADS))
os.environ.setdefault("MKL_NUM_THREADS", str(_QUOTA_THREADS))
os.environ.setdefault("OPENBLAS_NUM_THREADS", str(_QUOTA_THREADS))
os.environ.setdefault("OMP_WAIT_POLICY", "passive")
os.environ.setdefault("OMP_PROC_BIND", "false")

import numpy as np  # noqa: E402
import torch  # noqa: E402

torch.set_num_threads(_QUOTA_THREADS)
ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

import sigkernel_amd  # noqa: E402
from sigkernel_amd import _lib  # noqa: E402

HBM_PEAK_GBS = 8000.0        # MI355X HBM3E peak, /opt/skills/guides/MI355X_MICROARCH.md
# MI355X fp64 VECTOR peak (FMA = 2 flop): SURVEY 8(d)'s figure, AMD's public 78.6 TFLOP/s = 256 CUs x 4 SIMDs x 16 fp64 FMA lanes/clk
# x 2 flop x 2.4 GHz -- half of the 157.3 TFLOP/s the microarchitecture guide lists for FP32 (vector and matrix); the guide has no
# fp64 row of its own
FP64_VECTOR_PEAK_TF = 78.6
PEAK_SOURCE = ("SURVEY 8(d): AMD's public MI355X fp64 VECTOR figure, 78.6 TFLOP/s = 256 CUs x 4 SIMDs x 16 fp64 FMA lanes/clk x 2 flop x "
               "2.4 GHz -- half of the 157.3 TFLOP/s FP32 vector / matrix rows of /opt/skills/guides/MI355X_MICROARCH.md, which has no "
               "fp64 row; tools/ubench/fma_rate measures 63 TFLOP/s of independent v_fma_f64 at the ~2.1 GHz the chip sustains")


def fwd_ops_per_pair(kname, D, Mc, Nc, dyadic):
    """FMA-class fp64 lane operations of one forward PDE with the static kernel inside: 3 per fine cell (the stencil) + per coarse
    cell 3 (linear, on the pre-scaled increment) or 4 (rbf) coefficient operations + the static kernel (linear: D FMAs; rbf: 2 D for
    the distance, 19 for the exponential, 4 for the 4-corner difference)."""
    per_coarse = (3 + D) if kname == "linear" else (4 + 2 * D + 23)
    return ((Mc << dyadic) * (Nc << dyadic)) * 3 + Mc * Nc * per_coarse


def adj_ops_per_pair(kname, D, Mc, Nc, dyadic):
    """... of one fused adjoint: 7 per fine cell (the reverse stencil 3, K recomputed backwards 3, their product 1) + per coarse cell
    10 coefficient operations (a, b, 1/b by Newton, a/b) + the static kernel's chain rule (rbf: the node 2 D + 21, the 4-corner
    difference 3, the weights' 4-corner sums and products 12, the 2 D accumulators; linear: D for the increment, D + 1 for W dy)."""
    per_coarse = (11 + 2 * D) if kname == "linear" else (46 + 4 * D)
    return ((Mc << dyadic) * (Nc << dyadic)) * 7 + Mc * Nc * per_coarse

CONFIGS = {
    # name: rows of X (per GPU under weak scaling), B, M, N, D, static kernel, dyadic, dtype, mode, description
    "c3": dict(A=512, B=512, M=128, N=128, D=8, kernel="linear", dyadic=1, dtype=torch.float64, mode="gram",
               desc="BASELINE configs[2]: batch 512x512, len 128, dim 8, LinearKernel, dyadic 1, fp64, compute_Gram sym=False"),
    "c2": dict(A=128, B=128, M=64, N=64, D=3, kernel="rbf", dyadic=1, dtype=torch.float64, mode="gram", sym=True,
               desc="BASELINE configs[1]: batch 128, len 64, dim 3, RBFKernel(1.0), dyadic 1, fp64, compute_Gram(X, X, sym=True) "
                    "(entries = the 128 x 128 matrix returned; the 8256 pairs on and above the diagonal are solved)"),
    "c4": dict(A=2048, B=2048, M=64, N=64, D=4, kernel="rbf", dyadic=2, dtype=torch.float64, mode="mmd",
               desc="BASELINE configs[3]: batch_x 2048, batch_y 2048, len 64, dim 4, RBFKernel(1.0), dyadic 2, fp64, "
                    "compute_mmd(X, Y).backward() (3 Gram matrices + 2 adjoint-PDE Grams), Gram rows sharded over the GPUs"),
    "c4mini": dict(A=512, B=512, M=64, N=64, D=4, kernel="rbf", dyadic=2, dtype=torch.float64, mode="gram",
                   desc="BASELINE configs[3] reduced to 512x512 pairs: len 64, dim 4, RBFKernel(1.0), dyadic 2, fp64, compute_Gram"),
    "mmd64": dict(A=64, B=64, M=64, N=64, D=3, kernel="rbf", dyadic=1, dtype=torch.float64, mode="mmd",
                  desc="a training-sized step: compute_mmd(X, Y).backward(), 64 x 64 paths of BASELINE configs[1]'s shape (len 64, dim 3, "
                       "RBFKernel(1.0), dyadic 1, fp64)"),
    "mmd32": dict(A=32, B=32, M=64, N=64, D=3, kernel="rbf", dyadic=1, dtype=torch.float64, mode="mmd",
                  desc="a training-sized step: compute_mmd(X, Y).backward(), 32 x 32 paths of BASELINE configs[1]'s shape"),
    "c5": dict(A=256, B=256, M=512, N=512, D=16, kernel="rbf", dyadic=2, dtype=torch.float32, mode="gram",
               desc="BASELINE configs[4]: batch 256x256, len 512, dim 16, RBFKernel(1.0), dyadic 2, fp32, compute_Gram "
                    "(grid 2044x2044 per pair)"),
}


def make_paths(A, M, D, seed, dtype):
    """Scaled random walks: kernel values stay O(1)."""
    g = torch.Generator().manual_seed(seed)
    X = torch.cumsum(torch.randn(A, M, D, generator=g, dtype=torch.float64), dim=1) / np.sqrt(M * D)
    return X.to(dtype)


def static_kernel(name):
    return sigkernel_amd.LinearKernel() if name == "linear" else sigkernel_amd.RBFKernel(1.0)


def cpu_model():
    try:
        for line in open("/proc/cpuinfo"):
            if line.startswith("model name"):
                return line.split(":", 1)[1].strip()
    except OSError:
        pass
    return "unknown"


def usable_threads():
    """Threads the oracle may run on: the hardware threads visible to the process capped by the container's cgroup CPU quota (16 on the
    GPU boxes, which show 256 hardware threads; see the top of this file)."""
    return _QUOTA_THREADS


def cpu_baseline(Xc, Yc, kname, dyadic, budget_s=20.0):
    """Time the CPU oracle (kind "port": the reference is Python/Cython and cannot travel) on a bounded sample of the SAME
    workload: the first `rows` rows of X against all of Y, every pair's static kernel + increments + PDE solve inside ONE
    OpenMP region (oracle.gram_pipeline: per-thread scratch, first touch by the thread that uses it) -- on every host thread
    (`value`, the generous baseline the >= 10x target is judged against) and on ONE thread (`single_thread_value`: the
    reference's Cython solver is single-threaded, cython_backend.pyx:75,100).  `speedup_over_1_thread` says how well the
    all-threads figure scales; the round-2 baseline (torch static kernel + serial increments outside the parallel solve)
    reached 5x on 128 threads."""
    from oracle import oracle as O
    cores = os.cpu_count() or 1
    quota = cgroup_cpu_quota()
    # threads = the CPUs this process may actually use: the box's hardware threads capped by the container's cgroup CPU quota
    # (16 on the round-3 GPU boxes -- 256 hardware threads are visible, but more than 16 busy threads are throttled: measured
    # 16.6x on 16 threads, 14.8x on 128)
    threads = usable_threads()
    B, M, N = Yc.shape[0], Xc.shape[1], Yc.shape[1]
    kind, param = (0, 1.0) if kname == "linear" else (1, 1.0)
    Xn, Yn = Xc.double().numpy(), Yc.double().numpy()

    def run(x, y, nthreads):
        t0 = time.perf_counter()
        vals = O.gram_pipeline(x, y, kind, param, dyadic, nthreads=nthreads)
        return vals, time.perf_counter() - t0

    run(Xn[:1], Yn, threads)                       # warm-up: thread pool, page faults
    # calibrate on a prefix, then size each sample to its share of the budget: 60 % all threads, 40 % one thread
    nb1 = max(1, min(B, 32))
    _, t1 = run(Xn[:1], Yn[:nb1], 1)
    per_pair_1t = t1 / nb1
    crow = max(1, min(Xc.shape[0], 4))
    _, tm = run(Xn[:crow], Yn, threads)
    per_row_mt = tm / crow
    rows = int(max(1, min(Xc.shape[0], 0.6 * budget_s / max(per_row_mt, 1e-9))))
    vals, t_all = run(Xn[:rows], Yn, threads)
    pairs = rows * B
    n1 = int(max(1, min(Xc.shape[0] * B, 0.4 * budget_s / max(per_pair_1t, 1e-9))))
    rows1, b1 = (n1 // B, B) if n1 >= B else (1, n1)
    _, t_1 = run(Xn[:rows1], Yn[:b1], 1)
    b1 = rows1 * b1
    return {
        "value": pairs / t_all,
        "unit": "entries/s",
        "cores": threads,
        "kind": "port",
        "cpu_model": cpu_model(),
        "sample": "first %d of %d rows of X against all %d paths of Y (%d pairs, len %dx%d, dyadic %d); static kernel + increments "
                  "+ solve per pair inside one OpenMP region (oracle.gram_pipeline), %d threads"
                  % (rows, Xc.shape[0], B, pairs, M, N, dyadic, threads),
        "seconds": t_all,
        "single_thread_value": b1 / t_1,
        "single_thread_sample": "%d pairs (%d row(s) of X), same code on 1 thread, %.1f s" % (b1, rows1, t_1),
        "threads_used": threads,
        "speedup_over_1_thread": (pairs / t_all) / (b1 / t_1),
        "host_hardware_threads": cores,
        "cgroup_cpu_quota": quota,
        "linear_extrapolation_to_all_hardware_threads": (b1 / t_1) * cores,
        "note": "threads_used = hardware threads visible to the process capped by its cgroup CPU quota (beyond it the kernel "
                "throttles: more threads do not run faster); the extrapolation multiplies the one-thread rate by every hardware "
                "thread of the box -- an upper bound no run here can reach",
    }, vals, rows


def cgroup_cpu_quota():
    """CPUs' worth of time the container may use per period (cgroup v2 cpu.max, v1 cfs_quota/period); None: unlimited."""
    try:
        q, per = open("/sys/fs/cgroup/cpu.max").read().split()[:2]
        return None if q == "max" else float(q) / float(per)
    except Exception:
        pass
    try:
        q = float(open("/sys/fs/cgroup/cpu/cpu.cfs_quota_us").read())
        per = float(open("/sys/fs/cgroup/cpu/cpu.cfs_period_us").read())
        return None if q <= 0 else q / per
    except Exception:
        return None


def time_launches(fn, reps):
    """Per-call durations (ms) from HIP events recorded on the stream the calls are launched on (torch's current one)."""
    for _ in range(2):
        fn()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(reps + 1)]
    ev[0].record()
    for i in range(reps):
        fn()
        ev[i + 1].record()
    torch.cuda.synchronize()
    return [ev[i].elapsed_time(ev[i + 1]) for i in range(reps)]


def traffic_entry(key, pairs):
    """HBM bytes per launch from the PMC pass kept under profiles/ (tools/pmc_*.sh), if it matches this launch size."""
    tpath = os.path.join(ROOT, "profiles", "traffic.json")
    try:
        ent = json.load(open(tpath)).get(key)
        if ent and ent.get("pairs_per_launch") == pairs:
            return ent.get("hbm_bytes_per_launch")
    except Exception:
        pass
    return None


def live_traffic(config, kernel_regex, timeout_s=90):
    """HBM bytes per launch of the dominant kernel measured IN THIS RUN: a child `bench.py --config <c> --no-extras` under
    `rocprofv3 --kernel-trace --pmc TCC_EA0_RDREQ_sum TCC_EA0_RDREQ_128B_sum TCC_EA0_WRREQ_sum TCC_EA0_WRREQ_64B_sum` (a pass of
    its own: counters are never combined with API tracing), corrected as the microarchitecture guide prescribes -- 128-byte read
    requests x 128 B + the others x 64 B; 64-byte write requests x 64 B + the others x 32 B -- averaged over the dispatches that
    match `kernel_regex`.  None when rocprofv3 is missing, fails or times out (the figure of the round's committed pass is used)."""
    import csv
    import glob
    import shutil
    import subprocess
    import tempfile
    if shutil.which("rocprofv3") is None:
        return None
    tmp = tempfile.mkdtemp(prefix="sk_pmc_", dir="/tmp")
    try:
        cmd = ["rocprofv3", "--kernel-trace", "--pmc", "TCC_EA0_RDREQ_sum", "TCC_EA0_RDREQ_128B_sum", "TCC_EA0_WRREQ_sum", "TCC_EA0_WRREQ_64B_sum",
               "--kernel-include-regex", kernel_regex, "-f", "csv", "-d", tmp, "-o", "pmc", "--",
               sys.executable, os.path.abspath(__file__), "--config", config, "--steps", "3", "--warmup", "1", "--no-extras"]
        env = dict(os.environ, TMPDIR="/tmp")
        for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
            env.pop(k, None)
        # (its own process group: on a timeout the profiler AND the python under it are ended -- by the group this call started,
        # never by a pattern)
        proc = subprocess.Popen(cmd, cwd="/tmp", env=env, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, start_new_session=True)
        try:
            if proc.wait(timeout=timeout_s) != 0:
                return None
        except subprocess.TimeoutExpired:
            import signal
            try:
                os.killpg(proc.pid, signal.SIGKILL)
            except OSError:
                pass
            proc.wait()
            return None
        acc = {}
        for path in glob.glob(os.path.join(tmp, "**", "*counter_collection.csv"), recursive=True):
            for r in csv.DictReader(open(path)):
                acc.setdefault(r["Counter_Name"], []).append(float(r["Counter_Value"]))
        if not acc.get("TCC_EA0_RDREQ_sum"):
            return None
        m = {k: sum(v) / len(v) for k, v in acc.items()}
        rd128, rd = m.get("TCC_EA0_RDREQ_128B_sum", 0.0), m.get("TCC_EA0_RDREQ_sum", 0.0)
        wr64, wr = m.get("TCC_EA0_WRREQ_64B_sum", 0.0), m.get("TCC_EA0_WRREQ_sum", 0.0)
        return {"hbm_bytes_per_launch": rd128 * 128 + max(rd - rd128, 0.0) * 64 + wr64 * 64 + max(wr - wr64, 0.0) * 32,
                "dispatches": len(acc["TCC_EA0_RDREQ_sum"])}
    except Exception:      # noqa: BLE001 -- a profiler problem must not cost the bench its line
        return None
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def traffic_source(key):
    """Which PMC pass (file under profiles/, round, counters) the traffic figure comes from."""
    try:
        return json.load(open(os.path.join(ROOT, "profiles", "traffic.json"))).get(key, {}).get("source")
    except Exception:
        return None


def free_port():
    import socket
    with socket.socket() as so:
        so.bind(("127.0.0.1", 0))
        return so.getsockname()[1]


def self_launch(gpus):
    """`python bench.py --gpus N` started without a launcher: re-execute under torch.distributed.run, N ranks on this node,
    rendezvous on 127.0.0.1 and a free port.  The ranks inherit stdout, so rank 0's JSON line is this process's output."""
    import subprocess
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(gpus),
           "--master-addr", "127.0.0.1", "--master-port", str(free_port()), os.path.abspath(__file__)] + sys.argv[1:]
    env = dict(os.environ, SK_BENCH_LAUNCH="self")
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")     # dmabuf IPC: what RCCL needs on these hosts
    env.setdefault("OMP_NUM_THREADS", str(max(1, _cpu_quota_threads() // gpus)))
    return subprocess.call(cmd, env=env)


def launch_check(args, world, rank, local_rank):
    """--launch-check: only the rendezvous (RCCL on GPUs, gloo where there is none): every rank adds rank + 1, rank 0 prints what
    it saw.  What the non-GPU test of the self-launch runs."""
    import torch.distributed as dist
    on_gpu = torch.cuda.is_available()
    if on_gpu:
        torch.cuda.set_device(local_rank)
    dist.init_process_group("nccl" if on_gpu else "gloo", **({"device_id": torch.device("cuda", local_rank)} if on_gpu else {}))
    t = torch.tensor([rank + 1.0], device="cuda" if on_gpu else "cpu")
    dist.all_reduce(t)
    if rank == 0:
        print(json.dumps({"launch_check": True, "n_gpus": args.gpus, "world_size_seen": dist.get_world_size(),
                          "backend": dist.get_backend(), "rank_sum": float(t.item()),
                          "launch": os.environ.get("SK_BENCH_LAUNCH", "torchrun")}))
        sys.stdout.flush()
    dist.barrier()
    dist.destroy_process_group()


class Workload:
    """One BASELINE config on this rank: synthetic paths resident in HBM, the SigKernel that runs it, one `step`."""

    def __init__(self, name, world, scaling, dev, group, cfg=None):
        cfg = cfg or CONFIGS[name]       # (cfg: a reduced shape of the same config -- what the CPU / gloo test of the N > 1 line passes)
        self.name, self.cfg, self.world = name, cfg, world
        A, self.B, self.M, self.N, self.D = cfg["A"], cfg["B"], cfg["M"], cfg["N"], cfg["D"]
        self.kname, self.dyadic, self.dtype, self.mode = cfg["kernel"], cfg["dyadic"], cfg["dtype"], cfg["mode"]
        self.scaling = scaling or ("strong" if self.mode == "mmd" else "weak")
        if self.mode == "mmd" and self.scaling == "weak":
            raise SystemExit("%s is a fixed-size job: use --scaling strong" % name)
        self.A_total = A * world if self.scaling == "weak" else A
        self.sym = bool(cfg.get("sym"))
        # every rank holds the (small) inputs in full, exactly as SigKernel(process_group=...) expects; each solves its own rows
        self.Xc = make_paths(self.A_total, self.M, self.D, seed=1000, dtype=self.dtype)
        self.Yc = self.Xc if self.sym else make_paths(self.B, self.N, self.D, seed=7, dtype=self.dtype)
        if self.sym:
            self.B = self.A_total
        self.X = self.Xc.to(dev)
        self.Y = self.X if self.sym else self.Yc.to(dev)
        self.sk = sigkernel_amd.SigKernel(static_kernel(self.kname), self.dyadic, process_group=group)
        self.sk1 = sigkernel_amd.SigKernel(static_kernel(self.kname), self.dyadic)   # single-GPU instance for the rank-0 extras
        At, B = self.A_total, self.B
        self.entries_per_step = At * B if self.mode == "gram" else (At * At + B * B + At * B)
        self.cells_per_entry = ((self.M - 1) << self.dyadic) * ((self.N - 1) << self.dyadic)

    def step(self):
        if self.mode == "gram":
            return self.sk.compute_Gram(self.X, self.Y, sym=self.sym)   # N > 1: rows sharded, one all-gather (sigkernel_amd.distributed)
        Xg = self.X.detach().requires_grad_(True)
        loss = self.sk.compute_mmd(Xg, self.Y)
        loss.backward()
        return loss.detach(), Xg.grad

    def config(self):
        return {"workload": self.cfg["desc"], "name": self.name,
                "step": "compute_Gram" if self.mode == "gram" else "compute_mmd + backward (entries = the three Gram matrices of one step)",
                "batch_x": self.A_total, "rows_per_gpu": -(-self.A_total // self.world), "batch_y": self.B, "len_x": self.M,
                "len_y": self.N, "dim": self.D, "static_kernel": self.kname, "dyadic_order": self.dyadic,
                "parallelism": "SigKernel(process_group): gram rows sharded over %d GPU(s), 1 all-gather per Gram" % self.world}


def timed(step, steps, warmup, dist, dev):
    """W untimed steps, then exactly K steps between barrier + synchronize on both sides; the MAX over ranks.  (seconds, last output)"""
    def barrier():
        if dist is not None:
            dist.barrier()
        if torch.device(dev).type == "cuda":
            torch.cuda.synchronize()

    out = None
    for _ in range(warmup):
        out = step()
    barrier()
    t0 = time.perf_counter()
    for _ in range(steps):
        out = step()
    barrier()
    elapsed = time.perf_counter() - t0
    if dist is not None:
        t = torch.tensor([elapsed], dtype=torch.float64, device=dev)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())
    return elapsed, out


DUMP_BUDGET_BYTES = 64 << 20


def dump_outputs(outdir, wl, out):
    """--dump-outputs DIR: what the timed step returned in its last step, as DIR/<name>.npy -- float64 for fp64 configs, float32 for
    fp32 I/O: gram configs `gram` (the full matrix, A x B); mmd configs `mmd` (the scalar) and `grad` (d mmd / d X, A x M x D).  The
    inputs are seeded, so two builds run with the same arguments compare output for output.  An array beyond its share of the 64 MB
    budget (none of CONFIGS is, at up to 8 GPUs) is written as a fixed sample: its flat entries at seeded indices, which go to
    DIR/<name>_index.npy."""
    arrays = {"gram": out} if wl.mode == "gram" else {"mmd": out[0], "grad": out[1]}
    os.makedirs(outdir, exist_ok=True)
    share = DUMP_BUDGET_BYTES // len(arrays)
    for name, t in arrays.items():
        a = t.detach().cpu().numpy()
        a = a.astype(np.float64 if a.dtype == np.float64 else np.float32, copy=False)
        if a.nbytes > share:
            idx = np.sort(np.random.default_rng(0).choice(a.size, share // (a.itemsize + 8), replace=False)).astype(np.int64)
            np.save(os.path.join(outdir, name + "_index.npy"), idx)
            a = a.reshape(-1)[idx]
        np.save(os.path.join(outdir, name + ".npy"), a)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=10)     # (the first launches of a process run at lower clocks)
    ap.add_argument("--config", default="c3", choices=sorted(CONFIGS))
    ap.add_argument("--scaling", default=None, choices=["weak", "strong"])
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write the last timed step's outputs as DIR/<name>.npy (rank 0)")
    ap.add_argument("--full", action="store_true",
                    help="after the headline, the legs below: roofline / adjoint / parity / cpu_baseline, the other configs (N = 1); "
                         "the other scaling, collective times and configs[3], [4] under the process group (N > 1)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-extras", action="store_true", help="skip the roofline / adjoint / parity / cpu_baseline legs")
    ap.add_argument("--no-live-traffic", action="store_true", help="roofline.traffic from the round's committed PMC pass instead of a rocprofv3 child run")
    ap.add_argument("--no-configs", action="store_true", help="skip the other BASELINE configs timed after the headline (N = 1)")
    ap.add_argument("--cpu-budget-s", type=float, default=20.0)
    ap.add_argument("--force-dist", action="store_true",
                    help="initialise torch.distributed (RCCL) even with one rank: exercises the N>1 code path on a 1-GPU box")
    ap.add_argument("--launch-check", action="store_true", help="rendezvous only (no kernels): checks the launch path")
    args = ap.parse_args()
    if args.steps < 1 or args.warmup < 0:
        ap.error("--steps must be >= 1 and --warmup >= 0")

    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        raise SystemExit(self_launch(args.gpus))       # plain `python bench.py --gpus N`: spawn the N ranks ourselves
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:
        raise SystemExit("--gpus %d does not match WORLD_SIZE %d" % (args.gpus, world))
    if args.launch_check:
        if "MASTER_ADDR" not in os.environ:
            os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(free_port()), RANK="0", WORLD_SIZE="1")
        return launch_check(args, world, rank, local_rank)
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs an MI355X (no CPU fallback)")
    if local_rank >= torch.cuda.device_count():
        raise SystemExit("rank %d: LOCAL_RANK %d but only %d GPU(s) visible" % (rank, local_rank, torch.cuda.device_count()))
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    dist = None
    use_dist = world > 1 or args.force_dist
    if use_dist:
        import torch.distributed as dist
        if "MASTER_ADDR" not in os.environ:              # --force-dist without a launcher
            os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(free_port()), RANK="0", WORLD_SIZE="1")
        dist.init_process_group("nccl", device_id=dev)   # "nccl" is RCCL on ROCm
    group = dist.group.WORLD if use_dist else None

    wl = Workload(args.config, world, args.scaling, dev, group)
    be = _lib.get_backend()
    assert isinstance(be, _lib.HipBackend), "bench must run on the HIP back-end"

    elapsed, out = timed(wl.step, args.steps, args.warmup, dist, dev)
    if rank == 0 and args.dump_outputs:
        dump_outputs(args.dump_outputs, wl, out)
    value = wl.entries_per_step * args.steps / elapsed
    dname = "f64" if wl.dtype == torch.float64 else "f32"

    result = {
        "metric": "Gram entries/sec (%s)" % ("fp64" if wl.dtype == torch.float64 else "fp32 I/O, fp64 PDE state"),
        "value": value,
        "unit": "entries/s",
        "n_gpus": world,
        "steps": args.steps,
        "warmup": args.warmup,
        "ms_per_step": 1e3 * elapsed / args.steps,
        "higher_is_better": True,
        "scaling": wl.scaling,
        "vs_baseline": None,
        "dtype": dname,
        "data": "synthetic",
        "config": wl.config(),
        "grid_cells_per_s": value * wl.cells_per_entry,
        "launch": os.environ.get("SK_BENCH_LAUNCH", "torchrun" if "TORCHELASTIC_RUN_ID" in os.environ else "single process"),
        "world_size_seen": dist.get_world_size() if use_dist else 1,
    }

    if args.full and use_dist and wl.mode == "gram" and args.scaling is None:
        # the other scaling of the same config in the same line: BASELINE's ">= 6x at 8 GPUs" reads on the FIXED batch (strong:
        # the batch divided over the ranks); `value` above is the weak figure (the batch per GPU fixed).  At N = 1 they coincide.
        other = Workload(args.config, world, "strong" if wl.scaling == "weak" else "weak", dev, group)
        el2, _ = timed(other.step, args.steps, args.warmup, dist, dev)
        result[other.scaling + "_scaling"] = {
            "value": other.entries_per_step * args.steps / el2, "unit": "entries/s", "ms_per_step": 1e3 * el2 / args.steps,
            "batch_x": other.A_total, "rows_per_gpu": -(-other.A_total // world), "batch_y": other.B,
            "collectives": collectives_per_step(other.step, min(args.steps, 5), dist, dev),
            "note": "same config, same steps / warmup / barriers, timed right after the headline region"}
        del other
    if args.full and use_dist:
        # per-step time inside RCCL (all ranks take part; after the timed regions): what a shortfall of the scaling curve is made of
        result["collectives"] = collectives_per_step(wl.step, min(args.steps, 5), dist, dev)

    t_ex = time.perf_counter()
    if args.full and rank == 0 and not args.no_extras:
        extras(result, args, wl.cfg, wl.sk1, be, wl.X, wl.Y, wl.Xc, wl.Yc, out, wl.A_total, world, value)
    t_cf = time.perf_counter()
    if args.full and rank == 0 and not use_dist and not args.no_extras and not args.no_configs and args.config == "c3":
        del out
        result["configs"] = other_configs(dev, args)
    if args.full and use_dist and not args.no_configs and args.config == "c3":
        # N > 1 (or --force-dist): the configs BASELINE names for several GPUs -- configs[3] above all -- strong-scaled under the
        # same process group, every rank taking part, rank 0 checking its output against the oracle
        out = None
        result["configs"] = dist_configs(world, rank, dev, group, dist)
    if rank == 0:
        result["wall_s"] = {"timed_region": elapsed, "extras": t_cf - t_ex, "configs": time.perf_counter() - t_cf}
    if rank == 0:
        print(json.dumps(result))
        sys.stdout.flush()

    if use_dist:
        dist.barrier()
        dist.destroy_process_group()


def mmd_parity(wl, loss, grad, rows):
    """The timed compute_mmd(X, Y).backward() against the oracle: gradient rows `rows` in full (every pair of K_XX and K_XY that
    row takes part in, with the reference's 2x rule on K_XX, sigkernel.py:190-197, :410-412) and, for small batches, the scalar."""
    from oracle import oracle as O
    skern = static_kernel(wl.kname)
    A, B = wl.A_total, wl.B
    nt = usable_threads()
    Xr = wl.Xc[rows]
    wxx = np.full((len(rows), A), 1.0 / (A * (A - 1.0)))
    wxx[np.arange(len(rows)), rows] = 0.0
    wxy = np.full((len(rows), B), -2.0 / (A * B))
    want = 2.0 * O.gram_grad_weighted(Xr, wl.Xc, wxx, skern, wl.dyadic, nthreads=nt) + \
        O.gram_grad_weighted(Xr, wl.Yc, wxy, skern, wl.dyadic, nthreads=nt)
    got = grad[rows].double().cpu().numpy()
    gerr = float(np.max(np.abs(got - want)) / np.max(np.abs(want)))
    par = {"grad_rows_checked": [int(r) for r in rows], "grad_max_rel_err_vs_oracle": gerr, "grad_tolerance": 1e-6,
           "grad_ok": bool(gerr <= 1e-6), "mmd": float(loss)}
    if A * A + B * B + A * B <= 3 * 128 * 128:
        Kxx, Kyy = O.gram_forward(wl.Xc, wl.Xc, skern, wl.dyadic, nthreads=nt), O.gram_forward(wl.Yc, wl.Yc, skern, wl.dyadic, nthreads=nt)
        Kxy = O.gram_forward(wl.Xc, wl.Yc, skern, wl.dyadic, nthreads=nt)
        ref = (Kxx.sum() - np.trace(Kxx)) / (A * (A - 1.0)) + (Kyy.sum() - np.trace(Kyy)) / (B * (B - 1.0)) - 2.0 * Kxy.mean()
        # the MMD is a difference of O(1) means: judged against the means it is formed from
        par.update(mmd_oracle=float(ref), mmd_abs_err=abs(float(loss) - float(ref)), mmd_tolerance=1e-6 * float(abs(Kxy.mean())),
                   mmd_ok=bool(abs(float(loss) - float(ref)) <= 1e-6 * abs(Kxy.mean())))
    return par


def gram_parity(wl, K, n_chk):
    """n_chk random entries of the timed Gram matrix re-solved by the oracle."""
    from oracle import oracle as O
    skern = static_kernel(wl.kname)
    Kc = K.double().cpu().numpy()
    rng = np.random.default_rng(0)
    worst = 0.0
    for p in rng.integers(0, wl.A_total * wl.B, size=n_chk):
        a, b = divmod(int(p), wl.B)
        want = O.gram_forward(wl.Xc[a:a + 1], wl.Yc[b:b + 1], skern, wl.dyadic)[0, 0]
        worst = max(worst, abs(float(Kc[a, b]) - want) / abs(want))
    tol = 1e-6 if wl.dtype == torch.float64 else 1e-4       # fp32 I/O: the reference's own fp32 bar (test_mps.py:32)
    par = {"pairs_checked": int(n_chk), "max_rel_err_vs_oracle": worst, "tolerance": tol, "ok": bool(worst <= tol)}
    if wl.sym:
        par["exactly_symmetric"] = bool(np.array_equal(Kc, Kc.T))
    return par


def graph_replay_ms(wl, steps):
    """A training-sized step is launch-bound (dozens of small launches): the same compute_mmd(X, Y).backward() captured ONCE into a
    hipGraph (torch.cuda.CUDAGraph: the path has no synchronisation, no host read-back and no allocation outside torch's caching
    allocator) and replayed -- what a training loop with static shapes should do.  (ms per replay, gradient bit-identical to eager?)"""
    sX = wl.X.detach().clone().requires_grad_(True)

    def step():
        loss = wl.sk.compute_mmd(sX, wl.Y)
        loss.backward()
        return loss.detach()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):            # warm-up on a side stream, as torch's capture protocol asks
        for _ in range(3):
            step()
            sX.grad = None
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step()
    for _ in range(3):
        graph.replay()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        graph.replay()
    torch.cuda.synchronize()
    ms = 1e3 * (time.perf_counter() - t0) / steps
    Xe = wl.X.detach().clone().requires_grad_(True)
    wl.sk.compute_mmd(Xe, wl.Y).backward()
    return ms, bool(torch.equal(sX.grad, Xe.grad))


def other_configs(dev, args):
    """The other BASELINE configs (and two training-sized MMD steps) on this GPU, after the headline's timed region: 1 warm-up
    + 2 timed steps each between synchronisations, with a parity block per config -- so that the driver's default run carries a
    number for every config, not only the headline."""
    res = {}
    # (mmd32 / mmd64: 5 + 30 steps of ~0.4 ms -- after two warm-ups the allocator and the clocks are not settled: 0.44 instead of 0.31 ms)
    # (c4: two warm-up steps -- after one, the caching allocator may still be growing its pool of 17 GB edge blocks inside the timed
    # steps: 550 instead of 345 ms per step, one run in three)
    for name, steps, warmup in (("c2", 20, 3), ("mmd32", 30, 5), ("mmd64", 30, 5), ("c5", 2, 1), ("c4", 3, 2)):
        t_cfg = time.perf_counter()
        try:
            wl = Workload(name, 1, None, dev, None)
            elapsed, out = timed(wl.step, steps, warmup, None, dev)
            ent = {"workload": wl.cfg["desc"], "steps": steps, "warmup": warmup, "ms_per_step": 1e3 * elapsed / steps,
                   "value": wl.entries_per_step * steps / elapsed, "unit": "entries/s", "dtype": "f64" if wl.dtype == torch.float64 else "f32",
                   "grid_cells_per_s": wl.entries_per_step * steps / elapsed * wl.cells_per_entry}
            if wl.mode == "gram":
                ent["parity"] = gram_parity(wl, out, 64 if wl.cells_per_entry < 1e6 else 8)
            else:
                rows = np.array([0, wl.A_total - 1]) if wl.A_total > 128 else np.arange(wl.A_total)
                ent["parity"] = mmd_parity(wl, out[0], out[1], rows)
                if wl.A_total <= 128:      # launch-bound sizes: the same step replayed from a hipGraph
                    gms, same = graph_replay_ms(wl, 50)
                    ent["hip_graph"] = {"ms_per_step": gms, "value": wl.entries_per_step / (gms * 1e-3), "gradient_bit_identical_to_eager": same}
            res[name] = ent
            del out
            try:
                blocks = config_roofline(wl, ent["ms_per_step"])
                if blocks:
                    ent.update(blocks)
            except Exception as e:      # noqa: BLE001 -- the ceiling is an extra: its failure must not cost the config its number
                ent["roofline_error"] = "%s: %s" % (type(e).__name__, e)
            del wl
            torch.cuda.empty_cache()
            torch.cuda.synchronize()
            ent["wall_s"] = time.perf_counter() - t_cfg
        except Exception as e:      # noqa: BLE001 -- a failing secondary config must not cost the headline its line
            res[name] = {"error": "%s: %s" % (type(e).__name__, e)}
    return res


def config_roofline(wl, step_ms):
    """A `roofline` block for one of the secondary configs, by the headline's method: the algorithmic fp64 lane operations of the
    config's DOMINANT solver launch (x 2 flop) over that launch's duration, measured by HIP events on the launch stream around the
    host call that issues it (the staging launch of a few microseconds and -- for the adjoints -- the screen / rescue / fold launches
    are inside the bracket), against the fp64 vector peak; `step_frac`: the same for ALL solver launches of a step over the timed
    step.  Every config here runs fused kernels that never read the increment matrix: the binding ceiling is fp64 issue, not HBM."""
    from sigkernel_amd.sigkernel import _fused_forward
    be = _lib.get_backend()
    A, B, Mc, Nc, D, d, kn = wl.A_total, wl.B, wl.M - 1, wl.N - 1, wl.D, wl.dyadic, wl.kname
    sk = wl.sk1
    f_ops, a_ops = fwd_ops_per_pair(kn, D, Mc, Nc, d), adj_ops_per_pair(kn, D, Mc, Nc, d)
    blocks = {}

    def block(kernel, pairs, ops_per_pair, ms):
        avg = float(np.mean(ms))
        tf = 2.0 * pairs * ops_per_pair / (avg * 1e-3) / 1e12
        return {"bound": "fp64_valu", "achieved": tf, "peak": FP64_VECTOR_PEAK_TF, "unit": "TFLOP/s", "frac": tf / FP64_VECTOR_PEAK_TF,
                "kernel": kernel, "pairs_per_launch": int(pairs), "fp64_lane_ops_per_launch": int(pairs * ops_per_pair),
                "avg_launch_ms": avg, "min_launch_ms": float(np.min(ms)), "traffic": None}

    if wl.mode == "gram":
        if wl.sym:
            pairs, fn = A * (A + 1) // 2, (lambda: sk.compute_Gram(wl.X, wl.X, sym=True))
            kernel = "sk_solve_fwd_%s_sym_f64 (k_fwd_fused: the pairs on and above the diagonal, one launch)" % kn
        else:
            pairs, fn = A * B, (lambda: _fused_forward(be, sk.static_kernel, wl.X, wl.Y, d, False, gram=True))
            kernel = "sk_solve_fwd_static_* (k_fwd_fused_mb: several bands per pair)" if Mc > 128 else "sk_solve_fwd_%s_* (k_fwd_fused)" % kn
        if fn() is None:
            return None
        blocks["roofline"] = block(kernel, pairs, f_ops, time_launches(fn, 5))
        step_ops = pairs * f_ops
    elif A + B <= 256:
        # training-sized step (the one-launch loss route): K(X, [X; Y]) + the strict triangle of K(Y, Y) in ONE forward launch, the
        # rectangle's adjoint in one
        kind, param = (0, 1.0) if kn == "linear" else (1, 1.0)
        p_f, p_a = A * (A + B) + B * (B - 1) // 2, A * (A + B)
        Xd, Yd = wl.X.detach(), wl.Y.detach()
        res = be.loss_forward(kind, param, Xd, Yd, d, False, True, True)
        if res is None:
            return None
        ms_f = time_launches(lambda: be.loss_forward(kind, param, Xd, Yd, d, False, True, True), 10)
        blocks["roofline"] = block("sk_prep_cat_f64 + sk_solve_fwd_loss_f64 (k_fwd_fused, keeps the rectangle's edges) + sk_loss_value_f64",
                                   p_f, f_ops, ms_f)
        _, out, edges, (Zr, Zt, Zr_adj), wb = res
        adj = be.linear_adjoint_fused if kind == 0 else be.rbf_adjoint_fused
        run_a = lambda: adj(Xd, None, param, d, edges, wb, gram=True, kfinal=out[:p_a], naive=False, staged=(Zr_adj, Zt, A + B, wl.M))   # noqa: E731
        if run_a() is not None:
            blocks["roofline_adjoint"] = block("sk_%s_adjoint_fused_f64 (screen + k_adj_fused_* + rescue + fold)" % kn, p_a, a_ops,
                                               time_launches(run_a, 10))
        step_ops = p_f * f_ops + p_a * a_ops
    else:
        # BASELINE configs[3]: the dominant launch is the adjoint of K_XY (all A x B pairs, one launch); the step's solver work is
        # the triangle of K_XX and K_XY forward with edges, the triangle of K_YY, and the two adjoints
        Xd, Yd = wl.X.detach(), wl.Y.detach()
        res = _fused_forward(be, sk.static_kernel, Xd, Yd, d, False, gram=True, keep_edges=True)
        if res is None or res[1] is None:
            return None
        K, edges = res
        gen = torch.Generator().manual_seed(11)
        w = torch.randn(A, B, generator=gen, dtype=torch.float64).to(Xd.device)
        adj = be.linear_adjoint_fused if kn == "linear" else be.rbf_adjoint_fused
        run_a = lambda: adj(Xd, Yd, 1.0, d, edges, w, gram=True, kfinal=K)   # noqa: E731
        if run_a() is None:
            return None
        blocks["roofline"] = block("sk_%s_adjoint_fused_f64 on K_XY (k_adj_fused_*: reverse PDE + K recomputed + chain rule, one launch)" % kn,
                                   A * B, a_ops, time_launches(run_a, 3))
        del K, edges, res, w
        tri_x, tri_y = A * (A + 1) // 2, B * (B + 1) // 2
        step_ops = (tri_x + A * B + tri_y) * f_ops + (A * B + tri_x) * a_ops
    tf_step = 2.0 * step_ops / (step_ms * 1e-3) / 1e12
    blocks["step_frac"] = {"fp64_lane_ops_per_step": int(step_ops), "achieved": tf_step, "peak": FP64_VECTOR_PEAK_TF, "unit": "TFLOP/s",
                           "frac": tf_step / FP64_VECTOR_PEAK_TF,
                           "note": "every solver launch of one timed step (glue launches and host time included in the time, not in the operations)"}
    return blocks


def collectives_per_step(step, steps, dist, dev):
    """What a step spends in this package's collectives: `steps` extra steps AFTER the timed region with every all-gather / all-reduce
    bracketed by events (sigkernel_amd.distributed.record_collectives) -- per step: calls, milliseconds, bytes received."""
    from sigkernel_amd import distributed as skd
    skd.record_collectives(True)
    try:
        for _ in range(steps):
            step()
        summ = skd.collective_summary()
    finally:
        skd.record_collectives(False)
    if dist is not None:
        dist.barrier()
    res = {k: {"calls_per_step": v["calls"] / steps, "ms_per_step": v["ms"] / steps, "bytes_per_step": v["bytes"] / steps} for k, v in summ.items()}
    return {"all_gather_ms": res.get("all_gather", {}).get("ms_per_step", 0.0), "all_reduce_ms": res.get("all_reduce", {}).get("ms_per_step", 0.0),
            "detail": res, "steps": steps,
            "note": "HIP events on the caller's stream around each collective of sigkernel_amd.distributed, %d steps after the timed region "
                    "(rank 0's view: it includes the wait for the slowest rank to arrive)" % steps}


DIST_CONFIGS = (("c4", 3, 2), ("c5", 2, 1))     # (name, timed steps, warm-ups) of the N > 1 line


def dist_configs(world, rank, dev, group, dist, plan=DIST_CONFIGS, shapes=None):
    """The N > 1 line's `configs`: BASELINE configs[3] (compute_mmd(X, Y).backward() on 2048 + 2048 paths -- the config BASELINE.json
    names for 8 GPUs) and configs[4], STRONG-scaled under SigKernel(process_group): the fixed batch's rows divided over the ranks
    (sigkernel_amd.distributed).  Collective: called by every rank; timing as the headline's (barrier + synchronize on both sides, MAX
    over ranks); rank 0 adds the parity block -- gradient rows / Gram entries of the timed output against the oracle -- while the
    others wait at the next barrier.  shapes: {name: reduced config} (the gloo / CPU test)."""
    res = {}
    for name, steps, warmup in plan:
        t_cfg = time.perf_counter()
        ent = None
        try:
            wl = Workload(name, world, "strong", dev, group, cfg=(shapes or {}).get(name))
            elapsed, out = timed(wl.step, steps, warmup, dist, dev)
            cfg = wl.config()
            ent = {"workload": wl.cfg["desc"], "steps": steps, "warmup": warmup, "ms_per_step": 1e3 * elapsed / steps,
                   "value": wl.entries_per_step * steps / elapsed, "unit": "entries/s", "scaling": "strong", "n_gpus": world,
                   "world_size_seen": dist.get_world_size(group), "backend": dist.get_backend(group),
                   "rows_per_gpu": cfg["rows_per_gpu"], "parallelism": cfg["parallelism"],
                   "dtype": "f64" if wl.dtype == torch.float64 else "f32",
                   "grid_cells_per_s": wl.entries_per_step * steps / elapsed * wl.cells_per_entry}
            ent["collectives"] = collectives_per_step(wl.step, 2, dist, dev)      # (every rank takes part; after the timed region)
            if rank == 0:
                if wl.mode == "gram":
                    ent["parity"] = gram_parity(wl, out, 64 if wl.cells_per_entry < 1e6 else 8)
                else:
                    rows = np.array([0, wl.A_total - 1]) if wl.A_total > 128 else np.arange(wl.A_total)
                    ent["parity"] = mmd_parity(wl, out[0], out[1], rows)
            del wl, out
            if torch.device(dev).type == "cuda":
                torch.cuda.empty_cache()
            ent["wall_s"] = time.perf_counter() - t_cfg
        except Exception as e:      # noqa: BLE001 -- a failing secondary config must not cost the headline its line
            ent = {"error": "%s: %s" % (type(e).__name__, e)}
        res[name] = ent
    return res


def extras(result, args, cfg, sk, be, X, Y, Xc, Yc, out, A_total, world, value):
    """Rank 0, after the timed region: roofline of the dominant kernel, the adjoint leg, parity against the oracle and the
    CPU baseline."""
    from sigkernel_amd.sigkernel import _fused_forward, _increments
    from oracle import oracle as O
    A, B, M, N, D = cfg["A"], cfg["B"], cfg["M"], cfg["N"], cfg["D"]
    kname, dyadic, dtype, mode = cfg["kernel"], cfg["dyadic"], cfg["dtype"], cfg["mode"]
    sym = bool(cfg.get("sym"))
    s = X.element_size()
    Mc, Nc = M - 1, N - 1
    cells_per_entry = (Mc << dyadic) * (Nc << dyadic)
    alg_per_pair = Mc * Nc * s + s                                   # inc_c read once + 1 value out
    reps = max(3, min(args.steps, 10))
    Xr = X[:A]                                                       # one GPU's rows
    phases, t_ph = {}, [time.perf_counter()]

    def phase(name):
        torch.cuda.synchronize()
        now = time.perf_counter()
        phases[name] = now - t_ph[0]
        t_ph[0] = now
    result["extras_wall_s"] = phases

    # ---- (1) the kernel that dominates the forward step ----------------------------------------------------------------
    fused = _fused_forward(be, sk.static_kernel, Xr, Y, dyadic, False, gram=True) is not None
    if fused:
        run_fused = (lambda: sk.compute_Gram(Xr, Xr, sym=True)) if sym else \
            (lambda: _fused_forward(be, sk.static_kernel, Xr, Y, dyadic, False, gram=True))
        # Linear / RBF within the fused kernels' scope: one launch does static kernel + increments + PDE for the whole Gram;
        # nothing of size pairs x M x N touches HBM, so the ceiling is fp64 vector issue.  FMA-class lane operations per pair:
        # 3 per fine cell (stencil) + per coarse cell 3 (linear) / 4 (rbf) coefficient operations + the static kernel (linear:
        # D FMAs; rbf: 2 D for the distance, 19 for exp, 4 for the 4-corner difference).
        ms = time_launches(run_fused, reps)
        avg = float(np.mean(ms))
        pairs_f = A * (A + 1) // 2 if sym else A * B        # sym: the pairs on and above the diagonal, one launch
        # (linear, round 3: three coefficient operations per coarse cell on the pre-scaled increment, sk_linear_prescale)
        per_coarse = (3 + D) if kname == "linear" else (4 + 2 * D + 23)
        ops = pairs_f * (cells_per_entry * 3 + Mc * Nc * per_coarse)
        tflops = 2 * ops / (avg * 1e-3) / 1e12
        kern = "sk_solve_fwd_%s_%s (k_fwd_fused: static kernel + increments + PDE in one launch)" % (kname, "f64" if s == 8 else "f32")
        # (one rank only: with more, the other ranks sit in a collective's barrier while rank 0 profiles -- the committed pass serves)
        live = None if (args.no_live_traffic or sym or world > 1) else live_traffic(args.config, "k_fwd_fused")
        result["roofline"] = {
            "bound": "fp64_valu", "achieved": tflops, "peak": FP64_VECTOR_PEAK_TF, "unit": "TFLOP/s", "frac": tflops / FP64_VECTOR_PEAK_TF,
            "peak_source": PEAK_SOURCE,
            "traffic": live["hbm_bytes_per_launch"] if live else traffic_entry(args.config + "_fused", pairs_f),
            "traffic_source": ("measured in this run: rocprofv3 --kernel-trace --pmc TCC_EA0_RDREQ_sum TCC_EA0_RDREQ_128B_sum TCC_EA0_WRREQ_sum "
                               "TCC_EA0_WRREQ_64B_sum on a child bench.py --config %s --steps 3 --no-extras, %d dispatches of k_fwd_fused*, "
                               "request counts corrected per the microarchitecture guide" % (args.config, live["dispatches"])) if live
            else traffic_source(args.config + "_fused"),
            "traffic_committed_pass": traffic_entry(args.config + "_fused", pairs_f),
            "kernel": kern, "pairs_per_launch": pairs_f, "fp64_lane_ops_per_launch": ops, "avg_launch_ms": avg,
            "min_launch_ms": float(np.min(ms)),
            "cells_per_s": pairs_f * cells_per_entry / (avg * 1e-3),
            "note": "algorithmic FMA-class operations (stencil 3/cell, coefficients 3 (linear) or 4 (rbf) per coarse cell, static kernel) x 2 flop over the "
                    "launch time, against the fp64 vector peak; the increment matrix is never materialised, HBM traffic is the "
                    "paths (MBs).  tools/ubench/fma_rate measures 63 TFLOP/s of independent v_fma_f64 on this part "
                    "(profiles/r02_fma_rate.txt)",
            "hbm_equivalent_GBs": pairs_f * alg_per_pair / (avg * 1e-3) / 1e9,
            "hbm_equivalent_note": "SURVEY 8(d)'s algorithmic bytes (the increment matrix the streaming solver would read) over this "
                                   "kernel's time -- a rate for comparison with the streaming solver, NOT a fraction of anything: the "
                                   "kernel never reads those bytes (see traffic)",
        }

    phase("roofline_fused_incl_live_traffic")
    # ---- (2) the HBM-streaming solver (what north_star describes; every static kernel outside the fused scope):
    #          increments resident in HBM, solver kernel alone ---------------------------------------------------------
    rows = A
    while rows > 1 and 2 * rows * B * M * N * s > 40e9:
        rows //= 2
    with torch.no_grad():
        inc = _increments(be, sk.static_kernel, Xr[:rows], Y, gram=True)
    launch_ms = time_launches(lambda: be.solve_fwd(inc, dyadic), reps)
    avg_ms = float(np.mean(launch_ms))
    pairs = rows * B
    alg_bytes = pairs * alg_per_pair
    achieved = alg_bytes / (avg_ms * 1e-3) / 1e9
    streaming = {
        "bound": "hbm", "achieved": achieved, "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": achieved / HBM_PEAK_GBS,
        "traffic": traffic_entry(args.config, pairs), "traffic_source": traffic_source(args.config),
        "kernel": "sk_solve_fwd_%s (k_fwd_wave: increments streamed from HBM)" % ("f64" if s == 8 else "f32"),
        "pairs_per_launch": pairs, "algorithmic_bytes_per_launch": alg_bytes, "avg_launch_ms": avg_ms,
        "min_launch_ms": float(np.min(launch_ms)),
        "solver_only_entries_per_s": pairs / (avg_ms * 1e-3),
        "solver_only_cells_per_s": pairs * cells_per_entry / (avg_ms * 1e-3),
    }
    if fused:
        result["roofline_streaming_solver"] = streaming
    else:
        result["roofline"] = streaming
    del inc

    phase("streaming_solver")
    # ---- (3) the adjoint leg: compute_Gram with a gradient pending + backward, HIP events -------------------------------
    ra = A
    while ra > 8 and 4 * ra * B * M * N * 8 > 40e9 and not fused:
        ra //= 2
    gen = torch.Generator().manual_seed(5)
    w = torch.randn(ra, B, generator=gen, dtype=torch.float64)
    w[:, 32:] = 0.0                       # sparse upstream gradient: the oracle re-derives sampled rows from 32 pairs each
    wd = w.to(dtype).to(X.device)
    fwd_ms, bwd_ms = [], []
    grad = None
    for it in range(2 + min(reps, 5)):
        Xg = Xr[:ra].detach().clone().requires_grad_(True)
        e0, e1, e2 = (torch.cuda.Event(enable_timing=True) for _ in range(3))
        e0.record()
        K = sk.compute_Gram(Xg, Y)
        e1.record()
        (K * wd).sum().backward()
        e2.record()
        torch.cuda.synchronize()
        if it >= 2:
            fwd_ms.append(e0.elapsed_time(e1))
            bwd_ms.append(e1.elapsed_time(e2))
        grad = Xg.grad
    adj_bytes = ra * B * (3 * Mc * Nc * s + s)
    tot = (float(np.mean(fwd_ms)) + float(np.mean(bwd_ms))) * 1e-3
    result["adjoint"] = {
        "what": "compute_Gram(X[:%d], Y) with X.requires_grad (forward keeps the terminal edges) + backward of a weighted sum" % ra,
        "pairs": ra * B, "forward_ms": float(np.mean(fwd_ms)), "backward_ms": float(np.mean(bwd_ms)),
        "algorithmic_bytes": adj_bytes, "hbm_equivalent_GBs": adj_bytes / tot / 1e9, "hbm_equivalent_frac": adj_bytes / tot / 1e9 / HBM_PEAK_GBS,
        "entries_per_s_fwd_bwd": ra * B / tot,
        "note": "3 (M-1)(N-1) s + s bytes per entry (SURVEY 8(d)); LinearKernel / RBFKernel backward passes that fuse the "
                "static kernel move far fewer bytes -- this is the rate-equivalent the survey prescribes",
    }

    phase("adjoint")
    # ---- (4) parity of the timed output and of the gradient -----------------------------------------------------------
    skern = static_kernel(kname)
    rng = np.random.default_rng(0)
    if mode == "gram":
        Kc = out[:A].double().cpu().numpy()
    else:
        with torch.no_grad():
            Kc = sk.compute_Gram(Xr, Y).double().cpu().numpy()
    n_chk = 64 if cells_per_entry < 1e6 else 8
    idx = rng.integers(0, A * B, size=n_chk)
    worst = 0.0
    for p in idx:
        a, b = divmod(int(p), B)
        want = O.gram_forward(Xc[a:a + 1], Yc[b:b + 1], skern, dyadic)[0, 0]
        worst = max(worst, abs(float(Kc[a, b]) - want) / abs(want))
    tol = 1e-6 if dtype == torch.float64 else 1e-4       # fp32 I/O: the reference's own fp32 bar (test_mps.py:32)
    gworst, grows = 0.0, []
    if cells_per_entry < 1e6:
        for a in (0, ra - 1):
            gp = O.gram_grad_points(Xc[a:a + 1], Yc[:32], skern, dyadic, nthreads=usable_threads())   # (1,32,M,D)
            want = np.einsum("b,bmd->md", w[a, :32].numpy(), gp[0])
            got = grad[a].double().cpu().numpy()
            gworst = max(gworst, float(np.max(np.abs(got - want)) / np.max(np.abs(want))))
            grows.append(a)
    result["parity"] = {"pairs_checked": int(n_chk), "max_rel_err_vs_oracle": worst, "tolerance": tol, "ok": bool(worst <= tol),
                        "grad_rows_checked": grows, "grad_max_rel_err_vs_oracle": gworst if grows else None,
                        "grad_tolerance": 1e-6 if dtype == torch.float64 else 1e-4,
                        "grad_ok": bool(gworst <= (1e-6 if dtype == torch.float64 else 1e-4)) if grows else None}
    if mode == "mmd":
        result["parity"]["mmd"] = float(out[0])

    phase("parity_vs_oracle")
    # ---- (5) CPU baseline -----------------------------------------------------------------------------------------------
    if world == 1 and not args.no_cpu_baseline:
        cb, vals, nrows = cpu_baseline(Xc[:A], Yc, kname, dyadic, args.cpu_budget_s)
        # SURVEY 8(d)'s parity gate: max |K - K_ref| / max |K_ref| over the WHOLE sample (every entry the CPU port solved); the
        # entry-wise relative error is reported beside it -- it is dominated by the few entries near zero
        cb["max_norm_err_gpu_vs_cpu_sample"] = float(np.max(np.abs(Kc[:nrows] - vals)) / np.max(np.abs(vals)))
        cb["max_entrywise_rel_err_gpu_vs_cpu_sample"] = float(np.max(np.abs(Kc[:nrows] - vals) / np.abs(vals)))
        result["cpu_baseline"] = cb
        if mode == "gram":
            result["speedup_vs_cpu_baseline"] = value / cb["value"]
            result["speedup_vs_cpu_single_thread"] = value / cb["single_thread_value"]
        phase("cpu_baseline")


if __name__ == "__main__":
    main()
