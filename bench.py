#!/usr/bin/env python3
"""bench.py -- simplex iterations/s + time-to-optimal on the dense LP of BASELINE.json.

Workload (BASELINE.json configs[2], the config its metric is quoted on):
maximize c'x s.t. A x <= b, x >= 0, A dense 5000 x 50000 fp64 with
A_ij, c_j ~ U[0,1), b_i = n/8 + U n/4, generated into HBM once
by the counter-based generator (data: synthetic; generation is not timed).

A "step" is ONE FULL SOLVE: elp_load_dense_device (canonicalisation, the
row-major copy of A, the Y-row copy, phase decision) + elp_solve to
optimality, from A already resident in HBM -- what easylp$solve() does per
call (R/class.R:260-278).  `value` = simplex iterations of the K timed solves /
their wall time, i.e. the whole-solve iteration rate (A resident in HBM).
`time_to_optimal_s` follows SURVEY.md 8d (H2D included, generation excluded):
the best of three solves from A in host memory through elp_load_dense, the
entry point the R glue calls (`host_input.c3`); the HBM-resident time per
solve is `time_to_optimal_hbm_s`.

    python bench.py [--gpus N] [--steps K] [--warmup W] [--dump-outputs DIR] [--full]

A plain run sets up, runs the W warm-up and the K timed solves, and prints the
result line: the headline figures and what the timed solves' own statistics
give (`final`, `roofline`, `iteration_roofline`).  `time_to_optimal_s` is then
the HBM-resident time per solve (`time_to_optimal_source` says which).
`--dump-outputs DIR` writes what the last timed solve returned to its caller
(status, objective, x, duals, basis) as DIR/<name>.npy, float64; the LP is
seeded, so two builds run with the same arguments solve the same LP.
`--full` adds every other leg, each a run of its own: the steady-state window,
the other pricing rule, the solves from host memory (`host_input`), the
10000x500000 config, configs[1], the sparse and the reference-sized LPs, the
CPU oracle and HiGHS legs and the committed HBM-traffic profile; the per-leg
switches (--c4, --sparse, --window, --no-cpu, ...) select among them there.

Rank 0 prints one JSON line.  With N > 1 the columns are sharded over N
GPUs (strong scaling: `value` is the iteration rate of the one LP).  Default
`--mode ngpu`: ONE process drives the N devices through one handle
(elp_control.ngpu = N) -- what the R `.Call` path runs (R stays one synchronous
process) -- with the per-iteration min-loc through the direct
peer mailbox; A is generated on every device (untimed) and each rank reads its
own copy (elp_load_dense_device_multi).  When the driver starts N processes
under torchrun, rank 0 runs that one-process solve over all N devices and the
other ranks only take part in the barriers around the timed region (they
process no columns).  `--mode procs` keeps one process per GPU (elp_comm_init,
RCCL all-gather or, with --p2p 1, the IPC mailbox).
"""
from __future__ import annotations

import argparse
import json
import os
import platform
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

METRIC = "simplex iterations/sec + time-to-optimal, dense LP m=5k n=50k at 1/2/4/8 GPUs"
HBM_PEAK_GBS = 8000.0  # MI355X_MICROARCH.md: HBM3E 8.0 TB/s spec


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=10, help="timed full solves")
    ap.add_argument("--warmup", type=int, default=2, help="untimed full solves")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write what the last timed solve returned (status, objective, x, y, basis) as DIR/<name>.npy")
    ap.add_argument("--full", action="store_true",
                    help="also run the secondary legs (window, other pricing rule, host input, C4, C2, sparse, "
                         "small LPs, CPU baselines); the per-leg switches below select among them")
    ap.add_argument("--m", type=int, default=5000)
    ap.add_argument("--n", type=int, default=50000)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--cpu-iters", type=int, default=0,
                    help="cap on the CPU oracle's iterations (0: one full solve, ~20 s)")
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--highs", type=int, default=1,
                    help="N=1: SciPy HiGHS (highs-ds) CPU leg in a child process (cpu_baseline_highs)")
    ap.add_argument("--profile-price", type=int, default=1,
                    help="HIP events on the pricing dispatches of every 8th chunk (roofline)")
    ap.add_argument("--c4", type=int, default=1,
                    help="also solve the 10000x500000 column-sharded config (SURVEY config 4) to optimality")
    ap.add_argument("--mode", choices=["ngpu", "procs"], default="ngpu",
                    help="N>1: one process driving N devices (ngpu, the R path) or one process per GPU")
    ap.add_argument("--p2p", type=int, default=0,
                    help="--mode procs, N>1: per-iteration min-loc through the IPC mailbox (default: RCCL all-gather)")
    ap.add_argument("--exchange", type=int, default=0,
                    help="--mode ngpu: elp_control.exchange (0 peer mailbox when it probes, 1 collective)")
    ap.add_argument("--host-input", type=int, default=1,
                    help="also time the solve from A in host memory (elp_load_dense, what .Call pays)")
    ap.add_argument("--host-c4", type=int, default=1,
                    help="with --host-input: also the 10000x500000 LP from a 40 GB host array (N=1)")
    ap.add_argument("--force-sharded", action="store_true",
                    help="N=1: run the sharded pipeline on a 1-rank RCCL communicator (overhead probe)")
    ap.add_argument("--sparse", type=int, default=1,
                    help="also time the CSC path on a sparse LP (BASELINE config 5)")
    ap.add_argument("--small", type=int, default=1,
                    help="the reference-sized LPs / MIPs: resident solver, pipeline and CPU oracle times")
    ap.add_argument("--c2", type=int, default=1,
                    help="N=1: also BASELINE configs[1] (500 x 2000) to optimality from host memory")
    ap.add_argument("--sparse-m", type=int, default=1000)
    ap.add_argument("--sparse-n", type=int, default=10000)
    ap.add_argument("--sparse-steps", type=int, default=1000)
    ap.add_argument("--sparse-cpu-iters", type=int, default=200)
    ap.add_argument("--pricing", choices=["devex", "dantzig"], default="devex",
                    help="pricing rule (elp_control.pricing; devex is lp_solve's default)")
    ap.add_argument("--sync-every", type=int, default=32,
                    help="iterations enqueued between host polls (elp_control.sync_every)")
    ap.add_argument("--compare-rules", type=int, default=1,
                    help="N=1: also solve the LP to optimality with the other pricing rule")
    ap.add_argument("--window", type=int, default=1,
                    help="also report the steady-state rate over iterations [100, 1100) of one solve")
    a = ap.parse_args()
    a.rule = 1 if a.pricing == "devex" else 0
    if not a.full:  # a plain run: the timed solves and nothing beside them
        a.window = a.compare_rules = a.host_input = a.host_c4 = a.c4 = a.sparse = a.small = a.c2 = a.highs = 0
        a.no_cpu = True
    return a


def dump_outputs(path, sol):
    """--dump-outputs: what the last timed solve handed back (Problem.solution:
    elp_get_solution after elp_solve), one float64 array per file."""
    import numpy as np
    os.makedirs(path, exist_ok=True)
    if sol is None:  # (--steps 0: nothing was computed)
        return
    arrays = {"status": [sol.status], "objective": [sol.objval], "x": sol.x, "y": sol.y, "basis": sol.basis}
    for name, v in arrays.items():
        np.save(os.path.join(path, name + ".npy"), np.asarray(v, dtype=np.float64))


def relaunch_under_torchrun(args) -> int:
    """--gpus N > 1 without a launcher: start torchrun as a child before any GPU
    call (never exec from this process) and return its exit code."""
    import socket
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={args.gpus}",
           "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    return subprocess.call(cmd)


def host_info():
    model = platform.processor() or ""
    try:
        with open("/proc/cpuinfo") as f:
            for line in f:
                if line.startswith("model name"):
                    model = line.split(":", 1)[1].strip()
                    break
    except OSError:
        pass
    return model, os.cpu_count()


def enable_p2p(p, rank):
    """xGMI mailbox for the min-loc; collective and agreed by all ranks, so on
    failure every rank falls back to the RCCL all-gather together."""
    from easylp_amd._lib import ElpError
    try:
        p.comm_enable_p2p()
        return True
    except ElpError as e:
        if rank == 0:
            print(f"xGMI mailbox unavailable ({e}); RCCL all-gather min-loc", file=sys.stderr)
        return False


def ngpu_probe(args, local):
    """Torchrun-launched N > 1 in the default ngpu mode: before anything is
    timed, rank 0 checks that one handle can drive the N devices (RCCL
    communicator, peer mailbox probe, a small LP solved to optimality).  On
    failure every rank falls back to --mode procs (one process per GPU), so a
    node where the single-process path cannot run still yields a line."""
    import numpy as np
    from easylp_amd import Problem
    from easylp_amd._lib import ELP_OPTIMAL
    rng = np.random.default_rng(7)
    m, n = 64, 64 * args.gpus * 4
    A = np.asfortranarray(rng.random((m, n)))
    b = n / 8 + rng.random(m) * n / 4
    c = rng.random(n)
    try:
        if os.environ.get("ELP_BENCH_FAIL_NGPU"):  # (rehearses the fallback on a one-GPU box)
            raise RuntimeError("ELP_BENCH_FAIL_NGPU set")
        with Problem(m, n, device=local, ngpu=args.gpus, exchange=args.exchange) as p:
            p.load_dense(A, np.ones(m, np.int32), b, c, maximize=True)
            ok = p.solve() == ELP_OPTIMAL
            if not ok:
                print("ngpu probe: the probe LP did not solve to optimality", file=sys.stderr)
            return ok
    except Exception as e:  # (any failure: fall back, report it)
        print(f"ngpu probe failed ({e}); falling back to --mode procs", file=sys.stderr)
        return False


class Ctx:
    """Where the bench runs.  procs: `world` processes, one GPU each (ngpu 1).
    ngpu: one working process (rank 0) whose handle drives `ngpu` devices;
    torchrun's other ranks (if any) only join the barriers."""

    def __init__(self, args, world, rank, local, dist):
        import torch
        self.args, self.world, self.rank, self.local, self.dist = args, world, rank, local, dist
        self.mode = args.mode if args.gpus > 1 else "single"
        self.ngpu = args.gpus if self.mode == "ngpu" else 1
        ndev = torch.cuda.device_count()
        self.devices = [(local + r) % max(ndev, 1) for r in range(self.ngpu)]
        self.works = self.mode != "ngpu" or rank == 0

    def sync(self):
        import torch
        for dv in self.devices:
            torch.cuda.synchronize(dv)

    def barrier(self):
        self.sync()
        if self.world > 1:
            self.dist.barrier()

    def max_over_ranks(self, v):
        if self.world == 1:
            return v
        import torch
        t = torch.tensor([v], dtype=torch.float64)
        self.dist.all_reduce(t, op=self.dist.ReduceOp.MAX)
        return float(t.item())

    def parallelism(self, p2p, stats):
        if self.mode == "single":
            return "force-sharded x1, RCCL" if self.args.force_sharded else "single GPU"
        if self.mode == "procs":
            return "column-shard x%d processes, %s min-loc" % (self.world, "IPC mailbox" if p2p else "RCCL all-gather")
        ex = {1: "peer mailbox", 2: "collective (%s)" % ("RCCL" if len(set(self.devices)) == len(self.devices)
                                                      else "in-process")}.get(stats.get("exchange"), "?")
        return "ngpu x%d (one process), %s" % (self.ngpu, ex)


def make_problem(args, lib, m, n, ctx, **ctl):
    from easylp_amd import Problem
    from easylp_amd._lib import ELP_PROFILE_SAMPLE
    p = Problem(m, n, device=ctx.devices[0], verbose=ELP_PROFILE_SAMPLE if args.profile_price else 0,
                pricing=args.rule, sync_every=args.sync_every, ngpu=ctx.ngpu, exchange=args.exchange, **ctl)
    p2p = False
    if ctx.mode == "procs" or args.force_sharded:
        from easylp_amd.dist import share_unique_id
        p.comm_init(share_unique_id(lib, ctx.rank), ctx.world, ctx.rank)
        if args.p2p:
            p2p = enable_p2p(p, ctx.rank)
    return p, p2p


def place_A(seed, m, n, ctx):
    """The synthetic LP resident in HBM before anything is timed: on every device
    of the handle (each rank reads its own copy)."""
    from easylp_amd import generate_dense_device
    As = []
    for dv in ctx.devices:
        A, b, c = generate_dense_device(seed, m, n, dv)
        As.append(A)
    return As, b, c


def load_resident(p, As, b, c):
    import numpy as np
    dirs = np.ones(len(b), np.int32)
    if len(As) > 1:
        p.load_dense_device_multi([A.data_ptr() for A in As], dirs, b, c, maximize=True)
    else:
        p.load_dense_device(As[0].data_ptr(), dirs, b, c, maximize=True)


def full_solves(p, As, b, c, count, ctx):
    """`count` full solves (load from HBM + solve to optimality); per-solve stats."""
    recs = []
    for _ in range(count):
        t0 = time.perf_counter()
        load_resident(p, As, b, c)
        st = p.solve()
        el = time.perf_counter() - t0
        recs.append((st, el, p.stats()))
    ctx.sync()
    return recs


def price_roofline(stats_list):
    """Pricing-launch roofline over the given solves: algorithmic sweep bytes /
    the launches' time.  The time is the kernel's own clock (every workgroup of
    the sampled launches stamps s_memrealtime at entry and exit, first start ->
    last end: `avg_launch_us`); HIP events bound to the same dispatches
    (`avg_launch_us_events`) read the dispatch gap too and stay beside it."""
    secs_ev = sum(s["price_seconds"] for s in stats_list)
    secs = sum(s.get("price_seconds_stamps", 0.0) for s in stats_list)
    ns = sum(s.get("price_stamped_launches", 0) for s in stats_list)
    byts = sum(s["price_timed_bytes"] for s in stats_list)
    nl = sum(s["price_timed_launches"] for s in stats_list)
    src = "stamps"
    if not (secs > 0 and ns == nl):  # (no stamped launches: the events)
        secs, src = secs_ev, "events"
    ach = byts / secs / 1e9 if secs > 0 else None
    return {"achieved": ach, "peak": HBM_PEAK_GBS, "unit": "GB/s",
            "frac": ach / HBM_PEAK_GBS if ach else None,
            "bytes_per_launch": byts / nl if nl else None,
            "avg_launch_us": 1e6 * secs / nl if nl else None, "launches_timed": nl,
            "avg_launch_us_events": 1e6 * secs_ev / nl if nl else None,
            "frac_events": byts / secs_ev / 1e9 / HBM_PEAK_GBS if secs_ev > 0 else None,
            "launch_timer": src}


def iteration_roofline(stats_list):
    """Whole-iteration roofline (SURVEY.md 8d "report both per phase"): the
    iterations' algorithmic bytes (pricing sweep + select 8k^2 + FTRAN-z 8mk +
    ratio test 8k^2 + 16n + deferred update 32k^2 + 16m, accumulated on the
    device at the k of each iteration) / the simplex-loop wall time."""
    byts = sum(s["iter_bytes"] for s in stats_list)
    secs = sum(s["seconds_loop"] for s in stats_list)
    its = sum(s["iterations"] for s in stats_list)
    ach = byts / secs / 1e9 if secs > 0 else None
    return {"achieved": ach, "peak": HBM_PEAK_GBS, "unit": "GB/s",
            "frac": ach / HBM_PEAK_GBS if ach else None,
            "bytes_per_iteration": byts / its if its else None,
            "timer": "host wall clock of the simplex loops of the timed solves (load excluded)"}


def cpu_baseline(args):
    """The CPU oracle (same algorithm, 1 thread) solving the same LP: one full
    solve by default (about 20 s on one EPYC core), else the first --cpu-iters."""
    import numpy as np
    from oracle import generate_dense, solve_dense
    A, b, c = generate_dense(args.seed, args.m, args.n)
    kw = {"max_iter": args.cpu_iters} if args.cpu_iters > 0 else {}
    r = solve_dense(A, np.ones(args.m, np.int32), b, c, maximize=True, price_rule=args.rule, **kw)
    it, secs = r.stats["iterations"], r.stats["seconds"]
    model, ncpu = host_info()
    full = r.status == 0
    return {
        "value": it / secs if secs > 0 else None,
        "unit": "iterations/s",
        "cores": 1,
        "kind": "port",
        "time_to_optimal_s": secs if full else None,
        "iterations": it,
        "sample": ("oracle/ (C, -O3, 1 thread) %s of the same LP: %d iterations in %.1f s "
                   "(setup included, generation excluded)" % (
                       "one full solve" if full else "the first iterations", it, secs)),
        "host": {"cpu": model, "nproc": ncpu},
    }


def highs_child(argv):
    """`python bench.py --highs-child OUT M N SEED`: the second CPU stand-in of
    SURVEY.md 8d -- SciPy's HiGHS dual simplex (linprog method="highs-ds",
    presolve off), in its own process with OMP_NUM_THREADS=1 -- on the same LPs:
    configs[1] (500 x 2000) to optimality, configs[2] (M x N) over 1 and 201
    iterations (its set-up from the dense matrix alone takes ~30 s and varies by
    ~1 s, so the rate is the 200 iterations between the two runs), and the phase-1
    Netlib-scale sparse LP (kkt_20000x100000) to optimality.  Writes JSON to OUT."""
    import numpy as np
    import scipy
    import scipy.sparse as sp
    from scipy.optimize import linprog
    from oracle import generate_dense
    from easylp_amd.synth import sparse_kkt
    out_path, m3, n3, seed = argv[0], int(argv[1]), int(argv[2]), int(argv[3])
    res = {"solver": "SciPy %s HiGHS dual simplex (linprog highs-ds, presolve off, OMP_NUM_THREADS=1)"
                     % scipy.__version__}

    def run(Acsc, b, c, bounds, cap=None):
        opts = {"presolve": False}
        if cap:
            opts["maxiter"] = cap
        t = time.perf_counter()
        r = linprog(-c, A_ub=Acsc, b_ub=b, bounds=bounds, method="highs-ds", options=opts)
        return r, time.perf_counter() - t

    A, b, c = generate_dense(seed, 500, 2000)
    r, t = run(sp.csc_matrix(A), b, c, (0, None))
    res["c2"] = {"workload": "dense LP m=500 n=2000 seed %d, to optimality" % seed, "status": int(r.status),
                 "iterations": int(r.nit), "time_to_optimal_s": t, "value": r.nit / t, "unit": "iterations/s",
                 "objective": -float(r.fun)}
    fx = {f["name"]: f for f in json.load(open(os.path.join(ROOT, "tests", "golden", "sparse_lu.json")))}
    k = fx["kkt_20000x100000"]
    cp, ri, v, bk, ck, u, obj = sparse_kkt(k["seed"], k["m"], k["n"], k["k"])
    r, t = run(sp.csc_matrix((v, ri, cp), shape=(k["m"], k["n"])), bk, ck, list(zip(np.zeros(k["n"]), u)))
    res["kkt_20000x100000"] = {"workload": "sparse_kkt phase-1 LP m=20000 n=100000, to optimality",
                               "status": int(r.status), "iterations": int(r.nit), "time_to_optimal_s": t,
                               "value": r.nit / t, "unit": "iterations/s", "objective": -float(r.fun)}
    k = fx["kkt_feasible_20000x100000"]
    cp, ri, v, bk, ck, u, obj = sparse_kkt(k["seed"], k["m"], k["n"], k["k"], feasible_start=True)
    r, t = run(sp.csc_matrix((v, ri, cp), shape=(k["m"], k["n"])), bk, ck, list(zip(np.zeros(k["n"]), u)))
    res["kkt_feasible_20000x100000"] = {"workload": "sparse_kkt feasible-start LP m=20000 n=100000, to optimality",
                                        "status": int(r.status), "iterations": int(r.nit), "time_to_optimal_s": t,
                                        "value": r.nit / t, "unit": "iterations/s", "objective": -float(r.fun)}
    with open(out_path, "w") as f:  # (what is there so far, should the long leg be cut)
        json.dump(res, f)
    A, b, c = generate_dense(seed, m3, n3)
    Ac = sp.csc_matrix(A)
    del A
    r1, t1 = run(Ac, b, c, (0, None), cap=1)
    r201, t201 = run(Ac, b, c, (0, None), cap=201)
    it = int(r201.nit) - int(r1.nit)
    res["c3"] = {"workload": "dense LP m=%d n=%d seed %d, capped" % (m3, n3, seed),
                 "seconds_1_iteration": t1, "seconds_201_iterations": t201, "iterations": it,
                 "value": it / (t201 - t1) if t201 > t1 and it > 0 else None, "unit": "iterations/s",
                 "note": "set-up from the dense matrix (~%.0f s) excluded: rate over the iterations between "
                         "the 1- and 201-iteration runs" % t1}
    with open(out_path, "w") as f:
        json.dump(res, f)


class HighsLeg:
    """The HiGHS child, started when the timed region is over (one CPU core, in
    parallel with the remaining GPU legs), collected at the end."""

    def __init__(self, args):
        import tempfile
        self.path = os.path.join(tempfile.mkdtemp(prefix="elp_highs_"), "highs.json")
        env = dict(os.environ, OMP_NUM_THREADS="1", ELP_NO_TORCH="1")
        self.proc = subprocess.Popen([sys.executable, os.path.abspath(__file__), "--highs-child", self.path,
                                      str(args.m), str(args.n), str(args.seed)], env=env,
                                     stdout=subprocess.DEVNULL, stderr=subprocess.PIPE)

    def result(self, timeout):
        try:
            _, err = self.proc.communicate(timeout=timeout)
        except subprocess.TimeoutExpired:
            self.proc.kill()
            self.proc.communicate()
            err = b"timed out"
        try:
            r = json.load(open(self.path))
        except (OSError, ValueError):
            return {"error": (err or b"").decode(errors="replace")[-400:]}
        if self.proc.returncode:
            r["error"] = "incomplete (exit %s): %s" % (self.proc.returncode, (err or b"")[-200:].decode(errors="replace"))
        model, ncpu = host_info()
        r.update({"cores": 1, "kind": "port", "host": {"cpu": model, "nproc": ncpu}})
        return r


def committed_traffic(args):
    """HBM traffic per pricing launch from the committed rocprofv3 --pmc
    FETCH_SIZE pass of this same command (tools/gpu_check.sh ->
    profiles/pmc_traffic.json); used only when that pass ran the same LP,
    steps and warmup."""
    path = os.path.join(ROOT, "profiles", "pmc_traffic.json")
    try:
        t = json.load(open(path))
    except (OSError, ValueError):
        return None, None
    same = (t.get("m"), t.get("n"), t.get("warmup"), t.get("steps"), t.get("step")) == (
        args.m, args.n, args.warmup, args.steps, "full solve")
    if not same:
        return None, None
    return t["traffic_bytes_per_launch"], "profiles/pmc_traffic.json (rocprofv3 --pmc FETCH_SIZE, x2 gfx950)"


def c4_config(args, lib, ctx):
    """BASELINE config 4: dense LP m=10000 n=500000 (40 GB), columns sharded over
    the ranks, solved to optimality from A resident in HBM."""
    import torch
    m, n = 10000, 500000
    As, b, c = place_A(args.seed, m, n, ctx)
    p, _ = make_problem(args, lib, m, n, ctx)
    if ctx.mode == "procs":
        ctx.barrier()
    else:  # (torchrun's idle ranks of the ngpu mode only join the timed region's barriers)
        ctx.sync()
    t0 = time.perf_counter()
    load_resident(p, As, b, c)
    ctx.sync()
    t_load = time.perf_counter() - t0
    st = p.solve()
    ctx.sync()
    el = time.perf_counter() - t0
    s = p.stats()
    obj = p.solution(st).objval
    p.close()
    del As
    torch.cuda.empty_cache()
    if ctx.mode == "procs":
        el, t_load = ctx.max_over_ranks(el), ctx.max_over_ranks(t_load)
    sweep = price_roofline([s])
    sweep["rank"] = ctx.rank
    return {"workload": "dense random LP m=10000 n=500000 (SURVEY config 4), columns sharded x%d" % max(ctx.world, ctx.ngpu),
            "parallelism": ctx.parallelism(False, s),
            "status": st, "objective": obj, "iterations_to_optimal": s["iterations"],
            "time_to_optimal_s": el, "load_s": t_load,
            "value": s["iterations"] / el if el > 0 else None, "unit": "iterations/s (whole solve)",
            "bump_dim": s["bump_dim"], "y_rows": s["y_rows"], "refactors": s["refactors"],
            "gj_refactors": s["gj_refactors"], "max_inv_resid": s["max_inv_resid"],
            "price_sweep": sweep}


def host_input(args, lib, ctx, m, n, label, reps):
    """Time-to-optimal with A in host memory (incl. H2D, excl.
    generation): elp_load_dense from a numpy array -- the entry point the R glue
    calls -- through the pinned staging pipeline, to every device
    of the handle from one pass over host memory."""
    import numpy as np
    import torch
    from easylp_amd import generate_dense_device
    A, b, c = generate_dense_device(args.seed, m, n, ctx.devices[0])
    Ah = A.cpu().numpy().reshape(n, m).T  # column-major (m, n) view: no copy at load
    del A
    torch.cuda.empty_cache()
    p, _ = make_problem(args, lib, m, n, ctx)
    dirs = np.ones(m, np.int32)
    out = []
    for _ in range(reps):
        ctx.sync()
        t0 = time.perf_counter()
        p.load_dense(Ah, dirs, b, c, maximize=True)
        t_load = time.perf_counter() - t0
        st = p.solve()
        el = time.perf_counter() - t0
        s = p.stats()
        out.append({"status": st, "time_to_optimal_s": el, "load_s": t_load, "h2d_s": s["seconds_h2d"],
                    "h2d_GBps": s["h2d_bytes"] / s["seconds_h2d"] / 1e9 if s["seconds_h2d"] > 0 else None,
                    "iterations": s["iterations"]})
    obj = p.solution(out[-1]["status"]).objval
    p.close()
    del Ah
    best = min(out, key=lambda r: r["time_to_optimal_s"])
    return {"workload": "%s from host memory (elp_load_dense, pageable numpy A)" % label,
            "parallelism": ctx.parallelism(False, {"exchange": 0}) if ctx.ngpu == 1 else "ngpu x%d" % ctx.ngpu,
            "h2d_bytes": 8.0 * m * n, "objective": obj, "runs": out, "best": best}


def c2_config(args, local, reps=5):
    """BASELINE configs[1]: the dense 500 x 2000 LP (seed args.seed, the LP the
    HiGHS leg times as cpu_baseline_highs.c2) to optimality from host memory
    (elp_load_dense + elp_solve, what one easylp$solve() call pays): the best of
    `reps` solves after one untimed warm-up."""
    import numpy as np
    import torch
    from easylp_amd import Problem, generate_dense_device
    m, n = 500, 2000
    A, b, c = generate_dense_device(args.seed, m, n, local)
    Ah = A.cpu().numpy().reshape(n, m).T  # column-major (m, n) view
    del A
    torch.cuda.empty_cache()
    dirs = np.ones(m, np.int32)
    runs = []
    with Problem(m, n, device=local, pricing=args.rule) as p:
        for r in range(reps + 1):
            torch.cuda.synchronize(local)
            t0 = time.perf_counter()
            p.load_dense(Ah, dirs, b, c, maximize=True)
            st = p.solve()
            el = time.perf_counter() - t0
            s = p.stats()
            if r:
                runs.append({"status": st, "time_to_optimal_s": el, "iterations": s["iterations"]})
        obj = p.solution(st).objval
    best = min(runs, key=lambda r: r["time_to_optimal_s"])
    return {"workload": "dense random LP m=500 n=2000 seed %d (BASELINE configs[1]), from host memory" % args.seed,
            "status": best["status"], "objective": obj, "iterations": best["iterations"],
            "time_to_optimal_s": best["time_to_optimal_s"],
            "value": best["iterations"] / best["time_to_optimal_s"], "unit": "iterations/s (whole solve)",
            "runs": [r["time_to_optimal_s"] for r in runs]}


def small_lps(args, local, with_cpu, reps=5):
    """The models EasyLP's R front-end builds: the reference's
    DOP LP (tests/testthat/test-DOP.R:27-54), Klee-Minty n = 12 and 14
    (BASELINE configs[4]'s degenerate case, unscaled, Dantzig: 2^n - 1 pivots)
    and the MIP tests (test-students.R, test-investments.R), through the C ABI
    from host memory (load + solve, what one easylp$solve() call pays), best of
    `reps`: the resident solver (one launch, elp_resident.hip) and the
    multi-workgroup pipeline (resident = 2) beside the oracle on one host core
    (the same arithmetic; lp_solve itself is absent)."""
    import numpy as np
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    from conftest import load_known_answers, load_mip_known_answers
    from make_sparse import klee_minty
    from easylp_amd import Problem

    def gpu_time(m, n, load, is_int=None, **ctl):
        best, best_h, st, stats = None, None, None, None
        for r in range(reps + 1):
            th = time.perf_counter()
            with Problem(m, n, device=local, **ctl) as p:
                t0 = time.perf_counter()
                load(p)
                if is_int is not None:
                    p.set_int(is_int)
                st = p.solve()
                el = time.perf_counter() - t0
                stats = p.stats()
                obj = p.solution(st).objval
            eh = time.perf_counter() - th
            if r and (best is None or el < best):
                best = el
            if r and (best_h is None or eh < best_h):
                best_h = eh
        # seconds: load + solve; with_handle_seconds: elp_create .. elp_destroy
        # around them (R's flow: one handle per easylp$solve()), which includes
        # the stats / solution reads
        return {"seconds": best, "with_handle_seconds": best_h, "status": st, "objective": obj,
                "iterations": stats["iterations"],
                "resident": stats["resident"], "load_s": stats["seconds_load"],
                "kernel_us": stats["resident_ticks"] / 100.0 if stats["resident"] else None,
                "mip_nodes": stats["mip_nodes"] if is_int is not None else None}

    cases = []
    dop = next(r for r in load_known_answers() if r["name"] == "dop")
    cases.append(("dop", "test-DOP.R:27-54 LP (%d x %d), default controls" % dop["A"].shape, dop, {}, {}, None))
    for nk in (12, 14):
        A, dirs, rhs, obj, lo, up, mx = klee_minty(nk)
        rec = {"A": A.toarray(), "dir": dirs, "rhs": rhs, "obj": obj, "lo": lo, "up": up, "maximize": mx}
        cases.append(("klee_minty_%d" % nk, "Klee-Minty cube n = %d, unscaled, Dantzig (%d pivots)" % (nk, 2 ** nk - 1),
                      rec, {"pricing": 0, "scaling": 0}, {"price_rule": 0, "scaling": 0}, None))
    for r in load_mip_known_answers():
        if r["name"] in ("students", "investments"):
            cases.append(("mip_" + r["name"], "test-%s.R MIP (%d x %d, %d integer columns)" % (
                r["name"], r["m"], r["n"], int(r["is_int"].sum())), r, {}, {}, r["is_int"]))
    out = {}
    for name, what, rec, gctl, octl, is_int in cases:
        m, n = rec["A"].shape
        args_lp = (rec["A"], rec["dir"], rec["rhs"], rec["obj"], rec["lo"], rec["up"], rec["maximize"])
        load = (lambda p, a=args_lp: p.load_dense(*a))
        blk = {"workload": what,
               "resident": gpu_time(m, n, load, is_int, resident=0, **gctl),
               "pipeline": gpu_time(m, n, load, is_int, resident=2, **gctl)}
        if with_cpu:
            from oracle import solve_dense as orc, solve_mip
            ts = []
            for _ in range(reps):
                t0 = time.perf_counter()
                if is_int is None:
                    o = orc(*args_lp, **octl)
                else:
                    o = solve_mip(*args_lp, is_int, **octl)
                ts.append(time.perf_counter() - t0)
            blk["cpu_oracle"] = {"seconds": min(ts), "status": o.status, "objective": o.objval, "cores": 1}
            g = blk["resident"]["seconds"]
            blk["gpu_over_cpu_time"] = g / min(ts) if g else None
        out[name] = blk
    return out


def sparse_rate(args, local, with_cpu):
    """BASELINE config 5 on the CSC path (basis AUTO = the explicit bump
    inverse with k-sized buffers):
      * "Netlib scale": the 20 000 x 100 000 LPs of easylp_amd.synth.sparse_kkt
        (5 nonzeros per column, boxed columns, optimum known by construction
        and pinned by HiGHS in tests/golden/sparse_lu.json), both to
        optimality: the feasible-start one (primal) and the phase-1 one (dual
        simplex phase 1, lp_solve's SIMPLEX_DUAL_PRIMAL default);
      * the seeded 1000 x 10 000 packing LP (sparse_packing) to optimality and
        a steady-state window;
      * the Klee-Minty cube n = 12 (4095 Dantzig pivots on the unscaled cube).
    CPU legs: the oracle (column-chain pricing, price_mode 1, one thread) on
    the packing LP's first iterations and on Klee-Minty; the Netlib-scale LPs'
    CPU times are SciPy HiGHS's (cpu_baseline_highs: the oracle holds A dense,
    16 GB at that size)."""
    import json as _json
    import numpy as np
    from easylp_amd import Problem
    from easylp_amd.synth import sparse_kkt, sparse_packing
    out = {}
    fx = {f["name"]: f for f in _json.load(open(os.path.join(ROOT, "tests", "golden", "sparse_lu.json")))}
    basis_name = {1: "explicit bump inverse (k-sized buffers)"}
    # ---- Netlib scale: 20 000 x 100 000, feasible start, to optimality ----
    k = fx["kkt_feasible_20000x100000"]
    cp, ri, v, b, c, u, obj = sparse_kkt(k["seed"], k["m"], k["n"], k["k"], feasible_start=True)
    m, n = k["m"], k["n"]
    dirs, lo = np.ones(m, np.int32), np.zeros(n)
    with Problem(m, n, device=local, pricing=args.rule) as p:
        t0 = time.perf_counter()
        p.load_csc(cp, ri, v, dirs, b, c, lo, u, maximize=True)
        st = p.solve()
        tto = time.perf_counter() - t0
        s = p.stats()
        z = p.solution(st).objval
    big = {"workload": "sparse LP m=%d n=%d nnz=%d (sparse_kkt feasible_start, boxed; BASELINE configs[4] at "
                       "Netlib scale)" % (m, n, int(cp[-1])),
           "basis": basis_name.get(s["basis"], s["basis"]), "status": st, "objective": z,
           "objective_constructed": obj, "objective_highs": k["highs_objective"],
           "rel_err_vs_highs": abs(z - k["highs_objective"]) / abs(k["highs_objective"]),
           "iterations_to_optimal": s["iterations"], "bound_flips": s["bound_flips"], "refactors": s["refactors"],
           "time_to_optimal_s": tto, "load_s": s["seconds_load"],
           "value": s["iterations"] / tto if tto > 0 else None, "unit": "iterations/s (whole solve)",
           "basic_structurals": s["bump_dim"], "dense_inverse_bytes_avoided": 3 * 8 * m * m}
    out["netlib_scale"] = big
    # ---- the phase-1 LP of the same size: the dual simplex phase 1 (lp_solve's
    #      SIMPLEX_DUAL_PRIMAL) to optimality ----
    k = fx["kkt_20000x100000"]
    cp, ri, v, b, c, u, obj = sparse_kkt(k["seed"], k["m"], k["n"], k["k"])
    with Problem(m, n, device=local, pricing=args.rule, simplex=6) as p:
        t0 = time.perf_counter()
        p.load_csc(cp, ri, v, dirs, b, c, lo, u, maximize=True)
        st = p.solve()
        tto = time.perf_counter() - t0
        s = p.stats()
        z = p.solution(st).objval
    out["netlib_scale_phase1"] = {
        "workload": "sparse LP m=%d n=%d nnz=%d (sparse_kkt: %d rows with b < 0, one column in ten at its "
                    "upper bound in the optimum), dual simplex phase 1 + primal phase 2" % (
                        m, n, int(cp[-1]), int((b < 0).sum())),
        "simplex": "dual-primal" if s["simplex"] == 6 else "primal-primal",
        "status": st, "objective": z, "objective_highs": k["highs_objective"],
        "rel_err_vs_highs": abs(z - k["highs_objective"]) / abs(k["highs_objective"]),
        "iterations_to_optimal": s["iterations"], "dual_iterations": s["dual_iterations"],
        "bound_flips": s["bound_flips"], "refactors": s["refactors"], "basic_structurals": s["bump_dim"],
        "time_to_optimal_s": tto, "load_s": s["seconds_load"],
        "value": s["iterations"] / tto if tto > 0 else None, "unit": "iterations/s (whole solve)",
        "highs_iterations": k["highs_iterations"]}
    # ---- 1000 x 10 000 packing ----
    m, n = args.sparse_m, args.sparse_n
    cp, ri, v, b, c = sparse_packing(args.seed, m, n, 5)
    dirs = np.ones(m, np.int32)
    p = Problem(m, n, device=local, pricing=args.rule)
    t0 = time.perf_counter()
    p.load_csc(cp, ri, v, dirs, b, c, maximize=True)
    st = p.solve()
    tto = time.perf_counter() - t0
    s2 = p.stats()
    sol = p.solution(st)
    p.load_csc(cp, ri, v, dirs, b, c, maximize=True)  # steady-state window [100, 100 + steps)
    p.iterate(100)
    s0 = p.stats()
    t0 = time.perf_counter()
    p.iterate(args.sparse_steps)
    el = time.perf_counter() - t0
    s1 = p.stats()
    p.close()
    it = s1["iterations"] - s0["iterations"]
    out.update({"workload": "sparse LP m=%d n=%d nnz=%d (CSC)" % (m, n, int(cp[-1])),
                "basis": basis_name.get(s2["basis"], s2["basis"]),
                "value": s2["iterations"] / tto, "unit": "iterations/s (whole solve)",
                "time_to_optimal_s": tto, "status": st, "objective": sol.objval,
                "iterations_to_optimal": s2["iterations"], "basic_structurals": s2["bump_dim"],
                "window": {"iterations": [100, 100 + it], "value": it / el if el > 0 else None}})
    km = 12  # Klee-Minty cube: Dantzig's exponential path (2^n - 1 pivots) on the unscaled cube
    rows, cols, vals = [], [], []
    for i in range(km):
        for j in range(i + 1):
            rows.append(i)
            cols.append(j)
            vals.append(1.0 if i == j else 2.0 ** (i - j + 1))
    import scipy.sparse as sp
    K = sp.csc_matrix((vals, (rows, cols)), shape=(km, km))
    kb = np.array([5.0 ** (i + 1) for i in range(km)])
    kc = np.array([2.0 ** (km - 1 - j) for j in range(km)])
    with Problem(km, km, device=local, pricing=0, scaling=0) as pk:
        t0 = time.perf_counter()
        pk.load_csc(K.indptr, K.indices, K.data, np.ones(km, np.int32), kb, kc, maximize=True)
        kst = pk.solve()
        kt = time.perf_counter() - t0
        ks = pk.stats()
        kobj = pk.solution(kst).objval
    out["klee_minty"] = {"n": km, "pricing": "dantzig", "scaling": "off", "iterations": ks["iterations"],
                         "expected_iterations": 2 ** km - 1, "seconds": kt, "objective": kobj,
                         "expected": 5.0 ** km}
    if with_cpu:
        from oracle import solve_dense as orc
        from easylp_amd.synth import dense_of
        r = orc(dense_of(cp, ri, v, m, n), dirs, b, c, maximize=True, price_rule=args.rule, price_mode=1,
                max_iter=100 + args.sparse_cpu_iters)
        out["cpu_baseline"] = {"value": r.stats["iterations"] / r.stats["seconds"], "unit": "iterations/s",
                               "cores": 1, "kind": "port",
                               "sample": "oracle/elp_oracle.c (C, -O3, 1 thread, column-chain pricing) first %d "
                                         "iterations, setup included" % r.stats["iterations"]}
        t0 = time.perf_counter()
        rk = orc(K.toarray(), np.ones(km, np.int32), kb, kc, maximize=True, price_rule=0, price_mode=1, scaling=0)
        out["klee_minty"]["cpu_seconds"] = time.perf_counter() - t0
        out["klee_minty"]["cpu_iterations"] = rk.stats["iterations"]
        # (> 1: the GPU is slower -- 4095 latency-bound pivots of a 12 x 12 LP)
        out["klee_minty"]["gpu_over_cpu_time"] = kt / out["klee_minty"]["cpu_seconds"]
    return out


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--highs-child":
        return highs_child(sys.argv[2:])
    args = parse()
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if args.mode == "procs" and args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        sys.exit(relaunch_under_torchrun(args))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if world > 1 and args.gpus != world:
        raise SystemExit(f"--gpus {args.gpus} but WORLD_SIZE={world}")

    import torch
    import torch.distributed as dist

    if world > 1:
        dist.init_process_group("gloo", init_method="env://")
        if args.mode == "ngpu":
            ok = torch.tensor([1 if rank != 0 else (1 if ngpu_probe(args, local) else 0)], dtype=torch.int32)
            dist.broadcast(ok, 0)
            if not int(ok.item()):
                args.mode = "procs"
                args.fallback = "ngpu probe failed on rank 0: one process per GPU"
    elif args.force_sharded:
        os.environ["ELP_RCCL_SINGLE"] = "1"
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29533")
        dist.init_process_group("gloo", init_method="env://", rank=0, world_size=1)
    ctx = Ctx(args, world, rank, local, dist)
    if not ctx.works:
        # torchrun rank of the ngpu mode: rank 0's one process drives every GPU;
        # this rank joins the barriers around the timed region and the max, then
        # waits for the end (it touches no GPU)
        dist.barrier()
        dist.barrier()
        ctx.max_over_ranks(0.0)
        dist.barrier()
        dist.destroy_process_group()
        return
    torch.cuda.set_device(ctx.devices[0])

    from easylp_amd._lib import load

    lib = load()

    As, b, c = place_A(args.seed, args.m, args.n, ctx)  # resident in HBM, untimed
    p, p2p = make_problem(args, lib, args.m, args.n, ctx)

    full_solves(p, As, b, c, args.warmup, ctx)  # warmup (untimed)
    ctx.barrier()
    t0 = time.perf_counter()
    recs = full_solves(p, As, b, c, args.steps, ctx)
    ctx.barrier()
    elapsed = ctx.max_over_ranks(time.perf_counter() - t0)
    stats = [r[2] for r in recs]
    iters = sum(s["iterations"] for s in stats)
    value = iters / elapsed if elapsed > 0 else 0.0
    # the pricing kernel's time: HIP events bound to the pricing dispatches
    # (hipExtLaunchKernelGGL, on the solver's stream) of every 8th chunk of
    # iterations between host polls in the timed solves -- a uniform sample, so
    # the markers stay off most dispatches (events on all of them cost ~9 %)
    roof = dict(price_roofline(stats), timer="the pricing kernel's own s_memrealtime stamps (first workgroup start -> "
                "last workgroup end) on the pricing dispatches of every 8th chunk of the timed solves; HIP events "
                "bound to the same dispatches in avg_launch_us_events")
    last = stats[-1] if stats else p.stats()
    sol = p.solution(recs[-1][0]) if recs else None  # what the last timed solve returns to its caller
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, sol)
    final = {"status": recs[-1][0] if recs else None, "iterations_to_optimal": last["iterations"],
             "objective": sol.objval if recs else None,
             "bump_dim": last["bump_dim"], "y_rows": last["y_rows"], "refactors": last["refactors"],
             "gj_refactors": last["gj_refactors"], "max_inv_resid": last["max_inv_resid"],
             "load_s": sum(s["seconds_load"] for s in stats) / max(len(stats), 1),
             "price_launches_per_solve": last["price_launches"]}

    window = None  # steady state of one solve: iterations [100, 1100)
    if args.window:
        load_resident(p, As, b, c)
        p.iterate(100)
        ctx.sync()
        w0 = p.stats()
        tw = time.perf_counter()
        p.iterate(1000)
        ctx.sync()
        tw = time.perf_counter() - tw
        w1 = p.stats()
        wit = w1["iterations"] - w0["iterations"]
        wr = price_roofline([{k: w1[k] - w0[k] for k in ("price_seconds", "price_timed_bytes",
                                                         "price_timed_launches")}])
        window = {"iterations": [100, 100 + wit], "value": wit / tw if tw > 0 else None,
                  "us_per_iteration": 1e6 * tw / max(wit, 1), "price_frac": wr["frac"],
                  "price_avg_launch_us": wr["avg_launch_us"]}

    traffic, traffic_src = committed_traffic(args) if args.full and max(world, ctx.ngpu) == 1 else (None, None)
    highs = HighsLeg(args) if rank == 0 and max(world, ctx.ngpu) == 1 and args.highs and not args.no_cpu else None

    other = None  # the same LP to optimality under the other pricing rule
    if args.compare_rules and max(world, ctx.ngpu) == 1 and not args.force_sharded:
        from easylp_amd import Problem
        import numpy as np
        with Problem(args.m, args.n, device=local, pricing=1 - args.rule, sync_every=args.sync_every) as q:
            tq = time.perf_counter()
            q.load_dense_device(As[0].data_ptr(), np.ones(args.m, np.int32), b, c, maximize=True)
            qst = q.solve()
            tq = time.perf_counter() - tq
            qs = q.stats()
            other = {"pricing": "dantzig" if args.rule else "devex", "status": qst,
                     "objective": q.solution(qst).objval, "iterations_to_optimal": qs["iterations"],
                     "time_to_optimal_s": tq}
    parallelism = ctx.parallelism(p2p, last)
    p.close()
    del As
    torch.cuda.empty_cache()

    hosted = None
    if args.host_input and ctx.mode != "procs":
        hosted = {"c3": host_input(args, lib, ctx, args.m, args.n, "dense LP m=%d n=%d" % (args.m, args.n), 3)}
        torch.cuda.empty_cache()

    c4 = c4_config(args, lib, ctx) if args.c4 else None
    if hosted is not None and args.host_c4 and args.c4 and ctx.ngpu == 1:
        hosted["c4"] = host_input(args, lib, ctx, 10000, 500000, "dense LP m=10000 n=500000", 1)
        torch.cuda.empty_cache()

    cpu = None
    if rank == 0 and max(world, ctx.ngpu) == 1 and not args.no_cpu:
        cpu = cpu_baseline(args)

    sparse = None
    if args.sparse and max(world, ctx.ngpu) == 1:
        sparse = sparse_rate(args, local, rank == 0 and not args.no_cpu)

    c2 = c2_config(args, local) if args.c2 and max(world, ctx.ngpu) == 1 else None
    small = small_lps(args, local, rank == 0 and not args.no_cpu) if args.small and max(world, ctx.ngpu) == 1 else None

    highs_res = highs.result(timeout=400) if highs is not None else None
    # GPU / CPU on the same LPs (> 1: the GPU is faster)
    if c2 and highs_res and highs_res.get("c2"):
        c2["highs_time_to_optimal_s"] = highs_res["c2"]["time_to_optimal_s"]
        c2["speedup_vs_highs"] = highs_res["c2"]["time_to_optimal_s"] / c2["time_to_optimal_s"]
    for key, hk in (("netlib_scale_phase1", "kkt_20000x100000"), ("netlib_scale", "kkt_feasible_20000x100000")):
        if sparse and highs_res and highs_res.get(hk):
            blk = sparse[key]
            blk["highs_time_to_optimal_s"] = highs_res[hk]["time_to_optimal_s"]
            blk["speedup_vs_highs"] = blk["highs_time_to_optimal_s"] / blk["time_to_optimal_s"]
    # time to optimal includes the H2D copy of A (what .Call pays:
    # elp_load_dense from host memory); the HBM-resident figure stays beside it
    tto_hbm = elapsed / max(args.steps, 1)
    from_host = bool(hosted and hosted.get("c3"))
    tto = hosted["c3"]["best"]["time_to_optimal_s"] if from_host else tto_hbm
    amdahl = None
    if max(world, ctx.ngpu) > 1 and window:  # (the first multi-GPU record explains itself)
        sweep_us = window.get("price_avg_launch_us")
        amdahl = {"us_per_iteration": window["us_per_iteration"], "per_rank_sweep_us": sweep_us,
                  "replicated_chain_us": (window["us_per_iteration"] - sweep_us) if sweep_us else None,
                  "exchange": last.get("exchange"), "exchange_rtt_us": last.get("exchange_rtt_us"),
                  "note": "steady-state window [100, 1100) on rank 0: the sweep from HIP events on its pricing "
                          "dispatches, the chain = the rest of the iteration (select, FTRAN-z, ratio test, "
                          "exchange); exchange_rtt_us: one all-rank mailbox round measured by the set-up probe"}
    if rank == 0:
        line = {
            "metric": METRIC,
            "value": value,
            "unit": "iterations/s",
            "n_gpus": max(world, ctx.ngpu),
            "steps": args.steps,
            "warmup": args.warmup,
            "full": args.full,
            "ms_per_step": 1e3 * elapsed / max(args.steps, 1),
            "higher_is_better": True,
            "scaling": "strong",
            "vs_baseline": None,
            "dtype": "f64",
            "data": "synthetic (counter-based generator into HBM, seed %d)" % args.seed,
            "config": {
                "workload": "dense random LP m=%d n=%d (BASELINE configs[2]), step = one full solve "
                            "(load from HBM + solve to optimality)" % (args.m, args.n),
                "m": args.m, "n": args.n, "seed": args.seed,
                "parallelism": parallelism,
                "fallback": getattr(args, "fallback", None),
                "iterations_timed": iters,
                "pricing": args.pricing,
            },
            "time_to_optimal_s": tto,
            "time_to_optimal_source": "host_input.c3.best (elp_load_dense from host memory, H2D included)"
                                      if from_host else "the timed solves (A resident in HBM)",
            "time_to_optimal_hbm_s": tto_hbm,
            "final": final,
            "steady_state": window,
            "other_pricing": other,
            "roofline": {
                "kernel": "k_price (pricing sweep + %s argmin + deferred update)" % args.pricing,
                "bound": "hbm",
                **roof,
                "traffic": traffic,
                "traffic_source": traffic_src,
                #  C3's live AR rows (~100 MB per sweep) stay in the
                # 256 MiB Infinity Cache (MALL) between sweeps, and FETCH_SIZE counts
                # its hits: the fraction above is against the 8 TB/s HBM peak, but
                # the bytes come from the MALL.  The HBM figure is C4's 2 GB
                # non-temporal sweep, which no cache holds (scaling_config.price_sweep)
                "residency": "MALL-resident (C3 sweep ~100 MB < 256 MiB Infinity Cache)",
                "hbm_sweep": ({"workload": "C4 m=10000 n=500000 pricing sweep, non-temporal loads (beyond "
                                           "the Infinity Cache)",
                               "achieved": c4["price_sweep"]["achieved"], "frac": c4["price_sweep"]["frac"],
                               "avg_launch_us": c4["price_sweep"]["avg_launch_us"],
                               "bytes_per_launch": c4["price_sweep"]["bytes_per_launch"]}
                              if c4 and c4.get("price_sweep") else None),
            },
            "iteration_roofline": iteration_roofline(stats),
            "host_input": hosted,
            "cpu_baseline": cpu,
            "cpu_baseline_highs": highs_res,
            "amdahl": amdahl,
            "scaling_config": c4,
            "c2": c2,
            "sparse_config": sparse,
            "small_lps": small,
        }
        print(json.dumps(line), flush=True)
    if world > 1:
        if ctx.mode == "ngpu":
            dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
