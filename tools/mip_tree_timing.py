"""Small MIPs end to end: load + solve through the C ABI with
the branch and bound inside the resident tree kernel, against the same script
run on the parent commit (one launch per node) and the CPU oracle on one core.

Workloads: the reference's `investments` (20 x 6) and `cyingair` (14 x 8) MIPs
and two generated ones, 10 x 20 and 64 x 40 with binary columns
(tests/test_gpu_mip_tree.py's generator).  A repetition creates a handle,
loads the model, marks the integer columns and solves; the first repetition
(stream, spare buffers, code object) is not reported.

    python tools/mip_tree_timing.py --out parent.json
        on a checkout of the parent commit with its own library: existing API
        only, so the script runs there unchanged -- the baseline
    python tools/mip_tree_timing.py --baseline parent.json --out profiles/mip_tree_timing.json
        this library, the oracle, and the baseline's figures beside them

One JSON document; times in seconds, `spread` = max - min over the repetitions."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def gen(seed, m, n, ub):
    import numpy as np
    rng = np.random.default_rng(seed)
    A = rng.integers(1, 40, (m, n)).astype(float)
    b = np.floor(A.sum(axis=1) * 0.37 * ub / 3) + 0.5
    c = rng.integers(1, 60, n).astype(float)
    return A, np.ones(m, np.int32), b, c, np.zeros(n), np.full(n, float(ub)), True


def workloads():
    import numpy as np
    from conftest import load_mip_known_answers
    recs = {r["name"]: r for r in load_mip_known_answers()}
    out = []
    for name in ("investments", "cyingair"):
        r = recs[name]
        out.append((name, (r["A"], r["dir"], r["rhs"], r["obj"], r["lo"], r["up"], r["maximize"]), r["is_int"]))
    out.append(("gen 10x20 seed 0", gen(0, 10, 20, 1), np.ones(20, np.int32)))
    out.append(("gen 64x40 seed 2", gen(2, 64, 40, 1), np.ones(40, np.int32)))
    return out


def summary(ts):
    import numpy as np
    return {"reps": [float(t) for t in ts], "median": float(np.median(ts)), "min": float(min(ts)),
            "spread": float(max(ts) - min(ts))}


def gpu_leg(args, is_int, reps):
    from easylp_amd import Problem
    tl, ts, tt, first = [], [], [], None
    for _ in range(reps + 1):
        t0 = time.perf_counter()
        p = Problem(len(args[2]), len(args[3]))
        try:
            p.load_dense(*args)
            p.set_int(is_int)
            t1 = time.perf_counter()
            st = p.solve()
            t2 = time.perf_counter()
            s = p.stats()
            info = p.mip_info() if hasattr(p, "mip_info") else None
            res = (st, s["mip_nodes"], s["mip_lp_iterations"])
        finally:
            p.close()
        if first is None:
            first = res
            continue
        assert res == first, "the result changed between repetitions"
        tl.append(t1 - t0)
        ts.append(t2 - t1)
        tt.append(t2 - t0)
    return {"load": summary(tl), "solve": summary(ts), "load_solve": summary(tt), "status": first[0],
            "nodes": first[1], "lp_iterations": first[2], "mip_info": info}


def oracle_leg(args, is_int, reps):
    from oracle import solve_mip
    ts, res = [], None
    for _ in range(reps + 1):
        t0 = time.perf_counter()
        o = solve_mip(*args, is_int)
        ts.append(time.perf_counter() - t0)
        res = (o.status, o.stats["nodes"], o.stats["lp_iterations"])
    return {"solve": summary(ts[1:]), "status": res[0], "nodes": res[1], "lp_iterations": res[2]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--baseline", help="JSON of this script run on the parent commit")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out")
    a = ap.parse_args()
    assert a.reps >= 5
    import torch
    torch.cuda.init()
    from easylp_amd import _lib
    base = json.load(open(a.baseline))["workloads"] if a.baseline else {}
    doc = {"library": os.path.relpath(_lib.LIB_PATH, ROOT), "reps": a.reps, "device": torch.cuda.get_device_name(0),
           "workloads": {}}
    for name, args, is_int in workloads():
        w = {"m": len(args[2]), "n": len(args[3]), "gpu": gpu_leg(args, is_int, a.reps)}
        g = w["gpu"]
        line = (f"{name:18s} {g['nodes']:5d} nodes  load+solve {1e3 * g['load_solve']['median']:8.3f} ms "
                f"(+-{1e3 * g['load_solve']['spread']:.3f})  solve {1e3 * g['solve']['median']:8.3f} ms "
                f"(+-{1e3 * g['solve']['spread']:.3f})")
        if a.baseline:
            w["oracle_1core"] = oracle_leg(args, is_int, a.reps)
            o = w["oracle_1core"]
            assert (o["status"], o["nodes"], o["lp_iterations"]) == (g["status"], g["nodes"], g["lp_iterations"])
            w["solve_vs_oracle"] = g["solve"]["median"] / o["solve"]["median"]
            line += f"  oracle {1e3 * o['solve']['median']:8.3f} ms"
        if name in base:
            b = base[name]["gpu"]
            assert (b["status"], b["nodes"], b["lp_iterations"]) == (g["status"], g["nodes"], g["lp_iterations"])
            w["parent"] = b
            for k in ("solve", "load_solve"):
                w[f"speedup_{k}"] = b[k]["median"] / g[k]["median"]
                # the condition of DESIGN.md 16: faster by more than both spreads
                w[f"beats_parent_beyond_spread_{k}"] = bool(b[k]["median"] - g[k]["median"] > b[k]["spread"] + g[k]["spread"])
            line += (f"  parent load+solve {1e3 * b['load_solve']['median']:8.3f} ms (+-{1e3 * b['load_solve']['spread']:.3f})"
                     f"  x{w['speedup_load_solve']:.2f} (solve x{w['speedup_solve']:.2f})")
        doc["workloads"][name] = w
        print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(doc, f, indent=1)
    print(json.dumps({"out": a.out}))


if __name__ == "__main__":
    main()
