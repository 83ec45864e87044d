"""Throughput of many small LPs: elp_solve_batch against the
sequential elp_solve loop and the CPU oracle on one core.

Workloads: B = 1, 16, 64, 256 copies of Klee-Minty n = 10 (Dantzig, scaling
0), B copies of the DOP LP, and the fuzz set (fuzz_set(120), dense, the
per-seed pricing / refactor period of the tests).  Every repetition creates B
handles, loads them one by one (timed as `load`: loads stay per handle), then
solves them (timed as `solve`) and checks the statuses against the first
repetition's.

    python tools/batch_lp_timing.py --sequential --out seq.json
        the sequential leg alone: existing API only, so it runs on any earlier
        commit's library (ELP_LIB_PATH) -- the baseline
    python tools/batch_lp_timing.py --baseline seq.json --out profiles/batch_lp_timing.json
        batched + sequential (this library) + oracle legs, the baseline's
        figures and the ratios beside them

One JSON document; times in seconds, `spread` = max - min over the repetitions."""
import argparse
import ctypes
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))


def workloads():
    from conftest import load_known_answers
    from fuzz_lps import fuzz_set
    from make_sparse import klee_minty
    A, dirs, rhs, obj, lo, up, mx = klee_minty(10)
    km = ((A.toarray(), dirs, rhs, obj, lo, up, mx), {"pricing": 0, "scaling": 0})
    d = next(r for r in load_known_answers() if r["name"] == "dop")
    dop = ((d["A"], d["dir"], d["rhs"], d["obj"], d["lo"], d["up"], d["maximize"]), {})
    out = []
    for b in (1, 16, 64, 256):
        out.append((f"klee_minty_10 x {b}", [km] * b))
    for b in (1, 16, 64, 256):
        out.append((f"dop x {b}", [dop] * b))
    fz = [((r["A"], r["dir"], r["rhs"], r["obj"], r["lo"], r["up"], r["maximize"]),
           {"pricing": r["seed"] % 2, "refactor_period": 5 + r["seed"] % 40}) for r in fuzz_set(120)]
    out.append(("fuzz_set(120)", fz))
    return out


def summary(ts):
    import numpy as np
    return {"reps": [float(t) for t in ts], "median": float(np.median(ts)), "min": float(min(ts)),
            "spread": float(max(ts) - min(ts))}


def gpu_leg(lps, reps, batched):
    """(load summary, solve summary, statuses, batched count) over reps repetitions"""
    from easylp_amd import Problem
    from easylp_amd._lib import check, load
    lib = load()
    n = len(lps)
    tl, ts, first, nb_seen = [], [], None, 0
    for _ in range(reps + 1):  # (the first repetition warms the streams / spares up: not reported)
        ps = []
        try:
            t0 = time.perf_counter()
            for args, ctl in lps:
                p = Problem(len(args[2]), len(args[3]), **ctl)
                ps.append(p)
                p.load_dense(*args)
            t1 = time.perf_counter()
            st = (ctypes.c_int32 * n)()
            if batched:
                hs = (ctypes.c_void_p * n)(*[p._h for p in ps])
                nb = ctypes.c_int64(0)
                t1 = time.perf_counter()
                check(lib.elp_solve_batch(hs, n, st, ctypes.byref(nb)), "elp_solve_batch")
                t2 = time.perf_counter()
                nb_seen = int(nb.value)
            else:
                hs = [p._h for p in ps]
                one = ctypes.c_int32(0)
                ref = ctypes.byref(one)
                t1 = time.perf_counter()
                for i in range(n):
                    rc = lib.elp_solve(hs[i], ref)
                    st[i] = one.value
                    if rc:
                        check(rc, "elp_solve")
                t2 = time.perf_counter()
                nb_seen = sum(p.stats()["resident"] for p in ps)
            sts = list(st)
            if first is None:
                first = sts
                continue
            assert sts == first, "statuses changed between repetitions"
            tl.append(t1 - t0)
            ts.append(t2 - t1)
        finally:
            for p in ps:
                p.close()
    return summary(tl), summary(ts), first, nb_seen


def oracle_leg(lps, reps):
    from oracle import solve_dense as orc
    keys = {"pricing": "price_rule"}
    ts, sts = [], None
    for _ in range(reps):
        t0 = time.perf_counter()
        sts = [orc(*args, **{keys.get(k, k): v for k, v in ctl.items()}).status for args, ctl in lps]
        ts.append(time.perf_counter() - t0)
    return summary(ts), sts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sequential", action="store_true", help="the sequential elp_solve leg alone (existing API only)")
    ap.add_argument("--baseline", help="JSON of a --sequential run (an earlier commit's library)")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out")
    a = ap.parse_args()
    import torch
    torch.cuda.init()
    from easylp_amd import _lib
    base = json.load(open(a.baseline))["workloads"] if a.baseline else {}
    doc = {"library": os.path.relpath(_lib.LIB_PATH, ROOT), "reps": a.reps, "device": torch.cuda.get_device_name(0),
           "mode": "sequential" if a.sequential else "batched", "workloads": {}}
    for name, lps in workloads():
        w = {"lps": len(lps)}
        load_s, seq, sts, res = gpu_leg(lps, a.reps, batched=False)
        w["sequential"] = {"load": load_s, "solve": seq, "resident": res,
                           "lps_per_s": len(lps) / seq["median"]}
        if not a.sequential:
            load_b, bat, sts_b, nb = gpu_leg(lps, a.reps, batched=True)
            assert sts_b == sts, "batched statuses differ from the sequential loop's"
            w["batched"] = {"load": load_b, "solve": bat, "batched": nb, "lps_per_s": len(lps) / bat["median"],
                            "load_share": load_b["median"] / (load_b["median"] + bat["median"])}
            w["speedup_vs_sequential"] = seq["median"] / bat["median"]
            orc_s, sts_o = oracle_leg(lps, a.reps)
            assert sts_o == sts, "oracle statuses differ"
            w["oracle_1core"] = {"solve": orc_s, "lps_per_s": len(lps) / orc_s["median"]}
            w["throughput_vs_oracle"] = orc_s["median"] / bat["median"]
            if name in base:
                bs = base[name]["sequential"]["solve"]
                w["baseline_sequential"] = base[name]["sequential"]
                w["speedup_vs_baseline"] = bs["median"] / bat["median"]
                # the condition of DESIGN.md 15: faster by more than both spreads
                w["beats_baseline_beyond_spread"] = bool(bs["min"] - bat["median"] > 0 and
                                                         bs["median"] - bat["median"] > bs["spread"] + bat["spread"])
        doc["workloads"][name] = w
        line = f"{name:22s} seq {1e3 * seq['median']:9.3f} ms (+-{1e3 * seq['spread']:.3f})"
        if "batched" in w:
            line += (f"  batch {1e3 * w['batched']['solve']['median']:9.3f} ms (+-{1e3 * w['batched']['solve']['spread']:.3f})"
                     f"  x{w['speedup_vs_sequential']:.2f}  oracle {1e3 * w['oracle_1core']['solve']['median']:9.3f} ms"
                     f"  load {1e3 * w['batched']['load']['median']:9.3f} ms")
            if "speedup_vs_baseline" in w:
                line += f"  baseline x{w['speedup_vs_baseline']:.2f}"
        print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(doc, f, indent=1)
    print(json.dumps({"out": a.out, "mode": doc["mode"]}))


if __name__ == "__main__":
    main()
