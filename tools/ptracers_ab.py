#!/usr/bin/env python
"""A/B of the two passive-tracer routes on tutorial_global_oce_latlon (DESIGN.md section 3,
"Passive tracers"): N = 0, 1, 4, 8 copies of the experiment's age tracer, forward_step(200)
after 20 warm-up steps, ended by sync(), host clock; per N one model per route
(MGCM_PTR_BATCH is read when a step graph is captured), the two timed alternately, batched
first, three alternations in one process.

    python tools/ptracers_ab.py [--steps 200] [--warmup 20] [--reps 3] [--n 0,1,4,8]
                                [--parent-root DIR] [--out FILE]

--parent-root: a built tree of the parent commit (its mitgcm_amd package with the library, and
tests/golden); its N = 0 figure is taken the same way in a child process of its own for every
alternation, beside this build's in a child process too, so the N = 0 figure of this build can
be read beside the parent's run-to-run spread.
Prints one JSON line per measurement and a summary table; --out also writes them to a file."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# (a child process measuring another tree imports that tree's package: MGCM_AB_ROOT)
sys.path.insert(0, os.environ.get("MGCM_AB_ROOT") or ROOT)


def timed(m, steps):
    m.sync()
    t0 = time.perf_counter()
    m.forward_step(steps)
    m.sync()
    return (time.perf_counter() - t0) * 1e3 / steps


def measure(ns, steps, warmup, reps, label):
    from mitgcm_amd import configs
    rows = []
    for n in ns:
        models = {}
        for route in ((1, 0) if n else (1,)):
            os.environ["MGCM_PTR_BATCH"] = str(route)
            specs = configs.global_oce_latlon_ptracers() * n if n else None
            m = (configs.make_model(configs.global_oce_latlon, ptracers=specs) if n
                 else configs.make_model(configs.global_oce_latlon))
            m.forward_step(warmup)
            m.sync()
            models[route] = m
        for rep in range(reps):
            for route, m in models.items():
                os.environ["MGCM_PTR_BATCH"] = str(route)
                rows.append({"build": label, "n": n, "route": "batched" if route else "functional", "rep": rep,
                             "ms_per_step": timed(m, steps)})
                print(json.dumps(rows[-1]), flush=True)
        for m in models.values():
            m.close()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--n", default="0,1,4,8")
    ap.add_argument("--parent-root", default=None)
    ap.add_argument("--label", default="this")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    ns = [int(x) for x in a.n.split(",")]
    rows = []
    if a.parent_root:   # a fresh process per tree: a process binds one package and one library
        for rep in range(a.reps):
            for root, label in ((a.parent_root, "parent"), (ROOT, "this")):
                env = dict(os.environ)
                env["MGCM_AB_ROOT"] = os.path.abspath(root)
                out = subprocess.run([sys.executable, os.path.abspath(__file__), "--n", "0", "--reps", "1", "--steps",
                                      str(a.steps), "--warmup", str(a.warmup), "--label", label], env=env, check=True,
                                     stdout=subprocess.PIPE, text=True).stdout
                for line in out.splitlines():
                    if line.startswith("{"):
                        r = json.loads(line)
                        r["rep"] = rep
                        r["own_process"] = True
                        rows.append(r)
                        print(json.dumps(r), flush=True)
    rows += measure(ns, a.steps, a.warmup, a.reps, a.label)
    if a.label == "this" and len(ns) > 1:
        print("\n%-8s %3s %-11s %s" % ("build", "N", "route", "ms/step per alternation (min)"))
        keys = sorted({(r["build"], r["n"], r["route"], r.get("own_process", False)) for r in rows}, key=str)
        base = min(r["ms_per_step"] for r in rows if r["build"] == "this" and r["n"] == 0 and not r.get("own_process"))
        for k in keys:
            v = [r["ms_per_step"] for r in rows if (r["build"], r["n"], r["route"], r.get("own_process", False)) == k]
            inc = "" if k[1] == 0 else "  +%.4f ms per tracer" % ((min(v) - base) / k[1])
            print("%-8s %3d %-11s %s (%.4f)%s%s" % (k[0], k[1], k[2], " ".join("%.4f" % x for x in v), min(v), inc,
                                                   "  [own process]" if k[3] else ""))
    if a.out:
        with open(a.out, "w") as fh:
            for r in rows:
                fh.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
