#!/usr/bin/env python
"""A/B of the two passive-tracer routes on the cube sphere ("Passive
tracers"): global_ocean_cs32x15 (BASELINE config 3: staggered, r*, the tracers on the critical
path before UPDATE_R_STAR) with N = 0, 1, 4, 8 copies of a scheme-33 tracer started as salt,
useGMRedi = 0 (chosen when GM_AdvForm refused multi-dimensional GM tracers; since the residual
flow became a launch of its own, k_gm_residual_flow, every N >= 1 includes it), diffKr = 3e-5.  Per N one
model per route (MGCM_PTR_BATCH is read when a step graph is captured, and a model keeps the
route of its graphs); forward_step(100) after 20 warm-up steps, host clock around a
synchronise; the two routes timed alternately, batched first, three alternations in one process.

    python tools/ptracers_cube_ab.py [--steps 100] [--warmup 20] [--reps 3] [--n 0,1,4,8] [--out FILE]

Prints one JSON line per measurement, then a summary table with the route and the launches
each model reports (Model.ptracers_route); --out also writes the table and the lines to a file."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(m, steps):
    m.sync()
    t0 = time.perf_counter()
    m.forward_step(steps)
    m.sync()
    return (time.perf_counter() - t0) * 1e3 / steps


def make(n, route, cfg_out):
    from mitgcm_amd import configs
    os.environ["MGCM_PTR_BATCH"] = str(route)
    specs = [dict(advScheme=33, useGMRedi=0, diffKr=3e-5, init=cfg_out[2]["salt"]) for _ in range(n)] if n else None
    return configs.make_model(lambda: cfg_out, ptracers=specs)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--n", default="0,1,4,8")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from mitgcm_amd import configs
    cfg_out = configs.global_ocean_cs32x15()
    rows, routes = [], {}
    for n in [int(x) for x in a.n.split(",")]:
        models = {}
        for route in ((1, 0) if n else (0,)):
            m = make(n, route, cfg_out)
            m.forward_step(a.warmup)
            m.sync()
            models[route] = m
            routes[(n, route)] = m.ptracers_route()
        for rep in range(a.reps):
            for route, m in models.items():
                os.environ["MGCM_PTR_BATCH"] = str(route)
                rows.append({"n": n, "switch": route, "route": routes[(n, route)]["route"],
                             "launches": routes[(n, route)]["launches"], "rep": rep, "ms_per_step": timed(m, a.steps)})
                print(json.dumps(rows[-1]), flush=True)
        for m in models.values():
            m.close()
    base = min(r["ms_per_step"] for r in rows if r["n"] == 0) if any(r["n"] == 0 for r in rows) else None
    lines = ["%3s %-11s %8s  %s" % ("N", "route", "launches", "ms/step per alternation (min)")]
    for key in sorted({(r["n"], r["switch"]) for r in rows}):
        sel = [r for r in rows if (r["n"], r["switch"]) == key]
        v = [r["ms_per_step"] for r in sel]
        inc = "" if not key[0] or base is None else "  +%.4f ms per tracer" % ((min(v) - base) / key[0])
        lines.append("%3d %-11s %8d  %s (%.4f)%s" % (key[0], sel[0]["route"], sel[0]["launches"],
                                                     " ".join("%.4f" % x for x in v), min(v), inc))
    print("\n" + "\n".join(lines))
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n\n")
            for r in rows:
                fh.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
