#!/usr/bin/env python3
"""tcsc_gpu_sgemm_q8 on two builds of the library, A B A: did a change to the quantizer's arithmetic cost time?

The method is tools/q8_bench.py's: packed plans of a random ternary W of density 0.67 built on the device, one layer
step (sgemm_q8 with an fp32 Y) timed eagerly and as replays of a graph of 20 steps, HIP events, the median of --reps
windows; one child process per library ($TCSC_AMD_LIB names it), in the order A, B, A again.  A is the parent
commit's build, B this tree's; both run this tree's Python package, which only binds the symbols.  The acceptable
difference is the run's own spread: |A again - A|.  A point is `inside` when |B - A| is no larger than that, or B
lies between the two A's.

    python tools/q8_ab.py --parent-lib FILE [--lib FILE] [--ms 1 16] [--shapes 4096x4096] [--reps 7] --out FILE"""
import argparse
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "sparse-matrix-multiplication-benchmark_amd")
sys.path.insert(0, PKG)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def child(shapes, Ms, reps, out_path):
    import tcsc_amd
    import torch
    from bf16_bench import timed
    from q8_bench import KNOBS, make_plan, time_step

    tcsc_amd.require_gpu()
    for k in KNOBS:
        os.environ.pop(k, None)
    dev = torch.device("cuda:0")
    res = {"lib": tcsc_amd.LIB_PATH, "device": torch.cuda.get_device_name(0), "points": []}
    for K, N in shapes:
        plan = make_plan(torch, tcsc_amd, K, N, 1000 + K + N)
        for M in Ms:
            g = torch.Generator(device=dev)
            g.manual_seed(100 + M)
            Xf = torch.randn((M, K), device=dev, generator=g)
            B = torch.rand(N, device=dev, generator=g) - 0.5
            Y = torch.empty((M, N), device=dev)
            Xq = torch.empty((M, K), dtype=torch.int8, device=dev)
            S = torch.empty(M, device=dev)
            for xt in ("f32", "bf16"):
                X = Xf if xt == "f32" else Xf.to(torch.bfloat16)
                route = plan.launch_info_q8(M, xt)

                def step(st, X=X):
                    plan.sgemm_q8(X, Xq, S, B, Y, M, N, "prelu_basic", 0.2, st)

                t = time_step(torch, timed, step, reps)
                torch.cuda.synchronize()
                res["points"].append(dict(K=K, N=N, M=M, xtype=xt, route=list(route), t=t,
                                          y_sum_bits=int(Y.view(torch.int32).to(torch.int64).sum().item())))
        plan.destroy()
    with open(out_path, "w") as f:
        json.dump(res, f)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--parent-lib", help="libtcsc_amd.so built from the parent commit")
    ap.add_argument("--lib", default=os.path.join(PKG, "lib", "libtcsc_amd.so"))
    ap.add_argument("--ms", nargs="+", type=int, default=[1, 16])
    ap.add_argument("--shapes", nargs="+", default=["4096x4096"], metavar="KxN")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    ap.add_argument("--child-out", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    shapes = [tuple(int(v) for v in s.split("x")) for s in args.shapes]
    if args.child_out:
        child(shapes, args.ms, args.reps, args.child_out)
        return
    if not args.parent_lib or not os.path.exists(args.parent_lib) or not args.out:
        raise SystemExit("--parent-lib must name the parent commit's libtcsc_amd.so, and --out a file")
    runs = []
    with tempfile.TemporaryDirectory() as tmp:
        for n, lib in enumerate((args.parent_lib, args.lib, args.parent_lib)):
            out = os.path.join(tmp, f"run{n}.json")
            cmd = [sys.executable, os.path.abspath(__file__), "--child-out", out, "--reps", str(args.reps), "--ms",
                   *map(str, args.ms), "--shapes", *args.shapes]
            subprocess.run(cmd, env=dict(os.environ, TCSC_AMD_LIB=os.path.abspath(lib)), check=True, timeout=600)
            with open(out) as f:
                runs.append(json.load(f))
    res = {"method": "tools/q8_bench.py's time_step: eager and graph replays of 20 steps, HIP events, median of "
                     f"{args.reps} windows; one process per library in the order parent, this tree, parent again",
           "device": runs[0]["device"], "points": []}
    for a, b, a2 in zip(*(r["points"] for r in runs)):
        p = {k: a[k] for k in ("K", "N", "M", "xtype", "route")}
        p["bits_equal"] = a["y_sum_bits"] == b["y_sum_bits"] == a2["y_sum_bits"]
        for key in ("ms", "graph_ms"):
            pa, pb, pa2 = a["t"][key], b["t"][key], a2["t"][key]
            spread = abs(pa2 - pa)
            p[key] = dict(parent_us=1e3 * pa, this_us=1e3 * pb, parent_again_us=1e3 * pa2, spread_us=1e3 * spread,
                          this_over_parent=pb / pa,
                          inside=bool(abs(pb - pa) <= spread or min(pa, pa2) <= pb <= max(pa, pa2)))
        res["points"].append(p)
        print(f"{p['K']}x{p['N']} M={p['M']:2d} {p['xtype']:4s} route={p['route']} graph us: parent "
              f"{p['graph_ms']['parent_us']:.3f} this {p['graph_ms']['this_us']:.3f} parent again "
              f"{p['graph_ms']['parent_again_us']:.3f} inside={p['graph_ms']['inside']} | eager us: "
              f"{p['ms']['parent_us']:.3f} {p['ms']['this_us']:.3f} {p['ms']['parent_again_us']:.3f} "
              f"inside={p['ms']['inside']} bits={int(p['bits_equal'])}")
    res["all_inside"] = all(p[k]["inside"] for p in res["points"] for k in ("ms", "graph_ms"))
    res["all_bits_equal"] = all(p["bits_equal"] for p in res["points"])
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(f"all inside the spread: {res['all_inside']}; bits equal: {res['all_bits_equal']}; wrote {args.out}")


if __name__ == "__main__":
    main()
