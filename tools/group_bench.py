#!/usr/bin/env python3
"""Times the Q, K, V projections of an attention block -- one bf16 X, the subnorm in front, three ternary matrices
with column scales and biases, bf16 outputs -- as the one grouped call (tcsc_gpu_sgemm_q8_group)
against what a caller wrote before it existed.

tools/out_bench.py's protocol: HIP events around windows of replays of a captured graph of GRAPH_STEPS steps after a
warm-up, median per step of --reps windows.  A step is one bf16 X (M x K) in and one bf16 Y (M x sum of the members'
columns) out, of which every member writes its column slice, on packed plans of random ternary matrices of density
0.67.

Two legs, which give the same bytes (asserted: the SHA-256 of every member's slice of Y):

  (A) the parent commit's library doing the best a caller could write before: quantize_rows_i8_norm once and one
      sgemm_i8 with col_scale and a bf16 Y per member (`A_parent`, and once more after everything else,
      `A_parent_again`: the run's own spread)
  (B) the one new call on this tree's library (`B_new`)

and a second block without the norm at M <= 4, where (B) runs the quantizer inside the grouped decode launch
wherever tcsc_gpu_group_fuse_pays says so; there (A) is quantize_rows_i8 plus the member calls.

Three child processes, one library each, every point in each, in the order parent, new, parent_again.  The parent is
--parent-pkg: a build of the parent commit (its `tcsc_amd/` and `lib/`; $TCSC_AMD_LIB names its library).

Per point: spread = |A_parent_again - A_parent| / A_parent and `A_over_B`, the ratio of the parent's mean median to
(B).  One JSON document goes to --out (default profiles/group_bench.json) and a table to stdout.  Needs a gfx950 GPU.

    python tools/group_bench.py --parent-pkg DIR [--reps 5] [--shapes KxN1+N2+N3 ...] [--ms M ...] [--out FILE]
"""
import argparse
import hashlib
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "sparse-matrix-multiplication-benchmark_amd")
sys.path.insert(0, os.path.join(ROOT, "tools"))

SHAPES = [(2560, (2560, 640, 640)), (4096, (4096, 4096, 4096)), (8192, (8192, 1024, 1024))]  # K, the members' columns
MS = (1, 2, 4, 8, 16, 64, 2048)
PLAIN_MAX_M = 4  # the block without the norm: where the quantizer can run inside the launch
EPS = 1e-5
KNOBS = ("TCSC_PATH", "TCSC_SMALL_M", "TCSC_SLICES", "TCSC_MFMA_WGS", "TCSC_DECODE", "TCSC_QFUSE", "TCSC_W2GEMM")


def child(mode, shapes, ms, reps, out_path):
    """One library, every point.  mode: parent / parent_again (leg A), new (leg B)."""
    import tcsc_amd
    import torch

    from out_bench import make_plan, time_graph
    from bf16_bench import timed

    tcsc_amd.require_gpu()
    for k in KNOBS:
        os.environ.pop(k, None)
    is_new = os.path.realpath(tcsc_amd.LIB_PATH).startswith(os.path.realpath(PKG) + os.sep)
    assert is_new == (mode == "new"), f"mode {mode} on the wrong library ({tcsc_amd.LIB_PATH})"
    dev = torch.device("cuda:0")
    res = {"mode": mode, "lib": tcsc_amd.LIB_PATH, "device": torch.cuda.get_device_name(0), "points": []}
    for K, cols in shapes:
        plans = [make_plan(torch, tcsc_amd, K, n, 1000 * (i + 1) + K + n) for i, n in enumerate(cols)]
        for p in plans:
            p.reserve(max(ms))
        total = sum(cols)
        for M in ms:
            g = torch.Generator(device=dev)
            g.manual_seed(100 + M)
            X = torch.randn((M, K), device=dev, generator=g).to(torch.bfloat16)
            gamma = torch.rand(K, device=dev, generator=g) + 0.5
            bs = [torch.rand(n, device=dev, generator=g) - 0.5 for n in cols]
            cs = [torch.rand(n, device=dev, generator=g) * 0.04 + 0.01 for n in cols]  # per-column beta of an absmean rule
            Y = torch.empty((M, total), dtype=torch.bfloat16, device=dev)
            Ys = list(torch.split(Y, list(cols), dim=1))
            Xq = torch.empty((M, K), dtype=torch.int8, device=dev)
            S = torch.empty(M, device=dev)
            for norm in (True, False):
                if not norm and M > PLAIN_MAX_M:
                    continue
                p = {"K": K, "cols": list(cols), "M": M, "norm": norm}

                def leg_a(st):
                    if norm:
                        tcsc_amd.quantize_rows_i8_norm(X, Xq, S, M, K, gamma, EPS, st)
                    else:
                        tcsc_amd.quantize_rows_i8(X, Xq, S, M, K, st)
                    for plan, b, c, y in zip(plans, bs, cs, Ys):
                        plan.sgemm_i8(Xq, S, b, y, M, total, "basic", 0.0, st, col_scale=c)

                def leg_b(st):
                    tcsc_amd.sgemm_q8_group(plans, X, Xq, S, bs, Ys, M, [total] * len(cols), cs, gamma if norm else None,
                                            EPS if norm else None, st)

                leg = leg_b if mode == "new" else leg_a
                if mode == "new":
                    path, slices, fused = tcsc_amd.launch_info_group(plans, M, "bf16")
                    p["route"] = [path, slices, bool(fused and not norm)]  # with the norm the call is never fused
                p[("B_" if mode == "new" else "A_") + mode] = time_graph(torch, timed, leg, reps)
                Y.zero_()
                S.zero_()
                leg(torch.cuda.current_stream().cuda_stream)
                torch.cuda.synchronize()
                p["sha256"] = [hashlib.sha256(y.contiguous().view(torch.int16).cpu().numpy().tobytes()).hexdigest()
                               for y in Ys]
                p["scale_sha256"] = hashlib.sha256(S.cpu().numpy().tobytes()).hexdigest()
                res["points"].append(p)
        for p in plans:
            p.destroy()
        torch.cuda.empty_cache()
        print(f"[{mode}] K={K} cols={cols} done", file=sys.stderr, flush=True)
    with open(out_path, "w") as f:
        json.dump(res, f)


def run_child(mode, pkg, args, tmp):
    out = os.path.join(tmp, mode + ".json")
    env = dict(os.environ, PYTHONPATH=pkg + os.pathsep + os.environ.get("PYTHONPATH", ""),
               TCSC_AMD_LIB=os.path.join(pkg, "lib", "libtcsc_amd.so"))
    cmd = [sys.executable, os.path.abspath(__file__), "--child", mode, "--child-out", out, "--reps", str(args.reps),
           "--ms"] + [str(m) for m in args.ms] + ["--shapes"] + [f"{k}x" + "+".join(map(str, c)) for k, c in args.shape_list]
    subprocess.run(cmd, env=env, check=True, timeout=900)
    with open(out) as f:
        return json.load(f)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--parent-pkg", help="a build of the parent commit: the directory holding its tcsc_amd/ and lib/")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--shapes", nargs="+", default=None, metavar="KxN1+N2+..")
    ap.add_argument("--ms", nargs="+", type=int, default=list(MS))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "group_bench.json"))
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--child-out", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    args.shape_list = SHAPES if not args.shapes else [
        (int(s.lower().split("x")[0]), tuple(int(v) for v in s.lower().split("x")[1].split("+"))) for s in args.shapes]
    if args.child:
        child(args.child, args.shape_list, args.ms, args.reps, args.child_out)
        return
    if not args.parent_pkg or not os.path.exists(os.path.join(args.parent_pkg, "lib", "libtcsc_amd.so")):
        raise SystemExit("--parent-pkg must name a build of the parent commit (tcsc_amd/ and lib/libtcsc_amd.so)")
    parent = os.path.abspath(args.parent_pkg)
    with tempfile.TemporaryDirectory() as tmp:
        runs = [run_child("parent", parent, args, tmp), run_child("new", PKG, args, tmp),
                run_child("parent_again", parent, args, tmp)]
    res = {"tool": "tools/group_bench.py", "device": runs[0]["device"], "eps": EPS, "density": 0.67, "plan": "packed",
           "xtype": "bf16", "ytype": "bf16", "graph_steps": runs[0]["points"][0]["A_parent"]["graph_steps"],
           "timing": "HIP events around windows of replays of a captured graph of graph_steps steps; median per step of "
                     "--reps windows; one child process per library, in the order parent, new, parent_again",
           "legs": {"A": "parent: quantize_rows_i8_norm (norm false: quantize_rows_i8) once, then one sgemm_i8 with "
                         "col_scale into its bf16 column slice of Y per member",
                    "B": "new: sgemm_q8_group (norm false: without the norm) into the same slices"},
           "points": []}
    for a, b, c in zip(*(r["points"] for r in runs)):
        key = lambda p: (p["K"], p["cols"], p["M"], p["norm"])
        assert key(a) == key(b) == key(c)
        assert a["sha256"] == b["sha256"] == c["sha256"] and a["scale_sha256"] == b["scale_sha256"], \
            f"legs A and B differ at K={a['K']} cols={a['cols']} M={a['M']} norm={a['norm']}"
        p = {"K": a["K"], "cols": a["cols"], "M": a["M"], "norm": a["norm"], "route": b["route"], "A_parent": a["A_parent"],
             "B_new": b["B_new"], "A_parent_again": c["A_parent_again"], "bits_equal": True}
        a0, a1, bn = p["A_parent"]["graph_ms"], p["A_parent_again"]["graph_ms"], p["B_new"]["graph_ms"]
        p["spread"] = abs(a1 - a0) / a0
        p["A_over_B"] = 0.5 * (a0 + a1) / bn
        p["B_wins_beyond_spread"] = bool(bn < min(a0, a1) * (1.0 - p["spread"]))
        p["B_loses_beyond_spread"] = bool(bn > max(a0, a1) * (1.0 + p["spread"]))
        res["points"].append(p)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    for p in res["points"]:
        verdict = "wins" if p["B_wins_beyond_spread"] else "LOSES" if p["B_loses_beyond_spread"] else "level"
        print(f"K={p['K']} cols={'+'.join(map(str, p['cols']))} M={p['M']:4d} norm={int(p['norm'])} {p['route'][0]:6s} "
              f"fused={int(p['route'][2])} | us/step: (A) parent {1e3 * p['A_parent']['graph_ms']:8.2f} again "
              f"{1e3 * p['A_parent_again']['graph_ms']:8.2f} | (B) {1e3 * p['B_new']['graph_ms']:8.2f} | spread "
              f"{100 * p['spread']:4.1f}% A/B x{p['A_over_B']:.2f} {verdict}")


if __name__ == "__main__":
    main()
