#!/usr/bin/env python3
"""Times the output and down projections of a BitNet-style block with their skip connection, h = h + proj(subnorm(x))
-- one bf16 X, the subnorm in front, a ternary matrix with column scales and a bias, and a bf16 residual stream h
updated in place -- as the one residual call (tcsc_gpu_sgemm_q8_res) against what a caller wrote before
it existed.

tools/group_bench.py's protocol: HIP events around windows of replays of a captured graph of GRAPH_STEPS steps after a
warm-up, median per step of --reps windows, on packed plans of random ternary matrices of density 0.67.

Legs:

  (A)  the parent commit's library: sgemm_q8_norm with col_scale into a bf16 y, then torch's h.add_(y) (`A_parent`, and
       once more after everything else, `A_parent_again`: the run's own spread).  This rounds twice, to bf16 in the
       call and again in the add, so its bytes are not those of (B).
  (A') the parent's call into an fp32 y, then torch's y.add_(h) and h.copy_(y): the one-rounding composition, the
       bytes of (B) (`A1_parent`; asserted: the SHA-256 of h after one step from the same h, and of the scales).
  (B)  the one new call on this tree's library, Y = R = h (`B_new`).
  (old) sgemm_q8_norm without a residual into a bf16 y, on the parent, on this tree and on the parent again
       (`old_parent`, `old_new`, `old_parent_again`): the old entry point must not pay for the feature.

Three child processes, one library each, every point in each, in the order parent, new, parent_again.  The parent is
--parent-pkg: a build of the parent commit (its `tcsc_amd/` and `lib/`; $TCSC_AMD_LIB names its library).

Per point: spread = |A_parent_again - A_parent| / A_parent, `A_over_B` and `A1_over_B` (ratios to (B) of the parent's
mean median of (A) and of (A')), and for the old entry point `old_spread` and `old_within_spread`.  One JSON document
goes to --out (default profiles/res_bench.json) and a table to stdout.  Needs a gfx950 GPU.

    python tools/res_bench.py --parent-pkg DIR [--reps 5] [--shapes KxN ...] [--ms M ...] [--out FILE]
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

SHAPES = [(2560, 2560), (6912, 2560), (4096, 4096), (8192, 8192)]  # K x N: o_proj and down of the 2B4T shape, two squares
MS = (1, 2, 4, 8, 16, 64, 2048)
EPS = 1e-5
KNOBS = ("TCSC_PATH", "TCSC_SMALL_M", "TCSC_SLICES", "TCSC_MFMA_WGS", "TCSC_DECODE", "TCSC_QFUSE", "TCSC_W2GEMM")


def child(mode, shapes, ms, reps, out_path):
    """One library, every point.  mode: parent (legs A, A', old), parent_again (A, old), new (B, old)."""
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
    for K, N in shapes:
        plan = make_plan(torch, tcsc_amd, K, N, 2600 + K + N)
        plan.reserve(max(ms))
        for M in ms:
            g = torch.Generator(device=dev)
            g.manual_seed(100 + M)
            X = torch.randn((M, K), device=dev, generator=g).to(torch.bfloat16)
            gamma = torch.rand(K, device=dev, generator=g) + 0.5
            b = torch.rand(N, device=dev, generator=g) - 0.5
            c = torch.rand(N, device=dev, generator=g) * 0.04 + 0.01  # per-column beta of an absmean rule
            h0 = torch.randn((M, N), device=dev, generator=g).to(torch.bfloat16)
            h = h0.clone()
            y = torch.empty((M, N), dtype=torch.bfloat16, device=dev)
            y32 = torch.empty((M, N), device=dev)
            Xq = torch.empty((M, K), dtype=torch.int8, device=dev)
            S = torch.empty(M, device=dev)
            p = {"K": K, "N": N, "M": M}

            def old(st):
                plan.sgemm_q8_norm(X, Xq, S, b, y, M, N, gamma, EPS, "basic", 0.0, st, col_scale=c)

            def leg_a(st):
                old(st)
                h.add_(y)

            def leg_a1(st):
                plan.sgemm_q8_norm(X, Xq, S, b, y32, M, N, gamma, EPS, "basic", 0.0, st, col_scale=c)
                y32.add_(h)
                h.copy_(y32)

            def leg_b(st):
                plan.sgemm_q8_norm(X, Xq, S, b, h, M, N, gamma, EPS, "basic", 0.0, st, col_scale=c, residual=h)

            legs = {"parent": (("A", leg_a), ("A1", leg_a1), ("old", old)), "parent_again": (("A", leg_a), ("old", old)),
                    "new": (("B", leg_b), ("old", old))}[mode]
            for name, leg in legs:
                h.copy_(h0)
                p[f"{name}_{mode}"] = time_graph(torch, timed, leg, reps)
            if mode == "new":
                path, slices, fused = plan.launch_info_q8_norm(M, "bf16")
                p["route"] = [path, slices, bool(fused)]
            if mode != "parent_again":  # the bytes of one step from h0: (A') on the parent, (B) on this tree
                h.copy_(h0)
                S.zero_()
                (leg_b if mode == "new" else leg_a1)(torch.cuda.current_stream().cuda_stream)
                torch.cuda.synchronize()
                p["sha256"] = hashlib.sha256(h.view(torch.int16).cpu().numpy().tobytes()).hexdigest()
                p["scale_sha256"] = hashlib.sha256(S.cpu().numpy().tobytes()).hexdigest()
            res["points"].append(p)
        plan.destroy()
        torch.cuda.empty_cache()
        print(f"[{mode}] K={K} N={N} done", file=sys.stderr, flush=True)
    with open(out_path, "w") as f:
        json.dump(res, f)


def run_child(mode, pkg, args, tmp):
    out = os.path.join(tmp, mode + ".json")
    env = dict(os.environ, PYTHONPATH=pkg + os.pathsep + os.environ.get("PYTHONPATH", ""),
               TCSC_AMD_LIB=os.path.join(pkg, "lib", "libtcsc_amd.so"))
    cmd = [sys.executable, os.path.abspath(__file__), "--child", mode, "--child-out", out, "--reps", str(args.reps),
           "--ms"] + [str(m) for m in args.ms] + ["--shapes"] + [f"{k}x{n}" for k, n in args.shape_list]
    subprocess.run(cmd, env=env, check=True, timeout=900)
    with open(out) as f:
        return json.load(f)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--parent-pkg", help="a build of the parent commit: the directory holding its tcsc_amd/ and lib/")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--shapes", nargs="+", default=None, metavar="KxN")
    ap.add_argument("--ms", nargs="+", type=int, default=list(MS))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "res_bench.json"))
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--child-out", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    args.shape_list = SHAPES if not args.shapes else [tuple(int(v) for v in s.lower().split("x")) for s in args.shapes]
    if args.child:
        child(args.child, args.shape_list, args.ms, args.reps, args.child_out)
        return
    if not args.parent_pkg or not os.path.exists(os.path.join(args.parent_pkg, "lib", "libtcsc_amd.so")):
        raise SystemExit("--parent-pkg must name a build of the parent commit (tcsc_amd/ and lib/libtcsc_amd.so)")
    parent = os.path.abspath(args.parent_pkg)
    with tempfile.TemporaryDirectory() as tmp:
        runs = [run_child("parent", parent, args, tmp), run_child("new", PKG, args, tmp),
                run_child("parent_again", parent, args, tmp)]
    res = {"tool": "tools/res_bench.py", "device": runs[0]["device"], "eps": EPS, "density": 0.67, "plan": "packed",
           "xtype": "bf16", "ytype": "bf16", "graph_steps": runs[0]["points"][0]["A_parent"]["graph_steps"],
           "timing": "HIP events around windows of replays of a captured graph of graph_steps steps; median per step of "
                     "--reps windows; one child process per library, in the order parent, new, parent_again",
           "legs": {"A": "parent: sgemm_q8_norm with col_scale into a bf16 y, then torch h.add_(y) (two roundings)",
                    "A1": "parent: sgemm_q8_norm with col_scale into an fp32 y, then torch y.add_(h), h.copy_(y) (the "
                          "bytes of B)",
                    "B": "new: sgemm_q8_norm with col_scale and residual=h into h (tcsc_gpu_sgemm_q8_res, in place)",
                    "old": "sgemm_q8_norm with col_scale into a bf16 y, no residual: parent, new, parent again"},
           "points": []}
    for a, b, c in zip(*(r["points"] for r in runs)):
        key = lambda p: (p["K"], p["N"], p["M"])
        assert key(a) == key(b) == key(c)
        assert a["sha256"] == b["sha256"] and a["scale_sha256"] == b["scale_sha256"], \
            f"legs A' and B differ at K={a['K']} N={a['N']} M={a['M']}"
        p = {"K": a["K"], "N": a["N"], "M": a["M"], "route": b["route"], "A_parent": a["A_parent"],
             "A1_parent": a["A1_parent"], "B_new": b["B_new"], "A_parent_again": c["A_parent_again"],
             "old_parent": a["old_parent"], "old_new": b["old_new"], "old_parent_again": c["old_parent_again"],
             "bits_equal_A1_B": True}
        a0, a1, bn = p["A_parent"]["graph_ms"], p["A_parent_again"]["graph_ms"], p["B_new"]["graph_ms"]
        p["spread"] = abs(a1 - a0) / a0
        p["A_over_B"] = 0.5 * (a0 + a1) / bn
        p["A1_over_B"] = p["A1_parent"]["graph_ms"] / bn
        p["B_wins_beyond_spread"] = bool(bn < min(a0, a1) * (1.0 - p["spread"]))
        p["B_loses_beyond_spread"] = bool(bn > max(a0, a1) * (1.0 + p["spread"]))
        o0, o1, on = p["old_parent"]["graph_ms"], p["old_parent_again"]["graph_ms"], p["old_new"]["graph_ms"]
        p["old_spread"] = abs(o1 - o0) / o0
        p["old_new_over_parent"] = on / (0.5 * (o0 + o1))
        p["old_within_spread"] = bool(min(o0, o1) * (1.0 - p["old_spread"]) <= on <= max(o0, o1) * (1.0 + p["old_spread"]))
        res["points"].append(p)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    for p in res["points"]:
        verdict = "wins" if p["B_wins_beyond_spread"] else "LOSES" if p["B_loses_beyond_spread"] else "level"
        print(f"K={p['K']} N={p['N']} M={p['M']:4d} {p['route'][0]:6s} fused={int(p['route'][2])} | us/step: (A) parent "
              f"{1e3 * p['A_parent']['graph_ms']:8.2f} again {1e3 * p['A_parent_again']['graph_ms']:8.2f} (A') "
              f"{1e3 * p['A1_parent']['graph_ms']:8.2f} | (B) {1e3 * p['B_new']['graph_ms']:8.2f} | spread "
              f"{100 * p['spread']:4.1f}% A/B x{p['A_over_B']:.2f} A'/B x{p['A1_over_B']:.2f} {verdict} | old: parent "
              f"{1e3 * p['old_parent']['graph_ms']:8.2f} new {1e3 * p['old_new']['graph_ms']:8.2f} again "
              f"{1e3 * p['old_parent_again']['graph_ms']:8.2f} spread {100 * p['old_spread']:4.1f}% "
              f"{'within' if p['old_within_spread'] else 'OUTSIDE'}")


if __name__ == "__main__":
    main()
