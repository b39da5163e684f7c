#!/usr/bin/env python3
"""Times the gate/up half of a BitNet-style FFN -- subnorm in front, Y = relu(X Wg)^2 * (X Wu) as bf16 -- as the one
gated call (tcsc_gpu_sgemm_q8_glu) against what a caller wrote before it existed.

tools/out_bench.py's protocol: HIP events around windows of replays of a captured graph of GRAPH_STEPS steps after a
warm-up, median per step of --reps windows.  A step is one bf16 X (M x K) in and one bf16 Y (M x H) out on two packed
plans of random ternary K x H matrices of density 0.67, with per-column weight scales and biases on both halves.

Two legs, which give the same bf16 Y (asserted: the SHA-256 of Y's bytes):

  (A) the parent commit's library doing what a caller writes today: quantize_rows_i8_norm, two sgemm_i8 calls into
      fp32 tensors, then torch relu, square, mul and the copy into a bf16 tensor (`A_parent`, and once more after
      everything else, `A_parent_again`: the run's own spread)
  (B) the one new call on this tree's library (`B_new`)

Three child processes, one library each, every point in each, in the order parent, new, parent_again.  The parent is
--parent-pkg: a build of the parent commit (its `tcsc_amd/` and `lib/`; $TCSC_AMD_LIB names its library).

Per point: spread = |A_parent_again - A_parent| / A_parent and `A_over_B`, the ratio of the parent's median to (B).
One JSON document goes to --out (default profiles/glu_bench.json) and a table to stdout.  Needs a gfx950 GPU.

    python tools/glu_bench.py --parent-pkg DIR [--reps 5] [--shapes KxH ...] [--ms M ...] [--out FILE]
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

SHAPES = [(2560, 6912), (4096, 4096), (8192, 8192)]  # K x H
MS = (1, 2, 4, 8, 16, 64, 2048)
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
    for K, H in shapes:
        gate, up = make_plan(torch, tcsc_amd, K, H, 1000 + K + H), make_plan(torch, tcsc_amd, K, H, 2000 + K + H)
        gate.reserve(max(ms))
        up.reserve(max(ms))
        for M in ms:
            g = torch.Generator(device=dev)
            g.manual_seed(100 + M)
            X = torch.randn((M, K), device=dev, generator=g).to(torch.bfloat16)
            gamma = torch.rand(K, device=dev, generator=g) + 0.5
            bg = torch.rand(H, device=dev, generator=g) - 0.5
            bu = torch.rand(H, device=dev, generator=g) - 0.5
            cg = torch.rand(H, device=dev, generator=g) * 0.04 + 0.01  # per-column beta of an absmean rule
            cu = torch.rand(H, device=dev, generator=g) * 0.04 + 0.01
            G = torch.empty((M, H), device=dev)
            U = torch.empty((M, H), device=dev)
            Yb = torch.empty((M, H), dtype=torch.bfloat16, device=dev)
            Xq = torch.empty((M, K), dtype=torch.int8, device=dev)
            S = torch.empty(M, device=dev)
            p = {"K": K, "H": H, "M": M}

            def leg_a(st):  # st is torch's current stream: the torch launches go on it too
                tcsc_amd.quantize_rows_i8_norm(X, Xq, S, M, K, gamma, EPS, st)
                gate.sgemm_i8(Xq, S, bg, G, M, H, "basic", 0.0, st, col_scale=cg)
                up.sgemm_i8(Xq, S, bu, U, M, H, "basic", 0.0, st, col_scale=cu)
                torch.relu_(G)
                torch.square(G, out=G)
                G.mul_(U)
                Yb.copy_(G)

            def leg_b(st):
                tcsc_amd.sgemm_q8_glu(gate, up, X, Xq, S, bg, bu, Yb, M, H, "relu2", cg, cu, gamma, EPS, G, st)

            leg = leg_b if mode == "new" else leg_a
            if mode == "new":
                path, slices, _ = tcsc_amd.launch_info_glu(gate, up, M, "bf16")
                # fused: of this call, which has the norm ($TCSC_QFUSE is unset here)
                p["route"] = [path, slices, path == "decode" and tcsc_amd.glu_fuse_pays(M, K, H, "bf16", norm=True)]
            p[("B_" if mode == "new" else "A_") + mode] = time_graph(torch, timed, leg, reps)
            Yb.zero_()
            leg(torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
            p["yb_sha256"] = hashlib.sha256(Yb.view(torch.int16).cpu().numpy().tobytes()).hexdigest()
            res["points"].append(p)
        gate.destroy()
        up.destroy()
        torch.cuda.empty_cache()
        print(f"[{mode}] {K}x{H} done", file=sys.stderr, flush=True)
    with open(out_path, "w") as f:
        json.dump(res, f)


def run_child(mode, pkg, args, tmp):
    out = os.path.join(tmp, mode + ".json")
    env = dict(os.environ, PYTHONPATH=pkg + os.pathsep + os.environ.get("PYTHONPATH", ""),
               TCSC_AMD_LIB=os.path.join(pkg, "lib", "libtcsc_amd.so"))
    cmd = [sys.executable, os.path.abspath(__file__), "--child", mode, "--child-out", out, "--reps", str(args.reps),
           "--ms"] + [str(m) for m in args.ms] + ["--shapes"] + [f"{k}x{h}" for k, h in args.shape_list]
    subprocess.run(cmd, env=env, check=True, timeout=900)
    with open(out) as f:
        return json.load(f)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--parent-pkg", help="a build of the parent commit: the directory holding its tcsc_amd/ and lib/")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--shapes", nargs="+", default=None, metavar="KxH")
    ap.add_argument("--ms", nargs="+", type=int, default=list(MS))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "glu_bench.json"))
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
    res = {"tool": "tools/glu_bench.py", "device": runs[0]["device"], "act": "relu2", "eps": EPS, "density": 0.67,
           "plan": "packed", "xtype": "bf16", "ytype": "bf16", "graph_steps": runs[0]["points"][0]["A_parent"]["graph_steps"],
           "timing": "HIP events around windows of replays of a captured graph of graph_steps steps; median per step of "
                     "--reps windows; one child process per library, in the order parent, new, parent_again",
           "legs": {"A": "parent: quantize_rows_i8_norm, sgemm_i8 twice into fp32 (column scales, biases), then torch "
                         "relu_, square, mul_ and the copy into bf16",
                    "B": "new: sgemm_q8_glu with the norm, relu2 and a bf16 Y"},
           "points": []}
    for a, b, c in zip(*(r["points"] for r in runs)):
        assert (a["K"], a["H"], a["M"]) == (b["K"], b["H"], b["M"]) == (c["K"], c["H"], c["M"])
        assert a["yb_sha256"] == b["yb_sha256"] == c["yb_sha256"], f"legs A and B differ at {a['K']}x{a['H']} M={a['M']}"
        p = {"K": a["K"], "H": a["H"], "M": a["M"], "route": b["route"], "A_parent": a["A_parent"], "B_new": b["B_new"],
             "A_parent_again": c["A_parent_again"], "bits_equal": True}
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
        print(f"{p['K']}x{p['H']} M={p['M']:4d} {p['route'][0]:6s} fused={int(p['route'][2])} | us/step: (A) parent "
              f"{1e3 * p['A_parent']['graph_ms']:8.2f} again {1e3 * p['A_parent_again']['graph_ms']:8.2f} | (B) "
              f"{1e3 * p['B_new']['graph_ms']:8.2f} | spread {100 * p['spread']:4.1f}% A/B x{p['A_over_B']:.2f} {verdict}")


if __name__ == "__main__":
    main()
