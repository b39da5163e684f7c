#!/usr/bin/env python3
"""Times a complete ternary linear layer step -- column weight scales, bias, PReLU and a bf16 Y -- in the epilogue
of the int8 call (tcsc_gpu_sgemm_q8_out) against what a caller ran before it existed.

tools/q8_bench.py's method: HIP events around windows of replays of a captured graph of GRAPH_STEPS layer steps
after a warm-up, median per step of --reps windows.  A layer step is one bf16 activation tensor X (M x K) in and Y
out on a packed plan of a random ternary W of density 0.67, with the same X, scales, bias and Y at every step.

Three legs:

  (i)   sgemm_q8 as it was: fp32 Y, no column scale -- what the call costs without the feature; on the parent
        commit's library (`i_parent`, and once more after everything else, `i_parent_again`: the run's own
        spread of this leg) and on this tree's (`i_new`: the old entry point must not pay for the feature)
  (ii)  the composition a caller wrote on the parent's library: sgemm_q8 with a zero bias, then torch's y.mul_(c),
        y.add_(b), leaky_relu_ and a conversion into a bf16 tensor -- five launches, three more passes over an
        fp32 Y (`ii_parent`)
  (iii) sgemm_q8 with col_scale, the bias, the PReLU and a bf16 Y: this tree's library, the launches of (i) (`iii_new`)

Three child processes, one library each, every point in each, in the order parent, new, parent_again.  The parent
is --parent-pkg: a build of the parent commit (its `tcsc_amd/` and `lib/`; $TCSC_AMD_LIB names its library).  It may
have the feature itself (an A/B of the old entry point across a later change): legs (i) and (ii) run on any library.

Per point: spread = |i_parent_again - i_parent| / i_parent;  `iii_no_slower` = iii_new <= i_parent (1 + spread);
`i_unchanged` = |i_new - i_parent| <= spread i_parent taken over both parent measurements;  `ii_over_iii`, the
headline ratio.  The Y of (ii) and (iii) are compared as sums of bits where the arithmetic agrees (`bits_equal`:
(ii) multiplies and adds in the same order, so only a -0.0 product can differ, which the sum of bits shows).

One JSON document goes to --out (default profiles/out_bench.json) and a summary table to stdout.  Needs a gfx950 GPU.

    python tools/out_bench.py --parent-pkg DIR [--reps 5] [--shapes KxN ...] [--out FILE]
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "sparse-matrix-multiplication-benchmark_amd")

A = 0.2
SHAPES = [(4096, 4096), (8192, 8192), (2560, 6912), (6912, 2560)]  # K x N
MS = (1, 4, 16, 64, 2048)
GRAPH_STEPS = 20
KNOBS = ("TCSC_PATH", "TCSC_SMALL_M", "TCSC_SLICES", "TCSC_MFMA_WGS", "TCSC_DECODE", "TCSC_QFUSE", "TCSC_W2GEMM")


def make_plan(torch, tcsc_amd, K, N, seed):
    """A packed plan of a random ternary K x N W of density 0.67, built on the device."""
    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream().cuda_stream
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    u = torch.rand((K, N), device=dev, generator=g)
    Wd = torch.zeros((K, N), device=dev)
    Wd[u < 0.335] = 1.0
    Wd[(u >= 0.335) & (u < 0.67)] = -1.0
    del u
    csp = torch.empty(N + 1, dtype=torch.int32, device=dev)
    csn = torch.empty(N + 1, dtype=torch.int32, device=dev)
    n_pos, n_neg = tcsc_amd.gpu_from_dense(Wd, K, N, csp, csn, stream=stream)
    rip = torch.empty(max(n_pos, 1), dtype=torch.int32, device=dev)
    rin = torch.empty(max(n_neg, 1), dtype=torch.int32, device=dev)
    tcsc_amd.gpu_from_dense(Wd, K, N, csp, csn, rip, rin, stream=stream)
    del Wd
    plan = tcsc_amd.Plan.packed_from_device(K, N, csp, csn, rip, rin, stream=stream)
    plan.reserve(max(MS))
    return plan


def time_graph(torch, timed, step, reps):
    """Per-step time of a replayed graph of GRAPH_STEPS steps: step(stream) enqueues one."""
    step(torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        for _ in range(GRAPH_STEPS):
            step(torch.cuda.current_stream().cuda_stream)
    t = timed(torch, graph.replay, reps)
    del graph
    return {"graph_ms": t["ms"] / GRAPH_STEPS, "graph_ms_min": t["ms_min"] / GRAPH_STEPS,
            "graph_ms_max": t["ms_max"] / GRAPH_STEPS, "graph_steps": GRAPH_STEPS, "reps": t["reps"], "iters": t["iters"]}


def child(mode, shapes, reps, out_path):
    """One library, every point.  mode: parent (legs i and ii), parent_again (leg i), new (legs i and iii).  The
    package on sys.path and $TCSC_AMD_LIB were chosen by the process that started this one."""
    import tcsc_amd
    import torch

    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from bf16_bench import timed

    tcsc_amd.require_gpu()
    for k in KNOBS:
        os.environ.pop(k, None)
    # the parent may have the feature too (a later A/B of the old entry point): then it is told apart by its path
    is_new = os.path.realpath(tcsc_amd.LIB_PATH).startswith(os.path.realpath(PKG) + os.sep)
    assert is_new == (mode == "new"), f"mode {mode} on the wrong library ({tcsc_amd.LIB_PATH})"
    assert not is_new or "tcsc_gpu_sgemm_q8_out" in tcsc_amd.EXPORTED_SYMBOLS
    dev = torch.device("cuda:0")
    res = {"mode": mode, "lib": tcsc_amd.LIB_PATH, "device": torch.cuda.get_device_name(0), "points": []}
    for K, N in shapes:
        plan = make_plan(torch, tcsc_amd, K, N, 1000 + K + N)
        for M in MS:
            g = torch.Generator(device=dev)
            g.manual_seed(100 + M)
            X = torch.randn((M, K), device=dev, generator=g).to(torch.bfloat16)
            B = torch.rand(N, device=dev, generator=g) - 0.5
            Cs = torch.rand(N, device=dev, generator=g) * 0.04 + 0.01  # per-column beta of an absmean rule
            zero = torch.zeros(N, device=dev)
            Y = torch.empty((M, N), device=dev)
            Yb = torch.empty((M, N), dtype=torch.bfloat16, device=dev)
            Xq = torch.empty((M, K), dtype=torch.int8, device=dev)
            S = torch.empty(M, device=dev)
            p = {"K": K, "N": N, "M": M, "route": list(plan.launch_info_q8(M, "bf16"))}

            def leg_i(st):
                plan.sgemm_q8(X, Xq, S, B, Y, M, N, "prelu_basic", A, st)

            def leg_ii(st):  # st is torch's current stream: the torch launches go on it too
                plan.sgemm_q8(X, Xq, S, zero, Y, M, N, "basic", 0.0, st)
                Y.mul_(Cs)
                Y.add_(B)
                torch.nn.functional.leaky_relu_(Y, A)
                Yb.copy_(Y)

            def leg_iii(st):
                plan.sgemm_q8(X, Xq, S, B, Yb, M, N, "prelu_basic", A, st, col_scale=Cs)

            if mode == "new":
                p["i_new"] = time_graph(torch, timed, leg_i, reps)
                p["iii_new"] = time_graph(torch, timed, leg_iii, reps)
                last = leg_iii
            else:
                p["i_" + mode] = time_graph(torch, timed, leg_i, reps)
                if mode == "parent":
                    p["ii_parent"] = time_graph(torch, timed, leg_ii, reps)
                last = leg_ii
            Yb.zero_()
            last(torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
            p["yb_sum_bits"] = int(Yb.view(torch.int16).to(torch.int64).sum().item())
            res["points"].append(p)
        plan.destroy()
        torch.cuda.empty_cache()
        print(f"[{mode}] {K}x{N} done", file=sys.stderr, flush=True)
    with open(out_path, "w") as f:
        json.dump(res, f)


def run_child(mode, pkg, args, tmp):
    out = os.path.join(tmp, mode + ".json")
    env = dict(os.environ, PYTHONPATH=pkg + os.pathsep + os.environ.get("PYTHONPATH", ""),
               TCSC_AMD_LIB=os.path.join(pkg, "lib", "libtcsc_amd.so"))
    cmd = [sys.executable, os.path.abspath(__file__), "--child", mode, "--child-out", out, "--reps", str(args.reps),
           "--shapes"] + [f"{k}x{n}" for k, n in args.shape_list]
    subprocess.run(cmd, env=env, check=True, timeout=900)
    with open(out) as f:
        return json.load(f)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--parent-pkg", help="a build of the parent commit: the directory holding its tcsc_amd/ and lib/")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--shapes", nargs="+", default=None, metavar="KxN")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "out_bench.json"))
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--child-out", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    args.shape_list = SHAPES if not args.shapes else [tuple(int(v) for v in s.lower().split("x")) for s in args.shapes]
    if args.child:
        child(args.child, args.shape_list, args.reps, args.child_out)
        return
    if not args.parent_pkg or not os.path.exists(os.path.join(args.parent_pkg, "lib", "libtcsc_amd.so")):
        raise SystemExit("--parent-pkg must name a build of the parent commit (tcsc_amd/ and lib/libtcsc_amd.so)")
    parent = os.path.abspath(args.parent_pkg)
    with tempfile.TemporaryDirectory() as tmp:
        runs = [run_child("parent", parent, args, tmp), run_child("new", PKG, args, tmp),
                run_child("parent_again", parent, args, tmp)]
    res = {"tool": "tools/out_bench.py", "device": runs[0]["device"], "a": A, "variant": "prelu_basic", "density": 0.67,
           "plan": "packed", "xtype": "bf16", "graph_steps": GRAPH_STEPS,
           "timing": "HIP events around windows of replays of a captured graph of graph_steps layer steps; median per "
                     "step of --reps windows; one child process per library, in the order parent, new, parent_again",
           "legs": {"i": "sgemm_q8, fp32 Y, no column scale (parent twice, new once)",
                    "ii": "parent: sgemm_q8 with a zero bias, then torch mul_(c), add_(b), leaky_relu_, copy into bf16",
                    "iii": "new: sgemm_q8 with col_scale, bias, PReLU and a bf16 Y"},
           "points": []}
    for a, b, c in zip(*(r["points"] for r in runs)):
        assert (a["K"], a["N"], a["M"]) == (b["K"], b["N"], b["M"]) == (c["K"], c["N"], c["M"])
        p = {"K": a["K"], "N": a["N"], "M": a["M"], "route": a["route"], "i_parent": a["i_parent"],
             "ii_parent": a["ii_parent"], "i_new": b["i_new"], "iii_new": b["iii_new"], "i_parent_again": c["i_parent_again"]}
        assert a["route"] == b["route"]
        i0, i1 = p["i_parent"]["graph_ms"], p["i_parent_again"]["graph_ms"]
        inew, ii, iii = p["i_new"]["graph_ms"], p["ii_parent"]["graph_ms"], p["iii_new"]["graph_ms"]
        p["spread"] = abs(i1 - i0) / i0
        p["iii_over_i_parent"] = iii / i0
        p["iii_no_slower"] = bool(iii <= max(i0, i1) * (1.0 + p["spread"]))
        p["i_new_over_i_parent"] = inew / i0
        p["i_unchanged"] = bool(min(i0, i1) * (1.0 - p["spread"]) <= inew <= max(i0, i1) * (1.0 + p["spread"]))
        p["ii_over_iii"] = ii / iii
        p["bits_equal"] = a["yb_sum_bits"] == b["yb_sum_bits"]
        res["points"].append(p)
    res["all_iii_no_slower"] = all(p["iii_no_slower"] for p in res["points"])
    res["all_i_unchanged"] = all(p["i_unchanged"] for p in res["points"])
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    for p in res["points"]:
        print(f"{p['K']}x{p['N']} M={p['M']:4d} {p['route'][0]:6s} | us/step: (i) parent {1e3 * p['i_parent']['graph_ms']:8.2f} "
              f"again {1e3 * p['i_parent_again']['graph_ms']:8.2f} new {1e3 * p['i_new']['graph_ms']:8.2f} | (ii) "
              f"{1e3 * p['ii_parent']['graph_ms']:8.2f} | (iii) {1e3 * p['iii_new']['graph_ms']:8.2f} | spread "
              f"{100 * p['spread']:4.1f}% iii/i {p['iii_over_i_parent']:.3f} ok={int(p['iii_no_slower'])} i_new/i "
              f"{p['i_new_over_i_parent']:.3f} ok={int(p['i_unchanged'])} ii/iii x{p['ii_over_iii']:.2f} "
              f"bits={int(p['bits_equal'])}")
    print("all_iii_no_slower", res["all_iii_no_slower"], "all_i_unchanged", res["all_i_unchanged"])


if __name__ == "__main__":
    main()
