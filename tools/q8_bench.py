#!/usr/bin/env python3
"""Times tcsc_gpu_sgemm_q8 (the quantizer fused into the int8 decode call, k_decode8q) against what
a caller ran before it existed: the parent commit's library.

tools/decode_bench.py's method: HIP events around windows of back-to-back calls after a warm-up, median of --reps
windows, each point timed as eager calls (`ms`, bounded by the host's enqueue rate for launches this short) and as
replays of a captured graph of GRAPH_STEPS layer steps (`graph_ms`, per step: how a decode loop runs).  A layer step
is one activation tensor X (M x K, fp32 or bf16) in and Y out on a packed plan of a random ternary W of density
0.67, with the same X, bias and Y at every step.

Three child processes, one library each, every point in each:

  fused         this tree's library, $TCSC_QFUSE=1: sgemm_q8 as one launch (k_decode8q);
                beside it `unfused`: the same call under $TCSC_QFUSE=0 (k_quant_rows_i8, then k_decode8) -- the
                cross-check of the baseline on the new library
  parent        the parent commit's library and Python package (--parent-pkg: a build of the parent commit, its
                `tcsc_amd/` and `lib/`; $TCSC_AMD_LIB names its library): quantize_rows_i8 + sgemm_i8, and for
                bf16 x a widening copy into an fp32 buffer first, since that quantizer takes fp32 only
  fused_again   the first once more, after the parent's windows: the run's own spread

`pays` is what tcsc_gpu_quant_fuse_pays says.  Where it says 1 the acceptance is fused <= parent within the point's
own spread (first against third measurement), on both timings: `holds`, and `all_hold` over the table.  Where it
says 0 the table still shows what the fused call would cost (`graph_parent_over_fused` below 1: it loses).

One JSON document goes to --out (default profiles/q8_bench.json) and a summary table to stdout.  Needs a gfx950 GPU.

    python tools/q8_bench.py --parent-pkg DIR [--reps 5] [--shapes KxN ...] [--out FILE]
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
SHAPES = [(8192, 8192), (4096, 4096), (2560, 6912), (6912, 2560)]  # K x N
MS = (1, 2, 4, 8, 16)
XTYPES = ("f32", "bf16")
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


def time_step(torch, timed, step, reps):
    """Eager and graph-replayed time of one layer step: step(stream) enqueues it."""
    out = dict(timed(torch, lambda: step(torch.cuda.current_stream().cuda_stream), reps))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        for _ in range(GRAPH_STEPS):
            step(torch.cuda.current_stream().cuda_stream)
    t = timed(torch, graph.replay, reps)
    out.update(graph_ms=t["ms"] / GRAPH_STEPS, graph_ms_min=t["ms_min"] / GRAPH_STEPS,
               graph_ms_max=t["ms_max"] / GRAPH_STEPS, graph_steps=GRAPH_STEPS)
    del graph
    return out


def child(mode, shapes, reps, out_path):
    """One library, every point.  mode: fused (with unfused beside it), fused_again, parent.  The package on sys.path
    and $TCSC_AMD_LIB were chosen by the process that started this one."""
    import tcsc_amd
    import torch

    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from bf16_bench import timed

    tcsc_amd.require_gpu()
    for k in KNOBS:
        os.environ.pop(k, None)
    dev = torch.device("cuda:0")
    res = {"mode": mode, "lib": tcsc_amd.LIB_PATH, "device": torch.cuda.get_device_name(0), "points": []}
    for K, N in shapes:
        plan = make_plan(torch, tcsc_amd, K, N, 1000 + K + N)
        for M in MS:
            g = torch.Generator(device=dev)
            g.manual_seed(100 + M)
            Xf = torch.randn((M, K), device=dev, generator=g)
            B = torch.rand(N, device=dev, generator=g) - 0.5
            Y = torch.empty((M, N), device=dev)
            Xq = torch.empty((M, K), dtype=torch.int8, device=dev)
            S = torch.empty(M, device=dev)
            for xt in XTYPES:
                X = Xf if xt == "f32" else Xf.to(torch.bfloat16)
                wide = torch.empty((M, K), device=dev)  # the parent's fp32 copy of a bf16 X
                p = {"K": K, "N": N, "M": M, "xtype": xt}
                if mode == "parent":
                    assert not hasattr(tcsc_amd.Plan, "sgemm_q8"), "the parent package is this tree's"

                    def step(st, X=X, xt=xt):
                        src = X
                        if xt == "bf16":  # st is torch's current stream: the copy goes on it too
                            wide.copy_(X)
                            src = wide
                        tcsc_amd.quantize_rows_i8(src, Xq, S, M, K, st)
                        plan.sgemm_i8(Xq, S, B, Y, M, N, "prelu_basic", A, st)

                    p["route"] = plan.launch_info_i8(M)[0]
                    p["parent"] = time_step(torch, timed, step, reps)
                else:
                    def step(st, X=X):
                        plan.sgemm_q8(X, Xq, S, B, Y, M, N, "prelu_basic", A, st)

                    os.environ.pop("TCSC_QFUSE", None)
                    p["pays"] = int(tcsc_amd.quant_fuse_pays(M, K, N, xt))
                    p["default"] = list(plan.launch_info_q8(M, xt))
                    for name, knob in (("fused", "1"), ("unfused", "0")) if mode == "fused" else (("fused_again", "1"),):
                        os.environ["TCSC_QFUSE"] = knob
                        assert plan.launch_info_q8(M, xt) == ("decode", 1, knob == "1"), plan.launch_info_q8(M, xt)
                        p[name] = time_step(torch, timed, step, reps)
                    os.environ.pop("TCSC_QFUSE", None)
                step(torch.cuda.current_stream().cuda_stream)
                torch.cuda.synchronize()
                p["y_sum_bits"] = int(Y.view(torch.int32).to(torch.int64).sum().item())  # the same Y from every library
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "q8_bench.json"))
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--child-out", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    args.shape_list = SHAPES if not args.shapes else [tuple(int(v) for v in s.lower().split("x")) for s in args.shapes]
    if args.child:
        child(args.child, args.shape_list, args.reps, args.child_out)
        return
    if not args.parent_pkg or not os.path.exists(os.path.join(args.parent_pkg, "lib", "libtcsc_amd.so")):
        raise SystemExit("--parent-pkg must name a build of the parent commit (tcsc_amd/ and lib/libtcsc_amd.so)")
    with tempfile.TemporaryDirectory() as tmp:
        runs = [run_child("fused", PKG, args, tmp), run_child("parent", os.path.abspath(args.parent_pkg), args, tmp),
                run_child("fused_again", PKG, args, tmp)]
    res = {"tool": "tools/q8_bench.py", "device": runs[0]["device"], "a": A, "variant": "prelu_basic", "density": 0.67,
           "plan": "packed", "graph_steps": GRAPH_STEPS,
           "timing": "HIP events around windows of back-to-back steps; median per step of --reps windows; one child "
                     "process per library, in the order fused, parent, fused_again",
           "parent": "quantize_rows_i8 + sgemm_i8 of the parent commit's library; bf16 x: a widening copy first",
           "points": []}
    for a, b, c in zip(*(r["points"] for r in runs)):
        assert (a["K"], a["N"], a["M"], a["xtype"]) == (b["K"], b["N"], b["M"], b["xtype"]) == (c["K"], c["N"], c["M"], c["xtype"])
        p = dict(a, parent=b["parent"], parent_route=b["route"], fused_again=c["fused_again"])
        p["bits_equal_parent"] = a["y_sum_bits"] == b["y_sum_bits"] == c["y_sum_bits"]
        del p["y_sum_bits"]
        p["holds"] = True
        for key, tag in (("ms", "eager"), ("graph_ms", "graph")):
            f1, par, f3, unf = p["fused"][key], p["parent"][key], p["fused_again"][key], p["unfused"][key]
            p[tag + "_parent_over_fused"] = par / f1
            p[tag + "_unfused_over_fused"] = unf / f1
            p[tag + "_spread"] = abs(f3 - f1) / f1
            p[tag + "_fused_wins"] = bool(min(f1, f3) <= par * (1.0 + p[tag + "_spread"]))
            if p["pays"] and not p[tag + "_fused_wins"]:
                p["holds"] = False
        res["points"].append(p)
    res["all_hold"] = all(p["holds"] for p in res["points"])
    res["all_bits_equal"] = all(p["bits_equal_parent"] for p in res["points"])
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    for p in res["points"]:
        print(f"{p['K']}x{p['N']} M={p['M']:2d} {p['xtype']:4s} pays={p['pays']} | graph us: fused "
              f"{1e3 * p['fused']['graph_ms']:6.2f} (again {1e3 * p['fused_again']['graph_ms']:6.2f}) parent "
              f"{1e3 * p['parent']['graph_ms']:6.2f} x{p['graph_parent_over_fused']:.2f} unfused "
              f"{1e3 * p['unfused']['graph_ms']:6.2f} | eager us: fused {1e3 * p['fused']['ms']:6.2f} parent "
              f"{1e3 * p['parent']['ms']:6.2f} x{p['eager_parent_over_fused']:.2f} | wins graph "
              f"{int(p['graph_fused_wins'])} eager {int(p['eager_fused_wins'])} holds={p['holds']} "
              f"bits={int(p['bits_equal_parent'])}")
    print("all_hold", res["all_hold"], "all_bits_equal", res["all_bits_equal"])


if __name__ == "__main__":
    main()
