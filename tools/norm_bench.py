#!/usr/bin/env python3
"""Times the RMSNorm in the int8 call (tcsc_gpu_sgemm_q8_norm) against what a caller runs without it.

tools/q8_bench.py's method and its plans: HIP events around windows of replays of a captured graph of GRAPH_STEPS
layer steps after a warm-up, median per step of --reps windows.  A layer step is one activation tensor X (M x K,
fp32 or bf16) and a norm weight in, Y out, on a packed plan of a random ternary W of density 0.67.

Three columns per point (shape, M, x type), from three child processes, one library each:

  (i)   torch_parent  the parent commit's library and Python package (--parent-pkg) behind
                      torch.nn.functional.rms_norm: rms_norm(x, weight, eps) with a weight of x's type, so that
                      torch runs its fused kernel, then Plan.sgemm_q8 -- what a user writes today
  (ii)  two_launch    this tree's library, $TCSC_QFUSE=0: sgemm_q8_norm as the norm form of the quantizer, then the
                      int8 call (three launches where k_pack8 runs)
  (iii) fused         $TCSC_QFUSE=1: one launch of the norm form of k_decode8q, where the int8 route is decode
  and   two_launch_again / fused_again: (ii) and (iii) once more in a third process after the parent's windows --
        the run's own spread.

`all_bits_equal`: Y and the scales of (ii) and (iii) are the same bits at every point where both exist.  `pays` is
what tcsc_gpu_norm_fuse_pays says; `rule_holds` that wherever it says 1, (iii) is no slower than (ii) beyond the
point's spread.  The old entry point beside them: Plan.sgemm_q8 of the raw x under the default rule, on this
tree's library and on the parent's (`q8`, `q8_parent`, `q8_again`).

One JSON document goes to --out (default profiles/norm_bench.json) and a summary table to stdout.  Needs a gfx950 GPU.

A parent that has sgemm_q8_norm itself (an A/B across a later change) is also timed on (ii) and (iii):
`two_launch_parent`, `fused_parent`, and per point this tree's time over them and whether it is within this tree's
own spread.

    python tools/norm_bench.py --parent-pkg DIR [--reps 5] [--shapes KxN ...] [--out FILE]
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "sparse-matrix-multiplication-benchmark_amd")
sys.path.insert(0, os.path.join(ROOT, "tools"))

A = 0.2
EPS = 1e-6
SHAPES = [(4096, 4096), (8192, 8192), (2560, 6912), (6912, 2560)]  # K x N
MS = (1, 2, 4, 8, 16, 64, 2048)
XTYPES = ("f32", "bf16")
GRAPH_STEPS = 20
KNOBS = ("TCSC_PATH", "TCSC_SMALL_M", "TCSC_SLICES", "TCSC_MFMA_WGS", "TCSC_DECODE", "TCSC_QFUSE", "TCSC_W2GEMM")


def graph_time(torch, timed, step, reps):
    """Per-step time of `step(stream)` in a replayed graph of GRAPH_STEPS steps."""
    step(torch.cuda.current_stream().cuda_stream)  # warm: code objects, the allocator's pool
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
            "graph_ms_max": t["ms_max"] / GRAPH_STEPS, "iters": t["iters"], "reps": reps}


def child(mode, shapes, reps, out_path):
    """One library, every point.  mode: new, parent, new_again.  The package on sys.path and $TCSC_AMD_LIB were
    chosen by the process that started this one."""
    import tcsc_amd
    import torch
    from bf16_bench import timed
    from q8_bench import make_plan

    import q8_bench

    q8_bench.MS = MS  # make_plan reserves for the largest M
    tcsc_amd.require_gpu()
    for k in KNOBS:
        os.environ.pop(k, None)
    dev = torch.device("cuda:0")
    res = {"mode": mode, "lib": tcsc_amd.LIB_PATH, "device": torch.cuda.get_device_name(0), "points": []}
    for K, N in shapes:
        plan = make_plan(torch, tcsc_amd, K, N, 1000 + K + N)
        g = torch.Generator(device=dev)
        g.manual_seed(7 + K)
        gamma = torch.randn(K, device=dev, generator=g)
        for M in MS:
            g.manual_seed(100 + M)
            Xf = torch.randn((M, K), device=dev, generator=g)
            B = torch.rand(N, device=dev, generator=g) - 0.5
            Y = torch.empty((M, N), device=dev)
            Xq = torch.empty((M, K), dtype=torch.int8, device=dev)
            S = torch.empty(M, device=dev)
            for xt in XTYPES:
                X = Xf if xt == "f32" else Xf.to(torch.bfloat16)
                p = {"K": K, "N": N, "M": M, "xtype": xt, "route": plan.launch_info_i8(M)[0]}

                def q8(st, X=X):
                    plan.sgemm_q8(X, Xq, S, B, Y, M, N, "prelu_basic", A, st)

                if mode == "parent":
                    assert not os.path.realpath(tcsc_amd.LIB_PATH).startswith(os.path.realpath(PKG) + os.sep), \
                        "the parent package is this tree's"
                    if hasattr(tcsc_amd.Plan, "sgemm_q8_norm"):  # a parent that has the call: its two forms as well
                        for name, knob in (("two_launch_parent", "0"), ("fused_parent", "1")):
                            os.environ["TCSC_QFUSE"] = knob
                            if knob == "0" or plan.launch_info_q8_norm(M, xt)[0] == "decode":
                                p[name] = graph_time(torch, timed, lambda st, X=X: plan.sgemm_q8_norm(
                                    X, Xq, S, B, Y, M, N, gamma, EPS, "prelu_basic", A, st), reps)
                        os.environ.pop("TCSC_QFUSE", None)

                    gw = gamma.to(X.dtype)  # a weight of x's type: torch's fused rms_norm asks for it

                    def step(st, X=X, gw=gw):  # st is torch's current stream: the norm goes on it too
                        xn = torch.nn.functional.rms_norm(X, (K,), gw, EPS)
                        plan.sgemm_q8(xn, Xq, S, B, Y, M, N, "prelu_basic", A, st)

                    p["torch_parent"] = graph_time(torch, timed, step, reps)
                    p["q8_parent"] = graph_time(torch, timed, q8, reps)
                else:
                    def step(st, X=X):
                        plan.sgemm_q8_norm(X, Xq, S, B, Y, M, N, gamma, EPS, "prelu_basic", A, st)

                    again = "_again" if mode == "new_again" else ""
                    p["pays"] = int(tcsc_amd.norm_fuse_pays(M, K, N, xt))
                    p["default"] = list(plan.launch_info_q8_norm(M, xt))
                    p["q8" + again] = graph_time(torch, timed, q8, reps)
                    outs = {}
                    for name, knob in (("two_launch", "0"), ("fused", "1")):
                        os.environ["TCSC_QFUSE"] = knob
                        info = plan.launch_info_q8_norm(M, xt)
                        if knob == "1" and info[0] != "decode":
                            continue  # no fused form off the decode route
                        assert info[2] is (knob == "1"), info
                        p[name + again] = graph_time(torch, timed, step, reps)
                        Y.fill_(float("nan"))
                        S.fill_(float("nan"))
                        step(torch.cuda.current_stream().cuda_stream)
                        torch.cuda.synchronize()
                        outs[name] = (Y.view(torch.int32).clone(), S.view(torch.int32).clone())
                    os.environ.pop("TCSC_QFUSE", None)
                    if "fused" in outs:
                        p["bits_equal"] = bool(torch.equal(outs["fused"][0], outs["two_launch"][0]) and
                                               torch.equal(outs["fused"][1], outs["two_launch"][1]))
                    assert not bool(torch.isnan(Y).any())
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "norm_bench.json"))
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
        runs = [run_child("new", PKG, args, tmp), run_child("parent", os.path.abspath(args.parent_pkg), args, tmp),
                run_child("new_again", PKG, args, tmp)]
    res = {"tool": "tools/norm_bench.py", "device": runs[0]["device"], "a": A, "eps": EPS, "variant": "prelu_basic",
           "density": 0.67, "plan": "packed", "graph_steps": GRAPH_STEPS,
           "timing": "HIP events around windows of replays of a captured graph of graph_steps steps; median per step "
                     "of --reps windows; one child process per library, in the order new, parent, new_again",
           "columns": {"torch_parent": "torch.nn.functional.rms_norm + Plan.sgemm_q8 on the parent commit's library",
                       "two_launch": "sgemm_q8_norm under TCSC_QFUSE=0", "fused": "sgemm_q8_norm under TCSC_QFUSE=1",
                       "q8": "Plan.sgemm_q8 of the raw x, default rule (the old entry point)"},
           "points": []}
    for a, b, c in zip(*(r["points"] for r in runs)):
        assert (a["K"], a["N"], a["M"], a["xtype"]) == (b["K"], b["N"], b["M"], b["xtype"]) == (c["K"], c["N"], c["M"], c["xtype"])
        p = dict(a, torch_parent=b["torch_parent"], q8_parent=b["q8_parent"], q8_again=c["q8_again"],
                 two_launch_again=c["two_launch_again"])
        t2, t2b, tp = p["two_launch"]["graph_ms"], p["two_launch_again"]["graph_ms"], p["torch_parent"]["graph_ms"]
        p["spread"] = abs(t2b - t2) / t2
        p["torch_parent_over_two_launch"] = tp / t2
        p["two_launch_wins"] = bool(min(t2, t2b) <= tp)
        p["q8_spread"] = abs(p["q8_again"]["graph_ms"] - p["q8"]["graph_ms"]) / p["q8"]["graph_ms"]
        p["q8_over_parent"] = p["q8"]["graph_ms"] / p["q8_parent"]["graph_ms"]
        p["q8_within_spread"] = bool(min(p["q8"]["graph_ms"], p["q8_again"]["graph_ms"])
                                     <= p["q8_parent"]["graph_ms"] * (1.0 + p["q8_spread"]))
        for name in ("two_launch", "fused"):  # against a parent that has the call, within this tree's own spread
            if name + "_parent" in b and name in p:
                p[name + "_parent"] = b[name + "_parent"]
                mine = min(p[name]["graph_ms"], c[name + "_again"]["graph_ms"])
                sp = abs(c[name + "_again"]["graph_ms"] - p[name]["graph_ms"]) / p[name]["graph_ms"]
                p[name + "_over_parent"] = p[name]["graph_ms"] / b[name + "_parent"]["graph_ms"]
                p[name + "_within_spread"] = bool(mine <= b[name + "_parent"]["graph_ms"] * (1.0 + sp))
        p["holds"] = True
        if "fused" in p:
            p["fused_again"] = c["fused_again"]
            tf, tfb = p["fused"]["graph_ms"], p["fused_again"]["graph_ms"]
            p["spread"] = max(p["spread"], abs(tfb - tf) / tf)
            p["two_launch_over_fused"] = t2 / tf
            p["fused_wins"] = bool(min(tf, tfb) <= min(t2, t2b) * (1.0 + p["spread"]))
            p["fused_loses"] = bool(min(tf, tfb) > max(t2, t2b) * (1.0 + p["spread"]))
            p["holds"] = bool(not p["pays"] or p["fused_wins"])
        else:
            assert not p["pays"]
        res["points"].append(p)
    res["rule_holds"] = all(p["holds"] for p in res["points"])
    res["all_bits_equal"] = all(p["bits_equal"] for p in res["points"] if "bits_equal" in p)
    res["two_launch_wins_everywhere"] = all(p["two_launch_wins"] for p in res["points"])
    res["q8_within_spread_everywhere"] = all(p["q8_within_spread"] for p in res["points"])
    for name in ("two_launch", "fused"):
        pts = [p for p in res["points"] if name + "_within_spread" in p]
        if pts:
            res[name + "_within_spread_everywhere"] = all(p[name + "_within_spread"] for p in pts)
            print(name, "over parent: max", max(p[name + "_over_parent"] for p in pts), "within spread everywhere",
                  res[name + "_within_spread_everywhere"])
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    for p in res["points"]:
        fused = (f"fused {1e3 * p['fused']['graph_ms']:7.2f} (again {1e3 * p['fused_again']['graph_ms']:7.2f}) "
                 f"x{p['two_launch_over_fused']:.2f} wins={int(p['fused_wins'])} bits={int(p['bits_equal'])}"
                 if "fused" in p else "fused       -")
        print(f"{p['K']}x{p['N']} M={p['M']:4d} {p['xtype']:4s} {p['route']:6s} pays={p['pays']} | us/step: torch+parent "
              f"{1e3 * p['torch_parent']['graph_ms']:8.2f} two_launch {1e3 * p['two_launch']['graph_ms']:8.2f} (again "
              f"{1e3 * p['two_launch_again']['graph_ms']:8.2f}) x{p['torch_parent_over_two_launch']:.2f} | {fused} | q8 "
              f"{1e3 * p['q8']['graph_ms']:7.2f} parent {1e3 * p['q8_parent']['graph_ms']:7.2f} "
              f"x{p['q8_over_parent']:.3f} | spread {p['spread']:.3f} holds={p['holds']}")
    print("rule_holds", res["rule_holds"], "all_bits_equal", res["all_bits_equal"], "two_launch_wins_everywhere",
          res["two_launch_wins_everywhere"], "q8_within_spread_everywhere", res["q8_within_spread_everywhere"])


if __name__ == "__main__":
    main()
