#!/usr/bin/env python3
"""Times int8 calls of 16 .. 64 rows on packed plans: the row-tiled decode launch (k_decode8r)
against k_pack8 + k_gemm8w2, which is what the library runs above 16 rows by default.

tools/out_bench.py's method: HIP events around windows of replays of a captured graph of GRAPH_STEPS calls after a
warm-up, median per call of --reps windows.  Packed plans of a random ternary W of density 0.67; the same X, scales,
bias and Y at every step.  Three child processes, one library each, every point in each, in the order parent, new,
parent again; the parent is --parent-pkg, a build of the parent commit (its `tcsc_amd/` and `lib/`).

Per point (shape K x N, M rows), sgemm_i8 with row scales, bias and PReLU into an fp32 Y:

  A   the parent's call (twice: `A` and `A_again`, whose difference is the run's spread at the point)
  B   this tree's library with set_decode_rows(64)
  C   this tree's library at the default setting: the parent's route, which must not have moved

`b_wins`: B < min(A, A_again) by more than the spread;  `c_level`: C within the spread of the two A.  The bytes of Y
after A and after B are compared (sha256) and the run fails if any differ.

Two more tables say what a caller gets:
  `layer`     sgemm_q8_norm on bf16 x with a bf16 residual in place (a BitNet block's down projection with its skip
              connection: the quantizer's launch, then the int8 call) at 2560 x 2560 and 6912 x 2560
  `rotation`  the plain call at 8192 x 8192 over a rotation of 20 plans with the same W in 20 allocations, one per
              step of the graph, so that every step streams its image from HBM

`--table` prints the README's table from an existing JSON and needs no GPU.

    python tools/decode_rows_bench.py --parent-pkg DIR [--reps 5] [--out FILE]
    python tools/decode_rows_bench.py --table [--out FILE]
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

A = 0.2
SHAPES = [(2560, 2560), (2560, 6912), (6912, 2560), (4096, 4096), (8192, 8192)]  # K x N
MS = (16, 17, 24, 32, 33, 48, 64)
LAYER_SHAPES = [(2560, 2560), (6912, 2560)]
ROTATION_SHAPE = (8192, 8192)
GRAPH_STEPS = 20
EPS = 1e-5
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


def time_graph(torch, timed, steps, reps):
    """Per-step time of a replayed graph of GRAPH_STEPS steps: steps[i % len](stream) enqueues step i."""
    for s in steps:
        s(torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        for i in range(GRAPH_STEPS):
            steps[i % len(steps)](torch.cuda.current_stream().cuda_stream)
    t = timed(torch, graph.replay, reps)
    del graph
    return {"graph_ms": t["ms"] / GRAPH_STEPS, "graph_ms_min": t["ms_min"] / GRAPH_STEPS,
            "graph_ms_max": t["ms_max"] / GRAPH_STEPS, "graph_steps": GRAPH_STEPS, "reps": t["reps"], "iters": t["iters"]}


def sha(t):
    return hashlib.sha256(t.contiguous().cpu().numpy().tobytes()).hexdigest()


def child(mode, reps, out_path, shapes, ms):
    """One library, every point.  mode: parent / parent_again (leg A), new (legs B and C)."""
    import tcsc_amd
    import torch

    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from bf16_bench import timed

    tcsc_amd.require_gpu()
    for k in KNOBS:
        os.environ.pop(k, None)
    is_new = os.path.realpath(tcsc_amd.LIB_PATH).startswith(os.path.realpath(PKG) + os.sep)
    assert is_new == (mode == "new"), f"mode {mode} on the wrong library ({tcsc_amd.LIB_PATH})"
    dev = torch.device("cuda:0")
    legs = ("B", "C") if is_new else ("A",)
    res = {"mode": mode, "lib": tcsc_amd.LIB_PATH, "device": torch.cuda.get_device_name(0),
           "cus": torch.cuda.get_device_properties(0).multi_processor_count, "points": [], "layer": [], "rotation": []}

    def setting(plans, leg):
        if is_new:
            for p in plans:
                p.set_decode_rows(64 if leg == "B" else 16)

    def inputs(M, K, N):
        g = torch.Generator(device=dev)
        g.manual_seed(100 + M)
        Xq = torch.randint(-127, 128, (M, K), device=dev, generator=g, dtype=torch.int32).to(torch.int8)
        S = torch.rand(M, device=dev, generator=g) * 0.05 + 1e-3
        B = torch.rand(N, device=dev, generator=g) - 0.5
        return Xq, S, B

    for K, N in shapes:
        plan = make_plan(torch, tcsc_amd, K, N, 1000 + K + N)
        for M in ms:
            Xq, S, B = inputs(M, K, N)
            Y = torch.empty((M, N), device=dev)
            p = {"K": K, "N": N, "M": M}
            for leg in legs:
                setting([plan], leg)
                p[leg] = time_graph(torch, timed, [lambda st: plan.sgemm_i8(Xq, S, B, Y, M, N, "prelu_basic", A, st)], reps)
                p[leg]["route"] = list(plan.launch_info_i8(M))
                if is_new:
                    p[leg]["launch"] = list(plan.launch_info_decode(M))
                Y.fill_(float("nan"))
                plan.sgemm_i8(Xq, S, B, Y, M, N, "prelu_basic", A, torch.cuda.current_stream().cuda_stream)
                torch.cuda.synchronize()
                p[leg]["sha256"] = sha(Y)
            res["points"].append(p)
        if (K, N) in LAYER_SHAPES:  # the down projection with its skip connection
            for M in ms:
                g = torch.Generator(device=dev)
                g.manual_seed(300 + M)
                X = torch.randn((M, K), device=dev, generator=g).to(torch.bfloat16)
                gamma = torch.rand(K, device=dev, generator=g) + 0.5
                B = torch.rand(N, device=dev, generator=g) - 0.5
                Cs = torch.rand(N, device=dev, generator=g) * 0.04 + 0.01
                R = torch.randn((M, N), device=dev, generator=g).to(torch.bfloat16)
                Yb = R.clone()
                Xq = torch.empty((M, K), dtype=torch.int8, device=dev)
                S = torch.empty(M, device=dev)
                p = {"K": K, "N": N, "M": M}

                def step(st):
                    plan.sgemm_q8_norm(X, Xq, S, B, Yb, M, N, gamma, EPS, "basic", 0.0, st, col_scale=Cs, residual=Yb)

                for leg in legs:
                    setting([plan], leg)
                    p[leg] = time_graph(torch, timed, [step], reps)
                    p[leg]["route"] = list(plan.launch_info_q8_norm(M, "bf16"))
                    Yb.copy_(R)
                    step(torch.cuda.current_stream().cuda_stream)
                    torch.cuda.synchronize()
                    p[leg]["sha256"] = sha(Yb.view(torch.int16))
                res["layer"].append(p)
        if (K, N) == ROTATION_SHAPE:  # 20 plans, one per step of the graph: every image comes from HBM
            image = plan.w2_image(torch.cuda.current_stream().cuda_stream)
            ring = [plan] + [tcsc_amd.Plan.packed_from_image(image, K, N, 0, 0, torch.cuda.current_stream().cuda_stream)
                             for _ in range(GRAPH_STEPS - 1)]
            for q in ring[1:]:
                q.reserve(max(MS))
            for M in ms:
                Xq, S, B = inputs(M, K, N)
                Y = torch.empty((M, N), device=dev)
                p = {"K": K, "N": N, "M": M, "plans": len(ring)}
                for leg in legs:
                    setting(ring, leg)
                    steps = [(lambda st, q=q: q.sgemm_i8(Xq, S, B, Y, M, N, "prelu_basic", A, st)) for q in ring]
                    p[leg] = time_graph(torch, timed, steps, reps)
                res["rotation"].append(p)
            for q in ring[1:]:
                q.destroy()
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
           "--shapes"] + [f"{k}x{n}" for k, n in args.shape_list] + ["--ms"] + [str(m) for m in args.ms]
    subprocess.run(cmd, env=env, check=True, timeout=900)
    with open(out) as f:
        return json.load(f)


def merge(runs, key, check_bits):
    out = []
    for a, b, c in zip(*(r[key] for r in runs)):
        assert (a["K"], a["N"], a["M"]) == (b["K"], b["N"], b["M"]) == (c["K"], c["N"], c["M"])
        p = {"K": a["K"], "N": a["N"], "M": a["M"], "A": a["A"], "B": b["B"], "C": b["C"], "A_again": c["A"]}
        a0, a1 = p["A"]["graph_ms"], p["A_again"]["graph_ms"]
        tb, tc = p["B"]["graph_ms"], p["C"]["graph_ms"]
        lo, hi = min(a0, a1), max(a0, a1)
        p["spread"] = (hi - lo) / lo
        p["a_over_b"] = lo / tb
        p["b_wins"] = bool(tb < lo * (1.0 - p["spread"]))
        p["b_loses"] = bool(tb > hi * (1.0 + p["spread"]))
        p["c_level"] = bool(lo * (1.0 - p["spread"]) <= tc <= hi * (1.0 + p["spread"]))
        if check_bits:
            p["bits_equal"] = a["A"]["sha256"] == b["B"]["sha256"] == b["C"]["sha256"]
        out.append(p)
    return out


def us(p, leg):
    return 1e3 * p[leg]["graph_ms"]


def table(res):
    """The README's table, from the JSON."""
    def verdict(p):
        if p["M"] <= 16:
            return "same launch"
        return "yes" if p["b_wins"] else "LOSES" if p["b_loses"] else "level"

    lines = ["| K x N | M | (A) parent, µs | again | (B) decode_rows 64, µs | (RT, T) | (C) default, µs | spread | A / B | B wins |",
             "|---|---|---|---|---|---|---|---|---|---|"]
    for p in res["points"]:
        rt, t = p["B"].get("launch", [0, 0])[:2]
        lines.append(f"| {p['K']} x {p['N']} | {p['M']} | {us(p, 'A'):.2f} | {us(p, 'A_again'):.2f} | {us(p, 'B'):.2f} | "
                     f"({rt}, {t}) | {us(p, 'C'):.2f} | {100 * p['spread']:.1f} % | {p['a_over_b']:.2f} | "
                     f"{verdict(p)} |")
    for key, what in (("layer", "q8_norm + bf16 residual in place"), ("rotation", "rotation of 20 plans")):
        for p in res[key]:
            lines.append(f"| {p['K']} x {p['N']}, {what} | {p['M']} | {us(p, 'A'):.2f} | {us(p, 'A_again'):.2f} | "
                         f"{us(p, 'B'):.2f} | | {us(p, 'C'):.2f} | {100 * p['spread']:.1f} % | {p['a_over_b']:.2f} | "
                         f"{verdict(p)} |")
    return "\n".join(lines)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--parent-pkg", help="a build of the parent commit: the directory holding its tcsc_amd/ and lib/")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--shapes", nargs="+", default=None, metavar="KxN")
    ap.add_argument("--ms", nargs="+", type=int, default=list(MS))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "decode_rows_bench.json"))
    ap.add_argument("--table", action="store_true", help="print the README table from --out and exit")
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--child-out", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    args.shape_list = SHAPES if not args.shapes else [tuple(int(v) for v in s.lower().split("x")) for s in args.shapes]
    if args.table:
        with open(args.out) as f:
            print(table(json.load(f)))
        return
    if args.child:
        child(args.child, args.reps, args.child_out, args.shape_list, args.ms)
        return
    if not args.parent_pkg or not os.path.exists(os.path.join(args.parent_pkg, "lib", "libtcsc_amd.so")):
        raise SystemExit("--parent-pkg must name a build of the parent commit (tcsc_amd/ and lib/libtcsc_amd.so)")
    parent = os.path.abspath(args.parent_pkg)
    with tempfile.TemporaryDirectory() as tmp:
        runs = [run_child("parent", parent, args, tmp), run_child("new", PKG, args, tmp),
                run_child("parent_again", parent, args, tmp)]
    res = {"tool": "tools/decode_rows_bench.py", "device": runs[0]["device"], "cus": runs[1]["cus"], "a": A,
           "variant": "prelu_basic", "density": 0.67, "plan": "packed", "graph_steps": GRAPH_STEPS,
           "timing": "HIP events around windows of replays of a captured graph of graph_steps calls; median per call of "
                     "--reps windows; one child process per library, in the order parent, new, parent again",
           "legs": {"A": "parent commit: sgemm_i8 (k_pack8 + k_gemm8w2 above 16 rows), twice",
                    "B": "this tree, set_decode_rows(64): k_decode8r above 16 rows",
                    "C": "this tree, default setting"},
           "points": merge(runs, "points", True), "layer": merge(runs, "layer", True),
           "rotation": merge(runs, "rotation", False)}
    every = res["points"] + res["layer"]
    res["all_bits_equal"] = all(p["bits_equal"] for p in every)
    res["c_not_level"] = [[p["K"], p["N"], p["M"]] for p in res["points"] if not p["c_level"]]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(table(res))
    print("all_bits_equal", res["all_bits_equal"], "c_not_level", res["c_not_level"])
    if not res["all_bits_equal"]:
        raise SystemExit("A and B differ in their bytes at some point")


if __name__ == "__main__":
    main()
