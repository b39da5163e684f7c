#!/usr/bin/env python3
"""Times the int8 decode path (k_decode8 on the 2-bit image) against what the library ran before it.

tools/i8_bench.py's method: one process, HIP events around windows of back-to-back
calls after a warm-up, median of --reps windows.  Per shape K x N and density one
plan with the int8 and the 2-bit image; per M three timings of tcsc_gpu_sgemm_i8
on it, same X, scales, bias and Y:

  decode        $TCSC_DECODE=1: k_decode8
  fallback      $TCSC_DECODE=0: what the library did before -- k_small_m at
                M <= 4 (4 bytes per nonzero of the merged CSC copy), k_gemm8 above
                (1 byte per weight); the route is recorded
  decode_again  the first once more, after the fallback's windows: the run's own
                spread

Each is timed twice: as eager calls (`ms`), where a call this short is bounded by
the host's enqueue rate, and as replays of a captured graph of GRAPH_CALLS calls
(`graph_ms`, per call), which is how a decode loop runs and what shows the
kernels' own time.

`default_route` is what the call takes with $TCSC_DECODE unset and `pays` what
tcsc_gpu_decode_pays says: where pays is 1 the acceptance is decode <= fallback
within the spread, on both timings.  `image_GBps` is the 2-bit image's bytes over
the graph-replayed decode time.

Warm and cold: back-to-back calls on one plan find its 2-bit image (16.8 MB at
8192 x 8192) in the 256 MiB Infinity Cache.  --cold-plans P builds P plans of
distinct W at 8192 x 8192 (their 2-bit images together exceed the cache from 17
on) and times a rotation over them: the figure that describes a model's layers.

One JSON document goes to --out (default profiles/decode_bench.json) and a
summary table to stdout.  Needs a gfx950 GPU: without one it fails.

    python tools/decode_bench.py [--reps 7] [--cold-plans 20] [--shapes KxN ...] [--out FILE]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "sparse-matrix-multiplication-benchmark_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import tcsc_amd  # noqa: E402
import bf16_bench  # noqa: E402  (timed(): the same windows)

A = 0.2
# K x N: a 2B-class BitNet's projections, and the squares
SHAPES = [(2560, 6912), (6912, 2560), (4096, 4096), (8192, 8192)]
MS = (1, 4, 8, 16)
# at 4096^2 also the densities around the rule's 1/16, at the M where the fallback is k_small_m
LOW_DENSITIES = (0.06, 0.1, 0.33)
LOW_MS = (1, 4)
GRAPH_CALLS = 20  # calls per captured graph (a whole rotation when there are more plans)


def make_plan(torch, K, N, density, seed):
    """A default-built plan (no $TCSC_PATH) of a random ternary K x N W of that density, with both images."""
    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream().cuda_stream
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    u = torch.rand((K, N), device=dev, generator=g)
    Wd = torch.zeros((K, N), device=dev)
    Wd[u < density / 2] = 1.0
    Wd[(u >= density / 2) & (u < density)] = -1.0
    del u
    csp = torch.empty(N + 1, dtype=torch.int32, device=dev)
    csn = torch.empty(N + 1, dtype=torch.int32, device=dev)
    n_pos, n_neg = tcsc_amd.gpu_from_dense(Wd, K, N, csp, csn, stream=stream)
    rip = torch.empty(max(n_pos, 1), dtype=torch.int32, device=dev)
    rin = torch.empty(max(n_neg, 1), dtype=torch.int32, device=dev)
    tcsc_amd.gpu_from_dense(Wd, K, N, csp, csn, rip, rin, stream=stream)
    del Wd
    plan = tcsc_amd.Plan.from_device(K, N, csp, csn, rip, rin, stream=stream)
    plan.keep = (csp, csn, rip, rin)
    plan.reserve(max(MS))
    if not (plan.enable_i8(stream) and plan.enable_w2(stream)):
        raise SystemExit(f"no int8 / 2-bit image at {K} x {N}, density {density}")
    return plan, n_pos + n_neg


def inputs(torch, M, K, N, seed):
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    Xq = torch.randint(-127, 128, (M, K), device=dev, generator=g, dtype=torch.int32).to(torch.int8)
    S = torch.rand(M, device=dev, generator=g) * 0.05 + 1e-3
    B = torch.rand(N, device=dev, generator=g) - 0.5
    return Xq, S, B


def time_routes(torch, plans, M, K, N, nnz, reps):
    """The three timings of one point; `plans` is one plan (warm) or the rotation (cold)."""
    stream = torch.cuda.current_stream().cuda_stream
    Xq, S, B = inputs(torch, M, K, N, 100 + M)
    Y = torch.empty((M, N), device=Xq.device)
    turn = [0]

    def call():
        plan = plans[turn[0] % len(plans)]
        turn[0] += 1
        plan.sgemm_i8(Xq, S, B, Y, M, N, "prelu_basic", A, stream)

    os.environ.pop("TCSC_DECODE", None)
    out = {"M": M, "pays": int(tcsc_amd.decode_pays(M, K, N, nnz)), "default_route": plans[0].launch_info_i8(M)[0]}
    got = {}
    for name, knob in (("decode", "1"), ("fallback", "0"), ("decode_again", "1")):
        os.environ["TCSC_DECODE"] = knob
        route = plans[0].launch_info_i8(M)[0]
        assert (route == "decode") == (knob == "1"), (name, route)
        out[name] = dict(bf16_bench.timed(torch, call, reps), route=route)
        n = max(GRAPH_CALLS, len(plans))
        turn[0] = 0
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            st = torch.cuda.current_stream().cuda_stream
            for _ in range(n):
                plan = plans[turn[0] % len(plans)]
                turn[0] += 1
                plan.sgemm_i8(Xq, S, B, Y, M, N, "prelu_basic", A, st)
        t = bf16_bench.timed(torch, graph.replay, reps)
        out[name].update(graph_ms=t["ms"] / n, graph_ms_min=t["ms_min"] / n, graph_ms_max=t["ms_max"] / n,
                         graph_calls=n)
        del graph
        turn[0] = 0
        call()
        torch.cuda.synchronize()
        got[name] = Y.clone()
    os.environ.pop("TCSC_DECODE", None)
    if out["fallback"]["route"] == "mfma":  # k_gemm8 runs the same epilogue on the same exact sums
        out["bits_equal_fallback"] = bool(torch.equal(got["decode"].view(torch.int32), got["fallback"].view(torch.int32)))
    else:  # k_small_m rounds s * q first: close, not equal
        out["max_abs_diff_fallback"] = float((got["decode"] - got["fallback"]).abs().max())
    out["holds"] = True
    for key, tag in (("ms", "eager"), ("graph_ms", "graph")):
        d, f, d2 = out["decode"][key], out["fallback"][key], out["decode_again"][key]
        out[tag + "_fallback_over_decode"] = f / d
        out[tag + "_spread"] = abs(d2 - d) / d  # run-to-run spread of the decode timing in this run
        if out["pays"] and min(d, d2) > f * (1.0 + out[tag + "_spread"]):
            out["holds"] = False
    out["image_GBps"] = tcsc_amd.w2_image_bytes(K, N) / (out["decode"]["graph_ms"] * 1e-3) / 1e9
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--cold-plans", type=int, default=20)
    ap.add_argument("--shapes", nargs="+", default=None, metavar="KxN",
                    help="only these shapes at density 0.67, no low densities (A/B builds via $TCSC_AMD_LIB)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "decode_bench.json"))
    args = ap.parse_args()
    import torch

    tcsc_amd.require_gpu()
    for k in ("TCSC_PATH", "TCSC_SMALL_M", "TCSC_SLICES", "TCSC_MFMA_WGS", "TCSC_DECODE"):
        os.environ.pop(k, None)
    res = {"tool": "tools/decode_bench.py", "lib": os.path.relpath(tcsc_amd.LIB_PATH, ROOT), "device": torch.cuda.get_device_name(0), "a": A, "variant": "prelu_basic",
           "timing": "HIP events around windows of back-to-back calls; median per call of --reps windows",
           "warm": [], "cold": []}
    points = [(K, N, 0.67, MS) for K, N in SHAPES] + [(4096, 4096, d, LOW_MS) for d in LOW_DENSITIES]
    if args.shapes:
        points = [(int(k), int(n), 0.67, MS) for k, n in (s.lower().split("x") for s in args.shapes)]
    for K, N, density, Ms in points:
        plan, nnz = make_plan(torch, K, N, density, 1000 + K + N)
        row = {"K": K, "N": N, "density": density, "nnz": nnz, "w2_image_bytes": tcsc_amd.w2_image_bytes(K, N),
               "i8_image_bytes": N * ((K + 127) // 128 * 128), "csc_entry_bytes": 4 * nnz,
               "points": [time_routes(torch, [plan], M, K, N, nnz, args.reps) for M in Ms]}
        res["warm"].append(row)
        plan.destroy()
        torch.cuda.empty_cache()
    if args.cold_plans > 0:
        K = N = 8192
        plans, nnz = [], 0
        for i in range(args.cold_plans):
            plan, nnz = make_plan(torch, K, N, 0.67, 5000 + i)
            plans.append(plan)
        res["cold"].append({"K": K, "N": N, "density": 0.67, "nnz_last": nnz, "plans": len(plans),
                            "w2_images_bytes": len(plans) * tcsc_amd.w2_image_bytes(K, N),
                            "points": [time_routes(torch, plans, M, K, N, nnz, args.reps) for M in MS]})
        for plan in plans:
            plan.destroy()
    res["all_hold"] = all(p["holds"] for kind in ("warm", "cold") for row in res[kind] for p in row["points"])
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    for kind in ("warm", "cold"):
        for row in res[kind]:
            for p in row["points"]:
                print(f"{kind} {row['K']}x{row['N']} d={row['density']} M={p['M']:2d} pays={p['pays']} "
                      f"default={p['default_route']:6s} | graph: decode {1e3 * p['decode']['graph_ms']:7.2f} us "
                      f"(again {1e3 * p['decode_again']['graph_ms']:7.2f}) {p['fallback']['route']:5s} "
                      f"{1e3 * p['fallback']['graph_ms']:7.2f} us x{p['graph_fallback_over_decode']:.2f} "
                      f"{p['image_GBps']:6.0f} GB/s | eager: decode {1e3 * p['decode']['ms']:7.2f} us "
                      f"{p['fallback']['route']:5s} {1e3 * p['fallback']['ms']:7.2f} us "
                      f"x{p['eager_fallback_over_decode']:.2f} | holds={p['holds']}")
    print("all_hold", res["all_hold"])


if __name__ == "__main__":
    main()
