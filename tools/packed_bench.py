#!/usr/bin/env python3
"""Times tcsc_gpu_sgemm_i8 on a packed plan (k_pack8 + k_gemm8w2 on the 2-bit image) against the
same call on an ordinary plan of the same W (k_pack8 + k_gemm8 on the int8 image: what the library ran before).

tools/decode_bench.py's method: one process, HIP events around windows of back-to-back calls after a warm-up,
median of --reps windows; each configuration as eager calls (`ms`) and as replays of a captured graph of
GRAPH_CALLS calls (`graph_ms`, per call: the kernels' own time).  Per shape K x N (density 0.67, prelu_basic) one
ordinary plan (default-built, with the int8 and the 2-bit image) and one packed plan from the same device arrays;
per M, same X, scales, bias and Y:

  base        the ordinary plan's int8 call (route recorded: mfma = k_gemm8)
  packed      the packed plan's call
  base_again  the first once more, after the packed windows: the run's own spread
  knob        the ordinary plan under $TCSC_W2GEMM=1: k_gemm8w2 on a plan that holds everything else too

`bits_equal` says whether packed and base gave the same bits, `bits_equal_knob` the same for the knob.  For
M <= 256 the acceptance is packed <= base within the run's first-against-third spread of the baseline, on the
graph timing; for M >= 512 the call is compute-bound and the ratio is recorded, not gated.  Both plans'
device_bytes (after reserve(max M)) and the 2-bit image's bytes go into each row.

One JSON document goes to --out (default profiles/packed_bench.json) and a summary table to stdout.  Needs a
gfx950 GPU: without one it fails.

    python tools/packed_bench.py [--reps 7] [--shapes KxN ...] [--ms M ...] [--out FILE]
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
import decode_bench  # noqa: E402  (inputs(): the same X, scales and bias)

A = 0.2
SHAPES = [(8192, 8192), (4096, 4096), (2560, 6912), (6912, 2560)]
MS = (17, 32, 64, 128, 256, 512, 2048)
GATED_M = 256
DENSITY = 0.67
GRAPH_CALLS = 20
KNOBS = ("TCSC_PATH", "TCSC_SMALL_M", "TCSC_SLICES", "TCSC_MFMA_WGS", "TCSC_DECODE", "TCSC_W2GEMM")


def make_plans(torch, K, N, seed, max_M):
    """(ordinary plan with both images, packed plan) of one random ternary K x N W, both reserved for max_M rows."""
    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream().cuda_stream
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    u = torch.rand((K, N), device=dev, generator=g)
    Wd = torch.zeros((K, N), device=dev)
    Wd[u < DENSITY / 2] = 1.0
    Wd[(u >= DENSITY / 2) & (u < DENSITY)] = -1.0
    del u
    csp = torch.empty(N + 1, dtype=torch.int32, device=dev)
    csn = torch.empty(N + 1, dtype=torch.int32, device=dev)
    n_pos, n_neg = tcsc_amd.gpu_from_dense(Wd, K, N, csp, csn, stream=stream)
    rip = torch.empty(max(n_pos, 1), dtype=torch.int32, device=dev)
    rin = torch.empty(max(n_neg, 1), dtype=torch.int32, device=dev)
    tcsc_amd.gpu_from_dense(Wd, K, N, csp, csn, rip, rin, stream=stream)
    del Wd
    plan = tcsc_amd.Plan.from_device(K, N, csp, csn, rip, rin, stream=stream)
    plan.reserve(max_M)
    if not (plan.enable_i8(stream) and plan.enable_w2(stream)):
        raise SystemExit(f"no int8 / 2-bit image at {K} x {N}")
    packed = tcsc_amd.Plan.packed_from_device(K, N, csp, csn, rip, rin, stream=stream)
    created = packed.info()["device_bytes"]
    packed.reserve(max_M)
    torch.cuda.synchronize()
    return plan, packed, created, n_pos + n_neg


def time_point(torch, plan, packed, M, K, N, reps):
    stream = torch.cuda.current_stream().cuda_stream
    Xq, S, B = decode_bench.inputs(torch, M, K, N, 100 + M)
    Y = torch.empty((M, N), device=Xq.device)
    out = {"M": M, "gated": M <= GATED_M, "packed_route": list(packed.launch_info_i8(M))}
    got = {}
    for name, p, knob in (("base", plan, None), ("packed", packed, None), ("base_again", plan, None),
                          ("knob", plan, "1")):
        os.environ.pop("TCSC_W2GEMM", None)
        if knob:
            os.environ["TCSC_W2GEMM"] = knob

        def call(st=stream):
            p.sgemm_i8(Xq, S, B, Y, M, N, "prelu_basic", A, st)

        out[name] = dict(bf16_bench.timed(torch, call, reps), route=list(p.launch_info_i8(M)))
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            st = torch.cuda.current_stream().cuda_stream
            for _ in range(GRAPH_CALLS):
                call(st)
        t = bf16_bench.timed(torch, graph.replay, reps)
        out[name].update(graph_ms=t["ms"] / GRAPH_CALLS, graph_ms_min=t["ms_min"] / GRAPH_CALLS,
                         graph_ms_max=t["ms_max"] / GRAPH_CALLS, graph_calls=GRAPH_CALLS)
        del graph
        Y.fill_(float("nan"))
        call()
        torch.cuda.synchronize()
        got[name] = Y.clone()
    os.environ.pop("TCSC_W2GEMM", None)
    same = lambda a, b: bool(torch.equal(got[a].view(torch.int32), got[b].view(torch.int32)))  # noqa: E731
    out["bits_equal"], out["bits_equal_knob"] = same("packed", "base"), same("knob", "base")
    for key, tag in (("ms", "eager"), ("graph_ms", "graph")):
        b, q, b2 = out["base"][key], out["packed"][key], out["base_again"][key]
        out[tag + "_base_over_packed"] = b / q
        out[tag + "_base_over_knob"] = b / out["knob"][key]
        out[tag + "_spread"] = abs(b2 - b) / min(b, b2)  # first against third: the baseline's spread in this run
    b, b2 = out["base"]["graph_ms"], out["base_again"]["graph_ms"]
    out["holds"] = (not out["gated"]) or out["packed"]["graph_ms"] <= max(b, b2)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--shapes", nargs="+", default=None, metavar="KxN")
    ap.add_argument("--ms", nargs="+", type=int, default=list(MS))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "packed_bench.json"))
    args = ap.parse_args()
    import torch

    tcsc_amd.require_gpu()
    for k in KNOBS:
        os.environ.pop(k, None)
    shapes = SHAPES if not args.shapes else [tuple(int(v) for v in s.lower().split("x")) for s in args.shapes]
    res = {"tool": "tools/packed_bench.py", "lib": os.path.relpath(tcsc_amd.LIB_PATH, ROOT),
           "device": torch.cuda.get_device_name(0), "a": A, "variant": "prelu_basic", "density": DENSITY,
           "timing": "HIP events around windows of back-to-back calls; median per call of --reps windows; "
                     "graph_ms is per call of a captured graph of graph_calls calls",
           "gate": f"M <= {GATED_M}: packed graph_ms <= max(base, base_again) graph_ms", "rows": []}
    for K, N in shapes:
        plan, packed, created, nnz = make_plans(torch, K, N, 1000 + K + N, max(args.ms))
        row = {"K": K, "N": N, "nnz": nnz, "w2_image_bytes": tcsc_amd.w2_image_bytes(K, N),
               "packed_device_bytes_created": created, "packed_device_bytes": packed.info()["device_bytes"],
               "ordinary_device_bytes": plan.info()["device_bytes"],
               "points": [time_point(torch, plan, packed, M, K, N, args.reps) for M in args.ms]}
        res["rows"].append(row)
        plan.destroy()
        packed.destroy()
        torch.cuda.empty_cache()
    pts = [p for row in res["rows"] for p in row["points"]]
    res["all_hold"] = all(p["holds"] for p in pts)
    res["all_bits_equal"] = all(p["bits_equal"] and p["bits_equal_knob"] for p in pts)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    for row in res["rows"]:
        print(f"{row['K']}x{row['N']}: device_bytes packed {row['packed_device_bytes_created']} at creation, "
              f"{row['packed_device_bytes']} reserved; ordinary {row['ordinary_device_bytes']}")
        for p in row["points"]:
            print(f"  M={p['M']:4d} {p['base']['route'][0]}/{p['base']['route'][1]} | graph: base "
                  f"{1e3 * p['base']['graph_ms']:8.2f} us (again {1e3 * p['base_again']['graph_ms']:8.2f}) packed "
                  f"{1e3 * p['packed']['graph_ms']:8.2f} us x{p['graph_base_over_packed']:.2f} knob "
                  f"{1e3 * p['knob']['graph_ms']:8.2f} us | eager: base {1e3 * p['base']['ms']:8.2f} packed "
                  f"{1e3 * p['packed']['ms']:8.2f} us x{p['eager_base_over_packed']:.2f} | bits "
                  f"{int(p['bits_equal'])}{int(p['bits_equal_knob'])} gated={int(p['gated'])} holds={p['holds']}")
    print("all_hold", res["all_hold"], "all_bits_equal", res["all_bits_equal"])


if __name__ == "__main__":
    main()
