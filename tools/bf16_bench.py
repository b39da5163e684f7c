#!/usr/bin/env python3
"""Times tcsc_gpu_sgemm_bf16 next to tcsc_gpu_sgemm on one GPU.

At cfg 5, cfg 4 and cfg 2 (tcsc_amd.workloads.CONFIGS), in one process, with
HIP events around windows of back-to-back launches after a warm-up (median of
--reps windows):

  fp32        tcsc_gpu_sgemm on fp32 X (the config's variant)
  bf16        tcsc_gpu_sgemm_bf16 on the same X rounded to bf16, same plan
  cast        torch's X.float() of the bf16 X: what a bf16 caller of the fp32
              entry point pays on top of `fp32`
  kernels     per-kernel mean microseconds of either call from torch's profiler
              (k_split3 / k_pack1, k_gemm3, k_fixup or k_reduce_fix; k_transpose --
              its bf16 instantiation reported as k_transpose_bf16 --, k_stream,
              ...), a few calls each, apart from the timed windows

The two calls must agree: `check` records whether the bf16 call's bits equal
the fp32 call's on the widened X.  One JSON line goes to --out (default
profiles/bf16_bench.json) and to stdout.  Needs a gfx950 GPU: without one it
fails, it never falls back.

    python tools/bf16_bench.py [--cfgs 5 4 2] [--reps 7] [--out FILE]
"""
import argparse
import json
import os
import re
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "sparse-matrix-multiplication-benchmark_amd"))

import tcsc_amd  # noqa: E402
from tcsc_amd import workloads  # noqa: E402

A = 0.2
# the library's kernels by name, longer names first where one is a prefix of another
KERNELS = ("k_transpose", "k_stream", "k_reduce_fix", "k_reduce4", "k_reduce", "k_split3", "k_pack1", "k_gemm3",
           "k_fixup", "k_small_m")
# k_transpose<VEC, TX> is one template: its instantiations are reported apart by X's type (demangled, or the
# type's letter in the mangled name), under the names the three kernels had, so old and new profiles compare
# (and a library from before the template, given through $TCSC_AMD_LIB, reports under the same keys)
TRANSPOSE = re.compile(r"k_transpose(?:_(bf16|i8)|<\w+, ([a-z ]+)>|ILb[01]E([fta]))")
TRANSPOSE_KEY = {"float": "k_transpose", "f": "k_transpose", "unsigned short": "k_transpose_bf16",
                 "t": "k_transpose_bf16", "signed char": "k_transpose_i8", "a": "k_transpose_i8"}


def kernel_name(key):
    """The reporting name of a profiler event, None when it is not one of the library's kernels."""
    m = TRANSPOSE.search(key)
    if m:
        old, demangled, letter = m.groups()
        return "k_transpose_" + old if old else TRANSPOSE_KEY.get(demangled or letter, "k_transpose")
    return next((k for k in KERNELS if k in key), None)  # demangled or not


def timed(torch, fn, reps, min_window_s=0.05):
    """Per-call milliseconds of fn(): median and min over `reps` event-timed windows
    of `iters` back-to-back calls, iters sized from a first timed call so that a
    window lasts at least min_window_s."""
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    iters = max(3, min(1000, int(min_window_s * 1e3 / max(e0.elapsed_time(e1), 1e-3)) + 1))
    per_call = []
    for _ in range(reps):
        e0.record()
        for _ in range(iters):
            fn()
        e1.record()
        e1.synchronize()
        per_call.append(e0.elapsed_time(e1) / iters)
    return {"ms": statistics.median(per_call), "ms_min": min(per_call), "ms_max": max(per_call), "iters": iters,
            "reps": reps}


def kernel_split(torch, fn, calls=5):
    """{kernel name: mean microseconds per call} of the library's kernels in fn(), by torch's profiler."""
    from torch.profiler import ProfilerActivity, profile

    fn()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        for _ in range(calls):
            fn()
        torch.cuda.synchronize()
    out = {}
    for ev in prof.key_averages():
        name = kernel_name(ev.key)
        if name is None:
            continue
        total = getattr(ev, "device_time_total", None)
        if total is None:
            total = getattr(ev, "cuda_time_total", 0.0)
        out[name] = out.get(name, 0.0) + float(total) / calls
    return out


def bench_cfg(torch, cfg, reps):
    dev = torch.device("cuda:0")
    M, K, N = cfg.M, cfg.K, cfg.N
    stream = torch.cuda.current_stream().cuda_stream
    inp = workloads.make_device_inputs(cfg, 0, N, dev)
    X, B, Wd = inp["X"], inp["B"], inp["Wd"]
    csp = torch.empty(N + 1, dtype=torch.int32, device=dev)
    csn = torch.empty(N + 1, dtype=torch.int32, device=dev)
    n_pos, n_neg = tcsc_amd.gpu_from_dense(Wd, K, N, csp, csn, stream=stream)
    rip = torch.empty(max(n_pos, 1), dtype=torch.int32, device=dev)
    rin = torch.empty(max(n_neg, 1), dtype=torch.int32, device=dev)
    tcsc_amd.gpu_from_dense(Wd, K, N, csp, csn, rip, rin, stream=stream)
    del Wd, inp
    plan = tcsc_amd.Plan.from_device(K, N, csp, csn, rip, rin, stream=stream)
    plan.reserve(M)
    Xb = X.to(torch.bfloat16)
    Xw = Xb.float()  # the bf16 values as fp32: what the two calls must agree on
    Y = torch.empty((M, N), device=dev)
    Yb = torch.empty((M, N), device=dev)
    cast = {}

    def fp32():
        plan.sgemm(X, B, Y, M, N, cfg.variant, A, stream)

    def bf16():
        plan.sgemm_bf16(Xb, B, Yb, M, N, cfg.variant, A, stream)

    def do_cast():
        cast["x"] = Xb.float()

    out = {"M": M, "K": K, "N": N, "density": cfg.density, "variant": cfg.variant, "nnz": n_pos + n_neg,
           "paths": {"fp32": plan.launch_info(M), "bf16": plan.launch_info_bf16(M)},
           "plan_device_bytes": plan.info()["device_bytes"]}
    out["fp32"] = timed(torch, fp32, reps)
    out["bf16"] = timed(torch, bf16, reps)
    out["fp32_again"] = timed(torch, fp32, reps)  # the same quantity after the bf16 windows: the run's own spread
    out["cast"] = timed(torch, do_cast, reps)
    try:
        out["kernels_us"] = {"fp32": kernel_split(torch, fp32), "bf16": kernel_split(torch, bf16)}
    except Exception as e:  # the profiler is torch's, not the library's: say so and keep the timed windows
        out["kernels_us"] = {"error": f"{type(e).__name__}: {e}"}
    # the bits of the fp32 call on the widened X (same path and K split only)
    plan.sgemm(Xw, B, Y, M, N, cfg.variant, A, stream)
    plan.sgemm_bf16(Xb, B, Yb, M, N, cfg.variant, A, stream)
    torch.cuda.synchronize()
    out["check"] = {"same_route": out["paths"]["fp32"] == out["paths"]["bf16"],
                    "bits_equal_fp32_on_widened_x": bool(torch.equal(Y.view(torch.int32), Yb.view(torch.int32))),
                    "max_abs_diff": float((Y - Yb).abs().max())}
    out["ratios"] = {"bf16_over_fp32": out["bf16"]["ms"] / out["fp32"]["ms"],
                     "bf16_over_fp32_plus_cast": out["bf16"]["ms"] / (out["fp32"]["ms"] + out["cast"]["ms"])}
    assert plan.info()["device_bytes"] == out["plan_device_bytes"], "a bf16 call grew the reserved plan"
    plan.destroy()
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--cfgs", type=int, nargs="+", default=[5, 4, 2])
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bf16_bench.json"))
    args = ap.parse_args()
    import torch

    tcsc_amd.require_gpu()
    res = {"tool": "tools/bf16_bench.py", "device": torch.cuda.get_device_name(0), "a": A,
           "timing": "HIP events around windows of back-to-back calls; median per call; kernels_us by torch.profiler",
           "cfgs": {f"cfg{i}": bench_cfg(torch, workloads.CONFIGS[i], args.reps) for i in args.cfgs}}
    line = json.dumps(res)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
