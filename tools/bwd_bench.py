#!/usr/bin/env python3
"""Times the backward pass next to the forward on one GPU.

At cfg 4 and cfg 2 (tcsc_amd.workloads.CONFIGS), in one process, with HIP
events around windows of back-to-back launches after a warm-up:

  forward        tcsc_gpu_sgemm on the plan of W (the config's variant)
  sgemm_t        tcsc_gpu_sgemm_t on the transposed plan, dX = G . W^T
  prelu_backward tcsc_gpu_prelu_backward with db (dZ out of place: 3 M N 4 bytes)
  torch_prelu    torch.where(Y < 0, a * G, G) followed by .sum(0), timed as one
                 quantity: the baseline of prelu_backward
  dense_dx       tcsc_gpu_dense_sgemm (rocBLAS fp32) on a dense W^T: the baseline
                 of sgemm_t
  tplan_build_ms Plan.transposed_from_device, host clock around the call (it
                 synchronises), second build of two

One JSON line goes to --out (default profiles/bwd_bench.json) and to stdout.
Needs a gfx950 GPU: without one it fails, it never falls back.

    python tools/bwd_bench.py [--cfgs 4 2] [--reps 7] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "sparse-matrix-multiplication-benchmark_amd"))

import tcsc_amd  # noqa: E402
from tcsc_amd import workloads  # noqa: E402

HBM_PEAK = 8.0e12  # bytes/s, MI355X
A = 0.2


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
    return {"ms": statistics.median(per_call), "ms_min": min(per_call), "iters": iters, "reps": reps}


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
    plan = tcsc_amd.Plan.from_device(K, N, csp, csn, rip, rin, stream=stream)
    plan.reserve(M)
    build_ms = []
    tplan = None
    for _ in range(2):
        if tplan is not None:
            tplan.destroy()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        tplan = tcsc_amd.Plan.transposed_from_device(K, N, csp, csn, rip, rin, stream=stream)
        build_ms.append((time.perf_counter() - t0) * 1e3)
    tplan.reserve(M)
    g = torch.Generator(device=dev)
    g.manual_seed(cfg.seed + 77)
    G = torch.rand((M, N), generator=g, device=dev) * 2 - 1
    Y = torch.empty((M, N), device=dev)
    DZ = torch.empty((M, N), device=dev)
    DB = torch.empty(N, device=dev)
    DX = torch.empty((M, K), device=dev)
    DXd = torch.empty((M, K), device=dev)
    WdT = Wd.t().contiguous()
    zeros_k = torch.zeros(K, device=dev)

    def fwd():
        plan.sgemm(X, B, Y, M, N, cfg.variant, A, stream)

    def dx():
        tplan.sgemm_t(G, DX, M, K, stream)

    def prelu():
        tcsc_amd.prelu_backward(G, Y, A, DZ, DB, M, N, stream=stream)

    ref = {}

    def torch_prelu():
        ref["dz"] = torch.where(Y < 0, A * G, G)
        ref["db"] = ref["dz"].sum(0)

    def dense_dx():
        tcsc_amd.dense_sgemm(G, WdT, zeros_k, DXd, M, K, N, K, "basic", 0.0, stream)

    out = {"M": M, "K": K, "N": N, "density": cfg.density, "variant": cfg.variant, "nnz": n_pos + n_neg,
           "tplan_build_ms": build_ms[-1], "tplan_build_first_ms": build_ms[0],
           "plan_device_bytes": plan.info()["device_bytes"], "tplan_device_bytes": tplan.info()["device_bytes"],
           "paths": {"forward": plan.launch_info(M), "sgemm_t": tplan.launch_info(M)}}
    out["forward"] = timed(torch, fwd, reps)  # leaves the Y the PReLU mask reads
    out["sgemm_t"] = timed(torch, dx, reps)
    out["prelu_backward"] = timed(torch, prelu, reps)
    out["torch_prelu"] = timed(torch, torch_prelu, reps)
    out["dense_dx"] = timed(torch, dense_dx, reps)
    torch.cuda.synchronize()
    # the timed calls computed the same things
    out["check"] = {"dz_equal_torch": bool(torch.equal(DZ, ref["dz"])),
                    "db_max_abs_diff_vs_torch": float((DB - ref["db"]).abs().max()),
                    "dx_max_abs_diff_vs_dense": float((DX - DXd).abs().max()),
                    "dx_max_abs": float(DX.abs().max())}
    pb = 3 * M * N * 4
    out["prelu_backward"]["bytes"] = pb
    out["prelu_backward"]["fraction_of_8TBps"] = pb / (out["prelu_backward"]["ms"] * 1e-3) / HBM_PEAK
    out["ratios"] = {"sgemm_t_over_forward": out["sgemm_t"]["ms"] / out["forward"]["ms"],
                     "prelu_backward_over_torch": out["prelu_backward"]["ms"] / out["torch_prelu"]["ms"],
                     "sgemm_t_over_dense_dx": out["sgemm_t"]["ms"] / out["dense_dx"]["ms"]}
    plan.destroy()
    tplan.destroy()
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--cfgs", type=int, nargs="+", default=[4, 2])
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bwd_bench.json"))
    args = ap.parse_args()
    import torch

    tcsc_amd.require_gpu()
    res = {"tool": "tools/bwd_bench.py", "device": torch.cuda.get_device_name(0), "a": A,
           "timing": "HIP events around windows of back-to-back calls; median per call",
           "cfgs": {f"cfg{i}": bench_cfg(torch, workloads.CONFIGS[i], args.reps) for i in args.cfgs}}
    line = json.dumps(res)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
