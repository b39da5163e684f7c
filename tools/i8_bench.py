#!/usr/bin/env python3
"""Times tcsc_gpu_sgemm_i8 next to tcsc_gpu_sgemm_bf16 and tcsc_gpu_sgemm on one GPU.

tools/bf16_bench.py's method: at cfg 5, cfg 2 and cfg 4 (tcsc_amd.workloads.CONFIGS),
in one process, all calls on one plan, HIP events around windows of back-to-back
launches after a warm-up (median of --reps windows):

  fp32        tcsc_gpu_sgemm on fp32 X (the config's variant)
  bf16        tcsc_gpu_sgemm_bf16 on the same X rounded to bf16: the yardstick,
              the fastest way the library had to do this work
  i8          tcsc_gpu_sgemm_i8 on the rows of X quantized by
              tcsc_gpu_quantize_rows_i8, with their scales (after enable_i8)
  quant       tcsc_gpu_quantize_rows_i8 alone
  kernels     per-kernel mean microseconds of each call from torch's profiler
              (k_pack8, k_gemm8, k_reduce_i8; k_pack1, k_gemm3, ...), a few calls
              each, apart from the timed windows

`check` records whether the int8 call's bits equal the float32 formula
act(fl(fl(float32(S)) * s) + b) with S from an int32 torch matmul of the same
operands on a sample of rows (MFMA path), or the fp32 call's on Xs = s * q
(gather).  One JSON line goes to --out (default profiles/i8_bench.json) and to
stdout.  Needs a gfx950 GPU: without one it fails, it never falls back.

    python tools/i8_bench.py [--cfgs 5 2 4] [--reps 7] [--out FILE]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "sparse-matrix-multiplication-benchmark_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import tcsc_amd  # noqa: E402
from tcsc_amd import workloads  # noqa: E402
import bf16_bench  # noqa: E402  (timed(), kernel_split(): the same windows and profiler)

A = 0.2
# (the transposes are told apart by bf16_bench.kernel_name: k_transpose, k_transpose_bf16, k_transpose_i8)
bf16_bench.KERNELS = ("k_transpose", "k_stream", "k_reduce_fix", "k_reduce_i8", "k_reduce4", "k_reduce", "k_split3",
                      "k_pack1", "k_pack8", "k_gemm3", "k_gemm8", "k_fixup", "k_small_m", "k_quant_rows_i8")


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
    rows = torch.arange(0, M, max(1, M // 64), device=dev)[:64]  # the checked sample
    plan = tcsc_amd.Plan.from_device(K, N, csp, csn, rip, rin, stream=stream)
    plan.reserve(M)
    before = plan.info()["device_bytes"]
    has_i8 = plan.enable_i8(stream)
    Xb = X.to(torch.bfloat16)
    Xq = torch.empty((M, K), dtype=torch.int8, device=dev)
    S = torch.empty(M, device=dev)
    tcsc_amd.quantize_rows_i8(X, Xq, S, M, K, stream)
    Y = torch.empty((M, N), device=dev)
    Y8 = torch.empty((M, N), device=dev)

    def fp32():
        plan.sgemm(X, B, Y, M, N, cfg.variant, A, stream)

    def bf16():
        plan.sgemm_bf16(Xb, B, Y, M, N, cfg.variant, A, stream)

    def i8():
        plan.sgemm_i8(Xq, S, B, Y8, M, N, cfg.variant, A, stream)

    def quant():
        tcsc_amd.quantize_rows_i8(X, Xq, S, M, K, stream)

    out = {"M": M, "K": K, "N": N, "density": cfg.density, "variant": cfg.variant, "nnz": n_pos + n_neg,
           "has_i8": bool(has_i8), "i8_image_bytes": plan.info()["device_bytes"] - before,
           "paths": {"fp32": plan.launch_info(M), "bf16": plan.launch_info_bf16(M), "i8": plan.launch_info_i8(M)},
           "plan_device_bytes": plan.info()["device_bytes"]}
    out["fp32"] = bf16_bench.timed(torch, fp32, reps)
    out["bf16"] = bf16_bench.timed(torch, bf16, reps)
    out["i8"] = bf16_bench.timed(torch, i8, reps)
    out["bf16_again"] = bf16_bench.timed(torch, bf16, reps)  # the yardstick after the i8 windows: the run's own spread
    out["quant"] = bf16_bench.timed(torch, quant, reps)
    try:
        out["kernels_us"] = {"fp32": bf16_bench.kernel_split(torch, fp32), "bf16": bf16_bench.kernel_split(torch, bf16),
                             "i8": bf16_bench.kernel_split(torch, i8), "quant": bf16_bench.kernel_split(torch, quant)}
    except Exception as e:  # the profiler is torch's, not the library's: say so and keep the timed windows
        out["kernels_us"] = {"error": f"{type(e).__name__}: {e}"}
    # the int8 call against its contract on a sample of rows
    i8()
    torch.cuda.synchronize()
    prelu = "prelu" in cfg.variant
    if out["paths"]["i8"][0] == "mfma":
        Wi = Wd.to(torch.float64)
        Sx = (Xq[rows].to(torch.float64) @ Wi)  # exact: |S| <= 127 K < 2^53
        v = Sx.to(torch.float32) * S[rows][:, None] + B[None, :]
        want = torch.where(v < 0, A * v, v) if prelu else v
        out["check"] = {"rows": int(rows.numel()), "max_abs_sum": float(Sx.abs().max()),
                        "bits_equal_formula": bool(torch.equal(want.view(torch.int32), Y8[rows].view(torch.int32)))}
    else:
        Xs = S[:, None] * Xq.float()
        plan.sgemm(Xs, B, Y, M, N, cfg.variant, A, stream)
        torch.cuda.synchronize()
        out["check"] = {"same_route": out["paths"]["fp32"] == out["paths"]["i8"],
                        "bits_equal_fp32_on_scaled_x": bool(torch.equal(Y.view(torch.int32), Y8.view(torch.int32)))}
    del Wd, inp
    out["ratios"] = {"i8_over_bf16": out["i8"]["ms"] / out["bf16"]["ms"],
                     "i8_over_fp32": out["i8"]["ms"] / out["fp32"]["ms"],
                     "bf16_over_fp32": out["bf16"]["ms"] / out["fp32"]["ms"]}
    k = out["kernels_us"]
    if "i8" in k and "k_gemm8" in k["i8"] and "k_gemm3" in k.get("bf16", {}):
        out["ratios"]["k_gemm8_over_k_gemm3_one_part"] = k["i8"]["k_gemm8"] / k["bf16"]["k_gemm3"]
    assert plan.info()["device_bytes"] == out["plan_device_bytes"], "a call grew the reserved plan"
    plan.destroy()
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--cfgs", type=int, nargs="+", default=[5, 2, 4])
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "i8_bench.json"))
    args = ap.parse_args()
    import torch

    tcsc_amd.require_gpu()
    res = {"tool": "tools/i8_bench.py", "device": torch.cuda.get_device_name(0), "a": A,
           "timing": "HIP events around windows of back-to-back calls; median per call; kernels_us by torch.profiler",
           "cfgs": {f"cfg{i}": bench_cfg(torch, workloads.CONFIGS[i], args.reps) for i in args.cfgs}}
    line = json.dumps(res)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
