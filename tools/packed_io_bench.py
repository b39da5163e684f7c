#!/usr/bin/env python3
"""Times loading a packed plan from a saved 2-bit image and unpacking an image to TCSC against the
builders that start from the TCSC arrays or from the dense matrix.

Per shape K x N (density 0.67, one random ternary W made on the device), in one child process under its own
`timeout`, every call timed as wall-clock around the call (each synchronises its stream), median of --reps after
one untimed call:

  create_packed_device        tcsc_gpu_plan_create_packed_device on W's TCSC arrays (what existed before)
  create_packed_image_device  tcsc_gpu_plan_create_packed_image_device on the image of that plan
  create_packed_image         tcsc_gpu_plan_create_packed_image on the same image in pageable host memory
  from_dense                  tcsc_gpu_from_dense on the dense W, both calls of the pair
  w2_to_tcsc                  tcsc_gpu_w2_to_tcsc on the image, both calls of the pair

`same_image`, `same_info` and `same_arrays` say whether the loaded plan and the unpacked arrays equal the ones they
are measured against.  Nothing is gated: nobody has measured these before.  The expectation recorded with every row
is that loading (a quarter byte per weight, read once) beats the build from TCSC (the index arrays walked
ceil(K / 1024) times); `expectation_held` says whether it did.

The parent starts one child per shape and stops at the first that fails or runs out of time.  One JSON document
goes to --out (default profiles/packed_io_bench.json) and a table to stdout.  Needs a gfx950 GPU.

    python tools/packed_io_bench.py [--reps 7] [--shapes KxN ...] [--timeout 240] [--out FILE]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "sparse-matrix-multiplication-benchmark_amd"))

SHAPES = [(8192, 8192), (4096, 4096), (2560, 6912), (6912, 2560)]
DENSITY = 0.67


def median_ms(torch, reps, fn):
    fn()  # untimed: first-call allocations, code loading
    times = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        times.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(times)


def child(K, N, reps):
    import torch

    import tcsc_amd

    tcsc_amd.require_gpu()
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev)
    g.manual_seed(1900 + K + N)
    u = torch.rand((K, N), device=dev, generator=g)
    Wd = torch.zeros((K, N), device=dev)
    Wd[u < DENSITY / 2] = 1.0
    Wd[(u >= DENSITY / 2) & (u < DENSITY)] = -1.0
    del u
    csp = torch.empty(N + 1, dtype=torch.int32, device=dev)
    csn = torch.empty(N + 1, dtype=torch.int32, device=dev)
    arrays = {}

    def from_dense():
        n_pos, n_neg = tcsc_amd.gpu_from_dense(Wd, K, N, csp, csn)
        rip = torch.empty(max(n_pos, 1), dtype=torch.int32, device=dev)
        rin = torch.empty(max(n_neg, 1), dtype=torch.int32, device=dev)
        tcsc_amd.gpu_from_dense(Wd, K, N, csp, csn, rip, rin)
        arrays["dense"] = (csp, csn, rip[:n_pos], rin[:n_neg])

    row = {"K": K, "N": N, "density": DENSITY, "reps": reps}
    row["from_dense_ms"] = median_ms(torch, reps, from_dense)
    _, _, rip, rin = arrays["dense"]
    row["nnz"] = rip.numel() + rin.numel()
    row["tcsc_bytes"] = 4 * (row["nnz"] + 2 * (N + 1))
    row["image_bytes"] = tcsc_amd.w2_image_bytes(K, N)

    plans = {}

    def keep(name, plan):
        if name in plans:
            plans[name].destroy()
        plans[name] = plan

    row["create_packed_device_ms"] = median_ms(
        torch, reps, lambda: keep("tcsc", tcsc_amd.Plan.packed_from_device(K, N, csp, csn, rip, rin)))
    img = plans["tcsc"].w2_image()
    torch.cuda.synchronize()
    host = img.cpu().numpy()
    row["create_packed_image_device_ms"] = median_ms(
        torch, reps, lambda: keep("image", tcsc_amd.Plan.packed_from_image(img, K, N)))
    row["create_packed_image_ms"] = median_ms(
        torch, reps, lambda: keep("host", tcsc_amd.Plan.packed_from_image(host, K, N)))
    row["same_image"] = all(bool(torch.equal(plans[n].w2_image(), img)) for n in ("image", "host"))
    row["same_info"] = all(plans[n].info() == plans["tcsc"].info() for n in ("image", "host"))

    def unpack():
        arrays["image"] = tcsc_amd.w2_to_tcsc(img, K, N)

    row["w2_to_tcsc_ms"] = median_ms(torch, reps, unpack)
    row["same_arrays"] = all(bool(torch.equal(a, b)) for a, b in zip(arrays["image"], arrays["dense"]))
    row["load_over_build"] = row["create_packed_image_device_ms"] / row["create_packed_device_ms"]
    row["unpack_over_from_dense"] = row["w2_to_tcsc_ms"] / row["from_dense_ms"]
    row["expectation_held"] = row["load_over_build"] < 1.0
    for p in plans.values():
        p.destroy()
    print("ROW " + json.dumps(row), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--shapes", nargs="*", default=[f"{k}x{n}" for k, n in SHAPES])
    ap.add_argument("--timeout", type=int, default=240, help="seconds for one shape's child process")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "packed_io_bench.json"))
    ap.add_argument("--child", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        K, N = (int(v) for v in a.child.split("x"))
        child(K, N, a.reps)
        return 0
    rows = []
    for shape in a.shapes:
        cmd = ["timeout", "-k", "10", str(a.timeout), sys.executable, os.path.abspath(__file__), "--child", shape,
               "--reps", str(a.reps)]
        r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
        if r.returncode != 0:  # a fault, an abort or the time limit: nothing more is started on the GPU
            print(f"{shape}: child ended with status {r.returncode}; stopping", file=sys.stderr)
            return 1
        rows += [json.loads(line[4:]) for line in r.stdout.splitlines() if line.startswith("ROW ")]
    doc = {"tool": "tools/packed_io_bench.py", "method": "wall-clock around each synchronising call, median of reps",
           "expectation": "create_packed_image_device faster than create_packed_device (a quarter byte per weight read "
                          "once against the index arrays walked ceil(K / 1024) times)", "rows": rows}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(f"{'K x N':>12} {'from TCSC':>10} {'image dev':>10} {'image host':>10} {'load/build':>10} "
          f"{'from_dense':>10} {'w2_to_tcsc':>10} {'ratio':>6}  ok")
    for r in rows:
        ok = r["same_image"] and r["same_info"] and r["same_arrays"]
        print(f"{r['K']:>5} x {r['N']:<5} {r['create_packed_device_ms']:>10.3f} {r['create_packed_image_device_ms']:>10.3f} "
              f"{r['create_packed_image_ms']:>10.3f} {r['load_over_build']:>10.3f} {r['from_dense_ms']:>10.3f} "
              f"{r['w2_to_tcsc_ms']:>10.3f} {r['unpack_over_from_dense']:>6.2f}  {ok}")
    return 0 if all(r["same_image"] and r["same_info"] and r["same_arrays"] for r in rows) else 1


if __name__ == "__main__":
    sys.exit(main())
