#!/usr/bin/env python3
"""Times the gated and the grouped int8 call at 16 .. 64 rows on the one row-tiled decode launch (k_decode8gr /
k_decode8mr) against the MFMA route the same call took before: the table the rules
tcsc_gpu_glu_rows_pays and tcsc_gpu_group_rows_pays are fitted to.

tools/group_bench.py's and tools/glu_bench.py's protocol: HIP events around windows of replays of a captured graph of
GRAPH_STEPS steps after a warm-up, median per step of --reps windows.  A step is one bf16 X (M x K) in, the RMSNorm
and the quantizer in front, and bf16 outputs with column scales and biases, on packed plans of random ternary
matrices of density 0.67:

  grouped  tcsc_gpu_sgemm_q8_group on K = 2560 with 2560 + 640 + 640 columns, 4096 with 3 x 4096, 8192 with
           8192 + 1024 + 1024;
  gated    tcsc_gpu_sgemm_q8_glu, relu^2, on 2560 x 6912, 4096 x 4096 and 8192 x 8192.

Three variants, which give the same bytes (asserted: the SHA-256 of every output and of the row scales):

  (A) the parent commit's library, the call as it is (`A_us`: two samples, from a child process before and one after
      everything else -- their difference is the run's own spread);
  (B) this tree's library with tcsc_gpu_plan_set_decode_rows_multi(64) on every plan: the new route;
  (C) this tree's library at the default setting, 16: what every existing caller gets.

Three child processes, one library each, every point in each, in the order parent, new, parent again.  The parent is
--parent-pkg: a build of the parent commit (its `tcsc_amd/` and `lib/`; $TCSC_AMD_LIB names its library).

Per point: spread = |A1 - A0| / A0, `A_over_B` (the parent's mean over B), `B_beats_both` (B below both samples of
A: the only points at which a pays rule may say 1) and `C_within_spread`.  One JSON document goes to --out (default
profiles/multi_rows_bench.json) and a table to stdout.  Needs a gfx950 GPU.

    python tools/multi_rows_bench.py --parent-pkg DIR [--reps 5] [--ms M ...] [--out FILE]
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
sys.path.insert(0, os.path.join(ROOT, "tools"))

GROUP_SHAPES = [(2560, (2560, 640, 640)), (4096, (4096, 4096, 4096)), (8192, (8192, 1024, 1024))]
GLU_SHAPES = [(2560, 6912), (4096, 4096), (8192, 8192)]
MS = (16, 17, 24, 32, 33, 48, 64)
EPS = 1e-5
KNOBS = ("TCSC_PATH", "TCSC_SMALL_M", "TCSC_SLICES", "TCSC_MFMA_WGS", "TCSC_DECODE", "TCSC_QFUSE", "TCSC_W2GEMM")


def sha(torch, t):
    t = t.contiguous()
    if t.dtype == torch.bfloat16:
        t = t.view(torch.int16)
    return hashlib.sha256(t.cpu().numpy().tobytes()).hexdigest()


def child(mode, ms, reps, out_path):
    """One library, every point.  mode: parent / parent_again (variant A), new (variants B and C)."""
    import tcsc_amd
    import torch

    from bf16_bench import timed
    from out_bench import make_plan, time_graph

    tcsc_amd.require_gpu()
    for k in KNOBS:
        os.environ.pop(k, None)
    is_new = os.path.realpath(tcsc_amd.LIB_PATH).startswith(os.path.realpath(PKG) + os.sep)
    assert is_new == (mode == "new"), f"mode {mode} on the wrong library ({tcsc_amd.LIB_PATH})"
    dev = torch.device("cuda:0")
    res = {"mode": mode, "lib": tcsc_amd.LIB_PATH, "device": torch.cuda.get_device_name(0),
           "num_cus": torch.cuda.get_device_properties(0).multi_processor_count, "points": []}
    variants = (("B", 64), ("C", 16)) if mode == "new" else (("A", None),)

    def measure(p, plans, M, step, outs, S):
        for tag, rows in variants:
            if rows is not None:
                for plan in plans:
                    plan.set_decode_rows_multi(rows)
            p[tag] = time_graph(torch, timed, step, reps)
            for t in outs:
                t.zero_()
            S.zero_()
            step(torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
            p[tag + "_sha256"] = [sha(torch, t) for t in outs] + [sha(torch, S)]
        res["points"].append(p)

    def inputs(M, K, cols, seed):
        g = torch.Generator(device=dev)
        g.manual_seed(seed)
        X = torch.randn((M, K), device=dev, generator=g).to(torch.bfloat16)
        gamma = torch.rand(K, device=dev, generator=g) + 0.5
        bs = [torch.rand(n, device=dev, generator=g) - 0.5 for n in cols]
        cs = [torch.rand(n, device=dev, generator=g) * 0.04 + 0.01 for n in cols]  # per-column beta of an absmean rule
        return X, gamma, bs, cs, torch.empty((M, K), dtype=torch.int8, device=dev), torch.empty(M, device=dev)

    for K, cols in GROUP_SHAPES:
        plans = [make_plan(torch, tcsc_amd, K, n, 1000 * (i + 1) + K + n) for i, n in enumerate(cols)]
        for plan in plans:
            plan.reserve(max(ms))
        total = sum(cols)
        for M in ms:
            X, gamma, bs, cs, Xq, S = inputs(M, K, cols, 100 + M)
            Y = torch.empty((M, total), dtype=torch.bfloat16, device=dev)
            Ys = list(torch.split(Y, list(cols), dim=1))

            def step(st):
                tcsc_amd.sgemm_q8_group(plans, X, Xq, S, bs, Ys, M, [total] * len(cols), cs, gamma, EPS, st)

            p = {"call": "group", "K": K, "cols": list(cols), "M": M}
            if mode == "new":
                for plan in plans:
                    plan.set_decode_rows_multi(64)
                p["route_B"] = tcsc_amd.launch_info_group(plans, M, "bf16")[0]
                p["launch_B"] = list(tcsc_amd.launch_info_group_decode(plans, M))
            measure(p, plans, M, step, Ys, S)
        for plan in plans:
            plan.destroy()
        torch.cuda.empty_cache()
        print(f"[{mode}] group K={K} cols={cols} done", file=sys.stderr, flush=True)

    for K, H in GLU_SHAPES:
        plans = [make_plan(torch, tcsc_amd, K, H, 2000 * (i + 1) + K + H) for i in range(2)]
        for plan in plans:
            plan.reserve(max(ms))
        for M in ms:
            X, gamma, bs, cs, Xq, S = inputs(M, K, (H, H), 200 + M)
            Y = torch.empty((M, H), dtype=torch.bfloat16, device=dev)
            G = torch.empty((M, H), device=dev)

            def step(st):
                tcsc_amd.sgemm_q8_glu(plans[0], plans[1], X, Xq, S, bs[0], bs[1], Y, M, H, "relu2", cs[0], cs[1], gamma, EPS,
                                      G, st)

            p = {"call": "glu", "K": K, "cols": [H], "M": M}
            if mode == "new":
                for plan in plans:
                    plan.set_decode_rows_multi(64)
                p["route_B"] = tcsc_amd.launch_info_glu(plans[0], plans[1], M, "bf16")[0]
                p["launch_B"] = list(tcsc_amd.launch_info_glu_decode(plans[0], plans[1], M))
            measure(p, plans, M, step, [Y], S)
        for plan in plans:
            plan.destroy()
        torch.cuda.empty_cache()
        print(f"[{mode}] glu K={K} H={H} done", file=sys.stderr, flush=True)
    with open(out_path, "w") as f:
        json.dump(res, f)


def run_child(mode, pkg, args, tmp):
    out = os.path.join(tmp, mode + ".json")
    env = dict(os.environ, PYTHONPATH=pkg + os.pathsep + os.environ.get("PYTHONPATH", ""),
               TCSC_AMD_LIB=os.path.join(pkg, "lib", "libtcsc_amd.so"))
    cmd = [sys.executable, os.path.abspath(__file__), "--child", mode, "--child-out", out, "--reps", str(args.reps),
           "--ms"] + [str(m) for m in args.ms]
    subprocess.run(cmd, env=env, check=True, timeout=600)
    with open(out) as f:
        return json.load(f)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--parent-pkg", help="a build of the parent commit: the directory holding its tcsc_amd/ and lib/")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--ms", nargs="+", type=int, default=list(MS))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "multi_rows_bench.json"))
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--child-out", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        child(args.child, args.ms, args.reps, args.child_out)
        return
    if not args.parent_pkg or not os.path.exists(os.path.join(args.parent_pkg, "lib", "libtcsc_amd.so")):
        raise SystemExit("--parent-pkg must name a build of the parent commit (tcsc_amd/ and lib/libtcsc_amd.so)")
    parent = os.path.abspath(args.parent_pkg)
    with tempfile.TemporaryDirectory() as tmp:
        runs = [run_child("parent", parent, args, tmp), run_child("new", PKG, args, tmp),
                run_child("parent_again", parent, args, tmp)]
    res = {"tool": "tools/multi_rows_bench.py", "device": runs[1]["device"], "num_cus": runs[1]["num_cus"], "eps": EPS,
           "density": 0.67, "plan": "packed", "xtype": "bf16", "ytype": "bf16", "act": "relu2",
           "graph_steps": runs[0]["points"][0]["A"]["graph_steps"],
           "timing": "HIP events around windows of replays of a captured graph of graph_steps steps; median per step of "
                     "--reps windows; one child process per library, in the order parent, new, parent again",
           "variants": {"A": "the parent commit's library: sgemm_q8_group / sgemm_q8_glu with the norm (two samples)",
                        "B": "this tree, set_decode_rows_multi(64) on every plan: the row-tiled decode launch above 16 rows",
                        "C": "this tree at the default setting (16)"},
           "points": []}
    for a, b, c in zip(*(r["points"] for r in runs)):
        key = lambda p: (p["call"], p["K"], p["cols"], p["M"])
        assert key(a) == key(b) == key(c)
        assert a["A_sha256"] == b["B_sha256"] == b["C_sha256"] == c["A_sha256"], f"the variants' bytes differ at {key(a)}"
        a0, a1 = 1e3 * a["A"]["graph_ms"], 1e3 * c["A"]["graph_ms"]
        bu, cu = 1e3 * b["B"]["graph_ms"], 1e3 * b["C"]["graph_ms"]
        p = {"call": a["call"], "K": a["K"], "cols": a["cols"], "M": a["M"], "route_B": b["route_B"],
             "launch_B": b["launch_B"], "A_us": [a0, a1], "B_us": bu, "C_us": cu, "bits_equal": True,
             "spread": abs(a1 - a0) / a0, "A_over_B": 0.5 * (a0 + a1) / bu, "B_beats_both": bool(bu < min(a0, a1))}
        p["B_loses"] = bool(bu > max(a0, a1))
        p["C_within_spread"] = bool(min(a0, a1) * (1 - p["spread"]) <= cu <= max(a0, a1) * (1 + p["spread"]))
        res["points"].append(p)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    for p in res["points"]:
        verdict = "wins" if p["B_beats_both"] else "LOSES" if p["B_loses"] else "level"
        print(f"{p['call']:5s} K={p['K']} cols={'+'.join(map(str, p['cols']))} M={p['M']:3d} {p['route_B']:6s} "
              f"rt,t,wgs={p['launch_B']} | us/step: (A) {p['A_us'][0]:8.2f} {p['A_us'][1]:8.2f} | (B) {p['B_us']:8.2f} | "
              f"(C) {p['C_us']:8.2f}{'' if p['C_within_spread'] else ' !'} | spread {100 * p['spread']:4.1f}% "
              f"A/B x{p['A_over_B']:.2f} {verdict}")


if __name__ == "__main__":
    main()
