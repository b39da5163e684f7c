"""bench.py without --full on one GPU: the contract line of a plain run
(--steps honoured, ms_per_step consistent with value, none of --full's
lines) and --dump-outputs: DIR/Y.npy holds, in float32, the documented row
sample of what the timed path computed in its last step -- recomputed here
in-process from the same seeded inputs and compared bit for bit.  The shape
(cfg 2 stretched to M=2048, N=8192: a 64-MiB Y) is the smallest that makes
the dump sample rows instead of writing them all."""
import dataclasses
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import tcsc_amd
from conftest import ROOT
from tcsc_amd import workloads

pytestmark = pytest.mark.gpu

FULL_ONLY = ("validation", "dense_baseline", "bcsr", "host_api", "reference_order", "graph", "other_configs",
             "cpu_baseline", "alt_shard")


def test_plain_run_is_headline_only_and_dumps_last_output(tmp_path):
    import torch

    tcsc_amd.require_gpu()
    out = tmp_path / "dump"
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
           "--config", "2", "--override", "M=2048,N=8192", "--dump-outputs", str(out)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=120, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    lines = [json.loads(x) for x in r.stdout.splitlines() if x.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    d = lines[0]
    assert d["steps"] == 3 and d["warmup"] == 1 and d["n_gpus"] == 1
    assert d["unit"] == "G-add-ops/s" and d["higher_is_better"] is True and d["dtype"] == "f32" and d["metric"]
    assert d["ms_per_step"] > 0
    cfg = dataclasses.replace(workloads.CONFIGS[2], M=2048, N=8192)
    per_step = workloads.add_ops(cfg.M, d["config"]["nnz_per_gpu"], cfg.N)
    assert d["value"] * 1e9 * d["ms_per_step"] * 1e-3 == pytest.approx(per_step, rel=1e-9)
    assert not [k for k in FULL_ONLY if k in d]
    assert "kernel_ms" not in d["roofline"] and "step_parts_ms" not in d["roofline"]

    assert sorted(os.listdir(out)) == ["Y.npy"]
    Yd = np.load(out / "Y.npy")
    rows = (48 << 20) // (4 * cfg.N)
    assert rows < cfg.M  # the sampled form of the dump
    assert Yd.dtype == np.float32 and Yd.shape == (rows, cfg.N) and d["outputs"]["shape"] == [rows, cfg.N]
    assert Yd.nbytes <= 64 << 20

    # the same step in this process: seeded inputs, W built on the device, one launch
    dev = torch.device("cuda:0")
    inp = workloads.make_device_inputs(cfg, 0, cfg.N, dev)
    csp = torch.empty(cfg.N + 1, dtype=torch.int32, device=dev)
    csn = torch.empty(cfg.N + 1, dtype=torch.int32, device=dev)
    npos, nneg = tcsc_amd.gpu_from_dense(inp["Wd"], cfg.K, cfg.N, csp, csn)
    assert npos + nneg == d["config"]["nnz_per_gpu"]
    rip = torch.empty(max(npos, 1), dtype=torch.int32, device=dev)
    rin = torch.empty(max(nneg, 1), dtype=torch.int32, device=dev)
    tcsc_amd.gpu_from_dense(inp["Wd"], cfg.K, cfg.N, csp, csn, rip, rin)
    plan = tcsc_amd.Plan.from_device(cfg.K, cfg.N, csp, csn, rip, rin)
    plan.reserve(cfg.M)
    Y = torch.empty((cfg.M, cfg.N), device=dev)
    plan.sgemm(inp["X"], inp["B"], Y, cfg.M, cfg.N, cfg.variant, 0.2)
    torch.cuda.synchronize()
    idx = np.sort(np.random.default_rng(0).choice(cfg.M, rows, replace=False))
    want = Y[torch.from_numpy(idx).to(dev)].cpu().numpy()
    plan.destroy()
    np.testing.assert_array_equal(Yd.view(np.uint32), want.view(np.uint32))
