"""What the three cost models decide, recorded: tests/golden/routing_table.json.

Run once on a gfx950 GPU, at the commit whose routing is to be held, with none
of TCSC_PATH, TCSC_SLICES, TCSC_MFMA_WGS, TCSC_SMALL_M and TCSC_GEO set:

    python tests/golden/gen_routing.py

For every (K, N) of SHAPES and density of DENSITIES it builds a fast-order plan
of a random ternary W (fixed seed), once as it is and once with enable_i8(),
reserves 4096 rows and records, for every M of MS:
    launch_info, launch_info_bf16, launch_info_i8   (path, K slices) each
    workspace(M) for auto, 'gather', 'mfma', 'small' (bytes wanted)
    launch_geometry(M)
and once per plan the bytes reserve(4096) holds.  tests/test_gpu_workspace.py
rebuilds the same plans through record() and compares entry by entry.

    python tests/golden/gen_routing.py --bound

needs no GPU: tcsc_gpu_workspace_bound_i8 over the sweep of tests/test_i8_api.py ->
tests/golden/routing/i8_workspace_bound.npz, which that file's CPU test compares with.
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
TABLE = os.path.join(HERE, "routing_table.json")

SHAPES = ((256, 256), (1024, 1024), (2048, 2048), (700, 2048))
DENSITIES = (0.02, 0.05, 0.07, 0.1, 0.2, 0.5)
MS = (1, 2, 4, 5, 8, 16, 63, 64, 65, 128, 200, 256, 257, 512, 1024, 2048, 4096)
RESERVE_M = 4096
SEED = 20261020
KNOBS = ("TCSC_PATH", "TCSC_SLICES", "TCSC_MFMA_WGS", "TCSC_SMALL_M", "TCSC_GEO")
PATH_CODE = {"gather": 0, "mfma": 2, "small": 3}


def ternary(K, N, density):
    """K x N of +1 / -1 / 0, about density * K * N nonzeros, half of each sign."""
    r = np.random.default_rng([SEED, K, N, int(round(density * 1000))]).random((K, N))
    return np.where(r < density / 2, 1.0, np.where(r < density, -1.0, 0.0)).astype(np.float32)


def key(K, N, density, i8):
    return f"K{K}-N{N}-d{density}-{'i8' if i8 else 'plain'}"


def record(tcsc_amd, K, N):
    """{key: {"reserved": bytes, "rows": [[M, f32 path, slices, bf16 path, slices, i8 path, slices,
    workspace auto, gather, mfma, small, geometry], ...]}} for every density of DENSITIES, with and without the
    int8 image."""
    out = {}
    for density in DENSITIES:
        W = tcsc_amd.TcscMatrix.from_dense(ternary(K, N, density))
        for i8 in (False, True):
            plan = tcsc_amd.Plan(W)
            if i8:
                plan.enable_i8()
            plan.reserve(RESERVE_M)
            rows = []
            for M in MS:
                row = [M]
                for info in (plan.launch_info, plan.launch_info_bf16, plan.launch_info_i8):
                    path, slices = info(M)
                    row += [PATH_CODE[path], slices]
                row += [plan.workspace(M, p)[0] for p in (None, "gather", "mfma", "small")]
                row.append(plan.launch_geometry(M))
                rows.append(row)
            out[key(K, N, density, i8)] = {"reserved": plan.workspace(RESERVE_M)[1], "rows": rows}
            plan.destroy()
        W.free()
    return out


# tcsc_gpu_workspace_bound_i8 needs no plan and no device: --bound records it over the sweep of
# tests/test_i8_api.py, for each $TCSC_MFMA_WGS that test sets ("" = unset), into routing/i8_workspace_bound.npz
# (a folder of its own: every .npz next to this file is a golden GEMM case)
BOUND = os.path.join(HERE, "routing", "i8_workspace_bound.npz")
BOUND_MS = (1, 4, 5, 17, 63, 64, 65, 96, 127, 128, 129, 200, 256, 257, 1000, 2048, 4097)
BOUND_KS = (1, 63, 64, 65, 127, 128, 129, 300, 511, 512, 513, 1023, 1100, 2047, 2048, 2049, 3000, 4095, 8192, 8193,
            16384, 20000, 100003)
BOUND_NS = (1, 64, 130, 255, 256, 257, 300, 512, 600, 1024, 4096, 8192, 16384)
BOUND_WGS = ("", "0", "64", "4096")


def bound_sweep(lib):
    """int64 [M][K][N][2] over the sweep: (int8 bytes, fp32 bytes) under the current environment."""
    import ctypes as C

    out = np.zeros((len(BOUND_MS), len(BOUND_KS), len(BOUND_NS), 2), np.int64)
    i8, f32 = C.c_size_t(), C.c_size_t()
    for a, M in enumerate(BOUND_MS):
        for b, K in enumerate(BOUND_KS):
            for c, N in enumerate(BOUND_NS):
                assert lib.tcsc_gpu_workspace_bound_i8(M, K, N, C.byref(i8), C.byref(f32)) == 0
                out[a, b, c] = i8.value, f32.value
    return out


def main_bound():
    sys.path.insert(0, os.path.join(ROOT, "sparse-matrix-multiplication-benchmark_amd"))
    import tcsc_amd

    lib = tcsc_amd.lib()
    tables = {}
    for wgs in BOUND_WGS:
        os.environ.pop("TCSC_MFMA_WGS", None)
        if wgs:
            os.environ["TCSC_MFMA_WGS"] = wgs
        tables["wgs_" + (wgs or "unset")] = bound_sweep(lib)
    os.environ.pop("TCSC_MFMA_WGS", None)
    os.makedirs(os.path.dirname(BOUND), exist_ok=True)
    np.savez_compressed(BOUND, Ms=np.array(BOUND_MS), Ks=np.array(BOUND_KS), Ns=np.array(BOUND_NS), **tables)
    print(f"{len(tables)} sweeps of {tables['wgs_unset'].size // 2} shapes -> {BOUND} ({os.path.getsize(BOUND)} bytes)")


def main():
    if sys.argv[1:] == ["--bound"]:
        return main_bound()
    set_ = [k for k in KNOBS if k in os.environ]
    if set_:
        sys.exit(f"unset {', '.join(set_)} first: the table records the default routing")
    sys.path.insert(0, os.path.join(ROOT, "sparse-matrix-multiplication-benchmark_amd"))
    import tcsc_amd

    tcsc_amd.require_gpu()
    table = {}
    for K, N in SHAPES:
        table.update(record(tcsc_amd, K, N))
    # the table is only a judge if it sees both answers of every model and a disagreement between them
    answers = [set(), set(), set()]
    disagree = 0
    for e in table.values():
        for row in e["rows"]:
            paths = row[1:7:2]
            for a, p in zip(answers, paths):
                a.add(p)
            disagree += len(set(paths)) > 1
    for name, a in zip(("fp32", "bf16", "int8"), answers):
        assert {PATH_CODE["gather"], PATH_CODE["mfma"]} <= a, f"{name}: only paths {sorted(a)} in the table"
    assert disagree > 0, "no (plan, M) where the three types take different paths"
    with open(TABLE, "w") as f:
        f.write("{\n" + ",\n".join(f' "{k}": {json.dumps(v, separators=(",", ":"))}' for k, v in table.items())
                + "\n}\n")
    print(f"{len(table)} plans x {len(MS)} M -> {TABLE} ({os.path.getsize(TABLE)} bytes); "
          f"{disagree} (plan, M) where the types disagree")


if __name__ == "__main__":
    main()
