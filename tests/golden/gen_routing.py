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

    python tests/golden/gen_routing.py --knobs

records the forced and special routes into tests/golden/routing_knobs.json (a GPU again; it sets and
clears the knobs itself).  For each plan of KNOB_PLANS, as a fast-order, a reference-order and a
transposed plan, created and reserved for 512 rows under each TCSC_SLICES of KNOB_SLICES (the third
plan also under TCSC_PATH=gather and TCSC_GEO=22: no MFMA image, the wide streams), and then for every TCSC_GEO of KNOB_GEO
and TCSC_COMBINE of KNOB_COMBINE, queries only: launch_info, launch_geometry (the error text where
TCSC_GEO=22 is refused), the combine mode and workspace(M) of each path, for every M of KNOB_MS.
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


# ---- the forced and special routes: --knobs -> routing_knobs.json -------------
KNOB_TABLE = os.path.join(HERE, "routing_knobs.json")
# name: K, N, density, environment at creation and reserve.  The first is the shape whose split-K slabs peak
# inside the reserved range, the second has the MFMA image, the third is tests/test_gpu_wide.py's, made as
# there: without the MFMA image its density would earn it, and with the wide streams.
KNOB_PLANS = {"slabs": (512, 4096, 0.02, {}), "image": (1024, 512, 0.5, {}),
              "wide": (120, 500, 0.08, {"TCSC_PATH": "gather", "TCSC_GEO": "22"})}
KNOB_KINDS = ("fast", "reference", "transposed")
KNOB_MS = (1, 4, 5, 64, 200, 339, 512)
KNOB_RESERVE_M = 512
KNOB_SLICES = (None, "1", "2", "4")
KNOB_GEO = (None, "16", "22")
KNOB_COMBINE = (None, "0", "1")
KNOB_ENV = ("TCSC_SLICES", "TCSC_GEO", "TCSC_COMBINE")


def set_knobs(**env):
    """Sets each environment knob given to its value, or clears it for None."""
    for k, v in env.items():
        os.environ.pop(k, None)
        if v is not None:
            os.environ[k] = v


def knob_key(name, kind, slices, geo, combine):
    return f"{name}-{kind}-slices_{slices}-geo_{geo}-combine_{combine}".replace("None", "unset")


def knob_plan(tcsc_amd, W, kind):
    if kind == "transposed":
        return tcsc_amd.Plan.transposed(W)
    tcsc_amd.set_order("reference" if kind == "reference" else "fast")
    try:
        return tcsc_amd.Plan(W)
    finally:
        tcsc_amd.set_order("fast")


def record_knobs(tcsc_amd, name):
    """{key: {"reserved": bytes, "rows": [[M, path, slices, geometry or its error, combine mode, workspace auto,
    gather, mfma, small], ...]}} for every kind of plan and knob setting of one entry of KNOB_PLANS.  Leaves
    the knobs cleared."""
    import ctypes as C

    K, N, density, made_under = KNOB_PLANS[name]
    L = tcsc_amd.lib()
    out = {}
    W = tcsc_amd.TcscMatrix.from_dense(ternary(K, N, density))
    try:
        for kind in KNOB_KINDS:
            for slices in KNOB_SLICES:
                set_knobs(TCSC_SLICES=slices, TCSC_GEO=None, TCSC_COMBINE=None)
                set_knobs(**made_under)
                plan = knob_plan(tcsc_amd, W, kind)
                plan.reserve(KNOB_RESERVE_M)
                set_knobs(TCSC_PATH=None)
                for geo in KNOB_GEO:
                    for combine in KNOB_COMBINE:
                        set_knobs(TCSC_GEO=geo, TCSC_COMBINE=combine)
                        rows = []
                        for M in KNOB_MS:
                            path, s = plan.launch_info(M)
                            try:
                                g = plan.launch_geometry(M)
                            except tcsc_amd.TcscError:
                                g = tcsc_amd.last_error()
                            mode = C.c_int()
                            assert L.tcsc_gpu_launch_combine(plan.handle, M, C.byref(mode)) == 0
                            rows.append([M, PATH_CODE[path], s, g, mode.value]
                                        + [plan.workspace(M, p)[0] for p in (None, "gather", "mfma", "small")])
                        out[knob_key(name, kind, slices, geo, combine)] = {
                            "reserved": plan.workspace(KNOB_RESERVE_M)[1], "rows": rows}
                plan.destroy()
    finally:
        set_knobs(TCSC_PATH=None, **{k: None for k in KNOB_ENV})
        W.free()
    return out


def knob_changes(table):
    """How many (plan, kind, other knobs, M) answers each knob, and the reference order, changes against the
    same entry with that knob unset (the fast order)."""
    changed = {"TCSC_SLICES": 0, "TCSC_GEO": 0, "TCSC_COMBINE": 0, "reference": 0}
    for name in KNOB_PLANS:
        for kind in KNOB_KINDS:
            for s in KNOB_SLICES:
                for g in KNOB_GEO:
                    for c in KNOB_COMBINE:
                        e = table[knob_key(name, kind, s, g, c)]
                        for knob, base in (("TCSC_SLICES", (name, kind, None, g, c)), ("TCSC_GEO", (name, kind, s, None, c)),
                                           ("TCSC_COMBINE", (name, kind, s, g, None)), ("reference", (name, "fast", s, g, c))):
                            if knob == "reference" and kind != "reference":
                                continue
                            b = table[knob_key(*base)]
                            changed[knob] += sum(x != y for x, y in zip(e["rows"], b["rows"])) + (e["reserved"] != b["reserved"])
    return changed


def main_knobs():
    set_ = [k for k in KNOBS + KNOB_ENV if k in os.environ]
    if set_:
        sys.exit(f"unset {', '.join(sorted(set(set_)))} first: the generator sets the knobs itself")
    sys.path.insert(0, os.path.join(ROOT, "sparse-matrix-multiplication-benchmark_amd"))
    import tcsc_amd

    tcsc_amd.require_gpu()
    table = {}
    for name in KNOB_PLANS:
        table.update(record_knobs(tcsc_amd, name))
    # a knob that never changed an answer is not pinned by the table
    changed = knob_changes(table)
    for knob, n in changed.items():
        assert n > 0, f"{knob} changed no answer in the table"
    refused = sum(isinstance(r[3], str) for e in table.values() for r in e["rows"])
    wide = sum(r[3] == 22 for e in table.values() for r in e["rows"])
    assert refused > 0 and wide > 0, f"TCSC_GEO=22: {refused} refusals and {wide} wide launches in the table"
    modes = {r[4] for e in table.values() for r in e["rows"]}
    assert len(modes) > 1, f"only combine modes {sorted(modes)} in the table"
    with open(KNOB_TABLE, "w") as f:
        f.write("{\n" + ",\n".join(f' "{k}": {json.dumps(v, separators=(",", ":"))}' for k, v in table.items())
                + "\n}\n")
    print(f"{len(table)} entries x {len(KNOB_MS)} M -> {KNOB_TABLE} ({os.path.getsize(KNOB_TABLE)} bytes); answers changed: "
          f"{changed}; {refused} refusals, {wide} wide, combine modes {sorted(modes)}")


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
    if sys.argv[1:] == ["--knobs"]:
        return main_knobs()
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
