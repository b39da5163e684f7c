"""The 22-column geometry of k_stream on the CPU: its generated loop and the
rounds model that chooses it (DESIGN.md §4 "Two geometries").

The loop (csrc/gather_asm_w22.inc, tools/gen_gather_asm.py --cw 22 --batch 3
--cap 30 --prefix TCSCW) runs through the instruction interpreter of
tests/test_gather_gen.py for every stream length from 0 to 2 * cap + batch:
each entry read once and FMA'd twice, nothing past the end, every path
leaving the pointer at the next header.  wide_pays is checked on a table of
shapes through the library's C entry point (pure host arithmetic).
"""
import os

import pytest

import test_gather_gen as tg
import tcsc_amd

gen = tg.gen
WIDE = dict(cw=22, batch=3, cap=30)


def test_wide_loop_gathers_each_entry_once():
    g = gen.Geo(budget=128, depth=1, touch=0, tail=1, pf=0, **WIDE)
    lines = gen.generate_tail(g)
    for n in range(2 * g.cap + g.batch + 1):
        reads, fmas = tg.simulate(g, lines, n // g.batch, n % g.batch)
        assert sorted(reads) == list(range(n)) and set(reads.values()) <= {1}, n
        assert sorted(fmas) == list(range(n)) and set(fmas.values()) <= {2}, n


def test_wide_register_map():
    """88 accumulators + 24 X registers leave v0..v15 to the kernel around the
    loop; every slot index 4 * slot (slot < 22) stays inside the accumulators;
    the asm operands cover them in tuples the compiler can pin."""
    g = gen.Geo(budget=128, depth=1, touch=0, tail=1, pf=0, **WIDE)
    assert (g.acc, g.xbase, g.nx) == (16, 104, 24)
    assert g.acc + 4 * g.cw == g.xbase and g.xbase + g.nx == 128
    widths, mixed = gen.acc_vectors(g)
    assert mixed and widths == [32, 32, 16, 8] and sum(widths) == 4 * g.cw
    # the 16-column loop keeps its equal vectors
    assert gen.acc_vectors(gen.Geo(16, 4, 24, 128)) == ([32, 32], False)


def test_batch_4_does_not_fit_22_columns():
    """88 + 32 X registers leave 8 VGPRs for everything else: the generator
    refuses (it wants 12), which is why the shipped wide loop is batch 3."""
    with pytest.raises(AssertionError):
        gen.Geo(22, 4, 24, 128)


def test_shipped_wide_include_matches_generator(tmp_path):
    out = tmp_path / "gather_asm_w22.inc"
    gen.write_inc(str(out), gen.Geo(budget=128, depth=1, touch=0, tail=1, **WIDE), "TCSCW")
    with open(os.path.join(tg.ROOT, "sparse-matrix-multiplication-benchmark_amd", "csrc", "gather_asm_w22.inc")) as f:
        text = f.read()
    assert text == out.read_text()
    # no macro of the 16-column include is redefined
    with open(os.path.join(tg.ROOT, "sparse-matrix-multiplication-benchmark_amd", "csrc", "gather_asm.inc")) as f:
        narrow = {ln.split()[1].split("(")[0] for ln in f if ln.startswith("#define ")}
    wide = {ln.split()[1].split("(")[0] for ln in text.splitlines() if ln.startswith("#define ")}
    assert wide and not (wide & narrow)


# (M, ncols, CUs, pays): cfg 4 pays (1024 workgroups in 4 rounds against 752 in
# 3); cfg 2/3 (1024 x 4096), cfg 5 (2048 x 8192), one block of cfg 4 cut 8 ways
# (4096 x 2048) all fit one round either way, where wider workgroups only cost
PAYS = [(4096, 16384, 256, True), (1024, 4096, 256, False), (2048, 8192, 256, False), (4096, 2048, 256, False),
        (128, 256, 256, False), (0, 16384, 256, False), (4096, 0, 256, False), (4096, 16384, 0, False)]


@pytest.mark.parametrize("M,ncols,cus,pays", PAYS)
def test_wide_pays_table(M, ncols, cus, pays):
    tcsc_amd.build()
    assert bool(tcsc_amd.lib().tcsc_gpu_wide_pays(M, ncols, cus)) == pays
