# A/B and diagnostic variant builds of libtcsc_amd.so (not part of the
# product build).  Run from the package directory so the product Makefile's
# variables and object rules apply:
#
#   make -C sparse-matrix-multiplication-benchmark_amd -f ../tools/ab.mk lib/abl/libtcsc_amd_pfs0.so
#
# Every target writes under lib/abl, lib/geo or lib/wid, which .gpurunignore
# keeps out of GPU pushes; an A/B session lists the builds it needs in its
# own gpurun command (tools/ab.sh) after removing them from .gpurunignore.
include Makefile

# A variant recompiles one or a few of the product's objects with its own
# macros and links them with the rest of the product's $(OBJS), so a file
# added to the library reaches every variant:
#   $(call ab_rest,<product objects replaced>)              the other objects (prerequisites)
#   $(call ab_link,<product objects replaced>,<their replacements>)
# K_OBJ: the gather kernels alone.  KA_OBJS: also the two C-ABI files, for
# variants whose macros change constants of tcsc_internal.h that the host
# code reads (plan layout, tcsc::kTM).
K_OBJ   := $(OBJ)/tcsc_kernels.o
KA_OBJS := $(K_OBJ) $(OBJ)/tcsc_api.o $(OBJ)/tcsc_host.o
ab_rest  = $(filter-out $(1),$(OBJS))
ab_link  = $(HIPCC) $(HIPFLAGS) -shared -o $@ $(2) $(call ab_rest,$(1)) -lpthread -L$(ROCM)/lib -lrocblas -Wl,-rpath,$(ROCM)/lib
# the two C-ABI files with the macros $(1) into $(2)_api.o and $(2)_host.o
ab_abi   = $(HIPCC) $(HIPFLAGS) $(1) -c $(SRC)/tcsc_api.cpp -o $(2)_api.o && \
           $(HIPCC) -x c++ $(CXXFLAGS) $(1) -c $(SRC)/tcsc_host.cpp -o $(2)_host.o

# Timing-only ablation builds of the gather loop (tools/gen_gather_asm.py):
# lib/abl/libtcsc_amd_abl<N>.so, loaded via TCSC_AMD_LIB=... (results wrong).
ABLS := 1 3 4 5 6
ablation: $(foreach a,$(ABLS),lib/abl/libtcsc_amd_abl$(a).so)

lib/abl/libtcsc_amd_abl%.so: $(SRC)/tcsc_kernels.hip $(call ab_rest,$(K_OBJ)) $(HDRS) $(SRC)/gather_asm.inc
	@mkdir -p lib/abl $(OBJ)/abl
	$(HIPCC) $(HIPFLAGS) -DTCSC_ABLATION=$* -c $(SRC)/tcsc_kernels.hip -o $(OBJ)/abl/k$*.o
	$(call ab_link,$(K_OBJ),$(OBJ)/abl/k$*.o)

# diagnostic build: s_memtime stamps of the chunk loop's waits written into Y
lib/abl/libtcsc_amd_stamps.so: $(SRC)/tcsc_kernels.hip $(call ab_rest,$(K_OBJ)) $(HDRS) $(SRC)/gather_asm.inc
	@mkdir -p lib/abl $(OBJ)/abl
	$(HIPCC) $(HIPFLAGS) -DTCSC_STAMPS -c $(SRC)/tcsc_kernels.hip -o $(OBJ)/abl/k_stamps.o
	$(call ab_link,$(K_OBJ),$(OBJ)/abl/k_stamps.o)

# diagnostic build: per-interval, per-wave timeline of the chunk loop written into Y (tools/trace.py)
lib/abl/libtcsc_amd_trace.so: $(SRC)/tcsc_kernels.hip $(call ab_rest,$(K_OBJ)) $(HDRS) $(SRC)/gather_asm.inc
	@mkdir -p lib/abl $(OBJ)/abl
	$(HIPCC) $(HIPFLAGS) -DTCSC_TRACE -c $(SRC)/tcsc_kernels.hip -o $(OBJ)/abl/k_trace.o
	$(call ab_link,$(K_OBJ),$(OBJ)/abl/k_trace.o)

# staging variants (A/B): lib/abl/libtcsc_amd_dma<waves>_<early>.so
lib/abl/libtcsc_amd_dma%.so: $(SRC)/tcsc_kernels.hip $(call ab_rest,$(K_OBJ)) $(HDRS) $(SRC)/gather_asm.inc
	@mkdir -p lib/abl $(OBJ)/abl
	$(HIPCC) $(HIPFLAGS) -DTCSC_DMA_WAVES=$(word 1,$(subst _, ,$*)) -DTCSC_DMA_EARLY=$(word 2,$(subst _, ,$*)) -c $(SRC)/tcsc_kernels.hip -o $(OBJ)/abl/k_dma$*.o
	$(call ab_link,$(K_OBJ),$(OBJ)/abl/k_dma$*.o)

# decode-kernel variants (A/B): lib/abl/libtcsc_amd_dec<waves>_<tiles>.so, waves per
# workgroup and column tiles per workgroup (0 = the product's rule); the same results, other timings
lib/abl/libtcsc_amd_dec%.so: $(SRC)/tcsc_decode.hip $(call ab_rest,$(OBJ)/tcsc_decode.o) $(HDRS)
	@mkdir -p lib/abl $(OBJ)/abl
	$(HIPCC) $(HIPFLAGS) -DTCSC_DEC_WAVES=$(word 1,$(subst _, ,$*)) -DTCSC_DEC_TILES=$(word 2,$(subst _, ,$*)) -c $(SRC)/tcsc_decode.hip -o $(OBJ)/abl/dec$*.o
	$(call ab_link,$(OBJ)/tcsc_decode.o,$(OBJ)/abl/dec$*.o)

# the row-tiled decode kernel's column tiles (A/B): lib/abl/libtcsc_amd_decr<tiles>.so, column tiles
# per workgroup of k_decode8r (capped at 8 / row tiles; 0 = the product's rule); the same results, other timings
lib/abl/libtcsc_amd_decr%.so: $(SRC)/tcsc_decode.hip $(call ab_rest,$(OBJ)/tcsc_decode.o) $(HDRS)
	@mkdir -p lib/abl $(OBJ)/abl
	$(HIPCC) $(HIPFLAGS) -DTCSC_DECR_TILES=$* -c $(SRC)/tcsc_decode.hip -o $(OBJ)/abl/decr$*.o
	$(call ab_link,$(OBJ)/tcsc_decode.o,$(OBJ)/abl/decr$*.o)

# the same without the X staging (gather cost alone): lib/abl/libtcsc_amd_abl<N>_nd.so
ablation-nodma: $(foreach a,0 1 3 4 5,lib/abl/libtcsc_amd_abl$(a)_nd.so)

lib/abl/libtcsc_amd_abl%_nd.so: $(SRC)/tcsc_kernels.hip $(call ab_rest,$(K_OBJ)) $(HDRS) $(SRC)/gather_asm.inc
	@mkdir -p lib/abl $(OBJ)/abl
	$(HIPCC) $(HIPFLAGS) -DTCSC_ABLATION=$* -DTCSC_NODMA -c $(SRC)/tcsc_kernels.hip -o $(OBJ)/abl/k$*_nd.o
	$(call ab_link,$(K_OBJ),$(OBJ)/abl/k$*_nd.o)

# Gather-geometry variants: lib/geo/libtcsc_amd_w<W>_cw<CW>_b<B>_c<CAP>_tk<TK>_nb<NBUF>[_d<D>].so
# (waves per workgroup, columns per wave, batch, SGPR stream capacity, K rows
# per chunk, LDS ring buffers, batches in flight; the VGPR budget per wave follows from W:
# 512 / (W/4)).  Plan and kernel are built from the same constants.
GEOS := w16_cw16_b4_c16_tk48_nb3 w16_cw16_b4_c32_tk48_nb3 w12_cw24_b4_c32_tk48_nb3 w16_cw16_b4_c24_tk64_nb2
geometry: $(foreach g,$(GEOS),lib/geo/libtcsc_amd_$(g).so)

geo_f = $(patsubst $(2)%,%,$(word $(3),$(subst _, ,$(1))))
geo_budget = $(shell echo $$(( 512 / ($(call geo_f,$(1),w,1) / 4) / 8 * 8 )))
geo_defs = -DTCSC_WAVES=$(call geo_f,$(1),w,1) -DTCSC_CW=$(call geo_f,$(1),cw,2) -DTCSC_BATCH=$(call geo_f,$(1),b,3) \
           -DTCSC_TK=$(call geo_f,$(1),tk,5) -DTCSC_NBUF=$(call geo_f,$(1),nb,6)

$(OBJ)/geo/gather_%.inc: ../tools/gen_gather_asm.py
	@mkdir -p $(OBJ)/geo
	python3 ../tools/gen_gather_asm.py --cw $(call geo_f,$*,cw,2) --batch $(call geo_f,$*,b,3) \
	    --cap $(call geo_f,$*,c,4) --budget $(call geo_budget,$*) --depth $(or $(call geo_f,$*,d,7),1) --touch $(or $(patsubst t%,%,$(filter t%,$(word 8,$(subst _, ,$*)))),0) -o $@ > /dev/null

lib/geo/libtcsc_amd_%.so: $(OBJ)/geo/gather_%.inc $(SRC)/tcsc_kernels.hip $(SRC)/tcsc_api.cpp $(SRC)/tcsc_host.cpp $(HDRS) $(call ab_rest,$(KA_OBJS))
	@mkdir -p lib/geo
	$(HIPCC) $(HIPFLAGS) $(call geo_defs,$*) -DTCSC_GATHER_INC='"$(abspath $(OBJ)/geo/gather_$*.inc)"' \
	    -c $(SRC)/tcsc_kernels.hip -o $(OBJ)/geo/k_$*.o
	$(call ab_abi,$(call geo_defs,$*),$(OBJ)/geo/a_$*)
	$(call ab_link,$(KA_OBJS),$(OBJ)/geo/k_$*.o $(OBJ)/geo/a_$*_api.o $(OBJ)/geo/a_$*_host.o)

.SECONDARY:
.PHONY: ablation ablation-nodma geometry
# Per-rank column widths (TCSC_WIDTHS, tcsc_internal.h): lib/wid/libtcsc_amd_wd<A>_<B>_<C>_<D>.so,
# waves of age rank r own <r-th> columns each, accumulators for the widest.
comma := ,
wid_cw = $(shell printf '%s\n' $(subst _, ,$(1)) | sort -n | tail -n 1)
wid_defs = -DTCSC_CW=$(call wid_cw,$(1)) -DTCSC_WIDTHS=$(subst _,$(comma),$(1))
$(OBJ)/wid/gather_cw%.inc: ../tools/gen_gather_asm.py
	@mkdir -p $(OBJ)/wid
	python3 ../tools/gen_gather_asm.py --cw $* -o $@ > /dev/null

.SECONDEXPANSION:
lib/wid/libtcsc_amd_wd%.so: $(OBJ)/wid/gather_cw$$(call wid_cw,$$*).inc $(SRC)/tcsc_kernels.hip $(SRC)/tcsc_api.cpp $(SRC)/tcsc_host.cpp $(HDRS) $(call ab_rest,$(KA_OBJS))
	@mkdir -p lib/wid $(OBJ)/wid
	$(HIPCC) $(HIPFLAGS) $(call wid_defs,$*) \
	    -DTCSC_GATHER_INC='"$(abspath $(OBJ)/wid/gather_cw$(call wid_cw,$*).inc)"' -c $(SRC)/tcsc_kernels.hip -o $(OBJ)/wid/k_$*.o
	$(call ab_abi,$(call wid_defs,$*),$(OBJ)/wid/a_$*)
	$(call ab_link,$(KA_OBJS),$(OBJ)/wid/k_$*.o $(OBJ)/wid/a_$*_api.o $(OBJ)/wid/a_$*_host.o)

# stream-prefetch on/off (A/B): lib/abl/libtcsc_amd_pfs<0|1>.so (distance and width: TCSC_PF_DIST / TCSC_PF_LINES)
lib/abl/libtcsc_amd_pfs%.so: $(SRC)/tcsc_kernels.hip $(SRC)/tcsc_api.cpp $(SRC)/tcsc_host.cpp $(call ab_rest,$(KA_OBJS)) $(HDRS) $(SRC)/gather_asm.inc
	@mkdir -p lib/abl $(OBJ)/abl
	$(HIPCC) $(HIPFLAGS) -DTCSC_PF_S=$* -c $(SRC)/tcsc_kernels.hip -o $(OBJ)/abl/k_pfs$*.o
	$(call ab_abi,-DTCSC_PF_S=$*,$(OBJ)/abl/a_pfs$*)
	$(call ab_link,$(KA_OBJS),$(OBJ)/abl/k_pfs$*.o $(OBJ)/abl/a_pfs$*_api.o $(OBJ)/abl/a_pfs$*_host.o)

# k_fused (the persistent gather with in-kernel X^T production, round 4) left the
# library in round 5: the kernel, its launcher and its A/B variants are at commit
# 815156e (csrc/tcsc_kernels.hip k_fused, tools/ab.mk lib/abl/libtcsc_amd_f<v>.so).

# 4-byte entry cost proxy: the generated loop rebuilds the +-1
# multiplier from a sign bit with 2 SALU per entry (gen_gather_asm.py --sgn 1);
# results unchanged.  lib/abl/libtcsc_amd_sgn1.so
$(OBJ)/abl/gather_sgn%.inc: ../tools/gen_gather_asm.py
	@mkdir -p $(OBJ)/abl
	python3 ../tools/gen_gather_asm.py --sgn $* -o $@ > /dev/null

lib/abl/libtcsc_amd_sgn%.so: $(OBJ)/abl/gather_sgn%.inc $(SRC)/tcsc_kernels.hip $(call ab_rest,$(K_OBJ)) $(HDRS)
	@mkdir -p lib/abl $(OBJ)/abl
	$(HIPCC) $(HIPFLAGS) -DTCSC_GATHER_INC='"$(abspath $(OBJ)/abl/gather_sgn$*.inc)"' -c $(SRC)/tcsc_kernels.hip -o $(OBJ)/abl/k_sgn$*.o
	$(call ab_link,$(K_OBJ),$(OBJ)/abl/k_sgn$*.o)

# split-K combine slab loads: nontemporal (default) or cached (rnt0)
lib/abl/libtcsc_amd_rnt%.so: $(SRC)/tcsc_kernels.hip $(call ab_rest,$(K_OBJ)) $(HDRS) $(SRC)/gather_asm.inc
	@mkdir -p lib/abl $(OBJ)/abl
	$(HIPCC) $(HIPFLAGS) -DTCSC_REDUCE_NT=$* -c $(SRC)/tcsc_kernels.hip -o $(OBJ)/abl/k_rnt$*.o
	$(call ab_link,$(K_OBJ),$(OBJ)/abl/k_rnt$*.o)

# Direct X staging (A/B, round 5, DESIGN.md §4 k_transpose): the variant and its target
# lib/abl/libtcsc_amd_xs1.so are at commit b07f36f (measured slower, removed).
