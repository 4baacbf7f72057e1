# Builds libwdg_hip.so (gfx950 only) and the CPU oracle.  `python -c "import __graft_entry__ as g; g.build()"` calls this.
PKG      := when-do-gnns-help_amd
CSRC     := $(PKG)/csrc
HIPCC    ?= /opt/rocm/bin/hipcc
HIPFLAGS := --offload-arch=gfx950 -O3 -std=c++17 -fPIC -Iinclude -I$(CSRC) -Wall -Wno-unused-function -Wno-unused-value $(if $(STAMPS),-DWDG_STAMPS,) $(if $(DEPTH),-DWDG_PREFETCH_DEPTH=$(DEPTH),) $(EXTRA)
SRCS     := $(wildcard $(CSRC)/*.hip)
# link order: the units of the opt-in keep_best, learning-curve, AUC, sparse-first-layer, CSBM-H (synth_classes, qda), attention (gat, gat_scores) signed-attention (signed_att), polynomial-filter (poly_filter), two-hop pattern (two_hop), row top-k (topk_rows), GCNII layer (gcnii) and DropEdge (drop_edge) paths go LAST, so that every other kernel keeps the place in the library it had before
# they existed (the default paths are timed against the parent commit's build: DESIGN 4.20, 4.21)
LAST     := $(CSRC)/keep_best.hip $(CSRC)/confusion.hip $(CSRC)/xent_curve.hip $(CSRC)/auc.hip $(CSRC)/sparse_dense.hip $(CSRC)/synth_classes.hip $(CSRC)/qda.hip $(CSRC)/gat.hip $(CSRC)/gat_scores.hip $(CSRC)/signed_att.hip $(CSRC)/poly_filter.hip $(CSRC)/two_hop.hip $(CSRC)/topk_rows.hip $(CSRC)/gcnii.hip $(CSRC)/drop_edge.hip
# ... and behind them the neighbour sampler (neighbor_sample), on a line of its own: the list above ends where tests/test_abi_drop_edge.py reads it
LAST     += $(CSRC)/neighbor_sample.hip
# ... and behind it the neighbour maximum (neighbor_max), again on a line of its own
LAST     += $(CSRC)/neighbor_max.hip
# ... and behind every one of them the recurrence filter (recur_filter), in a list of its own: the lines above end where tests/test_abi_neighbor_max.py reads them
AFTER    := $(CSRC)/recur_filter.hip
# ... and behind that the neighbour moments (neighbor_moments), on a line of its own: the line above ends where tests/test_abi_recur_filter.py reads it
AFTER    += $(CSRC)/neighbor_moments.hip
SRCS     := $(filter-out $(LAST) $(AFTER),$(SRCS)) $(LAST) $(AFTER)
LINKFLAGS := --offload-arch=gfx950 -shared -fPIC
# per-file flags: the 32 steps of kernel_reg.hip's in-wave substitution (the solver's k2_factor_invert; the file holds the solver and
# nothing else) must unroll completely (their register indices and branch conditions are compile-time only then) - with the
# default budget the compiler peels 11 steps and rolls the rest
FLAGS_kernel_reg := -mllvm -pragma-unroll-threshold=200000
# (kernel_reg_large.hip factors its diagonal blocks with the same routine, csrc/kr_blocks.h)
FLAGS_kernel_reg_large := -mllvm -pragma-unroll-threshold=200000
# (kernel_reg_large_windows.hip IS kernel_reg_large.hip, compiled in its class-window form)
FLAGS_kernel_reg_large_windows := $(FLAGS_kernel_reg_large)
# gnb.hip reproduces numpy's fp32 sums bit for bit: no multiply-add may be fused (its source says so as well: #pragma clang fp contract(off))
FLAGS_gnb := -ffp-contract=off
# adam.hip's step is restated in numpy bit for bit: every multiply and add is its own rounded operation (the source says so as well)
FLAGS_adam := -ffp-contract=off
# acm_mix_packed.hip computes a replica's bits exactly as acm_mix.hip computes a job's: every multiply-add is written out (the source says so as well)
FLAGS_acm_mix_packed := -ffp-contract=off
# sparse_dense.hip's element is ONE fma chain, restated in numpy bit for bit: the fma is written out, nothing else is fused (the source says so as well)
FLAGS_sparse_dense := -ffp-contract=off
# qda.hip's fp64 discriminants are restated in numpy and the error counts compared for equality: every multiply and add is its own rounded operation (the source says so as well)
FLAGS_qda := -ffp-contract=off
# gat.hip's chains and sums are stated operation by operation in include/wdg.h: every fmaf is written out, nothing else is fused (the source says so as well)
FLAGS_gat := -ffp-contract=off
# gat_scores.hip's chains are stated in include/wdg.h and restated in numpy bit for bit: every fmaf is written out, nothing else is fused (the source says so as well)
FLAGS_gat_scores := -ffp-contract=off
# signed_att.hip's chains and sums are stated operation by operation in include/wdg.h, as gat.hip's are: every fmaf is written out, nothing else is fused
FLAGS_signed_att := -ffp-contract=off
# poly_filter.hip's chains, butterflies and fp64 sums are stated operation by operation in include/wdg.h: every fmaf is written out, nothing else is fused
FLAGS_poly_filter := -ffp-contract=off
# recur_filter.hip's hop is poly_filter.hip's row sum (csrc/filter_rows.h) and the recurrence's fmafs, stated in include/wdg.h: every fmaf is written out, nothing else is fused
FLAGS_recur_filter := -ffp-contract=off
# topk_rows.hip's key is ONE rounded product and its row norm an fmaf chain written out in include/wdg.h: nothing else is fused (the source says so as well)
FLAGS_topk_rows := -ffp-contract=off
# gcnii.hip's layer and its backward pass are stated operation by operation in include/wdg.h and restated in numpy bit for bit: every fmaf is written out, nothing else is fused
FLAGS_gcnii := -ffp-contract=off
# drop_edge.hip's aggregation is ONE fmaf chain per element, stated in include/wdg.h and restated in numpy bit for bit: the fmaf is written out, nothing else is fused
FLAGS_drop_edge := -ffp-contract=off
# neighbor_max.hip's backward pass is ONE fp32 add chain per element, stated in include/wdg.h and restated in numpy bit for bit: nothing is fused (the source says so as well)
FLAGS_neighbor_max := -ffp-contract=off
# neighbor_moments.hip's position chains, its centred second pass and its backward pass are stated operation by operation in include/wdg.h and restated in numpy bit for bit: every fmaf is written out, nothing else is fused
FLAGS_neighbor_moments := -ffp-contract=off
OBJS     := $(patsubst $(CSRC)/%.hip,build/%.o,$(SRCS))
LIB      := $(PKG)/lib/libwdg_hip.so

all: $(LIB) oracle

$(LIB): $(OBJS)
	@mkdir -p $(dir $@)
	$(HIPCC) $(LINKFLAGS) -o $@ $(OBJS)

# (the compiler's per-kernel resource report - registers, spills, scratch - is kept beside the object: tests/test_abi.py
# checks that no shipped kernel spills vector registers)
build/kernel_reg_large_windows.o: $(CSRC)/kernel_reg_large.hip
build/%.o: $(CSRC)/%.hip $(wildcard $(CSRC)/*.h) include/wdg.h
	@mkdir -p build
	$(HIPCC) $(HIPFLAGS) $(FLAGS_$*) -Rpass-analysis=kernel-resource-usage -c $< -o $@ 2> build/$*.rsrc || (cat build/$*.rsrc; exit 1)
	@grep -E "warning:|error:" build/$*.rsrc || true

# This file is the one place that knows how a unit is compiled.  Whatever else compiles one asks here:
#   make -s hipcc-line UNIT=spmm_quad      prints the compiler and the unit's options (tests/_device_code.py generates the device
#                                          code the ISA checks read with exactly this line + -S --cuda-device-only)
#   make variant UNIT=kernel_reg NAME=kr_prof VFLAGS=-DK2_PROFILE      (dev tools: scripts/dev/build_*_variant*.sh)
#                                          lib/variants/libwdg_hip_$(NAME).so = the shipped objects, UNIT's replaced by one compiled
#                                          with the unit's options + VFLAGS
hipcc-line:
	@echo $(HIPCC) $(HIPFLAGS) $(FLAGS_$(UNIT))

variant: $(OBJS)
	@mkdir -p build/variants $(PKG)/lib/variants
	$(HIPCC) $(HIPFLAGS) $(FLAGS_$(UNIT)) $(VFLAGS) -c $(CSRC)/$(UNIT).hip -o build/variants/$(UNIT)_$(NAME).o 2> build/variants/$(NAME).log
	$(HIPCC) $(LINKFLAGS) -o $(PKG)/lib/variants/libwdg_hip_$(NAME).so $(filter-out build/$(UNIT).o,$(OBJS)) build/variants/$(UNIT)_$(NAME).o
	@echo built $(PKG)/lib/variants/libwdg_hip_$(NAME).so

oracle: oracle/_build/libwdg_oracle.so

oracle/_build/libwdg_oracle.so: oracle/wdg_oracle.c
	@mkdir -p oracle/_build
	gcc -O2 -ffp-contract=off -shared -fPIC -o $@ $< -lm

clean:
	rm -rf build $(LIB) oracle/_build

.PHONY: all oracle clean hipcc-line variant
