# halo_fold_test (halo folding, cudecomp_halo_fold.h): one binary per data type, built on demand by
# tests/test_gpu_native_halo_fold.py with `make -C tests/native -f fold.mk build/halo_fold_test_<dtype>`.
# Compile and link lines of Makefile's halo_ops_test.
ROCM ?= /opt/rocm
LIBDIR := ../../cudecomp_amd/lib
OUT := build
FOLD_DTYPES := R32 R64 C32 C64 H16
FOLD_BINS := $(foreach d,$(FOLD_DTYPES),$(OUT)/halo_fold_test_$(d))
all: $(FOLD_BINS)
$(OUT)/obj/halo_fold_test_%.o: halo_fold_test.cpp native_test.h ../../include/cudecomp.h ../../include/cudecomp_amd.h ../../include/cudecomp_halo_fold.h
	@mkdir -p $(OUT)/obj
	$(ROCM)/bin/hipcc --offload-arch=gfx950 -O2 -std=c++17 -D$* -I../../include -c $< -o $@
$(FOLD_BINS): $(OUT)/%: $(OUT)/obj/%.o
	$(ROCM)/bin/hipcc --offload-arch=gfx950 $< -L$(LIBDIR) -lcudecomp -Wl,-rpath,'$$ORIGIN/../$(LIBDIR)' -Wl,-rpath,$(ROCM)/lib -o $@
.PHONY: all
