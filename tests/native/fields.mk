# halo_fields_test (multi-field halo updates, cudecomp_halo_fields.h): one binary per data type, built on demand by
# tests/test_gpu_native_halo_fields.py with `make -C tests/native -f fields.mk build/halo_fields_test_<dtype>`.
# Compile and link lines of Makefile's halo_ops_test.
ROCM ?= /opt/rocm
LIBDIR := ../../cudecomp_amd/lib
OUT := build
FIELDS_DTYPES := R32 R64 C64 H16
FIELDS_BINS := $(foreach d,$(FIELDS_DTYPES),$(OUT)/halo_fields_test_$(d))
all: $(FIELDS_BINS)
$(OUT)/obj/halo_fields_test_%.o: halo_fields_test.cpp native_test.h ../../include/cudecomp.h ../../include/cudecomp_amd.h ../../include/cudecomp_halo_fields.h
	@mkdir -p $(OUT)/obj
	$(ROCM)/bin/hipcc --offload-arch=gfx950 -O2 -std=c++17 -D$* -I../../include -c $< -o $@
$(FIELDS_BINS): $(OUT)/%: $(OUT)/obj/%.o
	$(ROCM)/bin/hipcc --offload-arch=gfx950 $< -L$(LIBDIR) -lcudecomp -Wl,-rpath,'$$ORIGIN/../$(LIBDIR)' -Wl,-rpath,$(ROCM)/lib -o $@
.PHONY: all
