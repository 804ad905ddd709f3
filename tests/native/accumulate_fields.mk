# halo_accumulate_fields_test (multi-field halo accumulation, cudecomp_halo_accumulate_fields.h): one binary per data type, built on
# demand by tests/test_gpu_native_halo_accumulate_fields.py with
# `make -C tests/native -f accumulate_fields.mk build/halo_accumulate_fields_test_<dtype>`.  Compile and link lines of fields.mk.
ROCM ?= /opt/rocm
LIBDIR := ../../cudecomp_amd/lib
OUT := build
ACCUMULATE_FIELDS_DTYPES := R32 R64 C64 H16
ACCUMULATE_FIELDS_BINS := $(foreach d,$(ACCUMULATE_FIELDS_DTYPES),$(OUT)/halo_accumulate_fields_test_$(d))
all: $(ACCUMULATE_FIELDS_BINS)
$(OUT)/obj/halo_accumulate_fields_test_%.o: halo_accumulate_fields_test.cpp native_test.h ../../include/cudecomp.h ../../include/cudecomp_amd.h ../../include/cudecomp_amd_fill.h ../../include/cudecomp_amd_accumulate_clear.h ../../include/cudecomp_halo_accumulate_fields.h
	@mkdir -p $(OUT)/obj
	$(ROCM)/bin/hipcc --offload-arch=gfx950 -O2 -std=c++17 -D$* -I../../include -c $< -o $@
$(ACCUMULATE_FIELDS_BINS): $(OUT)/%: $(OUT)/obj/%.o
	$(ROCM)/bin/hipcc --offload-arch=gfx950 $< -L$(LIBDIR) -lcudecomp -Wl,-rpath,'$$ORIGIN/../$(LIBDIR)' -Wl,-rpath,$(ROCM)/lib -o $@
.PHONY: all
