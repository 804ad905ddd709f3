# halo_wall_fields_test (multi-field wall halos, cudecomp_halo_wall_fields.h): one binary per data type, built on demand by
# tests/test_gpu_native_halo_wall_fields.py with `make -C tests/native -f wall_fields.mk build/halo_wall_fields_test_<dtype>`.
# Compile and link lines of fields.mk.
ROCM ?= /opt/rocm
LIBDIR := ../../cudecomp_amd/lib
OUT := build
WALL_FIELDS_DTYPES := R32 R64 C64 H16
WALL_FIELDS_BINS := $(foreach d,$(WALL_FIELDS_DTYPES),$(OUT)/halo_wall_fields_test_$(d))
all: $(WALL_FIELDS_BINS)
$(OUT)/obj/halo_wall_fields_test_%.o: halo_wall_fields_test.cpp native_test.h ../../include/cudecomp.h ../../include/cudecomp_amd.h ../../include/cudecomp_halo_wall_fields.h
	@mkdir -p $(OUT)/obj
	$(ROCM)/bin/hipcc --offload-arch=gfx950 -O2 -std=c++17 -D$* -I../../include -c $< -o $@
$(WALL_FIELDS_BINS): $(OUT)/%: $(OUT)/obj/%.o
	$(ROCM)/bin/hipcc --offload-arch=gfx950 $< -L$(LIBDIR) -lcudecomp -Wl,-rpath,'$$ORIGIN/../$(LIBDIR)' -Wl,-rpath,$(ROCM)/lib -o $@
.PHONY: all
