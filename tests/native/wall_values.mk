# halo_wall_values_test (wall values, cudecomp_halo_wall_values.h): one binary per data type, built on demand by
# tests/test_gpu_native_halo_wall_values.py with `make -C tests/native -f wall_values.mk build/halo_wall_values_test_<dtype>`.
# Compile and link lines of wall_fields.mk.
ROCM ?= /opt/rocm
LIBDIR := ../../cudecomp_amd/lib
OUT := build
WALL_VALUES_DTYPES := R32 R64 C64 H16
WALL_VALUES_BINS := $(foreach d,$(WALL_VALUES_DTYPES),$(OUT)/halo_wall_values_test_$(d))
all: $(WALL_VALUES_BINS)
$(OUT)/obj/halo_wall_values_test_%.o: halo_wall_values_test.cpp native_test.h ../../include/cudecomp.h ../../include/cudecomp_amd.h ../../include/cudecomp_halo_wall_values.h
	@mkdir -p $(OUT)/obj
	$(ROCM)/bin/hipcc --offload-arch=gfx950 -O2 -std=c++17 -D$* -I../../include -c $< -o $@
$(WALL_VALUES_BINS): $(OUT)/%: $(OUT)/obj/%.o
	$(ROCM)/bin/hipcc --offload-arch=gfx950 $< -L$(LIBDIR) -lcudecomp -Wl,-rpath,'$$ORIGIN/../$(LIBDIR)' -Wl,-rpath,$(ROCM)/lib -o $@
.PHONY: all
