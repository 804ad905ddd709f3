# transpose_fields_test (multi-field transposes, cudecomp_transpose_fields.h): one binary per data type, built on demand by
# tests/test_gpu_native_transpose_fields.py with `make -C tests/native -f transpose_fields.mk build/transpose_fields_test_<dtype>`.
# Compile and link lines of fields.mk.
ROCM ?= /opt/rocm
LIBDIR := ../../cudecomp_amd/lib
OUT := build
TF_DTYPES := R32 R64 C64 H16
TF_BINS := $(foreach d,$(TF_DTYPES),$(OUT)/transpose_fields_test_$(d))
all: $(TF_BINS)
$(OUT)/obj/transpose_fields_test_%.o: transpose_fields_test.cpp native_test.h ../../include/cudecomp.h ../../include/cudecomp_amd.h ../../include/cudecomp_transpose_fields.h
	@mkdir -p $(OUT)/obj
	$(ROCM)/bin/hipcc --offload-arch=gfx950 -O2 -std=c++17 -D$* -I../../include -c $< -o $@
$(TF_BINS): $(OUT)/%: $(OUT)/obj/%.o
	$(ROCM)/bin/hipcc --offload-arch=gfx950 $< -L$(LIBDIR) -lcudecomp -Wl,-rpath,'$$ORIGIN/../$(LIBDIR)' -Wl,-rpath,$(ROCM)/lib -o $@
.PHONY: all
