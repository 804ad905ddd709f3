/* halo_accumulate_fields_header.c -- cudecomp_halo_accumulate_fields.h as a C solver sees it: a C11 (and, compiled as such, a C++17)
 * translation unit, -Wall -Wextra -Werror, that includes the header -- alone, or after the headers named by BEFORE1..BEFORE7
 * (tests/test_halo_accumulate_fields_plan.py compiles both) -- and assigns every function it declares to a pointer whose type is
 * written out here by hand from the header text.  A prototype that changes -- an argument moved, a const dropped, a type widened --
 * is an incompatible-pointer error.  Nothing is called. */
#ifdef BEFORE1
#include BEFORE1
#endif
#ifdef BEFORE2
#include BEFORE2
#endif
#ifdef BEFORE3
#include BEFORE3
#endif
#ifdef BEFORE4
#include BEFORE4
#endif
#ifdef BEFORE5
#include BEFORE5
#endif
#ifdef BEFORE6
#include BEFORE6
#endif
#ifdef BEFORE7
#include BEFORE7
#endif
#include "cudecomp_halo_accumulate_fields.h"
#include "cudecomp_halo_accumulate_fields.h"

#if CUDECOMP_AMD_MAX_HALO_ACCUMULATE_FIELDS != 32
#error "CUDECOMP_AMD_MAX_HALO_ACCUMULATE_FIELDS"
#endif

/* cudecompAmdAccumulateFieldHalos{X,Y,Z}: the argument list of cudecompAmdUpdateFieldHalos* with `clear` before the stream */
typedef cudecompResult_t (*accumulate_fields_fn)(cudecompHandle_t handle, cudecompGridDesc_t grid_desc, void* const inputs[],
                                                 int32_t n_fields, void* work, cudecompDataType_t dtype, const int32_t halo_extents[],
                                                 const bool halo_periods[], int32_t dim, const int32_t padding[],
                                                 int32_t clear, hipStream_t stream);

accumulate_fields_fn const cudecomp_halo_accumulate_fields_header[3] = {
    cudecompAmdAccumulateFieldHalosX, cudecompAmdAccumulateFieldHalosY, cudecompAmdAccumulateFieldHalosZ};
