/* transpose_fields_header.c -- cudecomp_transpose_fields.h as a C solver sees it: a C11 (and, compiled as such, a C++17)
 * translation unit, -Wall -Wextra -Werror, that includes the header -- alone, or after the headers named by BEFORE1..BEFORE6
 * (tests/test_transpose_fields_plan.py compiles both) -- and assigns every function it declares to a pointer whose type is
 * written out here by hand from the header text.  A prototype that changes -- an argument moved, a const dropped, a type
 * widened -- is an incompatible-pointer error.  Nothing is called. */
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
#include "cudecomp_transpose_fields.h"
#include "cudecomp_transpose_fields.h"

#if CUDECOMP_AMD_MAX_TRANSPOSE_FIELDS != 32
#error "CUDECOMP_AMD_MAX_TRANSPOSE_FIELDS"
#endif

/* cudecompAmdTransposeFields{XToY,YToZ,ZToY,YToX}: the argument list of cudecompTranspose* with the two host arrays of device
 * pointers and their length in the place of `input` and `output` */
typedef cudecompResult_t (*fields_fn)(cudecompHandle_t handle, cudecompGridDesc_t grid_desc, void* const inputs[], void* const outputs[],
                                      int32_t n_fields, void* work, cudecompDataType_t dtype, const int32_t input_halo_extents[],
                                      const int32_t output_halo_extents[], const int32_t input_padding[],
                                      const int32_t output_padding[], hipStream_t stream);

fields_fn const cudecomp_transpose_fields_header[4] = {cudecompAmdTransposeFieldsXToY, cudecompAmdTransposeFieldsYToZ,
                                                       cudecompAmdTransposeFieldsZToY, cudecompAmdTransposeFieldsYToX};
