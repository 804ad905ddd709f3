/* headers_c11.c -- the four extension headers as a C solver sees them: a C11 translation unit, -Wall -Wextra -Werror, that includes
 * them in the order INC1..INC4 (tests/test_abi.py compiles every order; the default is the order of their dependencies reversed)
 * and assigns every function they declare to a pointer whose type is written out here by hand from the header text.  A prototype
 * that changes -- an argument moved, a const dropped, a type widened -- is an incompatible-pointer error.  Nothing is called. */
#ifndef INC1
#define INC1 "cudecomp_amd_reflect.h"
#define INC2 "cudecomp_amd_accumulate_clear.h"
#define INC3 "cudecomp_amd_fill.h"
#define INC4 "cudecomp_amd.h"
#endif
#include INC1
#include INC2
#include INC3
#include INC4

/* cudecomp_amd.h: values 1..3, beside the reference's -1..-4 */
_Static_assert(CUDECOMP_AMD_HALF == 1, "CUDECOMP_AMD_HALF");
_Static_assert(CUDECOMP_AMD_BFLOAT16 == 2, "CUDECOMP_AMD_BFLOAT16");
_Static_assert(CUDECOMP_AMD_HALF_COMPLEX == 3, "CUDECOMP_AMD_HALF_COMPLEX");

/* cudecompAmdAccumulateHalos{X,Y,Z} and cudecompAmdAccumulateAndClearHalos{X,Y,Z}: the argument list of cudecompUpdateHalos* */
typedef cudecompResult_t (*exchange_fn)(cudecompHandle_t handle, cudecompGridDesc_t grid_desc, void* input, void* work,
                                        cudecompDataType_t dtype, const int32_t halo_extents[], const bool halo_periods[],
                                        int32_t dim, const int32_t padding[], hipStream_t stream);
/* cudecompAmdFillHalos{X,Y,Z}: no work, the value behind the data type */
typedef cudecompResult_t (*fill_fn)(cudecompHandle_t handle, cudecompGridDesc_t grid_desc, void* input, cudecompDataType_t dtype,
                                    const void* value, const int32_t halo_extents[], const bool halo_periods[], int32_t dim,
                                    const int32_t padding[], hipStream_t stream);
/* cudecompAmdReflectHalos{X,Y,Z}: parity, then centering, in the place of the value */
typedef cudecompResult_t (*reflect_fn)(cudecompHandle_t handle, cudecompGridDesc_t grid_desc, void* input, cudecompDataType_t dtype,
                                       int32_t parity, int32_t centering, const int32_t halo_extents[], const bool halo_periods[],
                                       int32_t dim, const int32_t padding[], hipStream_t stream);

exchange_fn const cudecomp_headers_c11_exchange[6] = {
    cudecompAmdAccumulateHalosX,         cudecompAmdAccumulateHalosY,         cudecompAmdAccumulateHalosZ,
    cudecompAmdAccumulateAndClearHalosX, cudecompAmdAccumulateAndClearHalosY, cudecompAmdAccumulateAndClearHalosZ};
fill_fn const cudecomp_headers_c11_fill[3] = {cudecompAmdFillHalosX, cudecompAmdFillHalosY, cudecompAmdFillHalosZ};
reflect_fn const cudecomp_headers_c11_reflect[3] = {cudecompAmdReflectHalosX, cudecompAmdReflectHalosY, cudecompAmdReflectHalosZ};
