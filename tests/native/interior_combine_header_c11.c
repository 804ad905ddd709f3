/* cudecomp_interior_combine.h as a C11 translation unit (tests/test_interior_combine_abi.py): alone, or -- with -DOTHERS_FIRST /
 * -DOTHERS_LAST -- after / before the other extension headers; every function assigned to a pointer of the prototype written out by
 * hand, so a prototype that differs does not compile. */
#ifdef OTHERS_FIRST
#include "cudecomp_interior_planes.h"
#include "cudecomp_interior_profile.h"
#include "cudecomp_ext.h"
#endif
#include "cudecomp_interior_combine.h"
#include "cudecomp_interior_combine.h"
#ifdef OTHERS_LAST
#include "cudecomp_ext.h"
#include "cudecomp_interior_profile.h"
#include "cudecomp_interior_planes.h"
#endif

#ifndef SCALE_TYPE
#define SCALE_TYPE double
#endif

typedef cudecompResult_t (*interior_combine_fn)(cudecompHandle_t, cudecompGridDesc_t, void* const[], const void* const[], int32_t, int32_t,
                                                const double*, const double*, SCALE_TYPE, const double*, const double*, double, int32_t,
                                                cudecompDataType_t, const int32_t[], const int32_t[], hipStream_t);

static interior_combine_fn const functions[3] = {cudecompAmdCombineInteriorX, cudecompAmdCombineInteriorY, cudecompAmdCombineInteriorZ};

/* the operations are this header's, the field limit is cudecomp_interior_reduce.h's */
#if CUDECOMP_AMD_COMBINE_AXPY != 0 || CUDECOMP_AMD_COMBINE_XPBY != 1 || CUDECOMP_AMD_COMBINE_AXPBY != 2 || CUDECOMP_AMD_COMBINE_AX != 3 || \
    CUDECOMP_AMD_MAX_REDUCE_FIELDS != 32
#error "the macros of cudecomp_interior_combine.h"
#endif

int main(void) { return functions[0] == functions[1] || functions[1] == functions[2]; }
