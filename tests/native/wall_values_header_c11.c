/* cudecomp_halo_wall_values.h as a C11 translation unit (tests/test_wall_values_abi.py): alone, or -- with -DOTHERS_FIRST /
 * -DOTHERS_LAST -- after / before the other extension headers; every function assigned to a pointer of the prototype written out
 * by hand, so a prototype that differs does not compile. */
#ifdef OTHERS_FIRST
#include "cudecomp_amd.h"
#include "cudecomp_amd_fill.h"
#include "cudecomp_amd_reflect.h"
#include "cudecomp_halo_fold.h"
#include "cudecomp_halo_fields.h"
#include "cudecomp_halo_accumulate_fields.h"
#include "cudecomp_halo_wall_fields.h"
#include "cudecomp_transpose_fields.h"
#include "cudecomp_ext.h"
#endif
#include "cudecomp_halo_wall_values.h"
#include "cudecomp_halo_wall_values.h"
#ifdef OTHERS_LAST
#include "cudecomp_ext.h"
#include "cudecomp_transpose_fields.h"
#include "cudecomp_halo_wall_fields.h"
#include "cudecomp_halo_accumulate_fields.h"
#include "cudecomp_halo_fields.h"
#include "cudecomp_halo_fold.h"
#include "cudecomp_amd_reflect.h"
#include "cudecomp_amd_fill.h"
#include "cudecomp_amd.h"
#endif

#ifndef SIDES_TYPE
#define SIDES_TYPE int32_t
#endif

typedef cudecompResult_t (*wall_values_fn)(cudecompHandle_t, cudecompGridDesc_t, void*, cudecompDataType_t, int32_t, int32_t,
                                           SIDES_TYPE, const double[], const double[], const int32_t[], const bool[], int32_t,
                                           const int32_t[], hipStream_t);

static wall_values_fn const functions[3] = {cudecompAmdSetWallHalosX, cudecompAmdSetWallHalosY, cudecompAmdSetWallHalosZ};

_Static_assert(CUDECOMP_AMD_MAX_WALL_HALO == 8, "the widest halo the call accepts");

int main(void) { return functions[0] == functions[1] || functions[1] == functions[2]; }
