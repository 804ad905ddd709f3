/* cudecomp_halo_wall_planes.h as a C11 translation unit (tests/test_wall_planes_abi.py): alone, or -- with -DVALUES_FIRST /
 * -DVALUES_LAST -- after / before cudecomp_halo_wall_values.h and the other extension headers; every function assigned to a pointer
 * of the prototype written out by hand, so a prototype that differs does not compile. */
#ifdef VALUES_FIRST
#include "cudecomp_halo_wall_values.h"
#include "cudecomp_halo_wall_value_fields.h"
#include "cudecomp_amd_reflect.h"
#include "cudecomp_ext.h"
#endif
#include "cudecomp_halo_wall_planes.h"
#include "cudecomp_halo_wall_planes.h"
#ifdef VALUES_LAST
#include "cudecomp_ext.h"
#include "cudecomp_amd_reflect.h"
#include "cudecomp_halo_wall_value_fields.h"
#include "cudecomp_halo_wall_values.h"
#endif

#ifndef PLANE_TYPE
#define PLANE_TYPE const void*
#endif

typedef cudecompResult_t (*wall_planes_fn)(cudecompHandle_t, cudecompGridDesc_t, void*, cudecompDataType_t, int32_t, int32_t,
                                           int32_t, PLANE_TYPE, const void*, const int32_t[], const bool[], int32_t,
                                           const int32_t[], hipStream_t);

static wall_planes_fn const functions[3] = {cudecompAmdSetWallPlaneHalosX, cudecompAmdSetWallPlaneHalosY,
                                            cudecompAmdSetWallPlaneHalosZ};

int main(void) { return functions[0] == functions[1] || functions[1] == functions[2]; }
