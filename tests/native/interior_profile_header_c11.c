/* cudecomp_interior_profile.h as a C11 translation unit (tests/test_interior_profile_abi.py): alone, or -- with -DOTHERS_FIRST /
 * -DOTHERS_LAST -- after / before the other extension headers; every function assigned to a pointer of the prototype written out by
 * hand, so a prototype that differs does not compile. */
#ifdef OTHERS_FIRST
#include "cudecomp_halo_wall_planes.h"
#include "cudecomp_interior_reduce.h"
#include "cudecomp_ext.h"
#endif
#include "cudecomp_interior_profile.h"
#include "cudecomp_interior_profile.h"
#ifdef OTHERS_LAST
#include "cudecomp_ext.h"
#include "cudecomp_interior_reduce.h"
#include "cudecomp_halo_wall_planes.h"
#endif

#ifndef LD_TYPE
#define LD_TYPE int64_t
#endif

typedef cudecompResult_t (*interior_profile_fn)(cudecompHandle_t, cudecompGridDesc_t, const void* const[], const void* const[], int32_t,
                                                int32_t, int32_t, double*, LD_TYPE, void*, cudecompDataType_t, const int32_t[],
                                                const int32_t[], hipStream_t);
typedef cudecompResult_t (*workspace_fn)(int32_t, int64_t, int64_t*);

static interior_profile_fn const functions[3] = {cudecompAmdProfileInteriorX, cudecompAmdProfileInteriorY, cudecompAmdProfileInteriorZ};
static workspace_fn const workspace = cudecompAmdProfileInteriorWorkspaceBytes;

/* the operations and the field limit are cudecomp_interior_reduce.h's */
#if CUDECOMP_AMD_MAX_REDUCE_FIELDS != 32 || CUDECOMP_AMD_REDUCE_SUM != 0 || CUDECOMP_AMD_REDUCE_DOT != 1 || CUDECOMP_AMD_REDUCE_MAX_ABS != 2
#error "the macros of cudecomp_interior_reduce.h"
#endif

int main(void) { return functions[0] == functions[1] || functions[1] == functions[2] || workspace == 0; }
