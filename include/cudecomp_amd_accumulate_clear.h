/*
 * cudecomp_amd_accumulate_clear.h -- halo accumulate-and-clear: ghost cells summed into their owners and left as zero bytes, in
 * one call.  An extension of the cuDecomp API a solver may use, accepted by this library only.  Included by cudecomp_amd_fill.h,
 * which states the contract (its last section): the call is  cudecompAmdAccumulateHalos*(dim); cudecompAmdFillHalos*(dim, NULL)
 * byte for byte, with the argument list, the workspace, the transport, the asynchrony and the validation of the first.
 */
#ifndef CUDECOMP_AMD_ACCUMULATE_CLEAR_H
#define CUDECOMP_AMD_ACCUMULATE_CLEAR_H

#include "cudecomp_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

cudecompResult_t cudecompAmdAccumulateAndClearHalosX(cudecompHandle_t handle, cudecompGridDesc_t grid_desc, void* input, void* work,
                                                     cudecompDataType_t dtype, const int32_t halo_extents[],
                                                     const bool halo_periods[], int32_t dim, const int32_t padding[],
                                                     hipStream_t stream);
cudecompResult_t cudecompAmdAccumulateAndClearHalosY(cudecompHandle_t handle, cudecompGridDesc_t grid_desc, void* input, void* work,
                                                     cudecompDataType_t dtype, const int32_t halo_extents[],
                                                     const bool halo_periods[], int32_t dim, const int32_t padding[],
                                                     hipStream_t stream);
cudecompResult_t cudecompAmdAccumulateAndClearHalosZ(cudecompHandle_t handle, cudecompGridDesc_t grid_desc, void* input, void* work,
                                                     cudecompDataType_t dtype, const int32_t halo_extents[],
                                                     const bool halo_periods[], int32_t dim, const int32_t padding[],
                                                     hipStream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* CUDECOMP_AMD_ACCUMULATE_CLEAR_H */
