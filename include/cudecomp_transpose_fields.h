/*
 * cudecomp_transpose_fields.h -- multi-field transposes: several pencils in one exchange.  An extension of the cuDecomp API a
 * solver may use, accepted by this library only (cudecomp_halo_fields.h has the halo side of the same idea).
 *
 * A solver rarely transposes one field: a pseudo-spectral Navier-Stokes step moves three velocity components forward and up to
 * nine products back, a channel code u, v, w and p together.  Transposed one by one, n fields pay n pack launches, n all-to-alls
 * and n unpack launches, and at the grid sizes where a transpose is latency-bound the call is almost all fixed cost.
 * cudecompAmdTransposeFields{XToY,YToZ,ZToY,YToX} takes the lists of fields, packs all of them in one launch, sends ONE message
 * per peer that holds all fields' chunks, and unpacks all of them in one launch.
 */
#ifndef CUDECOMP_TRANSPOSE_FIELDS_H
#define CUDECOMP_TRANSPOSE_FIELDS_H

#include "cudecomp.h"

#ifdef __cplusplus
extern "C" {
#endif

/* the most fields one call takes: two 256-byte tables of pointers in the kernel arguments */
#define CUDECOMP_AMD_MAX_TRANSPOSE_FIELDS 32

/*
 * Arguments.  `inputs` and `outputs` are HOST arrays of n_fields device pointers: inputs[f] is a pencil of grid_desc along the
 * source axis of the function's name, outputs[f] one along its destination axis.  All fields share dtype, halo extents and
 * padding.  The arrays are read before the call returns: they may be temporaries, and the call may be captured into a hipGraph.
 * The remaining arguments are those of cudecompTranspose{XToY,YToZ,ZToY,YToX}.
 *
 * Result.  Afterwards every outputs[f] is byte for byte, over the whole buffer -- halo and padding cells included -- what
 * cudecompTranspose* of inputs[f] with the same remaining arguments would have made of it.  Out of place every inputs[f] is
 * unchanged.  No value is converted; all seven element types are accepted (the four of cudecomp.h and the three of
 * cudecomp_amd.h, whose values may be passed without including that header).
 *
 * In place.  Either inputs[f] == outputs[f] for every f, or for none.
 *
 * Workspace.  `work` holds n_fields x cudecompGetTransposeWorkspaceSize(...) elements of dtype; there is no query of its own.
 * That suffices: the call aligns the receive area once behind n_fields send areas, and alignElements(n * x) + n * y <=
 * n * (alignElements(x) + y).  Cells of `work` beyond that are never touched.  The workspace rules of the descriptor's
 * transpose_comm_backend apply as they do to the single call (the NVSHMEM and NVSHMEM_PL backends need a workspace from
 * cudecompMalloc).
 *
 * Validation.  The order, result codes and CUDECOMP:ERROR messages of the single transpose, with the lists checked where it
 * checks `input` and `output`.  Each of these is CUDECOMP_RESULT_INVALID_USAGE, found on the host before anything is launched:
 * inputs == NULL or outputs == NULL; n_fields < 1 or > CUDECOMP_AMD_MAX_TRANSPOSE_FIELDS; a NULL entry; two equal entries within
 * inputs or within outputs; inputs[f] == outputs[g] for f != g; a mix of in-place and out-of-place fields.  Fields that overlap
 * partly are the caller's error and are not detected.  Decompositions with empty pencils are refused as the single call refuses
 * them (CUDECOMP_RESULT_NOT_SUPPORTED).
 *
 * Collective and asynchronous.  Every rank calls with the same n_fields.  The call is enqueued on `stream` and can be captured
 * into a caller's hipGraph wherever the single transpose of the descriptor's backend can.
 *
 * One field.  n_fields == 1 IS the single call: the same plan, kernels and paths as cudecompTranspose*.
 *
 * Two fields or more.  The sequence is always pack launch, one exchange, unpack launch, through the workspace; each peer gets one
 * message that holds all fields' chunks.  Not used: sending from the input and receiving into the output where a single
 * transpose can; the per-peer and staged pipelines; the fused and direct put (the small-exchange fused put included); the
 * two-hop relay; the in-place rotation; the library's own whole-operation graph; the performance report; the autotuner.  Every
 * transpose backend enum is accepted and selects the transport -- RCCL, MPI or the one-sided peer transport -- of that plain
 * path; the _PL and _SM enums take the same path.  Without an exchange (one rank) the call is one launch out of place, two in
 * place when the layouts differ, and nothing in place when they agree.
 */
cudecompResult_t cudecompAmdTransposeFieldsXToY(cudecompHandle_t handle, cudecompGridDesc_t grid_desc, void* const inputs[],
                                                void* const outputs[], int32_t n_fields, void* work, cudecompDataType_t dtype,
                                                const int32_t input_halo_extents[], const int32_t output_halo_extents[],
                                                const int32_t input_padding[], const int32_t output_padding[],
                                                hipStream_t stream);
cudecompResult_t cudecompAmdTransposeFieldsYToZ(cudecompHandle_t handle, cudecompGridDesc_t grid_desc, void* const inputs[],
                                                void* const outputs[], int32_t n_fields, void* work, cudecompDataType_t dtype,
                                                const int32_t input_halo_extents[], const int32_t output_halo_extents[],
                                                const int32_t input_padding[], const int32_t output_padding[],
                                                hipStream_t stream);
cudecompResult_t cudecompAmdTransposeFieldsZToY(cudecompHandle_t handle, cudecompGridDesc_t grid_desc, void* const inputs[],
                                                void* const outputs[], int32_t n_fields, void* work, cudecompDataType_t dtype,
                                                const int32_t input_halo_extents[], const int32_t output_halo_extents[],
                                                const int32_t input_padding[], const int32_t output_padding[],
                                                hipStream_t stream);
cudecompResult_t cudecompAmdTransposeFieldsYToX(cudecompHandle_t handle, cudecompGridDesc_t grid_desc, void* const inputs[],
                                                void* const outputs[], int32_t n_fields, void* work, cudecompDataType_t dtype,
                                                const int32_t input_halo_extents[], const int32_t output_halo_extents[],
                                                const int32_t input_padding[], const int32_t output_padding[],
                                                hipStream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* CUDECOMP_TRANSPOSE_FIELDS_H */
