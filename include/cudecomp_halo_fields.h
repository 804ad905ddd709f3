/*
 * cudecomp_halo_fields.h -- multi-field halo updates: several pencils in one exchange.  An extension of the cuDecomp API a solver
 * may use, accepted by this library only (cudecomp_amd.h, cudecomp_amd_fill.h, cudecomp_amd_reflect.h and cudecomp_halo_fold.h
 * have the others).
 *
 * A solver rarely holds one field: three velocity components, u, v, w and p of a channel code, E and B of a particle code, the
 * 19 or 27 populations of a lattice-Boltzmann code.  Updating them one by one pays a pack launch, an exchange and an unpack
 * launch per field to send messages that are small already.  cudecompAmdUpdateFieldHalos{X,Y,Z} takes the list of fields, packs
 * all of them in one launch, sends ONE message per direction and unpacks all of them in one launch.
 */
#ifndef CUDECOMP_HALO_FIELDS_H
#define CUDECOMP_HALO_FIELDS_H

#include "cudecomp.h"

#ifdef __cplusplus
extern "C" {
#endif

/* the most fields one call takes: a 256-byte table of pointers in the kernel arguments (a D3Q27 lattice fits) */
#define CUDECOMP_AMD_MAX_HALO_FIELDS 32

/*
 * Arguments.  `inputs` is a HOST array of n_fields device pointers, each to a pencil of grid_desc along the axis in the function's
 * name; all fields have the same dtype, halo_extents and padding.  The array is read before the call returns: it may be a
 * temporary, and the call may be captured into a hipGraph.  The remaining arguments are those of cudecompUpdateHalos{X,Y,Z}.
 *
 * Result.  Afterwards every field is byte for byte what cudecompUpdateHalos{X,Y,Z} with the same remaining arguments would have
 * made of it alone.  Every cell a single call leaves alone is untouched: the interior, the padding, the halos of the other dims
 * outside the faces, and the side without a neighbour at a non-periodic edge.  No value is converted; all seven element types are
 * accepted (the four of cudecomp.h and the three of cudecomp_amd.h, whose values may be passed without including that header).
 *
 * Workspace.  `work` holds n_fields x cudecompGetHaloWorkspaceSize(...) elements of dtype; there is no query of its own.  (A
 * single call's workspace is four slots of one aligned face; this call uses four slots of n_fields faces aligned once, which is
 * never more.)  Cells of `work` beyond that are never touched.  The workspace rules of the descriptor's halo_comm_backend apply
 * as they do to the update (the NVSHMEM backends need a workspace from cudecompMalloc).
 *
 * Validation.  The order, result codes and CUDECOMP:ERROR messages of the update, with the list checked where the update checks
 * `input`: inputs == NULL, n_fields < 1 or > CUDECOMP_AMD_MAX_HALO_FIELDS, a NULL entry and two equal entries are each
 * CUDECOMP_RESULT_INVALID_USAGE, found on the host before anything is launched.  Fields that overlap partly are the caller's
 * error and are not detected.  As for the update, a call whose three halo_extents are all zero succeeds before the list is looked
 * at; halo_extents[dim] == 0 succeeds and does nothing; halos wider than a neighbour's slab and decompositions with empty pencils
 * are refused as the update refuses them.
 *
 * Collective and asynchronous.  Every rank calls with the same n_fields.  The call is enqueued on `stream`, never blocks the host
 * on GPU work beyond what the update does for the same backend, travels over the transport of the descriptor's halo_comm_backend
 * and can be captured into a hipGraph wherever the update can.
 *
 * One field.  n_fields == 1 IS the single call: the same plan, kernels and overlapped path as cudecompUpdateHalos{X,Y,Z}.
 *
 * Two fields or more.  The faces always travel packed through the workspace, one contiguous message of n_fields faces per
 * direction, also where a single field's faces are contiguous in the pencil and would travel from there.  The sequence is pack,
 * exchange, unpack, without the face-by-face overlap of the single update, and the performance report does not sample it.
 */
cudecompResult_t cudecompAmdUpdateFieldHalosX(cudecompHandle_t handle, cudecompGridDesc_t grid_desc, void* const inputs[],
                                              int32_t n_fields, void* work, cudecompDataType_t dtype,
                                              const int32_t halo_extents[], const bool halo_periods[], int32_t dim,
                                              const int32_t padding[], hipStream_t stream);
cudecompResult_t cudecompAmdUpdateFieldHalosY(cudecompHandle_t handle, cudecompGridDesc_t grid_desc, void* const inputs[],
                                              int32_t n_fields, void* work, cudecompDataType_t dtype,
                                              const int32_t halo_extents[], const bool halo_periods[], int32_t dim,
                                              const int32_t padding[], hipStream_t stream);
cudecompResult_t cudecompAmdUpdateFieldHalosZ(cudecompHandle_t handle, cudecompGridDesc_t grid_desc, void* const inputs[],
                                              int32_t n_fields, void* work, cudecompDataType_t dtype,
                                              const int32_t halo_extents[], const bool halo_periods[], int32_t dim,
                                              const int32_t padding[], hipStream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* CUDECOMP_HALO_FIELDS_H */
