! cudecomp_m.f90 -- Fortran interface (module `cudecomp`) to the MI355X pencil-decomposition library.
!
! Mirrors the Fortran API of the reference (src/cudecomp_m.cuf:182-541 interfaces, :560-1086 wrappers) so a
! Fortran solver keeps its `use cudecomp` and its calls, but is plain Fortran 2008 + iso_c_binding compiled by
! amdflang -- no CUDA Fortran: there is no `device` attribute on AMD, so device buffers are ordinary Fortran
! arrays / pointers whose *address* is a device address (what hipfort's hipMalloc, `!$omp target data
! use_device_addr` or cudecompMalloc below hand out).  The library never dereferences them on the host.
!
! Conventions that differ from the C API, all inherited from the reference module:
!   * axes, dims and memory orders are ONE-based (x/y/z = 1/2/3): `axis`, `dim`, `halo_axis`,
!     `transpose_mem_order`, `pencil_info%order` (reference :605-648, :808-822, :1001);
!   * `pencil_info%lo/hi` are one-based global coordinates (reference :646-648);
!   * multi-dimensional members are column-major: transpose_mem_order(3,3) is (position, axis) and the autotune
!     halo/padding tables are (3,4) = (dimension, transpose op);
!   * optional halo / padding / stream arguments default to zero / the null stream.
! Streams are `integer(cudecomp_stream_kind)` holding a hipStream_t by value (hipfort users:
! `transfer(stream_c_ptr, 0_cudecomp_stream_kind)`).

module cudecomp_internal
  use, intrinsic :: iso_c_binding
  implicit none
  public

  ! C struct cudecompGridDescConfig_t (include/cudecomp.h), 104 bytes
  type, bind(c) :: cudecompGridDescConfig_v1
    integer(c_int64_t) :: struct_size
    integer(c_int32_t) :: magic
    integer(c_int32_t) :: version
    integer(c_int32_t) :: gdims(3)
    integer(c_int32_t) :: gdims_dist(3)
    integer(c_int32_t) :: pdims(2)
    integer(c_int32_t) :: rank_order
    integer(c_int32_t) :: transpose_comm_backend
    logical(c_bool) :: transpose_axis_contiguous(3)
    integer(c_int32_t) :: transpose_mem_order(3, 3)
    integer(c_int32_t) :: halo_comm_backend
  end type cudecompGridDescConfig_v1

  ! C struct cudecompGridDescAutotuneOptions_t, 320 bytes
  type, bind(c) :: cudecompGridDescAutotuneOptions_v1
    integer(c_int64_t) :: struct_size
    integer(c_int32_t) :: magic
    integer(c_int32_t) :: version
    integer(c_int32_t) :: n_warmup_trials
    integer(c_int32_t) :: n_trials
    integer(c_int32_t) :: grid_mode
    integer(c_int32_t) :: dtype
    logical(c_bool) :: allow_uneven_decompositions
    logical(c_bool) :: disable_mpi_backends
    logical(c_bool) :: disable_nccl_backends
    logical(c_bool) :: disable_nvshmem_backends
    real(c_double) :: skip_threshold
    logical(c_bool) :: autotune_transpose_backend
    logical(c_bool) :: transpose_use_inplace_buffers(4)
    real(c_double) :: transpose_op_weights(4)
    integer(c_int32_t) :: transpose_input_halo_extents(3, 4)
    integer(c_int32_t) :: transpose_output_halo_extents(3, 4)
    integer(c_int32_t) :: transpose_input_padding(3, 4)
    integer(c_int32_t) :: transpose_output_padding(3, 4)
    logical(c_bool) :: autotune_halo_backend
    integer(c_int32_t) :: halo_extents(3)
    logical(c_bool) :: halo_periods(3)
    integer(c_int32_t) :: halo_axis
    integer(c_int32_t) :: halo_padding(3)
  end type cudecompGridDescAutotuneOptions_v1

  ! C struct cudecompPencilInfo_t, 96 bytes
  type, bind(c) :: cudecompPencilInfo_v1
    integer(c_int64_t) :: struct_size
    integer(c_int32_t) :: magic
    integer(c_int32_t) :: version
    integer(c_int32_t) :: shape(3)
    integer(c_int32_t) :: lo(3)
    integer(c_int32_t) :: hi(3)
    integer(c_int32_t) :: order(3)
    integer(c_int32_t) :: halo_extents(3)
    integer(c_int32_t) :: padding(3)
    integer(c_int64_t) :: size
  end type cudecompPencilInfo_v1
end module cudecomp_internal

module cudecomp
  use, intrinsic :: iso_c_binding
  use, intrinsic :: iso_fortran_env, only: int64, real32, real64
  use cudecomp_internal, only: cudecompGridDescConfig => cudecompGridDescConfig_v1, &
                               cudecompGridDescAutotuneOptions => cudecompGridDescAutotuneOptions_v1, &
                               cudecompPencilInfo => cudecompPencilInfo_v1
  implicit none
  private :: c_string_to_fortran

  integer, parameter :: cudecomp_stream_kind = c_intptr_t
  integer(c_int32_t), parameter, private :: STRUCT_VERSION = 1

  ! enum values as in include/cudecomp.h
  enum, bind(c)
    enumerator :: CUDECOMP_TRANSPOSE_COMM_MPI_P2P = 1
    enumerator :: CUDECOMP_TRANSPOSE_COMM_MPI_P2P_PL = 2
    enumerator :: CUDECOMP_TRANSPOSE_COMM_MPI_A2A = 3
    enumerator :: CUDECOMP_TRANSPOSE_COMM_NCCL = 4
    enumerator :: CUDECOMP_TRANSPOSE_COMM_NCCL_PL = 5
    enumerator :: CUDECOMP_TRANSPOSE_COMM_NVSHMEM = 6
    enumerator :: CUDECOMP_TRANSPOSE_COMM_NVSHMEM_PL = 7
    enumerator :: CUDECOMP_TRANSPOSE_COMM_NVSHMEM_SM = 8
  end enum
  enum, bind(c)
    enumerator :: CUDECOMP_HALO_COMM_MPI = 1
    enumerator :: CUDECOMP_HALO_COMM_MPI_BLOCKING = 2
    enumerator :: CUDECOMP_HALO_COMM_NCCL = 3
    enumerator :: CUDECOMP_HALO_COMM_NVSHMEM = 4
    enumerator :: CUDECOMP_HALO_COMM_NVSHMEM_BLOCKING = 5
  end enum
  enum, bind(c)
    enumerator :: CUDECOMP_AUTOTUNE_GRID_TRANSPOSE = 0
    enumerator :: CUDECOMP_AUTOTUNE_GRID_HALO = 1
  end enum
  enum, bind(c)
    enumerator :: CUDECOMP_RANK_ORDER_DEFAULT = 0
    enumerator :: CUDECOMP_RANK_ORDER_ROW_MAJOR = 1
    enumerator :: CUDECOMP_RANK_ORDER_COL_MAJOR = 2
  end enum
  enum, bind(c)
    enumerator :: CUDECOMP_FLOAT = -1
    enumerator :: CUDECOMP_DOUBLE = -2
    enumerator :: CUDECOMP_FLOAT_COMPLEX = -3
    enumerator :: CUDECOMP_DOUBLE_COMPLEX = -4
  end enum
  ! cudecomp_interior_reduce.h: the operations of cudecompAmdReduceInterior{X,Y,Z}, and the most fields a call takes
  integer(c_int32_t), parameter :: CUDECOMP_AMD_REDUCE_SUM = 0, CUDECOMP_AMD_REDUCE_DOT = 1, CUDECOMP_AMD_REDUCE_MAX_ABS = 2
  integer(c_int32_t), parameter :: CUDECOMP_AMD_PLANES_ADD = 0, CUDECOMP_AMD_PLANES_MUL = 1
  integer(c_int32_t), parameter :: CUDECOMP_AMD_COMBINE_AXPY = 0, CUDECOMP_AMD_COMBINE_XPBY = 1, CUDECOMP_AMD_COMBINE_AXPBY = 2, &
                                   CUDECOMP_AMD_COMBINE_AX = 3
  integer(c_int32_t), parameter :: CUDECOMP_AMD_MAX_REDUCE_FIELDS = 32
  enum, bind(c)
    enumerator :: CUDECOMP_RESULT_SUCCESS = 0
    enumerator :: CUDECOMP_RESULT_INVALID_USAGE = 1
    enumerator :: CUDECOMP_RESULT_NOT_SUPPORTED = 2
    enumerator :: CUDECOMP_RESULT_INTERNAL_ERROR = 3
    enumerator :: CUDECOMP_RESULT_CUDA_ERROR = 4
    enumerator :: CUDECOMP_RESULT_CUTENSOR_ERROR = 5
    enumerator :: CUDECOMP_RESULT_MPI_ERROR = 6
    enumerator :: CUDECOMP_RESULT_NCCL_ERROR = 7
    enumerator :: CUDECOMP_RESULT_NVSHMEM_ERROR = 8
    enumerator :: CUDECOMP_RESULT_NVML_ERROR = 9
  end enum

  ! opaque handles: one C pointer each, passed by value
  type, bind(c) :: cudecompHandle
    type(c_ptr) :: member = c_null_ptr
  end type cudecompHandle
  type, bind(c) :: cudecompGridDesc
    type(c_ptr) :: member = c_null_ptr
  end type cudecompGridDesc

  ! ---- generic names -------------------------------------------------------------------------------------
  interface cudecompInit
    module procedure cudecompInit_comm_int, cudecompInit_comm_f08
  end interface cudecompInit
  interface cudecompMalloc
    module procedure cudecompMallocR4, cudecompMallocR8, cudecompMallocC4, cudecompMallocC8, cudecompMallocPtr
  end interface cudecompMalloc
  interface cudecompFree
    module procedure cudecompFreeR4, cudecompFreeR8, cudecompFreeC4, cudecompFreeC8, cudecompFreePtr
  end interface cudecompFree

  ! ---- the C entry points (include/cudecomp.h) ----------------------------------------------------------------
  interface
    function cudecompInit_FC(handle, mpi_comm) bind(C, name="cudecompInit_F") result(res)
      import
      type(cudecompHandle) :: handle
      integer(c_int), value :: mpi_comm
      integer(c_int) :: res
    end function cudecompInit_FC

    function cudecompFinalize(handle) bind(C, name="cudecompFinalize") result(res)
      import
      type(cudecompHandle), value :: handle
      integer(c_int) :: res
    end function cudecompFinalize

    function cudecompGridDescCreateC(handle, grid_desc, config, config_struct_size, config_version, options, &
                                     options_struct_size, options_version) &
      bind(C, name="cudecompGridDescCreateVersioned") result(res)
      import
      type(cudecompHandle), value :: handle
      type(cudecompGridDesc) :: grid_desc
      type(c_ptr), value :: config
      integer(c_int64_t), value :: config_struct_size
      integer(c_int32_t), value :: config_version
      type(c_ptr), value :: options
      integer(c_int64_t), value :: options_struct_size
      integer(c_int32_t), value :: options_version
      integer(c_int) :: res
    end function cudecompGridDescCreateC

    function cudecompGridDescDestroy(handle, grid_desc) bind(C, name="cudecompGridDescDestroy") result(res)
      import
      type(cudecompHandle), value :: handle
      type(cudecompGridDesc), value :: grid_desc
      integer(c_int) :: res
    end function cudecompGridDescDestroy

    function cudecompGridDescConfigSetDefaultsC(config, struct_size, version) &
      bind(C, name="cudecompGridDescConfigSetDefaultsVersioned") result(res)
      import
      type(c_ptr), value :: config
      integer(c_int64_t), value :: struct_size
      integer(c_int32_t), value :: version
      integer(c_int) :: res
    end function cudecompGridDescConfigSetDefaultsC

    function cudecompGridDescAutotuneOptionsSetDefaultsC(options, struct_size, version) &
      bind(C, name="cudecompGridDescAutotuneOptionsSetDefaultsVersioned") result(res)
      import
      type(c_ptr), value :: options
      integer(c_int64_t), value :: struct_size
      integer(c_int32_t), value :: version
      integer(c_int) :: res
    end function cudecompGridDescAutotuneOptionsSetDefaultsC

    function cudecompGetPencilInfoC(handle, grid_desc, pencil_info, struct_size, version, axis, halo_extents, &
                                    padding) bind(C, name="cudecompGetPencilInfoVersioned") result(res)
      import
      type(cudecompHandle), value :: handle
      type(cudecompGridDesc), value :: grid_desc
      type(c_ptr), value :: pencil_info
      integer(c_int64_t), value :: struct_size
      integer(c_int32_t), value :: version
      integer(c_int32_t), value :: axis
      integer(c_int32_t) :: halo_extents(3), padding(3)
      integer(c_int) :: res
    end function cudecompGetPencilInfoC

    function cudecompGetGridDescConfigC(handle, grid_desc, config, struct_size, version) &
      bind(C, name="cudecompGetGridDescConfigVersioned") result(res)
      import
      type(cudecompHandle), value :: handle
      type(cudecompGridDesc), value :: grid_desc
      type(c_ptr), value :: config
      integer(c_int64_t), value :: struct_size
      integer(c_int32_t), value :: version
      integer(c_int) :: res
    end function cudecompGetGridDescConfigC

    function cudecompGetTransposeWorkspaceSize(handle, grid_desc, workspace_size) &
      bind(C, name="cudecompGetTransposeWorkspaceSize") result(res)
      import
      type(cudecompHandle), value :: handle
      type(cudecompGridDesc), value :: grid_desc
      integer(c_int64_t) :: workspace_size
      integer(c_int) :: res
    end function cudecompGetTransposeWorkspaceSize

    function cudecompGetHaloWorkspaceSizeC(handle, grid_desc, axis, halo_extents, workspace_size) &
      bind(C, name="cudecompGetHaloWorkspaceSize") result(res)
      import
      type(cudecompHandle), value :: handle
      type(cudecompGridDesc), value :: grid_desc
      integer(c_int32_t), value :: axis
      integer(c_int32_t) :: halo_extents(3)
      integer(c_int64_t) :: workspace_size
      integer(c_int) :: res
    end function cudecompGetHaloWorkspaceSizeC

    function cudecompGetDataTypeSize(dtype, dtype_size) bind(C, name="cudecompGetDataTypeSize") result(res)
      import
      integer(c_int), value :: dtype
      integer(c_int64_t) :: dtype_size
      integer(c_int) :: res
    end function cudecompGetDataTypeSize

    function cudecompMallocC(handle, grid_desc, buffer, buffer_size_bytes) bind(C, name="cudecompMalloc") result(res)
      import
      type(cudecompHandle), value :: handle
      type(cudecompGridDesc), value :: grid_desc
      type(c_ptr) :: buffer
      integer(c_size_t), value :: buffer_size_bytes
      integer(c_int) :: res
    end function cudecompMallocC

    function cudecompFreeC(handle, grid_desc, buffer) bind(C, name="cudecompFree") result(res)
      import
      type(cudecompHandle), value :: handle
      type(cudecompGridDesc), value :: grid_desc
      type(c_ptr), value :: buffer
      integer(c_int) :: res
    end function cudecompFreeC

    function cudecompTransposeCommBackendToStringC(comm_backend) &
      bind(C, name="cudecompTransposeCommBackendToString") result(res)
      import
      integer(c_int), value :: comm_backend
      type(c_ptr) :: res
    end function cudecompTransposeCommBackendToStringC

    function cudecompHaloCommBackendToStringC(comm_backend) &
      bind(C, name="cudecompHaloCommBackendToString") result(res)
      import
      integer(c_int), value :: comm_backend
      type(c_ptr) :: res
    end function cudecompHaloCommBackendToStringC

    function cudecompGetShiftedRankC(handle, grid_desc, axis, dim, displacement, periodic, shifted_rank) &
      bind(C, name="cudecompGetShiftedRank") result(res)
      import
      type(cudecompHandle), value :: handle
      type(cudecompGridDesc), value :: grid_desc
      integer(c_int32_t), value :: axis, dim, displacement
      logical(c_bool), value :: periodic
      integer(c_int32_t) :: shifted_rank
      integer(c_int) :: res
    end function cudecompGetShiftedRankC

    ! data-path entry points: buffers travel as raw addresses
    function cudecompTransposeXToY_C(handle, grid_desc, input, output, work, dtype, ihalo, ohalo, ipad, opad, &
                                     stream) bind(C, name="cudecompTransposeXToY") result(res)
      import
      type(cudecompHandle), value :: handle
      type(cudecompGridDesc), value :: grid_desc
      type(c_ptr), value :: input, output, work
      integer(c_int), value :: dtype
      integer(c_int32_t) :: ihalo(3), ohalo(3), ipad(3), opad(3)
      integer(c_intptr_t), value :: stream
      integer(c_int) :: res
    end function cudecompTransposeXToY_C

    function cudecompTransposeYToZ_C(handle, grid_desc, input, output, work, dtype, ihalo, ohalo, ipad, opad, &
                                     stream) bind(C, name="cudecompTransposeYToZ") result(res)
      import
      type(cudecompHandle), value :: handle
      type(cudecompGridDesc), value :: grid_desc
      type(c_ptr), value :: input, output, work
      integer(c_int), value :: dtype
      integer(c_int32_t) :: ihalo(3), ohalo(3), ipad(3), opad(3)
      integer(c_intptr_t), value :: stream
      integer(c_int) :: res
    end function cudecompTransposeYToZ_C

    function cudecompTransposeZToY_C(handle, grid_desc, input, output, work, dtype, ihalo, ohalo, ipad, opad, &
                                     stream) bind(C, name="cudecompTransposeZToY") result(res)
      import
      type(cudecompHandle), value :: handle
      type(cudecompGridDesc), value :: grid_desc
      type(c_ptr), value :: input, output, work
      integer(c_int), value :: dtype
      integer(c_int32_t) :: ihalo(3), ohalo(3), ipad(3), opad(3)
      integer(c_intptr_t), value :: stream
      integer(c_int) :: res
    end function cudecompTransposeZToY_C

    function cudecompTransposeYToX_C(handle, grid_desc, input, output, work, dtype, ihalo, ohalo, ipad, opad, &
                                     stream) bind(C, name="cudecompTransposeYToX") result(res)
      import
      type(cudecompHandle), value :: handle
      type(cudecompGridDesc), value :: grid_desc
      type(c_ptr), value :: input, output, work
      integer(c_int), value :: dtype
      integer(c_int32_t) :: ihalo(3), ohalo(3), ipad(3), opad(3)
      integer(c_intptr_t), value :: stream
      integer(c_int) :: res
    end function cudecompTransposeYToX_C

    function cudecompUpdateHalosX_C(handle, grid_desc, input, work, dtype, halo_extents, halo_periods, dim, &
                                    padding, stream) bind(C, name="cudecompUpdateHalosX") result(res)
      import
      type(cudecompHandle), value :: handle
      type(cudecompGridDesc), value :: grid_desc
      type(c_ptr), value :: input, work
      integer(c_int), value :: dtype
      integer(c_int32_t) :: halo_extents(3)
      logical(c_bool) :: halo_periods(3)
      integer(c_int32_t), value :: dim
      integer(c_int32_t) :: padding(3)
      integer(c_intptr_t), value :: stream
      integer(c_int) :: res
    end function cudecompUpdateHalosX_C

    function cudecompUpdateHalosY_C(handle, grid_desc, input, work, dtype, halo_extents, halo_periods, dim, &
                                    padding, stream) bind(C, name="cudecompUpdateHalosY") result(res)
      import
      type(cudecompHandle), value :: handle
      type(cudecompGridDesc), value :: grid_desc
      type(c_ptr), value :: input, work
      integer(c_int), value :: dtype
      integer(c_int32_t) :: halo_extents(3)
      logical(c_bool) :: halo_periods(3)
      integer(c_int32_t), value :: dim
      integer(c_int32_t) :: padding(3)
      integer(c_intptr_t), value :: stream
      integer(c_int) :: res
    end function cudecompUpdateHalosY_C

    function cudecompUpdateHalosZ_C(handle, grid_desc, input, work, dtype, halo_extents, halo_periods, dim, &
                                    padding, stream) bind(C, name="cudecompUpdateHalosZ") result(res)
      import
      type(cudecompHandle), value :: handle
      type(cudecompGridDesc), value :: grid_desc
      type(c_ptr), value :: input, work
      integer(c_int), value :: dtype
      integer(c_int32_t) :: halo_extents(3)
      logical(c_bool) :: halo_periods(3)
      integer(c_int32_t), value :: dim
      integer(c_int32_t) :: padding(3)
      integer(c_intptr_t), value :: stream
      integer(c_int) :: res
    end function cudecompUpdateHalosZ_C

    ! cudecomp_amd.h: halo accumulation, the transpose of the updates (ghost cells summed into their owners)
    function cudecompAmdAccumulateHalosX_C(handle, grid_desc, input, work, dtype, halo_extents, halo_periods, dim, &
                                           padding, stream) bind(C, name="cudecompAmdAccumulateHalosX") result(res)
      import
      type(cudecompHandle), value :: handle
      type(cudecompGridDesc), value :: grid_desc
      type(c_ptr), value :: input, work
      integer(c_int), value :: dtype
      integer(c_int32_t) :: halo_extents(3)
      logical(c_bool) :: halo_periods(3)
      integer(c_int32_t), value :: dim
      integer(c_int32_t) :: padding(3)
      integer(c_intptr_t), value :: stream
      integer(c_int) :: res
    end function cudecompAmdAccumulateHalosX_C

    function cudecompAmdAccumulateHalosY_C(handle, grid_desc, input, work, dtype, halo_extents, halo_periods, dim, &
                                           padding, stream) bind(C, name="cudecompAmdAccumulateHalosY") result(res)
      import
      type(cudecompHandle), value :: handle
      type(cudecompGridDesc), value :: grid_desc
      type(c_ptr), value :: input, work
      integer(c_int), value :: dtype
      integer(c_int32_t) :: halo_extents(3)
      logical(c_bool) :: halo_periods(3)
      integer(c_int32_t), value :: dim
      integer(c_int32_t) :: padding(3)
      integer(c_intptr_t), value :: stream
      integer(c_int) :: res
    end function cudecompAmdAccumulateHalosY_C

    function cudecompAmdAccumulateHalosZ_C(handle, grid_desc, input, work, dtype, halo_extents, halo_periods, dim, &
                                           padding, stream) bind(C, name="cudecompAmdAccumulateHalosZ") result(res)
      import
      type(cudecompHandle), value :: handle
      type(cudecompGridDesc), value :: grid_desc
      type(c_ptr), value :: input, work
      integer(c_int), value :: dtype
      integer(c_int32_t) :: halo_extents(3)
      logical(c_bool) :: halo_periods(3)
      integer(c_int32_t), value :: dim
      integer(c_int32_t) :: padding(3)
      integer(c_intptr_t), value :: stream
      integer(c_int) :: res
    end function cudecompAmdAccumulateHalosZ_C

    ! cudecomp_amd_fill.h: halo fill (the ghost cells an update would write receive one value)
    function cudecompAmdFillHalosX_C(handle, grid_desc, input, dtype, value, halo_extents, halo_periods, dim, &
                                     padding, stream) bind(C, name="cudecompAmdFillHalosX") result(res)
      import
      type(cudecompHandle), value :: handle
      type(cudecompGridDesc), value :: grid_desc
      type(c_ptr), value :: input
      integer(c_int), value :: dtype
      type(c_ptr), value :: value
      integer(c_int32_t) :: halo_extents(3)
      logical(c_bool) :: halo_periods(3)
      integer(c_int32_t), value :: dim
      integer(c_int32_t) :: padding(3)
      integer(c_intptr_t), value :: stream
      integer(c_int) :: res
    end function cudecompAmdFillHalosX_C

    function cudecompAmdFillHalosY_C(handle, grid_desc, input, dtype, value, halo_extents, halo_periods, dim, &
                                     padding, stream) bind(C, name="cudecompAmdFillHalosY") result(res)
      import
      type(cudecompHandle), value :: handle
      type(cudecompGridDesc), value :: grid_desc
      type(c_ptr), value :: input
      integer(c_int), value :: dtype
      type(c_ptr), value :: value
      integer(c_int32_t) :: halo_extents(3)
      logical(c_bool) :: halo_periods(3)
      integer(c_int32_t), value :: dim
      integer(c_int32_t) :: padding(3)
      integer(c_intptr_t), value :: stream
      integer(c_int) :: res
    end function cudecompAmdFillHalosY_C

    function cudecompAmdFillHalosZ_C(handle, grid_desc, input, dtype, value, halo_extents, halo_periods, dim, &
                                     padding, stream) bind(C, name="cudecompAmdFillHalosZ") result(res)
      import
      type(cudecompHandle), value :: handle
      type(cudecompGridDesc), value :: grid_desc
      type(c_ptr), value :: input
      integer(c_int), value :: dtype
      type(c_ptr), value :: value
      integer(c_int32_t) :: halo_extents(3)
      logical(c_bool) :: halo_periods(3)
      integer(c_int32_t), value :: dim
      integer(c_int32_t) :: padding(3)
      integer(c_intptr_t), value :: stream
      integer(c_int) :: res
    end function cudecompAmdFillHalosZ_C

    ! cudecomp_amd_fill.h: halo accumulate-and-clear (accumulation, then zero bytes into the ghost cells it has read)
    function cudecompAmdAccumulateAndClearHalosX_C(handle, grid_desc, input, work, dtype, halo_extents, halo_periods, dim, &
                                           padding, stream) bind(C, name="cudecompAmdAccumulateAndClearHalosX") result(res)
      import
      type(cudecompHandle), value :: handle
      type(cudecompGridDesc), value :: grid_desc
      type(c_ptr), value :: input, work
      integer(c_int), value :: dtype
      integer(c_int32_t) :: halo_extents(3)
      logical(c_bool) :: halo_periods(3)
      integer(c_int32_t), value :: dim
      integer(c_int32_t) :: padding(3)
      integer(c_intptr_t), value :: stream
      integer(c_int) :: res
    end function cudecompAmdAccumulateAndClearHalosX_C

    function cudecompAmdAccumulateAndClearHalosY_C(handle, grid_desc, input, work, dtype, halo_extents, halo_periods, dim, &
                                           padding, stream) bind(C, name="cudecompAmdAccumulateAndClearHalosY") result(res)
      import
      type(cudecompHandle), value :: handle
      type(cudecompGridDesc), value :: grid_desc
      type(c_ptr), value :: input, work
      integer(c_int), value :: dtype
      integer(c_int32_t) :: halo_extents(3)
      logical(c_bool) :: halo_periods(3)
      integer(c_int32_t), value :: dim
      integer(c_int32_t) :: padding(3)
      integer(c_intptr_t), value :: stream
      integer(c_int) :: res
    end function cudecompAmdAccumulateAndClearHalosY_C

    function cudecompAmdAccumulateAndClearHalosZ_C(handle, grid_desc, input, work, dtype, halo_extents, halo_periods, dim, &
                                           padding, stream) bind(C, name="cudecompAmdAccumulateAndClearHalosZ") result(res)
      import
      type(cudecompHandle), value :: handle
      type(cudecompGridDesc), value :: grid_desc
      type(c_ptr), value :: input, work
      integer(c_int), value :: dtype
      integer(c_int32_t) :: halo_extents(3)
      logical(c_bool) :: halo_periods(3)
      integer(c_int32_t), value :: dim
      integer(c_int32_t) :: padding(3)
      integer(c_intptr_t), value :: stream
      integer(c_int) :: res
    end function cudecompAmdAccumulateAndClearHalosZ_C

    ! cudecomp_amd_reflect.h: halo reflection (mirrored ghost cells at the non-periodic edges of the domain)
    function cudecompAmdReflectHalosX_C(handle, grid_desc, input, dtype, parity, centering, halo_extents, halo_periods, dim, &
                                        padding, stream) bind(C, name="cudecompAmdReflectHalosX") result(res)
      import
      type(cudecompHandle), value :: handle
      type(cudecompGridDesc), value :: grid_desc
      type(c_ptr), value :: input
      integer(c_int), value :: dtype
      integer(c_int32_t), value :: parity, centering
      integer(c_int32_t) :: halo_extents(3)
      logical(c_bool) :: halo_periods(3)
      integer(c_int32_t), value :: dim
      integer(c_int32_t) :: padding(3)
      integer(c_intptr_t), value :: stream
      integer(c_int) :: res
    end function cudecompAmdReflectHalosX_C

    function cudecompAmdReflectHalosY_C(handle, grid_desc, input, dtype, parity, centering, halo_extents, halo_periods, dim, &
                                        padding, stream) bind(C, name="cudecompAmdReflectHalosY") result(res)
      import
      type(cudecompHandle), value :: handle
      type(cudecompGridDesc), value :: grid_desc
      type(c_ptr), value :: input
      integer(c_int), value :: dtype
      integer(c_int32_t), value :: parity, centering
      integer(c_int32_t) :: halo_extents(3)
      logical(c_bool) :: halo_periods(3)
      integer(c_int32_t), value :: dim
      integer(c_int32_t) :: padding(3)
      integer(c_intptr_t), value :: stream
      integer(c_int) :: res
    end function cudecompAmdReflectHalosY_C

    function cudecompAmdReflectHalosZ_C(handle, grid_desc, input, dtype, parity, centering, halo_extents, halo_periods, dim, &
                                        padding, stream) bind(C, name="cudecompAmdReflectHalosZ") result(res)
      import
      type(cudecompHandle), value :: handle
      type(cudecompGridDesc), value :: grid_desc
      type(c_ptr), value :: input
      integer(c_int), value :: dtype
      integer(c_int32_t), value :: parity, centering
      integer(c_int32_t) :: halo_extents(3)
      logical(c_bool) :: halo_periods(3)
      integer(c_int32_t), value :: dim
      integer(c_int32_t) :: padding(3)
      integer(c_intptr_t), value :: stream
      integer(c_int) :: res
    end function cudecompAmdReflectHalosZ_C

    ! cudecomp_halo_wall_values.h: wall values (the reflection with one addend per ghost layer and side)
    function cudecompAmdSetWallHalosX_C(handle, grid_desc, input, dtype, parity, centering, sides, values_low, values_high, &
                                        halo_extents, halo_periods, dim, padding, stream) &
      bind(C, name="cudecompAmdSetWallHalosX") result(res)
      import
      type(cudecompHandle), value :: handle
      type(cudecompGridDesc), value :: grid_desc
      type(c_ptr), value :: input
      integer(c_int), value :: dtype
      integer(c_int32_t), value :: parity, centering, sides
      type(c_ptr), value :: values_low, values_high  ! host arrays of doubles (NULL for a side that `sides` does not name)
      integer(c_int32_t) :: halo_extents(3)
      logical(c_bool) :: halo_periods(3)
      integer(c_int32_t), value :: dim
      integer(c_int32_t) :: padding(3)
      integer(c_intptr_t), value :: stream
      integer(c_int) :: res
    end function cudecompAmdSetWallHalosX_C

    function cudecompAmdSetWallHalosY_C(handle, grid_desc, input, dtype, parity, centering, sides, values_low, values_high, &
                                        halo_extents, halo_periods, dim, padding, stream) &
      bind(C, name="cudecompAmdSetWallHalosY") result(res)
      import
      type(cudecompHandle), value :: handle
      type(cudecompGridDesc), value :: grid_desc
      type(c_ptr), value :: input
      integer(c_int), value :: dtype
      integer(c_int32_t), value :: parity, centering, sides
      type(c_ptr), value :: values_low, values_high  ! host arrays of doubles (NULL for a side that `sides` does not name)
      integer(c_int32_t) :: halo_extents(3)
      logical(c_bool) :: halo_periods(3)
      integer(c_int32_t), value :: dim
      integer(c_int32_t) :: padding(3)
      integer(c_intptr_t), value :: stream
      integer(c_int) :: res
    end function cudecompAmdSetWallHalosY_C

    function cudecompAmdSetWallHalosZ_C(handle, grid_desc, input, dtype, parity, centering, sides, values_low, values_high, &
                                        halo_extents, halo_periods, dim, padding, stream) &
      bind(C, name="cudecompAmdSetWallHalosZ") result(res)
      import
      type(cudecompHandle), value :: handle
      type(cudecompGridDesc), value :: grid_desc
      type(c_ptr), value :: input
      integer(c_int), value :: dtype
      integer(c_int32_t), value :: parity, centering, sides
      type(c_ptr), value :: values_low, values_high  ! host arrays of doubles (NULL for a side that `sides` does not name)
      integer(c_int32_t) :: halo_extents(3)
      logical(c_bool) :: halo_periods(3)
      integer(c_int32_t), value :: dim
      integer(c_int32_t) :: padding(3)
      integer(c_intptr_t), value :: stream
      integer(c_int) :: res
    end function cudecompAmdSetWallHalosZ_C

    ! cudecomp_halo_wall_planes.h: wall planes (the reflection with an addend per cell of the ghost slab, from device arrays)
    function cudecompAmdSetWallPlaneHalosX_C(handle, grid_desc, input, dtype, parity, centering, sides, planes_low, planes_high, &
                                             halo_extents, halo_periods, dim, padding, stream) &
      bind(C, name="cudecompAmdSetWallPlaneHalosX") result(res)
      import
      type(cudecompHandle), value :: handle
      type(cudecompGridDesc), value :: grid_desc
      type(c_ptr), value :: input
      integer(c_int), value :: dtype
      integer(c_int32_t), value :: parity, centering, sides
      type(c_ptr), value :: planes_low, planes_high  ! device arrays of `dtype` (NULL for a side that `sides` does not name)
      integer(c_int32_t) :: halo_extents(3)
      logical(c_bool) :: halo_periods(3)
      integer(c_int32_t), value :: dim
      integer(c_int32_t) :: padding(3)
      integer(c_intptr_t), value :: stream
      integer(c_int) :: res
    end function cudecompAmdSetWallPlaneHalosX_C

    function cudecompAmdSetWallPlaneHalosY_C(handle, grid_desc, input, dtype, parity, centering, sides, planes_low, planes_high, &
                                             halo_extents, halo_periods, dim, padding, stream) &
      bind(C, name="cudecompAmdSetWallPlaneHalosY") result(res)
      import
      type(cudecompHandle), value :: handle
      type(cudecompGridDesc), value :: grid_desc
      type(c_ptr), value :: input
      integer(c_int), value :: dtype
      integer(c_int32_t), value :: parity, centering, sides
      type(c_ptr), value :: planes_low, planes_high  ! device arrays of `dtype` (NULL for a side that `sides` does not name)
      integer(c_int32_t) :: halo_extents(3)
      logical(c_bool) :: halo_periods(3)
      integer(c_int32_t), value :: dim
      integer(c_int32_t) :: padding(3)
      integer(c_intptr_t), value :: stream
      integer(c_int) :: res
    end function cudecompAmdSetWallPlaneHalosY_C

    function cudecompAmdSetWallPlaneHalosZ_C(handle, grid_desc, input, dtype, parity, centering, sides, planes_low, planes_high, &
                                             halo_extents, halo_periods, dim, padding, stream) &
      bind(C, name="cudecompAmdSetWallPlaneHalosZ") result(res)
      import
      type(cudecompHandle), value :: handle
      type(cudecompGridDesc), value :: grid_desc
      type(c_ptr), value :: input
      integer(c_int), value :: dtype
      integer(c_int32_t), value :: parity, centering, sides
      type(c_ptr), value :: planes_low, planes_high  ! device arrays of `dtype` (NULL for a side that `sides` does not name)
      integer(c_int32_t) :: halo_extents(3)
      logical(c_bool) :: halo_periods(3)
      integer(c_int32_t), value :: dim
      integer(c_int32_t) :: padding(3)
      integer(c_intptr_t), value :: stream
      integer(c_int) :: res
    end function cudecompAmdSetWallPlaneHalosZ_C

    ! cudecomp_interior_reduce.h: sum, dot product and largest magnitude over the cells a rank owns.  Plain bind(c) interfaces: `a`
    ! and `b` are arrays of n_fields device addresses (b: c_null_ptr entries are refused for a dot product only), `results` and
    ! `work` device addresses, `op` one of CUDECOMP_AMD_REDUCE_SUM / _DOT / _MAX_ABS
    function cudecompAmdReduceInteriorWorkspaceBytes(n_fields, bytes) &
      bind(C, name="cudecompAmdReduceInteriorWorkspaceBytes") result(res)
      import
      integer(c_int32_t), value :: n_fields
      integer(c_int64_t) :: bytes
      integer(c_int) :: res
    end function cudecompAmdReduceInteriorWorkspaceBytes

    function cudecompAmdReduceInteriorX(handle, grid_desc, a, b, n_fields, op, results, work, dtype, halo_extents, padding, stream) &
      bind(C, name="cudecompAmdReduceInteriorX") result(res)
      import
      type(cudecompHandle), value :: handle
      type(cudecompGridDesc), value :: grid_desc
      type(c_ptr) :: a(*), b(*)
      integer(c_int32_t), value :: n_fields, op
      type(c_ptr), value :: results, work
      integer(c_int), value :: dtype
      integer(c_int32_t) :: halo_extents(3), padding(3)
      integer(c_intptr_t), value :: stream
      integer(c_int) :: res
    end function cudecompAmdReduceInteriorX

    function cudecompAmdReduceInteriorY(handle, grid_desc, a, b, n_fields, op, results, work, dtype, halo_extents, padding, stream) &
      bind(C, name="cudecompAmdReduceInteriorY") result(res)
      import
      type(cudecompHandle), value :: handle
      type(cudecompGridDesc), value :: grid_desc
      type(c_ptr) :: a(*), b(*)
      integer(c_int32_t), value :: n_fields, op
      type(c_ptr), value :: results, work
      integer(c_int), value :: dtype
      integer(c_int32_t) :: halo_extents(3), padding(3)
      integer(c_intptr_t), value :: stream
      integer(c_int) :: res
    end function cudecompAmdReduceInteriorY

    function cudecompAmdReduceInteriorZ(handle, grid_desc, a, b, n_fields, op, results, work, dtype, halo_extents, padding, stream) &
      bind(C, name="cudecompAmdReduceInteriorZ") result(res)
      import
      type(cudecompHandle), value :: handle
      type(cudecompGridDesc), value :: grid_desc
      type(c_ptr) :: a(*), b(*)
      integer(c_int32_t), value :: n_fields, op
      type(c_ptr), value :: results, work
      integer(c_int), value :: dtype
      integer(c_int32_t) :: halo_extents(3), padding(3)
      integer(c_intptr_t), value :: stream
      integer(c_int) :: res
    end function cudecompAmdReduceInteriorZ

    ! cudecomp_interior_profile.h: the reductions of cudecomp_interior_reduce.h over two dims of the interior, kept along `dim`.  The
    ! C entry points (zero-based dim); the wrappers cudecompAmdProfileInterior{X,Y,Z} below take dim = 1/2/3
    function cudecompAmdProfileInteriorWorkspaceBytes(n_fields, length, bytes) &
      bind(C, name="cudecompAmdProfileInteriorWorkspaceBytes") result(res)
      import
      integer(c_int32_t), value :: n_fields
      integer(c_int64_t), value :: length
      integer(c_int64_t) :: bytes
      integer(c_int) :: res
    end function cudecompAmdProfileInteriorWorkspaceBytes

    function cudecompAmdProfileInteriorX_C(handle, grid_desc, a, b, n_fields, op, dim, results, ld, work, dtype, halo_extents, &
                                           padding, stream) &
      bind(C, name="cudecompAmdProfileInteriorX") result(res)
      import
      type(cudecompHandle), value :: handle
      type(cudecompGridDesc), value :: grid_desc
      type(c_ptr) :: a(*), b(*)
      integer(c_int32_t), value :: n_fields, op, dim
      type(c_ptr), value :: results
      integer(c_int64_t), value :: ld
      type(c_ptr), value :: work
      integer(c_int), value :: dtype
      integer(c_int32_t) :: halo_extents(3), padding(3)
      integer(c_intptr_t), value :: stream
      integer(c_int) :: res
    end function cudecompAmdProfileInteriorX_C

    function cudecompAmdProfileInteriorY_C(handle, grid_desc, a, b, n_fields, op, dim, results, ld, work, dtype, halo_extents, &
                                           padding, stream) &
      bind(C, name="cudecompAmdProfileInteriorY") result(res)
      import
      type(cudecompHandle), value :: handle
      type(cudecompGridDesc), value :: grid_desc
      type(c_ptr) :: a(*), b(*)
      integer(c_int32_t), value :: n_fields, op, dim
      type(c_ptr), value :: results
      integer(c_int64_t), value :: ld
      type(c_ptr), value :: work
      integer(c_int), value :: dtype
      integer(c_int32_t) :: halo_extents(3), padding(3)
      integer(c_intptr_t), value :: stream
      integer(c_int) :: res
    end function cudecompAmdProfileInteriorY_C

    function cudecompAmdProfileInteriorZ_C(handle, grid_desc, a, b, n_fields, op, dim, results, ld, work, dtype, halo_extents, &
                                           padding, stream) &
      bind(C, name="cudecompAmdProfileInteriorZ") result(res)
      import
      type(cudecompHandle), value :: handle
      type(cudecompGridDesc), value :: grid_desc
      type(c_ptr) :: a(*), b(*)
      integer(c_int32_t), value :: n_fields, op, dim
      type(c_ptr), value :: results
      integer(c_int64_t), value :: ld
      type(c_ptr), value :: work
      integer(c_int), value :: dtype
      integer(c_int32_t) :: halo_extents(3), padding(3)
      integer(c_intptr_t), value :: stream
      integer(c_int) :: res
    end function cudecompAmdProfileInteriorZ_C

    ! cudecomp_interior_planes.h: the profile's adjoint -- every interior cell updated in place with the coefficient of its index
    ! along `dim`.  The C entry points (zero-based dim); the wrappers cudecompAmdApplyPlanesInterior{X,Y,Z} below take dim = 1/2/3
    function cudecompAmdApplyPlanesInteriorX_C(handle, grid_desc, fields, n_fields, op, dim, coef, ld, scale, dtype, halo_extents, &
                                               padding, stream) &
      bind(C, name="cudecompAmdApplyPlanesInteriorX") result(res)
      import
      type(cudecompHandle), value :: handle
      type(cudecompGridDesc), value :: grid_desc
      type(c_ptr) :: fields(*)
      integer(c_int32_t), value :: n_fields, op, dim
      type(c_ptr), value :: coef
      integer(c_int64_t), value :: ld
      real(c_double), value :: scale
      integer(c_int), value :: dtype
      integer(c_int32_t) :: halo_extents(3), padding(3)
      integer(c_intptr_t), value :: stream
      integer(c_int) :: res
    end function cudecompAmdApplyPlanesInteriorX_C

    function cudecompAmdApplyPlanesInteriorY_C(handle, grid_desc, fields, n_fields, op, dim, coef, ld, scale, dtype, halo_extents, &
                                               padding, stream) &
      bind(C, name="cudecompAmdApplyPlanesInteriorY") result(res)
      import
      type(cudecompHandle), value :: handle
      type(cudecompGridDesc), value :: grid_desc
      type(c_ptr) :: fields(*)
      integer(c_int32_t), value :: n_fields, op, dim
      type(c_ptr), value :: coef
      integer(c_int64_t), value :: ld
      real(c_double), value :: scale
      integer(c_int), value :: dtype
      integer(c_int32_t) :: halo_extents(3), padding(3)
      integer(c_intptr_t), value :: stream
      integer(c_int) :: res
    end function cudecompAmdApplyPlanesInteriorY_C

    function cudecompAmdApplyPlanesInteriorZ_C(handle, grid_desc, fields, n_fields, op, dim, coef, ld, scale, dtype, halo_extents, &
                                               padding, stream) &
      bind(C, name="cudecompAmdApplyPlanesInteriorZ") result(res)
      import
      type(cudecompHandle), value :: handle
      type(cudecompGridDesc), value :: grid_desc
      type(c_ptr) :: fields(*)
      integer(c_int32_t), value :: n_fields, op, dim
      type(c_ptr), value :: coef
      integer(c_int64_t), value :: ld
      real(c_double), value :: scale
      integer(c_int), value :: dtype
      integer(c_int32_t) :: halo_extents(3), padding(3)
      integer(c_intptr_t), value :: stream
      integer(c_int) :: res
    end function cudecompAmdApplyPlanesInteriorZ_C

    ! cudecomp_interior_combine.h: y <- a * x + b * y over the interior, the coefficients ratios of doubles in device memory.  The C
    ! entry points; the wrappers cudecompAmdCombineInterior{X,Y,Z} below make padding and stream optional
    function cudecompAmdCombineInteriorX_C(handle, grid_desc, y, x, n_fields, op, a_num, a_den, a_scale, b_num, b_den, b_scale, &
                                           coef_stride, dtype, halo_extents, padding, stream) &
      bind(C, name="cudecompAmdCombineInteriorX") result(res)
      import
      type(cudecompHandle), value :: handle
      type(cudecompGridDesc), value :: grid_desc
      type(c_ptr) :: y(*), x(*)
      integer(c_int32_t), value :: n_fields, op
      type(c_ptr), value :: a_num, a_den
      real(c_double), value :: a_scale
      type(c_ptr), value :: b_num, b_den
      real(c_double), value :: b_scale
      integer(c_int32_t), value :: coef_stride
      integer(c_int), value :: dtype
      integer(c_int32_t) :: halo_extents(3), padding(3)
      integer(c_intptr_t), value :: stream
      integer(c_int) :: res
    end function cudecompAmdCombineInteriorX_C

    function cudecompAmdCombineInteriorY_C(handle, grid_desc, y, x, n_fields, op, a_num, a_den, a_scale, b_num, b_den, b_scale, &
                                           coef_stride, dtype, halo_extents, padding, stream) &
      bind(C, name="cudecompAmdCombineInteriorY") result(res)
      import
      type(cudecompHandle), value :: handle
      type(cudecompGridDesc), value :: grid_desc
      type(c_ptr) :: y(*), x(*)
      integer(c_int32_t), value :: n_fields, op
      type(c_ptr), value :: a_num, a_den
      real(c_double), value :: a_scale
      type(c_ptr), value :: b_num, b_den
      real(c_double), value :: b_scale
      integer(c_int32_t), value :: coef_stride
      integer(c_int), value :: dtype
      integer(c_int32_t) :: halo_extents(3), padding(3)
      integer(c_intptr_t), value :: stream
      integer(c_int) :: res
    end function cudecompAmdCombineInteriorY_C

    function cudecompAmdCombineInteriorZ_C(handle, grid_desc, y, x, n_fields, op, a_num, a_den, a_scale, b_num, b_den, b_scale, &
                                           coef_stride, dtype, halo_extents, padding, stream) &
      bind(C, name="cudecompAmdCombineInteriorZ") result(res)
      import
      type(cudecompHandle), value :: handle
      type(cudecompGridDesc), value :: grid_desc
      type(c_ptr) :: y(*), x(*)
      integer(c_int32_t), value :: n_fields, op
      type(c_ptr), value :: a_num, a_den
      real(c_double), value :: a_scale
      type(c_ptr), value :: b_num, b_den
      real(c_double), value :: b_scale
      integer(c_int32_t), value :: coef_stride
      integer(c_int), value :: dtype
      integer(c_int32_t) :: halo_extents(3), padding(3)
      integer(c_intptr_t), value :: stream
      integer(c_int) :: res
    end function cudecompAmdCombineInteriorZ_C

    ! cudecomp_halo_wall_value_fields.h: wall values of several pencils, each with a parity and addends of its own
    function cudecompAmdSetWallFieldHalosX_C(handle, grid_desc, inputs, n_fields, dtype, parities, centering, sides, values_low, &
                                             values_high, halo_extents, halo_periods, dim, padding, stream) &
      bind(C, name="cudecompAmdSetWallFieldHalosX") result(res)
      import
      type(cudecompHandle), value :: handle
      type(cudecompGridDesc), value :: grid_desc
      type(c_ptr) :: inputs(*)
      integer(c_int32_t), value :: n_fields
      integer(c_int), value :: dtype
      integer(c_int32_t) :: parities(*)
      integer(c_int32_t), value :: centering, sides
      type(c_ptr), value :: values_low, values_high  ! host arrays of doubles, field-major (NULL for a side that `sides` does not name)
      integer(c_int32_t) :: halo_extents(3)
      logical(c_bool) :: halo_periods(3)
      integer(c_int32_t), value :: dim
      integer(c_int32_t) :: padding(3)
      integer(c_intptr_t), value :: stream
      integer(c_int) :: res
    end function cudecompAmdSetWallFieldHalosX_C

    function cudecompAmdSetWallFieldHalosY_C(handle, grid_desc, inputs, n_fields, dtype, parities, centering, sides, values_low, &
                                             values_high, halo_extents, halo_periods, dim, padding, stream) &
      bind(C, name="cudecompAmdSetWallFieldHalosY") result(res)
      import
      type(cudecompHandle), value :: handle
      type(cudecompGridDesc), value :: grid_desc
      type(c_ptr) :: inputs(*)
      integer(c_int32_t), value :: n_fields
      integer(c_int), value :: dtype
      integer(c_int32_t) :: parities(*)
      integer(c_int32_t), value :: centering, sides
      type(c_ptr), value :: values_low, values_high  ! host arrays of doubles, field-major (NULL for a side that `sides` does not name)
      integer(c_int32_t) :: halo_extents(3)
      logical(c_bool) :: halo_periods(3)
      integer(c_int32_t), value :: dim
      integer(c_int32_t) :: padding(3)
      integer(c_intptr_t), value :: stream
      integer(c_int) :: res
    end function cudecompAmdSetWallFieldHalosY_C

    function cudecompAmdSetWallFieldHalosZ_C(handle, grid_desc, inputs, n_fields, dtype, parities, centering, sides, values_low, &
                                             values_high, halo_extents, halo_periods, dim, padding, stream) &
      bind(C, name="cudecompAmdSetWallFieldHalosZ") result(res)
      import
      type(cudecompHandle), value :: handle
      type(cudecompGridDesc), value :: grid_desc
      type(c_ptr) :: inputs(*)
      integer(c_int32_t), value :: n_fields
      integer(c_int), value :: dtype
      integer(c_int32_t) :: parities(*)
      integer(c_int32_t), value :: centering, sides
      type(c_ptr), value :: values_low, values_high  ! host arrays of doubles, field-major (NULL for a side that `sides` does not name)
      integer(c_int32_t) :: halo_extents(3)
      logical(c_bool) :: halo_periods(3)
      integer(c_int32_t), value :: dim
      integer(c_int32_t) :: padding(3)
      integer(c_intptr_t), value :: stream
      integer(c_int) :: res
    end function cudecompAmdSetWallFieldHalosZ_C

    ! cudecomp_halo_fold.h: halo folding (the ghost cells the reflection writes, summed into their mirror images)
    function cudecompAmdFoldHalosX_C(handle, grid_desc, input, dtype, parity, centering, clear, halo_extents, halo_periods, dim, &
                                        padding, stream) bind(C, name="cudecompAmdFoldHalosX") result(res)
      import
      type(cudecompHandle), value :: handle
      type(cudecompGridDesc), value :: grid_desc
      type(c_ptr), value :: input
      integer(c_int), value :: dtype
      integer(c_int32_t), value :: parity, centering, clear
      integer(c_int32_t) :: halo_extents(3)
      logical(c_bool) :: halo_periods(3)
      integer(c_int32_t), value :: dim
      integer(c_int32_t) :: padding(3)
      integer(c_intptr_t), value :: stream
      integer(c_int) :: res
    end function cudecompAmdFoldHalosX_C

    function cudecompAmdFoldHalosY_C(handle, grid_desc, input, dtype, parity, centering, clear, halo_extents, halo_periods, dim, &
                                        padding, stream) bind(C, name="cudecompAmdFoldHalosY") result(res)
      import
      type(cudecompHandle), value :: handle
      type(cudecompGridDesc), value :: grid_desc
      type(c_ptr), value :: input
      integer(c_int), value :: dtype
      integer(c_int32_t), value :: parity, centering, clear
      integer(c_int32_t) :: halo_extents(3)
      logical(c_bool) :: halo_periods(3)
      integer(c_int32_t), value :: dim
      integer(c_int32_t) :: padding(3)
      integer(c_intptr_t), value :: stream
      integer(c_int) :: res
    end function cudecompAmdFoldHalosY_C

    function cudecompAmdFoldHalosZ_C(handle, grid_desc, input, dtype, parity, centering, clear, halo_extents, halo_periods, dim, &
                                        padding, stream) bind(C, name="cudecompAmdFoldHalosZ") result(res)
      import
      type(cudecompHandle), value :: handle
      type(cudecompGridDesc), value :: grid_desc
      type(c_ptr), value :: input
      integer(c_int), value :: dtype
      integer(c_int32_t), value :: parity, centering, clear
      integer(c_int32_t) :: halo_extents(3)
      logical(c_bool) :: halo_periods(3)
      integer(c_int32_t), value :: dim
      integer(c_int32_t) :: padding(3)
      integer(c_intptr_t), value :: stream
      integer(c_int) :: res
    end function cudecompAmdFoldHalosZ_C

    function cudecompAmdUpdateFieldHalosX_C(handle, grid_desc, inputs, n_fields, work, dtype, halo_extents, halo_periods, dim, &
                                            padding, stream) bind(C, name="cudecompAmdUpdateFieldHalosX") result(res)
      import
      type(cudecompHandle), value :: handle
      type(cudecompGridDesc), value :: grid_desc
      integer(c_int32_t), value :: n_fields
      type(c_ptr) :: inputs(*)
      type(c_ptr), value :: work
      integer(c_int), value :: dtype
      integer(c_int32_t) :: halo_extents(3)
      logical(c_bool) :: halo_periods(3)
      integer(c_int32_t), value :: dim
      integer(c_int32_t) :: padding(3)
      integer(c_intptr_t), value :: stream
      integer(c_int) :: res
    end function cudecompAmdUpdateFieldHalosX_C

    function cudecompAmdUpdateFieldHalosY_C(handle, grid_desc, inputs, n_fields, work, dtype, halo_extents, halo_periods, dim, &
                                            padding, stream) bind(C, name="cudecompAmdUpdateFieldHalosY") result(res)
      import
      type(cudecompHandle), value :: handle
      type(cudecompGridDesc), value :: grid_desc
      integer(c_int32_t), value :: n_fields
      type(c_ptr) :: inputs(*)
      type(c_ptr), value :: work
      integer(c_int), value :: dtype
      integer(c_int32_t) :: halo_extents(3)
      logical(c_bool) :: halo_periods(3)
      integer(c_int32_t), value :: dim
      integer(c_int32_t) :: padding(3)
      integer(c_intptr_t), value :: stream
      integer(c_int) :: res
    end function cudecompAmdUpdateFieldHalosY_C

    function cudecompAmdUpdateFieldHalosZ_C(handle, grid_desc, inputs, n_fields, work, dtype, halo_extents, halo_periods, dim, &
                                            padding, stream) bind(C, name="cudecompAmdUpdateFieldHalosZ") result(res)
      import
      type(cudecompHandle), value :: handle
      type(cudecompGridDesc), value :: grid_desc
      integer(c_int32_t), value :: n_fields
      type(c_ptr) :: inputs(*)
      type(c_ptr), value :: work
      integer(c_int), value :: dtype
      integer(c_int32_t) :: halo_extents(3)
      logical(c_bool) :: halo_periods(3)
      integer(c_int32_t), value :: dim
      integer(c_int32_t) :: padding(3)
      integer(c_intptr_t), value :: stream
      integer(c_int) :: res
    end function cudecompAmdUpdateFieldHalosZ_C

    function cudecompAmdAccumulateFieldHalosX_C(handle, grid_desc, inputs, n_fields, work, dtype, halo_extents, halo_periods, dim, &
                                                padding, clear, stream) bind(C, name="cudecompAmdAccumulateFieldHalosX") result(res)
      import
      type(cudecompHandle), value :: handle
      type(cudecompGridDesc), value :: grid_desc
      integer(c_int32_t), value :: n_fields
      type(c_ptr) :: inputs(*)
      type(c_ptr), value :: work
      integer(c_int), value :: dtype
      integer(c_int32_t) :: halo_extents(3)
      logical(c_bool) :: halo_periods(3)
      integer(c_int32_t), value :: dim
      integer(c_int32_t) :: padding(3)
      integer(c_int32_t), value :: clear
      integer(c_intptr_t), value :: stream
      integer(c_int) :: res
    end function cudecompAmdAccumulateFieldHalosX_C

    function cudecompAmdAccumulateFieldHalosY_C(handle, grid_desc, inputs, n_fields, work, dtype, halo_extents, halo_periods, dim, &
                                                padding, clear, stream) bind(C, name="cudecompAmdAccumulateFieldHalosY") result(res)
      import
      type(cudecompHandle), value :: handle
      type(cudecompGridDesc), value :: grid_desc
      integer(c_int32_t), value :: n_fields
      type(c_ptr) :: inputs(*)
      type(c_ptr), value :: work
      integer(c_int), value :: dtype
      integer(c_int32_t) :: halo_extents(3)
      logical(c_bool) :: halo_periods(3)
      integer(c_int32_t), value :: dim
      integer(c_int32_t) :: padding(3)
      integer(c_int32_t), value :: clear
      integer(c_intptr_t), value :: stream
      integer(c_int) :: res
    end function cudecompAmdAccumulateFieldHalosY_C

    function cudecompAmdAccumulateFieldHalosZ_C(handle, grid_desc, inputs, n_fields, work, dtype, halo_extents, halo_periods, dim, &
                                                padding, clear, stream) bind(C, name="cudecompAmdAccumulateFieldHalosZ") result(res)
      import
      type(cudecompHandle), value :: handle
      type(cudecompGridDesc), value :: grid_desc
      integer(c_int32_t), value :: n_fields
      type(c_ptr) :: inputs(*)
      type(c_ptr), value :: work
      integer(c_int), value :: dtype
      integer(c_int32_t) :: halo_extents(3)
      logical(c_bool) :: halo_periods(3)
      integer(c_int32_t), value :: dim
      integer(c_int32_t) :: padding(3)
      integer(c_int32_t), value :: clear
      integer(c_intptr_t), value :: stream
      integer(c_int) :: res
    end function cudecompAmdAccumulateFieldHalosZ_C

    ! cudecomp_halo_wall_fields.h: reflection and fold of several pencils, each with a parity of its own
    function cudecompAmdReflectFieldHalosX_C(handle, grid_desc, inputs, n_fields, dtype, parities, centering, halo_extents, halo_periods, &
                                            dim, padding, stream) bind(C, name="cudecompAmdReflectFieldHalosX") result(res)
      import
      type(cudecompHandle), value :: handle
      type(cudecompGridDesc), value :: grid_desc
      type(c_ptr) :: inputs(*)
      integer(c_int32_t), value :: n_fields
      integer(c_int), value :: dtype
      integer(c_int32_t) :: parities(*)
      integer(c_int32_t), value :: centering
      integer(c_int32_t) :: halo_extents(3)
      logical(c_bool) :: halo_periods(3)
      integer(c_int32_t), value :: dim
      integer(c_int32_t) :: padding(3)
      integer(c_intptr_t), value :: stream
      integer(c_int) :: res
    end function cudecompAmdReflectFieldHalosX_C

    function cudecompAmdReflectFieldHalosY_C(handle, grid_desc, inputs, n_fields, dtype, parities, centering, halo_extents, halo_periods, &
                                            dim, padding, stream) bind(C, name="cudecompAmdReflectFieldHalosY") result(res)
      import
      type(cudecompHandle), value :: handle
      type(cudecompGridDesc), value :: grid_desc
      type(c_ptr) :: inputs(*)
      integer(c_int32_t), value :: n_fields
      integer(c_int), value :: dtype
      integer(c_int32_t) :: parities(*)
      integer(c_int32_t), value :: centering
      integer(c_int32_t) :: halo_extents(3)
      logical(c_bool) :: halo_periods(3)
      integer(c_int32_t), value :: dim
      integer(c_int32_t) :: padding(3)
      integer(c_intptr_t), value :: stream
      integer(c_int) :: res
    end function cudecompAmdReflectFieldHalosY_C

    function cudecompAmdReflectFieldHalosZ_C(handle, grid_desc, inputs, n_fields, dtype, parities, centering, halo_extents, halo_periods, &
                                            dim, padding, stream) bind(C, name="cudecompAmdReflectFieldHalosZ") result(res)
      import
      type(cudecompHandle), value :: handle
      type(cudecompGridDesc), value :: grid_desc
      type(c_ptr) :: inputs(*)
      integer(c_int32_t), value :: n_fields
      integer(c_int), value :: dtype
      integer(c_int32_t) :: parities(*)
      integer(c_int32_t), value :: centering
      integer(c_int32_t) :: halo_extents(3)
      logical(c_bool) :: halo_periods(3)
      integer(c_int32_t), value :: dim
      integer(c_int32_t) :: padding(3)
      integer(c_intptr_t), value :: stream
      integer(c_int) :: res
    end function cudecompAmdReflectFieldHalosZ_C

    function cudecompAmdFoldFieldHalosX_C(handle, grid_desc, inputs, n_fields, dtype, parities, centering, clear, halo_extents, halo_periods, &
                                            dim, padding, stream) bind(C, name="cudecompAmdFoldFieldHalosX") result(res)
      import
      type(cudecompHandle), value :: handle
      type(cudecompGridDesc), value :: grid_desc
      type(c_ptr) :: inputs(*)
      integer(c_int32_t), value :: n_fields
      integer(c_int), value :: dtype
      integer(c_int32_t) :: parities(*)
      integer(c_int32_t), value :: centering, clear
      integer(c_int32_t) :: halo_extents(3)
      logical(c_bool) :: halo_periods(3)
      integer(c_int32_t), value :: dim
      integer(c_int32_t) :: padding(3)
      integer(c_intptr_t), value :: stream
      integer(c_int) :: res
    end function cudecompAmdFoldFieldHalosX_C

    function cudecompAmdFoldFieldHalosY_C(handle, grid_desc, inputs, n_fields, dtype, parities, centering, clear, halo_extents, halo_periods, &
                                            dim, padding, stream) bind(C, name="cudecompAmdFoldFieldHalosY") result(res)
      import
      type(cudecompHandle), value :: handle
      type(cudecompGridDesc), value :: grid_desc
      type(c_ptr) :: inputs(*)
      integer(c_int32_t), value :: n_fields
      integer(c_int), value :: dtype
      integer(c_int32_t) :: parities(*)
      integer(c_int32_t), value :: centering, clear
      integer(c_int32_t) :: halo_extents(3)
      logical(c_bool) :: halo_periods(3)
      integer(c_int32_t), value :: dim
      integer(c_int32_t) :: padding(3)
      integer(c_intptr_t), value :: stream
      integer(c_int) :: res
    end function cudecompAmdFoldFieldHalosY_C

    function cudecompAmdFoldFieldHalosZ_C(handle, grid_desc, inputs, n_fields, dtype, parities, centering, clear, halo_extents, halo_periods, &
                                            dim, padding, stream) bind(C, name="cudecompAmdFoldFieldHalosZ") result(res)
      import
      type(cudecompHandle), value :: handle
      type(cudecompGridDesc), value :: grid_desc
      type(c_ptr) :: inputs(*)
      integer(c_int32_t), value :: n_fields
      integer(c_int), value :: dtype
      integer(c_int32_t) :: parities(*)
      integer(c_int32_t), value :: centering, clear
      integer(c_int32_t) :: halo_extents(3)
      logical(c_bool) :: halo_periods(3)
      integer(c_int32_t), value :: dim
      integer(c_int32_t) :: padding(3)
      integer(c_intptr_t), value :: stream
      integer(c_int) :: res
    end function cudecompAmdFoldFieldHalosZ_C

    function cudecompAmdTransposeFieldsXToY_C(handle, grid_desc, inputs, outputs, n_fields, work, dtype, ihalo, ohalo, ipad, opad, &
                                                stream) bind(C, name="cudecompAmdTransposeFieldsXToY") result(res)
      import
      type(cudecompHandle), value :: handle
      type(cudecompGridDesc), value :: grid_desc
      type(c_ptr) :: inputs(*), outputs(*)
      integer(c_int32_t), value :: n_fields
      type(c_ptr), value :: work
      integer(c_int), value :: dtype
      integer(c_int32_t) :: ihalo(3), ohalo(3), ipad(3), opad(3)
      integer(c_intptr_t), value :: stream
      integer(c_int) :: res
    end function cudecompAmdTransposeFieldsXToY_C

    function cudecompAmdTransposeFieldsYToZ_C(handle, grid_desc, inputs, outputs, n_fields, work, dtype, ihalo, ohalo, ipad, opad, &
                                                stream) bind(C, name="cudecompAmdTransposeFieldsYToZ") result(res)
      import
      type(cudecompHandle), value :: handle
      type(cudecompGridDesc), value :: grid_desc
      type(c_ptr) :: inputs(*), outputs(*)
      integer(c_int32_t), value :: n_fields
      type(c_ptr), value :: work
      integer(c_int), value :: dtype
      integer(c_int32_t) :: ihalo(3), ohalo(3), ipad(3), opad(3)
      integer(c_intptr_t), value :: stream
      integer(c_int) :: res
    end function cudecompAmdTransposeFieldsYToZ_C

    function cudecompAmdTransposeFieldsZToY_C(handle, grid_desc, inputs, outputs, n_fields, work, dtype, ihalo, ohalo, ipad, opad, &
                                                stream) bind(C, name="cudecompAmdTransposeFieldsZToY") result(res)
      import
      type(cudecompHandle), value :: handle
      type(cudecompGridDesc), value :: grid_desc
      type(c_ptr) :: inputs(*), outputs(*)
      integer(c_int32_t), value :: n_fields
      type(c_ptr), value :: work
      integer(c_int), value :: dtype
      integer(c_int32_t) :: ihalo(3), ohalo(3), ipad(3), opad(3)
      integer(c_intptr_t), value :: stream
      integer(c_int) :: res
    end function cudecompAmdTransposeFieldsZToY_C

    function cudecompAmdTransposeFieldsYToX_C(handle, grid_desc, inputs, outputs, n_fields, work, dtype, ihalo, ohalo, ipad, opad, &
                                                stream) bind(C, name="cudecompAmdTransposeFieldsYToX") result(res)
      import
      type(cudecompHandle), value :: handle
      type(cudecompGridDesc), value :: grid_desc
      type(c_ptr) :: inputs(*), outputs(*)
      integer(c_int32_t), value :: n_fields
      type(c_ptr), value :: work
      integer(c_int), value :: dtype
      integer(c_int32_t) :: ihalo(3), ohalo(3), ipad(3), opad(3)
      integer(c_intptr_t), value :: stream
      integer(c_int) :: res
    end function cudecompAmdTransposeFieldsYToX_C

    function cudecomp_c_strlen(str) bind(C, name="strlen") result(n)
      import
      type(c_ptr), value :: str
      integer(c_size_t) :: n
    end function cudecomp_c_strlen
  end interface

contains

  ! ---- initialisation --------------------------------------------------------------------------------------
  ! `comm` is a Fortran MPI communicator handle (mpif.h / `use mpi`).  The non-MPI flavour of the library
  ! discovers its ranks from the launcher environment and only accepts the world communicator.
  function cudecompInit_comm_int(handle, comm) result(res)
    type(cudecompHandle) :: handle
    integer :: comm
    integer(c_int) :: res
    res = cudecompInit_FC(handle, int(comm, c_int))
  end function cudecompInit_comm_int

  ! `use mpi_f08` communicators: type(MPI_Comm) is a BIND(C) type with the single component MPI_VAL, so a
  ! structurally identical local definition names the same type.
  function cudecompInit_comm_f08(handle, comm) result(res)
    type, bind(c) :: MPI_Comm
      integer :: MPI_VAL
    end type MPI_Comm
    type(cudecompHandle) :: handle
    type(MPI_Comm) :: comm
    integer(c_int) :: res
    res = cudecompInit_FC(handle, int(comm%MPI_VAL, c_int))
  end function cudecompInit_comm_f08

  ! ---- configuration structs -------------------------------------------------------------------------------
  function cudecompGridDescConfigSetDefaults(config) result(res)
    type(cudecompGridDescConfig), target :: config
    integer(c_int) :: res
    res = cudecompGridDescConfigSetDefaultsC(c_loc(config), c_sizeof(config), STRUCT_VERSION)
    ! the C default is -1 ("unset") and stays -1 here: only valid orders are shifted to one-based on the way
    ! in and out, see cudecompGridDescCreate
  end function cudecompGridDescConfigSetDefaults

  function cudecompGridDescAutotuneOptionsSetDefaults(options) result(res)
    type(cudecompGridDescAutotuneOptions), target :: options
    integer(c_int) :: res
    res = cudecompGridDescAutotuneOptionsSetDefaultsC(c_loc(options), c_sizeof(options), STRUCT_VERSION)
    options%halo_axis = options%halo_axis + 1
  end function cudecompGridDescAutotuneOptionsSetDefaults

  ! config is in/out (autotuned pdims / backends are written back); options is optional
  function cudecompGridDescCreate(handle, grid_desc, config, options) result(res)
    type(cudecompHandle) :: handle
    type(cudecompGridDesc) :: grid_desc
    type(cudecompGridDescConfig), target :: config
    type(cudecompGridDescAutotuneOptions), optional, target :: options
    integer(c_int) :: res

    ! one-based -> zero-based.  "unset" (-1 from SetDefaults) becomes -2, which the library treats like any
    ! negative entry: unset when the whole table is, invalid otherwise -- same as the reference module.
    config%transpose_mem_order = config%transpose_mem_order - 1
    if (present(options)) then
      options%halo_axis = options%halo_axis - 1
      res = cudecompGridDescCreateC(handle, grid_desc, c_loc(config), c_sizeof(config), STRUCT_VERSION, &
                                    c_loc(options), c_sizeof(options), STRUCT_VERSION)
      options%halo_axis = options%halo_axis + 1
    else
      res = cudecompGridDescCreateC(handle, grid_desc, c_loc(config), c_sizeof(config), STRUCT_VERSION, &
                                    c_null_ptr, 0_c_int64_t, 0_c_int32_t)
    end if
    config%transpose_mem_order = config%transpose_mem_order + 1
  end function cudecompGridDescCreate

  function cudecompGetGridDescConfig(handle, grid_desc, config) result(res)
    type(cudecompHandle) :: handle
    type(cudecompGridDesc) :: grid_desc
    type(cudecompGridDescConfig), target :: config
    integer(c_int) :: res
    res = cudecompGetGridDescConfigC(handle, grid_desc, c_loc(config), c_sizeof(config), STRUCT_VERSION)
    config%transpose_mem_order = config%transpose_mem_order + 1
  end function cudecompGetGridDescConfig

  ! ---- geometry queries -------------------------------------------------------------------------------------
  function cudecompGetPencilInfo(handle, grid_desc, pencil_info, axis, halo_extents, padding) result(res)
    type(cudecompHandle) :: handle
    type(cudecompGridDesc) :: grid_desc
    type(cudecompPencilInfo), target :: pencil_info  ! order, lo, hi come back one-based
    integer :: axis                                  ! 1/2/3 = x/y/z
    integer, optional :: halo_extents(3), padding(3)
    integer(c_int) :: res
    integer(c_int32_t) :: h(3), p(3)
    h = 0
    p = 0
    if (present(halo_extents)) h = int(halo_extents, c_int32_t)
    if (present(padding)) p = int(padding, c_int32_t)
    res = cudecompGetPencilInfoC(handle, grid_desc, c_loc(pencil_info), c_sizeof(pencil_info), STRUCT_VERSION, &
                                 int(axis - 1, c_int32_t), h, p)
    if (res /= CUDECOMP_RESULT_SUCCESS) return
    pencil_info%order = pencil_info%order + 1
    pencil_info%lo = pencil_info%lo + 1
    pencil_info%hi = pencil_info%hi + 1
  end function cudecompGetPencilInfo

  function cudecompGetHaloWorkspaceSize(handle, grid_desc, axis, halo_extents, workspace_size) result(res)
    type(cudecompHandle) :: handle
    type(cudecompGridDesc) :: grid_desc
    integer :: axis
    integer :: halo_extents(3)
    integer(int64) :: workspace_size
    integer(c_int) :: res
    integer(c_int32_t) :: h(3)
    h = int(halo_extents, c_int32_t)
    res = cudecompGetHaloWorkspaceSizeC(handle, grid_desc, int(axis - 1, c_int32_t), h, workspace_size)
  end function cudecompGetHaloWorkspaceSize

  function cudecompGetShiftedRank(handle, grid_desc, axis, dim, displacement, periodic, shifted_rank) result(res)
    type(cudecompHandle) :: handle
    type(cudecompGridDesc) :: grid_desc
    integer :: axis, dim, displacement
    logical :: periodic
    integer(c_int32_t) :: shifted_rank
    integer(c_int) :: res
    logical(c_bool) :: periodic_c
    periodic_c = periodic
    res = cudecompGetShiftedRankC(handle, grid_desc, int(axis - 1, c_int32_t), int(dim - 1, c_int32_t), &
                                  int(displacement, c_int32_t), periodic_c, shifted_rank)
  end function cudecompGetShiftedRank

  function cudecompTransposeCommBackendToString(comm_backend) result(res)
    integer :: comm_backend
    character(len=:), allocatable :: res
    call c_string_to_fortran(cudecompTransposeCommBackendToStringC(int(comm_backend, c_int)), res)
  end function cudecompTransposeCommBackendToString

  function cudecompHaloCommBackendToString(comm_backend) result(res)
    integer :: comm_backend
    character(len=:), allocatable :: res
    call c_string_to_fortran(cudecompHaloCommBackendToStringC(int(comm_backend, c_int)), res)
  end function cudecompHaloCommBackendToString

  subroutine c_string_to_fortran(cstr, fstr)
    type(c_ptr), intent(in) :: cstr
    character(len=:), allocatable, intent(out) :: fstr
    character(kind=c_char), pointer :: chars(:)
    integer :: i, n
    if (.not. c_associated(cstr)) then
      fstr = ""
      return
    end if
    n = int(cudecomp_c_strlen(cstr))
    call c_f_pointer(cstr, chars, [n])
    allocate (character(len=n) :: fstr)
    do i = 1, n
      fstr(i:i) = chars(i)
    end do
  end subroutine c_string_to_fortran

  ! ---- workspace allocation -----------------------------------------------------------------------------------
  ! buffer_size counts ELEMENTS of the pointer's type (reference :677-740).  The returned pointer addresses
  ! device memory: pass it to the transposes / halo updates / device kernels, never index it on the host.
  function cudecompMallocR4(handle, grid_desc, buffer, buffer_size) result(res)
    type(cudecompHandle) :: handle
    type(cudecompGridDesc) :: grid_desc
    real(real32), pointer, contiguous :: buffer(:)
    integer(int64) :: buffer_size
    integer(c_int) :: res
    type(c_ptr) :: p
    p = c_null_ptr
    res = cudecompMallocC(handle, grid_desc, p, int(buffer_size * 4, c_size_t))
    call c_f_pointer(p, buffer, [buffer_size])
  end function cudecompMallocR4

  function cudecompMallocR8(handle, grid_desc, buffer, buffer_size) result(res)
    type(cudecompHandle) :: handle
    type(cudecompGridDesc) :: grid_desc
    real(real64), pointer, contiguous :: buffer(:)
    integer(int64) :: buffer_size
    integer(c_int) :: res
    type(c_ptr) :: p
    p = c_null_ptr
    res = cudecompMallocC(handle, grid_desc, p, int(buffer_size * 8, c_size_t))
    call c_f_pointer(p, buffer, [buffer_size])
  end function cudecompMallocR8

  function cudecompMallocC4(handle, grid_desc, buffer, buffer_size) result(res)
    type(cudecompHandle) :: handle
    type(cudecompGridDesc) :: grid_desc
    complex(real32), pointer, contiguous :: buffer(:)
    integer(int64) :: buffer_size
    integer(c_int) :: res
    type(c_ptr) :: p
    p = c_null_ptr
    res = cudecompMallocC(handle, grid_desc, p, int(buffer_size * 8, c_size_t))
    call c_f_pointer(p, buffer, [buffer_size])
  end function cudecompMallocC4

  function cudecompMallocC8(handle, grid_desc, buffer, buffer_size) result(res)
    type(cudecompHandle) :: handle
    type(cudecompGridDesc) :: grid_desc
    complex(real64), pointer, contiguous :: buffer(:)
    integer(int64) :: buffer_size
    integer(c_int) :: res
    type(c_ptr) :: p
    p = c_null_ptr
    res = cudecompMallocC(handle, grid_desc, p, int(buffer_size * 16, c_size_t))
    call c_f_pointer(p, buffer, [buffer_size])
  end function cudecompMallocC8

  ! raw form for codes that keep device memory as type(c_ptr) (hipfort style); size in BYTES
  function cudecompMallocPtr(handle, grid_desc, buffer, buffer_size_bytes) result(res)
    type(cudecompHandle) :: handle
    type(cudecompGridDesc) :: grid_desc
    type(c_ptr) :: buffer
    integer(int64) :: buffer_size_bytes
    integer(c_int) :: res
    buffer = c_null_ptr
    res = cudecompMallocC(handle, grid_desc, buffer, int(buffer_size_bytes, c_size_t))
  end function cudecompMallocPtr

  function cudecompFreeR4(handle, grid_desc, buffer) result(res)
    type(cudecompHandle) :: handle
    type(cudecompGridDesc) :: grid_desc
    real(real32), pointer, contiguous :: buffer(:)
    integer(c_int) :: res
    res = cudecompFreeC(handle, grid_desc, c_loc(buffer))
    nullify (buffer)
  end function cudecompFreeR4

  function cudecompFreeR8(handle, grid_desc, buffer) result(res)
    type(cudecompHandle) :: handle
    type(cudecompGridDesc) :: grid_desc
    real(real64), pointer, contiguous :: buffer(:)
    integer(c_int) :: res
    res = cudecompFreeC(handle, grid_desc, c_loc(buffer))
    nullify (buffer)
  end function cudecompFreeR8

  function cudecompFreeC4(handle, grid_desc, buffer) result(res)
    type(cudecompHandle) :: handle
    type(cudecompGridDesc) :: grid_desc
    complex(real32), pointer, contiguous :: buffer(:)
    integer(c_int) :: res
    res = cudecompFreeC(handle, grid_desc, c_loc(buffer))
    nullify (buffer)
  end function cudecompFreeC4

  function cudecompFreeC8(handle, grid_desc, buffer) result(res)
    type(cudecompHandle) :: handle
    type(cudecompGridDesc) :: grid_desc
    complex(real64), pointer, contiguous :: buffer(:)
    integer(c_int) :: res
    res = cudecompFreeC(handle, grid_desc, c_loc(buffer))
    nullify (buffer)
  end function cudecompFreeC8

  function cudecompFreePtr(handle, grid_desc, buffer) result(res)
    type(cudecompHandle) :: handle
    type(cudecompGridDesc) :: grid_desc
    type(c_ptr) :: buffer
    integer(c_int) :: res
    res = cudecompFreeC(handle, grid_desc, buffer)
    buffer = c_null_ptr
  end function cudecompFreePtr

  ! ---- transposes -----------------------------------------------------------------------------------------------
  ! input/output/work: any array (or first element of one) whose address is a device address; type, kind and
  ! rank are not checked, `dtype` says what the elements are.  input and output may be the same array
  ! (in-place).
  function cudecompTransposeXToY(handle, grid_desc, input, output, work, dtype, input_halo_extents, &
                                 output_halo_extents, input_padding, output_padding, stream) result(res)
    type(cudecompHandle) :: handle
    type(cudecompGridDesc) :: grid_desc
    type(*), dimension(..), target :: input, output, work
    integer :: dtype
    integer, optional :: input_halo_extents(3), output_halo_extents(3), input_padding(3), output_padding(3)
    integer(cudecomp_stream_kind), optional :: stream
    integer(c_int) :: res
    integer(c_int32_t) :: ih(3), oh(3), ip(3), op(3)
    integer(c_intptr_t) :: s
    call transpose_defaults(ih, oh, ip, op, s, input_halo_extents, output_halo_extents, input_padding, &
                            output_padding, stream)
    res = cudecompTransposeXToY_C(handle, grid_desc, c_loc(input), c_loc(output), c_loc(work), int(dtype, c_int), &
                                  ih, oh, ip, op, s)
  end function cudecompTransposeXToY

  function cudecompTransposeYToZ(handle, grid_desc, input, output, work, dtype, input_halo_extents, &
                                 output_halo_extents, input_padding, output_padding, stream) result(res)
    type(cudecompHandle) :: handle
    type(cudecompGridDesc) :: grid_desc
    type(*), dimension(..), target :: input, output, work
    integer :: dtype
    integer, optional :: input_halo_extents(3), output_halo_extents(3), input_padding(3), output_padding(3)
    integer(cudecomp_stream_kind), optional :: stream
    integer(c_int) :: res
    integer(c_int32_t) :: ih(3), oh(3), ip(3), op(3)
    integer(c_intptr_t) :: s
    call transpose_defaults(ih, oh, ip, op, s, input_halo_extents, output_halo_extents, input_padding, &
                            output_padding, stream)
    res = cudecompTransposeYToZ_C(handle, grid_desc, c_loc(input), c_loc(output), c_loc(work), int(dtype, c_int), &
                                  ih, oh, ip, op, s)
  end function cudecompTransposeYToZ

  function cudecompTransposeZToY(handle, grid_desc, input, output, work, dtype, input_halo_extents, &
                                 output_halo_extents, input_padding, output_padding, stream) result(res)
    type(cudecompHandle) :: handle
    type(cudecompGridDesc) :: grid_desc
    type(*), dimension(..), target :: input, output, work
    integer :: dtype
    integer, optional :: input_halo_extents(3), output_halo_extents(3), input_padding(3), output_padding(3)
    integer(cudecomp_stream_kind), optional :: stream
    integer(c_int) :: res
    integer(c_int32_t) :: ih(3), oh(3), ip(3), op(3)
    integer(c_intptr_t) :: s
    call transpose_defaults(ih, oh, ip, op, s, input_halo_extents, output_halo_extents, input_padding, &
                            output_padding, stream)
    res = cudecompTransposeZToY_C(handle, grid_desc, c_loc(input), c_loc(output), c_loc(work), int(dtype, c_int), &
                                  ih, oh, ip, op, s)
  end function cudecompTransposeZToY

  function cudecompTransposeYToX(handle, grid_desc, input, output, work, dtype, input_halo_extents, &
                                 output_halo_extents, input_padding, output_padding, stream) result(res)
    type(cudecompHandle) :: handle
    type(cudecompGridDesc) :: grid_desc
    type(*), dimension(..), target :: input, output, work
    integer :: dtype
    integer, optional :: input_halo_extents(3), output_halo_extents(3), input_padding(3), output_padding(3)
    integer(cudecomp_stream_kind), optional :: stream
    integer(c_int) :: res
    integer(c_int32_t) :: ih(3), oh(3), ip(3), op(3)
    integer(c_intptr_t) :: s
    call transpose_defaults(ih, oh, ip, op, s, input_halo_extents, output_halo_extents, input_padding, &
                            output_padding, stream)
    res = cudecompTransposeYToX_C(handle, grid_desc, c_loc(input), c_loc(output), c_loc(work), int(dtype, c_int), &
                                  ih, oh, ip, op, s)
  end function cudecompTransposeYToX

  subroutine transpose_defaults(ih, oh, ip, op, s, input_halo_extents, output_halo_extents, input_padding, &
                                output_padding, stream)
    integer(c_int32_t), intent(out) :: ih(3), oh(3), ip(3), op(3)
    integer(c_intptr_t), intent(out) :: s
    integer, optional, intent(in) :: input_halo_extents(3), output_halo_extents(3), input_padding(3), &
                                     output_padding(3)
    integer(cudecomp_stream_kind), optional, intent(in) :: stream
    ih = 0
    oh = 0
    ip = 0
    op = 0
    s = 0
    if (present(input_halo_extents)) ih = int(input_halo_extents, c_int32_t)
    if (present(output_halo_extents)) oh = int(output_halo_extents, c_int32_t)
    if (present(input_padding)) ip = int(input_padding, c_int32_t)
    if (present(output_padding)) op = int(output_padding, c_int32_t)
    if (present(stream)) s = stream
  end subroutine transpose_defaults

  ! ---- halo updates ---------------------------------------------------------------------------------------------
  function cudecompUpdateHalosX(handle, grid_desc, input, work, dtype, halo_extents, halo_periods, dim, padding, &
                                stream) result(res)
    type(cudecompHandle) :: handle
    type(cudecompGridDesc) :: grid_desc
    type(*), dimension(..), target :: input, work
    integer :: dtype
    integer :: halo_extents(3)
    logical :: halo_periods(3)
    integer :: dim  ! 1/2/3 = x/y/z
    integer, optional :: padding(3)
    integer(cudecomp_stream_kind), optional :: stream
    integer(c_int) :: res
    integer(c_int32_t) :: h(3), p(3)
    logical(c_bool) :: per(3)
    integer(c_intptr_t) :: s
    call halo_defaults(h, per, p, s, halo_extents, halo_periods, padding, stream)
    res = cudecompUpdateHalosX_C(handle, grid_desc, c_loc(input), c_loc(work), int(dtype, c_int), h, per, &
                                 int(dim - 1, c_int32_t), p, s)
  end function cudecompUpdateHalosX

  function cudecompUpdateHalosY(handle, grid_desc, input, work, dtype, halo_extents, halo_periods, dim, padding, &
                                stream) result(res)
    type(cudecompHandle) :: handle
    type(cudecompGridDesc) :: grid_desc
    type(*), dimension(..), target :: input, work
    integer :: dtype
    integer :: halo_extents(3)
    logical :: halo_periods(3)
    integer :: dim
    integer, optional :: padding(3)
    integer(cudecomp_stream_kind), optional :: stream
    integer(c_int) :: res
    integer(c_int32_t) :: h(3), p(3)
    logical(c_bool) :: per(3)
    integer(c_intptr_t) :: s
    call halo_defaults(h, per, p, s, halo_extents, halo_periods, padding, stream)
    res = cudecompUpdateHalosY_C(handle, grid_desc, c_loc(input), c_loc(work), int(dtype, c_int), h, per, &
                                 int(dim - 1, c_int32_t), p, s)
  end function cudecompUpdateHalosY

  function cudecompUpdateHalosZ(handle, grid_desc, input, work, dtype, halo_extents, halo_periods, dim, padding, &
                                stream) result(res)
    type(cudecompHandle) :: handle
    type(cudecompGridDesc) :: grid_desc
    type(*), dimension(..), target :: input, work
    integer :: dtype
    integer :: halo_extents(3)
    logical :: halo_periods(3)
    integer :: dim
    integer, optional :: padding(3)
    integer(cudecomp_stream_kind), optional :: stream
    integer(c_int) :: res
    integer(c_int32_t) :: h(3), p(3)
    logical(c_bool) :: per(3)
    integer(c_intptr_t) :: s
    call halo_defaults(h, per, p, s, halo_extents, halo_periods, padding, stream)
    res = cudecompUpdateHalosZ_C(handle, grid_desc, c_loc(input), c_loc(work), int(dtype, c_int), h, per, &
                                 int(dim - 1, c_int32_t), p, s)
  end function cudecompUpdateHalosZ

  ! ---- halo accumulation (cudecomp_amd.h): same arguments as the updates ----------------------------------------
  function cudecompAmdAccumulateHalosX(handle, grid_desc, input, work, dtype, halo_extents, halo_periods, dim, padding, &
                                       stream) result(res)
    type(cudecompHandle) :: handle
    type(cudecompGridDesc) :: grid_desc
    type(*), dimension(..), target :: input, work
    integer :: dtype
    integer :: halo_extents(3)
    logical :: halo_periods(3)
    integer :: dim  ! 1/2/3 = x/y/z
    integer, optional :: padding(3)
    integer(cudecomp_stream_kind), optional :: stream
    integer(c_int) :: res
    integer(c_int32_t) :: h(3), p(3)
    logical(c_bool) :: per(3)
    integer(c_intptr_t) :: s
    call halo_defaults(h, per, p, s, halo_extents, halo_periods, padding, stream)
    res = cudecompAmdAccumulateHalosX_C(handle, grid_desc, c_loc(input), c_loc(work), int(dtype, c_int), h, per, &
                                        int(dim - 1, c_int32_t), p, s)
  end function cudecompAmdAccumulateHalosX

  function cudecompAmdAccumulateHalosY(handle, grid_desc, input, work, dtype, halo_extents, halo_periods, dim, padding, &
                                       stream) result(res)
    type(cudecompHandle) :: handle
    type(cudecompGridDesc) :: grid_desc
    type(*), dimension(..), target :: input, work
    integer :: dtype
    integer :: halo_extents(3)
    logical :: halo_periods(3)
    integer :: dim
    integer, optional :: padding(3)
    integer(cudecomp_stream_kind), optional :: stream
    integer(c_int) :: res
    integer(c_int32_t) :: h(3), p(3)
    logical(c_bool) :: per(3)
    integer(c_intptr_t) :: s
    call halo_defaults(h, per, p, s, halo_extents, halo_periods, padding, stream)
    res = cudecompAmdAccumulateHalosY_C(handle, grid_desc, c_loc(input), c_loc(work), int(dtype, c_int), h, per, &
                                        int(dim - 1, c_int32_t), p, s)
  end function cudecompAmdAccumulateHalosY

  function cudecompAmdAccumulateHalosZ(handle, grid_desc, input, work, dtype, halo_extents, halo_periods, dim, padding, &
                                       stream) result(res)
    type(cudecompHandle) :: handle
    type(cudecompGridDesc) :: grid_desc
    type(*), dimension(..), target :: input, work
    integer :: dtype
    integer :: halo_extents(3)
    logical :: halo_periods(3)
    integer :: dim
    integer, optional :: padding(3)
    integer(cudecomp_stream_kind), optional :: stream
    integer(c_int) :: res
    integer(c_int32_t) :: h(3), p(3)
    logical(c_bool) :: per(3)
    integer(c_intptr_t) :: s
    call halo_defaults(h, per, p, s, halo_extents, halo_periods, padding, stream)
    res = cudecompAmdAccumulateHalosZ_C(handle, grid_desc, c_loc(input), c_loc(work), int(dtype, c_int), h, per, &
                                        int(dim - 1, c_int32_t), p, s)
  end function cudecompAmdAccumulateHalosZ

  ! ---- halo fill (cudecomp_amd_fill.h): the arguments of the updates without work, plus an optional value ---------
  function cudecompAmdFillHalosX(handle, grid_desc, input, dtype, halo_extents, halo_periods, dim, padding, stream, &
                                 value) result(res)
    type(cudecompHandle) :: handle
    type(cudecompGridDesc) :: grid_desc
    type(*), dimension(..), target :: input
    integer :: dtype
    integer :: halo_extents(3)
    logical :: halo_periods(3)
    integer :: dim  ! 1/2/3 = x/y/z
    integer, optional :: padding(3)
    integer(cudecomp_stream_kind), optional :: stream
    type(*), target, optional :: value  ! one element of dtype, read before the call returns; absent: zero bytes
    integer(c_int) :: res
    integer(c_int32_t) :: h(3), p(3)
    logical(c_bool) :: per(3)
    integer(c_intptr_t) :: s
    type(c_ptr) :: v
    call halo_defaults(h, per, p, s, halo_extents, halo_periods, padding, stream)
    v = c_null_ptr
    if (present(value)) v = c_loc(value)
    res = cudecompAmdFillHalosX_C(handle, grid_desc, c_loc(input), int(dtype, c_int), v, h, per, int(dim - 1, c_int32_t), p, s)
  end function cudecompAmdFillHalosX

  function cudecompAmdFillHalosY(handle, grid_desc, input, dtype, halo_extents, halo_periods, dim, padding, stream, &
                                 value) result(res)
    type(cudecompHandle) :: handle
    type(cudecompGridDesc) :: grid_desc
    type(*), dimension(..), target :: input
    integer :: dtype
    integer :: halo_extents(3)
    logical :: halo_periods(3)
    integer :: dim
    integer, optional :: padding(3)
    integer(cudecomp_stream_kind), optional :: stream
    type(*), target, optional :: value
    integer(c_int) :: res
    integer(c_int32_t) :: h(3), p(3)
    logical(c_bool) :: per(3)
    integer(c_intptr_t) :: s
    type(c_ptr) :: v
    call halo_defaults(h, per, p, s, halo_extents, halo_periods, padding, stream)
    v = c_null_ptr
    if (present(value)) v = c_loc(value)
    res = cudecompAmdFillHalosY_C(handle, grid_desc, c_loc(input), int(dtype, c_int), v, h, per, int(dim - 1, c_int32_t), p, s)
  end function cudecompAmdFillHalosY

  function cudecompAmdFillHalosZ(handle, grid_desc, input, dtype, halo_extents, halo_periods, dim, padding, stream, &
                                 value) result(res)
    type(cudecompHandle) :: handle
    type(cudecompGridDesc) :: grid_desc
    type(*), dimension(..), target :: input
    integer :: dtype
    integer :: halo_extents(3)
    logical :: halo_periods(3)
    integer :: dim
    integer, optional :: padding(3)
    integer(cudecomp_stream_kind), optional :: stream
    type(*), target, optional :: value
    integer(c_int) :: res
    integer(c_int32_t) :: h(3), p(3)
    logical(c_bool) :: per(3)
    integer(c_intptr_t) :: s
    type(c_ptr) :: v
    call halo_defaults(h, per, p, s, halo_extents, halo_periods, padding, stream)
    v = c_null_ptr
    if (present(value)) v = c_loc(value)
    res = cudecompAmdFillHalosZ_C(handle, grid_desc, c_loc(input), int(dtype, c_int), v, h, per, int(dim - 1, c_int32_t), p, s)
  end function cudecompAmdFillHalosZ

  ! ---- halo accumulate-and-clear (cudecomp_amd_fill.h): same arguments as the accumulation --------------------------
  function cudecompAmdAccumulateAndClearHalosX(handle, grid_desc, input, work, dtype, halo_extents, &
      halo_periods, dim, padding, &
                                       stream) result(res)
    type(cudecompHandle) :: handle
    type(cudecompGridDesc) :: grid_desc
    type(*), dimension(..), target :: input, work
    integer :: dtype
    integer :: halo_extents(3)
    logical :: halo_periods(3)
    integer :: dim  ! 1/2/3 = x/y/z
    integer, optional :: padding(3)
    integer(cudecomp_stream_kind), optional :: stream
    integer(c_int) :: res
    integer(c_int32_t) :: h(3), p(3)
    logical(c_bool) :: per(3)
    integer(c_intptr_t) :: s
    call halo_defaults(h, per, p, s, halo_extents, halo_periods, padding, stream)
    res = cudecompAmdAccumulateAndClearHalosX_C(handle, grid_desc, c_loc(input), c_loc(work), int(dtype, c_int), h, per, &
                                        int(dim - 1, c_int32_t), p, s)
  end function cudecompAmdAccumulateAndClearHalosX

  function cudecompAmdAccumulateAndClearHalosY(handle, grid_desc, input, work, dtype, halo_extents, &
      halo_periods, dim, padding, &
                                       stream) result(res)
    type(cudecompHandle) :: handle
    type(cudecompGridDesc) :: grid_desc
    type(*), dimension(..), target :: input, work
    integer :: dtype
    integer :: halo_extents(3)
    logical :: halo_periods(3)
    integer :: dim
    integer, optional :: padding(3)
    integer(cudecomp_stream_kind), optional :: stream
    integer(c_int) :: res
    integer(c_int32_t) :: h(3), p(3)
    logical(c_bool) :: per(3)
    integer(c_intptr_t) :: s
    call halo_defaults(h, per, p, s, halo_extents, halo_periods, padding, stream)
    res = cudecompAmdAccumulateAndClearHalosY_C(handle, grid_desc, c_loc(input), c_loc(work), int(dtype, c_int), h, per, &
                                        int(dim - 1, c_int32_t), p, s)
  end function cudecompAmdAccumulateAndClearHalosY

  function cudecompAmdAccumulateAndClearHalosZ(handle, grid_desc, input, work, dtype, halo_extents, &
      halo_periods, dim, padding, &
                                       stream) result(res)
    type(cudecompHandle) :: handle
    type(cudecompGridDesc) :: grid_desc
    type(*), dimension(..), target :: input, work
    integer :: dtype
    integer :: halo_extents(3)
    logical :: halo_periods(3)
    integer :: dim
    integer, optional :: padding(3)
    integer(cudecomp_stream_kind), optional :: stream
    integer(c_int) :: res
    integer(c_int32_t) :: h(3), p(3)
    logical(c_bool) :: per(3)
    integer(c_intptr_t) :: s
    call halo_defaults(h, per, p, s, halo_extents, halo_periods, padding, stream)
    res = cudecompAmdAccumulateAndClearHalosZ_C(handle, grid_desc, c_loc(input), c_loc(work), int(dtype, c_int), h, per, &
                                        int(dim - 1, c_int32_t), p, s)
  end function cudecompAmdAccumulateAndClearHalosZ

  ! ---- halo reflection (cudecomp_amd_reflect.h): the arguments of the fill with parity and centering in the place of the value ----
  function cudecompAmdReflectHalosX(handle, grid_desc, input, dtype, parity, centering, halo_extents, halo_periods, dim, &
                                    padding, stream) result(res)
    type(cudecompHandle) :: handle
    type(cudecompGridDesc) :: grid_desc
    type(*), dimension(..), target :: input
    integer :: dtype
    integer :: parity     ! +1: even mirror; -1: odd mirror (sign bits flipped)
    integer :: centering  ! 0: about the face between ghost and interior cells; 1: about the first / last interior cell
    integer :: halo_extents(3)
    logical :: halo_periods(3)
    integer :: dim  ! 1/2/3 = x/y/z
    integer, optional :: padding(3)
    integer(cudecomp_stream_kind), optional :: stream
    integer(c_int) :: res
    integer(c_int32_t) :: h(3), p(3)
    logical(c_bool) :: per(3)
    integer(c_intptr_t) :: s
    call halo_defaults(h, per, p, s, halo_extents, halo_periods, padding, stream)
    res = cudecompAmdReflectHalosX_C(handle, grid_desc, c_loc(input), int(dtype, c_int), int(parity, c_int32_t), &
                                      int(centering, c_int32_t), h, per, int(dim - 1, c_int32_t), p, s)
  end function cudecompAmdReflectHalosX

  function cudecompAmdReflectHalosY(handle, grid_desc, input, dtype, parity, centering, halo_extents, halo_periods, dim, &
                                    padding, stream) result(res)
    type(cudecompHandle) :: handle
    type(cudecompGridDesc) :: grid_desc
    type(*), dimension(..), target :: input
    integer :: dtype
    integer :: parity     ! +1: even mirror; -1: odd mirror (sign bits flipped)
    integer :: centering  ! 0: about the face between ghost and interior cells; 1: about the first / last interior cell
    integer :: halo_extents(3)
    logical :: halo_periods(3)
    integer :: dim  ! 1/2/3 = x/y/z
    integer, optional :: padding(3)
    integer(cudecomp_stream_kind), optional :: stream
    integer(c_int) :: res
    integer(c_int32_t) :: h(3), p(3)
    logical(c_bool) :: per(3)
    integer(c_intptr_t) :: s
    call halo_defaults(h, per, p, s, halo_extents, halo_periods, padding, stream)
    res = cudecompAmdReflectHalosY_C(handle, grid_desc, c_loc(input), int(dtype, c_int), int(parity, c_int32_t), &
                                      int(centering, c_int32_t), h, per, int(dim - 1, c_int32_t), p, s)
  end function cudecompAmdReflectHalosY

  function cudecompAmdReflectHalosZ(handle, grid_desc, input, dtype, parity, centering, halo_extents, halo_periods, dim, &
                                    padding, stream) result(res)
    type(cudecompHandle) :: handle
    type(cudecompGridDesc) :: grid_desc
    type(*), dimension(..), target :: input
    integer :: dtype
    integer :: parity     ! +1: even mirror; -1: odd mirror (sign bits flipped)
    integer :: centering  ! 0: about the face between ghost and interior cells; 1: about the first / last interior cell
    integer :: halo_extents(3)
    logical :: halo_periods(3)
    integer :: dim  ! 1/2/3 = x/y/z
    integer, optional :: padding(3)
    integer(cudecomp_stream_kind), optional :: stream
    integer(c_int) :: res
    integer(c_int32_t) :: h(3), p(3)
    logical(c_bool) :: per(3)
    integer(c_intptr_t) :: s
    call halo_defaults(h, per, p, s, halo_extents, halo_periods, padding, stream)
    res = cudecompAmdReflectHalosZ_C(handle, grid_desc, c_loc(input), int(dtype, c_int), int(parity, c_int32_t), &
                                      int(centering, c_int32_t), h, per, int(dim - 1, c_int32_t), p, s)
  end function cudecompAmdReflectHalosZ

  ! ---- wall values (cudecomp_halo_wall_values.h): the arguments of the reflection with `sides` and the two host arrays of
  ! addends after the centering ----
  function cudecompAmdSetWallHalosX(handle, grid_desc, input, dtype, parity, centering, sides, values_low, values_high, &
                                    halo_extents, halo_periods, dim, padding, stream) result(res)
    type(cudecompHandle) :: handle
    type(cudecompGridDesc) :: grid_desc
    type(*), dimension(..), target :: input
    integer :: dtype
    integer :: parity     ! +1: even mirror; -1: odd mirror (sign bits flipped)
    integer :: centering  ! 0: about the face between ghost and interior cells; 1: about the first / last interior cell
    integer :: sides      ! 1: the low halo; 2: the high halo; 3: both
    ! halo_extents(dim) doubles per side (complex types: twice as many, re and im interleaved), layer 1 next to the wall; host
    ! arrays, read before the call returns; the one of a side that `sides` does not name may be left out
    real(c_double), optional, target :: values_low(*), values_high(*)
    integer :: halo_extents(3)
    logical :: halo_periods(3)
    integer :: dim  ! 1/2/3 = x/y/z
    integer, optional :: padding(3)
    integer(cudecomp_stream_kind), optional :: stream
    integer(c_int) :: res
    integer(c_int32_t) :: h(3), p(3)
    logical(c_bool) :: per(3)
    integer(c_intptr_t) :: s
    type(c_ptr) :: lo, hi
    call halo_defaults(h, per, p, s, halo_extents, halo_periods, padding, stream)
    lo = c_null_ptr
    hi = c_null_ptr
    if (present(values_low)) lo = c_loc(values_low)
    if (present(values_high)) hi = c_loc(values_high)
    res = cudecompAmdSetWallHalosX_C(handle, grid_desc, c_loc(input), int(dtype, c_int), int(parity, c_int32_t), &
                                      int(centering, c_int32_t), int(sides, c_int32_t), lo, hi, h, per, int(dim - 1, c_int32_t), p, s)
  end function cudecompAmdSetWallHalosX

  function cudecompAmdSetWallHalosY(handle, grid_desc, input, dtype, parity, centering, sides, values_low, values_high, &
                                    halo_extents, halo_periods, dim, padding, stream) result(res)
    type(cudecompHandle) :: handle
    type(cudecompGridDesc) :: grid_desc
    type(*), dimension(..), target :: input
    integer :: dtype
    integer :: parity     ! +1: even mirror; -1: odd mirror (sign bits flipped)
    integer :: centering  ! 0: about the face between ghost and interior cells; 1: about the first / last interior cell
    integer :: sides      ! 1: the low halo; 2: the high halo; 3: both
    ! halo_extents(dim) doubles per side (complex types: twice as many, re and im interleaved), layer 1 next to the wall; host
    ! arrays, read before the call returns; the one of a side that `sides` does not name may be left out
    real(c_double), optional, target :: values_low(*), values_high(*)
    integer :: halo_extents(3)
    logical :: halo_periods(3)
    integer :: dim  ! 1/2/3 = x/y/z
    integer, optional :: padding(3)
    integer(cudecomp_stream_kind), optional :: stream
    integer(c_int) :: res
    integer(c_int32_t) :: h(3), p(3)
    logical(c_bool) :: per(3)
    integer(c_intptr_t) :: s
    type(c_ptr) :: lo, hi
    call halo_defaults(h, per, p, s, halo_extents, halo_periods, padding, stream)
    lo = c_null_ptr
    hi = c_null_ptr
    if (present(values_low)) lo = c_loc(values_low)
    if (present(values_high)) hi = c_loc(values_high)
    res = cudecompAmdSetWallHalosY_C(handle, grid_desc, c_loc(input), int(dtype, c_int), int(parity, c_int32_t), &
                                      int(centering, c_int32_t), int(sides, c_int32_t), lo, hi, h, per, int(dim - 1, c_int32_t), p, s)
  end function cudecompAmdSetWallHalosY

  function cudecompAmdSetWallHalosZ(handle, grid_desc, input, dtype, parity, centering, sides, values_low, values_high, &
                                    halo_extents, halo_periods, dim, padding, stream) result(res)
    type(cudecompHandle) :: handle
    type(cudecompGridDesc) :: grid_desc
    type(*), dimension(..), target :: input
    integer :: dtype
    integer :: parity     ! +1: even mirror; -1: odd mirror (sign bits flipped)
    integer :: centering  ! 0: about the face between ghost and interior cells; 1: about the first / last interior cell
    integer :: sides      ! 1: the low halo; 2: the high halo; 3: both
    ! halo_extents(dim) doubles per side (complex types: twice as many, re and im interleaved), layer 1 next to the wall; host
    ! arrays, read before the call returns; the one of a side that `sides` does not name may be left out
    real(c_double), optional, target :: values_low(*), values_high(*)
    integer :: halo_extents(3)
    logical :: halo_periods(3)
    integer :: dim  ! 1/2/3 = x/y/z
    integer, optional :: padding(3)
    integer(cudecomp_stream_kind), optional :: stream
    integer(c_int) :: res
    integer(c_int32_t) :: h(3), p(3)
    logical(c_bool) :: per(3)
    integer(c_intptr_t) :: s
    type(c_ptr) :: lo, hi
    call halo_defaults(h, per, p, s, halo_extents, halo_periods, padding, stream)
    lo = c_null_ptr
    hi = c_null_ptr
    if (present(values_low)) lo = c_loc(values_low)
    if (present(values_high)) hi = c_loc(values_high)
    res = cudecompAmdSetWallHalosZ_C(handle, grid_desc, c_loc(input), int(dtype, c_int), int(parity, c_int32_t), &
                                      int(centering, c_int32_t), int(sides, c_int32_t), lo, hi, h, per, int(dim - 1, c_int32_t), p, s)
  end function cudecompAmdSetWallHalosZ

  ! ---- wall planes (cudecomp_halo_wall_planes.h): the arguments of the wall values with two DEVICE arrays in the place of the host
  ! arrays of addends ----
  function cudecompAmdSetWallPlaneHalosX(handle, grid_desc, input, dtype, parity, centering, sides, planes_low, planes_high, &
                                         halo_extents, halo_periods, dim, padding, stream) result(res)
    type(cudecompHandle) :: handle
    type(cudecompGridDesc) :: grid_desc
    type(*), dimension(..), target :: input
    integer :: dtype
    integer :: parity     ! +1: even mirror; -1: odd mirror (sign bits flipped)
    integer :: centering  ! 0: about the face between ghost and interior cells; 1: about the first / last interior cell
    integer :: sides      ! 1: the low halo; 2: the high halo; 3: both
    ! device arrays of `dtype`: the pencil's shape with the extent along `dim` replaced by halo_extents(dim), dense in the pencil's
    ! memory order; along `dim` index 1 is the layer next to the wall.  Only read, when the kernel runs; the one of a side that
    ! `sides` does not name may be left out
    type(*), dimension(..), optional, target :: planes_low, planes_high
    integer :: halo_extents(3)
    logical :: halo_periods(3)
    integer :: dim  ! 1/2/3 = x/y/z
    integer, optional :: padding(3)
    integer(cudecomp_stream_kind), optional :: stream
    integer(c_int) :: res
    integer(c_int32_t) :: h(3), p(3)
    logical(c_bool) :: per(3)
    integer(c_intptr_t) :: s
    type(c_ptr) :: lo, hi
    call halo_defaults(h, per, p, s, halo_extents, halo_periods, padding, stream)
    lo = c_null_ptr
    hi = c_null_ptr
    if (present(planes_low)) lo = c_loc(planes_low)
    if (present(planes_high)) hi = c_loc(planes_high)
    res = cudecompAmdSetWallPlaneHalosX_C(handle, grid_desc, c_loc(input), int(dtype, c_int), int(parity, c_int32_t), &
                                           int(centering, c_int32_t), int(sides, c_int32_t), lo, hi, h, per, int(dim - 1, c_int32_t), p, s)
  end function cudecompAmdSetWallPlaneHalosX

  function cudecompAmdSetWallPlaneHalosY(handle, grid_desc, input, dtype, parity, centering, sides, planes_low, planes_high, &
                                         halo_extents, halo_periods, dim, padding, stream) result(res)
    type(cudecompHandle) :: handle
    type(cudecompGridDesc) :: grid_desc
    type(*), dimension(..), target :: input
    integer :: dtype
    integer :: parity     ! +1: even mirror; -1: odd mirror (sign bits flipped)
    integer :: centering  ! 0: about the face between ghost and interior cells; 1: about the first / last interior cell
    integer :: sides      ! 1: the low halo; 2: the high halo; 3: both
    ! device arrays of `dtype`: the pencil's shape with the extent along `dim` replaced by halo_extents(dim), dense in the pencil's
    ! memory order; along `dim` index 1 is the layer next to the wall.  Only read, when the kernel runs; the one of a side that
    ! `sides` does not name may be left out
    type(*), dimension(..), optional, target :: planes_low, planes_high
    integer :: halo_extents(3)
    logical :: halo_periods(3)
    integer :: dim  ! 1/2/3 = x/y/z
    integer, optional :: padding(3)
    integer(cudecomp_stream_kind), optional :: stream
    integer(c_int) :: res
    integer(c_int32_t) :: h(3), p(3)
    logical(c_bool) :: per(3)
    integer(c_intptr_t) :: s
    type(c_ptr) :: lo, hi
    call halo_defaults(h, per, p, s, halo_extents, halo_periods, padding, stream)
    lo = c_null_ptr
    hi = c_null_ptr
    if (present(planes_low)) lo = c_loc(planes_low)
    if (present(planes_high)) hi = c_loc(planes_high)
    res = cudecompAmdSetWallPlaneHalosY_C(handle, grid_desc, c_loc(input), int(dtype, c_int), int(parity, c_int32_t), &
                                           int(centering, c_int32_t), int(sides, c_int32_t), lo, hi, h, per, int(dim - 1, c_int32_t), p, s)
  end function cudecompAmdSetWallPlaneHalosY

  function cudecompAmdSetWallPlaneHalosZ(handle, grid_desc, input, dtype, parity, centering, sides, planes_low, planes_high, &
                                         halo_extents, halo_periods, dim, padding, stream) result(res)
    type(cudecompHandle) :: handle
    type(cudecompGridDesc) :: grid_desc
    type(*), dimension(..), target :: input
    integer :: dtype
    integer :: parity     ! +1: even mirror; -1: odd mirror (sign bits flipped)
    integer :: centering  ! 0: about the face between ghost and interior cells; 1: about the first / last interior cell
    integer :: sides      ! 1: the low halo; 2: the high halo; 3: both
    ! device arrays of `dtype`: the pencil's shape with the extent along `dim` replaced by halo_extents(dim), dense in the pencil's
    ! memory order; along `dim` index 1 is the layer next to the wall.  Only read, when the kernel runs; the one of a side that
    ! `sides` does not name may be left out
    type(*), dimension(..), optional, target :: planes_low, planes_high
    integer :: halo_extents(3)
    logical :: halo_periods(3)
    integer :: dim  ! 1/2/3 = x/y/z
    integer, optional :: padding(3)
    integer(cudecomp_stream_kind), optional :: stream
    integer(c_int) :: res
    integer(c_int32_t) :: h(3), p(3)
    logical(c_bool) :: per(3)
    integer(c_intptr_t) :: s
    type(c_ptr) :: lo, hi
    call halo_defaults(h, per, p, s, halo_extents, halo_periods, padding, stream)
    lo = c_null_ptr
    hi = c_null_ptr
    if (present(planes_low)) lo = c_loc(planes_low)
    if (present(planes_high)) hi = c_loc(planes_high)
    res = cudecompAmdSetWallPlaneHalosZ_C(handle, grid_desc, c_loc(input), int(dtype, c_int), int(parity, c_int32_t), &
                                           int(centering, c_int32_t), int(sides, c_int32_t), lo, hi, h, per, int(dim - 1, c_int32_t), p, s)
  end function cudecompAmdSetWallPlaneHalosZ

  ! ---- halo folding (cudecomp_halo_fold.h): the arguments of the reflection with `clear` after the centering ----
  function cudecompAmdFoldHalosX(handle, grid_desc, input, dtype, parity, centering, clear, halo_extents, halo_periods, dim, &
                                    padding, stream) result(res)
    type(cudecompHandle) :: handle
    type(cudecompGridDesc) :: grid_desc
    type(*), dimension(..), target :: input
    integer :: dtype
    integer :: parity     ! +1: the ghost cells are added as they are; -1: with their sign bits flipped first
    integer :: centering  ! 0: about the face between ghost and interior cells; 1: about the first / last interior cell
    integer :: clear      ! 1: the ghost cells that were read hold zero bytes afterwards; 0: they are only read
    integer :: halo_extents(3)
    logical :: halo_periods(3)
    integer :: dim  ! 1/2/3 = x/y/z
    integer, optional :: padding(3)
    integer(cudecomp_stream_kind), optional :: stream
    integer(c_int) :: res
    integer(c_int32_t) :: h(3), p(3)
    logical(c_bool) :: per(3)
    integer(c_intptr_t) :: s
    call halo_defaults(h, per, p, s, halo_extents, halo_periods, padding, stream)
    res = cudecompAmdFoldHalosX_C(handle, grid_desc, c_loc(input), int(dtype, c_int), int(parity, c_int32_t), &
                                      int(centering, c_int32_t), int(clear, c_int32_t), h, per, int(dim - 1, c_int32_t), p, s)
  end function cudecompAmdFoldHalosX

  function cudecompAmdFoldHalosY(handle, grid_desc, input, dtype, parity, centering, clear, halo_extents, halo_periods, dim, &
                                    padding, stream) result(res)
    type(cudecompHandle) :: handle
    type(cudecompGridDesc) :: grid_desc
    type(*), dimension(..), target :: input
    integer :: dtype
    integer :: parity     ! +1: the ghost cells are added as they are; -1: with their sign bits flipped first
    integer :: centering  ! 0: about the face between ghost and interior cells; 1: about the first / last interior cell
    integer :: clear      ! 1: the ghost cells that were read hold zero bytes afterwards; 0: they are only read
    integer :: halo_extents(3)
    logical :: halo_periods(3)
    integer :: dim  ! 1/2/3 = x/y/z
    integer, optional :: padding(3)
    integer(cudecomp_stream_kind), optional :: stream
    integer(c_int) :: res
    integer(c_int32_t) :: h(3), p(3)
    logical(c_bool) :: per(3)
    integer(c_intptr_t) :: s
    call halo_defaults(h, per, p, s, halo_extents, halo_periods, padding, stream)
    res = cudecompAmdFoldHalosY_C(handle, grid_desc, c_loc(input), int(dtype, c_int), int(parity, c_int32_t), &
                                      int(centering, c_int32_t), int(clear, c_int32_t), h, per, int(dim - 1, c_int32_t), p, s)
  end function cudecompAmdFoldHalosY

  function cudecompAmdFoldHalosZ(handle, grid_desc, input, dtype, parity, centering, clear, halo_extents, halo_periods, dim, &
                                    padding, stream) result(res)
    type(cudecompHandle) :: handle
    type(cudecompGridDesc) :: grid_desc
    type(*), dimension(..), target :: input
    integer :: dtype
    integer :: parity     ! +1: the ghost cells are added as they are; -1: with their sign bits flipped first
    integer :: centering  ! 0: about the face between ghost and interior cells; 1: about the first / last interior cell
    integer :: clear      ! 1: the ghost cells that were read hold zero bytes afterwards; 0: they are only read
    integer :: halo_extents(3)
    logical :: halo_periods(3)
    integer :: dim  ! 1/2/3 = x/y/z
    integer, optional :: padding(3)
    integer(cudecomp_stream_kind), optional :: stream
    integer(c_int) :: res
    integer(c_int32_t) :: h(3), p(3)
    logical(c_bool) :: per(3)
    integer(c_intptr_t) :: s
    call halo_defaults(h, per, p, s, halo_extents, halo_periods, padding, stream)
    res = cudecompAmdFoldHalosZ_C(handle, grid_desc, c_loc(input), int(dtype, c_int), int(parity, c_int32_t), &
                                      int(centering, c_int32_t), int(clear, c_int32_t), h, per, int(dim - 1, c_int32_t), p, s)
  end function cudecompAmdFoldHalosZ

  ! ---- multi-field halo updates (include/cudecomp_halo_fields.h): n_fields pencils, one exchange --------------------------
  ! inputs: the device addresses of the n_fields pencils (c_loc of each field); the other arguments as for cudecompUpdateHalosX
  function cudecompAmdUpdateFieldHalosX(handle, grid_desc, inputs, n_fields, work, dtype, halo_extents, halo_periods, dim, padding, &
                                        stream) result(res)
    type(cudecompHandle) :: handle
    type(cudecompGridDesc) :: grid_desc
    integer :: n_fields
    type(c_ptr), intent(in) :: inputs(n_fields)
    type(*), dimension(..), target :: work
    integer :: dtype
    integer :: halo_extents(3)
    logical :: halo_periods(3)
    integer :: dim  ! 1/2/3 = x/y/z
    integer, optional :: padding(3)
    integer(cudecomp_stream_kind), optional :: stream
    integer(c_int) :: res
    integer(c_int32_t) :: h(3), p(3)
    logical(c_bool) :: per(3)
    integer(c_intptr_t) :: s
    call halo_defaults(h, per, p, s, halo_extents, halo_periods, padding, stream)
    res = cudecompAmdUpdateFieldHalosX_C(handle, grid_desc, inputs, int(n_fields, c_int32_t), c_loc(work), int(dtype, c_int), h, per, &
                                         int(dim - 1, c_int32_t), p, s)
  end function cudecompAmdUpdateFieldHalosX

  ! inputs: the device addresses of the n_fields pencils (c_loc of each field); the other arguments as for cudecompUpdateHalosY
  function cudecompAmdUpdateFieldHalosY(handle, grid_desc, inputs, n_fields, work, dtype, halo_extents, halo_periods, dim, padding, &
                                        stream) result(res)
    type(cudecompHandle) :: handle
    type(cudecompGridDesc) :: grid_desc
    integer :: n_fields
    type(c_ptr), intent(in) :: inputs(n_fields)
    type(*), dimension(..), target :: work
    integer :: dtype
    integer :: halo_extents(3)
    logical :: halo_periods(3)
    integer :: dim  ! 1/2/3 = x/y/z
    integer, optional :: padding(3)
    integer(cudecomp_stream_kind), optional :: stream
    integer(c_int) :: res
    integer(c_int32_t) :: h(3), p(3)
    logical(c_bool) :: per(3)
    integer(c_intptr_t) :: s
    call halo_defaults(h, per, p, s, halo_extents, halo_periods, padding, stream)
    res = cudecompAmdUpdateFieldHalosY_C(handle, grid_desc, inputs, int(n_fields, c_int32_t), c_loc(work), int(dtype, c_int), h, per, &
                                         int(dim - 1, c_int32_t), p, s)
  end function cudecompAmdUpdateFieldHalosY

  ! inputs: the device addresses of the n_fields pencils (c_loc of each field); the other arguments as for cudecompUpdateHalosZ
  function cudecompAmdUpdateFieldHalosZ(handle, grid_desc, inputs, n_fields, work, dtype, halo_extents, halo_periods, dim, padding, &
                                        stream) result(res)
    type(cudecompHandle) :: handle
    type(cudecompGridDesc) :: grid_desc
    integer :: n_fields
    type(c_ptr), intent(in) :: inputs(n_fields)
    type(*), dimension(..), target :: work
    integer :: dtype
    integer :: halo_extents(3)
    logical :: halo_periods(3)
    integer :: dim  ! 1/2/3 = x/y/z
    integer, optional :: padding(3)
    integer(cudecomp_stream_kind), optional :: stream
    integer(c_int) :: res
    integer(c_int32_t) :: h(3), p(3)
    logical(c_bool) :: per(3)
    integer(c_intptr_t) :: s
    call halo_defaults(h, per, p, s, halo_extents, halo_periods, padding, stream)
    res = cudecompAmdUpdateFieldHalosZ_C(handle, grid_desc, inputs, int(n_fields, c_int32_t), c_loc(work), int(dtype, c_int), h, per, &
                                         int(dim - 1, c_int32_t), p, s)
  end function cudecompAmdUpdateFieldHalosZ


  ! ---- multi-field halo accumulation (include/cudecomp_halo_accumulate_fields.h): n_fields pencils, one exchange ------------
  ! the arguments of cudecompAmdUpdateFieldHalosX with `clear` (0 / 1: zero bytes into the ghost cells that were read) after `dim`,
  ! before the optional ones
  function cudecompAmdAccumulateFieldHalosX(handle, grid_desc, inputs, n_fields, work, dtype, halo_extents, halo_periods, dim, clear, &
                                            padding, stream) result(res)
    type(cudecompHandle) :: handle
    type(cudecompGridDesc) :: grid_desc
    integer :: n_fields
    type(c_ptr), intent(in) :: inputs(n_fields)
    type(*), dimension(..), target :: work
    integer :: dtype
    integer :: halo_extents(3)
    logical :: halo_periods(3)
    integer :: dim  ! 1/2/3 = x/y/z
    integer :: clear  ! 0 / 1
    integer, optional :: padding(3)
    integer(cudecomp_stream_kind), optional :: stream
    integer(c_int) :: res
    integer(c_int32_t) :: h(3), p(3)
    logical(c_bool) :: per(3)
    integer(c_intptr_t) :: s
    call halo_defaults(h, per, p, s, halo_extents, halo_periods, padding, stream)
    res = cudecompAmdAccumulateFieldHalosX_C(handle, grid_desc, inputs, int(n_fields, c_int32_t), c_loc(work), int(dtype, c_int), h, &
                                             per, int(dim - 1, c_int32_t), p, int(clear, c_int32_t), s)
  end function cudecompAmdAccumulateFieldHalosX

  function cudecompAmdAccumulateFieldHalosY(handle, grid_desc, inputs, n_fields, work, dtype, halo_extents, halo_periods, dim, clear, &
                                            padding, stream) result(res)
    type(cudecompHandle) :: handle
    type(cudecompGridDesc) :: grid_desc
    integer :: n_fields
    type(c_ptr), intent(in) :: inputs(n_fields)
    type(*), dimension(..), target :: work
    integer :: dtype
    integer :: halo_extents(3)
    logical :: halo_periods(3)
    integer :: dim  ! 1/2/3 = x/y/z
    integer :: clear  ! 0 / 1
    integer, optional :: padding(3)
    integer(cudecomp_stream_kind), optional :: stream
    integer(c_int) :: res
    integer(c_int32_t) :: h(3), p(3)
    logical(c_bool) :: per(3)
    integer(c_intptr_t) :: s
    call halo_defaults(h, per, p, s, halo_extents, halo_periods, padding, stream)
    res = cudecompAmdAccumulateFieldHalosY_C(handle, grid_desc, inputs, int(n_fields, c_int32_t), c_loc(work), int(dtype, c_int), h, &
                                             per, int(dim - 1, c_int32_t), p, int(clear, c_int32_t), s)
  end function cudecompAmdAccumulateFieldHalosY

  function cudecompAmdAccumulateFieldHalosZ(handle, grid_desc, inputs, n_fields, work, dtype, halo_extents, halo_periods, dim, clear, &
                                            padding, stream) result(res)
    type(cudecompHandle) :: handle
    type(cudecompGridDesc) :: grid_desc
    integer :: n_fields
    type(c_ptr), intent(in) :: inputs(n_fields)
    type(*), dimension(..), target :: work
    integer :: dtype
    integer :: halo_extents(3)
    logical :: halo_periods(3)
    integer :: dim  ! 1/2/3 = x/y/z
    integer :: clear  ! 0 / 1
    integer, optional :: padding(3)
    integer(cudecomp_stream_kind), optional :: stream
    integer(c_int) :: res
    integer(c_int32_t) :: h(3), p(3)
    logical(c_bool) :: per(3)
    integer(c_intptr_t) :: s
    call halo_defaults(h, per, p, s, halo_extents, halo_periods, padding, stream)
    res = cudecompAmdAccumulateFieldHalosZ_C(handle, grid_desc, inputs, int(n_fields, c_int32_t), c_loc(work), int(dtype, c_int), h, &
                                             per, int(dim - 1, c_int32_t), p, int(clear, c_int32_t), s)
  end function cudecompAmdAccumulateFieldHalosZ


  ! ---- multi-field wall halos (include/cudecomp_halo_wall_fields.h): n_fields pencils, a parity per field, one launch ---------
  ! the arguments of cudecompAmdReflectHalosX / cudecompAmdFoldHalosX with the list of fields and its length in the place of `input`
  ! and the list of parities (+1 / -1 per field) in the place of `parity`
  function cudecompAmdReflectFieldHalosX(handle, grid_desc, inputs, n_fields, dtype, parities, centering, halo_extents, halo_periods, dim, &
                                         padding, stream) result(res)
    type(cudecompHandle) :: handle
    type(cudecompGridDesc) :: grid_desc
    integer :: n_fields
    type(c_ptr), intent(in) :: inputs(n_fields)
    integer :: dtype
    integer, intent(in) :: parities(n_fields)  ! per field, +1: mirrored as it is; -1: with the sign bits flipped
    integer :: centering  ! 0: about the face between ghost and interior cells; 1: about the first / last interior cell
    integer :: halo_extents(3)
    logical :: halo_periods(3)
    integer :: dim  ! 1/2/3 = x/y/z
    integer, optional :: padding(3)
    integer(cudecomp_stream_kind), optional :: stream
    integer(c_int) :: res
    integer(c_int32_t) :: h(3), p(3), par(max(n_fields, 1))
    logical(c_bool) :: per(3)
    integer(c_intptr_t) :: s
    call halo_defaults(h, per, p, s, halo_extents, halo_periods, padding, stream)
    par = 0
    if (n_fields >= 1) par(1:n_fields) = int(parities, c_int32_t)
    res = cudecompAmdReflectFieldHalosX_C(handle, grid_desc, inputs, int(n_fields, c_int32_t), int(dtype, c_int), par, &
                                           int(centering, c_int32_t), h, per, int(dim - 1, c_int32_t), p, s)
  end function cudecompAmdReflectFieldHalosX

  function cudecompAmdReflectFieldHalosY(handle, grid_desc, inputs, n_fields, dtype, parities, centering, halo_extents, halo_periods, dim, &
                                         padding, stream) result(res)
    type(cudecompHandle) :: handle
    type(cudecompGridDesc) :: grid_desc
    integer :: n_fields
    type(c_ptr), intent(in) :: inputs(n_fields)
    integer :: dtype
    integer, intent(in) :: parities(n_fields)  ! per field, +1: mirrored as it is; -1: with the sign bits flipped
    integer :: centering  ! 0: about the face between ghost and interior cells; 1: about the first / last interior cell
    integer :: halo_extents(3)
    logical :: halo_periods(3)
    integer :: dim  ! 1/2/3 = x/y/z
    integer, optional :: padding(3)
    integer(cudecomp_stream_kind), optional :: stream
    integer(c_int) :: res
    integer(c_int32_t) :: h(3), p(3), par(max(n_fields, 1))
    logical(c_bool) :: per(3)
    integer(c_intptr_t) :: s
    call halo_defaults(h, per, p, s, halo_extents, halo_periods, padding, stream)
    par = 0
    if (n_fields >= 1) par(1:n_fields) = int(parities, c_int32_t)
    res = cudecompAmdReflectFieldHalosY_C(handle, grid_desc, inputs, int(n_fields, c_int32_t), int(dtype, c_int), par, &
                                           int(centering, c_int32_t), h, per, int(dim - 1, c_int32_t), p, s)
  end function cudecompAmdReflectFieldHalosY

  function cudecompAmdReflectFieldHalosZ(handle, grid_desc, inputs, n_fields, dtype, parities, centering, halo_extents, halo_periods, dim, &
                                         padding, stream) result(res)
    type(cudecompHandle) :: handle
    type(cudecompGridDesc) :: grid_desc
    integer :: n_fields
    type(c_ptr), intent(in) :: inputs(n_fields)
    integer :: dtype
    integer, intent(in) :: parities(n_fields)  ! per field, +1: mirrored as it is; -1: with the sign bits flipped
    integer :: centering  ! 0: about the face between ghost and interior cells; 1: about the first / last interior cell
    integer :: halo_extents(3)
    logical :: halo_periods(3)
    integer :: dim  ! 1/2/3 = x/y/z
    integer, optional :: padding(3)
    integer(cudecomp_stream_kind), optional :: stream
    integer(c_int) :: res
    integer(c_int32_t) :: h(3), p(3), par(max(n_fields, 1))
    logical(c_bool) :: per(3)
    integer(c_intptr_t) :: s
    call halo_defaults(h, per, p, s, halo_extents, halo_periods, padding, stream)
    par = 0
    if (n_fields >= 1) par(1:n_fields) = int(parities, c_int32_t)
    res = cudecompAmdReflectFieldHalosZ_C(handle, grid_desc, inputs, int(n_fields, c_int32_t), int(dtype, c_int), par, &
                                           int(centering, c_int32_t), h, per, int(dim - 1, c_int32_t), p, s)
  end function cudecompAmdReflectFieldHalosZ

  function cudecompAmdFoldFieldHalosX(handle, grid_desc, inputs, n_fields, dtype, parities, centering, clear, halo_extents, halo_periods, dim, &
                                         padding, stream) result(res)
    type(cudecompHandle) :: handle
    type(cudecompGridDesc) :: grid_desc
    integer :: n_fields
    type(c_ptr), intent(in) :: inputs(n_fields)
    integer :: dtype
    integer, intent(in) :: parities(n_fields)  ! per field, +1: mirrored as it is; -1: with the sign bits flipped
    integer :: centering  ! 0: about the face between ghost and interior cells; 1: about the first / last interior cell
    integer :: clear      ! 1: the ghost cells that were read hold zero bytes afterwards; 0: they are only read
    integer :: halo_extents(3)
    logical :: halo_periods(3)
    integer :: dim  ! 1/2/3 = x/y/z
    integer, optional :: padding(3)
    integer(cudecomp_stream_kind), optional :: stream
    integer(c_int) :: res
    integer(c_int32_t) :: h(3), p(3), par(max(n_fields, 1))
    logical(c_bool) :: per(3)
    integer(c_intptr_t) :: s
    call halo_defaults(h, per, p, s, halo_extents, halo_periods, padding, stream)
    par = 0
    if (n_fields >= 1) par(1:n_fields) = int(parities, c_int32_t)
    res = cudecompAmdFoldFieldHalosX_C(handle, grid_desc, inputs, int(n_fields, c_int32_t), int(dtype, c_int), par, &
                                           int(centering, c_int32_t), int(clear, c_int32_t), h, per, int(dim - 1, c_int32_t), p, s)
  end function cudecompAmdFoldFieldHalosX

  function cudecompAmdFoldFieldHalosY(handle, grid_desc, inputs, n_fields, dtype, parities, centering, clear, halo_extents, halo_periods, dim, &
                                         padding, stream) result(res)
    type(cudecompHandle) :: handle
    type(cudecompGridDesc) :: grid_desc
    integer :: n_fields
    type(c_ptr), intent(in) :: inputs(n_fields)
    integer :: dtype
    integer, intent(in) :: parities(n_fields)  ! per field, +1: mirrored as it is; -1: with the sign bits flipped
    integer :: centering  ! 0: about the face between ghost and interior cells; 1: about the first / last interior cell
    integer :: clear      ! 1: the ghost cells that were read hold zero bytes afterwards; 0: they are only read
    integer :: halo_extents(3)
    logical :: halo_periods(3)
    integer :: dim  ! 1/2/3 = x/y/z
    integer, optional :: padding(3)
    integer(cudecomp_stream_kind), optional :: stream
    integer(c_int) :: res
    integer(c_int32_t) :: h(3), p(3), par(max(n_fields, 1))
    logical(c_bool) :: per(3)
    integer(c_intptr_t) :: s
    call halo_defaults(h, per, p, s, halo_extents, halo_periods, padding, stream)
    par = 0
    if (n_fields >= 1) par(1:n_fields) = int(parities, c_int32_t)
    res = cudecompAmdFoldFieldHalosY_C(handle, grid_desc, inputs, int(n_fields, c_int32_t), int(dtype, c_int), par, &
                                           int(centering, c_int32_t), int(clear, c_int32_t), h, per, int(dim - 1, c_int32_t), p, s)
  end function cudecompAmdFoldFieldHalosY

  function cudecompAmdFoldFieldHalosZ(handle, grid_desc, inputs, n_fields, dtype, parities, centering, clear, halo_extents, halo_periods, dim, &
                                         padding, stream) result(res)
    type(cudecompHandle) :: handle
    type(cudecompGridDesc) :: grid_desc
    integer :: n_fields
    type(c_ptr), intent(in) :: inputs(n_fields)
    integer :: dtype
    integer, intent(in) :: parities(n_fields)  ! per field, +1: mirrored as it is; -1: with the sign bits flipped
    integer :: centering  ! 0: about the face between ghost and interior cells; 1: about the first / last interior cell
    integer :: clear      ! 1: the ghost cells that were read hold zero bytes afterwards; 0: they are only read
    integer :: halo_extents(3)
    logical :: halo_periods(3)
    integer :: dim  ! 1/2/3 = x/y/z
    integer, optional :: padding(3)
    integer(cudecomp_stream_kind), optional :: stream
    integer(c_int) :: res
    integer(c_int32_t) :: h(3), p(3), par(max(n_fields, 1))
    logical(c_bool) :: per(3)
    integer(c_intptr_t) :: s
    call halo_defaults(h, per, p, s, halo_extents, halo_periods, padding, stream)
    par = 0
    if (n_fields >= 1) par(1:n_fields) = int(parities, c_int32_t)
    res = cudecompAmdFoldFieldHalosZ_C(handle, grid_desc, inputs, int(n_fields, c_int32_t), int(dtype, c_int), par, &
                                           int(centering, c_int32_t), int(clear, c_int32_t), h, per, int(dim - 1, c_int32_t), p, s)
  end function cudecompAmdFoldFieldHalosZ


  ! ---- multi-field wall values (include/cudecomp_halo_wall_value_fields.h): n_fields pencils, a parity and addends per field -----
  ! the arguments of cudecompAmdSetWallHalosX with the list of fields and its length in the place of `input`, the list of parities
  ! (+1 / -1 per field) in the place of `parity`, and values_low / values_high field-major: halo_extents(dim) doubles per field
  ! (complex types: twice as many), field 1 first, layer 1 next to the wall
  function cudecompAmdSetWallFieldHalosX(handle, grid_desc, inputs, n_fields, dtype, parities, centering, sides, values_low, values_high, &
                                         halo_extents, halo_periods, dim, padding, stream) result(res)
    type(cudecompHandle) :: handle
    type(cudecompGridDesc) :: grid_desc
    integer :: n_fields
    type(c_ptr), intent(in) :: inputs(n_fields)
    integer :: dtype
    integer, intent(in) :: parities(n_fields)  ! per field, +1: even mirror; -1: odd mirror (sign bits flipped)
    integer :: centering  ! 0: about the face between ghost and interior cells; 1: about the first / last interior cell
    integer :: sides      ! 1: the low halo; 2: the high halo; 3: both
    ! host arrays, read before the call returns; the one of a side that `sides` does not name may be left out
    real(c_double), optional, target :: values_low(*), values_high(*)
    integer :: halo_extents(3)
    logical :: halo_periods(3)
    integer :: dim  ! 1/2/3 = x/y/z
    integer, optional :: padding(3)
    integer(cudecomp_stream_kind), optional :: stream
    integer(c_int) :: res
    integer(c_int32_t) :: h(3), p(3), par(max(n_fields, 1))
    logical(c_bool) :: per(3)
    integer(c_intptr_t) :: s
    type(c_ptr) :: lo, hi
    call halo_defaults(h, per, p, s, halo_extents, halo_periods, padding, stream)
    par = 0
    if (n_fields >= 1) par(1:n_fields) = int(parities, c_int32_t)
    lo = c_null_ptr
    hi = c_null_ptr
    if (present(values_low)) lo = c_loc(values_low)
    if (present(values_high)) hi = c_loc(values_high)
    res = cudecompAmdSetWallFieldHalosX_C(handle, grid_desc, inputs, int(n_fields, c_int32_t), int(dtype, c_int), par, &
                                           int(centering, c_int32_t), int(sides, c_int32_t), lo, hi, h, per, int(dim - 1, c_int32_t), p, s)
  end function cudecompAmdSetWallFieldHalosX

  function cudecompAmdSetWallFieldHalosY(handle, grid_desc, inputs, n_fields, dtype, parities, centering, sides, values_low, values_high, &
                                         halo_extents, halo_periods, dim, padding, stream) result(res)
    type(cudecompHandle) :: handle
    type(cudecompGridDesc) :: grid_desc
    integer :: n_fields
    type(c_ptr), intent(in) :: inputs(n_fields)
    integer :: dtype
    integer, intent(in) :: parities(n_fields)  ! per field, +1: even mirror; -1: odd mirror (sign bits flipped)
    integer :: centering  ! 0: about the face between ghost and interior cells; 1: about the first / last interior cell
    integer :: sides      ! 1: the low halo; 2: the high halo; 3: both
    ! host arrays, read before the call returns; the one of a side that `sides` does not name may be left out
    real(c_double), optional, target :: values_low(*), values_high(*)
    integer :: halo_extents(3)
    logical :: halo_periods(3)
    integer :: dim  ! 1/2/3 = x/y/z
    integer, optional :: padding(3)
    integer(cudecomp_stream_kind), optional :: stream
    integer(c_int) :: res
    integer(c_int32_t) :: h(3), p(3), par(max(n_fields, 1))
    logical(c_bool) :: per(3)
    integer(c_intptr_t) :: s
    type(c_ptr) :: lo, hi
    call halo_defaults(h, per, p, s, halo_extents, halo_periods, padding, stream)
    par = 0
    if (n_fields >= 1) par(1:n_fields) = int(parities, c_int32_t)
    lo = c_null_ptr
    hi = c_null_ptr
    if (present(values_low)) lo = c_loc(values_low)
    if (present(values_high)) hi = c_loc(values_high)
    res = cudecompAmdSetWallFieldHalosY_C(handle, grid_desc, inputs, int(n_fields, c_int32_t), int(dtype, c_int), par, &
                                           int(centering, c_int32_t), int(sides, c_int32_t), lo, hi, h, per, int(dim - 1, c_int32_t), p, s)
  end function cudecompAmdSetWallFieldHalosY

  function cudecompAmdSetWallFieldHalosZ(handle, grid_desc, inputs, n_fields, dtype, parities, centering, sides, values_low, values_high, &
                                         halo_extents, halo_periods, dim, padding, stream) result(res)
    type(cudecompHandle) :: handle
    type(cudecompGridDesc) :: grid_desc
    integer :: n_fields
    type(c_ptr), intent(in) :: inputs(n_fields)
    integer :: dtype
    integer, intent(in) :: parities(n_fields)  ! per field, +1: even mirror; -1: odd mirror (sign bits flipped)
    integer :: centering  ! 0: about the face between ghost and interior cells; 1: about the first / last interior cell
    integer :: sides      ! 1: the low halo; 2: the high halo; 3: both
    ! host arrays, read before the call returns; the one of a side that `sides` does not name may be left out
    real(c_double), optional, target :: values_low(*), values_high(*)
    integer :: halo_extents(3)
    logical :: halo_periods(3)
    integer :: dim  ! 1/2/3 = x/y/z
    integer, optional :: padding(3)
    integer(cudecomp_stream_kind), optional :: stream
    integer(c_int) :: res
    integer(c_int32_t) :: h(3), p(3), par(max(n_fields, 1))
    logical(c_bool) :: per(3)
    integer(c_intptr_t) :: s
    type(c_ptr) :: lo, hi
    call halo_defaults(h, per, p, s, halo_extents, halo_periods, padding, stream)
    par = 0
    if (n_fields >= 1) par(1:n_fields) = int(parities, c_int32_t)
    lo = c_null_ptr
    hi = c_null_ptr
    if (present(values_low)) lo = c_loc(values_low)
    if (present(values_high)) hi = c_loc(values_high)
    res = cudecompAmdSetWallFieldHalosZ_C(handle, grid_desc, inputs, int(n_fields, c_int32_t), int(dtype, c_int), par, &
                                           int(centering, c_int32_t), int(sides, c_int32_t), lo, hi, h, per, int(dim - 1, c_int32_t), p, s)
  end function cudecompAmdSetWallFieldHalosZ


  ! ---- multi-field transposes (include/cudecomp_transpose_fields.h): n_fields pencils, one exchange ------------------------
  ! inputs / outputs: the device addresses of the n_fields input / output pencils (c_loc of each field), all in place or all out
  ! of place; the other arguments as for cudecompTransposeXToY
  function cudecompAmdTransposeFieldsXToY(handle, grid_desc, inputs, outputs, n_fields, work, dtype, input_halo_extents, &
                                          output_halo_extents, input_padding, output_padding, stream) result(res)
    type(cudecompHandle) :: handle
    type(cudecompGridDesc) :: grid_desc
    integer :: n_fields
    type(c_ptr), intent(in) :: inputs(n_fields), outputs(n_fields)
    type(*), dimension(..), target :: work
    integer :: dtype
    integer, optional :: input_halo_extents(3), output_halo_extents(3), input_padding(3), output_padding(3)
    integer(cudecomp_stream_kind), optional :: stream
    integer(c_int) :: res
    integer(c_int32_t) :: ih(3), oh(3), ip(3), op(3)
    integer(c_intptr_t) :: s
    call transpose_defaults(ih, oh, ip, op, s, input_halo_extents, output_halo_extents, input_padding, &
                            output_padding, stream)
    res = cudecompAmdTransposeFieldsXToY_C(handle, grid_desc, inputs, outputs, int(n_fields, c_int32_t), c_loc(work), &
                                           int(dtype, c_int), ih, oh, ip, op, s)
  end function cudecompAmdTransposeFieldsXToY

  ! inputs / outputs: the device addresses of the n_fields input / output pencils (c_loc of each field), all in place or all out
  ! of place; the other arguments as for cudecompTransposeYToZ
  function cudecompAmdTransposeFieldsYToZ(handle, grid_desc, inputs, outputs, n_fields, work, dtype, input_halo_extents, &
                                          output_halo_extents, input_padding, output_padding, stream) result(res)
    type(cudecompHandle) :: handle
    type(cudecompGridDesc) :: grid_desc
    integer :: n_fields
    type(c_ptr), intent(in) :: inputs(n_fields), outputs(n_fields)
    type(*), dimension(..), target :: work
    integer :: dtype
    integer, optional :: input_halo_extents(3), output_halo_extents(3), input_padding(3), output_padding(3)
    integer(cudecomp_stream_kind), optional :: stream
    integer(c_int) :: res
    integer(c_int32_t) :: ih(3), oh(3), ip(3), op(3)
    integer(c_intptr_t) :: s
    call transpose_defaults(ih, oh, ip, op, s, input_halo_extents, output_halo_extents, input_padding, &
                            output_padding, stream)
    res = cudecompAmdTransposeFieldsYToZ_C(handle, grid_desc, inputs, outputs, int(n_fields, c_int32_t), c_loc(work), &
                                           int(dtype, c_int), ih, oh, ip, op, s)
  end function cudecompAmdTransposeFieldsYToZ

  ! inputs / outputs: the device addresses of the n_fields input / output pencils (c_loc of each field), all in place or all out
  ! of place; the other arguments as for cudecompTransposeZToY
  function cudecompAmdTransposeFieldsZToY(handle, grid_desc, inputs, outputs, n_fields, work, dtype, input_halo_extents, &
                                          output_halo_extents, input_padding, output_padding, stream) result(res)
    type(cudecompHandle) :: handle
    type(cudecompGridDesc) :: grid_desc
    integer :: n_fields
    type(c_ptr), intent(in) :: inputs(n_fields), outputs(n_fields)
    type(*), dimension(..), target :: work
    integer :: dtype
    integer, optional :: input_halo_extents(3), output_halo_extents(3), input_padding(3), output_padding(3)
    integer(cudecomp_stream_kind), optional :: stream
    integer(c_int) :: res
    integer(c_int32_t) :: ih(3), oh(3), ip(3), op(3)
    integer(c_intptr_t) :: s
    call transpose_defaults(ih, oh, ip, op, s, input_halo_extents, output_halo_extents, input_padding, &
                            output_padding, stream)
    res = cudecompAmdTransposeFieldsZToY_C(handle, grid_desc, inputs, outputs, int(n_fields, c_int32_t), c_loc(work), &
                                           int(dtype, c_int), ih, oh, ip, op, s)
  end function cudecompAmdTransposeFieldsZToY

  ! inputs / outputs: the device addresses of the n_fields input / output pencils (c_loc of each field), all in place or all out
  ! of place; the other arguments as for cudecompTransposeYToX
  function cudecompAmdTransposeFieldsYToX(handle, grid_desc, inputs, outputs, n_fields, work, dtype, input_halo_extents, &
                                          output_halo_extents, input_padding, output_padding, stream) result(res)
    type(cudecompHandle) :: handle
    type(cudecompGridDesc) :: grid_desc
    integer :: n_fields
    type(c_ptr), intent(in) :: inputs(n_fields), outputs(n_fields)
    type(*), dimension(..), target :: work
    integer :: dtype
    integer, optional :: input_halo_extents(3), output_halo_extents(3), input_padding(3), output_padding(3)
    integer(cudecomp_stream_kind), optional :: stream
    integer(c_int) :: res
    integer(c_int32_t) :: ih(3), oh(3), ip(3), op(3)
    integer(c_intptr_t) :: s
    call transpose_defaults(ih, oh, ip, op, s, input_halo_extents, output_halo_extents, input_padding, &
                            output_padding, stream)
    res = cudecompAmdTransposeFieldsYToX_C(handle, grid_desc, inputs, outputs, int(n_fields, c_int32_t), c_loc(work), &
                                           int(dtype, c_int), ih, oh, ip, op, s)
  end function cudecompAmdTransposeFieldsYToX


  ! ---- interior profiles (cudecomp_interior_profile.h): `a` and `b` are arrays of n_fields device addresses, `results` and `work`
  ! device addresses, `op` one of CUDECOMP_AMD_REDUCE_SUM / _DOT / _MAX_ABS; field f, entry k owns the two doubles at
  ! results(2 * (f * ld + k)), f and k counted from 0 ----
  function cudecompAmdProfileInteriorX(handle, grid_desc, a, b, n_fields, op, dim, results, ld, work, dtype, halo_extents, padding, &
                                       stream) result(res)
    type(cudecompHandle) :: handle
    type(cudecompGridDesc) :: grid_desc
    type(c_ptr) :: a(*), b(*)
    integer :: n_fields, op
    integer :: dim  ! 1/2/3 = x/y/z
    type(c_ptr) :: results, work
    integer(c_int64_t) :: ld
    integer :: dtype
    integer :: halo_extents(3)
    integer, optional :: padding(3)
    integer(cudecomp_stream_kind), optional :: stream
    integer(c_int) :: res
    integer(c_int32_t) :: h(3), p(3)
    integer(c_intptr_t) :: s
    h = int(halo_extents, c_int32_t)
    p = 0
    s = 0
    if (present(padding)) p = int(padding, c_int32_t)
    if (present(stream)) s = stream
    res = cudecompAmdProfileInteriorX_C(handle, grid_desc, a, b, int(n_fields, c_int32_t), int(op, c_int32_t), &
                                        int(dim - 1, c_int32_t), results, ld, work, int(dtype, c_int), h, p, s)
  end function cudecompAmdProfileInteriorX

  function cudecompAmdProfileInteriorY(handle, grid_desc, a, b, n_fields, op, dim, results, ld, work, dtype, halo_extents, padding, &
                                       stream) result(res)
    type(cudecompHandle) :: handle
    type(cudecompGridDesc) :: grid_desc
    type(c_ptr) :: a(*), b(*)
    integer :: n_fields, op
    integer :: dim  ! 1/2/3 = x/y/z
    type(c_ptr) :: results, work
    integer(c_int64_t) :: ld
    integer :: dtype
    integer :: halo_extents(3)
    integer, optional :: padding(3)
    integer(cudecomp_stream_kind), optional :: stream
    integer(c_int) :: res
    integer(c_int32_t) :: h(3), p(3)
    integer(c_intptr_t) :: s
    h = int(halo_extents, c_int32_t)
    p = 0
    s = 0
    if (present(padding)) p = int(padding, c_int32_t)
    if (present(stream)) s = stream
    res = cudecompAmdProfileInteriorY_C(handle, grid_desc, a, b, int(n_fields, c_int32_t), int(op, c_int32_t), &
                                        int(dim - 1, c_int32_t), results, ld, work, int(dtype, c_int), h, p, s)
  end function cudecompAmdProfileInteriorY

  function cudecompAmdProfileInteriorZ(handle, grid_desc, a, b, n_fields, op, dim, results, ld, work, dtype, halo_extents, padding, &
                                       stream) result(res)
    type(cudecompHandle) :: handle
    type(cudecompGridDesc) :: grid_desc
    type(c_ptr) :: a(*), b(*)
    integer :: n_fields, op
    integer :: dim  ! 1/2/3 = x/y/z
    type(c_ptr) :: results, work
    integer(c_int64_t) :: ld
    integer :: dtype
    integer :: halo_extents(3)
    integer, optional :: padding(3)
    integer(cudecomp_stream_kind), optional :: stream
    integer(c_int) :: res
    integer(c_int32_t) :: h(3), p(3)
    integer(c_intptr_t) :: s
    h = int(halo_extents, c_int32_t)
    p = 0
    s = 0
    if (present(padding)) p = int(padding, c_int32_t)
    if (present(stream)) s = stream
    res = cudecompAmdProfileInteriorZ_C(handle, grid_desc, a, b, int(n_fields, c_int32_t), int(op, c_int32_t), &
                                        int(dim - 1, c_int32_t), results, ld, work, int(dtype, c_int), h, p, s)
  end function cudecompAmdProfileInteriorZ

  ! ---- interior plane updates (cudecomp_interior_planes.h): `fields` is an array of n_fields device addresses, `coef` a device
  ! address laid out as the profile's results, `op` one of CUDECOMP_AMD_PLANES_ADD / _MUL; the cell of interior index k along dim
  ! (counted from 0) of field f takes scale * the pair at coef(2 * (f * ld + k)); ld = 0: all fields share row 0 ----
  function cudecompAmdApplyPlanesInteriorX(handle, grid_desc, fields, n_fields, op, dim, coef, ld, scale, dtype, halo_extents, padding, &
                                           stream) result(res)
    type(cudecompHandle) :: handle
    type(cudecompGridDesc) :: grid_desc
    type(c_ptr) :: fields(*)
    integer :: n_fields, op
    integer :: dim  ! 1/2/3 = x/y/z
    type(c_ptr) :: coef
    integer(c_int64_t) :: ld
    real(c_double) :: scale
    integer :: dtype
    integer :: halo_extents(3)
    integer, optional :: padding(3)
    integer(cudecomp_stream_kind), optional :: stream
    integer(c_int) :: res
    integer(c_int32_t) :: h(3), p(3)
    integer(c_intptr_t) :: s
    h = int(halo_extents, c_int32_t)
    p = 0
    s = 0
    if (present(padding)) p = int(padding, c_int32_t)
    if (present(stream)) s = stream
    res = cudecompAmdApplyPlanesInteriorX_C(handle, grid_desc, fields, int(n_fields, c_int32_t), int(op, c_int32_t), &
                                            int(dim - 1, c_int32_t), coef, ld, scale, int(dtype, c_int), h, p, s)
  end function cudecompAmdApplyPlanesInteriorX

  function cudecompAmdApplyPlanesInteriorY(handle, grid_desc, fields, n_fields, op, dim, coef, ld, scale, dtype, halo_extents, padding, &
                                           stream) result(res)
    type(cudecompHandle) :: handle
    type(cudecompGridDesc) :: grid_desc
    type(c_ptr) :: fields(*)
    integer :: n_fields, op
    integer :: dim  ! 1/2/3 = x/y/z
    type(c_ptr) :: coef
    integer(c_int64_t) :: ld
    real(c_double) :: scale
    integer :: dtype
    integer :: halo_extents(3)
    integer, optional :: padding(3)
    integer(cudecomp_stream_kind), optional :: stream
    integer(c_int) :: res
    integer(c_int32_t) :: h(3), p(3)
    integer(c_intptr_t) :: s
    h = int(halo_extents, c_int32_t)
    p = 0
    s = 0
    if (present(padding)) p = int(padding, c_int32_t)
    if (present(stream)) s = stream
    res = cudecompAmdApplyPlanesInteriorY_C(handle, grid_desc, fields, int(n_fields, c_int32_t), int(op, c_int32_t), &
                                            int(dim - 1, c_int32_t), coef, ld, scale, int(dtype, c_int), h, p, s)
  end function cudecompAmdApplyPlanesInteriorY

  function cudecompAmdApplyPlanesInteriorZ(handle, grid_desc, fields, n_fields, op, dim, coef, ld, scale, dtype, halo_extents, padding, &
                                           stream) result(res)
    type(cudecompHandle) :: handle
    type(cudecompGridDesc) :: grid_desc
    type(c_ptr) :: fields(*)
    integer :: n_fields, op
    integer :: dim  ! 1/2/3 = x/y/z
    type(c_ptr) :: coef
    integer(c_int64_t) :: ld
    real(c_double) :: scale
    integer :: dtype
    integer :: halo_extents(3)
    integer, optional :: padding(3)
    integer(cudecomp_stream_kind), optional :: stream
    integer(c_int) :: res
    integer(c_int32_t) :: h(3), p(3)
    integer(c_intptr_t) :: s
    h = int(halo_extents, c_int32_t)
    p = 0
    s = 0
    if (present(padding)) p = int(padding, c_int32_t)
    if (present(stream)) s = stream
    res = cudecompAmdApplyPlanesInteriorZ_C(handle, grid_desc, fields, int(n_fields, c_int32_t), int(op, c_int32_t), &
                                            int(dim - 1, c_int32_t), coef, ld, scale, int(dtype, c_int), h, p, s)
  end function cudecompAmdApplyPlanesInteriorZ

  ! ---- interior combinations (cudecomp_interior_combine.h): `y` and `x` are arrays of n_fields device addresses, `op` one of
  ! CUDECOMP_AMD_COMBINE_AXPY / _XPBY / _AXPBY / _AX; a = (a_scale * a_num(2i + c)) / a_den(2i) with i = f * coef_stride, the four
  ! coefficient arrays device addresses laid out as the reduction's results (c_null_ptr: the pair (1, 0) / no division); b likewise ----
  function cudecompAmdCombineInteriorX(handle, grid_desc, y, x, n_fields, op, a_num, a_den, a_scale, b_num, b_den, b_scale, &
                                       coef_stride, dtype, halo_extents, padding, stream) result(res)
    type(cudecompHandle) :: handle
    type(cudecompGridDesc) :: grid_desc
    type(c_ptr) :: y(*), x(*)
    integer :: n_fields, op
    type(c_ptr) :: a_num, a_den
    real(c_double) :: a_scale
    type(c_ptr) :: b_num, b_den
    real(c_double) :: b_scale
    integer :: coef_stride  ! 0: all fields share pair 0; 1: field f takes pair f
    integer :: dtype
    integer :: halo_extents(3)
    integer, optional :: padding(3)
    integer(cudecomp_stream_kind), optional :: stream
    integer(c_int) :: res
    integer(c_int32_t) :: h(3), p(3)
    integer(c_intptr_t) :: s
    h = int(halo_extents, c_int32_t)
    p = 0
    s = 0
    if (present(padding)) p = int(padding, c_int32_t)
    if (present(stream)) s = stream
    res = cudecompAmdCombineInteriorX_C(handle, grid_desc, y, x, int(n_fields, c_int32_t), int(op, c_int32_t), a_num, a_den, &
                                        a_scale, b_num, b_den, b_scale, int(coef_stride, c_int32_t), int(dtype, c_int), h, p, s)
  end function cudecompAmdCombineInteriorX

  function cudecompAmdCombineInteriorY(handle, grid_desc, y, x, n_fields, op, a_num, a_den, a_scale, b_num, b_den, b_scale, &
                                       coef_stride, dtype, halo_extents, padding, stream) result(res)
    type(cudecompHandle) :: handle
    type(cudecompGridDesc) :: grid_desc
    type(c_ptr) :: y(*), x(*)
    integer :: n_fields, op
    type(c_ptr) :: a_num, a_den
    real(c_double) :: a_scale
    type(c_ptr) :: b_num, b_den
    real(c_double) :: b_scale
    integer :: coef_stride  ! 0: all fields share pair 0; 1: field f takes pair f
    integer :: dtype
    integer :: halo_extents(3)
    integer, optional :: padding(3)
    integer(cudecomp_stream_kind), optional :: stream
    integer(c_int) :: res
    integer(c_int32_t) :: h(3), p(3)
    integer(c_intptr_t) :: s
    h = int(halo_extents, c_int32_t)
    p = 0
    s = 0
    if (present(padding)) p = int(padding, c_int32_t)
    if (present(stream)) s = stream
    res = cudecompAmdCombineInteriorY_C(handle, grid_desc, y, x, int(n_fields, c_int32_t), int(op, c_int32_t), a_num, a_den, &
                                        a_scale, b_num, b_den, b_scale, int(coef_stride, c_int32_t), int(dtype, c_int), h, p, s)
  end function cudecompAmdCombineInteriorY

  function cudecompAmdCombineInteriorZ(handle, grid_desc, y, x, n_fields, op, a_num, a_den, a_scale, b_num, b_den, b_scale, &
                                       coef_stride, dtype, halo_extents, padding, stream) result(res)
    type(cudecompHandle) :: handle
    type(cudecompGridDesc) :: grid_desc
    type(c_ptr) :: y(*), x(*)
    integer :: n_fields, op
    type(c_ptr) :: a_num, a_den
    real(c_double) :: a_scale
    type(c_ptr) :: b_num, b_den
    real(c_double) :: b_scale
    integer :: coef_stride  ! 0: all fields share pair 0; 1: field f takes pair f
    integer :: dtype
    integer :: halo_extents(3)
    integer, optional :: padding(3)
    integer(cudecomp_stream_kind), optional :: stream
    integer(c_int) :: res
    integer(c_int32_t) :: h(3), p(3)
    integer(c_intptr_t) :: s
    h = int(halo_extents, c_int32_t)
    p = 0
    s = 0
    if (present(padding)) p = int(padding, c_int32_t)
    if (present(stream)) s = stream
    res = cudecompAmdCombineInteriorZ_C(handle, grid_desc, y, x, int(n_fields, c_int32_t), int(op, c_int32_t), a_num, a_den, &
                                        a_scale, b_num, b_den, b_scale, int(coef_stride, c_int32_t), int(dtype, c_int), h, p, s)
  end function cudecompAmdCombineInteriorZ

  subroutine halo_defaults(h, per, p, s, halo_extents, halo_periods, padding, stream)
    integer(c_int32_t), intent(out) :: h(3), p(3)
    logical(c_bool), intent(out) :: per(3)
    integer(c_intptr_t), intent(out) :: s
    integer, intent(in) :: halo_extents(3)
    logical, intent(in) :: halo_periods(3)
    integer, optional, intent(in) :: padding(3)
    integer(cudecomp_stream_kind), optional, intent(in) :: stream
    h = int(halo_extents, c_int32_t)
    per = halo_periods
    p = 0
    s = 0
    if (present(padding)) p = int(padding, c_int32_t)
    if (present(stream)) s = stream
  end subroutine halo_defaults

end module cudecomp
