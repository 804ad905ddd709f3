! transpose_fields_test.f90 -- Fortran twin of tests/native/transpose_fields_test.cpp: multi-field transposes
! (cudecomp_transpose_fields.h) through the wrappers cudecompAmdTransposeFields{XToY,YToZ,ZToY,YToX} of module `cudecomp`, fp64.
! Per case: --fields N pencils (slices of one buffer from cudecompMalloc, their addresses passed as arrays of type(c_ptr)) are
! uploaded twice; one copy runs the cycle X -> Y -> Z -> Y -> X through the fields wrappers, the other through N single
! cudecompTranspose* calls per hop; after every hop every buffer of both copies -- inputs, outputs, halo and padding cells, a tail
! -- is downloaded and compared bit for bit.  The oracle is the single call.
!
!   --gx --gy --gz, --pr --pc, --backend, --ac      as for transpose_test
!   --hex --hey --hez / --pdx --pdy --pdz           halo extents / padding of every pencil (by global axis)
!   --fields N  the number of pencils (1 .. 32)     --inplace   inputs(f) and outputs(f) are the same pencil
!   --nullhalo  halos and padding absent (needs zero halos and padding)       --stream   `stream` present: a stream this program created
!   --self-check-swap-fields    hand the wrapper its outputs in reversed order while comparing in order: the case must FAIL
! At the end rank 0 prints one line "WRAPPER <name>" per wrapper that was called in a case that passed.
program transpose_fields_test
  use, intrinsic :: iso_c_binding
  use, intrinsic :: iso_fortran_env, only: int32, int64, real32, real64, error_unit
  use cudecomp
  use test_support
  implicit none

  interface
    function hipStreamDestroy(stream) bind(C, name="hipStreamDestroy") result(res)
      import
      integer(c_intptr_t), value :: stream
      integer(c_int) :: res
    end function hipStreamDestroy
  end interface

  integer, parameter :: TAIL = 64
  character(len=32), parameter :: WRAPPER_NAMES(4) = [character(len=32) :: &
    "cudecompAmdTransposeFieldsXToY", "cudecompAmdTransposeFieldsYToZ", "cudecompAmdTransposeFieldsZToY", &
    "cudecompAmdTransposeFieldsYToX"]

  type(cudecompHandle) :: handle
  integer :: rank, nranks, ndev, dtype_sel, dtype, wpe, i, ncases, res, nfailed, u, stat, argn, k
  integer(int64) :: es
  character(len=1024) :: line, arg, testfile, progname
  character(len=1024), allocatable :: cases(:)
  logical :: from_file
  integer :: c0, c1, rate
  logical :: called(4), called_in_case(4)
  integer(cudecomp_stream_kind) :: my_stream
  logical :: have_stream

  ! the case the wrappers are called for (call_wrapper and its callers are internal procedures of the program)
  type(cudecompGridDesc) :: cs_grid_desc
  real(real32), pointer, contiguous :: cs_data(:), cs_work(:)
  type(c_ptr) :: cs_in(32), cs_out(32)
  integer :: cs_halo(3), cs_pad(3), cs_nf

  rank = env_int("RANK", env_int("PMI_RANK", env_int("OMPI_COMM_WORLD_RANK", 0)))
  nranks = env_int("WORLD_SIZE", env_int("PMI_SIZE", env_int("OMPI_COMM_WORLD_SIZE", 1)))
  dtype_sel = 2
  dtype = CUDECOMP_DOUBLE
  es = 8
  wpe = 1
  call get_command_argument(0, progname)
  called = .false.
  have_stream = .false.

  from_file = .false.
  testfile = ""
  line = ""
  argn = command_argument_count()
  do i = 1, argn
    call get_command_argument(i, arg)
    if ((trim(arg) == "-f" .or. trim(arg) == "--testfile") .and. i < argn) then
      call get_command_argument(i + 1, testfile)
      from_file = .true.
    end if
    line = trim(line)//" "//trim(arg)
  end do
  if (from_file) then
    ncases = 0
    open (newunit=u, file=trim(testfile), status="old", action="read", iostat=stat)
    if (stat /= 0) error stop "cannot open the test file"
    do
      read (u, '(a)', iostat=stat) arg
      if (stat /= 0) exit
      if (len_trim(arg) > 0) ncases = ncases + 1
    end do
    rewind (u)
    allocate (cases(ncases))
    i = 0
    do
      read (u, '(a)', iostat=stat) arg
      if (stat /= 0) exit
      if (len_trim(arg) > 0) then
        i = i + 1
        cases(i) = arg
      end if
    end do
    close (u)
  else
    ncases = 1
    allocate (cases(1))
    cases(1) = line
  end if

  call hipcheck(hipGetDeviceCount(ndev), "hipGetDeviceCount")
  call hipcheck(hipSetDevice(mod(env_int("LOCAL_RANK", rank), ndev)), "hipSetDevice")
  call check(cudecompInit(handle, WORLD_COMM), "cudecompInit")

  nfailed = 0
  call system_clock(c0, rate)
  if (from_file .and. rank == 0) write (*, '(a,i0,a)') "Running ", ncases, " tests..."
  do i = 1, ncases
    if (from_file .and. rank == 0) write (*, '(a,a,a,a)') "command: ", trim(progname), " ", trim(cases(i))
    nfail = 0
    called_in_case = .false.
    call run_case(trim(cases(i)))
    res = reduce_verdict(min(nfail, 1), i)
    if (nfail == 0) called = called .or. called_in_case
    if (rank == 0) then
      if (from_file) then
        if (res /= 0) then
          write (*, '(a)') " FAILED"
        else
          write (*, '(a)') " PASSED"
        end if
      end if
      if (res /= 0) nfailed = nfailed + 1
      if (from_file .and. mod(i, 10) == 0) then
        call system_clock(c1)
        write (*, '(a,i0,a,i0,a,f0.3,a)') "Completed ", i, "/", ncases, " tests, running time ", real(c1 - c0)/real(rate), " s"
      end if
    else if (nfail /= 0) then
      nfailed = nfailed + 1
    end if
    if (res /= 0 .or. nfail /= 0) exit  ! after a failed case the ranks are no longer in step: what follows is no evidence
  end do
  if (have_stream) call hipcheck(hipStreamDestroy(my_stream), "hipStreamDestroy")
  call check(cudecompFinalize(handle), "cudecompFinalize")
  if (rank == 0) then
    do k = 1, 4
      if (called(k)) write (*, '(a,a)') "WRAPPER ", trim(WRAPPER_NAMES(k))
    end do
    call system_clock(c1)
    if (from_file) write (*, '(a,f0.3,a)') "Completed all tests, running time ", real(c1 - c0)/real(rate), " s,"
    if (nfailed == 0) then
      if (from_file) then
        write (*, '(a)') "Passed all tests."
      else
        write (*, '(a)') "PASSED"
      end if
    else
      write (*, '(a,i0,a,i0,a)') "Failed ", nfailed, "/", ncases, " tests."
    end if
  end if
  if (nfailed /= 0) error stop 1

contains
  ! one of the four wrappers; absent optional arguments stay absent all the way down
  function call_wrapper(op, halo_o, pad_o, stream_o) result(r)
    integer, intent(in) :: op
    integer, optional :: halo_o(3), pad_o(3)
    integer(cudecomp_stream_kind), optional :: stream_o
    integer(c_int) :: r
    r = -1
    called_in_case(op) = .true.
    select case (op)
    case (1); r = cudecompAmdTransposeFieldsXToY(handle, cs_grid_desc, cs_in(1:cs_nf), cs_out(1:cs_nf), cs_nf, cs_work, dtype, &
                                                 halo_o, halo_o, pad_o, pad_o, stream_o)
    case (2); r = cudecompAmdTransposeFieldsYToZ(handle, cs_grid_desc, cs_in(1:cs_nf), cs_out(1:cs_nf), cs_nf, cs_work, dtype, &
                                                 halo_o, halo_o, pad_o, pad_o, stream_o)
    case (3); r = cudecompAmdTransposeFieldsZToY(handle, cs_grid_desc, cs_in(1:cs_nf), cs_out(1:cs_nf), cs_nf, cs_work, dtype, &
                                                 halo_o, halo_o, pad_o, pad_o, stream_o)
    case (4); r = cudecompAmdTransposeFieldsYToX(handle, cs_grid_desc, cs_in(1:cs_nf), cs_out(1:cs_nf), cs_nf, cs_work, dtype, &
                                                 halo_o, halo_o, pad_o, pad_o, stream_o)
    end select
  end function call_wrapper

  ! halos / padding and `stream` present or absent
  function with_forms(op, use_hp, use_stream) result(r)
    integer, intent(in) :: op
    logical, intent(in) :: use_hp, use_stream
    integer(c_int) :: r
    if (use_hp .and. use_stream) then
      r = call_wrapper(op, halo_o=cs_halo, pad_o=cs_pad, stream_o=my_stream)
    else if (use_hp) then
      r = call_wrapper(op, halo_o=cs_halo, pad_o=cs_pad)
    else if (use_stream) then
      r = call_wrapper(op, stream_o=my_stream)
    else
      r = call_wrapper(op)
    end if
  end function with_forms

  ! the single transpose of one field (slices of the data buffer), with the same halos and padding
  function single_call(op, a, b, work1) result(r)
    integer, intent(in) :: op
    real(real32), target :: a(:), b(:), work1(:)
    integer(c_int) :: r
    r = -1
    select case (op)
    case (1); r = cudecompTransposeXToY(handle, cs_grid_desc, a, b, work1, dtype, cs_halo, cs_halo, cs_pad, cs_pad)
    case (2); r = cudecompTransposeYToZ(handle, cs_grid_desc, a, b, work1, dtype, cs_halo, cs_halo, cs_pad, cs_pad)
    case (3); r = cudecompTransposeZToY(handle, cs_grid_desc, a, b, work1, dtype, cs_halo, cs_halo, cs_pad, cs_pad)
    case (4); r = cudecompTransposeYToX(handle, cs_grid_desc, a, b, work1, dtype, cs_halo, cs_halo, cs_pad, cs_pad)
    end select
  end function single_call

  subroutine run_case(cmd)
    character(len=*), intent(in) :: cmd
    type(cmdline) :: c
    type(cudecompGridDescConfig) :: config
    type(cudecompPencilInfo) :: p
    integer :: gd(3), pd(2), backend, ac, op, f, ax, cur, nxt, side, nsides, copy
    logical :: inplace, nullhalo, use_stream, swap
    integer(int64) :: bad, nwords, fw, w, wsz, off
    integer(int64), allocatable, target :: u8(:), d8(:)
    real(real32), pointer, contiguous :: work1(:)
    integer(c_int) :: r

    call tokenize(cmd, c)
    gd(1) = opt_int(c, "--gx", 32)
    gd(2) = opt_int(c, "--gy", 32)
    gd(3) = opt_int(c, "--gz", 32)
    pd(1) = opt_int(c, "--pr", 0)
    pd(2) = opt_int(c, "--pc", 0)
    backend = opt_int(c, "--backend", 0)
    ac = opt_int(c, "--ac", 0)
    cs_halo(1) = opt_int(c, "--hex", 0)
    cs_halo(2) = opt_int(c, "--hey", 0)
    cs_halo(3) = opt_int(c, "--hez", 0)
    cs_pad(1) = opt_int(c, "--pdx", 0)
    cs_pad(2) = opt_int(c, "--pdy", 0)
    cs_pad(3) = opt_int(c, "--pdz", 0)
    cs_nf = opt_int(c, "--fields", 3)
    inplace = find_opt(c, "--inplace") /= 0
    nullhalo = find_opt(c, "--nullhalo") /= 0
    use_stream = find_opt(c, "--stream") /= 0
    swap = find_opt(c, "--self-check-swap-fields") /= 0
    if (backend == 0 .or. (nullhalo .and. (any(cs_pad /= 0) .or. any(cs_halo /= 0))) .or. cs_nf < 1 .or. cs_nf > 32) then
      write (error_unit, '(a)') "bad case line: --backend required, --nullhalo needs zero halos and padding, --fields 1..32"
      nfail = nfail + 1
      return
    end if
    if (use_stream .and. .not. have_stream) then
      call hipcheck(hipStreamCreate(my_stream), "hipStreamCreate")
      have_stream = .true.
    end if

    call check(cudecompGridDescConfigSetDefaults(config), "cudecompGridDescConfigSetDefaults")
    config%gdims = gd
    config%gdims_dist = gd
    config%pdims = pd
    config%transpose_axis_contiguous = (ac /= 0)
    config%transpose_comm_backend = backend
    r = cudecompGridDescCreate(handle, cs_grid_desc, config)
    if (r /= CUDECOMP_RESULT_SUCCESS) then
      write (error_unit, '(a,i0)') "cudecompGridDescCreate returned ", r
      nfail = nfail + 1
      return
    end if

    nwords = 0
    do ax = 1, 3
      call check(cudecompGetPencilInfo(handle, cs_grid_desc, p, ax, cs_halo, cs_pad), "cudecompGetPencilInfo")
      nwords = max(nwords, p%size)
    end do
    nwords = nwords + TAIL            ! 8-byte words of one buffer
    fw = nwords*2                     ! 4-byte words of one buffer
    nsides = merge(1, 2, inplace)
    ! the data buffer: [copy 1: fields call | copy 2: single calls] x [side] x [field]
    call check(cudecompMalloc(handle, cs_grid_desc, cs_data, fw*cs_nf*nsides*2), "cudecompMalloc data")
    call check(cudecompGetTransposeWorkspaceSize(handle, cs_grid_desc, wsz), "cudecompGetTransposeWorkspaceSize")
    call check(cudecompMalloc(handle, cs_grid_desc, cs_work, max(wsz, 1_int64)*cs_nf*2), "cudecompMalloc work")
    call check(cudecompMalloc(handle, cs_grid_desc, work1, max(wsz, 1_int64)*2), "cudecompMalloc single work")
    allocate (u8(nwords), d8(nwords))

    ! small integers that name (rank, field, cell), another pattern in the second buffers
    do copy = 1, 2
      do side = 1, nsides
        do f = 1, cs_nf
          do w = 1, nwords
            if (side == 1) then
              u8(w) = transfer(real(mod((w - 1)*7 + (f - 1)*131 + rank*17, 1021_int64), real64), 0_int64)
            else
              u8(w) = transfer(real(mod((w - 1)*3 + (f - 1)*29 + 5, 509_int64) + 1024, real64), 0_int64)
            end if
          end do
          off = slice(copy, side, f, nsides, fw)
          call hipcheck(hipMemcpy(c_loc(cs_data(off + 1)), c_loc(u8), int(nwords*8, c_size_t), hipMemcpyHostToDevice), "H2D")
        end do
      end do
    end do

    cur = 1
    do op = 1, 4
      nxt = merge(cur, 3 - cur, inplace)
      do f = 1, cs_nf
        cs_in(f) = c_loc(cs_data(slice(1, cur, f, nsides, fw) + 1))
        if (swap .and. .not. inplace) then
          cs_out(f) = c_loc(cs_data(slice(1, nxt, cs_nf + 1 - f, nsides, fw) + 1))
        else
          cs_out(f) = c_loc(cs_data(slice(1, nxt, f, nsides, fw) + 1))
        end if
      end do
      r = with_forms(op, .not. nullhalo, use_stream)
      if (r /= CUDECOMP_RESULT_SUCCESS) then
        write (error_unit, '(a,i0,a,i0)') "MISMATCH: the fields transpose ", op, " returned ", r
        nfail = nfail + 1
        exit
      end if
      call hipcheck(hipDeviceSynchronize(), "sync")
      do f = 1, cs_nf
        r = single_call(op, cs_data(slice(2, cur, f, nsides, fw) + 1:slice(2, cur, f, nsides, fw) + fw), &
                        cs_data(slice(2, nxt, f, nsides, fw) + 1:slice(2, nxt, f, nsides, fw) + fw), work1)
        if (r /= CUDECOMP_RESULT_SUCCESS) then
          write (error_unit, '(a,i0,a,i0)') "MISMATCH: the single transpose ", op, " returned ", r
          nfail = nfail + 1
        end if
      end do
      call hipcheck(hipDeviceSynchronize(), "sync")
      do side = 1, nsides
        do f = 1, cs_nf
          call hipcheck(hipMemcpy(c_loc(d8), c_loc(cs_data(slice(1, side, f, nsides, fw) + 1)), int(nwords*8, c_size_t), &
                                  hipMemcpyDeviceToHost), "D2H")
          call hipcheck(hipMemcpy(c_loc(u8), c_loc(cs_data(slice(2, side, f, nsides, fw) + 1)), int(nwords*8, c_size_t), &
                                  hipMemcpyDeviceToHost), "D2H")
          bad = count(d8 /= u8)
          if (bad /= 0) then
            nfail = nfail + 1
            write (error_unit, '(a,i0,a,i0,a,i0,a,i0,a,i0)') "MISMATCH: ", bad, " words of field ", f, " side ", side, &
              " differ from the single call after transpose ", op, " on rank ", rank
          end if
        end do
      end do
      if (nfail /= 0) exit
      cur = nxt
    end do
    if (swap .and. nfail == 0) write (error_unit, '(a)') "the swapped fields went unnoticed"

    call check(cudecompFree(handle, cs_grid_desc, work1), "cudecompFree single work")
    call check(cudecompFree(handle, cs_grid_desc, cs_work), "cudecompFree work")
    call check(cudecompFree(handle, cs_grid_desc, cs_data), "cudecompFree data")
    call check(cudecompGridDescDestroy(handle, cs_grid_desc), "cudecompGridDescDestroy")

  end subroutine run_case

  ! 4-byte words in front of buffer (copy, side, field) of the data buffer
  integer(int64) function slice(copy, side, f, nsides, fw)
    integer, intent(in) :: copy, side, f, nsides
    integer(int64), intent(in) :: fw
    slice = (int(((copy - 1)*nsides + (side - 1)), int64)*cs_nf + (f - 1))*fw
  end function slice

end program transpose_fields_test
