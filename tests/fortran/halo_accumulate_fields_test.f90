! halo_accumulate_fields_test.f90 -- Fortran twin of tests/native/halo_accumulate_fields_test.cpp: multi-field halo accumulation
! (cudecomp_halo_accumulate_fields.h) through the wrappers cudecompAmdAccumulateFieldHalos{X,Y,Z} of module `cudecomp`, fp64.  Per
! case: --fields N pencils (slices of one buffer from cudecompMalloc, their addresses passed as an array of type(c_ptr)) are uploaded
! twice; the fields call runs along dims 3, 2, 1 in turn on the first set through the X, Y or Z wrapper of --ax (--clear 0 / 1), the
! single wrapper the header names as its definition (cudecompAmdAccumulateHalos* / cudecompAmdAccumulateAndClearHalos*) on every
! pencil of the second set; after every dim every field is downloaded and the whole buffer -- halos of all dims, padding, a poisoned
! tail -- compared bit for bit with its twin.  A dim along which the rank has a neighbour and a halo must have changed every field.
! The same case lines in FORTRAN conventions (--ax and --mem_order one-based).
!
!   the options of halo_test, plus
!   --fields N  the number of pencils (1 .. 32)             --clear C   0 / 1
!   --nullpad   `padding` absent (needs zero padding)       --stream   `stream` present: a stream this program created
!   --self-check-shift-dim      call along mod(dim, 3) + 1 while the single calls run along dim: the case must FAIL
! At the end rank 0 prints one line "WRAPPER <name>" per wrapper that was called in a case that passed.
program halo_accumulate_fields_test
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

  integer, parameter :: POISON = -77, TAIL = 64
  character(len=32), parameter :: WRAPPER_NAMES(3) = [character(len=32) :: &
    "cudecompAmdAccumulateFieldHalosX", "cudecompAmdAccumulateFieldHalosY", "cudecompAmdAccumulateFieldHalosZ"]

  type(cudecompHandle) :: handle
  integer :: rank, nranks, ndev, dtype_sel, dtype, wpe, i, ncases, res, nfailed, u, stat, argn, k
  integer(int64) :: es
  character(len=1024) :: line, arg, testfile, progname
  character(len=1024), allocatable :: cases(:)
  logical :: from_file
  integer :: c0, c1, rate
  logical :: called(3), called_in_case(3)
  integer(cudecomp_stream_kind) :: my_stream
  logical :: have_stream

  ! the case the wrappers are called for (call_wrapper and its callers are internal procedures of the program)
  type(cudecompGridDesc) :: cs_grid_desc
  real(real32), pointer, contiguous :: cs_data(:), cs_work(:), cs_single_work(:)
  type(c_ptr) :: cs_fields(32)
  integer :: cs_halo(3), cs_pad(3), cs_nf, cs_clear
  logical :: cs_periods(3)

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
    do k = 1, 3
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

  ! one of the three wrappers; absent optional arguments stay absent all the way down
  function call_wrapper(axis, dim, pad_o, stream_o) result(r)
    integer, intent(in) :: axis, dim
    integer, optional :: pad_o(3)
    integer(cudecomp_stream_kind), optional :: stream_o
    integer(c_int) :: r
    r = -1
    called_in_case(axis) = .true.
    select case (axis)
    case (1); r = cudecompAmdAccumulateFieldHalosX(handle, cs_grid_desc, cs_fields(1:cs_nf), cs_nf, cs_work, dtype, cs_halo, &
                                                   cs_periods, dim, cs_clear, pad_o, stream_o)
    case (2); r = cudecompAmdAccumulateFieldHalosY(handle, cs_grid_desc, cs_fields(1:cs_nf), cs_nf, cs_work, dtype, cs_halo, &
                                                   cs_periods, dim, cs_clear, pad_o, stream_o)
    case (3); r = cudecompAmdAccumulateFieldHalosZ(handle, cs_grid_desc, cs_fields(1:cs_nf), cs_nf, cs_work, dtype, cs_halo, &
                                                   cs_periods, dim, cs_clear, pad_o, stream_o)
    end select
  end function call_wrapper

  ! `padding` and `stream` present or absent
  function with_forms(axis, dim, use_pad, use_stream) result(r)
    integer, intent(in) :: axis, dim
    logical, intent(in) :: use_pad, use_stream
    integer(c_int) :: r
    if (use_pad .and. use_stream) then
      r = call_wrapper(axis, dim, pad_o=cs_pad, stream_o=my_stream)
    else if (use_pad) then
      r = call_wrapper(axis, dim, pad_o=cs_pad)
    else if (use_stream) then
      r = call_wrapper(axis, dim, stream_o=my_stream)
    else
      r = call_wrapper(axis, dim)
    end if
  end function with_forms

  integer(int64) function bits8(v)
    integer, intent(in) :: v
    bits8 = transfer(real(v, real64), 0_int64)
  end function bits8

  ! the single call along `dim` on the pencil that begins at word `first` of cs_data
  function call_single(axis, dim, first, use_pad) result(r)
    integer, intent(in) :: axis, dim
    integer(int64), intent(in) :: first
    logical, intent(in) :: use_pad
    integer(c_int) :: r
    integer :: pd3(3)
    pd3 = 0
    if (use_pad) pd3 = cs_pad
    r = -1
    if (cs_clear /= 0) then
      select case (axis)
      case (1); r = cudecompAmdAccumulateAndClearHalosX(handle, cs_grid_desc, cs_data(first:), cs_single_work, dtype, cs_halo, cs_periods, dim, pd3)
      case (2); r = cudecompAmdAccumulateAndClearHalosY(handle, cs_grid_desc, cs_data(first:), cs_single_work, dtype, cs_halo, cs_periods, dim, pd3)
      case (3); r = cudecompAmdAccumulateAndClearHalosZ(handle, cs_grid_desc, cs_data(first:), cs_single_work, dtype, cs_halo, cs_periods, dim, pd3)
      end select
    else
      select case (axis)
      case (1); r = cudecompAmdAccumulateHalosX(handle, cs_grid_desc, cs_data(first:), cs_single_work, dtype, cs_halo, cs_periods, dim, pd3)
      case (2); r = cudecompAmdAccumulateHalosY(handle, cs_grid_desc, cs_data(first:), cs_single_work, dtype, cs_halo, cs_periods, dim, pd3)
      case (3); r = cudecompAmdAccumulateHalosZ(handle, cs_grid_desc, cs_data(first:), cs_single_work, dtype, cs_halo, cs_periods, dim, pd3)
      end select
    end if
  end function call_single

  subroutine run_case(cmd)
    character(len=*), intent(in) :: cmd
    type(cmdline) :: c
    type(cudecompGridDescConfig) :: config
    type(cudecompPencilInfo) :: p
    integer :: gd(3), gdd(3), pd(2), backend, axis, iper(3), mo(3), ac, rank_order, dim, ax2, f
    integer :: call_dim, k2, hk, n, l(3), i0, i1, i2, shown
    logical :: nullpad, use_stream, shift, low, high, padding, active
    integer(int64) :: bad, idx, nwords, w, wsz, fw
    logical, allocatable :: cell(:)
    integer(int64), allocatable, target :: u8(:), d8(:), before(:, :)
    integer(c_int32_t) :: nb
    integer(c_int) :: r

    call tokenize(cmd, c)
    gd(1) = opt_int(c, "--gx", 256)
    gd(2) = opt_int(c, "--gy", 256)
    gd(3) = opt_int(c, "--gz", 256)
    pd(1) = opt_int(c, "--pr", 0)
    pd(2) = opt_int(c, "--pc", 0)
    rank_order = opt_int(c, "--rank-order", 0)
    backend = opt_int(c, "--backend", 0)
    ac = opt_int(c, "--ac", 0)
    gdd = 0
    call opt_ints(c, "--gd", gdd)
    cs_halo(1) = opt_int(c, "--hex", 1)
    cs_halo(2) = opt_int(c, "--hey", 1)
    cs_halo(3) = opt_int(c, "--hez", 1)
    iper(1) = opt_int(c, "--hpx", 1)
    iper(2) = opt_int(c, "--hpy", 1)
    iper(3) = opt_int(c, "--hpz", 1)
    cs_pad(1) = opt_int(c, "--pdx", 0)
    cs_pad(2) = opt_int(c, "--pdy", 0)
    cs_pad(3) = opt_int(c, "--pdz", 0)
    axis = opt_int(c, "--ax", 1)
    cs_nf = opt_int(c, "--fields", 3)
    cs_clear = opt_int(c, "--clear", 0)
    cs_periods = (iper /= 0)
    mo = -1
    call opt_ints(c, "--mem_order", mo)
    nullpad = find_opt(c, "--nullpad") /= 0
    use_stream = find_opt(c, "--stream") /= 0
    shift = find_opt(c, "--self-check-shift-dim") /= 0
    if (axis < 1 .or. axis > 3 .or. backend == 0 .or. (nullpad .and. any(cs_pad /= 0)) .or. cs_nf < 1 .or. cs_nf > 32 .or. cs_clear < 0 .or. cs_clear > 1) then
      write (error_unit, '(a)') "bad case line: --ax 1..3, --backend required, --nullpad needs zero padding, --fields 1..32, --clear 0 / 1"
      nfail = nfail + 1
      return
    end if
    if (use_stream .and. .not. have_stream) then
      call hipcheck(hipStreamCreate(my_stream), "hipStreamCreate")
      have_stream = .true.
    end if

    call check(cudecompGridDescConfigSetDefaults(config), "cudecompGridDescConfigSetDefaults")
    config%gdims = gd
    config%gdims_dist = gd - gdd
    config%pdims = pd
    config%rank_order = rank_order
    config%transpose_axis_contiguous = (ac /= 0)
    if (find_opt(c, "--mem_order") /= 0) then
      do ax2 = 1, 3
        config%transpose_mem_order(:, ax2) = mo
      end do
    end if
    config%halo_comm_backend = backend
    r = cudecompGridDescCreate(handle, cs_grid_desc, config)
    if (r /= CUDECOMP_RESULT_SUCCESS) then
      write (error_unit, '(a,i0)') "cudecompGridDescCreate returned ", r
      nfail = nfail + 1
      return
    end if

    call check(cudecompGetPencilInfo(handle, cs_grid_desc, p, axis, cs_halo, cs_pad), "cudecompGetPencilInfo")
    nwords = p%size + TAIL            ! 8-byte words of one field
    fw = nwords*2                     ! 4-byte words of one field
    call check(cudecompMalloc(handle, cs_grid_desc, cs_data, fw*cs_nf*2), "cudecompMalloc data")  ! the fields, then their twins
    call check(cudecompGetHaloWorkspaceSize(handle, cs_grid_desc, axis, cs_halo, wsz), "cudecompGetHaloWorkspaceSize")
    call check(cudecompMalloc(handle, cs_grid_desc, cs_work, max(wsz, 1_int64)*cs_nf*2), "cudecompMalloc work")
    call check(cudecompMalloc(handle, cs_grid_desc, cs_single_work, max(wsz, 1_int64)*2), "cudecompMalloc single work")
    do f = 1, cs_nf
      cs_fields(f) = c_loc(cs_data((f - 1)*fw + 1))
    end do

    allocate (cell(p%size), u8(nwords), d8(nwords), before(nwords, cs_nf))
    ! what is uploaded: ((7 e + 3 f) mod 11) - 5 in cell e (zero-based) of field f (zero-based), -77 in padding and tail
    cell = .false.
    idx = 0
    do i2 = 1, p%shape(3)
      do i1 = 1, p%shape(2)
        do i0 = 1, p%shape(1)
          idx = idx + 1
          l = [i0, i1, i2]
          padding = .false.
          do k2 = 1, 3
            hk = cs_halo(p%order(k2))
            n = (p%hi(k2) - p%lo(k2) + 1) + 2*hk
            if (l(k2) > n) padding = .true.
          end do
          cell(idx) = .not. padding
        end do
      end do
    end do
    do f = 1, cs_nf
      u8 = bits8(POISON)
      do w = 1, p%size
        if (cell(w)) u8(w) = bits8(int(modulo(7*(w - 1) + 3*(f - 1), 11_int64)) - 5)
      end do
      before(:, f) = u8
      call hipcheck(hipMemcpy(cs_fields(f), c_loc(u8), int(nwords*8, c_size_t), hipMemcpyHostToDevice), "H2D")
      call hipcheck(hipMemcpy(c_loc(cs_data((cs_nf + f - 1)*fw + 1)), c_loc(u8), int(nwords*8, c_size_t), hipMemcpyHostToDevice), "H2D")
    end do

    do dim = 3, 1, -1
      call check(cudecompGetShiftedRank(handle, cs_grid_desc, axis, dim, -1, cs_periods(dim), nb), "cudecompGetShiftedRank")
      low = nb /= -1
      call check(cudecompGetShiftedRank(handle, cs_grid_desc, axis, dim, 1, cs_periods(dim), nb), "cudecompGetShiftedRank")
      high = nb /= -1
      active = cs_halo(dim) > 0 .and. (low .or. high)

      call_dim = dim
      if (shift) call_dim = mod(dim, 3) + 1
      r = with_forms(axis, call_dim, .not. nullpad, use_stream)
      do f = 1, cs_nf
        if (r == CUDECOMP_RESULT_SUCCESS) r = call_single(axis, dim, (cs_nf + f - 1)*fw + 1, .not. nullpad)
      end do
      if (r /= CUDECOMP_RESULT_SUCCESS) then
        write (error_unit, '(a,i0,a,i0)') "MISMATCH: the accumulation along dim ", call_dim, " returned ", r
        nfail = nfail + 1
        exit
      end if
      call hipcheck(hipDeviceSynchronize(), "sync")

      do f = 1, cs_nf
        bad = 0
        shown = 0
        call hipcheck(hipMemcpy(c_loc(d8), cs_fields(f), int(nwords*8, c_size_t), hipMemcpyDeviceToHost), "D2H")
        call hipcheck(hipMemcpy(c_loc(u8), c_loc(cs_data((cs_nf + f - 1)*fw + 1)), int(nwords*8, c_size_t), hipMemcpyDeviceToHost), "D2H")
        do w = 1, nwords
          if (d8(w) /= u8(w)) then
            bad = bad + 1
            if (shown < 4) write (error_unit, '(a,i0,a,i0,a,i0,a,z16.16,a,z16.16)') "rank ", rank, ": field ", f, " word ", w, &
              " holds ", d8(w), ", the single call made ", u8(w)
            shown = shown + 1
          end if
        end do
        if (bad /= 0) then
          nfail = nfail + 1
          write (error_unit, '(a,i0,a,i0,a,i0,a,i0)') "MISMATCH: ", bad, " words of field ", f, " differ after the accumulation along dim ", &
            dim, " on rank ", rank
        end if
        if (active .and. all(u8 == before(:, f))) then
          nfail = nfail + 1
          write (error_unit, '(a,i0,a,i0)') "MISMATCH: the single accumulation changed nothing of field ", f, " along dim ", dim
        end if
        before(:, f) = u8
      end do
      if (shift) exit
    end do

    call check(cudecompFree(handle, cs_grid_desc, cs_single_work), "cudecompFree single work")
    call check(cudecompFree(handle, cs_grid_desc, cs_work), "cudecompFree work")
    call check(cudecompFree(handle, cs_grid_desc, cs_data), "cudecompFree data")
    call check(cudecompGridDescDestroy(handle, cs_grid_desc), "cudecompGridDescDestroy")

  end subroutine run_case

end program halo_accumulate_fields_test
