! halo_fields_test.f90 -- Fortran twin of tests/native/halo_fields_test.cpp: multi-field halo updates (cudecomp_halo_fields.h)
! through the wrappers cudecompAmdUpdateFieldHalos{X,Y,Z} of module `cudecomp`, fp64.  Per case: --fields N pencils (slices of one
! buffer from cudecompMalloc, their addresses passed as an array of type(c_ptr)) are uploaded, the fields call runs along dims 1, 2, 3
! in turn through the X, Y or Z wrapper of --ax, and after every dim every field is downloaded and the whole buffer -- halos of all
! dims, padding, a poisoned tail -- compared bit for bit with the closed form of the C++ twin (see there: a table "does the cell
! still hold the +8 it started with", carried from dim to dim).
! The same case lines in FORTRAN conventions (--ax and --mem_order one-based).
!
!   the options of halo_test, plus
!   --fields N  the number of pencils (1 .. 32)
!   --nullpad   `padding` absent (needs zero padding)       --stream   `stream` present: a stream this program created
!   --self-check-shift-dim      call along mod(dim, 3) + 1 while expecting dim: the case must FAIL
! At the end rank 0 prints one line "WRAPPER <name>" per wrapper that was called in a case that passed.
program halo_fields_test
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

  integer, parameter :: BUMP = 8, POISON = -77, TAIL = 64
  character(len=32), parameter :: WRAPPER_NAMES(3) = [character(len=32) :: &
    "cudecompAmdUpdateFieldHalosX", "cudecompAmdUpdateFieldHalosY", "cudecompAmdUpdateFieldHalosZ"]

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
  real(real32), pointer, contiguous :: cs_data(:), cs_work(:)
  type(c_ptr) :: cs_fields(32)
  integer :: cs_halo(3), cs_pad(3), cs_nf
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
    case (1); r = cudecompAmdUpdateFieldHalosX(handle, cs_grid_desc, cs_fields(1:cs_nf), cs_nf, cs_work, dtype, cs_halo, cs_periods, &
                                               dim, pad_o, stream_o)
    case (2); r = cudecompAmdUpdateFieldHalosY(handle, cs_grid_desc, cs_fields(1:cs_nf), cs_nf, cs_work, dtype, cs_halo, cs_periods, &
                                               dim, pad_o, stream_o)
    case (3); r = cudecompAmdUpdateFieldHalosZ(handle, cs_grid_desc, cs_fields(1:cs_nf), cs_nf, cs_work, dtype, cs_halo, cs_periods, &
                                               dim, pad_o, stream_o)
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

  ! words = what field ff holds in the model's current state (a standard-conforming sibling of run_case: an internal procedure
  ! may not contain another)
  subroutine encode_field(ff, ncells, cell, bumped, base, words)
    integer, intent(in) :: ff
    integer(int64), intent(in) :: ncells
    logical, intent(in) :: cell(:), bumped(:)
    integer, intent(in) :: base(:)
    integer(int64), intent(out) :: words(:)
    integer(int64) :: e
    words = bits8(POISON)
    do e = 1, ncells
      if (cell(e)) words(e) = bits8(base(e) + 20*(ff - 1) + merge(BUMP, 0, bumped(e)))
    end do
  end subroutine encode_field

  subroutine run_case(cmd)
    character(len=*), intent(in) :: cmd
    type(cmdline) :: c
    type(cudecompGridDescConfig) :: config
    type(cudecompPencilInfo) :: p
    integer :: gd(3), gdd(3), pd(2), backend, axis, iper(3), mo(3), ac, rank_order, dim, ax2, f
    integer :: call_dim, kd, h, n, j, l(3), g(3), hk, i0, i1, i2, shown, kof(3)
    logical :: nullpad, use_stream, shift, low, high, padding, ghost
    integer(int64) :: bad, idx, nwords, stride(3), w, wsz, fw
    integer, allocatable :: base(:)
    logical, allocatable :: cell(:), bumped(:)
    integer(int64), allocatable, target :: u8(:), d8(:)
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
    cs_periods = (iper /= 0)
    mo = -1
    call opt_ints(c, "--mem_order", mo)
    nullpad = find_opt(c, "--nullpad") /= 0
    use_stream = find_opt(c, "--stream") /= 0
    shift = find_opt(c, "--self-check-shift-dim") /= 0
    if (axis < 1 .or. axis > 3 .or. backend == 0 .or. (nullpad .and. any(cs_pad /= 0)) .or. cs_nf < 1 .or. cs_nf > 32) then
      write (error_unit, '(a)') "bad case line: --ax 1..3, --backend required, --nullpad needs zero padding, --fields 1..32"
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
    call check(cudecompMalloc(handle, cs_grid_desc, cs_data, fw*cs_nf), "cudecompMalloc data")
    call check(cudecompGetHaloWorkspaceSize(handle, cs_grid_desc, axis, cs_halo, wsz), "cudecompGetHaloWorkspaceSize")
    call check(cudecompMalloc(handle, cs_grid_desc, cs_work, max(wsz, 1_int64)*cs_nf*2), "cudecompMalloc work")
    do f = 1, cs_nf
      cs_fields(f) = c_loc(cs_data((f - 1)*fw + 1))
    end do

    allocate (base(p%size), cell(p%size), bumped(p%size), u8(nwords), d8(nwords))
    stride = [1_int64, int(p%shape(1), int64), int(p%shape(1), int64)*p%shape(2)]
    do kd = 1, 3
      kof(p%order(kd)) = kd
    end do

    ! what is uploaded: V_f + 8 in the ghost cells of ANY dim, -77 in padding and tail
    base = 0
    cell = .false.
    bumped = .false.
    idx = 0
    do i2 = 1, p%shape(3)
      do i1 = 1, p%shape(2)
        do i0 = 1, p%shape(1)
          idx = idx + 1
          l = [i0, i1, i2]
          padding = .false.
          ghost = .false.
          do k = 1, 3
            ax2 = p%order(k)
            hk = cs_halo(ax2)
            n = (p%hi(k) - p%lo(k) + 1) + 2*hk
            if (l(k) > n) padding = .true.
            if (l(k) <= hk .or. l(k) > n - hk) ghost = .true.
            g(ax2) = modulo((p%lo(k) - 1) + (l(k) - 1 - hk), gd(ax2))  ! zero-based, wrapped
          end do
          if (padding) cycle
          cell(idx) = .true.
          bumped(idx) = ghost
          base(idx) = modulo(g(1) + 3*g(2) + 5*g(3), 7)
        end do
      end do
    end do
    do f = 1, cs_nf
      call encode_field(f, p%size, cell, bumped, base, u8)
      call hipcheck(hipMemcpy(cs_fields(f), c_loc(u8), int(nwords*8, c_size_t), hipMemcpyHostToDevice), "H2D")
    end do

    do dim = 1, 3
      call check(cudecompGetShiftedRank(handle, cs_grid_desc, axis, dim, -1, cs_periods(dim), nb), "cudecompGetShiftedRank")
      low = nb /= -1
      call check(cudecompGetShiftedRank(handle, cs_grid_desc, axis, dim, 1, cs_periods(dim), nb), "cudecompGetShiftedRank")
      high = nb /= -1
      kd = kof(dim)
      h = cs_halo(dim)
      n = (p%hi(kd) - p%lo(kd) + 1) + 2*h  ! the extent along dim without padding
      ! a halo cell along dim on a side with a neighbour takes the state of the cell at the same position of the other two dims that
      ! is interior along dim (zero-based index h)
      if (h > 0) then
        idx = 0
        do i2 = 1, p%shape(3)
          do i1 = 1, p%shape(2)
            do i0 = 1, p%shape(1)
              idx = idx + 1
              if (.not. cell(idx)) cycle
              l = [i0, i1, i2]
              j = l(kd) - 1
              if ((j < h .and. low) .or. (j >= n - h .and. j < n .and. high)) bumped(idx) = bumped(idx + (h - j)*stride(kd))
            end do
          end do
        end do
      end if

      call_dim = dim
      if (shift) call_dim = mod(dim, 3) + 1
      r = with_forms(axis, call_dim, .not. nullpad, use_stream)
      if (r /= CUDECOMP_RESULT_SUCCESS) then
        write (error_unit, '(a,i0,a,i0)') "MISMATCH: the fields update along dim ", call_dim, " returned ", r
        nfail = nfail + 1
        exit
      end if
      call hipcheck(hipDeviceSynchronize(), "sync")

      do f = 1, cs_nf
        call encode_field(f, p%size, cell, bumped, base, u8)
        bad = 0
        shown = 0
        call hipcheck(hipMemcpy(c_loc(d8), cs_fields(f), int(nwords*8, c_size_t), hipMemcpyDeviceToHost), "D2H")
        do w = 1, nwords
          if (d8(w) /= u8(w)) then
            bad = bad + 1
            if (shown < 4) write (error_unit, '(a,i0,a,i0,a,i0,a,z16.16,a,z16.16)') "rank ", rank, ": field ", f, " word ", w, &
              " holds ", d8(w), ", expected ", u8(w)
            shown = shown + 1
          end if
        end do
        if (bad /= 0) then
          nfail = nfail + 1
          write (error_unit, '(a,i0,a,i0,a,i0,a,i0)') "MISMATCH: ", bad, " words of field ", f, " differ after the update along dim ", &
            dim, " on rank ", rank
        end if
      end do
      if (shift) exit
    end do

    call check(cudecompFree(handle, cs_grid_desc, cs_work), "cudecompFree work")
    call check(cudecompFree(handle, cs_grid_desc, cs_data), "cudecompFree data")
    call check(cudecompGridDescDestroy(handle, cs_grid_desc), "cudecompGridDescDestroy")

  end subroutine run_case

end program halo_fields_test
