! halo_wall_values_test.f90 -- Fortran twin of tests/native/halo_wall_values_test.cpp: wall values (cudecomp_halo_wall_values.h)
! through the wrappers cudecompAmdSetWallHalos{X,Y,Z} of module `cudecomp` and nothing else; fp64 or complex fp64 by the program's
! name (halo_wall_values_test_R64, ..._C64).  Per case: one pencil is uploaded and the call runs along dims 1, 2, 3 in turn through
! the X, Y or Z wrapper of --ax; after every call the whole buffer -- halos of all dims, padding, a poisoned tail -- is downloaded and
! compared bit for bit with the header's definition applied on the host to the whole pencil: on the sides that --sides names and
! where cudecompGetShiftedRank names no neighbour, for k in [0, h), c = --centering and s = --parity (zero-based cells),
!   low side:   cell(h-1-k) = s cell(h+k+c)     + a_low(k+1)
!   high side:  cell(n-h+k) = s cell(n-h-1-k-c) + a_high(k+1)
! A dim along which the rank has a wall, a halo and a named side must have changed the pencil.  Payload: the twin's payload(e, 0) in
! cell e (zero-based), payload(e, 50) in the imaginary part; -77 in padding and tail.  Addends: layer k1 = 1 .. h (layer 1 next to
! the wall), called dim d = 1 .. 3: a_low(k1) = 100 + 10 k1 + d, a_high(k1) = -(200 + 10 k1 + d), imaginary parts + 5 and - 5 from
! those, re and im interleaved (2 h doubles).  Small integers, never zero: every sum is exact and no result is -0.
! The value arrays are local to the procedure that calls the wrapper and are overwritten with NaNs as soon as it has returned, before
! any synchronisation; the array of the side that --sides leaves out is absent or holds NaNs.
! The same case lines in FORTRAN conventions (--ax, --dim and --mem_order one-based).
!
!   the options of halo_test, plus
!   --parity P  +1 / -1        --centering C  0 / 1        --sides S  1 low, 2 high, 3 both
!   --nullpad   `padding` absent (needs zero padding)       --stream   `stream` present: a stream this program created
!   --unnamed null | garbage   the array of the side --sides leaves out: absent, or NaNs that must leave no trace
!   --expect-refusal invalid | unsupported  --dim D   one call along D: CUDECOMP_RESULT_INVALID_USAGE / CUDECOMP_RESULT_NOT_SUPPORTED
!                              and an untouched pencil (--sides is passed as given)
!   --named-null               (with --expect-refusal) the arrays of the sides that --sides names are absent
!   --self-check-reverse-layers     the expectation uses a(h-k): the case must FAIL
!   --self-check-swap-sides         the expectation exchanges the two arrays: the case must FAIL
! At the end rank 0 prints one line "WRAPPER <name>" per wrapper that was called in a case that passed.
program halo_wall_values_test
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

  integer, parameter :: POISON = -77, TAIL = 64, MAXV = 32
  character(len=32), parameter :: WRAPPER_NAMES(3) = [character(len=32) :: &
    "cudecompAmdSetWallHalosX", "cudecompAmdSetWallHalosY", "cudecompAmdSetWallHalosZ"]

  type(cudecompHandle) :: handle
  integer :: rank, nranks, ndev, dtype, wpe, i, ncases, res, nfailed, u, stat, argn, k
  character(len=1024) :: line, arg, testfile, progname
  character(len=1024), allocatable :: cases(:)
  logical :: from_file
  integer :: c0, c1, rate
  logical :: called(3), called_in_case(3)
  integer(cudecomp_stream_kind) :: my_stream
  logical :: have_stream

  ! the case the wrappers are called for (call_wrapper and its callers are internal procedures of the program)
  type(cudecompGridDesc) :: cs_grid_desc
  real(real32), pointer, contiguous :: cs_data(:)
  integer :: cs_halo(3), cs_pad(3), cs_parity, cs_centering, cs_sides
  logical :: cs_periods(3)

  rank = env_int("RANK", env_int("PMI_RANK", env_int("OMPI_COMM_WORLD_RANK", 0)))
  nranks = env_int("WORLD_SIZE", env_int("PMI_SIZE", env_int("OMPI_COMM_WORLD_SIZE", 1)))
  if (dtype_from_program_name() == 4) then
    dtype = CUDECOMP_DOUBLE_COMPLEX
    wpe = 2
  else
    dtype = CUDECOMP_DOUBLE
    wpe = 1
  end if
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

  ! component q (0 re, 1 im) of the addend of ghost layer k1 (1 next to the wall) on `side` (1 low, 2 high) for the call along `dim`
  integer function addend(side, k1, dim, q)
    integer, intent(in) :: side, k1, dim, q
    if (side == 1) then
      addend = 100 + 10*k1 + dim + 5*q
    else
      addend = -(200 + 10*k1 + dim + 5*q)
    end if
  end function addend

  ! one of the three wrappers; absent optional arguments stay absent all the way down
  function call_wrapper(axis, dim, low_o, high_o, pad_o, stream_o) result(r)
    integer, intent(in) :: axis, dim
    real(c_double), optional, target :: low_o(*), high_o(*)
    integer, optional :: pad_o(3)
    integer(cudecomp_stream_kind), optional :: stream_o
    integer(c_int) :: r
    r = -1
    called_in_case(axis) = .true.
    select case (axis)
    case (1); r = cudecompAmdSetWallHalosX(handle, cs_grid_desc, cs_data, dtype, cs_parity, cs_centering, cs_sides, low_o, high_o, &
                                           cs_halo, cs_periods, dim, pad_o, stream_o)
    case (2); r = cudecompAmdSetWallHalosY(handle, cs_grid_desc, cs_data, dtype, cs_parity, cs_centering, cs_sides, low_o, high_o, &
                                           cs_halo, cs_periods, dim, pad_o, stream_o)
    case (3); r = cudecompAmdSetWallHalosZ(handle, cs_grid_desc, cs_data, dtype, cs_parity, cs_centering, cs_sides, low_o, high_o, &
                                           cs_halo, cs_periods, dim, pad_o, stream_o)
    end select
  end function call_wrapper

  ! `padding` and `stream` present or absent
  function with_forms(axis, dim, use_pad, use_stream, low_o, high_o) result(r)
    integer, intent(in) :: axis, dim
    logical, intent(in) :: use_pad, use_stream
    real(c_double), optional, target :: low_o(*), high_o(*)
    integer(c_int) :: r
    if (use_pad .and. use_stream) then
      r = call_wrapper(axis, dim, low_o, high_o, pad_o=cs_pad, stream_o=my_stream)
    else if (use_pad) then
      r = call_wrapper(axis, dim, low_o, high_o, pad_o=cs_pad)
    else if (use_stream) then
      r = call_wrapper(axis, dim, low_o, high_o, stream_o=my_stream)
    else
      r = call_wrapper(axis, dim, low_o, high_o)
    end if
  end function with_forms

  ! the value arrays: temporaries of this procedure, present or absent, NaNs from the moment the wrapper has returned.  fill(side):
  ! the array holds the addends of `dim`, otherwise NaNs.
  function with_values(axis, dim, h, use_pad, use_stream, present_low, present_high, fill_low, fill_high) result(r)
    integer, intent(in) :: axis, dim, h
    logical, intent(in) :: use_pad, use_stream, present_low, present_high, fill_low, fill_high
    integer(c_int) :: r
    real(c_double) :: vlow(MAXV), vhigh(MAXV), nan
    integer :: k1, q
    nan = transfer(int(z'7FF8000000000000', int64), 1.0_real64)
    vlow = nan
    vhigh = nan
    do k1 = 1, h
      do q = 0, wpe - 1
        if (fill_low) vlow((k1 - 1)*wpe + q + 1) = real(addend(1, k1, dim, q), c_double)
        if (fill_high) vhigh((k1 - 1)*wpe + q + 1) = real(addend(2, k1, dim, q), c_double)
      end do
    end do
    if (present_low .and. present_high) then
      r = with_forms(axis, dim, use_pad, use_stream, low_o=vlow, high_o=vhigh)
    else if (present_low) then
      r = with_forms(axis, dim, use_pad, use_stream, low_o=vlow)
    else if (present_high) then
      r = with_forms(axis, dim, use_pad, use_stream, high_o=vhigh)
    else
      r = with_forms(axis, dim, use_pad, use_stream)
    end if
    vlow = nan
    vhigh = nan
  end function with_values

  integer(int64) function bits8(v)
    integer, intent(in) :: v
    bits8 = transfer(real(v, real64), 0_int64)
  end function bits8

  subroutine run_case(cmd)
    character(len=*), intent(in) :: cmd
    type(cmdline) :: c
    type(cudecompGridDescConfig) :: config
    type(cudecompPencilInfo) :: p
    integer :: gd(3), gdd(3), pd(2), backend, axis, iper(3), mo(3), ac, rank_order, dim, ax2, side, a_side, a_k
    integer :: k2, km, ka, kb, shown, iop, first, last, q, expected
    logical :: nullpad, use_stream, garbage, refusal, named_null, reverse, swap, wall(2), writes(2), named(2), pres(2), active, bad_line
    integer(int64) :: bad, nwords, w, ext(3), stride(3), i0, i1, i2, h, n, cc, k, ghost, inner, ia, ib, at, gi, ii
    integer, allocatable :: m(:), before(:)
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
    cs_parity = opt_int(c, "--parity", 1)
    cs_centering = opt_int(c, "--centering", 0)
    cs_sides = opt_int(c, "--sides", 3)
    cs_periods = (iper /= 0)
    mo = -1
    call opt_ints(c, "--mem_order", mo)
    nullpad = find_opt(c, "--nullpad") /= 0
    use_stream = find_opt(c, "--stream") /= 0
    named_null = find_opt(c, "--named-null") /= 0
    reverse = find_opt(c, "--self-check-reverse-layers") /= 0
    swap = find_opt(c, "--self-check-swap-sides") /= 0
    bad_line = .false.
    garbage = .false.
    iop = find_opt(c, "--unnamed")
    if (iop /= 0) then
      if (iop >= c%n) then
        bad_line = .true.
      else if (trim(c%tok(iop + 1)) == "garbage") then
        garbage = .true.
      else if (trim(c%tok(iop + 1)) /= "null") then
        bad_line = .true.
      end if
    end if
    expected = CUDECOMP_RESULT_SUCCESS
    iop = find_opt(c, "--expect-refusal")
    refusal = iop /= 0
    first = 1
    last = 3
    if (refusal) then
      if (iop >= c%n) then
        bad_line = .true.
      else if (trim(c%tok(iop + 1)) == "invalid") then
        expected = CUDECOMP_RESULT_INVALID_USAGE
      else if (trim(c%tok(iop + 1)) == "unsupported") then
        expected = CUDECOMP_RESULT_NOT_SUPPORTED
      else
        bad_line = .true.
      end if
      first = opt_int(c, "--dim", 0)
      last = first
      if (first < 1 .or. first > 3) bad_line = .true.
    end if
    if (bad_line .or. axis < 1 .or. axis > 3 .or. backend == 0 .or. (nullpad .and. any(cs_pad /= 0)) .or. cs_centering < 0 .or. &
        cs_centering > 1 .or. abs(cs_parity) /= 1 .or. (.not. refusal .and. (cs_sides < 1 .or. cs_sides > 3)) .or. &
        (named_null .and. .not. refusal) .or. any(cs_halo*wpe > MAXV)) then
      write (error_unit, '(a)') "bad case line: --parity +1 / -1, --centering 0 / 1, --sides 1..3, --unnamed null | garbage, --ax 1..3, "// &
        "--backend required, --nullpad needs zero padding, --expect-refusal invalid | unsupported with --dim 1..3"
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
    nwords = (p%size + TAIL)*wpe      ! 8-byte words
    call check(cudecompMalloc(handle, cs_grid_desc, cs_data, nwords*2), "cudecompMalloc data")

    ! the pencil's own cells: extent without padding and stride of every memory position
    do k2 = 1, 3
      ext(k2) = (p%hi(k2) - p%lo(k2) + 1) + 2*cs_halo(p%order(k2))
    end do
    stride(1) = 1
    stride(2) = p%shape(1)
    stride(3) = int(p%shape(1), int64)*p%shape(2)
    allocate (m(nwords), before(nwords), u8(nwords), d8(nwords))
    m = POISON
    do i2 = 0, ext(3) - 1
      do i1 = 0, ext(2) - 1
        do i0 = 0, ext(1) - 1
          w = i0 + i1*stride(2) + i2*stride(3)
          do q = 0, wpe - 1
            m(w*wpe + q + 1) = int(modulo(modulo(modulo(2654435761_int64*w + 97*50*q, 2147483647_int64)*48271, 2147483647_int64), &
                                          11_int64)) + 1
          end do
        end do
      end do
    end do
    do w = 1, nwords
      u8(w) = bits8(m(w))
    end do
    call hipcheck(hipMemcpy(c_loc(cs_data), c_loc(u8), int(nwords*8, c_size_t), hipMemcpyHostToDevice), "H2D")

    do dim = first, last
      call check(cudecompGetShiftedRank(handle, cs_grid_desc, axis, dim, -1, cs_periods(dim), nb), "cudecompGetShiftedRank")
      wall(1) = nb == -1
      call check(cudecompGetShiftedRank(handle, cs_grid_desc, axis, dim, 1, cs_periods(dim), nb), "cudecompGetShiftedRank")
      wall(2) = nb == -1
      h = cs_halo(dim)
      do side = 1, 2
        named(side) = iand(cs_sides, side) /= 0
        if (refusal .and. (cs_sides < 1 .or. cs_sides > 3)) named(side) = .true.
        ! a side is written where it is named and the rank owns the domain's edge
        writes(side) = .not. refusal .and. named(side) .and. wall(side)
        ! a named side's array is present (unless the refusal asks for its absence), the other one is absent or garbage
        if (named(side)) then
          pres(side) = .not. named_null
        else
          pres(side) = garbage
        end if
      end do
      active = h > 0 .and. (writes(1) .or. writes(2))

      r = with_values(axis, dim, int(h), .not. nullpad, use_stream, pres(1), pres(2), named(1), named(2))
      if (r /= expected) then
        write (error_unit, '(a,i0,a,i0,a,i0)') "MISMATCH: the call along dim ", dim, " returned ", r, ", not ", expected
        nfail = nfail + 1
        if (r /= CUDECOMP_RESULT_SUCCESS) exit
      end if
      call hipcheck(hipDeviceSynchronize(), "sync")
      if (use_stream) call hipcheck(hipStreamSynchronize(my_stream), "stream sync")

      km = 1  ! the memory position of `dim`
      do k2 = 1, 3
        if (p%order(k2) == dim) km = k2
      end do
      ka = mod(km, 3) + 1
      kb = mod(km + 1, 3) + 1
      n = ext(km)
      cc = cs_centering
      before = m
      do side = 1, 2
        if (.not. writes(side) .or. h == 0) cycle
        do k = 0, h - 1
          if (side == 1) then
            ghost = h - 1 - k
            inner = h + k + cc
          else
            ghost = n - h + k
            inner = n - h - 1 - k - cc
          end if
          a_side = side
          if (swap) a_side = 3 - side
          a_k = int(k) + 1
          if (reverse) a_k = int(h - k)
          do ib = 0, ext(kb) - 1
            do ia = 0, ext(ka) - 1
              at = ia*stride(ka) + ib*stride(kb)
              do q = 0, wpe - 1
                gi = (at + ghost*stride(km))*wpe + q + 1
                ii = (at + inner*stride(km))*wpe + q + 1
                m(gi) = cs_parity*m(ii) + addend(a_side, a_k, dim, q)
              end do
            end do
          end do
        end do
      end do
      bad = 0
      shown = 0
      call hipcheck(hipMemcpy(c_loc(d8), c_loc(cs_data), int(nwords*8, c_size_t), hipMemcpyDeviceToHost), "D2H")
      do w = 1, nwords
        if (d8(w) /= bits8(m(w))) then
          bad = bad + 1
          if (shown < 4) write (error_unit, '(a,i0,a,i0,a,z16.16,a,z16.16)') "rank ", rank, ": word ", w, &
            " holds ", d8(w), ", the header says ", bits8(m(w))
          shown = shown + 1
        end if
      end do
      if (bad /= 0) then
        nfail = nfail + 1
        write (error_unit, '(a,i0,a,i0,a,i0)') "MISMATCH: ", bad, " words differ after the call along dim ", dim, " on rank ", rank
      end if
      if (active .and. all(m == before)) then
        nfail = nfail + 1
        write (error_unit, '(a,i0)') "MISMATCH: the definition changed nothing along dim ", dim
      end if
      if ((reverse .or. swap) .and. nfail /= 0) exit  ! the model has left the pencil: nothing more to learn
    end do
    if ((reverse .or. swap) .and. nfail == 0) write (error_unit, '(a)') "the altered expectation went unnoticed"

    call check(cudecompFree(handle, cs_grid_desc, cs_data), "cudecompFree data")
    call check(cudecompGridDescDestroy(handle, cs_grid_desc), "cudecompGridDescDestroy")

  end subroutine run_case

end program halo_wall_values_test
