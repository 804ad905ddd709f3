! halo_fold_test.f90 -- Fortran twin of tests/native/halo_fold_test.cpp: halo folding (cudecomp_halo_fold.h) through the generic
! wrappers cudecompAmdFoldHalos{X,Y,Z} of module `cudecomp`.  Per case and per dim 1, 2, 3 SEPARATELY: upload a fresh pencil, call
! the fold once along `dim` through the X, Y or Z wrapper of --ax, download, compare the whole buffer -- halos of all dims, padding,
! a poisoned tail -- bit for bit with the closed forms of the C++ twin (see there for the initial content and the rules).
! The same case lines in FORTRAN conventions (--ax, --dim and --mem_order one-based); data type from the executable's name.
!
!   the options of halo_test, plus
!   --parity +1|-1  --centering 0|1  --clear 0|1
!   --nullpad   `padding` absent (needs zero padding)       --stream   `stream` present: a stream this program created
!   --expect-refusal --dim D    one call along D (4 can be asked for): CUDECOMP_RESULT_INVALID_USAGE and an untouched pencil
!   --self-check-shift-dim      call along mod(dim, 3) + 1 while expecting dim: the case must FAIL
! At the end rank 0 prints one line "WRAPPER <name>" per wrapper that was called in a case that passed.
program halo_fold_test
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
  character(len=24), parameter :: WRAPPER_NAMES(3) = [character(len=24) :: &
    "cudecompAmdFoldHalosX", "cudecompAmdFoldHalosY", "cudecompAmdFoldHalosZ"]

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
  real(real32), pointer, contiguous :: cs_data(:)
  integer :: cs_halo(3), cs_pad(3), cs_parity, cs_centering, cs_clear
  logical :: cs_periods(3)

  rank = env_int("RANK", env_int("PMI_RANK", env_int("OMPI_COMM_WORLD_RANK", 0)))
  nranks = env_int("WORLD_SIZE", env_int("PMI_SIZE", env_int("OMPI_COMM_WORLD_SIZE", 1)))
  dtype_sel = dtype_from_program_name()
  select case (dtype_sel)
  case (1); dtype = CUDECOMP_FLOAT; es = 4; wpe = 1
  case (2); dtype = CUDECOMP_DOUBLE; es = 8; wpe = 1
  case (3); dtype = CUDECOMP_FLOAT_COMPLEX; es = 8; wpe = 2
  case default; dtype = CUDECOMP_DOUBLE_COMPLEX; es = 16; wpe = 2
  end select
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
    case (1); r = cudecompAmdFoldHalosX(handle, cs_grid_desc, cs_data, dtype, cs_parity, cs_centering, cs_clear, cs_halo, &
                                        cs_periods, dim, pad_o, stream_o)
    case (2); r = cudecompAmdFoldHalosY(handle, cs_grid_desc, cs_data, dtype, cs_parity, cs_centering, cs_clear, cs_halo, &
                                        cs_periods, dim, pad_o, stream_o)
    case (3); r = cudecompAmdFoldHalosZ(handle, cs_grid_desc, cs_data, dtype, cs_parity, cs_centering, cs_clear, cs_halo, &
                                        cs_periods, dim, pad_o, stream_o)
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

  ! the bits of one real component holding the small integer v
  integer(int32) function bits4(v)
    integer, intent(in) :: v
    bits4 = transfer(real(v, real32), 0_int32)
  end function bits4

  integer(int64) function bits8(v)
    integer, intent(in) :: v
    bits8 = transfer(real(v, real64), 0_int64)
  end function bits8

  subroutine run_case(cmd)
    character(len=*), intent(in) :: cmd
    type(cmdline) :: c
    type(cudecompGridDescConfig) :: config
    type(cudecompPencilInfo) :: p
    integer :: gd(3), gdd(3), pd(2), backend, axis, iper(3), mo(3), ac, rank_order, dim, ax2, s
    integer :: first, last, mdim, call_dim, kd, h, n, j, q, src, ce, l(3), g(3), hk, i0, i1, i2, shown
    logical :: nullpad, use_stream, refusal, shift, low, high, padding, ghost
    integer(int64) :: bad, idx, nwords, stride(3), w
    integer, allocatable :: iv(:), wv(:), gg(:)
    logical, allocatable :: cell(:)
    integer(int32), allocatable, target :: u4(:), d4(:)
    integer(int64), allocatable, target :: u8(:), d8(:)
    integer(int32) :: want4
    integer(int64) :: want8
    integer(c_int32_t) :: nb
    integer(c_int) :: r, expected
    character(len=8), parameter :: opname = "fold"

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
    cs_periods = (iper /= 0)
    mo = -1
    call opt_ints(c, "--mem_order", mo)
    cs_parity = opt_int(c, "--parity", 1)
    cs_centering = opt_int(c, "--centering", 0)
    cs_clear = opt_int(c, "--clear", 0)
    nullpad = find_opt(c, "--nullpad") /= 0
    use_stream = find_opt(c, "--stream") /= 0
    refusal = find_opt(c, "--expect-refusal") /= 0
    shift = find_opt(c, "--self-check-shift-dim") /= 0
    if (axis < 1 .or. axis > 3 .or. backend == 0 .or. (nullpad .and. any(cs_pad /= 0))) then
      write (error_unit, '(a)') "bad case line: --ax 1..3, --backend required, --nullpad needs zero padding"
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
    call check(cudecompMalloc(handle, cs_grid_desc, cs_data, (p%size + TAIL)*es/4), "cudecompMalloc data")

    nwords = (p%size + TAIL)*wpe
    allocate (iv(nwords), wv(nwords), gg(nwords), cell(p%size))
    if (es/wpe == 4) then
      allocate (u4(nwords), d4(nwords))
    else
      allocate (u8(nwords), d8(nwords))
    end if
    stride = [1_int64, int(p%shape(1), int64), int(p%shape(1), int64)*p%shape(2)]

    first = 1
    last = 3
    if (refusal) then
      first = opt_int(c, "--dim", 1)
      last = first
    end if
    do dim = first, last
      mdim = dim
      if (dim < 1 .or. dim > 3) mdim = 1  ! (a refused dim: any initial content will do)
      call check(cudecompGetShiftedRank(handle, cs_grid_desc, axis, mdim, -1, cs_periods(mdim), nb), "cudecompGetShiftedRank")
      low = nb /= -1
      call check(cudecompGetShiftedRank(handle, cs_grid_desc, axis, mdim, 1, cs_periods(mdim), nb), "cudecompGetShiftedRank")
      high = nb /= -1
      do kd = 1, 3
        if (p%order(kd) == mdim) exit
      end do
      h = cs_halo(mdim)
      n = (p%hi(kd) - p%lo(kd) + 1) + 2*h  ! the extent along dim without padding

      ! what is uploaded: G + 8 in the ghost cells along dim, -77 in padding and tail
      iv = POISON
      gg = 0
      cell = .false.
      idx = 0
      do i2 = 1, p%shape(3)
        do i1 = 1, p%shape(2)
          do i0 = 1, p%shape(1)
            idx = idx + 1
            l = [i0, i1, i2]
            padding = .false.
            do k = 1, 3
              ax2 = p%order(k)
              hk = cs_halo(ax2)
              if (l(k) > (p%hi(k) - p%lo(k) + 1) + 2*hk) padding = .true.
              g(ax2) = modulo((p%lo(k) - 1) + (l(k) - 1 - hk), gd(ax2))  ! zero-based, wrapped
            end do
            if (padding) cycle
            cell(idx) = .true.
            j = l(kd) - 1
            ghost = j < h .or. j >= n - h
            gg((idx - 1)*wpe + 1) = modulo(g(1) + 3*g(2) + 5*g(3), 7)
            if (wpe == 2) gg(idx*wpe) = modulo(2*g(1) + g(2) + 3*g(3), 7)
            do q = 1, wpe
              iv((idx - 1)*wpe + q) = gg((idx - 1)*wpe + q) + merge(BUMP, 0, ghost)
            end do
          end do
        end do
      end do
      ! what the header says one fold along dim leaves
      wv = iv
      s = merge(-1, 1, cs_parity == -1)
      ce = cs_centering
      if (.not. refusal .and. h > 0) then
        idx = 0
        do i2 = 1, p%shape(3)
          do i1 = 1, p%shape(2)
            do i0 = 1, p%shape(1)
              idx = idx + 1
              if (.not. cell(idx)) cycle
              l = [i0, i1, i2]
              j = l(kd) - 1
              ! low side: cell(h + k + c) += s * cell(h - 1 - k); high side: cell(n - h - 1 - k - c) += s * cell(n - h + k)
              if (.not. low .and. j >= h + ce .and. j < 2*h + ce) then
                src = h - 1 - (j - h - ce)
                do q = 1, wpe
                  wv((idx - 1)*wpe + q) = wv((idx - 1)*wpe + q) + s*iv((idx - 1 + (src - j)*stride(kd))*wpe + q)
                end do
              end if
              if (.not. high .and. j >= n - 2*h - ce .and. j < n - h - ce) then
                src = n - h + (n - h - 1 - ce - j)
                do q = 1, wpe
                  wv((idx - 1)*wpe + q) = wv((idx - 1)*wpe + q) + s*iv((idx - 1 + (src - j)*stride(kd))*wpe + q)
                end do
              end if
              if (cs_clear /= 0 .and. ((.not. low .and. j < h) .or. (.not. high .and. j >= n - h))) then
                do q = 1, wpe
                  wv((idx - 1)*wpe + q) = 0
                end do
              end if
            end do
          end do
        end do
      end if

      if (es/wpe == 4) then
        do w = 1, nwords
          u4(w) = bits4(iv(w))
        end do
        call hipcheck(hipMemcpy(c_loc(cs_data), c_loc(u4), int(nwords*4, c_size_t), hipMemcpyHostToDevice), "H2D")
      else
        do w = 1, nwords
          u8(w) = bits8(iv(w))
        end do
        call hipcheck(hipMemcpy(c_loc(cs_data), c_loc(u8), int(nwords*8, c_size_t), hipMemcpyHostToDevice), "H2D")
      end if

      call_dim = dim
      if (shift) call_dim = mod(dim, 3) + 1
      r = with_forms(axis, call_dim, .not. nullpad, use_stream)
      expected = CUDECOMP_RESULT_SUCCESS
      if (refusal) expected = CUDECOMP_RESULT_INVALID_USAGE
      if (r /= expected) then
        write (error_unit, '(a,a,a,i0,a,i0,a,i0)') "MISMATCH: ", trim(opname), " along dim ", call_dim, " returned ", r, &
          ", expected ", expected
        nfail = nfail + 1
        if (r /= CUDECOMP_RESULT_SUCCESS .and. .not. refusal) exit
      end if
      call hipcheck(hipDeviceSynchronize(), "sync")

      bad = 0
      shown = 0
      if (es/wpe == 4) then
        call hipcheck(hipMemcpy(c_loc(d4), c_loc(cs_data), int(nwords*4, c_size_t), hipMemcpyDeviceToHost), "D2H")
        do w = 1, nwords
          want4 = bits4(wv(w))
          if (d4(w) /= want4) then
            bad = bad + 1
            if (shown < 4) write (error_unit, '(a,i0,a,i0,a,z8.8,a,z8.8,a,z8.8)') "rank ", rank, ": word ", w, " holds ", d4(w), &
              ", expected ", want4, ", uploaded ", u4(w)
            shown = shown + 1
          end if
        end do
      else
        call hipcheck(hipMemcpy(c_loc(d8), c_loc(cs_data), int(nwords*8, c_size_t), hipMemcpyDeviceToHost), "D2H")
        do w = 1, nwords
          want8 = bits8(wv(w))
          if (d8(w) /= want8) then
            bad = bad + 1
            if (shown < 4) write (error_unit, '(a,i0,a,i0,a,z16.16,a,z16.16,a,z16.16)') "rank ", rank, ": word ", w, " holds ", &
              d8(w), ", expected ", want8, ", uploaded ", u8(w)
            shown = shown + 1
          end if
        end do
      end if
      if (bad /= 0) then
        nfail = nfail + 1
        write (error_unit, '(a,i0,a,a,a,i0,a,i0)') "MISMATCH: ", bad, " words differ after ", trim(opname), " along dim ", dim, &
          " on rank ", rank
      end if
    end do

    call check(cudecompFree(handle, cs_grid_desc, cs_data), "cudecompFree data")
    call check(cudecompGridDescDestroy(handle, cs_grid_desc), "cudecompGridDescDestroy")
  end subroutine run_case

end program halo_fold_test
