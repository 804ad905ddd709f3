! halo_wall_fields_test.f90 -- Fortran twin of tests/native/halo_wall_fields_test.cpp: multi-field wall halos
! (cudecomp_halo_wall_fields.h) through the wrappers cudecompAmdReflectFieldHalos{X,Y,Z} and cudecompAmdFoldFieldHalos{X,Y,Z} of module
! `cudecomp`, fp64.  Per case: one pencil per entry of --parities (slices of one buffer from cudecompMalloc, their addresses passed
! as an array of type(c_ptr)) is uploaded; --op reflect runs the field reflection along dims 1, 2, 3 in turn, --op fold the field fold
! (--clear 0 / 1) along dims 3, 2, 1, through the X, Y or Z wrapper of --ax; after every dim every field is downloaded and the whole
! buffer -- halos of all dims, padding, a poisoned tail -- compared bit for bit with the header's formulas applied on the host to the
! whole pencil: on the sides where cudecompGetShiftedRank names no neighbour, for k in [0, h) and c = --centering (zero-based cells),
! the reflection sets cell(h-1-k) = s cell(h+k+c) and cell(n-h+k) = s cell(n-h-1-k-c); the fold adds cell(h+k+c) += s cell(h-1-k),
! then cell(n-h-1-k-c) += s cell(n-h+k), and with --clear 1 leaves zero in the ghost cells it has read; s = the field's parity.  A dim
! along which the rank has a wall and a halo must have changed every field.  Payload: the twin's payload(e, f) in cell e (zero-based)
! of field f (zero-based): 1 .. 11 without a pattern along any stride and without a zero, so that a flipped sign always shows; -77 in
! padding and tail.
! The same case lines in FORTRAN conventions (--ax and --mem_order one-based).
!
!   the options of halo_test, plus
!   --op reflect | fold        --parities P1 P2 ...  one +1 / -1 per field (1 .. 32): the number of fields is their number
!   --centering C  0 / 1       --clear C   0 / 1 (fold)
!   --nullpad   `padding` absent (needs zero padding)       --stream   `stream` present: a stream this program created
!   --self-check-shift-dim      call along mod(dim, 3) + 1 while expecting dim: the case must FAIL
! At the end rank 0 prints one line "WRAPPER <name>" per wrapper that was called in a case that passed.
program halo_wall_fields_test
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
  character(len=32), parameter :: WRAPPER_NAMES(6) = [character(len=32) :: &
    "cudecompAmdReflectFieldHalosX", "cudecompAmdReflectFieldHalosY", "cudecompAmdReflectFieldHalosZ", &
    "cudecompAmdFoldFieldHalosX", "cudecompAmdFoldFieldHalosY", "cudecompAmdFoldFieldHalosZ"]

  type(cudecompHandle) :: handle
  integer :: rank, nranks, ndev, dtype_sel, dtype, wpe, i, ncases, res, nfailed, u, stat, argn, k
  integer(int64) :: es
  character(len=1024) :: line, arg, testfile, progname
  character(len=1024), allocatable :: cases(:)
  logical :: from_file
  integer :: c0, c1, rate
  logical :: called(6), called_in_case(6)
  integer(cudecomp_stream_kind) :: my_stream
  logical :: have_stream

  ! the case the wrappers are called for (call_wrapper and its callers are internal procedures of the program)
  type(cudecompGridDesc) :: cs_grid_desc
  real(real32), pointer, contiguous :: cs_data(:)
  type(c_ptr) :: cs_fields(32)
  integer :: cs_halo(3), cs_pad(3), cs_nf, cs_clear, cs_centering, cs_par(32)
  logical :: cs_fold
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
    do k = 1, 6
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

  ! one of the six wrappers; absent optional arguments stay absent all the way down
  function call_wrapper(axis, dim, pad_o, stream_o) result(r)
    integer, intent(in) :: axis, dim
    integer, optional :: pad_o(3)
    integer(cudecomp_stream_kind), optional :: stream_o
    integer(c_int) :: r
    r = -1
    if (cs_fold) then
      called_in_case(3 + axis) = .true.
      select case (axis)
      case (1); r = cudecompAmdFoldFieldHalosX(handle, cs_grid_desc, cs_fields(1:cs_nf), cs_nf, dtype, cs_par(1:cs_nf), cs_centering, &
                                               cs_clear, cs_halo, cs_periods, dim, pad_o, stream_o)
      case (2); r = cudecompAmdFoldFieldHalosY(handle, cs_grid_desc, cs_fields(1:cs_nf), cs_nf, dtype, cs_par(1:cs_nf), cs_centering, &
                                               cs_clear, cs_halo, cs_periods, dim, pad_o, stream_o)
      case (3); r = cudecompAmdFoldFieldHalosZ(handle, cs_grid_desc, cs_fields(1:cs_nf), cs_nf, dtype, cs_par(1:cs_nf), cs_centering, &
                                               cs_clear, cs_halo, cs_periods, dim, pad_o, stream_o)
      end select
    else
      called_in_case(axis) = .true.
      select case (axis)
      case (1); r = cudecompAmdReflectFieldHalosX(handle, cs_grid_desc, cs_fields(1:cs_nf), cs_nf, dtype, cs_par(1:cs_nf), cs_centering, &
                                                  cs_halo, cs_periods, dim, pad_o, stream_o)
      case (2); r = cudecompAmdReflectFieldHalosY(handle, cs_grid_desc, cs_fields(1:cs_nf), cs_nf, dtype, cs_par(1:cs_nf), cs_centering, &
                                                  cs_halo, cs_periods, dim, pad_o, stream_o)
      case (3); r = cudecompAmdReflectFieldHalosZ(handle, cs_grid_desc, cs_fields(1:cs_nf), cs_nf, dtype, cs_par(1:cs_nf), cs_centering, &
                                                  cs_halo, cs_periods, dim, pad_o, stream_o)
      end select
    end if
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

  subroutine run_case(cmd)
    character(len=*), intent(in) :: cmd
    type(cmdline) :: c
    type(cudecompGridDescConfig) :: config
    type(cudecompPencilInfo) :: p
    integer :: gd(3), gdd(3), pd(2), backend, axis, iper(3), mo(3), ac, rank_order, dim, ax2, f, step, side
    integer :: call_dim, k2, km, ka, kb, shown, iop
    logical :: nullpad, use_stream, shift, wall(2), active, bad_line
    integer(int64) :: bad, nwords, w, fw, ext(3), stride(3), i0, i1, i2, h, n, cc, k, ghost, inner, ia, ib, at, gi, ii
    integer, allocatable :: m(:, :), before(:)
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
    cs_centering = opt_int(c, "--centering", 0)
    cs_clear = opt_int(c, "--clear", 0)
    cs_par = 0
    call opt_ints(c, "--parities", cs_par)
    cs_nf = count(cs_par /= 0)
    bad_line = cs_nf < 1 .or. any(abs(cs_par(1:max(cs_nf, 1))) /= 1)
    iop = find_opt(c, "--op")
    cs_fold = .false.
    if (iop == 0 .or. iop >= c%n) then
      bad_line = .true.
    else if (trim(c%tok(iop + 1)) == "fold") then
      cs_fold = .true.
    else if (trim(c%tok(iop + 1)) /= "reflect") then
      bad_line = .true.
    end if
    cs_periods = (iper /= 0)
    mo = -1
    call opt_ints(c, "--mem_order", mo)
    nullpad = find_opt(c, "--nullpad") /= 0
    use_stream = find_opt(c, "--stream") /= 0
    shift = find_opt(c, "--self-check-shift-dim") /= 0
    if (bad_line .or. axis < 1 .or. axis > 3 .or. backend == 0 .or. (nullpad .and. any(cs_pad /= 0)) .or. cs_centering < 0 .or. &
        cs_centering > 1 .or. cs_clear < 0 .or. cs_clear > 1) then
      write (error_unit, '(a)') "bad case line: --op reflect | fold, --parities of +1 / -1, --ax 1..3, --backend required, "// &
        "--nullpad needs zero padding, --centering and --clear 0 / 1"
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
    do f = 1, cs_nf
      cs_fields(f) = c_loc(cs_data((f - 1)*fw + 1))
    end do

    ! the pencil's own cells: extent without padding and stride of every memory position
    do k2 = 1, 3
      ext(k2) = (p%hi(k2) - p%lo(k2) + 1) + 2*cs_halo(p%order(k2))
    end do
    stride(1) = 1
    stride(2) = p%shape(1)
    stride(3) = int(p%shape(1), int64)*p%shape(2)
    allocate (m(nwords, cs_nf), before(nwords), u8(nwords), d8(nwords))
    m = POISON
    do f = 1, cs_nf
      do i2 = 0, ext(3) - 1
        do i1 = 0, ext(2) - 1
          do i0 = 0, ext(1) - 1
            w = i0 + i1*stride(2) + i2*stride(3)
            m(w + 1, f) = int(modulo(modulo(modulo(2654435761_int64*w + 97*(f - 1), 2147483647_int64)*48271, 2147483647_int64), &
                                     11_int64)) + 1
          end do
        end do
      end do
      do w = 1, nwords
        u8(w) = bits8(m(w, f))
      end do
      call hipcheck(hipMemcpy(cs_fields(f), c_loc(u8), int(nwords*8, c_size_t), hipMemcpyHostToDevice), "H2D")
    end do

    do step = 1, 3
      dim = step
      if (cs_fold) dim = 4 - step
      call check(cudecompGetShiftedRank(handle, cs_grid_desc, axis, dim, -1, cs_periods(dim), nb), "cudecompGetShiftedRank")
      wall(1) = nb == -1
      call check(cudecompGetShiftedRank(handle, cs_grid_desc, axis, dim, 1, cs_periods(dim), nb), "cudecompGetShiftedRank")
      wall(2) = nb == -1
      active = cs_halo(dim) > 0 .and. (wall(1) .or. wall(2))

      call_dim = dim
      if (shift) call_dim = mod(dim, 3) + 1
      r = with_forms(axis, call_dim, .not. nullpad, use_stream)
      if (r /= CUDECOMP_RESULT_SUCCESS) then
        write (error_unit, '(a,i0,a,i0)') "MISMATCH: the call along dim ", call_dim, " returned ", r
        nfail = nfail + 1
        exit
      end if
      call hipcheck(hipDeviceSynchronize(), "sync")
      if (use_stream) call hipcheck(hipStreamSynchronize(my_stream), "stream sync")

      km = 1  ! the memory position of `dim`
      do k2 = 1, 3
        if (p%order(k2) == dim) km = k2
      end do
      ka = mod(km, 3) + 1
      kb = mod(km + 1, 3) + 1
      h = cs_halo(dim)
      n = ext(km)
      cc = cs_centering
      do f = 1, cs_nf
        before = m(:, f)
        do side = 1, 2
          if (.not. wall(side) .or. h == 0) cycle
          do k = 0, h - 1
            if (side == 1) then
              ghost = h - 1 - k
              inner = h + k + cc
            else
              ghost = n - h + k
              inner = n - h - 1 - k - cc
            end if
            do ib = 0, ext(kb) - 1
              do ia = 0, ext(ka) - 1
                at = ia*stride(ka) + ib*stride(kb)
                gi = at + ghost*stride(km) + 1
                ii = at + inner*stride(km) + 1
                if (cs_fold) then
                  m(ii, f) = m(ii, f) + cs_par(f)*m(gi, f)
                  if (cs_clear /= 0) m(gi, f) = 0
                else
                  m(gi, f) = cs_par(f)*m(ii, f)
                end if
              end do
            end do
          end do
        end do
        bad = 0
        shown = 0
        call hipcheck(hipMemcpy(c_loc(d8), cs_fields(f), int(nwords*8, c_size_t), hipMemcpyDeviceToHost), "D2H")
        do w = 1, nwords
          if (d8(w) /= bits8(m(w, f))) then
            bad = bad + 1
            if (shown < 4) write (error_unit, '(a,i0,a,i0,a,i0,a,z16.16,a,z16.16)') "rank ", rank, ": field ", f, " word ", w, &
              " holds ", d8(w), ", the header says ", bits8(m(w, f))
            shown = shown + 1
          end if
        end do
        if (bad /= 0) then
          nfail = nfail + 1
          write (error_unit, '(a,i0,a,i0,a,i0,a,i0)') "MISMATCH: ", bad, " words of field ", f, " differ after the call along dim ", &
            dim, " on rank ", rank
        end if
        if (active .and. all(m(:, f) == before)) then
          nfail = nfail + 1
          write (error_unit, '(a,i0,a,i0)') "MISMATCH: the formulas changed nothing of field ", f, " along dim ", dim
        end if
      end do
      if (shift) exit
    end do

    call check(cudecompFree(handle, cs_grid_desc, cs_data), "cudecompFree data")
    call check(cudecompGridDescDestroy(handle, cs_grid_desc), "cudecompGridDescDestroy")

  end subroutine run_case

end program halo_wall_fields_test
