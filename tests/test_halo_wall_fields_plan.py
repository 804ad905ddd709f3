"""Multi-field wall halos (cudecomp_halo_wall_fields.h: cudecompAmdReflectFieldHalos{X,Y,Z}, cudecompAmdFoldFieldHalos{X,Y,Z})
without a GPU: the C interface (symbols, prototypes against the ctypes argtypes), every refusal through the C ABI in its order of
precedence and against the single calls, calls with nothing to write, and the launch description of the mirrored field-move
kernels (cudecompExtDescribeMirroredFieldMoves) for the moves of the single plans over a sweep of geometries."""
import ctypes as C
import itertools
import os
import re
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
import cudecomp_amd as cd  # noqa: E402

HEADER = "cudecomp_halo_wall_fields.h"
REFLECT = ["cudecompAmdReflectFieldHalos" + a for a in "XYZ"]
FOLD = ["cudecompAmdFoldFieldHalos" + a for a in "XYZ"]
EXT = ["cudecompExtRunMirroredFieldMoves", "cudecompExtDescribeMirroredFieldMoves", "cudecompExtHaloPlanCount"]
ARITH = {cd.HALF: "_Float16", cd.HALF_COMPLEX: "_Float16", cd.BFLOAT16: "__bf16", cd.FLOAT: "float", cd.FLOAT_COMPLEX: "float",
         cd.DOUBLE: "double", cd.DOUBLE_COMPLEX: "double"}
ES = {cd.HALF: 2, cd.BFLOAT16: 2, cd.HALF_COMPLEX: 4, cd.FLOAT: 4, cd.FLOAT_COMPLEX: 8, cd.DOUBLE: 8, cd.DOUBLE_COMPLEX: 16}
NC = {cd.HALF: 1, cd.BFLOAT16: 1, cd.HALF_COMPLEX: 2, cd.FLOAT: 1, cd.FLOAT_COMPLEX: 2, cd.DOUBLE: 1, cd.DOUBLE_COMPLEX: 2}
MODES = (cd.MIRROR_REFLECT, cd.MIRROR_FOLD, cd.MIRROR_FOLD_TAKE)
KINDS = {cd.MIRROR_REFLECT: (31, 32), cd.MIRROR_FOLD: (33, 34), cd.MIRROR_FOLD_TAKE: (35, 36)}  # (rows, element-wise)


def spell(d, es, dtype):
    """the template spelling of what cudecompExtDescribeMirroredFieldMoves answers (csrc/kernels.cc spellKernelName)"""
    k = d["kind"]
    if k == 31:
        return "rows_fields_reflect_kernel<%d,%d>" % (d["vec"], d["access"])
    if k == 32:
        return "generic_fields_reflect_kernel<%d>" % es
    if k in (33, 35):
        return "rows_fields_fold_kernel<%s,%d,%d,%s>" % (ARITH[dtype], d["vec"], d["access"], "true" if k == 35 else "false")
    assert k in (34, 36), d
    return "generic_fields_fold_kernel<%s,%d,%s>" % (ARITH[dtype], NC[dtype], "true" if k == 36 else "false")


# ---- ABI ---------------------------------------------------------------------------------------------------------------------
def _prototypes(header):
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", header)).read(), flags=re.S)
    return {name: [" ".join(a.split()) for a in args.split(",")]
            for name, args in re.findall(r"cudecompResult_t\s+(cudecomp\w+)\s*\(([^)]*)\)\s*;", src)}


def test_the_six_symbols_are_declared_and_exported():
    assert cd.AMD_REFLECT_FIELDS_SYMBOLS == REFLECT and cd.AMD_FOLD_FIELDS_SYMBOLS == FOLD and cd.MAX_HALO_WALL_FIELDS == 32
    assert cd.AMD_WALL_FIELDS_SYMBOLS == REFLECT + FOLD
    assert sorted(_prototypes(HEADER)) == sorted(REFLECT + FOLD)
    L = cd.lib()
    for name in REFLECT + FOLD + EXT:
        assert hasattr(L, name), name
    assert set(EXT) <= set(cd.EXT_SYMBOLS) & set(_prototypes("cudecomp_ext.h"))
    text = open(os.path.join(ROOT, "include", HEADER)).read()
    assert '#include "cudecomp.h"' in text and re.search(r"#define\s+CUDECOMP_AMD_MAX_HALO_WALL_FIELDS\s+32\b", text)
    assert not HEADER.startswith("cudecomp_amd") and HEADER not in cd.AMD_HEADER_SYMBOLS


def test_prototypes_agree_with_the_argtypes():
    """the single calls' prototypes with (inputs, n_fields) in the place of `input` and `parities` in the place of `parity`: as many
    parameters as argtypes, pointers at the same positions, everything else a 32-bit integer on both sides"""
    L = cd.lib()
    opaque = ("cudecompHandle_t", "cudecompGridDesc_t", "hipStream_t")
    protos = _prototypes(HEADER)
    singles = dict(_prototypes("cudecomp_amd_reflect.h"), **_prototypes("cudecomp_halo_fold.h"))
    for name in REFLECT + FOLD:
        params, argtypes = protos[name], getattr(L, name).argtypes
        assert len(params) == len(argtypes) == (12 if name in REFLECT else 13), (name, params)
        in_header = ["*" in p or "[" in p or p.split()[0] in opaque for p in params]
        in_python = [t is C.c_void_p or t is C.c_char_p or hasattr(t, "contents") for t in argtypes]
        assert in_header == in_python, (name, params, argtypes)
        assert all(p.split()[0] in ("int32_t", "cudecompDataType_t") for p, ptr in zip(params, in_header) if not ptr), (name, params)
        assert all(t is C.c_int32 for t, ptr in zip(argtypes, in_python) if not ptr), (name, argtypes)
        single = singles[name.replace("FieldHalos", "Halos")]
        assert params[2:4] == ["void* const inputs[]", "int32_t n_fields"] and single[2] == "void* input"
        assert params[5] == "const int32_t parities[]" and single[4] == "int32_t parity"
        assert params[:2] + params[4:5] + params[6:] == single[:2] + single[3:4] + single[5:]
    ext = _prototypes("cudecomp_ext.h")
    for name in EXT:
        assert len(getattr(L, name).argtypes) == len(ext[name]), name


@pytest.mark.parametrize("language", ["c11", "c++17"])
def test_header_compiles(language):
    """alone, and before and after the other extension headers, -Wall -Wextra -Werror"""
    cc = "gcc" if language == "c11" else "g++"
    if shutil.which(cc) is None:
        pytest.skip("no " + cc)
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    base = [cc, "-std=" + language, "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-D__HIP_PLATFORM_AMD__",
            "-I" + os.path.join(ROOT, "include"), "-isystem", os.path.join(rocm, "include"), "-x", "c" if language == "c11" else "c++", "-"]
    others = ["cudecomp_amd.h", "cudecomp_amd_fill.h", "cudecomp_amd_reflect.h", "cudecomp_halo_fold.h", "cudecomp_halo_fields.h",
              "cudecomp_transpose_fields.h", "cudecomp_halo_accumulate_fields.h"]
    uses = ("int main(void) {\n  void* f[1] = {0};\n  const int32_t par[1] = {1}, h[3] = {0, 0, 0};\n"
            "  return (int)cudecompAmdReflectFieldHalosX(0, 0, f, 1, CUDECOMP_DOUBLE, par, 0, h, 0, 0, 0, 0) +\n"
            "         (int)cudecompAmdFoldFieldHalosZ(0, 0, f, 1, CUDECOMP_DOUBLE, par, 0, 1, h, 0, 0, 0, 0) + "
            "(CUDECOMP_AMD_MAX_HALO_WALL_FIELDS != 32);\n}\n")
    for order in ([HEADER], [HEADER] + others, others + [HEADER]):
        res = subprocess.run(base, input="".join('#include "%s"\n' % h for h in order) + uses, capture_output=True, text=True)
        assert res.returncode == 0 and not res.stderr.strip(), (order, res.stderr[-3000:])


# ---- refusals through the C ABI ------------------------------------------------------------------------------------------------
GDIMS = (12, 10, 8)


@pytest.fixture(scope="module")
def descriptor():
    h = cd.cudecompInit()
    gd = cd.cudecompGridDescCreate(h, cd.make_config(GDIMS, (1, 1)))
    yield h, gd
    cd.cudecompGridDescDestroy(h, gd)
    cd.cudecompFinalize(h)


def _call(h, gd, op, axis, ptrs, n, parities, halo=(1, 1, 1), dim=0, centering=0, clear=0, periods=(False, False, False), dtype=cd.DOUBLE):
    fn = getattr(cd.lib(), (REFLECT if op == "reflect" else FOLD)[axis])
    arr = None if ptrs is None else (C.c_void_p * max(1, len(ptrs)))(*ptrs)
    par = None if parities is None else (C.c_int32 * max(1, len(parities)))(*parities)
    hh = None if halo is None else (C.c_int32 * 3)(*halo)
    more = (clear,) if op == "fold" else ()
    return fn(h, gd, arr, n, dtype, par, centering, *more, hh, (C.c_bool * 3)(*periods), dim, None, None)


def _single(h, gd, op, axis, ptr, parity, halo=(1, 1, 1), dim=0, centering=0, clear=0, periods=(False, False, False), dtype=cd.DOUBLE):
    fn = getattr(cd.lib(), ("cudecompAmdReflectHalos" if op == "reflect" else "cudecompAmdFoldHalos") + "XYZ"[axis])
    hh = None if halo is None else (C.c_int32 * 3)(*halo)
    more = (clear,) if op == "fold" else ()
    return fn(h, gd, ptr, dtype, parity, centering, *more, hh, (C.c_bool * 3)(*periods), dim, None, None)


def _message(capfd):
    err = capfd.readouterr().err
    found = re.findall(r"CUDECOMP:ERROR: .*\((.*)\)", err)
    return found[-1] if found else err


@pytest.mark.parametrize("op", ["reflect", "fold"])
def test_refusals(descriptor, capfd, op):
    """all found on the host, before anything is launched (the pointers are not device memory, and there is no device here):
    INVALID_USAGE with the single calls' message format"""
    h, gd = descriptor
    fake = [0x10000 * (i + 1) for i in range(33)]
    ones = [1] * 33
    cases = [("inputs argument cannot be null", None, 3, ones), ("n_fields argument out of range", fake[:3], 0, ones),
             ("n_fields argument out of range", fake[:3], -1, ones), ("n_fields argument out of range", fake, 33, ones),
             ("inputs argument cannot hold a null entry", [fake[0], None, fake[2]], 3, ones),
             ("inputs argument cannot hold the same field twice", [fake[0], fake[1], fake[0]], 3, ones),
             ("parities argument cannot be null", fake[:3], 3, None),
             ("parity argument must be +1 or -1", fake[:3], 3, [1, 0, -1]),
             ("parity argument must be +1 or -1", fake[:3], 3, [1, -1, 2]),
             ("parity argument must be +1 or -1", fake[:1], 1, [3]),
             ("parity argument must be +1 or -1", fake[:32], 32, [-1] * 31 + [-2])]
    capfd.readouterr()
    for axis in range(3):
        for message, ptrs, n, parities in cases:
            assert _call(h, gd, op, axis, ptrs, n, parities) == cd.RESULT_INVALID_USAGE, (axis, message)
            assert _message(capfd) == message, (axis, message)
        # the single call says the same kind of thing about its `input` and the same thing about its `parity`
        assert _single(h, gd, op, axis, None, 1) == cd.RESULT_INVALID_USAGE and _message(capfd) == "input argument cannot be null"
        assert _single(h, gd, op, axis, fake[0], 0) == cd.RESULT_INVALID_USAGE and _message(capfd) == "parity argument must be +1 or -1"
        # precedence: halo_extents, then the list, then parities == NULL, then dim, then what the fill refuses, then the parities,
        # centering, clear, then the mirror that reaches beyond the interior
        assert _call(h, gd, op, axis, None, 0, None, halo=None, dim=7, centering=5, clear=5) == cd.RESULT_INVALID_USAGE
        assert _message(capfd) == "halo_extents argument cannot be null"
        assert _call(h, gd, op, axis, None, 0, None, dim=7, centering=5, clear=5) == cd.RESULT_INVALID_USAGE
        assert _message(capfd) == "inputs argument cannot be null"
        assert _call(h, gd, op, axis, fake[:3], 3, None, dim=7, centering=5, clear=5) == cd.RESULT_INVALID_USAGE
        assert _message(capfd) == "parities argument cannot be null"
        assert _call(h, gd, op, axis, fake[:3], 3, [1, 5, 1], dim=7, centering=5, clear=5) == cd.RESULT_INVALID_USAGE
        assert _message(capfd) == "dim argument out of range"
        wide = [1, 1, 1]
        wide[(axis + 1) % 3] = 40  # (wider than the pencil)
        for n in (1, 3):
            rc = _call(h, gd, op, axis, fake[:n], n, [5] * n, halo=wide, dim=(axis + 1) % 3, centering=5, clear=5, periods=(True, True, True))
            message = _message(capfd)
            assert rc == _single(h, gd, op, axis, fake[0], 5, halo=wide, dim=(axis + 1) % 3, centering=5, clear=5, periods=(True, True, True)) != cd.RESULT_SUCCESS
            assert message == _message(capfd), message  # (whichever of its checks the single call reaches first)
            assert _call(h, gd, op, axis, fake[:n], n, [1] * (n - 1) + [5], centering=5, clear=5) == cd.RESULT_INVALID_USAGE
            assert _message(capfd) == "parity argument must be +1 or -1"
            assert _call(h, gd, op, axis, fake[:n], n, [-1] * n, centering=5, clear=5) == cd.RESULT_INVALID_USAGE
            assert _message(capfd) == "centering argument must be 0 or 1"
            assert _call(h, gd, op, axis, fake[:n], n, [-1] * n, centering=-1) == cd.RESULT_INVALID_USAGE
            assert _message(capfd) == "centering argument must be 0 or 1"
            if op == "fold":
                for clear in (2, -1, 256):
                    assert _call(h, gd, op, axis, fake[:n], n, [-1] * n, centering=1, clear=clear) == cd.RESULT_INVALID_USAGE
                    assert _message(capfd) == "clear argument must be 0 or 1"
            # h + centering > n - 2h on a side that would be written: dim 2 has 8 interior cells, so h = 8 with centering 1 and h = 9
            # are refused, with the single call's message.  (The tuples that fit are shown below on the stateless planners: through
            # the C ABI they would go on to the device and launch on these made-up pointers.)
            for hz, c in ((8, 1), (9, 0)):
                rc = _call(h, gd, op, axis, fake[:n], n, [-1] * n, halo=(0, 0, hz), dim=2, centering=c, periods=(True, True, False))
                message = _message(capfd)
                want = _single(h, gd, op, axis, fake[0], -1, halo=(0, 0, hz), dim=2, centering=c, periods=(True, True, False))
                assert rc == want == cd.RESULT_INVALID_USAGE and message == _message(capfd) and "reaches beyond the interior" in message
                # ... and not where nothing would be written
                assert _call(h, gd, op, axis, fake[:n], n, [-1] * n, halo=(0, 0, hz), dim=2, centering=c, periods=(True, True, True)) == \
                    cd.RESULT_SUCCESS
                assert capfd.readouterr().err == ""
        # the same bound on the plans the field calls are derived from, without a device or a launch: what fits is planned with both
        # sides, what does not is refused
        spec = cd.make_grid_spec(GDIMS, (1, 1), ((0, 1, 2),) * 3)
        for hz, c, fine in ((4, 1, True), (8, 0, True), (8, 1, False), (9, 0, False)):
            def plan():
                if op == "reflect":
                    return cd.cudecompExtPlanHaloReflect(spec, 0, axis, (0, 0, hz), (1, 1, 0), 2, None, c, False)
                return cd.cudecompExtPlanHaloFold(spec, 0, axis, (0, 0, hz), (1, 1, 0), 2, None, c, False, 1)
            if fine:
                assert plan().n_pre == 2
            else:
                with pytest.raises(cd.CudecompError) as info:
                    plan()
                assert info.value.code == cd.RESULT_INVALID_USAGE and "reaches beyond the interior" in _message(capfd)


@pytest.mark.parametrize("op", ["reflect", "fold"])
def test_nothing_to_write_succeeds_without_a_device(descriptor, capfd, op):
    h, gd = descriptor
    fake = [0x10000 * (i + 1) for i in range(32)]
    capfd.readouterr()
    for axis, n, clear in itertools.product(range(3), (1, 2, 32), (0, 1)):
        par = [(-1) ** f for f in range(n)]
        # every halo zero: the lists of fields are not looked at; the parities, centering and clear are
        assert _call(h, gd, op, axis, None, n, par, halo=(0, 0, 0), dim=9, clear=clear) == cd.RESULT_SUCCESS
        assert _call(h, gd, op, axis, None, n, None, halo=(0, 0, 0)) == cd.RESULT_INVALID_USAGE
        assert _message(capfd) == "parities argument cannot be null"
        assert _call(h, gd, op, axis, None, 33, [1] * 33, halo=(0, 0, 0)) == cd.RESULT_INVALID_USAGE
        assert _message(capfd) == "n_fields argument out of range"
        assert _call(h, gd, op, axis, None, n, [1] * (n - 1) + [0], halo=(0, 0, 0)) == cd.RESULT_INVALID_USAGE
        assert _message(capfd) == "parity argument must be +1 or -1"
        assert _call(h, gd, op, axis, None, n, par, halo=(0, 0, 0), centering=2) == cd.RESULT_INVALID_USAGE
        assert _message(capfd) == "centering argument must be 0 or 1"
        # no halo along the dim; a periodic dim
        assert _call(h, gd, op, axis, fake[:n], n, par, halo=(1, 0, 1), dim=1, clear=clear) == cd.RESULT_SUCCESS
        assert _call(h, gd, op, axis, fake[:n], n, par, halo=(1, 2, 1), dim=1, periods=(False, True, False), clear=clear) == cd.RESULT_SUCCESS
        assert capfd.readouterr().err == ""
    # a rank away from the edge: the middle rank of three along a dim has neighbours on both sides (stateless planner: no sides)
    spec = cd.make_grid_spec((8, 12, 8), (3, 1), ((0, 1, 2),) * 3)
    for planner in (cd.cudecompExtPlanHaloReflect, cd.cudecompExtPlanHaloFold):
        assert planner(spec, 1, 0, (1, 1, 1), (0, 0, 0), 1).n_pre == 0 and planner(spec, 0, 0, (1, 1, 1), (0, 0, 0), 1).n_pre == 1


# ---- the launch description ------------------------------------------------------------------------------------------------
def _moves_of(plan):
    return [plan.pre[i] for i in range(plan.n_pre)]


def _single_choice(move, address, es, mode, dtype, force):
    """the single call's classification of one move (cudecompExtDescribeMoves with the unsigned mirror modes of cudecompExtRunMoves)"""
    single_mode = {cd.MIRROR_REFLECT: cd.MOVES_REFLECT, cd.MIRROR_FOLD: cd.MOVES_FOLD, cd.MIRROR_FOLD_TAKE: cd.MOVES_FOLD_TAKE}[mode]
    launches = cd.cudecompExtDescribeMoves([move], [address, address, 0], es, single_mode, dtype, force)
    assert len(launches) == 1
    return launches[0]


@pytest.mark.parametrize("dtype", [cd.DOUBLE, cd.HALF, cd.FLOAT_COMPLEX, cd.DOUBLE_COMPLEX, cd.BFLOAT16], ids=["fp64", "fp16", "complex64", "complex128", "bf16"])
def test_launch_description_over_geometries(dtype):
    """the moves of the single reflection and fold plans (parity +1: unsigned) over grids, layouts, axes, dims, halos, paddings and
    centerings, described as mirrored field-move lists of 2, 3, 9 and 32 fields: ONE launch for the one or two sides (the ordered
    fold: one per side), rows or element-wise as the single call classifies the same move, blocks == n_fields * blocks_per_field,
    the spelled name, independent of the mask of signs; the lanes are the narrowest any field's address allows"""
    es = ES[dtype]
    base = 1 << 32
    seen = set()
    orders = (((0, 1, 2),) * 3, ((0, 1, 2), (1, 2, 0), (2, 0, 1)), ((1, 0, 2), (2, 1, 0), (0, 2, 1)))
    combos = itertools.product(((11, 9, 7), (3, 16, 130)), orders, range(3), range(3), ((1, 1, 1), (2, 2, 2), (3, 2, 1)),
                               ((0, 0, 0), (1, 2, 0)), (0, 1))
    for i, (gdims, order, axis, dim, halo, padding, centering) in enumerate(combos):
        spec = cd.make_grid_spec(gdims, (1, 1), order)
        info = cd.cudecompExtPencilInfo(spec, 0, axis, halo, padding)
        stride = int(info.size) + 37  # elements between two fields
        for mode in MODES:
            try:
                if mode == cd.MIRROR_REFLECT:
                    plan = cd.cudecompExtPlanHaloReflect(spec, 0, axis, halo, (0, 0, 0), dim, padding, centering, False)
                else:
                    plan = cd.cudecompExtPlanHaloFold(spec, 0, axis, halo, (0, 0, 0), dim, padding, centering, False, int(mode == cd.MIRROR_FOLD_TAKE))
            except cd.CudecompError as e:
                assert e.code == cd.RESULT_INVALID_USAGE  # (the mirror reaches beyond the interior)
                continue
            moves = _moves_of(plan)
            assert len(moves) == 2
            ordered = mode != cd.MIRROR_REFLECT and bool(plan.reserved & 2)
            n = (2, 3, 9, 32)[i % 4]
            force = (0, 1, 2)[(i // 4) % 3]
            fields = [base + f * stride * es for f in range(n)]
            for group in ([[moves[0]], [moves[1]]] if ordered else [moves]):
                d = cd.cudecompExtDescribeMirroredFieldMoves(group, fields, es, mode, dtype, 0, force)
                assert d == cd.cudecompExtDescribeMirroredFieldMoves(group, fields, es, mode, dtype, (1 << n) - 1, force)
                assert d["blocks"] == n * d["blocks_per_field"] and d["blocks_per_field"] >= len(group), d
                singles = [_single_choice(m, a, es, mode, dtype, force) for m in group for a in fields]  # (every field's own address)
                rows = all(s["kind"] in (16, 18, 20) for s in singles)  # (K_ROWS_REFLECT, K_ROWS_FOLD, K_ROWS_FOLD_TAKE)
                assert d["kind"] == KINDS[mode][0 if rows else 1], (gdims, order, axis, dim, halo, padding, d, singles)
                if len({s["vec"] for s in singles}) == 1:  # (the lanes of every single call: the same workgroups per field)
                    assert d["blocks_per_field"] == sum(s["blocks"] for s in singles[::n]), (d, singles)
                name = spell(d, es, dtype)
                assert name.startswith(("rows_fields_" if rows else "generic_fields_") + ("reflect" if mode == cd.MIRROR_REFLECT else "fold"))
                if rows:
                    assert d["access"] == (1 if force & 2 else 0) and d["vec"] == min(s["vec"] for s in singles) and d["vec"] >= es
                else:
                    assert d["access"] == 0 and d["vec"] == es
                if force & 1:
                    assert not rows
                seen.add((mode, rows, ordered))
    assert {(m, r) for m, r, _ in seen} == set(itertools.product(MODES, (True, False))), seen
    assert any(o for _, _, o in seen)


def test_the_planner_refuses_what_is_no_mirrored_list():
    """internal errors of the list planner, before any launch: a list without a mirrored dim is fine (one cell thick), but the
    workspace, a row pitch, an unknown mode, a sign bit beyond the fields and a data type that does not fit the element size are not"""
    m = cd.make_move((4, 3, 2), (1, -6, 40), (1, 6, 40), src_off=100, dst_off=300, src_buf=0, dst_buf=0)
    fields = [1 << 20, 2 << 20]
    assert cd.cudecompExtDescribeMirroredFieldMoves([m], fields, 8, cd.MIRROR_REFLECT, cd.DOUBLE)["kind"] == 31
    for bad, code in ((dict(mode=3), cd.RESULT_INVALID_USAGE), (dict(fields_neg=4), cd.RESULT_INVALID_USAGE),
                      (dict(dtype=cd.FLOAT), cd.RESULT_INVALID_USAGE)):
        args = dict(mode=cd.MIRROR_FOLD, dtype=cd.DOUBLE, fields_neg=1)
        args.update(bad)
        with pytest.raises(cd.CudecompError) as info:
            cd.cudecompExtDescribeMirroredFieldMoves([m], fields, 8, args["mode"], args["dtype"], args["fields_neg"])
        assert info.value.code == code, bad
    for change in (dict(src_buf=2), dict(dst_buf=2), dict(row_pitch=8)):
        kw = dict(src_off=100, dst_off=300, src_buf=0, dst_buf=0)
        kw.update(change)
        with pytest.raises(cd.CudecompError) as info:
            cd.cudecompExtDescribeMirroredFieldMoves([cd.make_move((4, 3, 2), (1, -6, 40), (1, 6, 40), **kw)], fields, 8, cd.MIRROR_FOLD, cd.DOUBLE)
        assert info.value.code == cd.RESULT_INTERNAL_ERROR, change
    # two mirrored dims
    with pytest.raises(cd.CudecompError):
        cd.cudecompExtDescribeMirroredFieldMoves([cd.make_move((4, 3, 2), (1, -6, -40), (1, 6, 40), src_off=100, dst_off=300, src_buf=0, dst_buf=0)],
                                                 fields, 8, cd.MIRROR_REFLECT, cd.DOUBLE)
    # the copying, adding and taking lists keep refusing a negative stride
    with pytest.raises(cd.CudecompError) as info:
        cd.cudecompExtDescribeFieldMovesOp([m], fields, 0, 0, 8, cd.MOVES_COPY, cd.DOUBLE)
    assert info.value.code == cd.RESULT_INTERNAL_ERROR
