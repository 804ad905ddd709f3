"""The ORDER in which the entry points of a halo family check their arguments, pinned by the message of the refusal: a call with
every argument wrong is refused for the first check; putting that argument right, for the second; and so on down the ladder.  The
tests of each family (tests/test_abi.py for the update, tests/test_halo_*_plan.py for the others) run their own family through it.
Everything happens on the host: no pointer is device memory and the last call of a ladder has nothing to do."""
import ctypes as C
import re

import cudecomp_amd as cd

_i3, _b3 = (C.c_int32 * 3), (C.c_bool * 3)
_FIELDS = (C.c_void_p * 2)(0x10000, 0x20000)

# argument -> (wrong value, right value, message of the check); None for handle / descriptor: filled in per call
_CHECKS = {
    "handle": (None, None, "invalid handle"),
    "gd": (None, None, "invalid grid descriptor"),
    "dtype": (99, cd.FLOAT, "unknown data type"),
    "halo": (None, _i3(1, 1, 1), "halo_extents argument cannot be null"),
    "input": (None, 1, "input argument cannot be null"),
    "inputs": (None, _FIELDS, "inputs argument cannot be null"),
    "n_fields": (0, 2, "n_fields argument out of range"),
    "work": (None, 1, "work argument cannot be null"),
    "dim": (7, 0, "dim argument out of range"),
    "parity": (0, 1, "parity argument must be +1 or -1"),
    "centering": (2, 0, "centering argument must be 0 or 1"),
    "clear": (2, 0, "clear argument must be 0 or 1"),
}

# family -> (symbols, the arguments in the order of the C prototype, the ladder: the arguments in the order they are checked,
#            the arguments still checked when every halo is zero -- "ZERO" marks where that call returns)
FAMILIES = {
    "update": (["cudecompUpdateHalos" + a for a in "XYZ"], "handle gd input work dtype halo periods dim pad stream",
               "handle gd dtype halo ZERO input work dim", ""),
    "accumulate": (cd.AMD_SYMBOLS, "handle gd input work dtype halo periods dim pad stream",
                   "handle gd dtype halo ZERO input work dim", ""),
    "accumulate_clear": (cd.AMD_ACCUMULATE_CLEAR_SYMBOLS, "handle gd input work dtype halo periods dim pad stream",
                         "handle gd dtype halo ZERO input work dim", ""),
    "fill": (cd.AMD_FILL_SYMBOLS, "handle gd input dtype value halo periods dim pad stream",
             "handle gd dtype halo ZERO input dim", ""),
    "reflect": (cd.AMD_REFLECT_SYMBOLS, "handle gd input dtype parity centering halo periods dim pad stream",
                "handle gd dtype halo ZERO input dim parity centering", "parity centering"),
    "fold": (cd.AMD_FOLD_SYMBOLS, "handle gd input dtype parity centering clear halo periods dim pad stream",
             "handle gd dtype halo ZERO input dim parity centering clear", "parity centering clear"),
    "fields": (cd.AMD_FIELDS_SYMBOLS, "handle gd inputs n_fields work dtype halo periods dim pad stream",
               "handle gd dtype halo ZERO inputs n_fields work dim", ""),
    "accumulate_fields": (cd.AMD_ACCUMULATE_FIELDS_SYMBOLS, "handle gd inputs n_fields work dtype halo periods dim pad clear stream",
                          "handle gd dtype halo clear ZERO inputs n_fields work dim", ""),
}


def _refused_for(fn, order, args, message, capfd):
    assert fn(*[args[a] for a in order]) == cd.RESULT_INVALID_USAGE, message
    err = capfd.readouterr().err
    assert re.search(r"CUDECOMP:ERROR: .*Invalid usage\. \(%s\)" % re.escape(message), err), (message, err)


def check(family, capfd):
    symbols, order, ladder, in_zero = FAMILIES[family]
    order, ladder, in_zero = order.split(), ladder.split(), in_zero.split()
    h = cd.cudecompInit()
    gd = cd.cudecompGridDescCreate(h, cd.make_config((9, 10, 11), (1, 1)))
    right = {"handle": h, "gd": gd}
    mirrored = family in ("reflect", "fold")  # (a non-periodic dim has cells to mirror; a periodic one has cells to update)
    capfd.readouterr()
    for name in symbols:
        fn = getattr(cd.lib(), name)
        args = {a: _CHECKS[a][0] for a in ladder if a != "ZERO"}
        args.update(periods=_b3(*(mirrored,) * 3), pad=None, stream=None, value=None)
        for step, a in enumerate(ladder):
            if a == "ZERO":  # every halo zero: success whatever follows, but for the arguments the contract names
                zero = dict(args, halo=_i3(0, 0, 0))
                for z in in_zero:
                    _refused_for(fn, order, zero, _CHECKS[z][2], capfd)
                    zero[z] = _CHECKS[z][1]
                assert fn(*[zero[x] for x in order]) == cd.RESULT_SUCCESS, (name, "all halos zero")
                assert capfd.readouterr().err == ""
                continue
            _refused_for(fn, order, args, _CHECKS[a][2], capfd)
            args[a] = right.get(a, _CHECKS[a][1])
        assert fn(*[args[x] for x in order]) == cd.RESULT_SUCCESS, (name, "every argument right")
        assert capfd.readouterr().err == ""
        if mirrored:  # the plan's own refusal comes after parity, centering and clear
            far = dict(args, halo=_i3(9, 0, 0), periods=None, centering=1)
            for z in in_zero:
                _refused_for(fn, order, dict(far, **{x: _CHECKS[x][0] for x in in_zero[in_zero.index(z):]}), _CHECKS[z][2], capfd)
            _refused_for(fn, order, far, "halo reflection reaches beyond the interior of the pencil", capfd)
    cd.cudecompGridDescDestroy(h, gd)
    cd.cudecompFinalize(h)
