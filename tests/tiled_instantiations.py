"""Every instantiation of the LDS-tiled single-field copy kernels (transpose_kernel, transpose_window_kernel,
transpose_lines_kernel, transpose_rowlines_kernel) and of the remote-store forms of the row and element-wise copies
(rows_kernel<VB,3>, rows_shifted_kernel<VB,3>, generic_kernel<ES,true>), each with a recipe that reaches it through
cudecompExtDescribeMoves / cudecompExtRunMoves: tests/test_tiled_instantiation_table.py checks the table on the CPU,
tests/test_gpu_tiled_kernel_instantiations.py runs it.  numpy-free and torch-free at import.

INVENTORY spells the names from the four dispatch tables: launchT (csrc/kernels_transpose.hip), CD_WINDOW_SHAPES
(csrc/kernels_dev.h) with the STREAM values of launchWindowBatch, launchLinesBatch and launchRowLinesBatch, and launchRowsBatch
(csrc/kernels_rows.hip).  The remote-store policy (STREAM 3) is reached on local memory with destination bases: a list with
bases is a list of one-sided sends, whatever memory the bases name.

A recipe is two geometries -- a wide move and a small one with clearly unequal workgroup counts -- plus the flags, the
destination offset and whether the destinations are bases.  The shapes are the smallest at which every branch of the kernel is
live:
  plain      2 x 2 tiles x 3 planes = 12 workgroups: the XCD walk (per = 1) permutes 8 and leaves 4 in its tail; one tile is
             interior (the unguarded copy), the others end inside the move along i, along j and along both.  Vector lanes:
             TI + 3 VW by TJ + 5 VW; element-wise lanes: TI + 3 by TJ + 5 (odd).  STREAM 2: row pitches of both sides on the
             128-byte grid (16-byte elements: planes of the destination on the 4-KiB grid as well); STREAM 4: the source pitch off
             that grid, dword-aligned; STREAM 3: bases.  The longer tiles: source rows more than 8 destination rows apart.
  window     the destination one lane vector off the 64-byte grid, its row pitch odd (rows of a tile at different phases);
             2 TJ + 5 VW (2 TJ + 5) along j: a left-edge window (jb < 0), an interior one and a right-edge one; 2 x 3 x 3 = 18.
  lines      the geometry of _lines in tests/test_gpu_kernel_names.py: rows of 256 cells, three planes, a gap of 2 cells that
             the kernel reads back and rewrites; the move carries its row pitch.
  row lines  the geometry of _rowlines there: rows of 2 (TJ + 128 / ES) + 1 cells, gap 2.  The kernel knows three kinds of tile
             by i alone: the wide move has the unguarded one and the ragged one, the small move (exactly TI rows, where the lane
             width allows it) the one that ends with the plane's last row.
  rows       the wide and short shapes of tests/test_gpu_kernel_instantiations.py (300 / 301 vectors x 9 rows x 3 planes,
             7 vectors x 9 x 5; shifted rows: the shortest row the kernel takes), with bases.
  generic    no unit stride along the rows on either side.  The small move is the 7 x 9 x 5 one of that module (2 workgroups);
             the wide one is 7 x 37 x 9 with a destination-fast dim (10 workgroups): two moves of 315 elements would have equal
             workgroup counts, and a list of them no filler workgroups.
The small move of every tiled recipe is one tile row that ends inside the move, with 2 planes.  No buffer reaches 4 MiB."""
import cudecomp_amd as cd
from tests import move_lists as ML

GENERIC, STREAMING, ALWAYS, I_FIRST, J_FIRST = 1, 2, 4, 64, 128  # flags of cudecompExtRunMoves / cudecompExtDescribeMoves

# (element size, elements per lane, tile i, tile j)
PLAIN_SHAPES = ((2, 8, 128, 128), (2, 1, 64, 64), (4, 4, 64, 128), (4, 1, 64, 64), (8, 2, 64, 64), (8, 1, 64, 64), (16, 1, 32, 32))
WINDOW_SHAPES = ((4, 4, 64, 128), (4, 1, 64, 128), (8, 2, 64, 64), (8, 1, 64, 64), (16, 1, 32, 32))
TF = {True: "true", False: "false"}

# {(family, element size): names}
INVENTORY = {}
for _es in (2, 4, 8, 16):
    INVENTORY[("transpose", _es)] = ["transpose_kernel<%d,%d,%d,%d,%d,%s>" % (e, vw, ti, tj, s, TF[e != 16])
                                     for (e, vw, ti, tj) in PLAIN_SHAPES if e == _es for s in (0, 2, 3, 4)]
INVENTORY[("transpose", 8)].append("transpose_kernel<8,2,64,128,2,true>")
INVENTORY[("transpose", 16)].append("transpose_kernel<16,1,32,64,2,false>")
for _es in (4, 8, 16):
    _shapes = [x for x in WINDOW_SHAPES if x[0] == _es]
    INVENTORY[("window", _es)] = ["transpose_window_kernel<%d,%d,%d,%d,%d>" % (x + (s,)) for x in _shapes for s in (0, 3, 4)]
    INVENTORY[("lines", _es)] = ["transpose_lines_kernel<%d,%d,%d,%d,%d,128>" % (x + (s,)) for x in _shapes for s in (0, 4)]
    INVENTORY[("rowlines", _es)] = ["transpose_rowlines_kernel<%d,%d,%d,%d,%d,128>" % (x + (s,)) for x in _shapes for s in (0, 4)]
INVENTORY[("remote", 2)] = ["rows_kernel<2,3>", "generic_kernel<2,true>"]
INVENTORY[("remote", 4)] = ["rows_kernel<4,3>", "rows_shifted_kernel<4,3>", "generic_kernel<4,true>"]
INVENTORY[("remote", 8)] = ["rows_kernel<8,3>", "rows_shifted_kernel<16,3>", "rows_shifted_kernel<8,3>", "generic_kernel<8,true>"]
INVENTORY[("remote", 16)] = ["rows_kernel<16,3>", "generic_kernel<16,true>"]
GROUPS = sorted(INVENTORY, key=lambda g: (("transpose", "window", "lines", "rowlines", "remote").index(g[0]), g[1]))
TILED = ("transpose", "window", "lines", "rowlines")
COUNTS = {"transpose": 30, "window": 15, "lines": 10, "rowlines": 10, "remote": 11}
# instantiations no move reaches, with the reason from classify(): none
UNREACHABLE = {}


def spell(l):
    """the kernel's name from a described launch, by the rules of spellKernelName / streamArgOf (csrc/kernels.cc, kernels_batch.h)"""
    kind, a = ML.KINDS[l["kind"]], l["access"]
    row = 3 if a == 3 else (1 if a >= 1 else 0)
    win = 4 if a == 2 else a
    if kind == "rows":
        return "rows_kernel<%d,%d>" % (l["vec"], row)
    if kind == "rows_shifted":
        return "rows_shifted_kernel<%d,%d>" % (l["vec"], row)
    if kind == "generic":
        return "generic_kernel<%d,%s>" % (l["es"], TF[a == 3])
    if kind == "transpose":
        return "transpose_kernel<%d,%d,%d,%d,%d,%s>" % (l["es"], l["vec"], l["tile_i"], l["tile_j"], a, TF[l["es"] != 16])
    if kind == "transpose_window":
        return "transpose_window_kernel<%d,%d,%d,%d,%d>" % (l["es"], l["vec"], l["tile_i"], l["tile_j"], win)
    if kind in ("transpose_lines", "transpose_rowlines"):
        return "%s_kernel<%d,%d,%d,%d,%d,128>" % (kind, l["es"], l["vec"], l["tile_i"], l["tile_j"], win)
    return "%s<?>" % kind


def up(n, m):
    return -(-n // m) * m


class Recipe:
    """wide / small: (extent, source strides, destination strides, row pitch) in elements; dims (i, j, k) of the tiled families:
    i unit-stride in the source, j in the destination, k the plane"""

    def __init__(self, name, family, es, wide, small, flags=0, doff=0, bases=False, tile=None):
        self.name, self.family, self.es, self.wide, self.small = name, family, es, wide, small
        self.flags, self.doff, self.bases, self.tile = flags, doff, bases, tile

    def moves(self, which):
        """the list "wide", "small" or "both": every move in a region of its own that begins on a multiple of 256 elements, so a
        move sits in the list at the alignment it has alone; with bases every destination is a buffer of its own"""
        geos = {"wide": [self.wide], "small": [self.small], "both": [self.wide, self.small]}[which]
        if not self.bases:
            p = ML.Packer(gap=3, align=256)
            for extent, ss, ds, pitch in geos:
                p.add(extent, ss, ds, 0, self.doff, row_pitch=pitch)
            return p.moves
        out, soff = [], 0
        for extent, ss, ds, pitch in geos:
            out.append(cd.make_move(extent, ss, ds, soff, self.doff, 0, 1, pitch))
            soff = up(soff + ML.span(extent, ss) + 3, 256)
        return out

    def tiles(self, geo):
        """(tiles wholly inside the move, tiles that end inside it, workgroups) of one geometry, by the conditions of the kernels"""
        (ei, ej, ek), _, ds, _ = geo
        ti, tj = self.tile
        t0 = -(-ei // ti)
        inside_i = [(b + 1) * ti <= ei for b in range(t0)]
        if self.family == "transpose":
            t1, planes = -(-ej // tj), ek
            inside_j = [(b + 1) * tj <= ej for b in range(t1)]
        elif self.family == "rowlines":  # kind 2 of the kernel: the row after the tile's last one exists too
            t1, planes = (ds[0] - 1 + 128 // self.es - 1) // tj + 1, ek
            inside_i, inside_j = [(b + 1) * ti < ei for b in range(t0)], [True] * t1
        else:  # windows: over j (64-byte units), or over the linear positions of the slab (128-byte units)
            u = (64 if self.family == "window" else 128) // self.es
            length, planes = (ej, ek) if self.family == "window" else ((ek - 1) * ds[2] + ej, 1)
            t1 = -(-(length + u - 1) // tj)
            inside_j = [b * tj - (u - 1) >= 0 and b * tj - (u - 1) + tj + u - 1 <= length for b in range(t1)]
        inside = sum(a and b for a in inside_i for b in inside_j) * planes
        return inside, t0 * t1 * planes - inside, t0 * t1 * planes


def _plain(es, vw, ti, tj, s):
    ei, ej = (ti + 3 * vw, tj + 5 * vw) if vw > 1 else (ti + 3, tj + 5)
    line = 128 // es
    if s in (2, 4):  # destination rows and planes on the 128-byte grid (planes: the 4-KiB grid)
        sj = up(ei + 1, line) + (0 if s == 2 else max(1, 4 // es))
        ss = (1, sj, sj * (ej + 1))
        di = up(ej + 1, line)
        ds = (di, 1, up(di * (ei + 1), 4096 // es))
    else:
        ss, ds = (1, ei + 6, (ei + 6) * ej + 10), (ej + 2, 1, (ej + 2) * ei + 6)
    small = (ti - 3 * vw if vw > 1 else ti - 3, ej, 2)
    name = "transpose_kernel<%d,%d,%d,%d,%d,%s>" % (es, vw, ti, tj, s, TF[es != 16])
    return Recipe(name, "transpose", es, ((ei, ej, 3), ss, ds, 0), (small, ss, ds, 0), STREAMING if s in (2, 4) else 0, 0, s == 3, (ti, tj))


def _far_source(es, vw, ti, tj, extent, ss, ds):
    name = "transpose_kernel<%d,%d,%d,%d,2,%s>" % (es, vw, ti, tj, TF[es != 16])
    small = (ti - 3 * vw if vw > 1 else ti - 3, extent[1], 2)
    return Recipe(name, "transpose", es, (extent, ss, ds, 0), (small, ss, ds, 0), STREAMING, 0, False, (ti, tj))


def _window(es, vw, ti, tj, s):
    ei, ej = (ti + 3 * vw, 2 * tj + 5 * vw) if vw > 1 else (ti + 3, 2 * tj + 5)
    di = ej + 3 + ej % 2  # odd: consecutive rows at different phases of the 64-byte unit
    ss, ds = (1, ei + 2, (ei + 2) * ej + 6), (di, 1, di * ei + 5)
    small = (ti - 3 * vw if vw > 1 else ti - 3, ej, 2)
    name = "transpose_window_kernel<%d,%d,%d,%d,%d>" % (es, vw, ti, tj, s)
    return Recipe(name, "window", es, ((ei, ej, 3), ss, ds, 0), (small, ss, ds, 0), ALWAYS | (STREAMING if s == 4 else 0), vw, s == 3, (ti, tj))


def _lines(es, vw, ti, tj, s):
    ei, ej, gap = ti + 3 * vw if vw > 1 else ti + 3, 256, 2
    dk = ej + gap
    ss, ds = (1, ei, ei * ej), (dk * 5, 1, dk)
    small = (ti - 3 * vw if vw > 1 else ti - 3, ej, 2)
    name = "transpose_lines_kernel<%d,%d,%d,%d,%d,128>" % (es, vw, ti, tj, s)
    return Recipe(name, "lines", es, ((ei, ej, 3), ss, ds, dk), (small, ss, ds, dk), ALWAYS | (STREAMING if s == 4 else 0), 1, False, (ti, tj))


def _rowlines(es, vw, ti, tj, s):
    ei, ej, gap = ti + 3 * vw if vw > 1 else ti + 3, 2 * (tj + 128 // es) + 1, 2
    di = ej + gap
    ss, ds = (1, ei * 3, ei), (di, 1, di * (ei + 2))
    # exactly TI rows: the tile that ends with the plane's last row (a multiple of TI holds whole vectors: not for element-wise
    # lanes of 4- and 8-byte elements, which keep a ragged tile)
    small = (ti if vw > 1 or es == 16 else ti - 3, ej, 2)
    name = "transpose_rowlines_kernel<%d,%d,%d,%d,%d,128>" % (es, vw, ti, tj, s)
    return Recipe(name, "rowlines", es, ((ei, ej, 3), ss, ds, di), (small, ss, ds, di), ALWAYS | (STREAMING if s == 4 else 0), 1, False, (ti, tj))


def _rows(nvec, planes, vb, es):
    w, h = nvec * vb // es, 9
    sp, dp = w + 4 + (w & 1), w + 8 + (w & 1)
    return (w, h, planes), (1, sp, sp * (h + 1)), (1, dp, dp * (h + 2)), 0


def _remote(es):
    out = [Recipe("rows_kernel<%d,3>" % es, "remote", es, _rows(300 if es == 16 else 301, 3, es, es), _rows(7, 5, es, es), 0, 0, True)]
    # destination rows one element off the 64-byte grid; the short row is the shortest the kernel takes (256 bytes and more)
    for vb, e, short in ((16, 8, 17), (8, 8, 33), (4, 4, 65)):
        if e == es:
            out.append(Recipe("rows_shifted_kernel<%d,3>" % vb, "remote", es, _rows(300 if vb == 16 else 301, 3, vb, es),
                              _rows(short, 5, vb, es), ALWAYS, 1, True))
    out.append(Recipe("generic_kernel<%d,true>" % es, "remote", es, ((7, 37, 9), (2, 17, 646), (40, 1, 290), 0),
                      ((7, 9, 5), (2, 17, 170), (3, 23, 230), 0), 0, 0, True))
    return out


def recipes(family, es):
    """the recipes of one group, in the order of INVENTORY[(family, es)]"""
    if family == "transpose":
        out = [_plain(e, vw, ti, tj, s) for (e, vw, ti, tj) in PLAIN_SHAPES if e == es for s in (0, 2, 3, 4)]
        if es == 8:
            out.append(_far_source(8, 2, 64, 128, (70, 138, 3), (1, 1280, 80), (144, 1, 10192)))
        if es == 16:
            out.append(_far_source(16, 1, 32, 64, (35, 69, 3), (1, 768, 40), (72, 1, 2560)))
        return out
    if family == "remote":
        return _remote(es)
    make, modes = {"window": (_window, (0, 3, 4)), "lines": (_lines, (0, 4)), "rowlines": (_rowlines, (0, 4))}[family]
    return [make(e, vw, ti, tj, s) for (e, vw, ti, tj) in WINDOW_SHAPES if e == es for s in modes]


def launches_of(recipe):
    """(list, further flags) of every launch of a recipe: the wide move alone, the small one alone, both as one list; the tiled
    kernels run the wide move twice more, the tile walk forced i first and j first"""
    out = [("wide", 0), ("small", 0), ("both", 0)]
    if recipe.family in TILED:
        out += [("wide", I_FIRST), ("wide", J_FIRST)]
    return out
