// kernels_batch.h -- what csrc/kernels.cc (host: classification, batching) and the kernel code objects share: the record of a
// kernel choice (KernelChoice), the launch descriptor (Batch) and the launchers.  The code objects the classifier dispatches
// to: kernels_rows.hip, kernels_transpose.hip (four, one per element size), kernels_window.hip, kernels_lines.hip,
// kernels_rowlines.hip, kernels_accumulate.hip, kernels_fill.hip, kernels_take.hip, kernels_reflect.hip, kernels_fold.hip, kernels_wall.hip, kernels_wall_plane.hip;
// kernels_rotate.hip and sync.hip are launched by the executor (and compiled as one unit, kernels_executor.hip; kernels_fill.hip, kernels_reflect.hip and kernels_reduce.hip -- the reductions of a box, launchReduce -- likewise as kernels_edge.hip,
// kernels_accumulate.hip and kernels_take.hip as kernels_sum.hip; kernels_profile.hip -- the profiles of a box along one dim, launchProfile -- in two parts, inside kernels_window.hip and kernels_rows.hip; kernels_planes.hip -- the plane updates of a box along one dim, launchPlanes -- in two parts, inside kernels_lines.hip and kernels_rowlines.hip; kernels_combine.hip -- the combinations of two boxes, launchCombine -- in four parts, inside the four units of kernels_transpose.hip); kernels_field_transpose.hip (lists of field-moves: multi-field
// halo phases and transposes), kernels_field_accumulate.hip (the same lists adding or taking: multi-field halo accumulation) and
// kernels_field_mirror.hip (the same lists mirrored, with a sign per field: multi-field wall halos) are reached through
// launchFieldMoveList (kernels.h); kernels_field_wall.hip (the mirrored lists adding an addend per field and layer: multi-field wall
// values, reached through the same launcher as a wall list) is compiled into the unit kernels_executor.hip.  Seventeen code objects in all.  The row and element-wise kernels of all of
// them share one workgroup decode (kernels_walk.h) and their launchers one dispatch (kernels_dispatch.h).
//
// Why several translation units: every .hip file becomes ONE code object inside the library's .hip_fatbin, and a single
// code object beyond roughly 0.6-0.7 MB puts the whole process into a regime where every small synchronous operation costs
// 14 ms (bisected in round 5, profiles/r05_code_size.md: the same 0.74 MB of device code split over two code objects is
// harmless, in one code object it is not).  The kernels therefore live in several small code objects -- row copies + generic,
// the LDS-tiled transposes per element size (kernels_transpose.hip compiled four times), the window transposes, ... -- and
// tests/test_abi.py guards the size of each.  That guard (400,000 bytes per code object) is also why the wall-plane kernels are not
// appended to kernels_wall.hip: 317 KB and 320 KB in one unit would exceed it; kernels_wall_plane.hip is a code object of its own.
#pragma once
#include <hip/hip_runtime_api.h>

#include <cstdint>

#include "errors.h"

namespace cudecomp {

// arithmetic of an add-move (Move3D::add): the REAL type the elements consist of (complex elements are two of them)
enum ArithType { ARITH_NONE = 0, ARITH_F16 = 1, ARITH_BF16 = 2, ARITH_F32 = 3, ARITH_F64 = 4 };

namespace kern {

constexpr int kMaxBatch = 8;
constexpr int kThreads = 256;
constexpr int kRowsUnroll = 4;
constexpr long long kStreamBytes = 32ll << 20;  // moves at least this large use non-temporal access
constexpr int kMaxWallHalo = 8;                 // layers a wall-move's addend table holds (CUDECOMP_AMD_MAX_WALL_HALO)

struct DevMove {
  const char* src;
  char* dst;
  long long e[3];   // extents   (units depend on the kernel, see the launchers)
  long long ss[3];  // src strides (rows_fill_kernel, which has no source: ss[0] = row length in bytes); negative along the
                    // mirrored dim of a reflect- or fold-move, and only there
  long long ds[3];  // dst strides
};

// tile walk of the LDS-tiled transposes: bits of Batch::p1
constexpr int kWalkXcd = 1;            // every XCD gets a contiguous run of tiles
constexpr int kWalkJFirst = 2;         // along the destination rows (j) first; clear: along the source rows (i) first
constexpr int kWalkRunOverPlanes = 4;  // transpose_kernel: the runs of p0 are over batch planes; clear: over tiles along j
constexpr int kWalkLines = 8;          // the walk of transpose_lines_kernel
constexpr int kWalkRowLines = 16;      // the walk of transpose_rowlines_kernel
constexpr int kWalkGroupShift = 8;     // transpose_lines_kernel: p1 >> kWalkGroupShift = tile rows per group (0: all)

struct Batch {
  int n;
  int interleave;  // 1: workgroup b serves move b % n (moves with REMOTE destinations: keeps every xGMI link busy
                   // for the whole launch instead of draining one peer's chunk after the other)
  // p0, p1 per kind of kernel (KernelKind):
  //   row copies and additions   p0 = log2 of the lanes per row; p1 = row length in BYTES (rows_shifted_kernel only);
  //                              rows_dense_kernel reads neither
  //   transposes                 p0 = run length of the tile walk (tiles or planes; 0 / 1 = no runs), p1 = kWalk* bits
  //   element-wise               p0 = the dim the lanes run along, p1 unused
  //   fills                      p0 as for rows / element-wise; p1 unused
  //   takes                      p0 as for rows / element-wise; p1 unused
  //   reflections                p0 as for rows / element-wise; p1 unused
  //   folds                      p0 as for rows / element-wise; p1 unused
  //   wall-moves                 p0 as for rows / element-wise; p1 = the entry of e[] that is the mirrored dim, whose index is the
  //                              destination layer (rows: 1 the row, 2 the plane); -1: the mirrored dim is one cell thick, layer 0
  int p0[kMaxBatch];
  int p1[kMaxBatch];
  unsigned int first_block[kMaxBatch + 1];
  unsigned int t0[kMaxBatch];             // tiles along dim 0
  unsigned int t1[kMaxBatch];             // tiles along dim 1
  DevMove m[kMaxBatch];
};

// The addends of a launch of wall-moves (kernels_wall.hip): a kernel argument of its own beside the Batch, which stays as it is.
// Row i belongs to move i of the Batch; entry j is the addend of DESTINATION layer j along the mirrored dim -- the element, already
// converted to the call's type, replicated to 16 bytes.  Lanes hold whole elements and start on an element's boundary, so the low
// VB bytes of an entry serve every lane.
struct WallTable {
  unsigned int w[kMaxBatch][kMaxWallHalo][4];
};
static_assert(sizeof(Batch) + sizeof(WallTable) + 16 <= 2048, "Batch, sign mask and addend table stay well under the 4 KB of kernel arguments");

// The third operand of a launch of wall-plane moves (kernels_wall_plane.hip; Move3D::plane): a kernel argument of its own beside the
// Batch, which stays as it is.  Entry i belongs to move i of the Batch: the address of the plane entry that destination index
// (0, 0, 0) adds, and three SIGNED strides in the units of that move's DevMove (rows: s[0] unused, s[1] and s[2] in bytes;
// element-wise: elements) -- negative along the mirrored dim of a low side, and only there.  Not a table of values: the values stay
// in device memory and are read when the kernel runs, so a replayed graph applies what the planes hold then.  8 x 32 bytes.
struct PlaneOperand {
  const char* p;
  long long s[3];
};
struct PlaneOperands {
  PlaneOperand m[kMaxBatch];
};
static_assert(sizeof(PlaneOperands) == kMaxBatch * 32, "one pointer and three strides per move of the launch");
static_assert(sizeof(Batch) + sizeof(PlaneOperands) + 16 <= 2048, "Batch, sign mask and plane operands stay well under the 4 KB of kernel arguments");

// ---- lists of field-moves: up to kMaxBatch moves, each for up to kMaxFields (input, output) pairs of buffers, in ONE launch
// (kernels_field_transpose.hip; multi-field halo updates and transposes, include/cudecomp_halo_fields.h and
// include/cudecomp_transpose_fields.h) ------------------------------------------------------------------------------------------
// The geometry is held once per move, with byte OFFSETS in the place of DevMove's pointers.  Each end of a move names its base:
// kEndInput "field f's entry of the input table", kEndOutput "field f's entry of the output table", kEndWork "the workspace at
// f * a per-move byte step" (the fields' pieces of one peer's chunk lie one behind the other).  Workgroup b serves the move
// whose [first_block[i], first_block[i + 1]) holds it; inside the move, field rel / blocks and that field's workgroup
// rel % blocks -- one decode per workgroup.  The struct travels in the kernel arguments and stays under their 4 KB (1.7 KB).
constexpr int kMaxFields = 32;  // two 256-byte tables of pointers in the kernel arguments
constexpr int kEndInput = 0, kEndOutput = 1, kEndWork = 2;

struct FieldMove {
  long long src_off, dst_off;    // bytes from the base of that end
  long long src_step, dst_step;  // kEndWork ends: bytes between the pieces of consecutive fields (0 for table ends)
  long long e[3];                // transpose_fields_kernel: {ei, ej, ek}, ss = {1, sj, sk}, ds = {di, 1, dk} in ELEMENTS;
  long long ss[3];               // rows_fields_kernel: vectors per row / rows / planes, strides in BYTES;
  long long ds[3];               // generic_fields_kernel: extents and strides in ELEMENTS
  int src_end, dst_end;          // kEnd*
  int p0;                        // rows: log2 of the lanes per row; element-wise: the dim the lanes run along
  unsigned int t0, t1;           // transposes: tiles along i / j; rows: tile columns / tile rows per plane
  unsigned int blocks;           // workgroups PER FIELD
};

struct FieldMoveBatch {
  int n, n_fields;
  unsigned int first_block[kMaxBatch + 1];  // first_block[i + 1] - first_block[i] = n_fields * m[i].blocks
  char* work;
  FieldMove m[kMaxBatch];
  char* in[kMaxFields];
  char* out[kMaxFields];
};
static_assert(sizeof(FieldMoveBatch) < 4096, "FieldMoveBatch must fit the kernel arguments");

// The addends of a launch of wall field-moves (kernels_field_wall.hip: multi-field wall values,
// include/cudecomp_halo_wall_value_fields.h): a kernel argument of its own beside the FieldMoveBatch, which stays as it is.  Fields x
// sides x layers entries of 16 bytes would be 8 KB, so the table is COMPACT: kFieldWallTableBytes of `es`-byte entries, each the
// converted element once.  The entry of (move i of the launch, field f of the launch, DESTINATION layer j along the mirrored dim)
// sits at byte ((i * n_fields + f) * layers + j) * es; the host has reversed the low side (kernels.cc fieldWallTableOf).  A lane
// holds whole elements and starts on an element's boundary: it replicates the entry to its width in registers, no phase arises.
constexpr int kFieldWallTableBytes = 2048;
struct FieldWallTable {
  unsigned int w[kFieldWallTableBytes / 4];
};
// ... and how the kernels find a lane's entry: `layers` of the formula above, the element size, and per move of the launch the entry
// of the kernel's e[] whose index is the destination layer -- Batch::p1's meaning for wall-moves (rows: 1 the row, 2 the plane;
// element-wise: the dim; -1: the mirrored dim is one cell thick, layer 0).
struct FieldWallWalk {
  int layers, es;
  int along[kMaxBatch];
};
static_assert(sizeof(FieldMoveBatch) + sizeof(FieldWallTable) + sizeof(FieldWallWalk) + 16 + 8 <= 4096,
              "FieldMoveBatch, addend table, walk, sign mask and the mask of fields stay under the 4 KB of kernel arguments");

// ---- reductions of a box of cells (kernels_reduce.hip; interior reductions, include/cudecomp_interior_reduce.h) ------------------
// Stage one writes one pair of fp64 partials per workgroup, field f's at work[2 * (f * kReduceMaxBlocks + workgroup)]; stage two
// combines a field's pairs.  kReduceMaxBlocks caps the workgroups per field, whatever the box: the workspace depends on the number of
// fields alone (kMaxFields * kReduceMaxBlocks * 16 bytes = 1 MiB at most), and eight workgroups per CU of an MI355X are in flight.
constexpr int kReduceSum = 0, kReduceDot = 1, kReduceMaxAbs = 2;  // CUDECOMP_AMD_REDUCE_*
constexpr int kReduceMaxBlocks = 2048;
// a single row longer than this is cut into rows of this many bytes: a multiple of every element size, and one short of 4 KiB so that
// a cut row touches at most 256 slots of the 16-byte grid -- one tile column -- whatever its phase on that grid
constexpr long long kReduceChunkBytes = 4080;
struct ReduceGeom {
  // rows: bytes; the last row of every plane may be shorter (a cut row).  element-wise: unused
  long long row_bytes, last_row_bytes, rows, planes, s1, s2;
  long long slots;             // rows: 16-byte slots a row can touch at most
  unsigned long long tiles;    // rows: t0 * t1 * planes
  unsigned int t0, t1;         // rows: tile columns / tile rows per plane
  long long e[3], s[3];        // element-wise: extents and strides in ELEMENTS
  long long box_off;           // bytes from a field's pointer to the first cell of the box
  long long rd_lo, rd_hi;      // rows: the bytes [rd_lo, rd_hi) relative to the first cell of the box may be read
  int p0;                      // rows: log2 of the lanes per row; element-wise: the dim the lanes run along
  int reals;                   // reals per element: 1, or 2 for the complex types
  int n_fields;
  int stream;                  // rows: 1 non-temporal loads (KernelChoice::access), 0 default caching
  unsigned int blocks;         // workgroups PER FIELD, at most kReduceMaxBlocks
};
struct ReduceFields {
  const char* a[kMaxFields];
  const char* b[kMaxFields];  // DOT only
};
static_assert(sizeof(ReduceGeom) + sizeof(ReduceFields) + 8 <= 2048, "geometry, the two tables of fields and the workspace stay well under the 4 KB of kernel arguments");

// ---- profiles of a box of cells along one dim (kernels_profile.hip; interior profiles, include/cudecomp_interior_profile.h) -------
// The reduction over two dims of the box, kept along the third: L entries per field.  Stage one cuts the cells of an entry into
// `parts` parts and writes one pair of fp64 partials per (field, part, entry) to work[2 * ((f * parts + part) * L + k)]; stage two
// combines an entry's parts in index order.  parts * L never exceeds max(L, kProfilePairsPerField), parts never kProfileMaxParts:
// the workspace is a function of the number of fields and of L alone.
constexpr int kProfilePairsPerField = 65536;
constexpr int kProfileMaxParts = 1024;
constexpr int kProfileBlocks = 4096;  // stage-one workgroups per field the planner aims at: sixteen per CU of an MI355X
struct ProfileGeom {
  long long L;                 // entries per field: the extent of the kept dim
  long long sk;                // segments, element-wise: BYTES between two entries
  long long row_bytes;         // segments: a row of the contiguous dim; columns: a row of the kept dim (L elements)
  long long rows;              // segments: rows of one entry; columns: all rows of the box, e1 * e2
  long long e1, e2;            // columns, element-wise: the two reduced extents, e1 the one of the smaller stride
  long long s1, s2;            // their strides in BYTES (segments: s1 between the rows of an entry); columns: multiples of 16
  long long rows_per_part;     // columns: part p walks the rows [p * rows_per_part, (p + 1) * rows_per_part)
  long long slots;             // segments, columns: 16-byte slots a row can touch at most
  long long box_off;           // bytes from a field's pointer to the first cell of the box
  long long rd_lo, rd_hi;      // the bytes [rd_lo, rd_hi) relative to the first cell of the box may be read
  unsigned int t0, t1;         // segments: tile columns / tile rows of an entry; columns: t0 tile columns
  unsigned int parts;          // parts per entry, 0: an empty entry (no stage one)
  int p0;                      // segments, columns: log2 of the lanes per row
  int reals;                   // reals per element: 1, or 2 for the complex types
  int n_fields;
  int stream;                  // 1 non-temporal loads (KernelChoice::access), 0 default caching
  int final_lanes_log2;        // stage two: log2 of the lanes per entry (0 or 6)
};
static_assert(sizeof(ProfileGeom) + sizeof(ReduceFields) + 8 <= 2048, "geometry, the two tables of fields and the workspace stay well under the 4 KB of kernel arguments");

// ---- plane updates of a box of cells along one dim (kernels_planes.hip; interior plane updates, include/cudecomp_interior_planes.h) --
// The profile's adjoint: every cell of the box is updated IN PLACE with the coefficient of its index k along the kept dim,
// u <- u + c or u <- u * c, c = scale * the pair at coef[2 * (f * ld + k)] rounded once to the real type.  One stage, no workspace; a
// launch stores the bytes of the box's cells and no others.
constexpr int kPlanesAdd = 0, kPlanesMul = 1;  // CUDECOMP_AMD_PLANES_*
struct PlanesGeom {
  long long L;                 // entries per field: the extent of the kept dim
  long long sk;                // rows, element-wise: BYTES between two entries
  long long row_bytes;         // rows: a row of the contiguous dim; columns: a row of the kept dim (L elements)
  long long rows;              // rows: rows of one entry; columns: all rows of the box, e1 * e2
  long long e1, e2;            // columns, element-wise: the two other extents, e1 the one of the smaller stride
  long long s1, s2;            // their strides in BYTES (rows: s1 between the rows of an entry); columns: multiples of 16
  long long rows_per_part;     // columns: part p walks the rows [p * rows_per_part, (p + 1) * rows_per_part)
  long long slots;             // rows, columns: 16-byte slots a row can touch at most
  long long box_off;           // bytes from a field's pointer to the first cell of the box
  long long rd_lo, rd_hi;      // the bytes [rd_lo, rd_hi) relative to the first cell of the box may be read
  long long ld;                // pairs of doubles between the coefficient rows of two fields; 0: all fields share row 0
  double scale;                // the host factor of every coefficient
  unsigned int t0, t1;         // rows: tile columns / tile rows of an entry; columns: t0 tile columns
  unsigned int parts;          // rows, element-wise: parts per entry; columns: parts of the rows; 0: an empty box (no launch)
  int p0;                      // rows, columns: log2 of the lanes per row
  int reals;                   // reals per element: 1, or 2 for the complex types
  int n_fields;
  int stream;                  // 1 non-temporal loads and stores (KernelChoice::access), 0 default caching
  int op;                      // kPlanesAdd, kPlanesMul
};
struct PlanesFields {
  char* a[kMaxFields];
};
static_assert(sizeof(PlanesGeom) + sizeof(PlanesFields) + 8 <= 2048, "geometry, the table of fields and the coefficients stay well under the 4 KB of kernel arguments");

// ---- combinations of two boxes of cells (kernels_combine.hip; interior combinations, include/cudecomp_interior_combine.h) ----------
// y <- a * x + b * y over the same box of x[f] and y[f], the coefficients ratios of doubles in device memory:
// a = (a_scale * a_num[2i + c]) / a_den[2i], i = f * coef_stride, rounded once to the real type; b likewise.  The reduction's geometry
// (ReduceGeom's rows, planes and tiles; a long single row cut into rows of kReduceChunkBytes); one stage, no workspace; a launch
// stores the bytes of the cells of y's box and no others.
constexpr int kCombineAxpy = 0, kCombineXpby = 1, kCombineAxpby = 2, kCombineAx = 3;  // CUDECOMP_AMD_COMBINE_*
// workgroups per field the planner aims at: eight per CU of an MI355X, the most that are resident with four waves each (DESIGN.md
// section 4)
constexpr int kCombineBlocks = 2048;
struct CombineGeom {
  // rows: bytes; the last row of every plane may be shorter (a cut row).  element-wise: unused
  long long row_bytes, last_row_bytes, rows, planes, s1, s2;
  long long slots;             // rows: 16-byte slots a row can touch at most
  unsigned long long tiles;    // rows: t0 * t1 * planes
  unsigned int t0, t1;         // rows: tile columns / tile rows per plane
  long long e[3], s[3];        // element-wise: extents and strides in ELEMENTS
  long long box_off;           // bytes from a field's pointer to the first cell of the box
  long long rd_lo, rd_hi;      // rows: the bytes [rd_lo, rd_hi) relative to the first cell of the box may be read, of x[f] and of y[f] alike
  double a_scale, b_scale;     // the host factors of the two coefficients
  int p0;                      // rows: log2 of the lanes per row; element-wise: the dim the lanes run along
  int reals;                   // reals per element: 1, or 2 for the complex types
  int n_fields;
  int stream;                  // rows: 1 non-temporal loads and stores (KernelChoice::access), 0 default caching
  int op;                      // kCombine*
  int coef_stride;             // 0: all fields share the pair 0 of every coefficient array; 1: field f takes pair f
  unsigned int blocks;         // workgroups PER FIELD; 0: an empty box (no launch)
};
struct CombineFields {
  char* y[kMaxFields];
  const char* x[kMaxFields];
};
// the four coefficient arrays (device memory, read when the kernel runs); a null `num` stands for the pair (1.0, 0.0), a null `den`
// for no division; the coefficient an op does not use is all null here, whatever the caller passed
struct CombineCoefs {
  const double* a_num;
  const double* a_den;
  const double* b_num;
  const double* b_den;
};
static_assert(sizeof(CombineGeom) + sizeof(CombineFields) + sizeof(CombineCoefs) <= 2048, "geometry, the two tables of fields and the coefficients stay well under the 4 KB of kernel arguments");

}  // namespace kern

// ---- what runs: one record per kernel choice ----------------------------------------------------------------------------------
// csrc/kernels.cc classify() fills it; the batching key, the launchers and the kernel's name (lastKernelName) all read it.
enum KernelKind {
  K_ROWS,                // rows_kernel
  K_ROWS_SHIFTED,        // rows_shifted_kernel: lanes on the destination's 64-byte grid
  K_ROWS_DENSE,          // rows_dense_kernel: whole lines across the row ends (Move3D::dst_row_pitch)
  K_TRANSPOSE,           // transpose_kernel
  K_TRANSPOSE_WINDOW,    // transpose_window_kernel: destination rows off the 64-byte grid
  K_TRANSPOSE_LINES,     // transpose_lines_kernel: windows over the linear positions of adjacent rows (128-byte units)
  K_TRANSPOSE_ROWLINES,  // transpose_rowlines_kernel: the tile's own rows are the adjacent ones (128-byte units)
  K_GENERIC,             // generic_kernel
  K_ROWS_ADD,            // rows_accumulate_kernel (dst += src)
  K_GENERIC_ADD,         // generic_accumulate_kernel
  K_ROWS_FILL,           // rows_fill_kernel (dst = value): lanes on the destination's 16-byte grid
  K_GENERIC_FILL,        // generic_fill_kernel
  K_ROWS_TAKE,           // rows_take_kernel (dst = src; src = 0)
  K_GENERIC_TAKE,        // generic_take_kernel
  K_ROWS_ADD_TAKE,       // rows_accumulate_take_kernel (dst += src; src = 0)
  K_GENERIC_ADD_TAKE,    // generic_accumulate_take_kernel
  K_ROWS_REFLECT,        // rows_reflect_kernel (dst = src or dst = -src, the source backwards along the row or plane index)
  K_GENERIC_REFLECT,     // generic_reflect_kernel
  K_ROWS_FOLD,           // rows_fold_kernel (dst += src or dst += -src, the source backwards along the row or plane index) = 18
  K_GENERIC_FOLD,        // generic_fold_kernel = 19
  K_ROWS_FOLD_TAKE,      // rows_fold_kernel with TAKE (... ; src = 0) = 20
  K_GENERIC_FOLD_TAKE,   // generic_fold_kernel with TAKE = 21
  K_ROWS_FIELDS,         // rows_fields_kernel (dst = src, one move of a FieldMoveBatch for every field) = 22
  K_GENERIC_FIELDS,      // generic_fields_kernel = 23
  K_TRANSPOSE_FIELDS,    // transpose_fields_kernel (LDS-tiled) = 24
  K_ROWS_FIELDS_ADD,          // rows_fields_accumulate_kernel (dst += src, one move of a FieldMoveBatch for every field) = 25
  K_GENERIC_FIELDS_ADD,       // generic_fields_accumulate_kernel = 26
  K_ROWS_FIELDS_TAKE,         // rows_fields_take_kernel (dst = src; src = 0) = 27
  K_GENERIC_FIELDS_TAKE,      // generic_fields_take_kernel = 28
  K_ROWS_FIELDS_ADD_TAKE,     // rows_fields_accumulate_kernel with TAKE (dst += src; src = 0) = 29
  K_GENERIC_FIELDS_ADD_TAKE,  // generic_fields_accumulate_kernel with TAKE = 30
  K_ROWS_FIELDS_REFLECT,      // rows_fields_reflect_kernel (dst = +-src per field, the source backwards along the row or plane index) = 31
  K_GENERIC_FIELDS_REFLECT,   // generic_fields_reflect_kernel = 32
  K_ROWS_FIELDS_FOLD,         // rows_fields_fold_kernel (dst += +-src per field, the source backwards) = 33
  K_GENERIC_FIELDS_FOLD,      // generic_fields_fold_kernel = 34
  K_ROWS_FIELDS_FOLD_TAKE,    // rows_fields_fold_kernel with TAKE (... ; src = 0) = 35
  K_GENERIC_FIELDS_FOLD_TAKE, // generic_fields_fold_kernel with TAKE = 36
  K_ROWS_WALL,                // rows_wall_kernel (dst = +-src + addend of the destination layer, the source backwards along the row or plane index) = 37
  K_GENERIC_WALL,             // generic_wall_kernel = 38
  K_ROWS_FIELDS_WALL,         // rows_fields_wall_kernel (dst = +-src per field + the field's addend of the destination layer) = 39
  K_GENERIC_FIELDS_WALL,      // generic_fields_wall_kernel = 40
  K_ROWS_WALL_PLANE,          // rows_wall_plane_kernel (dst = +-src + the plane entry of the destination cell, the source backwards along the row or plane index) = 41
  K_GENERIC_WALL_PLANE,       // generic_wall_plane_kernel = 42
  K_ROWS_REDUCE,              // reduce_rows_kernel (a box of cells to two fp64 partials per workgroup; no destination) = 43
  K_GENERIC_REDUCE,           // reduce_elements_kernel = 44
  K_ROWS_PROFILE,             // profile_rows_kernel (the kept dim not contiguous: an entry is a set of contiguous rows) = 45
  K_COLUMNS_PROFILE,          // profile_columns_kernel (the kept dim contiguous: a lane owns a 16-byte slot of the row and walks down the rows) = 46
  K_GENERIC_PROFILE,          // profile_elements_kernel = 47
  K_ROWS_PLANES,              // planes_rows_kernel (the kept dim not contiguous: one coefficient per row, read-modify-write on the 16-byte grid) = 48
  K_COLUMNS_PLANES,           // planes_columns_kernel (the kept dim contiguous: a lane owns a 16-byte slot of the row and its coefficients) = 49
  K_GENERIC_PLANES,           // planes_elements_kernel = 50
  K_ROWS_COMBINE,             // combine_rows_kernel (lanes on the 16-byte grid of x and y, which share their phase on it) = 51
  K_GENERIC_COMBINE           // combine_elements_kernel = 52
};
struct KernelChoice {
  KernelKind kind;
  int es;           // element size in bytes
  int vec;          // row and element-wise kinds: bytes per lane; transposes: elements per lane (1 = element-wise lanes)
  int ti, tj;       // transposes: the tile (elements, i x j); 0 otherwise
  int access;       // copies: 0 default caching, 2 non-temporal loads + stores, 3 non-temporal loads + remote (system-scope
                    // write-through) stores, 4 cached loads + non-temporal stores; additions: 0, 1 non-temporal source loads;
                    // fills: 0, 1 non-temporal stores; takes: 0, 1 non-temporal source loads and zero stores (plain take: all of it);
                    // reflections and wall-moves: 0, 1 non-temporal loads and stores; folds: 0, 1 non-temporal source loads and zero stores;
                    // reductions and profiles: 0, 1 non-temporal loads; plane updates and combinations: 0, 1 non-temporal loads and stores;
                    // field-moves: 0, 1 non-temporal loads and stores; transpose_fields_kernel: 0, 2; adding / taking
                    // field-moves: as additions / takes; mirrored field-moves: as reflections / folds; wall field-moves: as reflections
  ArithType arith;  // additions, folds, wall-moves, reflections that flip the sign bits, mirrored field-moves (whatever their signs):
                    // the real type the elements consist of; ARITH_NONE otherwise
  bool neg;         // folds, wall-moves: the sign bits of the source are flipped before the addition (one sign mask per launch)
  bool guard;       // transpose_fields_kernel: some tile of the move ends inside the move (the GUARD template argument); false otherwise
  bool operator==(const KernelChoice& o) const {
    return kind == o.kind && es == o.es && vec == o.vec && ti == o.ti && tj == o.tj && access == o.access && arith == o.arith &&
           neg == o.neg && guard == o.guard;
  }
};
constexpr int kLinesUnitBytes = 128;  // alignment unit of the lines and row-lines kernels

// Residency of the LDS-tiled transposes: the dynamic LDS (bytes) a launch asks for on top of its kernel's static tile.  No kernel
// references that memory; it only limits how many workgroups share a CU (160 KiB of LDS).  Pure host code (csrc/kernels.cc, where
// the rule and its measurements are); 0 for everything but the streaming transposes with a far-strided side it names.
int residencyPadBytes(const KernelChoice& k, const kern::Batch& b);
inline int residencyPadBytes(const KernelChoice&, const kern::FieldMoveBatch&) { return 0; }  // lists of field-moves: never

// How a normalized move is executed on the GPU: the three families KernelStats (kernels.h) counts; KernelKind names the kernel.
enum MoveClass {
  MOVE_ROWS_VEC = 0,   // rows contiguous on both sides: row copy or addition, 2 ... 16 B/lane (the widest the row length allows)
  MOVE_TRANSPOSE = 1,  // source rows along another dim than destination rows, both extents >= 4: LDS-tiled transposition
  MOVE_GENERIC = 2,    // anything else (no unit stride, 1-element rows, forced): element-wise
  MOVE_CLASS_COUNT = 3
};

// One row per KernelKind, in the order of the enum: the class of the kind and the rule by which it turns an access mode into the
// STREAM template argument of its kernels (kernels_dev.h, storePolicyOf).
enum StreamRule {
  STREAM_AS_ACCESS,    // the access mode itself
  STREAM_CACHED,       // always 0: the element-wise kernels of the local families
  STREAM_REMOTE_ONLY,  // 3 for remote destinations, else 0: the element-wise copy and addition
  STREAM_ROW_COPY,     // 3 remote, 1 any streaming mode, else 0: row copies stream loads and stores together
  STREAM_WINDOW        // 2 -> 4, else the mode: always cached loads, the overlap rows of neighbouring windows hit in L2
};
struct KindTraits {
  MoveClass cls;
  StreamRule stream;
};
constexpr KindTraits kKindTraits[] = {
    {MOVE_ROWS_VEC, STREAM_ROW_COPY},      // K_ROWS
    {MOVE_ROWS_VEC, STREAM_ROW_COPY},      // K_ROWS_SHIFTED
    {MOVE_ROWS_VEC, STREAM_ROW_COPY},      // K_ROWS_DENSE
    {MOVE_TRANSPOSE, STREAM_AS_ACCESS},    // K_TRANSPOSE
    {MOVE_TRANSPOSE, STREAM_WINDOW},       // K_TRANSPOSE_WINDOW
    {MOVE_TRANSPOSE, STREAM_WINDOW},       // K_TRANSPOSE_LINES
    {MOVE_TRANSPOSE, STREAM_WINDOW},       // K_TRANSPOSE_ROWLINES
    {MOVE_GENERIC, STREAM_REMOTE_ONLY},    // K_GENERIC
    {MOVE_ROWS_VEC, STREAM_AS_ACCESS},     // K_ROWS_ADD
    {MOVE_GENERIC, STREAM_REMOTE_ONLY},    // K_GENERIC_ADD
    {MOVE_ROWS_VEC, STREAM_AS_ACCESS},     // K_ROWS_FILL
    {MOVE_GENERIC, STREAM_CACHED},         // K_GENERIC_FILL
    {MOVE_ROWS_VEC, STREAM_AS_ACCESS},     // K_ROWS_TAKE
    {MOVE_GENERIC, STREAM_CACHED},         // K_GENERIC_TAKE
    {MOVE_ROWS_VEC, STREAM_AS_ACCESS},     // K_ROWS_ADD_TAKE
    {MOVE_GENERIC, STREAM_CACHED},         // K_GENERIC_ADD_TAKE
    {MOVE_ROWS_VEC, STREAM_AS_ACCESS},     // K_ROWS_REFLECT
    {MOVE_GENERIC, STREAM_CACHED},         // K_GENERIC_REFLECT
    {MOVE_ROWS_VEC, STREAM_AS_ACCESS},     // K_ROWS_FOLD
    {MOVE_GENERIC, STREAM_CACHED},         // K_GENERIC_FOLD
    {MOVE_ROWS_VEC, STREAM_AS_ACCESS},     // K_ROWS_FOLD_TAKE
    {MOVE_GENERIC, STREAM_CACHED},         // K_GENERIC_FOLD_TAKE
    {MOVE_ROWS_VEC, STREAM_AS_ACCESS},     // K_ROWS_FIELDS
    {MOVE_GENERIC, STREAM_CACHED},         // K_GENERIC_FIELDS
    {MOVE_TRANSPOSE, STREAM_AS_ACCESS},    // K_TRANSPOSE_FIELDS
    {MOVE_ROWS_VEC, STREAM_AS_ACCESS},     // K_ROWS_FIELDS_ADD
    {MOVE_GENERIC, STREAM_CACHED},         // K_GENERIC_FIELDS_ADD
    {MOVE_ROWS_VEC, STREAM_AS_ACCESS},     // K_ROWS_FIELDS_TAKE
    {MOVE_GENERIC, STREAM_CACHED},         // K_GENERIC_FIELDS_TAKE
    {MOVE_ROWS_VEC, STREAM_AS_ACCESS},     // K_ROWS_FIELDS_ADD_TAKE
    {MOVE_GENERIC, STREAM_CACHED},         // K_GENERIC_FIELDS_ADD_TAKE
    {MOVE_ROWS_VEC, STREAM_AS_ACCESS},     // K_ROWS_FIELDS_REFLECT
    {MOVE_GENERIC, STREAM_CACHED},         // K_GENERIC_FIELDS_REFLECT
    {MOVE_ROWS_VEC, STREAM_AS_ACCESS},     // K_ROWS_FIELDS_FOLD
    {MOVE_GENERIC, STREAM_CACHED},         // K_GENERIC_FIELDS_FOLD
    {MOVE_ROWS_VEC, STREAM_AS_ACCESS},     // K_ROWS_FIELDS_FOLD_TAKE
    {MOVE_GENERIC, STREAM_CACHED},         // K_GENERIC_FIELDS_FOLD_TAKE
    {MOVE_ROWS_VEC, STREAM_AS_ACCESS},     // K_ROWS_WALL
    {MOVE_GENERIC, STREAM_CACHED},         // K_GENERIC_WALL
    {MOVE_ROWS_VEC, STREAM_AS_ACCESS},     // K_ROWS_FIELDS_WALL
    {MOVE_GENERIC, STREAM_CACHED},         // K_GENERIC_FIELDS_WALL
    {MOVE_ROWS_VEC, STREAM_AS_ACCESS},     // K_ROWS_WALL_PLANE
    {MOVE_GENERIC, STREAM_CACHED},         // K_GENERIC_WALL_PLANE
    {MOVE_ROWS_VEC, STREAM_AS_ACCESS},     // K_ROWS_REDUCE
    {MOVE_GENERIC, STREAM_CACHED},         // K_GENERIC_REDUCE
    {MOVE_ROWS_VEC, STREAM_AS_ACCESS},     // K_ROWS_PROFILE
    {MOVE_ROWS_VEC, STREAM_AS_ACCESS},     // K_COLUMNS_PROFILE
    {MOVE_GENERIC, STREAM_CACHED},         // K_GENERIC_PROFILE
    {MOVE_ROWS_VEC, STREAM_AS_ACCESS},     // K_ROWS_PLANES
    {MOVE_ROWS_VEC, STREAM_AS_ACCESS},     // K_COLUMNS_PLANES
    {MOVE_GENERIC, STREAM_CACHED},         // K_GENERIC_PLANES
    {MOVE_ROWS_VEC, STREAM_AS_ACCESS},     // K_ROWS_COMBINE
    {MOVE_GENERIC, STREAM_CACHED},         // K_GENERIC_COMBINE
};
static_assert(sizeof(kKindTraits) / sizeof(kKindTraits[0]) == K_GENERIC_COMBINE + 1, "one row per KernelKind");

// the row of a kind; a value outside the enum is an internal error, never a read past the table
inline const KindTraits& kindTraits(KernelKind kind) {
  if (kind < K_ROWS || kind > K_GENERIC_COMBINE) CD_INTERNAL_ERROR("kernel kind out of range");
  return kKindTraits[kind];
}
inline MoveClass classOf(KernelKind kind) { return kindTraits(kind).cls; }

// the STREAM template argument with which a kind of kernel serves an access mode
inline int streamArgOf(KernelKind kind, int access) {
  switch (kindTraits(kind).stream) {
    case STREAM_AS_ACCESS: return access;
    case STREAM_CACHED: return 0;
    case STREAM_REMOTE_ONLY: return access == 3 ? 3 : 0;
    case STREAM_WINDOW: return access == 2 ? 4 : access;
    case STREAM_ROW_COPY: break;
  }
  return access == 3 ? 3 : (access >= 1 ? 1 : 0);
}

// ---- launchers, one per code object (host side; csrc/kernels.cc decides what runs): each selects its instantiation from the
// record and fails with an internal error when there is none.
void launchRowsBatch(const KernelChoice& k, const kern::Batch& b, unsigned int blocks, hipStream_t stream);  // K_ROWS*, K_GENERIC
int rowsDenseBytesPerBlock();  // bytes of a plane's span one workgroup of the dense row copy covers
// kernels_transpose.hip: 2-, 4- and 8-byte elements use the XOR-swizzled LDS tile, 16-byte elements the padded one
void launchTransposeBatch2(const KernelChoice& k, const kern::Batch& b, unsigned int blocks, hipStream_t stream);
void launchTransposeBatch4(const KernelChoice& k, const kern::Batch& b, unsigned int blocks, hipStream_t stream);
void launchTransposeBatch8(const KernelChoice& k, const kern::Batch& b, unsigned int blocks, hipStream_t stream);
void launchTransposeBatch16(const KernelChoice& k, const kern::Batch& b, unsigned int blocks, hipStream_t stream);
void launchWindowBatch(const KernelChoice& k, const kern::Batch& b, unsigned int blocks, hipStream_t stream);
void launchLinesBatch(const KernelChoice& k, const kern::Batch& b, unsigned int blocks, hipStream_t stream);
void launchRowLinesBatch(const KernelChoice& k, const kern::Batch& b, unsigned int blocks, hipStream_t stream);
// kernels_accumulate.hip: add-moves (dst += src).  Rows: the Batch of rows_kernel.  Generic: extents / strides in elements.
void launchAccumulateBatch(const KernelChoice& k, const kern::Batch& b, unsigned int blocks, hipStream_t stream);
// kernels_fill.hip: fill-moves (dst = value).  `pattern`: the 16 bytes every 16-byte-aligned slot of the destination receives
// -- the element replicated; it travels as a kernel argument of its own.  Rows: e[0] = 16-byte slots per row (upper bound),
// ss[0] = row bytes, ds[1], ds[2] in bytes.  Generic: extents / strides in elements.
struct FillPattern {
  unsigned int w[4];
};
void launchFillBatch(const KernelChoice& k, const kern::Batch& b, const FillPattern& pattern, unsigned int blocks, hipStream_t stream);
// kernels_take.hip: take-moves (the copy or the addition, then src = 0).  The Batch of the row copies / additions and of their
// generic forms; local buffers only.
void launchTakeBatch(const KernelChoice& k, const kern::Batch& b, unsigned int blocks, hipStream_t stream);
// kernels_reflect.hip: reflect-moves (dst = src or dst = -src with the source running backwards along one dim).  Rows: the Batch of
// rows_kernel with SIGNED byte strides ss[1], ss[2] (the mirror is folded into them).  Generic: extents / strides in elements,
// signed.  k.arith != ARITH_NONE: the sign bit of every real of that type is inverted; the mask travels as a 16-byte kernel
// argument of its own.  Local buffers only.
struct SignMask {
  unsigned int w[4];
};
// the sign bit of every real of `arith` in 16 bytes (little endian): 2-byte reals 0x8000 in every half word, 4-byte reals the top
// bit of every word, 8-byte reals the top bit of every second word; all zero without a real type
inline SignMask signMaskOf(ArithType arith) {
  switch (arith) {
    case ARITH_F16:
    case ARITH_BF16: return {{0x80008000u, 0x80008000u, 0x80008000u, 0x80008000u}};
    case ARITH_F32: return {{0x80000000u, 0x80000000u, 0x80000000u, 0x80000000u}};
    case ARITH_F64: return {{0u, 0x80000000u, 0u, 0x80000000u}};
    default: return {{0, 0, 0, 0}};
  }
}
void launchReflectBatch(const KernelChoice& k, const kern::Batch& b, unsigned int blocks, hipStream_t stream);
// kernels_fold.hip: fold-moves (dst += src or dst += -src with the source running backwards along one dim; the TAKE kinds then
// store zero bytes to the source cells).  The Batch of the reflections: rows with SIGNED byte strides ss[1], ss[2], generic with
// signed strides in elements.  k.arith: the real type of the addition; k.neg: the sign mask of that type travels as a 16-byte
// kernel argument of its own, all zero otherwise.  Local buffers only.
void launchFoldBatch(const KernelChoice& k, const kern::Batch& b, unsigned int blocks, hipStream_t stream);
// kernels_wall.hip: wall-moves (Move3D::affine: dst = src + a or dst = -src + a with the source running backwards along one dim, a the
// addend of the destination's layer along that dim).  The Batch of the reflections (rows with SIGNED byte strides, generic with
// signed strides in elements) with Batch::p1 naming the mirrored entry of e[]; k.arith: the real type of the addition, always;
// k.neg: the sign bits of the source are flipped first.  `table`: the addends in destination order (kernels.cc wallTableOf reverses
// the low side, so the kernels pay nothing for the mirror).  Lanes never narrower than one element.  Local buffers only.
// WallAddends is what a caller of launchMoves hands over: per side (0 low, 1 high) the converted element of every ghost layer k,
// counted from the wall outward, its `es` bytes at the start of a 16-byte slot.
struct WallAddends {
  unsigned char v[2][kern::kMaxWallHalo][16];
};
void launchWallBatch(const KernelChoice& k, const kern::Batch& b, const kern::WallTable& table, unsigned int blocks, hipStream_t stream);
// kernels_wall_plane.hip: wall-plane moves (Move3D::plane: dst = src + plane or dst = -src + plane with the source running backwards
// along one dim, the plane entry that of the destination cell).  The Batch of the reflections (rows with SIGNED byte strides,
// generic with signed strides in elements); `planes`: the third operand of every move in the same units.  k.arith: the real type of
// the addition, always; k.neg: the sign bits of the source are flipped first.  Lanes never narrower than one element.  Local buffers
// only.  WallPlanes is what a caller of launchMoves hands over: the base of the low and of the high plane (device memory).
struct WallPlanes {
  const void* base[2];
};
void launchWallPlaneBatch(const KernelChoice& k, const kern::Batch& b, const kern::PlaneOperands& planes, unsigned int blocks,
                          hipStream_t stream);
// kernels_field_transpose.hip: lists of field-moves (plain copies of exactly the cells of the moves; local buffers only)
void launchFieldMoveBatch(const KernelChoice& k, const kern::FieldMoveBatch& b, unsigned int blocks, hipStream_t stream);
// kernels_field_accumulate.hip: lists of field-moves that add (k.arith: the real type), take or both; local buffers only
void launchFieldAccumulateBatch(const KernelChoice& k, const kern::FieldMoveBatch& b, unsigned int blocks, hipStream_t stream);
// kernels_field_mirror.hip: lists of mirrored field-moves (reflect- or fold-moves: SIGNED source strides, rows in bytes, generic in
// elements).  k.arith: the real type of the elements, always; bit f of fields_neg: the sign bits of field f's source are flipped on
// the way (the mask of that type and fields_neg travel as kernel arguments of their own).  Local buffers only.
void launchFieldMirrorBatch(const KernelChoice& k, const kern::FieldMoveBatch& b, unsigned int fields_neg, unsigned int blocks,
                            hipStream_t stream);
// kernels_field_wall.hip: lists of wall field-moves (reflect-moves with Move3D::affine: SIGNED source strides, rows in bytes, generic
// in elements).  k.arith: the real type of the addition, always; bit f of fields_neg: the sign bits of field f's source are flipped
// first; `table` and `walk` as above.  Lanes never narrower than one element.  Local buffers only.
void launchFieldWallBatch(const KernelChoice& k, const kern::FieldMoveBatch& b, unsigned int fields_neg, const kern::FieldWallTable& table,
                          const kern::FieldWallWalk& walk, unsigned int blocks, hipStream_t stream);
// kernels_reduce.hip (in the unit kernels_edge.hip): reductions of a box of cells.  Stage one: k.kind K_ROWS_REDUCE or K_GENERIC_REDUCE,
// k.arith the real type, `op` one of kern::kReduce*; g.blocks * g.n_fields workgroups, each writing its pair of partials to `work`.
// Stage two: one workgroup per field combines `partials` pairs (0: an empty box) and writes results[2f], results[2f + 1].
void launchReduceStageOne(const KernelChoice& k, int op, const kern::ReduceGeom& g, const kern::ReduceFields& fields, double* work,
                          hipStream_t stream);
void launchReduceFinal(int op, int n_fields, unsigned int partials, double* results, const double* work, hipStream_t stream);
// kernels_profile.hip (in the units kernels_window.hip and kernels_rows.hip): profiles of a box of cells along one dim.  Stage one:
// k.kind K_ROWS_PROFILE, K_COLUMNS_PROFILE or K_GENERIC_PROFILE, k.arith the real type, `op` one of kern::kReduce*; each workgroup
// writes its partials to `work`.  Stage two: a lane (or a wave, g.final_lanes_log2) per (field, entry) combines g.parts pairs (0: +0.0)
// and writes results[2 * (f * ld + k)] and the double after it.
void launchProfileRows(const KernelChoice& k, int op, const kern::ProfileGeom& g, const kern::ReduceFields& fields, double* work,
                       hipStream_t stream);
void launchProfileColumnsOrElements(const KernelChoice& k, int op, const kern::ProfileGeom& g, const kern::ReduceFields& fields,
                                    double* work, hipStream_t stream);
void launchProfileFinal(int op, const kern::ProfileGeom& g, double* results, long long ld, const double* work, hipStream_t stream);
// kernels_planes.hip (in the units kernels_lines.hip and kernels_rowlines.hip): plane updates of a box of cells along one dim, in
// place.  k.kind K_ROWS_PLANES, or K_COLUMNS_PLANES / K_GENERIC_PLANES; k.arith the real type; g.op, g.scale and g.ld with `coef`
// (device memory, read when the kernel runs) say what is added or multiplied.
void launchPlanesRows(const KernelChoice& k, const kern::PlanesGeom& g, const kern::PlanesFields& fields, const double* coef,
                      hipStream_t stream);
void launchPlanesColumnsOrElements(const KernelChoice& k, const kern::PlanesGeom& g, const kern::PlanesFields& fields, const double* coef,
                                   hipStream_t stream);
// kernels_combine.hip (in the four units of kernels_transpose.hip): y <- a * x + b * y over a box of cells.  k.kind K_ROWS_COMBINE
// (launchCombineRows2 / 4 / 8: the real types of 2, 4 and 8 bytes, one unit each) or K_GENERIC_COMBINE (launchCombineElements: every
// type); k.arith the real type; g.op, the scales and `coefs` (device memory, read when the kernel runs) say what is combined.
void launchCombineRows2(const KernelChoice& k, const kern::CombineGeom& g, const kern::CombineFields& fields, const kern::CombineCoefs& coefs,
                        hipStream_t stream);
void launchCombineRows4(const KernelChoice& k, const kern::CombineGeom& g, const kern::CombineFields& fields, const kern::CombineCoefs& coefs,
                        hipStream_t stream);
void launchCombineRows8(const KernelChoice& k, const kern::CombineGeom& g, const kern::CombineFields& fields, const kern::CombineCoefs& coefs,
                        hipStream_t stream);
void launchCombineElements(const KernelChoice& k, const kern::CombineGeom& g, const kern::CombineFields& fields, const kern::CombineCoefs& coefs,
                           hipStream_t stream);
// kernels_rotate.hip: in-place rotation of a cubic n^3 array (direction +1: new[p0,p1,p2] = old[p2,p0,p1]; -1: the inverse)
bool rotateSupported(int es, long long n);
void launchRotate(void* buffer, long long n, int es, int direction, hipStream_t stream);

}  // namespace cudecomp
