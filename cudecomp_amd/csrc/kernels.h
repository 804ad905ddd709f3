// kernels.h -- host entry points of the HIP data-movement kernels (kernels.cc: classification and batching; kernels_batch.h:
// the record of a kernel choice and the list of code objects the kernels live in).
#pragma once
#include <hip/hip_runtime_api.h>

#include <vector>

#include "kernels_batch.h"
#include "plan.h"

namespace cudecomp {

// (MoveClass, the three families KernelStats counts: kernels_batch.h, beside the table that gives every KernelKind its class)
struct KernelStats {  // filled per launch when requested (tests, bench bookkeeping)
  int launches[MOVE_CLASS_COUNT] = {0, 0, 0};
  i64 elements[MOVE_CLASS_COUNT] = {0, 0, 0};
};

struct KernelTuning {
  int force_class = -1;          // tests / CUDECOMP_FORCE_GENERIC_KERNELS: force MOVE_GENERIC (2) to cross-check the fast paths
  bool no_streaming = false;     // never use non-temporal access (CUDECOMP_DISABLE_STREAMING_ACCESS=1)
  bool force_streaming = false;  // tests: non-temporal access regardless of the move size
  int walk_order = -1;           // tests: transposes walk tiles i first (0) / j first (1, without runs); -1 = by strides
  int dense_rows = -1;           // moves of whole rows onto halo-carrying pencils: 0 = never rewrite the halo / padding cells between
                                 // consecutive rows (no rows_dense_kernel, no transpose_lines_kernel / transpose_rowlines_kernel: the shifted / window kernels
                                 // instead); CUDECOMP_PRESERVE_OUTPUT_HALOS=1
  int window_mode = -1;          // tests: transposes onto rows off the 64-byte grid: -1 window kernel for moves >= 1 MiB, 0 never, 1 always
};

// Execute `n` independent moves (disjoint destinations) of `es`-byte elements.  bufs[BufId] are the
// device pointers of the input / output / workspace buffers.  Asynchronous on `stream`.
// Copy moves (Move3D::add == false) need nothing else.  Add-moves (dst += src; kernels_accumulate.hip) need `arith`, the real
// type the elements consist of (arithOf(dtype), internal.h), and a local destination; they run as row or element-wise
// additions over exactly the cells of the move -- never the transposing, shifted, dense or window forms.
// Fill-moves (Move3D::fill: dst = value; kernels_fill.hip) take `fill_value`, one element of `es` bytes read before the call
// returns (nullptr: all-zero bytes), and a local destination; they run as row or element-wise fills that store exactly the
// cells of the move and load nothing.
// Take-moves (Move3D::take, copy or add; kernels_take.hip) store zero bytes to the source cells they have read: local buffers
// only, sources disjoint from all destinations and from each other; row or element-wise forms over exactly the cells of the move.
// Reflect-moves (Move3D::reflect: the source runs backwards along one dim; kernels_reflect.hip) copy between disjoint cells of a
// local buffer, as rows or element-wise, over exactly the cells of the move; with Move3D::negate they need `arith`, the real
// type whose sign bits are flipped.
// Fold-moves (Move3D::reflect with Move3D::add; kernels_fold.hip) add the source, running backwards along one dim, onto disjoint
// cells of the same local buffer, with its sign bits flipped first under Move3D::negate, and clear it under Move3D::take; they
// always need `arith`.
// Wall-moves (Move3D::affine on a reflect-move; kernels_wall.hip) add the addend of the destination's layer along the mirrored dim
// after the optional sign flip, in `arith`, which they always need.  `wall_addends` holds the converted addends of the call per
// side and ghost layer (kernels_batch.h WallAddends), read before the call returns; a move names its side.  At most
// kern::kMaxWallHalo layers; anything else on such a move is an internal error before any launch.
// Wall-plane moves (Move3D::plane on a reflect-move; kernels_wall_plane.hip) add, after the optional sign flip and in `arith`, which
// they always need, the entry of a device array that Move3D::plane_off and Move3D::ps name for the destination cell.  `wall_planes`
// holds the bases of the call's low and high plane (kernels_batch.h WallPlanes); only the POINTERS are read here, the contents when
// the kernel runs.  Any number of layers; anything else on such a move is an internal error before any launch.
void launchMoves(const Move3D* moves, int n, void* const bufs[3], int es, hipStream_t stream,
                 const KernelTuning* tuning = nullptr, KernelStats* stats = nullptr,
                 void* const* dst_base_override = nullptr,  // per-move destination base (remote buffers)
                 ArithType arith = ARITH_NONE, const void* fill_value = nullptr, const WallAddends* wall_addends = nullptr,
                 const WallPlanes* wall_planes = nullptr);

// One row of the addend table a launch of wall-moves carries (kern::WallTable): `layers` entries of 16 bytes in DESTINATION order
// along the mirrored dim -- the high side's (side 1) ghost layer k at index k, the low side's (side 0) at layers - 1 - k -- each the
// `es`-byte element replicated; the rest zero.  Pure host code.
void wallTableRow(const WallAddends& addends, int side, int layers, int es, unsigned char out[kern::kMaxWallHalo * 16]);

// One kernel launch of a list of moves: what runs, its descriptor, its workgroups (the padded count of an interleaved launch)
// and which entries of the list it serves.
struct Launch {
  KernelChoice k;
  kern::Batch b;
  kern::PlaneOperands planes;    // wall-plane moves: planes.m[i] is the third operand of b.m[i] (zero otherwise)
  unsigned int blocks;
  MoveClass cls;
  i64 elements;                  // of all its moves
  int index[kern::kMaxBatch];    // index[i]: the list entry b.m[i] is
};
// WHICH launches launchMoves makes for a list, in order (pure host code, no device needed; the arguments are launchMoves's):
// empty moves dropped, the rest regrouped by equal KernelChoice in the order of first appearance, groups cut at kMaxBatch
// moves and before the move whose workgroups would take the sum past 2^31 - 1, interleaved when there are several moves that
// are no local transposes.  Throws what launchMoves throws, before anything is launched.
std::vector<Launch> planLaunches(const Move3D* moves, int n, void* const bufs[3], int es, const KernelTuning* tuning = nullptr,
                                 void* const* dst_base_override = nullptr, ArithType arith = ARITH_NONE,
                                 const WallPlanes* wall_planes = nullptr);

// How a move WOULD run (no launch, no device needed): class, kernel variant, tile, tile counts, walk parameters, access mode.
// out[10] = {class, variant, tile_i (row copies: 0 plain / 1 shifted / 2 dense kernel), tile_j, tiles_i, tiles_j, batch, p0 (run length), p1 (walk bits: 1 XCD-contiguous, 2 j first,
// 4 runs over batch planes, 8 transpose_lines_kernel, 16 transpose_rowlines_kernel), access mode}.  (Tests of the planning logic: tests/test_kernel_plan.py.)
void describeMove(const Move3D& m, const void* src, void* dst, int es, const KernelTuning* tuning, long long out[10]);

// ---- lists of field-moves: a list of moves, each for several (input, output) pairs of buffers (kernels_field_transpose.hip,
// kernels_field_accumulate.hip, kernels_field_mirror.hip, kernels_field_wall.hip) ----
// The request: the moves of one phase of a multi-field transpose (include/cudecomp_transpose_fields.h) or of a multi-field halo call
// (include/cudecomp_halo_fields.h and its siblings), which share their geometry among the fields.  The planners and the launcher
// below take nothing else.  A list that breaks a rule marked (internal error) is refused before anything is launched.
struct FieldMoveList {
  // moves[0 .. n - 1].  Each move's shared geometry is classified once: rows (rowVectors' rule) when its fastest dim is contiguous on
  // both sides, the LDS-tiled transposition (chooseTranspose's lane-width rule, one tile per element size and lane width) when source
  // and destination rows run along different dims of at least 4 elements, element by element (genericGeometry's) otherwise.  Moves
  // with equal KernelChoice share a launch, in the order of first appearance, cut at kMaxBatch moves (and before 2^31 - 1
  // workgroups).  The kernels copy exactly the cells of the moves -- never a window, lines, shifted or dense form: a move with fill,
  // negate or dst_row_pitch is an internal error; a move of more than 2^31 - 1 workgroups is NOT_SUPPORTED.
  // The OPERATION of a list (kernels_field_accumulate.hip) is what its moves carry, the same on every move (internal error): copy
  // (neither flag), add (Move3D::add: dst += src in `arith`, with the operand order of the single accumulation), take (Move3D::take:
  // dst = src; src = 0) or add-take (both).  Adding and taking lists run as rows or element by element, never transposed, over
  // exactly the cells of their moves; sources are disjoint from all destinations.  An add whose destination is the workspace and a
  // take whose source is the workspace are internal errors.
  const Move3D* moves = nullptr;
  int n = 0;
  // the fields' pieces of a workspace end: an end of moves[i] in BUF_WORK lies at work + (offset + f * work_steps[i]) elements for
  // field f (nullptr: all zero; a negative step is an internal error)
  const i64* work_steps = nullptr;
  // n_fields (1 .. kern::kMaxFields) fields: an end of a move in BUF_IN lies in inputs[f] + offset, an end in BUF_OUT in
  // outputs[f] + offset.  No null entry; an output end without `outputs` is an internal error.  Buffers are only looked at as
  // addresses by the planners.  For 2-byte elements the lanes narrow as soon as ANY field's address, any workspace piece or any
  // stride is 2 mod 4.
  void* const* inputs = nullptr;
  void* const* outputs = nullptr;
  int n_fields = 0;
  void* work = nullptr;  // a workspace end without a workspace is an internal error
  int es = 0;            // element size in bytes: 2, 4, 8 or 16
  // the real type the elements consist of: needed by adding lists and, always, by mirrored ones (whose sign mask is that of the
  // type); one the element size does not fit is an internal error
  ArithType arith = ARITH_NONE;
  // the phases of a halo call (their one or two sides): ONE kernel choice serves the list, hence one launch -- rows only when every
  // move has contiguous rows, then the narrowest of the moves' lane widths; never the transposition; non-temporal access when the
  // LARGEST move reaches kStreamBytes per field.  More than 2^31 - 1 workgroups in all are then NOT_SUPPORTED, not a second launch.
  bool one_choice = false;
  // MIRRORED lists (kernels_field_mirror.hip: the one or two sides of a multi-field reflection or fold,
  // include/cudecomp_halo_wall_fields.h): every move is a reflect-move (Move3D::reflect: one dim with a negative source stride,
  // src_off at the source cell of its index 0) or a fold-move (with Move3D::add, and Move3D::take when it clears its source), both
  // ends in the fields' own buffers.  Move3D::negate is NOT used: the signs travel in fields_neg and are no part of the kernel
  // choice, so one plan and one kernel serve every combination of parities.  Each move is classified as the single calls classify
  // it (rows when the fastest dim is contiguous on both sides and not the mirrored one, element by element otherwise -- lanes along
  // the longest dim when there is no destination-fast one -- never transposed).  Without `mirrored` a reflect-move, a sign or a
  // negative stride is an internal error; with it a move that is no reflect-move, carries negate, fill or dst_row_pitch, touches
  // the workspace or takes without adding is one.
  bool mirrored = false;
  // mirrored lists: bit f says that the sign bits of field f's source are flipped on the way (parity -1); a bit of a field the list
  // does not have, or any bit of a list that is not mirrored, is an internal error
  unsigned int fields_neg = 0;
  // WALL lists (kernels_field_wall.hip: the one or two sides of a multi-field wall-value call,
  // include/cudecomp_halo_wall_value_fields.h): non-null exactly for them.  moves[0 .. n - 1], n <= 2, are wall-moves (Move3D::reflect
  // with Move3D::affine naming the side, no Move3D::negate) between cells of the fields' own buffers; addends[f] holds field f's
  // converted addends per side and ghost layer (WallAddends, kernels_batch.h), read before the call returns.  Such a list is planned
  // as a mirrored list with one_choice, whatever those two members say; its fields are `inputs`, and `outputs`, `work` and
  // `work_steps` are not read.
  // Launch rule: with S the moves that have cells, h the layers (the extent of the mirrored dim) and es the element size, one launch
  // serves F = min(kern::kMaxFields, kern::kFieldWallTableBytes / (S * h * es)) consecutive fields -- what its compact addend table
  // holds -- and the list makes ceil(n_fields / F) launches in field order.
  const WallAddends* addends = nullptr;
  // Of the tuning the lists read three switches (nullptr: none set): force_class == MOVE_GENERIC the element-wise kernel,
  // force_streaming non-temporal access regardless of the size, no_streaming cached access regardless of the size (and of
  // force_streaming).  Access otherwise, unmeasured for these kernels: copies are cached while a move is below kStreamBytes PER
  // FIELD, non-temporal loads and stores from there; adding and taking lists follow the accumulation's rule by the same size --
  // non-temporal source loads and, with take, non-temporal zero stores (the plain take: all of it), the destination of an add
  // always cached; mirrored and wall lists the reflection's / the fold's rule.  The element-wise kernels always cache.
  const KernelTuning* tuning = nullptr;
};
struct FieldMoveLaunch {
  KernelChoice k;
  kern::FieldMoveBatch b;
  unsigned int blocks;            // of all its moves and fields
  unsigned int blocks_per_field;  // of all its moves
  unsigned int fields_neg;        // mirrored lists: the fields whose sign bits are flipped (0 otherwise)
  MoveClass cls;
  i64 elements;                   // of all its moves and fields
  int index[kern::kMaxBatch];     // index[i]: the list entry b.m[i] is
  int along[kern::kMaxBatch];     // wall field-moves: the entry of b.m[i].e[] whose index is the destination layer (-1 otherwise)
};
// WHICH launches launchFieldMoveList makes for a list that is no wall list, in order (pure host code, no device needed; `addends` is
// not read)
std::vector<FieldMoveLaunch> planFieldMoveLaunches(const FieldMoveList& list);

struct FieldWallLaunch {
  FieldMoveLaunch l;           // its fields are fields[first_field .. first_field + l.b.n_fields)
  kern::FieldWallTable table;  // entry (move i of the launch, field f of the launch, destination layer j) at ((i * nf + f) * h + j) * es
  kern::FieldWallWalk walk;
  int first_field;
};
int fieldsPerWallLaunch(int sides, int layers, int es);  // F of the wall lists' launch rule
// WHICH launches launchFieldMoveList makes for a wall list, in order (pure host code, no device needed): per run of F fields the one
// launch planFieldMoveLaunches gives the sides, with the run's addend table
std::vector<FieldWallLaunch> planFieldWallLaunches(const FieldMoveList& list);

// Launch the list, asynchronous on `stream`: planFieldMoveLaunches' launches, or planFieldWallLaunches' for a wall list.
void launchFieldMoveList(const FieldMoveList& list, hipStream_t stream, KernelStats* stats = nullptr);

// ---- reductions of a box of cells (kernels_reduce.hip; include/cudecomp_interior_reduce.h) --------------------------------------
// The request: the same box of `es`-byte elements of every field a[f] (and b[f], DOT only), reduced to two doubles per field.
// Buffers are only looked at as addresses by the planner.
struct ReduceRequest {
  const void* const* a = nullptr;  // n_fields (1 .. kern::kMaxFields) fields, no null entry
  const void* const* b = nullptr;  // DOT: the second operands, b[f] == a[f] allowed; not read otherwise
  int n_fields = 0;
  int op = 0;                      // kern::kReduceSum, kReduceDot, kReduceMaxAbs
  int es = 0;                      // element size in bytes
  ArithType arith = ARITH_NONE;    // the real type the elements consist of (one or two of them)
  i64 extent[3] = {0, 0, 0};       // the box, in elements; strides non-negative
  i64 strides[3] = {0, 0, 0};
  i64 box_off = 0;                 // elements from a field's pointer to the first cell of the box
  // what may be read: the bytes [-readable_before, span + readable_after) around the box, span = the bytes from its first cell to
  // the end of its last; the same for every field
  i64 readable_before = 0, readable_after = 0;
  const KernelTuning* tuning = nullptr;  // force_class == MOVE_GENERIC the element-wise kernel; force_streaming, no_streaming
};
// HOW a request runs (pure host code, no device needed).  Rows -- lanes on the 16-byte grid of memory -- when the box has a
// contiguous dim, every field sits on a boundary of its real type, DOT operands share their phase on the 16-byte grid and complex DOT
// fields sit on element boundaries; element by element otherwise.  Contiguous dims are merged first (rowVectors' rule for copies),
// and a box that is one long row is cut into rows of kern::kReduceChunkBytes.  Non-temporal loads from kStreamBytes per field on.
struct ReducePlan {
  KernelChoice k;       // kind K_ROWS_REDUCE / K_GENERIC_REDUCE; vec = bytes per lane (16 / one element); access 0, 1
  kern::ReduceGeom g;   // g.blocks: stage-one workgroups per field, 0 for an empty box
  i64 read_lo, read_hi; // lowest byte read and one past the highest, relative to the first cell of field 0's box (0, 0: empty box)
};
ReducePlan planReduce(const ReduceRequest& r);
// Launch it, asynchronous on `stream`: stage one (unless the box is empty) into `work` (reduceWorkspaceBytes(n_fields) bytes of
// device memory), stage two into results[0 .. 2 * n_fields).  Nothing is allocated, nothing waits.
void launchReduce(const ReduceRequest& r, double* results, void* work, hipStream_t stream, KernelStats* stats = nullptr);
inline i64 reduceWorkspaceBytes(int n_fields) { return (i64)n_fields * kern::kReduceMaxBlocks * 2 * (i64)sizeof(double); }

// ---- profiles of a box of cells along one dim (kernels_profile.hip; include/cudecomp_interior_profile.h) ------------------------
// The request: ReduceRequest's box, reduced over two of its dims and KEPT along extent[keep]: extent[keep] pairs of doubles per field.
struct ProfileRequest {
  const void* const* a = nullptr;  // n_fields (1 .. kern::kMaxFields) fields, no null entry
  const void* const* b = nullptr;  // DOT: the second operands; not read otherwise
  int n_fields = 0;
  int op = 0;                      // kern::kReduceSum, kReduceDot, kReduceMaxAbs
  int es = 0;                      // element size in bytes
  ArithType arith = ARITH_NONE;    // the real type the elements consist of
  i64 extent[3] = {0, 0, 0};       // the box, in elements; strides non-negative
  i64 strides[3] = {0, 0, 0};
  int keep = 0;                    // the dim of the box that is kept, 0 .. 2
  i64 box_off = 0;                 // elements from a field's pointer to the first cell of the box
  i64 readable_before = 0, readable_after = 0;  // as ReduceRequest's
  const KernelTuning* tuning = nullptr;         // force_class == MOVE_GENERIC the element-wise kernel; force_streaming, no_streaming
};
// HOW a request runs (pure host code, no device needed).  The contiguous dim is the one of stride 1 (of several, one longer than a
// cell).  Fields on a boundary of their real type, DOT operands at one phase of the 16-byte grid, complex DOT fields on element
// boundaries (planReduce's rules) and:
//   the kept dim is not the contiguous one                                     -> K_ROWS_PROFILE (an entry is a set of contiguous rows)
//   it is, and both other dims longer than a cell have pitches of 16 bytes' multiples -> K_COLUMNS_PROFILE (a lane per 16-byte slot of the row)
//   anything else, or forced                                                   -> K_GENERIC_PROFILE (element by element)
// g.parts parts per entry: at most kern::kProfileMaxParts and at most max(1, kern::kProfilePairsPerField / L), so parts * L pairs of
// partials per field fit profileWorkspaceBytes(n_fields, L).  Dims are not merged: an entry's rows stay the rows of the box.
struct ProfilePlan {
  KernelChoice k;        // kind K_ROWS_PROFILE / K_COLUMNS_PROFILE / K_GENERIC_PROFILE; vec = bytes per lane (16 / one element); access 0, 1
  kern::ProfileGeom g;   // g.L entries; g.parts == 0: no stage one (L == 0: no launch at all; an empty entry: zeros are written)
  i64 blocks;            // stage-one workgroups per field
  i64 read_lo, read_hi;  // lowest byte read and one past the highest, relative to the first cell of field 0's box (0, 0: nothing read)
};
ProfilePlan planProfile(const ProfileRequest& r);
// Launch it, asynchronous on `stream`: stage one into `work` (profileWorkspaceBytes(n_fields, extent[keep]) bytes of device memory),
// stage two into results[2 * (f * ld + k)], k < extent[keep] <= ld.  Nothing is allocated, nothing waits; extent[keep] == 0: no launch.
void launchProfile(const ProfileRequest& r, double* results, i64 ld, void* work, hipStream_t stream, KernelStats* stats = nullptr);
inline i64 profileWorkspaceBytes(int n_fields, i64 length) {
  return (i64)n_fields * (length > kern::kProfilePairsPerField ? length : (i64)kern::kProfilePairsPerField) * 2 * (i64)sizeof(double);
}

// ---- plane updates of a box of cells along one dim (kernels_planes.hip; include/cudecomp_interior_planes.h) ----------------------
// The request: ProfileRequest's box of every field a[f], updated IN PLACE with the coefficient of each cell's index k along
// extent[keep]: u <- u + c (kern::kPlanesAdd) or u <- u * c (kern::kPlanesMul), c = scale * the pair at coef[2 * (f * ld + k)]
// rounded once to the real type (real types: the first double alone; complex: (re, im), MUL the complex product).
struct PlanesRequest {
  void* const* a = nullptr;        // n_fields (1 .. kern::kMaxFields) fields, no null entry, no two equal
  int n_fields = 0;
  int op = 0;                      // kern::kPlanesAdd, kPlanesMul
  int es = 0;                      // element size in bytes
  ArithType arith = ARITH_NONE;    // the real type the elements consist of
  i64 extent[3] = {0, 0, 0};       // the box, in elements; strides non-negative
  i64 strides[3] = {0, 0, 0};
  int keep = 0;                    // the dim of the box whose index picks the coefficient, 0 .. 2
  i64 box_off = 0;                 // elements from a field's pointer to the first cell of the box
  i64 readable_before = 0, readable_after = 0;  // as ReduceRequest's
  i64 ld = 0;                      // pairs between the coefficient rows of two fields, >= extent[keep]; 0: every field takes row 0
  double scale = 1.0;
  const KernelTuning* tuning = nullptr;         // force_class == MOVE_GENERIC the element-wise kernel; force_streaming, no_streaming
};
// HOW a request runs (pure host code, no device needed).  planProfile's rules: the contiguous dim is the one of stride 1 (of several,
// one longer than a cell); fields on a boundary of their real type -- for the complex product, of their element -- and:
//   the kept dim is not the contiguous one                                     -> K_ROWS_PLANES (one coefficient per row)
//   it is, and both other dims longer than a cell have pitches of 16 bytes' multiples -> K_COLUMNS_PLANES (a lane per 16-byte slot of the row)
//   anything else, or forced                                                   -> K_GENERIC_PLANES (element by element)
// Non-temporal loads and stores from kStreamBytes per field on.  One launch serves all fields; an empty box makes none.
struct PlanesPlan {
  KernelChoice k;          // kind K_ROWS_PLANES / K_COLUMNS_PLANES / K_GENERIC_PLANES; vec = bytes per lane (16 / one element); access 0, 1
  kern::PlanesGeom g;      // g.parts == 0: an empty box, no launch
  i64 blocks;              // workgroups per field
  i64 read_lo, read_hi;    // lowest byte read and one past the highest, relative to the first cell of field 0's box (0, 0: nothing read)
  i64 write_lo, write_hi;  // lowest byte stored and one past the highest, likewise: 0 and the box's span, whatever the form
};
PlanesPlan planPlanes(const PlanesRequest& r);
// Launch it, asynchronous on `stream`; `coef` is device memory whose CONTENTS are read when the kernel runs.  Nothing is allocated,
// nothing waits; an empty box: no launch.
void launchPlanes(const PlanesRequest& r, const double* coef, hipStream_t stream, KernelStats* stats = nullptr);

// ---- combinations of two boxes of cells (kernels_combine.hip; include/cudecomp_interior_combine.h) -------------------------------
// The request: ReduceRequest's box of every field y[f], overwritten with a * x[f] + b * y[f] (kern::kCombineAxpy: a * x + y,
// kCombineXpby: x + b * y, kCombineAxpby, kCombineAx: a * x, y never read); a = (a_scale * a_num[2i + c]) / a_den[2i], i = f *
// coef_stride, rounded once to the real type, b likewise; a null num stands for (1.0, 0.0), a null den for no division.  Buffers are
// only looked at as addresses by the planner.
struct CombineRequest {
  void* const* y = nullptr;        // n_fields (1 .. kern::kMaxFields) fields, no null entry, no two equal
  const void* const* x = nullptr;  // as many; equal entries allowed, none equal to an entry of y
  int n_fields = 0;
  int op = 0;                      // kern::kCombineAxpy, kCombineXpby, kCombineAxpby, kCombineAx
  int es = 0;                      // element size in bytes
  ArithType arith = ARITH_NONE;    // the real type the elements consist of
  i64 extent[3] = {0, 0, 0};       // the box, in elements; strides non-negative; the same in x[f] and y[f]
  i64 strides[3] = {0, 0, 0};
  i64 box_off = 0;                 // elements from a field's pointer to the first cell of the box
  i64 readable_before = 0, readable_after = 0;  // as ReduceRequest's, of x[f] and of y[f] alike
  double a_scale = 1.0, b_scale = 1.0;
  int coef_stride = 0;             // 0: all fields share pair 0; 1: field f takes pair f
  const KernelTuning* tuning = nullptr;         // force_class == MOVE_GENERIC the element-wise kernel; force_streaming, no_streaming
};
// HOW a request runs (pure host code, no device needed).  Rows -- lanes on the 16-byte grid of memory, K_ROWS_COMBINE -- when the box
// has a contiguous dim, every x[f] and y[f] sits on a boundary of its real type (complex types: of its element) and x[f] and y[f]
// share their phase on the 16-byte grid; element by element (K_GENERIC_COMBINE) otherwise, or forced.  Contiguous dims are merged by
// planReduce's rules, and a box that is one long row is cut into rows of kern::kReduceChunkBytes.  Non-temporal loads and stores from
// kStreamBytes per field on.  One launch serves all fields; an empty box makes none.
struct CombinePlan {
  KernelChoice k;              // kind K_ROWS_COMBINE / K_GENERIC_COMBINE; vec = bytes per lane (16 / one element); access 0, 1
  kern::CombineGeom g;         // g.blocks == 0: an empty box, no launch
  i64 blocks;                  // workgroups per field
  i64 read_x_lo, read_x_hi;    // lowest byte of x[0] read and one past the highest, relative to the first cell of its box (0, 0: nothing read)
  i64 read_y_lo, read_y_hi;    // the same of y[0]; AX: 0, 0
  i64 write_lo, write_hi;      // lowest byte of y[0] stored and one past the highest, likewise: 0 and the box's span, whatever the form
};
CombinePlan planCombine(const CombineRequest& r);
// Launch it, asynchronous on `stream`; the four arrays are device memory whose CONTENTS are read when the kernel runs, those of the
// coefficient the op does not use are not passed on.  Nothing is allocated, nothing waits; an empty box: no launch.
void launchCombine(const CombineRequest& r, const double* a_num, const double* a_den, const double* b_num, const double* b_den,
                   hipStream_t stream, KernelStats* stats = nullptr);

// data-movement launches this process has made so far (launchMoves, launchFieldMoveList, both stages of launchReduce and launchProfile, launchPlanes and launchCombine; tests count launches per call with it)
long long dataLaunchCount();

// name (template spelling) of the data-movement kernel launched last by this process, "" before the first launch
const char* lastKernelName();

// ---- sync.hip: device-side signals of the one-sided exchanges ------------------------------------------------
constexpr int kMaxFlags = 64;  // one lane per flag
struct FlagList {
  int n = 0;
  unsigned long long* f[kMaxFlags];
  void add(unsigned long long* p) { f[n++] = p; }
};
// Flags hold  call number * kFlagScale + step  (monotonic): step 0 = the call has begun, 1 .. kFlagScale-2 = that many
// stages of a staged exchange have landed, kFlagDone = everything of the call has landed.
constexpr unsigned long long kFlagScale = 16;
constexpr int kFlagBegun = 0, kFlagDone = (int)kFlagScale - 1;
// epoch (device memory) += 1; every flag of `begun` = epoch * kFlagScale
void launchEpochBegin(unsigned long long* epoch, const FlagList& begun, hipStream_t stream);
// every flag = *epoch * kFlagScale + step
void launchSignal(const unsigned long long* epoch, const FlagList& flags, hipStream_t stream, int step = kFlagDone);
// returns (on the stream) when every flag >= *epoch * kFlagScale + step; after timeout_s seconds writes a code to *status
// and gives up
void launchWait(const unsigned long long* epoch, const FlagList& flags, unsigned long long* status, double timeout_s,
                hipStream_t stream, int step = kFlagDone);

// stamp / verify the first word of every 4-KiB page of a shared buffer (see sync.hip)
void launchTagPages(void* base, size_t bytes, unsigned long long seed, hipStream_t stream);
void launchCheckPages(const void* base, size_t bytes, unsigned long long seed, unsigned long long* bad, hipStream_t stream);
// debug aid: out2[0] += sum of the 32-bit words of [p, p + bytes), out2[1] += position-weighted sum (mod 2^64); a tail of 1 - 3
// bytes counts as one more word, zero-extended, at index bytes / 4 (no byte past p + bytes is read); bytes == 0: no launch
void launchChecksum(const void* p, size_t bytes, unsigned long long* out2, hipStream_t stream);

}  // namespace cudecomp
