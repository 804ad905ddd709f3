// kernels.cc -- host side of the data-movement kernels: how a Move3D (plan.h) is executed on the GPU.
//
// A move is normalised (unit dims dropped, contiguous dims fused, dims sorted by source stride) and classified: classify()
// writes WHAT runs into one KernelChoice (kernels_batch.h: the kind of kernel -- row copy plain / shifted / dense, LDS-tiled
// transposition plain / window / lines / row lines, element-wise, the two additions, the two fills, the four takes, the two reflections, the four folds, the two wall-moves, the two wall-plane moves -- element size, lane width,
// tile, access mode) and HOW it walks into the Batch fields beside it.  Moves with equal choices are batched (up to kMaxBatch moves, e.g.
// the per-peer pack copies of one transpose, share one launch; the descriptors travel in the kernel argument segment).  The
// batching key, the launcher's instantiation and the kernel's name all come from that one record.  The kernels live in
// kernels_rows.hip, kernels_transpose.hip (one code object per element size), kernels_window.hip, kernels_lines.hip,
// kernels_rowlines.hip, kernels_accumulate.hip, kernels_fill.hip, kernels_take.hip, kernels_reflect.hip, kernels_fold.hip, kernels_wall.hip and kernels_wall_plane.hip; kernels_rotate.hip (the in-place rotation) is launched by the executor,
// transpose.cc; kernels_field_transpose.hip (lists of field-moves: the moves of a halo or transpose phase for several pencils in
// one launch), kernels_field_accumulate.hip (the same lists adding or taking: multi-field halo accumulation) and
// kernels_field_mirror.hip (the same lists mirrored, with a sign per field: multi-field wall halos) have an entry of their own at
// the end of this file, launchFieldMoveList.  kernels_batch.h says why they are separate
// code objects.
//
// 2-byte elements (fp16, bf16) take the row copy (plain kernel), the LDS-tiled transposition (128 x 128 tiles with 16-byte
// lanes, 64 x 64 element-wise) and the generic kernel only: never the window, lines, row-lines, shifted-rows, dense-rows or
// rotation kernels, whose 2-byte forms are not written (the row kernels copy row ends in 4-byte pieces).  Their accesses of 4
// bytes or more are issued only at dword-aligned addresses: the vector width follows from the base addresses and the byte
// strides, not only from the extents.
//
// Pure data movement: no MFMA; the bound is HBM (8 TB/s spec, ~6.3 TB/s achievable copy rate).
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "errors.h"
#include "kernels.h"
#include "kernels_batch.h"

namespace cudecomp {

using namespace kern;

namespace {

// ---------------------------------------------------------------------------------------------
// classification
// ---------------------------------------------------------------------------------------------
struct Classified {
  KernelChoice k;  // what runs
  DevMove dm;      // ... and how: the move in the kernel's units, the walk (Batch::p0 / p1), the tile counts
  int p0, p1;
  unsigned int t0, t1;
  unsigned long long blocks;
  i64 elements;
  PlaneOperand po;  // wall-plane moves: the third operand in the kernel's units (zero otherwise)
};

constexpr long long kDenseMaxGapBytes = 512;  // widest gap between rows the dense row copy rewrites (halo + padding cells)

int arithBytes(int arith) { return arith == ARITH_F64 ? 8 : (arith == ARITH_F32 ? 4 : 2); }

int ilog2ceil(long long x) {
  int l = 0;
  while ((1LL << l) < x) ++l;
  return l;
}

// 2-byte elements: accesses of 4 bytes or more only at dword-aligned addresses -- both bases and every stride (elements, or-ed
// together) the lanes step by.  A row that starts at 2 mod 4 (odd halo, extent or offset) is moved in 2-byte pieces.
bool halfMisaligned(const DevMove& dm, int es, long long strides) {
  return es == 2 && ((reinterpret_cast<uintptr_t>(dm.src) | reinterpret_cast<uintptr_t>(dm.dst) | (uintptr_t)(strides * es)) & 3) != 0;
}

// Rows contiguous on both sides (also the all-extents-1 case), copied or added.  Widest vector, of at most `widest` bytes, that
// divides the row length; addresses only need the element's natural alignment (see GlobalBytes).
void rowVectors(Classified& c, const Move3D& m, int widest = 16) {
  const int es = c.k.es;
  int vb = widest;
  while (vb > es && (m.extent[0] * es) % vb != 0) vb >>= 1;
  if (halfMisaligned(c.dm, es, m.ss[1] | m.ss[2] | m.ds[1] | m.ds[2])) vb = 2;
  c.k.vec = vb;
  c.dm.e[0] = m.extent[0] * es / vb;
  c.dm.e[1] = m.extent[1];
  c.dm.e[2] = m.extent[2];
  for (int i = 1; i < 3; ++i) {
    c.dm.ss[i] = m.ss[i] * es;
    c.dm.ds[i] = m.ds[i] * es;
  }
}

// lanes per row (p0 = their log2) and workgroups of rows_kernel, rows_shifted_kernel and rows_accumulate_kernel
void rowTiles(Classified& c) {
  c.p0 = std::min(8, ilog2ceil(c.dm.e[0]));
  const long long lpr = 1LL << c.p0, rows_per_block = (long long)(kThreads >> c.p0) * kRowsUnroll;
  c.t0 = (unsigned int)((c.dm.e[0] + lpr - 1) / lpr);
  c.t1 = (unsigned int)((c.dm.e[1] + rows_per_block - 1) / rows_per_block);
  c.blocks = (unsigned long long)c.t0 * c.t1 * (unsigned long long)c.dm.e[2];
}

// element-wise, copied or added: lanes along the destination-fast dim when there is one; without one along dim 0, or
// (along_longest: reflections and folds, whose mirrored dim never sits in slot 0) along the longest dim
void genericGeometry(Classified& c, const Move3D& m, bool along_longest = false) {
  c.k.vec = c.k.es;
  c.p0 = -1;
  for (int i = 0; i < 3; ++i) {
    c.dm.e[i] = m.extent[i];
    c.dm.ss[i] = m.ss[i];
    c.dm.ds[i] = m.ds[i];
    if (m.ds[i] == 1 && m.extent[i] > 1) c.p0 = i;
  }
  if (c.p0 < 0) {
    c.p0 = 0;
    for (int i = 1; along_longest && i < 3; ++i)
      if (m.extent[i] > m.extent[c.p0]) c.p0 = i;
  }
  const unsigned long long want = ((unsigned long long)c.elements + kThreads - 1) / kThreads;
  c.blocks = std::min<unsigned long long>(std::max<unsigned long long>(want, 1), 8192);
}

// Rows that land off the 64-byte grid (and are long enough for it to matter): lanes laid out from the unit boundary
// below each row's start (rows_shifted_kernel), one unit of slack vectors per row.  Not for 2-byte elements: the shifted
// and dense kernels copy the row ends in 4-byte pieces (so no rows_dense_kernel either)
bool offerShiftedRows(Classified& c, const Move3D& m, const KernelTuning& tuning) {
  const int es = c.k.es;
  const uintptr_t dst_bits = reinterpret_cast<uintptr_t>(c.dm.dst) | (uintptr_t)c.dm.ds[1] | (uintptr_t)c.dm.ds[2];
  const int shift_mode = tuning.window_mode;  // -1 auto, 0 never, 1 whenever the destination is misaligned
  if (es == 2 || (dst_bits & 63) == 0 || m.extent[0] * es < 256 || shift_mode == 0 || (shift_mode != 1 && c.elements * es < (1ll << 20)))
    return false;
  c.p1 = (int)(m.extent[0] * es);  // row length in bytes (rows longer than 2 GiB keep the plain kernel, which does not read it)
  if (m.extent[0] * es > 0x7fffffffLL) return false;
  c.k.kind = K_ROWS_SHIFTED;
  return true;
}

// ... and when the move covers whole interior rows of a halo-carrying pencil (the planner says so and names the pencil's
// row pitch: dst_row_pitch) and the gap between consecutive rows is a few halo / padding cells: the dense walk of
// rows_dense_kernel, which writes whole lines across the row ends.  Local destinations only; dim 1 must be the one that
// steps by the pencil's row pitch (a move one row tall per plane has no such dim: its rows are whole planes apart, with
// other moves' rows in between).  A row that normalizeMove has fused with the next dim -- no gap -- keeps the shifted kernel.
bool offerDenseRows(Classified& c, const Move3D& in, const Move3D& m, const KernelTuning& tuning, bool remote) {
  const int es = c.k.es;
  i64 planned_row = -1;
  for (int i = 0; i < 3; ++i)
    if (in.ss[i] == 1 && in.ds[i] == 1 && in.extent[i] > 1) planned_row = in.extent[i];
  if (in.dst_row_pitch <= 0 || remote || planned_row != m.extent[0] || c.dm.e[1] <= 1 || tuning.dense_rows == 0) return false;
  DevMove d = c.dm;
  if (d.e[2] > 1 && d.ds[2] < d.ds[1]) {
    std::swap(d.e[1], d.e[2]);
    std::swap(d.ss[1], d.ss[2]);
    std::swap(d.ds[1], d.ds[2]);
  }
  const long long row_bytes = m.extent[0] * es, gap = d.ds[1] - row_bytes;
  const long long span = (d.e[1] - 1) * d.ds[1] + row_bytes;
  const bool planes_apart = d.e[2] == 1 || span <= d.ds[2];
  if (d.e[1] <= 1 || d.ds[1] != in.dst_row_pitch * es || gap <= 0 || gap > kDenseMaxGapBytes || gap * 8 > row_bytes || !planes_apart)
    return false;
  c.k.kind = K_ROWS_DENSE;
  c.k.vec = 16;
  c.dm = d;
  c.dm.e[0] = row_bytes;
  c.p0 = 0;
  const long long per = rowsDenseBytesPerBlock();
  c.t0 = (unsigned int)((span + 63 + per - 1) / per);  // (+63: the lanes start at the 64-byte boundary below the first row)
  c.t1 = 1;
  c.blocks = (unsigned long long)c.t0 * (unsigned long long)c.dm.e[2];
  return true;
}

// Lane width (elements) of a transposition whose geometry is in c.dm: 16 bytes per lane whenever both tile edges hold whole
// vectors (dword alignment suffices, see GlobalBytes).  2-byte elements: only when every lane address is dword-aligned too --
// bases and the byte strides of both sides
int transposeLaneWidth(const Classified& c) {
  const int es = c.k.es;
  int vw = 16 / es;
  if (c.dm.e[0] % vw != 0 || c.dm.e[1] % vw != 0) vw = 1;
  if (halfMisaligned(c.dm, es, c.dm.ss[1] | c.dm.ss[2] | c.dm.ds[0] | c.dm.ds[2])) vw = 1;
  return vw;
}

// Kernel (plain or window), lane width, access mode, tile and tile counts of a transposition whose geometry is in c.dm; also
// j_first (tile walk along the destination rows first) and aligned (plain kernel, both sides' rows on the 128-byte grid).
void chooseTranspose(Classified& c, const KernelTuning& tuning, bool& j_first, bool& aligned) {
  const int es = c.k.es;
  const int vw = transposeLaneWidth(c);
  c.k.vec = vw;
  // Tile walk order inside an XCD's run: j first makes consecutive tiles extend the same DESTINATION rows
  // (contiguous write stream per row), i first the same source rows.  Measured on 8 GiB permutations
  // (profiles/r01_tuning.md): j first wins or ties for line-aligned moves (8-11 % at 16-byte elements and on
  // the strided-read side at 4-byte elements; 4-byte moves whose destination rows are the far-strided side
  // lose 1-3 % and keep i first), i first wins by 5-10 % for misaligned moves, where L2 merges the
  // partially read lines of neighbouring tiles.
  // (2-byte elements: the rule of 4-byte ones, whose 16-byte-lane tile has the same shape in bytes)
  j_first = (es != 4 && es != 2) || c.dm.ss[1] > c.dm.ds[0];
  // Rows that do not start on cache-line boundaries (halo-shifted or odd-extent pencils) leave partially covered
  // lines at both ends of every tile row.
  //  * Misaligned SOURCE rows only: the partially used lines are shared with the neighbouring tile; cached loads let
  //    L2 serve the second use (non-temporal loads fetch them twice), the aligned stores keep streaming.
  //  * Misaligned DESTINATION rows: partial 64-byte units written by two tiles are what costs (a cached store lets L2
  //    merge some: fp32 3.0 -> 4.4 TB/s, fp64 3.9 -> 4.8 TB/s on a halo-shifted 8 GiB permutation); the window kernel
  //    writes whole units instead (4.8 -> 5.1-5.3 TB/s), with streaming stores.
  const uintptr_t src_bits = reinterpret_cast<uintptr_t>(c.dm.src) | (uintptr_t)(c.dm.ss[1] * es) | (uintptr_t)(c.dm.ss[2] * es);
  const uintptr_t dst_bits = reinterpret_cast<uintptr_t>(c.dm.dst) | (uintptr_t)(c.dm.ds[0] * es) | (uintptr_t)(c.dm.ds[2] * es);
  const uintptr_t align_req = 128;
  const bool src_mis = src_bits % align_req != 0, dst_mis = dst_bits % 64 != 0;
  const int window_mode = tuning.window_mode;  // -1 auto, 0 never, 1 whenever the destination is misaligned
  // 2-byte elements never take the window kernel, nor therefore transpose_lines_kernel / transpose_rowlines_kernel: their
  // 2-byte forms are not written; the plain kernel writes misaligned destinations correctly
  const bool window = es != 2 && dst_mis && window_mode != 0 && (window_mode == 1 || c.elements * es >= (1ll << 20));
  c.k.kind = window ? K_TRANSPOSE_WINDOW : K_TRANSPOSE;
  if (window) {
    if (c.k.access == 2) c.k.access = 4;  // cached loads (the overlap rows hit in L2), streaming whole-unit stores
    j_first = true;
  } else if (src_mis || dst_bits % align_req != 0) {
    if (c.k.access == 2) {
      if (dst_bits % align_req != 0) c.k.access = 0;
      else c.k.access = 4;
    }
    j_first = false;
  }
  // One measured outlier: 16-byte elements whose destination batch stride is not a multiple of 4 KiB (rows padded by a
  // cache line) lose a third of their rate with streaming stores (8 GiB permutation: 4.0 ms streaming, 3.4 ms cached;
  // 4- and 8-byte elements with the same padding prefer streaming, profiles/r02_tuning.md).
  if (es == 16 && c.k.access == 2 && !window && c.dm.e[2] > 1 && ((uintptr_t)(c.dm.ds[2] * es) % 4096) != 0) c.k.access = 0;
  if (tuning.walk_order >= 0) j_first = tuning.walk_order == 1;  // (tests)
  aligned = !window && !src_mis && dst_bits % align_req == 0;
  // The tile (elements, i x j) -- 2-byte: 128 x 128 with 16-byte lanes, 64 x 64 element-wise; 4- and 8-byte: 64 x 64; 16-byte:
  // 32 x 32 -- is twice as long along j in three cases:
  // (window kernel, 4-byte elements: 64 x 128 tiles -- a 64-byte unit is 16 elements, the longer window halves the
  // share of overlap rows)
  // 4-byte elements, 16-byte lanes, plain kernel: 64 x 128 tiles (512-byte destination segments; measured on
  // the 8-GiB fp32 cycle, profiles/r04_tuning.md: 11.22 ms against 11.69 for 64 x 64 and 128 x 64)
  // Large line-aligned moves whose SOURCE rows are the far-strided side (the inverse hops of an axis-contiguous cycle): twice
  // as many source rows per tile, 1-KiB destination segments.  Measured on the 8-GiB permutations (profiles/r05_tuning.md):
  // fp64 64 x 128 2.69 -> 2.65 ms, complex128 32 x 64 2.70 -> 2.66 ms; the forward hops lose with these tiles and keep theirs.
  const bool far_src = aligned && c.k.access == 2 && c.dm.ss[1] > 8 * c.dm.ds[0];
  bool longer = es == 4 && (window || vw == 4);
  if (far_src && ((es == 8 && vw == 2) || es == 16)) longer = true;
  c.k.ti = es == 2 ? (vw == 8 ? 128 : 64) : (es == 16 ? 32 : 64);
  c.k.tj = es == 2 ? c.k.ti : (longer ? 2 : 1) * c.k.ti;
  c.t0 = (unsigned int)((c.dm.e[0] + c.k.ti - 1) / c.k.ti);
  c.t1 = (unsigned int)((c.dm.e[1] + (window ? 64 / es - 1 : 0) + c.k.tj - 1) / c.k.tj);
}

// Far-strided DESTINATION (the forward hops of an axis-contiguous cycle: destination rows e.g. 8 MiB apart, source rows
// near): walk j in RUNS -- kRunBytes of every destination row of a tile row, then the next tile row, then the next run.
// The workgroups in flight on an XCD then write a few long contiguous runs (64 rows x 256 KiB) instead of one short run
// in very many rows (plain j first) or 512-byte pieces of 1024 rows (i first).  When the rows of consecutive batch planes
// are adjacent in the destination the planner has fused them into j (normalizeMove), so a run spans planes; if they are
// not fused (padded planes) the run is over batch planes instead (kWalkRunOverPlanes).  Measured on the 8-GiB permutations,
// two boxes (profiles/r05_tuning.md): fp64 2.91-2.93 -> 2.81 ms, complex128 2.99 -> 2.86, fp32 2.89 -> 2.86; runs of
// 128 KiB ... 2 MiB are within 1 %.
void offerRunWalk(Classified& c, const KernelTuning& tuning, bool aligned, bool& j_first) {
  const int es = c.k.es, tj = c.k.tj;
  const bool far_dst = aligned && c.k.access == 2 && c.dm.ds[0] > 8 * c.dm.ss[1];
  if (!far_dst || tuning.walk_order >= 0) return;
  constexpr long long kRunBytes = 256 << 10;
  const long long want = std::max<long long>(1, kRunBytes / ((long long)tj * es));  // tiles of one run
  if ((long long)c.t1 >= 2 * want) {  // runs of tiles along j
    long long run = want;
    while (run > 1 && c.t1 % run != 0) --run;  // (a divisor of the tile count: the walk stays a plain mixed-radix number)
    if (run >= want / 4 && run >= 4) {
      c.p0 = (int)run;
      j_first = true;
    }
  } else if (c.dm.e[2] > 1 && c.dm.ds[2] < c.dm.ds[0] && (long long)c.t1 * tj * es <= (64 << 10)) {  // runs of batch planes
    long long run = std::max<long long>(1, kRunBytes / std::max<long long>(1, c.dm.ds[2] * es));
    while (run > 1 && c.dm.e[2] % run != 0) --run;
    if (run >= 4) {
      c.p0 = (int)run;
      c.p1 |= kWalkRunOverPlanes;
      j_first = true;
    }
  }
}

// Destination rows off the 64-byte grid AND the rows of consecutive batch planes adjacent in memory (forward hops of an
// axis-contiguous cycle onto a halo-carrying pencil): every row begins and ends inside a cache line whose other part
// belongs to the next plane -- for the window kernel another workgroup, much later; the partly written lines cost the
// forward hops a sixth of their rate (0.60 against 0.72 of the HBM peak, profiles/r05_tuning.md section 3).  When the
// planner says the move covers whole interior rows of the pencil (dst_row_pitch: the gap cells are then halo / padding
// cells nobody else writes during the operation, the contract of rows_dense_kernel) j and k are fused into the slab's
// linear positions and the windows run ACROSS the row ends (transpose_lines_kernel, kernels_lines.hip).
bool offerLines(Classified& c, i64 planned_row, i64 row_pitch) {
  const int es = c.k.es, tj = c.k.tj;
  constexpr int ub = kLinesUnitBytes;
  const long long ej = c.dm.e[1], ek = c.dm.e[2], dk = c.dm.ds[2], gap = dk - ej;
  const long long span = (ek - 1) * dk + ej;
  if (ek <= 1 || planned_row != ej || dk != row_pitch || gap <= 0 || gap * es > kDenseMaxGapBytes || gap * 8 > ej ||
      c.dm.ds[0] < span || span >= (1ll << 30) || c.dm.e[0] >= (1ll << 30) || dk < tj + ub / es)
    return false;
  c.k.kind = K_TRANSPOSE_LINES;
  // 16-byte lanes need whole vectors along i only: the windows run over linear positions, whatever the row length
  c.k.vec = (es < 16 && c.dm.e[0] % (16 / es) == 0) ? 16 / es : 1;
  c.t1 = (unsigned int)((span + ub / es - 1 + tj - 1) / tj);  // windows along the linear positions (+ one unit of phase slack)
  // Tile walk (kernels_lines.hip): groups of 16 tile rows; inside a group short runs of 2 KiB per slab (four windows of
  // 8-byte elements) for all its rows, then the next run -- the source is read plane by plane in whole rows, every
  // slab's write stream advances steadily.  Wider moves (several groups: more than 1024 slabs) take runs of 32 KiB.
  // Measured on two boxes, fp64 forward hops onto halo pencils (profiles/r06_tuning.md): 1024^3 halo 1 window kernel
  // 3.52 ms -> 3.14 (2 KiB; 32 KiB 3.19-3.29, 256 KiB 3.45-3.77); config 5's pencil X->Y (2048 slabs) 1.72-1.77 -> 1.55-1.61
  // (32 KiB; 2 KiB 1.66), Y->Z (260-element rows) 1.81 -> 1.66 (2 KiB; 32 KiB 1.79-1.86).
  constexpr long long kGroup = 16;
  const bool several_groups = kGroup < (long long)c.t0;
  const long long run_kib = several_groups ? 32 : 2;
  const long long run = std::max<long long>(1, (run_kib << 10) / ((long long)tj * es));
  c.p0 = (long long)c.t1 >= 2 * run ? (int)run : 0;
  c.p1 = kWalkXcd | kWalkJFirst | kWalkLines;  // along the destination first
  if (several_groups) c.p1 |= (int)(kGroup << kWalkGroupShift);
  c.blocks = (unsigned long long)c.t0 * c.t1;
  return true;
}

// ... and the other orientation: the tile's OWN rows i are the adjacent ones (inverse hops of the cycle, unpack-side
// permutations; batch planes far apart).  The line at the end of row i holds the gap and the head of row i + 1 -- the
// same tile column of the next row: a row's last window runs on into it (transpose_rowlines_kernel, kernels_rowlines.hip).
bool offerRowLines(Classified& c, i64 planned_row, i64 row_pitch) {
  const int es = c.k.es, tj = c.k.tj;
  constexpr int ub = kLinesUnitBytes;
  const long long ei = c.dm.e[0], ej = c.dm.e[1], ek = c.dm.e[2], di = c.dm.ds[0], dk = c.dm.ds[2], rgap = di - ej;
  if (planned_row != ej || di != row_pitch || rgap <= 0 || rgap * es > kDenseMaxGapBytes || rgap * 8 > ej ||
      ej <= 2 * (tj + ub / es) || ei < 2 || ei >= (1ll << 30) || di >= (1ll << 30) || (ek != 1 && dk < (ei - 1) * di + ej))
    return false;
  c.k.kind = K_TRANSPOSE_ROWLINES;
  c.k.vec = (es < 16 && ei % (16 / es) == 0) ? 16 / es : 1;
  c.t1 = (unsigned int)((di - 1 + ub / es - 1) / tj + 1);  // windows per row: through the one that holds the last gap cell
  c.p0 = 0;
  c.p1 = kWalkXcd | kWalkJFirst | kWalkRowLines;  // windows first
  c.blocks = (unsigned long long)c.t0 * c.t1 * (unsigned long long)ek;
  return true;
}

// Dims (i, j, k) of a transposition: i the source's unit-stride dim (0 of the normalised move), j the destination's (t), k the other
void transposeGeometry(Classified& c, const Move3D& m, int t) {
  const int k = 3 - t;
  c.dm.e[0] = m.extent[0];
  c.dm.e[1] = m.extent[t];
  c.dm.e[2] = m.extent[k];
  c.dm.ss[0] = 1;
  c.dm.ss[1] = m.ss[t];
  c.dm.ss[2] = m.ss[k];
  c.dm.ds[0] = m.ds[0];
  c.dm.ds[1] = 1;
  c.dm.ds[2] = m.ds[k];
}

// LDS-tiled transposition: dim t of the normalised move is the destination's unit-stride dim
void classifyTranspose(Classified& c, const Move3D& in, const Move3D& m, int t, const KernelTuning& tuning, bool remote) {
  transposeGeometry(c, m, t);
  bool j_first, aligned;
  chooseTranspose(c, tuning, j_first, aligned);
  c.p0 = 0;
  c.p1 = kWalkXcd;
  offerRunWalk(c, tuning, aligned, j_first);
  if (j_first) c.p1 |= kWalkJFirst;
  c.blocks = (unsigned long long)c.t0 * c.t1 * (unsigned long long)c.dm.e[2];
  if (c.k.kind == K_TRANSPOSE_WINDOW && in.dst_row_pitch > 0 && !remote && tuning.dense_rows != 0) {
    i64 planned_row = -1;
    for (int i = 0; i < 3; ++i)
      if (in.ds[i] == 1 && in.extent[i] > 1) planned_row = in.extent[i];
    if (!offerLines(c, planned_row, in.dst_row_pitch)) offerRowLines(c, planned_row, in.dst_row_pitch);
  }
}

// Fill-moves (Move3D::fill): rows whose fastest dim is contiguous in the destination, or element by element; nothing else.
// The row kernel lays its lanes on the destination's 16-byte grid, from the boundary below each row's start: e[0] = the most
// 16-byte slots a row can touch at any phase (addresses are 2-byte aligned at least), ss[0] = the row length in bytes.
void classifyFill(Classified& c, const Move3D& m, const KernelTuning& tuning, bool streaming) {
  const int es = c.k.es;
  c.dm.src = nullptr;
  if (tuning.force_class != MOVE_GENERIC && m.ds[0] <= 1) {
    c.k.kind = K_ROWS_FILL;
    c.k.vec = 16;
    c.k.access = streaming ? 1 : 0;
    const long long row_bytes = m.extent[0] * es;
    c.dm.e[0] = (row_bytes + 14 + 15) / 16;
    c.dm.e[1] = m.extent[1];
    c.dm.e[2] = m.extent[2];
    c.dm.ss[0] = row_bytes;
    for (int i = 1; i < 3; ++i) c.dm.ds[i] = m.ds[i] * es;
    rowTiles(c);
    return;
  }
  c.k.kind = K_GENERIC_FILL;
  c.k.access = 0;  // (always cached stores)
  genericGeometry(c, m);
}

// layers of a wall-move (Move3D::affine): the extent of its one mirrored dim; -1 when it has none, several, or more layers than
// the addend table holds
int wallLayers(const Move3D& in) {
  int mirrored = -1;
  for (int i = 0; i < 3; ++i) {
    if (in.ss[i] >= 0) continue;
    if (mirrored >= 0) return -1;
    mirrored = i;
  }
  if (mirrored < 0 || in.extent[mirrored] < 1 || in.extent[mirrored] > kMaxWallHalo) return -1;
  return (int)in.extent[mirrored];
}

// The geometry of a reflect- or fold-move as the kernels take it.  Such a move never passes normalizeMove as a whole: the mirrored
// dim (the one with the negative source stride) is set aside, the other two are normalised (and fused) as those of a copy, and the
// mirrored dim comes back as the row or plane index, slower than the row.  mirrored_fastest: it is the fastest memory axis of
// either side -- rows reversed in themselves, which only the element-wise kernels serve.
Move3D mirrorGeometry(const Move3D& in, bool& mirrored_fastest) {
  int mirrored = -1;
  for (int i = 0; i < 3; ++i) {
    if (in.ds[i] < 0) CD_INTERNAL_ERROR("negative destination stride");
    if (in.ss[i] >= 0) continue;
    if (mirrored >= 0) CD_INTERNAL_ERROR("reflect-move with more than one mirrored dim");
    mirrored = i;
  }
  Move3D m = in;
  const bool live = mirrored >= 0 && in.extent[mirrored] > 1;  // (a mirrored dim one cell thick has no direction)
  if (mirrored >= 0) {
    m.extent[mirrored] = 1;
    m.ss[mirrored] = m.ds[mirrored] = 0;
  }
  normalizeMove(m);  // at most two dims remain, in slots 0 and 1
  if (live) {  // back in, slower than the row: slot 1 or 2, ordered by the size of the source stride
    const int at = (m.extent[1] > 1 && m.ss[1] < -in.ss[mirrored]) ? 2 : 1;
    if (at == 1) {
      m.extent[2] = m.extent[1];
      m.ss[2] = m.ss[1];
      m.ds[2] = m.ds[1];
    }
    m.extent[at] = in.extent[mirrored];
    m.ss[at] = in.ss[mirrored];
    m.ds[at] = in.ds[mirrored];
  }
  mirrored_fastest = live && (in.ss[mirrored] == -1 || in.ds[mirrored] <= 1);
  return m;
}

// Reflect-moves (Move3D::reflect; `arith` the real type when the sign bits are flipped): the row geometry of the copy when the
// fastest dim is contiguous on both sides and is not the mirrored one -- the mirror then is the sign of the source's row or plane
// stride -- or the element-wise one; nothing else (only the cells of the move are touched); mirrorGeometry above.  Access mode:
// the project's rule, cached below kStreamBytes, non-temporal loads and stores from there (unmeasured for this kernel, DESIGN.md
// section 4); the element-wise kernel always caches.
// Fold-moves (Move3D::reflect with Move3D::add, `arith` their real type; Move3D::take as well when they clear their source) come
// the same way and are offered the same two geometries and nothing else.  Access mode: the accumulation's rule, cached below
// kStreamBytes, from there non-temporal source loads and zero stores, the destination always cached (unmeasured for these
// kernels too); the element-wise kernel always caches.
// Wall-moves (Move3D::affine: reflect-moves that add the addend of the destination's layer along the mirrored dim) come the same
// way once more: the two geometries of the reflection and nothing else, its access rule (unmeasured here too), lanes never narrower
// than one element -- and Batch::p1 names the entry of the kernel's e[] that is the mirrored dim (-1 when it is one cell thick).
Classified classifyReflect(const Move3D& in, void* const bufs[3], int es, const KernelTuning& tuning, bool remote, ArithType arith) {
  const bool wall = in.affine != 0;
  const bool fold = in.add && !wall;
  if (wall) {
    if (in.fill || in.take || in.add || in.dst_row_pitch != 0 || remote)
      CD_INTERNAL_ERROR("wall-moves only reflect the cells of a local buffer and add their layer's value");
    if (in.affine != 1 && in.affine != 2) CD_INTERNAL_ERROR("wall-move without a side");
    if (arith == ARITH_NONE) CD_INTERNAL_ERROR("wall-move without an arithmetic type");
    if (es % arithBytes(arith) != 0 || es / arithBytes(arith) > 2) CD_INTERNAL_ERROR("element size does not fit the arithmetic type");
    if (wallLayers(in) < 0) CD_INTERNAL_ERROR("wall-move without a mirrored dim, or with more layers than the addend table holds");
  } else if (fold) {
    if (in.fill || in.dst_row_pitch != 0 || remote) CD_INTERNAL_ERROR("fold-moves only add onto the cells of a local buffer");
    if (arith == ARITH_NONE) CD_INTERNAL_ERROR("fold-move without an arithmetic type");
    if (es % arithBytes(arith) != 0 || es / arithBytes(arith) > 2) CD_INTERNAL_ERROR("element size does not fit the arithmetic type");
  } else {
    if (in.fill || in.take || in.dst_row_pitch != 0 || remote)
      CD_INTERNAL_ERROR("reflect-moves only copy the cells of a local buffer");
    if (in.negate && (arith == ARITH_NONE || es % arithBytes(arith) != 0 || es / arithBytes(arith) > 2))
      CD_INTERNAL_ERROR("reflect-move that flips sign bits without a real type that fits the element size");
  }
  bool mirrored_fastest;
  const Move3D m = mirrorGeometry(in, mirrored_fastest);
  Classified c{};
  c.k.es = es;
  c.k.arith = (fold || wall || in.negate) ? arith : ARITH_NONE;
  c.k.neg = (fold || wall) && in.negate;
  int along = -1;  // wall-moves: the entry of the kernel's e[] whose index is the layer
  for (int i = 0; wall && i < 3; ++i)
    if (m.ss[i] < 0) along = i;
  c.elements = in.elements();
  const bool streaming = (c.elements * es >= kStreamBytes || tuning.force_streaming) && !tuning.no_streaming;
  c.dm.src = static_cast<const char*>(bufs[in.src_buf]) + in.src_off * es;
  c.dm.dst = static_cast<char*>(bufs[in.dst_buf]) + in.dst_off * es;
  if (tuning.force_class != MOVE_GENERIC && m.ss[0] <= 1 && m.ds[0] <= 1 && !mirrored_fastest) {
    c.k.kind = wall ? K_ROWS_WALL : (fold ? (in.take ? K_ROWS_FOLD_TAKE : K_ROWS_FOLD) : K_ROWS_REFLECT);
    c.k.access = streaming ? 1 : 0;
    rowVectors(c, m);
    if (c.k.vec < es) CD_INTERNAL_ERROR("reflect-move narrower than one element");
    rowTiles(c);
    if (wall) c.p1 = along;
    return c;
  }
  c.k.kind = wall ? K_GENERIC_WALL : (fold ? (in.take ? K_GENERIC_FOLD_TAKE : K_GENERIC_FOLD) : K_GENERIC_REFLECT);
  c.k.access = 0;
  genericGeometry(c, m, true);  // no destination-fast dim: along the longest
  if (wall) c.p1 = along;
  return c;
}

// Wall-plane moves (Move3D::plane: reflect-moves whose addend is the entry of a device array at the destination cell) have THREE
// operands, and every rule of the reflection's classification takes all three into account:
//  - the mirrored dim is set aside, the other two are ordered by source stride and merge into longer rows only if they are
//    contiguous in source, destination AND plane; the mirrored dim comes back as the row or plane index (mirrorGeometry's slots);
//  - rows when the fastest dim is contiguous on all three operands and is not the mirrored one, element by element otherwise;
//  - the lane width is the widest of 16, 8, 4 and 2 bytes that is not below the element and divides the row length, all three byte
//    bases and all three operands' row and plane strides -- which holds the 2-byte rule (4 bytes and more only at dword-aligned
//    addresses, halfMisaligned) for the plane as well.
// Access: the reflection's rule, and the plane, read once per call, streams with the payload (unmeasured).
Classified classifyWallPlane(const Move3D& in, void* const bufs[3], int es, const KernelTuning& tuning, bool remote, ArithType arith,
                             const WallPlanes* planes) {
  if (in.fill || in.take || in.add || in.affine != 0 || in.dst_row_pitch != 0 || remote)
    CD_INTERNAL_ERROR("wall-plane moves only reflect the cells of a local buffer and add their plane's entries");
  if (in.plane != 1 && in.plane != 2) CD_INTERNAL_ERROR("wall-plane move without a side");
  if (!planes || !planes->base[in.plane - 1]) CD_INTERNAL_ERROR("wall-plane moves without the call's planes");
  if (arith == ARITH_NONE) CD_INTERNAL_ERROR("wall-plane move without an arithmetic type");
  if (es % arithBytes(arith) != 0 || es / arithBytes(arith) > 2) CD_INTERNAL_ERROR("element size does not fit the arithmetic type");
  int mirrored = -1;
  for (int i = 0; i < 3; ++i) {
    if (in.ds[i] < 0) CD_INTERNAL_ERROR("negative destination stride");
    if (in.ss[i] >= 0) {
      if (in.ps[i] < 0) CD_INTERNAL_ERROR("a plane runs backwards only along the mirrored dim");
      continue;
    }
    if (mirrored >= 0) CD_INTERNAL_ERROR("reflect-move with more than one mirrored dim");
    mirrored = i;
  }
  if (mirrored < 0) CD_INTERNAL_ERROR("wall-plane move without a mirrored dim");
  // the two dims that are not mirrored, by source stride; fused when contiguous on all three operands
  struct D {
    i64 e, s, d, p;
  };
  D dims[3];
  int n = 0;
  for (int i = 0; i < 3; ++i)
    if (i != mirrored && in.extent[i] != 1) dims[n++] = {in.extent[i], in.ss[i], in.ds[i], in.ps[i]};
  if (n == 2 && (dims[1].s != dims[0].s ? dims[1].s < dims[0].s : dims[1].d < dims[0].d)) std::swap(dims[0], dims[1]);
  if (n == 2) {
    for (int i = 0; i < 2; ++i) {
      const D &a = dims[i], &b = dims[1 - i];
      if (b.s == a.s * a.e && b.d == a.d * a.e && b.p == a.p * a.e) {
        dims[0] = {a.e * b.e, a.s, a.d, a.p};
        n = 1;
        break;
      }
    }
  }
  const bool live = in.extent[mirrored] > 1;  // (a mirrored dim one cell thick has no direction)
  if (live) {  // back in, slower than the row: slot 1 or 2, ordered by the size of the source stride
    const int at = (n == 2 && dims[1].s < -in.ss[mirrored]) ? 2 : 1;
    for (int i = n; i < at; ++i) dims[i] = {1, 0, 0, 0};
    if (at == 1) dims[2] = n == 2 ? dims[1] : D{1, 0, 0, 0};
    dims[at] = {in.extent[mirrored], in.ss[mirrored], in.ds[mirrored], in.ps[mirrored]};
    n = 3;
  }
  for (int i = n; i < 3; ++i) dims[i] = {1, 0, 0, 0};
  const i64 plane_fastest = in.ps[mirrored] < 0 ? -in.ps[mirrored] : in.ps[mirrored];
  const bool mirrored_fastest = live && (in.ss[mirrored] == -1 || in.ds[mirrored] <= 1 || plane_fastest <= 1);
  const bool rows_fit = dims[0].e == 1 || (dims[0].s == 1 && dims[0].d == 1 && dims[0].p == 1);

  Classified c{};
  c.k.es = es;
  c.k.arith = arith;
  c.k.neg = in.negate;
  c.elements = in.elements();
  const bool streaming = (c.elements * es >= kStreamBytes || tuning.force_streaming) && !tuning.no_streaming;
  c.dm.src = static_cast<const char*>(bufs[in.src_buf]) + in.src_off * es;
  c.dm.dst = static_cast<char*>(bufs[in.dst_buf]) + in.dst_off * es;
  c.po.p = static_cast<const char*>(planes->base[in.plane - 1]) + in.plane_off * es;
  if (tuning.force_class != MOVE_GENERIC && rows_fit && !mirrored_fastest) {
    c.k.kind = K_ROWS_WALL_PLANE;
    c.k.access = streaming ? 1 : 0;
    uintptr_t bits = reinterpret_cast<uintptr_t>(c.dm.src) | reinterpret_cast<uintptr_t>(c.dm.dst) | reinterpret_cast<uintptr_t>(c.po.p);
    for (int i = 1; i < 3; ++i) {
      c.dm.ss[i] = dims[i].s * es;
      c.dm.ds[i] = dims[i].d * es;
      c.po.s[i] = dims[i].p * es;
      bits |= (uintptr_t)(dims[i].s < 0 ? -c.dm.ss[i] : c.dm.ss[i]) | (uintptr_t)c.dm.ds[i] | (uintptr_t)(dims[i].p < 0 ? -c.po.s[i] : c.po.s[i]);
    }
    int vb = 16;
    while (vb > es && ((dims[0].e * es) % vb != 0 || (bits & (uintptr_t)(vb - 1)) != 0)) vb >>= 1;
    c.k.vec = vb;
    c.dm.e[0] = dims[0].e * es / vb;
    c.dm.e[1] = dims[1].e;
    c.dm.e[2] = dims[2].e;
    rowTiles(c);
    return c;
  }
  c.k.kind = K_GENERIC_WALL_PLANE;
  c.k.access = 0;
  Move3D m = in;
  for (int i = 0; i < 3; ++i) {
    m.extent[i] = dims[i].e;
    m.ss[i] = dims[i].s;
    m.ds[i] = dims[i].d;
    c.po.s[i] = dims[i].p;
  }
  genericGeometry(c, m, true);  // no destination-fast dim: along the longest
  return c;
}

// Copy moves take any kind of kernel.  Add-moves (Move3D::add, `arith` their real type) take the row geometry of the copy
// (same extent / address / stride rule) or the element-wise one and nothing else: never shifted, dense or transposing forms
// (only the cells of the move are touched), never a remote destination, never lanes narrower than one real.  Take-moves
// (Move3D::take, with or without `add`: the copy or the addition, then zero bytes into the source cells) are offered the same two
// geometries and nothing else, for the same reason -- and because the zero must go where the lane's load went, at its width.
Classified classify(const Move3D& in, void* const bufs[3], int es, const KernelTuning& tuning, void* dst_base, bool remote,
                    ArithType arith, const WallPlanes* planes = nullptr) {
  if (in.negate && !in.reflect) CD_INTERNAL_ERROR("only reflect- and fold-moves flip sign bits");
  if ((in.affine != 0 || in.plane != 0) && !in.reflect) CD_INTERNAL_ERROR("only reflect-moves add a wall's values");
  if (in.plane != 0) return classifyWallPlane(in, bufs, es, tuning, remote || dst_base != nullptr, arith, planes);
  if (in.reflect && in.take && !in.add) CD_INTERNAL_ERROR("a reflect-move that clears its source must be a fold-move (add)");
  if (in.reflect) return classifyReflect(in, bufs, es, tuning, remote || dst_base != nullptr, arith);
  Move3D m = in;
  if (in.fill) {  // no source: nothing but the destination decides the order and the fusion of the dims
    if (in.add || in.take || in.dst_row_pitch != 0 || remote) CD_INTERNAL_ERROR("fill-moves only store the cells of a local destination");
    for (int i = 0; i < 3; ++i) m.ss[i] = m.ds[i];
  }
  normalizeMove(m);
  const bool add = in.add, take = in.take;
  if (take && (in.dst_row_pitch != 0 || remote)) CD_INTERNAL_ERROR("take-moves only touch the cells of local buffers");
  if (add) {
    if (arith == ARITH_NONE) CD_INTERNAL_ERROR("add-move without an arithmetic type");
    if (remote) CD_INTERNAL_ERROR("add-moves never have remote destinations");
    if (es % arithBytes(arith) != 0 || es / arithBytes(arith) > 2) CD_INTERNAL_ERROR("element size does not fit the arithmetic type");
  }
  Classified c{};
  c.k.es = es;
  c.k.arith = add ? arith : ARITH_NONE;
  c.elements = m.elements();
  const bool streaming = (c.elements * es >= kStreamBytes || tuning.force_streaming) && !tuning.no_streaming;
  // Additions: the source is read once: non-temporal loads for large moves.  The destination is read and rewritten by the
  // same lane: default stores (non-temporal ones measured the same).
  // Takes: the zeroes follow the fill's rule for its stores (cached below kStreamBytes, non-temporal from there), the rest the
  // rule of the copy / the addition; whether a store to a line just loaded wants another rule is unmeasured.
  if (add || take) c.k.access = streaming ? 1 : 0;
  else c.k.access = remote ? 3 : (streaming ? 2 : 0);  // (a peer's memory: write-through stores, whatever the size)
  c.dm.src = static_cast<const char*>(bufs[m.src_buf]) + m.src_off * es;
  c.dm.dst = static_cast<char*>(dst_base ? dst_base : bufs[m.dst_buf]) + m.dst_off * es;
  if (in.fill) {
    classifyFill(c, m, tuning, streaming);
    return c;
  }
  const bool force_generic = tuning.force_class == MOVE_GENERIC;

  if (!force_generic && m.ss[0] <= 1 && m.ds[0] <= 1) {
    c.k.kind = take ? (add ? K_ROWS_ADD_TAKE : K_ROWS_TAKE) : (add ? K_ROWS_ADD : K_ROWS);
    rowVectors(c, m);
    if (add && c.k.vec < arithBytes(arith)) CD_INTERNAL_ERROR("add-move narrower than one real of its arithmetic type");
    if (!add && !take && offerShiftedRows(c, m, tuning)) {
      if (offerDenseRows(c, in, m, tuning, remote)) return c;
      c.dm.e[0] += 64 / c.k.vec;  // one unit of slack vectors per row (see rows_shifted_kernel)
    }
    rowTiles(c);
    return c;
  }

  int t = -1;
  if (!force_generic && !add && !take && m.ss[0] == 1) {
    if (m.ds[1] == 1) t = 1;
    if (m.ds[2] == 1) t = 2;
  }
  if (t > 0 && m.extent[0] >= 4 && m.extent[t] >= 4) {
    classifyTranspose(c, in, m, t, tuning, remote);
    return c;
  }

  c.k.kind = take ? (add ? K_GENERIC_ADD_TAKE : K_GENERIC_TAKE) : (add ? K_GENERIC_ADD : K_GENERIC);
  if (add || take) c.k.access = 0;
  genericGeometry(c, m);
  return c;
}

const char* arithName(int arith) {
  static const char* const names[] = {"", "_Float16", "__bf16", "float", "double"};  // by ArithType
  return names[arith];
}

char g_last_kernel[96] = "";

// what ran last, in the words of the kernel templates (bench.py reports its dominant kernel from here)
void spellKernelName(const KernelChoice& k) {
  char* const out = g_last_kernel;
  constexpr size_t n = sizeof(g_last_kernel);
  const int s = streamArgOf(k.kind, k.access);
  switch (k.kind) {
    case K_ROWS: snprintf(out, n, "rows_kernel<%d,%d>", k.vec, s); break;
    case K_ROWS_SHIFTED: snprintf(out, n, "rows_shifted_kernel<%d,%d>", k.vec, s); break;
    case K_ROWS_DENSE: snprintf(out, n, "rows_dense_kernel<%d>", s); break;
    case K_TRANSPOSE:  // (2-, 4- and 8-byte elements: swizzled LDS tile)
      snprintf(out, n, "transpose_kernel<%d,%d,%d,%d,%d,%s>", k.es, k.vec, k.ti, k.tj, s, k.es != 16 ? "true" : "false");
      break;
    case K_TRANSPOSE_WINDOW: snprintf(out, n, "transpose_window_kernel<%d,%d,%d,%d,%d>", k.es, k.vec, k.ti, k.tj, s); break;
    case K_TRANSPOSE_LINES:
    case K_TRANSPOSE_ROWLINES:
      snprintf(out, n, "%s<%d,%d,%d,%d,%d,%d>", k.kind == K_TRANSPOSE_LINES ? "transpose_lines_kernel" : "transpose_rowlines_kernel",
               k.es, k.vec, k.ti, k.tj, s, kLinesUnitBytes);
      break;
    case K_GENERIC: snprintf(out, n, "generic_kernel<%d,%s>", k.es, s == 3 ? "true" : "false"); break;
    case K_ROWS_ADD: snprintf(out, n, "rows_accumulate_kernel<%s,%d,%d>", arithName(k.arith), k.vec, s); break;
    case K_GENERIC_ADD: snprintf(out, n, "generic_accumulate_kernel<%s,%d>", arithName(k.arith), k.es / arithBytes(k.arith)); break;
    case K_ROWS_FILL: snprintf(out, n, "rows_fill_kernel<%d,%d>", k.vec, s); break;
    case K_GENERIC_FILL: snprintf(out, n, "generic_fill_kernel<%d>", k.es); break;
    case K_ROWS_TAKE: snprintf(out, n, "rows_take_kernel<%d,%d>", k.vec, s); break;
    case K_GENERIC_TAKE: snprintf(out, n, "generic_take_kernel<%d>", k.es); break;
    case K_ROWS_ADD_TAKE: snprintf(out, n, "rows_accumulate_take_kernel<%s,%d,%d>", arithName(k.arith), k.vec, s); break;
    case K_GENERIC_ADD_TAKE:
      snprintf(out, n, "generic_accumulate_take_kernel<%s,%d>", arithName(k.arith), k.es / arithBytes(k.arith));
      break;
    case K_ROWS_REFLECT: snprintf(out, n, "rows_reflect_kernel<%d,%d,%s>", k.vec, s, k.arith != ARITH_NONE ? "true" : "false"); break;
    case K_GENERIC_REFLECT: snprintf(out, n, "generic_reflect_kernel<%d,%s>", k.es, k.arith != ARITH_NONE ? "true" : "false"); break;
    case K_ROWS_FOLD:
    case K_ROWS_FOLD_TAKE:
      snprintf(out, n, "rows_fold_kernel<%s,%d,%d,%s>", arithName(k.arith), k.vec, s, k.kind == K_ROWS_FOLD_TAKE ? "true" : "false");
      break;
    case K_GENERIC_FOLD:
    case K_GENERIC_FOLD_TAKE:
      snprintf(out, n, "generic_fold_kernel<%s,%d,%s>", arithName(k.arith), k.es / arithBytes(k.arith),
               k.kind == K_GENERIC_FOLD_TAKE ? "true" : "false");
      break;
    case K_ROWS_WALL:
      snprintf(out, n, "rows_wall_kernel<%s,%d,%d,%s>", arithName(k.arith), k.vec, s, k.neg ? "true" : "false");
      break;
    case K_GENERIC_WALL: snprintf(out, n, "generic_wall_kernel<%s,%d,%s>", arithName(k.arith), k.es, k.neg ? "true" : "false"); break;
    case K_ROWS_WALL_PLANE:
      snprintf(out, n, "rows_wall_plane_kernel<%s,%d,%d,%s>", arithName(k.arith), k.vec, s, k.neg ? "true" : "false");
      break;
    case K_GENERIC_WALL_PLANE:
      snprintf(out, n, "generic_wall_plane_kernel<%s,%d,%s>", arithName(k.arith), k.es, k.neg ? "true" : "false");
      break;
    case K_ROWS_FIELDS: snprintf(out, n, "rows_fields_kernel<%d,%d>", k.vec, s); break;
    case K_GENERIC_FIELDS: snprintf(out, n, "generic_fields_kernel<%d>", k.es); break;
    case K_TRANSPOSE_FIELDS:
      snprintf(out, n, "transpose_fields_kernel<%d,%d,%d,%d,%d,%s>", k.es, k.vec, k.ti, k.tj, s, k.guard ? "true" : "false");
      break;
    case K_ROWS_FIELDS_ADD:
    case K_ROWS_FIELDS_ADD_TAKE:
      snprintf(out, n, "rows_fields_accumulate_kernel<%s,%d,%d,%s>", arithName(k.arith), k.vec, s,
               k.kind == K_ROWS_FIELDS_ADD_TAKE ? "true" : "false");
      break;
    case K_GENERIC_FIELDS_ADD:
    case K_GENERIC_FIELDS_ADD_TAKE:
      snprintf(out, n, "generic_fields_accumulate_kernel<%s,%d,%s>", arithName(k.arith), k.es / arithBytes(k.arith),
               k.kind == K_GENERIC_FIELDS_ADD_TAKE ? "true" : "false");
      break;
    case K_ROWS_FIELDS_TAKE: snprintf(out, n, "rows_fields_take_kernel<%d,%d>", k.vec, s); break;
    case K_GENERIC_FIELDS_TAKE: snprintf(out, n, "generic_fields_take_kernel<%d>", k.es); break;
    case K_ROWS_FIELDS_REFLECT: snprintf(out, n, "rows_fields_reflect_kernel<%d,%d>", k.vec, s); break;
    case K_GENERIC_FIELDS_REFLECT: snprintf(out, n, "generic_fields_reflect_kernel<%d>", k.es); break;
    case K_ROWS_FIELDS_FOLD:
    case K_ROWS_FIELDS_FOLD_TAKE:
      snprintf(out, n, "rows_fields_fold_kernel<%s,%d,%d,%s>", arithName(k.arith), k.vec, s,
               k.kind == K_ROWS_FIELDS_FOLD_TAKE ? "true" : "false");
      break;
    case K_GENERIC_FIELDS_FOLD:
    case K_GENERIC_FIELDS_FOLD_TAKE:
      snprintf(out, n, "generic_fields_fold_kernel<%s,%d,%s>", arithName(k.arith), k.es / arithBytes(k.arith),
               k.kind == K_GENERIC_FIELDS_FOLD_TAKE ? "true" : "false");
      break;
    case K_ROWS_FIELDS_WALL: snprintf(out, n, "rows_fields_wall_kernel<%s,%d,%d>", arithName(k.arith), k.vec, s); break;
    case K_GENERIC_FIELDS_WALL: snprintf(out, n, "generic_fields_wall_kernel<%s,%d>", arithName(k.arith), k.es); break;
    case K_ROWS_REDUCE:
    case K_GENERIC_REDUCE: break;  // (launchReduce spells them: the operation is no part of the record)
    case K_ROWS_PROFILE:
    case K_COLUMNS_PROFILE:
    case K_GENERIC_PROFILE: break;  // (launchProfile likewise)
    case K_ROWS_PLANES:
    case K_COLUMNS_PLANES:
    case K_GENERIC_PLANES: break;  // (launchPlanes likewise: planes_rows_kernel / planes_columns_kernel<T,MODE>, planes_elements_kernel<T>)
    case K_ROWS_COMBINE:
    case K_GENERIC_COMBINE: break;  // (launchCombine likewise: combine_rows_kernel<T,OP,complex>, combine_elements_kernel<T>)
  }
}

// The 16 bytes a fill stores into every 16-byte-aligned slot of its destination: byte i of a slot lies (i - a) mod es into an
// element, a = the address of any cell of the move (all are congruent mod es).  For naturally aligned pencils this is the
// element replicated; a destination that is only aligned to half its element (the C alignment of the complex types) gets the
// rotated pattern and the same stores.  The moves of one launch lie whole elements apart (base + offset * es), so one pattern
// serves them all.
FillPattern fillPatternOf(const void* value, int es, const void* cell) {
  unsigned char v[16] = {0}, bytes[16];
  if (value) std::memcpy(v, value, es);
  const int a = (int)(reinterpret_cast<uintptr_t>(cell) % (uintptr_t)es);
  for (int i = 0; i < 16; ++i) bytes[i] = v[((i - a) % es + es) % es];
  FillPattern p;
  std::memcpy(p.w, bytes, 16);
  return p;
}

long long g_data_launches = 0;

// The addend table of a launch of wall-moves: row i for move i of the Batch, in DESTINATION order along the mirrored dim.  The high
// side's ghost layer k is destination index k; the low side's is extent - 1 - k, so the low side is reversed here and the kernels
// index by destination layer.  Every entry is the element replicated to 16 bytes.
WallTable wallTableOf(const Launch& l, const Move3D* moves, const WallAddends* addends) {
  if (!addends) CD_INTERNAL_ERROR("wall-moves without the call's addends");
  const int es = l.k.es;
  WallTable t;
  std::memset(&t, 0, sizeof(t));
  for (int i = 0; i < l.b.n; ++i) {
    const Move3D& m = moves[l.index[i]];
    const int layers = wallLayers(m), side = m.affine - 1;
    if (layers < 0 || side < 0 || side > 1) CD_INTERNAL_ERROR("a launch of wall-moves holds a move that is none");
    wallTableRow(*addends, side, layers, es, reinterpret_cast<unsigned char*>(t.w[i]));
  }
  return t;
}

void launchBatch(const Launch& l, const Move3D* moves, const void* fill_value, const WallAddends* addends, hipStream_t stream) {
  const KernelChoice& k = l.k;
  const Batch& b = l.b;
  const unsigned int blocks = l.blocks;
  spellKernelName(k);
  ++g_data_launches;
  switch (k.kind) {
    case K_ROWS:
    case K_ROWS_SHIFTED:
    case K_ROWS_DENSE:
    case K_GENERIC: launchRowsBatch(k, b, blocks, stream); break;
    case K_TRANSPOSE:
      if (k.es == 2) launchTransposeBatch2(k, b, blocks, stream);
      else if (k.es == 4) launchTransposeBatch4(k, b, blocks, stream);
      else if (k.es == 8) launchTransposeBatch8(k, b, blocks, stream);
      else launchTransposeBatch16(k, b, blocks, stream);
      break;
    case K_TRANSPOSE_WINDOW: launchWindowBatch(k, b, blocks, stream); break;
    case K_TRANSPOSE_LINES: launchLinesBatch(k, b, blocks, stream); break;
    case K_TRANSPOSE_ROWLINES: launchRowLinesBatch(k, b, blocks, stream); break;
    case K_ROWS_ADD:
    case K_GENERIC_ADD: launchAccumulateBatch(k, b, blocks, stream); break;
    case K_ROWS_FILL:
    case K_GENERIC_FILL: launchFillBatch(k, b, fillPatternOf(fill_value, k.es, b.m[0].dst), blocks, stream); break;
    case K_ROWS_TAKE:
    case K_GENERIC_TAKE:
    case K_ROWS_ADD_TAKE:
    case K_GENERIC_ADD_TAKE: launchTakeBatch(k, b, blocks, stream); break;
    case K_ROWS_REFLECT:
    case K_GENERIC_REFLECT: launchReflectBatch(k, b, blocks, stream); break;
    case K_ROWS_FOLD:
    case K_GENERIC_FOLD:
    case K_ROWS_FOLD_TAKE:
    case K_GENERIC_FOLD_TAKE: launchFoldBatch(k, b, blocks, stream); break;
    case K_ROWS_WALL:
    case K_GENERIC_WALL: launchWallBatch(k, b, wallTableOf(l, moves, addends), blocks, stream); break;
    case K_ROWS_WALL_PLANE:
    case K_GENERIC_WALL_PLANE: launchWallPlaneBatch(k, b, l.planes, blocks, stream); break;
    case K_ROWS_FIELDS:
    case K_GENERIC_FIELDS:
    case K_TRANSPOSE_FIELDS:
    case K_ROWS_FIELDS_ADD:
    case K_GENERIC_FIELDS_ADD:
    case K_ROWS_FIELDS_TAKE:
    case K_GENERIC_FIELDS_TAKE:
    case K_ROWS_FIELDS_ADD_TAKE:
    case K_GENERIC_FIELDS_ADD_TAKE:
    case K_ROWS_FIELDS_REFLECT:
    case K_GENERIC_FIELDS_REFLECT:
    case K_ROWS_FIELDS_FOLD:
    case K_GENERIC_FIELDS_FOLD:
    case K_ROWS_FIELDS_FOLD_TAKE:
    case K_GENERIC_FIELDS_FOLD_TAKE:
    case K_ROWS_FIELDS_WALL:
    case K_GENERIC_FIELDS_WALL: CD_INTERNAL_ERROR("lists of field-moves are launched by launchFieldMoveList and launchFieldWallList");
    case K_ROWS_REDUCE:
    case K_GENERIC_REDUCE: CD_INTERNAL_ERROR("reductions are launched by launchReduce");
    case K_ROWS_PROFILE:
    case K_COLUMNS_PROFILE:
    case K_GENERIC_PROFILE: CD_INTERNAL_ERROR("profiles are launched by launchProfile");
    case K_ROWS_PLANES:
    case K_COLUMNS_PLANES:
    case K_GENERIC_PLANES: CD_INTERNAL_ERROR("plane updates are launched by launchPlanes");
    case K_ROWS_COMBINE:
    case K_GENERIC_COMBINE: CD_INTERNAL_ERROR("combinations are launched by launchCombine");
  }
}

const KernelTuning kDefaultTuning;

}  // namespace

// Residency of the large far-strided transposes: fewer workgroups per CU than their tiles leave room for.  The workgroups in
// flight then hold fewer, shorter-lived fronts on the far-strided rows (the reading of the run walk, offerRunWalk).  Measured on
// the 8-GiB cycles, settings alternating inside one process on one set of buffers and as whole bench runs against the parent
// commit (profiles/transpose_residency.json):
//   fp64 forward hops (64 x 64 tile, 32 KiB, run walk over tiles): 3 per CU instead of 5, 2.83-2.84 -> 2.82 ms; 4 per CU
//     changes nothing, 2 per CU costs 0.14 ms
//   fp64 inverse hops (64 x 128 tile, 64 KiB): 1 per CU instead of 2, 2.67 -> 2.62-2.63 ms.  (The same tile staged through 32
//     KiB in two halves, which would allow 3 and 4 per CU, measured 0.03 / 0.07 / 0.09 ms per hop SLOWER at 2 / 3 / 4 per CU.)
//   complex128 forward hops (32 x 32 tile, padded rows: 16.5 KiB, run walk): 4 per CU instead of 8, 2.86-2.87 -> 2.75 ms;
//     3, 5 and 6 per CU lie between
//   fp32 forward hops (64 x 128 tile): 3 and 4 per CU within the noise of 5; they launch as before
// The rule reads only what the launch knows: the kernel choice, and for the forward hops that EVERY move of the launch walks in
// runs of tiles along j.
int residencyPadBytes(const KernelChoice& k, const Batch& b) {
  if (k.kind != K_TRANSPOSE || k.access != 2) return 0;
  if (k.es == 8 && k.vec == 2 && k.ti == 64 && k.tj == 128) return 32 << 10;  // far-strided source: 64 + 32 KiB, one per CU
  const bool f64 = k.es == 8 && k.vec == 2 && k.ti == 64 && k.tj == 64, c128 = k.es == 16 && k.vec == 1 && k.ti == 32 && k.tj == 32;
  if (!f64 && !c128) return 0;
  for (int i = 0; i < b.n; ++i)  // far-strided destination, runs of tiles (offerRunWalk)
    if (b.p0[i] <= 1 || !(b.p1[i] & kWalkJFirst) || (b.p1[i] & kWalkRunOverPlanes)) return 0;
  return f64 ? 16 << 10 : 23 << 10;  // 32 + 16 KiB: three per CU; 16.5 + 23 KiB: four
}

void wallTableRow(const WallAddends& addends, int side, int layers, int es, unsigned char out[kern::kMaxWallHalo * 16]) {
  if (side < 0 || side > 1 || layers < 0 || layers > kMaxWallHalo || (es != 2 && es != 4 && es != 8 && es != 16))
    CD_INTERNAL_ERROR("addend table row out of range");
  std::memset(out, 0, kMaxWallHalo * 16);
  for (int j = 0; j < layers; ++j) {
    const unsigned char* v = addends.v[side][side == 0 ? layers - 1 - j : j];
    for (int k = 0; k < 16; ++k) out[16 * j + k] = v[k % es];
  }
}

const char* lastKernelName() { return g_last_kernel; }
long long dataLaunchCount() { return g_data_launches; }

void describeMove(const Move3D& m, const void* src, void* dst, int es, const KernelTuning* tuning, long long out[10]) {
  Move3D mm = m;  // (keeps dst_row_pitch)
  mm.src_buf = BUF_IN;
  mm.dst_buf = BUF_OUT;
  mm.src_off = mm.dst_off = 0;
  void* bufs[3] = {const_cast<void*>(src), dst, nullptr};
  const Classified c = classify(mm, bufs, es, tuning ? *tuning : kDefaultTuning, nullptr, false, ARITH_NONE);
  const KernelChoice& k = c.k;
  // "variant": the lane width, plus 300 for the longer tiles of the plain transposes (tests/golden/kernel_choice_pins.json);
  // row copies: the kernel (plain / shifted / dense) in the tile_i slot
  const int variant = k.vec + (k.kind == K_TRANSPOSE && k.tj > k.ti ? 300 : 0);
  const int ti = k.kind == K_ROWS_DENSE ? 2 : (k.kind == K_ROWS_SHIFTED ? 1 : k.ti);
  const long long v[10] = {(long long)classOf(k.kind), variant, ti, k.tj, c.t0, c.t1, c.dm.e[2], c.p0, c.p1, k.access};
  for (int i = 0; i < 10; ++i) out[i] = v[i];
}

std::vector<Launch> planLaunches(const Move3D* moves, int n, void* const bufs[3], int es, const KernelTuning* tuning,
                                 void* const* dst_base_override, ArithType arith, const WallPlanes* wall_planes) {
  const bool remote = dst_base_override != nullptr;
  const KernelTuning& t = tuning ? *tuning : kDefaultTuning;
  if (es != 2 && es != 4 && es != 8 && es != 16) CD_INTERNAL_ERROR("unsupported element size");
  std::vector<Classified> cs;
  std::vector<int> index;  // cs[i] is moves[index[i]]
  cs.reserve(n);
  index.reserve(n);
  for (int i = 0; i < n; ++i) {
    if (moves[i].elements() == 0) continue;
    cs.push_back(classify(moves[i], bufs, es, t, dst_base_override ? dst_base_override[i] : nullptr, remote, arith, wall_planes));
    index.push_back(i);
  }
  // moves of one phase are independent, so they may be regrouped by kernel flavour
  std::vector<Launch> launches;
  std::vector<bool> done(cs.size(), false);
  for (size_t i = 0; i < cs.size(); ++i) {
    if (done[i]) continue;
    Launch l{};
    Batch& b = l.b;
    l.k = cs[i].k;
    l.cls = classOf(cs[i].k.kind);
    unsigned long long blocks = 0;
    for (size_t j = i; j < cs.size() && b.n < kMaxBatch; ++j) {
      if (done[j] || !(cs[j].k == cs[i].k)) continue;
      if (blocks + cs[j].blocks > 0x7fffffffULL) {
        if (b.n == 0) CD_NOT_SUPPORTED("single block move too large for one launch");
        break;
      }
      b.first_block[b.n] = (unsigned int)blocks;
      b.m[b.n] = cs[j].dm;
      b.p0[b.n] = cs[j].p0;
      b.p1[b.n] = cs[j].p1;
      b.t0[b.n] = cs[j].t0;
      b.t1[b.n] = cs[j].t1;
      l.planes.m[b.n] = cs[j].po;
      blocks += cs[j].blocks;
      l.elements += cs[j].elements;
      l.index[b.n] = index[j];
      ++b.n;
      done[j] = true;
    }
    b.first_block[b.n] = (unsigned int)blocks;
    // Sibling row copies of one phase (the P chunks of an unpack, say) each touch one slice of every destination row:
    // run one after the other, a 2-KiB slice of every 8-KiB row keeps part of the memory channels idle.  Served round
    // robin, the workgroups in flight cover whole rows (C3 per-rank unpacks: 0.43-0.47 -> 0.35 ms, r02_tuning.md).
    // Transposes keep their XCD-contiguous tile walk (interleaving them measured slightly slower).
    if ((dst_base_override || l.cls != MOVE_TRANSPOSE) && b.n > 1) {
      unsigned long long widest = 0;
      for (int k = 0; k < b.n; ++k) widest = std::max<unsigned long long>(widest, b.first_block[k + 1] - b.first_block[k]);
      if (widest * b.n <= 0x7fffffffULL) {
        b.interleave = 1;
        blocks = widest * b.n;
      }
    }
    l.blocks = (unsigned int)blocks;
    launches.push_back(l);
  }
  return launches;
}

void launchMoves(const Move3D* moves, int n, void* const bufs[3], int es, hipStream_t stream,
                 const KernelTuning* tuning, KernelStats* stats, void* const* dst_base_override, ArithType arith,
                 const void* fill_value, const WallAddends* wall_addends, const WallPlanes* wall_planes) {
  for (const Launch& l : planLaunches(moves, n, bufs, es, tuning, dst_base_override, arith, wall_planes)) {
    launchBatch(l, moves, fill_value, wall_addends, stream);
    if (stats) {
      stats->launches[l.cls] += 1;
      stats->elements[l.cls] += l.elements;
    }
  }
}

// ---------------------------------------------------------------------------------------------
// lists of field-moves (kernels.h FieldMoveList; kernels_field_transpose.hip and its siblings)
// ---------------------------------------------------------------------------------------------
namespace {

// the families of field-move kernels and the kinds of each: {rows, element-wise}
enum FieldFamily { FIELDS_COPY, FIELDS_ADD, FIELDS_TAKE, FIELDS_ADD_TAKE, FIELDS_REFLECT, FIELDS_FOLD, FIELDS_FOLD_TAKE, FIELDS_WALL };
constexpr KernelKind kFieldKinds[][2] = {
    {K_ROWS_FIELDS, K_GENERIC_FIELDS},           {K_ROWS_FIELDS_ADD, K_GENERIC_FIELDS_ADD},
    {K_ROWS_FIELDS_TAKE, K_GENERIC_FIELDS_TAKE}, {K_ROWS_FIELDS_ADD_TAKE, K_GENERIC_FIELDS_ADD_TAKE},
    {K_ROWS_FIELDS_REFLECT, K_GENERIC_FIELDS_REFLECT}, {K_ROWS_FIELDS_FOLD, K_GENERIC_FIELDS_FOLD},
    {K_ROWS_FIELDS_FOLD_TAKE, K_GENERIC_FIELDS_FOLD_TAKE}, {K_ROWS_FIELDS_WALL, K_GENERIC_FIELDS_WALL}};
struct FieldListOp {  // the operation of a list: what every one of its moves carries
  bool add, take, wall;
  FieldFamily family;
};
struct FieldMoveItem {  // a move with cells on its way into a launch
  Classified c;   // the kernel choice and the geometry in the kernel's units (of c.dm.src / dst only the alignment is read)
  Move3D norm;    // the shared geometry, normalised (mirrored lists: the mirrored dim back in as the row or plane index)
  FieldMove fm;
  int index;      // the list entry it is
  bool rows_fit;  // its fastest dim is contiguous on both sides (and not the mirrored one)
  int along;      // wall lists: the entry of the kernel's e[] whose index is the destination layer (the mirrored one); -1 otherwise
};

// the rules of the list as a whole; "one operation per list" gives the operation
FieldListOp checkFieldMoveList(const FieldMoveList& r) {
  const int es = r.es;
  if (es != 2 && es != 4 && es != 8 && es != 16) CD_INTERNAL_ERROR("unsupported element size");
  if (r.n < 0 || (r.n > 0 && !r.moves)) CD_INTERNAL_ERROR("field-move list without moves");
  if (r.n_fields < 1 || r.n_fields > kMaxFields || !r.inputs) CD_INTERNAL_ERROR("field count out of range");
  for (int f = 0; f < r.n_fields; ++f)
    if (!r.inputs[f] || (r.outputs && !r.outputs[f])) CD_INTERNAL_ERROR("null field buffer");
  FieldListOp op{};
  for (int i = 0; i < r.n; ++i) {
    if (i == 0) op.add = r.moves[i].add, op.take = r.moves[i].take;
    else if (r.moves[i].add != op.add || r.moves[i].take != op.take) CD_INTERNAL_ERROR("the field-moves of one list carry different operations");
  }
  if (op.add || r.mirrored) {  // (a mirrored list always: the sign mask is that of its real type)
    if (r.arith == ARITH_NONE) CD_INTERNAL_ERROR(r.mirrored ? "mirrored field-move without a real type" : "adding field-move without an arithmetic type");
    if (es % arithBytes(r.arith) != 0 || es / arithBytes(r.arith) > 2) CD_INTERNAL_ERROR("element size does not fit the arithmetic type");
  }
  if (!r.mirrored && r.fields_neg != 0) CD_INTERNAL_ERROR("only mirrored field-moves carry signs");
  if (r.mirrored && r.n_fields < kMaxFields && (r.fields_neg >> r.n_fields) != 0) CD_INTERNAL_ERROR("sign bit of a field the list does not have");
  if (r.mirrored && op.take && !op.add) CD_INTERNAL_ERROR("a mirrored field-move that clears its source must add (fold)");
  // wall field-moves (kernels_field_wall.hip): a mirrored list whose moves all name a side (Move3D::affine); neither adds nor takes
  for (int i = 0; i < r.n; ++i) {
    if (i == 0) op.wall = r.moves[i].affine != 0;
    else if ((r.moves[i].affine != 0) != op.wall) CD_INTERNAL_ERROR("the field-moves of one list carry different operations");
  }
  if (op.wall && (!r.mirrored || op.add || op.take)) CD_INTERNAL_ERROR("wall field-moves are mirrored and neither add onto their destination nor take");
  if (op.wall) op.family = FIELDS_WALL;
  else if (r.mirrored) op.family = op.add ? (op.take ? FIELDS_FOLD_TAKE : FIELDS_FOLD) : FIELDS_REFLECT;
  else op.family = op.take ? (op.add ? FIELDS_ADD_TAKE : FIELDS_TAKE) : (op.add ? FIELDS_ADD : FIELDS_COPY);
  return op;
}

// the rules of one move (empty ones included)
void checkFieldMove(const FieldMoveList& r, const FieldListOp& op, const Move3D& in) {
  if (r.mirrored) {  // (reflect- or fold-moves between cells of the fields' own buffers; their signs travel in fields_neg)
    if (!in.reflect || in.negate || in.fill || in.plane != 0 || in.dst_row_pitch != 0 || in.src_buf == BUF_WORK || in.dst_buf == BUF_WORK)
      CD_INTERNAL_ERROR("mirrored field-moves reflect or fold exactly their cells of the fields' buffers, unsigned");
    if (op.wall && ((in.affine != 1 && in.affine != 2) || wallLayers(in) < 0))
      CD_INTERNAL_ERROR("wall field-move without a side or a mirrored dim, or with more layers than the addend table holds");
  } else if (in.fill || in.reflect || in.negate || in.affine != 0 || in.plane != 0 || in.dst_row_pitch != 0) {
    CD_INTERNAL_ERROR("field-moves copy, add or take exactly their cells");
  }
  if (op.add && in.dst_buf == BUF_WORK) CD_INTERNAL_ERROR("adding field-moves never add onto the workspace");
  if (op.take && in.src_buf == BUF_WORK) CD_INTERNAL_ERROR("taking field-moves never clear the workspace");
  if ((in.src_buf == BUF_WORK || in.dst_buf == BUF_WORK) && !r.work) CD_INTERNAL_ERROR("field-move through a workspace that was not given");
  if ((in.src_buf == BUF_OUT || in.dst_buf == BUF_OUT) && !r.outputs) CD_INTERNAL_ERROR("field-move onto an output list that was not given");
  for (int d = 0; d < 3; ++d)
    if ((in.ss[d] < 0 && !r.mirrored) || in.ds[d] < 0 || in.extent[d] < 0) CD_INTERNAL_ERROR("negative stride or extent in a field-move");
}

// every move with cells, checked: first its shared geometry, normalised, its ends, and the addresses every field's first element can
// have or-ed together (the 2-byte rule: all fields' pencils and all workspace pieces) ...
std::vector<FieldMoveItem> classifyFieldMoves(const FieldMoveList& r, const FieldListOp& op) {
  const int es = r.es;
  const char* const w = static_cast<const char*>(r.work);
  std::vector<FieldMoveItem> items;
  items.reserve(r.n);
  for (int i = 0; i < r.n; ++i) {
    const Move3D& in = r.moves[i];
    checkFieldMove(r, op, in);
    if (in.elements() == 0) continue;
    const i64 step = r.work_steps ? r.work_steps[i] : 0;
    if (step < 0) CD_INTERNAL_ERROR("negative workspace step in a field-move");
    FieldMoveItem it{};
    it.index = i;
    it.along = -1;
    it.norm = in;
    bool mirrored_fastest = false;
    if (r.mirrored) it.norm = mirrorGeometry(in, mirrored_fastest);
    else normalizeMove(it.norm);
    FieldMove& fm = it.fm;
    fm.src_end = in.src_buf == BUF_WORK ? kEndWork : (in.src_buf == BUF_OUT ? kEndOutput : kEndInput);
    fm.dst_end = in.dst_buf == BUF_WORK ? kEndWork : (in.dst_buf == BUF_OUT ? kEndOutput : kEndInput);
    fm.src_off = in.src_off * es;
    fm.dst_off = in.dst_off * es;
    fm.src_step = fm.src_end == kEndWork ? step * es : 0;
    fm.dst_step = fm.dst_end == kEndWork ? step * es : 0;
    uintptr_t address_bits = 0;
    for (int f = 0; f < r.n_fields; ++f) {
      const char* sb = fm.src_end == kEndWork ? w + f * fm.src_step : static_cast<const char*>(fm.src_end == kEndOutput ? r.outputs[f] : r.inputs[f]);
      const char* db = fm.dst_end == kEndWork ? w + f * fm.dst_step : static_cast<const char*>(fm.dst_end == kEndOutput ? r.outputs[f] : r.inputs[f]);
      address_bits |= reinterpret_cast<uintptr_t>(sb) + (uintptr_t)fm.src_off;
      address_bits |= reinterpret_cast<uintptr_t>(db) + (uintptr_t)fm.dst_off;
    }
    it.c.k.es = es;
    it.c.k.arith = (op.add || r.mirrored) ? r.arith : ARITH_NONE;
    it.c.elements = it.norm.elements();
    it.c.dm.src = reinterpret_cast<const char*>(address_bits);
    it.c.dm.dst = reinterpret_cast<char*>(address_bits);
    it.rows_fit = it.norm.ss[0] <= 1 && it.norm.ds[0] <= 1 && !mirrored_fastest;
    items.push_back(it);
  }
  // ... then the kernel choice of each and its geometry in that kernel's units
  const KernelTuning& tuning = r.tuning ? *r.tuning : kDefaultTuning;
  const bool force_generic = tuning.force_class == MOVE_GENERIC;
  // one_choice: rows only if every move has contiguous rows, then the narrowest of their lanes; the largest move decides the access
  bool all_rows = !force_generic;
  int lanes = 16;
  i64 largest = 0;
  for (size_t i = 0; r.one_choice && i < items.size(); ++i) {
    all_rows = all_rows && items[i].rows_fit;
    largest = std::max(largest, items[i].c.elements);
    if (!all_rows) continue;
    Classified c = items[i].c;
    rowVectors(c, items[i].norm);
    lanes = std::min(lanes, c.k.vec);
  }
  for (FieldMoveItem& it : items) {
    const Move3D& m = it.norm;
    Classified& c = it.c;
    // (the access rule, unmeasured for these kernels: kernels.h FieldMoveList::tuning)
    const bool streaming = ((r.one_choice ? largest : c.elements) * es >= kStreamBytes || tuning.force_streaming) && !tuning.no_streaming;
    int t = -1;
    if (!force_generic && !r.one_choice && op.family == FIELDS_COPY && m.ss[0] == 1) {  // (additions, takes and mirrors never transpose)
      if (m.ds[1] == 1) t = 1;
      if (m.ds[2] == 1) t = 2;
    }
    if (r.one_choice ? all_rows : (!force_generic && it.rows_fit)) {
      c.k.kind = kFieldKinds[op.family][0];
      c.k.access = streaming ? 1 : 0;
      rowVectors(c, m, lanes);
      if (c.k.vec < es) CD_INTERNAL_ERROR("field-move narrower than one element");
      rowTiles(c);
    } else if (t > 0 && m.extent[0] >= 4 && m.extent[t] >= 4) {
      c.k.kind = K_TRANSPOSE_FIELDS;
      c.k.access = streaming ? 2 : 0;
      transposeGeometry(c, m, t);
      // one tile per element size and lane width: 2-byte 128 x 128 with 16-byte lanes, 64 x 64 element-wise; 4-byte 64 x 128 /
      // 64 x 64; 8-byte 64 x 64; 16-byte 32 x 32
      const int vw = transposeLaneWidth(c);
      c.k.vec = vw;
      c.k.ti = es == 2 ? (vw == 8 ? 128 : 64) : (es == 16 ? 32 : 64);
      c.k.tj = es == 4 && vw == 4 ? 128 : c.k.ti;
      c.k.guard = c.dm.e[0] % c.k.ti != 0 || c.dm.e[1] % c.k.tj != 0;
      c.t0 = (unsigned int)((c.dm.e[0] + c.k.ti - 1) / c.k.ti);
      c.t1 = (unsigned int)((c.dm.e[1] + c.k.tj - 1) / c.k.tj);
      c.blocks = (unsigned long long)c.t0 * c.t1 * (unsigned long long)c.dm.e[2];
    } else {
      c.k.kind = kFieldKinds[op.family][1];
      c.k.access = 0;
      genericGeometry(c, m, r.mirrored);  // (mirrored, without a destination-fast dim: along the longest, as the single calls)
    }
    if (c.blocks == 0 || c.blocks * (unsigned long long)r.n_fields > 0x7fffffffULL)
      CD_NOT_SUPPORTED("single block move too large for one launch");
    FieldMove& fm = it.fm;
    for (int d = 0; d < 3; ++d) {
      fm.e[d] = c.dm.e[d];
      fm.ss[d] = c.dm.ss[d];
      fm.ds[d] = c.dm.ds[d];
      if (op.wall && m.ss[d] < 0) it.along = d;
    }
    fm.p0 = c.p0;
    fm.t0 = c.t0;
    fm.t1 = c.t1;
    fm.blocks = (unsigned int)c.blocks;
  }
  return items;
}

// moves of one phase are independent: regrouped by equal kernel choice in the order of first appearance, cut at kMaxBatch
std::vector<FieldMoveLaunch> groupFieldMoves(const FieldMoveList& r, const std::vector<FieldMoveItem>& items) {
  const int n_fields = r.n_fields;
  std::vector<FieldMoveLaunch> launches;
  std::vector<bool> done(items.size(), false);
  for (size_t i = 0; i < items.size(); ++i) {
    if (done[i]) continue;
    FieldMoveLaunch l{};
    FieldMoveBatch& b = l.b;
    l.k = items[i].c.k;
    l.cls = classOf(l.k.kind);
    l.fields_neg = r.fields_neg;
    b.n_fields = n_fields;
    b.work = static_cast<char*>(r.work);
    for (int f = 0; f < n_fields; ++f) {
      b.in[f] = static_cast<char*>(r.inputs[f]);
      b.out[f] = r.outputs ? static_cast<char*>(r.outputs[f]) : nullptr;
    }
    unsigned long long blocks = 0;
    for (size_t j = i; j < items.size() && b.n < kMaxBatch; ++j) {
      const Classified& c = items[j].c;
      if (done[j] || !(c.k == l.k)) continue;
      const unsigned long long mine = c.blocks * (unsigned long long)n_fields;
      if (blocks + mine > 0x7fffffffULL) {  // (never the first of a group: checked per move above)
        if (r.one_choice) CD_NOT_SUPPORTED("field-moves too large for one launch");
        break;
      }
      b.first_block[b.n] = (unsigned int)blocks;
      b.m[b.n] = items[j].fm;
      blocks += mine;
      l.elements += c.elements * n_fields;
      l.blocks_per_field += (unsigned int)c.blocks;
      l.index[b.n] = items[j].index;
      l.along[b.n] = items[j].along;
      ++b.n;
      done[j] = true;
    }
    for (int k = b.n; k <= kMaxBatch; ++k) b.first_block[k] = (unsigned int)blocks;
    l.blocks = (unsigned int)blocks;
    launches.push_back(l);
  }
  return launches;
}

// a launch of a list: named, counted, made, accounted
template <typename Make>
void runFieldLaunch(const FieldMoveLaunch& l, KernelStats* stats, Make make) {
  spellKernelName(l.k);
  ++g_data_launches;
  make();
  if (stats) {
    stats->launches[l.cls] += 1;
    stats->elements[l.cls] += l.elements;
  }
}

}  // namespace

std::vector<FieldMoveLaunch> planFieldMoveLaunches(const FieldMoveList& list) {
  const FieldListOp op = checkFieldMoveList(list);
  return groupFieldMoves(list, classifyFieldMoves(list, op));
}

int fieldsPerWallLaunch(int sides, int layers, int es) {
  if (sides < 1 || sides > kMaxBatch || layers < 1 || layers > kMaxWallHalo || (es != 2 && es != 4 && es != 8 && es != 16))
    CD_INTERNAL_ERROR("wall field-moves out of the addend table's range");
  return std::min(kMaxFields, kFieldWallTableBytes / (sides * layers * es));
}

std::vector<FieldWallLaunch> planFieldWallLaunches(const FieldMoveList& list) {
  const Move3D* moves = list.moves;
  const int n = list.n, n_fields = list.n_fields, es = list.es;
  if (n_fields < 1 || n_fields > kMaxFields || !list.inputs) CD_INTERNAL_ERROR("field count out of range");
  if (n < 0 || n > 2 || (n > 0 && !moves)) CD_INTERNAL_ERROR("wall field-moves: the one or two sides of a call");
  if (n_fields < kMaxFields && (list.fields_neg >> n_fields) != 0) CD_INTERNAL_ERROR("sign bit of a field the list does not have");
  if (!list.addends) CD_INTERNAL_ERROR("wall field-moves without the call's addends");
  std::vector<FieldWallLaunch> out;
  // S, the sides written, and h, the layers: those of the moves that have cells
  int sides = 0, layers = 0;
  for (int i = 0; i < n; ++i) {
    if (moves[i].elements() == 0) continue;
    const int mine = wallLayers(moves[i]);
    if (mine < 0 || (moves[i].affine != 1 && moves[i].affine != 2))
      CD_INTERNAL_ERROR("wall field-move without a side or a mirrored dim, or with more layers than the addend table holds");
    layers = std::max(layers, mine);
    ++sides;
  }
  if (sides == 0) return out;
  const int per_launch = fieldsPerWallLaunch(sides, layers, es);
  // a run of fields: the sides as a mirrored list with one choice, both ends in the fields' own buffers
  FieldMoveList run = list;
  run.work_steps = nullptr;
  run.work = nullptr;
  run.one_choice = run.mirrored = true;
  for (int f0 = 0; f0 < n_fields; f0 += per_launch) {
    const int nf = std::min(per_launch, n_fields - f0);
    run.inputs = run.outputs = list.inputs + f0;
    run.n_fields = nf;
    run.fields_neg = (list.fields_neg >> f0) & (nf == kMaxFields ? 0xffffffffu : ((1u << nf) - 1u));
    std::vector<FieldMoveLaunch> ls = planFieldMoveLaunches(run);
    if (ls.size() != 1 || ls[0].b.n != sides) CD_INTERNAL_ERROR("the sides of a wall-value call did not come out as one launch");
    FieldWallLaunch w{};
    w.l = ls[0];
    w.first_field = f0;
    w.walk.layers = layers;
    w.walk.es = es;
    unsigned char* bytes = reinterpret_cast<unsigned char*>(w.table.w);
    for (int i = 0; i < w.l.b.n; ++i) {
      const Move3D& m = moves[w.l.index[i]];
      const int mine = wallLayers(m), side = m.affine - 1;
      w.walk.along[i] = w.l.along[i];
      for (int f = 0; f < nf; ++f)
        for (int j = 0; j < mine; ++j)  // destination order: the low side reversed, as wallTableRow
          std::memcpy(bytes + ((size_t)(i * nf + f) * layers + j) * es, list.addends[f0 + f].v[side][side == 0 ? mine - 1 - j : j], es);
    }
    out.push_back(w);
  }
  return out;
}

void launchFieldMoveList(const FieldMoveList& list, hipStream_t stream, KernelStats* stats) {
  if (list.addends) {  // a wall list: one launch per run of fields whose addends fit the table
    for (const FieldWallLaunch& w : planFieldWallLaunches(list))
      runFieldLaunch(w.l, stats, [&] { launchFieldWallBatch(w.l.k, w.l.b, w.l.fields_neg, w.table, w.walk, w.l.blocks, stream); });
    return;
  }
  for (const FieldMoveLaunch& l : planFieldMoveLaunches(list)) {
    if (l.k.kind >= K_ROWS_FIELDS_WALL) CD_INTERNAL_ERROR("wall field-moves without the call's addends");
    runFieldLaunch(l, stats, [&] {
      if (l.k.kind >= K_ROWS_FIELDS_REFLECT) launchFieldMirrorBatch(l.k, l.b, l.fields_neg, l.blocks, stream);
      else if (l.k.kind >= K_ROWS_FIELDS_ADD) launchFieldAccumulateBatch(l.k, l.b, l.blocks, stream);
      else launchFieldMoveBatch(l.k, l.b, l.blocks, stream);
    });
  }
}

// ---------------------------------------------------------------------------------------------
// reductions of a box of cells (kernels_reduce.hip)
// ---------------------------------------------------------------------------------------------
// The dims of a box that count, by stride, contiguous ones merged (rowVectors' rule for copies): e[0] x e[1] x e[2] elements at strides
// s[] with e[0] the row, `nd` of them longer than a cell.  Answers whether the box has rows at all: a dim of stride 1.
static bool mergeBoxDims(const i64 (&extent)[3], const i64 (&strides)[3], i64 (&e)[3], i64 (&s)[3], int& nd) {
  e[0] = e[1] = e[2] = 1, s[0] = s[1] = s[2] = 0;
  nd = 0;
  int unit = -1;  // a dim of stride 1 that is one cell long is still the row (a pencil one cell thick along its fastest axis)
  for (int i = 0; i < 3; ++i) {
    if (extent[i] > 1) e[nd] = extent[i], s[nd] = strides[i], ++nd;
    else if (strides[i] == 1) unit = i;
  }
  for (int i = 0; i < nd; ++i)
    for (int j = i + 1; j < nd; ++j)
      if (s[j] < s[i]) std::swap(s[i], s[j]), std::swap(e[i], e[j]);
  if (nd > 0 && nd < 3 && s[0] != 1 && unit >= 0) {  // rows of one cell
    for (int i = nd; i > 0; --i) e[i] = e[i - 1], s[i] = s[i - 1];
    e[0] = 1, s[0] = 1, ++nd;
  }
  const bool rows = nd == 0 || s[0] == 1;
  if (nd == 0) s[0] = 1;
  while (rows && nd >= 2 && s[1] == e[0]) {  // the next dim follows without a gap: one longer row
    e[0] *= e[1];
    e[1] = e[2], s[1] = s[2];
    e[2] = 1, s[2] = 0;
    --nd;
  }
  if (rows && nd == 3 && s[2] == e[1] * s[1]) e[1] *= e[2], e[2] = 1, s[2] = 0, --nd;
  return rows;
}

// The row walk of a merged box on the 16-byte grid, for ReduceGeom and CombineGeom alike: rows of e[0] elements, a box that is one
// long row cut into rows of kReduceChunkBytes (the last one what is left); 16-byte slots a row can touch, lanes per row, tiles.
template <typename Geom> static void setRowWalk(Geom& g, const i64 (&e)[3], const i64 (&s)[3], int nd, int es) {
  g.row_bytes = g.last_row_bytes = e[0] * es;
  g.rows = e[1], g.planes = e[2];
  g.s1 = s[1] * es, g.s2 = s[2] * es;
  if (nd <= 1 && g.row_bytes > kReduceChunkBytes) {
    g.rows = (g.row_bytes + kReduceChunkBytes - 1) / kReduceChunkBytes;
    g.last_row_bytes = g.row_bytes - (g.rows - 1) * kReduceChunkBytes;
    g.row_bytes = g.s1 = kReduceChunkBytes;
  }
  g.slots = (g.row_bytes + 14 + 15) / 16;
  g.p0 = std::min(8, ilog2ceil(g.slots));
  const i64 lpr = 1LL << g.p0, rows_per_tile = (i64)(kThreads >> g.p0) * kRowsUnroll;
  const i64 t0 = (g.slots + lpr - 1) / lpr, t1 = (g.rows + rows_per_tile - 1) / rows_per_tile;
  if (t0 > 0xffffffffLL || t1 > 0xffffffffLL) CD_NOT_SUPPORTED("a box of more than 2^32 - 1 tiles along one dim");
  g.t0 = (unsigned int)t0, g.t1 = (unsigned int)t1;
  g.tiles = (unsigned long long)t0 * (unsigned long long)t1 * (unsigned long long)g.planes;
}

ReducePlan planReduce(const ReduceRequest& r) {
  if (r.n_fields < 1 || r.n_fields > kMaxFields || !r.a) CD_INTERNAL_ERROR("a reduction of 1 .. kMaxFields fields");
  if (r.op != kReduceSum && r.op != kReduceDot && r.op != kReduceMaxAbs) CD_INTERNAL_ERROR("reduction operation out of range");
  if (r.op == kReduceDot && !r.b) CD_INTERNAL_ERROR("a dot product without its second operands");
  if (r.arith == ARITH_NONE) CD_INTERNAL_ERROR("a reduction needs the real type of its elements");
  const int es = r.es, rs = arithBytes(r.arith);
  if (es != rs && es != 2 * rs) CD_INTERNAL_ERROR("element size does not match the real type");
  if (r.box_off < 0 || r.readable_before < 0 || r.readable_after < 0) CD_INTERNAL_ERROR("negative offset of a reduction");
  const KernelTuning& tuning = r.tuning ? *r.tuning : kDefaultTuning;
  ReducePlan p;
  std::memset(&p, 0, sizeof(p));
  p.k.es = es;
  p.k.arith = r.arith;
  ReduceGeom& g = p.g;
  g.reals = es / rs;
  g.n_fields = r.n_fields;
  g.box_off = r.box_off * es;
  i64 cells = 1, last = 0;  // `last`: the element offset of the box's last cell
  for (int i = 0; i < 3; ++i) {
    if (r.extent[i] < 0 || r.strides[i] < 0) CD_INTERNAL_ERROR("negative extent or stride of a reduction");
    cells *= r.extent[i];
    last += (r.extent[i] - 1) * r.strides[i];
    g.e[i] = r.extent[i];
    g.s[i] = r.strides[i];
  }
  const i64 span = (last + 1) * es;
  g.rd_lo = -r.readable_before;
  g.rd_hi = span + r.readable_after;
  p.k.kind = K_GENERIC_REDUCE;
  p.k.vec = es;
  if (cells == 0) return p;  // (no stage one: g.blocks == 0)
  p.k.access = ((cells * es >= kStreamBytes || tuning.force_streaming) && !tuning.no_streaming) ? 1 : 0;

  // the dims that count, by stride; contiguous ones merged
  i64 e[3], s[3];
  int nd;
  bool rows = mergeBoxDims(r.extent, r.strides, e, s, nd);
  // the row kernel's lanes lie on the 16-byte grid of `a`: every field on a boundary of its real type; the second operand of a
  // DOT at the same phase of that grid; a complex DOT pairs real and imaginary part inside one vector
  for (int f = 0; f < r.n_fields && rows; ++f) {
    const uintptr_t a = reinterpret_cast<uintptr_t>(r.a[f]);
    if (a % (uintptr_t)rs != 0) rows = false;
    if (r.op == kReduceDot) {
      const uintptr_t b = reinterpret_cast<uintptr_t>(r.b[f]);
      if ((a & 15) != (b & 15)) rows = false;
      if (g.reals == 2 && a % (uintptr_t)es != 0) rows = false;
    }
  }
  if (tuning.force_class == MOVE_GENERIC) rows = false;

  if (!rows) {
    g.p0 = 0;
    for (int i = 0; i < 3; ++i)
      if (r.strides[i] == 1 && r.extent[i] > 1) g.p0 = i;
    const i64 want = (cells + kThreads - 1) / kThreads;
    g.blocks = (unsigned int)std::min<i64>(std::max<i64>(want, 1), kReduceMaxBlocks);
    p.read_lo = 0;
    p.read_hi = span;
    return p;
  }

  p.k.kind = K_ROWS_REDUCE;
  p.k.vec = 16;
  g.stream = p.k.access;
  setRowWalk(g, e, s, nd, es);
  g.blocks = (unsigned int)std::min<unsigned long long>(g.tiles, kReduceMaxBlocks);
  // what field 0 reads: whole 16-byte vectors from the boundary below the first cell to the boundary above the last, where the
  // readable range holds them; the cells alone where it does not
  const uintptr_t first_cell = reinterpret_cast<uintptr_t>(r.a[0]) + (uintptr_t)g.box_off;
  const i64 below = (i64)(first_cell & 15), above = (i64)((16 - ((first_cell + (uintptr_t)span) & 15)) & 15);
  const auto whole = [&](i64 slot) { return slot >= g.rd_lo && slot + 16 <= g.rd_hi; };  // (the kernel's test of a vector)
  p.read_lo = whole(-below) ? -below : 0;
  p.read_hi = whole(span + above - 16) ? span + above : span;
  return p;
}

void launchReduce(const ReduceRequest& r, double* results, void* work, hipStream_t stream, KernelStats* stats) {
  const ReducePlan p = planReduce(r);
  if (p.g.blocks > 0) {
    ReduceFields fields;
    std::memset(&fields, 0, sizeof(fields));
    for (int f = 0; f < r.n_fields; ++f) {
      fields.a[f] = static_cast<const char*>(r.a[f]);
      if (r.op == kReduceDot) fields.b[f] = static_cast<const char*>(r.b[f]);
    }
    if (p.k.kind == K_ROWS_REDUCE)
      snprintf(g_last_kernel, sizeof(g_last_kernel), "reduce_rows_kernel<%s,%d>", arithName(p.k.arith), r.op);
    else
      snprintf(g_last_kernel, sizeof(g_last_kernel), "reduce_elements_kernel<%s,%d>", arithName(p.k.arith), r.op);
    ++g_data_launches;
    launchReduceStageOne(p.k, r.op, p.g, fields, static_cast<double*>(work), stream);
    if (stats) {
      const MoveClass cls = classOf(p.k.kind);
      stats->launches[cls] += 1;
      stats->elements[cls] += (i64)r.n_fields * r.extent[0] * r.extent[1] * r.extent[2];
    }
  } else {
    snprintf(g_last_kernel, sizeof(g_last_kernel), "reduce_final_kernel<%d>", r.op);
  }
  ++g_data_launches;
  launchReduceFinal(r.op, r.n_fields, p.g.blocks, results, static_cast<const double*>(work), stream);
}

// ---------------------------------------------------------------------------------------------
// profiles of a box of cells along one dim (kernels_profile.hip)
// ---------------------------------------------------------------------------------------------
ProfilePlan planProfile(const ProfileRequest& r) {
  if (r.n_fields < 1 || r.n_fields > kMaxFields || !r.a) CD_INTERNAL_ERROR("a profile of 1 .. kMaxFields fields");
  if (r.op != kReduceSum && r.op != kReduceDot && r.op != kReduceMaxAbs) CD_INTERNAL_ERROR("reduction operation out of range");
  if (r.op == kReduceDot && !r.b) CD_INTERNAL_ERROR("a dot product without its second operands");
  if (r.arith == ARITH_NONE) CD_INTERNAL_ERROR("a profile needs the real type of its elements");
  if (r.keep < 0 || r.keep > 2) CD_INTERNAL_ERROR("the kept dim of a profile is 0, 1 or 2");
  const int es = r.es, rs = arithBytes(r.arith);
  if (es != rs && es != 2 * rs) CD_INTERNAL_ERROR("element size does not match the real type");
  if (r.box_off < 0 || r.readable_before < 0 || r.readable_after < 0) CD_INTERNAL_ERROR("negative offset of a profile");
  const KernelTuning& tuning = r.tuning ? *r.tuning : kDefaultTuning;
  ProfilePlan p;
  std::memset(&p, 0, sizeof(p));
  p.k.kind = K_GENERIC_PROFILE;
  p.k.es = es;
  p.k.vec = es;
  p.k.arith = r.arith;
  ProfileGeom& g = p.g;
  g.reals = es / rs;
  g.n_fields = r.n_fields;
  g.box_off = r.box_off * es;
  i64 cells = 1, last = 0;  // `last`: the element offset of the box's last cell
  for (int i = 0; i < 3; ++i) {
    if (r.extent[i] < 0 || r.strides[i] < 0) CD_INTERNAL_ERROR("negative extent or stride of a profile");
    cells *= r.extent[i];
    last += (r.extent[i] - 1) * r.strides[i];
  }
  const i64 L = r.extent[r.keep];
  g.L = L;
  if (cells == 0) return p;  // (no stage one: g.parts == 0)
  if (L > 0x7fffffffLL) CD_NOT_SUPPORTED("a profile of more than 2^31 - 1 entries");
  const i64 span = (last + 1) * es;
  g.rd_lo = -r.readable_before;
  g.rd_hi = span + r.readable_after;
  p.k.access = ((cells * es >= kStreamBytes || tuning.force_streaming) && !tuning.no_streaming) ? 1 : 0;
  g.stream = p.k.access;
  // parts per entry: what the workspace holds at most, and no more than fills the device -- about kProfileBlocks workgroups per field
  const i64 cap = std::min<i64>(std::max<i64>(kProfilePairsPerField / L, 1), kProfileMaxParts);
  const i64 per_entry = std::min<i64>(cap, std::max<i64>(kProfileBlocks / L, 1));

  // the two reduced dims, the one of the smaller stride first (a dim of one cell has no stride that counts)
  int o1 = (r.keep + 1) % 3, o2 = (r.keep + 2) % 3;
  const auto pitch = [&](int d) { return r.extent[d] > 1 ? r.strides[d] : 0; };
  if (r.extent[o2] > 1 && (r.extent[o1] == 1 || r.strides[o2] < r.strides[o1])) std::swap(o1, o2);
  int c = -1;  // the contiguous dim
  for (int i = 0; i < 3; ++i)
    if (r.strides[i] == 1 && (c < 0 || (r.extent[c] == 1 && r.extent[i] > 1))) c = i;
  // lanes on the 16-byte grid of `a`: planReduce's rules
  bool fast = c >= 0 && tuning.force_class != MOVE_GENERIC;
  for (int f = 0; f < r.n_fields && fast; ++f) {
    const uintptr_t a = reinterpret_cast<uintptr_t>(r.a[f]);
    if (a % (uintptr_t)rs != 0) fast = false;
    if (r.op == kReduceDot) {
      const uintptr_t b = reinterpret_cast<uintptr_t>(r.b[f]);
      if ((a & 15) != (b & 15)) fast = false;
      if (g.reals == 2 && a % (uintptr_t)es != 0) fast = false;
    }
  }
  const i64 plane_cells = r.extent[o1] * r.extent[o2];
  // the column form: every row of the box at one phase of the 16-byte grid
  if (fast && c == r.keep && ((pitch(o1) * es) % 16 != 0 || (pitch(o2) * es) % 16 != 0 || plane_cells > 0x7fffffffLL)) fast = false;

  if (!fast) {
    g.e1 = r.extent[o1], g.e2 = r.extent[o2];
    g.s1 = pitch(o1) * es, g.s2 = pitch(o2) * es;
    g.sk = r.strides[r.keep] * es;
    g.parts = (unsigned int)std::min<i64>(per_entry, (plane_cells + kThreads - 1) / kThreads);
    p.blocks = L * g.parts;
    p.read_lo = 0;
    p.read_hi = span;
  } else {
    p.k.vec = 16;
    if (c != r.keep) {
      const int o = 3 - c - r.keep;
      p.k.kind = K_ROWS_PROFILE;
      g.row_bytes = r.extent[c] * es;
      g.rows = r.extent[o];
      g.s1 = pitch(o) * es;
      g.sk = r.strides[r.keep] * es;
      g.slots = (g.row_bytes + 14 + 15) / 16;
      g.p0 = std::min(8, ilog2ceil(g.slots));
      const i64 lpr = 1LL << g.p0, rows_per_tile = (i64)(kThreads >> g.p0) * kRowsUnroll;
      const i64 t0 = (g.slots + lpr - 1) / lpr, t1 = (g.rows + rows_per_tile - 1) / rows_per_tile;
      if (t0 > 0xffffffffLL || t1 > 0xffffffffLL) CD_NOT_SUPPORTED("a profile of more than 2^32 - 1 tiles along one dim");
      g.t0 = (unsigned int)t0, g.t1 = (unsigned int)t1;
      g.parts = (unsigned int)std::min<i64>(per_entry, t0 * t1);
      p.blocks = L * g.parts;
    } else {
      p.k.kind = K_COLUMNS_PROFILE;
      g.row_bytes = L * es;
      g.e1 = r.extent[o1], g.e2 = r.extent[o2];
      g.s1 = pitch(o1) * es, g.s2 = pitch(o2) * es;
      g.rows = plane_cells;
      g.slots = (g.row_bytes + 14 + 15) / 16;
      g.p0 = std::min(5, ilog2ceil(g.slots));  // at most 32 slots per row-lane: eight row-lanes and more per workgroup
      const i64 lpr = 1LL << g.p0, rows_per_pass = (i64)(kThreads >> g.p0) * kRowsUnroll;
      const i64 t0 = (g.slots + lpr - 1) / lpr;
      if (t0 > 0xffffffLL) CD_NOT_SUPPORTED("a profile of more than 2^24 - 1 tile columns");
      g.t0 = (unsigned int)t0;
      const i64 want = std::min<i64>(std::min<i64>(cap, std::max<i64>(kProfileBlocks / t0, 1)), (g.rows + rows_per_pass - 1) / rows_per_pass);
      g.rows_per_part = ((g.rows + want - 1) / want + rows_per_pass - 1) / rows_per_pass * rows_per_pass;  // whole passes
      g.parts = (unsigned int)((g.rows + g.rows_per_part - 1) / g.rows_per_part);
      p.blocks = t0 * g.parts;
    }
    // what field 0 reads: whole 16-byte vectors from the boundary below the first cell to the boundary above the last, where the
    // readable range holds them; the cells alone where it does not
    const uintptr_t first_cell = reinterpret_cast<uintptr_t>(r.a[0]) + (uintptr_t)g.box_off;
    const i64 below = (i64)(first_cell & 15), above = (i64)((16 - ((first_cell + (uintptr_t)span) & 15)) & 15);
    const auto whole = [&](i64 slot) { return slot >= g.rd_lo && slot + 16 <= g.rd_hi; };  // (the kernels' test of a vector)
    p.read_lo = whole(-below) ? -below : 0;
    p.read_hi = whole(span + above - 16) ? span + above : span;
  }
  if (p.blocks * r.n_fields > 0x7fffffffLL) CD_NOT_SUPPORTED("a profile of more than 2^31 - 1 workgroups");
  g.final_lanes_log2 = g.parts >= 16 ? 6 : 0;
  return p;
}

void launchProfile(const ProfileRequest& r, double* results, i64 ld, void* work, hipStream_t stream, KernelStats* stats) {
  const ProfilePlan p = planProfile(r);
  if (p.g.L == 0) return;  // nothing to write
  if (ld < p.g.L) CD_INTERNAL_ERROR("the leading dimension of a profile is shorter than the profile");
  if (p.g.parts > 0) {
    ReduceFields fields;
    std::memset(&fields, 0, sizeof(fields));
    for (int f = 0; f < r.n_fields; ++f) {
      fields.a[f] = static_cast<const char*>(r.a[f]);
      if (r.op == kReduceDot) fields.b[f] = static_cast<const char*>(r.b[f]);
    }
    const char* const name = p.k.kind == K_ROWS_PROFILE ? "profile_rows_kernel" : p.k.kind == K_COLUMNS_PROFILE ? "profile_columns_kernel" : "profile_elements_kernel";
    snprintf(g_last_kernel, sizeof(g_last_kernel), "%s<%s,%d>", name, arithName(p.k.arith), r.op);
    ++g_data_launches;
    if (p.k.kind == K_ROWS_PROFILE) launchProfileRows(p.k, r.op, p.g, fields, static_cast<double*>(work), stream);
    else launchProfileColumnsOrElements(p.k, r.op, p.g, fields, static_cast<double*>(work), stream);
    if (stats) {
      const MoveClass cls = classOf(p.k.kind);
      stats->launches[cls] += 1;
      stats->elements[cls] += (i64)r.n_fields * r.extent[0] * r.extent[1] * r.extent[2];
    }
  } else {
    snprintf(g_last_kernel, sizeof(g_last_kernel), "profile_final_kernel<%d>", r.op);
  }
  ++g_data_launches;
  launchProfileFinal(r.op, p.g, results, ld, static_cast<const double*>(work), stream);
}

// ---------------------------------------------------------------------------------------------
// plane updates of a box of cells along one dim (kernels_planes.hip)
// ---------------------------------------------------------------------------------------------
PlanesPlan planPlanes(const PlanesRequest& r) {
  if (r.n_fields < 1 || r.n_fields > kMaxFields || !r.a) CD_INTERNAL_ERROR("a plane update of 1 .. kMaxFields fields");
  if (r.op != kPlanesAdd && r.op != kPlanesMul) CD_INTERNAL_ERROR("plane-update operation out of range");
  if (r.arith == ARITH_NONE) CD_INTERNAL_ERROR("a plane update needs the real type of its elements");
  if (r.keep < 0 || r.keep > 2) CD_INTERNAL_ERROR("the kept dim of a plane update is 0, 1 or 2");
  const int es = r.es, rs = arithBytes(r.arith);
  if (es != rs && es != 2 * rs) CD_INTERNAL_ERROR("element size does not match the real type");
  if (es == 2 * rs && r.arith == ARITH_BF16) CD_INTERNAL_ERROR("bf16 has no complex type");
  if (r.box_off < 0 || r.readable_before < 0 || r.readable_after < 0) CD_INTERNAL_ERROR("negative offset of a plane update");
  const KernelTuning& tuning = r.tuning ? *r.tuning : kDefaultTuning;
  PlanesPlan p;
  std::memset(&p, 0, sizeof(p));
  p.k.kind = K_GENERIC_PLANES;
  p.k.es = es;
  p.k.vec = es;
  p.k.arith = r.arith;
  PlanesGeom& g = p.g;
  g.reals = es / rs;
  g.n_fields = r.n_fields;
  g.op = r.op;
  g.scale = r.scale;
  g.box_off = r.box_off * es;
  i64 cells = 1, last = 0;  // `last`: the element offset of the box's last cell
  for (int i = 0; i < 3; ++i) {
    if (r.extent[i] < 0 || r.strides[i] < 0) CD_INTERNAL_ERROR("negative extent or stride of a plane update");
    cells *= r.extent[i];
    last += (r.extent[i] - 1) * r.strides[i];
  }
  const i64 L = r.extent[r.keep];
  g.L = L;
  if (r.ld != 0 && r.ld < L) CD_INTERNAL_ERROR("the leading dimension of the coefficients is shorter than the kept extent");
  g.ld = r.ld;
  if (cells == 0) return p;  // (no launch: g.parts == 0)
  if (L > 0x7fffffffLL) CD_NOT_SUPPORTED("a plane update of more than 2^31 - 1 entries");
  const i64 span = (last + 1) * es;
  g.rd_lo = -r.readable_before;
  g.rd_hi = span + r.readable_after;
  p.k.access = ((cells * es >= kStreamBytes || tuning.force_streaming) && !tuning.no_streaming) ? 1 : 0;
  g.stream = p.k.access;
  const i64 per_entry = std::max<i64>(kProfileBlocks / L, 1);  // parts per entry: about kProfileBlocks workgroups per field

  // the two other dims, the one of the smaller stride first (a dim of one cell has no stride that counts)
  int o1 = (r.keep + 1) % 3, o2 = (r.keep + 2) % 3;
  const auto pitch = [&](int d) { return r.extent[d] > 1 ? r.strides[d] : 0; };
  if (r.extent[o2] > 1 && (r.extent[o1] == 1 || r.strides[o2] < r.strides[o1])) std::swap(o1, o2);
  int c = -1;  // the contiguous dim
  for (int i = 0; i < 3; ++i)
    if (r.strides[i] == 1 && (c < 0 || (r.extent[c] == 1 && r.extent[i] > 1))) c = i;
  // lanes on the 16-byte grid: every field on a boundary of its real type; the complex product pairs the reals 2k, 2k + 1 of a slot,
  // so its fields sit on element boundaries
  bool fast = c >= 0 && tuning.force_class != MOVE_GENERIC;
  const uintptr_t need = (r.op == kPlanesMul && g.reals == 2) ? (uintptr_t)es : (uintptr_t)rs;
  for (int f = 0; f < r.n_fields && fast; ++f)
    if (reinterpret_cast<uintptr_t>(r.a[f]) % need != 0) fast = false;
  const i64 plane_cells = r.extent[o1] * r.extent[o2];
  // the column form: every row of the box at one phase of the 16-byte grid
  if (fast && c == r.keep && ((pitch(o1) * es) % 16 != 0 || (pitch(o2) * es) % 16 != 0 || plane_cells > 0x7fffffffLL)) fast = false;

  if (!fast) {
    g.e1 = r.extent[o1], g.e2 = r.extent[o2];
    g.s1 = pitch(o1) * es, g.s2 = pitch(o2) * es;
    g.sk = pitch(r.keep) * es;
    g.parts = (unsigned int)std::min<i64>(per_entry, (plane_cells + kThreads - 1) / kThreads);
    p.blocks = L * g.parts;
    p.read_lo = 0;
    p.read_hi = span;
    p.write_hi = (L - 1) * g.sk + (g.e1 - 1) * g.s1 + (g.e2 - 1) * g.s2 + es;
  } else {
    p.k.vec = 16;
    if (c != r.keep) {
      const int o = 3 - c - r.keep;
      p.k.kind = K_ROWS_PLANES;
      g.row_bytes = r.extent[c] * es;
      g.rows = r.extent[o];
      g.s1 = pitch(o) * es;
      g.sk = pitch(r.keep) * es;
      g.slots = (g.row_bytes + 14 + 15) / 16;
      g.p0 = std::min(8, ilog2ceil(g.slots));
      const i64 lpr = 1LL << g.p0, rows_per_tile = (i64)(kThreads >> g.p0) * kRowsUnroll;
      const i64 t0 = (g.slots + lpr - 1) / lpr, t1 = (g.rows + rows_per_tile - 1) / rows_per_tile;
      if (t0 > 0xffffffffLL || t1 > 0xffffffffLL) CD_NOT_SUPPORTED("a plane update of more than 2^32 - 1 tiles along one dim");
      g.t0 = (unsigned int)t0, g.t1 = (unsigned int)t1;
      g.parts = (unsigned int)std::min<i64>(per_entry, t0 * t1);
      p.blocks = L * g.parts;
      p.write_hi = (L - 1) * g.sk + (g.rows - 1) * g.s1 + g.row_bytes;
    } else {
      p.k.kind = K_COLUMNS_PLANES;
      g.row_bytes = L * es;
      g.e1 = r.extent[o1], g.e2 = r.extent[o2];
      g.s1 = pitch(o1) * es, g.s2 = pitch(o2) * es;
      g.rows = plane_cells;
      g.slots = (g.row_bytes + 14 + 15) / 16;
      g.p0 = std::min(5, ilog2ceil(g.slots));  // at most 32 slots per row-lane: eight row-lanes and more per workgroup
      const i64 lpr = 1LL << g.p0, rows_per_pass = (i64)(kThreads >> g.p0) * kRowsUnroll;
      const i64 t0 = (g.slots + lpr - 1) / lpr;
      if (t0 > 0xffffffLL) CD_NOT_SUPPORTED("a plane update of more than 2^24 - 1 tile columns");
      g.t0 = (unsigned int)t0;
      const i64 want = std::min<i64>(std::max<i64>(kProfileBlocks / t0, 1), (g.rows + rows_per_pass - 1) / rows_per_pass);
      g.rows_per_part = ((g.rows + want - 1) / want + rows_per_pass - 1) / rows_per_pass * rows_per_pass;  // whole passes
      g.parts = (unsigned int)((g.rows + g.rows_per_part - 1) / g.rows_per_part);
      p.blocks = t0 * g.parts;
      p.write_hi = (g.e1 - 1) * g.s1 + (g.e2 - 1) * g.s2 + g.row_bytes;
    }
    // what field 0 reads: whole 16-byte vectors from the boundary below the first cell to the boundary above the last, where the
    // readable range holds them; the cells alone where it does not (planProfile's closed form: the loads are loadSlot's)
    const uintptr_t first_cell = reinterpret_cast<uintptr_t>(r.a[0]) + (uintptr_t)g.box_off;
    const i64 below = (i64)(first_cell & 15), above = (i64)((16 - ((first_cell + (uintptr_t)span) & 15)) & 15);
    const auto whole = [&](i64 slot) { return slot >= g.rd_lo && slot + 16 <= g.rd_hi; };  // (the kernels' test of a vector)
    p.read_lo = whole(-below) ? -below : 0;
    p.read_hi = whole(span + above - 16) ? span + above : span;
  }
  p.write_lo = 0;  // (the first cell of the box is the first cell of its first row)
  if (p.blocks * r.n_fields > 0x7fffffffLL) CD_NOT_SUPPORTED("a plane update of more than 2^31 - 1 workgroups");
  return p;
}

void launchPlanes(const PlanesRequest& r, const double* coef, hipStream_t stream, KernelStats* stats) {
  const PlanesPlan p = planPlanes(r);
  if (p.g.parts == 0) return;  // an empty box
  for (int f = 0; f < r.n_fields; ++f)
    for (int e = 0; e < f; ++e)
      if (r.a[e] == r.a[f]) CD_INTERNAL_ERROR("a field is named twice in a plane update");
  PlanesFields fields;
  std::memset(&fields, 0, sizeof(fields));
  for (int f = 0; f < r.n_fields; ++f) fields.a[f] = static_cast<char*>(r.a[f]);
  if (p.k.kind == K_GENERIC_PLANES) {
    snprintf(g_last_kernel, sizeof(g_last_kernel), "planes_elements_kernel<%s>", arithName(p.k.arith));
  } else {
    const int mode = r.op == kPlanesAdd ? 0 : p.g.reals == 2 ? 2 : 1;
    snprintf(g_last_kernel, sizeof(g_last_kernel), "%s<%s,%d>", p.k.kind == K_ROWS_PLANES ? "planes_rows_kernel" : "planes_columns_kernel",
             arithName(p.k.arith), mode);
  }
  ++g_data_launches;
  if (p.k.kind == K_ROWS_PLANES) launchPlanesRows(p.k, p.g, fields, coef, stream);
  else launchPlanesColumnsOrElements(p.k, p.g, fields, coef, stream);
  if (stats) {
    const MoveClass cls = classOf(p.k.kind);
    stats->launches[cls] += 1;
    stats->elements[cls] += (i64)r.n_fields * r.extent[0] * r.extent[1] * r.extent[2];
  }
}

// ---------------------------------------------------------------------------------------------
// combinations of two boxes of cells (kernels_combine.hip)
// ---------------------------------------------------------------------------------------------
CombinePlan planCombine(const CombineRequest& r) {
  if (r.n_fields < 1 || r.n_fields > kMaxFields || !r.x || !r.y) CD_INTERNAL_ERROR("a combination of 1 .. kMaxFields fields");
  if (r.op < kCombineAxpy || r.op > kCombineAx) CD_INTERNAL_ERROR("combination operation out of range");
  if (r.arith == ARITH_NONE) CD_INTERNAL_ERROR("a combination needs the real type of its elements");
  if (r.coef_stride != 0 && r.coef_stride != 1) CD_INTERNAL_ERROR("the coefficient stride of a combination is 0 or 1");
  const int es = r.es, rs = arithBytes(r.arith);
  if (es != rs && es != 2 * rs) CD_INTERNAL_ERROR("element size does not match the real type");
  if (es == 2 * rs && r.arith == ARITH_BF16) CD_INTERNAL_ERROR("bf16 has no complex type");
  if (r.box_off < 0 || r.readable_before < 0 || r.readable_after < 0) CD_INTERNAL_ERROR("negative offset of a combination");
  const KernelTuning& tuning = r.tuning ? *r.tuning : kDefaultTuning;
  CombinePlan p;
  std::memset(&p, 0, sizeof(p));
  p.k.kind = K_GENERIC_COMBINE;
  p.k.es = es;
  p.k.vec = es;
  p.k.arith = r.arith;
  CombineGeom& g = p.g;
  g.reals = es / rs;
  g.n_fields = r.n_fields;
  g.op = r.op;
  g.a_scale = r.a_scale, g.b_scale = r.b_scale;
  g.coef_stride = r.coef_stride;
  g.box_off = r.box_off * es;
  i64 cells = 1, last = 0;  // `last`: the element offset of the box's last cell
  for (int i = 0; i < 3; ++i) {
    if (r.extent[i] < 0 || r.strides[i] < 0) CD_INTERNAL_ERROR("negative extent or stride of a combination");
    cells *= r.extent[i];
    last += (r.extent[i] - 1) * r.strides[i];
    g.e[i] = r.extent[i];
    g.s[i] = r.strides[i];
  }
  const i64 span = (last + 1) * es;
  g.rd_lo = -r.readable_before;
  g.rd_hi = span + r.readable_after;
  if (cells == 0) return p;  // (no launch: g.blocks == 0)
  const bool reads_y = r.op != kCombineAx;
  p.k.access = ((cells * es >= kStreamBytes || tuning.force_streaming) && !tuning.no_streaming) ? 1 : 0;

  // the dims that count, by stride; contiguous ones merged (planReduce's rules)
  i64 e[3], s[3];
  int nd;
  bool rows = mergeBoxDims(r.extent, r.strides, e, s, nd);
  // the row kernel's lanes lie on the 16-byte grid of y: every field on a boundary of its real type -- a complex one of its element,
  // whose two reals a lane pairs inside one vector -- and x[f] at the phase of y[f] on that grid
  const uintptr_t need = (uintptr_t)es;  // (es == rs for the real types)
  for (int f = 0; f < r.n_fields && rows; ++f) {
    const uintptr_t x = reinterpret_cast<uintptr_t>(r.x[f]), y = reinterpret_cast<uintptr_t>(r.y[f]);
    if (x % need != 0 || y % need != 0 || (x & 15) != (y & 15)) rows = false;
  }
  if (tuning.force_class == MOVE_GENERIC) rows = false;
  p.write_lo = 0, p.write_hi = span;  // (the first cell of the box is the first stored, the end of its last cell the end of the last)

  if (!rows) {
    g.p0 = 0;
    for (int i = 0; i < 3; ++i)
      if (r.strides[i] == 1 && r.extent[i] > 1) g.p0 = i;
    const i64 want = (cells + kThreads - 1) / kThreads;
    g.blocks = (unsigned int)std::min<i64>(std::max<i64>(want, 1), kCombineBlocks);
    p.read_x_lo = 0, p.read_x_hi = span;
    p.read_y_lo = 0, p.read_y_hi = reads_y ? span : 0;
  } else {
    p.k.kind = K_ROWS_COMBINE;
    p.k.vec = 16;
    g.stream = p.k.access;
    setRowWalk(g, e, s, nd, es);
    g.blocks = (unsigned int)std::min<unsigned long long>(g.tiles, kCombineBlocks);
    // what is read of x[0] and of y[0], which share their phase: whole 16-byte vectors from the boundary below the first cell to the
    // boundary above the last, where the readable range holds them; the cells alone where it does not (planReduce's closed form)
    const uintptr_t first_cell = reinterpret_cast<uintptr_t>(r.y[0]) + (uintptr_t)g.box_off;
    const i64 below = (i64)(first_cell & 15), above = (i64)((16 - ((first_cell + (uintptr_t)span) & 15)) & 15);
    const auto whole = [&](i64 slot) { return slot >= g.rd_lo && slot + 16 <= g.rd_hi; };  // (the kernel's test of a vector)
    p.read_x_lo = whole(-below) ? -below : 0;
    p.read_x_hi = whole(span + above - 16) ? span + above : span;
    if (reads_y) p.read_y_lo = p.read_x_lo, p.read_y_hi = p.read_x_hi;
  }
  p.blocks = g.blocks;
  if (p.blocks * r.n_fields > 0x7fffffffLL) CD_NOT_SUPPORTED("a combination of more than 2^31 - 1 workgroups");
  return p;
}

void launchCombine(const CombineRequest& r, const double* a_num, const double* a_den, const double* b_num, const double* b_den,
                   hipStream_t stream, KernelStats* stats) {
  const CombinePlan p = planCombine(r);
  if (p.g.blocks == 0) return;  // an empty box
  for (int f = 0; f < r.n_fields; ++f) {
    for (int e = 0; e < f; ++e)
      if (r.y[e] == r.y[f]) CD_INTERNAL_ERROR("a field is written twice in a combination");
    for (int e = 0; e < r.n_fields; ++e)
      if (r.x[e] == r.y[f]) CD_INTERNAL_ERROR("a field is read and written in a combination");
  }
  CombineFields fields;
  std::memset(&fields, 0, sizeof(fields));
  for (int f = 0; f < r.n_fields; ++f) fields.y[f] = static_cast<char*>(r.y[f]), fields.x[f] = static_cast<const char*>(r.x[f]);
  const bool uses_a = r.op != kCombineXpby, uses_b = r.op == kCombineXpby || r.op == kCombineAxpby;
  const CombineCoefs coefs = {uses_a ? a_num : nullptr, uses_a ? a_den : nullptr, uses_b ? b_num : nullptr, uses_b ? b_den : nullptr};
  if (p.k.kind == K_GENERIC_COMBINE)
    snprintf(g_last_kernel, sizeof(g_last_kernel), "combine_elements_kernel<%s>", arithName(p.k.arith));
  else
    snprintf(g_last_kernel, sizeof(g_last_kernel), "combine_rows_kernel<%s,%d,%s>", arithName(p.k.arith), r.op, p.g.reals == 2 ? "true" : "false");
  ++g_data_launches;
  if (p.k.kind == K_GENERIC_COMBINE) launchCombineElements(p.k, p.g, fields, coefs, stream);
  else if (arithBytes(p.k.arith) == 2) launchCombineRows2(p.k, p.g, fields, coefs, stream);
  else if (arithBytes(p.k.arith) == 4) launchCombineRows4(p.k, p.g, fields, coefs, stream);
  else launchCombineRows8(p.k, p.g, fields, coefs, stream);
  if (stats) {
    const MoveClass cls = classOf(p.k.kind);
    stats->launches[cls] += 1;
    stats->elements[cls] += (i64)r.n_fields * r.extent[0] * r.extent[1] * r.extent[2];
  }
}

}  // namespace cudecomp
