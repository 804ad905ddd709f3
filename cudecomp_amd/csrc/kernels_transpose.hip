// kernels_transpose.hip -- instantiations of the LDS-tiled transposition (kernels_tile.h) for ONE element size; compiled four
// times (-DCUDECOMP_TRANSPOSE_ES=2 | 4 | 8 | 16), i.e. four code objects (see kernels_dev.h for why there are several).
//
// Tiles per element size (elements, i x j; i runs along the source rows, j along the destination rows):
//    2-byte  128 x 128 with 16-byte lanes (8 elements per lane, the 8 x 8 block transposed by byte permutes), 64 x 64
//            element-wise (odd extents, rows at 2 mod 4: kernels.cc classify())
//    4-byte   64 x 128 with 16-byte lanes (512-byte destination segments: profiles/r04_tuning.md), 64 x 64 element-wise
//    8-byte   64 x 64; 64 x 128 for large moves whose SOURCE rows are the far-strided side (profiles/r05_tuning.md)
//   16-byte   32 x 32 (padded LDS rows; the swizzled layout measures slower for them); 32 x 64 for far-strided sources
// Access modes 0 / 2 / 3 / 4 (storePolicyOf).
#include "kernels_tile.h"

#include "errors.h"

#ifndef CUDECOMP_TRANSPOSE_ES
#error "compile with -DCUDECOMP_TRANSPOSE_ES=2, 4, 8 or 16"
#endif

namespace cudecomp {
using namespace kern;

namespace {

constexpr bool SWZ = CUDECOMP_TRANSPOSE_ES != 16;  // XOR-swizzled LDS tile; 16-byte elements: padded rows

template <int STREAM>
bool launchT(const KernelChoice& k, const Batch& b, unsigned int blocks, hipStream_t stream) {
#if CUDECOMP_TRANSPOSE_ES == 2
  CD_TILED_SHAPE(transpose_kernel, 2, 8, 128, 128, STREAM, SWZ)
  CD_TILED_SHAPE(transpose_kernel, 2, 1, 64, 64, STREAM, SWZ)
#elif CUDECOMP_TRANSPOSE_ES == 4
  CD_TILED_SHAPE(transpose_kernel, 4, 4, 64, 128, STREAM, SWZ)
  CD_TILED_SHAPE(transpose_kernel, 4, 1, 64, 64, STREAM, SWZ)
#elif CUDECOMP_TRANSPOSE_ES == 8
  if constexpr (STREAM == 2) {  // (the longer tiles are instantiated for streaming moves only)
    CD_TILED_SHAPE(transpose_kernel, 8, 2, 64, 128, 2, true)
  }
  CD_TILED_SHAPE(transpose_kernel, 8, 2, 64, 64, STREAM, SWZ)
  CD_TILED_SHAPE(transpose_kernel, 8, 1, 64, 64, STREAM, SWZ)
#else
  if constexpr (STREAM == 2) {  // (as for 8-byte elements)
    CD_TILED_SHAPE(transpose_kernel, 16, 1, 32, 64, 2, false)
  }
  CD_TILED_SHAPE(transpose_kernel, 16, 1, 32, 32, STREAM, SWZ)
#endif
  return false;
}

void launchAny(const KernelChoice& k, const Batch& b, unsigned int blocks, hipStream_t stream) {
  const int s = streamArgOf(k.kind, k.access);
  const bool ok = s == 4 ? launchT<4>(k, b, blocks, stream)
                         : (s == 3 ? launchT<3>(k, b, blocks, stream) : (s == 2 ? launchT<2>(k, b, blocks, stream) : launchT<0>(k, b, blocks, stream)));
  if (!ok) CD_INTERNAL_ERROR("no transpose kernel of this element size for this lane width, tile and access mode");
  CD_CHECK_HIP(hipGetLastError());
}

}  // namespace

#if CUDECOMP_TRANSPOSE_ES == 2
void launchTransposeBatch2(const KernelChoice& k, const Batch& b, unsigned int blocks, hipStream_t stream) { launchAny(k, b, blocks, stream); }
#elif CUDECOMP_TRANSPOSE_ES == 4
void launchTransposeBatch4(const KernelChoice& k, const Batch& b, unsigned int blocks, hipStream_t stream) { launchAny(k, b, blocks, stream); }
#elif CUDECOMP_TRANSPOSE_ES == 8
void launchTransposeBatch8(const KernelChoice& k, const Batch& b, unsigned int blocks, hipStream_t stream) { launchAny(k, b, blocks, stream); }
#else
void launchTransposeBatch16(const KernelChoice& k, const Batch& b, unsigned int blocks, hipStream_t stream) { launchAny(k, b, blocks, stream); }
#endif

}  // namespace cudecomp

// the combinations of two boxes (kernels_combine.hip) are compiled into these units, one part each -- the row kernel of the real types
// as wide as this unit's elements, and the element-wise kernel in the unit of the 16-byte elements: the family cannot be a code object
// of its own, and these four have the room (kernels_batch.h says why the library keeps the number of its code objects)
#define CD_COMBINE_PART CUDECOMP_TRANSPOSE_ES
#include "kernels_combine.hip"
