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
void launchT(int variant, const Batch& b, unsigned int blocks, hipStream_t stream) {
  const dim3 grid(blocks), block(kThreads);
#if CUDECOMP_TRANSPOSE_ES == 2
  if (variant == 8) transpose_kernel<2, 8, 128, 128, STREAM, SWZ><<<grid, block, 0, stream>>>(b);
  else transpose_kernel<2, 1, 64, 64, STREAM, SWZ><<<grid, block, 0, stream>>>(b);
#elif CUDECOMP_TRANSPOSE_ES == 4
  if (variant == 304) transpose_kernel<4, 4, 64, 128, STREAM, SWZ><<<grid, block, 0, stream>>>(b);
  else transpose_kernel<4, 1, 64, 64, STREAM, SWZ><<<grid, block, 0, stream>>>(b);
#elif CUDECOMP_TRANSPOSE_ES == 8
  if (variant == 302) {
    if constexpr (STREAM == 2) transpose_kernel<8, 2, 64, 128, 2, true><<<grid, block, 0, stream>>>(b);
    else CD_INTERNAL_ERROR("64 x 128 tiles are instantiated for streaming moves only");
  } else if (variant == 2) transpose_kernel<8, 2, 64, 64, STREAM, SWZ><<<grid, block, 0, stream>>>(b);
  else transpose_kernel<8, 1, 64, 64, STREAM, SWZ><<<grid, block, 0, stream>>>(b);
#else
  if (variant == 301) {
    if constexpr (STREAM == 2) transpose_kernel<16, 1, 32, 64, 2, false><<<grid, block, 0, stream>>>(b);
    else CD_INTERNAL_ERROR("32 x 64 tiles are instantiated for streaming moves only");
  } else transpose_kernel<16, 1, 32, 32, STREAM, SWZ><<<grid, block, 0, stream>>>(b);
#endif
  CD_CHECK_HIP(hipGetLastError());
}

void launchAny(int variant, int stream_access, const Batch& b, unsigned int blocks, hipStream_t stream) {
  if (stream_access == 4) launchT<4>(variant, b, blocks, stream);
  else if (stream_access == 3) launchT<3>(variant, b, blocks, stream);
  else if (stream_access == 2) launchT<2>(variant, b, blocks, stream);
  else launchT<0>(variant, b, blocks, stream);
}

}  // namespace

#if CUDECOMP_TRANSPOSE_ES == 2
void launchTransposeBatch2(int variant, int stream_access, const Batch& b, unsigned int blocks, hipStream_t stream) {
  launchAny(variant, stream_access, b, blocks, stream);
}
#elif CUDECOMP_TRANSPOSE_ES == 4
void launchTransposeBatch4(int variant, int stream_access, const Batch& b, unsigned int blocks, hipStream_t stream) {
  launchAny(variant, stream_access, b, blocks, stream);
}
#elif CUDECOMP_TRANSPOSE_ES == 8
void launchTransposeBatch8(int variant, int stream_access, const Batch& b, unsigned int blocks, hipStream_t stream) {
  launchAny(variant, stream_access, b, blocks, stream);
}
#else
void launchTransposeBatch16(int variant, int stream_access, const Batch& b, unsigned int blocks, hipStream_t stream) {
  launchAny(variant, stream_access, b, blocks, stream);
}
#endif

}  // namespace cudecomp
