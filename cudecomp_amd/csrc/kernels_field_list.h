// kernels_field_list.h -- the workgroup decode of the lists of field-moves (kern::FieldMoveBatch, kernels_batch.h), shared by the
// code objects that serve them: kernels_field_transpose.hip (copies), kernels_field_accumulate.hip (additions and takes) and
// kernels_field_mirror.hip (reflections and folds with a sign per field).
#pragma once
#include "kernels_dev.h"

namespace cudecomp {
namespace kern {

// workgroup -> (move, field, workgroup index inside that field's move)
__device__ __forceinline__ void locateFieldMove(const FieldMoveBatch& b, unsigned int block, int& mi, unsigned int& f, unsigned int& lb) {
  mi = 0;
#pragma unroll
  for (int i = 1; i < kMaxBatch; ++i)
    if (i < b.n && block >= b.first_block[i]) mi = i;
  const unsigned int rel = block - b.first_block[mi];
  const unsigned int per = b.m[mi].blocks;
  f = rel / per;
  lb = rel - f * per;
}

__device__ __forceinline__ const char* sourceOf(const FieldMoveBatch& b, const FieldMove& m, unsigned int f) {
  const char* base = m.src_end == kEndWork ? b.work + (long long)f * m.src_step : (m.src_end == kEndOutput ? b.out[f] : b.in[f]);
  return base + m.src_off;
}
__device__ __forceinline__ char* destinationOf(const FieldMoveBatch& b, const FieldMove& m, unsigned int f) {
  char* base = m.dst_end == kEndWork ? b.work + (long long)f * m.dst_step : (m.dst_end == kEndOutput ? b.out[f] : b.in[f]);
  return base + m.dst_off;
}

}  // namespace kern
}  // namespace cudecomp
