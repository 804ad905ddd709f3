// filler_kernels.h -- device code that is never launched, to grow a code object by a chosen amount (code-size bisect of round 5:
// a code object of its own through scripts/probe/filler.hip, or -include'd into one of the library's .hip files).
// -DFILLER_NK=<kernels> -DFILLER_BODY=<statements per kernel>.
#pragma once
#include <hip/hip_runtime.h>

#include <utility>
#ifndef FILLER_NK
#define FILLER_NK 48
#endif
#ifndef FILLER_BODY
#define FILLER_BODY 256
#endif
template <int I>
__global__ void cudecomp_filler_k(float* p) {
  float a = p[threadIdx.x], b = p[threadIdx.x + 64];
#pragma unroll
  for (int k = 0; k < FILLER_BODY; ++k) {
    a = a * (1.0f + 0.001f * (I * 131 + k)) + b;
    b = b * (0.5f + 0.003f * (I * 17 + k * 3)) - a;
  }
  p[threadIdx.x] = a + b;
}
typedef void (*cudecomp_filler_fn)(float*);
template <int... Is>
static void cudecompFillerTable(cudecomp_filler_fn* t, std::integer_sequence<int, Is...>) {
  ((t[Is] = cudecomp_filler_k<Is>), ...);
}
// referenced so that the kernels are emitted; never called
extern "C" __attribute__((visibility("default"), used)) void cudecomp_filler_anchor(cudecomp_filler_fn* t) {
  cudecompFillerTable(t, std::make_integer_sequence<int, FILLER_NK>{});
}
