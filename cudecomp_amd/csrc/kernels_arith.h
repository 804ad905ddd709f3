// kernels_arith.h -- the addition of the add-moves (Move3D::add), shared by the code objects that add: kernels_accumulate.hip
// (dst += src) and kernels_take.hip (dst += src; src = 0).  a + b on raw lane payloads, in the arithmetic of the call's data type:
// T = _Float16 (IEEE binary16 addition, packed), __bf16 (RNE-to-bf16 of the fp32 sum of the widened operands), float, double.
#pragma once
#include "kernels_dev.h"

namespace cudecomp {
namespace kern {

typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef float f32x2 __attribute__((ext_vector_type(2)));

// ---- a + b on the raw bits of one T (2-byte types: of the PAIR held by a dword) ---------------------------------------------
template <typename T> struct Arith;
template <> struct Arith<float> {
  static __device__ __forceinline__ unsigned int dword(unsigned int a, unsigned int b) {
    return __float_as_uint(__uint_as_float(a) + __uint_as_float(b));
  }
};
template <> struct Arith<_Float16> {
  static __device__ __forceinline__ unsigned int dword(unsigned int a, unsigned int b) {  // v_pk_add_f16
    return __builtin_bit_cast(unsigned int, (f16x2)(__builtin_bit_cast(f16x2, a) + __builtin_bit_cast(f16x2, b)));
  }
  static __device__ __forceinline__ unsigned short one(unsigned short a, unsigned short b) {
    return __builtin_bit_cast(unsigned short, (_Float16)(__builtin_bit_cast(_Float16, a) + __builtin_bit_cast(_Float16, b)));
  }
};
template <> struct Arith<__bf16> {
  // widening is a shift (exact); the fp32 sums are rounded to nearest even by the packed convert (v_cvt_pk_bf16_f32)
  static __device__ __forceinline__ unsigned int dword(unsigned int a, unsigned int b) {
    f32x2 s;
    s.x = __uint_as_float(a << 16) + __uint_as_float(b << 16);
    s.y = __uint_as_float(a & 0xffff0000u) + __uint_as_float(b & 0xffff0000u);
    return __builtin_bit_cast(unsigned int, __builtin_convertvector(s, bf16x2));
  }
  static __device__ __forceinline__ unsigned short one(unsigned short a, unsigned short b) {
    const float s = __uint_as_float((unsigned int)a << 16) + __uint_as_float((unsigned int)b << 16);
    return __builtin_bit_cast(unsigned short, (__bf16)s);
  }
};
__device__ __forceinline__ u32x2 addDouble(const u32x2& a, const u32x2& b) {
  return __builtin_bit_cast(u32x2, __builtin_bit_cast(double, a) + __builtin_bit_cast(double, b));
}

// ---- a + b and a * b on ONE real held as its type (the plane updates, kernels_planes.hip): IEEE for _Float16, float and double;
// __bf16: RNE-to-bf16 of the fp32 result of the widened operands, as Arith<__bf16> above.  Every result is rounded on its own: no
// caller's expression is contracted into an fma through these
template <typename T, int OP> __device__ __forceinline__ T arithReal(T a, T b) {  // OP 0: a + b, 1: a * b, 2: a - b
#pragma clang fp contract(off)
  if constexpr (sizeof(T) == 2 && !__is_same(T, _Float16)) {
    const float x = __uint_as_float((unsigned int)__builtin_bit_cast(unsigned short, a) << 16);
    const float y = __uint_as_float((unsigned int)__builtin_bit_cast(unsigned short, b) << 16);
    const float s = OP == 0 ? x + y : OP == 1 ? x * y : x - y;
    return (__bf16)s;
  } else {
    return OP == 0 ? (T)(a + b) : OP == 1 ? (T)(a * b) : (T)(a - b);
  }
}
template <typename T> __device__ __forceinline__ T addReal(T a, T b) { return arithReal<T, 0>(a, b); }
template <typename T> __device__ __forceinline__ T mulReal(T a, T b) { return arithReal<T, 1>(a, b); }
template <typename T> __device__ __forceinline__ T subReal(T a, T b) { return arithReal<T, 2>(a, b); }

// a + b over a VB-byte lane payload
template <typename T, int VB>
__device__ __forceinline__ Bytes<VB> addPayload(const Bytes<VB>& a, const Bytes<VB>& b) {
  static_assert(VB >= (int)sizeof(T), "a lane holds whole elements");
  if constexpr (sizeof(T) == 8) {
    if constexpr (VB == 8) {
      return addDouble(a, b);
    } else {
      u32x4 r;
      r.xy = addDouble(a.xy, b.xy);
      r.zw = addDouble(a.zw, b.zw);
      return r;
    }
  } else if constexpr (VB == 2) {
    return Arith<T>::one(a, b);
  } else if constexpr (VB == 4) {
    return Arith<T>::dword(a, b);
  } else {
    Bytes<VB> r;
#pragma unroll
    for (int k = 0; k < VB / 4; ++k) r[k] = Arith<T>::dword(a[k], b[k]);
    return r;
  }
}

}  // namespace kern
}  // namespace cudecomp
