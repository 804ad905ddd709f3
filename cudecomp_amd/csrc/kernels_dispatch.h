// kernels_dispatch.h -- host side of the kernel code objects: from the numbers of a KernelChoice (kernels_batch.h) to the template
// arguments of the instantiation that serves it.  Each function calls a generic lambda with a tag type and answers false when no
// instantiation exists; the lambda names the kernel, so every launcher spells its ladder once:
//   dispatchArith(k.arith, [&](auto t) { using T = typename decltype(t)::type;
//     return dispatchLaneWidth<T>(k.vec, [&](auto w) { dispatchAccess(s, [&](auto a) {
//       some_kernel<T, decltype(w)::value, decltype(a)::value><<<grid, block, 0, stream>>>(b); }); }); });
// Only what is listed is instantiated: the forms no data type can reach (lanes narrower than a real) never exist.
// Included by the .hip files only.
#pragma once
#include <type_traits>

#include "kernels_batch.h"

namespace cudecomp {
namespace kern {

template <typename T> struct TypeTag {
  using type = T;
};

// f(std::integral_constant<int, V>) for the V of the list that equals v
template <int... Vs, typename F> bool dispatchInt(int v, F&& f) {
  return ((v == Vs ? (f(std::integral_constant<int, Vs>{}), true) : false) || ...);
}

// the real type of an addition, a fold or a sign flip; f returns whether it found its kernel
template <typename F> bool dispatchArith(ArithType arith, F&& f) {
  switch (arith) {
    case ARITH_F16: return f(TypeTag<_Float16>{});
    case ARITH_BF16: return f(TypeTag<__bf16>{});
    case ARITH_F32: return f(TypeTag<float>{});
    case ARITH_F64: return f(TypeTag<double>{});
    default: return false;
  }
}

// bytes per lane of a row kernel whose lanes hold whole reals of T: 8-byte reals take 16 or 8 bytes, 4-byte reals 4 as well,
// 2-byte reals 2 as well.  (Kernels without a real type pass a 2-byte one: every width.)
template <typename T, typename F> bool dispatchLaneWidth(int vb, F&& f) {
  if constexpr (sizeof(T) == 2) return dispatchInt<16, 8, 4, 2>(vb, f);
  else if constexpr (sizeof(T) == 4) return dispatchInt<16, 8, 4>(vb, f);
  else return dispatchInt<16, 8>(vb, f);
}

// reals per element of an element-wise kernel with a real type: 1, or 2 for the complex types; bf16 has no complex type
template <typename T, typename F> bool dispatchReals(int es, F&& f) {
  if constexpr (std::is_same<T, __bf16>::value) return dispatchInt<1>(es / (int)sizeof(T), f);
  else return dispatchInt<1, 2>(es / (int)sizeof(T), f);
}

// element sizes of the untyped element-wise kernels
template <typename F> bool dispatchElementSize(int es, F&& f) { return dispatchInt<2, 4, 8, 16>(es, f); }

// the STREAM argument of the kernels with two access modes: 1 streaming, everything else default caching
template <typename F> void dispatchAccess(int stream_arg, F&& f) { dispatchInt<0, 1>(stream_arg == 1 ? 1 : 0, f); }

// f(std::true_type) or f(std::false_type); answers what f answers
template <typename F> auto dispatchBool(bool v, F&& f) {
  if (v) return f(std::true_type{});
  return f(std::false_type{});
}

}  // namespace kern
}  // namespace cudecomp
