// halo_wall_values_test.cpp -- wall values (cudecomp_halo_wall_values.h: cudecompAmdSetWallHalos{X,Y,Z}) as a C / C++ solver calls
// them: through the header's prototypes, nothing else.  Per case: one pencil is uploaded and the call runs along dims 0, 1, 2 in turn
// through the X, Y or Z entry point of --ax; after every call the WHOLE buffer -- halos of all dims, padding and a poisoned tail
// behind the pencil -- is downloaded and compared, bit for bit, with the header's definition applied on the host to the whole pencil:
// on the sides that --sides names AND where cudecompGetShiftedRank names no neighbour, for k in [0, h), c = --centering and s =
// --parity,
//   low side:   cell(h-1-k) = s cell(h+k+c)     + a_low[k]
//   high side:  cell(n-h+k) = s cell(n-h-1-k-c) + a_high[k]
// the other two dims run over their halos and not over their padding.  A dim along which the rank has a wall, a halo and a named
// side must have changed the pencil: otherwise the case shows nothing and fails.  Command line, test-file mode and output protocol
// of halo_test.cpp (native_test.h).
//
// Payload: cell e (its position in the buffer) holds payload(e, 0) of halo_wall_fields_test.cpp, the imaginary part of a complex
// element payload(e, 50): 1 .. 11 without a pattern along any stride; padding cells and the tail hold -77.
//
// Addends: exact integers, distinct per layer, side and called dim, never zero.  With k1 = k + 1 (layer 1 next to the wall) and d =
// dim + 1: a_low[k] = 100 + 10 k1 + d, a_high[k] = -(200 + 10 k1 + d); the imaginary parts are a_low[k] + 5 and a_high[k] - 5.  A
// ghost value grows by at most 233 (238 for an imaginary part) per dim, so every magnitude stays below 11 + 3 * 238 = 725 < 2048:
// every sum is exact in fp16 and in every wider type.  A sum of two non-zero operands that cancels is +0 in round-to-nearest, never
// -0: the host model is integer arithmetic, compared bit for bit, without a tolerance.
//
// The value arrays live in a scope of their own and are overwritten with NaNs as soon as the call has returned, BEFORE any
// synchronisation ("they may be temporaries"); the array of the side that --sides leaves out is NULL or an array of NaNs ("is not
// looked at and may be NULL").
//
//   the options of halo_test, plus
//   --parity P            +1 / -1
//   --centering C         0 / 1
//   --sides S             1 low, 2 high, 3 both
//   --nullpad             pass padding = NULL (only valid when the padding is zero)
//   --unnamed null | garbage   what is passed for the side --sides leaves out: NULL, or NaNs that must leave no trace
//   --expect-refusal invalid | unsupported  --dim D   ONE call along D: it must return CUDECOMP_RESULT_INVALID_USAGE /
//                         CUDECOMP_RESULT_NOT_SUPPORTED and leave the pencil byte-identical (--sides is passed as given)
//   --named-null          (with --expect-refusal) NULL for the sides that --sides names
//   --self-check-reverse-layers          the expectation uses a[h-1-k]: the case must FAIL
//   --self-check-swap-sides              the expectation exchanges the two arrays: the case must FAIL
#include "native_test.h"

#include <limits>

#include "cudecomp_halo_wall_values.h"

namespace {

const int kPoison = -77, kTailElements = 64;

#if defined(C64) || defined(C32)
const int kComp = 2;
#else
const int kComp = 1;
#endif
#if defined(H16)
using real_t = uint16_t;
#elif defined(R32) || defined(C32)
using real_t = float;
#else
using real_t = double;
#endif

int payload(int64_t e, int f) {
  const int64_t m = 2147483647;
  return (int)(((2654435761LL * e + 97 * f) % m * 48271 % m) % 11) + 1;
}

real_t encodeReal(int v) {
#if defined(H16)
  return halfBitsOfInt(v);
#else
  return (real_t)v;
#endif
}

// component q of the addend of ghost layer k (zero-based) on `side` (0 low, 1 high) for the call along `dim`
int addend(int side, int k, int dim, int q) {
  const int base = 10 * (k + 1) + (dim + 1);
  return side == 0 ? 100 + base + 5 * q : -(200 + base + 5 * q);
}

// the prototype as the header gives it; a mismatch with the definitions is a compile error here or a wrong result below
typedef cudecompResult_t (*wall_values_fn)(cudecompHandle_t, cudecompGridDesc_t, void*, cudecompDataType_t, int32_t, int32_t, int32_t,
                                           const double[], const double[], const int32_t[], const bool[], int32_t, const int32_t[],
                                           hipStream_t);
wall_values_fn const kSetWall[3] = {cudecompAmdSetWallHalosX, cudecompAmdSetWallHalosY, cudecompAmdSetWallHalosZ};

int runCase(cudecompHandle_t handle, const Options& o, bool silent) {
  const int rank = worldRank();
  const std::array<int, 3> g = {o.geti("gx", 256), o.geti("gy", 256), o.geti("gz", 256)};
  const std::array<int, 3> gd = o.get3("gd", {0, 0, 0});
  const std::array<int, 3> halo = {o.geti("hex", 1), o.geti("hey", 1), o.geti("hez", 1)};
  const bool pb[3] = {o.geti("hpx", 1) != 0, o.geti("hpy", 1) != 0, o.geti("hpz", 1) != 0};
  const std::array<int, 3> pad = {o.geti("pdx", 0), o.geti("pdy", 0), o.geti("pdz", 0)};
  const int axis = o.geti("ax", 0), backend = o.geti("backend", 0), centering = o.geti("centering", 0), parity = o.geti("parity", 1),
            sides = o.geti("sides", 3);
  if (axis < 0 || axis > 2) throw TestFailure("--ax out of range");
  if (parity != 1 && parity != -1) throw TestFailure("--parity must be +1 or -1");
  if (centering != 0 && centering != 1) throw TestFailure("--centering out of range");
  const bool nullpad = o.has("nullpad"), refusal = o.has("expect-refusal"), named_null = o.has("named-null");
  const bool reverse = o.has("self-check-reverse-layers"), swap = o.has("self-check-swap-sides");
  if (nullpad && (pad[0] || pad[1] || pad[2])) throw TestFailure("--nullpad needs zero padding");
  if (!refusal && (sides < 1 || sides > 3)) throw TestFailure("--sides must be 1, 2 or 3");
  if (named_null && !refusal) throw TestFailure("--named-null needs --expect-refusal");
  bool garbage = false;
  if (o.has("unnamed")) {
    const std::vector<std::string>& u = o.values.at("unnamed");
    if (u.size() != 1 || (u[0] != "null" && u[0] != "garbage")) throw TestFailure("--unnamed must be null or garbage");
    garbage = u[0] == "garbage";
  }
  cudecompResult_t expected = CUDECOMP_RESULT_SUCCESS;
  if (refusal) {
    const std::vector<std::string>& e = o.values.at("expect-refusal");
    if (e.size() == 1 && e[0] == "invalid") expected = CUDECOMP_RESULT_INVALID_USAGE;
    else if (e.size() == 1 && e[0] == "unsupported") expected = CUDECOMP_RESULT_NOT_SUPPORTED;
    else throw TestFailure("--expect-refusal must be invalid or unsupported");
    if (!o.has("dim") || o.geti("dim", -1) < 0 || o.geti("dim", -1) > 2) throw TestFailure("--expect-refusal needs --dim 0 .. 2");
  }

  cudecompGridDescConfig_t config;
  T_CHECK_CD(cudecompGridDescConfigSetDefaults(&config));
  config.pdims[0] = o.geti("pr", 0);
  config.pdims[1] = o.geti("pc", 0);
  config.rank_order = (cudecompRankOrder_t)o.geti("rank-order", 0);
  for (int i = 0; i < 3; ++i) {
    config.gdims[i] = g[i];
    config.gdims_dist[i] = g[i] - gd[i];
    config.transpose_axis_contiguous[i] = o.geti("ac", 0) != 0;
  }
  if (o.has("mem_order")) {
    for (int ax = 0; ax < 3; ++ax)
      for (int i = 0; i < 3; ++i) config.transpose_mem_order[ax][i] = (ax == axis) ? o.geti("mem_order", i, i) : i;
  }
  if (backend == 0) throw TestFailure("--backend is required (no autotuning here)");
  config.halo_comm_backend = (cudecompHaloCommBackend_t)backend;

  cudecompGridDesc_t gdesc;
  T_CHECK_CD(cudecompGridDescCreate(handle, &gdesc, &config, nullptr));
  if (!silent && rank == 0)
    printf("running the wall values (parity %d, centering %d, sides %d) on %d x %d x %d spatial grid, %d x %d process grid...\n", parity,
           centering, sides, g[0], g[1], g[2], config.pdims[0], config.pdims[1]);

  int failures = 0;
  void* dev = nullptr;
  try {
    cudecompPencilInfo_t p;
    int32_t halo32[3] = {halo[0], halo[1], halo[2]}, pad32[3] = {pad[0], pad[1], pad[2]};
    T_CHECK_CD(cudecompGetPencilInfo(handle, gdesc, &p, axis, halo32, pad32));
    const int64_t reals = (int64_t)(p.size + kTailElements) * kComp;
    const size_t total_bytes = (size_t)reals * sizeof(real_t);
    const int32_t* pad_arg = nullptr;
    if (!nullpad) pad_arg = pad32;

    // the pencil's own cells: extent without padding and stride of every memory position
    int64_t ext[3], stride[3];
    for (int k = 0; k < 3; ++k) {
      ext[k] = (p.hi[k] - p.lo[k] + 1) + 2 * halo[p.order[k]];
      stride[k] = k == 0 ? 1 : stride[k - 1] * p.shape[k - 1];
    }
    // the model: small integers per real, poison in the padding and the tail
    std::vector<int> m((size_t)reals, kPoison);
    for (int64_t i2 = 0; i2 < ext[2]; ++i2)
      for (int64_t i1 = 0; i1 < ext[1]; ++i1)
        for (int64_t i0 = 0; i0 < ext[0]; ++i0) {
          const int64_t e = i0 + i1 * stride[1] + i2 * stride[2];
          m[e * kComp] = payload(e, 0);
          if (kComp == 2) m[e * kComp + 1] = payload(e, 50);
        }
    std::vector<real_t> host((size_t)reals), want((size_t)reals);
    for (int64_t e = 0; e < reals; ++e) want[e] = encodeReal(m[e]);
    T_CHECK_HIP(hipMalloc(&dev, total_bytes));
    uploadPencil(dev, want.data(), total_bytes);

    const int first = refusal ? o.geti("dim", 0) : 0, last = refusal ? first : 2;
    for (int dim = first; dim <= last; ++dim) {
      int32_t lo = -1, hi = -1;
      T_CHECK_CD(cudecompGetShiftedRank(handle, gdesc, axis, dim, -1, pb[dim], &lo));
      T_CHECK_CD(cudecompGetShiftedRank(handle, gdesc, axis, dim, +1, pb[dim], &hi));
      // a side is written where it is named and the rank owns the domain's edge
      const bool writes[2] = {!refusal && (sides & 1) && lo == -1, !refusal && (sides & 2) && hi == -1};
      const bool active = halo[dim] > 0 && (writes[0] || writes[1]);
      const int h = halo[dim], len = std::max(1, h * kComp);
      cudecompResult_t r;
      {  // the value arrays are temporaries: they end with this scope, and hold NaNs from the moment the call has returned
        const double nan = std::numeric_limits<double>::quiet_NaN();
        std::vector<double> values[2] = {std::vector<double>((size_t)len, nan), std::vector<double>((size_t)len, nan)};
        const double* arg[2] = {nullptr, nullptr};
        for (int side = 0; side < 2; ++side) {
          const bool named = refusal ? (sides < 1 || sides > 3 || (sides & (1 << side)) != 0) : (sides & (1 << side)) != 0;
          if (named) {
            for (int k = 0; k < h; ++k)
              for (int q = 0; q < kComp; ++q) values[side][(size_t)k * kComp + q] = addend(side, k, dim, q);
            if (!named_null) arg[side] = values[side].data();
          } else if (garbage) {
            arg[side] = values[side].data();  // NaNs
          }
        }
        r = kSetWall[axis](handle, gdesc, dev, kDtype, parity, centering, sides, arg[0], arg[1], halo32, pb, dim, pad_arg, 0);
        for (int side = 0; side < 2; ++side) std::fill(values[side].begin(), values[side].end(), nan);
      }
      if (r != expected) {
        fprintf(stderr, "rank %d: the call along dim %d returned %d, not %d\n", rank, dim, (int)r, (int)expected);
        ++failures;
        if (r != CUDECOMP_RESULT_SUCCESS) break;
      }
      T_CHECK_HIP(hipDeviceSynchronize());
      // the header's definition on the model
      int km = 0;  // the memory position of `dim`
      for (int k = 0; k < 3; ++k)
        if (p.order[k] == dim) km = k;
      const int ka = (km + 1) % 3, kb = (km + 2) % 3;
      const int64_t n = ext[km], c = centering;
      const std::vector<int> before = m;
      for (int side = 0; side < 2 && h > 0; ++side) {
        if (!writes[side]) continue;
        for (int64_t k = 0; k < h; ++k) {
          const int64_t ghost = side == 0 ? h - 1 - k : n - h + k, inner = side == 0 ? h + k + c : n - h - 1 - k - c;
          const int a_side = swap ? 1 - side : side, a_k = reverse ? (int)(h - 1 - k) : (int)k;
          for (int64_t ia = 0; ia < ext[ka]; ++ia)
            for (int64_t ib = 0; ib < ext[kb]; ++ib)
              for (int q = 0; q < kComp; ++q) {
                const int64_t at = ia * stride[ka] + ib * stride[kb];
                m[(at + ghost * stride[km]) * kComp + q] = parity * m[(at + inner * stride[km]) * kComp + q] + addend(a_side, a_k, dim, q);
              }
        }
      }
      T_CHECK_HIP(hipMemcpy(host.data(), dev, total_bytes, hipMemcpyDeviceToHost));
      for (int64_t e = 0; e < reals; ++e) want[e] = encodeReal(m[e]);
      int64_t bad = 0;
      for (int64_t e = 0; e < reals; ++e) {
        if (!std::memcmp(&host[e], &want[e], sizeof(real_t))) continue;
        if (++bad > 2) continue;
        const int64_t cell = e / kComp;
        fprintf(stderr, "rank %d: dim %d: element %lld (%lld, %lld, %lld of %d x %d x %d, order %d %d %d) is not what the header says\n", rank, dim,
                (long long)cell, (long long)(cell % p.shape[0]), (long long)((cell / p.shape[0]) % p.shape[1]),
                (long long)(cell / ((int64_t)p.shape[0] * p.shape[1])), p.shape[0], p.shape[1], p.shape[2], p.order[0], p.order[1], p.order[2]);
      }
      if (bad) {
        fprintf(stderr, "rank %d: %lld reals differ after the wall values along dim %d\n", rank, (long long)bad, dim);
        ++failures;
      }
      if (active && m == before) {
        fprintf(stderr, "rank %d: the definition along dim %d changed nothing: the case shows nothing\n", rank, dim);
        ++failures;
      }
      if ((reverse || swap) && failures) break;  // the model has left the pencil: nothing more to learn
    }
    if ((reverse || swap) && !failures) fprintf(stderr, "rank %d: the altered expectation went unnoticed\n", rank);
  } catch (...) {
    if (dev) (void)hipFree(dev);
    (void)cudecompGridDescDestroy(handle, gdesc);
    throw;
  }
  if (dev) (void)hipFree(dev);
  notePaths(handle, gdesc);
  T_CHECK_CD(cudecompGridDescDestroy(handle, gdesc));
  return failures ? 1 : 0;
}

}  // namespace

int main(int argc, char** argv) { return nativeMain(argc, argv, runCase); }
