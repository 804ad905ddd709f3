// halo_wall_fields_test.cpp -- multi-field wall halos (cudecomp_halo_wall_fields.h: cudecompAmdReflectFieldHalos{X,Y,Z},
// cudecompAmdFoldFieldHalos{X,Y,Z}) as a C / C++ solver calls them: through the header's prototypes, nothing else.  Per case: one
// pencil per entry of --parities is uploaded; --op reflect runs the field reflection along dims 0, 1, 2 in turn, --op fold the field
// fold (--clear 0 / 1) along dims 2, 1, 0, through the X, Y or Z entry point of --ax; after every dim every field is downloaded and
// the WHOLE buffer -- halos of all dims, padding and a poisoned tail behind the pencil -- is compared with the header's formulas
// applied on the host to the whole pencil: on the sides where cudecompGetShiftedRank names no neighbour, for k in [0, h) and c =
// --centering, the reflection sets cell(h-1-k) = s cell(h+k+c) and cell(n-h+k) = s cell(n-h-1-k-c); the fold adds cell(h+k+c) += s
// cell(h-1-k), then cell(n-h-1-k-c) += s cell(n-h+k), and with --clear 1 leaves zero in the ghost cells it has read; s = the field's
// parity; the other two dims run over their halos and not over their padding.  A dim along which the rank has a wall and a halo
// must have changed every field.  Command line, test-file mode and output protocol of halo_test.cpp (native_test.h).
//
// Payload: field f, cell e (its position in the buffer) holds payload(e, f) = (48271 ((2654435761 e + 97 f) mod (2^31 - 1)) mod (2^31 - 1))
// mod 11 + 1, the imaginary part of a complex element payload(e, f + 50): 1 .. 11 without a pattern along any stride (a linear
// congruence in e repeats along the mirrored dim of some pencils, and a mirror then changes nothing), and no zero, so that a flipped
// sign always shows; padding cells and the tail hold -77.  Small integers, exact in every type used (fp16 up to 2048); a cell is the
// sum of at most 8 cells.
//
//   the options of halo_test, plus
//   --op reflect | fold
//   --parities P0 P1 ...  one +1 / -1 per field (1 .. 32 of them): the number of fields is their number
//   --centering C         0 / 1
//   --clear C             0 / 1 (fold)
//   --nullpad             pass padding = NULL (only valid when the padding is zero)
//   --self-check-shift-dim               call along (dim + 1) % 3 while expecting dim: the case must FAIL
#include "native_test.h"

#include "cudecomp_halo_wall_fields.h"

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

// the prototypes as the header gives them; a mismatch with the definitions is a compile error here or a wrong result below
typedef cudecompResult_t (*reflect_fn)(cudecompHandle_t, cudecompGridDesc_t, void* const[], int32_t, cudecompDataType_t, const int32_t[],
                                       int32_t, const int32_t[], const bool[], int32_t, const int32_t[], hipStream_t);
typedef cudecompResult_t (*fold_fn)(cudecompHandle_t, cudecompGridDesc_t, void* const[], int32_t, cudecompDataType_t, const int32_t[],
                                    int32_t, int32_t, const int32_t[], const bool[], int32_t, const int32_t[], hipStream_t);
reflect_fn const kReflect[3] = {cudecompAmdReflectFieldHalosX, cudecompAmdReflectFieldHalosY, cudecompAmdReflectFieldHalosZ};
fold_fn const kFold[3] = {cudecompAmdFoldFieldHalosX, cudecompAmdFoldFieldHalosY, cudecompAmdFoldFieldHalosZ};

int runCase(cudecompHandle_t handle, const Options& o, bool silent) {
  const int rank = worldRank();
  const std::array<int, 3> g = {o.geti("gx", 256), o.geti("gy", 256), o.geti("gz", 256)};
  const std::array<int, 3> gd = o.get3("gd", {0, 0, 0});
  const std::array<int, 3> halo = {o.geti("hex", 1), o.geti("hey", 1), o.geti("hez", 1)};
  const bool pb[3] = {o.geti("hpx", 1) != 0, o.geti("hpy", 1) != 0, o.geti("hpz", 1) != 0};
  const std::array<int, 3> pad = {o.geti("pdx", 0), o.geti("pdy", 0), o.geti("pdz", 0)};
  const int axis = o.geti("ax", 0), backend = o.geti("backend", 0), centering = o.geti("centering", 0), clear = o.geti("clear", 0);
  if (axis < 0 || axis > 2) throw TestFailure("--ax out of range");
  auto op_it = o.values.find("op");
  if (op_it == o.values.end() || op_it->second.size() != 1 || (op_it->second[0] != "reflect" && op_it->second[0] != "fold"))
    throw TestFailure("--op must be reflect or fold");
  const bool fold = op_it->second[0] == "fold";
  auto par_it = o.values.find("parities");
  if (par_it == o.values.end() || par_it->second.empty() || par_it->second.size() > CUDECOMP_AMD_MAX_HALO_WALL_FIELDS)
    throw TestFailure("--parities needs 1 .. 32 values");
  const int nf = (int)par_it->second.size();
  std::vector<int32_t> parities(nf);
  for (int f = 0; f < nf; ++f) {
    parities[f] = std::atoi(par_it->second[f].c_str());
    if (parities[f] != 1 && parities[f] != -1) throw TestFailure("--parities holds +1 and -1 only");
  }
  if (centering != 0 && centering != 1) throw TestFailure("--centering out of range");
  if (clear != 0 && clear != 1) throw TestFailure("--clear out of range");
  const bool nullpad = o.has("nullpad"), shift = o.has("self-check-shift-dim");
  if (nullpad && (pad[0] || pad[1] || pad[2])) throw TestFailure("--nullpad needs zero padding");

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
    printf("running the %s of %d fields (centering %d, clear %d) on %d x %d x %d spatial grid, %d x %d process grid...\n",
           fold ? "fold" : "reflection", nf, centering, clear, g[0], g[1], g[2], config.pdims[0], config.pdims[1]);

  int failures = 0;
  std::vector<void*> dev(nf, nullptr);
  auto release = [&]() {
    for (void* q : dev)
      if (q) (void)hipFree(q);
  };
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
    std::vector<std::vector<int>> model(nf, std::vector<int>((size_t)reals, kPoison));
    for (int f = 0; f < nf; ++f)
      for (int64_t i2 = 0; i2 < ext[2]; ++i2)
        for (int64_t i1 = 0; i1 < ext[1]; ++i1)
          for (int64_t i0 = 0; i0 < ext[0]; ++i0) {
            const int64_t e = i0 + i1 * stride[1] + i2 * stride[2];
            model[f][e * kComp] = payload(e, f);
            if (kComp == 2) model[f][e * kComp + 1] = payload(e, f + 50);
          }
    std::vector<real_t> host((size_t)reals), want((size_t)reals);
    for (int f = 0; f < nf; ++f) {
      for (int64_t e = 0; e < reals; ++e) want[e] = encodeReal(model[f][e]);
      T_CHECK_HIP(hipMalloc(&dev[f], total_bytes));
      uploadPencil(dev[f], want.data(), total_bytes);
    }
    for (int step = 0; step < 3; ++step) {
      const int dim = fold ? 2 - step : step;
      int32_t lo = -1, hi = -1;
      T_CHECK_CD(cudecompGetShiftedRank(handle, gdesc, axis, dim, -1, pb[dim], &lo));
      T_CHECK_CD(cudecompGetShiftedRank(handle, gdesc, axis, dim, +1, pb[dim], &hi));
      const bool wall[2] = {lo == -1, hi == -1};
      const bool active = halo[dim] > 0 && (wall[0] || wall[1]);
      const int call_dim = shift ? (dim + 1) % 3 : dim;
      const cudecompResult_t r = fold ? kFold[axis](handle, gdesc, dev.data(), nf, kDtype, parities.data(), centering, clear, halo32, pb, call_dim, pad_arg, 0)
                                      : kReflect[axis](handle, gdesc, dev.data(), nf, kDtype, parities.data(), centering, halo32, pb, call_dim, pad_arg, 0);
      if (r != CUDECOMP_RESULT_SUCCESS) {
        fprintf(stderr, "rank %d: the call along dim %d returned %d\n", rank, call_dim, (int)r);
        ++failures;
        break;
      }
      T_CHECK_HIP(hipDeviceSynchronize());
      // the header's formulas on the model
      int km = 0;  // the memory position of `dim`
      for (int k = 0; k < 3; ++k)
        if (p.order[k] == dim) km = k;
      const int ka = (km + 1) % 3, kb = (km + 2) % 3;
      const int64_t h = halo[dim], n = ext[km], c = centering;
      for (int f = 0; f < nf; ++f) {
        const std::vector<int> before = model[f];
        std::vector<int>& m = model[f];
        for (int side = 0; side < 2 && h > 0; ++side) {
          if (!wall[side]) continue;
          for (int64_t k = 0; k < h; ++k) {
            const int64_t ghost = side == 0 ? h - 1 - k : n - h + k, inner = side == 0 ? h + k + c : n - h - 1 - k - c;
            for (int64_t ia = 0; ia < ext[ka]; ++ia)
              for (int64_t ib = 0; ib < ext[kb]; ++ib)
                for (int q = 0; q < kComp; ++q) {
                  const int64_t at = ia * stride[ka] + ib * stride[kb];
                  int& gcell = m[(at + ghost * stride[km]) * kComp + q];
                  int& icell = m[(at + inner * stride[km]) * kComp + q];
                  if (fold) {
                    icell += parities[f] * gcell;
                    if (clear) gcell = 0;
                  } else {
                    gcell = parities[f] * icell;
                  }
                }
          }
        }
        T_CHECK_HIP(hipMemcpy(host.data(), dev[f], total_bytes, hipMemcpyDeviceToHost));
        for (int64_t e = 0; e < reals; ++e) want[e] = encodeReal(m[e]);
        int64_t bad = 0;
        for (int64_t e = 0; e < reals; ++e) {
          if (!std::memcmp(&host[e], &want[e], sizeof(real_t))) continue;
          if (++bad > 2) continue;
          const int64_t cell = e / kComp;
          fprintf(stderr, "rank %d: field %d (parity %d) dim %d: element %lld (%lld, %lld, %lld of %d x %d x %d, order %d %d %d) is not what the header says\n",
                  rank, f, (int)parities[f], dim, (long long)cell, (long long)(cell % p.shape[0]), (long long)((cell / p.shape[0]) % p.shape[1]),
                  (long long)(cell / ((int64_t)p.shape[0] * p.shape[1])), p.shape[0], p.shape[1], p.shape[2], p.order[0], p.order[1], p.order[2]);
        }
        if (bad) {
          fprintf(stderr, "rank %d: %lld reals of field %d differ after the %s along dim %d\n", rank, (long long)bad, f, fold ? "fold" : "reflection", dim);
          ++failures;
        }
        if (active && m == before) {
          fprintf(stderr, "rank %d: the formulas along dim %d changed nothing of field %d: the case shows nothing\n", rank, dim, f);
          ++failures;
        }
      }
      if (shift) {  // the pencils now hold what the OTHER dim made of them: nothing more to learn
        if (!failures) fprintf(stderr, "rank %d: the shifted dim went unnoticed\n", rank);
        break;
      }
    }
  } catch (...) {
    release();
    (void)cudecompGridDescDestroy(handle, gdesc);
    throw;
  }
  release();
  notePaths(handle, gdesc);
  T_CHECK_CD(cudecompGridDescDestroy(handle, gdesc));
  return failures ? 1 : 0;
}

}  // namespace

int main(int argc, char** argv) { return nativeMain(argc, argv, runCase); }
