// halo_accumulate_fields_test.cpp -- multi-field halo accumulation (cudecomp_halo_accumulate_fields.h:
// cudecompAmdAccumulateFieldHalos{X,Y,Z}) as a C / C++ solver calls it: through the headers' prototypes, nothing else.  Per case:
// --fields N pencils are uploaded twice; the fields call runs along dims 2, 1, 0 in turn on the first set through the X, Y or Z
// entry point of --ax (one workspace of N x cudecompGetHaloWorkspaceSize elements from cudecompMalloc, --clear 0 / 1), the single
// call the header names as its definition -- cudecompAmdAccumulateHalos{X,Y,Z} (cudecomp_amd.h) or
// cudecompAmdAccumulateAndClearHalos{X,Y,Z} (cudecomp_amd_fill.h) -- on every pencil of the second set; after every dim every field
// is downloaded and the WHOLE buffer -- halos of all dims, padding and a poisoned tail behind the pencil -- is compared byte for byte
// with its twin.  A dim along which the rank has a neighbour and a halo must have changed every field.  Command line, test-file
// mode and output protocol of halo_test.cpp (native_test.h).
//
// Payload: field f, cell e (its position in the buffer) holds ((7 e + 3 f) mod 11) - 5, the imaginary part of a complex element
// ((5 e + f) mod 9) - 4; padding cells and the tail hold -77.  Small integers, exact in every type used (fp16 up to 2048); a cell
// is the sum of at most 27 cells.
//
//   the options of halo_test, plus
//   --fields N            the number of pencils (1 .. 32)
//   --clear C             0 / 1
//   --nullpad             pass padding = NULL (only valid when the padding is zero)
//   --self-check-shift-dim               call along (dim + 1) % 3 while the single calls run along dim: the case must FAIL
#include "native_test.h"

#include "cudecomp_amd_fill.h"
#include "cudecomp_halo_accumulate_fields.h"

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

real_t encodeReal(int v) {
#if defined(H16)
  return halfBitsOfInt(v);
#else
  return (real_t)v;
#endif
}

// the prototypes as the headers give them; a mismatch with the definitions is a compile error here or a wrong result below
typedef cudecompResult_t (*fields_fn)(cudecompHandle_t, cudecompGridDesc_t, void* const[], int32_t, void*, cudecompDataType_t,
                                      const int32_t[], const bool[], int32_t, const int32_t[], int32_t, hipStream_t);
typedef cudecompResult_t (*single_fn)(cudecompHandle_t, cudecompGridDesc_t, void*, void*, cudecompDataType_t, const int32_t[],
                                      const bool[], int32_t, const int32_t[], hipStream_t);
fields_fn const kFields[3] = {cudecompAmdAccumulateFieldHalosX, cudecompAmdAccumulateFieldHalosY, cudecompAmdAccumulateFieldHalosZ};
single_fn const kSingle[2][3] = {
    {cudecompAmdAccumulateHalosX, cudecompAmdAccumulateHalosY, cudecompAmdAccumulateHalosZ},
    {cudecompAmdAccumulateAndClearHalosX, cudecompAmdAccumulateAndClearHalosY, cudecompAmdAccumulateAndClearHalosZ}};

int runCase(cudecompHandle_t handle, const Options& o, bool silent) {
  const int rank = worldRank();
  const std::array<int, 3> g = {o.geti("gx", 256), o.geti("gy", 256), o.geti("gz", 256)};
  const std::array<int, 3> gd = o.get3("gd", {0, 0, 0});
  const std::array<int, 3> halo = {o.geti("hex", 1), o.geti("hey", 1), o.geti("hez", 1)};
  const bool pb[3] = {o.geti("hpx", 1) != 0, o.geti("hpy", 1) != 0, o.geti("hpz", 1) != 0};
  const std::array<int, 3> pad = {o.geti("pdx", 0), o.geti("pdy", 0), o.geti("pdz", 0)};
  const int axis = o.geti("ax", 0), backend = o.geti("backend", 0), nf = o.geti("fields", 3), clear = o.geti("clear", 0);
  if (axis < 0 || axis > 2) throw TestFailure("--ax out of range");
  if (nf < 1 || nf > CUDECOMP_AMD_MAX_HALO_ACCUMULATE_FIELDS) throw TestFailure("--fields out of range");
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
    printf("running the accumulation of %d fields (clear %d) on %d x %d x %d spatial grid, %d x %d process grid, %s halo backend...\n",
           nf, clear, g[0], g[1], g[2], config.pdims[0], config.pdims[1], cudecompHaloCommBackendToString(config.halo_comm_backend));

  int failures = 0;
  std::vector<void*> dev(nf, nullptr), twin(nf, nullptr);
  void *work = nullptr, *single_work = nullptr;
  auto release = [&]() {
    for (void* q : dev)
      if (q) (void)hipFree(q);
    for (void* q : twin)
      if (q) (void)hipFree(q);
    if (work) (void)cudecompFree(handle, gdesc, work);
    if (single_work) (void)cudecompFree(handle, gdesc, single_work);
  };
  try {
    cudecompPencilInfo_t p;
    int32_t halo32[3] = {halo[0], halo[1], halo[2]}, pad32[3] = {pad[0], pad[1], pad[2]};
    T_CHECK_CD(cudecompGetPencilInfo(handle, gdesc, &p, axis, halo32, pad32));
    const int es = kComp * (int)sizeof(real_t);
    const int64_t reals = (int64_t)(p.size + kTailElements) * kComp;
    const size_t total_bytes = (size_t)reals * sizeof(real_t);
    int64_t wsz = 0;
    T_CHECK_CD(cudecompGetHaloWorkspaceSize(handle, gdesc, axis, halo32, &wsz));
    T_CHECK_CD(cudecompMalloc(handle, gdesc, &work, (size_t)std::max<int64_t>(wsz, 1) * nf * es));
    T_CHECK_CD(cudecompMalloc(handle, gdesc, &single_work, (size_t)std::max<int64_t>(wsz, 1) * es));
    const int32_t* pad_arg = nullptr;
    if (!nullpad) pad_arg = pad32;

    // which cells are the pencil's (not padding)
    std::vector<char> inside((size_t)p.size, 0);
    int64_t idx = 0;
    for (int i2 = 0; i2 < p.shape[2]; ++i2)
      for (int i1 = 0; i1 < p.shape[1]; ++i1)
        for (int i0 = 0; i0 < p.shape[0]; ++i0, ++idx) {
          const int l[3] = {i0, i1, i2};
          bool padding = false;
          for (int k = 0; k < 3; ++k)
            if (l[k] >= (p.hi[k] - p.lo[k] + 1) + 2 * halo[p.order[k]]) padding = true;
          inside[idx] = !padding;
        }
    std::vector<real_t> host((size_t)reals), want((size_t)reals);
    std::vector<std::vector<real_t>> before(nf);
    for (int f = 0; f < nf; ++f) {
      want.assign((size_t)reals, encodeReal(kPoison));
      for (int64_t e = 0; e < p.size; ++e)
        if (inside[e]) {
          want[e * kComp] = encodeReal((int)((7 * e + 3 * f) % 11) - 5);
          if (kComp == 2) want[e * kComp + 1] = encodeReal((int)((5 * e + f) % 9) - 4);
        }
      T_CHECK_HIP(hipMalloc(&dev[f], total_bytes));
      T_CHECK_HIP(hipMalloc(&twin[f], total_bytes));
      uploadPencil(dev[f], want.data(), total_bytes);
      uploadPencil(twin[f], want.data(), total_bytes);
      before[f] = want;
    }
    for (int dim = 2; dim >= 0; --dim) {
      int32_t lo = -1, hi = -1;
      T_CHECK_CD(cudecompGetShiftedRank(handle, gdesc, axis, dim, -1, pb[dim], &lo));
      T_CHECK_CD(cudecompGetShiftedRank(handle, gdesc, axis, dim, +1, pb[dim], &hi));
      const bool active = halo[dim] > 0 && (lo != -1 || hi != -1);
      const int call_dim = shift ? (dim + 1) % 3 : dim;
      cudecompResult_t r = kFields[axis](handle, gdesc, dev.data(), nf, work, kDtype, halo32, pb, call_dim, pad_arg, clear, 0);
      for (int f = 0; f < nf && r == CUDECOMP_RESULT_SUCCESS; ++f)
        r = kSingle[clear][axis](handle, gdesc, twin[f], single_work, kDtype, halo32, pb, dim, pad_arg, 0);
      if (r != CUDECOMP_RESULT_SUCCESS) {
        fprintf(stderr, "rank %d: the accumulation along dim %d returned %d\n", rank, call_dim, (int)r);
        ++failures;
        break;
      }
      T_CHECK_HIP(hipDeviceSynchronize());
      for (int f = 0; f < nf; ++f) {
        T_CHECK_HIP(hipMemcpy(host.data(), dev[f], total_bytes, hipMemcpyDeviceToHost));
        T_CHECK_HIP(hipMemcpy(want.data(), twin[f], total_bytes, hipMemcpyDeviceToHost));
        int64_t bad = 0;
        for (int64_t e = 0; e < reals; ++e) {
          if (!std::memcmp(&host[e], &want[e], sizeof(real_t))) continue;
          if (++bad > 2) continue;
          const int64_t c = e / kComp;
          fprintf(stderr, "rank %d: field %d dim %d: element %lld (%lld, %lld, %lld of %d x %d x %d, order %d %d %d) differs from the single call\n",
                  rank, f, dim, (long long)c, (long long)(c % p.shape[0]), (long long)((c / p.shape[0]) % p.shape[1]),
                  (long long)(c / ((int64_t)p.shape[0] * p.shape[1])), p.shape[0], p.shape[1], p.shape[2], p.order[0], p.order[1], p.order[2]);
        }
        if (bad) {
          fprintf(stderr, "rank %d: %lld reals of field %d differ after the accumulation along dim %d\n", rank, (long long)bad, f, dim);
          ++failures;
        }
        if (active && !std::memcmp(want.data(), before[f].data(), total_bytes)) {
          fprintf(stderr, "rank %d: the single accumulation along dim %d changed nothing of field %d: the case shows nothing\n", rank, dim, f);
          ++failures;
        }
        for (int64_t e = p.size * kComp; e < reals; ++e)
          if (std::memcmp(&host[e], &before[f][e], sizeof(real_t))) {
            fprintf(stderr, "rank %d: the tail behind field %d changed\n", rank, f);
            ++failures;
            break;
          }
        before[f] = want;
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
