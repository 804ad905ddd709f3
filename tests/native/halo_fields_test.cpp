// halo_fields_test.cpp -- multi-field halo updates (cudecomp_halo_fields.h: cudecompAmdUpdateFieldHalos{X,Y,Z}) as a C / C++ solver
// calls them: through the header's prototypes, nothing else.  Per case: --fields N pencils are uploaded, the fields call runs along
// dims 0, 1, 2 in turn through the X, Y or Z entry point of --ax (one workspace of N x cudecompGetHaloWorkspaceSize elements from
// cudecompMalloc), every field is downloaded after every dim and the WHOLE buffer -- halos of all dims, padding and a poisoned tail
// behind the pencil -- is compared byte for byte with a closed form built on the host from the text of the header,
// cudecompGetPencilInfo and cudecompGetShiftedRank.  Command line, test-file mode and output protocol of halo_test.cpp
// (native_test.h).
//
// Closed form.  A non-padding cell of field f starts as V_f(c) + 8 * [the cell lies in a halo of ANY dim], c its global coordinate
// wrapped in all three dims, V_f(c) = (c0 + 3 c1 + 5 c2) mod 7 + 20 f (the imaginary part of a complex element the same with
// (2 c0 + c1 + 3 c2) mod 7).  The update along `dim` copies the neighbour's face cells: a halo cell along `dim` on a side with a
// neighbour (cudecompGetShiftedRank) takes the CURRENT value of the cell of the same wrapped coordinate `dim` that is interior
// along `dim` -- on every rank, for the same position of the other two dims, that cell has one state, which the host tracks per
// dim: bumped or not.  So a state table "is the +8 still there" per cell, updated dim after dim, is the whole model.  Padding
// cells and the tail hold -77.  All payloads are small integers, exact in every type used (fp16 up to 2048).
//
//   the options of halo_test, plus
//   --fields N            the number of pencils (1 .. 32)
//   --nullpad             pass padding = NULL (only valid when the padding is zero)
//   --self-check-shift-dim               call along (dim + 1) % 3 while expecting dim: the case must FAIL (the comparison can fail)
#include "native_test.h"

#include "cudecomp_halo_fields.h"

namespace {

const int kBump = 8, kPoison = -77, kTailElements = 64;

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

// the prototype as the header gives it; a mismatch with the definitions is a compile error here or a wrong result below
typedef cudecompResult_t (*fields_fn)(cudecompHandle_t, cudecompGridDesc_t, void* const[], int32_t, void*, cudecompDataType_t,
                                      const int32_t[], const bool[], int32_t, const int32_t[], hipStream_t);
fields_fn const kFields[3] = {cudecompAmdUpdateFieldHalosX, cudecompAmdUpdateFieldHalosY, cudecompAmdUpdateFieldHalosZ};

struct Cell {
  bool inside = false;   // a cell of the pencil (not padding)
  bool bumped = false;   // still holds the +8 it started with
  int base[2] = {0, 0};  // V_0 of its wrapped global coordinate, per component
};

int runCase(cudecompHandle_t handle, const Options& o, bool silent) {
  const int rank = worldRank();
  const std::array<int, 3> g = {o.geti("gx", 256), o.geti("gy", 256), o.geti("gz", 256)};
  const std::array<int, 3> gd = o.get3("gd", {0, 0, 0});
  const std::array<int, 3> halo = {o.geti("hex", 1), o.geti("hey", 1), o.geti("hez", 1)};
  const bool pb[3] = {o.geti("hpx", 1) != 0, o.geti("hpy", 1) != 0, o.geti("hpz", 1) != 0};
  const std::array<int, 3> pad = {o.geti("pdx", 0), o.geti("pdy", 0), o.geti("pdz", 0)};
  const int axis = o.geti("ax", 0), backend = o.geti("backend", 0), nf = o.geti("fields", 3);
  if (axis < 0 || axis > 2) throw TestFailure("--ax out of range");
  if (nf < 1 || nf > CUDECOMP_AMD_MAX_HALO_FIELDS) throw TestFailure("--fields out of range");
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
    printf("running the update of %d fields on %d x %d x %d spatial grid, %d x %d process grid, %s halo backend...\n", nf, g[0], g[1],
           g[2], config.pdims[0], config.pdims[1], cudecompHaloCommBackendToString(config.halo_comm_backend));

  int failures = 0;
  std::vector<void*> dev(nf, nullptr);
  void* work = nullptr;
  auto release = [&]() {
    for (void* q : dev)
      if (q) (void)hipFree(q);
    if (work) (void)cudecompFree(handle, gdesc, work);
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
    const int32_t* pad_arg = nullptr;
    if (!nullpad) pad_arg = pad32;

    // the model: one table of cells (the same for every field), the state "bumped" per cell
    std::vector<Cell> cells((size_t)p.size);
    const int64_t stride[3] = {1, p.shape[0], (int64_t)p.shape[0] * p.shape[1]};
    int kOf[3] = {0, 0, 0};
    for (int k = 0; k < 3; ++k) kOf[p.order[k]] = k;
    int64_t idx = 0;
    for (int i2 = 0; i2 < p.shape[2]; ++i2)
      for (int i1 = 0; i1 < p.shape[1]; ++i1)
        for (int i0 = 0; i0 < p.shape[0]; ++i0, ++idx) {
          const int l[3] = {i0, i1, i2};
          int64_t gc[3];
          bool padding = false, ghost = false;
          for (int k = 0; k < 3; ++k) {
            const int ax = p.order[k], hk = halo[ax], n = (p.hi[k] - p.lo[k] + 1) + 2 * hk;
            if (l[k] >= n) padding = true;
            if (l[k] < hk || l[k] >= n - hk) ghost = true;
            const int64_t x = p.lo[k] + (l[k] - hk);
            gc[ax] = ((x % g[ax]) + g[ax]) % g[ax];
          }
          if (padding) continue;
          Cell& c = cells[idx];
          c.inside = true;
          c.bumped = ghost;
          c.base[0] = (int)((gc[0] + 3 * gc[1] + 5 * gc[2]) % 7);
          c.base[1] = (int)((2 * gc[0] + gc[1] + 3 * gc[2]) % 7);
        }
    auto encodeField = [&](std::vector<real_t>& out, int f) {
      out.assign((size_t)reals, encodeReal(kPoison));
      for (int64_t e = 0; e < p.size; ++e)
        if (cells[e].inside)
          for (int q = 0; q < kComp; ++q) out[e * kComp + q] = encodeReal(cells[e].base[q] + 20 * f + (cells[e].bumped ? kBump : 0));
    };

    std::vector<real_t> host((size_t)reals), want;
    for (int f = 0; f < nf; ++f) {
      T_CHECK_HIP(hipMalloc(&dev[f], total_bytes));
      encodeField(want, f);
      uploadPencil(dev[f], want.data(), total_bytes);
    }
    for (int dim = 0; dim < 3; ++dim) {
      // what a halo cell along `dim` receives is the state of the cell it copies: the neighbour's cell with the same position in the
      // other two dims, interior along `dim`.  Whether THAT cell is bumped depends only on its position in the other two dims (and
      // on the dims updated so far), which the receiver shares: it is the state of the receiver's own cell at the same other-dims
      // position and any interior index along `dim`.
      int32_t lo = -1, hi = -1;
      T_CHECK_CD(cudecompGetShiftedRank(handle, gdesc, axis, dim, -1, pb[dim], &lo));
      T_CHECK_CD(cudecompGetShiftedRank(handle, gdesc, axis, dim, +1, pb[dim], &hi));
      const int kd = kOf[dim], h = halo[dim], n = (p.hi[kd] - p.lo[kd] + 1) + 2 * h;
      if (h > 0) {
        idx = 0;
        for (int i2 = 0; i2 < p.shape[2]; ++i2)
          for (int i1 = 0; i1 < p.shape[1]; ++i1)
            for (int i0 = 0; i0 < p.shape[0]; ++i0, ++idx) {
              if (!cells[idx].inside) continue;
              const int l[3] = {i0, i1, i2};
              const int j = l[kd];
              const bool low = j < h, high = j >= n - h && j < n;
              if ((low && lo != -1) || (high && hi != -1))
                cells[idx].bumped = cells[idx + (int64_t)(h - j) * stride[kd]].bumped;  // (index h: the first interior cell along dim)
            }
      }
      const int call_dim = shift ? (dim + 1) % 3 : dim;
      const cudecompResult_t r = kFields[axis](handle, gdesc, dev.data(), nf, work, kDtype, halo32, pb, call_dim, pad_arg, 0);
      if (r != CUDECOMP_RESULT_SUCCESS) {
        fprintf(stderr, "rank %d: the fields update along dim %d returned %d\n", rank, call_dim, (int)r);
        ++failures;
        break;
      }
      T_CHECK_HIP(hipDeviceSynchronize());
      for (int f = 0; f < nf; ++f) {
        encodeField(want, f);
        T_CHECK_HIP(hipMemcpy(host.data(), dev[f], total_bytes, hipMemcpyDeviceToHost));
        int64_t bad = 0;
        for (int64_t e = 0; e < reals; ++e) {
          if (!std::memcmp(&host[e], &want[e], sizeof(real_t))) continue;
          if (++bad > 2) continue;
          const int64_t c = e / kComp;
          fprintf(stderr, "rank %d: field %d dim %d: element %lld (%lld, %lld, %lld of %d x %d x %d, order %d %d %d) differs from the closed form\n",
                  rank, f, dim, (long long)c, (long long)(c % p.shape[0]), (long long)((c / p.shape[0]) % p.shape[1]),
                  (long long)(c / ((int64_t)p.shape[0] * p.shape[1])), p.shape[0], p.shape[1], p.shape[2], p.order[0], p.order[1], p.order[2]);
        }
        if (bad) {
          fprintf(stderr, "rank %d: %lld reals of field %d differ after the update along dim %d\n", rank, (long long)bad, f, dim);
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
