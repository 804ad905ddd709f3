// transpose_fields_test.cpp -- multi-field transposes (cudecomp_transpose_fields.h: cudecompAmdTransposeFields{XToY,YToZ,ZToY,YToX})
// as a C / C++ solver calls them: through the header's prototypes, nothing else.  Per case: --fields N pencils are uploaded twice;
// one copy runs the cycle X -> Y -> Z -> Y -> X through the fields calls (one workspace of N x cudecompGetTransposeWorkspaceSize
// elements from cudecompMalloc), the other through N single cudecompTranspose* calls per hop; after every hop every buffer of
// both copies -- inputs and outputs, halo and padding cells and a poisoned tail included -- is downloaded and compared byte for
// byte.  The oracle is the single call.  Command line, test-file mode and output protocol of transpose_test.cpp (native_test.h).
//
//   --gx --gy --gz, --pr --pc, --backend, --ac, --mem_order   as for transpose_test
//   --hex --hey --hez / --pdx --pdy --pdz   halo extents / padding of every pencil (by global axis)
//   --fields N            the number of pencils (1 .. 32)
//   --inplace             inputs[f] == outputs[f] for every field
//   --nullhalo            pass NULL for halos and padding (only valid when they are zero)
//   --self-check-swap-fields    hand the fields call its outputs in reversed order while comparing in order: the case must FAIL
#include "native_test.h"

#include "cudecomp_transpose_fields.h"

namespace {

const int kTailElements = 64;

// the prototype as the header gives it; a mismatch with the definitions is a compile error here or a wrong result below
typedef cudecompResult_t (*fields_fn)(cudecompHandle_t, cudecompGridDesc_t, void* const[], void* const[], int32_t, void*,
                                      cudecompDataType_t, const int32_t[], const int32_t[], const int32_t[], const int32_t[],
                                      hipStream_t);
typedef cudecompResult_t (*single_fn)(cudecompHandle_t, cudecompGridDesc_t, void*, void*, void*, cudecompDataType_t, const int32_t[],
                                      const int32_t[], const int32_t[], const int32_t[], hipStream_t);
fields_fn const kFields[4] = {cudecompAmdTransposeFieldsXToY, cudecompAmdTransposeFieldsYToZ, cudecompAmdTransposeFieldsZToY,
                              cudecompAmdTransposeFieldsYToX};
single_fn const kSingle[4] = {cudecompTransposeXToY, cudecompTransposeYToZ, cudecompTransposeZToY, cudecompTransposeYToX};
const char* const kOpName[4] = {"XToY", "YToZ", "ZToY", "YToX"};
const int kOpIn[4] = {0, 1, 2, 1}, kOpOut[4] = {1, 2, 1, 0};

int runCase(cudecompHandle_t handle, const Options& o, bool silent) {
  const int rank = worldRank();
  const std::array<int, 3> g = {o.geti("gx", 32), o.geti("gy", 32), o.geti("gz", 32)};
  const int32_t halo[3] = {o.geti("hex", 0), o.geti("hey", 0), o.geti("hez", 0)};
  const int32_t pad[3] = {o.geti("pdx", 0), o.geti("pdy", 0), o.geti("pdz", 0)};
  const int backend = o.geti("backend", 0), nf = o.geti("fields", 3);
  const bool inplace = o.has("inplace"), nullhalo = o.has("nullhalo"), swap = o.has("self-check-swap-fields");
  if (nf < 1 || nf > CUDECOMP_AMD_MAX_TRANSPOSE_FIELDS) throw TestFailure("--fields out of range");
  if (nullhalo && (halo[0] || halo[1] || halo[2] || pad[0] || pad[1] || pad[2])) throw TestFailure("--nullhalo needs zero halos and padding");

  cudecompGridDescConfig_t config;
  T_CHECK_CD(cudecompGridDescConfigSetDefaults(&config));
  config.pdims[0] = o.geti("pr", 0);
  config.pdims[1] = o.geti("pc", 0);
  for (int i = 0; i < 3; ++i) {
    config.gdims[i] = g[i];
    config.transpose_axis_contiguous[i] = o.geti("ac", 0) != 0;
  }
  if (backend == 0) throw TestFailure("--backend is required (no autotuning here)");
  config.transpose_comm_backend = (cudecompTransposeCommBackend_t)backend;

  cudecompGridDesc_t gdesc;
  T_CHECK_CD(cudecompGridDescCreate(handle, &gdesc, &config, nullptr));
  if (!silent && rank == 0)
    printf("running the cycle of %d fields on %d x %d x %d spatial grid, %d x %d process grid, %s transpose backend...\n", nf, g[0],
           g[1], g[2], config.pdims[0], config.pdims[1], cudecompTransposeCommBackendToString(config.transpose_comm_backend));

  int failures = 0;
  // [copy: 0 fields call, 1 single calls][side: 0 / 1 of the ping-pong][field]
  std::vector<void*> dev[2][2];
  void *work = nullptr, *work1 = nullptr;
  auto release = [&]() {
    for (auto& copy : dev)
      for (auto& side : copy)
        for (void* q : side)
          if (q) (void)hipFree(q);
    if (work) (void)cudecompFree(handle, gdesc, work);
    if (work1) (void)cudecompFree(handle, gdesc, work1);
  };
  try {
    cudecompPencilInfo_t p[3];
    int64_t nel = 0;
    for (int ax = 0; ax < 3; ++ax) {
      T_CHECK_CD(cudecompGetPencilInfo(handle, gdesc, &p[ax], ax, halo, pad));
      nel = std::max<int64_t>(nel, p[ax].size);
    }
    nel += kTailElements;
    const size_t bytes = (size_t)nel * sizeof(elem_t);
    int64_t wsz = 0;
    T_CHECK_CD(cudecompGetTransposeWorkspaceSize(handle, gdesc, &wsz));
    wsz = std::max<int64_t>(wsz, 1);
    T_CHECK_CD(cudecompMalloc(handle, gdesc, &work, (size_t)wsz * nf * sizeof(elem_t)));
    T_CHECK_CD(cudecompMalloc(handle, gdesc, &work1, (size_t)wsz * sizeof(elem_t)));

    // payload: small integers that name (rank, field, cell), exact in every type; another pattern in the second buffers
    std::vector<elem_t> host((size_t)nel), other((size_t)nel);
    for (int copy = 0; copy < 2; ++copy)
      for (int side = 0; side < (inplace ? 1 : 2); ++side) dev[copy][side].assign(nf, nullptr);
    for (int f = 0; f < nf; ++f) {
      for (int64_t e = 0; e < nel; ++e) {
        make(host[(size_t)e], (double)((e * 7 + f * 131 + rank * 17) % 1021));
        make(other[(size_t)e], (double)((e * 3 + f * 29 + 5) % 509 + 1024));
      }
      for (int copy = 0; copy < 2; ++copy) {
        T_CHECK_HIP(hipMalloc(&dev[copy][0][f], bytes));
        uploadPencil(dev[copy][0][f], host.data(), bytes);
        if (!inplace) {
          T_CHECK_HIP(hipMalloc(&dev[copy][1][f], bytes));
          uploadPencil(dev[copy][1][f], other.data(), bytes);
        }
      }
    }
    const int32_t* h_arg = nullhalo ? nullptr : halo;
    const int32_t* p_arg = nullhalo ? nullptr : pad;
    int cur = 0;
    for (int op = 0; op < 4 && !failures; ++op) {
      const int nxt = inplace ? cur : 1 - cur;
      std::vector<void*> ins(dev[0][cur]), outs(dev[0][nxt]);
      if (swap && !inplace) std::reverse(outs.begin(), outs.end());
      const cudecompResult_t r = kFields[op](handle, gdesc, ins.data(), outs.data(), nf, work, kDtype, h_arg, h_arg, p_arg, p_arg, 0);
      if (r != CUDECOMP_RESULT_SUCCESS) {
        fprintf(stderr, "rank %d: the fields transpose %s returned %d\n", rank, kOpName[op], (int)r);
        ++failures;
        break;
      }
      std::fill(ins.begin(), ins.end(), nullptr);  // the arrays were read before the call returned
      std::fill(outs.begin(), outs.end(), nullptr);
      for (int f = 0; f < nf; ++f)
        T_CHECK_CD(kSingle[op](handle, gdesc, dev[1][cur][f], dev[1][nxt][f], work1, kDtype, h_arg, h_arg, p_arg, p_arg, 0));
      T_CHECK_HIP(hipDeviceSynchronize());
      for (int side = 0; side < (inplace ? 1 : 2); ++side)
        for (int f = 0; f < nf; ++f) {
          T_CHECK_HIP(hipMemcpy(host.data(), dev[0][side][f], bytes, hipMemcpyDeviceToHost));
          T_CHECK_HIP(hipMemcpy(other.data(), dev[1][side][f], bytes, hipMemcpyDeviceToHost));
          int64_t bad = 0, first = -1;
          for (int64_t e = 0; e < nel; ++e)
            if (std::memcmp(&host[(size_t)e], &other[(size_t)e], sizeof(elem_t)) && bad++ == 0) first = e;
          if (bad) {
            fprintf(stderr, "rank %d: %lld elements of field %d (%s of %s, pencils along %d -> %d) differ from the single call, first %lld\n",
                    rank, (long long)bad, f, side == nxt ? "output" : "input", kOpName[op], kOpIn[op], kOpOut[op], (long long)first);
            ++failures;
          }
        }
      cur = nxt;
    }
    if (swap && !failures) fprintf(stderr, "rank %d: the swapped fields went unnoticed\n", rank);
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
