// halo_fold_test.cpp -- halo folding (cudecomp_halo_fold.h: cudecompAmdFoldHalos{X,Y,Z}) as a C / C++ solver calls it: through the
// header's prototypes and the macros of cudecomp_amd.h, nothing else.  Per case and per dim 0, 1, 2 SEPARATELY: upload a fresh
// pencil, call the fold once along `dim` through the X, Y or Z entry point of --ax, download, compare the WHOLE buffer -- halos of
// all dims, padding and a poisoned tail behind the pencil -- byte for byte with an expectation built on the host from the text of
// the header, cudecompGetPencilInfo and cudecompGetShiftedRank.  Command line, test-file mode and output protocol of halo_test.cpp
// (native_test.h).
//
// Initial content, as in halo_ops_test.cpp: a non-padding cell holds G(c) + 8 * [the cell lies in the low or high halo along dim],
// c its global coordinate wrapped in all three dims, G = (c0 + 3 c1 + 5 c2) mod 7; the imaginary part of a complex element the same
// with G' = (2 c0 + c1 + 3 c2) mod 7.  Padding cells and the tail hold -77.  All payloads are small integers: every sum (magnitude at
// most 6 + 2 * 14) is exact in every type, bfloat16 included, and no addend is zero, so parity -1 is the subtraction of integers.
//
//   the options of halo_test, plus
//   --parity +1|-1  --centering 0|1  --clear 0|1
//   --nullpad             pass padding = NULL (only valid when the padding is zero)
//   --dtype half|bf16|half_complex       (H16 build) the 2-byte type, chosen at run time through the macros of cudecomp_amd.h
//   --expect-refusal --dim D             ONE call along D (passed as given, so 3 can be asked for): it must return
//                                        CUDECOMP_RESULT_INVALID_USAGE and leave every byte as uploaded
//   --self-check-shift-dim               call along (dim + 1) % 3 while expecting dim: the case must FAIL (the comparison can fail)
#include "native_test.h"

#include "cudecomp_halo_fold.h"

namespace {

enum Comp { F32, F64, F16, BF16 };  // one real component

struct Format {
  cudecompDataType_t dtype;
  Comp comp;
  int ncomp;  // 1 real, 2 complex
  int compBytes() const { return comp == F64 ? 8 : (comp == F32 ? 4 : 2); }
  int bytes() const { return ncomp * compBytes(); }
};

Format formatOf(const Options& o) {
#if defined(H16)
  auto it = o.values.find("dtype");
  const std::string sel = (it == o.values.end() || it->second.empty()) ? "half" : it->second[0];
  if (sel == "half") return {CUDECOMP_AMD_HALF, F16, 1};
  if (sel == "bf16") return {CUDECOMP_AMD_BFLOAT16, BF16, 1};
  if (sel == "half_complex") return {CUDECOMP_AMD_HALF_COMPLEX, F16, 2};
  throw TestFailure("--dtype must be half, bf16 or half_complex");
#elif defined(R32)
  (void)o;
  return {CUDECOMP_FLOAT, F32, 1};
#elif defined(C32)
  (void)o;
  return {CUDECOMP_FLOAT_COMPLEX, F32, 2};
#elif defined(C64)
  (void)o;
  return {CUDECOMP_DOUBLE_COMPLEX, F64, 2};
#else
  (void)o;
  return {CUDECOMP_DOUBLE, F64, 1};
#endif
}

// the bytes of one real component holding the small integer v
void encode(unsigned char* dst, int v, Comp comp) {
  switch (comp) {
    case F64: {
      const double d = (double)v;
      std::memcpy(dst, &d, 8);
    } break;
    case F32: {
      const float f = (float)v;
      std::memcpy(dst, &f, 4);
    } break;
    case F16: {
      const uint16_t b = halfBitsOfInt(v);
      std::memcpy(dst, &b, 2);
    } break;
    case BF16: {  // the upper half of the binary32 pattern: exact for integers of magnitude up to 256
      const float f = (float)v;
      uint32_t w;
      std::memcpy(&w, &f, 4);
      const uint16_t b = (uint16_t)(w >> 16);
      std::memcpy(dst, &b, 2);
    } break;
  }
}

const int kBump = 8, kPoison = -77, kTailElements = 64;

// the prototype as the header gives it; a mismatch with the definitions is a compile error here or a wrong result below
typedef cudecompResult_t (*fold_fn)(cudecompHandle_t, cudecompGridDesc_t, void*, cudecompDataType_t, int32_t, int32_t, int32_t,
                                    const int32_t[], const bool[], int32_t, const int32_t[], hipStream_t);
fold_fn const kFold[3] = {cudecompAmdFoldHalosX, cudecompAmdFoldHalosY, cudecompAmdFoldHalosZ};

struct Case {
  Format f;
  int axis, parity, centering, clear;
  std::array<int, 3> g, halo, pad;
  std::array<bool, 3> periods;
};

// integers of every real component of the pencil: `init` what is uploaded for a call along `dim`, `want` what the
// header says the pencil holds after one fold along `dim`; low / high: does cudecompGetShiftedRank give a neighbour
struct Model {
  std::vector<int> init, want;
};

Model buildModel(const Case& c, const cudecompPencilInfo_t& p, int dim, bool low, bool high, bool refused) {
  const int nc = c.f.ncomp;
  Model m;
  m.init.assign((size_t)p.size * nc, kPoison);
  int kd = 0;
  for (int k = 0; k < 3; ++k)
    if (p.order[k] == dim) kd = k;
  const int64_t stride[3] = {1, p.shape[0], (int64_t)p.shape[0] * p.shape[1]};
  const int h = c.halo[dim], n = (p.hi[kd] - p.lo[kd] + 1) + 2 * h;  // the extent along dim without padding
  std::vector<int> G((size_t)p.size * nc, 0);
  std::vector<unsigned char> cell(p.size, 0);  // 1: a cell of the pencil (not padding)
  int64_t idx = 0;
  for (int i2 = 0; i2 < p.shape[2]; ++i2)
    for (int i1 = 0; i1 < p.shape[1]; ++i1)
      for (int i0 = 0; i0 < p.shape[0]; ++i0, ++idx) {
        const int l[3] = {i0, i1, i2};
        int64_t gc[3];
        bool padding = false;
        for (int k = 0; k < 3; ++k) {
          const int ax = p.order[k], hk = c.halo[ax];
          if (l[k] >= (p.hi[k] - p.lo[k] + 1) + 2 * hk) padding = true;
          const int64_t x = p.lo[k] + (l[k] - hk);
          gc[ax] = ((x % c.g[ax]) + c.g[ax]) % c.g[ax];
        }
        if (padding) continue;
        cell[idx] = 1;
        const bool ghost = l[kd] < h || l[kd] >= n - h;
        G[idx * nc] = (int)((gc[0] + 3 * gc[1] + 5 * gc[2]) % 7);
        if (nc == 2) G[idx * nc + 1] = (int)((2 * gc[0] + gc[1] + 3 * gc[2]) % 7);
        for (int q = 0; q < nc; ++q) m.init[idx * nc + q] = G[idx * nc + q] + (ghost ? kBump : 0);
      }
  m.want = m.init;
  if (refused || h == 0) return m;
  idx = 0;
  for (int i2 = 0; i2 < p.shape[2]; ++i2)
    for (int i1 = 0; i1 < p.shape[1]; ++i1)
      for (int i0 = 0; i0 < p.shape[0]; ++i0, ++idx) {
        if (!cell[idx]) continue;
        const int l[3] = {i0, i1, i2};
        const int j = l[kd];
        const int s = c.parity == -1 ? -1 : 1, ce = c.centering;
        // low side: cell(h + k + c) += s * cell(h - 1 - k); high side: cell(n - h - 1 - k - c) += s * cell(n - h + k); both may hit a cell
        if (!low && j >= h + ce && j < 2 * h + ce) {
          const int src = h - 1 - (j - h - ce);
          for (int q = 0; q < nc; ++q) m.want[idx * nc + q] += s * m.init[(idx + (int64_t)(src - j) * stride[kd]) * nc + q];
        }
        if (!high && j >= n - 2 * h - ce && j < n - h - ce) {
          const int src = n - h + (n - h - 1 - ce - j);
          for (int q = 0; q < nc; ++q) m.want[idx * nc + q] += s * m.init[(idx + (int64_t)(src - j) * stride[kd]) * nc + q];
        }
        if (c.clear && ((!low && j < h) || (!high && j >= n - h)))
          for (int q = 0; q < nc; ++q) m.want[idx * nc + q] = 0;
      }
  return m;
}

void encodeAll(std::vector<elem_t>& out, size_t total_bytes, const std::vector<int>& v, const Format& f) {
  out.assign(total_bytes / sizeof(elem_t), elem_t());
  unsigned char* b = reinterpret_cast<unsigned char*>(out.data());
  const int cb = f.compBytes();
  for (size_t i = 0; i < total_bytes / cb; ++i)  // (behind the pencil: the tail, poisoned)
    encode(b + i * cb, i < v.size() ? v[i] : kPoison, f.comp);
}

int runCase(cudecompHandle_t handle, const Options& o, bool silent) {
  const int rank = worldRank();
  Case c;
  c.g = {o.geti("gx", 256), o.geti("gy", 256), o.geti("gz", 256)};
  const std::array<int, 3> gd = o.get3("gd", {0, 0, 0});
  c.halo = {o.geti("hex", 1), o.geti("hey", 1), o.geti("hez", 1)};
  c.periods = {o.geti("hpx", 1) != 0, o.geti("hpy", 1) != 0, o.geti("hpz", 1) != 0};
  c.pad = {o.geti("pdx", 0), o.geti("pdy", 0), o.geti("pdz", 0)};
  c.axis = o.geti("ax", 0);
  const int backend = o.geti("backend", 0);
  if (c.axis < 0 || c.axis > 2) throw TestFailure("--ax out of range");
  c.f = formatOf(o);
  const std::string opname = "fold";
  c.parity = o.geti("parity", 1);
  c.centering = o.geti("centering", 0);
  c.clear = o.geti("clear", 0);
  const bool nullpad = o.has("nullpad"), refusal = o.has("expect-refusal"), shift = o.has("self-check-shift-dim");
  if (nullpad && (c.pad[0] || c.pad[1] || c.pad[2])) throw TestFailure("--nullpad needs zero padding");

  cudecompGridDescConfig_t config;
  T_CHECK_CD(cudecompGridDescConfigSetDefaults(&config));
  config.pdims[0] = o.geti("pr", 0);
  config.pdims[1] = o.geti("pc", 0);
  config.rank_order = (cudecompRankOrder_t)o.geti("rank-order", 0);
  for (int i = 0; i < 3; ++i) {
    config.gdims[i] = c.g[i];
    config.gdims_dist[i] = c.g[i] - gd[i];
    config.transpose_axis_contiguous[i] = o.geti("ac", 0) != 0;
  }
  if (o.has("mem_order")) {
    for (int ax = 0; ax < 3; ++ax)
      for (int i = 0; i < 3; ++i) config.transpose_mem_order[ax][i] = (ax == c.axis) ? o.geti("mem_order", i, i) : i;
  }
  if (backend == 0) throw TestFailure("--backend is required (no autotuning here)");
  config.halo_comm_backend = (cudecompHaloCommBackend_t)backend;

  cudecompGridDesc_t gdesc;
  T_CHECK_CD(cudecompGridDescCreate(handle, &gdesc, &config, nullptr));
  if (!silent && rank == 0)
    printf("running %s on %d x %d x %d spatial grid, %d x %d process grid, %s halo backend...\n", opname.c_str(), c.g[0], c.g[1],
           c.g[2], config.pdims[0], config.pdims[1], cudecompHaloCommBackendToString(config.halo_comm_backend));

  int failures = 0;
  elem_t* data = nullptr;
  try {
    cudecompPencilInfo_t p;
    T_CHECK_CD(cudecompGetPencilInfo(handle, gdesc, &p, c.axis, c.halo.data(), c.pad.data()));
    const int es = c.f.bytes();
    const size_t total_bytes = (size_t)(p.size + kTailElements) * es;
    const int64_t nel = (int64_t)(total_bytes / sizeof(elem_t));
    data = TestBuffer::get(0, nel);

    int32_t halo32[3] = {c.halo[0], c.halo[1], c.halo[2]}, pad32[3] = {c.pad[0], c.pad[1], c.pad[2]};
    const bool pb[3] = {c.periods[0], c.periods[1], c.periods[2]};
    const int32_t* pad_arg = nullptr;
    if (!nullpad) pad_arg = pad32;

    std::vector<elem_t> init, want, host((size_t)nel);
    const int first = refusal ? o.geti("dim", 0) : 0, last = refusal ? first : 2;
    for (int dim = first; dim <= last; ++dim) {
      const int mdim = (dim < 0 || dim > 2) ? 0 : dim;  // (a refused dim: any initial content will do)
      int32_t lo = -1, hi = -1;
      T_CHECK_CD(cudecompGetShiftedRank(handle, gdesc, c.axis, mdim, -1, pb[mdim], &lo));
      T_CHECK_CD(cudecompGetShiftedRank(handle, gdesc, c.axis, mdim, +1, pb[mdim], &hi));
      const Model m = buildModel(c, p, mdim, lo != -1, hi != -1, refusal);
      encodeAll(init, total_bytes, m.init, c.f);
      encodeAll(want, total_bytes, m.want, c.f);
      uploadPencil(data, init.data(), total_bytes);
      const bool stale_input = InputGate::get().checkInput("halo_fold", data, init, nel, 0);
      if (stale_input) ++failures;

      const int call_dim = shift ? (dim + 1) % 3 : dim;
      const cudecompResult_t r = kFold[c.axis](handle, gdesc, data, c.f.dtype, c.parity, c.centering, c.clear, halo32, pb, call_dim,
                                               pad_arg, 0);
      const cudecompResult_t expected = refusal ? CUDECOMP_RESULT_INVALID_USAGE : CUDECOMP_RESULT_SUCCESS;
      if (r != expected) {
        fprintf(stderr, "rank %d: %s along dim %d returned %d, expected %d\n", rank, opname.c_str(), call_dim, (int)r, (int)expected);
        ++failures;
        if (r != CUDECOMP_RESULT_SUCCESS && !refusal) break;
      }
      T_CHECK_HIP(hipDeviceSynchronize());
      T_CHECK_HIP(hipMemcpy(host.data(), data, total_bytes, hipMemcpyDeviceToHost));
      InputGate::get().checkDownload("halo_fold", data, host, nel, 0);
      const unsigned char *got = reinterpret_cast<const unsigned char*>(host.data()),
                          *ref = reinterpret_cast<const unsigned char*>(want.data()),
                          *was = reinterpret_cast<const unsigned char*>(init.data());
      int64_t bad = 0;
      for (int64_t e = 0; e < p.size + kTailElements; ++e) {
        if (!std::memcmp(got + e * es, ref + e * es, es)) continue;
        if (++bad > 2) continue;
        auto hex = [&](const unsigned char* b) {
          std::string s;
          char t[4];
          for (int i = es - 1; i >= 0; --i) std::snprintf(t, sizeof t, "%02x", b[e * es + i]), s += t;
          return s;
        };
        fprintf(stderr, "rank %d: %s dim %d: element %lld (%lld, %lld, %lld of %d x %d x %d, order %d %d %d) holds %s, expected %s, uploaded %s\n",
                rank, opname.c_str(), dim, (long long)e, (long long)(e % p.shape[0]), (long long)((e / p.shape[0]) % p.shape[1]),
                (long long)(e / ((int64_t)p.shape[0] * p.shape[1])), p.shape[0], p.shape[1], p.shape[2], p.order[0], p.order[1],
                p.order[2], hex(got).c_str(), hex(ref).c_str(), hex(was).c_str());
      }
      if (bad) {
        fprintf(stderr, "rank %d: %lld elements differ after %s along dim %d%s\n", rank, (long long)bad, opname.c_str(), dim,
                stale_input ? " (the input gate had TRIPPED for this case: stale upload)" : " (input gate: the upload was intact before the call)");
        ++failures;
      }
    }
  } catch (...) {
    if (data && !TestBuffer::reuse()) (void)hipFree(data);
    (void)cudecompGridDescDestroy(handle, gdesc);
    throw;
  }
  TestBuffer::put(data);
  notePaths(handle, gdesc);
  T_CHECK_CD(cudecompGridDescDestroy(handle, gdesc));
  return failures ? 1 : 0;
}

}  // namespace

int main(int argc, char** argv) { return nativeMain(argc, argv, runCase); }
