// The library product of the prompt pass, called natively with a PINNED algorithm (host code only; no kernel of ours):
//   y[b][rows][N] (fp32) = a[b][rows][K'] (fp16) . w[b][N][K']^T (fp16), fp32 accumulation, row-major - hipBLASLt's TN form.
// torch.mm / torch.bmm run the library's first heuristic choice for a shape; here an int selects the algorithm by the
// library's solution index among the (up to 64) candidates its heuristic lists for the problem, -1 = the first choice.
//
// Which copy of the library: PyTorch bundles its own libhipblaslt.so and has loaded it long before this file runs; the
// system's headers and library are another version.  So nothing here links against hipBLASLt: the C entry points (and
// the one helper that returns a solution index from the algorithm struct) are resolved at run time from the copy that
// is ALREADY in the process (dl_iterate_phdr + RTLD_NOLOAD - a second copy is never loaded).  Only C types cross the
// boundary: opaque descriptor pointers created by the library itself, and the 16-byte + size_t algorithm struct.
// Without a loaded copy psg_lt_gemm_init returns PSG_ERR_UNSUPPORTED and the caller stays on torch.mm.
#include <dlfcn.h>
#include <link.h>

#include <hipblaslt/hipblaslt.h>

#include <map>
#include <mutex>
#include <tuple>

#include "psg_common.h"

namespace {

struct LtApi {
  decltype(&hipblasLtCreate) create = nullptr;
  decltype(&hipblasLtDestroy) destroy = nullptr;
  decltype(&hipblasLtGetVersion) version = nullptr;
  decltype(&hipblasLtMatmulDescCreate) desc_create = nullptr;
  decltype(&hipblasLtMatmulDescDestroy) desc_destroy = nullptr;
  decltype(&hipblasLtMatmulDescSetAttribute) desc_set = nullptr;
  decltype(&hipblasLtMatrixLayoutCreate) layout_create = nullptr;
  decltype(&hipblasLtMatrixLayoutDestroy) layout_destroy = nullptr;
  decltype(&hipblasLtMatrixLayoutSetAttribute) layout_set = nullptr;
  decltype(&hipblasLtMatmulPreferenceCreate) pref_create = nullptr;
  decltype(&hipblasLtMatmulPreferenceDestroy) pref_destroy = nullptr;
  decltype(&hipblasLtMatmulPreferenceSetAttribute) pref_set = nullptr;
  decltype(&hipblasLtMatmulAlgoGetHeuristic) heuristic = nullptr;
  decltype(&hipblasLtMatmul) matmul = nullptr;
  int (*index_of)(hipblasLtMatmulAlgo_t&) = nullptr;      // hipblaslt_ext::getIndexFromAlgo
};

constexpr int kMaxCand = 64;

// (rows, N, K, lda, ldw, ldy, batch, stride_a, stride_w, stride_y, algo, workspace bytes)
using ProblemKey = std::tuple<int, int, int, int64_t, int64_t, int64_t, int, int64_t, int64_t, int64_t, int, int64_t>;

struct Problem {                                           // descriptors of one problem (host memory of the library's)
  hipblasLtMatmulDesc_t desc = nullptr;
  hipblasLtMatrixLayout_t lw = nullptr, la = nullptr, ly = nullptr;
};

struct Plan {                                              // a problem with its algorithm resolved: what a launch needs
  Problem p;
  hipblasLtMatmulAlgo_t algo;
  int64_t ws_need = 0;
  int index = -1;
  int fell_back = 0;
};

struct PsgLt {
  LtApi api;
  hipblasLtHandle_t handle = nullptr;
  int version = 0;
  std::mutex mu;
  std::map<ProblemKey, Plan> plans;
};

int find_loaded(struct dl_phdr_info* info, size_t, void* out) {
  const char* name = info->dlpi_name;
  if (name && strstr(name, "libhipblaslt.so")) {
    snprintf((char*)out, 1024, "%s", name);
    return 1;
  }
  return 0;
}

bool resolve(LtApi& api) {
  char path[1024] = "";
  if (!dl_iterate_phdr(find_loaded, path)) {
    psg_set_error("psg_lt_gemm_init: no libhipblaslt.so is loaded in this process (PyTorch loads its own)");
    return false;
  }
  void* so = dlopen(path, RTLD_NOLOAD | RTLD_NOW);         // NOLOAD: a handle to the loaded copy, or NULL - never a load
  if (!so) {
    psg_set_error("psg_lt_gemm_init: %s is mapped but dlopen(RTLD_NOLOAD) failed: %s", path, dlerror());
    return false;
  }
  bool ok = true;
  auto sym = [&](auto& fn, const char* name) {
    fn = reinterpret_cast<std::remove_reference_t<decltype(fn)>>(dlsym(so, name));
    if (!fn && ok) {
      psg_set_error("psg_lt_gemm_init: %s does not export %s", path, name);
      ok = false;
    }
  };
  sym(api.create, "hipblasLtCreate");
  sym(api.destroy, "hipblasLtDestroy");
  sym(api.version, "hipblasLtGetVersion");
  sym(api.desc_create, "hipblasLtMatmulDescCreate");
  sym(api.desc_destroy, "hipblasLtMatmulDescDestroy");
  sym(api.desc_set, "hipblasLtMatmulDescSetAttribute");
  sym(api.layout_create, "hipblasLtMatrixLayoutCreate");
  sym(api.layout_destroy, "hipblasLtMatrixLayoutDestroy");
  sym(api.layout_set, "hipblasLtMatrixLayoutSetAttribute");
  sym(api.pref_create, "hipblasLtMatmulPreferenceCreate");
  sym(api.pref_destroy, "hipblasLtMatmulPreferenceDestroy");
  sym(api.pref_set, "hipblasLtMatmulPreferenceSetAttribute");
  sym(api.heuristic, "hipblasLtMatmulAlgoGetHeuristic");
  sym(api.matmul, "hipblasLtMatmul");
  sym(api.index_of, "_ZN13hipblaslt_ext16getIndexFromAlgoER22_hipblasLtMatmulAlgo_t");
  return ok;
}

void free_problem(const LtApi& api, Problem& p) {
  if (p.lw) api.layout_destroy(p.lw);
  if (p.la) api.layout_destroy(p.la);
  if (p.ly) api.layout_destroy(p.ly);
  if (p.desc) api.desc_destroy(p.desc);
  p = Problem();
}

#define LT_TRY(call, what)                                                       \
  do {                                                                           \
    hipblasStatus_t s__ = (call);                                                \
    if (s__ != HIPBLAS_STATUS_SUCCESS) {                                         \
      psg_set_error("%s: %s failed (hipblasStatus %d)", who, what, (int)s__);     \
      free_problem(api, p);                                                      \
      return PSG_ERR_HIP;                                                        \
    }                                                                            \
  } while (0)

// Row-major y[rows][N] = a[rows][K] w[N][K]^T is the column-major product y^T [N x rows] = op_T(w: K x N, ld ldw) .
// (a: K x rows, ld lda): the library's A is w, its B is a.
int make_problem(const LtApi& api, const char* who, int rows, int N, int K, int64_t lda, int64_t ldw, int64_t ldy, int batch,
                 int64_t stride_a, int64_t stride_w, int64_t stride_y, Problem& p) {
  LT_TRY(api.desc_create(&p.desc, HIPBLAS_COMPUTE_32F, HIP_R_32F), "MatmulDescCreate");
  const int32_t ta = HIPBLAS_OP_T, tb = HIPBLAS_OP_N;
  LT_TRY(api.desc_set(p.desc, HIPBLASLT_MATMUL_DESC_TRANSA, &ta, sizeof(ta)), "DescSetAttribute(TRANSA)");
  LT_TRY(api.desc_set(p.desc, HIPBLASLT_MATMUL_DESC_TRANSB, &tb, sizeof(tb)), "DescSetAttribute(TRANSB)");
  LT_TRY(api.layout_create(&p.lw, HIP_R_16F, K, N, ldw), "MatrixLayoutCreate(w)");
  LT_TRY(api.layout_create(&p.la, HIP_R_16F, K, rows, lda), "MatrixLayoutCreate(a)");
  LT_TRY(api.layout_create(&p.ly, HIP_R_32F, N, rows, ldy), "MatrixLayoutCreate(y)");
  if (batch > 1) {
    const int32_t b = batch;
    const struct { hipblasLtMatrixLayout_t l; int64_t stride; } ls[3] = {{p.lw, stride_w}, {p.la, stride_a}, {p.ly, stride_y}};
    for (const auto& e : ls) {
      LT_TRY(api.layout_set(e.l, HIPBLASLT_MATRIX_LAYOUT_BATCH_COUNT, &b, sizeof(b)), "LayoutSetAttribute(BATCH_COUNT)");
      LT_TRY(api.layout_set(e.l, HIPBLASLT_MATRIX_LAYOUT_STRIDED_BATCH_OFFSET, &e.stride, sizeof(e.stride)),
             "LayoutSetAttribute(STRIDED_BATCH_OFFSET)");
    }
  }
  return PSG_OK;
}

// The heuristic's candidates for the problem within `max_ws` bytes of workspace, in the library's order
int list_candidates(PsgLt* lt, const char* who, Problem& p, int64_t max_ws, hipblasLtMatmulHeuristicResult_t* res, int* got) {
  const LtApi& api = lt->api;
  hipblasLtMatmulPreference_t pref = nullptr;
  LT_TRY(api.pref_create(&pref), "MatmulPreferenceCreate");
  const uint64_t ws = (uint64_t)(max_ws > 0 ? max_ws : 0);
  hipblasStatus_t s = api.pref_set(pref, HIPBLASLT_MATMUL_PREF_MAX_WORKSPACE_BYTES, &ws, sizeof(ws));
  if (s == HIPBLAS_STATUS_SUCCESS) s = api.heuristic(lt->handle, p.desc, p.lw, p.la, p.ly, p.ly, pref, kMaxCand, res, got);
  api.pref_destroy(pref);
  if (s != HIPBLAS_STATUS_SUCCESS || *got <= 0) {
    psg_set_error("%s: the library lists no algorithm for this problem (hipblasStatus %d)", who, (int)s);
    free_problem(api, p);
    return PSG_ERR_UNSUPPORTED;
  }
  return PSG_OK;
}

int check_shape(const char* who, int rows, int N, int K, int64_t lda, int64_t ldw, int64_t ldy, int batch, int64_t stride_a,
                int64_t stride_w, int64_t stride_y) {
  PSG_REQUIRE(rows > 0 && N > 0 && K > 0 && batch > 0, PSG_ERR_INVALID, "%s: rows=%d N=%d K=%d batch=%d", who, rows, N, K, batch);
  PSG_REQUIRE(lda >= K && ldw >= K && ldy >= N, PSG_ERR_INVALID, "%s: lda=%lld ldw=%lld (K=%d) ldy=%lld (N=%d)", who,
              (long long)lda, (long long)ldw, K, (long long)ldy, N);
  PSG_REQUIRE(batch == 1 || (stride_a >= 0 && stride_w >= 0 && stride_y > 0), PSG_ERR_INVALID,
              "%s: batch strides %lld / %lld / %lld", who, (long long)stride_a, (long long)stride_w, (long long)stride_y);
  // the batches of y must not overlap: either whole matrices apart, or column blocks of one row (ldy >= batch * N)
  PSG_REQUIRE(batch == 1 || stride_y >= (int64_t)(rows - 1) * ldy + N || (stride_y >= N && ldy >= (int64_t)(batch - 1) * stride_y + N),
              PSG_ERR_INVALID, "%s: the %d results overlap (stride_y=%lld ldy=%lld)", who, batch, (long long)stride_y, (long long)ldy);
  return PSG_OK;
}

PsgLt* lt_of(psg_ctx* ctx) { return static_cast<PsgLt*>(ctx->lt); }

}  // namespace

void psg_lt_release(psg_ctx* ctx) {
  PsgLt* lt = lt_of(ctx);
  if (!lt) return;
  for (auto& kv : lt->plans) free_problem(lt->api, kv.second.p);
  if (lt->handle) lt->api.destroy(lt->handle);
  delete lt;
  ctx->lt = nullptr;
}

extern "C" int psg_lt_gemm_init(psg_ctx* ctx, int* lib_version) {
  PSG_REQUIRE(ctx, PSG_ERR_INVALID, "psg_lt_gemm_init: ctx is NULL");
  if (!ctx->lt) {
    PsgLt* lt = new PsgLt();
    if (!resolve(lt->api)) {
      delete lt;
      return PSG_ERR_UNSUPPORTED;
    }
    int dev = -1;
    (void)hipGetDevice(&dev);
    if (dev != ctx->device) (void)hipSetDevice(ctx->device);    // the handle belongs to the current device
    hipblasStatus_t s = lt->api.create(&lt->handle);
    if (s == HIPBLAS_STATUS_SUCCESS) s = lt->api.version(lt->handle, &lt->version);
    if (dev >= 0 && dev != ctx->device) (void)hipSetDevice(dev);
    if (s != HIPBLAS_STATUS_SUCCESS) {
      psg_set_error("psg_lt_gemm_init: hipblasLtCreate / GetVersion failed (hipblasStatus %d)", (int)s);
      if (lt->handle) lt->api.destroy(lt->handle);
      delete lt;
      return PSG_ERR_HIP;
    }
    ctx->lt = lt;
  }
  if (lib_version) *lib_version = lt_of(ctx)->version;
  return PSG_OK;
}

extern "C" int psg_lt_gemm_candidates(psg_ctx* ctx, int rows, int N, int K, int64_t lda, int64_t ldw, int64_t ldy, int batch,
                                      int64_t stride_a, int64_t stride_w, int64_t stride_y, int64_t max_ws_bytes,
                                      int max_count, int* indices, int64_t* ws_bytes, int* count) {
  const char* who = "psg_lt_gemm_candidates";
  PSG_REQUIRE(ctx && indices && ws_bytes && count && max_count > 0, PSG_ERR_INVALID, "%s: NULL argument", who);
  PSG_REQUIRE(ctx->lt, PSG_ERR_INVALID, "%s: call psg_lt_gemm_init first", who);
  if (int rc = check_shape(who, rows, N, K, lda, ldw, ldy, batch, stride_a, stride_w, stride_y)) return rc;
  PsgLt* lt = lt_of(ctx);
  std::lock_guard<std::mutex> lock(lt->mu);
  Problem p;
  if (int rc = make_problem(lt->api, who, rows, N, K, lda, ldw, ldy, batch, stride_a, stride_w, stride_y, p)) return rc;
  hipblasLtMatmulHeuristicResult_t res[kMaxCand];
  int got = 0;
  if (int rc = list_candidates(lt, who, p, max_ws_bytes, res, &got)) return rc;
  int n = 0;
  for (int i = 0; i < got && n < max_count; ++i) {
    if (res[i].state != HIPBLAS_STATUS_SUCCESS) continue;
    indices[n] = lt->api.index_of(res[i].algo);
    ws_bytes[n] = (int64_t)res[i].workspaceSize;
    ++n;
  }
  *count = n;
  free_problem(lt->api, p);
  return PSG_OK;
}

extern "C" int psg_lt_gemm(psg_ctx* ctx, const void* a, const void* w, float* y, int rows, int N, int K, int64_t lda,
                           int64_t ldw, int64_t ldy, int batch, int64_t stride_a, int64_t stride_w, int64_t stride_y, int algo,
                           void* workspace, int64_t workspace_bytes, int* fell_back, void* stream) {
  const char* who = "psg_lt_gemm";
  PSG_REQUIRE(ctx && a && w && y, PSG_ERR_INVALID, "%s: NULL argument", who);
  PSG_REQUIRE(ctx->lt, PSG_ERR_INVALID, "%s: call psg_lt_gemm_init first (no handle is created inside a launch)", who);
  PSG_REQUIRE(workspace_bytes >= 0 && (workspace_bytes == 0 || workspace) && ((uintptr_t)workspace & 15) == 0, PSG_ERR_INVALID,
              "%s: workspace %p of %lld bytes (16-byte aligned, or none)", who, workspace, (long long)workspace_bytes);
  PSG_REQUIRE((((uintptr_t)a | (uintptr_t)w | (uintptr_t)y) & 3) == 0, PSG_ERR_INVALID, "%s: misaligned operand", who);
  if (int rc = check_shape(who, rows, N, K, lda, ldw, ldy, batch, stride_a, stride_w, stride_y)) return rc;
  PsgLt* lt = lt_of(ctx);
  const LtApi& api = lt->api;
  std::lock_guard<std::mutex> lock(lt->mu);
  const ProblemKey key(rows, N, K, lda, ldw, ldy, batch, stride_a, stride_w, stride_y, algo, workspace_bytes);
  auto it = lt->plans.find(key);
  if (it == lt->plans.end()) {                             // host work only: descriptors + one heuristic query, then cached
    Plan pl;
    if (int rc = make_problem(api, who, rows, N, K, lda, ldw, ldy, batch, stride_a, stride_w, stride_y, pl.p)) return rc;
    hipblasLtMatmulHeuristicResult_t res[kMaxCand];
    int got = 0;
    if (int rc = list_candidates(lt, who, pl.p, workspace_bytes, res, &got)) return rc;
    int first = -1, pick = -1;
    for (int i = 0; i < got; ++i) {
      if (res[i].state != HIPBLAS_STATUS_SUCCESS || (int64_t)res[i].workspaceSize > workspace_bytes) continue;
      if (first < 0) first = i;
      if (algo >= 0 && pick < 0 && api.index_of(res[i].algo) == algo) pick = i;
    }
    if (first < 0) {
      psg_set_error("%s: no listed algorithm fits %lld bytes of workspace", who, (long long)workspace_bytes);
      free_problem(api, pl.p);
      return PSG_ERR_UNSUPPORTED;
    }
    pl.fell_back = algo >= 0 && pick < 0;
    if (pick < 0) pick = first;
    pl.algo = res[pick].algo;
    pl.ws_need = (int64_t)res[pick].workspaceSize;
    pl.index = api.index_of(res[pick].algo);
    it = lt->plans.emplace(key, pl).first;
  }
  Plan& pl = it->second;
  if (fell_back) *fell_back = pl.fell_back;
  const float alpha = 1.f, beta = 0.f;
  hipblasStatus_t s = api.matmul(lt->handle, pl.p.desc, &alpha, w, pl.p.lw, a, pl.p.la, &beta, y, pl.p.ly, y, pl.p.ly, &pl.algo,
                                 workspace, (size_t)workspace_bytes, (hipStream_t)stream);
  if (s != HIPBLAS_STATUS_SUCCESS) {
    psg_set_error("%s: hipblasLtMatmul failed (hipblasStatus %d, solution %d)", who, (int)s, pl.index);
    return PSG_ERR_HIP;
  }
  return PSG_OK;
}
