// Device containers behind the C-ABI: Matrix / Vector<int> / CSRMatrix / COOMatrix, the library
// context (one HIP stream per device), error state and the launch profiler.
//
// Replaces implicit/gpu/matrix.cu (reference) -- plain hipMalloc-backed storage instead of RMM
// buffers and managed memory; the Thrust lambdas (copy_rowids, assign_rows, convert_array) and
// calculate_norms_kernel become the small wave64 kernels below.
#include <hip/hip_fp16.h>

#include <algorithm>
#include <cstring>
#include <map>
#include <mutex>
#include <thread>

#include "common.h"
#include "long_tail_route.h"

namespace imp {

static thread_local std::string g_last_error;
void set_last_error(const std::string &msg) { g_last_error = msg; }

static std::mutex g_ctx_mutex;
// leaked on purpose: the contexts own device buffers, and static destructors run after the HIP runtime has shut down
static auto &g_contexts = *new std::map<int, std::unique_ptr<Context>>;
static auto &g_derived = *new std::vector<DerivedCache *>;  // (leaked like the contexts; guarded by g_ctx_mutex)

Context &ctx() {
  int dev = 0;
  IMP_CHECK_HIP(hipGetDevice(&dev));
  std::lock_guard<std::mutex> lock(g_ctx_mutex);
  auto it = g_contexts.find(dev);
  if (it == g_contexts.end()) {
    auto c = std::make_unique<Context>();
    c->device = dev;
    IMP_CHECK_HIP(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
    hipDeviceProp_t prop;
    IMP_CHECK_HIP(hipGetDeviceProperties(&prop, dev));
    c->num_cus = prop.multiProcessorCount;
    if (const char *e = getenv("IMP_OVERSUB")) c->oversub = std::max(1, atoi(e));
    g_derived.push_back(&c->pad.y_key);  // registered for good: a context is never destroyed
    it = g_contexts.emplace(dev, std::move(c)).first;
  }
  return *it->second;
}

void register_derived_cache(DerivedCache *c) {
  std::lock_guard<std::mutex> lock(g_ctx_mutex);
  g_derived.push_back(c);
}
void unregister_derived_cache(DerivedCache *c) {
  std::lock_guard<std::mutex> lock(g_ctx_mutex);
  g_derived.erase(std::remove(g_derived.begin(), g_derived.end(), c), g_derived.end());
}

void note_device_write(const void *dst, size_t bytes) {
  const char *a = static_cast<const char *>(dst);
  std::lock_guard<std::mutex> lock(g_ctx_mutex);
  for (DerivedCache *d : g_derived) {
    const char *b = static_cast<const char *>(d->src);
    if (b && a < b + d->bytes && b < a + bytes) d->src = nullptr;
  }
}
// the one place that decides which memory the library can vouch for: its own, and only until the address is handed out
static bool trusted(const imp_matrix *m) { return m->storage && m->storage->owned && !m->storage->exposed; }
void DerivedCache::bind(const imp_matrix *m) {
  std::lock_guard<std::mutex> lock(g_ctx_mutex);
  src = trusted(m) ? m->as() : nullptr, bytes = m->bytes();
}
bool DerivedCache::made_from(const imp_matrix *m) const {
  std::lock_guard<std::mutex> lock(g_ctx_mutex);
  return src && src == m->as() && bytes == m->bytes() && trusted(m);
}
void DerivedCache::drop() {
  std::lock_guard<std::mutex> lock(g_ctx_mutex);
  src = nullptr;
}

std::unique_lock<std::recursive_mutex> lock_device() {
  try {
    return std::unique_lock<std::recursive_mutex>(ctx().mutex);
  } catch (...) {
    return std::unique_lock<std::recursive_mutex>();  // no usable device: the body reports the error itself
  }
}

// "set to 0 turns it off": on unless the variable is set to a number that reads as zero
static bool env_unless_zero(const char *name) {
  const char *e = getenv(name);
  return !(e && atoi(e) == 0);
}
const SolverSwitches &solver_switches() {
  static const SolverSwitches s = [] {
    SolverSwitches v;
    v.nm = env_unless_zero("IMP_NM");
    v.w256 = getenv("IMP_F256_OLD") == nullptr;
    v.cg_pad = getenv("IMP_NO_PAD") == nullptr;
    v.chol_nm = env_unless_zero("IMP_CHOL_NM");
    v.chol_pad = v.chol_nm && env_unless_zero("IMP_CHOL_PAD");
    return v;
  }();
  return s;
}

void sync() { IMP_CHECK_HIP(hipStreamSynchronize(stream())); }
void sync_call() {
  if (!ctx().deferred) sync();
}

unsigned long long *reset_fail_word() {
  unsigned long long *w = ctx().fail_word.reserve(1);
  IMP_CHECK_HIP(hipMemsetAsync(w, 0xFF, sizeof(unsigned long long), stream()));  // every byte set: kNoFailure
  return w;
}
int64_t read_fail_word(const unsigned long long *w) {
  unsigned long long failed = 0;
  IMP_CHECK_HIP(hipMemcpyAsync(&failed, w, sizeof(failed), hipMemcpyDeviceToHost, stream()));
  sync();
  return failed == kNoFailure ? -1 : (int64_t)failed;
}

// ---- profiler -----------------------------------------------------------------------------------
struct ProfEntry {
  double total_ms = 0;
  int64_t launches = 0;
};
struct ProfPending {
  const char *name;
  hipEvent_t start, stop;
};
static std::recursive_mutex g_prof_mutex;  // the profiler tables are process-wide; per-device call locks do not cover them
static bool g_prof_on = false;
static std::string g_prof_filter;
static std::map<std::string, ProfEntry> g_prof;
static std::vector<ProfPending> g_prof_pending;
static std::vector<hipEvent_t> g_event_pool;

bool prof_enabled() { return g_prof_on; }
bool prof_unfiltered() {
  std::lock_guard<std::recursive_mutex> plock(g_prof_mutex);
  return g_prof_on && g_prof_filter.empty();
}

static hipEvent_t get_event() {
  if (!g_event_pool.empty()) {
    hipEvent_t e = g_event_pool.back();
    g_event_pool.pop_back();
    return e;
  }
  hipEvent_t e;
  IMP_CHECK_HIP(hipEventCreate(&e));
  return e;
}

static void prof_account(const ProfPending &p) {
  float ms = 0;
  if (hipEventElapsedTime(&ms, p.start, p.stop) == hipSuccess) {
    auto &e = g_prof[p.name];
    e.total_ms += ms;
    e.launches += 1;
  }
  g_event_pool.push_back(p.start);
  g_event_pool.push_back(p.stop);
}

// Recycle the event pairs whose kernels have finished (no waiting): creating fresh events for every launch of a long
// timed loop costs far more stream time than recording them.
static void prof_collect_finished() {
  size_t done = 0;
  while (done < g_prof_pending.size() && hipEventQuery(g_prof_pending[done].stop) == hipSuccess) prof_account(g_prof_pending[done++]);
  if (done) g_prof_pending.erase(g_prof_pending.begin(), g_prof_pending.begin() + (long)done);
}

ProfScope::ProfScope(const char *n) : name(n) {
  if (!g_prof_on) return;
  std::lock_guard<std::recursive_mutex> plock(g_prof_mutex);
  if (!g_prof_filter.empty() && !strstr(n, g_prof_filter.c_str())) return;
  if (g_event_pool.size() < 2 && g_prof_pending.size() >= 32) prof_collect_finished();
  start = get_event();
  stop = get_event();
  IMP_CHECK_HIP(hipEventRecord(start, stream()));
}

ProfScope::~ProfScope() {
  if (!start) return;
  std::lock_guard<std::recursive_mutex> plock(g_prof_mutex);
  (void)hipEventRecord(stop, stream());
  g_prof_pending.push_back({name, start, stop});
}

static void prof_flush() {
  std::lock_guard<std::recursive_mutex> plock(g_prof_mutex);
  if (g_prof_pending.empty()) return;
  sync();
  for (auto &p : g_prof_pending) prof_account(p);
  g_prof_pending.clear();
}

// ---- storage ------------------------------------------------------------------------------------
// Recycled small blocks (<= 4 MB, at most 32 per size class and device: a worst case of ~250 MB) are only a cache: an allocation
// that fails gives them all back to the runtime and tries once more.  Safe to hand out without a fence because every library
// stream is joined to the ONE library stream before an entry point returns (class streams, exchange stream, occupy stream),
// and the next user of a block queues its work behind that stream.
static void flush_small_blocks() {
  // only the CALLING thread's device: its lists are what a failed allocation on this device can get back, and it is the one
  // device this thread may synchronise before the blocks go (kernels still in flight on it may touch a recycled block; another
  // device's lists are left to that device's own out-of-memory path)
  std::vector<void *> blocks;
  Context &c = ctx();
  {
    std::lock_guard<std::mutex> g(c.small_mutex);
    for (auto &list : c.small_free) {
      blocks.insert(blocks.end(), list.begin(), list.end());
      list.clear();
    }
  }
  if (!blocks.empty()) (void)hipDeviceSynchronize();
  for (void *b : blocks) (void)hipFree(b);
}
static void device_malloc(void **out, size_t bytes) {
  hipError_t e = hipMalloc(out, bytes);
  if (e == hipErrorOutOfMemory) {
    (void)hipGetLastError();
    flush_small_blocks();
    e = hipMalloc(out, bytes);
  }
  IMP_CHECK_HIP(e);
}

Storage::Storage(size_t bytes_, bool zero) : bytes(bytes_) {
  if (bytes) {
    if (bytes <= kSmallMax) {
      size_class = 8;
      while (((size_t)1 << size_class) < bytes) ++size_class;
      home = &ctx();
      {
        std::lock_guard<std::mutex> g(home->small_mutex);
        auto &list = home->small_free[size_class];
        if (!list.empty()) {
          ptr = list.back();
          list.pop_back();
        }
      }
      if (!ptr) device_malloc(&ptr, (size_t)1 << size_class);
    } else {
      device_malloc(&ptr, bytes);
    }
    if (zero) IMP_CHECK_HIP(hipMemsetAsync(ptr, 0, bytes, stream()));
  }
}
Storage::~Storage() {
  if (!owned || !ptr) return;
  note_device_write(ptr, bytes);  // the memory is about to be re-used for something else
  if (home) {
    std::lock_guard<std::mutex> g(home->small_mutex);
    auto &list = home->small_free[size_class];
    if (list.size() < 32) {
      list.push_back(ptr);
      return;
    }
  }
  (void)hipFree(ptr);
}

// ---- small kernels ------------------------------------------------------------------------------
template <typename T>
__global__ void gather_rows_kernel(const T *__restrict__ src, const int32_t *__restrict__ rowids,
                                   T *__restrict__ dst, size_t nrows, size_t cols) {
  size_t total = nrows * cols;
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total;
       i += (size_t)gridDim.x * blockDim.x) {
    size_t r = i / cols, c = i - r * cols;
    dst[i] = src[(size_t)rowids[r] * cols + c];
  }
}

template <typename T>
__global__ void scatter_rows_kernel(T *__restrict__ dst, const int32_t *__restrict__ rowids,
                                    const T *__restrict__ src, size_t nrows, size_t cols) {
  size_t total = nrows * cols;
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total;
       i += (size_t)gridDim.x * blockDim.x) {
    size_t r = i / cols, c = i - r * cols;
    dst[(size_t)rowids[r] * cols + c] = src[i];
  }
}

__global__ void cast_f32_f16_kernel(const float *__restrict__ src, __half *__restrict__ dst, size_t n) {
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x)
    dst[i] = __float2half(src[i]);
}
__global__ void cast_f16_f32_kernel(const __half *__restrict__ src, float *__restrict__ dst, size_t n) {
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x)
    dst[i] = __half2float(src[i]);
}

// rows of f columns copied with F >= f, the new columns zero, fp16 converted on the way; *skip set: the copy in `dst` is still
// the one the caller needs (pad_check_kernel, als_pad.hip)
template <typename T>
__global__ void pad_rows_kernel(const T *__restrict__ src, float *__restrict__ dst, size_t rows, int f, int F,
                                const int *__restrict__ skip) {
  if (skip && *skip) return;
  const size_t n = rows * (size_t)F;
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    const size_t r = i / F;
    const int c = (int)(i - r * F);
    dst[i] = c < f ? (float)src[r * f + c] : 0.f;
  }
}
template <typename T> void pad_rows(int grid, const T *src, float *dst, size_t rows, int f, int F, const int *skip) {
  pad_rows_kernel<T><<<grid, 256, 0, stream()>>>(src, dst, rows, f, F, skip);
}
template void pad_rows<float>(int, const float *, float *, size_t, int, int, const int *);
template void pad_rows<__half>(int, const __half *, float *, size_t, int, int, const int *);

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

// one wavefront per row: coalesced strided read, butterfly sum, zero norms -> 1e-10
// (matrix.cu:173-188; CPU semantics cpu/matrix_factorization_base.py:233-247)
template <typename T>
__global__ void row_norms_kernel(const T *__restrict__ data, float *__restrict__ out, size_t rows, size_t cols) {
  size_t wave = (blockIdx.x * (size_t)blockDim.x + threadIdx.x) >> 6;
  size_t nwaves = ((size_t)gridDim.x * blockDim.x) >> 6;
  int lane = threadIdx.x & 63;
  for (size_t r = wave; r < rows; r += nwaves) {
    float s = 0.f;
    for (size_t c = lane; c < cols; c += 64) {
      float v = (float)data[r * cols + c];
      s += v * v;
    }
    s = wave_sum(s);
    if (lane == 0) {
      float n = sqrtf(s);
      out[r] = n == 0.f ? 1e-10f : n;
    }
  }
}

static int grid_for(size_t work_items, int block = 256) {
  size_t blocks = (work_items + block - 1) / block;
  size_t cap = (size_t)ctx().num_cus * 8;
  return (int)std::max<size_t>(1, std::min(blocks, cap));
}

// stand-in for a resident collective kernel (imp_debug_occupy): 256 threads and 32 KB of LDS per workgroup, spinning on the
// constant-rate wall clock
__global__ __launch_bounds__(256) void occupy_kernel(long long ticks) {
  extern __shared__ float pad[];
  pad[threadIdx.x] = 0.f;
  const long long t0 = wall_clock64();
  while (wall_clock64() - t0 < ticks) __builtin_amdgcn_s_sleep(32);
}

// imp_debug_core_clock: one wavefront counts core-clock cycles (s_memtime) over a stretch of the constant-rate wall clock
__global__ void core_clock_kernel(long long ticks, unsigned long long *out) {
  const long long w0 = wall_clock64();
  const unsigned long long c0 = __builtin_amdgcn_s_memtime();
  long long w1 = w0;
  while (w1 - w0 < ticks) {
    __builtin_amdgcn_s_sleep(8);
    w1 = wall_clock64();
  }
  const unsigned long long c1 = __builtin_amdgcn_s_memtime();
  if (threadIdx.x == 0) out[0] = c1 - c0, out[1] = (unsigned long long)(w1 - w0);
}

imp_matrix *new_matrix(size_t rows, size_t cols, size_t itemsize, bool zero) {
  if (itemsize != 4 && itemsize != 2) throw std::invalid_argument("invalid itemsize for Matrix (must be 2 or 4)");
  return new imp_matrix(rows, cols, itemsize, std::make_shared<Storage>(rows * cols * itemsize, zero));
}

std::unique_ptr<imp_matrix> astype(const imp_matrix *src, size_t itemsize) {
  std::unique_ptr<imp_matrix> m(new_matrix(src->rows, src->cols, itemsize, false));
  size_t n = src->rows * src->cols;
  if (n) {
    if (itemsize == src->itemsize) {
      IMP_CHECK_HIP(hipMemcpyAsync(m->mut(), src->as(), src->bytes(), hipMemcpyDeviceToDevice, stream()));
    } else if (itemsize == 2) {
      IMP_PROF("cast_f32_f16");
      cast_f32_f16_kernel<<<grid_for(n), 256, 0, stream()>>>(src->as<float>(), m->mut<__half>(), n);
    } else {
      IMP_PROF("cast_f16_f32");
      cast_f16_f32_kernel<<<grid_for(n), 256, 0, stream()>>>(src->as<__half>(), m->mut<float>(), n);
    }
    IMP_CHECK_HIP(hipGetLastError());
  }
  sync();
  return m;
}

}  // namespace imp

using namespace imp;

extern "C" {

const char *imp_last_error(void) { return g_last_error.c_str(); }

const char *imp_version(void) { return "implicit_hip 0.1 (gfx950)"; }

int imp_get_device_count(int *count) {
  return guarded([&] {
    int c = 0;
    IMP_CHECK_HIP(hipGetDeviceCount(&c));
    if (c <= 0) throw std::runtime_error("no HIP device available");
    *count = c;
  });
}

int imp_set_device(int device) {
  return guarded([&] { IMP_CHECK_HIP(hipSetDevice(device)); });
}
int imp_set_oversubscribe(int factor) {
  return guarded([&] {
    if (factor < 1 || factor > 64) throw std::invalid_argument("oversubscription factor must be in [1, 64]");
    ctx().oversub = factor;
  });
}
int imp_get_oversubscribe(int *factor) {
  return guarded([&] { *factor = ctx().oversub; });
}
int imp_set_deferred_sync(int on) {
  return guarded([&] {
    if (!on) {
      sync();  // leaving the mode: everything queued so far is complete on return
    }
    ctx().deferred = on != 0;
  });
}
int imp_debug_occupy(int workgroups, int microseconds) {
  return guarded([&] {
    if (workgroups <= 0 || microseconds <= 0) return;
    auto &c = ctx();
    if (!c.occupy_stream) IMP_CHECK_HIP(hipStreamCreateWithFlags(&c.occupy_stream, hipStreamNonBlocking));
    int rate_khz = 100000;  // wall_clock64 ticks per millisecond
    IMP_CHECK_HIP(hipDeviceGetAttribute(&rate_khz, hipDeviceAttributeWallClockRate, c.device));
    const long long ticks = (long long)microseconds * rate_khz / 1000;
    occupy_kernel<<<workgroups, 256, 32 * 1024, c.occupy_stream>>>(ticks);
    IMP_CHECK_HIP(hipGetLastError());
  });
}
int imp_debug_core_clock(int microseconds, double *mhz) {
  return guarded([&] {
    if (!mhz) throw std::invalid_argument("imp_debug_core_clock: null output");
    auto &c = ctx();
    int rate_khz = 100000;
    IMP_CHECK_HIP(hipDeviceGetAttribute(&rate_khz, hipDeviceAttributeWallClockRate, c.device));
    DeviceArray<unsigned long long> out;
    out.alloc(2, microseconds >= 0);  // (beside: no fill -- it would be queued BEHIND the work on the library stream; the probe writes both words)
    // microseconds < 0: the probe runs on the side stream BESIDE whatever is queued on the library stream (deferred mode: the
    // clock the kernels of a queued step run at, not the clock the chip recovers to behind them)
    const bool beside = microseconds < 0;
    if (beside && !c.occupy_stream) IMP_CHECK_HIP(hipStreamCreateWithFlags(&c.occupy_stream, hipStreamNonBlocking));
    hipStream_t st = beside ? c.occupy_stream : stream();
    core_clock_kernel<<<1, 64, 0, st>>>((long long)std::max(1, std::abs(microseconds)) * rate_khz / 1000, out.data());
    IMP_CHECK_HIP(hipGetLastError());
    unsigned long long h[2] = {0, 0};
    IMP_CHECK_HIP(hipMemcpyAsync(h, out.data(), sizeof(h), hipMemcpyDeviceToHost, st));
    if (beside) IMP_CHECK_HIP(hipStreamSynchronize(st));
    else sync();
    *mhz = h[1] ? (double)h[0] / ((double)h[1] / rate_khz * 1e3) : 0.0;  // cycles per microsecond
  });
}
int imp_get_device(int *device) {
  return guarded([&] { IMP_CHECK_HIP(hipGetDevice(device)); });
}
int imp_solver_fixup_rows(unsigned long long *count, int reset) {
  return guarded([&] {
    sync();  // the counter is written by kernels on the library stream
    unsigned long long *total = fixup_total();
    if (count) *count = *total;
    if (reset) *total = 0ull;
  });
}
int imp_device_synchronize(void) {
  return guarded([&] {
    sync();
    IMP_CHECK_HIP(hipDeviceSynchronize());
  });
}
int imp_release_workspaces(void) {
  return guarded([&] {
    sync();
    auto &c = ctx();
    // scratch the solver paths grow on demand and otherwise keep for the life of the process (a 10 M-row replica padded from
    // f = 100 to 128 is 5 GB): dropped here, re-allocated by the next call that needs them
    c.gram_ws = {};
    c.long_ws = {};
    c.pad.release();
    c.nm_fix_rows = {};
    c.w256_ws = {};
    c.subspace_pred = {};
    c.subspace_ws = {};
    c.slim_diag = {};
    c.slim_ws = {};
    c.slim_items = 0;
    std::lock_guard<std::mutex> g(c.small_mutex);
    for (auto &list : c.small_free) {
      for (void *p : list) (void)hipFree(p);
      list.clear();
    }
  });
}
int imp_mem_get_info(size_t *free_bytes, size_t *total_bytes) {
  return guarded([&] { IMP_CHECK_HIP(hipMemGetInfo(free_bytes, total_bytes)); });
}

// ---- host-side helper: parallel CSR transpose ------------------------------------------------------
// fit() needs both orientations of the confidence matrix (the reference transposes on the host with scipy, implicit/gpu/als.py:121:
// single-threaded, 0.11 s for configs[2]'s 17 M nonzeros -- a third of this path's whole set-up).  Stable counting
// transpose over T threads: thread t owns a run of rows balanced by nonzeros and counts its entries per column; the
// column offsets of thread t are the column's start plus the counts of the threads before it; every thread then scatters
// its rows in order -- rows stay sorted inside every output row, bit-identical to scipy's result on canonical input.
int imp_host_csr_transpose(int32_t rows, int32_t cols, int64_t nnz, const int32_t *indptr, const int32_t *indices, const float *data,
                           int32_t *t_indptr, int32_t *t_indices, float *t_data, int threads) {
  return guarded_host([&] {
    if (rows < 0 || cols < 0 || nnz < 0 || nnz > INT32_MAX) throw std::invalid_argument("host_csr_transpose: sizes out of range");
    if (indptr[0] != 0 || indptr[rows] != nnz) throw std::invalid_argument("host_csr_transpose: indptr does not span the nonzeros");
    // per-thread histograms cost T x cols counters: keep them under 256 MB
    int T = std::max(1, std::min(threads > 0 ? threads : (int)std::thread::hardware_concurrency() / 2, 32));
    while (T > 1 && (size_t)T * (size_t)cols > ((size_t)64 << 20)) --T;
    if (nnz < (1 << 16)) T = 1;
    std::vector<int32_t> cut(T + 1, rows);
    cut[0] = 0;
    for (int t = 1; t < T; ++t) {
      const int64_t target = nnz * t / T;
      cut[t] = (int32_t)(std::lower_bound(indptr, indptr + rows + 1, (int32_t)target) - indptr);
      cut[t] = std::min(rows, std::max(cut[t], cut[t - 1]));
    }
    // a decreasing indptr would send the scatter below out of bounds: checked before anything is indexed through it
    for (int32_t r = 0; r < rows; ++r)
      if (indptr[r + 1] < indptr[r]) throw std::invalid_argument("host_csr_transpose: indptr must be non-decreasing (row " + std::to_string(r) + ")");
    std::vector<std::vector<int32_t>> hist(T);
    for (auto &h : hist) h.assign((size_t)cols, 0);  // allocated HERE: a bad_alloc inside a worker thread would terminate the process
    std::string error;
    std::mutex error_mutex;
    auto parallel = [&](auto &&fn) {
      // an exception escaping a std::thread body calls std::terminate, and so does destroying a joinable thread: every
      // body is fenced, every started thread joined, and the first failure is re-thrown on the calling thread
      auto fenced = [&](int t) {
        try {
          fn(t);
        } catch (const std::exception &e) {
          std::lock_guard<std::mutex> g(error_mutex);
          if (error.empty()) error = std::string("host_csr_transpose: ") + e.what();
        } catch (...) {
          std::lock_guard<std::mutex> g(error_mutex);
          if (error.empty()) error = "host_csr_transpose: unknown failure in a worker thread";
        }
      };
      std::vector<std::thread> pool;
      pool.reserve((size_t)T);
      int started = 1;
      try {
        for (; started < T; ++started) pool.emplace_back(fenced, started);
      } catch (...) {  // the system refused another thread: the caller's thread does the remaining shares
      }
      fenced(0);
      for (int t = started; t < T; ++t) fenced(t);
      for (auto &th : pool) th.join();
      if (!error.empty()) throw std::invalid_argument(error);
    };
    parallel([&](int t) {
      auto &h = hist[t];
      for (int64_t k = indptr[cut[t]]; k < indptr[cut[t + 1]]; ++k) {
        const int32_t c = indices[k];
        if (c < 0 || c >= cols) throw std::invalid_argument("column index out of range");
        ++h[c];
      }
    });
    // column totals -> t_indptr; then every thread's histogram becomes its first output slot per column
    parallel([&](int t) {  // columns split evenly over the threads
      const int32_t c0 = (int32_t)((int64_t)cols * t / T), c1 = (int32_t)((int64_t)cols * (t + 1) / T);
      for (int32_t c = c0; c < c1; ++c) {
        int32_t sum = 0;
        for (int u = 0; u < T; ++u) sum += hist[u][c];
        t_indptr[c + 1] = sum;
      }
    });
    t_indptr[0] = 0;
    for (int32_t c = 0; c < cols; ++c) t_indptr[c + 1] += t_indptr[c];
    parallel([&](int t) {
      const int32_t c0 = (int32_t)((int64_t)cols * t / T), c1 = (int32_t)((int64_t)cols * (t + 1) / T);
      for (int32_t c = c0; c < c1; ++c) {
        int32_t at = t_indptr[c];
        for (int u = 0; u < T; ++u) {
          const int32_t n = hist[u][c];
          hist[u][c] = at;
          at += n;
        }
      }
    });
    parallel([&](int t) {
      auto &pos = hist[t];
      for (int32_t r = cut[t]; r < cut[t + 1]; ++r)
        for (int32_t k = indptr[r]; k < indptr[r + 1]; ++k) {
          const int32_t at = pos[indices[k]]++;
          t_indices[at] = r;
          t_data[at] = data[k];
        }
    });
  });
}

// ---- host-side helper: the schedule imp_csr_create builds, returned to the caller ---------------------
// Validation and planner are the functions imp_csr_create calls (csr_schedule.hip); the knobs are arguments here, not the
// environment.  `which` picks the long-row plan that is copied out: 0 plan_all, 1 plan_chol, 2 plan_nm.
int imp_host_csr_plan(int32_t rows, int32_t cols, const int32_t *indptr, const int32_t *indices, int32_t segment, int32_t stripe,
                      int32_t nm_segment, int32_t num_cus, int which, int32_t *order, int32_t *bin_start, int32_t *row_seg,
                      int64_t seg_capacity, int32_t *seg_row, int32_t *seg_begin, int32_t *seg_end, int32_t *seg_exec,
                      int32_t *xcd_start, int32_t *info) {
  return guarded_host([&] {
    if (which < 0 || which > 2) throw std::invalid_argument("host_csr_plan: which must be 0 (all), 1 (chol) or 2 (nm)");
    if (nm_segment < 0) throw std::invalid_argument("host_csr_plan: nm_segment must be positive, or 0 for the automatic length");
    if (rows < 0) throw std::invalid_argument("negative dimension for CSRMatrix");
    validate_csr(rows, cols, rows ? (int64_t)indptr[rows] : 0, indptr, indices);
    PlanKnobs knobs;
    knobs.segment = segment, knobs.stripe = stripe, knobs.nm_segment = nm_segment, knobs.num_cus = num_cus;
    const HostSchedule s = plan_csr(rows, cols, indptr, indices, knobs);
    const HostPlan &p = which == 0 ? s.plan_all : which == 1 ? s.plan_chol : s.plan_nm;
    if (p.n_seg > seg_capacity) throw std::invalid_argument("host_csr_plan: the plan has more segments than seg_capacity");
    std::copy(s.order.begin(), s.order.end(), order);
    std::copy(s.bin_start, s.bin_start + imp_csr::kBins + 1, bin_start);
    std::copy(p.row_seg.begin(), p.row_seg.end(), row_seg);
    std::copy(p.seg_row.begin(), p.seg_row.end(), seg_row);
    std::copy(p.seg_begin.begin(), p.seg_begin.end(), seg_begin);
    std::copy(p.seg_end.begin(), p.seg_end.end(), seg_end);
    std::copy(p.seg_exec.begin(), p.seg_exec.end(), seg_exec);
    std::copy(p.xcd_start, p.xcd_start + 9, xcd_start);
    const int32_t fields[8] = {p.n_long, p.n_seg, p.striped, s.n_chol_long, s.nm_segment, s.nm_multi_rows, s.nm_multi_segs, 0};
    std::copy(fields, fields + 8, info);
  });
}

// ---- host-side helper: the ticket bases of the chained mid-row launch (team_tickets.h) ----------------
// One launch of the bookkeeping launch_team_chain keeps per device, on a state the caller owns: next[3][8] is advanced in
// place, base[3][8] and draws[3][8] are what the launch is told and how many tickets it draws per queue.
int imp_host_chain_tickets(uint32_t *next, const int32_t *count, int32_t workgroups, const int32_t *teams_per_workgroup, uint32_t *base,
                           uint32_t *draws) {
  return guarded_host([&] {
    constexpr int NC = ChainTickets::kClasses, NQ = ChainTickets::kQueues;
    ChainTickets t;
    int32_t c[NC], n[NC];
    uint32_t b[NC][NQ];
    if (workgroups <= 0) throw std::invalid_argument("host_chain_tickets: the grid holds at least one workgroup");
    for (int k = 0; k < NC; ++k) {
      if (count[k] < 0 || count[k] >= ChainTickets::kMaxCount || teams_per_workgroup[k] <= 0)
        throw std::invalid_argument("host_chain_tickets: a class holds 0 .. 2^30 - 1 rows and a workgroup at least one team");
      c[k] = count[k], n[k] = teams_per_workgroup[k];
      for (int q = 0; q < NQ; ++q) t.next[k][q] = next[k * NQ + q];
    }
    t.launch(c, workgroups, n, b);
    for (int k = 0; k < NC; ++k)
      for (int q = 0; q < NQ; ++q) {
        draws[k * NQ + q] = t.next[k][q] - next[k * NQ + q];
        next[k * NQ + q] = t.next[k][q], base[k * NQ + q] = b[k][q];
      }
  });
}

// The same for the chained 1024-thread launch (launch_wide_chain): next[2][8], rows[2] = rows of (256,512] and short rows; the
// short rows are ticketed in groups of 16.
int imp_host_wide_tickets(uint32_t *next, const int32_t *rows, int32_t workgroups, uint32_t *base, uint32_t *draws) {
  return guarded_host([&] {
    constexpr int NC = WideTickets::kClasses, NQ = WideTickets::kQueues;
    WideTickets t;
    uint32_t b[NC][NQ];
    if (workgroups <= 0) throw std::invalid_argument("host_wide_tickets: the grid holds at least one workgroup");
    for (int k = 0; k < NC; ++k) {
      if (rows[k] < 0 || rows[k] >= WideTickets::kMaxCount)
        throw std::invalid_argument("host_wide_tickets: a class holds 0 .. 2^30 - 1 rows");
      for (int q = 0; q < NQ; ++q) t.next[k][q] = next[k * NQ + q];
    }
    const int32_t r[NC] = {rows[0], rows[1]};
    t.launch_rows(r, workgroups, b);
    for (int k = 0; k < NC; ++k)
      for (int q = 0; q < NQ; ++q) {
        draws[k * NQ + q] = t.next[k][q] - next[k * NQ + q];
        next[k * NQ + q] = t.next[k][q], base[k * NQ + q] = b[k][q];
      }
  });
}

// ---- host-side helper: who runs the tail of the long-row path of a CG half sweep (long_tail_route.h) --
// out[2] = {finish, fixup} in the numbering of LongTailRoute.
int imp_host_long_tail_route(const int32_t *chain_count, const int32_t *wide_count, int32_t n_multi, int32_t capacity, int32_t chained,
                             int32_t *out) {
  return guarded_host([&] {
    if (n_multi < 0 || capacity < 0 || n_multi > capacity)
      throw std::invalid_argument("host_long_tail_route: 0 <= n_multi <= capacity (the rows of more than one segment are long rows)");
    for (int k = 0; k < 3; ++k)
      if (chain_count[k] < 0) throw std::invalid_argument("host_long_tail_route: a class holds no fewer than 0 rows");
    for (int k = 0; k < 2; ++k)
      if (wide_count[k] < 0) throw std::invalid_argument("host_long_tail_route: a class holds no fewer than 0 rows");
    const int32_t chain[3] = {chain_count[0], chain_count[1], chain_count[2]}, wide[2] = {wide_count[0], wide_count[1]};
    const LongTailRoute r = long_tail_route(chain, wide, n_multi, capacity, chained != 0);
    out[0] = r.finish, out[1] = r.fixup;
  });
}

// ---- Matrix -------------------------------------------------------------------------------------
int imp_matrix_create(size_t rows, size_t cols, const void *host_data, size_t itemsize, imp_matrix **out) {
  return guarded([&] {
    imp_matrix *m = new_matrix(rows, cols, itemsize, host_data == nullptr);
    std::unique_ptr<imp_matrix> guard(m);
    if (host_data && m->bytes()) {
      IMP_CHECK_HIP(hipMemcpyAsync(m->mut(), host_data, m->bytes(), hipMemcpyHostToDevice, stream()));
    }
    sync();
    *out = guard.release();
  });
}

int imp_matrix_wrap_device(size_t rows, size_t cols, void *device_ptr, size_t itemsize, imp_matrix **out) {
  return guarded([&] {
    if (itemsize != 4 && itemsize != 2) throw std::invalid_argument("invalid itemsize for Matrix (must be 2 or 4)");
    *out = new imp_matrix(rows, cols, itemsize, std::make_shared<Storage>(device_ptr));
  });
}

int imp_matrix_row(const imp_matrix *src, size_t rowid, imp_matrix **out) {
  return guarded([&] {
    if (rowid >= src->rows) throw std::invalid_argument("row index out of bounds for matrix");
    *out = new imp_matrix(src->rows_view(rowid, 1));  // the C ABI's views are handles of their own: constness ends here
  });
}

int imp_matrix_slice(const imp_matrix *src, size_t start, size_t end, imp_matrix **out) {
  return guarded([&] {
    if (end < start) throw std::invalid_argument("end_rowid < start_rowid for matrix slice");
    if (end > src->rows) throw std::invalid_argument("row index out of bounds for matrix");
    *out = new imp_matrix(src->rows_view(start, end - start));
  });
}

int imp_matrix_gather(const imp_matrix *src, const imp_intvector *rowids, imp_matrix **out) {
  return guarded([&] {
    std::unique_ptr<imp_matrix> m(new_matrix(rowids->size, src->cols, src->itemsize, false));
    size_t total = m->rows * m->cols;
    if (total) {
      IMP_PROF("gather_rows");
      if (src->itemsize == 4)
        gather_rows_kernel<float><<<grid_for(total), 256, 0, stream()>>>(
            src->as<float>(), rowids->v.data(), m->mut<float>(), m->rows, m->cols);
      else
        gather_rows_kernel<__half><<<grid_for(total), 256, 0, stream()>>>(
            src->as<__half>(), rowids->v.data(), m->mut<__half>(), m->rows, m->cols);
      IMP_CHECK_HIP(hipGetLastError());
    }
    sync();
    *out = m.release();
  });
}

int imp_matrix_resize(imp_matrix *m, size_t rows, size_t cols) {
  return guarded([&] {
    if (cols != m->cols) throw std::logic_error("changing number of columns in Matrix::resize is not implemented yet");
    if (rows < m->rows) throw std::logic_error("reducing number of rows in Matrix::resize is not implemented yet");
    auto storage = std::make_shared<Storage>(rows * cols * m->itemsize, true);
    if (m->bytes()) IMP_CHECK_HIP(hipMemcpyAsync(storage->ptr, m->as(), m->bytes(), hipMemcpyDeviceToDevice, stream()));
    sync();
    *m = imp_matrix(rows, cols, m->itemsize, storage);
  });
}

int imp_matrix_assign_rows(imp_matrix *m, const imp_intvector *rowids, const imp_matrix *other) {
  return guarded([&] {
    if (other->cols != m->cols) throw std::invalid_argument("column dimension mismatch for Matrix::assign_rows");
    if (other->rows != rowids->size) throw std::invalid_argument("row dimension mismatch for Matrix::assign_rows");
    // the reference scatters fp32 only (matrix.cu:133-134); fp16 -> fp16 is accepted here as well, so that a half-precision
    // model's partial_fit_* stays on the device
    if (other->itemsize != m->itemsize) throw std::invalid_argument("dtype mismatch for Matrix::assign_rows");
    size_t total = other->rows * other->cols;
    void *dst = m->mut();
    if (total) {
      IMP_PROF("scatter_rows");
      if (m->itemsize == 4)
        scatter_rows_kernel<float><<<grid_for(total), 256, 0, stream()>>>((float *)dst, rowids->v.data(), other->f32(), other->rows,
                                                                          other->cols);
      else
        scatter_rows_kernel<__half><<<grid_for(total), 256, 0, stream()>>>((__half *)dst, rowids->v.data(), other->as<__half>(),
                                                                           other->rows, other->cols);
      IMP_CHECK_HIP(hipGetLastError());
    }
    sync();
  });
}

int imp_matrix_astype(const imp_matrix *src, size_t itemsize, imp_matrix **out) {
  return guarded([&] { *out = astype(src, itemsize).release(); });
}

int imp_matrix_calculate_norms(const imp_matrix *src, imp_matrix **out) {
  return guarded([&] {
    std::unique_ptr<imp_matrix> m(new_matrix(1, src->rows, 4, false));
    if (src->rows) {
      IMP_PROF("row_norms");
      int grid = grid_for(src->rows * 64);
      if (src->itemsize == 4)
        row_norms_kernel<float><<<grid, 256, 0, stream()>>>(src->as<float>(), m->mut<float>(), src->rows, src->cols);
      else
        row_norms_kernel<__half><<<grid, 256, 0, stream()>>>(src->as<__half>(), m->mut<float>(), src->rows, src->cols);
      IMP_CHECK_HIP(hipGetLastError());
    }
    sync();
    *out = m.release();
  });
}

int imp_matrix_to_host(const imp_matrix *m, void *host_out) {
  return guarded([&] {
    if (m->bytes()) IMP_CHECK_HIP(hipMemcpyAsync(host_out, m->as(), m->bytes(), hipMemcpyDeviceToHost, stream()));
    sync();
  });
}

int imp_matrix_from_host(imp_matrix *m, const void *host_in) {
  return guarded([&] {
    void *dst = m->mut();
    if (m->bytes()) IMP_CHECK_HIP(hipMemcpyAsync(dst, host_in, m->bytes(), hipMemcpyHostToDevice, stream()));
    sync();
  });
}

int imp_matrix_copy_rows(imp_matrix *dst, size_t dst_row, const imp_matrix *src, size_t src_row, size_t rows) {
  return guarded([&] {
    if (dst->cols != src->cols || dst->itemsize != src->itemsize)
      throw std::invalid_argument("copy_rows: the two matrices must have rows of the same width and itemsize");
    if (dst_row + rows > dst->rows || src_row + rows > src->rows) throw imp::out_of_range_error("copy_rows: row range out of bounds");
    const size_t row_bytes = dst->cols * dst->itemsize;
    void *to = dst->mut_rows(dst_row, rows);
    if (rows && row_bytes)
      IMP_CHECK_HIP(hipMemcpyAsync(to, src->as<char>() + src_row * row_bytes, rows * row_bytes, hipMemcpyDeviceToDevice, stream()));
    sync_call();  // queue-only in deferred mode, like the exchange it stands in for
  });
}

int imp_matrix_shape(const imp_matrix *m, size_t *rows, size_t *cols, size_t *itemsize) {
  return guarded([&] {
    if (rows) *rows = m->rows;
    if (cols) *cols = m->cols;
    if (itemsize) *itemsize = m->itemsize;
  });
}

int imp_matrix_device_ptr(const imp_matrix *m, void **ptr) {
  return guarded([&] {
    *ptr = m->expose();
  });
}

int imp_matrix_destroy(imp_matrix *m) {
  return guarded([&] { delete m; });
}

// ---- Vector<int> --------------------------------------------------------------------------------
int imp_intvector_create(const int32_t *host_data, size_t size, imp_intvector **out) {
  return guarded([&] {
    auto v = std::make_unique<imp_intvector>();
    v->size = size;
    v->v.upload(host_data, size);
    sync();
    *out = v.release();
  });
}
int imp_intvector_destroy(imp_intvector *v) {
  return guarded([&] { delete v; });
}

// ---- CSR / COO -----------------------------------------------------------------------------------
// IMP_SEGMENT / IMP_STRIPE / IMP_NM_SEGMENT: segment length and column-stripe width of the streamed long-row plan, segment
// length of the normal-matrix work list (read per CSRMatrix; unset = the planner's defaults)
static PlanKnobs plan_knobs_from_env() {
  PlanKnobs k;
  if (const char *e = getenv("IMP_SEGMENT")) k.segment = std::max(32, atoi(e));
  if (const char *e = getenv("IMP_STRIPE")) k.stripe = std::max(0, atoi(e));
  if (const char *e = getenv("IMP_NM_SEGMENT")) k.nm_segment = std::max(64, atoi(e));
  k.num_cus = ctx().num_cus;
  return k;
}

// a validated matrix (or row block) -> device arrays and schedule
static std::unique_ptr<imp_csr> make_csr(int32_t rows, int32_t cols, int64_t nnz, const int32_t *indptr, const int32_t *indices,
                                         const float *data, const PlanKnobs &knobs) {
  auto m = std::make_unique<imp_csr>();
  m->rows = rows;
  m->cols = cols;
  m->nnz = nnz;
  m->indptr.upload(indptr, (size_t)rows + 1);
  m->indices.upload(indices, (size_t)nnz);
  m->data.upload(data, (size_t)nnz);
  const HostSchedule s = plan_csr(rows, cols, indptr, indices, knobs);
  m->order.upload(s.order.data(), s.order.size());
  std::copy(s.bin_start, s.bin_start + imp_csr::kBins + 1, m->bin_start);
  m->plan_all.upload(s.plan_all);
  m->plan_chol.upload(s.plan_chol);
  m->plan_nm.upload(s.plan_nm);
  m->n_chol_long = s.n_chol_long;
  m->nm_segment = s.nm_segment;
  m->nm_multi_rows = s.nm_multi_rows;
  m->nm_multi_segs = s.nm_multi_segs;
  sync();  // the uploads read pageable host memory: the schedule's vectors (and the caller's arrays) live until here
  return m;
}

int imp_csr_create(int32_t rows, int32_t cols, int64_t nnz, const int32_t *indptr, const int32_t *indices,
                   const float *data, imp_csr **out) {
  return guarded([&] {
    validate_csr(rows, cols, nnz, indptr, indices);
    *out = make_csr(rows, cols, nnz, indptr, indices, data, plan_knobs_from_env()).release();
  });
}

// int64 row offsets (scipy switches indptr AND indices to int64 once nnz >= 2^31; the CPU reference accepts both widths,
// _als.pyx:76).  Up to `part_limit` nonzeros the matrix is one block; beyond that it is cut into consecutive row blocks of
// at most that many nonzeros each -- the kernels keep their 32-bit offsets.  IMP_CSR_PART_NNZ lowers the limit (tests).
int imp_csr_create64(int32_t rows, int32_t cols, int64_t nnz, const int64_t *indptr, const int32_t *indices, const float *data,
                     imp_csr **out) {
  return guarded([&] {
    validate_csr(rows, cols, nnz, indptr, indices);
    int64_t part_limit = INT32_MAX;
    if (const char *e = getenv("IMP_CSR_PART_NNZ")) part_limit = std::max<int64_t>(1, std::min<int64_t>(INT32_MAX, atoll(e)));
    const PlanKnobs knobs = plan_knobs_from_env();
    auto build = [&](int32_t r0, int32_t r1) {
      std::vector<int32_t> local((size_t)(r1 - r0) + 1);
      const int64_t base = indptr[r0];
      for (int32_t r = r0; r <= r1; ++r) local[r - r0] = (int32_t)(indptr[r] - base);
      return make_csr(r1 - r0, cols, indptr[r1] - base, local.data(), indices + base, data + base, knobs);
    };
    if (nnz <= part_limit) {
      *out = build(0, rows).release();
      return;
    }
    auto top = std::make_unique<imp_csr>();
    top->rows = rows, top->cols = cols, top->nnz = nnz;
    for (int32_t r0 = 0; r0 < rows;) {
      int32_t r1 = r0;
      while (r1 < rows && indptr[r1 + 1] - indptr[r0] <= part_limit) ++r1;
      if (r1 == r0) throw std::invalid_argument("a single row exceeds the per-block nonzero limit of CSRMatrix");
      top->part_row0.push_back(r0);
      top->parts.push_back(build(r0, r1));
      r0 = r1;
    }
    *out = top.release();
  });
}

int imp_csr_shape(const imp_csr *m, int32_t *rows, int32_t *cols, int64_t *nonzeros) {
  return guarded([&] {
    if (rows) *rows = m->rows;
    if (cols) *cols = m->cols;
    if (nonzeros) *nonzeros = m->nnz;
  });
}

int imp_csr_destroy(imp_csr *m) {
  return guarded([&] { delete m; });
}

int imp_coo_create(int32_t rows, int32_t cols, int64_t nnz, const int32_t *row, const int32_t *col,
                   const float *data, imp_coo **out) {
  return guarded([&] {
    if (rows < 0 || cols < 0 || nnz < 0) throw std::invalid_argument("negative dimension for COOMatrix");
    auto m = std::make_unique<imp_coo>();
    m->rows = rows;
    m->cols = cols;
    m->nnz = nnz;
    m->row.upload(row, (size_t)nnz);
    m->col.upload(col, (size_t)nnz);
    if (data) m->data.upload(data, (size_t)nnz);
    sync();
    *out = m.release();
  });
}

// (row, col) pattern of a host CSR matrix -> device COO.  One wavefront per row writes the row ids, every thread copies its
// share of the column ids; both inputs are read from page-locked host memory in place (coalesced, once)
__global__ void coo_from_csr_kernel(const int32_t *__restrict__ indptr, const int32_t *__restrict__ indices, int rows, int64_t nnz,
                                    int32_t *__restrict__ row_out, int32_t *__restrict__ col_out) {
  const size_t t = blockIdx.x * (size_t)blockDim.x + threadIdx.x, n = (size_t)gridDim.x * blockDim.x;
  for (size_t i = t; i < (size_t)nnz; i += n) col_out[i] = indices[i];
  const int lane = threadIdx.x & 63;
  for (size_t r = t >> 6; r < (size_t)rows; r += n >> 6) {
    const int b = indptr[r], e = indptr[r + 1];
    for (int j = b + lane; j < e; j += 64) row_out[j] = (int32_t)r;
  }
}

int imp_coo_create_from_csr_pattern(int32_t rows, int32_t cols, const void *indptr, int indptr_is_64, const int32_t *indices,
                                    imp_coo **out) {
  return guarded([&] {
    if (rows < 0 || cols < 0) throw std::invalid_argument("negative dimension for COOMatrix");
    if (!indptr) throw std::invalid_argument("COOMatrix.from_csr_pattern: indptr is required");
    const int64_t *p64 = indptr_is_64 ? static_cast<const int64_t *>(indptr) : nullptr;
    const int32_t *p32 = indptr_is_64 ? nullptr : static_cast<const int32_t *>(indptr);
    auto at = [&](int64_t i) -> int64_t { return p64 ? p64[i] : (int64_t)p32[i]; };
    const int64_t base = at(0), nnz = at(rows) - base;
    if (nnz < 0 || nnz > INT32_MAX) throw std::invalid_argument("COOMatrix.from_csr_pattern: nonzero count out of range");
    if (nnz && !indices) throw std::invalid_argument("COOMatrix.from_csr_pattern: indices are required");
    auto m = std::make_unique<imp_coo>();
    m->rows = rows, m->cols = cols, m->nnz = nnz;
    m->row.alloc((size_t)nnz);
    m->col.alloc((size_t)nnz);
    if (nnz) {
      Context &c = ctx();
      const size_t words = (size_t)rows + 1 + (size_t)nnz;
      if (!c.pin_stage_ev) IMP_CHECK_HIP(hipEventCreateWithFlags(&c.pin_stage_ev, hipEventDisableTiming));
      else IMP_CHECK_HIP(hipEventSynchronize(c.pin_stage_ev));  // the previous expand kernel is done with the buffer
      if (c.pin_stage_bytes < words * 4) {
        if (c.pin_stage) (void)hipHostFree(c.pin_stage);
        c.pin_stage = nullptr, c.pin_stage_bytes = 0;
        const size_t want = std::max(words * 4 * 2, (size_t)1 << 20);
        IMP_CHECK_HIP(hipHostMalloc(&c.pin_stage, want, hipHostMallocDefault));
        c.pin_stage_bytes = want;
      }
      int32_t *sp = static_cast<int32_t *>(c.pin_stage), *si = sp + rows + 1;
      int64_t prev = 0;
      for (int64_t r = 0; r <= rows; ++r) {
        const int64_t v = at(r) - base;
        if (v < prev || v > nnz) throw std::invalid_argument("COOMatrix.from_csr_pattern: indptr must be non-decreasing");
        sp[r] = (int32_t)v, prev = v;
      }
      std::memcpy(si, indices + base, (size_t)nnz * 4);
      const int grid = (int)std::min<size_t>(((size_t)std::max<int64_t>(nnz, (int64_t)rows * 64) + 255) / 256, (size_t)c.num_cus * 8);
      coo_from_csr_kernel<<<grid, 256, 0, stream()>>>(sp, si, rows, nnz, m->row.data(), m->col.data());
      IMP_CHECK_HIP(hipGetLastError());
      IMP_CHECK_HIP(hipEventRecord(c.pin_stage_ev, stream()));
      // no host wait: the caller's arrays have been copied, and whatever reads the matrix is queued behind the kernel
    }
    *out = m.release();
  });
}

int imp_coo_destroy(imp_coo *m) {
  return guarded([&] { delete m; });
}

// ---- profiler -------------------------------------------------------------------------------------
int imp_prof_enable(int on) {
  return guarded([&] {
    std::lock_guard<std::recursive_mutex> plock(g_prof_mutex);
    prof_flush();
    g_prof_on = on != 0;
  });
}
int imp_prof_filter(const char *substr) {
  return guarded([&] {
    std::lock_guard<std::recursive_mutex> plock(g_prof_mutex);
    prof_flush();
    g_prof_filter = substr ? substr : "";
  });
}
int imp_prof_reset(void) {
  return guarded([&] {
    std::lock_guard<std::recursive_mutex> plock(g_prof_mutex);
    prof_flush();
    g_prof.clear();
  });
}
int imp_prof_get(const char *kernel, double *total_ms, int64_t *launches) {
  return guarded([&] {
    std::lock_guard<std::recursive_mutex> plock(g_prof_mutex);
    prof_flush();
    auto it = g_prof.find(kernel);
    if (total_ms) *total_ms = it == g_prof.end() ? 0.0 : it->second.total_ms;
    if (launches) *launches = it == g_prof.end() ? 0 : it->second.launches;
  });
}
int imp_prof_names(char *buf, size_t buflen) {
  return guarded([&] {
    std::lock_guard<std::recursive_mutex> plock(g_prof_mutex);
    prof_flush();
    std::string s;
    for (auto &kv : g_prof) {
      if (!s.empty()) s += "\n";
      s += kv.first;
    }
    if (buflen) {
      size_t n = std::min(buflen - 1, s.size());
      memcpy(buf, s.data(), n);
      buf[n] = 0;
    }
  });
}

}  // extern "C"
