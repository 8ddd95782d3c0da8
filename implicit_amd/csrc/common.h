// Internal shared declarations for libimplicit_hip.so (not part of the C-ABI).
#ifndef IMPLICIT_AMD_CSRC_COMMON_H_
#define IMPLICIT_AMD_CSRC_COMMON_H_

#include <hip/hip_runtime.h>

#include <climits>
#include <cstdint>
#include <cstdio>
#include <memory>
#include <mutex>
#include <optional>
#include <stdexcept>
#include <string>
#include <type_traits>
#include <vector>

#include "../../include/implicit_hip.h"
#include "csr_schedule.h"
#include "team_tickets.h"

namespace imp {

// ---- error plumbing: C++ exceptions inside, status codes at the extern "C" edge -------------
struct out_of_range_error : std::runtime_error {
  using std::runtime_error::runtime_error;
};

void set_last_error(const std::string &msg);

#define IMP_CHECK_HIP(expr)                                                                    \
  do {                                                                                         \
    hipError_t _e = (expr);                                                                    \
    if (_e != hipSuccess) {                                                                    \
      throw std::runtime_error(std::string("HIP error: ") + hipGetErrorString(_e) + " (" +    \
                               __FILE__ + ":" + std::to_string(__LINE__) + ")");             \
    }                                                                                          \
  } while (0)

// ---- per-device context: one stream, lazily created; owns every scratch buffer the kernels share ------------------
struct Context;
Context &ctx();  // context of the current device
// Serialises the C-ABI calls of one device: the library stream, the profiler's pending events and the workspaces below
// are shared by everything that runs on a device, and ctypes drops the GIL around every call -- two Python threads
// calling into the same device would otherwise interleave kernels on the same scratch buffers (the reference allocates
// its temporaries per call).  Calls on different devices do not block each other.
std::unique_lock<std::recursive_mutex> lock_device();

// wraps the body of every extern "C" function
template <typename F> int guarded(F &&body) {
  try {
    auto lock = lock_device();
    body();
    return IMP_OK;
  } catch (const std::invalid_argument &e) {
    set_last_error(e.what());
    return IMP_INVALID_ARGUMENT;
  } catch (const out_of_range_error &e) {
    set_last_error(e.what());
    return IMP_OUT_OF_RANGE;
  } catch (const std::exception &e) {
    set_last_error(e.what());
    return IMP_RUNTIME_ERROR;
  } catch (...) {
    set_last_error("unknown error");
    return IMP_RUNTIME_ERROR;
  }
}

// host-only entry points (no stream, no workspace): same error mapping without the device's call lock, so that they can run
// beside device calls of another thread (fit() transposes the matrix while the first CSR uploads)
template <typename F> int guarded_host(F &&body) {
  try {
    body();
    return IMP_OK;
  } catch (const std::invalid_argument &e) {
    set_last_error(e.what());
    return IMP_INVALID_ARGUMENT;
  } catch (const out_of_range_error &e) {
    set_last_error(e.what());
    return IMP_OUT_OF_RANGE;
  } catch (const std::exception &e) {
    set_last_error(e.what());
    return IMP_RUNTIME_ERROR;
  } catch (...) {
    set_last_error("unknown error");
    return IMP_RUNTIME_ERROR;
  }
}

inline hipStream_t stream();
void sync();  // hipStreamSynchronize on the library stream
// end of a C-ABI call that only queues device work (solver sweeps, gramian, all-reduce): host wait unless the device is in
// deferred mode (imp_set_deferred_sync), where the caller orders a whole iteration with ONE imp_device_synchronize
void sync_call();
unsigned long long *fixup_total();  // als_cg_fixup.hip: host-mapped count of the rows the fix-up kernel re-solved on this device
// The A/B and parity switches of the two ALS solvers, read from the environment once per process (containers.hip).  Every
// route they select stays reachable: tests/test_gpu_solver_routes.py runs each of them.
struct SolverSwitches {
  bool nm;        // CG f = 64 / 128: long rows through their explicit normal matrix, als_cg_nm.hip (IMP_NM=0: streamed passes)
  bool w256;      // CG f = 256: rows of <= 256 nonzeros on the resident lock-step kernels, als_cg_w256.hip (IMP_F256_OLD set: all streamed)
  bool cg_pad;    // CG: other factor counts below 256 zero-padded onto f = 64 / 128 / 256 (IMP_NO_PAD set: the generic kernels)
  bool chol_nm;   // Cholesky f = 128: normal matrices on the matrix cores, als_cg_nm.hip (IMP_CHOL_NM=0: the workgroup kernel)
  bool chol_pad;  // Cholesky 64 < f < 128: zero-padded onto f = 128 (IMP_CHOL_PAD=0, or IMP_CHOL_NM=0: the workgroup kernel)
};
const SolverSwitches &solver_switches();

// ---- launch-time profiler (HIP events on the library stream) ------------------------------------
struct ProfScope {
  explicit ProfScope(const char *name);
  ~ProfScope();
  const char *name;
  hipEvent_t start = nullptr, stop = nullptr;
};
bool prof_enabled();
bool prof_unfiltered();  // on, and with no name filter: every scope is timed (a per-kernel pass such as bench.py --full's)
#define IMP_PROF(name) ::imp::ProfScope _prof_scope_(name)
// A scope INSIDE another one (a count of its own for part of what the outer scope times): recorded only when a name filter is
// set -- an unfiltered per-kernel pass adds the scopes up and would count its time twice.
struct NestedProfScope {
  std::optional<ProfScope> scope;
  explicit NestedProfScope(const char *name) {
    if (prof_enabled() && !prof_unfiltered()) scope.emplace(name);
  }
};
#define IMP_PROF_NESTED(name) ::imp::NestedProfScope _prof_nested_(name)

// ---- device storage ---------------------------------------------------------------------------
struct Context;
struct Storage {
  void *ptr = nullptr;
  size_t bytes = 0;
  bool owned = true;
  // small blocks (<= kSmallMax) come from, and return to, their device's free lists instead of hipMalloc / hipFree: a
  // recommend() batch creates and destroys an IntVector and a COO filter (20-50 us of allocator time per object, hipFree
  // synchronises).  Safe without a synchronisation: every side stream (row-class streams, exchange stream) is joined to the
  // library stream of its device before the entry point that used it returns, so a recycled block's next use -- queued on that
  // stream -- is ordered behind its last.  The lists are a cache: an allocation that fails empties them and retries.
  Context *home = nullptr;
  int size_class = -1;
  bool exposed = false;  // the address left the library (imp_matrix_device_ptr): writes to it can no longer be tracked
  static constexpr size_t kSmallMax = (size_t)4 << 20;
  Storage(size_t bytes_, bool zero);
  Storage(void *foreign) : ptr(foreign), owned(false) {}
  ~Storage();
  Storage(const Storage &) = delete;
  Storage &operator=(const Storage &) = delete;
};

template <typename T> struct DeviceArray {
  std::shared_ptr<Storage> storage;
  size_t size = 0;
  T *data() const { return storage ? reinterpret_cast<T *>(storage->ptr) : nullptr; }
  void alloc(size_t n, bool zero = false) {
    storage = std::make_shared<Storage>(n * sizeof(T), zero);
    size = n;
  }
  // grow-only workspace: a new block only when this one is shorter than n (then zeroed if asked; one that is kept is not touched)
  T *reserve(size_t n, bool zero = false) {
    if (size < n) alloc(n, zero);
    return data();
  }
  void upload(const T *host, size_t n) {
    alloc(n);
    if (n) IMP_CHECK_HIP(hipMemcpyAsync(data(), host, n * sizeof(T), hipMemcpyHostToDevice, stream()));
  }
};
// a C-ABI entry point is about to write `bytes` at `dst` through the library (or the memory is being freed, or its address is
// leaving the library): whatever a registered DerivedCache was made from memory the range overlaps is dropped -- wherever the
// cache lives (device addresses are unique across the devices of a process; a Storage may die on a thread whose current device
// is not the one that holds the cache).  Called by the write accessors of imp_matrix below, never by an entry point itself.
void note_device_write(const void *dst, size_t bytes);
// Something derived from a matrix and kept across calls (the fragment-ordered fp16 planes of an item matrix in a KnnQuery
// handle, topk.hip; the zero-padded copy of Y, PaddedSystem), named by the memory it was made from.  Holds for memory only
// the library writes: a Storage whose address was handed out (imp_matrix_device_ptr) or that wraps foreign memory
// (imp_matrix_wrap_device) is never bound to.  The key is only touched under the lock note_device_write takes (containers.hip).
struct DerivedCache {
  void bind(const imp_matrix *m);             // made from m as it is now; from nothing when the library cannot vouch for m's memory
  bool made_from(const imp_matrix *m) const;  // bound to m's address and size, not written since, and m still vouched for
  void drop();

 private:
  friend void note_device_write(const void *, size_t);
  const void *src = nullptr;
  size_t bytes = 0;
};
void register_derived_cache(DerivedCache *c);
void unregister_derived_cache(DerivedCache *c);

// Workspaces of a zero-padded half sweep (als_pad.hip): X, Y and the gramian with F >= f columns, and which matrix `y` is a
// padded copy of -- the chunks of a sharded CG half sweep solve against the same Y, one padded copy serves them all.
struct PaddedSystem {
  DeviceArray<float> x, y, gram;
  DeviceArray<int> same;  // device flag: the gramian of this call equals the one `y` was made under
  DerivedCache y_key;     // registered with its context (ctx())
  size_t y_rows = 0;
  int y_f = 0, y_F = 0;
  void release() {
    y_key.drop();
    x = {}, y = {}, gram = {};
  }
};

// Scratch buffers are per DEVICE (a process may drive several devices through imp_set_device) and are only touched under
// that device's call lock.
struct Context {
  int device = 0;
  hipStream_t stream = nullptr;
  int num_cus = 256;
  // Persistent row kernels launch `slots()` workgroups, each with a fixed share of the rows.  oversub > 1 (multi-GPU
  // driver, imp_set_oversubscribe) launches that many times more workgroups with proportionally smaller shares: when part
  // of the device is held by another stream's kernels (RCCL send / recv) the workgroups that have to wait for a slot no
  // longer carry a full share, and the hardware dispatcher balances the rest.
  int oversub = 1;
  // imp_set_deferred_sync: the queue-only entry points return without a host wait (the multi-GPU driver queues a whole
  // iteration -- K solve chunks, their exchanges, two all-reduces -- and waits once)
  bool deferred = false;
  hipStream_t occupy_stream = nullptr;  // imp_debug_occupy
  std::recursive_mutex mutex;
  std::mutex small_mutex;                  // the free lists below (a Storage may die on a thread that holds another device's lock)
  std::vector<void *> small_free[24];      // [log2 size]: recycled device blocks of 256 B .. 4 MB (Storage)
  // page-locked, device-addressable staging of imp_coo_create_from_csr_pattern: the expand kernel reads it in place; the event
  // marks that kernel's end (the next call waits for it before overwriting the buffer)
  void *pin_stage = nullptr;
  size_t pin_stage_bytes = 0;
  hipEvent_t pin_stage_ev = nullptr;
  DeviceArray<float> gram_ws;     // split-K partial gramians (gramian.hip)
  DeviceArray<float> long_ws;     // partial vectors / CG state of the long rows (als_cg.hip)
  PaddedSystem pad;               // zero-padded copies for factor counts that ride the kernels of a wider one (als_pad.hip)
  DeviceArray<double> loss_buf;   // 4 accumulators of the loss kernel (solver.hip)
  DeviceArray<unsigned long long> fail_word;    // smallest failing row / pivot of the call in flight: Cholesky and subspace sweeps, explain, spd_inverse (reset_fail_word)
  DeviceArray<float> barrier_word;              // operand of the RCCL barrier (comm.hip)
  unsigned long long *fixup_total = nullptr;     // host-mapped: rows re-solved by the fp32 fix-up kernel since the last imp_solver_fixup_rows(reset)
  DeviceArray<float> w256_ws;                    // fp16-split gramian in fragment order + header (als_cg_w256.hip)
  DeviceArray<unsigned> nm_fix_rows;             // rows the normal-matrix kernels left to the fix-up kernel (operands beyond the fp16 range)
  DeviceArray<unsigned> chain_counters;          // ticket counters of the chained mid-row classes, zeroed once and never reset (als_cg_qf.hip)
  ChainTickets chain_tickets;                    // what those counters read after everything queued so far (team_tickets.h)
  DeviceArray<unsigned> wide_counters;           // the same for the chained 1024-thread classes (launch_wide_chain)
  WideTickets wide_tickets;
  DeviceArray<int> nm_ticket;                    // work counter of the normal-matrix kernel (als_cg_nm.hip), reset by every launch
  DeviceArray<unsigned long long> pair_stats;    // [0], [1]: the two counts of a pairwise SGD call (bpr_update: correct / skipped; warp_update: satisfied / trials), [2]: the id check's violation bits (pair_sgd.hip)
  DeviceArray<float> lmf_ws;                     // partial sums of the long rows' segments of lmf_update (lmf.hip)
  DeviceArray<double> knn_acc;                   // dense per-worker accumulators of sparse_topk_product, kept at a sentinel (knn.hip)
  DeviceArray<int32_t> knn_touched;              // the workers' touched-column lists (knn.hip)
  int knn_cols = -1;                             // column count knn_acc is laid out for
  DeviceArray<float> subspace_pred;              // predictions of a subspace half sweep, one per nonzero in CSR order (als_subspace.hip)
  DeviceArray<float> subspace_ws;                // its long rows' segment partials, block steps and failure flags
  DeviceArray<float> slim_diag;                  // the diagonal of A, copied aside by the check of imp_slim_solve (slim.hip)
  DeviceArray<int32_t> slim_ws;                  // its column order, sweep counts, ticket and the two counts of imp_slim_stats
  size_t slim_items = 0;                         // order of the last imp_slim_solve: where the counts sit in slim_ws
};
inline hipStream_t stream() { return ctx().stream; }

// ---- host-side launch conventions ----------------------------------------------
// Dynamic LDS beyond the default limit needs the kernel's opt-in before the launch.  The attribute belongs to the kernel on
// the CURRENT device; the call costs a microsecond or two and most launchers make it every time.
template <typename K> void allow_dynamic_lds(K *kernel, size_t bytes) {
  IMP_CHECK_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
}
// The same once per kernel AND DEVICE, for launches short enough for the call to weigh and kernels whose `bytes` never
// change.  Never once per process: a process may drive several devices (imp_set_device), and the second one would launch the
// kernel without its LDS.  The flags are only touched under a device's call lock, each device its own byte.
template <auto Kernel> void allow_dynamic_lds_once(size_t bytes) {
  static bool done[64] = {};
  const int dev = ctx().device;
  if (dev >= 0 && dev < 64 && done[dev]) return;
  allow_dynamic_lds(Kernel, bytes);
  if (dev >= 0 && dev < 64) done[dev] = true;
}

// The device word a sweep's kernels atomicMin their failing row (or pivot) into: ctx().fail_word, one per device.
constexpr unsigned long long kNoFailure = ~0ULL;
unsigned long long *reset_fail_word();                 // set to kNoFailure on the library stream (containers.hip)
int64_t read_fail_word(const unsigned long long *w);   // waits for the stream; -1, or the smallest index recorded

// containers.hip
imp_matrix *new_matrix(size_t rows, size_t cols, size_t itemsize, bool zero);  // invalid_argument unless itemsize is 2 or 4
std::unique_ptr<imp_matrix> astype(const imp_matrix *src, size_t itemsize);    // converted (or plain) copy, complete on return
// dst[r][0 .. F) = src[r][0 .. f), zeros beyond; does nothing when *skip is set (pad_check_kernel, als_pad.hip).  The caller
// chooses the grid (256 threads) and owns the profiler scope and the error check.
template <typename T> void pad_rows(int grid, const T *src, float *dst, size_t rows, int f, int F, const int *skip = nullptr);
// als_cg.hip
void zero_rows(const int32_t *order, int first, int count, float *X, int f);
}  // namespace imp

// ---- handle definitions (opaque in the public header) -------------------------------------------
// The device pointer is private: reading gives const pointers, and the only way to a mutable one is an accessor that reports
// the write (note_device_write) for exactly the bytes it hands out -- nothing derived from the matrix outlives a write to it.
struct imp_matrix {
  size_t rows = 0, cols = 0, itemsize = 4;
  std::shared_ptr<imp::Storage> storage;
  imp_matrix() = default;
  imp_matrix(size_t rows_, size_t cols_, size_t itemsize_, std::shared_ptr<imp::Storage> s)
      : rows(rows_), cols(cols_), itemsize(itemsize_), storage(std::move(s)), data(storage ? storage->ptr : nullptr) {}
  size_t bytes() const { return rows * cols * itemsize; }
  template <typename T = void> const T *as() const { return static_cast<const T *>(data); }
  const float *f32() const { return check_f32(), as<float>(); }
  // rows [first, first + count), about to be written
  template <typename T = void> T *mut_rows(size_t first, size_t count) {
    if (std::is_same<T, float>::value) check_f32();
    char *p = static_cast<char *>(data) + first * cols * itemsize;
    imp::note_device_write(p, count * cols * itemsize);
    return reinterpret_cast<T *>(p);
  }
  template <typename T = void> T *mut() { return mut_rows<T>(0, rows); }
  // rows [first, first + count) as a matrix of their own that shares the storage; const of a const matrix
  imp_matrix rows_view(size_t first, size_t count) { return view(*this, first, count); }
  const imp_matrix rows_view(size_t first, size_t count) const { return view(*this, first, count); }
  bool overlaps(const imp_matrix *o) const {  // the two share device memory
    const char *a = as<char>(), *b = o->as<char>();
    return bytes() && o->bytes() && a < b + o->bytes() && b < a + bytes();
  }
  // imp_matrix_device_ptr: whoever holds the address may write through it -- nothing derived from this memory is cached from
  // now on, and what was derived from it before is dropped
  void *expose() const {
    if (storage) storage->exposed = true;
    imp::note_device_write(data, bytes());
    return data;
  }

 private:
  void *data = nullptr;  // may point inside storage (views)
  void check_f32() const {
    if (itemsize != 4) throw std::runtime_error("can't cast Matrix to float*");
  }
  static imp_matrix view(const imp_matrix &m, size_t first, size_t count) {
    imp_matrix v = m;
    v.rows = count;
    v.data = static_cast<char *>(m.data) + first * m.cols * m.itemsize;
    return v;
  }
};

struct imp_intvector {
  imp::DeviceArray<int32_t> v;
  size_t size = 0;
};

// Device view of the long-row plan (passed to kernels by value).
struct LongPlanDev {
  int n_long, n_seg;
  const int32_t *rows;       // [n_long]   row id of each long row
  const int32_t *row_seg;    // [n_long+1] first segment of each long row
  const int32_t *seg_row;    // [n_seg]    long-row index of each segment
  const int32_t *seg_begin;  // [n_seg]    nnz range of each segment
  const int32_t *seg_end;    // [n_seg]
  const int32_t *seg_exec;   // [n_seg]    execution order of the partial kernel: segment ids grouped by XCD
  int xcd_start[9];          // seg_exec[xcd_start[x] .. xcd_start[x+1]) is swept by the workgroups with blockIdx % 8 == x
};

// Host-side owner of one long-row plan (device arrays + the per-XCD cut of the execution order).
struct LongPlan {
  int32_t n_long = 0, n_seg = 0;
  imp::DeviceArray<int32_t> row_seg, seg_row, seg_begin, seg_end, seg_exec;
  int32_t xcd_start[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
  void upload(const imp::HostPlan &p) {  // queued on the library stream: `p` has to outlive the next sync()
    n_long = p.n_long, n_seg = p.n_seg;
    seg_exec.upload(p.seg_exec.data(), p.seg_exec.size());
    row_seg.upload(p.row_seg.data(), p.row_seg.size());
    seg_row.upload(p.seg_row.data(), p.seg_row.size());
    seg_begin.upload(p.seg_begin.data(), p.seg_begin.size());
    seg_end.upload(p.seg_end.data(), p.seg_end.size());
    for (int x = 0; x < 9; ++x) xcd_start[x] = p.xcd_start[x];
  }
  LongPlanDev dev(const int32_t *rows) const {
    LongPlanDev d{n_long, n_seg, rows, row_seg.data(), seg_row.data(), seg_begin.data(), seg_end.data(), seg_exec.data(), {0}};
    for (int x = 0; x < 9; ++x) d.xcd_start[x] = xcd_start[x];
    return d;
  }
};

// Rows are scheduled in length classes so that the work per wavefront is even and the longest rows
// start first (SURVEY section 7 "load imbalance"): `order` = row ids sorted by descending nnz;
// class b covers order[bin_start[b] .. bin_start[b+1]) and holds the rows with
// kClassMax[b+1] < nnz <= kClassMax[b]:
//   0 long  (> 512 nnz): cut into segments of <= kSegment nnz (column-striped when the rows re-use the gathered
//        matrix enough, see build_plan in csr_schedule.hip), segment-parallel CG passes
//   1..4 mid (256,512], (128,256], (64,128], (32,64]: a TEAM of 16/8/4/2 wavefronts per row, every
//        wavefront keeps one 32-row gathered tile in registers for all passes
//   5 short (16,32] and 6 short (0,16]: one wavefront per row, resident tile of 32 / 16 entries, 16 rows per
//        workgroup in lock step (MFMA gramian product)
//   7 empty
struct imp_csr : imp::CsrClasses {
  int32_t rows = 0, cols = 0;
  int64_t nnz = 0;
  imp::DeviceArray<int32_t> indptr, indices;
  imp::DeviceArray<float> data;
  imp::DeviceArray<int32_t> order;
  int32_t bin_start[kBins + 1] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
  // long-row plans: `plan_all` covers every row of class 0 (> kLongRow nonzeros) and is what the generic kernels (and the f = 64 /
  // 128 path under IMP_NM=0) stream.  Rows of more than kCholLongRow nonzeros (the first n_chol_long entries of `order`) cut into
  // plain runs of kCholSegment: the A-build of the f = 64 Cholesky kernel is segment-parallel for them (als_cholesky.hip)
  LongPlan plan_all;
  LongPlan plan_chol;
  int32_t n_chol_long = 0;
  // every row of class 0 cut into plain runs of `nm_segment` nonzeros (2048 .. 16384: about eight segments per CU and launch, so
  // that neither the tail of the launch nor the partial matrices of the cut rows weigh): the work list of the normal-matrix
  // kernels (als_cg_nm.hip).  The first nm_multi_rows rows (those longer than one segment) own the first nm_multi_segs segments.
  LongPlan plan_nm;
  int32_t nm_segment = 2048, nm_multi_rows = 0, nm_multi_segs = 0;
  // A matrix with more than 2^31 - 1 nonzeros (imp_csr_create64) is held as consecutive row blocks, each a complete
  // imp_csr of its own with int32 offsets; the top-level object then only carries rows / cols / nnz and the solver
  // entry points walk the blocks (every row solve is independent of the others).
  std::vector<std::unique_ptr<imp_csr>> parts;
  std::vector<int32_t> part_row0;  // first row of each block
  int32_t nonempty() const { return bin_start[kBins - 1]; }
  int32_t first_empty() const { return bin_start[kBins - 1]; }
  int32_t n_empty() const { return bin_start[kBins] - bin_start[kBins - 1]; }
};

struct imp_coo {
  int32_t rows = 0, cols = 0;
  int64_t nnz = 0;
  imp::DeviceArray<int32_t> row, col;
  imp::DeviceArray<float> data;
};

namespace imp {
// als_pad.hip: the first rows_of_X rows of X, Y and the gramian zero-padded to F columns in ctx().pad (the gramian with a unit
// diagonal block), as views; pad_out copies the solved rows back.  reuse_y: keep the copy of Y for the next call against the same
// matrix under the same gramian (compared on the device) -- and use the one the previous call kept.
struct PaddedViews {
  imp_matrix X, Y, YtY;
};
PaddedViews pad_in(const imp_matrix *X, const imp_matrix *Y, const imp_matrix *YtY, size_t rows_of_X, int F, bool reuse_y);
void pad_out(imp_matrix *X, size_t rows_of_X, int F);
// als_cg_nm.hip: Cholesky half sweep at f = 128 through the rows' normal matrices on the matrix cores; what it could not factorise
// comes back as a device-side list for the workgroup-per-row fp32 kernel (als_cholesky.hip)
struct CholNmList {
  const unsigned *count, *rows;
  int capacity;
};
CholNmList least_squares_cholesky_nm(const imp_csr *C, float *X, const float *Y, size_t y_rows, const float *YtY, float reg);
// als_cg_fixup.hip: the fp32 one-wavefront-per-row solver for the rows listed in rows[0 .. *count) (F = 64 / 128, float / __half)
template <int F, typename T>
void launch_cg_fixup(const unsigned *count, const unsigned *rows, int capacity, const imp_csr *C, T *X, const T *Y, const float *A0,
                     int cg_steps);

// ---- the solver routes behind solver.hip, one block of rows each (an imp_csr without parts) ------
// gramian.hip: out = Y^T Y + reg I
void gramian(const float *Y, long n_rows, int f, float reg, float *out);
void gramian_half(const void *Y, long n_rows, int f, float reg, float *out);  // fp16 rows, fp32 products
// als_cg.hip and the kernels it dispatches to
bool cg_native_half(int f);
void least_squares_cg(const imp_csr *C, imp_matrix *X, const imp_matrix *YtY, const imp_matrix *Y, int cg_steps);
// What is pending behind the normal-matrix kernel of a CG half sweep (als_cg_nm.hip), handed from its launcher to the class
// dispatch, which decides who runs it (long_tail_route.h): the first n_multi rows of the plan were built in more than one
// segment and wait for the sum of their partial images and the CG on it; rows a solve could not finish in fp16-split operands
// are listed in fix_rows (ctl[2] counts them, at most `capacity`) for the fp32 fix-up.
struct NmTail {
  LongPlanDev plan{};
  int n_multi = 0;
  float *gram_img = nullptr, *partial = nullptr;
  int *ctl = nullptr;
  unsigned *fix_rows = nullptr;
  int capacity = 0;  // 0: no normal-matrix launch, nothing is pending
};
// als_cg_q.hip: the classes below the long rows, and the tail of the long rows
template <typename T> void least_squares_cg_q(const imp_csr *C, T *X, const T *Y, const float *A0, int f, int cg_steps, const NmTail &tail);
void least_squares_cg_w256(const imp_csr *C, float *X, const float *Y, const float *A0, int cg_steps);                    // als_cg_w256.hip
// als_cg_nm.hip: the gramian image and the normal-matrix kernel, queued; cg_nm_finish: the stand-alone reduce + finish of its tail
template <typename T> NmTail least_squares_cg_nm(const imp_csr *C, T *X, const T *Y, size_t y_rows, const float *A0, int f, int cg_steps);
template <typename T> void cg_nm_finish(const NmTail &tail, T *X, int f, int cg_steps);
// als_cholesky.hip, als_subspace.hip: -1, or the smallest failing row of the block
int64_t least_squares_cholesky(const imp_csr *C, imp_matrix *X, const imp_matrix *YtY, const imp_matrix *Y, double reg);
int64_t least_squares_subspace(const imp_csr *C, imp_matrix *X, const imp_matrix *YtY, const imp_matrix *Y, double reg, int block_size,
                               int sweeps);
// topk.hip: the handle's max_temp_memory, for rank.hip and ease.hip, which share the handle's budget only
size_t knn_temp_budget(const imp_knn *k);
}  // namespace imp

#endif  // IMPLICIT_AMD_CSRC_COMMON_H_
