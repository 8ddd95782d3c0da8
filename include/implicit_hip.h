/*
 * implicit_hip.h -- C-ABI of libimplicit_hip.so, the MI355X (gfx950) replacement for the
 * native half of benfred/implicit's `implicit.gpu` plug-in.
 *
 * Every entry point below is what a binding for this path binds instead of the reference's C++
 * classes (which Cython reaches through implicit/gpu/{matrix,als,knn,random,utils}.pxd).  The
 * reference interface each one replaces is cited as file:line relative to the reference tree.
 * Plain pointers, sizes and opaque handles only: no C++ types, no torch types.
 *
 * Conventions
 *   - every function returns an imp_status; on failure imp_last_error() (thread-local) holds the
 *     message.  The mapping to the reference's exceptions (implicit/gpu/utils.h:15-73 and the
 *     Cython `except +` translation) is: IMP_INVALID_ARGUMENT -> std::invalid_argument ->
 *     ValueError; IMP_OUT_OF_RANGE -> IndexError; IMP_RUNTIME_ERROR -> std::runtime_error /
 *     std::logic_error -> RuntimeError.  No C++ exception ever crosses this boundary.
 *   - all calls are synchronous on return, like the reference's (cudaDeviceSynchronize after each
 *     kernel, implicit/gpu/als.cu:147,151,196,276; sync_stream, knn.cu:254).  Work is issued on
 *     one library-owned HIP stream per device.
 *   - matrices are row-major; itemsize 4 = fp32, 2 = fp16 storage (implicit/gpu/matrix.h:23-90).
 *   - handles own device memory; row/slice views share their parent's storage by reference count
 *     (reference: shared_ptr<rmm::device_buffer>, matrix.h:90).
 */
#ifndef IMPLICIT_HIP_H_
#define IMPLICIT_HIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum {
  IMP_OK = 0,
  IMP_INVALID_ARGUMENT = 1, /* ValueError   */
  IMP_OUT_OF_RANGE = 2,     /* IndexError   */
  IMP_RUNTIME_ERROR = 3     /* RuntimeError */
} imp_status;

typedef struct imp_matrix imp_matrix;       /* implicit::gpu::Matrix       matrix.h:23-90  */
typedef struct imp_intvector imp_intvector; /* implicit::gpu::Vector<int>  matrix.h:12-21  */
typedef struct imp_csr imp_csr;             /* implicit::gpu::CSRMatrix    matrix.h:92-99  */
typedef struct imp_coo imp_coo;             /* implicit::gpu::COOMatrix    matrix.h:101-108 */
typedef struct imp_solver imp_solver;       /* implicit::gpu::LeastSquaresSolver  als.h:11-24 */
typedef struct imp_knn imp_knn;             /* implicit::gpu::KnnQuery     knn.h:15-35     */
typedef struct imp_random imp_random;       /* implicit::gpu::RandomState  random.h:10-21  */
typedef struct imp_comm imp_comm;           /* NEW: RCCL communicator (reference: "TODO: multi-gpu", als.cu:169) */

/* ---- library / device ------------------------------------------------------------------- */
const char *imp_last_error(void);
/* get_device_count(), utils.h:75-79: fails with IMP_RUNTIME_ERROR when no device is usable. */
int imp_get_device_count(int *count);
int imp_set_device(int device);
int imp_get_device(int *device);
/* NEW (multi-GPU robustness).  The row kernels are persistent: by default exactly as many workgroups as the device holds at
 * once, each with a fixed share of the rows.  While another stream's kernels (RCCL send / recv) hold part of the device, the
 * workgroups that must wait for a slot would do their whole share late.  factor > 1 launches factor x as many workgroups
 * with proportionally smaller shares; the hardware dispatcher then balances them over the slots that are free. */
int imp_set_oversubscribe(int factor);
int imp_get_oversubscribe(int *factor);
/* NEW.  Every call is synchronous on return by default (convention above).  on = 1 puts the CURRENT device into deferred
 * mode: imp_solver_calculate_yty, imp_solver_least_squares and imp_comm_allreduce_sum only queue their work on the library
 * stream and return; the caller orders a whole iteration with one imp_device_synchronize (which also reports a timed-out
 * cluster exchange).  The multi-GPU driver uses it so that a chunk's exchange is queued without a host round trip per chunk.
 * on = 0 waits for everything queued and restores the default. */
int imp_set_deferred_sync(int on);
/* Measurement aid: occupies `workgroups` x (256 threads, 32 KB LDS) for about `microseconds` on a stream of its own. */
int imp_debug_occupy(int workgroups, int microseconds);
/* Measurement aid: the shader core clock right now, in MHz -- a one-wavefront kernel queued on the library stream counts core
 * cycles over `microseconds` of the constant-rate wall clock (behind whatever is queued: the clock the chip has recovered to).
 * microseconds < 0: the probe runs on a side stream BESIDE the work queued on the library stream (deferred mode) -- the clock
 * the queued kernels themselves run at (a power-limited chip clocks an MFMA-heavy kernel well below its idle clock). */
int imp_debug_core_clock(int microseconds, double *mhz);
int imp_device_synchronize(void);
/* NEW.  Rows of CG sweeps on the CURRENT device that a fast kernel declined to store and the fp32 one-wavefront-per-row fix-up
 * kernel re-solved instead, since the last reset: rows of a cluster whose exchange through memory was lost, and long rows whose
 * fp16-split matrix-core operands left the fp16 range (factors or confidences far outside anything ALS produces).  Results are
 * correct either way; a non-zero count says the sweep ran slower than it should.  Waits for the library stream. */
int imp_solver_fixup_rows(unsigned long long *count, int reset);
int imp_mem_get_info(size_t *free_bytes, size_t *total_bytes);
/* NEW: frees the per-device scratch buffers the solver paths grow on demand (split-K gramian partials, long-row CG state, the
 * zero-padded copies other factor counts ride the f = 64 / 128 / 256 kernels on, cluster exchange slots, the predictions and
 * segment partials of imp_solver_least_squares_subspace); the next call that
 * needs one allocates it again.  fit() calls it when it returns. */
int imp_release_workspaces(void);
const char *imp_version(void);

/* NEW, host-side helper (no device work, usable without a GPU): stable parallel transpose of a CSR matrix with int32 offsets
 * (the reference's fit transposes on the host with scipy, implicit/gpu/als.py:121).  Outputs are caller-allocated:
 * t_indptr[cols + 1], t_indices[nonzeros], t_data[nonzeros]; row ids inside every output row come out ascending.
 * threads <= 0: half the hardware threads, at most 32. */
int imp_host_csr_transpose(int32_t rows, int32_t cols, int64_t nonzeros, const int32_t *indptr, const int32_t *indices,
                           const float *data, int32_t *t_indptr, int32_t *t_indices, float *t_data, int threads);

/* NEW, host-side helper (no device work, usable without a GPU): the row schedule and one long-row plan exactly as
 * imp_csr_create builds them, with the knobs as arguments: segment (nonzeros per segment of the streamed plan; IMP_SEGMENT),
 * stripe (its column-stripe width; < 0 automatic, 0 never striped; IMP_STRIPE), nm_segment (segment of the normal-matrix work
 * list; 0 automatic; IMP_NM_SEGMENT), num_cus (compute units the automatic nm_segment is sized for).  which: 0 the streamed
 * plan of every row > 512 nonzeros, 1 the Cholesky plan of the rows > 1024, 2 the normal-matrix work list.  Outputs are
 * caller-allocated: order[rows] (row ids by descending length), bin_start[9] (length classes of `order`), row_seg[rows + 1] (the
 * first n_long + 1 entries are written), seg_row / seg_begin / seg_end / seg_exec[seg_capacity] (n_seg entries are written; a
 * segment holds at least one nonzero, so indptr[rows] always suffices; IMP_INVALID_ARGUMENT if the plan does not fit),
 * xcd_start[9], info[8] = {n_long, n_seg, striped, n_chol_long, nm_segment, nm_multi_rows, nm_multi_segs, 0}.  The matrix is
 * validated as by imp_csr_create. */
int imp_host_csr_plan(int32_t rows, int32_t cols, const int32_t *indptr, const int32_t *indices, int32_t segment, int32_t stripe,
                      int32_t nm_segment, int32_t num_cus, int which, int32_t *order, int32_t *bin_start, int32_t *row_seg,
                      int64_t seg_capacity, int32_t *seg_row, int32_t *seg_begin, int32_t *seg_end, int32_t *seg_exec,
                      int32_t *xcd_start, int32_t *info);

/* Host code, no device involved: one launch of the ticket bookkeeping of the chained mid-row CG classes (team widths 8, 4, 2,
 * eight queues each; csrc/team_tickets.h) on a state the caller owns.  next[3][8]: the values the queues' device counters read
 * before the launch, advanced in place (modulo 2^32) by the tickets the launch draws; count[3]: rows per class (0 .. 2^30 - 1);
 * workgroups: the grid (> 0); teams_per_workgroup[3] (> 0).  Outputs: base[3][8], the counter values the kernel is told, and
 * draws[3][8]. */
int imp_host_chain_tickets(uint32_t *next, const int32_t *count, int32_t workgroups, const int32_t *teams_per_workgroup, uint32_t *base,
                           uint32_t *draws);

/* Host code, no device involved: the same for the chained 1024-thread CG classes -- (256,512], one 16-wavefront team per row, and
 * the short rows, ticketed in groups of 16 consecutive schedule rows; one team per workgroup in both.  next[2][8], rows[2]
 * (0 .. 2^30 - 1 each), workgroups (> 0); outputs base[2][8] and draws[2][8]. */
int imp_host_wide_tickets(uint32_t *next, const int32_t *rows, int32_t workgroups, uint32_t *base, uint32_t *draws);

/* Host code, no device involved: who runs the tail of the long-row path of a CG half sweep (csrc/long_tail_route.h).
 * chain_count[3]: rows of (128,256], (64,128], (32,64]; wide_count[2]: rows of (256,512] and short rows; n_multi: long rows of
 * more than one segment; capacity: entries of the fix list (0 <= n_multi <= capacity); chained: non-zero where the half sweep
 * takes the two chained launches.  out[0]: 0 nothing to finish, 1 stand-alone reduce + finish, 2 the head of the team chain;
 * out[1]: 0 no fix-up, 1 stand-alone ahead of the classes, 2 stand-alone behind the team chain, 3 the head of the wide chain. */
int imp_host_long_tail_route(const int32_t *chain_count, const int32_t *wide_count, int32_t n_multi, int32_t capacity, int32_t chained,
                             int32_t *out);

/* ---- Matrix (matrix.h:23-90, matrix.cu:34-220) -------------------------------------------- */
/* Matrix(rows, cols, data, allocate=true, itemsize): allocates; copies rows*cols*itemsize bytes
 * from host_data when non-NULL, zero-fills otherwise (matrix.cu:80-96). */
int imp_matrix_create(size_t rows, size_t cols, const void *host_data, size_t itemsize, imp_matrix **out);
/* Matrix(rows, cols, device_ptr, allocate=false, itemsize): wraps foreign device memory, never
 * frees it (matrix.cu:93-95; __cuda_array_interface__ path of _cuda.pyx:99-104). */
int imp_matrix_wrap_device(size_t rows, size_t cols, void *device_ptr, size_t itemsize, imp_matrix **out);
/* Matrix(other, rowid): one-row view sharing storage (matrix.cu:34-40). */
int imp_matrix_row(const imp_matrix *m, size_t rowid, imp_matrix **out);
/* Matrix(other, start, end): row-range view sharing storage (matrix.cu:42-53). */
int imp_matrix_slice(const imp_matrix *m, size_t start, size_t end, imp_matrix **out);
/* Matrix(other, rowids): gather-copy of the selected rows (matrix.cu:55-78). */
int imp_matrix_gather(const imp_matrix *m, const imp_intvector *rowids, imp_matrix **out);
/* Matrix::resize: grows rows only, zero-fills the new rows (matrix.cu:98-120). */
int imp_matrix_resize(imp_matrix *m, size_t rows, size_t cols);
/* Matrix::assign_rows(rowids, other): scatter rows of `other` (fp32 only, matrix.cu:122-143). */
int imp_matrix_assign_rows(imp_matrix *m, const imp_intvector *rowids, const imp_matrix *other);
/* Matrix::astype(itemsize): fp32 <-> fp16 copy (matrix.cu:153-171). */
int imp_matrix_astype(const imp_matrix *m, size_t itemsize, imp_matrix **out);
/* Matrix::calculate_norms(): 1 x rows fp32 L2 norms, zeros replaced by 1e-10 (matrix.cu:173-215). */
int imp_matrix_calculate_norms(const imp_matrix *m, imp_matrix **out);
/* Matrix::to_host (matrix.cu:217-220). */
int imp_matrix_to_host(const imp_matrix *m, void *host_out);
/* NEW: overwrite the matrix from host memory (same shape/itemsize); used to re-seed parity runs. */
int imp_matrix_from_host(imp_matrix *m, const void *host_in);
/* NEW: device-to-device copy of `rows` whole rows, src[src_row ..] -> dst[dst_row ..] (same width and itemsize), queued on
 * the library stream (queue-only in deferred mode).  What an exchange between LOGICAL ranks that share one device is made
 * of (implicit_amd/gpu/local_comm.py: the N-rank driver exercised on one GPU). */
int imp_matrix_copy_rows(imp_matrix *dst, size_t dst_row, const imp_matrix *src, size_t src_row, size_t rows);
int imp_matrix_shape(const imp_matrix *m, size_t *rows, size_t *cols, size_t *itemsize);
int imp_matrix_device_ptr(const imp_matrix *m, void **ptr);
int imp_matrix_destroy(imp_matrix *m);

/* ---- Vector<int> / CSRMatrix / COOMatrix (matrix.cu:13-32, 222-280) ------------------------- */
int imp_intvector_create(const int32_t *host_data, size_t size, imp_intvector **out);
int imp_intvector_destroy(imp_intvector *v);
/* CSRMatrix(rows, cols, nonzeros, indptr, indices, data): H2D copy into plain device memory (the
 * reference uses managed memory + ReadMostly advise, matrix.cu:222-251).  Also builds the
 * row-length bins the solver kernels schedule from (device-side metadata, not visible here). */
int imp_csr_create(int32_t rows, int32_t cols, int64_t nonzeros, const int32_t *indptr,
                   const int32_t *indices, const float *data, imp_csr **out);
/* NEW: the same with 64-bit row offsets (the CPU reference accepts both widths, _als.pyx:76; the CUDA class is int32
 * only, matrix.h:92-99).  More than 2^31 - 1 nonzeros are held as consecutive row blocks internally; indices stay
 * int32 (cols < 2^31). */
int imp_csr_create64(int32_t rows, int32_t cols, int64_t nonzeros, const int64_t *indptr,
                     const int32_t *indices, const float *data, imp_csr **out);
int imp_csr_shape(const imp_csr *m, int32_t *rows, int32_t *cols, int64_t *nonzeros);
int imp_csr_destroy(imp_csr *m);
int imp_coo_create(int32_t rows, int32_t cols, int64_t nonzeros, const int32_t *row,
                   const int32_t *col, const float *data, imp_coo **out);
/* NEW: the (row, col) pattern of a HOST CSR matrix as a device COO without values -- all the top-k filters read
 * (knn.cu:197-214 reads row / col only).  `indptr`: rows + 1 offsets, int32 or int64 (`indptr_is_64`); `indices`: int32.
 * Both are copied to page-locked staging and expanded by a kernel: no blocking upload, no host-side row expansion.
 * recommend() builds one per batch (the reference: scipy tocoo() + three Vector uploads, matrix_factorization_base.py:109-112,
 * matrix.cu:253-262). */
int imp_coo_create_from_csr_pattern(int32_t rows, int32_t cols, const void *indptr, int indptr_is_64,
                                    const int32_t *indices, imp_coo **out);
int imp_coo_destroy(imp_coo *m);

/* ---- LeastSquaresSolver (als.h:11-24, als.cu:118-281) ---------------------------------------- */
int imp_solver_create(imp_solver **out);
int imp_solver_destroy(imp_solver *s);
/* calculate_yty(Y, &YtY, regularization): YtY(f x f fp32) = Y^T Y + reg*I  (als.cu:122-152).
 * MFMA (v_mfma_f32_32x32x2_f32) split over row blocks with a fixed-order second stage. */
int imp_solver_calculate_yty(imp_solver *s, const imp_matrix *Y, imp_matrix *YtY, float regularization);
/* least_squares(Cui, &X, YtY, Y, cg_steps): warm-started CG half sweep, X in place; YtY is the
 * regularised gramian (als.cu:154-197; numerics follow the CPU oracle _als.pyx:152-248). */
int imp_solver_least_squares(imp_solver *s, const imp_csr *cui, imp_matrix *X, const imp_matrix *YtY,
                             const imp_matrix *Y, int cg_steps);
/* NEW (the reference GPU path has no Cholesky solver; mirrors the CPU _als._least_squares,
 * _als.pyx:75-142): YtY is UNregularised, `regularization` (double) is added to the diagonal,
 * the previous X is ignored.  On a non-positive-definite row returns IMP_INVALID_ARGUMENT
 * (ValueError, as _als.pyx:136-138) and *failed_row = that row (else -1). */
int imp_solver_least_squares_cholesky(imp_solver *s, const imp_csr *cui, imp_matrix *X,
                                      const imp_matrix *YtY, const imp_matrix *Y,
                                      double regularization, int64_t *failed_row);
/* NEW (no reference counterpart): the block-subspace half sweep of iALS++ (Rendle, Krichene, Zhang, Koren 2021) for large
 * factor counts.  fp32 X and Y, f <= 1024, 1 <= block_size <= 32, sweeps >= 1; YtY is UNregularised.  With w_j = |c_j| - 1 and
 * c+_j = max(c_j, 0) a row's system is A x = b, A = YtY + regularization I + sum_j w_j y_j y_j^T, b = sum_j c+_j y_j, as in
 * imp_solver_least_squares_cholesky.  A sweep starts from the stored x (warm start): p_j = x . y_j for every stored entry; then
 * for the blocks S = [0, k), [k, 2k), ... in order (k = block_size, the last one possibly shorter)
 *   g = (YtY x)_S + regularization x_S + sum_j (w_j p_j - c+_j) y_j[S],  H = YtY_SS + regularization I + sum_j w_j y_j[S] y_j[S]^T,
 *   delta = -H^-1 g by Cholesky,  x_S += delta,  p_j += delta . y_j[S];
 * sweeps > 1 repeats the block loop without recomputing p.  block_size >= f is the exact solve.  Empty rows become zero.  A
 * non-positive pivot in any block of any row returns IMP_INVALID_ARGUMENT with *failed_row = the smallest such row (else -1);
 * the other rows are solved, a failing row's contents are unspecified.  No floating-point atomics: equal inputs give bitwise
 * equal outputs.  Argument errors are reported before any launch.  Waits for its result also in deferred-sync mode, as
 * imp_solver_least_squares_cholesky does. */
int imp_solver_least_squares_subspace(imp_solver *s, const imp_csr *cui, imp_matrix *X, const imp_matrix *YtY,
                                      const imp_matrix *Y, double regularization, int block_size, int sweeps,
                                      int64_t *failed_row);
/* calculate_loss(Cui, X, Y, regularization) (als.cu:253-281; oracle _als.pyx:257-308). */
int imp_solver_calculate_loss(imp_solver *s, const imp_csr *cui, const imp_matrix *X,
                              const imp_matrix *Y, float regularization, float *loss_out);
/* NEW: explanations of ALS recommendations (the reference explains on the CPU only, implicit/cpu/als.py explain).  For every
 * row u of cui (alpha already applied) explain_factor builds A_u = YtY + regularization I + sum_j (|c_j| - 1) y_j y_j^T --
 * YtY is UNregularised, the matrix of the Cholesky half sweep -- and writes its Cholesky factor L, lower triangular with zeros
 * above the diagonal, into rows [u f, (u + 1) f) of `weights`: caller-allocated fp32, (cui.rows * f) x f.  f <= 256; Y fp32.
 * On a non-positive pivot returns IMP_INVALID_ARGUMENT and *failed_row = the smallest failing row (else -1), as
 * imp_solver_least_squares_cholesky. */
int imp_solver_explain_factor(imp_solver *s, const imp_csr *cui, const imp_matrix *YtY, const imp_matrix *Y,
                              double regularization, imp_matrix *weights, int64_t *failed_row);
/* NEW: for row u and each of its items_per_row ids i = itemids[u * items_per_row + m]: w = A_u^-1 y_i by two triangular solves
 * with the row's L from `weights`; liked item j (c_j > 0) contributes s_j = c_j (w . y_j).  Outputs are HOST buffers:
 * total[rows * items_per_row] = sum_j s_j, and ids / scores[rows * items_per_row * n], the n largest contributions under
 * (score descending, id descending), padded with (-1, -FLT_MAX).  Deterministic: no floating-point atomics.  Ids outside Y,
 * n < 1, items_per_row < 1 and a weights matrix that is not fp32 (cui.rows * f) x f are IMP_INVALID_ARGUMENT before any
 * launch. */
int imp_solver_explain(imp_solver *s, const imp_csr *cui, const imp_matrix *Y, const imp_matrix *weights,
                       const imp_intvector *itemids, int items_per_row, int n, float *total, int32_t *ids, float *scores);

/* ---- KnnQuery (knn.h:15-35, knn.cu:56-265) ---------------------------------------------------- */
/* KnnQuery(max_temp_memory): 0 = min(free/2, 4 GiB) (knn.cu:56-75). */
int imp_knn_create(size_t max_temp_memory, imp_knn **out);
int imp_knn_destroy(imp_knn *k);
/* topk(items, query, k, indices, distances, item_norms, query_filter, item_filter) (knn.cu:77-265).
 * indices/distances are caller-allocated [query.rows x k] HOST or DEVICE buffers (auto-detected,
 * knn.cu:40-54,147-164).  Rows are written best-first in the total order (score desc, column
 * desc); when k > items.rows only the first items.rows entries of each row are written
 * (knn.cu:239).  Filtered entries score -FLT_MAX (topk.pyx:51). */
int imp_knn_topk(imp_knn *k, const imp_matrix *items, const imp_matrix *query, int topk,
                 int32_t *indices, float *distances, const imp_matrix *item_norms,
                 const imp_coo *query_filter, const imp_intvector *item_filter);
/* NEW: scores, and for n >= 1 ranks, a candidate list per query row (csrc/rank.hip).  items (n_items x w) and query (rows x w): fp32
 * or fp16 in any pairing, any w >= 1.  HOST inputs: offsets[rows + 1] and candidates[offsets[rows]], row r being scored against
 * the items candidates[offsets[r] .. offsets[r + 1]); optionally the liked pattern as CSR, one row per query, columns strictly
 * increasing inside a row (both pointers NULL: no filter).  A score is the dot product over the w stored columns, fp16 widened
 * exactly, products and sums fp32 in an order that depends on w alone: the same (query row, item row) bits give the same
 * score bits whatever the list, row, chunk or mode.  A candidate stored in the query's liked row scores -FLT_MAX and takes part
 * like any other.  HOST outputs: n == 0: scores[offsets[rows]] in the candidates' own order, `indices` is not touched; n >= 1:
 * indices / scores[rows x n], each row the best min(n, length) candidates of its list, best first in the total order (score
 * desc, id desc, -0.0 as +0.0), the tail id -1, score -FLT_MAX; an id repeated in a list is scored and returned as often.  Rows
 * are processed in chunks that fit the handle's max_temp_memory; the chunking changes no result.  Deterministic: no
 * floating-point atomics.  IMP_INVALID_ARGUMENT before any launch, nothing written: column counts that differ, a matrix neither
 * fp32 nor fp16, offsets that do not start at 0 or that decrease, a candidate id outside [0, n_items), a liked row not strictly
 * increasing, n < 0, a list of more than 4096 candidates with n > 1024, a single row whose temporaries exceed max_temp_memory
 * (the message names the bytes). */
int imp_knn_rank(imp_knn *k, const imp_matrix *items, const imp_matrix *query, const int64_t *offsets,
                 const int32_t *candidates, int n, const int64_t *liked_indptr, const int32_t *liked_indices,
                 int32_t *indices, float *scores);

/* ---- RandomState (random.h:10-21, random.cu:14-40) ------------------------------------------- */
int imp_random_create(int64_t seed, imp_random **out);
int imp_random_destroy(imp_random *r);
int imp_random_uniform(imp_random *r, size_t rows, size_t cols, float low, float high, imp_matrix **out);
int imp_random_randn(imp_random *r, size_t rows, size_t cols, float mean, float stddev, imp_matrix **out);

/* ---- BPR training (bpr.h:8-13, bpr.cu:72-125) ------------------------------------------------------ */
/* One SGD pass of Bayesian Personalized Ranking over `samples` sampled (user, liked, disliked) triples (samples < 0: nnz, one
 * epoch).  userids / itemids: the COO row / column ids of the training matrix (nnz each); indptr: its CSR row pointer
 * (X.rows + 1 entries; row indices sorted when verify_negative is set).  X (users x C), Y (items x C), fp32, C = factors + 1
 * in 2 .. 1024, column C-1 the item bias (users hold 1.0 there; X[:, C-1] is never written).  The update is the reference's
 * CPU one (implicit/cpu/bpr.pyx:249-302), the sample pairs a counter-based Philox stream of (seed, sample index, nnz):
 * bpr.hip states both.  *correct: samples with z < 0.5; *skipped: samples whose negative the user had liked.  Synchronous,
 * deferred mode included.  Every id is checked on the device before the update runs: IMP_OUT_OF_RANGE (IndexError), with
 * X and Y untouched, for a user id outside X, an item id outside Y or an indptr entry outside [0, nnz].
 * IMP_INVALID_ARGUMENT: column counts differ or outside 2 .. 1024, a matrix not fp32, userids / itemids of different sizes,
 * indptr not X.rows + 1 long.  nnz = 0 returns (0, 0) without a launch. */
int imp_bpr_update(const imp_intvector *userids, const imp_intvector *itemids, const imp_intvector *indptr, imp_matrix *X,
                   imp_matrix *Y, float learning_rate, float regularization, int64_t seed, int verify_negative, int64_t samples,
                   int64_t *correct, int64_t *skipped);

/* ---- WARP training (no reference counterpart: Weston et al., "WSABIE") ------------------------------------------------- */
/* One SGD pass of WARP-loss matrix factorization over `samples` sampled positives (samples < 0: nnz, one epoch).  userids,
 * itemids, indptr, X, Y: as imp_bpr_update, row indices sorted.  Each positive (u, i) meets up to max_sampled (1 .. 4096)
 * uniformly drawn items j; a draw the user has liked is consumed without effect; the first j with X[u].Y[j] > X[u].Y[i] - 1
 * ends the sample with an SGD step weighted by min(10, log(max(1, (items - 1) / trials used))).  The positives and the
 * candidates are counter-based Philox streams of (seed, sample index): warp.hip states the contract in full.  *satisfied:
 * samples without a violating draw (nothing written for them); *trials: draws consumed over all samples.  Synchronous,
 * deferred mode included.  Ids are checked on the device first: IMP_OUT_OF_RANGE (IndexError), X and Y untouched, as
 * imp_bpr_update.  IMP_INVALID_ARGUMENT: column counts differ or outside 2 .. 1024, a matrix not fp32, max_sampled outside
 * 1 .. 4096, userids / itemids of different sizes, indptr not X.rows + 1 long.  nnz = 0 returns (0, 0) without a launch. */
int imp_warp_update(const imp_intvector *userids, const imp_intvector *itemids, const imp_intvector *indptr, imp_matrix *X,
                    imp_matrix *Y, float learning_rate, float regularization, int64_t seed, int max_sampled, int64_t samples,
                    int64_t *satisfied, int64_t *trials);

/* ---- LMF training (no reference GPU counterpart: implicit/lmf.py raises for use_gpu=True) --------------------------- */
/* One Adagrad half-sweep of Logistic Matrix Factorization: X (rows of cui x C) is updated against the read-only Y (columns
 * of cui x C), deriv_sum_sq (shape of X) accumulates the squared gradients.  fp32, C = factors + 2 in 3 .. 1024.  The
 * update is the reference's CPU one (implicit/cpu/lmf.pyx lmf_update), including its cap of K = min(C, n * neg_prop)
 * negatives per row of n nonzeros; the negatives are a counter-based Philox stream of (seed, row, k): lmf.hip states both.
 * Rows without a nonzero are not touched; afterwards column one_col of X is 1.0 in every row (-1: no column).  The result
 * is deterministic (bitwise equal for equal inputs).  Synchronous, deferred mode included.  nnz = 0 only sets one_col.
 * IMP_INVALID_ARGUMENT, with X and deriv_sum_sq untouched: X.rows != cui rows, Y.rows != cui columns, column counts or
 * deriv_sum_sq's shape disagree, a matrix not fp32, C outside 3 .. 1024, neg_prop < 0, one_col outside [-1, C), X, Y and
 * deriv_sum_sq sharing storage, or a CSR held in several blocks (more than 2^31 - 1 nonzeros; not supported). */
int imp_lmf_update(const imp_csr *cui, imp_matrix *X, const imp_matrix *Y, imp_matrix *deriv_sum_sq, float learning_rate,
                   float regularization, int neg_prop, int64_t seed, int one_col);

/* ---- item-item nearest neighbours (reference: the CPU all_pairs_knn / NearestNeighboursScorer, _nearest_neighbours.pyx) -- */
typedef struct imp_spmat imp_spmat; /* fp64-valued CSR, device-resident: int64 offsets, int32 column ids */
/* Copies a host CSR to the device.  IMP_INVALID_ARGUMENT: negative sizes, more than 2^31 - 1 nonzeros, indptr not running
 * from 0 to nnz or decreasing, a column id outside [0, cols). */
int imp_spmat_create(int32_t rows, int32_t cols, int64_t nnz, const int64_t *indptr, const int32_t *indices,
                     const double *data, imp_spmat **out);
int imp_spmat_destroy(imp_spmat *m);
/* Row r of A.B over its TOUCHED columns (reached by at least one pair A[r,u] B[u,j], a 0.0 sum included), fp64, each
 * column's sum in A[r]'s stored order as the reference's SparseMatrixMultiplier takes it (knn.hip states the contract).
 * zero_own_columns: every touched column that is also a column of A[r] gets 0.0 and stays a candidate (remove_own_likes).
 * ids / scores: rows(A) x k on the host, each row the k best under (score, id) descending; counts[r] = min(k, touched);
 * entries past counts[r] hold id -1 and score -inf.  Deterministic; exact for any k.  Synchronous.
 * IMP_INVALID_ARGUMENT, nothing written: A.cols != B.rows, k < 1, more than 2^31 - 1 nonzeros, zero_own_columns with
 * A.cols != B.cols, or a column repeated within a row of B. */
int imp_sparse_topk_product(const imp_spmat *A, const imp_spmat *B, int k, int zero_own_columns, int32_t *ids,
                            double *scores, int32_t *counts);

/* ---- NEW: ranking metrics of recommendation rows (reference: the host loop of implicit/evaluation.pyx:366-475) ---------- */
typedef struct imp_eval imp_eval; /* held-out pattern on the device + six running sums */
/* Both entry points below take the held-out (test) matrix as a HOST CSR pattern: rows + 1 offsets starting at 0, int32 or
 * int64 (`indptr_is_64`), int32 `indices`, every row strictly increasing inside [0, cols) (sorted, no duplicates); k, the
 * length of a recommendation row; and two tables of k doubles, cg[i] = 1 / log2(i + 2) and its running sum (the caller
 * computes them, the library never evaluates a logarithm).  IMP_INVALID_ARGUMENT: a row not strictly increasing, an index
 * outside [0, cols), k < 1, a negative dimension, offsets that decrease or do not start at 0.
 * The six sums, in this order: relevant (hits), pr_div (sum of min(k, likes)), sum_ap, sum_ndcg, sum_auc, total (rows
 * counted); precision = relevant / pr_div, map / ndcg / auc = sum / total (evaluation.pyx:470-475).  Per row
 * (csrc/eval_metrics.h): an id that is negative or >= cols is a miss; a row whose user has nothing held out adds nothing
 * and is not counted. */
/* Copies the pattern (64-bit offsets) and the tables to the device; the sums start at zero. */
int imp_eval_create(int32_t rows, int32_t cols, const void *indptr, int indptr_is_64, const int32_t *indices, int k,
                    const double *cg, const double *cg_sum, imp_eval **out);
/* ids: n x k matrix of itemsize 4 holding int32 bit patterns (what imp_knn_topk writes into a device buffer); userids: the
 * n rows of the pattern they were recommended for, any order, repeats allowed.  A user id outside [0, rows) is skipped
 * like a user with nothing held out (never indexed with).  Queues two kernels on the library stream and returns without a
 * host wait, unless per_row is given: a HOST array of n * 4 doubles that receives every row's hits and its ap, ndcg and
 * auc terms (zeros for a skipped row).  No floating-point atomics: the same calls on the same data give the same bits. */
int imp_eval_add(imp_eval *e, const imp_matrix *ids, const imp_intvector *userids, double *per_row);
/* Waits for the library stream and reads the six sums. */
int imp_eval_result(imp_eval *e, double *out);
int imp_eval_reset(imp_eval *e);
int imp_eval_destroy(imp_eval *e);
/* Host code, no device involved: the same sums (written to sums[6], added up in row order) and per-row output for n rows
 * of HOST ids (n x k int32) through the same per-row function.  IMP_OUT_OF_RANGE: a user id outside [0, rows). */
int imp_host_ranking_metrics(int32_t rows, int32_t cols, const void *indptr, int indptr_is_64, const int32_t *indices, int k,
                             const double *cg, const double *cg_sum, const int32_t *ids, const int32_t *userids, int64_t n,
                             double *sums, double *per_row);

/* ---- NEW: IVF-Flat approximate nearest neighbours (reference: the faiss.GpuIndexIVFFlat the wrappers of implicit/ann/faiss.py
 * build; here a native index, csrc/ivf.hip) ------------------------------------------------------------------------------- */
typedef struct imp_ivf imp_ivf; /* centroids + inverted lists of fp32 vectors, device-resident */
/* Builds the index over the rows of `vectors` (fp32 or fp16, widened; 1 .. 1024 columns) on the device: the centroids start
 * as the unit-normalised rows init_rows[0 .. nlist) (a zero row stays zero); `iterations` rounds of spherical k-means follow
 * -- every vector goes to the centroid of largest inner product, ties to the larger list id; every centroid becomes the
 * normalised mean of its list, summed in ascending vector id, an empty list or a zero mean keeping the old centroid -- and
 * the lists are rebuilt against the final centroids.  Deterministic.  IMP_INVALID_ARGUMENT: nlist outside 1 .. rows,
 * iterations < 0, a column count outside 1 .. 1024; IMP_OUT_OF_RANGE: an initial row id outside the matrix. */
int imp_ivf_build(const imp_matrix *vectors, int nlist, int iterations, const int32_t *init_rows, imp_ivf **out);
int imp_ivf_shape(const imp_ivf *ix, size_t *rows, size_t *cols, int *nlist);
/* Bytes of temporaries one chunk of queries of a search may take; 0 restores the default min(free / 2, 4 GiB) of KnnQuery.
 * The index keeps the temporaries of its last search for the next one; this call frees them. */
int imp_ivf_set_temp_memory(imp_ivf *ix, size_t max_temp_memory);
/* HOST outputs, each nullable: centroids[nlist x cols], list_offsets[nlist + 1], list_ids[rows] (list l holds the vectors
 * list_ids[list_offsets[l] .. list_offsets[l + 1]), ascending). */
int imp_ivf_lists(const imp_ivf *ix, float *centroids, int64_t *list_offsets, int32_t *list_ids);
/* The k best vectors of each query (fp32 or fp16, the index's column count) among the P = min(nprobe, nlist) lists whose
 * centroids have the largest inner product with it.  indices / distances: [query.rows x k], host or device, best first in the
 * total order (score desc, id desc), scores exact fp32 fmaf chains over the columns in order; where the probed lists hold
 * fewer than k vectors the tail is id -1, score -FLT_MAX.  probes (nullable): [query.rows x P], the probed lists, best first
 * (score desc, list id desc).  Queries are processed in chunks that fit the temporary budget; the chunking changes no
 * result.  IMP_INVALID_ARGUMENT: k outside 1 .. 1024, nprobe < 1, P > 1024, a column count that differs. */
int imp_ivf_search(imp_ivf *ix, const imp_matrix *query, int k, int nprobe, int32_t *indices, float *distances, int32_t *probes);
int imp_ivf_destroy(imp_ivf *ix);

/* ---- NEW: EASE, the closed-form item-item model B = I - P diag(P)^-1, P = (X^T X + reg I)^-1 (Steck 2019; no reference
 * counterpart; csrc/ease.hip, csrc/spd_inverse.hip).  No floating-point atomics anywhere: equal inputs give
 * bitwise equal outputs.  All four calls are synchronous. ---------------------------------------------------------------- */
/* G (caller-allocated fp32, items x items) = X^T X + regularization I from BOTH orientations of the same matrix: item_users
 * (items x users) and user_items (users x items, no column repeated within a row).  G[i][j], j <= i, is the fp32 sum of the
 * separately rounded products x_ui x_uj over the co-occurring users u in item_users[i]'s stored order, the diagonal plus
 * regularization last; j > i is a copy, so G is exactly symmetric.  Exact when the values are integers and every partial sum
 * stays below 2^24; otherwise |G[i][j] - exact| <= (c_ij + 1) 2^-24 sum_u |x_ui x_uj| with c_ij co-occurring users.
 * IMP_INVALID_ARGUMENT before any launch: shapes or nonzero counts that do not agree, more than 2^31 - 1 nonzeros, a G that
 * is not fp32 items x items. */
int imp_ease_gram(const imp_csr *item_users, const imp_csr *user_items, float regularization, imp_matrix *G);
/* In-place inverse of a symmetric positive definite fp32 n x n matrix by a blocked Cholesky inverse on the fp32 matrix
 * instruction.  Only the lower triangle of A is read; the full, exactly symmetric inverse is written.  On a pivot that is not
 * positive (or NaN) returns IMP_INVALID_ARGUMENT with *failed_pivot = the smallest failing index (else -1), the rule of
 * imp_solver_least_squares_cholesky; A is then unspecified.  Workspace: one more n x n fp32 matrix plus n nb floats (nb =
 * 128, n rounded up to it); IMP_RUNTIME_ERROR with a message naming the bytes when it cannot be allocated.  IMP_INVALID_ARGUMENT before any
 * launch: a matrix that is not square fp32. */
int imp_spd_inverse(imp_matrix *A, int64_t *failed_pivot);
/* In place on a square fp32 matrix: B[i][j] = -(P[i][j] / P[j][j]) for i != j, one IEEE fp32 division and a sign flip;
 * B[j][j] = 0.  IMP_INVALID_ARGUMENT with P untouched: a diagonal entry that is zero or not finite, a matrix that is not
 * square fp32. */
int imp_ease_weights(imp_matrix *P);
/* The topk best columns of x B for every row x of a HOST CSR matrix (rows + 1 int64 offsets from 0, int32 columns strictly
 * increasing inside a row and inside [0, items), fp32 values); B: fp32 items x items on the device.  The score of column j
 * for a row with stored entries (i_1, x_1), (i_2, x_2), ... is ((0 + x_1 B[i_1][j]) + x_2 B[i_2][j]) + ..., every product and
 * sum a separately rounded fp32 operation in stored order; an empty row scores 0 everywhere.  filter_liked: the row's own
 * columns score -FLT_MAX and stay candidates (the rule of imp_knn_topk); the ids of item_filter (nullable) likewise.  HOST
 * outputs ids / scores[rows x topk], best first in the total order (score desc, id desc, -0.0 as +0.0); the tail past
 * min(topk, items) is id -1, score -FLT_MAX.  Rows are processed in chunks that fit the handle's max_temp_memory; the
 * chunking changes no result.  IMP_INVALID_ARGUMENT before any launch, nothing written: topk outside 1 .. 1024, a B that is
 * not square fp32, negative rows, offsets that do not start at 0 or that decrease, a column outside the model, a row not
 * strictly increasing, an item_filter id outside the model, a single row whose temporaries exceed max_temp_memory. */
int imp_ease_topk(imp_knn *k, const imp_matrix *B, int32_t rows, const int64_t *indptr, const int32_t *indices,
                  const float *data, int topk, int filter_liked, const imp_intvector *item_filter, int32_t *ids,
                  float *scores);

/* ---- NEW: SLIM, the elastic-net item-item model (Ning & Karypis, ICDM 2011; no reference counterpart; csrc/slim.hip,
 * DESIGN 4.20): `items` independent problems in Gram form, solved by cyclic coordinate descent.  No floating-point atomics:
 * equal inputs give bitwise equal outputs, whatever ran before.  The call is synchronous. ------------------------------------ */
#define IMP_SLIM_MAX_ITEMS 40000 /* one workgroup keeps a column's running product (items floats) in its 160 KiB of LDS */
/* A: fp32 items x items, symmetric, what imp_ease_gram(.., regularization = l2) returns.  W (caller-allocated fp32, items x
 * items; its contents on entry do not matter): W[i][j] = the weight of source item i for target j, the layout of EASE's B, so
 * imp_ease_topk serves it; W[j][j] = +0.  Column j minimises  1/2 w^T A w - sum_i A[j][i] w_i + l1 sum_i |w_i|  subject to
 * w_j = 0 (and w >= 0 when `positive`), by this rule, every operation a separately rounded fp32 operation:
 *   w = 0, r = 0 (items floats each); for sweep s = 1 .. max_sweeps:
 *     dmax = 0; for i = 0 .. items - 1 ascending, i != j:
 *       a = A[i][i];  rho = (A[j][i] - r[i]) + a w[i]
 *       positive:  t = rho - l1;  new = t > 0 ? t / a : +0
 *       otherwise: new = rho > l1 ? (rho - l1) / a : rho < -l1 ? (rho + l1) / a : +0
 *       d = new - w[i];  if d != 0:  w[i] = new;  r[k] = r[k] + d A[i][k] for every k;  dmax = max(dmax, |d|)
 *     wmax = max_k |w[k]|;  the column stops when dmax <= tol wmax (a sweep that changed nothing stops it whatever tol is)
 *   sweeps[j] (HOST, items entries, nullable) = the number of sweeps column j ran.
 * r is never recomputed from w: its rounding accumulates, so tol = 0 means "exactly max_sweeps sweeps unless a sweep changes
 * nothing" (DESIGN 4.20).  Workspace: 3 items + 8 four-byte words, kept for the next call (imp_release_workspaces).
 * IMP_INVALID_ARGUMENT with W untouched: a NULL A or W, matrices that are not square fp32 of one order, A and W sharing
 * storage, l1 or tol negative or not finite, max_sweeps < 1, items > IMP_SLIM_MAX_ITEMS (the call is refused, not routed to a
 * slower kernel), a diagonal entry of A that is not finite or not > 0 (checked by a kernel before anything is written; the
 * message names the smallest such item).  items = 0 succeeds and does nothing. */
int imp_slim_solve(const imp_matrix *A, float l1, int positive, int max_sweeps, float tol, imp_matrix *W, int32_t *sweeps);
/* Measurement aid for profiles/slim_bench.py, NOT part of the model's contract (like imp_debug_occupy and imp_debug_core_clock:
 * no model or shim path depends on it, and it may change with the kernel): what the last imp_slim_solve on this device
 * counted -- the updates it applied (coordinates with d != 0, all columns) and the longest time one column held its
 * workgroup, in seconds. */
int imp_slim_stats(unsigned long long *updates, double *longest_column_seconds);

/* ---- NEW: the two products of the randomized truncated SVD behind PureSVD (Cremonesi, Koren, Turrin 2010; Halko,
 * Martinsson, Tropp 2011; no reference counterpart; csrc/svd.hip).  No floating-point atomics: equal inputs give
 * bitwise equal outputs.  Both calls are synchronous and read no row schedule but A's. --------------------------------------- */
/* out (caller-allocated fp32, rows x l) = A D for a CSR matrix A (rows x cols, fp32 values) and a dense fp32 D (cols x l),
 * 1 <= l <= 1024.  For a row of at most 1024 stored entries (j_1, a_1), (j_2, a_2), ... out[r][c] is
 * ((0 + a_1 D[j_1][c]) + a_2 D[j_2][c]) + ..., every product and every sum a separately rounded fp32 operation in stored
 * order.  A longer row is cut into runs of 1024 stored entries; each run is summed that way from 0 and the runs' sums are then
 * added in order, starting from the first run's.  An empty row gives zeros.  Exact when the values are integers and every
 * partial sum stays below 2^24.  IMP_INVALID_ARGUMENT before any launch, out untouched: an operand that is not fp32, shapes
 * that do not agree, l outside 1 .. 1024, more than 2^31 - 1 nonzeros, an out whose memory overlaps D's. */
int imp_csr_spmm(const imp_csr *A, const imp_matrix *D, imp_matrix *out);
/* out (caller-allocated fp32, rows x m) = Y W for a tall fp32 Y (rows x l) and a small fp32 W (l x m), 1 <= l, m <= 1024, on
 * the fp32 matrix instruction: exact fp32 products, summed over the l terms in a fixed order.  |out - exact| <= (l + 1) 2^-24
 * sum_i |y_i w_ij| per entry; exact when the values are integers and every partial sum stays below 2^24.  rows = 0 is a no-op.
 * IMP_INVALID_ARGUMENT before any launch, out untouched: an operand that is not fp32, shapes that do not agree, l or m outside
 * 1 .. 1024, an out whose memory overlaps Y's or W's. */
int imp_matrix_multiply_small(const imp_matrix *Y, const imp_matrix *W, imp_matrix *out);

/* ---- NEW: multi-GPU exchange over RCCL / xGMI (no reference counterpart) ------------------------ */
/* One process per GPU.  Rank 0 calls imp_comm_unique_id, the host side broadcasts the 128 bytes by
 * any means (torch.distributed store, MPI, a file) and every rank calls imp_comm_init_rank. */
#define IMP_COMM_UNIQUE_ID_BYTES 128
int imp_comm_unique_id(void *id_out);
int imp_comm_init_rank(const void *id, int nranks, int rank, imp_comm **out);
int imp_comm_destroy(imp_comm *c);
/* in-place sum all-reduce of an fp32 matrix (the f x f gramian). */
int imp_comm_allreduce_sum(imp_comm *c, imp_matrix *m);
/* all-gather of row shards: rank r contributes rows [row_offsets[r], row_offsets[r+1]) of `full`
 * (already in place in its own copy); afterwards every rank holds all rows. */
int imp_comm_allgather_rows(imp_comm *c, imp_matrix *full, const int64_t *row_offsets);
/* Pipelined form of the all-gather: rows [row_lo[r], row_hi[r]) are owned by rank r (nranks entries each).  _begin
 * queues the exchange on a second stream behind the work already queued on the library stream and returns; _end makes
 * the library stream wait for all exchanges queued since (no host wait).  A half sweep solved in K row chunks calls
 * _begin after each chunk and _end once, so chunk k travels over xGMI while chunk k+1 is being solved. */
int imp_comm_allgather_rows_begin(imp_comm *c, imp_matrix *full, const int64_t *row_lo, const int64_t *row_hi);
int imp_comm_allgather_rows_end(imp_comm *c);
/* Personalised exchange of row ranges (set-up of a sharded fit: pieces of the transposed shard).  Rows
 * [send_lo[p], send_hi[p]) of `send` go to rank p, where they arrive as rows [recv_lo[q], recv_hi[q]) of `recv` (q = the
 * sender); the two matrices must have rows of the same byte size, bytes travel untouched.  Synchronous. */
int imp_comm_alltoall_rows(imp_comm *c, const imp_matrix *send, const int64_t *send_lo, const int64_t *send_hi,
                           imp_matrix *recv, const int64_t *recv_lo, const int64_t *recv_hi);
int imp_comm_barrier(imp_comm *c);
/* out[0], out[1]: the number of ranks a one-per-rank sum all-reduce counts on the communicator of the library stream and on the
 * second communicator the pipelined exchange (allgather_rows_begin) runs on -- RCCL serialises the operations of one
 * communicator, so the gramian all-reduce and the row exchange never share one.  The benchmark driver asserts both == N. */
int imp_comm_ranks_seen(imp_comm *c, int *out);

/* ---- NEW: measurement hooks (bench.py's roofline leg) -------------------------------------------- */
/* When enabled every kernel launch is bracketed by HIP events on the library stream; totals are
 * accumulated per kernel name.  imp_prof_get returns 0 launches for unknown names. */
int imp_prof_enable(int on);
/* Restrict the event pairs to kernels whose name contains `substr` (NULL or "" = every kernel): an event pair costs a few
 * microseconds of stream time, so a timed region that only needs one kernel family should not pay for all of them. */
int imp_prof_filter(const char *substr);
int imp_prof_reset(void);
int imp_prof_get(const char *kernel, double *total_ms, int64_t *launches);
/* '\n'-separated list of kernel names seen so far, copied into buf (truncated to buflen). */
int imp_prof_names(char *buf, size_t buflen);

#ifdef __cplusplus
}
#endif
#endif /* IMPLICIT_HIP_H_ */
