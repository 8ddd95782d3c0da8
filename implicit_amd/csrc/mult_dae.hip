// K25: Mult-DAE -- the multinomial denoising autoencoder of Liang, Krishnan, Hoffman and Jebara, "Variational Autoencoders
// for Collaborative Filtering" (WWW 2018), one hidden layer: imp_dae_encode, imp_dae_gradients, imp_dae_step.
//
// No reference counterpart.  All parameters are float32:  W_in [items x H],  b_in [1 x H],  W_out [items x (H + 1)] with the
// output bias as its last column (the family's bias-last layout, so the serving kernels read it as an item-factor matrix).
// H is a multiple of 32 in 32 .. 512.  user_items is a CSR pattern (values are ignored: the rows are patterns) with
// cols = items, held in one block (nnz < 2^31), every row's indices strictly ascending (scipy's canonical form).  A batch is
// B row ids, B a multiple of 64; an id of -1 is an empty row (the padding of an epoch's last batch).
//   forward, for row u of the batch with n_u stored entries at the CSR positions pos = indptr[u] .. indptr[u + 1] - 1:
//     m_pos = 1 when dropout p = 0; otherwise R = Philox4x32-10(counter (pos, 0, 0, 7), key (seed_lo, seed_hi)) (philox.h) and
//             m_pos = 1 when float(R.x >> 8) * 2^-24 >= p (p as float32), else 0 -- a Bernoulli(1 - p) keep mask;
//     s_u   = 1 / ((1 - p) * sqrt(n_u)) in float32 as written, and the weight of entry pos is m_pos * s_u;
//     z_u   = b_in + sum over the row's kept entries, in stored order, of s_u * W_in[i_pos]   (multiply, then add);
//     h_u   = tanh(z_u);   logit_uj = W_out[j, :H] . h_u + W_out[j, H], the dot product one fp32 chain in ascending k;
//     loss  = (1 / B) sum_u (n_u * lse_u - sum_{i in row u} logit_ui),  lse_u = log sum_j exp(logit_uj) (the undropped row is
//             the target).  A row with n_u = 0 contributes nothing and divides nothing.
//   backward:  g_uj = (n_u * exp(logit_uj - lse_u) - x_uj) / B;   dW_out[j, :H] = sum_u g_uj h_u;   dW_out[j, H] = sum_u g_uj;
//     dh_u = sum_j g_uj W_out[j, :H];   dz = dh * (1 - h^2);   db_in = sum_u dz_u;   dW_in[i] = sum_u m_ui s_u dz_u.
//   Adam (imp_dae_step), densely over every parameter:  grad = gradient + reg * parameter for W_in and W_out[:, :H] (not for
//     the biases);  m = b1 m + (1 - b1) grad;  v = b2 v + (1 - b2) grad^2;  parameter -= lr * (m * c1) / (sqrt(v * c2) + eps)
//     with c1 = 1 / (1 - b1^t), c2 = 1 / (1 - b2^t) formed on the host in double for the step count t >= 1.
//
// Kernels (256 threads = 4 wavefronts each):
//   encode    one workgroup per batch row: 256 entries at a time are staged in the LDS with their weight (the Philox draw of
//             each position is made once, by one thread), then every thread adds the kept rows of W_in into its one or two
//             columns.  It writes h (B x H), and for training the transpose hT (H x B) as well.
//   decode    the B x items logit matrix is never stored.  Item tiles of 64 are owned by persistent workgroups (grid =
//             min(tiles, CUs), workgroup w owns tiles w, w + grid, ...).  The owner loads the tile's 64 rows of W_out into the
//             LDS once and then walks the batch in row blocks of 64.  Per row block every wavefront forms one 32 x 32 logit
//             tile with v_mfma_f32_32x32x2_f32, K = H: the A operand (32 batch rows of one k) straight from hT, 128 contiguous
//             bytes per half-wavefront, the B operand from the W tile.  The 64 x 64 logits go to the LDS plane G.
//             pass 1: four threads per row reduce G to (max, sum exp(. - max), sum of the row's liked logits in the tile)
//                     and write the triple to stats[tile][row].  merge: one wavefront per row folds the tiles' triples, lane l
//                     the tiles l, l + 64, ... in ascending order, then the 64 lanes by an xor butterfly -- a fixed order.
//             pass 2: forms the same tile again from the same operands in the same k order (one function, logit_tile), turns G
//                     into g (the liked entries of the CSR row that fall into the tile, found by a binary search of the
//                     sorted row, take their -1/B), adds the column sums to the bias gradient, and feeds both products
//                     while W and g are in the LDS:  g^T h into up to eight 32 x 32 accumulators per wavefront that live
//                     in registers across all row blocks (B operand: rows of h straight from memory, contiguous) and are
//                     written to the tile's own rows of dW_out once;  g W (K = 64) tile by tile, added to the workgroup's own
//                     partial dh (B x H, in memory; the same thread owns the same element every time, plain loads and
//                     stores).
//   finish    dh = the workgroups' partials folded in ascending workgroup order, dz = dh (1 - h^2); db_in and the loss by one
//             thread per column / one wavefront in a fixed order.  So loss, dW_out, dh, dz and db_in are bit-reproducible
//             on one device (the grid is a function of items and the CU count).
//   scatter   one workgroup per batch row adds s_u m_ui dz_u into row i of the zeroed dW_in with agent-scope fp32 atomic
//             adds (global_atomic_add_f32: _build.py passes -munsafe-fp-atomics).  An item liked by several users of the
//             batch receives the sum, in the order the adds arrive: dW_in, and with it a step, is NOT bit-reproducible
//             where three or more users of a batch share an item.
//   adam      one elementwise kernel over the three parameter arrays and their moments.  It applies nothing when the
//             encoder found a row that is not strictly ascending (the call then returns IMP_INVALID_ARGUMENT).
// Temporaries: h, hT, dh, dz (B H each), stats (3 B tiles), the partials (B H grid), and for imp_dae_step the gradients.
//
// LDS of decode: W tile 64 x (H + 1), G 64 x 65, bias 64, row words 3 x 64: (64 H + 4480) x 4 bytes, 148 992 at H = 512.
// Both leading dimensions are odd.  The logits read W as B[k = lane >> 5][n = item = lane & 31]: 32 rows H + 1 words apart,
// 32 different banks.  g W reads W as B[k = item][n = column]: 32 consecutive words.  g^T h reads G as A[m = item = lane &
// 31][k = row]: 32 consecutive words of one row; g W reads G as A[m = row = lane & 31][k = item]: 32 rows 65 words apart, 32
// banks.  One copy of g serves both operand orders without a conflict inside a half-wavefront.
//
// Visibility: everything a later kernel reads and whose 128-byte lines two workgroups may share (hT, the rows
// of dW_out, whose H + 1 words are not a multiple of a line, the encode output, the parameters Adam writes) is written with
// agent-scope stores, dW_in with agent-scope atomic adds.  The partials are 8 KB-aligned blocks with one writer each.
//
// Every address is bounded before it is used: row ids are checked on the host, column ids by imp_csr_create, the searches
// stay inside [indptr[u], indptr[u + 1]) and an entry is applied only when it lies inside the tile.
#include "mult_dae_kernels.h"

using namespace imp;

extern "C" int imp_dae_encode(const imp_csr *user_items, const int32_t *rows, int64_t n_rows, const imp_matrix *W_in,
                              const imp_matrix *b_in, imp_matrix *out) {
  return guarded([&] {
    const std::string w("dae_encode");
    if (!user_items || !W_in || !b_in || !out) throw std::invalid_argument(w + ": NULL argument");
    const int H = hidden_of(w, user_items, W_in, b_in, nullptr);
    if (n_rows < 0 || n_rows > INT32_MAX) throw std::invalid_argument(w + ": bad row count");
    if (out->itemsize != 4 || out->rows != (size_t)n_rows || out->cols != (size_t)H + 1) throw std::invalid_argument(w + ": out must be float32, rows x (hidden + 1)");
    if (out->overlaps(W_in) || out->overlaps(b_in)) throw std::invalid_argument(w + ": out shares storage with a parameter");
    check_rows(w, user_items, rows, n_rows);
    if (n_rows == 0) return;
    float *ws = ctx().dae_ws.reserve(round64(n_rows) + 64);
    int32_t *rows_d = reinterpret_cast<int32_t *>(ws);
    int *unsorted = reinterpret_cast<int *>(ws + round64(n_rows));
    IMP_CHECK_HIP(hipMemcpyAsync(rows_d, rows, (size_t)n_rows * 4, hipMemcpyHostToDevice, stream()));
    IMP_CHECK_HIP(hipMemsetAsync(unsorted, 0, 4, stream()));
    const Batch b{user_items->indptr.data(), user_items->indices.data(), rows_d, (int)n_rows, H, user_items->cols, 0.f, 0};
    {
      IMP_PROF("dae_encode");
      dae_encode_kernel<<<(unsigned)n_rows, 256, 0, stream()>>>(b, W_in->f32(), b_in->f32(), out->mut<float>(), H + 1, nullptr, unsorted);
      IMP_CHECK_HIP(hipGetLastError());
    }
    int flag = 0;
    IMP_CHECK_HIP(hipMemcpyAsync(&flag, unsorted, 4, hipMemcpyDeviceToHost, stream()));
    sync();  // the row ids are the caller's memory
    if (flag) throw std::invalid_argument(w + ": a row of user_items is not strictly ascending (sort_indices / sum_duplicates first)");
  });
}

extern "C" int imp_dae_gradients(const imp_csr *user_items, const int32_t *rows, int64_t batch_size, const imp_matrix *W_in,
                                 const imp_matrix *b_in, const imp_matrix *W_out, float dropout, int64_t seed, imp_matrix *dW_in,
                                 imp_matrix *db_in, imp_matrix *dW_out, imp_matrix *dh, imp_matrix *dz, float *loss) {
  return guarded([&] {
    const std::string w("dae_gradients");
    if (!user_items || !W_in || !b_in || !W_out || !loss) throw std::invalid_argument(w + ": NULL argument");
    const int H = hidden_of(w, user_items, W_in, b_in, W_out);
    check_batch(w, batch_size, dropout);
    same_shape(w, dW_in, W_in, "dW_in"), same_shape(w, db_in, b_in, "db_in"), same_shape(w, dW_out, W_out, "dW_out");
    for (const imp_matrix *m : {dh, dz})
      if (!m || m->itemsize != 4 || m->rows != (size_t)batch_size || m->cols != (size_t)H) throw std::invalid_argument(w + ": dh and dz must be float32, batch_size x hidden");
    const imp_matrix *outs[] = {dW_in, db_in, dW_out, dh, dz}, *ins[] = {W_in, b_in, W_out};
    for (int i = 0; i < 5; ++i) {
      for (const imp_matrix *p : ins)
        if (outs[i]->overlaps(p)) throw std::invalid_argument(w + ": a gradient shares storage with a parameter");
      for (int j = 0; j < i; ++j)
        if (outs[i]->overlaps(outs[j])) throw std::invalid_argument(w + ": two gradients share storage");
    }
    check_rows(w, user_items, rows, batch_size);
    const Gradients g{dW_in->mut<float>(), db_in->mut<float>(), dW_out->mut<float>(), dh->mut<float>(), dz->mut<float>()};
    *loss = finish(w, queue_gradients(user_items, rows, (int)batch_size, H, W_in->f32(), b_in->f32(), W_out->f32(), dropout, (uint64_t)seed, g));
  });
}

extern "C" int imp_dae_step(const imp_csr *user_items, const int32_t *rows, int64_t batch_size, imp_matrix *W_in, imp_matrix *b_in,
                            imp_matrix *W_out, imp_matrix *m_W_in, imp_matrix *v_W_in, imp_matrix *m_b_in, imp_matrix *v_b_in,
                            imp_matrix *m_W_out, imp_matrix *v_W_out, float dropout, int64_t seed, float learning_rate, float beta1,
                            float beta2, float eps, float regularization, int64_t step, float *loss) {
  return guarded([&] {
    const std::string w("dae_step");
    if (!user_items || !W_in || !b_in || !W_out || !loss) throw std::invalid_argument(w + ": NULL argument");
    const int H = hidden_of(w, user_items, W_in, b_in, W_out);
    check_batch(w, batch_size, dropout);
    if (step < 1) throw std::invalid_argument(w + ": step counts from 1");
    if (!(beta1 >= 0.f && beta1 < 1.f && beta2 >= 0.f && beta2 < 1.f && eps > 0.f)) throw std::invalid_argument(w + ": beta1, beta2 must lie in [0, 1) and eps above 0");
    same_shape(w, m_W_in, W_in, "m_W_in"), same_shape(w, v_W_in, W_in, "v_W_in"), same_shape(w, m_b_in, b_in, "m_b_in");
    same_shape(w, v_b_in, b_in, "v_b_in"), same_shape(w, m_W_out, W_out, "m_W_out"), same_shape(w, v_W_out, W_out, "v_W_out");
    const imp_matrix *all[] = {W_in, b_in, W_out, m_W_in, v_W_in, m_b_in, v_b_in, m_W_out, v_W_out};
    for (int i = 0; i < 9; ++i)
      for (int j = 0; j < i; ++j)
        if (all[i]->overlaps(all[j])) throw std::invalid_argument(w + ": two of the parameter and moment matrices share storage");
    check_rows(w, user_items, rows, batch_size);
    const size_t n_in = W_in->rows * (size_t)H, n_out = W_out->rows * (size_t)(H + 1);
    const Queued q = queue_gradients(user_items, rows, (int)batch_size, H, W_in->f32(), b_in->f32(), W_out->f32(), dropout, (uint64_t)seed, Gradients{});
    const Gradients &g = q.g;
    {
      IMP_PROF("dae_adam");
      AdamArgs a{};
      a.seg[0] = {W_in->mut<float>(), m_W_in->mut<float>(), v_W_in->mut<float>(), g.dW_in, n_in, H, H};
      a.seg[1] = {b_in->mut<float>(), m_b_in->mut<float>(), v_b_in->mut<float>(), g.db_in, (size_t)H, H, 0};
      a.seg[2] = {W_out->mut<float>(), m_W_out->mut<float>(), v_W_out->mut<float>(), g.dW_out, n_out, H + 1, H};
      a.lr = learning_rate, a.b1 = beta1, a.b2 = beta2, a.eps = eps, a.reg = regularization;
      a.c1 = (float)(1.0 / (1.0 - std::pow((double)beta1, (double)step)));
      a.c2 = (float)(1.0 / (1.0 - std::pow((double)beta2, (double)step)));
      a.unsorted = q.unsorted;
      dae_adam_kernel<<<(unsigned)std::min<size_t>((n_out + 255) / 256, (size_t)ctx().num_cus * 8), 256, 0, stream()>>>(a);
      IMP_CHECK_HIP(hipGetLastError());
    }
    *loss = finish(w, q);
  });
}
