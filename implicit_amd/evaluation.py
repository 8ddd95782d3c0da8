"""Train / test splits and ranking metrics, at the module path of implicit/evaluation.pyx.

The reference evaluates on the host: per batch of 1000 users, model.recommend, a download of the ids and a hash-set loop
(evaluation.pyx:423-466).  Here the metric arithmetic runs on the device (implicit_amd.gpu.RankingMetrics,
csrc/evaluation.hip); for the matrix-factorisation models the recommended ids never leave it: the batch's query rows, its
liked-items filter, KnnQuery.topk_device and RankingMetrics.add are queued back to back and the sums are read once at the
end.  Names, signatures and results are the reference's; `batch_size` is new.
"""
import numpy as np
from scipy.sparse import csr_matrix

from .utils import check_random_state

# users per top-k query.  profiles/eval_bench.py: at the configs[2] shape the time is level from 4096
# users per query up to a single query (0.71 - 0.73 s; 1.00 s at the reference's 1000), so memory decides: the filter and
# the query rows of a batch of this size stay below 20 MB.
DEFAULT_BATCH_SIZE = 32768


def _masked(coo, mask):
    return csr_matrix((coo.data[mask], (coo.row[mask], coo.col[mask])), shape=coo.shape, dtype=coo.dtype)


def train_test_split(ratings, train_percentage=0.8, random_state=None):
    """Randomly splits `ratings` into (train, test) CSR matrices: every stored entry goes to train with probability
    train_percentage, else to test (evaluation.pyx:14-48).  random_state: None, an int, a numpy RandomState or Generator,
    through utils.check_random_state; an int seed gives the reference's matrices.  Held-out entries with a negative value
    are dropped from test, as there."""
    coo = ratings.tocoo()
    draw = check_random_state(random_state).random(len(coo.data))
    to_train = draw < train_percentage
    train, test = _masked(coo, to_train), _masked(coo, ~to_train)
    test.data[test.data < 0] = 0
    test.eliminate_zeros()
    return train, test


def leave_k_out_split(ratings, K=1, train_only_size=0.0, random_state=None):
    """Leave-K-out split (evaluation.pyx:141-232): every eligible user, one with more than K + 1 stored ratings, has K of
    them, picked at random, moved to test; everything else is train.  train_only_size: the fraction of the users (at least
    one when > 0) that is kept out of test altogether.  Returns (train, test) CSR matrices with train + test == ratings.

    Differs from the reference in where the randomness comes from: it shuffles with numpy's GLOBAL state (np.random.random,
    evaluation.pyx:128) and uses random_state only to pick the train-only users; here both come from random_state, so a seed
    reproduces the split.  The values of a split therefore differ from the reference's; its properties are the same."""
    K = int(K)
    if K < 1:
        raise ValueError("The 'K' must be >= 1.")
    if not 0.0 <= train_only_size < 1.0:
        raise ValueError("The 'train_only_size' must be in the range (0.0 <= x < 1.0).")
    coo = ratings.tocoo()
    rng = check_random_state(random_state)
    counts = np.bincount(coo.row, minlength=coo.shape[0])
    eligible = counts > K + 1
    if train_only_size > 0.0:
        present = np.flatnonzero(counts)
        eligible[rng.choice(present, size=max(1, int(len(present) * train_only_size)), replace=False)] = False
    # a random order inside every user's entries; the first K of an eligible user are held out
    order = np.lexsort((rng.random(len(coo.row)), coo.row))
    start = np.concatenate(([0], np.cumsum(counts)))[coo.row[order]]
    held = np.zeros(len(coo.row), dtype=bool)
    held[order] = (np.arange(len(order)) - start < K) & eligible[coo.row[order]]
    return _masked(coo, ~held), _masked(coo, held)


def _canonical_pattern(test_user_items):
    """A copy of the held-out PATTERN in canonical form: rows sorted, duplicates merged, explicit zeros kept -- the
    reference counts every stored index as a like (it inserts them into a set, evaluation.pyx:441-442)."""
    m = test_user_items
    out = csr_matrix((np.ones(len(m.indices), dtype=np.int8), m.indices.copy(), m.indptr.copy()), shape=m.shape)
    out.sum_duplicates()  # sorts, merges; drops nothing
    return out


class _progress:
    """tqdm when available and asked for, otherwise a no-op."""

    def __init__(self, total, show):
        self.bar = None
        if show:
            try:
                from tqdm.auto import tqdm

                self.bar = tqdm(total=total)
            except ImportError:
                pass

    def update(self, n):
        if self.bar is not None:
            self.bar.update(n)

    def close(self):
        if self.bar is not None:
            self.bar.close()


def ranking_metrics_at_k(model, train_user_items, test_user_items, K=10, show_progress=True, num_threads=1,
                         batch_size=DEFAULT_BATCH_SIZE):
    """{"precision", "map", "ndcg", "auc"} at K of a fitted model (evaluation.pyx:366-475): every user with a held-out
    item, in ascending order, is recommended K items with the training items filtered, and the rows are scored against
    test_user_items (every stored index is a like: explicit zeros count, duplicates count once).

    batch_size: users per query (new; the reference is fixed at 1000).  num_threads is accepted and ignored.  ValueError for
    K < 1 or K > the number of items, where the reference reads out of bounds.  Runs on the GPU only."""
    import implicit_amd.gpu as gpu
    from .gpu.matrix_factorization_base import MatrixFactorizationBase

    if not gpu.HAS_CUDA:
        raise ValueError("No usable HIP device / extension: implicit_amd.evaluation computes its metrics on the GPU")
    if not isinstance(train_user_items, csr_matrix):
        train_user_items = train_user_items.tocsr()
    if not isinstance(test_user_items, csr_matrix):
        test_user_items = test_user_items.tocsr()
    K, batch_size = int(K), int(batch_size)
    if K < 1 or K > test_user_items.shape[1]:
        raise ValueError(f"K must lie in [1, number of items = {test_user_items.shape[1]}]")
    if batch_size < 1:
        raise ValueError("batch_size must be >= 1")

    test = _canonical_pattern(test_user_items)
    metrics = gpu.RankingMetrics(test, K)
    to_generate = np.flatnonzero(np.diff(test.indptr) > 0).astype(np.int32)
    on_device = isinstance(model, MatrixFactorizationBase)
    progress = _progress(len(to_generate), show_progress)
    for start in range(0, len(to_generate), batch_size):
        batch = to_generate[start:start + batch_size]
        liked = train_user_items[batch]
        if on_device:
            ids, _ = model.knn.topk_device(model.item_factors, model._user_query(batch), K,
                                           query_filter=model._liked_filter(liked))
        else:
            ids, _ = model.recommend(batch, liked, N=K)
            ids = np.ascontiguousarray(ids, dtype=np.int32)
        metrics.add(ids, batch)
        progress.update(len(batch))
    progress.close()
    s = metrics.sums()  # the one host wait
    return {"precision": s["relevant"] / s["pr_div"], "map": s["sum_ap"] / s["total"], "ndcg": s["sum_ndcg"] / s["total"],
            "auc": s["sum_auc"] / s["total"]}


def precision_at_k(model, train_user_items, test_user_items, K=10, show_progress=True, num_threads=1,
                   batch_size=DEFAULT_BATCH_SIZE):
    """P@K of a fitted model (evaluation.pyx:236-266)."""
    return ranking_metrics_at_k(model, train_user_items, test_user_items, K, show_progress, num_threads, batch_size)["precision"]


def mean_average_precision_at_k(model, train_user_items, test_user_items, K=10, show_progress=True, num_threads=1,
                                batch_size=DEFAULT_BATCH_SIZE):
    """MAP@K of a fitted model (evaluation.pyx:270-298)."""
    return ranking_metrics_at_k(model, train_user_items, test_user_items, K, show_progress, num_threads, batch_size)["map"]


def ndcg_at_k(model, train_user_items, test_user_items, K=10, show_progress=True, num_threads=1,
              batch_size=DEFAULT_BATCH_SIZE):
    """NDCG@K of a fitted model (evaluation.pyx:302-330)."""
    return ranking_metrics_at_k(model, train_user_items, test_user_items, K, show_progress, num_threads, batch_size)["ndcg"]


def AUC_at_k(model, train_user_items, test_user_items, K=10, show_progress=True, num_threads=1,
             batch_size=DEFAULT_BATCH_SIZE):
    """Limited AUC at K of a fitted model (evaluation.pyx:334-362)."""
    return ranking_metrics_at_k(model, train_user_items, test_user_items, K, show_progress, num_threads, batch_size)["auc"]
