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


# ---- full-catalogue metrics (NEW: no counterpart in the reference) -----------------------------------------------------------
def _full_rank_sums(ranks, offsets, candidates, Ks):
    """The metrics of full_ranking_metrics from the ranks of KnnQuery.target_ranks (float64, host): `ranks` aligned with the
    targets (-1: excluded), offsets the targets' row pointers, candidates |C_u| per row."""
    ranks, candidates = np.asarray(ranks, dtype=np.int64), np.asarray(candidates, dtype=np.float64)
    row = np.repeat(np.arange(len(offsets) - 1), np.diff(offsets))
    valid = ranks >= 0
    out = {"skipped": int((~valid).sum()), "recall": {}, "ndcg": {}}
    ranks, row = ranks[valid], row[valid]
    if not len(ranks):
        out.update(mpr=float("nan"), mrr=float("nan"), auc=float("nan"))
        out["recall"], out["ndcg"] = {K: float("nan") for K in Ks}, {K: float("nan") for K in Ks}
        return out
    order = np.lexsort((ranks, row))  # every user's ranks ascending
    ranks, row = ranks[order], row[order]
    users, first, n_u = np.unique(row, return_index=True, return_counts=True)
    cand = candidates[users]
    out["mpr"] = float(np.mean(ranks / np.maximum(candidates[row] - 1.0, 1.0)))
    out["mrr"] = float(np.mean(1.0 / (1.0 + ranks[first])))
    # target number p of a user, in ascending order, has rank - p negatives above it
    above = np.add.reduceat((ranks - (np.arange(len(ranks)) - np.repeat(first, n_u))).astype(np.float64), first)
    negatives = cand - n_u
    has = negatives > 0
    out["auc"] = float(np.mean(1.0 - above[has] / (n_u[has] * negatives[has]))) if has.any() else float("nan")
    for K in Ks:
        cg = 1.0 / np.log2(np.arange(2, K + 2))  # the discount table of ranking_metrics_at_k
        cg_sum = np.cumsum(cg)
        hit = ranks < K
        ideal = np.minimum(K, n_u)
        out["recall"][K] = float(hit.sum() / ideal.sum())
        dcg = np.add.reduceat(np.where(hit, cg[np.minimum(ranks, K - 1)], 0.0), first)
        out["ndcg"][K] = float(np.mean(dcg / cg_sum[ideal - 1]))
    return out


def full_ranking_metrics(model, train_user_items, test_user_items, K=(10,), show_progress=True,
                         batch_size=DEFAULT_BATCH_SIZE, return_ranks=False):
    """Metrics over the WHOLE catalogue of a fitted matrix-factorisation model: every held-out item's rank among all the items
    its user could be recommended (the items outside the user's train row; 0-based, exact score ties go to the lower id),
    computed by KnnQuery.target_ranks without a score matrix.  Every stored index of test_user_items is a target (the
    pattern only: values carry no weight); a target stored in the user's train row is no candidate and is left out.  Users
    with nothing held out are not queried.  Returns a dict:
      "mpr"     mean over the pairs of rank / max(candidates - 1, 1) -- the expected percentile rank of Hu, Koren and Volinsky
                (2008), unweighted, in [0, 1], lower is better
      "mrr"     mean over the users of 1 / (1 + best rank)
      "auc"     mean over the users of the exact AUC, positives = the user's targets, negatives = the other candidates
                (users without negatives are left out)
      "recall", "ndcg"   dicts keyed by each K: a target is a hit when rank < K; denominators and the discount table are
                those of ranking_metrics_at_k (sum of min(K, targets) over the users; the ideal DCG of min(K, targets) hits)
      "skipped" the targets left out
    return_ranks adds "ranks": {"users", "offsets", "targets", "ranks", "candidates"}, the queried users in ascending order
    and the arrays of KnnQuery.target_ranks over them (rank -1: skipped).  K: an int or a sequence of ints >= 1.
    NotImplementedError for a model whose scores are not dot products of factors.  Runs on the GPU only."""
    import implicit_amd.gpu as gpu
    from .ann.ivf import IVFModel
    from .gpu.matrix_factorization_base import MatrixFactorizationBase

    if isinstance(model, IVFModel):
        model = model.model  # the exact model the index was built over
    if not isinstance(model, MatrixFactorizationBase):
        raise NotImplementedError(f"full_ranking_metrics ranks by dot products of user and item factors; the scores of "
                                  f"{type(model).__name__} are not factor dot products")
    if not gpu.HAS_CUDA:
        raise ValueError("No usable HIP device / extension: implicit_amd.evaluation computes its metrics on the GPU")
    if not isinstance(train_user_items, csr_matrix):
        train_user_items = train_user_items.tocsr()
    if not isinstance(test_user_items, csr_matrix):
        test_user_items = test_user_items.tocsr()
    Ks = tuple(int(k) for k in (K if np.iterable(K) else (K,)))
    batch_size = int(batch_size)
    if not Ks or min(Ks) < 1:
        raise ValueError("every K must be >= 1")
    if batch_size < 1:
        raise ValueError("batch_size must be >= 1")

    test = _canonical_pattern(test_user_items)
    indptr = test.indptr.astype(np.int64)
    users = np.flatnonzero(np.diff(indptr) > 0).astype(np.int32)
    progress = _progress(len(users), show_progress)
    ranks, candidates, targets, counts = [], [], [], []
    for start in range(0, len(users), batch_size):
        batch = users[start:start + batch_size]
        rows = test[batch]
        r, c = model.knn.target_ranks(model.item_factors, model._user_query(batch), rows.indptr, rows.indices,
                                      query_filter=model._liked_filter(train_user_items[batch]))
        ranks.append(r), candidates.append(c), targets.append(rows.indices.astype(np.int32)), counts.append(np.diff(rows.indptr))
        progress.update(len(batch))
    progress.close()
    cat = lambda parts, dtype: np.concatenate(parts) if parts else np.zeros(0, dtype=dtype)  # noqa: E731
    ranks, candidates, targets = cat(ranks, np.int32), cat(candidates, np.int32), cat(targets, np.int32)
    offsets = np.concatenate(([0], np.cumsum(cat(counts, np.int64)))).astype(np.int64)
    out = _full_rank_sums(ranks, offsets, candidates, Ks)
    if return_ranks:
        out["ranks"] = {"users": users, "offsets": offsets, "targets": targets, "ranks": ranks, "candidates": candidates}
    return out


def mean_percentile_rank(model, train_user_items, test_user_items, show_progress=True, batch_size=DEFAULT_BATCH_SIZE):
    """The mean percentile rank of the held-out items over the whole catalogue (full_ranking_metrics)."""
    return full_ranking_metrics(model, train_user_items, test_user_items, (1,), show_progress, batch_size)["mpr"]


def mean_reciprocal_rank(model, train_user_items, test_user_items, show_progress=True, batch_size=DEFAULT_BATCH_SIZE):
    """The mean reciprocal rank of every user's best held-out item over the whole catalogue (full_ranking_metrics)."""
    return full_ranking_metrics(model, train_user_items, test_user_items, (1,), show_progress, batch_size)["mrr"]


def auc(model, train_user_items, test_user_items, show_progress=True, batch_size=DEFAULT_BATCH_SIZE):
    """The exact AUC, held-out items against every other candidate, averaged over the users (full_ranking_metrics)."""
    return full_ranking_metrics(model, train_user_items, test_user_items, (1,), show_progress, batch_size)["auc"]
