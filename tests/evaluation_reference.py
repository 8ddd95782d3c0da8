"""Plain numpy restatement of the ranking metrics of implicit_amd.evaluation (the definitions of the reference's
implicit/evaluation.pyx:444-475), for the cases a recorded fixture cannot cover.  Test infrastructure only.

For one user with held-out set L (pos = |L|, neg = items - pos) and recommended ids r[0 .. K):
    hit[i]  = r[i] in L                    (a negative or too large id is in no set)
    h[i]    = hits among positions 0 .. i
    P@K     : hits = h[K-1], divided (over all users) by sum of min(K, pos)
    AP      = sum_{hit i} h[i] / (i + 1) / min(K, pos)
    NDCG    = sum_{hit i} cg[i] / sum_{j < min(K, pos)} cg[j],   cg[i] = 1 / log2(i + 2)
    AUC     = (sum_{miss i} h[i] + (hits + pos) / 2 * (neg - misses)) / (pos * neg)
Users with nothing held out are not counted.  The sums over users are exact (math.fsum), i.e. not the order of any
implementation under test."""
import math

import numpy as np

SUMS = ("relevant", "pr_div", "sum_ap", "sum_ndcg", "sum_auc", "total")


def row_terms(ids, likes, items, K):
    """(hits, min(K, pos), ap, ndcg, auc) of one row; likes: any integer array (duplicates count once)."""
    likes = np.unique(likes)
    ids = np.asarray(ids)[:K]
    hit = np.isin(ids, likes) & (ids >= 0) & (ids < items)
    h = np.cumsum(hit)
    pos, hits = len(likes), int(h[-1])
    neg, div = items - pos, min(K, pos)
    cg = 1.0 / np.log2(np.arange(2, K + 2))
    at = np.flatnonzero(hit)
    ap = float(np.sum(h[at] / (at + 1.0))) / div
    ndcg = float(np.sum(cg[at])) / float(np.sum(cg[:div]))
    auc = (float(h[~hit].sum()) + (hits + pos) / 2.0 * (neg - (K - hits))) / (pos * float(neg))
    return hits, div, ap, ndcg, auc


def metrics(test, ids, userids, K):
    """test: scipy CSR (any stored entry is a like); ids: n x K; userids: n rows of `test`.  Returns (sums, per_row):
    the dict of SUMS and an n x 4 array of (hits, ap, ndcg, auc), zeros for users with nothing held out."""
    items = test.shape[1]
    per_row = np.zeros((len(userids), 4))
    cols = [[] for _ in SUMS]
    for r, u in enumerate(userids):
        likes = test.indices[test.indptr[u]:test.indptr[u + 1]]
        if len(likes) == 0:
            continue
        hits, div, ap, ndcg, auc = row_terms(ids[r], likes, items, K)
        per_row[r] = hits, ap, ndcg, auc
        for c, v in zip(cols, (hits, div, ap, ndcg, auc, 1.0)):
            c.append(v)
    return {name: math.fsum(c) for name, c in zip(SUMS, cols)}, per_row


def finish(s):
    return {"precision": s["relevant"] / s["pr_div"], "map": s["sum_ap"] / s["total"], "ndcg": s["sum_ndcg"] / s["total"],
            "auc": s["sum_auc"] / s["total"]}


def ranking_metrics_at_k(model, train, test, K, batch_size=1000):
    """The reference's driver loop over `model.recommend` (evaluation.pyx:423-435), scored by `metrics`."""
    users = np.flatnonzero(np.diff(test.indptr) > 0).astype(np.int32)
    all_ids = []
    for s in range(0, len(users), batch_size):
        batch = users[s:s + batch_size]
        ids, _ = model.recommend(batch, train[batch], N=K)
        all_ids.append(np.asarray(ids))
    sums, _ = metrics(test, np.concatenate(all_ids), users, K)
    return finish(sums)
