"""Which kernels a top-k call reaches: the host code of imp_knn_topk, route by route.

A route is named by the library's profiler scopes: the scopes with a launch during the one topk call must be exactly the set
written down for the case (from a run of the library before its host code was untangled, but for the two multi-batch cases of
the materialising path, see DEFAULT_SCOPES; bench.py reads the same names).  One
case per branch of the host code at the smallest shape that reaches it: the general path (k above the candidate capacity), the
materialising path by each of its conditions (few items per k, k > 256, f > 256, fewer items than k), the emit path in its
screened, cosine, padded, wide (f > 256), several-batch and exact-path-row forms, device outputs, and host outputs too large
for the page-locked stage.  The routes an environment switch selects run in a fresh child process (the switches are read once
per process).

Results are judged by the rule of test_gpu_topk_fuzz.py: float64 scores, the best k up to its fp32 near-tie tolerance,
distinct ids, the returned scores those of the returned ids; rows with fewer than k surviving items over the survivors only."""
import os
import subprocess
import sys
from collections import namedtuple

import numpy as np
import pytest
import scipy.sparse as sp

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

Case = namedtuple("Case", "name ni f nq k dt norms filters opt", defaults=(np.float32, False, False, None))
# opt: an integer -- KnnQuery(max_temp_memory = 4 * ni * opt), score rows for `opt` queries: 50 gives three batches that cannot start
# on the 128-row blocks of the resident kernel's query planes (scored as stored), 129 is rounded down to batches of 128 + 2; "sparse" -- row 0's filter leaves 3 items and
# row 1's exactly k; "again" -- a second call on the same handle; "device" -- topk_device
F32, F16 = np.float32, np.float16
CASES = [
    Case("general", 6000, 20, 5, 5000),
    Case("general-fp16", 6000, 20, 5, 5000, F16),
    Case("materialising", 3000, 64, 130, 10),
    Case("materialising-filters", 3000, 64, 130, 10, filters=True),
    Case("materialising-batches", 3000, 64, 130, 10, opt=50),
    Case("materialising-batches-129", 3000, 64, 130, 10, opt=129),
    Case("materialising-k300", 3000, 64, 7, 300),
    Case("materialising-f320", 3000, 320, 130, 10),
    Case("fewer-items-than-k", 40, 32, 3, 64),
    Case("fewer-items-than-k-device", 40, 32, 3, 64, opt="device"),
    Case("emit", 8192, 64, 130, 10),
    Case("emit-fp16", 8192, 64, 130, 10, F16),
    Case("emit-filters", 8192, 64, 130, 10, filters=True),
    Case("emit-k64", 32768, 32, 5, 64),
    Case("emit-cosine", 8192, 64, 130, 10, norms=True),
    Case("emit-padded", 8192, 100, 130, 10),
    Case("emit-padded-fp16", 8192, 100, 130, 10, F16),
    Case("emit-f320", 8192, 320, 130, 10),
    Case("emit-batches", 2048, 16, 2100, 4, filters="coo", opt="again"),
    Case("emit-exact-rows", 8192, 64, 130, 10, filters="coo", opt="sparse"),
    Case("emit-device", 8192, 64, 130, 10, opt="device"),
    Case("materialising-device", 3000, 64, 130, 10, opt="device"),
    Case("unstaged-host-outputs", 1024, 16, 16400, 1024),
]
BY_NAME = {c.name: c for c in CASES}

# ---- the scope sets, as the library gave them before the rewrite of its host code -- except materialising-batches and
# materialising-batches-129: there the earlier library ran resident launches off the 128-row grid of the query planes and failed
# the float64 rule, so these two sets are those of the rewritten host code --------------------------------------------------
GENERAL = {"score_gemm_lds", "topk_select"}
FILTERS = {"item_filter", "coo_filter"}
DIRECT = {"score_gemm", "topk_select_pruned", "topk_select"}                   # materialising, operands as stored
MATERIALISING = DIRECT | {"split_query_rows"}                                  # ... resident two-term planes
REFRESH = FILTERS | {"filter_tile_refresh"}
EMIT_UNSPLIT = {"score_gemm_subset", "topk_threshold", "score_gemm", "topk_select_candidates"}
EMIT = EMIT_UNSPLIT | {"split_query_rows"}
DEFAULT_SCOPES = {
    "general": GENERAL,
    "general-fp16": GENERAL | {"cast_f16_f32"},
    "materialising": MATERIALISING,
    "materialising-filters": MATERIALISING | REFRESH,
    "materialising-batches": DIRECT,
    "materialising-batches-129": MATERIALISING,
    "materialising-k300": MATERIALISING,
    "materialising-f320": DIRECT,
    "fewer-items-than-k": MATERIALISING,
    "fewer-items-than-k-device": MATERIALISING,
    "emit": EMIT,
    "emit-fp16": EMIT,
    "emit-filters": EMIT | FILTERS,
    "emit-k64": EMIT,
    "emit-cosine": EMIT,
    "emit-padded": EMIT | {"pad_factors"},
    "emit-padded-fp16": EMIT | {"pad_factors"},
    "emit-f320": EMIT,
    "emit-batches": EMIT | {"coo_filter"},
    "emit-exact-rows": EMIT | {"coo_filter", "topk_fallback"},
    "emit-device": EMIT,
    "materialising-device": MATERIALISING,
    "unstaged-host-outputs": MATERIALISING,
}
SWITCHED_NAMES = ["general", "general-fp16", "materialising", "materialising-k300", "materialising-f320", "emit", "emit-fp16",
                  "emit-filters", "emit-cosine", "emit-padded", "emit-padded-fp16", "emit-exact-rows"]


def _with(base, **changes):
    return {n: changes.get(n.replace("-", "_"), base[n]) for n in SWITCHED_NAMES}


_NO_FAST = {n: GENERAL | ({"cast_f16_f32"} if "fp16" in n else set()) for n in SWITCHED_NAMES}
_NO_EMIT = {n: (MATERIALISING if n.startswith("emit") else DEFAULT_SCOPES[n]) for n in SWITCHED_NAMES}
_UNSPLIT = {n: DEFAULT_SCOPES[n] - {"split_query_rows"} for n in SWITCHED_NAMES}
SWITCHED_SCOPES = {
    # the general path for everything: LDS-staged GEMM on fp32 (copies), exact select
    "IMP_TOPK_NO_FAST=1": _with(_NO_FAST, emit_filters=GENERAL | FILTERS, emit_exact_rows=GENERAL | {"coo_filter"}),
    # no subset GEMM, no candidate lists: every emit shape on the materialising path
    "IMP_TOPK_NO_EMIT=1": _with(_NO_EMIT, emit_filters=MATERIALISING | REFRESH, emit_padded=MATERIALISING | {"pad_factors"},
                                emit_padded_fp16=MATERIALISING | {"pad_factors"},
                                emit_exact_rows=MATERIALISING | {"coo_filter", "filter_tile_refresh"}),
    # six-product bf16 kernels: the emit path splits its query rows (same scope), the materialising path reads them as stored
    "IMP_TOPK_RESIDENT=0": _with(DEFAULT_SCOPES, materialising=DIRECT, materialising_k300=DIRECT),
    "IMP_TOPK_SCREEN=0": _with(DEFAULT_SCOPES),
    # exact-fp32 MFMA form: nothing is split
    "IMP_TOPK_FP32_MFMA=1": _with(_UNSPLIT),
    "IMP_TOPK_RESIDENT=1": _with(DEFAULT_SCOPES),
    "IMP_TOPK_SCREEN=1": _with(DEFAULT_SCOPES),
}


def _inputs(case):
    """(items, queries, float64 scores with the filtered entries at -inf, norms or None, keyword operands as numpy / scipy)."""
    rng = np.random.default_rng(1000 + CASES.index(case))
    items = (rng.standard_normal((case.ni, case.f)) * 0.1).astype(case.dt)
    q = (rng.standard_normal((case.nq, case.f)) * 0.1).astype(case.dt)
    S = q.astype(np.float64) @ items.astype(np.float64).T
    norms = liked = filt = None
    if case.norms:
        norms = np.linalg.norm(items.astype(np.float32), axis=1).astype(np.float32)
        norms[norms == 0] = 1e-10
        S = S / norms[None, :].astype(np.float64)
    if case.filters:
        liked = sp.random(case.nq, case.ni, density=min(0.5, 20.0 / case.ni), format="csr", dtype=np.float32,
                          random_state=int(rng.integers(1 << 30)))
        if case.opt == "sparse":
            dense = liked.toarray()
            for row, left in ((0, 3), (1, case.k)):
                dense[row] = 1.0
                dense[row, rng.permutation(case.ni)[:left]] = 0.0
            liked = sp.csr_matrix(dense)
        S[liked.nonzero()] = -np.inf
    if case.filters is True:
        filt = np.unique(rng.integers(0, case.ni, size=max(1, case.ni // 50))).astype(np.int32)
        S[:, filt] = -np.inf
    return items, q, S, norms, liked, filt


def judge(case, items, q, S, norms, ids, d):
    """The rule of test_gpu_topk_fuzz._check, on results already computed."""
    k, f, dt = case.k, case.f, case.dt
    I64, Q64 = items.astype(np.float64), q.astype(np.float64)
    avail = np.isfinite(S).sum(axis=1)
    noise = 16 * f * 6e-8 * (np.abs(Q64) @ np.abs(I64).mean(axis=0)) / (np.median(norms) if norms is not None else 1.0)
    for r in range(case.nq):
        kk = int(min(k, avail[r]))
        best = -np.sort(-S[r])[:kk]
        got = S[r, ids[r, :kk].astype(np.int64)]
        tol = 4e-6 * (np.abs(best) + 1e-30) + noise[r]
        assert np.isfinite(got).all() and len(set(ids[r, :kk].tolist())) == kk, (r, ids[r, :8])
        assert (np.abs(np.sort(got)[::-1] - best) <= tol).all(), (r, np.sort(got)[::-1][:4], best[:4])
        assert np.allclose(d[r, :kk], got, rtol=2e-3 if dt == np.float16 else 4e-5, atol=float(tol.max()))


def run_case(gpu, case):
    """One topk call (two for "again") under the profiler: (scopes with a launch, ids, distances), judged."""
    items, q, S, norms, liked, filt = _inputs(case)
    kw = {}
    if norms is not None:
        kw["item_norms"] = gpu.Matrix(norms.reshape(1, -1))
    if liked is not None:
        kw["query_filter"] = gpu.COOMatrix(liked.tocoo())
    if filt is not None:
        kw["item_filter"] = gpu.IntVector(filt)
    knn = gpu.KnnQuery(max_temp_memory=4 * case.ni * case.opt) if isinstance(case.opt, int) else gpu.KnnQuery()
    I, Q = gpu.Matrix(items), gpu.Matrix(q)
    for _ in range(2 if case.opt == "again" else 1):  # (the second call finds the bitmap as the first one left it)
        gpu.Profiler.reset()
        gpu.Profiler.enable(True)
        try:
            if case.opt == "device":
                ids, d = knn.topk_device(I, Q, case.k, **kw)
            else:
                ids, d = knn.topk(I, Q, case.k, **kw)
        finally:
            gpu.Profiler.enable(False)
        scopes = {n for n in gpu.Profiler.names() if gpu.Profiler.get(n)[1] > 0}
        if case.opt == "device":
            ids, d = ids.to_numpy().view(np.int32), d.to_numpy()
        assert ids.shape == d.shape == (case.nq, case.k) and ids.dtype == np.int32 and d.dtype == np.float32
        judge(case, items, q, S, norms, ids, d)
        k_eff = min(case.k, case.ni)
        assert not ids[:, k_eff:].any() and not d[:, k_eff:].any()  # entries past k_eff: what the caller's arrays held
    return scopes, ids, d


def check(gpu, case, want):
    scopes, _, _ = run_case(gpu, case)
    print(f"{case.name}: {sorted(scopes)}")
    assert scopes == want, (case.name, sorted(scopes ^ want))


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_default_route(gpu, case):
    check(gpu, case, DEFAULT_SCOPES[case.name])


def run_switched(switch):
    """Body of the child process of test_switched_route."""
    import warnings

    warnings.simplefilter("ignore")
    import implicit_amd.gpu as gpu

    for name in SWITCHED_NAMES:
        check(gpu, BY_NAME[name], SWITCHED_SCOPES[switch][name])
    print("routes ok")


@pytest.mark.parametrize("switch", list(SWITCHED_SCOPES))
def test_switched_route(gpu, switch):
    """The kernels an A/B switch selects (or, for the values that mean "on", leaves alone), judged like the default ones."""
    name, value = switch.split("=")
    code = (f"import sys; sys.path[:0] = [{ROOT!r}, {os.path.join(ROOT, 'tests')!r}]; "
            f"import test_gpu_topk_routes as t; t.run_switched({switch!r})")
    out = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, **{name: value}), capture_output=True, text=True,
                         timeout=300)
    print(out.stdout)
    assert out.returncode == 0 and "routes ok" in out.stdout, (out.stdout + out.stderr)[-3000:]
