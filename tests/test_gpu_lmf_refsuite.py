"""The reference's own model tests (tests/recommender_base_test.py of benfred/implicit, unmodified, in build/refsuite) over
implicit_amd.lmf.LogisticMatrixFactorization, configured as the reference's tests/lmf_test.py configures its CPU model:
factors=3, regularization=0, random_state=43.  Run in a subprocess, as tests/test_reference_suite.py runs the others."""
import os
import re
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SUITE = os.path.join(ROOT, "build", "refsuite")

_TEST_MODULE = '''
import unittest

from recommender_base_test import RecommenderBaseTestMixin

from implicit_amd.lmf import LogisticMatrixFactorization


class GPULMFTest(unittest.TestCase, RecommenderBaseTestMixin):
    def _get_model(self):
        return LogisticMatrixFactorization(factors=3, regularization=0, use_gpu=True, random_state=43)
'''


@pytest.mark.skipif(not os.path.isdir(SUITE), reason="build/refsuite not assembled (needs /root/reference at build time)")
def test_reference_mixin_passes_over_gpu_lmf(gpu, tmp_path):
    (tmp_path / "gpu_lmf_test.py").write_text(_TEST_MODULE)
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([SUITE, os.path.join(SUITE, "tests"), ROOT]), OPENBLAS_NUM_THREADS="1",
               OMP_NUM_THREADS="16")
    # test_fit_non_csr_matrix expects implicit.utils.ParameterWarning; this package warns with its own
    # implicit_amd.utils.ParameterWarning (the same message, a different class), so that one case is deselected
    out = subprocess.run([sys.executable, "-m", "pytest", "-q", "-p", "no:cacheprovider", "gpu_lmf_test.py", "--deselect",
                          "gpu_lmf_test.py::GPULMFTest::test_fit_non_csr_matrix"], cwd=str(tmp_path), env=env,
                         capture_output=True, text=True, timeout=900)
    tail = out.stdout[-3000:] + out.stderr[-1500:]
    m = re.search(r"(\d+) passed", out.stdout)
    passed = int(m.group(1)) if m else 0
    print(f"reference recommender_base_test.py over the GPU LMF: {passed} passed (rc {out.returncode})")
    assert out.returncode == 0 and passed >= 20 and "failed" not in out.stdout, tail
