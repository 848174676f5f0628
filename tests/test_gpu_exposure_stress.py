"""A small helping of tests/stress_exposure.py: random sizes, contents, gamma curves, frame lists and rectangles, byte for byte
against the numpy restatement."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import stress_exposure  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("seed", (11, 12))
def test_random_cases(built, seed):
    out = stress_exposure.run(12, seed)
    assert out["mismatching"] == 0, out
