"""CPU tier of the fixed-order sum: the restatement the GPU tests compare with `==` (tests/mesheval_restatement.py, fixed_order_sum) is a
sum at all, and its order is one that other orders do not reproduce -- without that, bit equality on the GPU would prove nothing."""
import math

import numpy as np
import pytest

import mesheval_restatement as mr


def test_fixed_order_sum_is_exact_for_one_and_two_rows():
    x = np.array([[0.1, 3.0], [0.2, -7.5]])
    assert np.array_equal(mr.fixed_order_sum(x[:1], 2), x[0])
    assert np.array_equal(mr.fixed_order_sum(x, 2), [0.1 + 0.2, 3.0 + -7.5])
    assert np.array_equal(mr.fixed_order_sum(np.zeros((0, 3)), 3), [0.0, 0.0, 0.0])


@pytest.mark.parametrize("n", [1, 255, 256, 257, 262144, 262145, 600001])
def test_fixed_order_sum_is_a_sum(n):
    """any order of n additions is within n eps sum|x| of the exact sum"""
    d = mr.sum_case(n)
    x = np.where(d < mr.SUM_MAX_DIST, d, 0.0)
    got = mr.fixed_order_sum(x[:, None], 1)[0]
    exact = math.fsum(x)
    assert abs(got - exact) <= n * np.finfo(np.float64).eps * math.fsum(np.abs(x))
    s, c = mr.sum_below(d, mr.SUM_MAX_DIST)
    assert s == got and c == np.count_nonzero(d < mr.SUM_MAX_DIST)


def test_the_order_matters_at_the_size_the_gpu_test_uses():
    d = mr.sum_case(600001)
    assert 0.05 < np.mean(d >= mr.SUM_MAX_DIST) < 0.15 and 0 < np.isinf(d).sum() < 0.01 * d.size
    x = np.where(d < mr.SUM_MAX_DIST, d, 0.0)[:, None]
    got = mr.fixed_order_sum(x, 1)[0]
    assert got != np.sum(x)                                             # numpy's pairwise order
    assert got != mr.fixed_order_sum(x, 1, max_blocks=512)[0]           # the same scheme over half the blocks
