"""The stand-in Eigen headers of oracle/refshim/ on their own: oracle/refshim/selftest.cpp builds
matrices with the operations the reference's tick sources use (comma initialiser, replicate, block
and head assignment, diagonal-to-dense, products, sparse insert / coeffRef and the compressed column
order); the same matrices are rebuilt here in numpy and compared exactly. The reference-parity
fixtures (tests/golden/ref_*.npz) were recorded through these headers, so an error here would be an
error in every expected value of tests/test_reference_parity.py."""
import os
import subprocess

import numpy as np
import pytest
from conftest import ROOT


@pytest.fixture(scope="module")
def shown():
    odir = os.path.join(ROOT, "oracle")
    subprocess.check_call(["make", "-s", "-C", odir, "selftest"])
    text = subprocess.check_output([os.path.join(odir, "lib", "refshim_selftest")], text=True)
    out = {}
    for line in text.splitlines():
        name, r, c, *v = line.split()
        out[name] = np.array([float(x) for x in v]).reshape(int(r), int(c))
    return out


def ramp(r, c, start):
    return start + 10.0 * np.arange(r)[:, None] + np.arange(c)[None, :]


def col(*v):
    return np.array(v, float).reshape(-1, 1)


def expected():
    v3, a3, c3, pair2 = col(1.5, -2.5, 3.25), col(1, 2, 3), col(0.5, 0.25, 0.125), col(-7, 9)
    Q = np.diag([10.0, 0.1, 0.0])
    x = col(0.1, 0.7, -3.0)
    big = np.zeros((5, 4))
    big[1:4, 2:4] = ramp(3, 2, 1.0)
    big[4, 0] = 1.0
    # dense form of the sparse matrix of selftest.cpp, and the stored pattern incl. explicit zeros
    stored = {(3, 0): 30.0, (0, 0): 0.0, (2, 2): -1.0, (1, 2): 7.0, (0, 2): 0.0}
    colptr, rowind, val = [0], [], []
    for j in range(3):
        for i in sorted(i for (i, jj) in stored if jj == j):
            rowind.append(i)
            val.append(stored[(i, j)])
        colptr.append(len(rowind))
    return {
        "comma_vec": v3,
        "comma_scalars": np.array([[1.0, 2, 3], [4, 5, 6]]),
        "comma_side": np.hstack([ramp(3, 3, 1.0), -np.eye(3)]),
        "comma_bands": np.vstack([np.hstack([ramp(2, 2, 1.0), ramp(2, 1, 50.0)]), ramp(1, 3, 70.0)]),
        "comma_stack": np.vstack([np.zeros((3, 1)), np.tile(pair2, (3, 1)), col(4, 5), pair2]),
        "head_comma": np.vstack([-a3, np.tile(-c3, (2, 1)), np.ones((2, 1))]),
        "replicate": np.tile(ramp(2, 3, 1.0), (2, 2)),
        "identity_3x2": np.eye(3, 2),
        "ones_2x3": np.ones((2, 3)),
        "block": big,
        "diag_dense": Q,
        # one nonzero term per row: equal to the elementwise product whatever the summation order
        "neg_diag_times_vec": -(np.diag(Q).reshape(-1, 1) * x),
        "matmul": ramp(2, 3, 1.0) @ ramp(3, 2, 0.5),  # small integers and halves: exact in any order
        "axpy": x + a3 * 0.01,
        "linear_index": ramp(2, 3, 1.0).reshape(-1, 1, order="F"),
        "resize_keep": col(4, -5, 6),
        "csc_colptr": col(*colptr),
        "csc_rowind": col(*rowind),
        "csc_val": col(*val),
        "setzero_nnz": col(0),
    }


def test_selftest_covers_every_expected_matrix(shown):
    assert sorted(shown) == sorted(expected())


@pytest.mark.parametrize("name", sorted(expected()))
def test_refshim_matches_numpy(shown, name):
    want = expected()[name]
    assert shown[name].shape == want.shape
    np.testing.assert_array_equal(shown[name], want)  # exact: the values are printed with %.17g
