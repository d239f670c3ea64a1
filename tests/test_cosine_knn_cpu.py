"""Host side of knn_graph(): graph_from_knn() on hand-written (idx, sim)."""
import numpy as np
import pytest

from rcppml_amd import similarity as S

# four columns, k = 2.  0 <-> 1 mutual; 2 names 0 but 0 does not name 2 (one-sided); 3's neighbours have non-positive cosines
IDX = np.array([[1, 3], [0, 2], [0, 1], [0, 1]])
SIM = np.array([[0.9, 0.0], [0.9, 0.5], [0.4, 0.5], [0.0, -0.2]])


@pytest.mark.parametrize("weights", S.GRAPH_WEIGHTS)
@pytest.mark.parametrize("symmetrize", S.GRAPH_SYMMETRIZE)
def test_graph_from_knn(weights, symmetrize):
    Sm = S.graph_from_knn(IDX, SIM, weights, symmetrize, laplacian=False).toarray()
    L = S.graph_from_knn(IDX, SIM, weights, symmetrize).toarray()
    w = (lambda v: 1.0) if weights == "binary" else (lambda v: v)
    want = np.zeros((4, 4))
    want[0, 1] = want[1, 0] = w(0.9)
    want[1, 2] = want[2, 1] = w(0.5)
    if symmetrize == "union":
        want[0, 2] = want[2, 0] = w(0.4)          # the one-sided edge: in the union, not in the mutual graph
    assert np.array_equal(Sm, want) and not Sm[3].any()          # non-positive cosines make no edge
    assert np.array_equal(L, L.T) and np.all(L[~np.eye(4, dtype=bool)] <= 0)
    assert np.array_equal(L, np.diag(want.sum(axis=1)) - want)
    assert np.all(np.abs(L.sum(axis=1)) <= 4 * 2.0 ** -52)
