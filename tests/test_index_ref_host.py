"""The numpy index references (tests/index_ref.py) against each other and against their dense
definitions, on small cases, without a GPU: three routes to the link pairs, the
destination-major order as one lexsort, the incidence lists as the transpose of the index
arrays, the complete object graph as np.nonzero of a block diagonal, and the scalar
definitions of the cluster lists, the ranges, the clamp and the lower bound."""
import numpy as np
import pytest

import index_ref as iref


def _adj(n, seed, p=0.3):
    rng = np.random.default_rng(seed)
    a = rng.random((n, n)) < p
    a = a | a.T
    np.fill_diagonal(a, False)
    return a


@pytest.mark.parametrize('n', [0, 1, 2, 7, 65, 130])
def test_three_routes_to_the_link_pairs(n):
    adj = _adj(n, n)
    want = np.nonzero(np.triu(adj, 1))
    ei = np.stack(np.nonzero(adj))
    ps, pd = iref.pairs_from_edge_index(ei)
    assert (ps == want[0]).all() and (pd == want[1]).all()
    row_ptr, col = iref.csr_from_adj(adj)
    ptr, ls, ld = iref.link_pairs(row_ptr, col)
    assert (ls == want[0]).all() and (ld == want[1]).all()
    dptr, ds, dd = iref.dense_pairs(adj.astype(np.uint8) * 7)
    assert (ds == want[0]).all() and (dd == want[1]).all()
    assert (ptr == dptr).all() and len(ptr) == n + 1 and ptr[n] == len(want[0])
    assert (iref.csr_rows(row_ptr) == ei[0]).all()


def test_symmetric_csr_has_its_named_rows():
    for n in (2, 65, 2049, 34817):
        row_ptr, col = iref.symmetric_csr(n, n)
        rows = iref.csr_rows(row_ptr)
        deg = np.diff(row_ptr)
        assert deg.max() <= iref.MAX_DEGREE and deg[0] == min(n - 1, iref.MAX_DEGREE)
        assert (col[rows == 0] > 0).all() and (col[rows == n - 1] < n - 1).all() and deg[n - 1]
        assert (col != rows).all()
        key = rows.astype(np.int64) * n + col
        assert (np.diff(key) > 0).all()                              # row-major, no duplicates
        assert np.array_equal(np.sort(col.astype(np.int64) * n + rows), key)   # symmetric
        if n > 2100:
            assert (deg[2040:2060] == 0).all()
        ptr, ps, pd = iref.link_pairs(row_ptr, col)
        assert len(ps) * 2 == len(col) and (ps < pd).all()


@pytest.mark.parametrize('n,E', [(1, 5), (9, 0), (9, 200), (70, 3000)])
def test_csr_by_dst_is_one_lexsort(n, E):
    rng = np.random.default_rng(E)
    ei = rng.integers(0, n, (2, E))                       # duplicates and self loops
    ptr, perm, src, dropped = iref.csr_by_dst(ei, n)
    pos = np.arange(E)
    assert (perm == np.lexsort((pos, ei[0], ei[1]))).all() and dropped == 0
    assert (src == ei[0][perm]).all()
    assert (iref.csr_rows(ptr) == ei[1][perm]).all() and ptr[n] == E
    bad = ei.astype(np.int64).copy()
    if E:
        bad[0, ::7], bad[1, 3::11], bad[1, 5::13] = -1, n, 2 ** 40
    ok = (bad >= 0).all(0) & (bad < n).all(0)
    ptr2, perm2, src2, dropped2 = iref.csr_by_dst(bad, n)
    assert dropped2 == E - ok.sum() and ptr2[n] == ok.sum()
    keep = pos[ok]
    want = keep[np.lexsort((keep, bad[0][keep], bad[1][keep]))]
    assert (perm2 == want).all() and (src2 == bad[0][want]).all()


@pytest.mark.parametrize('with_b', [False, True])
def test_incidence_is_the_transpose(with_b):
    rng = np.random.default_rng(3)
    n, m = 40, 300
    a = rng.integers(0, n, m)
    a[a == 17] = 16                                       # an empty node
    b = rng.integers(0, n, m) if with_b else None
    if with_b:
        b[b == 17] = 16
        b[:5] = a[:5]                                     # a[u] == b[u]: listed twice
    ptr, lst = iref.incidence(a, b, n)
    assert len(ptr) == n + 1 and ptr[0] == 0 and ptr[n] == m * (2 if with_b else 1)
    for v in range(n):
        got = lst[ptr[v]:ptr[v + 1]]
        want = np.nonzero(a == v)[0]
        if with_b:
            want = np.sort(np.concatenate([want, np.nonzero(b == v)[0]]))
        assert (got == want).all()
    assert ptr[17] == ptr[18]
    ptr0, lst0 = iref.incidence(np.zeros(0, np.int32), None, 0)
    assert ptr0.tolist() == [0] and len(lst0) == 0


@pytest.mark.parametrize('sizes,extra', [([], 0), ([], 3), ([0], 0), ([1], 0), ([2], 1),
                                          ([0, 3, 0, 0, 2, 1, 5, 0], 0),
                                          ([0, 3, 0, 0, 2, 1, 5, 0], 4)])
def test_complete_graph_is_nonzero_of_block_diagonal(sizes, extra):
    n = int(sum(sizes)) + extra
    adj = np.zeros((n, n), bool)
    o = 0
    for s in sizes:
        adj[o:o + s, o:o + s] = ~np.eye(s, dtype=bool)
        o += s
    row_ptr, col, ei = iref.object_complete_graph(sizes, n)
    want = np.stack(np.nonzero(adj))
    assert ei.shape == want.shape and (ei == want).all() and (col == want[1]).all()
    assert (row_ptr == iref.csr_from_adj(adj)[0]).all() and len(row_ptr) == n + 1


def test_object_row_ranges_are_the_reference_startidx():
    size = np.array([0, 3, 0, 2, 5, 1, 0, 4])
    begin, end = iref.object_row_ranges(size)
    assert begin.tolist() == [0, 0, 3, 0, 2, 5, 1, 0]      # begin[c] = size[c - 1], as written
    assert end.tolist() == np.cumsum(size).tolist()
    sobj, base = [0, 3, 3, 8], [10, 13, 13]                # an empty sample; sample 2 starts empty
    begin, end = iref.object_row_ranges(size, sobj, base)
    assert begin.tolist() == [10, 10, 13, 13, 15, 18, 14, 13]
    assert end.tolist() == [10, 13, 13, 15, 20, 21, 21, 25]


@pytest.mark.parametrize('n', [1, 2, 127, 300])
def test_cluster_lists_match_the_member_definition(n):
    for labels in (np.arange(n), np.zeros(n, np.int64), iref.random_labels(n, n)):
        assert (labels <= np.arange(n)).all() and (labels[labels] == labels).all()
        of, ptr, idx, ncl = iref.cluster_lists(labels)
        roots = np.unique(labels)
        assert ncl == len(roots) and len(ptr) == n + 1
        assert (ptr[ncl:] == n).all() and ptr[0] == 0
        for c, r in enumerate(roots):                      # np.nonzero(meas_to_cluster_id == c)
            members = np.nonzero(labels == r)[0]
            assert (idx[ptr[c]:ptr[c + 1]] == members).all() and (of[members] == c).all()


def test_csr_clamp_cuts_at_a_row_boundary():
    row_ptr = np.array([0, 4, 4, 4, 10, 16, 16, 20], np.int32)
    for cap in (20, 25):
        got = iref.csr_clamp(row_ptr, 20, cap)
        assert (got[0] == row_ptr).all() and got[1:] == (20, 20)
    assert iref.csr_clamp(row_ptr, 20, 19)[0].tolist() == [0, 4, 4, 4, 4, 4, 4, 4]   # 9 -> 4
    assert iref.csr_clamp(row_ptr, 20, 19)[1:] == (4, 20)
    assert iref.csr_clamp(row_ptr, 20, 8)[0].tolist() == [0, 4, 4, 4, 4, 4, 4, 4]    # boundary
    assert iref.csr_clamp(row_ptr, 20, 7)[0].tolist() == [0] * 8    # cap / 2 below the first row
    assert iref.csr_clamp(row_ptr, 20, 7)[1:] == (0, 20)


def test_scan_lower_bound_and_gathers():
    x = np.array([3, 0, 0, 5, 1])
    assert iref.exclusive_scan(x).tolist() == [0, 3, 3, 3, 8, 9]
    assert iref.exclusive_scan([]).tolist() == [0]
    s = np.array([1, 1, 4, 4, 4, 9], np.int32)
    q = np.array([0, 1, 2, 4, 9, 10], np.int32)
    assert iref.lower_bound(s, 6, q).tolist() == [0, 0, 2, 2, 5, 6]
    assert iref.lower_bound(s, 3, q).tolist() == [0, 0, 2, 2, 3, 3]
    x = np.arange(12, dtype=np.float32).reshape(4, 3)
    assert iref.gather(x, [3, 0]).tolist() == [[9, 10, 11], [0, 1, 2]]
    assert iref.pair_add_rows(x, 2, [0, 1], [3, 3]).tolist() == [[9, 11], [12, 14]]
    assert iref.i32_to_i64([-1, 2 ** 31 - 1]).dtype == np.int64
