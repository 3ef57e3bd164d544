"""The index builders of include/radar_gnn.h restated in numpy -- the prefix scans as
np.cumsum, the orderings as np.nonzero / stable np.argsort / np.lexsort -- and the inputs their
tests share (tests/test_index_ref_host.py, tests/test_gpu_index_builders.py).  One function per
entry, each the definition the header states.  No test lives here."""
import numpy as np

I32, I64 = np.int32, np.int64


def exclusive_scan(x):
    """n inputs -> n + 1 outputs: out[i] = sum(x[:i]), out[n] the total."""
    out = np.zeros(len(x) + 1, I64)
    np.cumsum(np.asarray(x, I64), out=out[1:])
    return out.astype(I32)


def csr_from_adj(adj):
    """np.where(adj) as a CSR: (row_ptr int32 [n + 1], col int32 [E])."""
    adj = np.asarray(adj) != 0
    r, c = np.nonzero(adj)
    return exclusive_scan(np.bincount(r, minlength=adj.shape[0])), c.astype(I32)


def csr_rows(row_ptr):
    """rg_csr_rows: the row of every CSR position."""
    row_ptr = np.asarray(row_ptr, I64)
    return np.repeat(np.arange(len(row_ptr) - 1), np.diff(row_ptr)).astype(I32)


def pairs_from_edge_index(ei):
    """rg_pairs_from_edge_index: the edges with ei[0] < ei[1], in edge order."""
    ei = np.asarray(ei, I64).reshape(2, -1)
    keep = np.nonzero(ei[0] < ei[1])[0]
    return ei[0][keep].astype(I32), ei[1][keep].astype(I32)


def link_pairs(row_ptr, col):
    """rg_link_pairs: the CSR positions with col > row, row-major: (pair_ptr int32 [n + 1],
    pair_src, pair_dst)."""
    rows = csr_rows(row_ptr)
    col = np.asarray(col, I32)[:len(rows)]
    keep = np.nonzero(col > rows)[0]
    ptr = exclusive_scan(np.bincount(rows[keep], minlength=len(row_ptr) - 1))
    return ptr, rows[keep], col[keep]


def csr_by_dst(ei, n_nodes):
    """rg_csr_by_dst: (dst_ptr int32 [n + 1], perm, src_sorted, dropped).  Edges with an
    endpoint outside [0, n_nodes) are dropped (their count is ``dropped``); the kept ones are
    ordered by (dst, src, position)."""
    ei = np.asarray(ei, I64).reshape(2, -1)
    pos = np.arange(ei.shape[1])
    ok = (ei[0] >= 0) & (ei[0] < n_nodes) & (ei[1] >= 0) & (ei[1] < n_nodes)
    pos, s, d = pos[ok], ei[0][ok], ei[1][ok]
    order = np.lexsort((pos, s, d))
    ptr = exclusive_scan(np.bincount(d, minlength=n_nodes)[:n_nodes])
    return ptr, pos[order].astype(I32), s[order].astype(I32), int(ei.shape[1] - ok.sum())


def incidence(a, b, n_nodes):
    """rg_incidence: node n lists every item u with a[u] == n, and again every u with
    b[u] == n (an item with a[u] == b[u] is listed twice), ascending: (ptr int32 [n + 1],
    list)."""
    a = np.asarray(a, I64)
    item = np.arange(len(a))
    node = a
    if b is not None:
        node = np.concatenate([a, np.asarray(b, I64)])
        item = np.concatenate([item, item])
    order = np.lexsort((item, node))
    return exclusive_scan(np.bincount(node, minlength=n_nodes)[:n_nodes]), item[order].astype(I32)


def csr_clamp(row_ptr, n_edges, cap):
    """rg_csr_clamp: (row_ptr, n_edges, need).  need = the edge count; past the capacity the
    CSR is cut at the last row boundary <= cap // 2."""
    row_ptr = np.asarray(row_ptr, I32).copy()
    if n_edges <= cap:
        return row_ptr, n_edges, n_edges
    cut = int(row_ptr[row_ptr <= cap // 2].max())
    return np.minimum(row_ptr, cut).astype(I32), cut, n_edges


def dense_pairs(adj):
    """rg_dense_pair_rows + rg_dense_pair_emit: np.nonzero(np.triu(adj, 1)) with the row
    offsets: (row_ptr int32 [n + 1], pair_src, pair_dst)."""
    up = np.triu(np.asarray(adj) != 0, 1)
    r, c = np.nonzero(up)
    return exclusive_scan(up.sum(1)), r.astype(I32), c.astype(I32)


def object_complete_graph(object_size, n_nodes):
    """rg_object_complete_graph: np.nonzero of the block-diagonal union of complete graphs
    without self loops, as (row_ptr int32 [n_nodes + 1], col, edge_index int64 [2, E]).  Rows
    past sum(object_size) have no edges."""
    size = np.asarray(object_size, I64)
    off = exclusive_scan(size).astype(I64)
    obj = np.repeat(np.arange(len(size)), size)           # object of each node
    deg = np.zeros(n_nodes, I64)
    deg[:len(obj)] = size[obj] - 1
    row_ptr = exclusive_scan(deg)
    src = np.repeat(np.arange(n_nodes), deg)
    t = np.arange(len(src)) - row_ptr.astype(I64)[src]    # position inside the row
    first = off[obj][src] if len(src) else src
    dst = first + t + (first + t >= src)                  # the row's own column is skipped
    return row_ptr, dst.astype(I32), np.stack([src, dst]).astype(I64)


def object_row_ranges(object_size, sample_obj_ptr=None, sample_node_base=None):
    """rg_object_row_ranges: per sample begin[first] = 0, begin[c] = object_size[c - 1] (the
    reference's startidx as written), end = cumsum(object_size); each + the sample's base."""
    size = np.asarray(object_size, I64)
    if sample_obj_ptr is None:
        sample_obj_ptr, sample_node_base = [0, len(size)], [0]
    begin, end = np.zeros(len(size), I64), np.zeros(len(size), I64)
    for s in range(len(sample_obj_ptr) - 1):
        a, e = int(sample_obj_ptr[s]), int(sample_obj_ptr[s + 1])
        if e > a:
            begin[a + 1:e] = size[a:e - 1]
            end[a:e] = np.cumsum(size[a:e])
            begin[a:e] += int(sample_node_base[s])
            end[a:e] += int(sample_node_base[s])
    return begin.astype(I32), end.astype(I32)


def cluster_lists(labels):
    """rg_cluster_lists: labels[i] = the lowest node of i's component.  Cluster ids number the
    roots in ascending order: (cluster_of int32 [N], cluster_ptr int32 [N + 1] whose entries
    past n_clusters repeat N, cluster_idx int32 [N], n_clusters)."""
    labels = np.asarray(labels, I64)
    n = len(labels)
    rank = exclusive_scan(labels == np.arange(n))
    of = rank[labels]
    ptr = exclusive_scan(np.bincount(of, minlength=n)[:n])
    return of.astype(I32), ptr, np.argsort(of, kind='stable').astype(I32), int(rank[n])


def lower_bound(sorted_, n, queries):
    """rg_lower_bound_i32: the first p in sorted[0..n) with sorted[p] >= q."""
    return np.searchsorted(np.asarray(sorted_)[:n], queries, side='left').astype(I32)


def gather(table, idx):
    """rg_gather_i32 / rg_gather_rows_f32: table[idx]."""
    return np.asarray(table)[np.asarray(idx, I64)]


def pair_add_rows(x, w, idx0, idx1):
    """rg_pair_add_rows_f32: x[idx0][:, :w] + x[idx1][:, :w], one float32 rounding."""
    x = np.asarray(x, np.float32)
    return x[np.asarray(idx0, I64), :w] + x[np.asarray(idx1, I64), :w]


def i32_to_i64(x):
    return np.asarray(x, I32).astype(I64)


# ----------------------------------------------------------------------------- shared inputs
# scan lengths: the lane, wave-chunk (2048) and one-launch (32768) limits and one past each, a
# ragged last tile, and 256 / 257 / 258 tile sums (the carry loop of the partial-sum scan)
SCAN_LENGTHS = (0, 1, 63, 64, 65, 2047, 2048, 2049, 32767, 32768, 32769, 34817, 524288, 524289,
                526337)
MAX_DEGREE = 1000  # the per-node sorts are per-thread insertion sorts


def symmetric_csr(n, seed):
    """A symmetric CSR on n nodes (columns ascending per row, no self loops) with: node 0 a hub
    of min(n - 1, MAX_DEGREE) neighbours (all above it), the last node linked only below,
    isolated nodes (every node = 3 mod 7 past the hub's reach, and a run of them across the
    2048 tile boundary), and random short links elsewhere.  (row_ptr, col)."""
    rng = np.random.default_rng(seed)
    if n < 2:
        return np.zeros(n + 1, I32), np.zeros(0, I32)
    hub = min(n - 1, MAX_DEGREE)
    a = [np.zeros(hub, I64)]
    b = [np.arange(1, hub + 1)]
    m = min(3 * n, 600000)
    u = rng.integers(1, n, m)
    v = np.minimum(u + rng.integers(1, 9, m), n - 1)
    keep = (u != v)
    for w in (u, v):  # isolated nodes away from the hub
        keep &= ~((w > hub) & ((w % 7 == 3) | ((w >= 2040) & (w < 2060))))
    a.append(u[keep])
    b.append(v[keep])
    if n - 1 > hub:  # the last node: neighbours below only
        a.append(np.array([n - 3, n - 2]))
        b.append(np.array([n - 1, n - 1]))
    a, b = np.concatenate(a), np.concatenate(b)
    a, b = a[a != b], b[a != b]
    key = np.unique(np.concatenate([a * n + b, b * n + a]))  # symmetric, sorted row-major
    r, c = key // n, key % n
    return exclusive_scan(np.bincount(r, minlength=n)), c.astype(I32)


def random_labels(n, seed):
    """Component labels as rg_cluster_radius writes them: labels[i] <= i is i's root and a
    root labels itself."""
    rng = np.random.default_rng(seed)
    is_root = rng.random(n) < 0.3
    if n:
        is_root[0] = True
    roots = np.nonzero(is_root)[0]
    upto = np.searchsorted(roots, np.arange(n), side='right')  # roots <= i
    pick = roots[(rng.random(n) * upto).astype(I64)] if n else roots
    return np.where(is_root, np.arange(n), pick).astype(I32)
