"""The integer plumbing under the matrix kernels -- the prefix scan (csrc/scan.hip) and the small
kernels that turn it into CSRs, pair lists, incidence lists, object graphs and cluster lists --
against the numpy definitions of tests/index_ref.py, at the scan's path changes, in buffers the
test owns.

Every entry is launched directly through _native.lib().  Each output is a view of exactly the
size include/radar_gnn.h states, inside an allocation with 256 sentinel bytes in front and
behind and a sentinel-filled body; the workspace has exactly *_workspace_size(...) bytes, which
is the number passed.  A case runs with the workspace body filled with 0x00 and again with 0xFF:
both runs must equal the reference exactly (all values are integers, or float32 results of one
rounding, so no tolerance is involved), every guard band must be intact, every documented
element written, every element the header leaves alone still the sentinel; and with
workspace_bytes - 1 the entry returns RG_ERR_ARG and writes nothing.

Scan lengths are index_ref.SCAN_LENGTHS: 0, 1, the lane / wave-chunk (2048) / one-launch
(32768) limits and one past each, a ragged last tile, and 256, 257 and 258 tile sums, where the
partial-sum scan's carry loop starts to iterate.  No node has more than 1000 entries (the
per-node orderings are per-thread insertion sorts).  No chain or conv kernel runs over a graph
built here; the out-of-range cases call the builder only."""
import functools

import numpy as np
import pytest
import torch

import index_ref as iref
from index_ref import SCAN_LENGTHS as S

pytestmark = pytest.mark.gpu

GUARD = 256
SENT = 0xA5
RG_ERR_ARG = 1
I32, I64, F32, U8 = np.int32, np.int64, np.float32, np.uint8


def sent(shape, dtype):
    """A host array of `shape` whose every byte is the sentinel."""
    shape = (shape,) if np.isscalar(shape) else tuple(shape)
    n = int(np.prod(shape, dtype=np.int64)) * np.dtype(dtype).itemsize
    return np.full(n, SENT, U8).view(dtype).reshape(shape)


def tail_kept(values, total, dtype=I32):
    """`values` followed by elements the entry leaves alone, `total` in all."""
    out = sent(total, dtype)
    out[:len(values)] = values
    return out


class Guarded:
    """guarded(shape, dtype, fill): a device view of exactly the stated size between two bands
    of GUARD sentinel bytes.  The body is pre-filled with `fill` (the sentinel by default);
    its base is 256-B aligned."""

    def __init__(self, dev, shape, dtype, fill=SENT):
        self.host = sent(shape, dtype)
        self.nbytes = self.host.nbytes
        self.raw = torch.full((GUARD + self.nbytes + GUARD,), SENT, dtype=torch.uint8, device=dev)
        self.ptr = self.raw.data_ptr() + GUARD
        assert self.ptr % 256 == 0
        if fill != SENT:
            self.raw[GUARD:GUARD + self.nbytes].fill_(fill)

    def upload(self, arr):
        arr = np.ascontiguousarray(arr, self.host.dtype)
        assert arr.shape == self.host.shape
        self.raw[GUARD:GUARD + self.nbytes].copy_(torch.from_numpy(arr.reshape(-1).view(U8)))
        return self

    def numpy(self):
        body = self.raw[GUARD:GUARD + self.nbytes].cpu().numpy()
        return body.view(self.host.dtype).reshape(self.host.shape)

    def check_guards(self, what):
        raw = self.raw.cpu().numpy()
        for band, name in ((raw[:GUARD], 'front'), (raw[GUARD + self.nbytes:], 'back')):
            hit = np.nonzero(band != SENT)[0]
            assert hit.size == 0, f'{what}: {name} guard overwritten at bytes {hit[:8].tolist()}'


def guarded(dev, shape, dtype, fill=SENT):
    return Guarded(dev, shape, dtype, fill)


def dev_in(dev, arr, dtype):
    """An input on the device (one spare element, so that an empty input still has a pointer)."""
    arr = np.ascontiguousarray(arr, dtype).reshape(-1)
    return torch.from_numpy(np.concatenate([arr, np.zeros(1, dtype)])).to(dev)


def _lib():
    from graph_neural_network_for_radar_perception_amd import _native as nat
    return nat.lib()


def _stream(dev):
    return torch.cuda.current_stream(dev).cuda_stream


def _same(got, want, what):
    want = np.ascontiguousarray(want, got.dtype)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    a = got.reshape(-1).view(U8).reshape(got.size, got.itemsize)
    b = want.reshape(-1).view(U8).reshape(want.size, got.itemsize)
    bad = np.nonzero((a != b).any(1))[0]
    assert bad.size == 0, (f'{what}: {bad.size} of {got.size} elements differ, first at '
                           f'{bad[:4].tolist()}: got {got.reshape(-1)[bad[:4]].tolist()} want '
                           f'{want.reshape(-1)[bad[:4]].tolist()}')


def run_case(dev, name, outs, call, want, ws_bytes=None, init=None):
    """The protocol of the module docstring for one case of entry `name`.
    outs: {buffer: (shape, dtype)} at the sizes the header states; init: {buffer: contents} for
    in/out buffers; call(fn, bufs, ws_ptr, ws_bytes) -> rc launches the entry; want: {buffer:
    the whole expected contents, the sentinel where the header leaves an element alone}."""
    lib = _lib()
    fn = getattr(lib, name)

    def fresh():
        bufs = {k: guarded(dev, shape, dt) for k, (shape, dt) in outs.items()}
        for k, arr in (init or {}).items():
            bufs[k].upload(arr)
        return bufs

    for fill in ((0x00, 0xFF) if ws_bytes is not None else (None,)):
        bufs = fresh()
        ws = guarded(dev, ws_bytes, U8, fill) if ws_bytes is not None else None
        rc = call(fn, bufs, ws.ptr if ws else None, ws_bytes)
        torch.cuda.synchronize(dev)
        assert rc == 0, (name, rc, lib.rg_last_error())
        what = f'{name} (workspace filled with {fill})'
        for k, g in bufs.items():
            g.check_guards(f'{what}: {k}')
            _same(g.numpy(), want[k], f'{what}: {k}')
        if ws:
            ws.check_guards(f'{what}: workspace')
    if ws_bytes is not None:
        bufs = fresh()
        ws = guarded(dev, ws_bytes, U8, 0x00)
        rc = call(fn, bufs, ws.ptr, ws_bytes - 1)
        torch.cuda.synchronize(dev)
        assert rc == RG_ERR_ARG, (name, 'workspace_bytes - 1', rc)
        for k, g in bufs.items():
            g.check_guards(f'{name} (short workspace): {k}')
            _same(g.numpy(), (init or {}).get(k, g.host), f'{name} (short workspace): {k}')
        ws.check_guards(f'{name} (short workspace): workspace')


# ----------------------------------------------------------------- rg_pairs_from_edge_index
def _edge_patterns(E):
    rng = np.random.default_rng(E + 1)
    n = max(E // 4, 3)
    ei = rng.integers(0, n, (2, E))                       # self loops and duplicates
    if E > 4:
        ei[:, 1] = ei[:, 0]
        ei[1, 2] = ei[0, 2]
    lo, hi = ei.min(0), ei.max(0)
    last = np.arange(E) >= (max(E, 1) - 1) // 2048 * 2048   # the last scan tile
    return {'random': ei, 'no pair': np.stack([hi, lo]), 'all pairs': np.stack([lo, hi + 1]),
            'pairs in the last tile only': np.where(last, np.stack([lo, hi + 1]),
                                                    np.stack([hi, lo]))}


@pytest.mark.parametrize('E', S)
def test_pairs_from_edge_index(cuda_device, E):
    dev = cuda_device
    wsb = _lib().rg_pairs_from_edge_index_workspace_size(E)
    for pattern, ei in _edge_patterns(E).items():
        ps, pd = iref.pairs_from_edge_index(ei)
        if pattern == 'no pair':
            assert len(ps) == 0
        elif pattern == 'all pairs':
            assert len(ps) == E
        d_ei = dev_in(dev, ei, I64)
        run_case(dev, 'rg_pairs_from_edge_index',
                 dict(pair_src=(len(ps), I32), pair_dst=(len(ps), I32), n_pairs=(1, I32)),
                 lambda fn, b, w, wb: fn(d_ei.data_ptr(), E, b['pair_src'].ptr, b['pair_dst'].ptr,
                                         b['n_pairs'].ptr, w, wb, _stream(dev)),
                 dict(pair_src=ps, pair_dst=pd, n_pairs=[len(ps)]), ws_bytes=wsb)


# ----------------------------------------------------------------------------- rg_incidence
def _incidence_items(n, with_b, seed):
    """Items over n nodes: a hub (the last non-empty node) of ~980 entries, empty nodes (every
    node = 2 mod 5 and runs across the 2048 and 32768 boundaries), a few items elsewhere."""
    rng = np.random.default_rng(seed)
    node = np.arange(n)
    empty = (node % 5 == 2) | ((node >= 2040) & (node < 2060)) | ((node >= 32760) & (node < 32780))
    allowed = node[~empty]
    m = min(2 * n, 300000)
    hub = 980 // (2 if with_b else 1)
    cols = []
    for _ in range(2 if with_b else 1):
        c = allowed[rng.integers(0, len(allowed), m + hub)]
        c[rng.permutation(m + hub)[:hub]] = allowed[-1]
        cols.append(c)
    if with_b:
        cols[1][:3] = cols[0][:3]                          # a[u] == b[u]: listed twice
    return cols[0], (cols[1] if with_b else None)


@pytest.mark.parametrize('with_b', [False, True], ids=['a', 'a+b'])
@pytest.mark.parametrize('n', S)
def test_incidence(cuda_device, n, with_b):
    dev = cuda_device
    lib = _lib()
    cases = [(np.zeros(0, I32), np.zeros(0, I32) if with_b else None)]        # n_items = 0
    if n:
        cases.append(_incidence_items(n, with_b, n))
    for a, b in cases:
        m = len(a)
        ptr, lst = iref.incidence(a, b, n)
        assert len(ptr) == n + 1 and len(lst) == m * (2 if with_b else 1)
        assert int(np.diff(ptr).max(initial=0)) <= iref.MAX_DEGREE
        d_a = dev_in(dev, a, I32)
        d_b = dev_in(dev, b, I32) if with_b else None
        run_case(dev, 'rg_incidence', dict(ptr=(n + 1, I32), list=(len(lst), I32)),
                 lambda fn, o, w, wb: fn(d_a.data_ptr(), d_b.data_ptr() if with_b else None, m, n,
                                         o['ptr'].ptr, o['list'].ptr, w, wb, _stream(dev)),
                 dict(ptr=ptr, list=lst), ws_bytes=lib.rg_incidence_workspace_size(n, m))


# ------------------------------------------------------------- rg_link_pairs and rg_csr_rows
@functools.lru_cache(maxsize=None)
def _csr(n):
    return iref.symmetric_csr(n, n + 11)


@pytest.mark.parametrize('n', S)
def test_link_pairs(cuda_device, n):
    """Also below the pair count: a row whose last pair lies past pair_capacity is skipped
    whole, nothing at or past pair_capacity is written, and n_pairs is still the true count."""
    dev = cuda_device
    row_ptr, col = _csr(n)
    ptr, ps, pd = iref.link_pairs(row_ptr, col)
    U = len(ps)
    assert 2 * U == len(col)
    d_rp, d_col = dev_in(dev, row_ptr, I32), dev_in(dev, col, I32)
    for cap in sorted({U, U // 2, max(U - 1, 0)}):
        done = int(ptr[ptr <= cap].max())                 # the rows that fit are a prefix
        run_case(dev, 'rg_link_pairs',
                 dict(pair_ptr=(n + 1, I32), pair_src=(cap, I32), pair_dst=(cap, I32),
                      n_pairs=(1, I32)),
                 lambda fn, o, w, wb: fn(d_rp.data_ptr(), d_col.data_ptr(), n, o['pair_ptr'].ptr,
                                         o['pair_src'].ptr, o['pair_dst'].ptr, cap,
                                         o['n_pairs'].ptr, w, wb, _stream(dev)),
                 dict(pair_ptr=ptr, pair_src=tail_kept(ps[:done], cap),
                      pair_dst=tail_kept(pd[:done], cap), n_pairs=[U]),
                 ws_bytes=_lib().rg_link_pairs_workspace_size(n))


@pytest.mark.parametrize('n', S)
def test_csr_rows(cuda_device, n):
    dev = cuda_device
    row_ptr, col = _csr(n)
    d_rp = dev_in(dev, row_ptr, I32)
    run_case(dev, 'rg_csr_rows', dict(out=(len(col), I32)),
             lambda fn, o, w, wb: fn(d_rp.data_ptr(), n, o['out'].ptr, _stream(dev)),
             dict(out=iref.csr_rows(row_ptr)))


# ---------------------------------------------------------------------------- rg_csr_by_dst
def _random_edges(n, seed):
    E = min(200 * n, 526337)                               # in-degree stays far below 1000
    ei = np.random.default_rng(seed).integers(0, max(n, 1), (2, E)).astype(I64)
    if E > 8:
        ei[:, 1] = ei[:, 0]                                # a duplicate, and a self loop
        ei[1, 2] = ei[0, 2]
    return ei


def _csr_by_dst_case(dev, ei, n, fill_value=None):
    E = ei.shape[1]
    ptr, perm, src, dropped = iref.csr_by_dst(ei, n)
    assert int(np.diff(ptr).max(initial=0)) <= iref.MAX_DEGREE and len(perm) == E - dropped
    d_ei = dev_in(dev, ei, I64)
    tail = (lambda v: tail_kept(v, E)) if fill_value is None else (
        lambda v: np.concatenate([v, np.full(E - len(v), fill_value, I32)]))
    run_case(dev, 'rg_csr_by_dst', dict(dst_ptr=(n + 1, I32), perm=(E, I32), src_sorted=(E, I32)),
             lambda fn, o, w, wb: fn(d_ei.data_ptr(), E, n, o['dst_ptr'].ptr, o['perm'].ptr,
                                     o['src_sorted'].ptr, w, wb, _stream(dev)),
             dict(dst_ptr=ptr, perm=tail(perm), src_sorted=tail(src)),
             ws_bytes=_lib().rg_csr_by_dst_workspace_size(n, E))
    return dropped


@pytest.mark.parametrize('n', S)
def test_csr_by_dst(cuda_device, n):
    assert _csr_by_dst_case(cuda_device, _random_edges(n, n + 5), n) == 0


@pytest.mark.parametrize('n', [1, 65, 2049, 32769, 526337])
def test_csr_by_dst_drops_and_reports_out_of_range_endpoints(cuda_device, n):
    """Edges with an endpoint of -1, n_nodes or 2**40 are dropped; dst_ptr[n_nodes] reports how
    many were kept; the rest is exact; the E - dst_ptr[n_nodes] tail entries of perm and
    src_sorted are written 0."""
    ei = _random_edges(n, n + 6)
    E = ei.shape[1]
    ei[0, 0::7], ei[1, 3::11], ei[0, 5::13], ei[1, E - 1] = -1, n, 2 ** 40, -1
    dropped = _csr_by_dst_case(cuda_device, ei, n, fill_value=0)
    assert dropped > E // 8


# ----------------------------------------------------------------------------- rg_csr_clamp
def _clamp_csrs():
    small = np.array([0, 4, 4, 4, 10, 16, 16, 20], I32)
    deg = np.random.default_rng(9).integers(0, 6, 5000)   # more rows than the kernel's threads
    deg[100:1300] = 0                                      # a long run of empty rows
    return [(small, c) for c in (25, 20, 19, 12, 9, 8, 7, 1, 0)] + [
        (iref.exclusive_scan(deg), c) for c in (10 ** 6, 2 * int(deg[:100].sum()) + 1, 5000, 3)]


@pytest.mark.parametrize('case', range(len(_clamp_csrs())))
def test_csr_clamp(cuda_device, case):
    """Capacity above, equal to and below the edge count; the cut on a row boundary (8: 4), inside
    a row (19 -> 9 -> 4), in a run of empty rows, and with capacity / 2 below the first row."""
    dev = cuda_device
    row_ptr, cap = _clamp_csrs()[case]
    n, E = len(row_ptr) - 1, int(row_ptr[-1])
    want_ptr, want_e, need = iref.csr_clamp(row_ptr, E, cap)
    run_case(dev, 'rg_csr_clamp', dict(row_ptr=(n + 1, I32), n_edges=(1, I32), need=(1, I32)),
             lambda fn, o, w, wb: fn(o['row_ptr'].ptr, n, o['n_edges'].ptr, cap, o['need'].ptr,
                                     _stream(dev)),
             dict(row_ptr=want_ptr, n_edges=[want_e], need=[need]),
             init=dict(row_ptr=row_ptr, n_edges=[E]))


# ------------------------------------------------- rg_dense_pair_rows and rg_dense_pair_emit
def _dense_adjacencies(n):
    rng = np.random.default_rng(n)
    last = np.zeros((n, n), U8)
    if n:
        last[:, n - 1] = 200
    return {'empty': np.zeros((n, n), U8), 'full': np.full((n, n), 255, U8),
            'lower triangle': np.tril(np.full((n, n), 3, U8), -1), 'last column': last,
            'random bytes': rng.integers(0, 256, (n, n)).astype(U8) * (rng.random((n, n)) < 0.1)}


@pytest.mark.parametrize('n', [0, 1, 2, 63, 64, 65, 129, 2049])
def test_dense_pairs(cuda_device, n):
    dev = cuda_device
    lib = _lib()
    for pattern, adj in _dense_adjacencies(n).items():
        ptr, ps, pd = iref.dense_pairs(adj)
        U = len(ps)
        assert U == {'empty': 0, 'full': n * (n - 1) // 2, 'lower triangle': 0,
                     'last column': max(n - 1, 0)}.get(pattern, U)
        d_adj = dev_in(dev, adj, U8)
        run_case(dev, 'rg_dense_pair_rows', dict(row_ptr=(n + 1, I32), n_pairs=(1, I32)),
                 lambda fn, o, w, wb: fn(d_adj.data_ptr(), n, o['row_ptr'].ptr, o['n_pairs'].ptr,
                                         w, wb, _stream(dev)),
                 dict(row_ptr=ptr, n_pairs=[U]),
                 ws_bytes=lib.rg_dense_pair_rows_workspace_size(n))
        d_ptr = dev_in(dev, ptr, I32)
        run_case(dev, 'rg_dense_pair_emit', dict(pair_src=(U, I32), pair_dst=(U, I32)),
                 lambda fn, o, w, wb: fn(d_adj.data_ptr(), n, d_ptr.data_ptr(), o['pair_src'].ptr,
                                         o['pair_dst'].ptr, _stream(dev)),
                 dict(pair_src=ps, pair_dst=pd))


# ----------------------------------------- rg_object_complete_graph and rg_object_row_ranges
def _object_sizes(n_obj):
    """Sizes drawn from {0, 1, 2, 3}, empty objects at the front, in the middle (a run) and at
    the end, and one object of 400 members."""
    if n_obj <= 2:
        return {0: [[]], 1: [[0], [1], [400]], 2: [[0, 3], [2, 0], [400, 1]]}[n_obj]
    size = np.random.default_rng(n_obj).integers(0, 4, n_obj)
    size[0] = size[n_obj // 2:n_obj // 2 + 3] = size[-1] = 0
    size[n_obj // 3] = 400
    return [size]


@pytest.mark.parametrize('n_obj', [0, 1, 2, 2049, 32769, 524289])
def test_object_complete_graph(cuda_device, n_obj):
    """col only, edge_index only and both; and n_nodes above sum(object_size): those rows have
    no edges."""
    dev = cuda_device
    wsb = _lib().rg_object_graph_workspace_size(n_obj)
    for size in _object_sizes(n_obj):
        d_size = dev_in(dev, size, I64)
        for extra in (0, 5):
            n = int(np.sum(size, dtype=I64)) + extra
            row_ptr, col, ei = iref.object_complete_graph(size, n)
            E = len(col)
            s64 = np.asarray(size, I64)
            assert E == int((s64 * (s64 - 1)).sum())
            for with_col, with_ei in ((True, False), (False, True), (True, True))[2 * (extra > 0):]:
                outs = dict(row_ptr=(n + 1, I32))
                want = dict(row_ptr=row_ptr)
                if with_col:
                    outs['col'], want['col'] = (E, I32), col
                if with_ei:
                    outs['ei'], want['ei'] = ((2, E), I64), ei
                run_case(dev, 'rg_object_complete_graph', outs,
                         lambda fn, o, w, wb: fn(d_size.data_ptr(), n_obj, n, E, o['row_ptr'].ptr,
                                                 o['col'].ptr if with_col else None,
                                                 o['ei'].ptr if with_ei else None, w, wb,
                                                 _stream(dev)),
                         want, ws_bytes=wsb)


@pytest.mark.parametrize('n_obj', [0, 1, 2, 2049, 32769, 524289])
def test_object_row_ranges(cuda_device, n_obj):
    """One sample (NULL sample arrays), then several: an empty sample, and a sample whose first
    object is empty (the sizes' middle run of empty objects starts one)."""
    dev = cuda_device
    wsb = _lib().rg_object_graph_workspace_size(n_obj)
    for size in _object_sizes(n_obj):
        d_size = dev_in(dev, size, I64)
        cuts = sorted({0, n_obj // 5, n_obj // 2, n_obj}) if n_obj else [0, 0]
        sobj = np.array(cuts[:2] + cuts[1:], I32)          # the second sample is empty
        base = np.concatenate([[0], np.cumsum(size, dtype=I64)])[sobj[:-1]] + 7
        assert n_obj < 3 or size[sobj[-2]] == 0
        d_sobj, d_base = dev_in(dev, sobj, I32), dev_in(dev, base, I32)
        for samples in (False, True):
            begin, end = iref.object_row_ranges(size, *((sobj, base) if samples else ()))
            run_case(dev, 'rg_object_row_ranges', dict(begin=(n_obj, I32), end=(n_obj, I32)),
                     lambda fn, o, w, wb: fn(d_size.data_ptr(), n_obj,
                                             d_sobj.data_ptr() if samples else None,
                                             d_base.data_ptr() if samples else None,
                                             len(sobj) - 1 if samples else 0, o['begin'].ptr,
                                             o['end'].ptr, w, wb, _stream(dev)),
                     dict(begin=begin, end=end), ws_bytes=wsb)


# -------------------------------------------------------------------------- rg_cluster_lists
@pytest.mark.parametrize('N', [1, 2, 127, 128, 255, 2047, 2048, 32767, 32768, 32769, 526337])
def test_cluster_lists(cuda_device, N):
    """cluster_ptr is exactly N + 1 ints (at N = 127, 255 and 2047 it ends on a 512-B boundary,
    where an allocator's rounding hides nothing): entries past n_clusters repeat N."""
    dev = cuda_device
    wsb = _lib().rg_cluster_lists_workspace_size(N)
    for labels in (np.arange(N, dtype=I32), np.zeros(N, I32), iref.random_labels(N, N)):
        of, ptr, idx, ncl = iref.cluster_lists(labels)
        assert len(ptr) == N + 1 and (ptr[ncl:] == N).all()
        d_lab = dev_in(dev, labels, I32)
        run_case(dev, 'rg_cluster_lists',
                 dict(cluster_of=(N, I32), cluster_ptr=(N + 1, I32), cluster_idx=(N, I32),
                      n_clusters=(1, I32)),
                 lambda fn, o, w, wb: fn(d_lab.data_ptr(), N, o['cluster_of'].ptr,
                                         o['cluster_ptr'].ptr, o['cluster_idx'].ptr,
                                         o['n_clusters'].ptr, w, wb, _stream(dev)),
                 dict(cluster_of=of, cluster_ptr=ptr, cluster_idx=idx, n_clusters=[ncl]),
                 ws_bytes=wsb)


# ------------------------------------------------------------------------- the small kernels
ROWS = (0, 1, 255, 256, 257)
WIDTHS = (1, 3, 64, 65)


@pytest.mark.parametrize('n_sorted', ROWS)
def test_lower_bound(cuda_device, n_sorted):
    """Queries below, equal to, between and above the sorted values (with duplicates); the
    length from the device (smaller than n_sorted, equal to it) or from the argument."""
    dev = cuda_device
    rng = np.random.default_rng(n_sorted)
    srt = np.sort(rng.integers(0, 60, n_sorted) * 3).astype(I32)     # multiples of 3, repeated
    d_srt = dev_in(dev, srt, I32)
    for nq in ROWS:
        q = rng.integers(-3, 185, nq).astype(I32)
        q[:4] = np.array([-5, 0, 178, 1000], I32)[:nq]
        d_q = dev_in(dev, q, I32)
        for n_dev in (None, n_sorted, n_sorted // 2, n_sorted + 9):   # the last: capped
            d_n = dev_in(dev, [n_dev], I32) if n_dev is not None else None
            n_used = n_sorted if n_dev is None else min(n_dev, n_sorted)
            run_case(dev, 'rg_lower_bound_i32', dict(out=(nq, I32)),
                     lambda fn, o, w, wb: fn(d_srt.data_ptr(), d_n.data_ptr() if d_n is not None
                                             else None, n_sorted, d_q.data_ptr(), nq, o['out'].ptr,
                                             _stream(dev)),
                     dict(out=iref.lower_bound(srt, n_used, q)))


@pytest.mark.parametrize('n', ROWS)
def test_gather_i32_and_i32_to_i64(cuda_device, n):
    dev = cuda_device
    rng = np.random.default_rng(n + 3)
    table = rng.integers(-2 ** 31, 2 ** 31, 300).astype(I32)
    idx = rng.integers(0, 300, n).astype(I32)
    d_t, d_i = dev_in(dev, table, I32), dev_in(dev, idx, I32)
    run_case(dev, 'rg_gather_i32', dict(out=(n, I32)),
             lambda fn, o, w, wb: fn(d_t.data_ptr(), d_i.data_ptr(), n, o['out'].ptr, _stream(dev)),
             dict(out=iref.gather(table, idx)))
    vals = table[:n].copy()
    vals[:2] = np.array([-2 ** 31, 2 ** 31 - 1], I32)[:n]
    d_v = dev_in(dev, vals, I32)
    run_case(dev, 'rg_i32_to_i64', dict(out=(n, I64)),
             lambda fn, o, w, wb: fn(d_v.data_ptr(), n, o['out'].ptr, _stream(dev)),
             dict(out=iref.i32_to_i64(vals)))


@pytest.mark.parametrize('w', WIDTHS)
@pytest.mark.parametrize('rows', ROWS)
def test_gather_rows_and_pair_add_rows(cuda_device, rows, w):
    """rg_gather_rows_f32 (dense rows) and rg_pair_add_rows_f32 into a window of a wider
    output (ld_out = w + 3): the three columns beside the window keep the sentinel."""
    dev = cuda_device
    rng = np.random.default_rng(rows * 100 + w)
    x = rng.standard_normal((90, w + 2)).astype(F32)
    i0, i1 = (rng.integers(0, 90, rows).astype(I32) for _ in range(2))
    d_i0, d_i1 = dev_in(dev, i0, I32), dev_in(dev, i1, I32)
    xc = np.ascontiguousarray(x[:, :w])
    d_xc, d_x = dev_in(dev, xc, F32), dev_in(dev, x, F32)
    run_case(dev, 'rg_gather_rows_f32', dict(out=((rows, w), F32)),
             lambda fn, o, ws, wb: fn(d_xc.data_ptr(), d_i0.data_ptr(), rows, w, o['out'].ptr,
                                      _stream(dev)),
             dict(out=iref.gather(xc, i0)))
    want = sent((rows, w + 3), F32)
    want[:, :w] = iref.pair_add_rows(x, w, i0, i1)
    run_case(dev, 'rg_pair_add_rows_f32', dict(out=((rows, w + 3), F32)),
             lambda fn, o, ws, wb: fn(d_x.data_ptr(), w + 2, w, d_i0.data_ptr(), d_i1.data_ptr(),
                                      rows, o['out'].ptr, w + 3, _stream(dev)),
             dict(out=want))


# ------------------------------------------------------------- DeviceGraph.from_edge_index
def _graph_edges():
    rng = np.random.default_rng(60000)
    ei = rng.integers(0, 60000, (2, 526337)).astype(I64)  # 258 scan tiles: the carry loop
    ei[:, 1] = ei[:, 0]
    ei[1, 2] = ei[0, 2]
    return ei


def test_from_edge_index_on_the_edge_scans_carry_path(cuda_device):
    from graph_neural_network_for_radar_perception_amd import engine
    dev = cuda_device
    n, ei = 60000, _graph_edges()
    g = engine.DeviceGraph.from_edge_index(torch.from_numpy(ei).to(dev), n)
    ptr, perm, src, dropped = iref.csr_by_dst(ei, n)
    ps, pd = iref.pairs_from_edge_index(ei)
    E = ei.shape[1]
    assert dropped == 0 and g.n_edges == E and g.n_pairs == len(ps) and g.n_nodes == n
    assert int(g.n_pairs_dev.item()) == len(ps)
    for name, got, want in (('seg_ptr', g.seg_ptr, ptr), ('perm', g.perm[:E], perm),
                            ('src', g.src[:E], src), ('dst', g.dst[:E], iref.csr_rows(ptr)),
                            ('pair_src', g.pair_src[:len(ps)], ps),
                            ('pair_dst', g.pair_dst[:len(pd)], pd)):
        _same(got.cpu().numpy(), want, name)


def test_from_edge_index_raises_for_out_of_range_endpoints(cuda_device):
    """The reference (index_select) raises for such an edge_index.  With count_pairs the build
    raises IndexError, naming the bound, in the host read of the pair count; without, the build
    stays free of host reads, the count stays on the graph as a device tensor, the tails of
    perm / src / dst are written, and the graph's first host read raises."""
    from graph_neural_network_for_radar_perception_amd import engine
    dev = cuda_device
    n = 60000
    for bad in (-1, n, 2 ** 40):
        ei = np.ascontiguousarray(_graph_edges()[:, :40000])
        ei[0, 5], ei[1, 39999] = bad, bad
        d_ei = torch.from_numpy(ei).to(dev)
        with pytest.raises(IndexError, match=r'\[0, 60000\)'):
            engine.DeviceGraph.from_edge_index(d_ei, n)
        g = engine.DeviceGraph.from_edge_index(d_ei, n, count_pairs=False)
        ptr, perm, src, dropped = iref.csr_by_dst(ei, n)
        assert dropped == 2 and g.n_pairs is None
        assert torch.is_tensor(g.n_kept_dev) and g.n_kept_dev.is_cuda
        assert int(g.n_kept_dev.item()) == ei.shape[1] - 2 == int(g.seg_ptr[n].item())
        for name, got, want in (('seg_ptr', g.seg_ptr, ptr), ('perm', g.perm, perm),
                                ('src', g.src, src), ('dst', g.dst, iref.csr_rows(ptr))):
            _same(got.cpu().numpy(), np.concatenate([want, np.zeros(len(got) - len(want), I32)]),
                  name)
        for _ in range(2):                                 # it does not pass on a second look
            with pytest.raises(IndexError, match=r'\[0, 60000\)'):
                g.pair_count()
    g = engine.DeviceGraph.from_edge_index(torch.from_numpy(_graph_edges()[:, :40000]).to(dev), n,
                                           count_pairs=False)
    assert g.n_pairs is None
    assert g.pair_count() == len(iref.pairs_from_edge_index(_graph_edges()[:, :40000])[0])
    assert g.n_pairs == g.pair_count()
