"""The training step's small kernels, each alone against an independent high-precision reference
(tests/train_kernels_ref.py, checked on the CPU by tests/test_train_kernels_host.py):
rg_ffn_backward(_gather), rg_segment_max_backward, rg_range_max_backward(_ordered),
rg_segment_amax_backward, rg_loss_graph(_backward), rg_cross_entropy(_backward) and
rg_object_focal_loss(_backward).

Every entry is launched directly through _native.lib().  Every output is a window of a larger
sentinel-filled allocation: padding columns (ld > C) where the entry takes a stride, and rows
before and after, all checked unchanged after the call.  Inputs are padded with the sentinel too.

Bounds are train_kernels_ref's: bit equality for the max-pool routings (small-integer gradients:
every sum is exact in any order, atomics included), 4 err32 + 2^-22 max|ref| for float32
arithmetic against float64, the project's bounds for the norm parameter gradients and the loss
values, 2 float32 ulp for the kernels that compute in float64.  With $RG_KERNEL_ERROR_REPORT set
every toleranced comparison appends one JSON line (profiles/train_kernels_error_ratio.jsonl is the
MI355X run)."""
import ctypes

import numpy as np
import pytest
import torch

import train_kernels_ref as R

pytestmark = pytest.mark.gpu

F32, F64, I32, I64 = np.float32, np.float64, np.int32, np.int64
SENT_BITS = np.array([0xA5A5A5A5], np.uint32).view(I32)[0]
SENT = np.array([SENT_BITS], I32).view(F32)[0]


def _nat():
    from graph_neural_network_for_radar_perception_amd import _native as nat
    return nat


def _st(dev):
    return torch.cuda.current_stream(dev).cuda_stream


class Buf:
    """float32 [rows][ld] on the device with C live columns, between guard rows (>= 64 floats
    before and after); everything but the live window holds the sentinel, the window `init`."""

    def __init__(self, dev, rows, C, ld=None, init=None):
        ld = C if ld is None else ld
        self.rows, self.C, self.ld = rows, C, ld
        self.pad = max(2, -(-64 // ld))
        host = np.full((rows + 2 * self.pad, ld), SENT, F32)
        if init is not None:
            host[self.pad:self.pad + rows, :C] = np.asarray(init, F32).reshape(rows, C)
        self.before = host.copy()
        self.t = torch.from_numpy(host).to(dev)
        self.ptr = self.t.data_ptr() + self.pad * ld * 4

    def read(self, what):
        """The live window, after checking that nothing around it changed."""
        h = self.t.cpu().numpy()
        out = h[self.pad:self.pad + self.rows, :self.C].copy()
        h = h.copy()
        h[self.pad:self.pad + self.rows, :self.C] = SENT
        bad = np.argwhere(h.view(I32) != SENT_BITS)
        assert bad.size == 0, (f'{what}: written outside its window at (row, column) '
                               f'{(bad[:4] - [self.pad, 0]).tolist()}')
        return out

    def untouched(self, what):
        assert R.same_bits(self.t.cpu().numpy(), self.before), f'{what}: written'


def dev_mat(dev, x, ld=None, dtype=F32):
    """An input [rows][ld] with sentinel padding columns and one spare row."""
    x = np.asarray(x, dtype)
    x = x[:, None] if x.ndim == 1 else x
    ld = x.shape[1] if ld is None else ld
    host = np.full((x.shape[0] + 1, ld), SENT if dtype == F32 else 0, dtype)
    host[:x.shape[0], :x.shape[1]] = x
    return torch.from_numpy(host).to(dev)


def dev_vec(dev, x, dtype):
    x = np.asarray(x, dtype).reshape(-1)
    return torch.from_numpy(np.concatenate([x, np.zeros(1, dtype)])).to(dev)


def _check_f32(kernel, case, tensor, got, ref64, ref32):
    ok, err, err32, b = R.within_f32_bound(got, ref64, ref32)
    R.record(kernel, case, tensor, err, err32, b)
    print(f'{kernel} {case} {tensor}: err {err:.3e} err32 {err32:.3e} bound {b:.3e}')
    assert ok, (kernel, case, tensor, err, err32, b)


def _check_abs(kernel, case, tensor, got, ref, bound, err32=0.0):
    err = abs(float(got) - float(ref))
    err = float('inf') if not np.isfinite(err) else err
    R.record(kernel, case, tensor, err, err32, bound)
    print(f'{kernel} {case} {tensor}: err {err:.3e} err32 {err32:.3e} bound {bound:.3e}')
    assert err <= bound, (kernel, case, tensor, float(got), float(ref), err, bound)


# -------------------------------------------------------- 1. rg_ffn_backward(_gather)
def _ffn_call(dev, z, da, act, has_norm, gidx=None, gscale=None, inplace=False, params=True,
              entry=None):
    """One launch (twice: the second must be bit-identical).  z [rows][C], da [rows or n_src][C]
    torch float32 on the host.  Returns dz and the accumulated (d_mu, d_std)."""
    nat = _nat()
    lib = nat.lib()
    rows, C = z.shape
    zin = dev_mat(dev, z.numpy(), C + 3)
    d_gidx = dev_vec(dev, gidx, I32) if gidx is not None else None
    d_gsc = dev_vec(dev, gscale, F32) if gscale is not None else None
    mu, sd = torch.tensor([R.FFN_M], device=dev), torch.tensor([R.FFN_S], device=dev)
    wsb = lib.rg_ffn_backward_workspace_size()
    gather = gidx is not None or entry == 'gather'
    outs = []
    for _ in range(2):
        ws = Buf(dev, 1, wsb // 4)
        dmu, dsd = Buf(dev, 1, 1, init=[R.FFN_PRE_MU]), Buf(dev, 1, 1, init=[R.FFN_PRE_STD])
        if inplace:
            dz = Buf(dev, rows, C, C + 1, init=da.numpy())
            da_ptr, ldda = dz.ptr, C + 1
        else:
            dz = Buf(dev, rows, C, C + 2)
            dain = dev_mat(dev, da.numpy(), C + 1)
            da_ptr, ldda = dain.data_ptr(), C + 1
        pm = (mu.data_ptr(), sd.data_ptr()) if (has_norm or params) else (None, None)
        pg = (dmu.ptr, dsd.ptr) if params else (None, None)
        head = (zin.data_ptr(), C + 3, da_ptr, ldda)
        tail = (rows, C, int(has_norm), pm[0], pm[1], nat.ACT[act], dz.ptr, dz.ld, pg[0], pg[1],
                ws.ptr, _st(dev))
        if gather:
            rc = lib.rg_ffn_backward_gather(*head, nat.ptr(d_gidx), nat.ptr(d_gsc), *tail)
        else:
            rc = lib.rg_ffn_backward(*head, *tail)
        nat.check(rc, 'rg_ffn_backward')
        torch.cuda.synchronize(dev)
        ws.read('workspace')
        outs.append((dz.read('dz'), float(dmu.read('d_mu')[0, 0]), float(dsd.read('d_std')[0, 0])))
    assert R.same_bits(outs[0][0], outs[1][0]) and outs[0][1:] == outs[1][1:], 'second call differs'
    return outs[0]


def _ffn_norm_check(kernel, case, got, z, da, act):
    dz, d_mu, d_std = got
    r64 = R.ffn_reference(z, da, act, torch.float64)
    r32 = R.ffn_reference(z, da, act, torch.float32)
    mask = R.kink_rows(r64['y'], act)
    assert R.kink_cap_ok(mask)
    keep = ~mask
    _check_f32(kernel, case, 'dz', dz[keep], r64['dz'][keep], r32['dz'][keep])
    extra = R.kink_extra(mask, da.numpy(), r64['n'])
    for name, val, pre in (('d_std', d_std, R.FFN_PRE_STD), ('d_mu', d_mu, R.FFN_PRE_MU)):
        ref = pre + r64[name]
        e32 = abs(float(F32(F32(pre) + F32(r32[name]))) - ref)
        _check_abs(kernel, case, name, val, ref, R.param_bound(r64['gy'], r64['n'], ref, extra), e32)


@pytest.mark.parametrize('C,act', R.FFN_NORM_CASES)
def test_ffn_backward_norm_matches_float64(cuda_device, C, act):
    """has_norm = 1 on both sides of every template switch (J = 1, 4, 8, 16 at C = 16 / 64 / 128)
    and a partial 16-lane group, rows {1, 3, 515}, ldz = C + 3, ldda = C + 1, lddz = C + 2,
    d_mu / d_std preloaded with 0.25 / -0.5, the second call bit-identical.  Rows whose float64
    |y| < 1e-5 at a leakyrelu / relu kink are left out of dz (the float32 y may take the other
    sign) and widen the parameter-gradient bound by their sum|da n| + sum|da|."""
    for rows in R.FFN_ROWS:
        z, da = R.ffn_inputs(C, rows, act)
        got = _ffn_call(cuda_device, z, da, act, True)
        _ffn_norm_check('rg_ffn_backward', f'C={C} {act} rows={rows}', got, z, da, act)


@pytest.mark.parametrize('C,act', R.FFN_LONG_CASES)
def test_ffn_backward_second_trip_of_the_row_loop(cuda_device, C, act):
    """32 773 rows = 2048 workgroups x 16 rows + 5."""
    z, da = R.ffn_inputs(C, R.FFN_LONG_ROWS, act)
    got = _ffn_call(cuda_device, z, da, act, True)
    _ffn_norm_check('rg_ffn_backward', f'C={C} {act} rows={R.FFN_LONG_ROWS}', got, z, da, act)


def test_ffn_backward_in_place_equals_out_of_place(cuda_device):
    z, da = R.ffn_inputs(64, 515)
    a = _ffn_call(cuda_device, z, da, 'leakyrelu', True)
    b = _ffn_call(cuda_device, z, da, 'leakyrelu', True, inplace=True)
    assert R.same_bits(a[0], b[0]) and a[1:] == b[1:]


@pytest.mark.parametrize('C', R.FFN_PLAIN_C)
@pytest.mark.parametrize('act', R.ACTS)
def test_ffn_backward_without_norm(cuda_device, C, act):
    """dz = da act'(z) on the stored float32 z: none / relu / leakyrelu bit-equal to the numpy
    float32 product, swish within the shared bound; d_mu / d_std null, and untouched where given."""
    for rows in R.FFN_ROWS:
        z, da = R.ffn_inputs(C, rows, act)
        for params in (False, True):
            dz, d_mu, d_std = _ffn_call(cuda_device, z, da, act, False, params=params)
            assert (d_mu, d_std) == (float(F32(R.FFN_PRE_MU)), float(F32(R.FFN_PRE_STD)))
            if act == 'swish':
                r64 = R.ffn_reference(z, da, act, torch.float64, has_norm=False)
                r32 = R.ffn_reference(z, da, act, torch.float32, has_norm=False)
                _check_f32('rg_ffn_backward', f'no norm C={C} swish rows={rows}', 'dz', dz,
                           r64['dz'], r32['dz'])
            else:
                assert R.same_bits(dz, da.numpy() * R.act_grad_f32(z.numpy(), act)), (rows, params)


@pytest.mark.parametrize('scaled', [False, True], ids=['gidx', 'gidx+gscale'])
def test_ffn_backward_gather_matches_float64(cuda_device, scaled):
    """C = 65, 515 rows, gidx with repeats and unused rows: against float64 of
    float32(da[gidx] * gscale[gidx])."""
    C, rows, n_src = 65, 515, 400
    z, _ = R.ffn_inputs(C, rows)
    _, da = R.ffn_inputs(C, n_src)
    gidx, gscale = R.gather_inputs(n_src, rows, 5)
    got = _ffn_call(cuda_device, z, da, 'leakyrelu', True, gidx=gidx,
                    gscale=gscale if scaled else None)
    eff = da.numpy()[gidx]
    if scaled:
        eff = (eff * gscale[gidx][:, None]).astype(F32)
    _ffn_norm_check('rg_ffn_backward_gather', f'C=65 rows=515 scaled={scaled}', got, z,
                    torch.from_numpy(np.ascontiguousarray(eff)), 'leakyrelu')


@pytest.mark.parametrize('C', [2, 5, 64])
def test_ffn_backward_degenerate_row(cuda_device, C):
    """A constant row (std = 0; at C = 2: z0 == z1) in the middle of ordinary rows.  torch's
    autograd on the CPU gives NaN for every entry of that row's dz, and through it for d_std and
    d_mu (sqrt'(0) = inf meets a zero; test_train_kernels_host.py asserts it).  The kernel's
    stated convention is coef = 0: n = 0, y = mu, dz = r gn - mean(r gn) with r = 1 / eps.  The
    neighbouring rows are those of the case without the constant row, d_mu / d_std finite and
    the sums over the other rows plus the row's sum(gy) in d_mu."""
    z, da, row = R.degenerate_inputs(C)
    dz, d_mu, d_std = _ffn_call(cuda_device, z, da, 'leakyrelu', True)
    want, bound = R.degenerate_convention(da[row].numpy(), C)
    err = R.max_err(dz[row], want)
    R.record('rg_ffn_backward', f'constant row C={C}', 'dz', err, 0.0, bound)
    assert err <= bound, (err, bound)
    others = np.arange(z.shape[0]) != row
    zo, dao = z[others], da[others]
    r64 = R.ffn_reference(zo, dao, 'leakyrelu', torch.float64)
    r32 = R.ffn_reference(zo, dao, 'leakyrelu', torch.float32)
    assert not R.kink_rows(r64['y'], 'leakyrelu').any()
    _check_f32('rg_ffn_backward', f'beside a constant row C={C}', 'dz', dz[others], r64['dz'],
               r32['dz'])
    assert np.isfinite(d_mu) and np.isfinite(d_std)
    gy_row = da[row].double().numpy()                      # act'(mu = 0.2) = 1
    gy = np.concatenate([r64['gy'], gy_row[None]])
    n = np.concatenate([r64['n'], np.zeros((1, C))])
    for name, val, ref in (('d_std', d_std, R.FFN_PRE_STD + r64['d_std']),
                           ('d_mu', d_mu, R.FFN_PRE_MU + r64['d_mu'] + gy_row.sum())):
        _check_abs('rg_ffn_backward', f'constant row C={C}', name, val, ref,
                   R.param_bound(gy, n, ref))


def test_ffn_backward_refusals(cuda_device):
    nat = _nat()
    lib = nat.lib()
    dev = cuda_device
    zin, dain = dev_mat(dev, np.zeros((8, 260), F32)), dev_mat(dev, np.zeros((8, 260), F32))
    mu, sd = torch.tensor([R.FFN_M], device=dev), torch.tensor([R.FFN_S], device=dev)
    ws = Buf(dev, 1, lib.rg_ffn_backward_workspace_size() // 4)
    for C, has_norm, act in ((0, 0, 2), (257, 1, 2), (257, 0, 2), (1, 1, 2), (4, 1, 4), (4, 0, -1)):
        dz, dmu, dsd = Buf(dev, 8, 260), Buf(dev, 1, 1, init=[0.0]), Buf(dev, 1, 1, init=[0.0])
        rc = lib.rg_ffn_backward(zin.data_ptr(), 260, dain.data_ptr(), 260, 8, C, has_norm,
                                 mu.data_ptr(), sd.data_ptr(), act, dz.ptr, 260, dmu.ptr, dsd.ptr,
                                 ws.ptr, _st(dev))
        torch.cuda.synchronize(dev)
        assert rc != 0, (C, has_norm, act)
        for b in (dz, dmu, dsd):
            b.untouched(f'refused C={C} has_norm={has_norm} act={act}')


# ------------------------------------------------------------ 2. rg_segment_max_backward
@pytest.mark.parametrize('C', R.SEGMAX_C)
def test_segment_max_backward_routes_to_the_first_maximum(cuda_device, C):
    """300 nodes, h quantised to multiples of 0.5 (ties are common) with NaN (wins, the first of
    several) and -inf entries; clusters of {0, 1, 2, 37, 300} members and three that share nodes;
    ld_h = C + 3, ld_p = C + 1, ld_dh = C + 2; integer dp added to an integer preload: bit-equal
    to the numpy loop, atomics included.  n_clusters = 0 is a no-op."""
    dev = cuda_device
    lib = _nat().lib()
    h, cptr, cidx, dp, dh0 = R.segment_max_case(C)
    want = R.segment_max_backward_ref(h, cptr, cidx, dp, dh0).astype(F32)
    d_h, d_dp = dev_mat(dev, h, C + 3), dev_mat(dev, dp, C + 1)
    d_ptr, d_idx = dev_vec(dev, cptr, I32), dev_vec(dev, cidx, I32)
    for n_cl in (len(cptr) - 1, 0):
        dh = Buf(dev, h.shape[0], C, C + 2, init=dh0)
        rc = lib.rg_segment_max_backward(d_h.data_ptr(), C + 3, C, d_ptr.data_ptr(),
                                         d_idx.data_ptr(), n_cl, d_dp.data_ptr(), C + 1, dh.ptr,
                                         C + 2, _st(dev))
        torch.cuda.synchronize(dev)
        assert rc == 0
        got = dh.read('dh')
        assert R.same_bits(got, want if n_cl else dh0), np.argwhere(got != (want if n_cl else dh0))[:4]
    R.record('rg_segment_max_backward', f'C={C}', 'dh', 0.0, 0.0, 0.0)


# ------------------------------------- 3. rg_range_max_backward and rg_range_max_backward_ordered
def _range_call(dev, ordered, x_d, ldx, C, b_d, e_d, n_obj, dp_d, ldp, dx, ws_short=False):
    lib = _nat().lib()
    if not ordered:
        rc = lib.rg_range_max_backward(x_d.data_ptr(), ldx, C, b_d.data_ptr(), e_d.data_ptr(),
                                       n_obj, dp_d.data_ptr(), ldp, dx.ptr, dx.ld, _st(dev))
        torch.cuda.synchronize(dev)
        return rc
    wsb = lib.rg_range_max_backward_ordered_workspace_size(n_obj, C)
    assert wsb % 4 == 0
    ws = Buf(dev, 1, max(wsb // 4, 1))
    rc = lib.rg_range_max_backward_ordered(x_d.data_ptr(), ldx, C, b_d.data_ptr(), e_d.data_ptr(),
                                           n_obj, dp_d.data_ptr(), ldp, dx.ptr, dx.ld, ws.ptr,
                                           wsb - 1 if ws_short else wsb, _st(dev))
    torch.cuda.synchronize(dev)
    if ws_short:
        ws.untouched('short workspace')
    else:
        ws.read('workspace')
    return rc


@pytest.mark.parametrize('C', R.RANGE_C)
@pytest.mark.parametrize('n_obj', R.RANGE_NOBJ)
def test_range_max_backward_routes_to_the_first_maximum(cuda_device, n_obj, C):
    """Both entry points bit-equal to the numpy loop (so to each other): ranges all from row 0
    with growing ends, the same with empty ranges (b == e, b > e) inside the run, nested /
    disjoint / single-row / empty ranges in turn, and all empty; n_obj around the scatter's
    U = 8 unroll, C around its 64-thread blocks; ldx = C + 3, ldp = C + 1, lddx = C + 2, integer
    d_pooled added to an integer preload.  A workspace one byte short is refused."""
    dev = cuda_device
    x, dp, dx0 = R.range_case(n_obj, C)
    d_x, d_dp = dev_mat(dev, x, C + 3), dev_mat(dev, dp, C + 1)
    for name, (b, e) in R.range_layouts(n_obj).items():
        want = R.range_max_backward_ref(x, b, e, dp, dx0).astype(F32)
        if name == 'all empty':
            assert R.same_bits(want, dx0)
        d_b, d_e = dev_vec(dev, b, I32), dev_vec(dev, e, I32)
        for ordered in (False, True):
            dx = Buf(dev, x.shape[0], C, C + 2, init=dx0)
            assert _range_call(dev, ordered, d_x, C + 3, C, d_b, d_e, n_obj, d_dp, C + 1, dx) == 0
            got = dx.read('dx')
            assert R.same_bits(got, want), (name, ordered, np.argwhere(got != want)[:4].tolist())
        dx = Buf(dev, x.shape[0], C, C + 2, init=dx0)
        assert _range_call(dev, True, d_x, C + 3, C, d_b, d_e, n_obj, d_dp, C + 1, dx,
                           ws_short=True) != 0
        dx.untouched('short workspace: dx')
    R.record('rg_range_max_backward(_ordered)', f'n_obj={n_obj} C={C}', 'dx', 0.0, 0.0, 0.0)


def test_range_max_backward_float_gradients_and_no_objects(cuda_device):
    """randn d_pooled into a zero dx: each entry is a sum of at most n_obj routed terms, within
    (n_obj - 1) 2^-24 sum|terms| of the float64 sum; two runs of the ordered entry bit-identical.
    n_obj = 0 is a no-op for both."""
    dev = cuda_device
    n_obj, C = 17, 65
    x, _, _ = R.range_case(n_obj, C)
    dp = np.random.default_rng(4).standard_normal((n_obj, C)).astype(F32)
    d_x, d_dp = dev_mat(dev, x, C + 3), dev_mat(dev, dp, C + 1)
    zero = np.zeros(x.shape, F32)
    for name, (b, e) in R.range_layouts(n_obj).items():
        ref = R.range_max_backward_ref(x, b, e, dp, zero)
        bound = (n_obj - 1) * 2.0 ** -24 * R.range_max_backward_ref(x, b, e, dp, zero, absolute=True)
        d_b, d_e = dev_vec(dev, b, I32), dev_vec(dev, e, I32)
        runs = []
        for ordered in (False, True, True):
            dx = Buf(dev, x.shape[0], C, C + 2, init=zero)
            assert _range_call(dev, ordered, d_x, C + 3, C, d_b, d_e, n_obj, d_dp, C + 1, dx) == 0
            runs.append(dx.read('dx'))
            err = np.abs(runs[-1].astype(F64) - ref)
            assert (err <= bound).all(), (name, ordered, float((err - bound).max()))
            R.record('rg_range_max_backward' + ('_ordered' if ordered else ''), f'randn {name}',
                     'dx', float(err.max()), 0.0, float(bound.max()))
        assert R.same_bits(runs[1], runs[2])
    rng = np.random.default_rng(5)
    dx0 = R.small_ints(rng, x.shape)
    d_b, d_e = dev_vec(dev, [0], I32), dev_vec(dev, [5], I32)
    for ordered in (False, True):
        dx = Buf(dev, x.shape[0], C, C + 2, init=dx0)
        assert _range_call(dev, ordered, d_x, C + 3, C, d_b, d_e, 0, d_dp, C + 1, dx) == 0
        assert R.same_bits(dx.read('dx'), dx0)


# ----------------------------------------------------------- 4. rg_segment_amax_backward
@pytest.mark.parametrize('C', R.AMAX_C)
def test_segment_amax_backward_shares_among_ties(cuda_device, C):
    """Finite quantised messages, segment sizes {0, 1, 2, 40}, ldm = C + 3, ldd = C + 1,
    ldo = C + 2: the messages equal to the maximum get float32(d_agg) / float32(cnt), one
    correctly rounded division, every other message +0.0 -- bit-equal to numpy float32.  (A NaN
    message is not a case: torch's amax propagates it, the kernel's comparisons skip it.)"""
    dev = cuda_device
    lib = _nat().lib()
    msg, seg_ptr, d_agg = R.amax_case(C)
    want = R.segment_amax_backward_ref(msg, seg_ptr, d_agg)
    d_m, d_g = dev_mat(dev, msg, C + 3), dev_mat(dev, d_agg, C + 1)
    d_ptr = dev_vec(dev, seg_ptr, I32)
    for n_seg in (len(seg_ptr) - 1, 0):
        out = Buf(dev, msg.shape[0], C, C + 2)
        rc = lib.rg_segment_amax_backward(d_m.data_ptr(), C + 3, C, d_ptr.data_ptr(), n_seg,
                                          d_g.data_ptr(), C + 1, out.ptr, C + 2, _st(dev))
        torch.cuda.synchronize(dev)
        assert rc == 0
        if n_seg:
            got = out.read('d_msg')
            assert R.same_bits(got, want), np.argwhere(got.view(I32) != want.view(I32))[:4].tolist()
        else:
            out.untouched('n_seg = 0')
    R.record('rg_segment_amax_backward', f'C={C}', 'd_msg', 0.0, 0.0, 0.0)


# ------------------------------------------------- 5. rg_loss_graph / rg_loss_graph_backward
def _loss_args(dev, case, keep):
    nat = _nat()
    a = nat.rg_loss_args()
    t = {k: dev_mat(dev, case[k].numpy()) for k in ('node_cls', 'node_reg', 'link', 'obj',
                                                      'node_offsets')}
    t.update({k: dev_vec(dev, case[k].numpy(), I64) for k in ('node_class', 'edge_class',
                                                              'obj_class')})
    t['class_w'] = dev_vec(dev, case['class_w'].numpy(), F32)
    keep.append(t)
    for k, v in t.items():
        setattr(a, k, v.data_ptr())
    a.n_nodes, a.n_pairs, a.n_clusters = (case[k].shape[0] for k in ('node_cls', 'link', 'obj'))
    a.n_classes = case['node_cls'].shape[1]
    a.mu_x, a.mu_y, a.sigma_x, a.sigma_y = case['mu_sigma']
    a.w_node_cls, a.w_node_reg, a.w_edge_cls, a.w_obj_cls = case['weights']
    return a


def _loss_run(dev, case, g):
    nat = _nat()
    lib = nat.lib()
    keep = []
    a = _loss_args(dev, case, keep)
    wsb = lib.rg_loss_workspace_size(a.n_nodes, a.n_pairs, a.n_clusters)
    ws, losses, acc = Buf(dev, 1, wsb // 4), Buf(dev, 1, 4, 6), Buf(dev, 1, 3, 5)
    nat.check(lib.rg_loss_graph(ctypes.byref(a), losses.ptr, acc.ptr, ws.ptr, wsb, _st(dev)),
              'rg_loss_graph')
    d_g = dev_vec(dev, g, F32)
    d = {k: Buf(dev, *case[k].shape) for k in ('node_cls', 'node_reg', 'link', 'obj')}
    nat.check(lib.rg_loss_graph_backward(ctypes.byref(a), d_g.data_ptr(), d['node_cls'].ptr,
                                         d['node_reg'].ptr, d['link'].ptr, d['obj'].ptr,
                                         _st(dev)), 'rg_loss_graph_backward')
    torch.cuda.synchronize(dev)
    ws.read('workspace')
    if case['obj'].shape[0] == 0:
        d['obj'].untouched('d_obj of a term with no rows')
    return losses.read('losses')[0], acc.read('acc')[0], {k: v.read('d_' + k) for k, v in d.items()}


def _loss_check(dev, case, g):
    name = f"{case['name']} g={tuple(g)}"
    losses, acc, grads = _loss_run(dev, case, g)
    ref_l, ref_g = R.loss_graph_reference(case, torch.float64, g)
    l32, g32 = R.loss_graph_reference(case, torch.float32, g)
    for i, term in enumerate(('node_cls', 'node_reg', 'edge_cls', 'obj_cls')):
        if np.isnan(ref_l[i]):
            assert np.isnan(losses[i]), (term, losses[i])
        else:
            _check_abs('rg_loss_graph', name, 'loss_' + term, losses[i], ref_l[i],
                       R.loss_bound(ref_l[i]), abs(l32[i] - ref_l[i]))
    for got, want in zip(acc, R.accuracies(case)):
        assert (np.isnan(got) and np.isnan(want)) or got == F32(want), (name, acc)
    for (k, v), gi in zip(grads.items(), g):
        assert np.isfinite(v).all(), k
        if gi == 0.0:
            assert (v == 0).all(), f'{k}: upstream gradient 0'
        _check_f32('rg_loss_graph_backward', name, 'd_' + k, v, ref_g[k], g32[k])


@pytest.mark.parametrize('case', R.loss_cases(), ids=lambda c: c['name'])
def test_loss_graph_matches_float64(cuda_device, case):
    """Four distinct loss weights, non-uniform class weights, mu / sigma = (0.4, -1.1, 2.5, 0.7),
    upstream gradient (0.3, -1.7, 2.0, 0.0) (the term with g = 0: gradient exactly zero) and the
    same reversed.  Cases: the second trip of the forward (pairs) and backward (nodes, pairs)
    grid-stride loops; link logits on the saturation grid squared with node / object rows scaled
    up to 1e4 (everything finite); n_classes 1, 2, 7, 64; exact ties (the first maximum, a link
    row with x0 == x1 is class 0; accuracies exact); and no clusters (losses[3] and acc[2] NaN as
    torch's 0 / 0, a guarded d_obj untouched)."""
    _loss_check(cuda_device, case, R.LOSS_G)
    if case['node_cls'].shape[0] < 1000:
        _loss_check(cuda_device, case, R.LOSS_G[::-1])


def test_loss_graph_refuses_65_classes(cuda_device):
    dev = cuda_device
    lib = _nat().lib()
    keep = []
    a = _loss_args(dev, R.loss_case('65 classes', nc=65, N=20, U=20, K=5, ties=False), keep)
    losses, acc, ws = Buf(dev, 1, 4), Buf(dev, 1, 3), Buf(dev, 1, 2048 * 3)
    assert lib.rg_loss_graph(ctypes.byref(a), losses.ptr, acc.ptr, ws.ptr, 2048 * 12, _st(dev)) != 0
    d = [Buf(dev, 20, 65), Buf(dev, 20, 2), Buf(dev, 20, 2), Buf(dev, 5, 65)]
    d_g = dev_vec(dev, R.LOSS_G, F32)
    assert lib.rg_loss_graph_backward(ctypes.byref(a), d_g.data_ptr(), *(b.ptr for b in d),
                                      _st(dev)) != 0
    torch.cuda.synchronize(dev)
    for b in [losses, acc, ws] + d:
        b.untouched('65 classes')


# ------------------------------------------- 6. rg_cross_entropy and rg_object_focal_loss
@pytest.mark.parametrize('nc', R.CE_NC)
@pytest.mark.parametrize('n', R.CE_N)
def test_cross_entropy_matches_float64(cuda_device, n, nc):
    """n around the one workgroup's stride of 256, ld = nc + 3, ld_d = nc + 2, rows scaled up to
    1e4, g = -2.5 on the device, exact ties (first maximum).  The kernels compute in float64:
    loss and every gradient entry within 2 float32 ulp of the float64 value."""
    dev = cuda_device
    lib = _nat().lib()
    x, k = R.ce_case(n, nc)
    ref_l, ref_d, ref_acc = R.cross_entropy_reference(x, k)
    d_x, d_k = dev_mat(dev, x.numpy(), nc + 3), dev_vec(dev, k.numpy(), I64)
    d_g = dev_vec(dev, [R.CE_G], F32)
    loss, acc, d = Buf(dev, 1, 1), Buf(dev, 1, 1), Buf(dev, n, nc, nc + 2)
    assert lib.rg_cross_entropy(d_x.data_ptr(), nc + 3, d_k.data_ptr(), n, nc, loss.ptr, acc.ptr,
                                _st(dev)) == 0
    assert lib.rg_cross_entropy_backward(d_x.data_ptr(), nc + 3, d_k.data_ptr(), n, nc,
                                         d_g.data_ptr(), d.ptr, nc + 2, _st(dev)) == 0
    torch.cuda.synchronize(dev)
    case = f'n={n} nc={nc}'
    for tensor, got, ref, scale in (('loss', loss.read('loss'), np.array([[ref_l]]), 0.0),
                                    ('d_logits', d.read('d'), ref_d, (nc + 4) * abs(R.CE_G) / n)):
        ok, ratio = R.within_ulp2(got, ref, scale)
        R.record('rg_cross_entropy' + ('_backward' if tensor != 'loss' else ''), case, tensor,
                 ratio, 0.0, 1.0)
        assert ok, (tensor, ratio)
    assert acc.read('acc')[0, 0] == F32(ref_acc)


def test_cross_entropy_without_rows(cuda_device):
    """n = 0: the forward refuses, the backward is a no-op."""
    dev = cuda_device
    lib = _nat().lib()
    d_x, d_k, d_g = dev_mat(dev, np.zeros((1, 7), F32)), dev_vec(dev, [0], I64), dev_vec(dev, [1], F32)
    loss, acc, d = Buf(dev, 1, 1), Buf(dev, 1, 1), Buf(dev, 0, 7, 9)
    assert lib.rg_cross_entropy(d_x.data_ptr(), 7, d_k.data_ptr(), 0, 7, loss.ptr, acc.ptr,
                                _st(dev)) != 0
    assert lib.rg_cross_entropy_backward(d_x.data_ptr(), 7, d_k.data_ptr(), 0, 7, d_g.data_ptr(),
                                         d.ptr, 9, _st(dev)) == 0
    torch.cuda.synchronize(dev)
    for b in (loss, acc, d):
        b.untouched('n = 0')


@pytest.mark.parametrize('nc', R.FOCAL_NC)
@pytest.mark.parametrize('n', R.FOCAL_N)
def test_object_focal_loss_matches_float64(cuda_device, n, nc):
    """The alpha-less focal loss summed over classes and divided by n, on the saturation grid laid
    into rows and randn * 3 rows; ld = nc + 3, ldd = nc + 2, g_loss = -2.5."""
    dev = cuda_device
    lib = _nat().lib()
    x, k = R.focal_case(n, nc)
    ref_l, ref_d = R.object_focal_reference(x, k, torch.float64)
    l32, d32 = R.object_focal_reference(x, k, torch.float32)
    d_x, d_k = dev_mat(dev, x.numpy(), nc + 3), dev_vec(dev, k.numpy(), I64)
    d_g = dev_vec(dev, [R.CE_G], F32)
    loss, d = Buf(dev, 1, 1), Buf(dev, n, nc, nc + 2)
    assert lib.rg_object_focal_loss(d_x.data_ptr(), nc + 3, d_k.data_ptr(), n, nc, loss.ptr,
                                    _st(dev)) == 0
    assert lib.rg_object_focal_loss_backward(d_x.data_ptr(), nc + 3, d_k.data_ptr(), n, nc,
                                             d_g.data_ptr(), d.ptr, nc + 2, _st(dev)) == 0
    torch.cuda.synchronize(dev)
    case = f'n={n} nc={nc}'
    _check_abs('rg_object_focal_loss', case, 'loss', loss.read('loss')[0, 0], ref_l,
               R.loss_bound(ref_l), abs(l32 - ref_l))
    got = d.read('d_logits')
    assert np.isfinite(got).all()
    _check_f32('rg_object_focal_loss_backward', case, 'd_logits', got, ref_d, d32)


def test_object_focal_loss_refusals(cuda_device):
    dev = cuda_device
    lib = _nat().lib()
    d_x, d_k, d_g = dev_mat(dev, np.zeros((4, 9), F32)), dev_vec(dev, [0] * 4, I64), dev_vec(dev, [1], F32)
    for n, nc, ld, ldd in ((0, 7, 9, 9), (4, 7, 6, 9), (4, 7, 9, 6)):
        loss, d = Buf(dev, 1, 1), Buf(dev, 4, 7, 9)
        if ldd >= nc:
            assert lib.rg_object_focal_loss(d_x.data_ptr(), ld, d_k.data_ptr(), n, nc, loss.ptr,
                                            _st(dev)) != 0
        assert lib.rg_object_focal_loss_backward(d_x.data_ptr(), ld, d_k.data_ptr(), n, nc,
                                                 d_g.data_ptr(), d.ptr, ldd, _st(dev)) != 0
        torch.cuda.synchronize(dev)
        loss.untouched('refused')
        d.untouched('refused')
