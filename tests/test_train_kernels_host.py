"""CPU checks of tests/train_kernels_ref.py, the references of tests/test_gpu_train_kernels.py:
every float64 reference against torch autograd of a restatement written independently of it
(torch.std, F.leaky_relu, F.cross_entropy, F.binary_cross_entropy_with_logits, torch max / amax),
the float32 loss restatement against oracle/train_ref.loss_graph, the mask and tie caps on every
case's inputs, and the bound helpers against perturbed results they must reject."""
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import train_kernels_ref as R

ALL_FFN = [(C, a, r) for C, a in R.FFN_NORM_CASES for r in R.FFN_ROWS] + \
          [(C, a, R.FFN_LONG_ROWS) for C, a in R.FFN_LONG_CASES]


def _ffn_independent(z, da, act, s=R.FFN_S, m=R.FFN_M):
    zz = z.double().clone().requires_grad_(True)
    sp = torch.tensor(s, dtype=torch.float64, requires_grad=True)
    mp = torch.tensor(m, dtype=torch.float64, requires_grad=True)
    n = (zz - zz.mean(1, keepdim=True)) / (torch.std(zz, dim=1, unbiased=True, keepdim=True) + 1e-5)
    y = sp * n + mp
    a = {'leakyrelu': lambda v: F.leaky_relu(v, 0.01), 'relu': F.relu, 'swish': F.silu,
         'none': lambda v: v}[act](y)
    (a * da.double()).sum().backward()
    return zz.grad.numpy(), float(sp.grad), float(mp.grad)


@pytest.mark.parametrize('C,act', R.FFN_NORM_CASES)
def test_ffn_reference_matches_independent_autograd_and_the_formula(C, act):
    for rows in R.FFN_ROWS:
        z, da = R.ffn_inputs(C, rows, act)
        ref = R.ffn_reference(z, da, act, torch.float64)
        dz, ds, dm = _ffn_independent(z, da, act)
        frm = R.ffn_formula(z, da, act)
        # dz is a difference of terms of the size of da / std (at C = 2 it nearly cancels)
        scale = 10 * max(np.abs(ref['dz']).max(), float(da.abs().max()))
        psum = np.abs(ref['gy'] * ref['n']).sum() + np.abs(ref['gy']).sum()
        for other_dz, other_s, other_m in ((dz, ds, dm), (frm['dz'], frm['d_std'], frm['d_mu'])):
            assert np.abs(other_dz - ref['dz']).max() <= 1e-11 * scale
            assert abs(other_s - ref['d_std']) <= 1e-12 * psum
            assert abs(other_m - ref['d_mu']) <= 1e-12 * psum


@pytest.mark.parametrize('C,act,rows', ALL_FFN)
def test_ffn_kink_mask_stays_under_its_cap(C, act, rows):
    """On the float64 reference alone: at most 1 % of a case's rows, none under 100 rows."""
    z, da = R.ffn_inputs(C, rows, act)
    ref = R.ffn_reference(z, da, act, torch.float64)
    mask = R.kink_rows(ref['y'], act)
    assert R.kink_cap_ok(mask), (int(mask.sum()), rows)
    if act in ('swish', 'none'):
        assert not mask.any()
    if C == 2:
        assert float((z[:, 0] - z[:, 1]).abs().min()) >= 0.5
    assert np.isfinite(ref['dz']).all()


def test_ffn_gather_inputs_have_repeats_and_unused_rows():
    gidx, gscale = R.gather_inputs(400, 515, 5)
    assert len(np.unique(gidx)) < 515 and len(np.unique(gidx)) < 400
    assert gidx.min() >= 0 and gidx.max() < 400 and (gscale > 0).all()


@pytest.mark.parametrize('C', [2, 5, 64])
def test_degenerate_row_autograd_is_nan_and_the_convention_is_the_formulas(C):
    """torch's autograd of the forward gives NaN for the whole constant row (sqrt'(0) = inf times
    a zero); the kernel's convention (coef = 0) is ffn_formula's, which the GPU test asserts."""
    z, da, row = R.degenerate_inputs(C)
    ref = R.ffn_reference(z, da, 'leakyrelu', torch.float64)
    assert np.isnan(ref['dz'][row]).all()
    others = np.arange(9) != row
    assert np.isfinite(ref['dz'][others]).all()
    assert not R.kink_rows(ref['y'][others], 'leakyrelu').any()
    assert (z[row] == z[row, 0]).all()
    conv, bound = R.degenerate_convention(da[row].numpy(), C)
    frm = R.ffn_formula(z, da, 'leakyrelu')['dz'][row]
    assert np.abs(conv - frm).max() <= bound           # eps as float32 against 1e-5
    assert bound <= 2e-5 * 1e5 * R.FFN_S * float(da[row].abs().max())


# --------------------------------------------------------------------------------- routing
def test_segment_max_loop_matches_torch_max_autograd():
    rng = np.random.default_rng(1)
    N, C = 60, 9
    h = rng.permutation(N * C).reshape(N, C).astype(np.float32)       # tie-free
    lists = [rng.permutation(N)[:k] for k in (1, 2, 17, 60, 5)]
    cptr = np.concatenate([[0], np.cumsum([len(x) for x in lists])]).astype(np.int32)
    cidx = np.concatenate(lists).astype(np.int32)
    dp = rng.standard_normal((len(lists), C))
    ht = torch.from_numpy(h).double().requires_grad_(True)
    sum((ht[torch.from_numpy(m)].max(0).values * torch.from_numpy(dp[c])).sum()
        for c, m in enumerate(lists)).backward()
    got = R.segment_max_backward_ref(h, cptr, cidx, dp, np.zeros((N, C)))
    assert np.abs(got - ht.grad.numpy()).max() <= 1e-12


def test_range_max_loop_matches_torch_max_autograd():
    rng = np.random.default_rng(2)
    Rr, C = R.RANGE_ROWS, 7
    x = rng.permutation(Rr * C).reshape(Rr, C).astype(np.float32)
    for name, (b, e) in R.range_layouts(9).items():
        dp = rng.standard_normal((9, C))
        xt = torch.from_numpy(x).double().requires_grad_(True)
        tot = sum((xt[bb:ee].max(0).values * torch.from_numpy(dp[o])).sum()
                  for o, (bb, ee) in enumerate(zip(b, e)) if bb < ee)
        want = np.zeros((Rr, C))
        if torch.is_tensor(tot):
            tot.backward()
            want = xt.grad.numpy()
        got = R.range_max_backward_ref(x, b, e, dp, np.zeros((Rr, C)))
        assert np.abs(got - want).max() <= 1e-12, name
    lay = R.range_layouts(17)
    assert (lay['prefix'][0] == 0).all() and (np.diff(lay['prefix'][1]) > 0).all()
    b, e = lay['prefix with empties']
    assert (b == e).any() and (b > e).any() and (b < e).sum() >= 8
    b, e = lay['mixed']
    assert (e - b == 1).any() and (b == e).any() and (b > e).any()


def test_amax_loop_matches_torch_amax_autograd():
    rng = np.random.default_rng(3)
    sizes = [0, 1, 2, 40, 0, 3]
    seg_ptr = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    M, C = int(seg_ptr[-1]), 5
    index = torch.from_numpy(np.repeat(np.arange(len(sizes)), sizes)).view(-1, 1).expand(M, C)
    d_agg = rng.standard_normal((len(sizes), C)).astype(np.float32)
    for msg in (rng.permutation(M * C).reshape(M, C).astype(np.float32),          # tie-free
                R.quantised(rng, (M, C))):                                        # ties share
        mt = torch.from_numpy(msg).requires_grad_(True)
        # the base is -7, not 0: torch's amax backward counts a base entry equal to the result as
        # one more tie even with include_self=False, and the quantised messages hold 0.0
        agg = torch.full((len(sizes), C), -7.0).scatter_reduce(0, index, mt, 'amax',
                                                               include_self=False)
        (agg * torch.from_numpy(d_agg)).sum().backward()
        got = R.segment_amax_backward_ref(msg, seg_ptr, d_agg)
        assert np.abs(got - mt.grad.numpy()).max() <= 1e-7 * np.abs(d_agg).max()
        assert not np.signbit(got[got == 0]).any()


def test_routing_cases_have_ties_and_specials():
    for C in R.SEGMAX_C:
        h, cptr, cidx, dp, dh0 = R.segment_max_case(C)
        assert np.isnan(h).any() and np.isinf(h).any()
        assert {0, 1, 2, 37, 300} <= set(np.diff(cptr).tolist())
        assert np.abs(dp).max() <= 8 and (dp == np.round(dp)).all() and (dh0 == np.round(dh0)).all()
        assert (len(cptr) - 1) * C > 256 or C < 64
    for C in R.AMAX_C:
        msg, seg_ptr, d_agg = R.amax_case(C)
        assert np.isfinite(msg).all() and {0, 1, 2, 40} <= set(np.diff(seg_ptr).tolist())


# ---------------------------------------------------------------------------------- losses
def _independent_losses(case, dtype):
    x = {k: case[k].detach().to(dtype).clone().requires_grad_(True)
         for k in ('node_cls', 'node_reg', 'link', 'obj')}
    nc = case['node_cls'].shape[1]
    mu_x, mu_y, sg_x, sg_y = case['mu_sigma']
    off = case['node_offsets'].to(dtype)
    t = torch.stack([(off[:, 0] - mu_x) / sg_x, (off[:, 1] - mu_y) / sg_y], 1)
    node_t = F.one_hot(case['node_class'], nc).to(dtype)
    edge_t = F.one_hot(case['edge_class'], 2).to(dtype)
    obj_t = F.one_hot(case['obj_class'], nc).to(dtype)
    p = torch.sigmoid(x['link'])
    ce = F.binary_cross_entropy_with_logits(x['link'], edge_t, reduction='none')
    fl = (0.25 * edge_t + 0.75 * (1 - edge_t)) * ce * (1 - (p * edge_t + (1 - p) * (1 - edge_t))) ** 2
    l0 = F.cross_entropy(x['node_cls'], node_t, case['class_w'].to(dtype), reduction='none')
    l1 = 0.5 * F.mse_loss(x['node_reg'], t, reduction='none').sum(-1)
    l3 = F.cross_entropy(x['obj'], obj_t, reduction='none')
    w = case['weights']
    losses = torch.stack([l0.sum() / l0.shape[0] * w[0], l1.sum() / l1.shape[0] * w[1],
                          fl.sum() / fl.shape[0] * w[2], l3.sum() / l3.shape[0] * w[3]])
    return losses, x


@pytest.mark.parametrize('case', R.loss_cases(), ids=lambda c: c['name'])
def test_loss_restatement_matches_autograd_of_the_functional_one(case):
    losses, grads = R.loss_graph_reference(case, torch.float64)
    want, x = _independent_losses(case, torch.float64)
    live = torch.isfinite(want.detach())
    (want[live] * torch.tensor(R.LOSS_G, dtype=torch.float64)[live]).sum().backward()
    want = want.detach().numpy()
    assert (np.isnan(losses) == np.isnan(want)).all()
    assert np.isnan(losses[3]) == (case['obj'].shape[0] == 0) and np.isfinite(losses[:3]).all()
    ok = np.isfinite(want)
    assert np.abs(losses[ok] - want[ok]).max() <= 1e-12 * np.abs(want[ok]).max()
    for k, v in x.items():
        wg = v.grad.numpy() if v.grad is not None else np.zeros(v.shape)
        assert np.isfinite(grads[k]).all()
        # the functional BCE backward differs from the restatement's at float64 rounding of
        # magnitudes up to |x| = 104
        assert np.abs(grads[k] - wg).max(initial=0.0) <= 1e-12 * max(1.0, np.abs(wg).max(initial=0.0)), k
    assert (grads['obj'] == 0).all()                                   # g[3] = 0


@pytest.mark.parametrize('case', R.loss_cases(), ids=lambda c: c['name'])
def test_float32_loss_restatement_matches_the_oracle(case):
    from oracle import train_ref
    nc = case['node_cls'].shape[1]
    w = case['weights']
    cfg = types.SimpleNamespace(num_classes=nc, num_edge_classes=2, node_cls_loss_weight=w[0],
                                node_reg_loss_weight=w[1], edge_cls_loss_weight=w[2],
                                obj_cls_loss_weight=w[3])
    mu_x, mu_y, sg_x, sg_y = case['mu_sigma']
    off = case['node_offsets']
    t = torch.stack([(off[:, 0] - mu_x) / sg_x, (off[:, 1] - mu_y) / sg_y], 1)
    orc = train_ref.loss_graph(cfg, case['class_w'],
                               (case['node_cls'], case['node_reg'], case['link'], case['obj']),
                               (case['node_class'], t, case['edge_class'], case['obj_class']))
    got, _ = R.loss_graph_ref(case, torch.float32)
    for i, k in enumerate(('loss_node_cls', 'loss_node_reg', 'loss_edge_cls', 'loss_obj_cls')):
        a, b = float(got[i].detach()), float(orc[k])
        assert (np.isnan(a) and np.isnan(b)) or abs(a - b) <= 2e-6 * max(1.0, abs(b)), (k, a, b)


@pytest.mark.parametrize('case', R.loss_cases(), ids=lambda c: c['name'])
def test_loss_cases_have_exact_ties_and_no_near_ties(case):
    for k in ('node_cls', 'obj', 'link'):
        assert R.top2_gap_ok(case[k].numpy()), k
    x = case['link'].numpy()
    assert (x[:, 0] == x[:, 1]).any()
    if case['node_cls'].shape[1] >= 2:
        s = np.sort(case['node_cls'].numpy(), 1)
        assert (s[:, -1] == s[:, -2]).sum() >= 3


def test_accuracies_match_compute_accuracy_without_ties():
    from oracle import train_ref
    case = R.loss_case('plain', ties=False, seed=9)
    acc = R.accuracies(case)
    for a, (x, k) in zip(acc, (('node_cls', 'node_class'), ('link', 'edge_class'),
                               ('obj', 'obj_class'))):
        assert abs(a - float(train_ref.compute_accuracy(case[x], case[k]))) <= 1e-7
    # the tie rules: first maximum; a link row with x0 == x1 counts as class 0
    assert R.first_max_accuracy(np.array([[1., 1.], [1., 1.]]), np.array([0, 1])) == 0.5
    assert R.first_max_accuracy(np.array([[0., 2., 2.]]), np.array([2])) == 0.0
    assert np.isnan(R.first_max_accuracy(np.zeros((0, 3)), np.zeros(0, np.int64)))


def test_saturation_grid_is_the_issues():
    x, k = R.sat_link()
    assert x.shape == (578, 2) and int(k.sum()) == 289
    assert sorted(set(np.abs(x.numpy()).reshape(-1).tolist())) == sorted(
        float(np.float32(v)) for v in (0.0, 1e-4, 1.0, 9.0, 17.0, 30.0, 88.0, 90.0, 104.0))


@pytest.mark.parametrize('n', R.CE_N)
@pytest.mark.parametrize('nc', R.CE_NC)
def test_cross_entropy_reference_matches_functional_autograd(n, nc):
    x, k = R.ce_case(n, nc)
    loss, d, acc = R.cross_entropy_reference(x, k)
    xx = x.double().requires_grad_(True)
    want = F.cross_entropy(xx, k, reduction='sum') / n
    (want * R.CE_G).backward()
    assert abs(loss - float(want)) <= 1e-12 * max(1.0, abs(float(want)))
    assert np.abs(d - xx.grad.numpy()).max() <= 1e-14 * abs(R.CE_G)
    assert R.top2_gap_ok(x.numpy()) and np.isfinite(d).all()
    assert 0.0 <= acc <= 1.0


@pytest.mark.parametrize('n', R.FOCAL_N)
@pytest.mark.parametrize('nc', R.FOCAL_NC)
def test_object_focal_reference_matches_functional_autograd(n, nc):
    x, k = R.focal_case(n, nc)
    loss, d = R.object_focal_reference(x, k, torch.float64)
    xx = x.double().requires_grad_(True)
    t = F.one_hot(k, nc).double()
    p = torch.sigmoid(xx)
    ce = F.binary_cross_entropy_with_logits(xx, t, reduction='none')
    want = (ce * (1 - (p * t + (1 - p) * (1 - t))) ** 2).sum() / n
    (want * R.CE_G).backward()
    assert abs(loss - float(want)) <= 1e-12 * max(1.0, abs(float(want)))
    assert np.abs(d - xx.grad.numpy()).max() <= 1e-12 * np.abs(d).max()
    assert np.isfinite(d).all() and np.isfinite(loss)
    if n * nc >= 17:
        assert {104.0, -104.0, 0.0} <= set(x.numpy().reshape(-1).tolist())


# ----------------------------------------------------------------------------- the bounds
def test_f32_bound_rejects_one_element_off_by_eight_bounds():
    z, da = R.ffn_inputs(64, 515)
    r64 = R.ffn_reference(z, da, 'leakyrelu', torch.float64)
    r32 = R.ffn_reference(z, da, 'leakyrelu', torch.float32)
    keep = ~R.kink_rows(r64['y'], 'leakyrelu')
    ok, err, err32, b = R.within_f32_bound(r32['dz'][keep], r64['dz'][keep], r32['dz'][keep])
    assert ok and 0 < err32 <= 1e-6 * np.abs(r64['dz']).max()
    bad = r32['dz'][keep].copy()
    bad[100, 7] += 8 * b
    assert not R.within_f32_bound(bad, r64['dz'][keep], r32['dz'][keep])[0]
    bad[100, 7] = np.nan
    assert not R.within_f32_bound(bad, r64['dz'][keep], r32['dz'][keep])[0]
    assert not R.within_ulp2(np.float64(np.float32(1.5)) * (1 + 4 * 2.0 ** -23), np.float64(1.5))[0]
    assert R.within_ulp2(np.float32(1.0 / 3), np.float64(1.0 / 3))[0]


def test_bit_equality_rejects_a_gradient_routed_to_the_second_tied_row():
    x = np.array([[1.0], [2.0], [2.0], [0.5]], np.float32)
    b, e = np.array([0], np.int32), np.array([4], np.int32)
    dp = np.array([[3.0]], np.float32)
    want = R.range_max_backward_ref(x, b, e, dp, np.zeros((4, 1))).astype(np.float32)
    assert want[:, 0].tolist() == [0.0, 3.0, 0.0, 0.0]
    moved = want.copy()
    moved[[1, 2]] = moved[[2, 1]]
    assert R.same_bits(want, want.copy()) and not R.same_bits(moved, want)
    assert not R.same_bits(np.float32([-0.0]), np.float32([0.0]))
    # NaN wins, the first of several
    x[[1, 3], 0] = np.nan
    assert R.range_max_backward_ref(x, b, e, dp, np.zeros((4, 1)))[:, 0].tolist() == [0, 3, 0, 0]


def test_param_bound_rejects_one_rows_sign_flipped():
    z, da = R.ffn_inputs(64, 515)
    r = R.ffn_reference(z, da, 'leakyrelu', torch.float64)
    b = R.param_bound(r['gy'], r['n'], r['d_std'])
    contrib = (r['gy'] * r['n']).sum(1)
    row = int(np.argmax(np.abs(contrib)))
    assert abs(-2 * contrib[row]) > b
    assert abs(float(np.float32(r['d_std'])) - r['d_std']) <= b
    frm = R.ffn_formula(z, da, 'leakyrelu')
    assert abs(frm['d_std'] - r['d_std']) <= b and abs(frm['d_mu'] - r['d_mu']) <= b
