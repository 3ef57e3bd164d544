"""References, case builders and bound helpers for the training step's small kernels
(tests/test_gpu_train_kernels.py runs the kernels, tests/test_train_kernels_host.py checks this
module on the CPU).  Plain torch-CPU / numpy: nothing of the native library is imported here.

Bounds (one output tensor at a time, err = max|got - ref64|):
  * f32_bound        4 err32 + 2^-22 max|ref64|, err32 = the error of torch's own float32 CPU
                     evaluation of the same reference against float64.  4: the kernels' other
                     summation trees (16-lane xor tree, per-lane strided partials) and their
                     expf / log1pf against torch's; the floor is four float32 roundings of the
                     largest entry, for tensors where torch's float32 happens to be exact.
  * param_bound      the norm parameter gradients, the bound of
                     test_dx_norm_backward_matches_two_steps: 1e-6 (sum|gy n| + sum|gy|), plus one
                     float32 rounding of the result.
  * loss_bound       1e-5 max(1, |ref|), the bound of test_loss_modules_match_oracle.
  * ulp2_bound       kernels that compute in float64 inside: 2 float32 ulp of the float64 value,
                     element by element (see the function for the two format terms beside it).
  * routing          the max-pool backwards route and never round: bit equality.
"""
import json
import os

import numpy as np
import torch

F32, F64, I32, I64 = np.float32, np.float64, np.int32, np.int64
ACTS = ('none', 'relu', 'leakyrelu', 'swish')
NORM_EPS = 1e-5
KINK = 1e-5          # |y64| below this: the float32 y may take the other sign


# ------------------------------------------------------------------------------------ bounds
def max_err(got, ref):
    got, ref = np.asarray(got, F64), np.asarray(ref, F64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    if got.size == 0:
        return 0.0
    d = np.abs(got - ref)
    return float('inf') if not np.isfinite(d).all() else float(d.max())


def f32_bound(err32, ref64):
    ref64 = np.asarray(ref64, F64)
    return 4.0 * float(err32) + 2.0 ** -22 * float(np.abs(ref64).max(initial=0.0))


def within_f32_bound(got, ref64, ref32):
    """(ok, err, err32, bound) of one tensor under f32_bound."""
    err, err32 = max_err(got, ref64), max_err(ref32, ref64)
    assert np.isfinite(err32), 'the float32 evaluation of the reference is not finite'
    b = f32_bound(err32, ref64)
    return err <= b, err, err32, b


def param_bound(gy, n, ref, extra=0.0):
    gy, n = np.asarray(gy, F64), np.asarray(n, F64)
    return 1e-6 * float(np.abs(gy * n).sum() + np.abs(gy).sum()) + 2.0 ** -24 * abs(float(ref)) \
        + float(extra)


def loss_bound(ref):
    return 1e-5 * max(1.0, abs(float(ref)))


FLT_MIN = float(np.finfo(F32).tiny)


def ulp2_bound(ref64, f64_scale=0.0):
    """Per element: 2 float32 ulp of the float64 value, plus two terms of the formats themselves:
    a result below the smallest normal float32 may be flushed to zero (FLT_MIN), and a float64
    evaluation of p - 1 with p = exp(.) / s carries float64's own rounding at magnitude 1
    (2^-53 x f64_scale, f64_scale = (nc + 4) |g| / n for the gradient: nc - 1 additions in s,
    exp, the division, the subtraction and the product), which is not small against 2 ulp of
    an entry of 1e-10."""
    ref64 = np.asarray(ref64, F64)
    a = np.abs(ref64).astype(F32)
    return 2.0 * np.spacing(a).astype(F64) + FLT_MIN + 2.0 ** -53 * float(f64_scale)


def within_ulp2(got, ref64, f64_scale=0.0):
    """(ok, worst err / bound) element by element."""
    got, ref64 = np.asarray(got, F64), np.asarray(ref64, F64)
    assert got.shape == ref64.shape
    if got.size == 0:
        return True, 0.0
    d = np.abs(got - ref64)
    if not np.isfinite(d).all():
        return False, float('inf')
    r = float((d / ulp2_bound(ref64, f64_scale)).max())
    return r <= 1.0, r


def same_bits(got, want):
    """Bit equality of two float32 arrays (so -0.0 != +0.0 and NaN payloads count)."""
    got, want = np.ascontiguousarray(got, F32), np.ascontiguousarray(want, F32)
    return got.shape == want.shape and bool((got.view(I32) == want.view(I32)).all())


def record(kernel, case, tensor, err, err32, bound):
    """One JSON line per (case, tensor) to the file $RG_KERNEL_ERROR_REPORT names."""
    path = os.environ.get('RG_KERNEL_ERROR_REPORT')
    if not path:
        return
    ratio = (err / bound) if bound > 0 else (0.0 if err == 0 else float('inf'))
    with open(path, 'a') as fh:
        fh.write(json.dumps({'kernel': kernel, 'case': case, 'tensor': tensor, 'err': err,
                             'err32': err32, 'bound': bound, 'err_over_bound': ratio}) + '\n')


# ----------------------------------------------------------------- 1. norm + activation backward
FFN_S, FFN_M = 1.3, 0.2
FFN_PRE_MU, FFN_PRE_STD = 0.25, -0.5
FFN_NORM_CASES = [(C, 'leakyrelu') for C in (2, 5, 16, 17, 64, 65, 128, 129, 256)] + \
                 [(C, a) for a in ('none', 'relu', 'swish') for C in (17, 64)]
FFN_ROWS = (1, 3, 515)
FFN_LONG_ROWS = 2048 * 16 + 5           # the second trip of the kernel's row loop
FFN_LONG_CASES = [(5, 'leakyrelu'), (64, 'leakyrelu')]
FFN_PLAIN_C = (1, 16, 65, 256)          # has_norm = 0


def ffn_inputs(C, rows, act='leakyrelu'):
    """z = randn * 2 + 0.3, da = randn (float32).  C = 2: rows with |z0 - z1| < 0.5 are redrawn
    (std near 0: the problem is ill-conditioned there, float32 itself is 2e-4 off)."""
    g = torch.Generator().manual_seed(7919 * C + 31 * rows + 101 * ACTS.index(act))
    z = torch.randn(rows, C, generator=g) * 2.0 + 0.3
    da = torch.randn(rows, C, generator=g)
    while C == 2:
        bad = (z[:, 0] - z[:, 1]).abs() < 0.5
        if not bool(bad.any()):
            break
        z[bad] = torch.randn(int(bad.sum()), 2, generator=g) * 2.0 + 0.3
    return z, da


def activation(y, act):
    if act == 'leakyrelu':
        return torch.where(y > 0, y, 0.01 * y)
    if act == 'relu':
        return torch.where(y > 0, y, torch.zeros_like(y))
    if act == 'swish':
        return y / (1.0 + torch.exp(-y))
    assert act == 'none'
    return y


def ffn_forward(z, s, m, act, has_norm=True):
    """The forward of the issue: a = act(s n + m), n = (z - mean) / (std + 1e-5), std unbiased.
    Returns (a, y, n); without the norm y = z and n is None."""
    if not has_norm:
        return activation(z, act), z, None
    C = z.shape[1]
    mean = z.sum(1, keepdim=True) / C
    d = z - mean
    std = ((d * d).sum(1, keepdim=True) / (C - 1)).sqrt()
    n = d / (std + NORM_EPS)
    y = s * n + m
    return activation(y, act), y, n


def ffn_reference(z, da, act, dtype, has_norm=True, s=FFN_S, m=FFN_M):
    """torch autograd of ffn_forward in `dtype`, given da: numpy float64 views of dz, d_std, d_mu
    (the sums alone, without a preload), y, n and gy = da act'(y)."""
    zz = z.detach().to(dtype).clone().requires_grad_(True)
    sp = torch.tensor(s, dtype=dtype, requires_grad=True)
    mp = torch.tensor(m, dtype=dtype, requires_grad=True)
    a, y, n = ffn_forward(zz, sp, mp, act, has_norm)
    if has_norm:
        y.retain_grad()
        (a * da.to(dtype)).sum().backward()
        gy = y.grad
    else:
        (a * da.to(dtype)).sum().backward()
        gy = zz.grad
    out = dict(dz=zz.grad.double().numpy(), y=y.detach().double().numpy(),
               gy=gy.double().numpy())
    if has_norm:
        out.update(d_std=float(sp.grad), d_mu=float(mp.grad), n=n.detach().double().numpy())
    return out


def ffn_formula(z, da, act, s=FFN_S, m=FFN_M):
    """The hand-derived backward the kernel's comment states, in float64 numpy."""
    z, da = z.double().numpy(), da.double().numpy()
    C = z.shape[1]
    d = z - z.mean(1, keepdims=True)
    std = np.sqrt((d * d).sum(1, keepdims=True) / (C - 1))
    r = 1.0 / (std + NORM_EPS)
    n = d * r
    y = s * n + m
    if act == 'leakyrelu':
        ga = np.where(y > 0, 1.0, 0.01)
    elif act == 'relu':
        ga = np.where(y > 0, 1.0, 0.0)
    elif act == 'swish':
        sg = 1.0 / (1.0 + np.exp(-y))
        ga = sg * (1.0 + y * (1.0 - sg))
    else:
        ga = np.ones_like(y)
    gy = da * ga
    gn = s * gy
    A = (gn * d).sum(1, keepdims=True)
    with np.errstate(divide='ignore', invalid='ignore'):
        coef = np.where(std > 0, r * r * A / ((C - 1) * std), 0.0)
    gd = r * gn - coef * d
    return dict(dz=gd - gd.mean(1, keepdims=True), d_std=float((gy * n).sum()),
                d_mu=float(gy.sum()))


def kink_rows(y64, act, has_norm=True):
    """Rows whose float32 y may take the other sign of a leakyrelu / relu kink under the norm."""
    rows = y64.shape[0]
    if not has_norm or act not in ('leakyrelu', 'relu'):
        return np.zeros(rows, bool)
    return (np.abs(y64) < KINK).any(1)


def kink_cap_ok(mask):
    """At most 1 % of a case's rows, none in cases under 100 rows."""
    rows = mask.size
    return int(mask.sum()) == 0 if rows < 100 else int(mask.sum()) <= rows // 100


def kink_extra(mask, da, n64):
    """The masked rows' sum|da n| + sum|da|: what their other sign can move d_std / d_mu by."""
    da = np.asarray(da, F64)[mask]
    return float(np.abs(da * n64[mask]).sum() + np.abs(da).sum())


def act_grad_f32(z, act):
    """act'(z) as float32, evaluated on float32 z (has_norm = 0: none / relu / leakyrelu)."""
    z = np.asarray(z, F32)
    if act == 'leakyrelu':
        return np.where(z > 0, F32(1), F32(0.01)).astype(F32)
    if act == 'relu':
        return np.where(z > 0, F32(1), F32(0)).astype(F32)
    assert act == 'none'
    return np.ones_like(z)


def gather_inputs(n_src, rows, seed):
    """gidx int32 [rows] into n_src source rows, with repeats and unused rows; gscale [n_src]."""
    rng = np.random.default_rng(seed)
    used = rng.permutation(n_src)[:n_src * 2 // 3]
    gidx = used[rng.integers(0, len(used), rows)].astype(I32)
    gscale = (1.0 / rng.integers(1, 9, n_src)).astype(F32)
    return gidx, gscale


def degenerate_inputs(C):
    """9 ordinary rows with a constant row (std = 0) at row 4; every sum of the constant row is
    exact in float32 (0.75 C and its quotient), so the kernel sees d = 0 and std = 0 exactly."""
    z, da = ffn_inputs(C, 9)
    z[4] = 0.75
    return z, da, 4


def degenerate_convention(da_row, C, s=FFN_S, m=FFN_M, act='leakyrelu'):
    """The kernel's convention at std = 0 (coef = 0): n = 0, y = m, gn = s da act'(m),
    r = 1 / eps, dz = r gn - mean(r gn).  float64; eps is the kernel's float32 constant.
    Returns (dz, bound).  The bound: each element carries <= 5 roundings of a value <= max|r gn|
    (eps, r, s gy, r gn, the subtraction), the mean C - 1 roundings of partial sums
    <= C max|r gn|, then divided by C: (C + 8) 2^-24 max|r gn|."""
    da_row = np.asarray(da_row, F64)
    ga = 1.0 if (act in ('none',) or m > 0) else (0.01 if act == 'leakyrelu' else 0.0)
    r = 1.0 / float(F32(NORM_EPS))
    g = r * s * ga * da_row
    return g - g.mean(), (C + 8) * 2.0 ** -24 * float(np.abs(g).max())


# ------------------------------------------------------------------ 2 - 4. max-pool backwards
def quantised(rng, shape, nan=0, ninf=0):
    """Multiples of 0.5 in [-2, 2] (ties are common), with a few NaN and -inf entries."""
    x = (rng.integers(-4, 5, shape) * 0.5).astype(F32)
    flat = x.reshape(-1)
    pos = rng.permutation(flat.size)
    flat[pos[:nan]] = np.nan
    flat[pos[nan:nan + ninf]] = -np.inf
    return x


def small_ints(rng, shape, lim=8):
    return rng.integers(-lim, lim + 1, shape).astype(F32)


def segment_max_backward_ref(h, cptr, cidx, dp, dh0):
    """dh0 + routed dp: per (cluster, channel) to the first member holding the maximum, a NaN
    member wins (the first NaN): np.argmax over the member values in list order.  float64 sums."""
    dh = np.asarray(dh0, F64).copy()
    C = h.shape[1]
    cols = np.arange(C)
    for c in range(len(cptr) - 1):
        mem = cidx[cptr[c]:cptr[c + 1]]
        if len(mem) == 0:
            continue
        am = np.argmax(h[mem], axis=0)
        dh[mem[am], cols] += np.asarray(dp[c], F64)
    return dh


def range_max_backward_ref(x, begin, end, dp, dx0, absolute=False):
    """The same rule over row ranges [begin, end); b >= e is empty.  absolute: sums of |terms|
    (the error bound of a float d_pooled)."""
    dx = np.asarray(dx0, F64).copy()
    cols = np.arange(x.shape[1])
    for o, (b, e) in enumerate(zip(begin, end)):
        if b >= e:
            continue
        am = np.argmax(x[b:e], axis=0)
        t = np.asarray(dp[o], F64)
        dx[b + am, cols] += np.abs(t) if absolute else t
    return dx


def segment_amax_backward_ref(msg, seg_ptr, d_agg):
    """Per (segment, channel): cnt messages equal the maximum, each gets float32(d_agg) /
    float32(cnt) (one correctly rounded division), every other message +0.0."""
    out = np.zeros(msg.shape, F32)
    for s in range(len(seg_ptr) - 1):
        b, e = seg_ptr[s], seg_ptr[s + 1]
        if b >= e:
            continue
        eq = msg[b:e] == msg[b:e].max(0, keepdims=True)
        g = np.asarray(d_agg[s], F32) / eq.sum(0).astype(F32)
        out[b:e] = np.where(eq, g[None, :], F32(0))
    return out


SEGMAX_NODES = 300
SEGMAX_C = (1, 7, 64, 130)


def segment_max_case(C):
    """300 nodes; clusters of {0, 1, 2, 37, 300} members (300: every node, shuffled) and three
    that share nodes; quantised h with NaN and -inf; integer dp and dh preload."""
    rng = np.random.default_rng(100 + C)
    N = SEGMAX_NODES
    h = quantised(rng, (N, C), nan=max(2, C // 8), ninf=max(2, C // 8))
    shared = rng.permutation(N)[:20]
    lists = [np.zeros(0, I64), rng.permutation(N)[:1], rng.permutation(N)[:2],
             rng.permutation(N)[:37], rng.permutation(N), np.zeros(0, I64),
             shared[:12], shared[6:], shared[::2]]
    cptr = np.concatenate([[0], np.cumsum([len(x) for x in lists])]).astype(I32)
    cidx = np.concatenate(lists).astype(I32)
    dp = small_ints(rng, (len(lists), C))
    dh0 = small_ints(rng, (N, C))
    return h, cptr, cidx, dp, dh0


RANGE_ROWS = 40
RANGE_NOBJ = (1, 7, 8, 9, 17)
RANGE_C = (1, 63, 64, 65, 130)


def range_layouts(n_obj, R=RANGE_ROWS):
    """name -> (begin, end) int32 [n_obj]."""
    o = np.arange(n_obj)
    prefix_e = np.minimum(1 + o * max(1, (R - 1) // max(n_obj - 1, 1)), R)
    out = {'prefix': (np.zeros(n_obj, I64), prefix_e)}
    # the reference's shape with empty ranges (b == e and b > e) inside the run
    b, e = np.zeros(n_obj, I64), prefix_e.copy()
    e[1::3] = 0
    b[2::6], e[2::6] = 5, 3
    out['prefix with empties'] = (b, e)
    # nested, disjoint, single-row and empty ranges in turn
    kind = o % 6
    b = np.select([kind == 0, kind == 1, kind == 2, kind == 3, kind == 4],
                  [o % 7, 10 + o % 5, (3 * o) % R, 7, 9], 20 + o % 10)
    e = np.select([kind == 0, kind == 1, kind == 2, kind == 3, kind == 4],
                  [R - o % 7, 20 - o % 5, (3 * o) % R + 1, 7, 2], np.minimum(23 + o % 10, R))
    out['mixed'] = (b, e)
    out['all empty'] = (np.full(n_obj, 3, I64), np.full(n_obj, 3, I64))
    return {k: (np.asarray(b, I32), np.asarray(e, I32)) for k, (b, e) in out.items()}


def range_case(n_obj, C):
    rng = np.random.default_rng(1000 * n_obj + C)
    x = quantised(rng, (RANGE_ROWS, C), nan=max(1, C // 16), ninf=max(1, C // 16))
    x[1, ::2] = 2.5                     # every second channel: row 1 holds every later maximum
    dp = small_ints(rng, (n_obj, C))
    dx0 = small_ints(rng, (RANGE_ROWS, C))
    return x, dp, dx0


AMAX_C = (1, 64, 130)


def amax_case(C):
    """Segment sizes {0, 1, 2, 40} (and again, shuffled), finite quantised messages."""
    rng = np.random.default_rng(300 + C)
    sizes = [0, 1, 2, 40, 0, 40, 2, 1, 0]
    seg_ptr = np.concatenate([[0], np.cumsum(sizes)]).astype(I32)
    msg = quantised(rng, (int(seg_ptr[-1]), C))
    d_agg = rng.standard_normal((len(sizes), C)).astype(F32)
    return msg, seg_ptr, d_agg


# ----------------------------------------------------------------------------- 5. loss graph
LOSS_W = (0.7, 1.9, 2.3, 0.45)          # node_cls, node_reg, edge_cls, obj_cls
LOSS_MU_SIGMA = (0.4, -1.1, 2.5, 0.7)   # mu_x, mu_y, sigma_x, sigma_y
LOSS_G = (0.3, -1.7, 2.0, 0.0)
SAT_GRID = (104.0, 90.0, 88.0, 30.0, 17.0, 9.0, 1.0, 1e-4)
ROW_SCALES = (1.0, 10.0, 100.0, 1e3, 1e4)


def class_weights(nc):
    return torch.tensor([0.5 + 0.37 * ((3 * c) % 5) for c in range(nc)], dtype=torch.float32)


def sat_grid():
    v = [s * x for x in SAT_GRID for s in (1.0, -1.0)] + [0.0]
    assert len(v) == 17
    return v


def sat_link():
    """Link logits on the grid squared, for both classes: 578 rows."""
    v = sat_grid()
    x = torch.tensor([[a, b] for a in v for b in v] * 2, dtype=torch.float32)
    k = torch.cat([torch.zeros(289, dtype=torch.int64), torch.ones(289, dtype=torch.int64)])
    return x, k


def focal(x, t, alpha):
    """sigmoid_focal_loss, gamma 2, alpha < 0: no alpha weighting.  ce written as
    log(1 + e^x) - x t (logaddexp: smooth at 0 for autograd)."""
    p = torch.sigmoid(x)
    ce = torch.logaddexp(torch.zeros_like(x), x) - x * t
    pt = p * t + (1.0 - p) * (1.0 - t)
    loss = ce * (1.0 - pt) * (1.0 - pt)
    if alpha >= 0:
        loss = (alpha * t + (1.0 - alpha) * (1.0 - t)) * loss
    return loss


def one_hot(k, nc, dtype):
    t = torch.zeros(k.shape[0], nc, dtype=dtype)
    if k.shape[0]:
        t[torch.arange(k.shape[0]), k] = 1.0
    return t


def ce_rows(x, k, w=None):
    """-w[k] log_softmax(x)[k] per row, the maximum subtracted first (as torch evaluates it: in
    float32 the row's size does not reach the result)."""
    if x.shape[0] == 0:
        return x.sum(1)
    sh = x - x.max(1, keepdim=True).values.detach()
    l = torch.log(torch.exp(sh).sum(1)) - sh.gather(1, k.view(-1, 1)).view(-1)
    return l * w[k] if w is not None else l


def loss_graph_ref(case, dtype):
    """Loss_Graph in `dtype` on the float32 inputs of `case` (a dict, see loss_case): the four
    weighted losses as a tensor [4] (inputs as leaves that require grad are returned too)."""
    x = {k: case[k].detach().to(dtype).clone().requires_grad_(True)
         for k in ('node_cls', 'node_reg', 'link', 'obj')}
    mu_x, mu_y, sg_x, sg_y = case['mu_sigma']
    off = case['node_offsets'].to(dtype)
    cw = case['class_w'].to(dtype)
    N, U, K = x['node_cls'].shape[0], x['link'].shape[0], x['obj'].shape[0]
    l0 = ce_rows(x['node_cls'], case['node_class'], cw).sum() / N
    t = torch.stack([(off[:, 0] - mu_x) / sg_x, (off[:, 1] - mu_y) / sg_y], 1)
    l1 = (0.5 * (x['node_reg'] - t) ** 2).sum() / N
    l2 = focal(x['link'], one_hot(case['edge_class'], 2, dtype), 0.25).sum() / U
    l3 = ce_rows(x['obj'], case['obj_class']).sum() / K
    w = case['weights']
    return torch.stack([l0 * w[0], l1 * w[1], l2 * w[2], l3 * w[3]]), x


def loss_graph_reference(case, dtype, g=LOSS_G):
    """losses float64 numpy [4] and the gradients of sum g_i loss_i (a term of zero rows adds
    nothing to the sum that is differentiated: its loss is NaN)."""
    losses, x = loss_graph_ref(case, dtype)
    gt = torch.tensor(g, dtype=dtype)
    live = torch.isfinite(losses.detach())
    (losses[live] * gt[live]).sum().backward()
    grads = {k: (v.grad if v.grad is not None else torch.zeros_like(v)).double().numpy()
             for k, v in x.items()}
    return losses.detach().double().numpy(), grads


def first_max_accuracy(x, k):
    x, k = np.asarray(x), np.asarray(k)
    if len(k) == 0:
        return float('nan')
    return float((np.argmax(x, 1) == k).sum() / F64(len(k)))


def accuracies(case):
    """compute_accuracy with the first maximum on ties: (segment, edge, object) in float64."""
    return [first_max_accuracy(case[a].numpy(), case[b].numpy())
            for a, b in (('node_cls', 'node_class'), ('link', 'edge_class'), ('obj', 'obj_class'))]


def top2_gap_ok(x):
    """Every row: an exact tie of its two largest logits, or a gap >= 1e-6 relative."""
    x = np.asarray(x, F64)
    if x.shape[0] == 0 or x.shape[1] < 2:
        return True
    s = np.sort(x, 1)
    gap = s[:, -1] - s[:, -2]
    return bool(((gap == 0) | (gap >= 1e-6 * np.maximum(np.abs(s[:, -1]), np.abs(s[:, -2])))).all())


def separate_near_ties(x):
    """In place: a row whose two largest logits differ by less than 1e-5 relative (and are not
    equal) gets its largest raised by 1e-3 of its size."""
    if x.shape[0] == 0 or x.shape[1] < 2:
        return x
    top = torch.topk(x, 2, dim=1)
    gap = top.values[:, 0] - top.values[:, 1]
    size = top.values.abs().max(1).values
    near = (gap > 0) & (gap < 1e-5 * size)
    rows = torch.nonzero(near).view(-1)
    x[rows, top.indices[rows, 0]] += 1e-3 * size[rows].clamp(min=1.0)
    return x


def loss_case(name, nc=7, N=300, U=500, K=40, seed=0, scales=(1.0,), sat=False, ties=True):
    g = torch.Generator().manual_seed(seed + 17 * nc)
    sc_n = torch.tensor(scales)[torch.arange(N) % len(scales)].view(-1, 1)
    sc_k = torch.tensor(scales)[torch.arange(K) % len(scales)].view(-1, 1)
    case = dict(
        name=name,
        node_cls=torch.randn(N, nc, generator=g) * 3 * sc_n,
        node_reg=torch.randn(N, 2, generator=g),
        link=torch.randn(U, 2, generator=g) * 2,
        obj=torch.randn(K, nc, generator=g) * 3 * sc_k,
        node_class=torch.randint(0, nc, (N,), generator=g),
        node_offsets=torch.randn(N, 2, generator=g) * 2,
        edge_class=torch.randint(0, 2, (U,), generator=g),
        obj_class=torch.randint(0, nc, (K,), generator=g),
        class_w=class_weights(nc), mu_sigma=LOSS_MU_SIGMA, weights=LOSS_W)
    if sat:
        case['link'], case['edge_class'] = sat_link()
    for key in ('node_cls', 'obj', 'link'):
        separate_near_ties(case[key])
    if ties:                            # exact ties: the first maximum, a tied link row is class 0
        for key, lab in (('node_cls', 'node_class'), ('obj', 'obj_class')):
            x = case[key]
            if nc >= 2 and x.shape[0] >= 6:
                for r in range(6):
                    a, b = r % nc, (r + 1 + r // 2) % nc
                    if a == b:
                        continue
                    top = x[r].abs().max() + 1.0
                    x[r, a] = x[r, b] = top
                    case[lab][r] = (min(a, b), max(a, b), (a + 2) % nc)[r % 3]
        if not sat and U >= 4:
            case['link'][:4, 1] = case['link'][:4, 0]
            case['edge_class'][:4] = torch.tensor([0, 1, 0, 1])
    return case


def loss_cases():
    out = [loss_case('second trips', N=65536 + 3, U=131072 + 77, K=5, seed=1),
           loss_case('saturation', N=300, K=40, seed=2, scales=ROW_SCALES, sat=True)]
    out += [loss_case(f'n_classes {nc}', nc=nc, N=257, U=300, K=33, seed=3) for nc in (1, 2, 7, 64)]
    out.append(loss_case('no clusters', K=0, seed=4))
    return out


# ----------------------------------------------------- 6. cross entropy and object focal loss
CE_N = (1, 255, 256, 257, 1000)
CE_NC = (1, 7, 32)
CE_G = -2.5
FOCAL_N = (1, 256, 257, 700)
FOCAL_NC = (1, 7)


def ce_case(n, nc):
    """Rows scaled by {1, 10, 100, 1e3, 1e4}, exact ties in the first rows."""
    g = torch.Generator().manual_seed(50 * n + nc)
    sc = torch.tensor(ROW_SCALES)[torch.arange(n) % 5].view(-1, 1)
    x = torch.randn(n, nc, generator=g) * 3 * sc
    k = torch.randint(0, nc, (n,), generator=g)
    separate_near_ties(x)
    if nc >= 2:
        for r in range(min(n, 6)):
            a, b = r % nc, (r + 1 + r // 2) % nc
            if a != b:
                x[r, a] = x[r, b] = x[r].abs().max() + 1.0
                k[r] = (min(a, b), max(a, b), (a + 2) % nc)[r % 3]
    return x, k


def cross_entropy_reference(x, k, g=CE_G):
    """float64: loss = sum(lse - x[k]) / n, d = g (softmax - onehot) / n with the label's entry
    as -g sum_{c != k} p_c / n (p_k - 1 without its cancellation), accuracy by first maximum."""
    xd = x.double()
    n = xd.shape[0]
    lse = torch.logsumexp(xd, 1, keepdim=True)
    loss = float((lse.view(-1) - xd.gather(1, k.view(-1, 1)).view(-1)).sum() / n)
    p = torch.exp(xd - lse)
    oh = one_hot(k, xd.shape[1], torch.bool)
    others = torch.where(oh, torch.zeros_like(p), p).sum(1, keepdim=True)
    d = torch.where(oh, -others.expand_as(p), p) * (g / n)
    return loss, d.numpy(), first_max_accuracy(x.numpy(), k.numpy())


def focal_case(n, nc):
    """The saturation grid laid into rows (cyclically), then randn * 3 rows."""
    g = torch.Generator().manual_seed(70 * n + nc)
    x = torch.randn(n, nc, generator=g) * 3
    v = torch.tensor(sat_grid(), dtype=torch.float32)
    m = min(n * nc, 4 * len(v) * nc) // nc * nc
    flat = x.view(-1)
    flat[:m] = v[(torch.arange(m) * 5) % len(v)]
    k = torch.randint(0, nc, (n,), generator=g)
    return x, k


def object_focal_reference(x, k, dtype, g=CE_G):
    """The alpha-less focal loss summed over classes and divided by n, and g d loss / d x."""
    xx = x.detach().to(dtype).clone().requires_grad_(True)
    loss = focal(xx, one_hot(k, x.shape[1], dtype), -1.0).sum() / x.shape[0]
    (loss * g).backward()
    return float(loss), xx.grad.double().numpy()
