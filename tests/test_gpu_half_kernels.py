"""The bf16 / fp16 kernels against their rounding-point emulation (tests/test_half_emulation.py):
rg_mlp_chain_fast (chain_fast_impl.h), the generic 16-bit rg_mlp_chain (mlp_chain.hip) and the
fused conv layer rg_conv_layer_fused_{waves,blocks} (conv_fused_impl.h).

Chains: every chain engine.ModelPlans builds for the yml architecture -- node and edge encoders,
conv msg (GATHER3) and upd (CONCAT2 + residual), node / offset / link (PAIRADD) / class heads,
the link head's node stem and cls_stem -- with trained and random weights, called as
engine.forward_batched calls them (ChainPlan.__call__), once with use_fast (asserting that the
fast kernel ran) and once on the generic kernel, each compared with emulate_chain of its own
rounding points, at 1, 33 and 3001 rows (3001: three input seeds and the drift check), at
100 003 rows (the persistent loops' second pass), with rows_dev below the launch rows and into
an output window.  Inputs and outputs live in buffers the test owns with sentinel rows in front
(64) and behind (128) and, for a window, sentinel columns; inputs must be unchanged afterwards.

Fused conv layer ('add' and 'mean'): test_half_emulation.hub_graph (in-degrees 0, 1, 31, 32, 33,
64, 65, a hub of 200, a whole empty 8-node run, an isolated last node, N % 8 != 0, E % 32 != 0)
through DeviceGraph.from_edge_index, and a kNN frame batch of 700, 1 and 33 nodes at k = 32,
under the wave table, the block table and plain 8-node runs; e has NaN rows past E, x_out is
prefilled with NaN between sentinel rows; every output finite, the readings against
emulate_conv within the bounds, every isolated node's row the update of a zero aggregate.

Bounds (test_half_emulation.BOUNDS): 1.5 x the worst reading measured on an MI355X over three
input seeds, both weight sets, both kernels / every schedule (profiles/half_emulation.jsonl,
written through $RG_HALF_REPORT):

    kind / type    share of elements   channels in a row   distance (spacings)   drift ratio
    chain / bf16   0.0030 -> 0.00449   40 -> 60            4.19 -> 6.27          1.034 -> 1.55
    chain / fp16   0.0263 -> 0.0394    45 -> 67            8.42 -> 12.6          1.129 -> 1.69
    conv / bf16    0.0013 -> 0.00198   4 -> 6              1.0 -> 1.5            1.002 -> 1.50
    conv / fp16    0.0040 -> 0.00594   11 -> 16            1.0 -> 1.5            1.000 -> 1.50

(measured worst -> bound; the share's worst over the runs of test_half_emulation.SMALL_NUMEL =
4096 elements or more, rows and distance over every run).  Smaller outputs -- the 1- and 33-row
runs -- are held to a count, ceil(share bound x elements) + min(row bound, output width), which
their readings above the nominal share stay inside: offset_head / random / fp16 / 33 rows 3 of 66
elements (0.045), edge_enc / random / fp16 / 1 row 5 of 64 (0.078), cls_stem / trained / bf16 /
33 rows 15 of 2112 (0.0071); edge_enc / random / fp16 / 33 rows reads 0.034, inside the nominal
0.0394.  That count is no third of a mutant's share; the distance bound separates there.  The
isolated rows of the conv layer take the nominal bounds with no allowance (every reading was 0).
The CPU noise floor of two valid evaluations of the emulation reads
0.0027 / 42 / 2.0 (chain bf16), 0.029 / 46 / 6.0 (chain fp16), 0.0004 / 2 / 0.12 (conv bf16) and
0.0059 / 8 / 1.0 (conv fp16): the kernels stand at it.  Isolated nodes' rows were bit-identical
to the update of a zero aggregate in every run.  The mildest caught mutants read 0.029 (share) /
20 (distance) for bf16 chains, 0.13 / 40.5 for fp16 chains, 0.0079 / 18 / 13.4 for the bf16 conv
layer and 0.027 / 49 / 5.0 for the fp16 one.  On an output of few elements (one row of 7
logits) the share allows one row's worth of differing elements (test_half_emulation.within).
The first measurement read 15 spacings on 5 of 100 003 fp16 edge-encoder rows: the fp16 build
rounds a multiply-add that only feeds a conversion once (v_fma_mixlo_f16), which the emulation
now does too (test_half_emulation.pack_once); the kernels were right.

Every test asserts bound <= mutant_floor / 3 (the mildest mutant caught on that metric on the
CPU), and the share it actually applies likewise, before it asserts a reading; by the floor's
construction that documents the margin -- what guards it are test_half_emulation's
mutant_is_caught tests.  The fast and the generic chain kernel are also compared with each
other.  Their weights are rounded differently (centred or not), so most elements differ at all
(share 0.3 .. 0.97, up to 61 channels of a row: reported, and no property a bound could
hold), while how far they part is a property of the chain: the largest distance is held per
chain at 1.5 x its measured worst (test_half_emulation.FAST_GENERIC: from 2.0 -> 3.0 spacings
for the fp16 update chain and 5.4 -> 8.03 for the bf16 node head to 207 -> 310 / 486 -> 728
for the trained offset head, whose two outputs nearly cancel).
"""
import json
import os

import pytest
import torch

import test_half_emulation as he
from test_chain_error_budget import error_ratios

pytestmark = pytest.mark.gpu

SENT = -776.0      # (a bf16 and fp16 value)
FRONT, BACK = 64, 128
SEEDS = (0, 1, 2)

dtype_p = pytest.mark.parametrize('dtype', list(he.HALVES))
weights_p = pytest.mark.parametrize('weights', ['trained', 'random'])
chain_p = pytest.mark.parametrize('chain', list(he.CHAINS))
aggr_p = pytest.mark.parametrize('aggr', ['add', 'mean'])


def _report(rec):
    print(json.dumps(rec))
    path = os.environ.get('RG_HALF_REPORT')
    if path:
        with open(path, 'a') as fh:
            fh.write(json.dumps(rec) + '\n')


class _Buf:
    """[FRONT + rows + BACK][ld] values of SENT; win = rows [FRONT, FRONT + rows), columns
    [col0, col0 + width).  check(): everything outside win[:written] still SENT."""

    def __init__(self, rows, width, dev, dtype, ld=None, col0=0, fill=None):
        self.rows, self.width, self.col0 = rows, width, col0
        self.buf = torch.full((FRONT + rows + BACK, ld or width), SENT, dtype=dtype, device=dev)
        self.win = self.buf[FRONT:FRONT + rows, col0:col0 + width]
        if fill is not None:
            self.win.copy_(fill)
            self.orig = self.buf.clone()

    def check(self, written=None):
        c = self.buf.clone()
        c[FRONT:FRONT + (self.rows if written is None else written),
          self.col0:self.col0 + self.width] = SENT
        assert bool((c == SENT).all()), 'a store outside the output window'

    def unchanged(self):
        assert torch.equal(self.buf.view(torch.uint8), self.orig.view(torch.uint8)), \
            'an input buffer was written'


# ------------------------------------------------------------------ models
_models = {}


def _model(weights, aggr, dev):
    """test_half_emulation.cpu_model's weights on the device (a module of its own)."""
    key = (weights, aggr)
    if key not in _models:
        from graph_neural_network_for_radar_perception_amd.config import default_config
        from graph_neural_network_for_radar_perception_amd.gnn_detector import Model_Training
        torch.manual_seed(77)
        m = Model_Training(default_config(aggregation=aggr), 'cpu')
        m.load_state_dict(he.cpu_model(weights, aggr).state_dict())
        _models[key] = m.to(dev).eval().requires_grad_(False)
    return _models[key]


def _plan(plans, chain):
    return {'node_enc': plans.node_enc, 'edge_enc': plans.edge_enc,
            'conv_msg': plans.convs[0].msg, 'conv_upd': plans.convs[0].upd,
            'node_head': plans.node_head, 'offset_head': plans.offset_head,
            'link_node': plans.link_node, 'link_pair': plans.link_pair,
            'cls_stem': plans.cls_stem, 'cls_head': plans.cls_head}[chain]


def _bounds(kind, dtype):
    """The bounds of a kind and type, each checked against the mutant floor first."""
    bound, floor = he.BOUNDS[kind, dtype], he.mutant_floor(kind, dtype)
    for k in he.METRICS:
        assert bound[k] <= floor[k] / 3, (kind, dtype, k, bound[k], floor[k])
    return bound


def _within(rd, kind, dtype, numel, width, small=True):
    """he.within, after the share it actually holds this output to is checked against the
    mutant floor: the nominal one from he.SMALL_NUMEL elements on and for small=False; the
    count rule of smaller outputs is no third of a mutant's share and is not claimed to be."""
    bound = he.BOUNDS[kind, dtype]
    share = he.share_bound(bound, numel, width, small)
    if numel >= he.SMALL_NUMEL or not small:
        assert share <= he.mutant_floor(kind, dtype)['share'] / 3, (kind, dtype, share)
    return he.within(rd, bound, numel, width, small)


# ------------------------------------------------------------------ chains
class _Case:
    """One chain of one weight set in one type: its plan, and the emulation's CPU specs."""

    def __init__(self, dev, dtype, weights, chain):
        from graph_neural_network_for_radar_perception_amd import _native as nat
        self.dev, self.dtype, self.chain, self.weights = dev, dtype, chain, weights
        self.half = he.HALVES[dtype]
        self.plan = _plan(_model(weights, 'add', dev).pred.plans(dtype), chain)
        self.specs = he.chain_specs(he.cpu_model(weights).pred)[chain]
        for a, b in zip(self.plan.specs, self.specs):
            assert torch.equal(a.weight.detach().cpu(), b.weight.detach()) and a.act == b.act
        self.mode_name, self.in_f32, self.out_half, _ = he.CHAINS[chain]
        self.mode = {'dense': nat.IN_DENSE, 'gather3': nat.IN_GATHER3, 'concat2': nat.IN_CONCAT2,
                     'pairadd': nat.IN_PAIRADD}[self.mode_name]
        self.out_dtype = self.half if self.out_half else torch.float32
        self.out_dim = self.plan.out_dim

    def buffers(self, kw):
        """The inputs of chain_inputs in sentinel buffers on the device."""
        dev = self.dev
        b = {}
        for k in ('x', 'in1', 'in2'):
            if kw.get(k) is not None:
                t = kw[k]
                b[k] = _Buf(t.shape[0], t.shape[1], dev, t.dtype, fill=t.to(dev))
        for k in ('idx0', 'idx1'):
            if kw.get(k) is not None:
                b[k] = kw[k].to(dev)
        return b

    def run(self, rows, b, out, fast, rows_dev=None):
        plan = self.plan
        plan.use_fast = fast
        plan.fast_ok = {}
        x = b['x'].win
        try:
            plan(rows, out, x, x.shape[1], mode=self.mode,
                 in1=b['in1'].win if 'in1' in b else None, w1=64 if 'in1' in b else 0,
                 in2=b['in2'].win if 'in2' in b else None, w2=64 if 'in2' in b else 0,
                 idx0=b.get('idx0'), idx1=b.get('idx1'),
                 residual=x if he.CHAINS[self.chain][3] else None, rows_dev=rows_dev)
            if fast:
                assert plan.fast_ok.get(self.mode) is True, 'the fast kernel was not taken'
            else:
                assert not plan.fast_ok
        finally:
            plan.use_fast = True
            plan.fast_ok = {}

    def emulate(self, kw, kernel, acc=torch.float32):
        with torch.no_grad():
            return he.emulate_chain(self.specs, half=self.half, acc_dtype=acc,
                                    out_half=self.out_half, kernel=kernel, **kw)

    def ref64(self, kw, kernel):
        with torch.no_grad():
            return he.ref64_chain(self.specs, half=self.half, out_half=self.out_half,
                                  kernel=kernel, **kw)


_emus = {}


def _emulated(case, rows, seed, drift):
    """(inputs, {kernel: (emulation, ref64 | None)}), computed once per chain, size and seed."""
    key = (case.dtype, case.weights, case.chain, rows, seed)
    if key not in _emus:
        kw = he.chain_inputs(case.chain, case.specs, rows, seed, case.half)
        emus = {k: (case.emulate(kw, k), case.ref64(kw, k) if drift else None)
                for k in ('fast', 'generic')}
        if rows > he.R:     # (the large cases are not kept)
            return kw, emus
        _emus[key] = (kw, emus)
    return _emus[key]


def _check_chain(case, rows, seed, test, drift=False, rows_dev=False):
    """Both kernels on `rows` rows against their emulations; the readings reported, then held."""
    bound = _bounds('chain', case.dtype)
    kw, emus = _emulated(case, rows, seed, drift)
    b = case.buffers(kw)
    outs, failures = {}, []
    for kernel in ('fast', 'generic'):
        ob = _Buf(rows, case.out_dim, case.dev, case.out_dtype)
        case.run(rows, b, ob.win, kernel == 'fast')
        ob.check()
        out = ob.win.cpu()
        assert torch.isfinite(out.float()).all()
        outs[kernel] = ob.win
        emu, r64 = emus[kernel]
        rd = he.readings(out, emu, case.half, case.out_half)
        rec = dict(test=test, kind='chain', dtype=case.dtype, chain=case.chain,
                   weights=case.weights, kernel=kernel, rows=rows, seed=seed, **rd)
        if drift:
            rms, mx = error_ratios(out, emu, r64)
            rec.update(rms_ratio=round(rms, 4), max_ratio=round(mx, 4))
            if max(rms, mx) > bound['T']:
                failures.append((kernel, 'drift', rms, mx))
        _report(rec)
        if not _within(rd, 'chain', case.dtype, out.numel(), case.out_dim):
            failures.append((kernel, rd))
        if rows_dev:
            n = rows // 2
            ob2 = _Buf(rows, case.out_dim, case.dev, case.out_dtype)
            case.run(rows, b, ob2.win, kernel == 'fast',
                     rows_dev=torch.tensor([n], dtype=torch.int32, device=case.dev))
            ob2.check(n)
            assert torch.equal(ob2.win[:n], ob.win[:n])
    for k in ('x', 'in1', 'in2'):
        if k in b:
            b[k].unchanged()
    fg = he.readings(outs['fast'].cpu(), outs['generic'].cpu().double(), case.half, case.out_half)
    _report(dict(test=test, kind='fast_generic', dtype=case.dtype, chain=case.chain,
                 weights=case.weights, rows=rows, seed=seed, **fg))
    if fg['dist'] > he.FAST_GENERIC[case.dtype][case.chain]:
        failures.append(('fast against generic', fg))
    assert not failures, failures


@dtype_p
@weights_p
@chain_p
@pytest.mark.parametrize('R', [1, 33, 3001])
def test_chain_rows(cuda_device, R, chain, weights, dtype):
    """A single row, a partial second tile, many tiles (three seeds, with the drift check):
    sentinels intact, inputs unchanged, rows_dev = R // 2 leaves the tail untouched, and the
    readings against the emulation within the bounds, for the fast and the generic kernel."""
    case = _Case(cuda_device, dtype, weights, chain)
    if R == he.R:
        for seed in SEEDS:
            _check_chain(case, R, seed, 'chain_rows', drift=True, rows_dev=seed == 0)
    else:
        _check_chain(case, R, 100 + R, 'chain_rows', rows_dev=R > 1)


@dtype_p
@pytest.mark.parametrize('chain', ['edge_enc', 'cls_stem'])
def test_chain_second_pass(cuda_device, chain, dtype):
    """100 003 rows: more 32-row tiles than the fast kernels' persistent grids hold waves (256
    workgroups of 12 waves for both chains: 98 304 rows) and more 16-row tiles than the generic
    kernel's, so waves loop -- through the encoders' next-tile prefetch (float32 rows) and
    through the plain 16-bit row loads."""
    _check_chain(_Case(cuda_device, dtype, 'trained', chain), 100_003, 7, 'chain_second_pass')


@dtype_p
@pytest.mark.parametrize('chain,ld,col0', [('node_enc', 72, 4), ('conv_upd', 80, 8),
                                           ('node_head', 8, 0), ('offset_head', 4, 0)])
def test_chain_output_window(cuda_device, chain, ld, col0, dtype):
    """Output rows as a column window of a wider buffer (77 rows): bit-identical to the
    contiguous output, every value beside the window keeps its sentinel."""
    R = 77
    case = _Case(cuda_device, dtype, 'trained', chain)
    kw = he.chain_inputs(chain, case.specs, R, 6, case.half)
    b = case.buffers(kw)
    for fast in (True, False):
        want = _Buf(R, case.out_dim, case.dev, case.out_dtype)
        case.run(R, b, want.win, fast)
        want.check()
        ob = _Buf(R, case.out_dim, case.dev, case.out_dtype, ld=ld, col0=col0)
        case.run(R, b, ob.win, fast)
        ob.check()
        assert torch.equal(ob.win, want.win)
    for k in ('x', 'in1', 'in2'):
        if k in b:
            b[k].unchanged()


# ------------------------------------------------------------------ the fused conv layer
_graphs = {}


def _hub_device_graph(dev):
    from graph_neural_network_for_radar_perception_amd.engine import DeviceGraph
    if 'hub' not in _graphs:
        ei, N = he.hub_graph()
        g = DeviceGraph.from_edge_index(ei.to(dev), N, count_pairs=False)
        _graphs['hub'] = (g, N, ei.shape[1], ei.shape[1] + 37)
    return _graphs['hub']


def _frame_device_graph(dev):
    from graph_neural_network_for_radar_perception_amd import graph_features as gf
    from graph_neural_network_for_radar_perception_amd import synthetic
    from graph_neural_network_for_radar_perception_amd.config import default_config
    if 'frames' not in _graphs:
        frames = [synthetic.make_frame(n, 70 + i) for i, n in enumerate([700, 1, 33])]
        batch = gf.FrameBatch.from_frames(frames, device=dev)
        gb = gf.build_graph_batch(batch, default_config(), k=32)
        E = int(gb.n_edges_dev.item())
        assert gb.capacity > E
        _graphs['frames'] = (gb.graph, batch.n_nodes, E, gb.capacity)
    return _graphs['frames']


SCHEDULES = ('waves', 'blocks', 'plain')


def _set_schedule(g, schedule):
    """As test_fused_conv_wave_schedule switches them: instance attributes over the class's."""
    waves, runs = {'waves': (type(g).CONV_WAVES, type(g).CONV_BLOCK_TABLE_MAX_RUNS),
                   'blocks': (0, type(g).CONV_BLOCK_TABLE_MAX_RUNS), 'plain': (0, 0)}[schedule]
    g.CONV_WAVES, g.CONV_BLOCK_TABLE_MAX_RUNS = waves, runs
    assert (g.conv_waves() is not None) == (schedule == 'waves')
    assert (g.conv_blocks()[0] is not None) == (schedule != 'plain')


def _check_conv(dev, dtype, weights, aggr, graph, seeds, test):
    from graph_neural_network_for_radar_perception_amd.engine import specs_from_modules as sp
    half = he.HALVES[dtype]
    bound = _bounds('conv', dtype)
    g, N, E, e_rows = _hub_device_graph(dev) if graph == 'hub' else _frame_device_graph(dev)
    assert int(g.seg_ptr[N].item()) == E
    seg, src, dst = g.seg_ptr.cpu(), g.src[:E].cpu(), g.dst[:E].cpu()
    if graph == 'hub':
        he.assert_hub_graph(seg, N)
    iso = (seg[1:] - seg[:-1]) == 0
    assert bool(iso[-1]) or graph != 'hub'
    assert int(iso.sum()) >= 1
    cv = _model(weights, aggr, dev).pred.plans(dtype).convs[0]
    assert cv.fused and cv.aggr == aggr
    blk = he.cpu_model(weights, aggr).pred.pass_messages.conv_blk[0]
    specs = sp(list(blk.msg)) + sp(list(blk.upd))
    failures = []
    for seed in seeds:
        x, e = he.conv_inputs(N, e_rows, seed, half)
        e[E:] = float('nan')
        with torch.no_grad():
            emu = he.emulate_conv(specs, x, e, src, dst, seg, aggr, half, torch.float32)
            r64 = he.ref64_conv(specs, x, e, src, dst, seg, aggr, half)
            zero = he.update_rows(specs[2], x[iso], torch.zeros(int(iso.sum()), 64), half,
                                  torch.float32)
        assert torch.equal(emu[iso], zero)
        xb = _Buf(N, 64, dev, half, fill=x.to(dev))
        eb = _Buf(e_rows, 64, dev, half, fill=e.to(dev))
        try:
            for schedule in SCHEDULES:
                _set_schedule(g, schedule)
                ob = _Buf(N, 64, dev, half, fill=torch.full((N, 64), float('nan')))
                assert cv.run_fused(xb.win, eb.win, g, ob.win) and cv.fused_ok
                ob.check()
                out = ob.win.cpu()
                assert torch.isfinite(out.float()).all(), 'a non-finite output'
                rd = he.readings(out, emu, half)
                rms, mx = error_ratios(out, emu, r64)
                rd_iso = he.readings(out[iso], zero, half)
                _report(dict(test=test, kind='conv', dtype=dtype, graph=graph, aggr=aggr,
                             weights=weights, schedule=schedule, seed=seed, **rd,
                             rms_ratio=round(rms, 4), max_ratio=round(mx, 4),
                             isolated=rd_iso))
                if not _within(rd, 'conv', dtype, out.numel(), 64) or max(rms, mx) > bound['T']:
                    failures.append((schedule, seed, rd, rms, mx))
                if not _within(rd_iso, 'conv', dtype, zero.numel(), 64, small=False):
                    failures.append((schedule, seed, 'isolated rows', rd_iso))
        finally:
            g.__dict__.pop('CONV_WAVES', None)               # back to the class defaults
            g.__dict__.pop('CONV_BLOCK_TABLE_MAX_RUNS', None)
        xb.unchanged()
        eb.unchanged()
    assert not failures, failures


@dtype_p
@weights_p
@aggr_p
def test_fused_conv_hub_graph(cuda_device, aggr, weights, dtype):
    """The hand-built graph under all three schedules, three input seeds."""
    _check_conv(cuda_device, dtype, weights, aggr, 'hub', SEEDS, 'fused_conv_hub_graph')


@dtype_p
@aggr_p
def test_fused_conv_frame_batch(cuda_device, aggr, dtype):
    """A kNN batch (k = 32) of frames of 700, 1 and 33 nodes: the one-node frame is isolated."""
    _check_conv(cuda_device, dtype, 'trained', aggr, 'frames', (0,), 'fused_conv_frame_batch')
