"""Gradient accumulation without a device: training.GradAccumulator's bookkeeping and errors,
the trainers' argument checks, and how train_sequence / train_dataset /
train_classifier_sequence group batches into outer iterations (a stub trainer records the
calls; the front-end stage is replaced by the identity).

Reference: modules/neural_net/gnn/training.py:189-333, classifier/training.py:138-236
(train_model_accumulate_grad: K micro-batches of (loss / K).backward(), one optimizer.step();
an empty batch contributes nothing; val_period and max_iters count outer iterations)."""
import numpy as np
import pytest
import torch

from graph_neural_network_for_radar_perception_amd import training
from graph_neural_network_for_radar_perception_amd.classifier import training as ct


class _Opt:
    def __init__(self, n=6):
        self.flat = torch.zeros(n)
        self.calls = []

    def step(self, grad, grad_scale=1.0, losses=None):
        self.calls.append((grad.clone(), grad_scale, losses.clone()))


class _Engine:
    def __init__(self, n=6, slots=4):
        self.flat_bucket = torch.zeros(n + slots)
        self.flat_grad, self.loss_slots = self.flat_bucket[:n], self.flat_bucket[n:]


# ------------------------------------------------------------------ the accumulator
def test_accumulator_errors():
    acc = training.GradAccumulator(_Opt(), 4)
    with pytest.raises(RuntimeError, match='without an open accumulation'):
        acc.apply()
    for bad in (0, -2):
        with pytest.raises(ValueError, match='n_accum'):
            acc.open(bad)
    assert acc.n_accum is None and acc.bucket is None        # nothing was begun
    acc.open(3)
    acc.open(3)
    with pytest.raises(ValueError, match='changed from 3 to 2'):
        acc.open(2)
    assert acc.apply() == 0 and acc.opt.calls == []          # world 1, nothing contributed
    with pytest.raises(RuntimeError):
        acc.apply()                                          # the apply closed it
    acc.open(2)                                              # ... so another K may follow
    assert acc.n_accum == 2


def test_accumulator_sums_in_order_and_applies_once(monkeypatch):
    opt, eng = _Opt(), _Engine()
    acc = training.GradAccumulator(opt, 4)
    reduces = []
    monkeypatch.setattr(training, 'allreduce_gradients',
                        lambda bucket, world: reduces.append((bucket, world)) or 0.5)
    K = 3
    g = torch.ones(4) / K
    grads = [torch.randn(6, generator=torch.Generator().manual_seed(s)) for s in (1, 2)]
    losses = [torch.tensor([1.0, 2.0, 3.0, 4.0]), torch.tensor([0.5, 0.25, 7.0, 1e-3])]
    acc.open(K)                                              # an empty micro-batch
    for gr, lo in zip(grads, losses):
        acc.open(K)
        assert torch.equal(acc.g(K), g)
        eng.flat_grad.copy_(gr)
        acc.add(eng, lo)
        assert torch.equal(eng.loss_slots, lo * g)
    assert acc.count == 2 and acc.g(K) is acc.g(K)           # made once per K
    assert acc.apply() == 2
    assert len(reduces) == 1 and reduces[0][0] is acc.bucket and reduces[0][1] == 1
    (grad, scale, slots), = opt.calls
    assert scale == 0.5
    assert torch.equal(grad, grads[0] + grads[1])
    assert torch.equal(slots, losses[0] * g + losses[1] * g)
    # the next accumulation starts from its first micro-batch, not from the old sum
    acc.open(1)
    eng.flat_grad.copy_(grads[1])
    acc.add(eng, losses[1])
    assert acc.apply() == 1
    assert torch.equal(opt.calls[1][0], grads[1]) and torch.equal(opt.calls[1][2], losses[1])


def test_accumulator_without_a_contribution_joins_the_allreduce_on_several_ranks(monkeypatch):
    opt = _Opt()
    acc = training.GradAccumulator(opt, 1)
    seen = []

    def reduce(bucket, world):
        seen.append((bucket.clone(), world))
        return 0.5

    monkeypatch.setattr(training, 'allreduce_gradients', reduce)
    acc.open(3)
    acc.bucket.fill_(3.0)                                    # stale values the apply must clear
    assert acc.apply(2) == 0
    (bucket, world), = seen
    assert world == 2 and not bool(bucket[:6].any()) and bool(torch.isnan(bucket[6:]).all())
    assert len(opt.calls) == 1 and bool(torch.isnan(opt.calls[0][2]).all())


def test_accumulator_refuses_another_engine_layout():
    acc = training.GradAccumulator(_Opt(6), 4)
    acc.open(2)
    with pytest.raises(ValueError, match='bucket'):
        acc.add(_Engine(7, 4), torch.zeros(4))
    with pytest.raises(RuntimeError):
        training.GradAccumulator(_Opt(6), 4).add(_Engine(), torch.zeros(4))


# ------------------------------------------------------------------ the trainers' checks
class _Empty:
    n_frames = 0
    n_objects = 0


def _bare(cls, slots):
    """A trainer with its accumulator only: the checks below run before anything else is used."""
    tr = cls.__new__(cls)
    tr.world = 1
    tr.opt = _Opt()
    tr.accum = training.GradAccumulator(tr.opt, slots)
    return tr


@pytest.mark.parametrize('which', ['detector', 'classifier'])
def test_trainer_argument_checks(which):
    if which == 'detector':
        tr = _bare(training.RadarGNNTrainer, 4)
        calls = [lambda k: tr.accumulate(None, {}, k), lambda k: tr.accumulate_frames(_Empty(), k)]
        empty = lambda k: tr.accumulate_frames(_Empty(), k)           # noqa: E731
    else:
        tr = _bare(ct.ClassifierTrainer, 1)
        calls = [lambda k: tr.accumulate_objects(None, None, None, None, None, 0, 0, 0, k),
                 lambda k: tr.accumulate_inputs(None, k)]
        empty = lambda k: tr.accumulate_inputs(_Empty(), k)           # noqa: E731
    with pytest.raises(RuntimeError, match='without an open accumulation'):
        tr.apply_accumulated()
    for call in calls:
        for bad in (0, -1):
            with pytest.raises(ValueError, match='n_accum'):
                call(bad)
    assert empty(3) is None                                  # opens the accumulation
    for call in calls:
        with pytest.raises(ValueError, match='changed from 3 to 4'):
            call(4)
    assert tr.apply_accumulated() == 0 and tr.opt.calls == []
    with pytest.raises(RuntimeError):
        tr.apply_accumulated()


# ------------------------------------------------------------------ the loops' grouping
class _Dev:
    device = torch.device('cpu')


class _StubTrainer:
    """Records every call; a batch is its positions, and one that holds a negative position
    stands for an empty batch."""

    def __init__(self):
        self.engine = _Dev()
        self.opt = _Opt()
        self.log = []

    def _out(self, pos):
        if (np.asarray(pos) < 0).any():
            return None
        return torch.full((4,), float(pos[0])), torch.zeros(3), None

    def step_frames(self, pos):
        self.log.append(('step', list(pos)))
        return self._out(pos)

    def accumulate_frames(self, pos, n_accum):
        self.log.append(('acc', list(pos), n_accum))
        return self._out(pos)

    def step_inputs(self, pos):
        self.log.append(('step', list(pos)))
        out = self._out(pos)
        return None if out is None else out[0][:1]

    def accumulate_inputs(self, pos, n_accum):
        self.log.append(('acc', list(pos), n_accum))
        out = self._out(pos)
        return None if out is None else out[0][:1]

    def apply_accumulated(self):
        self.log.append(('apply',))

    def save(self, path):
        self.log.append(('save', path))


class _Cfg:
    dataset_augmentation = False
    max_train_iter = 4


class _Set:
    def n_windows(self, window_size):
        return 10


@pytest.fixture
def identity_feed(monkeypatch):
    """The front-end stages replaced by the identity: the trainer is handed the positions."""
    def train_batch(store, trainer, pos, window_size, augmentation, ransac, n_accum=None):
        if n_accum is None:
            return None, trainer.step_frames(pos)
        return None, trainer.accumulate_frames(pos, n_accum)

    monkeypatch.setattr(training, '_train_batch', train_batch)
    monkeypatch.setattr(ct, '_sequence_inputs', lambda store, detector, cfg, pos, *a: pos)


@pytest.mark.parametrize('bad', [0, -3])
def test_loops_refuse_less_than_one_accumulation_step(identity_feed, bad):
    tr = _StubTrainer()
    with pytest.raises(ValueError, match='grad_accumulation_steps'):
        training.train_sequence(None, tr, _Cfg(), [0, 1], grad_accumulation_steps=bad)
    with pytest.raises(ValueError, match='grad_accumulation_steps'):
        training.train_dataset(_Set(), tr, _Cfg(), grad_accumulation_steps=bad)
    with pytest.raises(ValueError, match='grad_accumulation_steps'):
        ct.train_classifier_sequence(None, None, tr, _Cfg(), [0, 1],
                                     grad_accumulation_steps=bad)
    assert tr.log == []


def test_train_sequence_groups(identity_feed):
    order = [14, 3, 9, 0, 20, 7, 7, 11, 1, 18, 5, 16, 2]
    tr, seen = _StubTrainer(), []
    losses, acc = training.train_sequence(
        None, tr, _Cfg(), order, batch_windows=3, grad_accumulation_steps=2,
        on_step=lambda k, pos, flags, out: seen.append((k, list(pos), len(tr.log))))
    b = [order[i:i + 3] for i in range(0, 13, 3)]
    assert tr.log == [('acc', b[0], 2), ('acc', b[1], 2), ('apply',), ('acc', b[2], 2),
                      ('acc', b[3], 2), ('apply',), ('acc', b[4], 2), ('apply',)]
    assert [s[0] for s in seen] == [0, 0, 1, 1, 2] and [s[1] for s in seen] == b
    assert [s[2] for s in seen] == [1, 3, 4, 6, 8]           # a group's last one: after the apply
    assert losses.shape == (5, 4) and acc.shape == (5, 3)
    assert losses[:, 0].tolist() == [float(x[0]) for x in b]
    # K = 1: today's path, no accumulate call
    tr1, seen1 = _StubTrainer(), []
    training.train_sequence(None, tr1, _Cfg(), order, batch_windows=3,
                            on_step=lambda k, pos, flags, out: seen1.append(k))
    assert tr1.log == [('step', x) for x in b] and seen1 == [0, 1, 2, 3, 4]
    # an empty micro-batch keeps its place in the group and gives no row
    tr2 = _StubTrainer()
    lo, _ = training.train_sequence(None, tr2, _Cfg(), [4, -1, 6, 8], batch_windows=1,
                                    grad_accumulation_steps=3)
    assert tr2.log == [('acc', [4], 3), ('acc', [-1], 3), ('acc', [6], 3), ('apply',),
                       ('acc', [8], 3), ('apply',)]
    assert lo[:, 0].tolist() == [4.0, 6.0, 8.0]


def test_train_dataset_groups(identity_feed, monkeypatch):
    tr, seen, vals = _StubTrainer(), [], []
    monkeypatch.setattr(training, 'validate_sequence',
                        lambda *a: tr.log.append(('validate',)) or (1, 2, 3, 4, 5))
    torch.manual_seed(3)
    losses, acc, validations = training.train_dataset(
        _Set(), tr, _Cfg(), val_set=_Set(), max_iters=3, batch_windows=2, val_period=2,
        weights_path='w.pth', grad_accumulation_steps=2,
        on_step=lambda it, pos, flags, out: seen.append((it, list(pos))),
        on_validation=lambda it, res: vals.append(it))
    torch.manual_seed(3)
    gen = training.shuffled_batches(10, 2)
    want = [list(next(gen)) for _ in range(6)]
    assert [s[1] for s in seen] == want and [s[0] for s in seen] == [0, 0, 1, 1, 2, 2]
    tail = [('save', 'w.pth'), ('validate',)]
    assert tr.log == ([('acc', want[0], 2), ('acc', want[1], 2), ('apply',)] + tail
                      + [('acc', want[2], 2), ('acc', want[3], 2), ('apply',)]
                      + [('acc', want[4], 2), ('acc', want[5], 2), ('apply',)] + tail)
    assert vals == [0, 2] and [v[0] for v in validations] == [0, 2]
    assert losses.shape == (6, 4) and acc.shape == (6, 3)
    # K = 1 draws one batch per iteration through step_frames
    tr1 = _StubTrainer()
    torch.manual_seed(3)
    training.train_dataset(_Set(), tr1, _Cfg(), max_iters=3, batch_windows=2, val_period=1000)
    assert tr1.log == [('step', w) for w in want[:3]]


def test_train_classifier_sequence_groups(identity_feed):
    tr, seen = _StubTrainer(), []
    losses = ct.train_classifier_sequence(
        None, None, tr, _Cfg(), [5, 6, 7, -1, 9, 10, 11], batch_windows=2,
        grad_accumulation_steps=2,
        on_step=lambda k, pos, flags, loss, inp: seen.append((k, list(pos), loss is None)))
    assert tr.log == [('acc', [5, 6], 2), ('acc', [7, -1], 2), ('apply',), ('acc', [9, 10], 2),
                      ('acc', [11], 2), ('apply',)]
    assert seen == [(0, [5, 6], False), (0, [7, -1], True), (1, [9, 10], False),
                    (1, [11], False)]
    assert losses.tolist() == [5.0, 9.0, 11.0]
    tr1 = _StubTrainer()
    ct.train_classifier_sequence(None, None, tr1, _Cfg(), [5, 6, 7], batch_windows=2)
    assert tr1.log == [('step', [5, 6]), ('step', [7])]
