"""engine.PackedImages as a state machine, without a GPU: the native library is replaced by a
stub that records every rg_pack_linear / rg_pack_linear_ld call, the tensors live on the CPU."""
import pytest
import torch

from graph_neural_network_for_radar_perception_amd import _native as nat
from graph_neural_network_for_radar_perception_amd import engine

F32, FAST = nat.RG_F32, nat.RG_PACK_F32_FAST
DIMS = [6, 40, 24, 7]      # a chain 6 -> 40 -> 24 -> 7


class _Lib:
    """Records (weight ptr, bias ptr, in_dim, out_dim, fmt with RG_PACK_TRANSPOSE, ld, packed)."""

    def __init__(self):
        self.packs = []

    def rg_packed_linear_bytes(self, in_dim, out_dim, fmt):
        return 4 * (in_dim * out_dim + out_dim) + 4      # no multiple of 256: offsets get aligned

    def rg_pack_linear(self, w, b, in_dim, out_dim, fmt, packed, stream):
        self.packs.append((w, b, in_dim, out_dim, fmt, 0, packed))
        return 0

    def rg_pack_linear_ld(self, w, b, in_dim, out_dim, fmt, ld, packed, stream):
        self.packs.append((w, b, in_dim, out_dim, fmt, ld, packed))
        return 0


@pytest.fixture
def lib(monkeypatch):
    stub = _Lib()
    monkeypatch.setattr(nat, 'lib', lambda: stub)
    monkeypatch.setattr(nat, 'stream_ptr', lambda device=None: 0)
    return stub


def _specs(dims=DIMS):
    g = torch.Generator().manual_seed(1)
    return [engine.LayerSpec(torch.randn(o, i, generator=g), torch.randn(o, generator=g),
                             torch.randn(1, generator=g), torch.rand(1, generator=g) + 0.5,
                             'leakyrelu') for i, o in zip(dims[:-1], dims[1:])]


def _request_all(im):
    """One image set of every kind; returns their keys."""
    n = len(im.specs)
    keys = [((F32,) * n, False, None), ((FAST,) * n, False, None), ((F32,) * n, True, None),
            ((FAST,) * n, True, None), ((F32,), True, (0, 2, 3)), ((FAST,), True, (1, 8, 16))]
    for k in keys:
        im.get(*k)
    return keys


def _n_images(im, keys):
    return sum(1 if k[2] is not None else len(im.specs) for k in keys)


def test_second_request_does_not_pack(lib):
    im = engine.PackedImages(_specs(), 'cpu')
    keys = _request_all(im)
    assert len(lib.packs) == _n_images(im, keys)
    first = [im.get(*k) for k in keys]
    again = [im.get(*k) for k in keys]
    assert len(lib.packs) == _n_images(im, keys)
    assert all(a is b for a, b in zip(first, again))
    assert sorted(map(repr, im.held())) == sorted(map(repr, keys))
    # images of one set lie at 256-byte aligned offsets of one buffer, in layer order
    base = lib.packs[0][6]
    assert [p[6] - base for p in lib.packs[:3]] == [0, 1280, 5376]


def test_descriptors(lib):
    specs = _specs()
    im = engine.PackedImages(specs, 'cpu')
    (arr, n, out_dim), = im.get((F32,) * 3)
    assert (n, out_dim) == (3, 7)
    for d, s, p in zip(arr, specs, lib.packs):
        assert (d.in_dim, d.out_dim, d.flags) == (s.in_dim, s.out_dim, 0)
        assert d.act == nat.ACT['leakyrelu']
        assert (d.w_packed, d.norm_mu, d.norm_std) == (p[6], s.mu.data_ptr(), s.std.data_ptr())
    flagged = tuple(f | nat.RG_PACK_H2 | nat.RG_PACK_CENTERED
                    for f in (nat.RG_PACK_FAST_IN, nat.RG_PACK_FAST_CHAIN, nat.RG_PACK_FAST_CHAIN))
    arr = im.get(flagged)[0][0]
    assert all(d.flags == nat.RG_LAYER_H2 | nat.RG_LAYER_CENTERED for d in arr)
    assert [p[4] for p in lib.packs[3:]] == list(flagged)
    # transposed: one bare Linear per layer with the dims swapped
    groups = im.get((FAST,) * 3, True)
    assert len(groups) == 3
    for (arr, n, out_dim), s in zip(groups, specs):
        d = arr[0]
        assert (n, out_dim, d.in_dim, d.out_dim) == (1, s.in_dim, s.out_dim, s.in_dim)
        assert (d.act, d.flags, d.norm_mu, d.norm_std) == (0, 0, None, None)
    assert all(p[1] is None and p[4] == FAST | nat.RG_PACK_TRANSPOSE for p in lib.packs[6:])


def test_version_bump_makes_held_images_stale(lib):
    specs = _specs()
    im = engine.PackedImages(specs, 'cpu')
    keys = _request_all(im)[:4]         # the column blocks stay as they are below
    assert not im.refresh()
    with torch.no_grad():
        specs[1].weight.add_(1.0)
    assert im.refresh() and im.held() == []
    assert im.jobs() is None
    del lib.packs[:]
    for k in keys[:2]:
        im.get(*k)
    assert len(lib.packs) == 6 and len(im.held()) == 2      # only what was requested again
    for k in keys:
        im.get(*k)
    assert len(lib.packs) == 12 and len(im.held()) == 4
    assert not im.refresh()


def test_data_write_needs_invalidate(lib):
    specs = _specs()
    im = engine.PackedImages(specs, 'cpu')
    keys = _request_all(im)
    total = _n_images(im, keys)
    specs[0].weight.data.add_(1.0)      # behind the version counter
    assert not im.refresh()
    for k in keys:
        im.get(*k)
    assert len(lib.packs) == total
    im.invalidate()
    assert im.held() == []
    for k in keys:
        im.get(*k)
    assert len(lib.packs) == 2 * total
    assert lib.packs[total:] == lib.packs[:total]      # into the same buffers


def test_jobs_mirror_the_first_pack(lib):
    specs = _specs()
    im = engine.PackedImages(specs, 'cpu')
    keys = _request_all(im)
    jobs = im.jobs()
    assert len(jobs) == len(lib.packs) == _n_images(im, keys)
    as_pack = [(j.weight, j.bias, j.in_dim, j.out_dim,
                j.fmt | (nat.RG_PACK_TRANSPOSE if j.transpose else 0), j.ld, j.packed)
               for j in jobs]
    assert as_pack == lib.packs
    assert all(j.fmt in (F32, FAST) for j in jobs)
    blk = as_pack[-2]       # W_0[:, 2:5] transposed
    s = specs[0]
    assert blk[:6] == (s.weight.data_ptr() + 4 * 2, None, s.out_dim, 3,
                       F32 | nat.RG_PACK_TRANSPOSE, s.in_dim)
    whole = as_pack[0]
    assert whole[:6] == (s.weight.data_ptr(), s.bias.data_ptr(), s.in_dim, s.out_dim, F32, 0)


@pytest.mark.parametrize('fmt', [nat.RG_BF16, nat.RG_PACK_FAST_IN | nat.RG_PACK_H2,
                                 nat.RG_PACK_FAST_IN | nat.RG_PACK_X3, FAST | nat.RG_PACK_CENTERED])
def test_jobs_none_for_other_formats(lib, fmt):
    im = engine.PackedImages(_specs(), 'cpu')
    assert im.jobs() is None                # nothing packed
    im.get((FAST,) * 3)
    assert im.jobs() is None                # the generic image does not exist yet
    im.get((F32,) * 3)
    assert len(im.jobs()) == 6
    im.get((fmt,) * 3)
    assert im.jobs() is None


def test_jobs_none_when_an_image_is_packed_from_a_copy(lib):
    """The in-place launch reads the parameters where they lie: a converted weight, or specs
    derived from other parameters (sources), leave only the ordinary re-pack."""
    specs = _specs()
    specs[1].weight = specs[1].weight.double()
    im = engine.PackedImages(specs, 'cpu')
    im.get((F32,) * 3)
    assert im.jobs() is None
    derived = engine.PackedImages(_specs(), 'cpu', sources=_specs())
    derived.get((F32,) * 3)
    assert derived.jobs() is None


def test_seventeen_layers_in_full_groups_and_a_rest(lib):
    """A launch takes RG_MAX_LAYERS = 8 layers: 17 layers are two full groups and one of 1."""
    assert nat.MAX_LAYERS == 8
    specs = _specs([5] * 18)
    im = engine.PackedImages(specs, 'cpu')
    groups = im.get((F32,) * 17)
    assert [n for _, n, _ in groups] == [8, 8, 1]
    flat = [d.w_packed for arr, n, _ in groups for d in arr]
    assert flat == [p[6] for p in lib.packs] and len(set(flat)) == 17
    assert len(im.jobs()) == 17


def test_pack_specs_and_layer_array_match_a_request(lib):
    """The stand-alone helpers pack and describe exactly what a request does."""
    specs = _specs()
    fmts = [nat.RG_PACK_FAST_IN | nat.RG_PACK_H2 | nat.RG_PACK_CENTERED,
            nat.RG_PACK_FAST_CHAIN | nat.RG_PACK_H2, nat.RG_PACK_FAST_CHAIN | nat.RG_PACK_H2]
    buf, offs = engine.pack_specs(specs, fmts, 'cpu')
    arr = engine.layer_array(specs, buf.data_ptr(), offs, fmts)
    want = engine.PackedImages(specs, 'cpu').get(tuple(fmts))[0][0]
    assert offs == [0, 1280, 5376]
    assert [p[:6] for p in lib.packs[:3]] == [p[:6] for p in lib.packs[3:]]
    for a, b, off in zip(arr, want, offs):
        assert a.w_packed == buf.data_ptr() + off
        assert ([getattr(a, f) for f, _ in nat.rg_layer._fields_ if f != 'w_packed']
                == [getattr(b, f) for f, _ in nat.rg_layer._fields_ if f != 'w_packed'])
    assert [d.flags for d in arr] == [nat.RG_LAYER_H2 | nat.RG_LAYER_CENTERED, nat.RG_LAYER_H2,
                                      nat.RG_LAYER_H2]
