"""Every packed weight image (rg_pack_linear, rg_pack_linear_ld, rg_pack_linear_jobs), byte for
byte against a numpy packer written from the documented formats (include/radar_gnn.h),
not from the library's layout header: a packer and a kernel that drift apart show here, not as a
numerical failure far downstream.

The formats, W a Linear(in -> out) weight [out][in], image element t of a plane:
  RG_F32            float [m][s4][lane][e]   o = 16m + lane % 16, k = 16 s4 + 4 (lane / 16) + e
  RG_BF16           16-bit [m][s][lane][j]   o = 16m + lane % 16, k = 32 s + 8 (lane / 16) + j
  RG_PACK_F32_FAST  float [m][s4][lane][u]   o = 32m + lane % 32, k = 8 s4 + 4 (lane / 32) + u
  RG_PACK_FAST_*    16-bit [m][s][lane][j]   o = 32m + lane % 32, h = lane / 32,
       k-step s read from memory       k = 16 s + 8 h + j
       k-step s read from accumulators k = 32 (s / 2) + 16 (s % 2) + 8 (j / 4) + 4 h + j % 4
       FAST_IN: every step from memory; FAST_CHAIN: every step from accumulators; FAST_UPD: the
       steps of the first in / 2 columns from memory, the rest from accumulators (offset in / 2)
padding is zero.  The bias follows the planes as float32: in plain order padded to 16 (RG_F32,
RG_BF16) or to 32 (RG_BF16 | RG_PACK_X3), or in 32x32 accumulator order padded to 32 (every
32-row format): entry 32m + 16h + 4g + j = b[32m + 8g + 4h + j].
RG_PACK_X3: planes bf16(w), bf16(w - p0), bf16(w - p0 - p1), residues exact in float32.
RG_PACK_F16: IEEE fp16 instead of bf16.  RG_PACK_CENTERED: column k of W minus its mean over the
outputs (a sequential float32 sum, one float32 divide), the bias likewise.  RG_PACK_H2: s with
max |w| 2^s in [2^12, 2^13), |s| <= 64 (0 for an all-zero or non-finite maximum); planes
fp16(w 2^s), fp16(w 2^s - p0); the bias times 2^s; then 16 bytes {2^-s, 2^s, (int) s, 0}.

Shapes: (7, 64) a padded k-step, (64, 7) a padded M-tile, (40, 48) both and more than one of
each for the 16-row formats, (128, 64) several of each and the FAST_UPD split.
"""
import numpy as np
import pytest
import torch

from graph_neural_network_for_radar_perception_amd import _native as nat

pytestmark = pytest.mark.gpu

F32, BF16 = nat.RG_F32, nat.RG_BF16
FIN, FCH, FUPD, F32F = (nat.RG_PACK_FAST_IN, nat.RG_PACK_FAST_CHAIN, nat.RG_PACK_FAST_UPD,
                        nat.RG_PACK_F32_FAST)
CEN, TR, X3, F16, H2 = (nat.RG_PACK_CENTERED, nat.RG_PACK_TRANSPOSE, nat.RG_PACK_X3,
                        nat.RG_PACK_F16, nat.RG_PACK_H2)
FAST = (FIN, FCH, FUPD)
SHAPES = [(7, 64), (64, 7), (40, 48), (128, 64)]
GUARD = 256  # sentinel bytes behind every image: a write past its size is seen
NAMES = {F32: 'f32', BF16: 'bf16', FIN: 'fast_in', FCH: 'fast_chain', FUPD: 'fast_upd',
         F32F: 'f32_fast'}
FLAG_NAMES = {CEN: 'centered', TR: 'transpose', X3: 'x3', F16: 'f16', H2: 'h2'}


def combos():
    out = [F32, F32 | TR, BF16, BF16 | F16, BF16 | X3, BF16 | X3 | TR, F32F, F32F | TR]
    for f in FAST:
        out += [f, f | CEN, f | F16, f | F16 | CEN, f | X3, f | X3 | CEN]
    for f in (FIN, FCH):
        out += [f | H2, f | H2 | CEN]
    return out


def fmt_id(flags):
    return '-'.join([NAMES[flags & 0xff]] + [n for b, n in FLAG_NAMES.items() if flags & b])


# ------------------------------------------------------------------ the numpy packer
def ceil_to(n, p):
    return (n + p - 1) // p * p


def to_bf16(v):
    """float32 -> bf16 bits, round to nearest even (finite values)."""
    u = v.astype(np.float32).view(np.uint32).astype(np.uint64)
    return ((u + 0x7fff + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def from_bf16(h):
    return (h.astype(np.uint32) << 16).view(np.float32)


def to_f16(v):
    with np.errstate(over='ignore'):
        return v.astype(np.float32).astype(np.float16).view(np.uint16)


def from_f16(h):
    return h.view(np.float16).astype(np.float32)


def element_map(base, in_dim, out_dim):
    """(o, k) of every element of one plane, in image order."""
    if base in (F32, F32F):
        rows, kstep, per_lane = (16, 16, 4) if base == F32 else (32, 8, 4)
    else:
        rows, kstep, per_lane = (16, 32, 8) if base == BF16 else (32, 16, 8)
    mt, ks = ceil_to(out_dim, rows) // rows, ceil_to(in_dim, kstep) // kstep
    m, s, lane, j = np.meshgrid(np.arange(mt), np.arange(ks), np.arange(64), np.arange(per_lane),
                                indexing='ij')
    o = rows * m + lane % rows
    hi = lane // rows  # which group of lanes: 0..3 for 16-row tiles, 0..1 for 32-row tiles
    if base in (F32, BF16, F32F):
        k = kstep * s + per_lane * hi + j
    else:
        mem = {FIN: ks, FCH: 0, FUPD: ks // 2}[base]
        sc = s - mem
        k_mem = 16 * s + 8 * hi + j
        k_acc = 16 * mem + 32 * (sc // 2) + 16 * (sc % 2) + 8 * (j // 4) + 4 * hi + j % 4
        k = np.where(s < mem, k_mem, k_acc)
    return o.reshape(-1), k.reshape(-1)


def bias_order(n, accumulator):
    t = np.arange(n)
    if not accumulator:
        return t
    return 32 * (t >> 5) + 8 * ((t >> 2) & 3) + 4 * ((t >> 4) & 1) + (t & 3)


def seq_sum(a):
    """float32 sum over axis 0, one element after the other."""
    return np.cumsum(a, axis=0, dtype=np.float32)[-1]


def reference_image(W, b, in_dim, out_dim, flags):
    """W: the [out][in] float32 layer (already un-transposed); the image's bytes."""
    base = flags & 0xff
    W = W.astype(np.float32)
    if flags & CEN:
        W = W - seq_sum(W) / np.float32(out_dim)
    o, k = element_map(base, in_dim, out_dim)
    ok = (o < out_dim) & (k < in_dim)
    v = np.where(ok, W[np.minimum(o, out_dim - 1), np.minimum(k, in_dim - 1)], np.float32(0))
    v = v.astype(np.float32)

    wide = base in FAST or base == F32F
    nb = ceil_to(out_dim, 32 if (wide or flags & X3) else 16)
    f = bias_order(nb, wide)
    bias = np.zeros(nb, np.float32)
    if b is not None:
        bb = b.astype(np.float32)
        if flags & CEN:
            bb = bb - seq_sum(bb) / np.float32(out_dim)
        bias = np.where(f < out_dim, bb[np.minimum(f, out_dim - 1)], np.float32(0))
        bias = bias.astype(np.float32)

    if flags & H2:
        mx = np.float32(np.abs(W).max())
        s = 0
        if mx > 0 and np.isfinite(mx):
            s = int(min(max(13 - int(np.frexp(mx)[1]), -64), 64))
        up = np.float32(2.0) ** np.float32(s)
        with np.errstate(over='ignore', invalid='ignore'):
            vs = v * up
            p0 = to_f16(vs)
            p1 = to_f16(vs - from_f16(p0))
            bias = bias * up
        trailer = np.array([np.float32(2.0) ** np.float32(-s), up], np.float32).tobytes() + \
            np.array([s, 0], np.int32).tobytes()
        return p0.tobytes() + p1.tobytes() + bias.tobytes() + trailer
    if flags & X3:
        p0 = to_bf16(v)
        r1 = v - from_bf16(p0)
        p1 = to_bf16(r1)
        p2 = to_bf16(r1 - from_bf16(p1))
        return p0.tobytes() + p1.tobytes() + p2.tobytes() + bias.tobytes()
    if base in (F32, F32F):
        return v.tobytes() + bias.tobytes()
    return (to_f16(v) if flags & F16 else to_bf16(v)).tobytes() + bias.tobytes()


# ------------------------------------------------------------------ the library
@pytest.fixture(scope='module')
def lib():
    return nat.lib()


def image_bytes(lib, in_dim, out_dim, flags):
    return int(lib.rg_packed_linear_bytes(in_dim, out_dim, flags))


def new_image(n):
    return torch.full((n + GUARD,), 0xA5, dtype=torch.uint8, device='cuda')


def read_image(img):
    torch.cuda.synchronize()
    raw = img.cpu().numpy().tobytes()
    assert raw[-GUARD:] == b'\xa5' * GUARD, 'the pack wrote past rg_packed_linear_bytes'
    return raw[:-GUARD]


def weights(in_dim, out_dim, kind, seed):
    rng = np.random.default_rng(seed)
    W = rng.standard_normal((out_dim, in_dim)).astype(np.float32)
    b = rng.standard_normal(out_dim).astype(np.float32)
    if kind == 'zero':
        W[:] = 0
    elif kind == 'tiny':
        W *= np.float32(1e-30)
    elif kind == 'huge':
        W *= np.float32(1e30)
    return W, b


def storage(W, transpose, ld):
    """The matrix as the pack call reads it: [in][out] when transposed, rows ld floats apart
    (the columns beyond the row filled with a value no image may contain)."""
    A = np.ascontiguousarray(W.T if transpose else W)
    if ld:
        wide = np.full((A.shape[0], ld), 12345.0, np.float32)
        wide[:, :A.shape[1]] = A
        A = wide
    return torch.from_numpy(A).cuda()


def first_difference(got, ref):
    if len(got) != len(ref):
        return f'{len(got)} bytes, expected {len(ref)}'
    g, r = np.frombuffer(got, np.uint8), np.frombuffer(ref, np.uint8)
    d = np.flatnonzero(g != r)
    return f'{d.size} bytes differ, the first at byte {d[0]} of {len(ref)}' if d.size else ''


def pack(lib, W, b, in_dim, out_dim, flags, ld=None):
    Wd = storage(W, bool(flags & TR), ld or 0)
    bd = None if b is None else torch.from_numpy(b).cuda()
    img = new_image(image_bytes(lib, in_dim, out_dim, flags))
    st = nat.stream_ptr()
    if ld is None:
        rc = lib.rg_pack_linear(nat.ptr(Wd), nat.ptr(bd), in_dim, out_dim, flags, nat.ptr(img), st)
    else:
        rc = lib.rg_pack_linear_ld(nat.ptr(Wd), nat.ptr(bd), in_dim, out_dim, flags, ld,
                                   nat.ptr(img), st)
    nat.check(rc, 'rg_pack_linear')
    return read_image(img)


def shapes_of(flags):
    return [s for s in SHAPES if (flags & 0xff) != FUPD or s == (128, 64)]


CASES = [(f, s) for f in combos() for s in shapes_of(f)]


@pytest.mark.parametrize('flags,shape', CASES, ids=[f'{fmt_id(f)}-{s[0]}x{s[1]}' for f, s in CASES])
def test_pack_linear_bytes(lib, flags, shape):
    in_dim, out_dim = shape
    kinds = ['normal', 'zero'] + (['tiny', 'huge'] if flags & H2 else [])
    for kind in kinds:
        W, b = weights(in_dim, out_dim, kind, seed=in_dim * 1000 + out_dim)
        for bias in (b, None):
            ref = reference_image(W, bias, in_dim, out_dim, flags)
            assert len(ref) == image_bytes(lib, in_dim, out_dim, flags)
            got = pack(lib, W, bias, in_dim, out_dim, flags)
            assert got == ref, f'{kind}, bias {bias is not None}: {first_difference(got, ref)}'


LD_CASES = [(f, s) for f in (F32, F32 | TR, F32F, F32F | TR) for s in SHAPES]


@pytest.mark.parametrize('flags,shape', LD_CASES,
                         ids=[f'{fmt_id(f)}-{s[0]}x{s[1]}' for f, s in LD_CASES])
def test_pack_linear_ld_bytes(lib, flags, shape):
    in_dim, out_dim = shape
    W, b = weights(in_dim, out_dim, 'normal', seed=7 + in_dim)
    row = out_dim if flags & TR else in_dim
    for ld in (0, row, row + 5, 200):
        for bias in (b, None):
            ref = reference_image(W, bias, in_dim, out_dim, flags)
            got = pack(lib, W, bias, in_dim, out_dim, flags, ld=ld)
            assert got == ref, f'ld {ld}, bias {bias is not None}: {first_difference(got, ref)}'


def test_pack_linear_jobs_bytes(lib):
    """A mixed list of f32 jobs in one launch: every image is the reference's, which the
    individual packs above equal."""
    specs = []
    for i, (in_dim, out_dim) in enumerate(SHAPES):
        for fmt in (F32, F32F):
            for transpose in (0, 1):
                row = out_dim if transpose else in_dim
                ld = (0, row + 3)[(i + transpose) % 2]
                specs.append((in_dim, out_dim, fmt, transpose, ld, (i + fmt + transpose) % 3 != 0))
    keep, jobs, images, refs = [], (nat.rg_pack_job * len(specs))(), [], []
    for j, (in_dim, out_dim, fmt, transpose, ld, has_bias) in enumerate(specs):
        W, b = weights(in_dim, out_dim, 'normal', seed=100 + j)
        Wd = storage(W, bool(transpose), ld)
        bd = torch.from_numpy(b).cuda() if has_bias else None
        img = new_image(image_bytes(lib, in_dim, out_dim, fmt))
        keep += [Wd, bd]
        images.append(img)
        refs.append(reference_image(W, b if has_bias else None, in_dim, out_dim, fmt))
        jobs[j].weight, jobs[j].bias, jobs[j].packed = nat.ptr(Wd), nat.ptr(bd), nat.ptr(img)
        jobs[j].in_dim, jobs[j].out_dim, jobs[j].fmt = in_dim, out_dim, fmt
        jobs[j].transpose, jobs[j].ld = transpose, ld
    raw = np.frombuffer(bytes(jobs), np.uint8).copy()
    jobs_dev = torch.from_numpy(raw).cuda()
    nat.check(lib.rg_pack_linear_jobs(nat.ptr(jobs_dev), len(specs), nat.stream_ptr()),
              'rg_pack_linear_jobs')
    for spec, img, ref in zip(specs, images, refs):
        got = read_image(img)
        assert got == ref, f'{spec}: {first_difference(got, ref)}'


def test_h2_scale_rule(lib):
    """The trailer of an h2 image: max |w| 2^s in [2^12, 2^13) inside the clamp, s = -64 / 64
    at it, 0 for an all-zero layer."""
    in_dim, out_dim = 40, 48
    for kind, expect in (('zero', 0), ('tiny', 64), ('huge', -64), ('normal', None)):
        W, b = weights(in_dim, out_dim, kind, seed=3)
        raw = pack(lib, W, b, in_dim, out_dim, FIN | H2)
        down, up = np.frombuffer(raw[-16:-8], np.float32)
        s, zero = np.frombuffer(raw[-8:], np.int32)
        assert zero == 0 and down == np.float32(2.0) ** np.float32(-int(s))
        assert up == np.float32(2.0) ** np.float32(int(s))
        if expect is None:
            assert 2.0 ** 12 <= float(np.abs(W).max()) * 2.0 ** int(s) < 2.0 ** 13
        else:
            assert s == expect
