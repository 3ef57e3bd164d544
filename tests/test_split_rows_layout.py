"""The split-row format without a GPU: the numpy reference (tests/split_rows_ref.py) round-trips,
csrc/pack_layout.h's offset functions are a bijection onto the row's 256 bytes and agree with
the reference (tests/split_rows_layout_main.cpp, compiled with the host compiler), and the two
new entry points refuse what they must before any launch."""
import ctypes
import os
import shutil
import subprocess

import numpy as np

from split_rows_ref import decode_rows, encode_rows

HERE = os.path.dirname(os.path.abspath(__file__))


def _values():
    g = np.random.default_rng(5)
    v = (g.standard_normal((37, 64)) * np.exp(g.uniform(-12, 9, (37, 64)))).astype(np.float32)
    v[0, :8] = [0.0, -0.0, 0.125, -0.125, 2.0 ** -14, 2.0 ** -24, 65504.0, 1.0 + 2.0 ** -11]
    return v


def test_reference_round_trip():
    """encode -> decode gives fp16(v) and fp16(v - fp16(v)) in feature order; head + residue
    restores v to 2^-21 relative wherever the residue is a normal fp16, and to the fp16
    subnormal step 2^-24 (half of it after rounding) elsewhere; the encoded row is 256 bytes."""
    v = _values()
    s = encode_rows(v)
    assert s.dtype == np.float32 and s.shape == v.shape
    head, res = decode_rows(s)
    assert np.array_equal(head.view(np.uint16), v.astype(np.float16).view(np.uint16))
    r32 = v - head.astype(np.float32)
    assert np.array_equal(res.view(np.uint16), r32.astype(np.float16).view(np.uint16))
    back = head.astype(np.float64) + res.astype(np.float64)
    err = np.abs(back - v.astype(np.float64))
    assert (err <= np.maximum(2.0 ** -21 * np.abs(v), 2.0 ** -25)).all()
    # the bytes: group j = heads of features 8j .. 8j + 7, then their residues
    raw = s.view(np.uint16)
    for j in range(8):
        assert np.array_equal(raw[:, 16 * j:16 * j + 8], head.view(np.uint16)[:, 8 * j:8 * j + 8])
        assert np.array_equal(raw[:, 16 * j + 8:16 * j + 16], res.view(np.uint16)[:, 8 * j:8 * j + 8])


def test_header_offsets_are_a_bijection_and_match_the_reference(tmp_path):
    """pack_layout.h's split_row_head / split_row_res, compiled into a stand-alone program:
    every byte of the row used exactly once (the program checks and exits non-zero otherwise),
    and the offsets it prints are where the numpy reference puts each feature's terms."""
    cxx = shutil.which('g++') or shutil.which('c++') or shutil.which('clang++')
    if cxx is None:
        from graph_neural_network_for_radar_perception_amd import build
        cxx = build.HIPCC
    exe = str(tmp_path / 'split_rows_layout')
    subprocess.run([cxx, '-std=c++17', '-O1', '-Wall', '-I', os.path.join(HERE, '..', 'include'),
                    os.path.join(HERE, 'split_rows_layout_main.cpp'), '-o', exe], check=True,
                   capture_output=True, text=True, timeout=120)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=30)
    assert r.returncode == 0, r.stderr
    rows = [tuple(map(int, ln.split())) for ln in r.stdout.strip().split('\n')]
    assert [f for f, _, _ in rows] == list(range(64))
    # a row whose feature f is the only non-zero value: where do its head and residue land?
    for f, hb, rb in rows:
        v = np.zeros((1, 64), np.float32)
        v[0, f] = np.float32(1.0 + 2.0 ** -12)    # head 1.0, residue 2^-12
        raw = encode_rows(v).view(np.uint8)[0]
        nz = sorted(np.flatnonzero(raw).tolist())
        assert raw[hb + 1] == 0x3c and raw[hb] == 0          # fp16 1.0, little endian
        assert set(nz) <= {hb, hb + 1, rb, rb + 1} and (raw[rb] or raw[rb + 1])


_FAKE = ctypes.create_string_buffer(256 + 16)   # host memory: a launch would fault


def _fake16():
    a = ctypes.addressof(_FAKE)
    return (a + 15) // 16 * 16


def test_conv_split_refusals_before_any_launch():
    """rg_conv_layer_x3_split_for: b3 images, lde != 64 and a misaligned e are RG_ERR_ARG (the
    pointers are host memory: a launch would not come back)."""
    from graph_neural_network_for_radar_perception_amd import _native as nat
    from test_conv_terms_emulation import _layers
    lib = nat.lib()
    ws = lib.rg_conv_layer_x3_workspace_size(64)
    fake = _fake16()

    def call(arr, e, lde):
        return lib.rg_conv_layer_x3_split_for(
            arr, ctypes.byref(arr[3]), ctypes.byref(arr[4]), nat.REDUCE['add'], fake, 64, e, lde,
            fake, fake, fake, fake, 64, fake + 64, 64, fake + 128, None, fake, ws, None)
    h2, _ = _layers(nat, (1, 1, 1, 1, 1))
    b3, _ = _layers(nat, (0, 0, 0, 0, 0))
    assert call(b3, fake, 64) == 1 and b'RG_LAYER_H2' in lib.rg_last_error()
    assert call(h2, fake, 128) == 1 and b'lde' in lib.rg_last_error()
    assert call(h2, fake + 4, 64) == 1 and b'aligned' in lib.rg_last_error()
    assert call(h2, None, 64) == 1
    # uncentred images would take the block-queue edge launch, which reads float32 rows
    for d in h2:
        d.flags &= ~nat.RG_LAYER_CENTERED
    assert call(h2, fake, 64) == nat.RG_ERR_UNSUPPORTED


def test_chain_split_refusals_before_any_launch():
    """rg_mlp_chain_x3_split: a b3 chain, rows not 64 wide, ld_out != 64 and a misaligned
    output are RG_ERR_ARG."""
    from graph_neural_network_for_radar_perception_amd import _native as nat
    lib = nat.lib()
    fake = _fake16()
    dims = ((7, 256), (256, 128), (128, 128), (128, 64))

    def chain(h2, last_out=64):
        arr = (nat.rg_layer * 4)()
        for li, (d, (i, o)) in enumerate(zip(arr, dims)):
            d.w_packed, d.in_dim, d.out_dim = fake, i, (last_out if li == 3 else o)
            d.flags = nat.RG_LAYER_CENTERED | (nat.RG_LAYER_H2 if h2 else 0)
            d.act = nat.ACT['leakyrelu']
            if li:
                d.norm_mu = d.norm_std = fake
        return arr

    def call(arr, out, ld):
        return lib.rg_mlp_chain_x3_split(arr, 4, 100, None, nat.IN_DENSE, fake, 7, 7, None, None,
                                         out, ld, None)
    assert call(chain(False), fake, 64) == 1 and b'RG_LAYER_H2' in lib.rg_last_error()
    assert call(chain(True, 32), fake, 64) == 1
    assert call(chain(True), fake, 128) == 1 and b'stride' in lib.rg_last_error()
    assert call(chain(True), fake + 8, 64) == 1 and b'aligned' in lib.rg_last_error()
    assert call(chain(True), None, 64) == 1
