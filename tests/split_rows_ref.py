"""The split-row format in numpy, written from its description (include/radar_gnn.h,
rg_mlp_chain_x3_split) and not from csrc/pack_layout.h:

a row of 64 float32 values v keeps its 256 bytes; bytes [32 j, 32 j + 16) hold the fp16 heads
a0 = fp16(v) of features 8 j .. 8 j + 7 in order, bytes [32 j + 16, 32 j + 32) their fp16
residues a1 = fp16(v - a0) (the subtraction exact in float32).
"""
import numpy as np

W = 64


def encode_rows(e: np.ndarray) -> np.ndarray:
    """float32 [R, 64] -> float32 [R, 64] whose bytes are the rows' split form."""
    e = np.ascontiguousarray(e, np.float32)
    assert e.ndim == 2 and e.shape[1] == W
    head = e.astype(np.float16)
    res = (e - head.astype(np.float32)).astype(np.float16)
    out = np.empty((e.shape[0], 8, 2, 8), np.float16)      # [row][group][head | residue][8]
    out[:, :, 0, :] = head.reshape(-1, 8, 8)
    out[:, :, 1, :] = res.reshape(-1, 8, 8)
    return out.reshape(e.shape[0], 2 * W).view(np.float32)


def decode_rows(s: np.ndarray):
    """Split rows (float32-typed [R, 64]) -> (heads, residues), float16 [R, 64] each."""
    s = np.ascontiguousarray(s, np.float32)
    assert s.ndim == 2 and s.shape[1] == W
    h = s.view(np.float16).reshape(s.shape[0], 8, 2, 8)
    return (np.ascontiguousarray(h[:, :, 0, :]).reshape(-1, W),
            np.ascontiguousarray(h[:, :, 1, :]).reshape(-1, W))
