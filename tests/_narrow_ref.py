"""A second reading of the two weight-image layouts of include/lqer_hip.h, in numpy, for tests/test_weight_narrow_cpu.py and
tests/test_gpu_weight_narrow.py: where the code of (row, k) and the exponent byte of (row, 16-k segment) lie in a standard 576-byte
panel and in the compact panel of a 2- / 3-bit weight.  Written from the header's text, not from csrc/w_narrow.h, one element at a time."""
from __future__ import annotations

import numpy as np

STD_PANEL = 576


def exps_per_row(width: int, block: int, K: int) -> int:
    if block in (16, 32):
        return 64 // block
    if block <= 0 or block >= K or block % 64 == 0:
        return 1
    return 4


def panel_bytes(width: int, E: int) -> int:
    return 128 * width + 16 * E


def padded(N: int, K: int):
    return (N + 255) // 256 * 256, (K + 63) // 64 * 64


def pad_byte(width: int) -> int:
    return 127 - (width - 1)


def std_code(panel: np.ndarray, row: int, k: int):
    """(sign, magnitude) of weight (row, k) of a standard panel."""
    c, j8 = k // 8, k % 8
    off = row * 32 + (c & 1) * 16 + (c >> 1) * 4
    word = int(panel[off]) | int(panel[off + 1]) << 8 | int(panel[off + 2]) << 16 | int(panel[off + 3]) << 24
    p = 2 * j8 if j8 < 4 else 2 * (j8 - 4) + 1
    nib = (word >> (4 * p)) & 0xF
    return nib >> 3, nib & 7


def std_exp(panel: np.ndarray, row: int, seg: int) -> int:
    return int(panel[512 + row * 4 + seg])


def narrow_code(panel: np.ndarray, width: int, row: int, k: int):
    """(sign, magnitude) of weight (row, k) of a compact panel."""
    c, j8 = k // 8, k % 8
    q, half = c % 4, c // 4
    j, odd = j8 % 4, j8 // 4
    t = 2 * half + odd
    field = (int(panel[row * 16 + q * 4 + j]) >> (2 * t)) & 3
    if width == 2:
        return field >> 1, field & 1
    sbyte = int(panel[256 + row * 8 + (q >> 1) * 4 + j])
    return (sbyte >> (4 * (q & 1) + t)) & 1, field


def narrow_exp(panel: np.ndarray, width: int, E: int, row: int, seg: int) -> int:
    return int(panel[128 * width + row * E + seg * E // 4])


def random_std_image(N: int, K: int, width: int, block: int, seed: int) -> np.ndarray:
    """Random bytes that are a standard image of a width-`width` block_fp weight in blocks of `block`: magnitudes below 2^(width-1),
    random sign bits (zero magnitudes included), exponent bytes repeated per block - and, as the packer writes it, the byte of
    exponent 0 in every 16-k segment that starts at or past K."""
    rng = np.random.default_rng(seed)
    Np, Kp = padded(N, K)
    npk = Kp // 64
    img = np.zeros((Np // 16, npk, STD_PANEL), dtype=np.uint8)
    mag = rng.integers(0, 1 << (width - 1), size=(Np // 16, npk, 512), dtype=np.uint8)
    mag2 = rng.integers(0, 1 << (width - 1), size=(Np // 16, npk, 512), dtype=np.uint8)
    sg = rng.integers(0, 2, size=(2, Np // 16, npk, 512), dtype=np.uint8)
    img[:, :, :512] = mag | (sg[0] << 3) | (mag2 << 4) | (sg[1] << 7)
    L = Kp if (block <= 0 or block >= K) else block
    nblk = (Kp + L - 1) // L
    eb = rng.integers(1, 255, size=(Np, nblk), dtype=np.uint8)
    for seg in range(Kp // 16):
        col = eb[:, (seg * 16) // L] if seg * 16 < K else np.full(Np, pad_byte(width), dtype=np.uint8)
        img[:, seg // 4, 512 + (seg % 4): 576: 4] = col.reshape(Np // 16, 16)
    return img.reshape(-1)
