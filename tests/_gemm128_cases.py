"""Cases of the fused GEMM's 128-row tile kernel (lqer_amd/csrc/gemm_w4a8.hip, k_lqer_gemm<..., MT = 4>) whose outputs are pinned bit
for bit by tests/golden/gemm128_*.npz: shared by tests/golden/make_golden_gemm128.py, which recorded them on the parent of the commit
that changed the main loop's weight expand, and tests/test_gpu_gemm128_golden.py.  Every operand is MXINT data (every partial sum exact
in fp32), so no summation order and no expand may change a bit.  Inputs come from numpy's PCG64 stream and are checksummed in the
fixture, so a test run never depends on a random generator giving the same numbers on another machine.

The shapes are the smallest at which the tile's main loop, B_out re-quantization and store can go wrong:
  M 128 one tile | 130 a second tile with two live rows (clamped rows, store predicate)
  K 320 five k-steps (B_out in the prologue, ring tail no multiple of 4) | 1024 sixteen (the fewest that re-quantize B_out under the
    main loop: every step carries a piece) | 1088 seventeen (the first plain step behind the pieces)
  N 256 full column tiles | 272 the last column tile is 16 columns | 264 ... half of that, an odd multiple of 8 as row stride
  rank 32 | 8 (padded to 16) | 0 (no side path); bias or none; fp16 / bf16 / fp32 tensors (fp32: the accumulator's own bits)
  B_out in blocks of 16 (under the main loop, or pinned in front of it) | pass-through
  `huge`: a weight row with block maxima beyond 2^121 - exponent bytes the table-free expand cannot carry, the image takes the table form."""
import os
import zlib

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
DEV = "cuda:0"
DTYPES = {"f16": torch.float16, "bf16": torch.bfloat16, "f32": torch.float32}

CASES = [
    # M, K, N, rank, bias, B_out, dtype, extra
    (128, 320, 256, 32, False, "mx", "f16", ""),
    (130, 320, 256, 32, True, "mx", "bf16", ""),
    (130, 320, 264, 8, True, "mx", "f16", ""),
    (128, 320, 272, 32, True, "pass", "bf16", ""),
    (128, 1024, 256, 32, False, "mx", "f16", ""),
    (130, 1024, 272, 32, True, "mx", "bf16", ""),
    (128, 1024, 272, 32, False, "mx", "f16", ""),
    (130, 1024, 256, 32, False, "mx", "f16", "prologue"),   # blocks of 16 re-quantized in front of the main loop at sixteen k-steps
    (130, 1024, 264, 8, False, "pass", "f16", ""),
    (130, 1024, 272, 0, True, "mx", "f16", ""),             # no side path
    (130, 1088, 264, 32, False, "mx", "f16", ""),
    (130, 1088, 264, 32, True, "mx", "bf16", ""),
    (128, 1088, 256, 8, True, "mx", "bf16", ""),
    (130, 1088, 256, 32, False, "pass", "f16", ""),
    (128, 1088, 264, 8, True, "pass", "bf16", ""),
    (130, 1088, 272, 0, False, "mx", "bf16", ""),
    (130, 1024, 264, 32, True, "mx", "f32", ""),            # fp32 tensors: the accumulator's own bits
    (128, 320, 256, 8, False, "pass", "f32", ""),
    (130, 1024, 264, 0, True, "mx", "bf16", "huge"),        # (no side path: the table instantiations stage it, another summation order)
    (130, 1088, 272, 0, False, "mx", "f32", "huge"),
]
HUGE_ROW = 3


def case_id(c):
    M, K, N, r, bias, bout, dt, extra = c
    return f"m{M}_k{K}_n{N}_r{r}_{'b' if bias else 'nb'}_{bout}_{dt}" + (f"_{extra}" if extra else "")


def golden_path(c):
    return os.path.join(GOLDEN, f"gemm128_{case_id(c)}.npz")


def seed_of(c):
    return zlib.crc32(case_id(c).encode())


def make_inputs(c):
    """x [M, K] ~ N(0, 1) with an outlier channel, an all-zero row and an all-zero block; W ~ 0.02 N(0, 1) times a power of two per
    (row, block of 16) over seven binades, one block all zeros; A, B ~ 0.01 N(0, 1) snapped to the 8-bit MXINT grid; bias ~ 0.01 N(0, 1).
    `huge`: weight row HUGE_ROW holds mantissas times 2^119, one of 5..7 per block (block exponent 122: exponent byte 246) among -1..1, so
    that its sums stay far inside fp32 and bf16; its first block, which meets the outlier channel, is zero."""
    from bench import _snap_mxint8_dim0

    M, K, N, r, bias, bout, dt, extra = c
    g = np.random.Generator(np.random.PCG64(seed_of(c)))
    x = g.standard_normal((M, K)).astype(np.float32)
    x[:, 7] *= 30.0
    x[5] = 0.0
    x[1, 32:48] = 0.0
    W = (0.02 * g.standard_normal((N, K))).astype(np.float32)
    W *= np.repeat(np.exp2(g.integers(-3, 4, (N, (K + 15) // 16))), 16, axis=1)[:, :K].astype(np.float32)
    W[2, 16:32] = 0.0
    b = (0.01 * g.standard_normal(N)).astype(np.float32) if bias else None
    A = B = None
    if r > 0:
        A = _snap_mxint8_dim0(torch.from_numpy((0.01 * g.standard_normal((K, r))).astype(np.float32)))
        Bn = (0.01 * g.standard_normal((r, N))).astype(np.float32)
        B = _snap_mxint8_dim0(torch.from_numpy(Bn))
    if extra == "huge":
        m = g.integers(-1, 2, K).astype(np.float32)
        m[::16] = g.integers(5, 8, (K + 15) // 16) * np.where(g.integers(0, 2, (K + 15) // 16), -1.0, 1.0)
        m[:16] = 0.0
        W[HUGE_ROW] = m * np.float32(2.0 ** 119)
    return torch.from_numpy(x), torch.from_numpy(W), A, B, None if b is None else torch.from_numpy(b)


def crc(t):
    return zlib.crc32(t.detach().cpu().contiguous().view(torch.uint8).numpy().tobytes())


def input_crcs(inputs):
    return np.array([0 if t is None else crc(t) for t in inputs], dtype=np.int64)


def plant_negative_zeros(mod):
    """The packer writes +0 only; the kernel must also take the nibble 8 (-0).  Every third zero nibble of the packed image becomes one."""
    w = mod._packed["w"].reshape(-1).view(torch.uint8).view(-1, 576)
    codes = w[:, :512]
    idx = torch.arange(codes.numel(), device=codes.device).view(codes.shape) % 3 == 0
    lo = ((codes & 0x0F) == 0) & idx
    hi = ((codes & 0xF0) == 0) & idx
    codes |= lo.to(torch.uint8) * 0x08 + hi.to(torch.uint8) * 0x80
    return int(lo.sum() + hi.sum())


def run_case(lq, c, inputs):
    """y [M, N] of the case on 128-row tiles, as the bit patterns of its dtype (int16 / int32), and facts about the packed weight image:
    (planted -0 nibbles, nibble codes present, distinct exponent bytes)."""
    from bench import MXINT_Q
    from lqer_amd import _lib

    M, K, N, r, bias, bout, dt, extra = c
    x, W, A, B, b = inputs
    dtype = DTYPES[dt]
    qc = MXINT_Q if bout == "mx" else dict(MXINT_Q, B_out_quantizer={"name": "passthrough"})
    if r > 0:
        mod = lq.LinearFlexibleLqer(K, N, bias=bias, q_config=qc, l_config={"rank": r})
        sd = {"weight": W, "A": A, "B": B}
    else:
        mod = lq.LinearFlexible(K, N, bias=bias, q_config=dict(qc, name="flexible"))
        sd = {"weight": W}
    if bias:
        sd["bias"] = b
    mod.load_state_dict(sd)
    mod = mod.to(DEV).to(dtype)
    mod.tuning = _lib.TUNE_TILE_ROWS_128 | (_lib.TUNE_BOUT_IN_PROLOGUE if extra == "prologue" else 0)
    xd = x.to(dtype).to(DEV)
    mod(xd)  # builds the images
    planted = plant_negative_zeros(mod)
    img = mod._packed["w"].reshape(-1).view(torch.uint8).view(-1, 576)
    codes = torch.unique(torch.cat([img[:, :512] & 0x0F, img[:, :512] >> 4])).cpu().numpy()
    ebytes = torch.unique(img[:, 512:]).cpu().numpy()
    y = mod(xd)
    torch.cuda.synchronize()
    bits = y.contiguous().view(torch.int32 if dtype == torch.float32 else torch.int16).cpu().numpy().copy()
    return bits, (planted, codes, ebytes)
