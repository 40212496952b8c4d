"""Cases of the one-launch block-16 activation kernel (lqer_amd/csrc/act16_fused.hip) whose outputs are pinned bit for bit by
tests/golden/act16_fused_*.npz: shared by tests/golden/make_golden_act16.py, which recorded them, and tests/test_gpu_act16_golden.py.
The inputs are built from integer arithmetic and numpy's PCG64 stream and travel with the golden data (x) or are rebuilt and
checksummed (A), so a test run never depends on a random generator giving the same numbers on another machine."""
import ctypes as C
import os
import zlib

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
DEV = "cuda:0"
N = 256
RANKS = (16, 32, 64)
DTYPES = {"f16": torch.float16, "bf16": torch.bfloat16}
SHAPES = [
    # M, K
    (8, 512),     # one workgroup, one slab: seven of the eight waves idle
    (13, 640),    # ragged M; the second slab holds 128 of its 512 k: quarters past K
    (24, 4096),   # BASELINE configs[1]'s K: one slab per wave
    (16, 4608),   # wave 0 carries a second slab: requests across the loop's back edge
]


def golden_path(M, K):
    return os.path.join(GOLDEN, f"act16_fused_m{M}_k{K}.npz")


def make_x16(M, K):
    """fp16 tokens: N(0, 1), an outlier channel x30, an all-zero row, all-zero blocks, a block of fp16 subnormals, a block at fp16's top."""
    x = np.random.Generator(np.random.PCG64(1000 * M + K)).standard_normal((M, K)).astype(np.float32)
    x[:, 7] *= 30.0
    x[5 % M] = 0.0
    x[1, 32:64] = 0.0
    x[0, 16:32] = np.arange(1, 17, dtype=np.float32) * 2.0 ** -24 * np.where(np.arange(16) % 2, -1.0, 1.0)
    x[2, K - 16:] = 60000.0 - 1000.0 * np.arange(16, dtype=np.float32)
    return x.astype(np.float16)


def x_for(x16, name):
    """The kernel's input of dtype `name` from the recorded fp16 tokens.  bf16 also gets a block at an exponent that fp16 cannot hold
    (2^-123: 2^(mbits - e) is no normal float there, the quantizer's element routine runs instead of the fast one)."""
    t = torch.from_numpy(x16.astype(np.float32)).to(DTYPES[name])
    if name == "bf16":
        bits = np.array([0x0200 + 9 * i + (0x8000 if i % 3 == 0 else 0) for i in range(16)], dtype=np.uint16).view(np.int16)
        t[3, 48:64] = torch.from_numpy(bits).view(torch.bfloat16)
    return t


def make_a(K, r):
    """A [K, r] on the 8-bit MXINT grid (blocks of 16 along K): integer mantissas times a power of two per block - one bf16 limb."""
    k = np.arange(K, dtype=np.int64)[:, None]
    j = np.arange(r, dtype=np.int64)[None, :]
    m = (k * 37 + j * 101 + (k // 16) * 13 + (k * j) % 89) % 255 - 127
    e = -14 + (k // 16 + j) % 3
    return torch.from_numpy((m * np.exp2(e.astype(np.float64))).astype(np.float32))


def make_module(lq, K, r, dtype):
    from bench import MXINT_Q

    g = torch.Generator().manual_seed(K + r)  # (W and B do not reach the activation side's outputs)
    mod = lq.LinearFlexibleLqer(K, N, bias=False, q_config=MXINT_Q, l_config={"rank": r})
    mod.load_state_dict({"weight": 0.02 * torch.randn(N, K, generator=g), "A": make_a(K, r), "B": 0.01 * torch.randn(r, N, generator=g)})
    mod = mod.to(DEV).to(dtype)
    mod(torch.zeros(128, K, dtype=dtype, device=DEV))  # builds the images
    assert "a_t_b16" in mod._packed and not mod._x_i8
    return mod


def crc(t):
    return zlib.crc32(t.detach().cpu().contiguous().view(torch.uint8).numpy().tobytes())


class ActSide:
    """lqer_quantize_act_xa through the C ABI on the module's a_limbs = -2 image with the one-launch kernel forced (at these token counts
    the default is the two-launch route); the workspace is pre-filled, so what the kernel leaves untouched shows."""

    def __init__(self, mod, xd):
        from lqer_amd import _lib, ops

        self.L, self.xd, self.p = _lib.lib(), xd, mod._packed
        self.M, self.K = xd.shape
        self.desc = mod._desc()
        self.desc.tuning = _lib.TUNE_ACT16_FUSED
        L = self.L
        self.Kp, self.Mp, self.rp = L.lqer_padded_k(self.K), L.lqer_padded_m(self.M), L.lqer_padded_r(mod.rank)
        self.ws = torch.full((ops.linear_sizes(self.desc, self.M).workspace,), 0x5A, dtype=torch.uint8, device=DEV)
        self.xq = self.ws.data_ptr()
        self.xaq = self.xq + ((self.Mp * self.Kp * 2 + 255) // 256) * 256
        self.scr = self.xaq + ((self.Mp * self.rp * 2 + 255) // 256) * 256
        self.nscr = L.lqer_lowrank_xa_scratch_bytes(C.byref(self.desc), self.M)
        self.dt = ops.dtype_code(xd)

    def launch(self):
        from lqer_amd import _lib

        _lib.check(self.L.lqer_quantize_act_xa(C.byref(self.desc), self.xd.data_ptr(), self.dt, self.M, self.K, self.p["a_t_b16"].data_ptr(), -2,
                                               self.xq, self.xaq, self.scr, self.nscr, torch.cuda.current_stream().cuda_stream), "quantize_act_xa")

    def read(self):
        """(image rows of every workgroup that ran [8 ceil(M / 8), Kp], xAq [M, rp]) as int16 bit patterns on the CPU."""
        torch.cuda.synchronize()
        rows = 8 * ((self.M + 7) // 8)
        img = self.ws[: self.Mp * self.Kp * 2].view(torch.int16).view(self.Mp, self.Kp)[:rows].cpu().numpy().copy()
        off = self.xaq - self.xq
        xa = self.ws[off: off + self.Mp * self.rp * 2].view(torch.int16).view(self.Mp, self.rp)[: self.M].cpu().numpy().copy()
        return img, xa
