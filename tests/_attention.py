"""What the attention test modules share: the CPU comparator of the fused quantized attention (see tests/test_gpu_attention_fused.py
for its construction and its own spread), mask tensors, seeded inputs.  CPU only."""
import json
import os

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
CFG = json.load(open(os.path.join(HERE, "golden", "matmul_config.json")))
DEV = "cuda:0"
BAR = 1e-3


def _rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


def _causal_mask(s, t, dtype, pad=None, batch=1):
    """eager_mask's tensor: 0 where key j is visible to query i (j <= i + t - s), the dtype's most negative finite value elsewhere;
    `pad` masks the first keys of the LAST batch element as well (a left-padded sequence: its early rows are fully masked)."""
    i, j = torch.arange(s)[:, None], torch.arange(t)[None, :]
    dead = (j > i + (t - s))[None, None].expand(batch, 1, s, t).clone()
    if pad:
        dead[-1, :, :, :pad] = True
    return torch.zeros(batch, 1, s, t, dtype=dtype).masked_fill_(dead, torch.finfo(dtype).min)


def comparator(q, k, v, scaling, mask=None, cfg0=None, cfg1=None, acc=torch.float32):
    """CPU tensors of dtype DT -> (O, S2, P) in DT.  cfg0 / cfg1: the two matmul configs (default: CFG for both).  acc=torch.float64
    evaluates the two products and the softmax in fp64 instead (the quantizers stay the oracle's, in fp32): the distance between the
    two evaluations is the comparator's own spread, the part of the bar that no kernel can be asked to undercut."""
    from oracle import lqer_oracle as O

    cfg0, cfg1 = cfg0 or CFG, cfg1 or CFG
    dt = q.dtype
    b, h, s, d = q.shape
    hk, t = k.shape[1], k.shape[2]
    rep = lambda x: x[:, :, None].expand(b, hk, h // hk, t, d).reshape(b * h, t, d).float()

    def product(x, y, cfg):
        if acc == torch.float32:
            return O.matmul_flexible(x, y, cfg)
        xq = O.get_quantizer(cfg.get("x_quantizer", cfg["default"]))(x)
        yq = O.get_quantizer(cfg.get("w_quantizer", cfg["default"]))(y)
        return torch.matmul(xq.to(acc), yq.to(acc))

    S = product(q.reshape(b * h, s, d).float(), rep(k).transpose(1, 2), cfg0).reshape(b, h, s, t).to(dt)
    S2 = (S.float() * torch.tensor(scaling, dtype=torch.float32)).to(dt)
    if mask is not None:
        S2 = (S2.float() + mask.float()).to(dt)
    P = torch.softmax(S2.to(acc), dim=-1).to(dt)
    out = product(P.reshape(b * h, s, t).float(), rep(v), cfg1).reshape(b, h, s, d).to(dt)
    return out, S2, P


def _randn(shape, dtype, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (scale * torch.randn(*shape, generator=g)).to(dtype)


def _pad(s, t):
    return max(0, t - s - 3)  # the last batch element is left-padded by this many keys: every row keeps a visible key


def _mask(mode, b, s, t, dtype):
    """none / causal / 'mask': the causal tensor whose last batch element is left-padded."""
    if mode == "none":
        return None
    return _causal_mask(s, t, dtype, pad=_pad(s, t) if mode == "mask" else None, batch=b)
