"""Generate tests/golden/quantizers_expfield.npz: the REFERENCE's block_fp quantizer on narrow exponent fields (both clamps
active) and every width, imported the same way as make_golden.py.  Run once, in the build container:
    python tests/golden/make_golden_expfield.py

Only data is written: inputs (the ladder of tests/_formats.py, fp32), the reference's outputs and one meta row per vector,
    meta = [width, exponent_width, has_bias, exponent_bias, skip_first_dim, block...]
The archive is written with fixed zip timestamps, so a second run gives the same bytes.
"""
import io
import os
import sys
import zipfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))                   # tests/: _formats
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))  # the repository root: oracle (imported by _formats)

from make_golden import import_reference  # noqa: E402

import _formats as F  # noqa: E402


def main():
    _, get_q = import_reference()
    bfp = get_q("block_fp")
    g = {}

    def add(name, x, fid, width, block, skip):
        ew, eb = F.FORMATS[fid]
        y = bfp(x.clone(), width=width, exponent_width=ew, exponent_bias=eb, block_size=list(block), skip_first_dim=skip)
        g[f"{name}/x"] = x.numpy()
        g[f"{name}/y"] = y.numpy()
        g[f"{name}/meta"] = np.array([width, ew, int(eb is not None), 0 if eb is None else eb, int(skip)] + list(block), dtype=np.int64)

    pairs = sorted(set(F.ACT_PAIRS + F.W4_PAIRS + F.W8_PAIRS))
    for n, (fid, width) in enumerate(pairs):
        add(f"b16/{F.pair_id((fid, width))}", F.ladder(fid, torch.float32, 8, 64, 16, seed=n), fid, width, [1, 16], True)
    for n, (fid, width) in enumerate((("e4", 4), ("e3bm2", 8), ("e5b20", 4))):
        add(f"b128/{F.pair_id((fid, width))}", F.ladder(fid, torch.float32, 6, 256, 128, seed=100 + n), fid, width, [1, 128], False)
        add(f"row/{F.pair_id((fid, width))}", F.ladder(fid, torch.float32, 12, 80, -1, seed=110 + n), fid, width, [1, -1], True)
        # 2-D tiles [4, 16] with skip_first_dim = false: four consecutive rows share the ladder's scale of the first
        t = F.ladder(fid, torch.float32, 3, 48, 16, seed=120 + n)
        jit = (0.5 + 0.5 * torch.rand(3, 4, 48, generator=torch.Generator().manual_seed(130 + n)))
        add(f"tile4x16/{F.pair_id((fid, width))}", (t[:, None, :] * jit).reshape(12, 48)[:10].contiguous(), fid, width, [4, 16], False)
    x3 = F.ladder("e4", torch.float32, 10, 48, 16, seed=140).reshape(2, 5, 48).contiguous()
    add("act3d/e4-w8", x3, "e4", 8, [1, 16], True)
    t = F.ladder("e3b6", torch.float32, 6, 48, 16, seed=141)  # [2, 16] tiles of a 3-D activation: row pairs share a ladder row's scale
    jit = 0.5 + 0.5 * torch.rand(6, 2, 48, generator=torch.Generator().manual_seed(142))
    add("act3d_tile/e3b6-w4", (t[:, None, :] * jit).reshape(2, 6, 48).contiguous(), "e3b6", 4, [2, 16], True)

    path = os.path.join(HERE, "quantizers_expfield.npz")
    with zipfile.ZipFile(path, "w", compression=zipfile.ZIP_DEFLATED) as zf:
        for key in sorted(g):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.ascontiguousarray(g[key]), allow_pickle=False)
            info = zipfile.ZipInfo(key + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            zf.writestr(info, buf.getvalue())
    print("quantizers_expfield.npz:", len(g), "arrays,", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
