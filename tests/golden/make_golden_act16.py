"""Records what the one-launch block-16 activation kernel (lqer_amd/csrc/act16_fused.hip) writes for the cases of tests/_act16_cases.py:
the bf16 activation image and xAq as bit patterns, per input dtype (and rank, for xAq), with the fp16 tokens they were computed from
and a checksum of each A^T image.  Run once on a GPU box, on the commit whose outputs are to be pinned (the library that is loaded can
be chosen with LQER_AMD_LIB):  python tests/golden/make_golden_act16.py
Only data is written: results of this project's own library."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import _act16_cases as A  # noqa: E402


def main():
    import lqer_amd

    for M, K in A.SHAPES:
        x16 = A.make_x16(M, K)
        g = {"x": x16}
        for name, dtype in A.DTYPES.items():
            xd = A.x_for(x16, name).to(A.DEV)
            for r in A.RANKS:
                side = A.ActSide(A.make_module(lqer_amd, K, r, dtype), xd)
                side.launch()
                img, xa = side.read()
                if f"img_{name}" in g:
                    assert np.array_equal(g[f"img_{name}"], img)  # (the image does not depend on the rank)
                g[f"img_{name}"] = img
                g[f"xaq_{name}_r{r}"] = xa
                g[f"crc_a_{name}_r{r}"] = np.array([A.crc(side.p["a_t_b16"])], dtype=np.int64)
        np.savez_compressed(A.golden_path(M, K), **g)
        print(f"M={M} K={K}: {len(g)} arrays, {os.path.getsize(A.golden_path(M, K))} bytes")


if __name__ == "__main__":
    main()
