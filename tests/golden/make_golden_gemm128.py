"""Records what the fused GEMM's 128-row tile kernel (lqer_amd/csrc/gemm_w4a8.hip) computes for the cases of tests/_gemm128_cases.py: y as
bit patterns, with the case's seed and the checksums of the inputs it was computed from.  Run once on a GPU box, on the commit whose
outputs are to be pinned - the parent of a change to the kernel - from that commit's own tree (so that its library and Python package
are the ones loaded), with this tree's tests/ directory in front:  python tests/golden/make_golden_gemm128.py [output directory]
Only data is written: results of this project's own library."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
if os.environ.get("LQER_GOLDEN_TREE"):  # the tree whose library computes the outputs (default: this one)
    sys.path.insert(0, os.environ["LQER_GOLDEN_TREE"])
else:
    sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import _gemm128_cases as G  # noqa: E402


def main():
    import lqer_amd

    out = sys.argv[1] if len(sys.argv) > 1 else G.GOLDEN
    os.makedirs(out, exist_ok=True)
    print("library of", os.path.dirname(lqer_amd.__file__))
    for c in G.CASES:
        inputs = G.make_inputs(c)
        bits, (planted, codes, ebytes) = G.run_case(lqer_amd, c, inputs)
        path = os.path.join(out, os.path.basename(G.golden_path(c)))
        np.savez_compressed(path, y=bits, seed=np.array([G.seed_of(c)], dtype=np.int64), crc_inputs=G.input_crcs(inputs))
        print(f"{G.case_id(c)}: {os.path.getsize(path)} bytes, {planted} planted -0, {len(codes)} codes, exponent bytes {ebytes.min()}..{ebytes.max()} "
              f"({len(ebytes)} distinct), finite {bool(np.isfinite(bits.view(np.float32)).all()) if bits.dtype == np.int32 else '-'}", flush=True)


if __name__ == "__main__":
    main()
