"""Records what the library's host logic answers over the descriptor grid of tests/test_sizes_cpu.py - lqer_gemm_route,
lqer_gemm_tile_rows (error codes included: the refusals are part of the contract), lqer_linear_gemm_scratch_bytes and
lqer_decode_partials - into tests/golden/routes.json, which tests/test_routes_cpu.py holds every later library to.  No GPU needed.

    LQER_AMD_LIB=<liblqer_hip.so of the commit to record> python tests/golden/make_golden_routes.py

The answers are piecewise constant in the token count: a series is run-length encoded along TOKENS, equal series are stored once
(`series`), and so are equal lists of a descriptor's series (`rows`); `desc` has one index into `rows` per descriptor, in grid order."""
import ctypes as C
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import test_sizes_cpu as G  # noqa: E402  (the grid: format sets, KS, NS, RANKS, TOKENS)

PATH = os.path.join(HERE, "routes.json")
DTYPES = ("F32", "F16", "BF16")
TUNINGS = ("0", "TILE_ROWS_128", "TILE_ROWS_64", "I8_ROWS_128", "I8_ROWS_256")


def _rle(values):
    out = []
    for v in values:
        if out and out[-1][1:] == list(v):
            out[-1][0] += 1
        else:
            out.append([1, *v])
    return out


def unrle(series):
    return [tuple(run[1:]) for run in series for _ in range(run[0])]


def columns():
    """Names of the series of one descriptor, in the order walk() yields them."""
    cols = [f"route/tile_rows dtype={dt} tuning={tu}" for tu in TUNINGS for dt in DTYPES]
    return cols + [f"gemm_scratch_bytes/decode_partials tuning={tu}" for tu in TUNINGS]


def walk(lib):
    """(descriptor label, its run-length encoded series in columns() order) over the grid."""
    from lqer_amd import _lib

    for name, d in G._grid():
        label = f"{name} K={d.in_features} N={d.out_features} rank={d.rank}"
        p = C.byref(d)
        series, sizes = [], []
        for tu in TUNINGS:
            d.tuning = 0 if tu == "0" else getattr(_lib, "TUNE_" + tu)
            for dt in DTYPES:
                code = getattr(_lib, dt)
                series.append(_rle((lib.lqer_gemm_route(p, m, code), lib.lqer_gemm_tile_rows(p, m, code)) for m in G.TOKENS))
            sizes.append(_rle((lib.lqer_linear_gemm_scratch_bytes(p, m), lib.lqer_decode_partials(p, m)) for m in G.TOKENS))
        yield label, series + sizes


def record(lib):
    series, rows, desc = {}, {}, []
    for _, cols in walk(lib):
        ids = tuple(series.setdefault(json.dumps(s), len(series)) for s in cols)
        desc.append(rows.setdefault(ids, len(rows)))
    return {"tokens": list(G.TOKENS), "columns": columns(), "series": [json.loads(s) for s in series], "rows": [list(r) for r in rows],
            "desc": desc}


if __name__ == "__main__":
    from lqer_amd import _lib

    with open(PATH, "w") as f:
        json.dump(record(_lib.lib()), f, separators=(",", ":"))
        f.write("\n")
    print(PATH, os.path.getsize(PATH), "bytes; library", _lib.LIB_PATH)
