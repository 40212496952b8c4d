"""WHERE lqer_kv_pool_copy reads and writes (k_kv_pool_copy in csrc/kv_cache.hip), between guard zones (tests/_guard.py, as
tests/test_gpu_footprint.py): the destination pool and the image are payloads of EXACTLY lqer_kv_pool_bytes(_fmt) bytes at 16-byte
alignment - the first byte behind them is guard -, the source pool and the four id arrays are guarded read-only inputs.  The pools
hold pseudo-random bytes, not sequences: the copy knows no table and no length, and among random bytes an item that went to the wrong
place, or a piece of one that did not go, shows.  After a copy out of a pool into an image and one out of the image into another pool
- each naming the LAST page and the LAST slot of both its pools, and the first - the guards and the inputs are bit-unchanged and the
destination is, byte for byte, what it was with the named items replaced, by the header's layout restated here."""
import ctypes as C

import pytest
import torch

import _guard
import test_gpu_kv_swap as S

pytestmark = pytest.mark.gpu

DEV, HK, D = S.DEV, S.HK, 128  # 272 16-byte pieces per item with byte codes: the copy loop's second round
CASES = [(torch.bfloat16, None), (torch.bfloat16, (4, 4)), (torch.bfloat16, (8, 4)), (torch.float32, None)]
IDS = ["bf16-bytes", "bf16-K4V4", "bf16-K8V4", "f32-bytes"]


def layout(pages, slots, esz, bits):
    """[(offset, bytes of one (page or slot, kv head))] of the five sections, each rounded up to 256 bytes, and the total."""
    up = lambda x: (x + 255) // 256 * 256
    kb, vb = bits or (8, 8)
    out, at = [], 0
    for per, n in ((16 * D * kb // 8, pages), (D, pages), (16 * D * vb // 8, pages), (D, pages), (16 * D * esz, slots)):
        out.append((at, per))
        at += up(n * HK * per)
    return out, at


def expected(dst, dst_geom, src, src_geom, esz, bits, page_pairs, slot_pairs):
    """dst's bytes with, in every section, the named items of all kv heads replaced by src's."""
    want = dst.clone()
    (s_secs, _), (d_secs, _) = layout(*src_geom, esz, bits), layout(*dst_geom, esz, bits)
    for i, ((s_at, per), (d_at, _)) in enumerate(zip(s_secs, d_secs)):
        for a, b in (slot_pairs if i == 4 else page_pairs):
            want[d_at + b * HK * per:d_at + (b + 1) * HK * per] = src[s_at + a * HK * per:s_at + (a + 1) * HK * per]
    return want


def guarded_ids(ids, name):
    return _guard.guarded(4 * len(ids), align=16, fill=11, name=name).load(torch.tensor(ids, dtype=torch.int32, device=DEV))


def copy(src, src_geom, dst, dst_geom, dtype, fmts, page_pairs, slot_pairs):
    from lqer_amd import _lib, ops

    ids = [guarded_ids([p[i] for p in pairs], name) for pairs, i, name in
           ((page_pairs, 0, "src_page_ids"), (page_pairs, 1, "dst_page_ids"), (slot_pairs, 0, "src_slot_ids"), (slot_pairs, 1, "dst_slot_ids"))]
    before = dst.payload.clone()
    src.snapshot = src.arena.clone()  # (the image was written by the copy before: read-only from here)
    _lib.check(_lib.lib().lqer_kv_pool_copy(src.ptr, src.nbytes, *src_geom, dst.ptr, dst.nbytes, *dst_geom, ops._DT[dtype], HK, D, ids[0].ptr, ids[1].ptr,
                                            len(page_pairs), ids[2].ptr, ids[3].ptr, len(slot_pairs), *([C.byref(f) for f in fmts] or [None, None]),
                                            ops._stream(torch.device(DEV))), "lqer_kv_pool_copy")
    torch.cuda.synchronize()
    dst.check(), src.unchanged()
    for g in ids:
        g.unchanged()
    return before


@pytest.mark.parametrize("dtype, bits", CASES, ids=IDS)
def test_copy_stays_inside_its_pools(dtype, bits):
    from lqer_amd.kvcache import pool_bytes

    esz = torch.empty((), dtype=dtype).element_size()
    fmts = S.make(dtype, D, bits, pages=1, slots=1, room=1)._code_fmts()  # the K and V formats that name nibble storage, or none
    assert bool(fmts) == (bits is not None)
    geoms = {"pool": (24, 10), "image": (4, 3), "other": (6, 4)}
    g = {}
    for fill, (name, geom) in enumerate(geoms.items()):
        n = pool_bytes(dtype, *geom, HK, D, *fmts)
        assert n == layout(*geom, esz, bits)[1]
        g[name] = _guard.guarded(n, align=16, fill=3 + fill, name=name)
    # out of the pool into the image: the last and the first page and slot of both, one in between
    pages, slots = [(23, 3), (0, 0), (7, 1), (12, 2)], [(9, 2), (0, 0), (4, 1)]
    src = g["pool"].payload.clone()
    before = copy(g["pool"], geoms["pool"], g["image"], geoms["image"], dtype, fmts, pages, slots)
    want = expected(before, geoms["image"], src, geoms["pool"], esz, bits, pages, slots)
    assert torch.equal(g["image"].payload, want) and not torch.equal(want, before)
    # out of the image into another pool
    pages, slots = [(3, 5), (0, 0), (2, 2)], [(2, 3), (1, 0)]
    src = g["image"].payload.clone()
    before = copy(g["image"], geoms["image"], g["other"], geoms["other"], dtype, fmts, pages, slots)
    want = expected(before, geoms["other"], src, geoms["image"], esz, bits, pages, slots)
    assert torch.equal(g["other"].payload, want) and not torch.equal(want, before)
    # pages alone and slots alone: a count of 0 on the other side
    for pp, sp in (([(1, 4)], []), ([], [(0, 1)])):
        src = g["image"].payload.clone()
        before = copy(g["image"], geoms["image"], g["other"], geoms["other"], dtype, fmts, pp, sp)
        assert torch.equal(g["other"].payload, expected(before, geoms["other"], src, geoms["image"], esz, bits, pp, sp))
