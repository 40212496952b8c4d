"""Guard zones around device buffers handed to the C ABI (tests/test_gpu_footprint.py): a helper, imported like _envelope.py.

`guarded(nbytes, ...)` owns ONE uint8 device tensor laid out as  pre | payload | post :
  - the payload pointer is aligned to `align` (256: what the caching allocator gives; 16: the pointer is 16 mod 256, i.e. aligned
    to 16 bytes and to nothing coarser - for buffers whose contract is 16 bytes) and the payload is EXACTLY `nbytes` long, so the
    first byte behind it is guard;
  - pre is 4 KiB, post 64 KiB - or 256 * row_pitch_bytes + 64 KiB for row-structured buffers: 256 rows is the tallest tile of the
    library, so a whole stray row tile lands in the guard and not outside the allocation;
  - the arena is filled with a seeded pseudo-random byte pattern (or with 0xFF: NaN in every float type) and a device clone is
    kept as the snapshot; `check()` asserts that pre and post are bit-equal to it and names the first and last changed byte as an
    offset from the payload end (row / column when a pitch is known); `gaps_unchanged()` does the same for the columns N..ld-1
    between the rows of a strided window, `unchanged()` for a read-only input as a whole.
The helper never allocates a payload smaller than asked for and never shrinks anything."""
from __future__ import annotations

import torch

PRE = 4096
POST = 65536
TILE_ROWS = 256  # the tallest tile of the library

_DT_BYTES = {torch.float32: 4, torch.float16: 2, torch.bfloat16: 2, torch.int8: 1, torch.uint8: 1, torch.int16: 2, torch.int32: 4}


class Guarded:
    def __init__(self, nbytes: int, *, row_pitch_bytes: int = 0, align: int = 256, fill=0, name: str = "buffer", device="cuda:0"):
        assert nbytes >= 0 and align in (16, 256) and row_pitch_bytes >= 0
        self.name, self.nbytes, self.pitch = name, int(nbytes), int(row_pitch_bytes)
        self.post = TILE_ROWS * self.pitch + POST
        raw = torch.empty(PRE + self.nbytes + self.post + 512, dtype=torch.uint8, device=device)
        want = 0 if align == 256 else 16  # payload address modulo 256
        off = (want - (raw.data_ptr() + PRE)) % 256
        self.arena = raw[off: off + PRE + self.nbytes + self.post]  # pre | payload | post, nothing else
        self._raw = raw
        if fill == 0xFF:
            self.arena.fill_(0xFF)
        else:
            g = torch.Generator(device=device).manual_seed(0x6A11 + int(fill))
            self.arena.copy_(torch.randint(0, 256, (self.arena.numel(),), dtype=torch.uint8, device=device, generator=g))
        self.payload = self.arena[PRE: PRE + self.nbytes]
        self.ptr = self.arena.data_ptr() + PRE
        assert self.ptr % 256 == want and self.payload.numel() == self.nbytes
        self.snapshot = self.arena.clone()

    # -- contents ----------------------------------------------------------------------------------------------------------
    def load(self, t: torch.Tensor) -> "Guarded":
        """Copy a dense tensor's bytes to the head of the payload (an input) and take a new snapshot."""
        src = t.contiguous().reshape(-1).view(torch.uint8)
        assert src.numel() <= self.nbytes, f"{self.name}: {src.numel()} B do not fit the payload of {self.nbytes} B"
        self.payload[: src.numel()].copy_(src)
        self.snapshot = self.arena.clone()
        return self

    def load_rows(self, t: torch.Tensor, ld: int) -> "Guarded":
        """Copy t [M, N] into the window of row stride `ld` elements (the gaps keep the guard pattern) and take a new snapshot."""
        M, N = t.shape
        self.rows_view(M, N, ld, t.dtype).copy_(t)
        self.snapshot = self.arena.clone()
        return self

    def view(self, dtype, count=None, offset_bytes=0) -> torch.Tensor:
        esz = _DT_BYTES[dtype]
        n = (self.nbytes - offset_bytes) // esz if count is None else count
        return self.payload[offset_bytes: offset_bytes + n * esz].view(dtype)

    def rows_view(self, M: int, N: int, ld: int, dtype) -> torch.Tensor:
        """The [M, N] window of row stride `ld` elements at the head of the payload."""
        esz = _DT_BYTES[dtype]
        assert ld >= N and ((M - 1) * ld + N) * esz <= self.nbytes if M > 0 else True
        if M == 0:
            return self.payload[:0].view(dtype).reshape(0, N)
        flat = self.payload[: ((M - 1) * ld + N) * esz].view(dtype)
        return flat.as_strided((M, N), (ld, 1))

    # -- checks (call after torch.cuda.synchronize()) -----------------------------------------------------------------------
    def _where(self, idx: int) -> str:
        """Arena index -> text: offset from the payload end and, with a pitch, row / byte column counted from the payload start."""
        rel_end = idx - (PRE + self.nbytes)
        s = f"offset {rel_end:+d} B from the payload end"
        if idx < PRE:
            s += f" ({idx - PRE:+d} B from the payload start)"
        if self.pitch:
            rel = idx - PRE
            s += f" = row {rel // self.pitch}, byte column {rel % self.pitch} of pitch {self.pitch}"
        return s

    def _diff(self, lo: int, hi: int, mask=None):
        d = self.arena[lo:hi] != self.snapshot[lo:hi]
        if mask is not None:
            d &= mask
        if not bool(d.any()):
            return None
        nz = d.nonzero()
        return lo + int(nz[0]), lo + int(nz[-1]), int(nz.numel())

    def _fail(self, what: str, hit) -> str:
        first, last, n = hit
        return (f"GUARD TRIPPED: {self.name} ({self.nbytes} B): {what} changed: {n} byte(s), first at {self._where(first)}, last at {self._where(last)}")

    def check(self) -> None:
        """pre and post bit-equal to the snapshot."""
        for what, lo, hi in (("the guard IN FRONT of the payload", 0, PRE), ("the guard BEHIND the payload", PRE + self.nbytes, self.arena.numel())):
            hit = self._diff(lo, hi)
            assert hit is None, self._fail(what, hit)

    def unchanged(self) -> None:
        """A read-only input: guards AND payload bit-equal to the snapshot."""
        hit = self._diff(0, self.arena.numel())
        assert hit is None, self._fail("a read-only buffer", hit)

    def gaps_unchanged(self, M: int, N: int, ld: int, dtype) -> None:
        """Columns N..ld-1 of rows 0..M-2 (the payload ends with row M-1's last element) bit-equal to the snapshot."""
        esz = _DT_BYTES[dtype]
        if M <= 1 or ld == N:
            return
        span = ((M - 1) * ld + N) * esz
        col = torch.arange(span, device=self.arena.device) % (ld * esz)
        hit = self._diff(PRE, PRE + span, col >= N * esz)
        assert hit is None, self._fail(f"the gap between rows (columns {N}..{ld - 1})", hit)

    def payload_bytes(self) -> torch.Tensor:
        return self.payload.clone()


def guarded(nbytes: int, *, row_pitch_bytes: int = 0, align: int = 256, fill=0, name: str = "buffer", device="cuda:0") -> Guarded:
    return Guarded(nbytes, row_pitch_bytes=row_pitch_bytes, align=align, fill=fill, name=name, device=device)


def rows_bytes(M: int, N: int, ld: int, esz: int) -> int:
    """Bytes of an [M, N] window with row stride ld: up to and including the last element of row M-1, nothing behind it."""
    return ((M - 1) * ld + N) * esz if M > 0 else 0
