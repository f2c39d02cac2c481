"""A guarded, poisoned arena for the buffers a C-ABI caller owns (include/csa_hip.h: "the caller allocates every
output, the saved state and the workspace"). Works on CPU and CUDA tensors alike; no GPU is needed to import it.

Every buffer a test hands to the library is carved out of ONE uint8 allocation:

    ... | GUARD bytes of 0xA5 | body, prefilled with a poison byte | GUARD bytes of 0xA5 | ...

- A body is exactly as large as asked (the byte count of a *_bytes() query, or a tensor's shape); the space up to
  the next alignment boundary behind it belongs to the guard, so a store one element past either end is seen.
- A body starts at an address that is `align` modulo 256 (align < 256) or a multiple of 256: align=256 is what the
  caching allocator gives the op shim for state and workspace; align=16 is all the ABI asks of Q / K / V / X-like
  operands, and the body is then deliberately NOT 256-byte aligned.
- A strided body is a view (or several) of a larger container, e.g. a (B,H,R,d) output that is the head-major view
  of a (B,R,H,d+4) buffer, or dQ / dK / dV as the three views of one packed (B,R,3,H,d) gradient. The elements of
  the container that no view addresses (the gaps) are guard: they hold 0xA5 and must keep it.
- assert_guards_intact() checks every guard byte and gap element with one masked reduction on the device and
  names the nearest buffer and the byte offset of the first byte that changed.
- assert_written(view) checks that no addressed element still holds the 0xFF poison pattern (all bits set), and
  that a floating-point view is finite everywhere. All-ones is a NaN in fp32 and bf16, so an unwritten element of
  a float output can never pass for a value.

The poison byte is the arena's: a test runs the same call sequence in an arena poisoned 0x00 and in one poisoned
0xFF and compares the outputs bitwise; a kernel that reads state, workspace or output memory nobody wrote gives
different bits (0 * NaN = NaN in a padded row, an Abits word that reads as all edges, ...)."""
import torch

GUARD = 4096
GUARD_FILL = 0xA5
POISON_ZERO, POISON_ONES = 0x00, 0xFF
LINE = 256  # the allocator's granularity: bodies with align=256 start on it


class GuardError(AssertionError):
    pass


def _nbytes(shape, dtype):
    n = torch.empty((), dtype=dtype).element_size()
    for s in shape:
        n *= int(s)
    return n


class Arena:
    def __init__(self, device="cpu", capacity=32 << 20, poison=POISON_ONES):
        """capacity: bytes of the one allocation everything is carved from; carve() raises when it is used up."""
        assert 0 <= poison <= 255 and poison != GUARD_FILL
        self.device = torch.device(device)
        self.poison = poison
        self.buf = torch.empty(capacity + LINE, dtype=torch.uint8, device=self.device)
        self.is_guard = torch.empty(capacity + LINE, dtype=torch.bool, device=self.device)
        self.base = self.buf.data_ptr()
        self.used = 0
        self.records = []  # (name, body start, body bytes) in carve order

    # -----------------------------------------------------------------------------------------------------
    def carve(self, name, nbytes=None, shape=None, dtype=torch.float32, align=LINE, views=None):
        """A body of `nbytes` bytes (a uint8 tensor) or of `shape` / `dtype` (contiguous), with a guard on both sides.

        views: a function of the (shape, dtype) container that returns one view of it or a tuple of views (the strided
        bodies). Only the elements those views address are body; the rest of the container is guard. Returns what
        `views` returned."""
        assert (nbytes is None) != (shape is None) and name not in [r[0] for r in self.records]
        assert align in (4, 8, 16, 32, 64, 128, LINE)
        if shape is None:
            shape, dtype = (int(nbytes),), torch.uint8
        size = _nbytes(shape, dtype)
        start = self.used + GUARD
        start += (align % LINE - (self.base + start)) % LINE
        end = start + size
        new_used = end + GUARD + (-(end + GUARD)) % 16
        if new_used > self.buf.numel():
            raise GuardError(f"arena capacity {self.buf.numel()} exhausted at '{name}' ({size} bytes)")
        self.buf[self.used:new_used] = GUARD_FILL
        self.is_guard[self.used:new_used] = True
        body = self.buf[start:end].view(dtype).view(*shape) if size else self.buf[start:start].view(dtype).view(*shape)
        if views is None:
            self.is_guard[start:end] = False
            out = body
        else:
            # the same views of an alias of the mask mark the addressed elements (every byte of each element)
            out = views(body)
            ints = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[body.element_size()]
            marks = views(self.is_guard[start:end].view(torch.uint8).view(ints).view(*shape))
            for m in (marks if isinstance(marks, (tuple, list)) else (marks,)):
                m.zero_()
        self.records.append((name, start, size))
        self.used = new_used
        self.fill(name, self.poison)
        return out

    def fill(self, name, byte):
        """Sets every body byte of buffer `name` (its addressed elements only) to `byte`: a fresh poison."""
        _, start, size = next(r for r in self.records if r[0] == name)
        region = self.buf[start:start + size]
        region[~self.is_guard[start:start + size]] = byte

    def address_mod(self, name, mod=LINE):
        _, start, _ = next(r for r in self.records if r[0] == name)
        return (self.base + start) % mod

    # -----------------------------------------------------------------------------------------------------
    def assert_guards_intact(self, where=""):
        """Every guard byte and every gap element still holds GUARD_FILL (one masked reduction, one sync)."""
        buf, g = self.buf[:self.used], self.is_guard[:self.used]
        bad = (buf != GUARD_FILL) & g
        if not bool(bad.any()):
            return
        off = int(torch.nonzero(bad)[0])
        n = int(bad.sum())
        # the buffer whose body is nearest to the byte
        name, start, size = min(self.records, key=lambda r: 0 if r[1] <= off < r[1] + r[2] else
                                min(abs(off - r[1]), abs(off - (r[1] + r[2] - 1))))
        rel = off - start
        side = "before its start" if rel < 0 else "past its end" if rel >= size else "in a stride gap"
        raise GuardError(f"{where}: stray store near buffer '{name}' ({size} bytes): byte offset {rel} ({side}) holds "
                         f"0x{int(buf[off]):02x}, not the guard 0x{GUARD_FILL:02x}; {n} guard byte(s) changed in all")

    @staticmethod
    def assert_written(view, name="output"):
        """No addressed element of `view` is the 0xFF poison pattern; a floating-point view is finite everywhere."""
        if view.numel() == 0:
            return
        ints = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[view.element_size()]
        # value-preserving copy of the addressed elements only (contiguous), then their bits
        bits = view.contiguous().view(ints)
        ones = 0xFF if ints == torch.uint8 else -1
        unwritten = bits == ones
        if bool(unwritten.any()):
            idx = tuple(int(i) for i in torch.nonzero(unwritten)[0])
            raise GuardError(f"'{name}': element {idx} was never written (still the 0xFF poison); "
                             f"{int(unwritten.sum())} of {view.numel()} unwritten")
        if view.is_floating_point() and not bool(torch.isfinite(view).all()):
            idx = tuple(int(i) for i in torch.nonzero(~torch.isfinite(view))[0])
            raise GuardError(f"'{name}': element {idx} is {float(view[idx])}, not finite")
