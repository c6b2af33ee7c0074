"""Guard-band allocator of the kernel tests: every operand of a launch sits in the middle of a larger allocation whose margins hold a
poison byte, so that what a kernel does OUTSIDE an operand along the pixel direction - a pixel row before image 0 or after image
n - 1, a partial last tile past the end of y, a weight row past cout_pad x kpad, a workspace overrun - lands in memory the test owns
and is seen:
  * a WRITE changes margin bytes: Guard.assert_intact() names the operand, the side, the count and the first offset;
  * a READ picks up the poison, and shows in the test's value comparison wherever the value reaches a result.
Two poisons, because each is blind in one direction:
  * 0xFF is NaN in bf16, f16 and f32 (and -1 in int32): it survives a multiplication by a zero-padded weight, but a max or a compare
    can drop it;
  * 0x7F is 3.39e38 in bf16 and f32 (NaN in f16): a max pool or a compare carries it, a multiplication by zero makes it vanish.
The limit of the method: a stray read whose value a later select discards stays invisible, and so does a stray write of the poison's
own bytes (a max pool that stores the 3.39e38 it read from a 0x7F margin: the 0xFF run sees that write) - one more reason for two.

Margin per operand (margin_bytes): 64 KiB, or the bytes of one image plane [h, w, c_total] of the operand where that is more - the
over-reach of a tile or strip kernel is bounded by one band of one image -, rounded up to 256 so that the payload keeps the 256-byte
alignment of a plain allocation (the kernels use 16-byte vector and LDS-DMA loads)."""
import torch

POISONS = (0xFF, 0x7F)
MIN_MARGIN = 65536
ALIGN = 256


def _prod(shape):
    n = 1
    for v in shape:
        n *= int(v)
    return n


def itemsize(dtype):
    return torch.empty((), dtype=dtype).element_size()


def margin_bytes(shape, dtype, plane=None):
    """Margin of an operand: ``plane`` = elements of one image plane; by default everything but the leading dimension of a tensor
    of four and more dimensions (NHWC / NCHW / [bs, na, ny, nx, no])."""
    if plane is None:
        plane = _prod(shape[1:]) if len(shape) >= 4 else 0
    return (max(MIN_MARGIN, int(plane) * itemsize(dtype)) + ALIGN - 1) // ALIGN * ALIGN


def _aligned_raw(nbytes, poison, device):
    """A uint8 tensor of nbytes, filled with the poison, whose first byte is 256-byte aligned (a device allocation is; a host one is
    cut out of a slightly larger one)."""
    raw = torch.full((nbytes + ALIGN,), poison, dtype=torch.uint8, device=device)
    skip = -raw.data_ptr() % ALIGN
    return raw[skip:skip + nbytes]


class Guard:
    """Collector of one test's guarded allocations."""

    def __init__(self, poison, device):
        assert poison in POISONS
        self.poison, self.device, self.items = poison, device, []

    def alloc(self, name, shape, dtype, fill=None, plane=None):
        """guarded() with this collector's poison and device, recorded under ``name``."""
        return guarded(shape, dtype, fill, self.poison, self.device, self, name, plane)

    def like(self, name, src, plane=None):
        """A guarded copy of the tensor ``src`` (any device)."""
        t = self.alloc(name, src.shape, src.dtype, plane=plane)
        t.copy_(src)
        return t

    def report(self):
        """[(operand, "below" | "above", changed bytes, offset of the first one)]; offsets count from the payload's first byte
        (below: negative) / from the first byte after the payload (above: 0 is the byte right behind it)."""
        out = []
        for name, raw, rz, nbytes in self.items:
            for side, seg, base in (("below", raw[:rz], -rz), ("above", raw[rz + nbytes:], 0)):
                bad = seg != self.poison
                n = int(bad.sum())
                if n:
                    out.append((name, side, n, base + int(bad.nonzero()[0])))
        return out

    def assert_intact(self):
        rep = self.report()
        assert not rep, "writes outside an operand (poison 0x%02X): " % self.poison + "; ".join(
            f"{name}: {n} byte(s) {side} the payload changed, first at offset {off}" for name, side, n, off in rep)


def guarded(shape, dtype, fill, poison, device, collector=None, name="operand", plane=None):
    """A contiguous tensor of ``shape`` / ``dtype`` that is a view into the middle of a larger uint8 allocation: both margins
    (margin_bytes) hold the ``poison`` byte, the payload holds ``fill`` (a number, NaN included; None: zero bytes).  ``collector``
    (a Guard) records the allocation under ``name`` for its margin check."""
    shape = tuple(int(v) for v in shape)
    nbytes = _prod(shape) * itemsize(dtype)
    rz = margin_bytes(shape, dtype, plane)
    raw = _aligned_raw(nbytes + 2 * rz, poison, device)
    t = raw[rz:rz + nbytes].view(dtype).view(shape)
    if fill is None:
        raw[rz:rz + nbytes].zero_()
    else:
        t.fill_(fill)
    if collector is not None:
        collector.items.append((name, raw, rz, nbytes))
    return t


class Plain:
    """The same interface on plain allocations: the un-guarded run a guarded one is compared with."""
    poison = None

    def __init__(self, device):
        self.device = device

    def alloc(self, name, shape, dtype, fill=None, plane=None):
        shape = tuple(int(v) for v in shape)
        if fill is None:
            return torch.zeros(shape, dtype=dtype, device=self.device)
        return torch.full(shape, fill, dtype=dtype, device=self.device)

    def like(self, name, src, plane=None):
        return src.detach().clone().to(self.device).contiguous()

    def report(self):
        return []

    def assert_intact(self):
        pass
