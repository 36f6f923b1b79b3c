"""Out-of-view-write canaries for the image-side kernel tests (preprocess.hip, augment.hip, ccl.hip): one allocation, a view
of exactly the requested bytes at a requested alignment in its middle, a fixed byte pattern on both sides of it (and in it,
so an output a kernel did not write is as visible as one it wrote too far)."""
import numpy as np
import torch

CANARY = 0xA5                     # every byte of the allocation before the kernel runs
GUARD = 512                       # canary bytes on either side of the view (at least: the alignment slack adds to the front)


class Canaried:
    """`nbytes` bytes of `device` memory whose address is `skew` past a multiple of `align`, between two canary regions.
    u8 is the view as bytes, ptr its address, view(dtype, *shape) the same bytes typed (skew must suit the dtype)."""

    def __init__(self, nbytes, align=256, skew=0, device="cuda", guard=GUARD):
        assert nbytes >= 0 and align >= 1 and 0 <= skew < align and guard >= 1
        self.buf = torch.full((guard + align + nbytes + guard,), CANARY, dtype=torch.uint8, device=device)
        self.start = guard + (-(self.buf.data_ptr() + guard)) % align + skew
        self.nbytes = int(nbytes)
        self.u8 = self.buf[self.start:self.start + self.nbytes]
        self.ptr = self.buf.data_ptr() + self.start
        assert self.ptr % align == skew

    def view(self, dtype, *shape):
        return self.u8.view(dtype).view(*shape)

    def numpy(self, dtype, *shape):
        """Host copy of the view (after check(), which is where a stray write is reported)."""
        return self.u8.cpu().numpy().view(dtype).reshape(*shape)

    def untouched(self):
        """True while the view itself still holds the canary pattern (nothing was launched on it)."""
        return bool((self.u8 == CANARY).all())

    def check(self, what="view"):
        b = self.buf.cpu().numpy()
        lo, hi = b[:self.start], b[self.start + self.nbytes:]
        assert np.all(lo == CANARY), f"write below the {what}: {int((lo != CANARY).sum())} bytes of {self.nbytes}-byte view"
        assert np.all(hi == CANARY), f"write above the {what}: first at byte +{int(np.argmax(hi != CANARY))} past its end"


def canaried_like(array, align=256, skew=0, device="cuda"):
    """A Canaried view holding a copy of the numpy `array` (an input that must sit at a given alignment)."""
    a = np.ascontiguousarray(array)
    c = Canaried(a.nbytes, align, skew, device)
    c.u8.copy_(torch.from_numpy(a.reshape(-1).view(np.uint8)))
    return c


def check_all(*views):
    for i, v in enumerate(views):
        v.check(f"view {i}")
