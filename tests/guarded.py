"""Device buffers of exactly their contract size for the workspace tests
(tests/test_gpu_lists_workspace.py, tests/test_gpu_codec_workspace.py): a
view of `size` bytes inside a larger buffer, at a chosen distance past a
256-byte boundary, with at least GUARD bytes of a fill byte on either side.
One class serves every pointer argument of a call -- the workspace, an
encoder's d_out, a decoder's values, offsets, d_err, d_total -- so a write
before the pointer or past the contract size lands in the guards and is seen
there.  Test infrastructure only."""
import numpy as np

DEV = "cuda:0"
GUARD = 4096
FILL = 0xC3


class Guarded:
    """A view of exactly `size` bytes, `mis` bytes past a 256-byte boundary, with at least GUARD sentinel bytes on either side.
    init: the byte the view itself starts with (default: the guards' fill byte)."""

    def __init__(self, size, mis=0, init=None):
        import torch

        self.size = size
        self.big = torch.full((GUARD + 256 + size + GUARD,), FILL, dtype=torch.uint8, device=DEV)
        self.s = GUARD + (mis - (self.big.data_ptr() + GUARD)) % 256
        self.view = self.big[self.s: self.s + size]
        assert self.view.data_ptr() % 256 == mis and self.view.numel() == size
        if init is not None:
            self.view.fill_(init)

    def fill(self, what):
        """what: a byte, or a uint8 device tensor that is repeated over the view"""
        if isinstance(what, int):
            self.view.fill_(what)
        else:
            reps = -(-self.size // what.numel())
            self.view.copy_(what.repeat(reps)[: self.size])

    def put(self, a):
        """the bytes of the numpy array `a`, which has exactly the view's size"""
        import torch

        raw = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
        assert len(raw) == self.size
        if self.size:
            self.view.copy_(torch.from_numpy(raw))
        return self

    def as_(self, dtype):
        """the view as a tensor of `dtype` (torch.int32, torch.int64: the base must be aligned to it)"""
        return self.view.view(dtype)

    def read(self, dtype=np.uint8):
        """-> (the view's contents as `dtype`, True when both guards still hold the fill byte), in one copy"""
        got = self.big.cpu().numpy()
        ok = bool((got[: self.s] == FILL).all() and (got[self.s + self.size:] == FILL).all())
        return got[self.s: self.s + self.size].view(dtype), ok

    def intact(self):
        return self.read()[1]


Workspace = Guarded
