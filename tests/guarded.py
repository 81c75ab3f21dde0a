"""What the GPU tests of the single kernels share on the device side: the sentinels, the return codes, the upload, and ONE output buffer
that starts as sentinels between guard rows and proves after the call that nothing but the call's own part was written. torch; the
comparison against a reference lives in oracle/fp.py. Importing this file needs no device."""
import numpy as np
import torch

SENTINEL = 777.0          # float buffers: finite, fp16-exact, far outside every expected output
ISENTINEL = -123456789    # int buffers
OK, E_INVALID, E_WORKSPACE, E_STATE = 0, -1, -4, -5   # MDR_OK and MDR_E_* of include/mdr_hip.h


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def assert_untouched(a, message):
    """every element of `a` (numpy or torch) still holds the sentinel of its type"""
    assert bool((a == (ISENTINEL if str(a.dtype).endswith("int32") else SENTINEL)).all()), message


class Guarded:
    """One output buffer: `n` rows of shape `tail` (n elements if tail is empty) that belong to the call, `front` guard rows before and `back`
    behind them, everything filled with the sentinel, the call's own part with `init` (numpy: old values) if given. `own` is the device
    view to hand to the call. name / unit word the messages ("dx rows ..."); `outside` replaces the message for a written guard."""

    def __init__(self, n, tail, dtype, front, back, init=None, name="", unit="rows", outside=None):
        self.n, self.front, self.name, self.what, self.fresh = n, front, name, f"{name} {unit}".strip(), init is None
        self.outside = outside or f"{self.what} outside the call were written"
        self.buf = torch.full((front + n + back,) + tuple(tail), ISENTINEL if dtype == torch.int32 else SENTINEL, dtype=dtype, device="cuda")
        self.own = self.buf[front:front + n]
        if init is not None:
            self.own.copy_(dev(init).reshape(self.own.shape))

    def ptr(self, asked=True):
        from multihop_dense_retrieval_amd import _lib
        return _lib.ptr(self.own) if asked else None

    def checked(self, whole=None, valid=None, asked=True):
        """AFTER a synchronise: the call's own part of `whole` (default: the host copy of the buffer, numpy; a caller that stays on the device
        passes the buffer itself), having asserted that the guards kept their bits, that rows at or behind `valid` kept the sentinel, and that
        a buffer that was not asked for (and holds no old values) was not written at all."""
        whole = self.buf.cpu().numpy() if whole is None else whole
        lo, hi = self.front, self.front + self.n
        if lo:
            assert_untouched(whole[:lo], self.outside)
        assert_untouched(whole[hi:], self.outside)
        if not asked:
            if self.fresh:
                assert_untouched(whole, f"{self.name} written though not asked for")
        elif valid is not None:
            assert_untouched(whole[lo + valid:hi], f"{self.what} at or behind the valid count were written")
        return whole[lo:hi]
