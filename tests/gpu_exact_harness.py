"""What the exact GPU test files (tests/test_gpu_train_exact.py, tests/test_gpu_train_pointwise_exact.py) share: outputs between NaN guard
bands, workspaces of exactly the size the library asks for with a NaN guard behind them, operands inside NaN-filled buffers, and "run it twice,
the bits must agree".  Helpers only: no test lives here."""
import torch

from tests import train_exact_cases as tc

GUARD = 64                        # floats of NaN before and after every output and after every workspace
NAN_BITS = 0x7FC00000             # what torch.full(..., nan) writes


def _untouched(t):
    return bool((t.view(torch.int32) == NAN_BITS).all())


class _Out:
    """n floats of output between two guard bands, everything NaN"""

    def __init__(self, n, dev):
        self.n = int(n)
        self.buf = torch.full((GUARD + self.n + GUARD,), tc.NAN, device=dev)
        self.ptr = self.buf.data_ptr() + 4 * GUARD

    def values(self, shape):
        return self.buf[GUARD:GUARD + self.n].view(*shape)

    def guards_untouched(self):
        return _untouched(self.buf[:GUARD]) and _untouched(self.buf[GUARD + self.n:])


class _Workspace(_Out):
    """nbytes of workspace (a whole number of floats) with a guard band behind it"""

    def __init__(self, nbytes, dev):
        assert nbytes % 4 == 0 and nbytes > 0
        super().__init__(nbytes // 4, dev)
        self.bytes = int(nbytes)


def _device(placed, dev):
    """(the buffer on the device, the pointer to the operand's element (0,0,0)); fresh allocations are 256-byte aligned, which is what the
    host test assumes when it asks the routing query which kernel a case runs on"""
    buf = placed.buf.to(dev)
    assert buf.data_ptr() % 256 == 0
    return buf, buf.data_ptr() + 4 * placed.offset


def _same(got, ref, what, explain=None):
    got, ref = got.cpu(), ref.float()
    idx = tc.first_mismatch(got, ref)
    if idx is not None:
        more = explain(idx, float(got[idx])) if explain else ""
        raise AssertionError("%s: first differing index %s of %s: got %r, expected %r%s; %d of %d elements differ" % (
            what, idx, tuple(ref.shape), float(got[idx]), float(ref[idx]), more, int((~(got == ref)).sum()), ref.numel()))
    assert torch.equal(got, ref)


def _twice(launch, out_floats, ws_bytes, dev):
    """run `launch(out, ws)` twice on fresh NaN-filled buffers; the bits must agree, the guards must be NaN: returns the first output"""
    runs = []
    for _ in range(2):
        out, ws = _Out(out_floats, dev), (_Workspace(ws_bytes, dev) if ws_bytes else None)
        launch(out, ws)
        torch.cuda.synchronize()
        assert out.guards_untouched(), "the guard bands of the output were written"
        assert ws is None or _untouched(ws.buf[GUARD + ws.n:]) and _untouched(ws.buf[:GUARD]), "the kernel wrote outside its workspace"
        runs.append(out)
    assert torch.equal(runs[0].buf.view(torch.int32), runs[1].buf.view(torch.int32)), "two runs of the same call differ"
    return runs[0]


# ------------------------------------------------------------------------------------------------ byte-sized buffers of any element type
class Guarded:
    """`nbytes` bytes at a chosen byte offset from a 256-byte aligned address, inside a NaN-filled buffer with GUARD floats of NaN in front
    and behind: an output (left NaN), a workspace, or an operand (`put`).  `offset` moves the pointer off its natural alignment; the bytes
    skipped stay NaN and count as guard.  `compare`: whether two runs must leave the same bits here (not for workspaces)."""

    def __init__(self, nbytes, dev, offset=0, compare=True):
        self.nbytes, self.compare = int(nbytes), compare
        words = 2 * GUARD + (offset + self.nbytes + 3) // 4
        self.buf = torch.full((words,), tc.NAN, device=dev)
        assert self.buf.data_ptr() % 256 == 0
        self.lo = 4 * GUARD + offset
        self.ptr = self.buf.data_ptr() + self.lo

    def _bytes(self):
        return self.buf.view(torch.uint8)[self.lo:self.lo + self.nbytes]

    def view(self, dtype, *shape):
        t = self._bytes().view(dtype)
        return t.view(*shape) if shape else t

    def cpu(self, dtype, *shape):
        return self.view(dtype, *shape).cpu()

    def guards_untouched(self):
        c = self.buf.clone()
        c.view(torch.uint8)[self.lo:self.lo + self.nbytes] = torch.full_like(self.buf, tc.NAN).view(torch.uint8)[self.lo:self.lo + self.nbytes]
        return _untouched(c)


def put(t, dev, offset=0):
    """the CPU tensor t as an operand inside a NaN-filled buffer (None stays None)"""
    if t is None:
        return None
    t = t.contiguous()
    g = Guarded(t.numel() * t.element_size(), dev, offset)
    g.view(t.dtype).copy_(t.reshape(-1).to(dev))
    return g


def gptr(g):
    return None if g is None else g.ptr


def twice(run):
    """`run()` allocates fresh buffers, launches, and returns the list of its Guarded outputs and workspaces.  It runs twice: every guard band
    must still be NaN and every compared buffer must hold the same bits after both runs.  Returns the first run's list."""
    first = run()
    torch.cuda.synchronize()
    second = run()
    torch.cuda.synchronize()
    for i, (a, b) in enumerate(zip(first, second)):
        assert a.guards_untouched() and b.guards_untouched(), "buffer %d: bytes outside the buffer were written" % i
        if a.compare:
            assert torch.equal(a.buf.view(torch.int32), b.buf.view(torch.int32)), "buffer %d: two runs of the same call differ" % i
    return first


def same_bits(got, ref, what):
    """got, ref: CPU tensors of one 4-byte (or integer) type; equal bit for bit (so +0 is not -0, and a NaN equals the same NaN)"""
    assert got.shape == ref.shape and got.dtype == ref.dtype, "%s: %s %s against %s %s" % (what, got.dtype, tuple(got.shape), ref.dtype, tuple(ref.shape))
    view = {4: torch.int32, 8: torch.int64, 1: torch.uint8}[got.element_size()]
    g, r = got.contiguous().view(view), ref.contiguous().view(view)
    idx = tc.first_mismatch(g, r)
    if idx is not None:
        raise AssertionError("%s: first differing index %s of %s: got %r, expected %r; %d of %d elements differ" % (
            what, idx, tuple(ref.shape), got[idx].item(), ref[idx].item(), int((g != r).sum()), ref.numel()))
