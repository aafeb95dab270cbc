"""A guarded, poisoned arena for the device-pointer entry points (tests/device_buffer_cases.py, tests/test_gpu_device_buffers.py).

Every buffer a call is given comes out of an `Arena`: one uint8 tensor of guard + nbytes + guard bytes, the whole of it filled with the arena's
poison byte, the payload in the middle.  A kernel that writes past either end of a buffer lands in a guard the test owns -- `check()` finds the byte --
instead of in the slack of an allocator's block, where nothing looks; an output element the launch never writes still holds the poison, which with
0xA5 underneath cannot equal the reference.  guard = max(4096, 64 * row_bytes) rounded up to 256: a whole ragged workgroup of rows on either side.

Inputs (`init=`) go through the same helper: the payload holds the data, the guards the poison; their guards are checked like any other and
`unchanged()` says whether the read-only ones came back as they went in.

Works on device="cpu" too (tests/test_device_buffers_cpu.py).  On a GPU the fills and copies are enqueued on torch's current stream: allocate inside
`with torch.cuda.stream(s):` and they are ordered on s like the launches that follow."""
import numpy as np
import torch

ALIGN = 256
MIN_GUARD = 4096
GUARD_ROWS = 64


def guard_bytes(row_bytes):
    g = max(MIN_GUARD, GUARD_ROWS * int(row_bytes))
    return (g + ALIGN - 1) // ALIGN * ALIGN


class Buf:
    """one buffer of an arena: .ptr (device address of the payload), .view (typed tensor over the payload), .host() (the payload as numpy)"""

    def __init__(self, name, whole, guard, nbytes, dtype, sent):
        self.name, self.whole, self.guard, self.nbytes, self.dtype, self.sent = name, whole, guard, nbytes, np.dtype(dtype), sent
        self.payload = whole[guard:guard + nbytes]
        self.ptr = whole.data_ptr() + guard
        self.view = self.payload.view(_TORCH[self.dtype]) if nbytes else self.payload

    def host(self, shape=None):
        a = self.payload.cpu().numpy().view(self.dtype)
        return a if shape is None else a.reshape(shape)


_TORCH = {np.dtype(np.uint8): torch.uint8, np.dtype(np.int32): torch.int32, np.dtype(np.uint32): torch.int32, np.dtype(np.uint16): torch.int16,
          np.dtype(np.float64): torch.float64, np.dtype(np.uint64): torch.int64}


class Arena:
    def __init__(self, device, poison):
        self.device, self.poison = torch.device(device), int(poison) & 0xFF
        self.bufs = {}

    def buf(self, name, nbytes, row_bytes, dtype=np.uint8, init=None):
        """A buffer of nbytes whose rows are row_bytes long.  init: a numpy array of exactly nbytes -- an input, copied into the payload; else
        the payload holds the poison like the guards.  Returns (pointer, typed view of the payload); arena.bufs[name] keeps the rest."""
        assert name not in self.bufs, name
        nbytes, guard = int(nbytes), guard_bytes(row_bytes)
        total = guard + nbytes + guard
        # (the allocators promise less than 256 bytes of alignment on the host: take the slack and cut the tensor out at a multiple of 256)
        raw = torch.full((total + ALIGN,), self.poison, dtype=torch.uint8, device=self.device)
        off = -raw.data_ptr() % ALIGN
        whole = raw[off:off + total]
        sent = None
        if init is not None:
            sent = np.ascontiguousarray(init).view(np.uint8).reshape(-1).copy()
            assert sent.size == nbytes, (name, sent.size, nbytes)
            if nbytes:
                whole[guard:guard + nbytes].copy_(torch.from_numpy(sent))
        b = Buf(name, whole, guard, nbytes, dtype, sent)
        b._raw = raw
        self.bufs[name] = b
        return b.ptr, b.view

    def __getitem__(self, name):
        return self.bufs[name]

    def check(self):
        """the buffers whose guards no longer hold the poison: "name: front guard, first byte at payload - k" / "name: back guard, first byte at
        payload end + k" -- [] when no byte outside any payload was written"""
        bad = []
        for b in self.bufs.values():
            w = b.whole.cpu().numpy()
            front, back = w[:b.guard], w[b.guard + b.nbytes:]
            hit = np.flatnonzero(front != self.poison)
            if hit.size:
                bad.append("%s: front guard, first byte at payload - %d (%d bytes)" % (b.name, b.guard - int(hit[0]), hit.size))
            hit = np.flatnonzero(back != self.poison)
            if hit.size:
                bad.append("%s: back guard, first byte at payload end + %d (%d bytes)" % (b.name, int(hit[0]), hit.size))
        return bad

    def unchanged(self, name):
        """an input's payload is what went in"""
        b = self.bufs[name]
        assert b.sent is not None, name + " is no input"
        return np.array_equal(b.payload.cpu().numpy(), b.sent)
