"""Rows whose offsets need 64 bits, for the GPU tests of the learner's pitches (tests/test_gpu_wide_pitch.py).

``WideRows(rows, width, itemsize)`` is ONE large ``torch.empty`` allocation seen as `rows` rows of `width` elements at a
pitch chosen so that the first rows start below element 2^31 and the last ones (at least one, at most three) at or beyond
it -- and at or beyond byte 2^32: an index that a kernel computed as ``row * pitch`` in 32 bits, signed in elements or
unsigned in bytes, lands somewhere else.  Only the rows are ever written: the test puts its inputs there, and a guard of
`guard` elements behind every row holds a poison pattern that ``get`` finds again.  Everything between the rows is whatever
the allocator returned; no launch of the tests reads or writes it, and every address a launch forms from (pointer, row,
pitch, width) lies inside the allocation.  `views` > 1 lays that many such row sets side by side in the same allocation, each
`width + guard` elements further in, for entry points that take one pitch for several tensors.
"""
import numpy as np
import torch

POISON = -7
LIMIT_BYTES = 10 << 30        # the most a test's large buffer may take
DTYPES = {1: torch.uint8, 2: torch.int16, 4: torch.int32}


class WideRows:
    def __init__(self, rows, width, itemsize, views=1, guard=16, device="cuda:0"):
        assert rows >= 2 and width >= 1 and views >= 1
        beyond = min(3, max(1, rows // 8))                             # how many rows start at or beyond the limit
        span = max(1 << 31, (1 << 32) // itemsize)                     # elements: beyond int32 as an index AND beyond 2^32 bytes
        self.rows, self.width, self.itemsize, self.views = rows, width, itemsize, views
        self.slot = width + guard
        self.pitch = -(-span // (rows - beyond)) + 7                   # (odd on purpose: no alignment comes for free)
        self.first_beyond = rows - beyond
        assert (self.first_beyond - 1) * self.pitch < span <= self.first_beyond * self.pitch
        self.elements = (rows - 1) * self.pitch + views * self.slot
        assert self.elements * itemsize <= LIMIT_BYTES and views * self.slot <= self.pitch
        self.buffer = torch.empty(self.elements, dtype=DTYPES[itemsize], device=device)
        for v in range(views):
            self._slots(v).fill_(POISON)

    def _slots(self, v):
        return self.buffer.as_strided((self.rows, self.slot), (self.pitch, 1), v * self.slot)

    def view(self, v=0):
        """the [rows, width] strided view of row set v"""
        return self.buffer.as_strided((self.rows, self.width), (self.pitch, 1), v * self.slot)

    def ptr(self, v=0):
        return self.buffer.data_ptr() + v * self.slot * self.itemsize

    def put(self, bits, v=0):
        """write the element patterns `bits` [rows, width] (any numpy dtype of the item size)"""
        bits = np.ascontiguousarray(bits)
        assert bits.shape == (self.rows, self.width) and bits.dtype.itemsize == self.itemsize
        host = bits.view({1: np.uint8, 2: np.int16, 4: np.int32}[self.itemsize])
        self.view(v).copy_(torch.from_numpy(host).to(self.buffer.device))
        return self

    def get(self, v=0):
        """the [rows, width] element patterns as numpy; the guard behind every row must still hold the poison"""
        slots = self._slots(v).cpu().numpy()
        poison = np.array(POISON).astype(slots.dtype)
        assert (slots[:, self.width:] == poison).all(), "a launch wrote behind a row of a wide tensor"
        return np.ascontiguousarray(slots[:, :self.width])

    def close(self):
        self.buffer = None
