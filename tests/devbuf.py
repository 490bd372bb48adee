"""Device buffers at a chosen address residue mod 16, with guard bands inside the same allocation.

A fresh torch allocation starts 512-byte aligned and is rounded up to 512 bytes, so a kernel that
reads a few bytes past an input, or writes past an output, stays correct by accident: the bytes it
meets are zero and nobody looks at them.  `place` puts a payload at `backing[front:front + len]`
with `view.data_ptr() % 16 == residue` and at least `guard` bytes of poison on both sides:

* inputs: poison that a kernel reducing mod 17 cannot mistake for zero.  "canon" is seeded random
  bytes in 1..16 (an over-read sees a plausible, wrong coefficient), "raw" is 0xA5 (12 mod 17, not
  canonical).  0xEE (14 x 17) and 0xFF (15 x 17) are 0 mod 17 and would be invisible there.
* outputs: 0xEE, as elsewhere in the suite (`place_out`); a store past the payload shows.

`unchanged(backing, snapshot)` compares the whole backing buffer -- guard bands and payload -- with
its state before the call.  GUARD is 64 bytes everywhere: a load that over-reads by up to 15 bytes
stays inside the allocation.
"""
import numpy as np
import torch

GUARD = 64
OUT_GUARD = 0xEE
RAW = 0xA5


def poison_bytes(kind, count, seed=0):
    """`count` input poison bytes, none of them 0 mod 17"""
    if kind == "canon":
        p = np.random.default_rng(0xD0B0F + seed).integers(1, 17, count).astype(np.uint8)
    elif kind == "raw":
        p = np.full(count, RAW, np.uint8)
    else:
        raise ValueError("input poison is 'canon' or 'raw', not %r" % (kind,))
    assert np.all(p % 17 != 0), "input poison must be visible to a kernel that reduces mod 17"
    return p


def _layout(length, residue, guard):
    assert 0 <= residue < 16 and guard >= 0
    front = (guard + 15) // 16 * 16 + residue       # the allocation itself is 16-byte aligned
    return front, front + length + guard


def _finish(host, front, length, residue, guard):
    backing = torch.from_numpy(host).to("cuda")
    assert backing.data_ptr() % 16 == 0
    view = backing[front:front + length]
    assert view.dtype == torch.uint8 and view.is_cuda
    if length:
        assert view.data_ptr() % 16 == residue, (view.data_ptr() % 16, residue)
    assert front >= guard and backing.numel() - (front + length) >= guard
    return backing, view


def place(array, residue, guard=GUARD, poison="canon", seed=0):
    """(backing, view): `array`'s bytes on the device at an address that is `residue` mod 16, with
    at least `guard` input-poison bytes in front of it and behind it in the same allocation"""
    data = np.ascontiguousarray(np.frombuffer(array, np.uint8) if isinstance(array, (bytes, bytearray)) else array,
                                dtype=np.uint8).reshape(-1)
    front, total = _layout(len(data), residue, guard)
    host = poison_bytes(poison, total, seed)
    host[front:front + len(data)] = data
    return _finish(host, front, len(data), residue, guard)


def place_out(length, residue, guard=GUARD, fill=OUT_GUARD):
    """(backing, view): an output of exactly `length` bytes at `residue` mod 16, the payload and
    the guard bands all `fill` (0xEE)"""
    front, total = _layout(length, residue, guard)
    return _finish(np.full(total, fill, np.uint8), front, length, residue, guard)


def snapshot(backing):
    return backing.clone()


def unchanged(backing, snap):
    """the whole backing buffer, guard bands and payload, is what `snap` recorded"""
    return backing.shape == snap.shape and bool(torch.equal(backing, snap))


def guards_intact(backing, view, fill=OUT_GUARD):
    """every byte of `backing` outside `view` still holds `fill`"""
    off = view.storage_offset() - backing.storage_offset()    # (an empty view has no address of its own)
    return bool((backing[:off] == fill).all()) and bool((backing[off + view.numel():] == fill).all())
