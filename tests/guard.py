"""Guard bands around tensors handed to the kernels (tests/test_gpu_memory_bounds.py).

guarded() places an array in the middle of ONE torch.uint8 allocation,

    [ front guard | payload | back guard ]

both guards filled with one byte value.  A kernel that stores outside the payload changes a guard
byte (assert_guards_intact reports where); a kernel that loads outside it reads the guards' fill
(guarded_like: run the call with two different fills around its inputs and compare the results).

Size rule: each guard is at least FOUR times the array's per-env byte size (the bytes of one
index of the leading dimension; `env_bytes` overrides it for flat buffers such as a workspace),
rounded up to 256 B, and at least 4 KiB -- one wavefront's worth of spare rows, the reach of the
"spare rows replay the last env" idiom of the four-envs-per-wavefront kernels.  A stray access
FURTHER away than a guard's length lands outside the guards, possibly outside the allocation, and
goes unseen: these helpers do not bound it.

The payload starts at a multiple of 256 B from the allocation's base (torch's allocators align
the base itself to at least 64 B on the host and 512 B on the device), so it is 16-byte aligned;
offset_bytes = 8 or 4 shifts it by that much into the front guard's slack, for the weakest
alignment an interface allows.  The payload never touches either end of its allocation: whatever
an overrun of up to a guard's length reaches lies inside the same allocation.
"""
from __future__ import annotations

import dataclasses
import math

import torch

GUARD_MIN = 4096
GUARD_ALIGN = 256
GUARD_ROWS = 4


@dataclasses.dataclass
class Guard:
    base: torch.Tensor      # the whole uint8 allocation
    start: int              # payload's first byte in base
    nbytes: int             # payload bytes
    fill: int


def guard_bytes(env_bytes: int) -> int:
    """Length of each guard for an array of `env_bytes` bytes per env (the rule above)."""
    g = -(-GUARD_ROWS * int(env_bytes) // GUARD_ALIGN) * GUARD_ALIGN
    return max(GUARD_MIN, g)


def guarded(shape, dtype, device, fill=0xA5, offset_bytes=0, env_bytes=None) -> torch.Tensor:
    """An uninitialised-looking (every byte = `fill`) contiguous tensor of `shape` / `dtype` on
    `device` between two guards of guard_bytes(env_bytes) bytes (front: + offset_bytes) holding
    `fill`.  env_bytes defaults to the bytes of one index of the leading dimension.  The returned
    tensor carries its allocation (attribute _guard): keep THIS tensor, not a view of it, for
    assert_guards_intact."""
    shape = (int(shape),) if isinstance(shape, int) else tuple(int(s) for s in shape)
    item = torch.empty((), dtype=dtype).element_size()
    nbytes = item * math.prod(shape)
    if env_bytes is None:
        env_bytes = item * math.prod(shape[1:])
    if not 0 <= fill <= 0xFF:
        raise ValueError("fill: one byte")
    if offset_bytes < 0 or offset_bytes >= GUARD_ALIGN or offset_bytes % item:
        raise ValueError("offset_bytes: a multiple of the element size below 256")
    g = guard_bytes(env_bytes)
    start = g + offset_bytes
    base = torch.full((start + nbytes + g,), fill, dtype=torch.uint8, device=device)
    t = base[start:start + nbytes].view(dtype).view(shape)
    assert t.is_contiguous() and t.data_ptr() == base.data_ptr() + start
    t._guard = Guard(base, start, nbytes, fill)
    return t


def guarded_like(src: torch.Tensor, pad_fill: int, offset_bytes=0, env_bytes=None) -> torch.Tensor:
    """A copy of `src` in a guarded payload whose guards hold `pad_fill` (inputs: what a load past
    the array's ends would read)."""
    t = guarded(src.shape, src.dtype, src.device, fill=pad_fill, offset_bytes=offset_bytes,
                env_bytes=env_bytes)
    t.copy_(src)
    return t


def guard_damage(t: torch.Tensor):
    """None when every guard byte of `t` (from guarded / guarded_like) still holds its fill, else
    (first, last): the byte offsets RELATIVE TO THE PAYLOAD'S FIRST BYTE of the first and the last
    changed guard byte -- negative in the front guard, >= the payload's bytes in the back guard."""
    g = getattr(t, "_guard", None)
    if g is None:
        raise TypeError("not a tensor from guarded(): no guard to check (a view of one?)")
    end = g.start + g.nbytes
    hits = []
    for lo, part in ((0, g.base[:g.start]), (end, g.base[end:])):
        idx = torch.nonzero(part != g.fill).flatten()
        if idx.numel():
            hits += [lo + int(idx[0]) - g.start, lo + int(idx[-1]) - g.start]
    return (min(hits), max(hits)) if hits else None


def assert_guards_intact(t: torch.Tensor, name: str = "tensor") -> None:
    dmg = guard_damage(t)
    if dmg is None:
        return
    g = t._guard
    row = g.nbytes // max(t.shape[0], 1) if t.dim() else g.nbytes
    where = lambda o: (f"{-o} B before the payload" if o < 0 else
                       f"{o - g.nbytes} B past the payload's end")
    raise AssertionError(
        f"{name}: guard bytes changed, payload-relative offsets {dmg[0]} .. {dmg[1]} "
        f"(first {where(dmg[0])}, last {where(dmg[1])}; payload {g.nbytes} B, "
        f"{row} B per leading index, shape {tuple(t.shape)})")
