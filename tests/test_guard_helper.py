"""The guard-band helper (tests/guard.py) on CPU tensors: it catches a one-byte change at either
end of either guard, reports its offset, ignores the payload, and keeps its layout promises --
i.e. the GPU tests built on it (tests/test_gpu_memory_bounds.py) can fail."""
import pytest

torch = pytest.importorskip("torch")

from guard import (GUARD_MIN, assert_guards_intact, guard_bytes, guard_damage, guarded,
                   guarded_like)

CASES = [((5, 12), torch.float64, 0), ((5, 12), torch.float64, 8), ((5,), torch.int32, 4),
         ((5,), torch.int32, 0), ((3, 17, 6), torch.float64, 8), ((61, 331), torch.float64, 0)]


@pytest.mark.parametrize("shape,dtype,off", CASES)
def test_layout(shape, dtype, off):
    t = guarded(shape, dtype, "cpu", offset_bytes=off)
    g = t._guard
    assert tuple(t.shape) == shape and t.dtype == dtype and t.is_contiguous()
    assert g.nbytes == t.numel() * t.element_size()
    env = g.nbytes // shape[0]
    # payload: a multiple of 256 B (+ the offset asked for) from the allocation's base
    rel = t.data_ptr() - g.base.data_ptr()
    assert rel == g.start and rel % 256 == off
    # ... so with the allocator's own alignment it is 16-byte aligned, or exactly `off` short of it
    assert g.base.data_ptr() % 16 == 0 and t.data_ptr() % 16 == off
    # both guards: >= 4 env rows, >= 4 KiB, the nominal length a multiple of 256 B
    front, back = g.start, g.base.numel() - g.start - g.nbytes
    assert front - off == back == guard_bytes(env)
    assert back >= 4 * env and back >= GUARD_MIN and back % 256 == 0
    # every byte, payload included, starts as the fill
    assert (g.base == 0xA5).all()
    assert guard_damage(t) is None
    assert_guards_intact(t)


def test_guard_rule_values():
    assert guard_bytes(8) == 4096
    assert guard_bytes(1024) == 4096
    assert guard_bytes(1025) == 4352          # 4100 -> next multiple of 256
    assert guard_bytes(331 * 8) == 10752      # 10592 -> 42 * 256
    # a flat buffer (workspace): the caller names its per-env bytes
    t = guarded((100000,), torch.uint8, "cpu", env_bytes=7000)
    assert t._guard.start == guard_bytes(7000) == 28160


@pytest.mark.parametrize("shape,dtype,off", CASES[:4])
def test_planted_byte_is_caught_at_every_guard_edge(shape, dtype, off):
    t = guarded(shape, dtype, "cpu", offset_bytes=off, fill=0x5A)
    g = t._guard
    end, total = g.start + g.nbytes, g.base.numel()
    # (position in the allocation, offset relative to the payload's first byte)
    for pos in (0, g.start - 1, end, total - 1):
        assert guard_damage(t) is None
        old = int(g.base[pos])
        g.base[pos] = old ^ 0x01
        assert guard_damage(t) == (pos - g.start, pos - g.start)
        with pytest.raises(AssertionError) as ei:
            assert_guards_intact(t, "tau")
        msg = str(ei.value)
        assert msg.startswith("tau:") and f"offsets {pos - g.start} .. {pos - g.start}" in msg
        g.base[pos] = old
    # the byte just before the payload is offset -1, the one just past it offset nbytes
    g.base[g.start - 1] = 0
    g.base[end] = 0
    assert guard_damage(t) == (-1, g.nbytes)
    with pytest.raises(AssertionError, match=r"first 1 B before the payload, last 0 B past"):
        assert_guards_intact(t)


def test_first_and_last_of_several_changes():
    t = guarded((5, 12), torch.float64, "cpu")
    g = t._guard
    end = g.start + g.nbytes
    g.base[end + 96:end + 192] = 0           # one spare row of tau written past the end
    assert guard_damage(t) == (g.nbytes + 96, g.nbytes + 191)
    g.base[g.start - 40] = 1
    assert guard_damage(t) == (-40, g.nbytes + 191)


def test_payload_changes_are_silent():
    t = guarded((5, 12), torch.float64, "cpu")
    t.fill_(float("nan"))
    t[0, 0] = 1.0
    t[-1, -1] = -1.0
    assert_guards_intact(t)
    s = guarded((5,), torch.int32, "cpu", offset_bytes=4)
    s.fill_(-1)
    assert_guards_intact(s)


def test_fill_equal_to_written_value_is_the_documented_blind_spot():
    """A stray store of the fill byte itself cannot be seen: the GPU tests use fills (0xA5) no
    result consists of."""
    t = guarded((4,), torch.int32, "cpu")
    t._guard.base[0] = 0xA5
    assert guard_damage(t) is None


@pytest.mark.parametrize("pad", [0x00, 0xFF])
def test_guarded_like(pad):
    src = torch.arange(5 * 19, dtype=torch.float64).reshape(5, 19)
    t = guarded_like(src, pad, offset_bytes=8)
    assert torch.equal(t, src) and t.data_ptr() % 16 == 8
    g = t._guard
    assert (g.base[:g.start] == pad).all() and (g.base[g.start + g.nbytes:] == pad).all()
    assert_guards_intact(t)
    # 0xFF surroundings read as NaN doubles / -1 int32
    assert torch.isnan(g.base[:8].view(torch.float64)).all() or pad == 0


def test_misuse_is_refused():
    with pytest.raises(ValueError):
        guarded((4,), torch.float64, "cpu", offset_bytes=4)     # would misalign the elements
    with pytest.raises(ValueError):
        guarded((4,), torch.float64, "cpu", fill=256)
    t = guarded((4, 3), torch.float64, "cpu")
    with pytest.raises(TypeError):
        guard_damage(t[1:])                                       # a view has no guard record
