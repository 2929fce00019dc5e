"""tests/guarded.py itself, on CPU tensors: the carving is disjoint and aligned, fills land in the interior only, and a
byte planted in either guard is reported with the buffer's name and its offset."""
import numpy as np
import pytest
import torch

import guarded
from guarded import FILLS, GUARD, Arena, GuardError, guard_byte


def test_guards_are_64_kib_and_the_three_fills_are_the_documented_values():
    assert GUARD == 64 * 1024
    assert FILLS == (0x00, 0xFF, 0xA5)               # the zero fill first: the arrangement the suite already runs
    for fill in range(256):
        assert guard_byte(fill) != fill
    a = Arena("cpu")
    assert np.isnan(a.buf(8, 0xFF).numpy(np.float32)).all() and np.isnan(a.buf(8, 0xFF).numpy(np.float64)).all()
    assert (a.buf(8, 0xFF).numpy(np.int32) == -1).all() and (a.buf(8, 0xFF).numpy(np.int64) == -1).all()
    x = a.buf(8, 0xA5).numpy(np.float32)
    assert (x < 0).all() and (np.abs(x) < 1e-15).all() and a.buf(8, 0xA5).numpy(np.int64)[0] < -(1 << 62)
    assert not a.buf(8, 0x00).numpy(np.uint8).any()


@pytest.mark.parametrize("fill", FILLS, ids=guarded.fill_id)
@pytest.mark.parametrize("nbytes", [0, 1, 255, 256, 257, 4096, 100001])
def test_carving_is_aligned_disjoint_and_filled_only_inside(nbytes, fill):
    a = Arena("cpu")
    bufs = [a.buf(nbytes, fill, name="first"), a.buf(nbytes + 3, fill, align=512, name="second")]
    spans = []
    for b in bufs:
        assert b.data_ptr() % b.align == 0
        assert b.start >= GUARD and b.whole.numel() - b.end >= GUARD          # a whole guard on either side
        assert b.t.numel() == b.nbytes and (b.nbytes == 0 or b.t.data_ptr() == b.data_ptr())
        whole = b.whole.numpy()
        assert (whole[:b.start] == guard_byte(fill)).all() and (whole[b.end:] == guard_byte(fill)).all()
        assert (whole[b.start:b.end] == fill).all()
        spans.append((b.whole.data_ptr(), b.whole.data_ptr() + b.whole.numel()))
    assert spans[0][1] <= spans[1][0] or spans[1][1] <= spans[0][0]           # tensors of their own
    a.check()


@pytest.mark.parametrize("fill", FILLS, ids=guarded.fill_id)
@pytest.mark.parametrize("skew", [0, 2, 4, 8, 16, 254, 255])
def test_a_skewed_interior_starts_that_far_past_the_alignment_with_whole_guards(skew, fill):
    """skew bytes past a multiple of `align` and not a byte better than the skew says; fills, guards and the damage report
    are those of an aligned buffer"""
    a = Arena("cpu")
    x = np.arange(101, dtype=np.uint16)
    bufs = [a.buf(1001, fill, name="skewed", skew=skew), a.buf(64, fill, align=512, name="wide", skew=skew),
            a.const(x, name="x", skew=skew)]
    for b in bufs:
        assert b.skew == skew and b.data_ptr() % b.align == skew
        if skew:       # aligned to the skew's own lowest set bit, to nothing above it
            assert b.data_ptr() % (2 * (skew & -skew)) != 0
        assert b.start >= GUARD and b.whole.numel() - b.end >= GUARD
        assert b.t.numel() == b.nbytes and b.t.data_ptr() == b.data_ptr() == b.ptr.value
        whole = b.whole.numpy()
        assert (whole[:b.start] == guard_byte(b.fill)).all() and (whole[b.end:] == guard_byte(b.fill)).all()
    assert (bufs[0].whole.numpy()[bufs[0].start:bufs[0].end] == fill).all()
    assert np.array_equal(bufs[2].numpy(np.uint16), x)
    a.check()
    bufs[0].whole[bufs[0].start - 1] = 0x11
    assert bufs[0].guard_damage() == ("front", -1)
    bufs[2].whole[bufs[2].start + 3] ^= 1
    with pytest.raises(GuardError) as e:
        a.check_consts()
    assert "'x'" in str(e.value) and "byte 3" in str(e.value)
    with pytest.raises(AssertionError):
        a.buf(8, fill, align=16, skew=16)                                     # a skew is less than the alignment


def test_placement_states_the_skews_by_name_for_arenas_built_inside_it():
    table = {"planes": 2, "params": 16}
    with guarded.placement(lambda name: table.get(name, 0)):
        a = Arena("cpu")
        assert a.buf(10, 0x00, name="planes").data_ptr() % 256 == 2
        assert a.const(np.zeros(3, np.float32), name="params").data_ptr() % 256 == 16
        assert a.buf(10, 0x00, name="workspace").data_ptr() % 256 == 0
        assert a.buf(10, 0x00, name="planes", skew=0).data_ptr() % 256 == 0      # an explicit skew wins
        with guarded.placement(None):
            assert Arena("cpu").buf(10, 0x00, name="planes").data_ptr() % 256 == 0
        assert Arena("cpu").buf(10, 0x00, name="planes").data_ptr() % 256 == 2
    assert Arena("cpu").buf(10, 0x00, name="planes").data_ptr() % 256 == 0        # and nothing stays behind
    assert a.buf(10, 0x00, name="planes").data_ptr() % 256 == 2                   # an Arena keeps the placement it was built under
    a.check()


def test_typed_views_share_the_interior():
    a = Arena("cpu")
    b = a.buf(64, 0x00, name="typed")
    b.as_f32()[3] = 1.5
    b.as_i64()[7] = -2
    b.as_u16(4)[0] = 7
    assert b.as_f32().numel() == 16 and b.as_f64().numel() == 8 and b.as_i32().numel() == 16 and b.as_i16().numel() == 32
    assert b.numpy(np.float32)[3] == 1.5 and b.numpy(np.int64)[7] == -2 and b.numpy(np.uint16, 1)[0] == 7
    assert b.ptr.value == b.data_ptr() == b.as_u8().data_ptr()
    with pytest.raises(AssertionError):
        b.as_f32(17)
    a.check_guards()                                                          # writes through the views stayed inside


@pytest.mark.parametrize("side,where", [("front", -1), ("front", -GUARD), ("back", 0), ("back", GUARD - 1), ("front", -300)])
def test_a_planted_byte_is_reported_with_name_and_offset(side, where):
    a = Arena("cpu")
    a.buf(1000, 0xA5, name="innocent")
    b = a.buf(777, 0xFF, name="victim")
    a.check_guards()
    at = b.start + where if side == "front" else b.end + where
    b.whole[at] = 0x11
    want = where if side == "front" else 777 + where
    assert b.guard_damage() == (side, want)
    with pytest.raises(GuardError) as e:
        a.check_guards()
    msg = str(e.value)
    assert "'victim'" in msg and side in msg and f"offset {want} " in msg and "innocent" not in msg
    # the FIRST touched offset is the one named
    if side == "back":
        b.whole[b.end + GUARD - 1] = 0x22
        assert b.guard_damage() == (side, want)


def test_a_write_of_the_fill_value_into_a_guard_is_still_seen():
    """the guards never hold the interior's fill: a kernel that runs past the end storing what it found inside shows"""
    for fill in FILLS:
        a = Arena("cpu")
        b = a.buf(512, fill, name="ws")
        b.whole[b.end] = fill
        with pytest.raises(GuardError):
            a.check_guards()


def test_const_inputs_are_compared_bit_for_bit():
    a = Arena("cpu")
    x = np.arange(37, dtype=np.float32)
    c = a.const(x, name="x")
    assert np.array_equal(c.numpy(np.float32), x)
    a.check()
    c.as_f32()[5] = -0.0 + 5.0                                                # the same value: no change
    a.check_consts()
    c.as_u8()[21] ^= 1
    with pytest.raises(GuardError) as e:
        a.check_consts()
    assert "'x'" in str(e.value) and "byte 21" in str(e.value)
