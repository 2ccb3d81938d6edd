"""The harness of tests/test_gpu_workspace_contract.py can fail: tests/workspace_guard.py on the CPU, with torch writes where a
kernel's stray store would land.  No library call, no GPU."""
import numpy as np
import pytest

from tests.workspace_guard import BAND, BAND_BYTE, CANARY, GUARD, Guarded, WorkspaceGuard


def planted(n=1000, fill=0xFF, offset=0):
    g = WorkspaceGuard(n, fill=fill, offset=offset, device="cpu")
    g.snapshot()
    return g


def test_the_slice_has_exactly_n_bytes_between_two_bands():
    g = planted(1000, fill=0xFF)
    assert g.slice.numel() == 1000 and g.buf.numel() == 1000 + 2 * BAND and g.slice.dtype == g.buf.dtype
    assert bool((g.slice == 0xFF).all())
    assert bool((g.buf[:BAND] == BAND_BYTE).all()) and bool((g.buf[BAND + 1000:] == BAND_BYTE).all())
    assert g.slice.data_ptr() == g.buf.data_ptr() + BAND and g.slice.data_ptr() % 4096 == 0
    assert g.outside_changes() == []
    g.assert_outside_unchanged()
    assert bool((planted(7, fill=0x00).slice == 0).all())


@pytest.mark.parametrize("where,offset_from_slice", [("one byte before the slice", -1), ("one byte behind it", 1000),
                                                     ("the last byte of the far band", 1000 + BAND - 1),
                                                     ("the first byte of the near band", -BAND)])
def test_a_write_outside_the_slice_is_reported(where, offset_from_slice):
    g = planted(1000)
    g.buf[BAND + offset_from_slice] = 0x00
    assert g.outside_changes() == [offset_from_slice], where
    with pytest.raises(AssertionError, match="outside the slice"):
        g.assert_outside_unchanged(where)


def test_a_write_inside_the_slice_is_not_reported():
    g = planted(1000)
    g.slice.fill_(0x3C)
    g.slice[0], g.slice[999] = 1, 2
    g.assert_outside_unchanged()
    assert g.outside_changes() == []


def test_the_offset_slice_is_16_byte_and_not_32_byte_aligned():
    g = planted(1000, offset=16)
    p = g.slice.data_ptr()
    assert p % 16 == 0 and p % 32 != 0 and (p - 16) % 4096 == 0
    assert g.slice.numel() == 1000 and g.buf.numel() == 1000 + 2 * BAND
    g.buf[BAND - 1] = 0
    assert g.outside_changes() == [-1]


def test_a_shorter_slice_at_the_front_of_a_dirtied_workspace():
    """What the stale run does: a large call dirties its slice, a shorter slice is planted over its front without refilling, and
    everything behind the shorter slice -- the dirt included -- counts as outside."""
    g = planted(1000, fill=0xFF)
    g.slice[:] = 0x11                                                         # the large call
    front = g.replant(300)
    assert front.numel() == 300 and front.data_ptr() == g.buf.data_ptr() + BAND and bool((front == 0x11).all())
    with pytest.raises(AssertionError, match="snapshot"):
        g.outside_changes()
    g.snapshot()
    front.fill_(0x22)                                                         # the small call, inside its own slice
    g.assert_outside_unchanged()
    g.buf[BAND + 300] = 0x22                                                  # ... and one byte into the dirt behind it
    assert g.outside_changes() == [300]
    assert bool((g.replant(200, fill=0x00) == 0).all())


def test_guarded_canaries_go_false_on_a_planted_write():
    arrays = [np.arange(5, dtype=np.float32), np.zeros((3, 4), np.float32)]
    g = Guarded(arrays, device="cpu")
    assert g.buf.numel() == GUARD + 5 + GUARD + 12 + GUARD and g.canaries_intact()
    assert [v.numel() for v in g.views] == [5, 12] and g.ptrs()[1] - g.ptrs()[0] == 4 * (5 + GUARD)
    for v in g.views:
        v.fill_(3.0)                                                          # inside the tensors: not a canary
    assert g.canaries_intact()
    assert np.array_equal(g.host([(5,), (3, 4)])[1], np.full((3, 4), 3.0, np.float32))
    for at in (GUARD - 1, GUARD + 5, g.buf.numel() - 1):                      # in front of the first, behind it, the last canary
        h = Guarded(arrays, device="cpu")
        h.buf[at] = 0.0
        assert not h.canaries_intact(), at
    assert float(g.buf[0]) == CANARY
