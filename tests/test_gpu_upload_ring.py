"""gc_buffer_upload's pinned staging ring (8 segments of 512 KiB, gc_runtime.cpp stage_slot): uploads of at
most 512 KiB are copied into the ring and return before the device copy has run, so the caller may reuse
its source at once; a segment is reused only after the event recorded when it was left has completed.
Nothing else tests the wrap-around: about 13.8 MB of distinct seeded blocks (more than five laps of the
4 MiB ring; the 512 KiB block forces a segment change each cycle) whose sizes cycle over 1, 255, 256, 257
(the slot granularity is 256), 4,096, 100,000 and 524,288 bytes, every host source overwritten right after
its call, with 524,296-byte and 2 MiB uploads (the synchronous, unstaged path) interleaved; then one
download of everything, compared bit for bit."""

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SIZES = (1, 255, 256, 257, 4096, 100_000, 524_288)
CYCLES = 22
BIG = (524_296, 2 << 20)


def test_staged_uploads_survive_wraparound_and_source_reuse(ctx):
    from gcslam import _abi
    plan = []
    for c in range(CYCLES):
        plan += list(SIZES)
        if c % 5 == 2:
            plan.append(BIG[(c // 5) % 2])
    total = sum(plan)
    assert sum(s for s in plan if s <= 524_288) > 3 * 8 * 524_288 and set(BIG) <= set(plan)
    rng = np.random.default_rng(77)
    expect = rng.integers(0, 256, total, dtype=np.uint8)
    dev = _abi.DeviceArray(ctx, total, np.uint8)
    dev.zero()
    off = 0
    for s in plan:
        src = expect[off:off + s].copy()
        dev.view(s, off).upload(src)
        src[:] = ~src  # the call has returned: the source is the caller's again
        off += s
    got = dev.download()
    bad = np.nonzero(got != expect)[0]
    assert bad.size == 0, f"{bad.size} bytes differ, first at {bad[0]} of {total}"
    # and the ring still serves after the laps: a second pass over the same buffer in reverse block order
    expect2 = rng.integers(0, 256, total, dtype=np.uint8)
    offs = np.concatenate([[0], np.cumsum(plan)])
    for k in reversed(range(len(plan))):
        src = expect2[offs[k]:offs[k + 1]].copy()
        dev.view(plan[k], int(offs[k])).upload(src)
        src[:] = 0
    assert np.array_equal(dev.download(), expect2)
    dev.free()
