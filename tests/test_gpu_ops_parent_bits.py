"""The operators outside the hot path — visual pose evidence, surfels, camera splats, the OT association,
the map maintenance operators and the map update — against the bits the library gave before their
fixed-order sums moved into csrc/gc_blocksum.h and their scratch layouts onto the carver of gc_internal.h
(tests/golden/ops_parent.npz, recorded by tests/golden/make_ops_parent.py at commit f0d485b). The shared
helpers add the same values in the same association, so every output is the recorded array, bit for bit.

The cases are the smallest at which each shared piece can still go wrong: more collapse workgroups than
the second pass has chains (vpe multi_wg, surfel wide_centre), more Sinkhorn rows than threads with fewer
columns than compiled, three reduction workgroups on a map tile. None of these grids follows the
compute-unit count, so there is no skip condition."""

import numpy as np
import pytest

from tests.golden import make_ops_parent as G

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gold():
    return np.load(G.OUT)


@pytest.mark.parametrize("group", list(G.GROUPS))
def test_ops_are_bit_identical_with_parent(ctx, gold, group):
    got = G.GROUPS[group](ctx)
    want = [k for k in gold.files if k.startswith(group + "/")]
    assert want and sorted(got) == sorted(want)
    for k in want:
        assert got[k].dtype == gold[k].dtype and np.array_equal(got[k], gold[k]), k
