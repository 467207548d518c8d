"""The ten operators that take a gc_*_cfg struct against the bits the library gave while their configuration
was a double vector unpacked by position (tests/golden/cfg_parent.npz, recorded by
tests/golden/make_cfg_parent.py at commit 3b6486e). Every configuration field an operator reads has a value
there that no other field of its struct has, but for the coincidences a field's domain forces (the recorder's
docstring lists them), so a member read under another member's name changes the output. The inputs come from
the fixture, the calls go through the public Python API, and every output is compared byte for byte: all
ten repeated their own bytes when recorded twice, the OT association and the pipeline included."""

import numpy as np
import pytest

from tests.golden import make_cfg_parent as G

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gold():
    return np.load(G.OUT)


@pytest.mark.parametrize("name", list(G.OPS))
def test_configured_ops_are_bit_identical_with_parent(ctx, gold, name):
    got = G.OPS[name][1](ctx, G.inputs_of(gold, name))
    pre = f"out/{name}/"
    want = [k for k in gold.files if k.startswith(pre)]
    assert want and sorted(pre + k for k in got) == sorted(want)
    for k in want:
        assert G.same_bytes(got[k[len(pre):]], gold[k]), k
