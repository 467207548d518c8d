"""Scans the reference handles but a kernel may not, through the batched pipeline against the oracle
(test_gpu_configs._run_and_compare, every bar of the C3 test, the recorder raising): the node's first
scan on an empty map (Matrix-Fisher H = 0, R_mf = I, every map-side clamp active, L_trans near ε), all
weights zero (48 empty bins) on a warm and on an empty map, the weights of one half-space zero, every
point on a plane, every point on two corridor walls (oracle/cases.DEGENERATE). H = 3, 4,096 points, three
scans with the IMU/odom branch computed and the map / IW feedback, every hypothesis sampled.

tests/test_degenerate_cases.py shows on the CPU that the oracle itself is well-posed on each case (a 1-ulp
change of the points moves nothing by more than a tenth of its bar, T included), so no field is dropped
or loosened here. A single ray, and a plane on an empty map, are ill-posed in the reference itself and
are left out."""

import pytest

from oracle import cases
from test_gpu_configs import _pipeline, _run_and_compare

pytestmark = pytest.mark.gpu

H, N_AZ, N_SCANS = 3, 256, 3


def _case(name):
    case = cases.build(H=H, n_az=N_AZ, n_scans=N_SCANS, io="computed", **cases.DEGENERATE[name])
    assert case["n"] == 4096
    return case


@pytest.mark.parametrize("name", list(cases.DEGENERATE))
def test_degenerate_scans_match_oracle(ctx, name):
    case = _case(name)
    _run_and_compare(ctx, case, H, case["n"], list(range(H)), N_SCANS, True).close()


def test_first_scan_on_empty_map_with_inscan_certs(ctx):
    """The empty-map case with the in-scan ConditioningCerts on (gc_certs.hip: the predict / fusion
    certificates and every projection's cert_vec computed inside the scan)."""
    case = _case("empty_map")
    pipe = _pipeline(case, ctx, H, case["n"], True)
    pipe.set_inscan_certs(True)
    _run_and_compare(ctx, case, H, case["n"], list(range(H)), N_SCANS, True, pipe=pipe)
    pipe.close()
