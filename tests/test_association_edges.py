"""The association edge cases (assoc_cases.py) meet their own conditions, without a GPU: costs
separated (or tied exactly, in "ties" only), measurements off the cell boundaries, raw costs
capped, each named path reached, and the float64 oracle within 1/100 of every bar of
test_gpu_association_edges.py of a long-double restatement."""

import numpy as np
import pytest

import assoc_cases as AC


@pytest.mark.parametrize("name", list(AC.CASES))
def test_case_conditions(name):
    case = AC.build(name)
    m = AC.check_conditions(case)
    print(name, m)
    assert case["assoc"]["candidate_pool_indices"].shape == (case["N"], case["K"])
    assert case["view"]["valid_mask"].shape == (len(case["ids"]) * case["m_view"],)


def test_cases_reach_the_kernel_thresholds():
    """The shapes that select another path of the kernels."""
    c = {n: AC.build(n) for n in AC.CASES}

    def stencil(n):
        r, rz = c[n]["cfg"].get("r_xy", 1), c[n]["cfg"].get("r_z", 0)
        return (2 * rz + 1) * (3 * r * (r + 1) + 1)
    assert c["strided"]["N"] > 2 * 1024 and c["strided"]["N"] % 4 and 64 < stencil("strided") <= 128
    assert c["edge1025"]["N"] == 1025 and c["edge1025"]["K"] % 2 and c["edge1025"]["cfg"]["r_z"] > 0
    assert c["strided"]["K"] == c["longpool"]["K"] == c["full_view"]["K"] == 16
    assert stencil("longpool") * c["longpool"]["m_view"] == 64 * 112 and c["longpool"]["m_tile"] > 2048
    assert c["full_view"]["m_view"] == c["full_view"]["m_tile"]
    assert (c["lobes1"]["L"], c["lobes8"]["L"]) == (1, 8)
    assert (c["iters0"]["cfg"]["k_sinkhorn"], c["iters1"]["cfg"]["k_sinkhorn"]) == (0, 1)
    # no iteration: the plan is the kernel matrix itself (u = v = 1)
    a = c["iters0"]["assoc"]
    np.testing.assert_array_equal(a["row_masses"], np.exp(-a["cost_matrix"] / 0.1).sum(axis=1))
