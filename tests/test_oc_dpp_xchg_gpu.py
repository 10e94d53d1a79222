"""GPU tier of the register exchanges in the lean fp32 OC kernel (LFSD_OC_DPP_XCHG, csrc/cpdp_common.h row_bcast, csrc/cpdp_oc.h
backward_sc / costate_sweep_sc): the product library against the variant library built with the switch off
(lfsd_amd.runtime.build_variant_library), on the cases of tests/oc_dpp_cases.py: state, control and costate grids, cost, iteration
counts and status are torch.equal -- and so are the loss and the gradient the auxiliary sweeps make of them."""
import pytest
import torch

from conftest import build_variant_library
import oc_dpp_cases as C

pytestmark = pytest.mark.gpu

_SOLS = {}


def _pair(case):
    """(product oc, d, product solution, switch-off solution) of a case, solved once per session."""
    if case not in _SOLS:
        g20 = _pair("grid20")[3] if case == "maxiter3" else None
        ocs, out = [], []
        for variant in (False, True):
            oc, d = C.make_oc(case)
            if variant:
                oc.use_library(build_variant_library(oc, C.OFF_TAG, C.OFF_FLAGS))
            oc.compile()
            oc.setDevice("cuda:0", torch.float32)
            ocs.append(oc)
            out.append(C.solve(oc, d, case, "cuda:0", g20))
        _SOLS[case] = (ocs[0], d, out[0], out[1])
    return _SOLS[case]


@pytest.mark.parametrize("case", C.CASES)
def test_register_exchange_equal_to_lds_exchange(case):
    _, _, a, b = _pair(case)
    print(case, "status", a["status"].tolist(), "iters", a["iters"].tolist())
    C.assert_case(case, a, b)


def test_auxiliary_sweeps_see_no_difference():
    oc, d, a, b = _pair("grid20")
    aux = [oc.auxSysSolverBatch(s, d["taus"], d["waypoints"], d["interface"]) for s in (a, b)]
    for k in ("loss", "grad"):
        assert torch.equal(aux[0][k], aux[1][k]), k
        assert bool(torch.isfinite(aux[0][k]).all()), k
