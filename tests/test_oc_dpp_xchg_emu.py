"""CPU tier of the register exchanges in the lean fp32 OC kernel (LFSD_OC_DPP_XCHG, csrc/cpdp_common.h row_bcast, csrc/cpdp_oc.h
backward_sc / costate_sweep_sc): the emulator build of the product against the emulator build with the switch off, on the cases of
tests/oc_dpp_cases.py.  The emulator runs row_bcast through an exchange buffer indexed like the DPP row, so a wrong source lane
cannot stay equal; both builds start every kernel with NaN-filled LDS."""
import pytest
import torch

from conftest import build_emu_library
import oc_dpp_cases as C

_SOLS = {}


def _pair(case):
    """(product solution, switch-off solution) of a case, solved once per session."""
    if case not in _SOLS:
        g20 = _pair("grid20")[1] if case == "maxiter3" else None
        out = []
        for flags, tag in (((), ""), (C.OFF_FLAGS, C.OFF_TAG)):
            oc, d = C.make_oc(case)
            oc.use_library(build_emu_library(oc, flags, tag))
            oc.compile()
            oc.setDevice(dtype=torch.float32)
            out.append(C.solve(oc, d, case, "cpu", g20))
        _SOLS[case] = out
    return _SOLS[case]


@pytest.mark.parametrize("case", C.CASES)
def test_register_exchange_equal_to_lds_exchange(case):
    a, b = _pair(case)
    C.assert_case(case, a, b)
