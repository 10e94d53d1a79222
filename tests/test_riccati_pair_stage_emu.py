"""CPU tier of pair staging in the fp32 Riccati sweep (LFSD_RIC_PAIR_STAGE, csrc/cpdp_aux.h): the emulator build of the product
against the emulator build with the switch off, on the cases of tests/riccati_pair_cases.py.  Both builds start every kernel with
NaN-filled LDS, so a unit that read a node slot no pass had staged could not stay equal."""
import pytest
import torch

from conftest import build_emu_library
import riccati_pair_cases as C


@pytest.fixture(scope="module")
def pair():
    """(oc bound to the product build, oc bound to the switch-off build, inputs, the aux_substeps=1 / aux_rtol=0 runs of both)."""
    ocs = []
    for flags, tag in (((), ""), (C.OFF_FLAGS, C.OFF_TAG)):
        oc, d = C.make_oc()
        oc.use_library(build_emu_library(oc, flags, tag))
        oc.compile()
        oc.setDevice(dtype=torch.float32)
        ocs.append(oc)
    inp = C.inputs(d, "cpu")
    fixed1 = [C.run(oc, inp, 1, 0.0) for oc in ocs]
    return ocs[0], ocs[1], inp, fixed1


@pytest.mark.parametrize("substeps", [1, 2, 3])
def test_fixed_units_equal_to_one_unit_staging(pair, substeps):
    on, off, inp, fixed1 = pair
    skip = C.SKIP_ROW if substeps == 3 else None
    a, b = (fixed1 if substeps == 1 else [C.run(oc, inp, substeps, 0.0, skip_row=skip) for oc in (on, off)])
    C.assert_same(a, b, "aux_substeps=%d" % substeps, skip_row=skip)
    rows = [r for r in range(C.BATCH) if r != skip]
    for o in (a, b):
        u = o["stats"][rows, 0].tolist()
        assert all(v >= substeps * C.N_GRID and v % substeps == 0 for v in u), u


def test_redone_intervals_equal_to_one_unit_staging(pair):
    on, off, inp, fixed1 = pair
    a, b = (C.run(oc, inp, 1, C.RTOL) for oc in (on, off))
    C.assert_redone(fixed1[1], b)          # the one-unit build alone shows the redo
    # ... with the unit totals recorded for these inputs (both builds: the stats are part of what must be equal)
    assert fixed1[1]["stats"][:, 0].tolist() == C.EMU_UNITS_FIXED1 and fixed1[0]["stats"][:, 0].tolist() == C.EMU_UNITS_FIXED1
    assert b["stats"][:, 0].tolist() == C.EMU_UNITS_RTOL and a["stats"][:, 0].tolist() == C.EMU_UNITS_RTOL
    C.assert_same(a, b, "aux_rtol=%g" % C.RTOL)
