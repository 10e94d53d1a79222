"""GPU tier of pair staging in the fp32 Riccati sweep (LFSD_RIC_PAIR_STAGE, csrc/cpdp_aux.h): the product library against the
variant library built with the switch off (lfsd_amd.runtime.build_variant_library), on the cases of tests/riccati_pair_cases.py:
Z_grid, stats, loss and gradient are torch.equal."""
import pytest
import torch

from conftest import build_variant_library
import riccati_pair_cases as C

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pair():
    ocs = []
    for variant in (False, True):
        oc, d = C.make_oc()
        if variant:
            oc.use_library(build_variant_library(oc, C.OFF_TAG, C.OFF_FLAGS))
        oc.compile()
        oc.setDevice("cuda:0", torch.float32)
        ocs.append(oc)
    inp = C.inputs(d, "cuda:0")
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
    print("Riccati units per row: aux_rtol=0", fixed1[1]["stats"][:, 0].tolist(), "aux_rtol=%g" % C.RTOL, b["stats"][:, 0].tolist(),
          "(emulator: %s, %s)" % (C.EMU_UNITS_FIXED1, C.EMU_UNITS_RTOL))
    C.assert_redone(fixed1[1], b)          # the one-unit build alone shows the redo
    C.assert_same(a, b, "aux_rtol=%g" % C.RTOL)
