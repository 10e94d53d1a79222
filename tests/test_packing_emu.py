"""CPU tier of the lock-step packing cases (tests/packing_cases.py): the kernels through the SIMT emulator, pendulum in fp64 (8-lane
groups, 17 rows) and the cart-pole in fp32 (16-lane groups, 9 rows).  The emulator runs every lane as a fiber: the robot arm takes a
minute per solve on it and the quadrotor is covered there by the tests that already run it; the -m gpu tier
(tests/test_packing_gpu.py) runs every model in both precisions."""
import pytest
import torch

import packing_cases as P

CASES = [("pendulum", torch.float64), ("cartpole", torch.float32)]
IDS = ["pendulum-fp64", "cartpole-fp32"]
SUBSTEPS = 4          # of the identity tests (packing_cases.make); the oracle comparison runs at 16


@pytest.fixture
def prepare(emu):
    def bind(oc, dtype):
        emu(oc)
        oc.setDevice(dtype=dtype)
        return oc
    return bind


@pytest.mark.parametrize("kind,dtype", CASES, ids=IDS)
def test_every_slot_of_a_ragged_batch_vs_oracle(prepare, kind, dtype, oc_mapping):
    P.every_slot_vs_oracle(prepare, kind, dtype, oc_mapping)


@pytest.mark.parametrize("kind,dtype", CASES, ids=IDS)
def test_a_row_is_bit_identical_in_any_slot_with_any_partners_and_alone(prepare, kind, dtype, oc_mapping):
    P.slot_and_partner_independence(prepare, "emu", kind, dtype, oc_mapping, substeps=SUBSTEPS)


@pytest.mark.parametrize("kind,dtype", CASES, ids=IDS)
def test_skipped_rows_are_nan_and_leave_their_partners_alone(prepare, kind, dtype, oc_mapping):
    P.skipped_rows(prepare, "emu", kind, dtype, oc_mapping, merged=True, substeps=SUBSTEPS)


@pytest.mark.parametrize("kind,dtype", CASES[:1], ids=IDS[:1])
def test_a_row_at_the_iteration_limit_leaves_its_partners_alone(prepare, kind, dtype, oc_mapping):
    P.row_at_iteration_limit(prepare, kind, dtype, oc_mapping, substeps=SUBSTEPS)


@pytest.mark.parametrize("kind,dtype", CASES, ids=IDS)
def test_nothing_is_written_outside_the_batch(prepare, kind, dtype, oc_mapping):
    P.nothing_written_outside(prepare, "emu", kind, dtype, oc_mapping, substeps=SUBSTEPS)
