"""GPU tier of the lock-step packing cases (tests/packing_cases.py): the gfx950 product libraries on cuda:0, every model in both
precisions on both mappings -- every slot of two full wavefronts and a one-row tail against the tight oracle at parity_cases'
tolerances, and a row's bits in any slot, with any partners, next to skipped rows and alone.  The same cases pass on the SIMT emulator
(tests/test_packing_emu.py: pendulum fp64, cart-pole fp32)."""
import pytest
import torch

import packing_cases as P

pytestmark = pytest.mark.gpu

DTYPES = [torch.float64, torch.float32]
DTYPE_IDS = ["fp64", "fp32"]


def prepare(oc, dtype):
    oc.setDevice("cuda:0", dtype)
    return oc


@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("kind", P.MODELS)
def test_every_slot_of_a_ragged_batch_vs_oracle(kind, dtype, oc_mapping):
    P.every_slot_vs_oracle(prepare, kind, dtype, oc_mapping)


@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("kind", P.MODELS + ("rocket",))
def test_a_row_is_bit_identical_in_any_slot_with_any_partners_and_alone(kind, dtype, oc_mapping):
    P.slot_and_partner_independence(prepare, "gpu", kind, dtype, oc_mapping)


@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("kind", P.MODELS)
def test_skipped_rows_are_nan_and_leave_their_partners_alone(kind, dtype, oc_mapping):
    P.skipped_rows(prepare, "gpu", kind, dtype, oc_mapping)


@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("kind", sorted(P.LIMIT_ROW))
def test_a_row_at_the_iteration_limit_leaves_its_partners_alone(kind, dtype, oc_mapping):
    P.row_at_iteration_limit(prepare, kind, dtype, oc_mapping)


@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("kind", P.MODELS)
def test_nothing_is_written_outside_the_batch(kind, dtype, oc_mapping):
    P.nothing_written_outside(prepare, "gpu", kind, dtype, oc_mapping)
