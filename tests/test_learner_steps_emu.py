"""CPU tier of the learner's call sequence: three steps of every configuration of tests/learner_step_cases.py through the SIMT
emulator (pendulum, n_grid 10, B = 4, fp64) -- the calls to the model library, the event_hook names and the reuse of the solver's
buffers, step by step, against the literal lists of that module."""
import pytest
import torch

import lfsd_amd  # noqa: F401
import learner_step_cases as C


@pytest.fixture(scope="module")
def pendulum(emu):
    return C.make_model("pendulum", emu, None, torch.float64)


@pytest.mark.parametrize("name", list(C.CASES))
def test_steps_make_the_pinned_calls(pendulum, name):
    C.run_case("pendulum", *pendulum, name)
