"""GPU tier of the learner's call sequence: three steps of every configuration of tests/learner_step_cases.py on the gfx950
libraries in fp32 -- pendulum n_grid 10 and quadrotor n_grid 6 (32-lane groups, the other lock-step packing), B = 4.  The same
pendulum lists pass on the SIMT emulator in fp64 (tests/test_learner_steps_emu.py)."""
import pytest
import torch

import lfsd_amd  # noqa: F401
import learner_step_cases as C

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", params=["pendulum", "quadrotor"])
def model(request):
    return (request.param,) + C.make_model(request.param, lambda oc: None, "cuda:0", torch.float32)


@pytest.mark.parametrize("name", list(C.CASES))
def test_steps_make_the_pinned_calls_on_the_device(model, name):
    C.run_case(*model, name)
