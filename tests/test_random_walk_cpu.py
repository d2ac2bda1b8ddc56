"""CPU: the random-walk entry points of the C ABI (csrc/random_walk.hip) and their operators, without a GPU:
exports, argument validation before any launch, registration, scripting, and the CPU walk."""
import os

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("pdt_random_walk_advance", "pdt_random_walk_step", "pdt_random_walk_table")


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g

    from pydrobert_amd import _cabi

    if not os.path.exists(_cabi.LIB_PATH):
        g.build()
    return _cabi.lib()


def test_symbols_exported_and_declared(lib):
    from pydrobert_amd import _cabi

    header = open(os.path.join(ROOT, "include", "pdt_amd.h")).read()
    for name in NAMES:
        assert hasattr(lib, name) and name in _cabi.SIGNATURES and name + "(" in header


def test_abi_version_is_14(lib):
    from pydrobert_amd import _cabi

    assert _cabi.ABI_VERSION == 14 and lib.pdt_amd_abi_version() == 14


def test_empty_batches_and_bad_arguments_without_gpu(lib):
    from pydrobert_amd import _cabi

    OK, ARG = _cabi.PDT_OK, _cabi.PDT_E_ARG
    # advance: (lpt, sn, sv, N, V, u, u_sn, lpp, lp_sn, y_prev, S, ss, sn, lens, le_sn, y_next, lp_next, ctl, host, stream)
    assert lib.pdt_random_walk_advance(0, 5, 1, 0, 5, 0, 1, 0, 1, 0, 3, 1, 1, 0, 1, 0, 0, 0, 0, 0) == OK
    assert lib.pdt_random_walk_advance(0, 5, 1, 4, 5, 0, 1, 0, 1, 0, 3, 1, 1, 0, 1, 0, 0, 0, 0, 0) == ARG
    assert lib.pdt_random_walk_advance(0, 5, 1, 0, 0, 0, 1, 0, 1, 0, 3, 1, 1, 0, 1, 0, 0, 0, 0, 0) == ARG  # V < 1
    assert lib.pdt_random_walk_advance(0, 5, 1, -1, 5, 0, 1, 0, 1, 0, 3, 1, 1, 0, 1, 0, 0, 0, 0, 0) == ARG
    # step: (scores, sn, sv, N, V, u, has_eos, eos, y_t, lens, ended, lp, ctl, host, stream)
    assert lib.pdt_random_walk_step(0, 5, 1, 0, 5, 0, 1, 2, 0, 0, 0, 0, 0, 0, 0) == OK
    assert lib.pdt_random_walk_step(0, 5, 1, 4, 5, 0, 1, 2, 0, 0, 0, 0, 0, 0, 0) == ARG
    assert lib.pdt_random_walk_step(0, 5, 1, 0, -2, 0, 1, 2, 0, 0, 0, 0, 0, 0, 0) == ARG
    # table: (table, sr, R, U, V, stats, u, N, C, has_eos, eos, y, ctx, lens, ended, lp, ctl, host, stream)
    assert lib.pdt_random_walk_table(0, 5, 6, 6, 5, 0, 0, 0, 4, 1, 2, 0, 0, 0, 0, 0, 0, 0, 0) == OK
    assert lib.pdt_random_walk_table(0, 5, 6, 6, 5, 0, 0, 3, 0, 1, 2, 0, 0, 0, 0, 0, 0, 0, 0) == OK  # C == 0
    assert lib.pdt_random_walk_table(0, 5, 6, 6, 5, 0, 0, 3, 4, 1, 2, 0, 0, 0, 0, 0, 0, 0, 0) == ARG
    assert lib.pdt_random_walk_table(0, 4, 6, 6, 5, 0, 0, 0, 4, 1, 2, 0, 0, 0, 0, 0, 0, 0, 0) == ARG  # row stride < V
    assert lib.pdt_random_walk_table(0, 5, 0, 6, 5, 0, 0, 0, 4, 1, 2, 0, 0, 0, 0, 0, 0, 0, 0) == ARG  # no rows


def test_operators_registered_and_switch_listed(lib):
    import pydrobert_amd  # noqa: F401
    from pydrobert_amd import switches

    assert hasattr(torch.ops.pydrobert_amd, "random_walk_advance")
    assert hasattr(torch.ops.pydrobert_amd, "random_walk_step")
    assert "PDT_WALK_TABLE" in switches.names() and switches.get("PDT_WALK_TABLE") == 1


def test_random_walk_scripts_and_runs_on_cpu():
    from pydrobert_amd import functional as F
    from pydrobert_amd import modules as M

    from _toy_lm import ScriptableBigramLM

    lm = ScriptableBigramLM(torch.randn(6, 5).log_softmax(-1))
    walk = M.RandomWalk(lm, eos=0)
    assert walk.default_hook
    scripted = torch.jit.script(walk)
    torch.manual_seed(3)
    y, lens, lp = walk(None, 7, 9)
    assert y.shape[1] == 7 and y.size(0) <= 9 and lens.shape == lp.shape == (7,)
    torch.manual_seed(3)
    for a, b in zip((y, lens, lp), scripted(None, 7, 9)):
        assert torch.equal(a, b)
    y, lp = F.random_walk_advance(torch.zeros(4, 3).log_softmax(-1), torch.zeros(4), torch.zeros((0, 4), dtype=torch.long))
    assert y.shape == (1, 4) and lp.shape == (4,)

    class Hooked(M.RandomWalk):
        def update_log_probs_for_step(self, log_probs_prev, log_probs_t, y_prev, y_prev_lens, eos_mask):
            return log_probs_prev, log_probs_t

    assert not Hooked(lm, eos=0).default_hook
