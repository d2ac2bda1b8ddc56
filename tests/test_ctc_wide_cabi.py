"""CPU: the one-launch CTC prefix search for beams of 33 to 128 prefixes (csrc/ctc_search_wide.hip)
through the C ABI -- its two entry points validate their arguments and return early for an empty batch
before anything touches a GPU, and the workspace they ask for grows with the problem."""
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g

    from pydrobert_amd import _cabi

    if not os.path.exists(_cabi.LIB_PATH):
        g.build()
    return _cabi.lib()


def _search(lib, logits=1, T=5, N=2, V=40, lens=0, width=64, S=5, y=1, y_lens=1, y_probs=1, ws=1):
    """pdt_ctc_prefix_search_wide with made-up non-null pointers (never dereferenced: every call here
    returns before a launch)."""
    return lib.pdt_ctc_prefix_search_wide(logits, T, N, V, 1, 1, 1, lens, width, S, y, y_lens, y_probs, ws, 0)


def test_wide_search_validates_before_any_launch(lib):
    from pydrobert_amd import _cabi

    # an empty batch: nothing to do, whatever the pointers
    assert _search(lib, N=0) == _cabi.PDT_OK
    assert _search(lib, N=0, logits=0, y=0, y_lens=0, y_probs=0, ws=0) == _cabi.PDT_OK
    # null pointers with a non-empty batch
    for null in ("logits", "y", "y_lens", "y_probs", "ws"):
        assert _search(lib, **{null: 0}) == _cabi.PDT_E_ARG, null
    # sizes that make no sense
    assert _search(lib, width=0) == _cabi.PDT_E_ARG
    assert _search(lib, width=-3) == _cabi.PDT_E_ARG
    assert _search(lib, V=0) == _cabi.PDT_E_ARG
    assert _search(lib, T=-1) == _cabi.PDT_E_ARG
    assert _search(lib, N=-1) == _cabi.PDT_E_ARG
    assert _search(lib, S=-1) == _cabi.PDT_E_ARG
    # beyond what the kernel holds or its 32-bit indexes reach
    assert _search(lib, width=129) == _cabi.PDT_E_TOO_LONG
    assert _search(lib, width=128, V=(1 << 24)) == _cabi.PDT_E_TOO_LONG  # width * (V + 1) >= 2^31
    assert _search(lib, T=1 << 24) == _cabi.PDT_E_TOO_LONG
    # argument errors come first, as in pdt_ctc_prefix_search
    assert _search(lib, width=129, V=0) == _cabi.PDT_E_ARG
    # the narrow entry keeps its own limit
    assert lib.pdt_ctc_prefix_search(1, 5, 2, 40, 1, 1, 1, 0, 33, 5, 1, 1, 1, 1, 0) == _cabi.PDT_E_TOO_LONG


def test_wide_workspace_is_positive_and_monotone(lib):
    size = lib.pdt_ctc_prefix_search_wide_workspace_bytes
    base = size(50, 8, 300, 64)
    assert base >= 50 * 8 * 64 * 8  # the trie: one (parent, token) record per frame and entry
    for T, N, V, W in [(0, 1, 1, 1), (0, 0, 1, 33), (1, 1, 40, 33), (300, 1024, 1000, 128)]:
        assert size(T, N, V, W) > 0, (T, N, V, W)
    for lo, hi in zip([1, 9, 50, 300], [9, 50, 300, 1000]):
        assert size(lo, 8, 300, 64) < size(hi, 8, 300, 64)
        assert size(50, lo, 300, 64) < size(50, hi, 300, 64)
    widths = [1, 16, 32, 33, 64, 65, 100, 128]
    sizes = [size(50, 8, 300, w) for w in widths]
    assert sizes == sorted(sizes) and len(set(sizes)) == len(sizes)
    # the next-token tables move to the workspace beyond width 64: 2 * W * W words per utterance
    assert size(50, 8, 300, 65) - size(50, 8, 300, 64) >= 8 * 2 * 65 * 65 * 4
    # arguments the search does not take
    for T, N, V, W in [(-1, 8, 300, 64), (50, -1, 300, 64), (50, 8, 0, 64), (50, 8, 300, 0), (50, 8, 300, 129)]:
        assert size(T, N, V, W) == 0, (T, N, V, W)
