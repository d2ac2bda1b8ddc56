"""lm_lookup_kernel (csrc/lm_lookup.hip) at every form it takes, to the bit: the cases of
tests/_lookup_forms.py (asserted on the CPU by tests/test_lookup_forms_cpu.py) scored at every position --
as an int, a one-element tensor, per row and all at once -- against oracle.trie_log_probs with no tolerance,
through the forward index and without it, against the float64 brute force within the derived bound, and in
every layout of the history.

What the cases reach (from reading the kernel):
  * the 128-thread stride over the vocabulary and its groups of four loads: V = 128 | 129 | 512 | 513 | 641;
  * the successor pass: a context token with more than 128 (and more than 256) listed successors, tokens
    with none, contexts outside the vocabulary (no pass at all), successors that END in an out-of-vocabulary
    sos (id V: skipped, or they would land in column 0 of the next row);
  * the path without the forward index (empty succ_* tensors), equal to the indexed one;
  * find_child over 1, 200 and 299 children: first, last, inner, absent, below and above every label;
  * orders 2, 3, 4 (a sparse middle level: bo[3] decides) and 16 (the arrays' last slots); 17 is refused;
  * history tokens that are negative, V, V + 1, 2**40 and sos itself, positions padded with sos;
  * placeholder nodes at every level but the last;
  * ids of uint8 | int16 | int32 with n-grams on the top token ids."""
import copy
import functools

import numpy as np
import pytest
import torch

import _lookup_forms as forms
from pydrobert_amd import modules as M

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _model(name, device):
    return copy.deepcopy(forms.case_data(name).lm).to(device)


def _hist(name, device):
    return torch.from_numpy(forms.case_data(name).case[4]).to(device)


def _exact(act, exp, name, what):
    """Bit equality with the walk; names the case, the position and the first differing (row, v) pairs --
    and, for edges_o3, which differing rows follow a column ending in the hot token or in a c with a
    (c, sos) bigram: where a missing `v >= V` guard of the successor pass lands."""
    act = act.cpu().numpy()
    if np.array_equal(act, exp, equal_nan=True):
        return
    pairs = forms.mismatches(act.reshape(-1, act.shape[-1]), exp.reshape(-1, exp.shape[-1]))
    msg = "{} {}: differs from the walk at (row, v) {}".format(name, what, pairs)
    if name == "edges_o3" and act.shape == exp.shape:
        m, B = forms.marks(name), forms.case_data(name).case[4].shape[1]
        after = set((m["hot"] + 1).tolist()) | set((m["sos_pred"] + 1).tolist())
        rows = np.flatnonzero((act.reshape(-1, act.shape[-1]) != exp.reshape(-1, exp.shape[-1])).any(1))
        msg += "; rows after a hot / (c, sos) column among them: {}".format([int(r) for r in rows if r % B in after][:5])
    raise AssertionError(msg)


def _mixed_idx(S, B):
    return (np.arange(B) + 1) % (S + 1)  # (every position, neighbours at different ones)


@pytest.mark.parametrize("name", forms.NAMES)
def test_every_position_matches_the_walk_exactly(name, device):
    data, lm, hist = forms.case_data(name), _model(name, device), _hist(name, device)
    S, B = hist.shape
    assert data.case[5] == tuple(range(S + 1))
    for pos in data.case[5]:
        _exact(lm(hist, None, pos)[0], data.walk[pos], name, "position {} (int)".format(pos))
        one = torch.tensor([pos], device=device)
        _exact(lm(hist, None, one)[0], data.walk[pos], name, "position {} (one-element tensor)".format(pos))
    mixed = _mixed_idx(S, B)
    assert set(mixed.tolist()) == set(range(S + 1)) or B <= S
    exp = np.stack([data.walk[int(p)][b] for b, p in enumerate(mixed)])
    _exact(lm(hist, None, torch.from_numpy(mixed).to(device))[0], exp, name, "positions per row")
    full = lm(hist)
    assert full.shape == (S + 1, B, data.case[0])
    _exact(full, np.stack([data.walk[p] for p in range(S + 1)]), name, "every position (row = pos * B + b)")
    # no history at all: every row the all-sos context
    _exact(lm(hist[:0]), data.walk[0][None], name, "S = 0")
    _exact(lm(hist[:0], None, 0)[0], data.walk[0], name, "S = 0, position 0")


@pytest.mark.parametrize("name", forms.NAMES)
def test_with_and_without_the_forward_index(name, device):
    data, lm, hist = forms.case_data(name), _model(name, device), _hist(name, device)
    V, sos, order = data.case[:3]
    S, B = hist.shape
    assert lm.succ_start.numel() == V + lm.shift + 2  # (`have_index` of the op: the first call is indexed)
    none = torch.empty(0, dtype=torch.int32, device=device)
    assert none.numel() != V + lm.shift + 2
    op = torch.ops.pydrobert_amd.lookup_lm_log_probs
    tables = (lm.logps, lm.logbs, lm.child_start, lm.ids_wide)
    mixed = _mixed_idx(S, B)
    for what, idx in (("full", None), ("per row", torch.from_numpy(mixed).to(device)), ("last", torch.tensor(S, device=device))):
        indexed = op(hist, idx, *tables, lm.succ_start, lm.succ_tok, lm.succ_node, V, order, sos)
        plain = op(hist, idx, *tables, none, none, none, V, order, sos)
        assert torch.equal(indexed, plain), (name, what, forms.mismatches(indexed.cpu().numpy(), plain.cpu().numpy()))
    exp = np.concatenate([data.walk[p] for p in range(S + 1)])
    _exact(op(hist, None, *tables, none, none, none, V, order, sos), exp, name, "every position, no forward index")


@pytest.mark.parametrize("name", forms.NAMES)
def test_against_the_brute_force_within_the_derived_bound(name, device):
    data, lm, hist = forms.case_data(name), _model(name, device), _hist(name, device)
    act = lm(hist).cpu().numpy()
    for pos in data.case[5]:
        brute, bound = data.brute[pos], data.bound[pos]
        fin = np.isfinite(brute)
        assert np.array_equal(np.isfinite(act[pos]), fin) and not np.isnan(act[pos]).any(), (name, pos)
        diff = np.abs(act[pos][fin].astype(np.float64) - brute[fin])
        over = diff > bound[fin]
        assert not over.any(), (name, pos, float(diff[over].max()), np.argwhere(fin)[over][:5].tolist())


@pytest.mark.parametrize("name", forms.NAMES)
def test_history_layouts_give_the_same_bits(name, device):
    data, lm, hist = forms.case_data(name), _model(name, device), _hist(name, device)
    S, B = hist.shape
    full = lm(hist)
    assert hist.is_contiguous()
    turned = hist.t().contiguous().t()
    assert not turned.is_contiguous() or B == 1
    assert torch.equal(lm(turned), full)
    # int32 histories (2**40 has no int32: the largest one stands in for it, outside every vocabulary too)
    narrow = hist.clamp(max=2**31 - 1)
    assert torch.equal(lm(narrow.int()), lm(narrow)) and torch.equal(lm(narrow), full)
    assert torch.equal(lm(narrow.int(), None, S)[0], full[S])
    # full mode is the stack of the scalar positions
    assert torch.equal(torch.stack([lm(hist, None, p)[0] for p in range(S + 1)]), full)
    # one column (a view with the batch's stride) and a per-row idx of one entry
    for b in sorted({0, B // 2, B - 1}):
        for pos in (0, S // 2, S):
            got = lm(hist[:, b : b + 1], None, torch.tensor([pos], device=device))[0]
            _exact(got, data.walk[pos][b : b + 1], name, "column {} alone, position {}".format(b, pos))
    mixed = torch.from_numpy(_mixed_idx(S, B)).to(device)
    assert torch.equal(lm(turned, None, mixed)[0], lm(hist, None, mixed)[0])
    assert torch.equal(lm(hist, None, mixed - (S + 1))[0], lm(hist, None, mixed)[0])  # (from the end)


def test_rows_stay_in_their_rows(device):
    """A listed successor that ends in the out-of-vocabulary sos has id V: written, it would be column 0 of
    the NEXT row.  The rows after every column ending in the hot token or in a c with a (c, sos) bigram,
    at every position and per row, with the forward index."""
    name = "edges_o3"
    data, lm, hist = forms.case_data(name), _model(name, device), _hist(name, device)
    V, (S, B) = data.case[0], hist.shape
    assert int((lm.succ_tok == V).sum()) >= 3
    m = forms.marks(name)
    rows = np.array(sorted(set((m["hot"] + 1).tolist()) | set((m["sos_pred"] + 1).tolist())))
    assert len(rows) >= 10 and rows.max() < B
    full = lm(hist).cpu().numpy()
    for pos in range(1, S + 1):  # (the column before ends in hot / c at position S; at others it may)
        exp = data.walk[pos]
        bad = forms.mismatches(full[pos][rows], exp[rows])
        assert not bad, "position {}: rows {} after a hot / (c, sos) column differ at {}".format(pos, rows.tolist(), bad)
        assert np.array_equal(full[pos][rows, 0], exp[rows, 0])


def test_order_17_is_refused_and_16_scored(device):
    V, sos, dicts = forms.order17()
    lm = M.LookupLanguageModel(V, sos, dicts).to(device)
    assert lm.max_ngram == 17
    hist = torch.arange(1, 19, device=device).view(18, 1).expand(18, 3)
    with pytest.raises(RuntimeError, match="pdt_lookup_lm_log_probs: sequence too long for the MI355X kernel"):
        lm(hist, None, 17)
    with pytest.raises(RuntimeError, match="pdt_lookup_lm_log_probs: sequence too long"):
        lm(hist)
    # one order less: the kernel's arrays to their last slot, exactly
    data, lm16, h16 = forms.case_data("order16"), _model("order16", device), _hist("order16", device)
    S = h16.shape[0]
    assert lm16.max_ngram == 16 and S >= 16
    _exact(lm16(h16, None, S)[0], data.walk[S], "order16", "position {}".format(S))


def test_position_beyond_the_history_still_raises(device):
    name = "edges_o3"
    lm, hist = _model(name, device), _hist(name, device)
    S, B = hist.shape
    idx = torch.from_numpy(_mixed_idx(S, B)).to(device)
    lm(hist, None, idx)
    idx[B // 2] = S + 1
    with pytest.raises(RuntimeError):
        lm(hist, None, idx)
    with pytest.raises(RuntimeError):
        lm(hist, None, S + 1)
    with pytest.raises(RuntimeError):
        lm(hist, None, torch.full((B,), -S - 2, device=device))
