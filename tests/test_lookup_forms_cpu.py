"""The case table of tests/_lookup_forms.py on the CPU: what every case plants is in the model that
LookupLanguageModel builds from it, the forward index of the second level (`_widen`) is the bigram level of
the trie regrouped, and the two yardsticks of tests/test_lookup_forms_gpu.py agree with each other --
oracle.trie_log_probs (a walk of the trie's buffers in float32) against oracle.backoff_log_probs (the
recursion over the n-gram tables in float64): the same class (finite / -inf) everywhere, finite values
within 2 (order - 1) 2**-24 A, the bound derived in tests/_lookup_forms.py."""
import numpy as np
import pytest
import torch

import _lookup_forms as forms
from pydrobert_amd import modules as M


def _index(lm):
    V, U = lm.vocab_size, lm.vocab_size + lm.shift + 1
    return V, U, lm.succ_start.numpy(), lm.succ_tok.numpy(), lm.succ_node.numpy()


def test_every_vocabulary_edge_has_its_cases():
    assert set(forms.BY_VOCAB) == {128, 129, 512, 513, 641}
    for V, names in forms.BY_VOCAB.items():
        assert all(forms.build(n)[0] == V for n in names)
        assert len(names) >= 2 or forms.build(names[0])[2] == 3
    assert [forms.build("ids_u8_edge_%d" % V)[0] for V in (254, 255)] == [254, 255]
    assert [forms.build("ids_i16_edge_%d" % V)[0] for V in (32766, 32767)] == [32766, 32767]
    assert forms.build("tiny")[0] == 5 and set(sum(forms.BY_VOCAB.values(), ())) < set(forms.NAMES)


def test_builders_are_deterministic():
    a, b = forms.build("edges_o3"), forms.build("edges_o3")
    assert a[:3] == b[:3] and a[3] == b[3] and np.array_equal(a[4], b[4]) and a[5] == b[5]


@pytest.mark.parametrize("name,largest,empty,ending_in_sos", [
    ("edges_o3", 300, 300, 3), ("edges_in", 300, 300, 0), ("order2", 257, 300, 3), ("order4_sparse", 257, 0, 0),
])  # fmt: skip
def test_planted_successor_groups(name, largest, empty, ending_in_sos):
    data = forms.case_data(name)
    V, U, start, tok, node = _index(data.lm)
    sizes = np.diff(start)
    assert start.size == U + 1 and sizes.max() >= largest > 128, sizes.max()
    assert int((sizes[: U - 1] == 0).sum()) >= empty
    assert int((tok == V).sum()) >= ending_in_sos
    hist = data.case[4]
    if name.startswith("edges"):
        logps = data.lm.logps.numpy()
        assert int(np.isneginf(logps[U:]).sum()) >= 50  # placeholder nodes
        assert int(np.isneginf(logps[:V]).sum()) == 2  # (and two tokens of no unigram)
        assert sizes[forms.HOT] == sizes.max()
        assert (sizes[np.array(forms.EMPTY)] == 0).all()
        # children of one node for find_child's search: hundreds, and exactly one
        cs = data.lm.child_start.numpy()
        assert cs[forms.POP + 1] - cs[forms.POP] == 299 and cs[forms.ONE_CHILD + 1] - cs[forms.ONE_CHILD] == 1
        assert hist.shape[0] == 4 and hist.shape[1] >= 200 and data.case[5] == (0, 1, 2, 3, 4)
        m = forms.marks(name)
        assert len(m["hot"]) >= 8 and len(m["empty"]) >= 8 and len(m["sos_pred"]) >= 10
        last = set(hist[-1].tolist())
        assert {-7, V, V + 1, 2**40} <= last and (name != "edges_o3" or -1 in last)
        assert m["hot"].max() + 1 < hist.shape[1] and m["sos_pred"].max() + 1 < hist.shape[1]
        if name == "edges_o3":
            # (c, sos) for the hot token, two more, and sos itself; trigrams over real bigrams
            bi, tri = data.case[3][1], data.case[3][2]
            assert all((c, -1) in bi for c in (forms.HOT, 20, 21, -1))
            assert sum((-1, v) in bi for v in range(V)) >= 30
            assert sum(k[1:] in bi for k in tri) >= 150 and sum(k[1:] not in bi for k in tri) >= 50


def test_order4_contexts_without_their_4gram_and_the_reverse():
    V, sos, order, dicts, hist, positions = forms.build("order4_sparse")
    uni, bi, tri, four = dicts
    lone3 = [k for k in tri if not any(f[:3] == k for f in four)]
    lone4 = [f for f in four if f[:3] not in tri]
    assert len(lone3) >= 100 and len(lone4) >= 30
    # ... and both among the contexts the histories end on, so bo[3] is read both ways
    ends = {tuple(int(t) for t in hist[-3:, b]) for b in range(hist.shape[1])}
    assert len(ends & set(lone3)) >= 5 and len(ends & {f[:3] for f in lone4}) >= 5
    lm = forms.case_data("order4_sparse").lm
    U = V + 1
    assert int(np.isneginf(lm.logps.numpy()[U:]).sum()) >= 60  # placeholders at both middle levels


def test_order16_histories_match_to_their_depth():
    V, sos, order, dicts, hist, positions = forms.build("order16")
    assert order == 16 and V == 129 and positions == tuple(range(hist.shape[0] + 1))
    got = [forms.deepest_match(dicts, tuple(int(t) for t in hist[-15:, k])) for k in range(len(forms.O16_DEPTHS))]
    assert tuple(got) == forms.O16_DEPTHS == (1, 2, 7, 15, 16)
    lm = forms.case_data("order16").lm
    assert lm.max_ngram == 16 and 5e4 <= lm.logps.numel() <= 2e5
    assert int(np.isneginf(lm.logps.numpy()[V + 2 :]).sum()) > 0


@pytest.mark.parametrize("name,ids,offsets", [
    ("tiny", torch.uint8, torch.uint8), ("plain_128", torch.uint8, torch.int16),
    ("edges_o3", torch.int16, torch.int16), ("order16", torch.uint8, torch.int16),
    ("ids_u8_edge_254", torch.uint8, torch.int16), ("ids_u8_edge_255", torch.int16, torch.int16),
    ("ids_i16_edge_32766", torch.int16, torch.int32), ("ids_i16_edge_32767", torch.int32, torch.int32),
])  # fmt: skip
def test_buffer_dtypes(name, ids, offsets):
    data = forms.case_data(name)
    lm, V = data.lm, data.case[0]
    assert lm.ids.dtype == ids and lm.offsets.dtype == offsets, (lm.ids.dtype, lm.offsets.dtype)
    assert lm.ids_wide.dtype == torch.int32 and lm.child_start.dtype == torch.int32
    assert torch.equal(lm.ids_wide.long(), lm.ids.long())  # (no sign lost in the widening)
    if "_edge_" in name:
        # n-grams on the top token ids: V - 1 is a label at both levels and has children of its own
        assert int(lm.ids_wide.max()) == V - 1 and int((lm.ids_wide == V - 1).sum()) >= 5
        assert int(lm.child_start[V]) > int(lm.child_start[V - 1])
        assert data.case[4].shape[1] * len(data.case[5]) == (8 if "i16" in name else 150)


@pytest.mark.parametrize("name", forms.NAMES)
def test_forward_index_is_the_bigram_level_regrouped(name):
    lm = forms.case_data(name).lm
    V, U, start, tok, node = _index(lm)
    cs, ids = lm.child_start.numpy(), lm.ids_wide.numpy()
    # the bigram level by direct enumeration: children of the unigram nodes 0 .. U - 2
    level = [(int(ids[n - U]), v, n) for v in range(U - 1) for n in range(cs[v], cs[v + 1])]
    assert len(level) == node.size == tok.size == start[-1] and start[0] == 0 and (np.diff(start) >= 0).all()
    assert sorted(node.tolist()) == [n for _, _, n in sorted(level, key=lambda x: x[2])]  # each node once
    assert len(set(node.tolist())) == node.size
    group = np.repeat(np.arange(U), np.diff(start))
    assert np.array_equal(ids[node - U], group)  # in the group of its label
    under = np.searchsorted(cs[:U], node, side="right") - 1
    assert np.array_equal(tok, under)  # the unigram it hangs under
    assert sorted(level) == list(zip(group.tolist(), tok.tolist(), node.tolist()))  # ascending inside a group
    same = group[1:] == group[:-1]
    assert (np.diff(tok)[same] > 0).all()


@pytest.mark.parametrize("name", forms.NAMES)
def test_walk_agrees_with_the_brute_force(name):
    data = forms.case_data(name)
    V, sos, order, dicts, hist, positions = data.case
    worst = 0.0
    for pos in positions:
        walk, brute, bound = data.walk[pos], data.brute[pos], data.bound[pos]
        assert walk.dtype == np.float32 and walk.shape == brute.shape == bound.shape == (hist.shape[1], V)
        assert not np.isnan(walk).any() and not np.isposinf(walk).any()
        fin = np.isfinite(brute)
        assert np.array_equal(np.isfinite(walk), fin), (name, pos)
        assert np.isfinite(bound[fin]).all() and (bound[fin] > 0).all()
        diff = np.abs(walk[fin].astype(np.float64) - brute[fin])
        over = diff > bound[fin]
        assert not over.any(), (name, pos, float(diff[over].max()), np.argwhere(fin)[over][:5].tolist())
        worst = max(worst, float(diff.max()) if diff.size else 0.0)
    print("{}: largest walk - brute difference {:.3g}".format(name, worst))
    if name in ("edges_o3", "tiny"):
        assert any((~np.isfinite(data.brute[p])).any() for p in positions)  # the -inf class is populated


def test_history_token_v_is_sos_under_the_shift():
    """The one place where the tables need `table_hist`: id V is sos's, so the trie reads a history token V as
    sos; without the shift V is outside like any other."""
    data = forms.case_data("edges_o3")
    V, sos, order, dicts, hist, positions = data.case
    cols = np.flatnonzero(hist[-1] == V)
    twin = np.flatnonzero(hist[-1] == sos)
    assert len(cols) and len(twin)
    th = forms.table_hist(hist, V, sos)
    assert (th[-1, cols] == sos).all() and np.array_equal(th != hist, hist == V)
    inside = forms.case_data("edges_in").case
    assert forms.table_hist(inside[4], inside[0], inside[1]) is inside[4]


def test_order17_model_builds_on_the_cpu():
    lm = M.LookupLanguageModel(*forms.order17())
    assert lm.max_ngram == 17
