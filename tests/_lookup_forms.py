"""The case table of the LookupLanguageModel kernel's own tests (csrc/lm_lookup.hip), built on the CPU:
tests/test_lookup_forms_cpu.py asserts what every case plants, tests/test_lookup_forms_gpu.py scores the
cases on the device.

``build(name)`` returns ``(V, sos, order, prob_dicts, hist, positions)`` from a seeded generator.  The
STRUCTURE of a model (which n-grams exist) is planted by construction -- ``marks(name)`` names the tokens it
is planted on --; a random draw only picks values and the filler around the planted entries.  Every value
is a float32, so the float64 brute force (oracle.backoff_log_probs) sums exactly the numbers the trie holds.

``case_data(name)`` adds, once per case and position: the model on the CPU, the scalar walk of its trie
(oracle.trie_log_probs: the kernel's arithmetic in the kernel's order -- bit-exact yardstick), the brute
force, and the bound between the two:

    the walk does two float32 additions per order above the first, each with a relative error of at most
    2**-24 of its result, so  |walk - brute| <= 2 (order - 1) 2**-24 A  per element, where A is the brute
    force's recursion over the ABSOLUTE values of the same entries (``abs_scale``) and bounds every partial
    sum of the walk.  (At least one of the two additions of a step adds an exact 0 -- the step's other
    back-off was consumed or never there --, so first-order error is half the bound; the other half covers
    the (1 + 2**-24)**k growth of the partial sums with room to spare.)

A history token equal to V under the shift (sos outside the vocabulary) is the SAME context as sos -- id V is
where the trie keeps sos, reference _lm.py:470 --, which the n-gram tables spell ``sos``: ``table_hist``
rewrites it for the two table-based functions.  Every other token outside 0 .. V - 1 is a context no n-gram
has, for the kernel, the walk and the tables alike."""
import collections
import functools

import numpy as np

NINF = -float("inf")
NAMES = ("tiny", "edges_o3", "edges_in", "order2", "order4_sparse", "order16", "plain_128", "plain_129",
         "plain_512", "ids_u8_edge_254", "ids_u8_edge_255", "ids_i16_edge_32766", "ids_i16_edge_32767")  # fmt: skip
# every vocabulary edge of the kernel's strides (128 | 129: second trip of `v += 128`; 512 | 513 | 641: second
# group of four loads, and a partial one) carries at least two cases or a plain order-3 model
BY_VOCAB = {128: ("plain_128",), 129: ("plain_129", "order16"), 512: ("plain_512",),
            513: ("order2", "order4_sparse"), 641: ("edges_o3", "edges_in")}  # fmt: skip
BAD = (-7, 2**40)  # (with V and V + 1: the history tokens outside the vocabulary)


def _vals(rng, n):
    return [float(x) for x in rng.normal(size=n).astype(np.float32)]


def _fill(rng, V, sos, order, levels, no_unigram=()):
    """n-gram key sets (levels[n - 2] for order n >= 2) -> prob_dicts with float32 values, every token a
    unigram but ``no_unigram`` (and sos, when it is outside the vocabulary, a very unlikely one)."""
    shift = not 0 <= sos < V
    lp, bo = _vals(rng, V), _vals(rng, V)
    uni = {v: (lp[v], bo[v]) for v in range(V) if v not in no_unigram}
    if shift:
        uni[sos] = (-99.0, _vals(rng, 1)[0])
    dicts = [uni]
    for n, keys in enumerate(levels, 2):
        keys = sorted(set(keys))
        assert all(len(k) == n for k in keys)
        lp, bo = _vals(rng, len(keys)), _vals(rng, len(keys))
        dicts.append({k: (lp[i] if n == order else (lp[i], bo[i])) for i, k in enumerate(keys)})
    assert len(dicts) == order
    return dicts


def _columns(rng, tails, S, pool):
    """One history column per tail, the tail at its end and tokens of ``pool`` before it."""
    cols = [[int(t) for t in rng.choice(pool, S - len(tail))] + list(tail) for tail in tails]
    return np.array(cols, dtype=np.int64).T.copy()


# ---- V = 641, order 3: the planted structure -----------------------------------------------------------
HOT, POP, ONE_CHILD = 7, 11, 13  # (many successors | many predecessors | exactly one predecessor, 25)
EMPTY = range(300, 620)  # never the first token of a bigram, never the middle one of a trigram
SOS_PRED = (HOT, 20, 21)  # c with a bigram (c, sos)
TRI_FAN = range(100, 500, 2)  # a with the trigram (a, HOT, 12): 200 children of one bigram node


def _edges(V, sos, seed):
    rng = np.random.default_rng(seed)
    shift = not 0 <= sos < V
    bi, tri = set(), set()
    bi.update((HOT, v) for v in range(0, V, 2))  # 321 successors of one context token ...
    bi.add((HOT, V - 2))
    bi.update((c, POP) for c in range(1, 300))  # ... 299 children of one unigram node
    bi.add((25, ONE_CHILD))
    fill = [v for v in range(V) if v not in (POP, ONE_CHILD)]
    for c in range(20, 170):
        bi.update((c, int(v)) for v in rng.choice(fill, 1 + c % 5, replace=False))
    bi.update((c, sos) for c in SOS_PRED + (sos,))  # n-grams ENDING in sos
    bi.update((sos, v) for v in range(40, 70))  # sentence starts
    real = sorted(bi)
    pred = collections.defaultdict(list)
    for a, b in real:
        pred[b].append(a)
    ctx_tokens = list(range(1, 300)) + list(range(620, V))
    tri.update((a, HOT, 12) for a in TRI_FAN)
    for i, (b, c) in enumerate(k for k in real if 20 <= k[0] < 170):  # over existing bigrams
        if i % 2 == 0:
            tri.add((int(rng.choice(ctx_tokens)), b, c))
        if i % 3 == 0 and pred[b]:
            tri.add((pred[b][0], b, c))  # (its context a bigram too: a back-off at order 2)
    tri.update((sos, sos, v) for v in range(40, 50))
    tri.update((sos, 40, c) for c in range(3))
    tri.add((20, HOT, sos))
    over = len([k for k in tri if k[1:] in bi])
    hollow = {(b + 1, b, 2 * b + 1) for b in range(170, 230)}  # suffix bigram absent: placeholder nodes
    assert not any(k[1:] in bi for k in hollow) and over >= 150
    tri |= hollow
    assert not any(k[0] in EMPTY for k in bi) and not any(k[1] in EMPTY for k in tri)
    dicts = _fill(rng, V, sos, 3, [bi, tri], no_unigram=(250, 630))
    tails = [(x, HOT) for x in (100, 498, 300, 301, 5, V - 1, sos, 12, 20)]
    for e in (300, 301, 450, 619):
        tails += [(HOT, e), (25, e)]
    for a, b, c in sorted(tri)[::5][:60]:  # on real trigrams, and one token off them
        tails += [(a, b), (a + 1, b), (a, b + 1)]
    for bad in BAD + (V, V + 1) + ((sos,) if shift else ()):
        tails += [(HOT, bad), (bad, HOT), (bad, bad)]
    tails += [(x, POP) for x in (1, 299, 150, 0, V - 1, 400)]  # first | last | inner child, below, above, absent
    tails += [(25, ONE_CHILD), (26, ONE_CHILD), (24, ONE_CHILD)]
    for c in SOS_PRED[1:]:
        tails += [(HOT, c), (c, c)]
    tails += [tuple(int(t) for t in rng.integers(0, V, 2)) for _ in range(20)]
    hist = _columns(rng, tails, 4, list(range(40, 70)) + [HOT, POP, 20, 21, 25, sos])
    assert hist.shape[1] >= 200
    return V, sos, 3, dicts, hist, tuple(range(5))


def _order2(V, sos, seed):
    rng = np.random.default_rng(seed)
    bi = {(HOT, v) for v in range(0, V, 2)}
    bi.update((c, POP) for c in range(1, 200))
    for c in range(20, 120):
        bi.update((c, int(v)) for v in rng.choice(V, 1 + c % 4, replace=False))
    bi.update((c, sos) for c in SOS_PRED + (sos,))
    bi.update((sos, v) for v in range(40, 70))
    dicts = _fill(rng, V, sos, 2, [bi], no_unigram=(250,))
    tails = [(t,) for t in (HOT, 300, 450, V - 1, 0, 20, 21, 25, POP, sos, V, V + 1) + BAD]
    tails += [(int(t),) for t in rng.integers(0, V, 50)]
    hist = _columns(rng, tails, 3, list(range(20, 70)) + [HOT, sos, 300])
    return V, sos, 2, dicts, hist, tuple(range(4))


def _order4_sparse(V, sos, seed):
    """Sentences over 1 .. 199 with every bigram and trigram; the 4-grams of every other sentence only
    (``lone3``: trigram contexts whose 4-gram is absent); 4-grams led by a token no trigram starts with
    (``lone4``: the reverse); 4-grams over 300 .. 399 with nothing below them (placeholders at both middle
    levels)."""
    rng = np.random.default_rng(seed)
    sents = [[int(t) for t in rng.integers(1, 200, 8)] for _ in range(60)]
    bi, tri, four, lone3, lone4, hollow = set(), set(), set(), [], [], []
    for i, s in enumerate(sents):
        if i < 12:
            s = [sos] * 3 + s  # sentence starts, padded to the full context
        bi.update(tuple(s[j : j + 2]) for j in range(len(s) - 1) if s[j + 1] != sos)
        tri.update(tuple(s[j : j + 3]) for j in range(len(s) - 2) if s[j + 2] != sos)
        if i % 2 == 0:
            four.update(tuple(s[j : j + 4]) for j in range(len(s) - 3) if s[j + 3] != sos)
    for i, s in enumerate(sents):
        if i % 2:
            lone3 += [tuple(s[j : j + 4]) for j in range(len(s) - 3) if tuple(s[j : j + 4]) not in four]
        elif i >= 12:
            lone4.append((200 + i,) + tuple(s[1:4]))
    four.update(lone4)
    for i in range(30):
        hollow.append((300 + i, 330 + i, 360 + i, 390 + (i % 10)))
    four.update(hollow)
    bi.update((HOT, v) for v in range(0, V, 2))  # (second trip of the successor pass at this order too)
    assert lone3 and all(k[:3] in tri and k not in four for k in lone3)
    assert all(k[:3] not in tri and k[1:] in tri for k in lone4)
    assert all(k[1:] not in tri and k[2:] not in bi for k in hollow)
    dicts = _fill(rng, V, sos, 4, [bi, tri, four])
    tails = [tuple(s[j : j + 5]) for s in sents[:14] for j in (0, 3)]
    tails += [k[:3] for k in lone3[:8]] + [k[:3] for k in lone4[:8]] + [k[:3] for k in hollow[:6]]
    tails += [(k[0] + 1,) + k[1:3] for k in hollow[:3]] + [k[:2] + (k[2] + 1,) for k in lone3[:3]]
    tails += [(HOT, HOT, HOT), (1, 2, HOT), (-7, 5, 6), (5, V, 6), (5, 6, 2**40), (sos, sos, sos)]
    hist = _columns(rng, tails, 5, list(range(1, 200)))
    return V, sos, 4, dicts, hist, tuple(range(6))


# ---- order 16 ------------------------------------------------------------------------------------------
O16_DEPTHS = (1, 2, 7, 15, 16)  # deepest n-gram matching history column k at its last position
O16_NEVER, O16_BREAK = 125, 126  # tokens of no n-gram but their unigrams


def _order16(V, sos, seed):
    """Chains of real 16-grams: every window of up to 16 tokens of 250 sentences over 0 .. 99 and 5 anchor
    sentences over 100 .. 119, each padded with sos in front; a seventh of the random sentences' n-grams of
    orders 3 .. 12 dropped (a placeholder where a longer one still needs them).  Column k of the histories
    ends on the first 15 tokens of anchor k, broken O16_DEPTHS[k] tokens from its end."""
    rng = np.random.default_rng(seed)
    N = 16
    levels = [set() for _ in range(N - 1)]
    sents = [[int(t) for t in rng.integers(100, 120, 24)] for _ in range(5)]
    sents += [[int(t) for t in rng.integers(0, 100, 24)] for _ in range(250)]
    for i, s in enumerate(sents):
        p = [sos] * (N - 1) + s
        for end in range(N, len(p) + 1):
            for n in range(2, N + 1):
                if i >= 5 and 3 <= n <= 12 and rng.random() < 1 / 7:
                    continue
                levels[n - 2].add(tuple(p[end - n : end]))
    dicts = _fill(rng, V, sos, N, levels)
    cols = []
    for k, depth in enumerate(O16_DEPTHS):
        col = [O16_NEVER, O16_NEVER] + sents[k][:15]
        if depth == 1:
            col[-1] = O16_NEVER
        elif depth < 16:
            col[-depth] = O16_BREAK
        cols.append(col)
    for s in sents[5:10]:
        cols.append(s[:17])  # from the sentence's start: sos-padded contexts that are n-grams
    cols.append(sents[10][3:20])
    cols.append([int(t) for t in rng.integers(0, V, 17)])
    hist = np.array(cols, dtype=np.int64).T.copy()
    return V, sos, N, dicts, hist, tuple(range(18))


def deepest_match(dicts, ctx):
    """Largest n such that the last n - 1 tokens of ``ctx`` start an n-gram of the tables."""
    best = 1
    for n in range(2, len(dicts) + 1):
        tail = tuple(ctx[len(ctx) - (n - 1) :])
        if any(k[:-1] == tail for k in dicts[n - 1]):
            best = n
    return best


# ---- plain models and the dtype edges of the host's buffers ---------------------------------------------
def _plain(V, sos, seed):
    rng = np.random.default_rng(seed)
    bi = {(3, v) for v in range(0, V, 2) if v < 400}
    for c in range(5, 60):
        bi.update((c, int(v)) for v in rng.choice(V, 1 + c % 6, replace=False))
    bi.update((sos, v) for v in range(10, 20))
    real = sorted(bi)
    tri = {(int(rng.integers(0, V)), b, c) for b, c in real[::3]}
    tri.update((c, c + 1, V - 1 - c) for c in range(70, 90))  # placeholders
    dicts = _fill(rng, V, sos, 3, [bi, tri])
    tails = [k[:2] for k in sorted(tri)[::4]][:20] + [(5, 3), (V - 1, 3), (3, 3), (0, V - 1), (V - 1, V - 1)]
    tails += [(3, V), (3, -7)] + [tuple(int(t) for t in rng.integers(0, V, 2)) for _ in range(13)]
    hist = _columns(rng, tails, 4, list(range(5, 60)) + [3, sos])
    return V, sos, 3, dicts, hist, tuple(range(5))


def _ids_edge(V, seed, cols):
    """sos = 0, so U = V + 1 decides the dtype of ``ids``; bigrams and trigrams among the top token ids."""
    rng = np.random.default_rng(seed)
    T = (V - 1, V - 2, V - 3, 1, 2)
    bi = {(a, b) for i, a in enumerate(T) for j, b in enumerate(T) if (i + j) % 4}
    bi.update((0, t) for t in T)
    tri = {(a, b, c) for i, a in enumerate(T) for j, b in enumerate(T) for k, c in enumerate(T)
           if (i + 2 * j + k) % 3 == 0}  # fmt: skip
    assert any(k[1:] not in bi for k in tri) and (V - 1, V - 1, V - 1) in tri
    dicts = _fill(rng, V, 0, 3, [bi, tri])
    if cols is None:  # 8 rows: two columns of three tokens, every position
        hist = np.array([[V - 1, V - 1, V - 2], [V - 3, 1, V - 1]], dtype=np.int64).T.copy()
    else:
        tails = [tuple(int(t) for t in rng.choice(T + (0, 3, V), 4)) for _ in range(cols)]
        hist = _columns(rng, tails, 4, T)
    return V, 0, 3, dicts, hist, tuple(range(hist.shape[0] + 1))


def _tiny(seed):
    rng = np.random.default_rng(seed)
    V = 5
    bi = {(a, b) for a in range(V) for b in range(V) if rng.random() < 0.5}
    tri = {(a, b, c) for a in range(V) for b in range(V) for c in range(V) if rng.random() < 0.5}
    dicts = _fill(rng, V, 0, 3, [bi, tri], no_unigram=(3,))
    hist = rng.integers(0, V, (4, 40)).astype(np.int64)
    return V, 0, 3, dicts, hist, tuple(range(5))


def build(name):
    """(V, sos, order, prob_dicts, hist, positions) of a case, the same at every call."""
    if name == "tiny":
        return _tiny(1)
    if name == "edges_o3":
        return _edges(641, -1, 2)
    if name == "edges_in":
        return _edges(641, 0, 3)
    if name == "order2":
        return _order2(513, -1, 4)
    if name == "order4_sparse":
        return _order4_sparse(513, 0, 5)
    if name == "order16":
        return _order16(129, -1, 6)
    if name.startswith("plain_"):
        V = int(name[6:])
        return _plain(V, 0 if V == 129 else -1, 7 + V)
    if name.startswith("ids_u8_edge_"):
        return _ids_edge(int(name[12:]), 8, 30)
    if name.startswith("ids_i16_edge_"):
        return _ids_edge(int(name[13:]), 9, None)
    raise KeyError(name)


def order17():
    """(V, sos, prob_dicts) one order beyond the kernel's sixteen: unigrams and one chain."""
    rng = np.random.default_rng(17)
    chain = tuple(range(1, 18))
    return 20, 0, _fill(rng, 20, 0, 17, [set() for _ in range(15)] + [{chain}])


def marks(name):
    """Columns of a case's histories by what their last token is planted as."""
    V, sos, order, dicts, hist, positions = case_data(name).case
    last = hist[-1]
    return {"hot": np.flatnonzero(last == HOT), "sos_pred": np.flatnonzero(np.isin(last, SOS_PRED + (sos,))),
            "empty": np.flatnonzero((last >= EMPTY[0]) & (last <= EMPTY[-1])),
            "outside": np.flatnonzero((last < 0) | (last >= V))}  # fmt: skip


# ---- the yardsticks, once per case ---------------------------------------------------------------------
def table_hist(hist, V, sos):
    if 0 <= sos < V:
        return hist
    return np.where(hist == V, sos, hist)


def by_context(prob_dicts):
    """by_context(...)[n][h] = the (w, log-probability) pairs of the n-grams h w."""
    N = len(prob_dicts)
    by_ctx = [None, None] + [collections.defaultdict(list) for _ in range(N - 1)]
    for n in range(2, N + 1):
        for k, val in prob_dicts[n - 1].items():
            by_ctx[n][k[:-1]].append((k[-1], val if n == N else val[0]))
    return by_ctx


def abs_scale(prob_dicts, vocab_size, sos, hist, idx, by_ctx=None):
    """(B, V) float64: oracle.backoff_log_probs' recursion over the absolute values of the same entries --
    A(h w) = |table[h w]| if present and finite, else |backoff(h)| + A(h[1:] w) --, bottom-up; inf where the
    brute force is -inf."""
    import oracle

    N, V = len(prob_dicts), vocab_size
    by_ctx = by_ctx or by_context(prob_dicts)
    uni = np.full(V, np.inf)
    for v, val in prob_dicts[0].items():
        if 0 <= v < V:
            uni[v] = abs(val if N == 1 else val[0])
    B = hist.shape[1]
    idx = np.broadcast_to(np.asarray(idx), (B,))
    out = np.empty((B, V))
    for b in range(B):
        ctx = oracle._lm.context_of(hist, b, int(idx[b]), N, sos)
        val = uni.copy()
        for n in range(2, N + 1):
            c = ctx[N - n :]
            e = prob_dicts[n - 2].get(c[0] if n == 2 else c)
            if e is not None:
                val = val + abs(e[1])
            for v, lp in by_ctx[n].get(c, ()):
                if 0 <= v < V and lp != NINF:
                    val[v] = abs(lp)
        out[b] = val
    return out


Data = collections.namedtuple("Data", "case lm walk brute bound")


@functools.lru_cache(maxsize=None)
def case_data(name):
    """The case, its model on the CPU, and per position the (B, V) walk, brute force and bound."""
    import oracle
    from pydrobert_amd import modules as M

    case = V, sos, order, dicts, hist, positions = build(name)
    lm = M.LookupLanguageModel(V, sos, dicts)
    bufs = [getattr(lm, k).numpy() for k in ("logps", "logbs", "ids", "offsets")]
    th = table_hist(hist, V, sos)
    walk, brute, bound = {}, {}, {}
    by_ctx = by_context(dicts)
    for pos in positions:
        # columns with one context at this position (all of them at position 0) share a row: the
        # yardsticks run on the first such column of the history itself
        ctxs = [oracle._lm.context_of(hist, b, pos, order, sos) for b in range(hist.shape[1])]
        first = {}
        for b, c in enumerate(ctxs):
            first.setdefault(c, b)
        reps = sorted(first.values())
        back = np.array([reps.index(first[c]) for c in ctxs])
        sub, tsub = np.ascontiguousarray(hist[:, reps]), np.ascontiguousarray(th[:, reps])
        walk[pos] = oracle.trie_log_probs(*bufs, V, sos, order, sub, pos)[back]
        brute[pos] = oracle.backoff_log_probs(dicts, V, sos, tsub, pos)[back]
        bound[pos] = (2 * (order - 1) * 2.0**-24 * abs_scale(dicts, V, sos, tsub, pos, by_ctx))[back]
    return Data(case, lm, walk, brute, bound)


def mismatches(act, exp, limit=5):
    """The first ``limit`` (row, v) pairs at which two float arrays differ in bits (NaN equal to NaN)."""
    act, exp = np.asarray(act), np.asarray(exp)
    if act.shape != exp.shape:
        return [("shape", act.shape, exp.shape)]
    bad = ~((act == exp) | (np.isnan(act) & np.isnan(exp)))
    return [tuple(int(x) for x in rc) for rc in np.argwhere(bad)[:limit]]
