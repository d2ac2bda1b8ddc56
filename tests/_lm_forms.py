"""Inputs of tests/test_lm_search_forms_gpu.py: CTCPrefixSearch with an n-gram LookupLanguageModel in the
loop at the shapes where the kernels take another form (csrc/ctc_lm_table.hip: the ten instances, the list
selection's tiers, the checkpoint spacing; csrc/ctc_lm_step.hip: the waves per element, the LDS capacity),
their oracle results and their near-tied utterances.  Everything here runs on the CPU and is computed once
per case (``case_data``); nothing is written to after that.

Near ties (the method of tests/test_ctc_wide_search_gpu.py): the oracle is run three more times on the
logits times ``1 + u * 4e-7``, ``u ~ U(-1, 1)``; an utterance whose beam changes in any run is marked and
left out of the EXACT comparison only.  The cases of exact ties are never marked: equal masses are equal in
every arithmetic, and the order among them is the oracle's (the lower token wins)."""
import collections
import functools
import zlib

import numpy as np

import oracle

BETA = 0.3
MASS_FLOOR = 1e-30  # every finite positive oracle mass: a flushed denormal must not decide a result
BLANK_SHARE = 0.87  # of the long inputs' frames (at 0.85 the smallest mass of V = 64, T = 200 is 3e-31: below the floor)

# kind: "peaky" = N(0, 1) + 8 on one class per frame; "blank" = the same with the blank peaking in BLANK_SHARE of
# the frames; "tied" = tokens (2i, 2i + 1) share their logit and every model score; "heavy" = every token
# logit equal, the blank one higher, every unigram equal.
# table / search: whether the one-launch routes take the case (csrc/ctc_lm_table.hip: V <= 5119;
# csrc/ctc_lm_step.hip: the rows fit the LDS) -- stated here, checked against what ran.
Case = collections.namedtuple("Case", "name V K T N order sos_in kind table search successors layout")


def _case(name, V, K, T, N=5, order=2, sos_in=False, kind="peaky", table=True, search=True, successors=6, layout=""):
    return Case(name, V, K, T, N, order, sos_in, kind, table, search, successors, layout)


INSTANCES = [(8, 16), (20, 32), (63, 16), (64, 17), (65, 32), (511, 16), (512, 32), (1023, 16), (1024, 9),
             (2047, 16), (2048, 32), (3071, 16), (3072, 5), (5119, 16), (5119, 32)]
TIE_SHAPES = [(70, 16), (300, 16), (300, 32), (700, 8)]
# the largest vocabulary pdt_ctc_lookup_lm_search's LDS plan admits at width 4 (tests/test_lm_table_plan_cpu.py
# pins it to the plan's arithmetic)
SEARCH_MAX_V_W4 = 20044

CASES = (
    [_case("inst_V%d_K%d" % (V, K), V, K, 8 if V >= 2048 else 12, 3 if (V, K) == (5119, 32) else 5) for V, K in INSTANCES]
    + [_case("inst_V5120_K8", 5120, 8, 8, table=False)]
    + [_case("tiny_V%d_K%d" % (V, K), V, K, 12) for V, K in [(3, 8), (7, 16), (19, 32), (2, 32)]]
    + [_case("order%d_V%d_K%d_sos%s" % (o, V, K, "in" if s else "out"), V, K, 12, order=o, sos_in=s)
       for o, V, K in [(3, 65, 16), (3, 130, 32), (4, 12, 32)] for s in (False, True)]
    + [_case("ckpt_V%d_K%d_T%d" % (V, K, T), V, K, T, 3, kind="blank") for V, K, T in [(8, 16, 200), (20, 32, 300), (64, 16, 200)]]
    + [_case("tied_V%d_K%d" % (V, K), V, K, 2, kind="tied") for V, K in TIE_SHAPES]
    + [_case("heavy_V%d_K%d" % (V, K), V, K, 2, kind="heavy") for V, K in TIE_SHAPES]
    + [_case("layout_batch_major", 65, 16, 6, layout="batch_major"), _case("layout_stride2", 65, 16, 6, layout="stride2"),
       _case("layout_N37", 65, 16, 6, 37)]
    + [_case("capacity_V%d" % SEARCH_MAX_V_W4, SEARCH_MAX_V_W4, 4, 3, 2, table=False, successors=2),
       _case("capacity_V%d" % (SEARCH_MAX_V_W4 + 1), SEARCH_MAX_V_W4 + 1, 4, 3, 2, table=False, search=False, successors=2)]
)
BY_NAME = {c.name: c for c in CASES}
CKPT_SHIFTS = {"ckpt_V8_K16_T200": (8, None), "ckpt_V20_K32_T300": (9, None), "ckpt_V64_K16_T200": (6, 6)}  # (at least, at most)
LONG_T = 200  # from here on the probabilities are compared as log-probabilities (tests/_drift.py)


def sos_of(case):
    return 1 if case.sos_in else case.V


def ngram_dicts(case, rng):
    """Back-off n-gram tables of ``case.order``: every token (and an outside sos) a unigram, about
    ``case.successors`` explicit bigrams per context, two trigrams per bigram, one 4-gram per trigram."""
    V, N, sos = case.V, case.order, sos_of(case)
    toks = list(range(V)) + ([] if case.sos_in else [sos])
    tied, heavy = case.kind == "tied", case.kind == "heavy"
    uni = rng.normal(size=len(toks)) - np.log(V)
    if tied:
        uni[: V - V % 2] = np.repeat(uni[: V - V % 2 : 2], 2)
    if heavy:
        uni[:V] = -np.log(V)
    bo = rng.normal(size=len(toks)) * 0.1 - 0.5
    dicts = [{t: (float(uni[i]), float(bo[i])) for i, t in enumerate(toks)}]
    prev = [(t,) for t in toks]
    for n in range(1, N):
        per = (min(case.successors, V), 2, 1)[min(n, 3) - 1]
        d = {}
        for ctx in prev:
            if tied:  # whole pairs, both tokens of a pair with one value
                nxt = [int(2 * j + h) for j in rng.choice(V // 2, max(1, per // 2), replace=False) for h in (0, 1)]
                vals = np.repeat(rng.normal(size=len(nxt) // 2) - 3.0 + 0.5 * n, 2)
            elif heavy:  # two tokens above the rest; the rest tie
                nxt = [int(v) for v in rng.choice(V, 2, replace=False)]
                vals = rng.normal(size=2) * 0.1 - np.log(V) + 2.0
            else:
                nxt = [int(v) for v in rng.choice(V, per, replace=False)]
                vals = rng.normal(size=per) - 3.0 + 0.5 * n
            for v, x in zip(nxt, vals):
                d[ctx + (v,)] = float(x) if n == N - 1 else (float(x), float(rng.normal() * 0.1 - 0.4))
        dicts.append(d)
        prev = list(d)
    return dicts


def logits_of(case, rng):
    V, T, N = case.V, case.T, case.N
    if case.kind == "heavy":
        lg = np.zeros((T, N, V + 1), np.float32)
        lg[:, :, V] = 1.0
        return lg
    if case.kind == "tied":
        lg = (rng.normal(size=(T, N, V + 1)) * 2.0).astype(np.float32)
        lg[:, :, 1:V:2] = lg[:, :, 0 : V - 1 : 2]
        return lg
    lg = rng.normal(size=(T, N, V + 1)).astype(np.float32)
    peak = rng.integers(0, V + 1, (T, N))
    if case.kind == "blank":
        peak = np.where(rng.random((T, N)) < BLANK_SHARE, V, rng.integers(0, V, (T, N)))
    boost = np.full((T, N), 8.0, np.float32)
    if case.kind == "peaky":
        # The valid mixture scales the model's share by 1 - p_blank, formed in float32: an ulp of p_blank (6e-8)
        # is a relative 6e-8 / (1 - p_blank) of it, whoever computes it -- 5e-5 when a blank peak of +8 stands
        # against three tokens, above the 1e-5 these cases are compared to.  A blank peak of at most ln V + 2.5
        # keeps 1 - p_blank near 0.1 and that error at 6e-7 a frame (+8 from V = 245 on).
        boost[peak == V] = min(8.0, np.log(V) + 2.5)
    np.put_along_axis(lg, peak[..., None], np.take_along_axis(lg, peak[..., None], 2) + boost[..., None], 2)
    return lg


def lens_of(case):
    T, N = case.T, case.N
    if case.kind == "blank":
        return np.array([T, T // 2 + 1, 33])
    # (a beam wider than the prefixes that exist holds masses that are exactly zero -- a repeated token needs
    # a blank in between -- until enough others exist: at V = 2, K = 32 from frame 2 to frame 5.  The tiny
    # vocabularies pass through those frames but do not stop in them: a tie among zeros decides nothing.)
    base = [T, 0, T - 2, 1, T - 1] if case.name.startswith("tiny") else [T, 0, T // 2 + 1, 1, T - 1]
    return np.array([base[i % 5] if i < 5 else (i * 7) % (T + 1) for i in range(N)])


def near_tied(lg, K, lens, olm, valid_mixture, exp):
    """(N,) bool: utterances whose oracle beam changes under a few-ulp change of the logits."""
    marked = np.zeros(lg.shape[1], bool)
    for seed in (0, 1, 2):
        u = np.random.default_rng(seed).uniform(-1.0, 1.0, lg.shape)
        y, yl, _ = oracle.ctc_prefix_search_lm((lg * (1.0 + u * 4e-7)).astype(np.float32), K, lens, olm, BETA, valid_mixture)
        marked |= (y != exp[0]).any((0, 2)) | (yl != exp[1]).any(1)
    return marked


def brute_force(lg, olm, valid_mixture):
    """{prefix: mass} of ONE utterance's logits (T, V + 1) under a bigram ``olm``, in float64: the sum over
    all (V + 1)^T alignments of the product of their frames' factors -- the blank's probability, a repeated
    class's probability, or, where a new token starts, the mixed extension probability after the prefix so
    far (the mix of CTCPrefixSearch).  What a beam that holds every prefix must return."""
    import itertools

    T, V = lg.shape[0], lg.shape[1] - 1
    p = np.exp(lg.astype(np.float64) - lg.max(1, keepdims=True))
    p /= p.sum(1, keepdims=True)
    factor = {}
    for c in list(range(V)) + [olm.sos]:
        row = olm._row((c,)).astype(np.float64)
        sm = np.exp(row - row.max())
        sm /= sm.sum()
        factor[c] = sm if valid_mixture else sm**BETA
    out = {}
    for path in itertools.product(range(V + 1), repeat=T):
        prefix, w = (), 1.0
        for t, c in enumerate(path):
            if c == V:
                w *= p[t, V]
            elif t > 0 and path[t - 1] == c:
                w *= p[t, c]
            else:
                f = factor[prefix[-1] if prefix else olm.sos][c]
                w *= (1.0 - BETA) * p[t, c] + BETA * f * (1.0 - p[t, V]) if valid_mixture else p[t, c] * f
                prefix += (c,)
        out[prefix] = out.get(prefix, 0.0) + w
    return out


def same_prefix_masses(y, yl, yp, exact, rtol=1e-5):
    """Whether one utterance's beam (y (S, W), yl (W,), yp (W,)) holds every prefix of ``exact`` with a positive
    mass exactly once, with that mass, and otherwise only zero masses and absent entries."""
    got = {}
    for k in np.flatnonzero(np.isfinite(yp) & (yp != 0)):
        key = tuple(int(v) for v in y[: yl[k], k])
        if key in got:
            return False
        got[key] = float(yp[k])
    want = {k: v for k, v in exact.items() if v > 0}
    return not np.isnan(yp).any() and set(got) == set(want) and all(abs(got[k] / want[k] - 1.0) <= rtol for k in want)


Data = collections.namedtuple("Data", "lg lens dicts sos exp marked")


@functools.lru_cache(maxsize=None)
def case_data(name):
    """The inputs of a case, and per mix (valid_mixture False, True) the oracle's result and the near-tied
    utterances.  Computed once; read-only."""
    case = BY_NAME[name]
    rng = np.random.default_rng(zlib.adler32(name.encode()))
    dicts = ngram_dicts(case, rng)
    lg, lens = logits_of(case, rng), lens_of(case)
    olm = oracle.NGramLM(case.V, sos_of(case), dicts)
    exp, marked = [], []
    for vm in (False, True):
        e = oracle.ctc_prefix_search_lm(lg, case.K, lens, olm, BETA, vm)
        m = np.zeros(case.N, bool) if case.kind in ("tied", "heavy") else near_tied(lg, case.K, lens, olm, vm, e)
        for a in e + (m,):
            a.setflags(write=False)
        exp.append(e)
        marked.append(m)
    lg.setflags(write=False)
    lens.setflags(write=False)
    return Data(lg, lens, dicts, sos_of(case), tuple(exp), tuple(marked))


EXACT = _case("exact_V2_K32_T4", 2, 32, 4, 3)  # every prefix of four frames over two tokens fits the beam (31 at most)


@functools.lru_cache(maxsize=None)
def exact_data():
    """(logits, lens, dicts, sos, per mix and utterance {prefix: mass}) of EXACT, by brute force."""
    rng = np.random.default_rng(zlib.adler32(EXACT.name.encode()))
    dicts = ngram_dicts(EXACT, rng)
    lg, lens = logits_of(EXACT, rng), np.array([4, 3, 2])
    olm = oracle.NGramLM(EXACT.V, sos_of(EXACT), dicts)
    exact = tuple(tuple(brute_force(lg[: lens[n], n], olm, vm) for n in range(EXACT.N)) for vm in (False, True))
    lg.setflags(write=False)
    return lg, lens, dicts, sos_of(EXACT), exact
