"""Inputs of tests/test_beam_forms_gpu.py: BeamSearch at the shapes where its kernels take another form
(csrc/beam_step.hip: the sorted list per prefix with 1, 2, 4 or 8 waves, the flat selection over all K' V
candidates; csrc/beam_search_table.hip: the two instances of the one-launch search, the walk over the trie in
tiles of 256 iterations), batches whose elements finish at different iterations, and tables that send the flat
selection down its two fallbacks -- with their oracle results (oracle.beam_search).  Everything here runs on
the CPU and is computed once per case (``case_data``); nothing is written to after that.
tests/test_beam_forms_cpu.py checks the conditions the inputs have to meet.

Kinds of cases:
  * "lookup": a bigram LookupLanguageModel (sos outside the vocabulary, U = V + 1) under ``M.BeamSearch``, every
    route of tests/test_lm_search_gpu.py's BEAM_ROUTES; the oracle runs around oracle.NGramLM.  Every bigram is
    explicit for V <= 128: with backed-off bigrams two orders of the same tokens sum to the same score up to
    rounding, and a beam that is wide relative to V is then near-tied by construction.
  * "sparse", "uniform", "masked": a dense (V + 1, V) table put straight under the table routes
    (``BeamSearch._bigram_table`` replaced), the oracle around oracle.TableLM.
      sparse   every row -inf except two entries: at width 16 the first three iterations have 2, 4 and 8 finite
               candidates -- the flat selection's threshold is -inf and -inf candidates fill up in flat order;
      sparse_fin  the same with eos the better of the two tokens after sos and finish_all_paths, three iterations:
               an ended path sits in a beam that is short of finite candidates, so its tokens other than eos are
               taken as -inf candidates, in flat order, and the entries they make stay ended (their length does
               not grow: the last token is still eos);
      sparse_end  the same, and the other token after sos is followed by eos alone: after two iterations both
               finite paths have ended, the rest of the beam is -inf continuations of the first ended path,
               which count as ended -- the element is found finished at iteration 2;
      uniform  every row constant with one lower entry, which is -inf: every candidate of every prefix ties
               EXACTLY (a finite lower entry would make the rows' log-sums differ by what the order of a sum
               rounds to), more than 64 survive the threshold and the chunked merge decides, lowest flat index
               first -- in the kernels and in the oracle's sort alike, so these cases are compared exactly too;
      masked   normal rows, a third of each -inf (a vocabulary entry without a unigram).
  * "mixed": batch element n starts from its own row V + n of a (V + N, V) table and then follows row
    ``last token`` (tests/_toy_lm.py: StartRowBigramLM; here: StartRowLM), eos raised by U(0, 0.5 ln V + 1.5) per
    row: the elements finish at different iterations, some never.

Near ties (the method of tests/_lm_forms.py): the oracle is run three more times with every model value times
``1 + u * 4e-7``, ``u ~ U(-1, 1)``; a case whose paths or lengths change in any run is near-tied.  NONE may be:
a marked case gets another salt in the table below (the salts that are not 0 were found that way)."""
import collections
import functools
import math
import zlib

import numpy as np

import _lm_forms
import oracle

RTOL, ATOL = 1e-5, 1e-6  # the bound of tests/test_lm_search_gpu.py for these searches

# step: the kernel of pdt_beam_search_step_table from the second iteration on (K' = W) -- "flat", or "list" + waves;
# dense: the same of pdt_beam_search_step (no rows: never flat); search: the instance of pdt_beam_search_table,
# None where it refuses.  The first iteration (K' = 1) is flat on the table step whenever V > 64, else list1.
# Stated here by hand, checked against the plan functions on the CPU and against what ran on the GPU.
Case = collections.namedtuple("Case", "name kind V W N iters eos fin pad salt bonus step dense search")
Shape = collections.namedtuple("Shape", "V W step dense search")

SHAPES = [
    # rows of at most 64 tokens: never flat, never the one-launch search
    Shape(2, 1, "list1", "list1", None), Shape(2, 5, "list4", "list4", None), Shape(3, 8, "list8", "list8", None),
    Shape(63, 16, "list8", "list8", None), Shape(64, 64, "list8", "list8", None), Shape(64, 8, "list8", "list8", None),
    # V = 65: the first flat V; the waves of the list form (dense routes, PDT_STEP_FLAT=0) at every width class
    Shape(65, 1, "flat", "list1", "rows16"), Shape(65, 2, "flat", "list2", "rows16"), Shape(65, 3, "flat", "list2", "rows16"),
    Shape(65, 5, "flat", "list4", "rows16"), Shape(65, 9, "flat", "list8", "rows16"), Shape(65, 16, "flat", "list8", "rows16"),
    Shape(65, 17, "flat", "list8", "chunks"), Shape(65, 33, "flat", "list8", "chunks"), Shape(65, 64, "flat", "list8", "chunks"),
    # K' ceil(V / 64) against 256
    Shape(128, 64, "flat", "list8", "chunks"), Shape(300, 40, "flat", "list8", "chunks"),
    Shape(1024, 16, "flat", "list8", "rows16"),  # exactly 256
    Shape(1025, 15, "flat", "list8", "chunks"),  # 255; rows beyond 1024 tokens leave ROWS16
    Shape(1025, 16, "list8", "list8", None),  # 272: list form from the second iteration on, flat on the first
    Shape(4095, 4, "flat", "list4", "chunks"),  # exactly 256; the largest V whose dense table stays within 64 MiB
    Shape(4095, 5, "list4", "list4", None), Shape(4095, 1, "flat", "list1", "chunks"),
]
RAW_SHAPES = [Shape(70, 16, "flat", "list8", "rows16"), Shape(130, 16, "flat", "list8", "rows16"),
              Shape(300, 40, "flat", "list8", "chunks"), Shape(1025, 15, "flat", "list8", "chunks"),
              Shape(1025, 16, "list8", "list8", None)]
MIXED_SHAPES = [Shape(9, 4, "list4", "list4", None), Shape(70, 6, "flat", "list4", "rows16"),
                Shape(130, 16, "flat", "list8", "rows16"), Shape(1025, 16, "list8", "list8", None)]
LONG = [(Shape(65, 16, "flat", "list8", "rows16"), 257), (Shape(70, 6, "flat", "list4", "rows16"), 600)]

# (name: salt) of the cases that were near-tied at salt 0; (name: bonus) of the eos cases whose default bonus
# (0.5 ln V + 0.5 on eos after every context) did not stop the search inside its iterations
TUNED = {  # name: (bonus or None, salt)
    "lookup_V2_W1_eos": (0.85, 1), "lookup_V2_W1_fin": (0.85, 2), "lookup_V2_W5_plain": (None, 4),
    "lookup_V2_W5_eos": (0.85, 1), "lookup_V3_W8_plain": (None, 7), "lookup_V3_W8_eos": (1.05, 5),
    "lookup_V64_W64_fin": (3.08, 0), "lookup_V65_W1_fin": (2.59, 4), "lookup_V65_W5_eos": (2.59, 7),
    "lookup_V65_W16_eos": (2.59, 6), "lookup_V65_W33_plain": (None, 1), "lookup_V65_W33_eos": (2.59, 1),
    "lookup_V65_W64_eos": (2.59, 1), "lookup_V65_W64_fin": (3.09, 0), "lookup_V128_W64_eos": (2.93, 1),
    "lookup_V128_W64_fin": (3.43, 0), "lookup_V300_W40_eos": (3.35, 2), "lookup_V300_W40_fin": (3.35, 6),
    "lookup_V1024_W16_fin": (3.97, 6), "lookup_V1025_W15_fin": (3.97, 7), "lookup_V1025_W16_eos": (3.97, 1),
    "lookup_V1025_W16_fin": (3.97, 5), "lookup_V4095_W4_eos": (4.66, 2), "lookup_V4095_W4_fin": (5.66, 7),
    "lookup_V4095_W5_eos": (4.66, 1), "lookup_V4095_W5_fin": (5.66, 4), "lookup_V4095_W1_eos": (5.66, 7),
    "lookup_V4095_W1_fin": (5.16, 1), "lookup_V63_W16_eos_nobatch": (2.57, 1), "masked_V300_W40": (None, 1),
    "mixed_V9_W4_eos": (None, 1), "mixed_V9_W4_fin": (None, 1), "mixed_V70_W6_eos": (None, 1),
}
SALTS = {k: v[1] for k, v in TUNED.items()}
BONUS = {k: v[0] for k, v in TUNED.items() if v[0] is not None}
ITERS = {}  # (name: iterations) of the cases no salt was found for: none


def _lookup(shape, opt, iters=None, N=3, tag=""):
    V, W = shape.V, shape.W
    name = "lookup_V%d_W%d_%s%s" % (V, W, opt, tag)
    if iters is None:
        iters = ITERS.get(name, 6 if W >= 40 else 12)
    eos = None if opt == "plain" else (V - 1) // 2
    pad = {"plain": -7, "eos": -3, "fin": 1}[opt]  # (1: a padding value that is also a token)
    bonus = BONUS.get(name, 0.5 * math.log(V) + 0.5)
    return Case(name, "lookup", V, W, N, iters, eos, opt == "fin", pad, SALTS.get(name, 0), bonus, *shape[2:])


def _raw(shape, kind):
    name = "%s_V%d_W%d" % (kind, shape.V, shape.W)
    iters = 4 if shape.W >= 40 else 6
    eos = None
    if kind in ("sparse_fin", "sparse_end"):  # eos and finish_all_paths while entries without a score are in the beam
        eos, iters = (shape.V - 1) // 2, 3 if kind == "sparse_fin" else 6
    return Case(name, kind, shape.V, shape.W, 2, iters, eos, eos is not None, -7, SALTS.get(name, 0), 0.0, *shape[2:])


def _mixed(shape, fin):
    name = "mixed_V%d_W%d_%s" % (shape.V, shape.W, "fin" if fin else "eos")
    return Case(name, "mixed", shape.V, shape.W, 6, 30, (shape.V - 1) // 2, fin, 1 if fin else -5, SALTS.get(name, 0),
                0.5 * math.log(shape.V) + 1.5, *shape[2:])


# The iteration that finds each element of a mixed batch finished (-1: none), as the oracle has it -- held against
# case_data on the CPU.  Without finish_all_paths an element finishes through its start row only (see _table), so
# the `done` branch runs beside active neighbours from iteration 1 or 2 on to the end, for 28 or 29 iterations, but
# no element STARTS to be finished later than iteration 2; with finish_all_paths the first finishes are spread over
# iterations 3 to 16, and where every element finishes the host's cut at the last of them is reached.
MIXED_FOUND = {
    "mixed_V9_W4_eos": [1, -1, 2, 2, 1, 1], "mixed_V9_W4_fin": [5, -1, -1, 5, 4, -1],
    "mixed_V70_W6_eos": [2, 1, 1, 2, -1, 1], "mixed_V70_W6_fin": [10, 3, 8, 5, 7, 6],
    "mixed_V130_W16_eos": [1, 2, 2, 2, 2, -1], "mixed_V130_W16_fin": [15, 11, 10, 11, 16, 10],
    "mixed_V1025_W16_eos": [-1, 2, 2, 2, 1, 2], "mixed_V1025_W16_fin": [13, 9, 11, 11, 11, 8],
}

CASES = (
    [_lookup(s, opt) for s in SHAPES for opt in ("plain", "eos", "fin")]
    + [_lookup(s, "plain", iters, 2, "_T%d" % iters) for s, iters in LONG]  # the walk's tiles: 256 + 1, 2 * 256 + 88
    + [_lookup(SHAPES[11], "eos", 1, 3, "_T1"), _lookup(SHAPES[11], "fin", 12, None, "_nobatch"),
       _lookup(SHAPES[3], "eos", 12, None, "_nobatch")]
    + [_raw(s, kind) for kind in ("sparse", "sparse_fin", "sparse_end", "uniform", "masked") for s in RAW_SHAPES]
    + [_mixed(s, fin) for s in MIXED_SHAPES for fin in (False, True)]
)
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)
LOOKUP = [c.name for c in CASES if c.kind == "lookup"]
RAW = [c.name for c in CASES if c.kind in ("sparse", "sparse_fin", "sparse_end", "uniform", "masked")]
MIXED = [c.name for c in CASES if c.kind == "mixed"]


class StartRowLM(oracle.TableLM):
    """The numpy twin of tests/_toy_lm.py's StartRowBigramLM: at index 0 batch element n reads row ``starts[n]``
    of the table, afterwards every prefix reads the row of its last token.  No state."""

    def __init__(self, table, starts):
        super().__init__(table)
        self.starts = np.asarray(starts, dtype=np.int64)

    def calc_idx_log_probs(self, hist, prev, idx):
        if int(np.max(idx)) == 0:
            assert hist.shape[1] == self.starts.shape[0]  # (K' = 1: flattened row b is batch element b)
            return self.table[self.starts], prev
        return super().calc_idx_log_probs(hist, prev, idx)


class Jitter:
    """``lm`` with every score times ``1 + u * 4e-7``: u ~ U(-1, 1) per (context, token), the same whenever the
    context comes back.  The context of a row is its last token; at index 0 the row's number in the batch."""

    def __init__(self, lm, seed):
        self.lm, self.seed, self.vocab_size, self._u = lm, seed, lm.vocab_size, {}

    def update_input(self, prev, hist):
        return self.lm.update_input(prev, hist)

    def extract_by_src(self, prev, src):
        return self.lm.extract_by_src(prev, src)

    def calc_idx_log_probs(self, hist, prev, idx):
        out, prev = self.lm.calc_idx_log_probs(hist, prev, idx)
        t = int(np.max(idx))
        keys = [-1 - b for b in range(hist.shape[1])] if t == 0 else [int(v) for v in hist[t - 1]]
        for k in set(keys):
            if k not in self._u:
                self._u[k] = np.random.default_rng([self.seed, k + (1 << 20)]).uniform(-1.0, 1.0, self.vocab_size)
        u = np.stack([self._u[k] for k in keys])
        return (np.asarray(out, np.float64) * (1.0 + u * 4e-7)).astype(np.float32), prev


LmSpec = collections.namedtuple("LmSpec", "V order sos_in kind successors")


def _dicts(case, rng):
    """The n-gram tables of a lookup case (tests/_lm_forms.py: ngram_dicts), eos raised after every context."""
    V = case.V
    dicts = _lm_forms.ngram_dicts(LmSpec(V, 2, False, "peaky", V if V <= 128 else 6), rng)
    if case.eos is not None:
        lp, bo = dicts[0][case.eos]
        dicts[0][case.eos] = (lp + case.bonus, bo)
        for key in dicts[1]:
            if key[1] == case.eos:
                dicts[1][key] += case.bonus
    return dicts


def _table(case, rng):
    V, W = case.V, case.W
    if case.kind.startswith("sparse"):
        table = np.full((V + 1, V), -np.inf, np.float32)
        for r in range(V + 1):
            table[r, rng.choice(V, 2, replace=False)] = rng.normal(size=2)
        if case.eos is not None:  # eos is the best token after sos: a path has ended by the second iteration
            other = int(rng.choice([v for v in range(V) if v != case.eos]))
            table[V] = -np.inf
            table[V, case.eos], table[V, other] = 1.0, 0.0
            if case.kind == "sparse_end":  # and the only token after the other one: every finite path ends at once
                table[other] = -np.inf
                table[other, case.eos] = 0.0
    elif case.kind == "uniform":
        table = np.repeat(rng.normal(size=(V + 1, 1)), V, 1).astype(np.float32)
        table[np.arange(V + 1), (5 * np.arange(V + 1) + 1) % 20] = -np.inf  # (among the first tokens: the winners skip it)
    elif case.kind == "masked":
        table = rng.normal(size=(V + 1, V)).astype(np.float32)
        for r in range(V + 1):
            table[r, rng.choice(V, V // 3, replace=False)] = -np.inf
    else:  # mixed
        table = rng.normal(size=(V + case.N, V)).astype(np.float32)
        table[:, case.eos] += rng.uniform(0.0, case.bonus, V + case.N).astype(np.float32)
        if not case.fin:
            # An element is finished once its FIRST path has ended, and an ended path keeps its score while the
            # others lose a few nats an iteration: with eos likely after every token every element is finished
            # by the third iteration (measured: first padding rows in {1, 2, 3} at every shape).  An element that
            # never finishes needs eos out of reach after the tokens, so here only the N start rows keep the
            # raised eos: it is first at once, enters the beam lower down and rises, or never enters.
            table[:V, case.eos] = -8.0
    return table


def oracle_lm(case, model):
    if case.kind == "lookup":
        return oracle.NGramLM(case.V, case.V, model)
    if case.kind == "mixed":
        return StartRowLM(model, case.V + np.arange(case.N))
    return oracle.TableLM(model)


def run_oracle(case, lm, N="case"):
    return oracle.beam_search(lm, case.W, case.eos, case.fin, case.pad, None, case.N if N == "case" else N, case.iters)


def same(act, exp):
    """Paths inside the lengths and the lengths themselves (tests/_lm_fixtures.py: same_paths)."""
    from _lm_fixtures import same_paths

    return same_paths(act[0], act[1], exp[0], exp[1])


def near_tied(case, model, exp):
    for seed in (0, 1, 2):
        if not same(run_oracle(case, Jitter(oracle_lm(case, model), seed)), exp):
            return True
    return False


def first_pad(case, exp):
    """(N,) the iteration that found each element finished -- the first row of y that is padding for it, where
    y has that row --, -1: none did.  An element is found finished at iteration t when its eos condition holds
    on the beam it enters t with; the beam is frozen from there.  Until then some path has not ended and is as
    long as the iterations run (an ended source offers one candidate, so a beam of ended paths only needs
    every source ended, which includes the first), hence t = the longest path of the final beam -- unless that
    is max_iters, where the search stopped before any iteration could find it."""
    y, lens, _ = exp
    if lens.ndim == 1:
        y, lens = y[:, None], lens[None]
    if case.eos is None:
        return np.full(lens.shape[0], -1)
    out = []
    for n in range(lens.shape[0]):
        ended = [lens[n, k] > 0 and y[lens[n, k] - 1, n, k] == case.eos for k in range(case.W)]
        done = all(ended) if case.fin else ended[0]
        longest = int(lens[n].max())
        out.append(longest if done and longest < case.iters else -1)
    return np.array(out)


Data = collections.namedtuple("Data", "model exp pad_rows marked")


@functools.lru_cache(maxsize=None)
def case_data(name):
    """(the model: n-gram dicts of a lookup case, else the table; the oracle's (y, lens, log-probs); the iteration
    that found every element finished (first_pad); whether the case is near-tied).  Computed once; read-only."""
    return compute(BY_NAME[name])


@functools.lru_cache(maxsize=None)
def short_data(name, iters):
    """(the case cut to ``iters`` iterations, the oracle's result): a sparse table's beam is full of finite paths
    from the iteration with 2^t >= W on, and what the entries without a score were no longer shows -- the
    first three iterations are compared on their own."""
    case = BY_NAME[name]._replace(iters=iters)
    exp = run_oracle(case, oracle_lm(case, case_data(name).model))
    for a in exp:
        a.setflags(write=False)
    return case, exp


def compute(case):
    name = case.name
    rng = np.random.default_rng([zlib.adler32(name.encode()), case.salt])
    model = _dicts(case, rng) if case.kind == "lookup" else _table(case, rng)
    exp = run_oracle(case, oracle_lm(case, model))
    marked = False if case.kind == "uniform" else near_tied(case, model, exp)
    pads = first_pad(case, exp)
    for a in exp + (pads,) + (() if case.kind == "lookup" else (model,)):
        a.setflags(write=False)
    return Data(model, exp, pads, marked)
