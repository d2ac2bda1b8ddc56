"""GPU: every kernel that reads through caller-chosen element strides, with one stride of 2^32 + A elements.

The inputs are views of one large, never-filled buffer (tests/_wide.py): slice 1 of the wide dimension
lies beyond 2^32 elements, and where a 32-bit wrap of its offsets lands there are decoys -- other values
of the same kind -- so a dropped ``(int64_t)`` cast, a stride narrowed to ``int`` or a product formed in
``int`` gives a wrong answer for slice 1 instead of passing.  Shapes are the smallest the family's own
form tests use; references and tolerances are those tests' (oracle.*, the float64 yardsticks, exact where
they are exact).  The layouts come from ``_wide.LAYOUTS`` and are checked on the CPU by
tests/test_wide_offsets_cpu.py.
"""
import warnings

import numpy as np
import pytest
import torch

import _loss_ref as LR
import _wide as W
import oracle
from pydrobert_amd import functional as F
from pydrobert_amd import modules as M

pytestmark = pytest.mark.gpu
DEV = "cuda"


class _Buffers:
    """One uninitialised buffer of MIN_NUMEL elements at a time: 16 GiB for 4-byte elements, 32 GiB for
    8-byte ones.  Asking for the other width frees the first before it allocates."""

    def __init__(self):
        self.buf, self.itemsize = None, 0

    def get(self, dtype):
        size = 8 if torch.empty((), dtype=dtype).element_size() == 8 else 4
        if self.itemsize != size:
            self.release()
            base = torch.int64 if size == 8 else torch.int32
            try:
                self.buf = torch.empty(W.MIN_NUMEL, dtype=base, device=DEV)
            except torch.cuda.OutOfMemoryError as e:
                pytest.skip("no room for the {} GiB buffer: {}".format(W.MIN_NUMEL * size >> 30, e))
            self.itemsize = size
        return self.buf if self.buf.dtype == dtype else self.buf.view(dtype)

    def release(self):
        if self.buf is not None:
            self.buf = None
            self.itemsize = 0
            torch.cuda.empty_cache()


@pytest.fixture(scope="module")
def buffers():
    b = _Buffers()
    yield b
    b.release()


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _wv(buffers, name, values, seed=0):
    values = values if torch.is_tensor(values) else torch.from_numpy(np.array(values))
    view = W.wide_case(buffers.get(values.dtype), name, values, seed)
    dim = W.LAYOUTS[name][2]
    assert view.stride(dim) > W.WRAP and view.shape == values.shape
    return view


def _same(a, b):
    for x, y in zip(a, b):
        assert torch.equal(x, y)


# ---- ctc_greedy_search ---------------------------------------------------------------------------
@pytest.mark.parametrize("dim", ["sn", "st"])
@pytest.mark.parametrize("V", [65, 1100])
def test_ctc_greedy_search(buffers, V, dim):
    """Row forms of csrc/row_reduce.hpp on both sides of 1024 tokens, as test_ctc_greedy_search_strided_logits;
    the batch stride wide (utterance 1 beyond 2^32) and the frame stride wide (frame 1).  ``paths`` is dense."""
    name = "greedy_%s_V%d" % (dim, V)
    Tn, N, _ = W.LAYOUTS[name][1]
    rng = np.random.default_rng(V)
    lg = rng.normal(size=(Tn, N, V)).astype(np.float32) * 3
    lens = np.array([7, Tn]) if dim == "sn" else np.array([2, 1, 2])
    x = _wv(buffers, name, lg)
    for is_probs in (False, True):
        e_max, e_paths, e_lens = oracle.ctc_greedy_search(lg, lens, V - 1, False, is_probs)
        a_max, a_paths, a_lens = (o.cpu().numpy() for o in F.ctc_greedy_search(x, _t(lens), V - 1, False, is_probs))
        wrong = [
            n for n in range(N)
            if not (a_lens[n] == e_lens[n] and np.array_equal(a_paths[:, n], e_paths[:, n])
                    and np.allclose(a_max[n], e_max[n], rtol=2e-5, atol=1e-3))
        ]  # fmt: skip
        assert not wrong, ("utterances with a wrong result", wrong, is_probs)


# ---- ctc_prefix_search ---------------------------------------------------------------------------
from test_decoding_gpu import (  # noqa: E402  (the family's own inputs and comparisons)
    _check_search, _cmp_beam_step, _cmp_ctc_step, _ctc_frame_inputs, _ctc_plan, _ctc_state, _peaky_logits,
)


def _ctc_lens(dim, T, N):
    return np.array([T - 2, T]) if dim == "sn" else np.array([2, 1, 2, 2, 0][:N])


@pytest.mark.parametrize("dim", ["sn", "st"])
@pytest.mark.parametrize(
    "form,V,K,rowreg",
    [("general", 70, 16, 1), ("rowreg", 513, 16, 1), ("lds_ring", 513, 16, 0), ("wide_beam", 70, 40, 1)],
)
def test_ctc_prefix_search(buffers, switch, form, V, K, rowreg, dim):
    """The one-producer kernel of ctc_search.hip (rows in registers, V < 320), long rows in the producers'
    registers (ctc_rowreg.hip) and in the LDS ring of three producers (PDT_CTC_ROWREG=0), and the
    workgroup kernel for beams beyond 32 (ctc_search_wide.hip): utterance 1, or frame 1, beyond 2^32."""
    switch("PDT_CTC_ROWREG", rowreg)
    rc, plan = _ctc_plan(V, min(K, 32))
    assert rc == 0 and (plan[3] == 3) == (form == "rowreg"), plan
    name = "ctc_%s_V%d" % (dim, V)
    T, N, _ = W.LAYOUTS[name][1]
    rng = np.random.default_rng(100 * V + K)
    lg = _peaky_logits(rng, T, N, V, scale=3.0 if K > 32 else (11.0 if V > 500 else 8.0))
    for lens in (None, _ctc_lens(dim, T, N)):
        exp = oracle.ctc_prefix_search(lg, K, lens)
        x = _wv(buffers, name, lg)
        tl = None if lens is None else _t(lens)
        act = F.ctc_prefix_search(x, K, tl)
        _check_search(act, exp, (form, dim, lens is None))


def test_ctc_prefix_search_default_shape_instance(buffers):
    """V = 256, W = 16 with contiguous utterances (lg_sn == 257): the instance of ctc_search.hip with the
    sizes as constants, two frames per producer pass, the steady tiers at their defaults.  Only the frame
    stride is free there: frame 1 lies beyond 2^32.  Same bits as the general kernel (a vocabulary axis
    with a stride) and the oracle's beams, as test_ctc_default_shape_instances_match_the_general_kernels."""
    T, N, Vp1 = W.LAYOUTS["ctc_default_st"][1]
    rng = np.random.default_rng(256)
    lg = _peaky_logits(rng, T, N, Vp1 - 1, scale=6.0)
    lens = np.array([2, 1, 2])
    x = _wv(buffers, "ctc_default_st", lg)
    assert x.stride(1) == 257 and x.stride(2) == 1
    for tl, ln in ((None, None), (_t(lens), lens)):
        act = F.ctc_prefix_search(x, 16, tl)
        _check_search(act, oracle.ctc_prefix_search(lg, 16, ln), ("default shape", ln is None))
        general = torch.zeros((T, N, 2 * Vp1), device=DEV)
        general[:, :, ::2] = _t(lg)
        _same(act, F.ctc_prefix_search(general[:, :, ::2], 16, tl))
        _same(act, F.ctc_prefix_search(x.contiguous(), 16, tl))


# ---- the searches with an n-gram model in the loop -----------------------------------------------
@pytest.mark.parametrize("dim", ["sn", "st"])
@pytest.mark.parametrize("route", ["table", "search"])
def test_ctc_prefix_search_with_a_lookup_lm(buffers, switch, route, dim):
    """The factor-table search (csrc/ctc_lm_table.hip: the logits, softmax fused) and the lookup-model
    search (csrc/ctc_lm_step.hip: the probabilities) at V = 65, K = 32 of tests/_lm_forms.py, against
    oracle.ctc_prefix_search_lm with the comparison of tests/test_lm_search_forms_gpu.py."""
    import _lm_forms as forms
    from test_lm_search_forms_gpu import ROUTES, _check, _search_and_its_route

    case, data = forms.BY_NAME["inst_V65_K32"], forms.case_data("inst_V65_K32")
    for sw, value in ROUTES[route].items():
        switch(sw, value)
    name = "ctc_lm_" + dim
    T, N, _ = W.LAYOUTS[name][1]
    lg = np.ascontiguousarray(data.lg[:T, :N])
    lens = np.array([T - 1, T]) if dim == "sn" else _ctc_lens(dim, T, N)
    olm = oracle.NGramLM(case.V, data.sos, data.dicts)
    lm = M.LookupLanguageModel(case.V, data.sos, [d.copy() for d in data.dicts]).to(DEV)
    for vm in (False, True):
        exp = oracle.ctc_prefix_search_lm(lg, case.K, lens, olm, forms.BETA, vm)
        marked = forms.near_tied(lg, case.K, lens, olm, vm, exp)
        beyond = np.array([False, True]) if dim == "sn" else lens == 2  # utterances that read beyond 2^32
        assert (~marked[beyond]).any(), "an utterance that reads beyond 2^32 must be compared exactly"
        search = M.CTCPrefixSearch(case.K, forms.BETA, lm, valid_mixture=vm)
        if route == "table":
            act, ran = _search_and_its_route(search, _wv(buffers, name, lg), _t(lens))
            assert ran == "_lm_table_search", ran
        else:  # (the module forms the probabilities with torch; the search reads them through their strides)
            probs = _wv(buffers, name, _t(lg).softmax(2).cpu())
            assert search._searches_from_one_call()
            with torch.no_grad():
                act = tuple(o.cpu().numpy() for o in search._lookup_lm_search(probs, _t(lens), int(lens.max())))
            exp = tuple(e[: int(lens.max())] if i == 0 else e for i, e in enumerate(exp))
        _check(act, exp, marked, ("wide " + dim, route, vm), False)


# ---- step operators ------------------------------------------------------------------------------
@pytest.mark.parametrize("Kp", [1, 9, 17])
def test_ctc_prefix_search_advance(buffers, Kp):
    """One wave per element (K' = 1) and eight waves in two and three rounds (K' = 9, 17), as
    test_ctc_prefix_search_advance_waves_per_element: the extension probabilities (N, K', V) with
    element 1 beyond 2^32."""
    rng = np.random.default_rng(9000 + Kp)
    N, V = 2, 70
    y, last, lens, (nb, b), isp = _ctc_state(rng, N, V, Kp)
    ext, nonext, blank = _ctc_frame_inputs(rng, N, V, Kp)
    exp = oracle.ctc_prefix_search_advance((ext, nonext, blank), Kp, (nb, b), y, last, lens, isp)
    x = _wv(buffers, "step_ext_Kp%d" % Kp, ext)
    rest = ((_t(nb), _t(b)), _t(y), _t(last), _t(lens), _t(isp))
    act = F.ctc_prefix_search_advance((x, _t(nonext), _t(blank)), Kp, *rest)
    _cmp_ctc_step(act, exp, Kp)


@pytest.mark.parametrize("Kp,flat", [(1, 0), (9, 0), (17, 0), (3, 1)])
def test_beam_search_advance(buffers, switch, Kp, flat):
    """The sorted-list form with one wave and with eight in two and three rounds (PDT_STEP_FLAT=0) and the
    one selection over all K' V candidates (the default for rows of 65 .. tokens): scores (N, K', V) with
    element 1 beyond 2^32, against the oracle as test_beam_search_advance_waves_per_element."""
    switch("PDT_STEP_FLAT", flat)
    rng = np.random.default_rng(9200 + Kp)
    N, V, W, S = 2, 70, 11, 4
    lpt = np.log(rng.dirichlet(np.ones(V), (N, Kp))).astype(np.float32)
    lpp = rng.normal(size=(N, Kp)).astype(np.float32)
    yp = rng.integers(0, V, (S, N, Kp))
    ypl = rng.integers(0, S + 1, (N, Kp))
    exp = oracle.beam_search_advance(lpt, W, lpp, yp, ypl)
    x = _wv(buffers, "step_ext_Kp%d" % Kp, lpt)
    act = F.beam_search_advance(x, W, _t(lpp), _t(yp), _t(ypl))
    _cmp_beam_step(act, exp, min(W, Kp * V), (Kp, flat))


@pytest.mark.parametrize("V", [64, 1000])
def test_random_walk_advance(buffers, V):
    """One wave per walk, rows of one and of sixteen 64-token chunks: log_probs_t (N, V) with walk 1 beyond
    2^32; tokens exact against the float64 rule of tests/test_random_walk_gpu.py."""
    from test_random_walk_gpu import _choose, _expected_y, _rows, rule

    rng = np.random.default_rng(V)
    N, S = 2, 3
    x = _rows(rng, 4, V)[[0, 2]]  # a plain row and one with -inf entries
    tok, u = _choose(rng, x)
    assert [rule(x[n], u[n]) for n in range(N)] == tok.tolist()
    lpp = _t(rng.normal(size=N).astype(np.float32))
    y_prev, lens = rng.integers(0, V, (S, N)), np.array([S, 1])
    lpt = _wv(buffers, "walk_V%d" % V, x)
    y, lp = torch.ops.pydrobert_amd.random_walk_advance(lpt, _t(u), lpp, _t(y_prev), _t(lens))
    assert np.array_equal(y.cpu().numpy(), _expected_y(y_prev, lens, tok))
    assert torch.equal(lp, lpp + _t(x).gather(1, _t(tok).unsqueeze(1)).squeeze(1))


# ---- hard-OCD loss -------------------------------------------------------------------------------
@pytest.mark.parametrize("V", [65, 1100])
def test_hard_ocd_loss(buffers, V):
    """Rows in registers and streamed rows (csrc/ocd_loss.hip), forward and backward, logits (H, N, V) with
    utterance 1 beyond 2^32: the float64 set form of tests/_loss_ref.py, as test_hocd_strided_logits."""
    rng = np.random.default_rng(V)
    H, N, R = 5, 2, 7
    ref = rng.integers(0, V, (R, N))
    ref[:3, 1] = (0, 64, V - 1)
    hyp = rng.integers(0, V, (H, N))
    logits = rng.normal(size=(H, N, V)).astype(np.float32) * 3
    Mult, _ = LR.oracle_multiplicity(ref, hyp, V)
    x64 = torch.from_numpy(logits).double().requires_grad_(True)
    le, _ = LR.set_loss(x64, Mult)
    gw = torch.from_numpy(rng.normal(size=tuple(le.shape)))
    (ge,) = torch.autograd.grad((le * gw).sum(), x64)
    x = _wv(buffers, "ocd_V%d" % V, logits).requires_grad_(True)
    la = F.hard_optimal_completion_distillation_loss(x, _t(ref), _t(hyp), reduction="none", warn=False)
    (ga,) = torch.autograd.grad((la * gw.float().to(DEV)).sum(), x)
    for n in range(N):
        ok, worst = LR.close(la[:, n], le[:, n], LR.loss_tol(V))
        assert ok, ("loss of utterance", n, worst)
        ok, worst = LR.close(ga[:, n], ge[:, n], LR.GRAD_TOL)
        assert ok, ("gradient of utterance", n, worst)
    for red in ("mean", "sum"):
        exp = oracle.hard_optimal_completion_distillation_loss(logits, ref, hyp, reduction=red)
        act = F.hard_optimal_completion_distillation_loss(x, _t(ref), _t(hyp), reduction=red, warn=False)
        ok, worst = LR.close(act, exp, LR.loss_tol(V))
        assert ok, (red, worst)


# ---- estimators ----------------------------------------------------------------------------------
MC_SHAPES = [("columns", 7, 2, 1, 0), ("wave", 65, 2, 1, 1), ("wide_sm", 2, 65, 0, 0)]  # (form, M, B, wide dim, plan)


def _mc_reduce_case(buffers, monkeypatch, dtype, form, k):
    """``f`` (M, B) with a wide column stride -- the lane-per-column form (M = 7) and the wave-per-column form
    (M = 65), column 1 beyond 2^32 -- and with a wide sample stride (M = 2): value and gradients against the
    float64 yardstick with the tolerances of tests/test_estimators_gpu.py."""
    import test_estimators_gpu as EG
    from pydrobert_amd import _cabi

    _, M, B, dim, plan = next(s for s in MC_SHAPES if s[0] == form)
    tag = "f32" if dtype == torch.float32 else "f64"
    name = "mat_%s_%dx%d_d%d" % (tag, M, B, dim)
    kind, mode, present = EG.CONFIGS[k]
    seen = []

    def wide(f, layout):
        v = _wv(buffers, name, f)
        seen.append(_cabi.lib().pdt_mc_reduce_plan(M, B, v.stride(0), v.stride(1)))
        return v

    monkeypatch.setattr(EG, "lay_out", wide)
    gen = torch.Generator().manual_seed(1000 * kind + 10 * mode + M)
    for is_log in (False, True):
        T = EG.draw(gen, present, M, (B,), dtype)
        EG.compare(kind, is_log, mode, T, dtype, "wide", "{} {} wide {}".format(EG.OPS[kind], form, is_log))
    assert seen == [plan, plan], seen


@pytest.mark.parametrize("k", [0, 4, 5], ids=["MEAN", "SCORE", "WEIGHTED"])
@pytest.mark.parametrize("form", [s[0] for s in MC_SHAPES])
def test_mc_reduce_float32(buffers, monkeypatch, form, k):
    _mc_reduce_case(buffers, monkeypatch, torch.float32, form, k)


def _imh_case(buffers, dtype):
    """``ratio`` (M, B) with column 1 beyond 2^32: exact against the loop of tests/_estimators_ref.py."""
    import _estimators_ref as ref
    from pydrobert_amd import _estimators

    gen = torch.Generator().manual_seed(11)
    M, B = 65, 2
    ratio = torch.randn((M, B), generator=gen).to(dtype)
    ratio0 = torch.randn((B,), generator=gen).to(dtype)
    log_u = torch.rand((M, B), generator=gen).log().to(dtype)
    ratio[torch.rand((M, B), generator=gen) < 0.15] = -float("inf")
    want = ref.imh_loop(ratio, ratio0, log_u)
    assert (want[0][:, 1] >= 0).any()
    r = _wv(buffers, "mat_%s_65x2_d1" % ("f32" if dtype == torch.float32 else "f64"), ratio)
    got = _estimators.imh_chain(r, ratio0.to(DEV), log_u.to(DEV))
    for a, b, what in zip(got, want, ("idx", "last", "last_idx")):
        assert torch.equal(a.cpu(), b), what


def test_imh_chain_float32(buffers):
    _imh_case(buffers, torch.float32)


# ---- returns -------------------------------------------------------------------------------------
def _return_case(buffers, dtype):
    """``r`` (T, N) with sequence 1 beyond 2^32, time-major and batch-major, both scan directions: the bound
    of tests/test_rl_comb_gpu.py's sweep."""
    from test_rl_comb_gpu import op, reference, within

    tag = "f32" if dtype == torch.float32 else "f64"
    x64 = torch.randn(65, 2, dtype=torch.float64)
    for reverse in (False, True):
        R64, unit = reference(x64, 0.999, reverse)
        got = op(_wv(buffers, "mat_%s_65x2_d1" % tag, x64.to(dtype)), 0.999, False, reverse)
        assert got.shape == (65, 2) and within(got.cpu(), R64, unit, dtype), ("time major", reverse)
        got = op(_wv(buffers, "mat_%s_2x65_d0" % tag, x64.T.contiguous().to(dtype)), 0.999, True, reverse)
        assert got.shape == (2, 65) and within(got.T.cpu(), R64, unit, dtype), ("batch major", reverse)


def test_time_distributed_return_float32(buffers):
    _return_case(buffers, torch.float32)


# ---- compaction and chunking ---------------------------------------------------------------------
@pytest.mark.parametrize("batch_first", [True, False])
@pytest.mark.parametrize("Fdim", [8, 3], ids=["words", "elements"])
def test_pad_masked_sequence(buffers, Fdim, batch_first):
    """Rows moved as 16-byte words (F = 8 float32) and element by element (F = 3), ``x`` and then the mask
    with sequence 1 beyond 2^32: the same elements as the torch body on the CPU, as tests/test_chunk_gpu.py."""
    T_, N = 37, 2
    x = torch.randn((N, T_, Fdim) if batch_first else (T_, N, Fdim))
    mask = torch.rand((N, T_) if batch_first else (T_, N)) < 0.6
    want, want_lens = F.pad_masked_sequence(x, mask, batch_first, -1.0)
    names = ("seq_2x37x%d_d0" % Fdim, "mask_2x37_d0") if batch_first else ("seq_37x2x%d_d1" % Fdim, "mask_37x2_d1")
    for which in ("x", "mask"):
        xd = _wv(buffers, names[0], x) if which == "x" else x.to(DEV)
        md = _wv(buffers, names[1], mask) if which == "mask" else mask.to(DEV)
        got, got_lens = F.pad_masked_sequence(xd, md, batch_first, -1.0)
        assert torch.equal(got_lens.cpu(), want_lens), which
        assert torch.equal(got.cpu(), want), which


@pytest.mark.parametrize("mode", ["constant", "reflect", "replicate"])
@pytest.mark.parametrize("Fdim", [8, 3], ids=["words", "elements"])
def test_chunk_by_slices(buffers, Fdim, mode):
    """``x`` (N, T, F) with sequence 1 beyond 2^32, both copy widths, every padding rule: the torch body."""
    x = torch.randn((2, 37, Fdim))
    slices = torch.tensor([[-3, 20], [5, 41]])
    lens = torch.tensor([30, 37])
    want, want_lens = F.chunk_by_slices(x, slices, lens, mode, 0.5)
    got, got_lens = F.chunk_by_slices(_wv(buffers, "seq_2x37x%d_d0" % Fdim, x), slices.to(DEV), lens.to(DEV), mode, 0.5)
    assert torch.equal(got_lens.cpu(), want_lens) and torch.equal(got.cpu(), want)


# ---- SpecAugment and the relaxed samplers --------------------------------------------------------
@pytest.mark.parametrize("freq,Fq", [(True, 10), (False, 12)], ids=["grids", "one_launch_warp"])
def test_spec_augment_apply_parameters(buffers, freq, Fq):
    """Features (N, T, F) with utterance 1 beyond 2^32 through the general kernel (time and frequency grids)
    and through the one-launch time-warp kernel (F a multiple of 4): the oracle on the valid frames, as
    tests/test_img_gpu.py."""
    from test_img_gpu import ATOL, _draw

    rng = np.random.default_rng(10 + freq)
    N, T_, order = 2, 50, 2
    feats = rng.normal(size=(N, T_, Fq)).astype(np.float32)
    lens = np.array([37, 50])
    params = _draw(rng, N, T_, Fq, lens.astype(np.float64), freq=freq)
    exp = oracle.spec_augment_apply_parameters(feats, params, order, lens)
    x = _wv(buffers, "spec_2x50x%d_d0" % Fq, feats)
    act = F.spec_augment_apply_parameters(x, tuple(_t(p) for p in params), order, _t(lens)).cpu().numpy()
    valid = np.arange(T_)[None, :, None] < lens[:, None, None]
    err = (np.abs(exp - act) * valid).max((1, 2))
    assert (err < ATOL).all(), err


def _relaxed_case(buffers, family, dtype):
    """The parameter rows (B, V) of the relaxed samplers with row 1 beyond 2^32.  The distributions normalise
    their parameters into a dense tensor, so a caller's strides reach the kernels only from the operator
    itself: rsample, log_prob (logits) and csample (probabilities) there, against the host's torch body in
    float64 with the tolerances of tests/test_distributions_gpu.py."""
    import _distributions_check as C
    import _distributions_ref as ref
    from pydrobert_amd import _relaxed as RX

    tag = "f32" if dtype == torch.float32 else "f64"
    fam = RX.GUMBEL if family == "gumbel" else RX.BERNOULLI
    eps = float(torch.finfo(dtype).eps)
    gen = torch.Generator().manual_seed(11)
    values = (2 * torch.randn((2, 70), generator=gen)).to(dtype)
    u = (torch.rand((3, 2, 70), generator=gen) * 0.96 + 0.02).to(dtype)
    logits = _wv(buffers, "mat_%s_2x70_d0" % tag, values)
    z64 = RX._TORCH[fam](RX.RSAMPLE, values.double(), u.double(), None)
    z = torch.ops.pydrobert_amd.relaxed(fam, RX.RSAMPLE, logits, u.to(DEV), None)
    assert ref.units(z, z64, eps) <= C.tolerance(family, "z", "float" + tag[1:])
    z_in = z64.to(dtype)
    lp = torch.ops.pydrobert_amd.relaxed(fam, RX.LOG_PROB, logits, z_in.to(DEV), None)
    lp64 = RX._TORCH[fam](RX.LOG_PROB, values.double(), z_in.double(), None)
    assert ref.units(lp, lp64, eps) <= C.tolerance(family, "log_prob", "float" + tag[1:])
    # csample reads probabilities (Gumbel: any positive scale), b the threshold of z
    pv = values.softmax(-1) * 3 if family == "gumbel" else values.sigmoid()
    v = (torch.rand((3, 2, 70), generator=gen) * 0.96 + 0.02).to(dtype)
    b = RX._TORCH[fam](RX.THRESHOLD, None, z_in, None)
    zc = torch.ops.pydrobert_amd.relaxed(fam, RX.CSAMPLE, _wv(buffers, "mat_%s_2x70_d0" % tag, pv), b.to(DEV), v.to(DEV))
    zc64 = RX._TORCH[fam](RX.CSAMPLE, pv.double(), b.double(), v.double())
    assert ref.units(zc, zc64, eps) <= C.tolerance(family, "zcond", "float" + tag[1:])


@pytest.mark.parametrize("family", ["gumbel", "bernoulli"])
def test_relaxed_samplers_float32(buffers, family):
    _relaxed_case(buffers, family, torch.float32)


# ---- feature deltas and soft attention -----------------------------------------------------------
@pytest.mark.parametrize("mode", ["replicate", "constant"])
def test_feat_deltas(buffers, mode):
    """x (N, T, D) = (2, 40, 260), the float32 vector form with two column tiles, utterance 1 beyond 2^32
    through the collapsed outermost stride: forward and gradient as tests/test_feats_gpu.py checks them."""
    import _feats_ref as R
    from test_feats_gpu import _check_deltas

    x = _wv(buffers, "feat_2x40x260_d0", R.delta_input((2, 40, 260), "float32"))
    _check_deltas(x, dict(order=2, width=2), mode)


@pytest.mark.parametrize("which", ["query", "key", "value"])
def test_dot_product_attention(buffers, which):
    """The stride lists of the attention descriptor: the query (N, K, D), then the key, then the value
    (T, N, 1, D) with batch element 1 beyond 2^32; output and the three gradients against the float64
    formula with the tolerances of test_long_and_wide_against_formula."""
    from test_attn_gpu import reference_formula

    torch.manual_seed(40)
    T_, D, N, K = 40, 16, 2, 3
    m = M.DotProductSoftAttention(D, 0, D ** -0.5)
    vals = dict(query=torch.randn(N, K, D), key=torch.randn(T_, N, 1, D), value=torch.randn(T_, N, 1, D))
    name = "attn_q_2x3x16_d0" if which == "query" else "attn_kv_40x2x1x16_d1"
    on = {n: (_wv(buffers, name, t) if n == which else t.to(DEV)).requires_grad_(True) for n, t in vals.items()}
    lens = torch.tensor([T_ // 3 + 1, T_], device=DEV)
    mask = torch.arange(T_, device=DEV).view(T_, 1, 1) < lens.view(1, N, 1)
    y = m(on["query"], on["key"], on["value"], mask)
    g = torch.randn_like(y)
    grads = torch.autograd.grad(y, tuple(on.values()), g)
    d64 = [t.double().to(DEV).requires_grad_(True) for t in vals.values()]
    y64 = reference_formula(m, *d64, mask)
    assert torch.allclose(y.double(), y64, rtol=1e-4, atol=1e-5), (y.double() - y64).abs().max()
    for a, b in zip(grads, torch.autograd.grad(y64, d64, g.double())):
        assert torch.allclose(a.double(), b, rtol=1e-3, atol=1e-4), (a.double() - b).abs().max()


# ---- dense tensors just over 2^31 elements -------------------------------------------------------
# The inputs start at element 2^31 of the buffer (W.dense_at_2_31) and are filled on the device; the
# operators allocate their outputs.  What was read before these ran, for the index each output is stored
# through: csrc/seq_ops.hip:150-158 (row * (int64_t)V), csrc/ocd_loss.hip:67, 120 (int64 row, row *
# (int64_t)V), csrc/mc_reduce.hip:138-143, 252-255 (int64 column / element index), csrc/relaxed.hip:124-131
# (int64 r, r * V), csrc/pad_variable.hip:54-63 and csrc/seq_chunk.hip:245-250, 289-292 (unsigned gid below
# 2^32 - 4096, zero-extended).  The uint8 cases of pad_variable and chunk_by_slices read a 16-step input (no
# offset near 2^31 on that side) and allocate it with torch; pad_masked_sequence's input is as long as its
# output and lies in the buffer.
def _filled(buffers, name, gen_seed, scale=3.0):
    x = W.dense_case(buffers.get(W.DENSE[name][0]), name)
    x.normal_(generator=torch.Generator(DEV).manual_seed(gen_seed)).mul_(scale)
    return x


def test_dense_sequence_log_probs(buffers):
    """(T, N, V) = (512, 4096, 1025): 2^31 + 2 M elements.  16 sequences -- those whose last steps' rows lie on
    both sides of element 2^31 among them -- forward and backward against float64, with the tolerances of
    test_sequence_ops_row_forms."""
    Tn, N, V = W.DENSE["slp_logits"][1]
    x = _filled(buffers, "slp_logits", 1).requires_grad_(True)
    hyp = torch.randint(0, V - 1, (Tn, N), device=DEV, generator=torch.Generator(DEV).manual_seed(2))
    eos = V - 1
    rows = W.rows_around(Tn * N, V)
    seqs = sorted({r % N for r in rows})
    hyp[Tn // 2, seqs[1]] = eos
    act = F.sequence_log_probs(x, hyp, 0, eos)
    (ga,) = torch.autograd.grad(act.sum(), x)
    sel = torch.tensor(seqs, device=DEV)
    xc = x.detach()[:, sel].double().cpu().requires_grad_(True)
    h = hyp[:, sel].cpu()
    first = torch.where((h == eos).any(0), (h == eos).long().argmax(0), torch.tensor(Tn)) + 1
    mask = torch.arange(Tn).unsqueeze(1) >= first.unsqueeze(0)
    ref = xc.log_softmax(-1).gather(-1, h.unsqueeze(-1)).squeeze(-1).masked_fill(mask, 0.0).sum(0)
    (ge,) = torch.autograd.grad(ref.sum(), xc)
    assert torch.allclose(act.detach()[sel].cpu().double(), ref.detach(), rtol=2e-5, atol=1e-4)
    assert torch.allclose(ga[:, sel].cpu().double(), ge, rtol=1e-4, atol=1e-5)
    assert ga[Tn // 2 + 1 :, seqs[1]].eq(0).all()  # (steps after the eos: zero rows)


def test_dense_hard_ocd_loss_backward(buffers):
    """(H, N, V) = (8, 262144, 1025): the gradient of the logits' size, 2^31 + 2 M elements, allocated by the
    operator.  16 utterances, those of the rows around element 2^31 among them, against the float64 set form."""
    H, N, V = W.DENSE["ocd_logits"][1]
    x = _filled(buffers, "ocd_logits", 3).requires_grad_(True)
    g = torch.Generator(DEV).manual_seed(4)
    ref_t = torch.randint(0, V, (6, N), device=DEV, generator=g)
    hyp_t = torch.randint(0, V, (H, N), device=DEV, generator=g)
    utts = sorted({r % N for r in W.rows_around(H * N, V)})
    la = F.hard_optimal_completion_distillation_loss(x, ref_t, hyp_t, reduction="none", warn=False)
    gw = torch.randn((H, N), device=DEV, generator=g)
    (ga,) = torch.autograd.grad((la * gw).sum(), x)
    sel = torch.tensor(utts, device=DEV)
    Mult, _ = LR.oracle_multiplicity(ref_t[:, sel].cpu().numpy(), hyp_t[:, sel].cpu().numpy(), V)
    x64 = x.detach()[:, sel].double().cpu().requires_grad_(True)
    le, _ = LR.set_loss(x64, Mult)
    (ge,) = torch.autograd.grad((le * gw[:, sel].double().cpu()).sum(), x64)
    ok, worst = LR.close(la[:, sel], le, LR.loss_tol(V))
    assert ok, worst
    ok, worst = LR.close(ga[:, sel], ge, LR.GRAD_TOL)
    assert ok, worst


def test_dense_mc_reduce_mean_in_log_space(buffers):
    """f (M, B) = (64, 2^25 + 2^14), 2^31 + 2^20 elements: MEAN in log space, forward and backward, on 16
    columns -- column 0, those whose last sample lies on either side of element 2^31, the last -- against
    the float64 yardstick with the tolerances of tests/test_estimators_gpu.py."""
    import _estimators_ref as ref
    import test_estimators_gpu as EG

    M, B = W.DENSE["mc_f"][1]
    f = _filled(buffers, "mc_f", 5, 2.0).requires_grad_(True)
    edge = W.HALF - (M - 1) * B
    cols = {0, edge - 1, edge, edge + 1, B - 1}
    rng = np.random.default_rng(6)
    while len(cols) < 16:
        cols.add(int(rng.integers(0, B)))
    sel = torch.tensor(sorted(cols), device=DEV)
    v = EG.X().mc_reduce(ref.MEAN, True, f)
    gup = torch.randn((B,), device=DEV, generator=torch.Generator(DEV).manual_seed(7))
    (gf,) = torch.autograd.grad(v, f, gup)
    f64 = f.detach()[:, sel].double().cpu().requires_grad_(True)
    want = ref.reduce64(ref.MEAN, True, 0, torch.float32, f=f64)
    (gw,) = torch.autograd.grad(want, f64, gup[sel].double().cpu())
    eps = float(torch.finfo(torch.float32).eps)
    assert ref.units(v[sel], want, eps) <= EG.op_tolerance(ref.MEAN, "v", torch.float32)
    assert ref.units(gf[:, sel], gw, eps) <= EG.op_tolerance(ref.MEAN, "g", torch.float32)


def test_dense_relaxed_gumbel_rsample(buffers):
    """Logits (B, V) = (2095200, 1025), B V over 2^31: rsample on 16 rows, the rows around element 2^31 among
    them, against the host's torch body in float64 with the tolerance of tests/test_distributions_gpu.py."""
    import _distributions_check as C
    import _distributions_ref as ref
    from pydrobert_amd import _relaxed as RX

    Bn, V = W.DENSE["gumbel_logits"][1]
    logits = _filled(buffers, "gumbel_logits", 8, 2.0)
    u = torch.rand((Bn, V), device=DEV, generator=torch.Generator(DEV).manual_seed(9)).mul_(0.96).add_(0.02)
    z = torch.ops.pydrobert_amd.relaxed(RX.GUMBEL, RX.RSAMPLE, logits, u, None)
    sel = torch.tensor(W.rows_around(Bn, V), device=DEV)
    want = RX._TORCH[RX.GUMBEL](RX.RSAMPLE, logits[sel].double().cpu(), u[sel].double().cpu(), None)
    assert ref.units(z[sel], want, float(torch.finfo(torch.float32).eps)) <= C.tolerance("gumbel", "z", "float32")


ROW, GUARD, STEPS_MAX = W.ROW, W.GUARD, W.STEPS_MAX  # 1023-byte steps: the copies move single bytes
STEPS_OVER = STEPS_MAX + 1  # one step over the guard
AT_2_31 = W.HALF // ROW  # the step that holds byte 2^31


def _bytes(shape, seed):
    return torch.randint(0, 256, shape, dtype=torch.uint8, device=DEV, generator=torch.Generator(DEV).manual_seed(seed))


def test_uint8_pad_variable_beyond_2_31():
    """The longest output the kernel takes, just under 2^32 bytes, whose data rows straddle byte 2^31
    (replicated edges on both sides): every row against plain indexing on the device; one step more is
    refused before the launch."""
    x = _bytes((1, 16, ROW), 1)
    left = AT_2_31 - 8
    lens = torch.tensor([16], device=DEV)
    pad = torch.tensor([[left], [STEPS_MAX - left - 16]], device=DEV)
    out = F.pad_variable(x, lens, pad, "replicate")
    assert out.shape == (1, STEPS_MAX, ROW) and W.HALF < out.numel() < GUARD
    assert torch.equal(out[0, left : left + 16], x[0])
    assert (out[0, :left] == x[0, 0]).all() and (out[0, left + 16 :] == x[0, 15]).all()
    del out
    pad = torch.tensor([[left], [STEPS_OVER - left - 16]], device=DEV)
    with pytest.raises(RuntimeError, match="too long"):
        F.pad_variable(x, lens, pad, "replicate")


def test_uint8_chunk_by_slices_beyond_2_31():
    """One chunk of just under 2^32 bytes that runs far beyond its sequence (replicate: the last step repeated
    up to and beyond byte 2^31); one step more is refused before the launch."""
    x = _bytes((1, 16, ROW), 2)
    lens = torch.tensor([16], device=DEV)
    out, n = F.chunk_by_slices(x, torch.tensor([[0, STEPS_MAX]], device=DEV), lens, "replicate")
    assert out.shape == (1, STEPS_MAX, ROW) and W.HALF < out.numel() < GUARD and n.tolist() == [STEPS_MAX]
    assert torch.equal(out[0, :16], x[0]) and (out[0, 16:] == x[0, 15]).all()
    del out
    with pytest.raises(RuntimeError, match="too long"):
        F.chunk_by_slices(x, torch.tensor([[0, STEPS_OVER]], device=DEV), lens, "replicate")


def test_uint8_pad_masked_sequence_beyond_2_31(buffers):
    """Two sequences of just under 2^31 bytes each, in and out: sequence 1's steps lie beyond byte 2^31 of an
    input that starts at byte 2^31 of the buffer (a sign-wrapped source offset would stay inside it); every
    row against boolean indexing on the device.  One step more per sequence is refused before the copy."""
    T_ = STEPS_MAX // 2
    x = W.dense_case(buffers.get(torch.uint8), "u8_masked")
    x.random_(0, 256, generator=torch.Generator(DEV).manual_seed(3))
    mask = torch.rand((2, T_), device=DEV, generator=torch.Generator(DEV).manual_seed(4)) < 0.7
    out, lens = F.pad_masked_sequence(x, mask, True, 9.0)
    assert W.HALF < out.numel() < GUARD and torch.equal(lens, mask.sum(1))
    for n in range(2):
        k = int(lens[n])
        assert torch.equal(out[n, :k], x[n][mask[n]]) and (out[n, k:] == 9).all()
    del out
    big = W.dense_at_2_31(buffers.get(torch.uint8), (2, T_ + 1, ROW))
    assert big.numel() >= GUARD
    with pytest.raises(RuntimeError, match="too long"):
        F.pad_masked_sequence(big, torch.ones((2, T_ + 1), dtype=torch.bool, device=DEV), True, 9.0)


# ---- string operators (int64 tokens: the 32 GiB buffer; keep these behind the float32 cases) -----
LEV = ["error_rate", "edit_distance", "prefix_error_rates", "prefix_edit_distances"]
COST_FLAVOURS = ["edit_distance", "prefix_edit_distances"]
# route of pdt_lev / pdt_oc_mask (csrc/pdt_api.hip) -> (operators that reach it, R, H, costs, switches)
STRING_ROUTES = {
    "bitpar_fused": (LEV, 150, 137, (1.0, 1.0, 1.0), {}),
    "bitpar_two_launches": (LEV, 150, 600, (1.0, 1.0, 1.0), {}),
    "skewed": (LEV, 150, 137, (3.0, 3.0, 4.0), {}),
    "rowsync_exact": (COST_FLAVOURS, 150, 137, (0.1, 0.7, 1.3), {}),
    "workgroup": (COST_FLAVOURS, 2049, 29, (0.1, 0.7, 1.3), {}),
    "oc_bitpar": (["optimal_completion"], 150, 137, (1.0, 1.0, 1.0), {"PDT_OC_BITPAR": 1}),
    "oc_rowsync": (["optimal_completion"], 150, 137, (1.0, 1.0, 1.0), {"PDT_OC_BITPAR": 0}),
    "oc_workgroup": (["optimal_completion"], 2049, 29, (1.0, 1.0, 1.0), {}),
}
STRING_CASES = [(route, name) for route, spec in STRING_ROUTES.items() for name in spec[0]]


@pytest.mark.parametrize("route,name", STRING_CASES)
def test_string_operators(buffers, switch, route, name):
    """Every route of pdt_lev and pdt_oc_mask, the wide batch stride on ``ref`` and on ``hyp`` in turn, both
    ``batch_first`` layouts; utterance 1's tokens lie beyond 2^32.  Exact, as tests/test_string_gpu.py."""
    _, R, H, costs, switches_ = STRING_ROUTES[route]
    for sw, value in switches_.items():
        switch(sw, value)
    if route.startswith("bitpar"):
        from pydrobert_amd import _cabi

        assert _cabi.lib().pdt_lev_workspace_bytes(R, H, 2) > 0  # (0: the cell-by-cell kernels would run)
    rng = np.random.default_rng(R + H)
    V, eos = 5, 5
    ref, hyp = rng.integers(0, V, (R, 2)), rng.integers(0, V, (H, 2))
    ref[R - 9, 0], hyp[H - 3, 0], hyp[H - 1, 1] = eos, eos, eos  # (utterance 1: the whole reference)
    kw = dict(eos=eos, ins_cost=costs[0], del_cost=costs[1], sub_cost=costs[2])
    for batch_first in (False, True):
        r, h = (ref.T.copy(), hyp.T.copy()) if batch_first else (ref, hyp)
        exp = getattr(oracle, name)(r, h, batch_first=batch_first, **kw)
        for which in ("ref", "hyp"):
            L = R if which == "ref" else H
            w = _wv(buffers, ("tok_bf_L%d" if batch_first else "tok_L%d") % L, r if which == "ref" else h)
            args = (w, _t(h)) if which == "ref" else (_t(r), w)
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                act = getattr(F, name)(*args, warn=False, batch_first=batch_first, **kw).cpu().numpy()
            assert exp.shape == act.shape and exp.dtype == act.dtype, (route, name, which, batch_first)
            bad = np.argwhere(~((exp == act) | (np.isnan(exp) & np.isnan(act)))) if exp.dtype.kind == "f" else np.argwhere(exp != act)
            assert not len(bad), (route, name, which, batch_first, bad[:5])


# ---- float64: the same 32 GiB buffer as the tokens ------------------------------------------------
@pytest.mark.parametrize("k", [0, 4, 5], ids=["MEAN", "SCORE", "WEIGHTED"])
@pytest.mark.parametrize("form", [s[0] for s in MC_SHAPES])
def test_mc_reduce_float64(buffers, monkeypatch, form, k):
    _mc_reduce_case(buffers, monkeypatch, torch.float64, form, k)


def test_imh_chain_float64(buffers):
    _imh_case(buffers, torch.float64)


def test_time_distributed_return_float64(buffers):
    _return_case(buffers, torch.float64)


@pytest.mark.parametrize("family", ["gumbel", "bernoulli"])
def test_relaxed_samplers_float64(buffers, family):
    _relaxed_case(buffers, family, torch.float64)
