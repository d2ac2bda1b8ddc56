"""CPU: pad_masked_sequence, chunk_by_slices, chunk_token_sequences_by_slices, slice_spect_data and their
Modules without a GPU -- the reference's signatures, constructor validation, error types, the torch bodies
against the goldens (tests/golden/chunk.npz, captured from the reference), scripting and tracing, and the
argument checks of the C entry points.

What the goldens compare (tests/golden/make_chunk_golden.py): integers and copied values exactly;
``chunked[n, :chunk_lens[n]]`` only for chunk_by_slices (beyond it the package holds ``value``, the reference
whatever its padding left); float64 gradients to 1e-12 relative (sums of a handful of copied terms)."""
import inspect
import json
import os

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
FUNCTIONS = ("pad_masked_sequence", "chunk_by_slices", "chunk_token_sequences_by_slices", "slice_spect_data")
MODULES = ("PadMaskedSequence", "ChunkBySlices", "ChunkTokenSequencesBySlices", "SliceSpectData")
EXC = {"RuntimeError": RuntimeError, "ValueError": ValueError, "NotImplementedError": NotImplementedError,
       "IndexError": IndexError}  # fmt: skip


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLD, "chunk.npz"))


def upstream(shape, dtype):
    n = int(np.prod(shape))
    return torch.cos(torch.arange(n, dtype=torch.float64) * 0.7).reshape(shape).to(dtype)


def head(y, yl):
    m = torch.arange(y.shape[1], device=y.device).unsqueeze(0) < yl.unsqueeze(1)
    return m.view(m.shape + (1,) * (y.dim() - 2))


def opt(gold, key, device="cpu"):
    return torch.from_numpy(gold[key]).to(device) if key in gold else None


def error_cases(F_, M_, device="cpu"):
    """The table of tests/golden/make_chunk_golden.py:error_cases."""
    x = torch.arange(12.0, device=device).view(2, 6)
    sl = torch.tensor([[-3, 2], [0, 8]]).to(device)
    refs = torch.zeros((2, 4, 3), dtype=torch.long, device=device)

    def t(v):
        return torch.tensor(v).to(device)

    return {
        "chunk_ndim": lambda: F_.chunk_by_slices(torch.zeros(3, device=device), sl),
        "chunk_lens_shape": lambda: F_.chunk_by_slices(x, sl, t([3])),
        "chunk_mode": lambda: F_.chunk_by_slices(x, sl, None, "circular"),
        "chunk_reflect_pad": lambda: F_.chunk_by_slices(x, sl, t([2, 6]), "reflect"),
        "chunk_replicate_len": lambda: F_.chunk_by_slices(x, sl, t([0, 6]), "replicate"),
        "masked_ndim": lambda: F_.pad_masked_sequence(torch.zeros(3, device=device), torch.ones(3, 1, dtype=torch.bool, device=device)),
        "masked_mask_ndim": lambda: F_.pad_masked_sequence(x, torch.ones(2, dtype=torch.bool, device=device)),
        "masked_mask_dtype": lambda: F_.pad_masked_sequence(x, torch.ones(2, 6, dtype=torch.long, device=device), True),
        "masked_mask_shape": lambda: F_.pad_masked_sequence(x, torch.ones(2, 5, dtype=torch.bool, device=device), True),
        "tokens_shape": lambda: F_.chunk_token_sequences_by_slices(torch.zeros((2, 4, 2), dtype=torch.long, device=device), sl),
        "tokens_slices_shape": lambda: F_.chunk_token_sequences_by_slices(refs, sl[:1]),
        "tokens_lens_shape": lambda: F_.chunk_token_sequences_by_slices(refs, sl, t([1])),
        "slice_ndim": lambda: F_.slice_spect_data(torch.zeros(3, device=device)),
        "slice_lobe": lambda: F_.slice_spect_data(x, lobe_size=-1),
        "slice_window": lambda: F_.slice_spect_data(x, window_type="casual"),
        "slice_policy": lambda: F_.slice_spect_data(x, policy="other"),
        "slice_in_lens_shape": lambda: F_.slice_spect_data(x, t([1])),
        "slice_ali_ndim": lambda: F_.slice_spect_data(refs, policy="ali"),
        "slice_ref_ndim": lambda: F_.slice_spect_data(x, policy="ref"),
        "slice_ref_size": lambda: F_.slice_spect_data(torch.zeros((2, 4, 2), dtype=torch.long, device=device), policy="ref"),
        "slice_other_lens_shape": lambda: F_.slice_spect_data(refs, None, t([1]), "ref"),
        "ctor_chunk_mode": lambda: M_.ChunkBySlices("circular"),
        "ctor_masked_batch_first": lambda: M_.PadMaskedSequence(1),
        "ctor_tokens_partial": lambda: M_.ChunkTokenSequencesBySlices(partial=1),
        "ctor_slice_policy": lambda: M_.SliceSpectData("other"),
        "ctor_slice_window": lambda: M_.SliceSpectData(window_type="casual"),
        "ctor_slice_lobe": lambda: M_.SliceSpectData(lobe_size=-1),
    }


def check_errors(gold, F_, M_, device="cpu"):
    names = json.loads(str(gold["errors"]))
    cases = error_cases(F_, M_, device)
    assert sorted(names) == sorted(cases)
    for key, fn in cases.items():
        assert names[key] != "none", key
        with pytest.raises(EXC[names[key]]):
            fn()


def check_chunk_goldens(gold, F_, device="cpu"):
    for k in range(int(gold["chunk_n"])):
        pre = "chunk_{}_".format(k)
        kw = json.loads(str(gold[pre + "kw"]))
        x = torch.from_numpy(gold[pre + "x"]).to(device).requires_grad_(True)
        y, yl = F_.chunk_by_slices(x, opt(gold, pre + "slices", device), opt(gold, pre + "lens", device), kw["mode"], kw["value"])
        exp, exp_l = torch.from_numpy(gold[pre + "y"]).to(device), torch.from_numpy(gold[pre + "ylens"]).to(device)
        assert y.shape == exp.shape and torch.equal(yl, exp_l) and yl.dtype == exp_l.dtype, (k, kw)
        keep = head(y, yl).expand_as(y)
        assert torch.equal(y[keep], exp[keep]), (k, kw)
        assert bool((y[~keep] == kw["value"]).all()), (k, kw)
        (gx,) = torch.autograd.grad(y, x, upstream(tuple(y.shape), x.dtype).to(device) * keep.to(x.dtype))
        gexp = torch.from_numpy(gold[pre + "gx"]).to(device)
        assert float((gx - gexp).abs().max()) <= 1e-12 * max(1.0, float(gexp.abs().max())), (k, kw)
    for n in (0, 3):
        shape = tuple(int(v) for v in gold["chunk_empty_{}_shape".format(n)])
        y, yl = F_.chunk_by_slices(torch.zeros(shape, device=device), torch.zeros((n, 2), dtype=torch.long, device=device))
        assert tuple(y.shape) == shape and np.array_equal(yl.cpu().numpy(), gold["chunk_empty_{}_ylens".format(n)])


def check_masked_goldens(gold, F_, device="cpu"):
    for k in range(int(gold["masked_n"])):
        pre = "masked_{}_".format(k)
        kw = json.loads(str(gold[pre + "kw"]))
        x = torch.from_numpy(gold[pre + "x"]).to(device)
        has_grad = pre + "gx" in gold
        x.requires_grad_(has_grad)
        y, yl = F_.pad_masked_sequence(x, torch.from_numpy(gold[pre + "mask"]).to(device), **kw)
        assert y.dtype == x.dtype and np.array_equal(y.detach().cpu().numpy(), gold[pre + "y"]), (k, kw)
        assert yl.dtype == torch.long and np.array_equal(yl.cpu().numpy(), gold[pre + "ylens"]), (k, kw)
        if has_grad:
            (gx,) = torch.autograd.grad(y, x, upstream(tuple(y.shape), x.dtype).to(device))
            assert np.abs(gx.cpu().numpy() - gold[pre + "gx"]).max() <= 1e-12, (k, kw)


def check_token_goldens(gold, F_, device="cpu"):
    for k in range(int(gold["tokens_n"])):
        pre = "tokens_{}_".format(k)
        kw = json.loads(str(gold[pre + "kw"]))
        y, yl = F_.chunk_token_sequences_by_slices(
            opt(gold, pre + "refs", device), opt(gold, pre + "slices", device), opt(gold, pre + "lens", device),
            kw["partial"], kw["retain"],
        )  # fmt: skip
        # (the stored y is the reference's with zeros beyond chunked_lens: the tail here is zero)
        assert np.array_equal(yl.cpu().numpy(), gold[pre + "ylens"]), (k, kw)
        assert y.dtype == torch.long and np.array_equal(y.cpu().numpy(), gold[pre + "y"]), (k, kw)
    y, yl = F_.chunk_token_sequences_by_slices(
        torch.zeros((3, 4), dtype=torch.long, device=device), torch.zeros((3, 2), dtype=torch.long, device=device)
    )
    shapes = gold["tokens_2d_shapes"]
    assert list(y.shape) == list(shapes[0][:2]) and list(yl.shape) == list(shapes[1][:1])


def check_slice_goldens(gold, F_, device="cpu"):
    for k in range(int(gold["slice_n"])):
        pre = "slice_{}_".format(k)
        kw = json.loads(str(gold[pre + "kw"]))
        kw.pop("defined")
        slices, sources = F_.slice_spect_data(
            opt(gold, pre + "input", device), opt(gold, pre + "in_lens", device), opt(gold, pre + "other_lens", device), **kw
        )
        assert slices.dtype == torch.long and sources.dtype == torch.long
        assert np.array_equal(slices.cpu().numpy(), gold[pre + "slices"]), (k, kw)
        assert np.array_equal(sources.cpu().numpy(), gold[pre + "sources"]), (k, kw)
    slices, sources = F_.slice_spect_data(torch.zeros((2, 0), device=device))
    assert list(slices.shape) == list(gold["slice_t0_shapes"][0]) and sources.shape == (0,)


def _params(fn):
    return [[p.name, p.default is not inspect.Parameter.empty, p.kind.name,
             repr(p.default) if p.default is not inspect.Parameter.empty else None]
            for p in inspect.signature(fn).parameters.values() if p.name != "self"]  # fmt: skip


def test_names_exported_and_signatures_match_reference():
    from pydrobert_amd import functional as F
    from pydrobert_amd import modules as M

    sig = json.load(open(os.path.join(GOLD, "chunk_signatures.json")))
    assert sorted(sig["functional"]) == sorted(FUNCTIONS) and sorted(sig["modules"]) == sorted(MODULES)
    for name, exp in sig["functional"].items():
        assert name in F.__all__ and _params(getattr(F, name)) == exp, name
    for name, exp in sig["modules"].items():
        cls = getattr(M, name)
        assert name in M.__all__
        assert _params(cls.__init__) == exp["__init__"], name
        assert _params(cls.forward) == exp["forward"], name
        assert list(cls.__constants__) == exp["__constants__"], name


def test_error_types_and_constructors(gold):
    from pydrobert_amd import functional as F
    from pydrobert_amd import modules as M

    check_errors(gold, F, M)
    reprs = json.loads(str(gold["reprs"]))
    ours = {
        "ChunkBySlices": [repr(M.ChunkBySlices()), repr(M.ChunkBySlices("reflect"))],
        "PadMaskedSequence": [repr(M.PadMaskedSequence(True, -1.0))],
        "SliceSpectData": [repr(M.SliceSpectData("ali", "causal", False, 3))],
        "ChunkTokenSequencesBySlices": [repr(M.ChunkTokenSequencesBySlices(p, r)) for p in (False, True) for r in (False, True)],
    }
    assert ours == reprs


def test_chunk_by_slices_cpu_body_matches_goldens(gold):
    from pydrobert_amd import functional as F

    assert int(gold["chunk_discarded"]) == 0 and int(gold["chunk_n"]) == 108
    check_chunk_goldens(gold, F)


def test_pad_masked_sequence_cpu_body_matches_goldens(gold):
    from pydrobert_amd import functional as F

    check_masked_goldens(gold, F)


def test_chunk_token_sequences_cpu_body_matches_goldens(gold):
    from pydrobert_amd import functional as F

    check_token_goldens(gold, F)


def test_slice_spect_data_cpu_body_matches_goldens(gold):
    from pydrobert_amd import functional as F

    assert int(gold["slice_n"]) == 3 * 2 * 4 * 9
    check_slice_goldens(gold, F)


def test_chunk_by_slices_replicate_start_past_the_end():
    """A non-empty slice that starts at or after the sequence end replicates the row's OWN last step (the
    reference's row carries a value of another batch element there)."""
    from pydrobert_amd import functional as F

    x = torch.arange(12.0).view(3, 4)
    y, yl = F.chunk_by_slices(x, torch.tensor([[5, 7], [0, 2], [3, 6]]), torch.tensor([2, 4, 4]), "replicate")
    assert yl.tolist() == [2, 2, 3] and y.shape == (3, 5)  # (T' is the largest right pad, 7 - 2)
    assert y[0].tolist() == [1.0, 1.0, 0.0, 0.0, 0.0] and y[1, :2].tolist() == [4.0, 5.0]
    assert y[2].tolist() == [11.0, 11.0, 11.0, 0.0, 0.0]


def test_modules_script_and_trace_cpu():
    from pydrobert_amd import modules as M

    x = torch.randn(3, 11, 4)
    mask = torch.rand(3, 11) < 0.5
    slices = torch.tensor([[-2, 5], [3, 14], [4, 4]])
    lens = torch.tensor([11, 9, 5])
    refs = torch.randint(0, 12, (3, 6, 3))
    refs[..., 2] = refs[..., 1] + 2
    ali = torch.randint(0, 3, (3, 11))
    cases = (
        (M.PadMaskedSequence(True, -1.0), (x, mask)),
        (M.PadMaskedSequence(), (x.transpose(0, 1), mask.t())),
        (M.ChunkBySlices("replicate"), (x, slices, lens)),
        (M.ChunkBySlices("constant", 2.0), (x, slices)),
        (M.ChunkTokenSequencesBySlices(True, True), (refs, slices, torch.tensor([6, 3, 0]))),
        (M.SliceSpectData("ali", "symmetric", False, 1), (ali, lens)),
        (M.SliceSpectData("fixed", "causal", True, 2), (x, lens)),
        (M.SliceSpectData("ref"), (refs, None, lens)),
    )
    for mod, args in cases:
        exp = mod(*args)
        got = torch.jit.script(mod)(*args)
        assert all(torch.equal(a, b) for a, b in zip(got, exp)), mod
        if all(a is not None for a in args):
            got = torch.jit.trace(mod, args)(*args)
            assert all(torch.equal(a, b) for a, b in zip(got, exp)), mod


def test_ops_registered_and_entry_points_validate():
    """The entry points check their arguments and return early for empty shapes before any launch, so these
    calls are safe without a GPU."""
    import __graft_entry__ as g
    import pydrobert_amd.functional  # noqa: F401
    from pydrobert_amd import _cabi

    for op in ("pad_masked_sequence", "pad_masked_sequence_backward", "chunk_by_slices", "chunk_by_slices_backward",
               "chunk_token_sequences_by_slices", "slice_spect_data"):  # fmt: skip
        assert hasattr(torch.ops.pydrobert_amd, op)
    if not os.path.exists(_cabi.LIB_PATH):
        g.build()
    lib = _cabi.lib()
    OK, ARG = _cabi.PDT_OK, _cabi.PDT_E_ARG
    assert lib.pdt_compact_mask(0, 0, 4, 4, 1, 0, 0, 4, 1, 0, 0) == OK  # N == 0
    assert lib.pdt_compact_mask(0, 2, 4, 4, 1, 0, 0, 4, 1, 0, 0) == ARG  # null pointers
    assert lib.pdt_compact_mask(0, -1, 4, 4, 1, 0, 0, 4, 1, 0, 0) == ARG
    assert lib.pdt_gather_steps(0, 2, 4, 0, 4, 4, 1, 0, 4, 1, 4, 0, 0, 0, 0) == OK  # F == 0
    assert lib.pdt_gather_steps(0, 2, 4, 3, 4, 12, 3, 0, 4, 1, 4, 0, 0, 0, 0) == ARG
    assert lib.pdt_chunk_by_slices(0, 0, 4, 3, 4, 12, 3, 0, 0, 0, 0, 5, 0, 0) == OK  # N == 0
    assert lib.pdt_chunk_by_slices(0, 2, 4, 3, 4, 12, 3, 0, 0, 0, 0, 0, 0, 0) == OK  # T' == 0
    assert lib.pdt_chunk_by_slices(0, 2, 4, 3, 4, 12, 3, 0, 0, 0, 0, 5, 0, 0) == ARG  # null pointers
    assert lib.pdt_chunk_by_slices(0, 2, 4, 3, 4, 12, 3, 0, 0, 7, 0, 5, 0, 0) == ARG  # bad mode
    assert lib.pdt_chunk_by_slices_backward(0, 0, 2, 0, 3, 0, 0, 0, 5, 0, 0) == OK  # T == 0
    assert lib.pdt_chunk_by_slices_backward(0, 2, 2, 4, 3, 0, 0, 0, 5, 0, 0) == ARG  # bad dtype
    assert lib.pdt_chunk_by_slices_backward(0, 0, 2, 4, 3, 0, 0, 0, 5, 0, 0) == ARG  # null pointers
    assert lib.pdt_chunk_stats(0, 0, 0, 4, 0, 0, 0) == OK  # N == 0
    assert lib.pdt_chunk_stats(0, 0, 2, 4, 0, 0, 0) == ARG  # null pointers
    assert lib.pdt_chunk_stats(0, 0, 2, -1, 0, 0, 0) == ARG
    assert lib.pdt_chunk_tokens(0, 0, 5, 0, 0, 0, 0, 0, 0, 0) == OK
    assert lib.pdt_chunk_tokens(0, 2, 5, 0, 0, 0, 0, 0, 0, 0) == ARG
    assert lib.pdt_slice_fixed(3, 0, 0, 0, 1, 1, 0, 0, 1, 0, 0, 0, 0) == OK  # no candidates
    assert lib.pdt_slice_fixed(3, 4, 0, 0, 0, 1, 0, 0, 1, 0, 0, 0, 0) == ARG  # shift < 1
    assert lib.pdt_slice_fixed(3, 4, 0, 0, 1, 1, 0, 0, 1, 0, 0, 0, 0) == ARG  # null pointers
    assert lib.pdt_slice_ref(0, 0, 4, 0, 0, 0, 0, 1, 0, 0, 0, 0, 0, 0) == OK
    assert lib.pdt_slice_ref(0, 2, 4, 0, 0, 0, 0, 1, 0, 0, 0, 0, 0, 0) == ARG
    assert lib.pdt_slice_ali_segments(0, 2, 0, 0, 0, 0, 0) == OK  # T == 0
    assert lib.pdt_slice_ali_segments(0, 2, 4, 0, 0, 0, 0) == ARG
    assert lib.pdt_slice_ali_emit(0, 0, 4, 0, 0, 0, 0, 1, 1, 0, 0, 0, 0) == OK
    assert lib.pdt_slice_ali_emit(0, 2, 4, 0, 0, 0, 0, 1, 1, 0, 0, 0, 0) == ARG
    assert lib.pdt_slice_ali_emit(0, 2, 4, 0, 0, 0, 0, -1, 1, 0, 0, 0, 0) == ARG
