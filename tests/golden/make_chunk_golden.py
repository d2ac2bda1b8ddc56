#!/usr/bin/env python
"""Generate tests/golden/chunk.npz and chunk_signatures.json from the LIVE reference's pad_masked_sequence,
chunk_by_slices, chunk_token_sequences_by_slices and slice_spect_data (and their Modules).

Run where the reference is installed (it never travels to the GPU machine):

    PDT_REFERENCE=<reference checkout> python tests/golden/make_chunk_golden.py

Every array is DATA: inputs this script draws and what the reference returned for them.  Case k of a
family stores its arrays under ``<family>_<k>_<name>`` and its arguments as a JSON string under
``<family>_<k>_kw``; error cases store the reference's exception type name.

chunk_by_slices: the stored outputs are the reference's; the script also restates the rule the package
follows (``rule`` below) and FAILS unless it equals the reference on every stored case, over
``chunked[n, :chunk_len[n]]``, the shape and ``chunk_lens``.  For replicate the draws are restricted to
non-empty slices with ``start < len`` (beyond that the reference's rows carry values of other batch
elements) and pads of at most ``T`` steps (beyond that the reference raises); ``chunk_discarded`` stores
how many draws a reference exception threw away AFTER the drawing rule was applied -- it must be 0.

slice_spect_data, where the reference raises: policy 'ali' for a row with in_lens[n] == T (in_lens=None
included) is captured as the reference's result on the input with one column appended and in_lens passed
explicitly; policy 'ref' with other_lens=None as the reference's result with the end of each row's last
triple passed explicitly.  Those cases carry ``"defined": true`` in their kw.
"""
import inspect
import itertools
import json
import os
import sys
import warnings

import numpy as np
import torch

REF = os.environ.get("PDT_REFERENCE", "/root/reference")
sys.path.insert(0, os.path.join(REF, "src"))
HERE = os.path.dirname(os.path.abspath(__file__))

import pydrobert.torch.functional as RF  # noqa: E402
import pydrobert.torch.modules as RM  # noqa: E402

warnings.simplefilter("ignore")
rng = np.random.default_rng(0xC4A27)
out = {}


def put(key, v):
    if isinstance(v, torch.Tensor):
        v = v.detach().cpu().numpy()
    out[key] = np.asarray(v)


def upstream(shape, dtype):
    """The fixed upstream gradient of every case (tests/test_chunk_*.py restate it)."""
    n = int(np.prod(shape))
    return torch.cos(torch.arange(n, dtype=torch.float64) * 0.7).reshape(shape).to(dtype)


def rule(x, slices, lens, mode, value):
    """chunk_by_slices as the package defines it, in loops."""
    N, T = x.shape[:2]
    chunk = np.maximum(slices[:, 1] - slices[:, 0], 0)
    rows = []
    for n in range(N):
        ln = T if lens is None else int(lens[n])
        row = []
        for t in range(int(chunk[n])):
            s = int(slices[n, 0]) + t
            if s < 0:
                s = -s if mode == "reflect" else 0 if mode == "replicate" else -1
            elif s >= ln:
                s = 2 * (ln - 1) - s if mode == "reflect" else ln - 1 if mode == "replicate" else -1
            row.append(x[n, s] if 0 <= s < ln else np.full(x.shape[2:], value, x.dtype))
        rows.append(row)
    return rows, chunk


def chunks():
    k = discarded = 0
    for mode, with_lens, rest, rep in itertools.product(
        ("constant", "reflect", "replicate"), (False, True), ((), (3,), (2, 2)), range(6)
    ):
        N, T = int(rng.integers(1, 5)), int(rng.integers(1, 9))
        lens = rng.integers(1, T + 1, N) if with_lens else None
        ln = lens if with_lens else np.full(N, T)
        if mode == "constant":  # anything from -T to 3T, empty and reversed slices included
            start = rng.integers(-T, 3 * T, N)
            end = start + rng.integers(-2, 2 * T, N)
        elif mode == "reflect":  # pads below the length (beyond that the reference raises)
            start = rng.integers(-(ln - 1), 2 * ln - 1)
            end = np.minimum(start + rng.integers(-1, 2 * T, N), 2 * ln - 1)
        else:  # replicate: non-empty, start < len, pads of at most T (the reference raises beyond: its pad
            # masks have T columns)
            start = rng.integers(-T, ln)
            end = np.minimum(start + rng.integers(1, 2 * T, N), ln + T)
        slices = np.stack([start, end], 1).astype(np.int64)
        x = torch.from_numpy(rng.standard_normal((N, T) + rest)).requires_grad_(True)
        tl = None if lens is None else torch.from_numpy(lens)
        try:
            y, yl = RF.chunk_by_slices(x, torch.from_numpy(slices), tl, mode, 0.25)
        except Exception:  # noqa: BLE001
            discarded += 1
            continue
        rows, chunk = rule(x.detach().numpy(), slices, lens, mode, 0.25)
        assert np.array_equal(yl.numpy(), chunk), (mode, slices, lens)
        left = np.where(chunk > 0, np.maximum(-slices[:, 0], 0), 0)
        right = np.where(chunk > 0, np.maximum(slices[:, 1] - ln, 0), 0)
        assert y.shape[1] == max(left.max(), chunk.max(), right.max())
        for n in range(N):
            got = y.detach().numpy()[n, : chunk[n]]
            assert np.array_equal(got, np.asarray(rows[n]).reshape(got.shape)), (mode, n, slices, lens)
        (gx,) = torch.autograd.grad(y, x, upstream(tuple(y.shape), x.dtype) * _head(y, yl))
        pre = "chunk_{}_".format(k)
        put(pre + "kw", json.dumps(dict(mode=mode, value=0.25, lens=with_lens)))
        put(pre + "x", x)
        put(pre + "slices", slices)
        if with_lens:
            put(pre + "lens", lens)
        put(pre + "y", y)
        put(pre + "ylens", yl)
        put(pre + "gx", gx)
        k += 1
    # N * T == 0
    for shape in ((0, 4, 2), (3, 0)):
        x = torch.zeros(shape)
        y, yl = RF.chunk_by_slices(x, torch.zeros((shape[0], 2), dtype=torch.long))
        put("chunk_empty_{}_shape".format(shape[0]), np.array(y.shape))
        put("chunk_empty_{}_ylens".format(shape[0]), yl)
    put("chunk_n", k)
    put("chunk_discarded", discarded)
    assert discarded == 0, discarded


def _head(y, yl):
    """1 on chunked[n, :chunk_len[n]], 0 beyond (what lies there is not part of the contract)."""
    m = torch.arange(y.shape[1]).unsqueeze(0) < yl.unsqueeze(1)
    return m.view(m.shape + (1,) * (y.dim() - 2)).to(y.dtype)


def masked():
    k = 0
    for dt, batch_first, rest in itertools.product(("int64", "float32", "float64", "bool"), (False, True), ((), (3,), (2, 2))):
        N, T = 5, 7
        shape = ((N, T) if batch_first else (T, N)) + rest
        x = torch.from_numpy(rng.standard_normal(shape) * 4)
        x = (x > 0) if dt == "bool" else x.to(getattr(torch, dt))
        mask = torch.from_numpy(rng.random((N, T)) < 0.5)
        mask[0], mask[1] = True, False  # an all-true and an all-false row
        if not batch_first:
            mask = mask.t()
        if x.is_floating_point():
            x.requires_grad_(True)
        y, yl = RF.pad_masked_sequence(x, mask, batch_first, 1.0)
        pre = "masked_{}_".format(k)
        put(pre + "kw", json.dumps(dict(batch_first=batch_first, padding_value=1.0)))
        put(pre + "x", x)
        put(pre + "mask", mask)
        put(pre + "y", y)
        put(pre + "ylens", yl)
        if dt == "float64":
            put(pre + "gx", torch.autograd.grad(y, x, upstream(tuple(y.shape), x.dtype))[0])
        k += 1
    put("masked_n", k)


def tokens():
    k = 0
    for partial, retain, with_lens, rep in itertools.product((False, True), (False, True), (False, True), range(3)):
        N, R = 4, 9
        tok = rng.integers(0, 20, (N, R))
        start = rng.integers(-2, 12, (N, R))
        end = start + rng.integers(-2, 6, (N, R))  # negative boundaries and end < start included
        refs = np.stack([tok, start, end], 2).astype(np.int64)
        s0 = rng.integers(-3, 8, N)
        slices = np.stack([s0, s0 + rng.integers(0, 10, N)], 1).astype(np.int64)
        lens = rng.integers(0, R + 1, N) if with_lens else None
        y, yl = RF.chunk_token_sequences_by_slices(
            torch.from_numpy(refs), torch.from_numpy(slices), None if lens is None else torch.from_numpy(lens),
            partial, retain,
        )  # fmt: skip
        head = (np.arange(R)[None] < yl.numpy()[:, None])[..., None]
        pre = "tokens_{}_".format(k)
        put(pre + "kw", json.dumps(dict(partial=partial, retain=retain, lens=with_lens)))
        put(pre + "refs", refs)
        put(pre + "slices", slices)
        if with_lens:
            put(pre + "lens", lens)
        put(pre + "y", np.where(head, y.numpy(), 0))  # (beyond chunked_lens the reference's memory is uninitialised)
        put(pre + "ylens", yl)
        k += 1
    put("tokens_n", k)
    y, yl = RF.chunk_token_sequences_by_slices(torch.zeros((3, 4), dtype=torch.long), torch.zeros((3, 2), dtype=torch.long))
    put("tokens_2d_shapes", np.array([list(y.shape) + [0], [yl.shape[0], 0, 0]]))


def slicing():
    k = 0
    windows = ("symmetric", "causal", "future")

    def store(policy, window, valid, lobe, ins, res, defined=False):
        nonlocal k
        pre = "slice_{}_".format(k)
        put(pre + "kw", json.dumps(dict(policy=policy, window_type=window, valid_only=valid, lobe_size=lobe,
                                        defined=defined)))  # fmt: skip
        for name, v in ins.items():
            if v is not None:
                put(pre + name, v)
        put(pre + "slices", res[0])
        put(pre + "sources", res[1])
        k += 1

    for window, valid, lobe in itertools.product(windows, (True, False), (0, 1, 2, 5)):
        # fixed
        for T, with_lens in ((11, False), (11, True), (3, True)):
            N = 3
            x = torch.zeros((N, T, 2))
            lens = torch.from_numpy(rng.integers(0, T + 1, N)) if with_lens else None
            if lens is not None:
                lens[0] = 0  # an empty row
            store("fixed", window, valid, lobe, dict(input=x, in_lens=lens),
                  RF.slice_spect_data(x, lens, None, "fixed", window, valid, lobe))  # fmt: skip
        # ali: in_lens < T (the reference runs), then the two defined forms
        N, T = 4, 12
        ali = torch.from_numpy(rng.integers(0, 3, (N, T)))
        lens = torch.from_numpy(rng.integers(1, T, N))
        lens[1] = 0
        store("ali", window, valid, lobe, dict(input=ali, in_lens=lens),
              RF.slice_spect_data(ali, lens, None, "ali", window, valid, lobe))  # fmt: skip
        wide = torch.cat([ali, ali[:, -1:]], 1)
        full = torch.full((N,), T)
        store("ali", window, valid, lobe, dict(input=ali), RF.slice_spect_data(wide, full, None, "ali", window, valid, lobe), True)
        lens2 = lens.clone()
        lens2[0] = T
        store("ali", window, valid, lobe, dict(input=ali, in_lens=lens2),
              RF.slice_spect_data(wide, lens2, None, "ali", window, valid, lobe), True)  # fmt: skip
        # ref
        N, T = 3, 8
        start = rng.integers(-1, 10, (N, T))
        refs = torch.from_numpy(np.stack([rng.integers(0, 9, (N, T)), start, start + rng.integers(-1, 5, (N, T))], 2))
        lens = torch.from_numpy(rng.integers(0, T + 1, N))
        lens[2] = 0
        other = torch.from_numpy(rng.integers(6, 14, N))
        store("ref", window, valid, lobe, dict(input=refs, in_lens=lens, other_lens=other),
              RF.slice_spect_data(refs, lens, other, "ref", window, valid, lobe))  # fmt: skip
        store("ref", window, valid, lobe, dict(input=refs, other_lens=other),
              RF.slice_spect_data(refs, None, other, "ref", window, valid, lobe))  # fmt: skip
        last = refs[torch.arange(N), (lens - 1).clamp_min(0), 2].masked_fill(lens == 0, 0)
        store("ref", window, valid, lobe, dict(input=refs, in_lens=lens),
              RF.slice_spect_data(refs, lens, last, "ref", window, valid, lobe), True)  # fmt: skip
    put("slice_n", k)
    res = RF.slice_spect_data(torch.zeros((2, 0)))
    put("slice_t0_shapes", np.array([list(res[0].shape), [res[1].shape[0], 0]]))


def error_cases(F_, M_):
    """The calls whose exception types are recorded; the tests run the same table on the package."""
    x, sl = torch.arange(12.0).view(2, 6), torch.tensor([[-3, 2], [0, 8]])
    refs = torch.zeros((2, 4, 3), dtype=torch.long)
    return {
        "chunk_ndim": lambda: F_.chunk_by_slices(torch.zeros(3), sl),
        "chunk_lens_shape": lambda: F_.chunk_by_slices(x, sl, torch.tensor([3])),
        "chunk_mode": lambda: F_.chunk_by_slices(x, sl, None, "circular"),
        "chunk_reflect_pad": lambda: F_.chunk_by_slices(x, sl, torch.tensor([2, 6]), "reflect"),
        "chunk_replicate_len": lambda: F_.chunk_by_slices(x, sl, torch.tensor([0, 6]), "replicate"),
        "masked_ndim": lambda: F_.pad_masked_sequence(torch.zeros(3), torch.ones(3, 1, dtype=torch.bool)),
        "masked_mask_ndim": lambda: F_.pad_masked_sequence(x, torch.ones(2, dtype=torch.bool)),
        "masked_mask_dtype": lambda: F_.pad_masked_sequence(x, torch.ones(2, 6, dtype=torch.long), True),
        "masked_mask_shape": lambda: F_.pad_masked_sequence(x, torch.ones(2, 5, dtype=torch.bool), True),
        "tokens_shape": lambda: F_.chunk_token_sequences_by_slices(torch.zeros((2, 4, 2), dtype=torch.long), sl),
        "tokens_slices_shape": lambda: F_.chunk_token_sequences_by_slices(refs, sl[:1]),
        "tokens_lens_shape": lambda: F_.chunk_token_sequences_by_slices(refs, sl, torch.tensor([1])),
        "slice_ndim": lambda: F_.slice_spect_data(torch.zeros(3)),
        "slice_lobe": lambda: F_.slice_spect_data(x, lobe_size=-1),
        "slice_window": lambda: F_.slice_spect_data(x, window_type="casual"),
        "slice_policy": lambda: F_.slice_spect_data(x, policy="other"),
        "slice_in_lens_shape": lambda: F_.slice_spect_data(x, torch.tensor([1])),
        "slice_ali_ndim": lambda: F_.slice_spect_data(refs, policy="ali"),
        "slice_ref_ndim": lambda: F_.slice_spect_data(x, policy="ref"),
        "slice_ref_size": lambda: F_.slice_spect_data(torch.zeros((2, 4, 2), dtype=torch.long), policy="ref"),
        "slice_other_lens_shape": lambda: F_.slice_spect_data(refs, None, torch.tensor([1]), "ref"),
        "ctor_chunk_mode": lambda: M_.ChunkBySlices("circular"),
        "ctor_masked_batch_first": lambda: M_.PadMaskedSequence(1),
        "ctor_tokens_partial": lambda: M_.ChunkTokenSequencesBySlices(partial=1),
        "ctor_slice_policy": lambda: M_.SliceSpectData("other"),
        "ctor_slice_window": lambda: M_.SliceSpectData(window_type="casual"),
        "ctor_slice_lobe": lambda: M_.SliceSpectData(lobe_size=-1),
    }


def errors():
    names = {}
    for key, fn in error_cases(RF, RM).items():
        try:
            fn()
            names[key] = "none"
        except Exception as e:  # noqa: BLE001
            names[key] = type(e).__name__
    put("errors", json.dumps(names))
    reprs = {
        "ChunkBySlices": [repr(RM.ChunkBySlices()), repr(RM.ChunkBySlices("reflect"))],
        "PadMaskedSequence": [repr(RM.PadMaskedSequence(True, -1.0))],
        "SliceSpectData": [repr(RM.SliceSpectData("ali", "causal", False, 3))],
        "ChunkTokenSequencesBySlices": [repr(RM.ChunkTokenSequencesBySlices(p, r)) for p in (False, True) for r in (False, True)],
    }
    put("reprs", json.dumps(reprs))


def params(fn):
    fn = getattr(fn, "__wrapped__", fn)
    return [[p.name, p.default is not inspect.Parameter.empty, p.kind.name, repr(p.default)
             if p.default is not inspect.Parameter.empty else None]
            for p in inspect.signature(fn).parameters.values() if p.name != "self"]


FUNCTIONS = ("pad_masked_sequence", "chunk_by_slices", "chunk_token_sequences_by_slices", "slice_spect_data")
MODULES = ("PadMaskedSequence", "ChunkBySlices", "ChunkTokenSequencesBySlices", "SliceSpectData")


def signatures():
    sig = {"functional": {n: params(getattr(RF, n)) for n in FUNCTIONS}, "modules": {}}
    for n in MODULES:
        cls = getattr(RM, n)
        sig["modules"][n] = {"__init__": params(cls.__init__), "forward": params(cls.forward),
                             "__constants__": list(cls.__constants__)}  # fmt: skip
    with open(os.path.join(HERE, "chunk_signatures.json"), "w") as f:
        json.dump(sig, f, indent=1, sort_keys=True)


if __name__ == "__main__":
    torch.manual_seed(0)
    chunks()
    masked()
    tokens()
    slicing()
    errors()
    signatures()
    np.savez_compressed(os.path.join(HERE, "chunk.npz"), **out)
    print("wrote chunk.npz:", len(out), "arrays,", os.path.getsize(os.path.join(HERE, "chunk.npz")), "bytes;",
          int(out["chunk_n"]), "chunk cases,", int(out["chunk_discarded"]), "discarded")
