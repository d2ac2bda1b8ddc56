"""CPU: feat_deltas / FeatureDeltas and mean_var_norm / MeanVarianceNormalization without a GPU -- the
reference's signatures, constructor validation, state_dict keys, error types, the CPU body against the
goldens (tests/golden/feats.npz, captured from the reference), scripting and tracing; and the pins of
tests/_feats_ref.py, the GPU suite's references, to the goldens and to the CPU bodies."""
import inspect
import json
import os

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLD, "feats.npz"))


def upstream(shape, dtype):
    n = int(np.prod(shape))
    return torch.cos(torch.arange(n, dtype=torch.float64) * 0.7).reshape(shape).to(dtype)


def _params(fn):
    return [[p.name, p.default is not inspect.Parameter.empty, p.kind.name,
             repr(p.default) if p.default is not inspect.Parameter.empty else None]
            for p in inspect.signature(fn).parameters.values() if p.name != "self"]  # fmt: skip


def test_signatures_match_reference():
    from pydrobert_amd import config
    from pydrobert_amd import functional as F
    from pydrobert_amd import modules as M

    sig = json.load(open(os.path.join(GOLD, "feats_signatures.json")))
    for name, exp in sig["functional"].items():
        assert _params(getattr(F, name)) == exp, name
    for name, exp in sig["modules"].items():
        cls = getattr(M, name)
        assert _params(cls.__init__) == exp["__init__"], name
        assert _params(cls.forward) == exp["forward"], name
    assert config.TINY == 1.1754943508222875e-38


def test_constructors_validate(gold):
    from pydrobert_amd import modules as M

    errors = json.loads(str(gold["errors"]))
    cases = {
        "ctor_order": lambda: M.FeatureDeltas(order=-1),
        "ctor_pad_mode": lambda: M.FeatureDeltas(pad_mode="zeros"),
        "ctor_mean_ndim": lambda: M.MeanVarianceNormalization(mean=torch.zeros(2, 2)),
        "ctor_mean_std_len": lambda: M.MeanVarianceNormalization(mean=torch.zeros(2), std=torch.ones(3)),
        "ctor_eps": lambda: M.MeanVarianceNormalization(eps=-1.0),
    }
    for key, fn in cases.items():
        with pytest.raises({"ValueError": ValueError, "RuntimeError": RuntimeError}[errors[key]]):
            fn()
    with pytest.raises(ValueError):
        M.FeatureDeltas(dim=1.5)
    with pytest.raises(ValueError):
        M.MeanVarianceNormalization(mean=torch.zeros(0))
    assert "order=2" in repr(M.FeatureDeltas()) and "eps=" in repr(M.MeanVarianceNormalization())


def test_error_types(gold):
    from pydrobert_amd import functional as F
    from pydrobert_amd import modules as M

    errors = json.loads(str(gold["errors"]))

    def store_after(n):
        m = M.MeanVarianceNormalization()
        m.accumulate(torch.randn(n, 3))
        m.store()

    cases = {
        "time_dim_range": lambda: F.feat_deltas(torch.randn(2, 5, 3), time_dim=3),
        "dim_range": lambda: F.feat_deltas(torch.randn(2, 5, 3), dim=3),
        "dim_range_stack": lambda: F.feat_deltas(torch.randn(2, 5, 3), dim=4, concatenate=False),
        "order_negative": lambda: F.feat_deltas(torch.randn(2, 5, 3), order=-1),
        "width_zero": lambda: F.feat_deltas(torch.randn(2, 5, 3), width=0),
        "reflect_too_short": lambda: F.feat_deltas(torch.randn(2, 4, 3), pad_mode="reflect"),
        "circular_too_short": lambda: F.feat_deltas(torch.randn(2, 3, 3), pad_mode="circular"),
        "empty_time": lambda: F.feat_deltas(torch.randn(2, 0, 3)),
        "mvn_dim_range": lambda: F.mean_var_norm(torch.randn(2, 5, 3), 3),
        "mvn_dim_range_neg": lambda: F.mean_var_norm(torch.randn(2, 5, 3), -4),
        "store_one_sample": lambda: store_after(1),
        "store_nothing": lambda: M.MeanVarianceNormalization().store(),
    }
    for key, fn in cases.items():
        exc = {"RuntimeError": RuntimeError, "IndexError": IndexError, "ValueError": ValueError}[errors[key]]
        with pytest.raises(exc):
            fn()
    with pytest.raises(TypeError):
        F.feat_deltas(torch.ones(2, 5, 3, dtype=torch.long))


def test_state_dict_keys(gold):
    from pydrobert_amd import modules as M

    assert sorted(M.FeatureDeltas().state_dict()) == json.loads(str(gold["deltas_keys_new"]))
    m = M.MeanVarianceNormalization(dim=1)
    assert sorted(m.state_dict()) == json.loads(str(gold["acc_keys_new"]))
    m.accumulate(torch.from_numpy(gold["acc_chunk_0"]))
    assert sorted(m.state_dict()) == json.loads(str(gold["acc_keys_accumulated"]))
    m.store()
    assert sorted(m.state_dict()) == json.loads(str(gold["acc_keys_stored"]))
    for order in range(4):
        for width in (1, 2, 3):
            f = M.FeatureDeltas(order=order, width=width).filters
            assert torch.equal(f, torch.from_numpy(gold["filters_{}_{}".format(order, width)]))


def test_deltas_cpu_body_matches_goldens(gold):
    from pydrobert_amd import functional as F

    for k in range(int(gold["deltas_n"])):
        pre = "deltas_{}_".format(k)
        kw = json.loads(str(gold[pre + "kw"]))
        x = torch.from_numpy(gold[pre + "x"]).requires_grad_(True)
        y = F.feat_deltas(x, **kw)
        assert y.shape == gold[pre + "y"].shape, kw
        assert np.abs(y.detach().numpy() - gold[pre + "y"]).max() <= 1e-6, kw
        (gx,) = torch.autograd.grad(y, x, upstream(tuple(y.shape), x.dtype))
        assert np.abs(gx.numpy() - gold[pre + "gx"]).max() <= 1e-6 * max(1.0, np.abs(gold[pre + "gx"]).max()), kw


def test_mvn_cpu_body_matches_goldens(gold):
    from pydrobert_amd import functional as F

    for k in range(int(gold["mvn_n"])):
        pre = "mvn_{}_".format(k)
        kw = json.loads(str(gold[pre + "kw"]))
        x = torch.from_numpy(gold[pre + "x"]).requires_grad_(True)
        mean = torch.from_numpy(gold[pre + "mean"]).requires_grad_(True) if pre + "mean" in gold else None
        std = torch.from_numpy(gold[pre + "std"]).requires_grad_(True) if pre + "std" in gold else None
        y = F.mean_var_norm(x, kw["dim"], mean, std)
        assert np.allclose(y.detach().numpy(), gold[pre + "y"], rtol=1e-6, atol=1e-6), kw
        ins = [t for t in (x, mean, std) if t is not None]
        grads = torch.autograd.grad(y, ins, upstream(tuple(x.shape), x.dtype))
        assert np.allclose(grads[0].numpy(), gold[pre + "gx"], rtol=1e-6, atol=1e-6), kw
        if mean is not None:
            assert np.allclose(grads[1].numpy(), gold[pre + "gmean"], rtol=1e-6, atol=1e-6), kw
        if std is not None:
            assert np.allclose(grads[-1].numpy(), gold[pre + "gstd"], rtol=1e-6, atol=1e-6), kw


def test_accumulate_store_cpu(gold):
    from pydrobert_amd import modules as M

    chunks = [torch.from_numpy(gold["acc_chunk_{}".format(i)]) for i in range(6)]
    for bessel in (False, True):
        m = M.MeanVarianceNormalization(dim=1)
        for c in chunks:
            m.accumulate(c)
        assert np.allclose(m.count.numpy(), gold["acc_count"], rtol=1e-12)
        assert np.allclose(m.sum.numpy(), gold["acc_sum"], rtol=1e-12)
        assert np.allclose(m.sumsq.numpy(), gold["acc_sumsq"], rtol=1e-12)
        m.store(bessel=bessel)
        assert np.allclose(m.mean.numpy(), gold["acc_mean_b{}".format(int(bessel))], rtol=1e-12)
        assert np.allclose(m.std.numpy(), gold["acc_std_b{}".format(int(bessel))], rtol=1e-12)


def test_modules_script_and_trace_cpu():
    from pydrobert_amd import modules as M

    x = torch.randn(3, 11, 4)
    for mod in (M.FeatureDeltas(), M.FeatureDeltas(0, 1, False, 3, 1, "constant", 0.5), M.MeanVarianceNormalization(1)):
        exp = mod(x)
        assert torch.allclose(torch.jit.script(mod)(x), exp)
        assert torch.allclose(torch.jit.trace(mod, x)(x), exp)
    sm = torch.jit.script(M.MeanVarianceNormalization())
    for _ in range(3):
        sm.accumulate(torch.randn(5, 4))
    sm.store(False, True)
    assert sm.count is not None and sm.std is not None and sm(x).shape == x.shape


def test_ops_registered_and_entry_points_declared():
    import pydrobert_amd.functional  # noqa: F401
    from pydrobert_amd import _cabi

    for op in ("feat_deltas", "feat_deltas_backward", "mean_var_norm", "mean_var_norm_backward", "mvn_accumulate"):
        assert hasattr(torch.ops.pydrobert_amd, op)
    header = open(os.path.join(ROOT, "include", "pdt_amd.h")).read()
    for name in ("pdt_feat_deltas", "pdt_feat_deltas_backward", "pdt_mvn_stats", "pdt_mvn_apply", "pdt_mvn_backward",
                 "pdt_mvn_stats_workspace_bytes"):
        assert name in _cabi.SIGNATURES and name + "(" in header


# ----------------------------------------------------------------------------------------------------------
# tests/_feats_ref.py, the references the GPU suite compares the kernels with: pinned to the reference's
# goldens and to the package's CPU bodies before any GPU run relies on them

import _feats_ref as R  # noqa: E402

_DELTA_DEFAULTS = dict(dim=-1, time_dim=-2, concatenate=True, pad_mode="replicate", value=0.0)


def _built_taps(kw):
    from pydrobert_amd import _feats

    return _feats._feat_delta_filters(kw.get("order", 2), kw.get("width", 2)).double()


def test_feats_ref_matches_goldens(gold):
    for k in range(int(gold["deltas_n"])):
        pre = "deltas_{}_".format(k)
        kw = json.loads(str(gold[pre + "kw"]))
        taps = _built_taps(kw)
        geo = {n: kw.get(n, d) for n, d in _DELTA_DEFAULTS.items()}
        x = torch.from_numpy(gold[pre + "x"])
        tol = 1e-6 if x.dtype == torch.float32 else 1e-12  # (the goldens' own precision)
        y = R.deltas_ref(x.numpy(), taps.numpy(), **geo)
        assert y.shape == gold[pre + "y"].shape and np.abs(y - gold[pre + "y"]).max() <= tol, kw
        xt = x.double().requires_grad_(True)
        yt = R.deltas_torch(xt, taps, **geo)
        assert np.abs(yt.detach().numpy() - y).max() <= 1e-13, kw
        (gx,) = torch.autograd.grad(yt, xt, upstream(tuple(yt.shape), x.dtype).double())
        assert np.abs(gx.numpy() - gold[pre + "gx"]).max() <= tol * max(1.0, np.abs(gold[pre + "gx"]).max()), kw
    for k in range(int(gold["mvn_n"])):
        pre = "mvn_{}_".format(k)
        kw = json.loads(str(gold[pre + "kw"]))
        x = torch.from_numpy(gold[pre + "x"])
        tol = 1e-6 if x.dtype == torch.float32 else 1e-12
        mean = torch.from_numpy(gold[pre + "mean"]) if pre + "mean" in gold else None
        std = torch.from_numpy(gold[pre + "std"]) if pre + "std" in gold else None
        y = R.mvn_ref(x.numpy(), kw["dim"], None if mean is None else mean.numpy(), None if std is None else std.numpy())[0]
        assert np.allclose(y, gold[pre + "y"], rtol=tol, atol=tol), kw
        ins = [t.double().requires_grad_(True) if t is not None else None for t in (x, mean, std)]
        yt = R.mvn_torch(ins[0], kw["dim"], ins[1], ins[2])
        assert np.allclose(yt.detach().numpy(), y, rtol=1e-13, atol=1e-13), kw
        grads = torch.autograd.grad(yt, [t for t in ins if t is not None], upstream(tuple(x.shape), x.dtype).double())
        assert np.allclose(grads[0].numpy(), gold[pre + "gx"], rtol=tol, atol=tol), kw
        if mean is not None:
            assert np.allclose(grads[1].numpy(), gold[pre + "gmean"], rtol=tol, atol=tol), kw
        if std is not None:
            assert np.allclose(grads[-1].numpy(), gold[pre + "gstd"], rtol=tol, atol=tol), kw


@pytest.mark.parametrize("case", R.DELTA_CASES, ids=[c[0] for c in R.DELTA_CASES])
def test_deltas_ref_matches_cpu_body(case):
    """deltas_ref and deltas_torch against each other and against the package's CPU body (forward and
    adjoint) at the GPU suite's shapes, with the built taps and with random ones.  The CPU body unfolds
    (T, K) windows, so it sits out the one shape whose windows take hundreds of MB, and its adjoint (windows
    over 4P more steps) the two with K > 16000, which it needs seconds for."""
    from pydrobert_amd import functional as F

    name, shape, dtype, kw, modes = case
    x = R.delta_input(shape, "float64")
    for taps in (_built_taps(kw), torch.randn(kw["order"] + 1, 1 + 2 * kw["order"] * kw["width"], dtype=torch.float64)):
        for mode in modes:
            geo = dict(_DELTA_DEFAULTS, pad_mode=mode, value=-0.5 if mode == "constant" else 0.0)
            geo.update({n: v for n, v in kw.items() if n in geo})
            y = R.deltas_ref(x.numpy(), taps.numpy(), **geo)
            xt = x.clone().requires_grad_(True)
            yt = R.deltas_torch(xt, taps, **geo)
            scale = max(1.0, np.abs(y).max())
            assert yt.shape == y.shape and np.abs(yt.detach().numpy() - y).max() <= 1e-12 * scale, (name, mode)
            if name == "shrink-deep":
                continue
            g = upstream(tuple(y.shape), torch.float64)
            (gt,) = torch.autograd.grad(yt, xt, g)
            xc = x.clone().requires_grad_(True)
            yc = F.feat_deltas(xc, _filters=taps, order=kw["order"], width=kw["width"], **geo)
            assert np.abs(yc.detach().numpy() - y).max() <= 1e-12 * scale, (name, mode)
            if taps.shape[1] > 16000:
                continue
            (gc,) = torch.autograd.grad(yc, xc, g)
            assert (gc - gt).abs().max().item() <= 1e-12 * max(1.0, gt.abs().max().item()), (name, mode)


@pytest.mark.parametrize("shape,dim", R.MVN_CASES, ids=str)
def test_mvn_ref_matches_cpu_body(shape, dim):
    from pydrobert_amd import functional as F

    x = R.mvn_input(shape, torch.float64)
    X = shape[dim]
    given_m = R.mvn_input((X,), torch.float64, seed=1)
    given_s = R.mvn_input((X,), torch.float64, seed=2).abs() + 0.5
    g = upstream(shape, torch.float64)
    for mean, std in ((None, None), (given_m, None), (None, given_s), (given_m, given_s)):
        y, m, s = R.mvn_ref(x.numpy(), dim, None if mean is None else mean.numpy(), None if std is None else std.numpy())
        ins = [t.clone().requires_grad_(True) if t is not None else None for t in (x, mean, std)]
        yt = R.mvn_torch(*ins[:1], dim, *ins[1:])
        assert np.allclose(yt.detach().numpy(), y, rtol=1e-12, atol=1e-12)
        gt = torch.autograd.grad(yt, [t for t in ins if t is not None], g)
        ins = [t.clone().requires_grad_(True) if t is not None else None for t in (x, mean, std)]
        yc, stats = torch.ops.pydrobert_amd.mean_var_norm(ins[0], dim, ins[1], ins[2], R.TINY)
        assert np.allclose(yc.detach().numpy(), y, rtol=1e-12, atol=1e-12)
        if mean is None or std is None:
            assert np.allclose(stats[0].numpy(), m if mean is None else R.mvn_ref(x.numpy(), dim)[1], rtol=1e-12, atol=1e-12)
            assert np.allclose(stats[1].numpy(), s if std is None else R.mvn_ref(x.numpy(), dim)[2], rtol=1e-9, atol=0)
        gc = torch.autograd.grad(yc, [t for t in ins if t is not None], g)
        for a, b in zip(gc, gt):
            # (the sums behind these gradients cancel: the bound is relative to the largest element)
            assert (a - b).abs().max().item() <= 1e-10 * max(1.0, b.abs().max().item())


@pytest.mark.parametrize("dtype", (torch.float16, torch.bfloat16), ids=str)
def test_mvn_16bit_cpu_body_within_recorded_ulps(dtype):
    """The figure the GPU suite's 16-bit bound is built from: the CPU body against mvn_ref_rounded."""
    worst = 0.0
    for shape, dim in R.MVN_CASES_16:
        x = R.mvn_input(shape, dtype)
        y = torch.ops.pydrobert_amd.mean_var_norm(x, dim, None, None, R.TINY)[0]
        worst = max(worst, R.ulps(y, R.mvn_ref_rounded(x, dim)[0], dtype))
    print("16-bit CPU body vs mvn_ref_rounded, {}: {} ulps".format(dtype, worst))
    assert worst <= R.MVN_16BIT_CPU_ULPS
