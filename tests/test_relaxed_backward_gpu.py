"""GPU: the backward kernels of csrc/relaxed.hip and the operator ``pydrobert_amd::relaxed_backward`` over them.

Yardstick: autograd through the float64 formulas of tests/_distributions_ref.py on the CPU, clamping at the eps of
the dtype under test, with the parameter expanded to every sample row as the leaf, so that the terms of the sum
over the samples come out one by one.  A summed gradient is held to ``tol eps (1 + sum_s |term_s|)`` per element,
``tol`` the stored golden tolerance ``C.tolerance(family, "g_" + output, dtype)`` (4 times the reference's own
deviation, at least 4 units).  The gradients of ``log_prob`` / ``clog_prob`` with respect to ``z`` / ``zcond`` are
elementwise and of the same depth as the parameter's: the same ``tol``, on ``eps (1 + |value|)``.  Every test
prints its largest figure, in those units, before it asserts.

Bounds set here, with their reasons:
* the kernel against the torch body on the device (kinks): 1.25 tol.  The kernel is within tol of the yardstick
  (test_every_form) and the body, which is the reference's arithmetic, within the tol / 4 that the golden maker
  measured of it.  The zero patterns are compared exactly.
* second derivatives (float64): 1e-9 (1 + |value|), what tests/test_distributions_gpu.py documents for the RELAX
  composition; the operator's derivative is autograd through the torch body, as the comparison is.
"""
import functools

import pytest
import torch

import _distributions_check as C
import _distributions_ref as ref

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
RSAMPLE, THRESHOLD, TLOG_PROB, CSAMPLE, LOG_PROB, CLOG_PROB = range(6)
OPS = {"rsample": RSAMPLE, "tlog_prob": TLOG_PROB, "csample": CSAMPLE, "log_prob": LOG_PROB, "clog_prob": CLOG_PROB}
OUTPUT = {"rsample": "z", "tlog_prob": "tlog_prob", "csample": "zcond", "log_prob": "log_prob", "clog_prob": "clog_prob"}
FAMILIES = ("gumbel", "bernoulli")
DTYPES = {"float32": torch.float32, "float64": torch.float64}


def _reduces(family, name):
    return family == "gumbel" and name in ("tlog_prob", "log_prob", "clog_prob")


def _lib():
    from pydrobert_amd import _cabi

    return _cabi.lib()


def backward(family, name, g, param, x1, x2, B, want=3, p_sr=None, p_sv=1):
    """One call of the C ABI on device tensors: ((B, V) or None, (R, V) or None)."""
    from pydrobert_amd import _cabi

    lib = _lib()
    V = x1.shape[-1]
    R = x1.numel() // V
    code = {torch.float32: 0, torch.float64: 1}[x1.dtype]
    assert g.is_contiguous() and x1.is_contiguous() and (x2 is None or x2.is_contiguous())
    assert g.numel() == (R if _reduces(family, name) else R * V) and R % B == 0
    assert param.numel() >= B * V or p_sr == 0 or p_sv == 0
    gp = torch.full((B, V), float("nan"), dtype=x1.dtype, device=DEV) if want & 1 else None
    gx = torch.full((R, V), float("nan"), dtype=x1.dtype, device=DEV) if want & 2 else None
    words = lib.pdt_relaxed_backward_workspace_bytes(code, R, B, V) // 8
    ws = torch.empty((max(words, 1),), dtype=torch.float64, device=DEV)
    fn = lib.pdt_relaxed_gumbel_backward if family == "gumbel" else lib.pdt_relaxed_bernoulli_backward
    rc = fn(OPS[name], code, g.data_ptr(), param.data_ptr(), B, V if p_sr is None else p_sr, p_sv, x1.data_ptr(),
            _cabi.ptr(x2), R, V, _cabi.ptr(gp), _cabi.ptr(gx), ws.data_ptr(), _cabi.stream_ptr(DEV))
    assert rc == 0, rc
    return gp, gx


@functools.lru_cache(maxsize=None)
def case(family, dt, S, B, V, seed=0):
    """Inputs of every method at one shape, in the dtype under test, on the CPU: the data are (S, B, V)."""
    dtype = DTYPES[dt]
    gen = torch.Generator().manual_seed(1000 * V + 10 * S + B + seed)
    eps = float(torch.finfo(dtype).eps)
    fam = ref.FAMILY[family]
    raw = 2 * torch.randn((B, V), dtype=torch.float64, generator=gen)
    logits = (raw.log_softmax(-1) if family == "gumbel" else raw).to(dtype)
    probs = (raw.softmax(-1) if family == "gumbel" else raw.sigmoid()).to(dtype)
    u, v = ((torch.rand((S, B, V), dtype=torch.float64, generator=gen) * 0.96 + 0.02).to(dtype) for _ in range(2))
    z = fam["rsample"](ref.f64(logits), ref.f64(u), eps).to(dtype)
    b = fam["threshold"](ref.f64(z)).to(dtype)
    zcond = fam["csample"](ref.f64(probs), ref.f64(b), ref.f64(v), eps).to(dtype)
    assert torch.equal(fam["threshold"](ref.f64(zcond)).to(dtype), b)
    return dict(logits=logits, probs=probs, u=u, v=v, z=z, b=b, zcond=zcond)


def arguments(name, t):
    """(param, x1, x2) of method ``name`` from the tensors of :func:`case`."""
    return {"rsample": (t["logits"], t["u"], None), "tlog_prob": (t["logits"], t["b"], None),
            "csample": (t["probs"], t["b"], t["v"]), "log_prob": (t["logits"], t["z"], None),
            "clog_prob": (t["logits"], t["zcond"], t["b"])}[name]


def yardstick(family, name, param_rows, x1, x2, up, eps):
    """float64 autograd on the CPU.  ``param_rows`` has the data's shape (a value per sample row); returns the
    terms of the parameter's gradient, one per sample row, and the gradient of x1 (None where there is none)."""
    fam = ref.FAMILY[family]
    leaf = ref.f64(param_rows).clone().requires_grad_(True)
    x1, x2, up = ref.f64(x1), None if x2 is None else ref.f64(x2), ref.f64(up)
    data = x1.clone().requires_grad_(name in ("log_prob", "clog_prob"))
    out = {"rsample": lambda: fam["rsample"](leaf, data, eps), "tlog_prob": lambda: fam["tlog_prob"](leaf, data),
           "csample": lambda: fam["csample"](leaf, data, x2, eps), "log_prob": lambda: fam["log_prob"](leaf, data),
           "clog_prob": lambda: fam["clog_prob"](leaf, data, x2)}[name]()
    assert torch.isfinite(out).all()
    grads = torch.autograd.grad(out, [leaf, data] if data.requires_grad else [leaf], up)
    return grads[0], (grads[1] if data.requires_grad else None)


def summed_units(got, terms, shape, eps):
    """|got - sum of the terms| in units of eps (1 + sum |term|), the largest over the elements."""
    shape = tuple(shape)
    # (a size-1 dimension of ``shape`` that the terms fill is summed too: moved in front, next to the sample rows)
    lead = terms.dim() - len(shape)
    inner = [lead + i for i, n in enumerate(shape) if n == 1 and terms.shape[lead + i] != 1]
    keep = [d for d in range(lead, terms.dim()) if d not in inner]
    terms = terms.permute(list(range(lead)) + inner + keep).contiguous()
    kept = tuple(terms.shape[lead + len(inner):])
    want = ref.exact_sum_to_size(terms, kept).reshape(shape)
    mag = terms.abs().reshape((-1,) + kept).sum(0).reshape(shape)
    got = got.detach().double().cpu().reshape(shape)
    assert torch.isfinite(got).all()
    return float(((got - want).abs() / (eps * (1 + mag))).max())


def smallest_parts_S(V):
    lib = _lib()
    return next(S for S in range(1, 100) if lib.pdt_relaxed_backward_parts(S, 1, V) > 1)


VS = (1, 2, 3, 5, 33, 64, 65, 130)
SB = ((1, 1), (1, 3), (2, 3), (7, 1))


@pytest.mark.parametrize("dt", list(DTYPES))
@pytest.mark.parametrize("name", list(OPS))
@pytest.mark.parametrize("family", FAMILIES)
def test_every_form(family, name, dt):
    """Both families, five methods, both dtypes, at the widths where the kernels change form, in the base form and
    in the parts form, against the yardstick; and the three ways to ask (parameter, data, both) bit for bit.

    Largest figures of the first run on an MI355X, in units, float32 / float64.  The parameter's gradient: rsample
    0.24 / 0.39, tlog_prob 0.14 / 0.12 (Gumbel) and 0.76 / 1.41 (logistic), csample 1.66 / 1.84 and 1.35 / 1.81,
    log_prob 0.78 / 1.15 and 1.03 / 1.55, clog_prob 0.82 / 1.25 and 1.44 / 2.01.  The data gradients, which have no
    stored tolerance of their own and take the parameter's (4 to 35): log_prob 0.80 / 1.20 (z, Gumbel) and
    0.86 / 1.56 (logistic), clog_prob 1.70 / 1.66 (zcond, Gumbel) and 0.86 / 2.16 (logistic)."""
    lib = _lib()
    dtype, eps = DTYPES[dt], float(torch.finfo(DTYPES[dt]).eps)
    tol = C.tolerance(family, "g_" + OUTPUT[name], dt)
    shapes = [(S, B, V) for V in VS for S, B in SB]
    in_parts = []
    for V in (5, 65):
        S = smallest_parts_S(V)
        assert lib.pdt_relaxed_backward_parts(S - 1, 1, V) == 1
        # (and the parts of several parameter rows, over more than one workgroup)
        in_parts += [(S, 1, V), (S + 3, 5 * lib.pdt_relaxed_rows_per_block(V) // 4 + 1, V)]
    worst = {"param": 0.0, "data": 0.0}
    for S, B, V in shapes + in_parts:
        parts = lib.pdt_relaxed_backward_parts(S * B, B, V)
        assert (parts > 1) == ((S, B, V) in in_parts), (S, B, V, parts)
        t = case(family, dt, S, B, V)
        param, x1, x2 = arguments(name, t)
        up = ref.upstream((S, B) if _reduces(family, name) else (S, B, V), dtype)
        terms, want_x1 = yardstick(family, name, param.expand(S, B, V), x1, x2, up, eps)
        on = [None if x is None else x.to(DEV) for x in (up, param, x1, x2)]
        both = backward(family, name, *on, B, 3 if want_x1 is not None else 1)
        worst["param"] = max(worst["param"], summed_units(both[0], terms, (B, V), eps))
        alone = backward(family, name, *on, B, 1)
        assert alone[1] is None and torch.equal(alone[0], both[0]), (S, B, V)
        if want_x1 is not None:
            worst["data"] = max(worst["data"], ref.units(both[1].reshape(S, B, V), want_x1, eps))
            data = backward(family, name, *on, B, 2)
            assert data[0] is None and torch.equal(data[1], both[1]), (S, B, V)
    print(family, name, dt, "tol", tol, {k: round(v, 2) for k, v in worst.items()})
    assert worst["param"] <= tol and worst["data"] <= tol, (worst, tol)


def _body(family, name, g, param, x1, x2, B):
    """The torch body on the same device tensors: ((B, V) summed over the sample rows, the gradient of x1)."""
    from pydrobert_amd import _relaxed as X

    fn = X._gumbel_backward if family == "gumbel" else X._bernoulli_backward
    d_param, d_x1, _ = fn(OPS[name], g, param, x1, x2)
    return d_param.sum_to_size(param.shape), d_x1


def _against_body(family, name, dt, g, param, x1, x2, what):
    """Zero pattern exactly, values to 1.25 tol, non-finite pattern exactly; returns the kernel's gradients."""
    eps = float(torch.finfo(DTYPES[dt]).eps)
    tol = 1.25 * C.tolerance(family, "g_" + OUTPUT[name], dt)
    B = param.shape[0]
    want = _body(family, name, g, param, x1, x2, B)
    has_x1 = name in ("log_prob", "clog_prob")
    got = backward(family, name, g.contiguous(), param, x1, x2, B, 3 if has_x1 else 1)
    # the magnitude of the sum: the body's terms, one per sample row
    from pydrobert_amd import _relaxed as X

    terms = (X._gumbel_backward if family == "gumbel" else X._bernoulli_backward)(OPS[name], g, param, x1, x2)[0]
    mag = terms.double().abs().expand(x1.shape).sum_to_size(param.shape)
    for a, b, m, label in ((got[0], want[0], mag, "param"),) + (((got[1], want[1], want[1].double().abs(), "data"),) if has_x1 else ()):
        a, b = a.reshape(b.shape), b
        assert torch.equal(torch.isnan(a), torch.isnan(b)), (what, label)
        assert torch.equal(torch.isinf(a) & (a > 0), torch.isinf(b) & (b > 0)), (what, label)
        assert torch.equal(torch.isinf(a) & (a < 0), torch.isinf(b) & (b < 0)), (what, label)
        fin = torch.isfinite(b)
        assert torch.equal((a == 0) & fin, (b == 0) & fin), (what, label, a, b)
        d = ((a.double() - b.double()).abs() / (eps * (1 + m)))[fin & torch.isfinite(m)]
        figure = float(d.max()) if d.numel() else 0.0
        print(family, name, dt, what, label, "units", round(figure, 2), "bound", tol)
        assert figure <= tol, (what, label)
    return got


@pytest.mark.parametrize("dt", list(DTYPES))
def test_kinks_gumbel(dt):
    dtype, eps = DTYPES[dt], float(torch.finfo(DTYPES[dt]).eps)
    gold = C.gold()
    t = lambda key: torch.from_numpy(gold[key]).to(dtype).to(DEV)  # noqa: E731
    # csample: the recorded rows where the min guard decides
    pre = "guard_{}_".format(dt)
    param, b, v = t(pre + "param").softmax(-1), t(pre + "b"), t(pre + "v")
    param, b, v = (x.reshape(-1, x.shape[-1]) for x in (param, b, v))
    assert ref.gumbel_guard(ref.f64(param).cpu(), ref.f64(b).cpu(), ref.f64(v).cpu(), eps).any()
    g = ref.upstream(b.shape, dtype).to(DEV)
    got, _ = _against_body("gumbel", "csample", dt, g, param, b, v, "guard")
    # (row 0: p_0 is 1 - 5e-5, unclamped, and b_0 = 0; -log v_0 / p_0 is lost in -log v_k, so the guard holds it)
    assert got[0, 0] == 0 and (got != 0).any()
    # csample: probabilities at and beyond the clamps, a row of b without a hot element, one with two nonzeros;
    # two sample rows per parameter row
    tiny = eps / 4
    probs = torch.tensor([[0.0, tiny, 0.5, 1.0, 0.3], [eps, 1 - eps, 1 - tiny, 0.2, 0.1], [0.1, 0.2, 0.3, 0.25, 0.15]],
                         dtype=dtype, device=DEV)
    assert (probs[:2] < eps).any() and (probs[:2] > 1 - eps).any()
    b = torch.tensor([[[0, 0, 1, 0, 0], [1, 0, 0, 0, 0], [0, 0, 0, 0, 0]],
                      [[0, 0, 0, 0, 1], [0, 0, 0, 1, 0], [1, 0, 1, 0, 0]]], dtype=dtype, device=DEV)
    v = (torch.rand((2, 3, 5), generator=torch.Generator().manual_seed(5), dtype=torch.float64) * 0.9 + 0.05).to(dtype).to(DEV)
    g = ref.upstream(b.shape, dtype).to(DEV)
    got, _ = _against_body("gumbel", "csample", dt, g, probs, b, v, "clamps and odd b")
    assert (got[0, :2] == 0).all() and got[0, 3] == 0 and got[1, 2] == 0 and (got != 0).any()
    # clog_prob: b off the arg-max, b without a hot element, b with two nonzeros, a tie in zcond with b on its
    # lower index (a hit) and on its higher (a miss)
    logits = torch.randn((6, 5), generator=torch.Generator().manual_seed(6), dtype=torch.float64).log_softmax(-1).to(dtype).to(DEV)
    zcond = torch.tensor([[0.1, 2.0, -1.0, 0.3, 0.2], [0.1, 2.0, -1.0, 0.3, 0.2], [0.1, 2.0, -1.0, 0.3, 0.2],
                          [0.1, 2.0, -1.0, 0.3, 0.2], [0.1, 2.0, -1.0, 2.0, 0.2], [0.1, 2.0, -1.0, 2.0, 0.2]],
                         dtype=dtype, device=DEV)
    b = torch.tensor([[0, 1, 0, 0, 0], [0, 0, 1, 0, 0], [0, 0, 0, 0, 0], [0, 1, 0, 1, 0], [0, 1, 0, 0, 0],
                      [0, 0, 0, 1, 0]], dtype=dtype, device=DEV)
    g = ref.upstream((6,), dtype).to(DEV) + 2
    gp, gx = _against_body("gumbel", "clog_prob", dt, g, logits, zcond, b, "misses and ties")
    for row, hit in enumerate((True, False, False, False, True, False)):
        assert bool((gp[row] != 0).any()) == hit and bool((gx[row] != 0).any()) == hit, row


@pytest.mark.parametrize("dt", list(DTYPES))
def test_kinks_bernoulli(dt):
    dtype, eps = DTYPES[dt], float(torch.finfo(DTYPES[dt]).eps)
    tiny = eps / 4
    probs = torch.tensor([[0.0, tiny, eps, 0.5, 1 - eps, 1 - tiny, 1.0]], dtype=dtype, device=DEV)
    b = torch.tensor([[[0, 1, 0, 1, 0, 1, 0]], [[1, 0, 1, 0, 1, 0, 1]]], dtype=dtype, device=DEV)
    v = (torch.rand((2, 1, 7), generator=torch.Generator().manual_seed(7), dtype=torch.float64) * 0.9 + 0.05).to(dtype).to(DEV)
    got, _ = _against_body("bernoulli", "csample", dt, ref.upstream(b.shape, dtype).to(DEV), probs, b, v, "clamps")
    assert (got[0, [0, 1, 5, 6]] == 0).all() and (got[0, 2:5] != 0).all()
    logits = torch.tensor([[0.3, -0.7, 1.1, 0.0, -2.0, 0.5]], dtype=dtype, device=DEV)
    zcond = torch.tensor([[[0.5, 0.5, -0.5, -0.5, 0.0, -0.0]], [[0.0, -0.0, 1.0, -1.0, 2.0, -2.0]]], dtype=dtype, device=DEV)
    b = torch.tensor([[[1, 0, 0, 1, 1, 1]], [[0, 0, 1, 0, 0, 1]]], dtype=dtype, device=DEV)
    gp, gx = _against_body("bernoulli", "clog_prob", dt, ref.upstream(b.shape, dtype).to(DEV) + 2, logits, zcond, b,
                           "misses and zeros")
    assert torch.equal(gx.reshape(2, 6) != 0, torch.tensor([[1, 0, 1, 0, 1, 1], [0, 0, 1, 1, 0, 0]], device=DEV).bool())


@pytest.mark.parametrize("family", FAMILIES)
def test_non_finite_values_spread_as_in_the_torch_body(family):
    """inf and NaN in the incoming gradient, and relaxed samples near -100 in float32 (exp(logits - z) overflows):
    the isnan and isinf patterns are the torch body's on the same device tensors, with one and with two sample rows
    per parameter row."""
    dt, dtype = "float32", torch.float32
    for S, B, V in ((1, 4, 5), (2, 3, 70)):
        t = {k: x.clone() for k, x in case(family, dt, S, B, V, seed=3).items()}
        t["z"][..., 0, 1] = -100.0
        t["zcond"][..., 0, 1] = -100.0
        t["zcond"][..., B - 1, :] -= 100.0  # (a whole row, its arg-max kept)
        for name in OPS:
            param, x1, x2 = (None if x is None else x.to(DEV) for x in arguments(name, t))
            g = ref.upstream((S, B) if _reduces(family, name) else (S, B, V), dtype).to(DEV)
            flat = g.view(-1)
            flat[0], flat[flat.numel() // 2], flat[-1] = float("inf"), float("nan"), -float("inf")
            _against_body(family, name, dt, g, param, x1, x2, "non-finite {} {}".format(S, V))


def _public(dist, name, data, sample=()):
    if name == "rsample":
        with C.noise(data[0]):
            return dist.rsample(sample)
    if name == "csample":
        with C.noise(data[1]):
            return dist.csample(data[0])
    return getattr(dist, name)(*data)


def _layout_check(family, dt, dist, data_shape, up_kind, what):
    """Every method of ``dist`` (its parameter in any layout, and in the graph), through ``autograd.grad`` with
    respect to the tensor the method reads: the gradient has that tensor's shape and holds to the summed bound."""
    dtype, eps = DTYPES[dt], float(torch.finfo(DTYPES[dt]).eps)
    fam = ref.FAMILY[family]
    gen = torch.Generator().manual_seed(41)
    data_shape = tuple(data_shape)
    read = {"logits": dist.logits, "probs": dist.probs}
    assert all(x.requires_grad for x in read.values())
    l64, p64 = ref.f64(dist.logits).cpu(), ref.f64(dist.probs).cpu()
    u, v = ((torch.rand(data_shape, dtype=torch.float64, generator=gen) * 0.96 + 0.02).to(dtype) for _ in range(2))
    z = fam["rsample"](l64, ref.f64(u), eps).to(dtype)
    b = fam["threshold"](ref.f64(z)).to(dtype)
    zcond = fam["csample"](p64, ref.f64(b), ref.f64(v), eps).to(dtype)
    sample = data_shape[:len(data_shape) - l64.dim()]
    worst = 0.0
    for name in OPS:
        x1, x2 = {"rsample": (u, None), "tlog_prob": (b, None), "csample": (b, v), "log_prob": (z, None),
                  "clog_prob": (zcond, b)}[name]
        wrt = read[ref.WRT[OUTPUT[name]]]
        if name == "rsample" and sample + tuple(l64.shape) != data_shape:
            continue  # (rsample draws the parameter's own shape: no data to broadcast)
        out = _public(dist, name, tuple(x.to(DEV) for x in (x1, x2) if x is not None), sample)
        assert tuple(out.shape) == (data_shape[:-1] if _reduces(family, name) else data_shape), (what, name)
        up = ref.upstream(out.shape, dtype)
        if up_kind == "expanded":
            up, up_dev = torch.full(out.shape, 0.5, dtype=dtype), torch.tensor(0.5, dtype=dtype, device=DEV).expand(out.shape)
            assert not up_dev.is_contiguous()
        elif up_kind == "slice":
            up_dev = torch.stack([up, -up], -1).to(DEV)[..., 0]
            assert not up_dev.is_contiguous()
        else:
            up_dev = up.to(DEV)
        (got,) = torch.autograd.grad(out, wrt, up_dev, retain_graph=True)
        assert got.shape == wrt.shape and got.dtype == dtype, (what, name)
        full = (p64 if name == "csample" else l64).expand(data_shape)
        terms, _ = yardstick(family, name, full, x1, x2, up, eps)
        figure = summed_units(got, terms, tuple(wrt.shape), eps)
        worst = max(worst, figure)
        assert figure <= C.tolerance(family, "g_" + OUTPUT[name], dt), (what, name, figure)
    print(family, dt, what, "units", round(worst, 2))


@pytest.mark.parametrize("dt", list(DTYPES))
@pytest.mark.parametrize("family", FAMILIES)
def test_layouts(family, dt):
    dtype = DTYPES[dt]
    gen = torch.Generator().manual_seed(43)
    base = (2 * torch.randn((3, 4, 70), generator=gen, dtype=torch.float64)).to(dtype).to(DEV)
    leaf = lambda t: t.detach().requires_grad_(True)  # noqa: E731  (a view keeps its strides)
    build = lambda t, from_probs=False: C.build(family, leaf(t), from_probs)  # noqa: E731
    check = lambda dist, shape, what, up="plain": _layout_check(family, dt, dist, shape, up, what)  # noqa: E731
    if family == "bernoulli":  # (the logits handed in are the tensor the kernels read)
        # stride 0 in front, between dimensions (the dense copy), on the row itself; a 0-dimensional parameter
        for view, what in ((base[0, 0].expand(2, 3, 70), "front"), (base[:, :1].expand(3, 4, 70), "between"),
                           (base[..., :1].expand(3, 4, 70), "row")):
            dist = build(view)
            assert 0 in dist.logits.stride() and dist.logits.shape == view.shape
            check(dist, (2,) + tuple(view.shape), what)
        assert base[0, 0, 0].dim() == 0
        check(build(base[0, 0, 0]), (5, 3), "scalar")
        check(build(base[0].sigmoid(), True), (2, 4, 70), "probs")
        check(build(base[0, :, :1].contiguous()), (3, 4, 5), "size-1 row")
    else:  # (the logits are normalised into a dense tensor: its expansion is what carries stride 0)
        dist = build(base[0]).expand([5, 4])
        assert dist.logits.stride(0) == 0
        check(dist, (2, 5, 4, 70), "front")
        dist = build(base[:, :1]).expand([3, 4])
        assert dist.logits.stride(1) == 0 and dist.logits.stride(0) != 0
        check(dist, (2, 3, 4, 70), "between")
        check(build(base[0].softmax(-1) * 3, True), (2, 4, 70), "probs")
    # a data argument over a size-1 batch dimension of the parameter: in the middle (a copy) and in front
    check(build(base[:2, :1, :7].contiguous()), (2, 3, 7), "size-1 inside")
    check(build(base[:1, :3, :7].contiguous()), (2, 3, 7), "size-1 in front")
    check(build(base[:2, :1, :7].contiguous()), (4, 2, 3, 7), "size-1 inside, samples")
    # the upstream gradient as an expanded scalar and as a non-contiguous slice
    check(build(base[0]), (3, 4, 70), "expanded upstream", "expanded")
    check(build(base[0]), (3, 4, 70), "sliced upstream", "slice")


@pytest.mark.parametrize("family", FAMILIES)
def test_determinism(family):
    lib = _lib()
    for S, B, V in ((7, 3, 65), (64, 1, 65), (40, 2, 5)):
        assert (lib.pdt_relaxed_backward_parts(S * B, B, V) > 1) == (B < 3)
        t = case(family, "float32", S, B, V, seed=9)
        for name in OPS:
            param, x1, x2 = (None if x is None else x.to(DEV) for x in arguments(name, t))
            g = ref.upstream((S, B) if _reduces(family, name) else (S, B, V), torch.float32).to(DEV)
            want = 3 if name in ("log_prob", "clog_prob") else 1
            first, again = (backward(family, name, g, param, x1, x2, B, want) for _ in range(2))
            assert torch.equal(first[0], again[0]) and (want == 1 or torch.equal(first[1], again[1]))


@pytest.mark.parametrize("family", FAMILIES)
def test_second_derivative(family):
    """create_graph=True through the operator, then the gradient of the squared norm of the estimate with respect
    to the incoming gradient, the parameter and z / zcond, against the same on the differentiable torch formulas."""
    from pydrobert_amd import _relaxed as X

    fam = X.GUMBEL if family == "gumbel" else X.BERNOULLI
    t = {k: x.to(DEV) for k, x in case(family, "float64", 4, 3, 5, seed=11).items()}
    for name in OPS:
        results = []
        for route in ("operator", "torch"):
            param, x1, x2 = arguments(name, t)
            param = param.clone().requires_grad_(True)
            has_x1 = name in ("log_prob", "clog_prob")
            x1 = x1.clone().requires_grad_(has_x1)
            fn = torch.ops.pydrobert_amd.relaxed if route == "operator" else (lambda f, o, *a: X._TORCH[f](o, *a))
            out = fn(fam, OPS[name], param, x1, x2)
            up = ref.upstream(out.shape).to(DEV).requires_grad_(True)
            first = torch.autograd.grad(out, [param] + ([x1] if has_x1 else []), up, create_graph=True)
            norm = sum(d.pow(2).sum() for d in first)
            second = torch.autograd.grad(norm, [up, param] + ([x1] if has_x1 else []), allow_unused=True)
            results.append((first, second))
        worst = 0.0
        for got, want in zip(results[0][0] + results[0][1], results[1][0] + results[1][1]):
            if got is None or want is None:  # (no path, or a zero)
                assert all(x is None or not x.any() for x in (got, want)), name
            else:
                worst = max(worst, float(((got - want).abs() / (1 + want.abs())).max().detach()))
        print(family, name, "second derivative", worst)
        assert worst <= 1e-9, name
        assert any(w is not None and w.abs().max() > 1e-3 for w in results[1][1]), name  # (a real one, not a zero)


def test_op_registration_and_compile():
    from torch.library import opcheck

    tests = ("test_schema", "test_faketensor", "test_autograd_registration")
    for family in FAMILIES:
        t = {k: x.to(DEV) for k, x in case(family, "float64", 2, 3, 5, seed=13).items()}
        for name in OPS:
            param, x1, x2 = arguments(name, t)
            has_x1 = name in ("log_prob", "clog_prob")
            g = ref.upstream((2, 3) if _reduces(family, name) else (2, 3, 5)).to(DEV).requires_grad_(True)
            args = (FAMILIES.index(family), OPS[name], 3 if has_x1 else 1, g, param.clone().requires_grad_(True),
                    x1.clone().requires_grad_(has_x1), x2)
            opcheck(torch.ops.pydrobert_amd.relaxed_backward.default, args, test_utils=tests)
    t = {k: x.to(DEV) for k, x in case("gumbel", "float32", 2, 3, 5, seed=13).items()}

    def fn(logits, z):
        return C.build("gumbel", logits, False, validate_args=False).log_prob(z).sum()

    grads = []
    for f in (fn, torch.compile(fn, backend="aot_eager", fullgraph=True)):
        logits, z = t["logits"].clone().requires_grad_(True), t["z"].clone().requires_grad_(True)
        grads.append(torch.autograd.grad(f(logits, z), [logits, z]))
    for a, b in zip(*grads):
        assert torch.equal(a, b)


def test_non_default_stream():
    """The backward kernels, both launches of the parts form included, are enqueued on torch's current stream."""
    def run():
        outs = []
        for S, B, V in ((3, 2, 65), (64, 1, 65)):
            t = case("gumbel", "float32", S, B, V, seed=15)
            for name in OPS:
                param, x1, x2 = (None if x is None else x.to(DEV) for x in arguments(name, t))
                g = ref.upstream((S, B) if _reduces("gumbel", name) else (S, B, V), torch.float32).to(DEV)
                outs += [x for x in backward("gumbel", name, g, param, x1, x2, B, 3 if name in ("log_prob", "clog_prob") else 1)
                         if x is not None]
            logits = t["logits"].to(DEV).requires_grad_(True)
            dist = C.build("gumbel", logits, False)
            outs += list(torch.autograd.grad(dist.clog_prob(t["zcond"].to(DEV), t["b"].to(DEV)).sum(), logits))
        return outs

    want = run()
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        got = run()
    side.synchronize()
    assert len(got) == len(want)
    for a, b in zip(got, want):
        assert torch.equal(a, b)


def test_no_derivative_of_the_noise():
    from pydrobert_amd import _relaxed as X

    logits = torch.randn(2, 3, device=DEV)
    u = (torch.rand(4, 2, 3, device=DEV) * 0.9 + 0.05).requires_grad_(True)
    z = torch.ops.pydrobert_amd.relaxed(X.GUMBEL, X.RSAMPLE, logits, u, None)
    with pytest.raises(NotImplementedError, match="method 0 has no derivative with respect to its first data argument"):
        z.sum().backward()
    b = torch.eye(3, device=DEV)[:2].expand(4, 2, 3)
    zc = torch.ops.pydrobert_amd.relaxed(X.BERNOULLI, X.CSAMPLE, logits.sigmoid().requires_grad_(True), b, u)
    with pytest.raises(NotImplementedError, match="method 3 has no derivative with respect to its second data argument"):
        zc.sum().backward()
