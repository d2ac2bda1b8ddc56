"""The yardstick of the fused ConcatSoftAttention score (csrc/concat_score.hip, ``pydrobert_amd::concat_score``).

* ``score_ref`` / ``grads_ref``: the float64 formula of the score and of its three gradients, written out (no
  autograd): e = sum_h v tanh(wq + wk); g = dE v (1 - tanh^2); dwq, dwk = g summed to their shapes; dv = sum dE tanh.
* ``plan_of``: a Python restatement of the plan the library reports through ``pdt_concat_score_plan``.
* ``CASES``: named cases, each with the plan form it claims to reach and, for float32, the measured bounds above the
  suite's: 8 x err32 rounded up to two digits, err32 the error against float64 of the formula in float32 arithmetic
  on the case's inputs (``formula32``: every operation written out, so the figure is the same on every machine).
  tests/test_concat_score_cpu.py recomputes each and holds the table to ``measured_bound`` exactly.

A case is a module call: ``query`` of shape ``q + (DQ,)``, ``key`` of shape ``k + (DK,)``, the attended axis ``dim``.
The operator sees wq = linear(query.unsqueeze(dim), W[:, :DQ], b) and wk = linear(key, W[:, DQ:]).  ``view`` changes
how wk reaches the operator: "t" a transposed view (hidden axis not innermost in memory), "x" expanded with
stride 0 along the axes where ``k`` has size 1 (so that nothing is grouped and wk's gradient has one slice per index).
"""
import functools

import numpy as np
import torch

DQ, DK = 3, 4
SUITE = {"float32": (2e-5, 1e-4), "float64": (1e-9, 1e-8)}  # (output, gradients): the suite's bounds
TENSORS = ("e", "wq", "wk", "v", "weight", "bias")

ROWS, FRAMES, MIN_FRAMES, CHUNK, LDS, FILL = 8, 32, 4, 2048, 57344, 1024


def plan_of(G, M, T, H, esz):
    """(rows per forward tile, H chunks, frames per forward workgroup, backward frame chunks, backward workspace
    bytes) of a call with G groups of M rows: csrc/concat_score.hip, concat_plan."""
    if G * M == 0 or T == 0 or H == 0:
        return dict(rt=0, hchunks=0, fpw=0, chunks=0, ws=0)
    hc = min(H, CHUNK)
    rt = min(ROWS, M, LDS // (hc * esz) - 1)
    tiles = -(-M // rt)
    fpw = FRAMES
    while fpw > MIN_FRAMES and G * tiles * -(-T // fpw) < FILL:
        fpw //= 2
    chunks = -(-T // FRAMES)
    ws = (G * chunks * H + (chunks * G * M * H if chunks > 1 else 0)) * esz
    return dict(rt=rt, hchunks=-(-H // hc), fpw=fpw, chunks=chunks, ws=ws)


def score_ref(wq, wk, v):
    return (torch.tanh(wq + wk) * v).sum(-1)


def grads_ref(grad_e, wq, wk, v):
    th = torch.tanh(wq + wk)
    ge = grad_e.unsqueeze(-1)
    g = ge * v * (1 - th * th)
    return g.sum_to_size(wq.shape), g.sum_to_size(wk.shape), (ge * th).reshape(-1, v.shape[0]).sum(0)


CASES = {}


def _case(name, test, dtype, q, k, dim, H, form, view=None, tol=None):
    assert name not in CASES, name
    CASES[name] = dict(test=test, dtype=dtype, q=tuple(q), k=tuple(k), dim=dim, H=H, form=form, view=view,
                       tol=dict(tol or {}))  # fmt: skip


def cases_of(test):
    return [n for n, c in CASES.items() if c["test"] == test]


def geometry(c):
    """(S, G, M) of a case: the score's shape, the groups and the rows per group the operator forms."""
    q1 = list(c["q"])
    q1.insert(c["dim"], 1)
    k = list(c["k"]) if c["view"] != "x" else [max(a, b) for a, b in zip(q1, c["k"])]
    S = [max(a, b) for a, b in zip(q1, k)]
    rows = [i for i in range(len(S)) if i != c["dim"] and S[i] > 1]
    M = int(np.prod([S[i] for i in rows if k[i] == 1], dtype=np.int64))
    R = int(np.prod([S[i] for i in rows], dtype=np.int64))
    return S, R // M, M


# the hidden axis: the lanes' tail (1, 5, 63 .. 65), several strides of the four loads in flight (257, 1000), the
# chunk loop and its one-element tail (2049).  Decode layout, 2 utterances of 3 beams, 5 frames.
_H_TOL = {1000: dict(e=4.2e-5), 2049: dict(e=5.8e-5)}  # 8 x err32: a sum of H terms of size |v|
for _H in (1, 5, 63, 64, 65, 257, 1000, 2049):
    _case("H%d" % _H, "hidden", "float32", (2, 3), (5, 2, 1), 0, _H,
          dict(rt=3, hchunks=2 if _H > 2048 else 1, fpw=4, chunks=1), tol=_H_TOL.get(_H))  # fmt: skip
_case("H65_f64", "hidden", "float64", (2, 3), (5, 2, 1), 0, 65, dict(rt=3, hchunks=1, fpw=4, chunks=1))
_case("H2049_f64", "hidden", "float64", (2, 3), (5, 2, 1), 0, 2049, dict(rt=2, hchunks=2, fpw=4, chunks=1))
# the group: 1 (training: query (N, Dq), key (T, N, Dk)), 8 beams, a full tile + 1, two tiles + 1
_case("M1", "group", "float32", (3,), (7, 3), 0, 65, dict(rt=1, hchunks=1, fpw=4, chunks=1))
for _M in (8, 9, 17):
    _case("M%d" % _M, "group", "float32", (2, _M), (7, 2, 1), 0, 65, dict(rt=8, hchunks=1, fpw=4, chunks=1))
_case("M17_f64", "group", "float64", (2, 17), (7, 2, 1), 0, 65, dict(rt=8, hchunks=1, fpw=4, chunks=1))
# a row tile reduced by LDS: float64, two chunks of 2048 features, 2 rows per tile for a group of 3
_case("lds_f64", "lds", "float64", (1, 3), (3, 1, 1), 0, 4096, dict(rt=2, hchunks=2, fpw=4, chunks=1))
_case("lds_f32", "lds", "float32", (1, 7), (3, 1, 1), 0, 2100, dict(rt=6, hchunks=2, fpw=4, chunks=1),
      tol=dict(e=4.6e-5))  # fmt: skip
# the attended axis: one frame, the 32-frame chunk and both sides of it, three backward chunks
for _T in (1, 31, 32, 33, 96):
    _form = dict(hchunks=1, fpw=4, chunks=-(-_T // 32))
    _case("T%d_train" % _T, "frames", "float32", (2,), (_T, 2), 0, 5, dict(rt=1, **_form))
    _case("T%d_decode" % _T, "frames", "float32", (2, 2), (_T, 2, 1), 0, 5, dict(rt=2, **_form))
_case("T96_f64", "frames", "float64", (2, 2), (96, 2, 1), 0, 5, dict(rt=2, hchunks=1, fpw=4, chunks=3))
# frames per forward workgroup: 32 once the rows fill the chip, 16 and 8 below (4 everywhere above).  The
# gradients of v, weight and bias are sums over 1 k to 9 k (row, frame) pairs here
_case("fpw32", "fill", "float32", (1024,), (1, 1024), 0, 5, dict(rt=1, hchunks=1, fpw=32, chunks=1))
_case("fpw16", "fill", "float32", (512,), (17, 512), 0, 5, dict(rt=1, hchunks=1, fpw=16, chunks=1))
_case("fpw8", "fill", "float32", (512, 2), (9, 512, 1), 0, 5, dict(rt=2, hchunks=1, fpw=8, chunks=1),
      tol=dict(v=1.7e-4, weight=1.2e-4))  # fmt: skip
# layouts: transformer-like (the group dim L is not innermost in memory), batch first, a transposed wk, a key
# expanded with stride 0 (nothing grouped: its gradient keeps one slice per beam)
_case("xfmr", "layout", "float32", (9, 3), (40, 1, 3), 0, 65, dict(rt=8, hchunks=1, fpw=4, chunks=2))
_case("xfmr_f64", "layout", "float64", (9, 3), (40, 1, 3), 0, 65, dict(rt=8, hchunks=1, fpw=4, chunks=2))
_case("batch_first", "layout", "float32", (3, 4), (3, 35, 1), 1, 65, dict(rt=4, hchunks=1, fpw=4, chunks=2))
_case("two_groups", "layout", "float32", (2, 3, 2), (6, 2, 1, 1), 0, 33, dict(rt=6, hchunks=1, fpw=4, chunks=1))
_case("transposed", "layout", "float32", (2, 3), (35, 2, 1), 0, 65, dict(rt=3, hchunks=1, fpw=4, chunks=2), view="t")
_case("expanded", "layout", "float32", (2, 3), (35, 2, 1), 0, 65, dict(rt=1, hchunks=1, fpw=4, chunks=2), view="x")
_case("expanded_f64", "layout", "float64", (2, 3), (35, 2, 1), 0, 65, dict(rt=1, hchunks=1, fpw=4, chunks=2),
      view="x")  # fmt: skip


@functools.lru_cache(maxsize=None)
def build_inputs(name):
    """float64 numpy inputs of a case, the same on every call: query, key, weight, bias, v and the upstream
    gradient of the score.  Treat as read-only."""
    c = CASES[name]
    rng = np.random.default_rng(sum(ord(ch) * (i + 1) for i, ch in enumerate(name)))
    S, _, _ = geometry(c)
    H = c["H"]
    x = dict(
        query=rng.normal(size=c["q"] + (DQ,)), key=rng.normal(size=c["k"] + (DK,)),
        weight=rng.normal(size=(H, DQ + DK)) * 0.5, bias=rng.normal(size=(H,)) * 0.5,
        v=rng.normal(size=(H,)), gout=rng.normal(size=tuple(S)),
    )  # fmt: skip
    for a in x.values():
        a.setflags(write=False)
    return x


def tensors(name, dtype, device):
    """The case's inputs as leaves of ``dtype`` on ``device`` (rounded to the case's own dtype first, so that every
    route sees the same numbers)."""
    c = CASES[name]
    own = torch.float32 if c["dtype"] == "float32" else torch.float64
    return {
        n: torch.from_numpy(a.copy()).to(own).to(device=device, dtype=dtype).requires_grad_(n != "gout")
        for n, a in build_inputs(name).items()
    }


def halves(name, t):
    """wq and wk of the case as the module forms them, and wk as the operator is to see it (``view``)."""
    c = CASES[name]
    wq = torch.nn.functional.linear(t["query"].unsqueeze(c["dim"]), t["weight"][:, :DQ], t["bias"])
    wk = torch.nn.functional.linear(t["key"], t["weight"][:, DQ:], None)
    return wq, wk


def as_seen(name, wk, S):
    c = CASES[name]
    if c["view"] == "t":  # the same values with the hidden axis outermost in memory
        return wk.movedim(-1, 0).contiguous().movedim(0, -1)
    if c["view"] == "x":
        return wk.expand(list(S) + [wk.shape[-1]])
    return wk


def run_case(name, score, dtype, device):
    """e and the gradients of ``TENSORS`` with ``score(wq, wk, v, dim)``: wq and wk are cut from the graph and fed as
    leaves (their gradients are the operator's own), then the chain goes on to weight and bias through torch."""
    c = CASES[name]
    t = tensors(name, dtype, device)
    S, _, _ = geometry(c)
    wq, wk = halves(name, t)
    lq = wq.detach().requires_grad_(True)
    lk = as_seen(name, wk.detach(), S).requires_grad_(True)
    lv = t["v"].detach().requires_grad_(True)
    e = score(lq, lk, lv, c["dim"])
    gq, gk, gv = torch.autograd.grad(e, (lq, lk, lv), t["gout"])
    gw, gb = torch.autograd.grad((wq, wk), (t["weight"], t["bias"]), (gq, gk.sum_to_size(wk.shape)))
    out = dict(e=e, wq=gq, wk=gk, v=gv, weight=gw, bias=gb)
    return {n: x.detach() for n, x in out.items()}


@functools.lru_cache(maxsize=None)
def expected(name):
    """The float64 reference of a case by the written-out formulas.  Cached: treat as read-only."""
    c = CASES[name]
    t = tensors(name, torch.float64, "cpu")
    S, _, _ = geometry(c)
    wq, wk = halves(name, t)
    seen = as_seen(name, wk.detach(), S)
    e = score_ref(wq.detach(), seen, t["v"].detach())
    gq, gk, gv = grads_ref(t["gout"], wq.detach(), seen, t["v"].detach())
    gw, gb = torch.autograd.grad((wq, wk), (t["weight"], t["bias"]), (gq, gk.sum_to_size(wk.shape)))
    return dict(e=e, wq=gq, wk=gk, v=gv, weight=gw, bias=gb)


def _tree_sum(x, dim):
    """The sum along ``dim`` as a balanced tree of elementwise additions (halves added, an odd length padded with a
    zero): every addition is one IEEE operation of ``x``'s type, in an order that is written here."""
    x = x.movedim(dim, 0)
    while x.shape[0] > 1:
        if x.shape[0] % 2:
            x = torch.cat([x, torch.zeros_like(x[:1])])
        half = x.shape[0] // 2
        x = x[:half] + x[half:]
    return x[0] if x.shape[0] else torch.zeros(x.shape[1:], dtype=x.dtype)


def _tree_sum_to(x, shape):
    """``x.sum_to_size(shape)`` with ``_tree_sum`` along each reduced axis, outermost first."""
    for i, n in enumerate(shape):
        if n == 1 and x.shape[i] != 1:
            x = _tree_sum(x, i).unsqueeze(i)
    return x


def _linear32(x, w, b):
    """x @ w.T (+ b) with the products added one after another in ``x``'s type."""
    out = x[..., None, 0] * w[:, 0]
    for i in range(1, w.shape[1]):
        out = out + x[..., None, i] * w[:, i]
    return out if b is None else out + b


def formula32(name):
    """The formulas in float32 arithmetic, every operation and its order written out so that the result is the same
    on every machine: products and sums are single IEEE float32 operations (the sums balanced trees), and tanh is
    the correctly rounded one (evaluated in float64, rounded to float32).  No library kernel whose order of
    summation or whose tanh depends on the host's vector width, BLAS or thread count takes part."""
    c = CASES[name]
    t = {n: x.detach() for n, x in tensors(name, torch.float32, "cpu").items()}
    S, _, _ = geometry(c)
    H = c["H"]
    x_q, x_k = t["query"].unsqueeze(c["dim"]), t["key"]
    wq = _linear32(x_q, t["weight"][:, :DQ], t["bias"])
    wk = _linear32(x_k, t["weight"][:, DQ:], None)
    seen = as_seen(name, wk, S)
    th = torch.tanh((wq + seen).double()).float()
    v = t["v"]
    e = _tree_sum(th * v, -1)
    ge = t["gout"].unsqueeze(-1)
    g = ge * v * (1 - th * th)
    gq, gk = _tree_sum_to(g, wq.shape), _tree_sum_to(g, seen.shape)
    gv = _tree_sum((ge * th).reshape(-1, H), 0)
    gk_own = _tree_sum_to(gk, wk.shape)
    gw_q = _tree_sum((gq.unsqueeze(-1) * x_q.unsqueeze(-2)).reshape(-1, H, DQ), 0)
    gw_k = _tree_sum((gk_own.unsqueeze(-1) * x_k.unsqueeze(-2)).reshape(-1, H, DK), 0)
    gb = _tree_sum(gq.reshape(-1, H), 0)
    return dict(e=e, wq=gq, wk=gk, v=gv, weight=torch.cat([gw_q, gw_k], 1), bias=gb)


def formula32_error(name):
    """err32 by tensor: the largest absolute error of ``formula32`` against ``expected``."""
    got = formula32(name)
    return {n: float((got[n].double() - ref).abs().max()) for n, ref in expected(name).items()}


def measured_bound(err32, suite):
    """The rule: the suite's bound, or 8 x err32 where that is larger, rounded up to two digits."""
    if 8 * err32 <= suite:
        return suite
    ex = int(np.floor(np.log10(8 * err32))) - 1
    return float("%.1e" % (np.ceil(8 * err32 / 10.0 ** ex - 1e-9) * 10.0 ** ex))


def bound(name, tensor):
    """(rtol, atol) of a tensor of a case: the suite's bound, or the case's measured one as atol."""
    c = CASES[name]
    suite = SUITE[c["dtype"]][0 if tensor == "e" else 1]
    return suite, c["tol"].get(tensor, suite)


def compare(name, got, log=print):
    """Every tensor of a run against ``expected`` within ``bound``.  Prints each figure first."""
    failures = []
    for n, ref in expected(name).items():
        x = got[n].double().cpu()
        rtol, atol = bound(name, n)
        assert x.shape == ref.shape, (n, x.shape, ref.shape)
        err = float((x - ref).abs().max()) if x.numel() else 0.0
        fine = bool(torch.isfinite(x).all()) and bool(((x - ref).abs() <= atol + rtol * ref.abs()).all())
        log("{} {}: max abs error {:.3e} (atol {:.1e}, rtol {:.1e}){}".format(name, n, err, atol, rtol, "" if fine else " FAIL"))
        if not fine:
            failures.append((n, err))
    assert not failures, (name, failures)


# the view beyond 2^32 elements (tests/_wide.py): wk (T, N, 1, H) with the batch stride wide
WIDE = dict(T=9, N=2, K=3, H=65, wide_dim=1)
