#!/usr/bin/env python
"""Generate tests/golden/attn.npz and attn_signatures.json from the LIVE reference's attention modules
(GlobalSoftAttention and its four subclasses).

Run in the build container only (the reference never travels to the GPU box):

    PYTHONPATH=/root/reference/src python tests/golden/make_attn_golden.py

Every array is DATA: inputs this script draws, the seeded parameters and what the reference returned for
them.  Case k stores ``case_<k>_spec`` (a JSON string: module, constructor arguments, dim, dtype),
``case_<k>_<input>``, ``case_<k>_param_<name>``, ``case_<k>_out`` and ``case_<k>_grad_<name>`` for every
input and parameter that receives a gradient.  Error cases store the reference's exception type name.
"""
import inspect
import json
import os
import sys
import warnings

import numpy as np
import torch

REF = os.environ.get("PDT_REFERENCE", "/root/reference")
sys.path.insert(0, os.path.join(REF, "src"))
HERE = os.path.dirname(os.path.abspath(__file__))

import pydrobert.torch.modules as RM  # noqa: E402

warnings.simplefilter("ignore")
rng = np.random.default_rng(0xA77E)
out = {}
NAMES = ("GlobalSoftAttention", "DotProductSoftAttention", "GeneralizedDotProductSoftAttention",
         "ConcatSoftAttention", "MultiHeadedAttention")


def put(key, v):
    if isinstance(v, torch.Tensor):
        v = v.detach().cpu().numpy()
    out[key] = np.array(v)  # (a copy: reset_parameters() writes the tensors in place)


def upstream(shape, dtype):
    """The fixed upstream gradient of every case (tests/test_attn_*.py restate it)."""
    n = int(np.prod(shape))
    return torch.cos(torch.arange(n, dtype=torch.float64) * 0.7).reshape(shape).to(dtype)


class CosineAttention(RM.GlobalSoftAttention):
    """A user subclass with its own score (tests/test_attn_*.py define the same one)."""

    def __init__(self, size, dim=0):
        super().__init__(size, size, dim)

    def score(self, query, key):
        query = query.unsqueeze(self.dim)
        return 3.0 * torch.nn.functional.cosine_similarity(query, key, dim=-1)


def build(spec):
    kind, args = spec["module"], spec["args"]
    if kind == "MultiHeadedAttention":
        head = build(spec["head"])
        return RM.MultiHeadedAttention(*args, single_head_attention=head, **spec.get("kw", {}))
    cls = CosineAttention if kind == "CosineAttention" else getattr(RM, kind)
    return cls(*args)


def length_mask(T, shape, t_axis, lens):
    """bool mask of `shape` whose t_axis positions below lens (broadcast over the other axes) are True."""
    t = torch.arange(T).view([-1 if i == t_axis else 1 for i in range(len(shape))])
    return t < lens


def case(k, spec, q_shape, k_shape, v_shape, mask=None, seed=0):
    dtype = getattr(torch, spec.get("dtype", "float64"))
    torch.manual_seed(seed)
    m = build(spec).to(dtype)
    q = torch.from_numpy(rng.standard_normal(q_shape)).to(dtype).requires_grad_(True)
    key = torch.from_numpy(rng.standard_normal(k_shape)).to(dtype).requires_grad_(True)
    value = torch.from_numpy(rng.standard_normal(v_shape)).to(dtype).requires_grad_(True)
    y = m(q, key, value, mask)
    params = dict(m.named_parameters())
    ins = [q, key, value] + list(params.values())
    grads = torch.autograd.grad(y, ins, upstream(tuple(y.shape), dtype), allow_unused=True)
    pre = "case_{}_".format(k)
    put(pre + "spec", json.dumps(spec))
    put(pre + "query", q)
    put(pre + "key", key)
    put(pre + "value", value)
    if mask is not None:
        put(pre + "mask", mask)
    put(pre + "out", y)
    for name, p in params.items():
        put(pre + "param_" + name, p)
    for name, g in zip(["query", "key", "value"] + list(params), grads):
        if g is not None:
            put(pre + "grad_" + name, g)


def cases():
    dot = lambda D, dim=0, s=1.0: {"module": "DotProductSoftAttention", "args": [D, dim, s]}  # noqa: E731
    gen = lambda Dq, Dk, dim=0, b=False: {"module": "GeneralizedDotProductSoftAttention", "args": [Dq, Dk, dim, b]}  # noqa: E731,E501
    cat = lambda Dq, Dk, dim=0, b=False, H=7: {"module": "ConcatSoftAttention", "args": [Dq, Dk, dim, b, H]}  # noqa: E731,E501
    lens3 = torch.tensor([5, 2, 4])
    specs = [
        # dim 0, 1, 2 and a negative dim
        (dot(4, 0), (3, 4), (5, 3, 4), (5, 3, 2), None),
        (dot(4, 1, 0.5), (3, 4), (3, 5, 4), (3, 5, 6), length_mask(5, (3, 5), 1, torch.tensor([[5], [1], [3]]))),
        (dot(4, 2), (2, 3, 4), (2, 3, 5, 4), (2, 3, 5, 3), torch.rand(2, 3, 5) < 0.7),
        (dot(4, -2), (3, 5, 4), (3, 5, 6, 4), (3, 5, 6, 2), None),
        # the beam pattern: query (N, K, D), key (T, N, 1, D), a length mask
        (dot(5, 0, 0.3), (3, 4, 5), (6, 3, 1, 5), (6, 3, 1, 7), length_mask(6, (6, 3, 1), 0, torch.tensor([[6], [2], [4]]))),
        # the transformer pattern: query (Lq, N, D), key (T, 1, N, D), a causal mask (T, Lq, 1)
        (dot(5, 0, 0.4), (4, 2, 5), (6, 1, 2, 5), (6, 1, 2, 3), (torch.arange(6).view(6, 1, 1) <= torch.arange(4).view(1, 4, 1) + 2)),
        # mask broadcast over a batch axis, and an all-masked row
        (dot(4, 0), (3, 4), (5, 3, 4), (5, 3, 2), length_mask(5, (5, 3), 0, torch.tensor([5, 0, 2]))),
        # value broadcast along T
        (dot(4, 0), (3, 4), (5, 3, 4), (1, 3, 2), length_mask(5, (5, 3), 0, lens3)),
        # T = 1 and T = 0
        (dot(4, 0), (3, 4), (1, 3, 4), (1, 3, 2), None),
        (dot(4, 0), (3, 4), (0, 3, 4), (0, 3, 2), None),
        (dot(4, 1), (3, 4), (3, 0, 4), (3, 0, 5), torch.zeros(3, 0, dtype=torch.bool)),
        # a user subclass with its own score
        ({"module": "CosineAttention", "args": [4, 0]}, (3, 4), (5, 3, 4), (5, 3, 2), length_mask(5, (5, 3), 0, lens3)),
        # generalized and concat, bias off and on
        (gen(3, 4, 0, False), (2, 3), (5, 2, 4), (5, 2, 3), None),
        (gen(3, 4, 1, True), (2, 3), (2, 5, 4), (2, 5, 3), length_mask(5, (2, 5), 1, torch.tensor([[5], [3]]))),
        (gen(3, 4, 0, True), (3, 2, 3), (5, 3, 1, 4), (5, 3, 1, 2), length_mask(5, (5, 3, 1), 0, torch.tensor([[5], [1], [3]]))),
        (cat(3, 4, 0, False), (2, 3), (5, 2, 4), (5, 2, 3), None),
        (cat(3, 4, 1, True), (2, 3), (2, 5, 4), (2, 5, 3), length_mask(5, (2, 5), 1, torch.tensor([[5], [3]]))),
        # multi-head: generalized and concat heads
        ({"module": "MultiHeadedAttention", "args": [6, 5, 4, 2], "kw": {"bias_WQ": True, "bias_WC": True},
          "head": gen(3, 2, 0, True)}, (4, 2, 6), (5, 1, 2, 5), (5, 1, 2, 4),
         length_mask(5, (5, 4, 1), 0, torch.tensor([[5], [1], [3], [4]]))),
        ({"module": "MultiHeadedAttention", "args": [6, 5, 4, 2], "kw": {"d_v": 3, "out_size": 7},
          "head": cat(3, 2, 1, False, 5)}, (3, 6), (3, 5, 5), (3, 5, 4), None),
        ({"module": "MultiHeadedAttention", "args": [8, 8, 8, 4], "head": dot(2, 0, 0.5)}, (4, 2, 8), (6, 1, 2, 8),
         (6, 1, 2, 8), (torch.arange(6).view(6, 1, 1) <= torch.arange(4).view(1, 4, 1) + 2)),
        # float32
        (dict(dot(8, 0, 0.25), dtype="float32"), (3, 4, 8), (9, 3, 1, 8), (9, 3, 1, 5), length_mask(9, (9, 3, 1), 0, torch.tensor([[9], [4], [7]]))),
        (dict(gen(6, 8, 0, True), dtype="float32"), (3, 6), (9, 3, 8), (9, 3, 5), None),
    ]  # fmt: skip
    for k, (spec, qs, ks, vs, mask) in enumerate(specs):
        spec.setdefault("dim", spec["args"][1 if spec["module"] in ("CosineAttention", "DotProductSoftAttention") else 2] if spec["module"] != "MultiHeadedAttention" else spec["head"]["args"][2])
        case(k, spec, qs, ks, vs, mask, seed=100 + k)
    put("case_n", len(specs))


def seeded():
    """Parameters after construction under manual_seed(7), then after reset_parameters()."""
    specs = {
        "gen": ("GeneralizedDotProductSoftAttention", (5, 6, 0, True)),
        "gen_nobias": ("GeneralizedDotProductSoftAttention", (5, 6)),
        "cat": ("ConcatSoftAttention", (5, 6, 0, True, 9)),
        "cat_nobias": ("ConcatSoftAttention", (5, 6)),
    }
    for tag, (name, args) in specs.items():
        torch.manual_seed(7)
        m = getattr(RM, name)(*args)
        for pname, p in m.state_dict().items():
            put("seed_{}_init_{}".format(tag, pname), p)
        m.reset_parameters()
        for pname, p in m.state_dict().items():
            put("seed_{}_reset_{}".format(tag, pname), p)
    torch.manual_seed(7)
    m = RM.MultiHeadedAttention(6, 5, 4, 2, RM.GeneralizedDotProductSoftAttention(3, 2, 0, True), bias_WQ=True)
    for pname, p in m.state_dict().items():
        put("seed_mha_init_{}".format(pname), p)
    m.reset_parameters()
    for pname, p in m.state_dict().items():
        put("seed_mha_reset_{}".format(pname), p)
    put("seed_tags", json.dumps(list(specs) + ["mha"]))


def errors():
    q, k, v = torch.randn(3, 4), torch.randn(5, 3, 4), torch.randn(5, 3, 2)
    dot = RM.DotProductSoftAttention(4)
    mha = RM.MultiHeadedAttention(4, 4, 2, 2, RM.DotProductSoftAttention(2))
    cases = {
        "query_ndim": lambda: dot(torch.randn(4), k, v),
        "value_ndim": lambda: dot(q, k, torch.randn(5, 3, 2, 1)),
        "query_size": lambda: dot(torch.randn(3, 5), k, v),
        "key_size": lambda: RM.GeneralizedDotProductSoftAttention(4, 3)(q, k, v),
        "dim_range": lambda: RM.DotProductSoftAttention(4, dim=2)(q, k, v),
        "dim_minus_one": lambda: RM.DotProductSoftAttention(4, dim=-1)(q, k, v),
        "broadcast": lambda: dot(torch.randn(2, 4), k, v),
        "mask_broadcast": lambda: dot(q, k, v, torch.ones(4, 3, dtype=torch.bool)),
        "mask_not_bool": lambda: dot(q, k, v, torch.ones(5, 3)),
        "mha_query_ndim": lambda: mha(torch.randn(4), k, v),
        "mha_dim_range": lambda: RM.MultiHeadedAttention(4, 4, 2, 2, RM.DotProductSoftAttention(2, dim=2))(q, k, v),
        "mha_value_size": lambda: mha(q, k, torch.randn(5, 3, 3)),
        "mha_score": lambda: mha.score(q, k),
        "mha_negative_dim": lambda: RM.MultiHeadedAttention(4, 4, 2, 2, RM.DotProductSoftAttention(2, dim=-2)),
        "ctor_size": lambda: RM.DotProductSoftAttention(0),
        "ctor_bias": lambda: RM.GeneralizedDotProductSoftAttention(3, 4, 0, "yes"),
        "ctor_hidden": lambda: RM.ConcatSoftAttention(3, 4, hidden_size=0),
        "ctor_heads": lambda: RM.MultiHeadedAttention(4, 4, 2, 0, RM.DotProductSoftAttention(2)),
    }
    names = {}
    for key, fn in cases.items():
        try:
            fn()
            names[key] = "none"
        except Exception as e:  # noqa: BLE001
            names[key] = type(e).__name__
    put("errors", json.dumps(names))


def params(fn):
    fn = getattr(fn, "__wrapped__", fn)
    return [[p.name, p.default is not inspect.Parameter.empty, p.kind.name, repr(p.default)
             if p.default is not inspect.Parameter.empty else None]
            for p in inspect.signature(fn).parameters.values() if p.name != "self"]


def signatures():
    sig = {"modules": {}}
    samples = {
        "DotProductSoftAttention": RM.DotProductSoftAttention(4, 1, 0.5),
        "GeneralizedDotProductSoftAttention": RM.GeneralizedDotProductSoftAttention(3, 4, 1, True),
        "ConcatSoftAttention": RM.ConcatSoftAttention(3, 4, 0, True, 9),
        "MultiHeadedAttention": RM.MultiHeadedAttention(6, 5, 4, 2, RM.GeneralizedDotProductSoftAttention(3, 2),
                                                        bias_WQ=True, bias_WC=True),
    }  # fmt: skip
    for n in NAMES:
        cls = getattr(RM, n)
        entry = {"__init__": params(cls.__init__), "forward": params(cls.forward),
                 "score": params(cls.score), "check_input": params(cls.check_input),
                 "__constants__": list(cls.__constants__)}  # fmt: skip
        if n in samples:
            entry["extra_repr"] = samples[n].extra_repr()
            entry["state_dict"] = sorted(samples[n].state_dict())
        sig["modules"][n] = entry
    with open(os.path.join(HERE, "attn_signatures.json"), "w") as f:
        json.dump(sig, f, indent=1, sort_keys=True)


torch.manual_seed(0)
cases()
seeded()
errors()
signatures()
np.savez_compressed(os.path.join(HERE, "attn.npz"), **out)
print("wrote attn.npz:", len(out), "arrays,", os.path.getsize(os.path.join(HERE, "attn.npz")), "bytes")
