"""The attention modules: the HIP route against the reference's formula restated in torch on the same device
(``score`` -> ``masked_fill`` -> ``softmax`` -> broadcast product summed over ``dim``), runs alternated in pairs
and timed with events; forward alone and forward + backward.

  python profiles/tools/time_attn.py [--reps 10] [--only decode_dot,concat_decode,...]

Shapes: decode (dot and generalized; N=128 utterances, K=8 beams, T=512, D=512, a length mask), a training
step (N=256, T=512, D=512, no group) and transformer self-attention (T=1000, N=16, D=64, four heads, causal).
Prints one JSON line per shape and pass: min / median ms of each route, and for the HIP forward the rate of
the key and value bytes it has to read (frames some row attends to, once per group) as TB/s and as a
fraction of the 8.0 TB/s HBM peak.

ConcatSoftAttention (hidden_size 1000) at the decode shape and at the training step (``concat_decode``,
``concat_training``) is timed on three routes in the same run: the module (its score in
``pydrobert_amd::concat_score``), the same module with the score's torch body ``_concat_score_torch`` (tanh at the
full broadcast shape times the hidden size), and the reference's expanded-concatenation formula.  Their lines
also give the growth of ``torch.cuda.max_memory_allocated`` over one call, and for the new forward the rate of
the wk bytes (T x groups x hidden, read once per group) end to end.  Each sample is one module call between device events, so these are
END-TO-END rates: the host's checks, planning and workspace allocation are in them.  For the kernels' own
times run the tool under ``rocprofv3 --kernel-trace --stats``."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "pydrobert-pytorch_amd"))

from pydrobert_amd import modules as M  # noqa: E402
from pydrobert_amd import _attn  # noqa: E402
from pydrobert_amd._attn import _softmax_pool, _unflatten  # noqa: E402

DEV = torch.device("cuda:0")
HBM_PEAK = 8.0e12


def formula(m, q, k, v, mask):
    """The reference's forward (_attn.py:212-223) with stock torch ops."""
    if isinstance(m, M.MultiHeadedAttention):
        qh = _unflatten(m.WQ(q), -1, [m.num_heads, m.d_q])
        kh = _unflatten(m.WK(k), -1, [m.num_heads, m.d_k])
        vh = _unflatten(m.WV(v), -1, [m.num_heads, m.d_v])
        cat = formula(m.single_head_attention, qh, kh, vh, None if mask is None else mask.unsqueeze(-2))
        return m.WC(cat.flatten(-2))
    return _softmax_pool(m.score(q, k), v, mask, m.dim)


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def shapes():
    g = torch.Generator(device=DEV).manual_seed(0)
    N, K, T, D = 128, 8, 512, 512
    lens = torch.randint(T // 2, T + 1, (N,), device=DEV, generator=g)
    dec_mask = torch.arange(T, device=DEV).view(T, 1, 1) < lens.view(1, N, 1)
    dec = (torch.randn(N, K, D, device=DEV), torch.randn(T, N, 1, D, device=DEV), torch.randn(T, N, 1, D, device=DEV))
    dec_bytes = int(lens.sum()) * D * 4 * 2
    Nt = 256
    tr = (torch.randn(Nt, D, device=DEV), torch.randn(T, Nt, D, device=DEV), torch.randn(T, Nt, D, device=DEV))
    Ts, Ns, Ds = 1000, 16, 64
    sa = (torch.randn(Ts, Ns, Ds, device=DEV), torch.randn(Ts, 1, Ns, Ds, device=DEV),
          torch.randn(Ts, 1, Ns, Ds, device=DEV))  # fmt: skip
    causal = torch.arange(Ts, device=DEV).view(Ts, 1, 1) <= torch.arange(Ts, device=DEV).view(1, Ts, 1)
    torch.manual_seed(0)
    return {
        "decode_dot": (M.DotProductSoftAttention(D, 0, D ** -0.5), dec, dec_mask, dec_bytes),
        "decode_generalized": (M.GeneralizedDotProductSoftAttention(D, D).to(DEV), dec, dec_mask, dec_bytes),
        "training_dot": (M.DotProductSoftAttention(D, 0, D ** -0.5), tr, None, T * Nt * D * 4 * 2),
        "self_attention_4heads": (
            M.MultiHeadedAttention(Ds, Ds, Ds, 4, M.DotProductSoftAttention(Ds // 4, 0, (Ds // 4) ** -0.5)).to(DEV),
            sa, causal, Ts * Ns * Ds * 4 * 2,  # (the heads' keys and values, once per group)
        ),
    }


def concat_torch_body(m, q, k, v, mask):
    """ConcatSoftAttention as it ran before the fused score: the two halves of W, tanh and the product with v in
    torch, then ``pydrobert_amd::attention_pool``."""
    Dq = q.size(-1)
    wq = torch.nn.functional.linear(q.unsqueeze(m.dim), m.weight[:, :Dq], m.bias)
    wk = torch.nn.functional.linear(k, m.weight[:, Dq:], None)
    return _attn.attention_pool(_attn._concat_score_torch(wq, wk, m.v), v, mask, m.dim)


def concat_reference(m, q, k, v, mask):
    """The reference's forward (_attn.py:344-361, 212-223): query and key expanded and concatenated."""
    q1 = q.unsqueeze(m.dim)
    shape = torch.broadcast_shapes(q1.shape[:-1], k.shape[:-1])
    cat = torch.cat([q1.expand(shape + q1.shape[-1:]), k.expand(shape + k.shape[-1:])], -1)
    hidden = torch.tanh(torch.nn.functional.linear(cat, m.weight, m.bias))
    return _softmax_pool(torch.nn.functional.linear(hidden, m.v.unsqueeze(0), None).squeeze(-1), v, mask, m.dim)


def concat_shapes():
    g = torch.Generator(device=DEV).manual_seed(1)
    N, K, T, D, H = 128, 8, 512, 512, 1000
    lens = torch.randint(T // 2, T + 1, (N,), device=DEV, generator=g)
    dec_mask = torch.arange(T, device=DEV).view(T, 1, 1) < lens.view(1, N, 1)
    dec = (torch.randn(N, K, D, device=DEV), torch.randn(T, N, 1, D, device=DEV), torch.randn(T, N, 1, D, device=DEV))
    Nt = 256
    tr = (torch.randn(Nt, D, device=DEV), torch.randn(T, Nt, D, device=DEV), torch.randn(T, Nt, D, device=DEV))
    torch.manual_seed(1)
    m = M.ConcatSoftAttention(D, D, 0, True, H).to(DEV)
    return {
        "concat_decode": (m, dec, dec_mask, T * N * H * 4, T * N * K * H),
        "concat_training": (m, tr, None, T * Nt * H * 4, T * Nt * H),
    }


def memory_growth(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - base


def concat_main(args, only):
    routes = (("hip", lambda m, *a: m(*a)), ("torch_body", concat_torch_body), ("reference", concat_reference))
    for name, (m, (q, k, v), mask, wk_bytes, tanhs) in concat_shapes().items():
        if only and name not in only:
            continue
        with torch.no_grad():
            outs = [f(m, q, k, v, mask) for _, f in routes]
        gy = torch.randn_like(outs[0])
        err = {n: float((o - outs[2]).abs().max()) for (n, _), o in zip(routes[:2], outs)}
        del outs
        qg, kg = (x.clone().requires_grad_(True) for x in (q, k))

        def fwd(f):
            return lambda: torch.no_grad()(f)(m, q, k, v, mask)

        def fwd_bwd(f):
            def run():
                m.zero_grad(set_to_none=True)
                qg.grad = kg.grad = None
                f(m, qg, kg, v, mask).backward(gy)
            return run

        for label, make in (("forward", fwd), ("forward_backward", fwd_bwd)):
            fns = [make(f) for _, f in routes]
            for _ in range(2):
                for fn in fns:
                    fn()
            times = [[] for _ in fns]
            for _ in range(args.reps):
                for ts, fn in zip(times, fns):
                    ts.append(timed(fn))
            rec = {"shape": name, "pass": label, "dtype": "float32", "tanh_evaluations": tanhs}
            for (n, _), ts, fn in zip(routes, times, fns):
                ts.sort()
                rec[n + "_ms_min"] = round(ts[0], 4)
                rec[n + "_ms_median"] = round(ts[len(ts) // 2], 4)
                rec[n + "_peak_growth_MB"] = round(memory_growth(fn) / 1e6, 2)
            med = lambda n: rec[n + "_ms_median"]  # noqa: E731
            rec["speedup_vs_torch_body"] = round(med("torch_body") / med("hip"), 2)
            rec["speedup_vs_reference"] = round(med("reference") / med("hip"), 2)
            if label == "forward":
                rate = wk_bytes / (med("hip") * 1e-3)
                rec.update({"wk_GB": round(wk_bytes / 1e9, 4), "wk_TBps_end_to_end": round(rate / 1e12, 3),
                            "max_abs_diff_vs_reference": err})  # fmt: skip
            print(json.dumps(rec), flush=True)
        del qg, kg
        m.zero_grad(set_to_none=True)
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--only", default="")
    args = ap.parse_args()
    only = set(filter(None, args.only.split(",")))
    concat_main(args, only)
    for name, (m, (q, k, v), mask, kv_bytes) in shapes().items():
        if only and name not in only:
            continue
        with torch.no_grad():
            y = m(q, k, v, mask)
            y_ref = formula(m, q, k, v, mask)
            err = float((y - y_ref).abs().max())
        gy = torch.randn_like(y)
        qg, kg, vg = (x.clone().requires_grad_(True) for x in (q, k, v))

        def fwd_bwd(f):
            def run():
                out = f(m, qg, kg, vg, mask)
                out.backward(gy)
            return run

        hip = lambda mod, a, b, c, mk: mod(a, b, c, mk)  # noqa: E731
        for label, h, r in (
            ("forward", lambda: torch.no_grad()(hip)(m, q, k, v, mask), lambda: torch.no_grad()(formula)(m, q, k, v, mask)),
            ("forward_backward", fwd_bwd(hip), fwd_bwd(formula)),
        ):  # fmt: skip
            for _ in range(2):
                h(), r()
            th, tr = [], []
            for _ in range(args.reps):
                th.append(timed(h))
                tr.append(timed(r))
            th.sort()
            tr.sort()
            rec = {
                "shape": name, "pass": label, "dtype": "float32",
                "hip_ms_min": round(th[0], 4), "hip_ms_median": round(th[len(th) // 2], 4),
                "formula_ms_min": round(tr[0], 4), "formula_ms_median": round(tr[len(tr) // 2], 4),
                "speedup_median": round(tr[len(tr) // 2] / th[len(th) // 2], 2),
            }  # fmt: skip
            if label == "forward":
                rate = kv_bytes / (th[len(th) // 2] * 1e-3)
                rec.update({"kv_GB": round(kv_bytes / 1e9, 4), "kv_TBps_end_to_end": round(rate / 1e12, 3),
                            "kv_frac_hbm_peak_end_to_end": round(rate / HBM_PEAK, 3),
                            "max_abs_diff_vs_formula": err})  # fmt: skip
            print(json.dumps(rec), flush=True)
        del qg, kg, vg
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
