"""pad_variable / RandomShift on the GPU: against the live
reference's outputs (tests/golden/pad.npz), the oracle on random shapes / dtypes -- up to outputs
of several workgroups, every word width -- and the backward kernel against autograd through an
equivalent gather graph, in float32 and float64."""
import os

import numpy as np
import pytest
import torch

import oracle
from pydrobert_amd import functional as F
from pydrobert_amd import modules as M

pytestmark = pytest.mark.gpu
DEV = "cuda"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pad.npz")


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


@pytest.mark.parametrize("mode", ["constant", "reflect", "replicate"])
def test_pad_variable_golden(mode):
    g = np.load(GOLDEN)
    act = M.PadVariable(mode, -1.5)(_t(g["x"]), _t(g["lens"]), _t(g["pad"]))
    assert np.array_equal(g["out_" + mode], act.cpu().numpy())
    act = F.pad_variable(_t(g["xi"]), _t(g["lens"]), _t(g["pad"]), mode, 7)
    assert act.dtype == torch.long and np.array_equal(g["outi_" + mode], act.cpu().numpy())


@pytest.mark.parametrize("mode", ["constant", "reflect", "replicate"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64, torch.float16, torch.int32, torch.uint8])
def test_pad_variable_random(mode, dtype):
    rng = np.random.default_rng(3)
    for shape in ((7, 33), (5, 20, 4), (3, 11, 2, 3), (4, 1, 5)):
        N, T = shape[:2]
        x = (rng.normal(size=shape) * 20).astype(np.float64)
        lens = rng.integers(1, T + 1, N)
        hi = np.maximum(lens - 1, 0) if mode == "reflect" else np.full(N, 12)
        pad = np.stack([rng.integers(0, hi + 1), rng.integers(0, hi + 1)])
        xt = torch.from_numpy(x).to(dtype)
        exp = oracle.pad_variable(xt.numpy(), lens, pad, mode, 3.0)
        act = F.pad_variable(xt.to(DEV), _t(lens), _t(pad), mode, 3.0)
        assert act.dtype == dtype and np.array_equal(exp, act.cpu().numpy()), (shape, mode)


def test_pad_variable_edge_cases():
    x = torch.randn((3, 5, 2), device=DEV)
    lens = torch.tensor([5, 3, 2], device=DEV)
    zero = torch.zeros((2, 3), dtype=torch.long, device=DEV)
    assert torch.equal(F.pad_variable(x, torch.tensor([5, 5, 5], device=DEV), zero), x)
    with pytest.raises(NotImplementedError, match="reflect"):
        F.pad_variable(x, lens, torch.tensor([[0, 3, 0], [0, 0, 0]], device=DEV), "reflect")
    with pytest.raises(RuntimeError, match="replicate"):
        F.pad_variable(x, torch.tensor([5, 0, 2], device=DEV), zero, "replicate")
    with pytest.raises(ValueError):
        F.pad_variable(x, lens[:2], zero)
    with pytest.raises(ValueError):
        F.pad_variable(x, lens, zero[:, :2])
    empty = F.pad_variable(x[:0], lens[:0], zero[:, :0])
    assert empty.shape == (0, 0, 2)


@pytest.mark.parametrize("mode", ["constant", "reflect", "replicate"])
def test_pad_variable_backward(mode):
    torch.manual_seed(4)
    N, T, Fq = 6, 12, 5
    x = torch.randn((N, T, Fq), device=DEV)
    lens = torch.tensor([12, 7, 3, 9, 12, 5], device=DEV)
    pad = torch.tensor([[2, 0, 1, 4, 0, 3], [1, 5, 2, 0, 0, 4]], device=DEV)
    x1 = x.clone().requires_grad_(True)
    y = F.pad_variable(x1, lens, pad, mode, 0.5)
    g = torch.randn_like(y)
    (act,) = torch.autograd.grad(y, x1, g)
    # equivalent differentiable graph: gather along time through the oracle's index map
    idx = np.tile(np.arange(T)[None], (N, 1))
    src = oracle.pad_variable(idx, lens.cpu().numpy(), pad.cpu().numpy(), mode, -1)
    src_t = torch.from_numpy(src).to(DEV)
    x2 = x.clone().requires_grad_(True)
    gathered = x2.gather(1, src_t.clamp(min=0).unsqueeze(2).expand(-1, -1, Fq))
    y2 = torch.where((src_t >= 0).unsqueeze(2), gathered, torch.full_like(gathered, 0.5))
    assert torch.equal(y, y2)
    (exp,) = torch.autograd.grad(y2, x2, g)
    assert torch.allclose(exp, act, atol=1e-5)


def test_random_shift():
    """Facts of the reference's tests/test_img.py:284-344: lengths grow within the bounds,
    the original sequence sits inside the output, eval mode is the identity."""
    torch.manual_seed(5)
    N, T, Fq = 50, 30, 4
    x = torch.rand((N, T, Fq), device=DEV) + 0.01
    lens = torch.randint(2, T + 1, (N,), device=DEV)
    for mode in ("reflect", "constant", "replicate"):
        shift = M.RandomShift((0.4, 0.6), mode, 0.0)
        out, out_lens = shift(x, lens)
        grow = out_lens - lens
        assert (grow >= 0).all() and (grow <= (0.4 * lens.float()).long() + (0.6 * lens.float()).long()).all()
        assert out.shape[:2] == (N, int(out_lens.max())) and out.shape[2:] == x.shape[2:]
        # beyond the new length: the fill value
        beyond = torch.arange(out.shape[1], device=DEV).unsqueeze(0) >= out_lens.unsqueeze(1)
        assert (out[beyond] == 0).all()
        if mode == "constant":  # the copy of x is the only non-zero stretch
            nz = (out.abs().sum(2) > 0).sum(1)
            assert torch.equal(nz, lens)
        shift.eval()
        same, same_lens = shift(x, lens)
        assert same is x and same_lens is lens
    with pytest.raises(NotImplementedError):
        M.RandomShift(1.5, "reflect")
    with pytest.raises(ValueError):
        M.RandomShift(-0.1)
    jit = torch.jit.script(M.RandomShift(0.3, "replicate"))
    out, out_lens = jit(x, lens)
    assert out.shape[1] == int(out_lens.max())


# ----------------------------------------------------------------------------------------------------------
# beyond one workgroup and one pass of the kPerThread loop: outputs of several thousand elements, every word
# width through more than one dtype, and the backward kernel in float32 and float64

_WIDE = {  # shape -> largest pad per side (reflect: at most len - 1)
    (9, 200, 7): 12,
    (3, 700, 1): 340,  # (more than 4096 output elements need T' > 1365)
    (64, 33): 12,
    (5, 60, 2, 3): 150,
}
_DTYPES = (torch.uint8, torch.bool, torch.int16, torch.bfloat16, torch.float32, torch.int64, torch.float64)


def _wide_case(shape, mode):
    """Deterministic (x float64, lens, pad) for one of the _WIDE shapes."""
    rng = np.random.default_rng(sum(shape))
    N, T = shape[:2]
    x = rng.normal(size=shape) * 20
    lens = rng.integers(max(1, T // 2), T + 1, N)
    lens[0] = lens[-1] = T
    hi = np.minimum(lens - 1, _WIDE[shape]) if mode == "reflect" else np.full(N, _WIDE[shape])
    pad = np.stack([rng.integers(0, hi + 1), rng.integers(0, hi + 1)])
    pad[:, -1] = hi[-1]  # (the widest pad on both sides of one row)
    return x, lens, pad


@pytest.mark.parametrize("mode", ["constant", "reflect", "replicate"])
@pytest.mark.parametrize("dtype", _DTYPES, ids=str)
def test_pad_variable_many_workgroups(mode, dtype):
    """Bit-equal to the oracle where the output takes several workgroups (1024 elements each) and a partial
    last one, with F = 1 and with trailing dims; 1-, 2-, 4- and 8-byte words through two dtypes each."""
    for shape in _WIDE:
        x, lens, pad = _wide_case(shape, mode)
        xt = torch.from_numpy(x).to(dtype) if dtype != torch.bool else torch.from_numpy(x > 0)
        act = F.pad_variable(xt.to(DEV), _t(lens), _t(pad), mode, 3.0)
        assert act.dtype == dtype
        if len(shape) == 3:
            assert act.numel() > 4096 and act.numel() % 1024 != 0, (shape, act.shape)
        if dtype == torch.bfloat16:  # (numpy has no bfloat16: the oracle moves the same bits as int16)
            fill = torch.tensor(3.0, dtype=dtype).view(torch.int16).item()
            exp = oracle.pad_variable(xt.view(torch.int16).numpy(), lens, pad, mode, fill)
            act = act.view(torch.int16)
        else:
            exp = oracle.pad_variable(xt.numpy(), lens, pad, mode, 3.0)
        assert act.shape == exp.shape and np.array_equal(exp, act.cpu().numpy()), (shape, mode)


def _gather_graph_grad(x, lens, pad, mode, g):
    """Gradient through an equivalent differentiable graph: a gather along time through the oracle's index
    map (the graph of test_pad_variable_backward)."""
    N, T = x.shape[:2]
    idx = np.tile(np.arange(T)[None], (N, 1))
    src = torch.from_numpy(oracle.pad_variable(idx, lens, pad, mode, -1)).to(x.device)
    x2 = x.clone().requires_grad_(True)
    gathered = x2.gather(1, src.clamp(min=0).unsqueeze(2).expand(-1, -1, x.shape[2]))
    y2 = torch.where((src >= 0).unsqueeze(2), gathered, torch.full_like(gathered, 0.5))
    return y2, torch.autograd.grad(y2, x2, g)[0]


@pytest.mark.parametrize("mode", ["constant", "reflect", "replicate"])
@pytest.mark.parametrize("dtype,tol", [(torch.float32, 1e-5), (torch.float64, 1e-12)], ids=("float32", "float64"))
def test_pad_variable_backward_many_workgroups(mode, dtype, tol):
    """The adjoint over 12600 input elements (13 workgroups), in float32 and -- not narrowed on the way -- in
    float64."""
    shape = (9, 200, 7)
    xn, lens, pad = _wide_case(shape, mode)
    x = torch.from_numpy(xn).to(DEV, dtype)
    x1 = x.clone().requires_grad_(True)
    y = F.pad_variable(x1, _t(lens), _t(pad), mode, 0.5)
    g = torch.randn(y.shape, device=DEV, dtype=torch.float64).to(dtype)
    (act,) = torch.autograd.grad(y, x1, g)
    y2, exp = _gather_graph_grad(x, lens, pad, mode, g)
    assert torch.equal(y, y2) and act.dtype == dtype
    assert (act - exp).abs().max().item() <= tol


@pytest.mark.parametrize("dtype,tol", [(torch.float32, 1e-5), (torch.float64, 1e-12)], ids=("float32", "float64"))
def test_pad_variable_backward_long_replicate_sum(dtype, tol):
    """Replicate by 150 on each side of a row of length 1: its one sample collects 301 gradients."""
    lens = np.array([1, 40, 17])
    pad = np.array([[150, 3, 0], [150, 0, 150]])
    x = torch.randn((3, 40, 5), device=DEV, dtype=dtype)
    x1 = x.clone().requires_grad_(True)
    y = F.pad_variable(x1, _t(lens), _t(pad), "replicate", 0.5)
    assert y.shape == (3, 301, 5)
    g = torch.randn(y.shape, device=DEV, dtype=torch.float64).to(dtype)
    (act,) = torch.autograd.grad(y, x1, g)
    y2, exp = _gather_graph_grad(x, lens, pad, "replicate", g)
    assert torch.equal(y, y2)
    # (301 float32 terms of size ~1 summed in order: within 1e-5 of autograd's own float32 sum only relative to
    # the sum's size, so the float32 bound scales with it; float64 needs no such room)
    assert (act - exp).abs().max().item() <= tol * max(1.0, exp.abs().max().item())
