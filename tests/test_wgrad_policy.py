"""CPU: the ONE weight-gradient rule of the linear layers (richsem_amd/functions/linear.py: linear_wgrad) and the autograd functions that
run on CPU tensors.  The library's kernel (linear_wgrad_bf16) is replaced by a recording stub that returns the fp32 product, so which
path ran is counted and what each path returns is compared bit for bit: the kernel path hands on what the kernel wrote, the other path
is the bf16 GEMM ``dy.t() @ x`` cast to float32 and the fp32 column sum."""
import pytest
import torch

from richsem_amd.functions import linear as lin
from richsem_amd.functions.linear import LinearBf16CachedFunction, LinearBf16Function, linear_wgrad


@pytest.fixture
def kernel_calls(monkeypatch):
    calls = []

    def stub(dy, x, with_bias=False):
        calls.append(bool(with_bias))
        dw = dy.float().t() @ x.float()
        return (dw, dy.sum(0, dtype=torch.float32)) if with_bias else dw

    monkeypatch.setattr(lin, "linear_wgrad_bf16", stub)
    return calls


def operands(T, cout, cin):
    g = torch.Generator().manual_seed(T + cout + cin)
    return torch.randn(T, cout, generator=g).to(torch.bfloat16), torch.randn(T, cin, generator=g).to(torch.bfloat16)


@pytest.mark.parametrize("want_b", [False, True])
@pytest.mark.parametrize("cout,cin", [(128, 128), (64, 128), (128, 192)])
@pytest.mark.parametrize("T", [1023, 1024])
def test_rule(kernel_calls, T, cout, cin, want_b):
    dy, x = operands(T, cout, cin)
    dw, db = linear_wgrad(dy, x, want_b)
    assert dw.dtype == torch.float32 and dw.shape == (cout, cin)
    if T == 1024 and cout % 128 == 0 and cin % 128 == 0:
        assert kernel_calls == [want_b]
        assert torch.equal(dw, dy.float().t() @ x.float())
    else:
        assert kernel_calls == []
        assert torch.equal(dw, (dy.t() @ x).float())
    if want_b:
        assert db.dtype == torch.float32 and torch.equal(db, dy.sum(0, dtype=torch.float32))
    else:
        assert db is None


def run_plain(T, train_w=True, train_b=True, dt=torch.float32):
    dy, x = operands(T, 128, 128)
    w = (torch.randn(128, 128, generator=torch.Generator().manual_seed(1)) / 16).to(dt).requires_grad_(train_w)
    b = torch.zeros(128, dtype=dt, requires_grad=train_b)
    LinearBf16Function.apply(x.requires_grad_(True), w, b).backward(dy)
    return dy, x.detach(), (w, b)


def run_cached(T, split, train_w=True, train_b=True, dt=torch.float32):
    dy, x = operands(T, 128, 128)
    w = (torch.randn(128, 128, generator=torch.Generator().manual_seed(1)) / 16).to(dt)
    b = torch.zeros(128, dtype=dt)
    ws, bs_ = ([w], [b]) if split is None else ([w[:split].clone(), w[split:].clone()], [b[:split].clone(), b[split:].clone()])
    params = [t.requires_grad_(train_w) for t in ws] + [t.requires_grad_(train_b) for t in bs_]
    LinearBf16CachedFunction.apply(x.requires_grad_(True), w.to(torch.bfloat16), b.to(torch.bfloat16), split, *params).backward(dy)
    return dy, x.detach(), params


RUNNERS = {"plain": run_plain, "cached": lambda T, **k: run_cached(T, None, **k), "cached_split": lambda T, **k: run_cached(T, 48, **k)}


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("T", [1023, 1024])
@pytest.mark.parametrize("form", list(RUNNERS))
def test_functions_take_the_rule(kernel_calls, form, T, dt):
    dy, x, params = RUNNERS[form](T, dt=dt)
    assert kernel_calls == ([True] if T == 1024 else [])
    dw = dy.float().t() @ x.float() if T == 1024 else (dy.t() @ x).float()
    db = dy.sum(0, dtype=torch.float32)
    nw = len(params) // 2
    assert all(p.grad is not None and p.grad.dtype == p.dtype == dt for p in params)
    assert torch.equal(torch.cat([p.grad for p in params[:nw]]), dw.to(dt))
    assert torch.equal(torch.cat([p.grad for p in params[nw:]]), db.to(dt))


@pytest.mark.parametrize("T", [1023, 1024])
@pytest.mark.parametrize("form", list(RUNNERS))
def test_a_frozen_parameter_gets_no_gradient(kernel_calls, form, T):
    _, _, params = RUNNERS[form](T, train_w=False)           # bias alone: a column sum, never the kernel
    nw = len(params) // 2
    assert kernel_calls == []
    assert all(p.grad is None for p in params[:nw]) and all(p.grad is not None for p in params[nw:])
    _, _, params = RUNNERS[form](T, train_b=False)           # weight alone: the kernel is not asked for the bias gradient
    assert kernel_calls == ([False] if T == 1024 else [])
    assert all(p.grad is not None for p in params[:nw]) and all(p.grad is None for p in params[nw:])


def test_min_tokens_is_the_one_threshold(kernel_calls, monkeypatch):
    monkeypatch.setattr(LinearBf16Function, "MIN_TOKENS", 512)
    for T, want in ((511, 0), (512, 1)):
        linear_wgrad(*operands(T, 128, 128), False)
        for run in RUNNERS.values():
            run(T)
        assert len(kernel_calls) == want * (1 + len(RUNNERS)), T
        kernel_calls.clear()
