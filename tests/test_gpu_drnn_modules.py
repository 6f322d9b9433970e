"""GPU (run with -m gpu): SimpleAttention and MatchingAttention of models.DialogueRNN as standalone autograd nodes
(csrc/attnpool.hip + mser_gemm) against the reference's own outputs and gradients (tests/golden/drnn_modules_attention.npz,
written by make_golden_drnn_modules.py), and at the trainer's widths against the reference's formulas in float64."""
import os

import numpy as np
import pytest
import torch

from gpu_util import DEV, maxabs

pytestmark = pytest.mark.gpu

TOL = 1e-4
TYPES = ("general", "general2", "dot", "concat", "simple")


@pytest.fixture(scope="module")
def G(golden_dir):
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return np.load(os.path.join(golden_dir, "drnn_modules_attention.npz"), allow_pickle=False)


def _module(G, t):
    from models.DialogueRNN import MatchingAttention, SimpleAttention
    D_mem, D_cand, D_a, _ = (int(v) for v in G["dims"])
    cand = D_mem if t in ("dot", "simple") else D_cand
    net = SimpleAttention(D_mem) if t == "simple" else MatchingAttention(D_mem, cand, D_a, t)
    sd = net.state_dict()
    with torch.no_grad():
        for n in sd:
            sd[n].copy_(torch.from_numpy(G[f"{t}/init/{n}"]))
    return net.to(DEV)


def _grad_ok(got, ref):
    ref = torch.as_tensor(np.asarray(ref)).double()
    return maxabs(got, ref) <= TOL * max(1.0, float(ref.norm()))


@pytest.mark.parametrize("S", (1, 7, 150))
@pytest.mark.parametrize("t", TYPES)
def test_attention_matches_reference_golden(G, t, S):
    net = _module(G, t)
    k = f"{t}/S{S}/"
    M = torch.from_numpy(G[k + "M"]).to(DEV).requires_grad_(True)
    x = torch.from_numpy(G[k + "x"]).to(DEV).requires_grad_(True)
    mask = torch.from_numpy(G[k + "mask"]).to(DEV)
    pool, alpha = net(M) if t == "simple" else net(M, x, mask)
    assert tuple(alpha.shape) == (M.shape[1], 1, S) and tuple(pool.shape) == (M.shape[1], M.shape[2])
    assert maxabs(pool, G[k + "pool"]) < TOL, maxabs(pool, G[k + "pool"])
    assert maxabs(alpha, G[k + "alpha"]) < TOL, maxabs(alpha, G[k + "alpha"])
    gp = torch.from_numpy(G[k + "gpool"]).to(DEV)
    ga = torch.from_numpy(G[k + "galpha"]).to(DEV)
    ((pool * gp).sum() + (alpha * ga).sum()).backward()
    assert _grad_ok(M.grad, G[k + "dM"]), ("dM", maxabs(M.grad, G[k + "dM"]))
    if t != "simple":
        assert _grad_ok(x.grad, G[k + "dx"]), ("dx", maxabs(x.grad, G[k + "dx"]))
    for n, p in net.named_parameters():
        assert p.grad is not None, n
        assert _grad_ok(p.grad, G[k + "d/" + n]), (n, maxabs(p.grad, G[k + "d/" + n]))


@pytest.mark.parametrize("t", ("general2", "dot"))
def test_attention_takes_strided_memory(G, t):
    """M as a view with non-packed row and batch strides gives what the packed copy gives (the kernels read the strides)."""
    net = _module(G, t)
    k = f"{t}/S150/"
    M0 = torch.from_numpy(G[k + "M"]).to(DEV)
    S, B, D = M0.shape
    big = torch.randn(B, S, D + 5, device=DEV)
    big[:, :, 3:3 + D] = M0.transpose(0, 1)
    Mv = big[:, :, 3:3 + D].transpose(0, 1)                       # [S, B, D], strides (D+5, S*(D+5), 1)
    assert Mv.stride() != M0.stride()
    x = torch.from_numpy(G[k + "x"]).to(DEV)
    mask = torch.from_numpy(G[k + "mask"]).to(DEV)
    with torch.no_grad():
        p0, a0 = net(M0, x, mask)
        p1, a1 = net(Mv, x, mask)
    assert maxabs(p0, p1) == 0.0 and maxabs(a0, a1) == 0.0


@pytest.mark.parametrize("t", TYPES)
def test_attention_empty_memory_is_a_host_case(G, t):
    """S = 0 (no history yet): a zero pool, an empty alpha and zero gradients, no launch on an empty memory."""
    from models.DialogueRNN import MatchingAttention, SimpleAttention
    net = (SimpleAttention(6) if t == "simple" else MatchingAttention(6, 6 if t == "dot" else 4, 5, t)).to(DEV)
    M = torch.zeros(0, 3, 6, device=DEV, requires_grad=True)
    x = torch.randn(3, 6 if t == "dot" else 4, device=DEV, requires_grad=True)
    pool, alpha = net(M) if t == "simple" else net(M, x, torch.ones(3, 0, device=DEV))
    assert tuple(pool.shape) == (3, 6) and tuple(alpha.shape) == (3, 1, 0) and float(pool.abs().sum()) == 0.0
    pool.sum().backward()
    assert tuple(M.grad.shape) == (0, 3, 6)
    for n, p in net.named_parameters():
        assert p.grad is not None and float(p.grad.abs().sum()) == 0.0, n


def test_attention_rejects_mismatched_shapes(G):
    """Where the reference's bmm / broadcast raises, so does the module -- before any launch (a [S, B] mask has the right number
    of elements and must not be read as [B, S])."""
    from models.DialogueRNN import MatchingAttention
    S, B = 7, 3
    M = torch.randn(S, B, 6, device=DEV)
    g2 = MatchingAttention(6, 4, att_type="general2").to(DEV)
    x = torch.randn(B, 4, device=DEV)
    with pytest.raises(ValueError):
        g2(M, x, torch.ones(S, B, device=DEV))
    with pytest.raises(ValueError):
        g2(M, x, torch.ones(S, device=DEV))
    with pytest.raises(ValueError):
        g2(M, torch.randn(B + 1, 4, device=DEV), torch.ones(B, S, device=DEV))
    with pytest.raises(ValueError):
        g2(torch.randn(S, B, 8, device=DEV), x)
    with pytest.raises(ValueError):
        MatchingAttention(6, 6, att_type="dot").to(DEV)(M, torch.randn(B, 5, device=DEV))
    p0, a0 = g2(M, x, torch.ones(B, S, device=DEV))
    p1, a1 = g2(M, x, torch.ones(1, S, device=DEV))               # broadcasts in the reference too
    assert maxabs(p0, p1) == 0.0 and maxabs(a0, a1) == 0.0


@pytest.mark.parametrize("t", ("dot", "general", "concat"))
def test_attention_ignored_mask_may_be_anything(G, t):
    """'dot', 'general' and 'concat' never read the mask, as in the reference: a CPU mask of any shape changes nothing."""
    from models.DialogueRNN import MatchingAttention
    S, B = 9, 4
    net = MatchingAttention(6, 6 if t == "dot" else 5, 7, t).to(DEV)
    M = torch.randn(S, B, 6, device=DEV)
    x = torch.randn(B, 6 if t == "dot" else 5, device=DEV)
    p0, a0 = net(M, x)
    p1, a1 = net(M, x, torch.zeros(S, B))
    assert maxabs(p0, p1) == 0.0 and maxabs(a0, a1) == 0.0


def _reference_formula(t, M, x, mask, W, bias, v):
    """model/DialogueRNN.py:6-77 restated (float64 on the CPU)."""
    if t == "simple":
        alpha = torch.softmax(M @ W.t(), dim=0).permute(1, 2, 0)
    elif t in ("dot", "general"):
        q = x if t == "dot" else x @ W.t()
        alpha = torch.softmax(torch.bmm(q.unsqueeze(1), M.permute(1, 2, 0)), dim=2)
    elif t == "general2":
        s = torch.bmm((x @ W.t() + bias).unsqueeze(1), M.permute(1, 2, 0)) * mask.unsqueeze(1)
        a_ = torch.softmax(s, dim=2) * mask.unsqueeze(1)
        alpha = a_ / a_.sum(dim=2, keepdim=True)
    else:                                                         # concat
        Mx = torch.cat([M.transpose(0, 1), x.unsqueeze(1).expand(-1, M.shape[0], -1)], 2)
        alpha = torch.softmax(torch.tanh(Mx @ W.t()) @ v.t(), 1).transpose(1, 2)
    return torch.bmm(alpha, M.transpose(0, 1))[:, 0, :], alpha


@pytest.mark.parametrize("t", TYPES)
def test_attention_at_trainer_widths_against_the_formula(G, t):
    """S = 200 history rows, B = 64, D_mem = 500 (the DialogueRNN's D_g): beyond the goldens, several trips of every feature and
    row loop (scores, pool, dM / dq, the 'concat' dA loop over alpha_dim = 100)."""
    from models.DialogueRNN import MatchingAttention, SimpleAttention
    S, B, D, Da = 200, 64, 500, 100
    Dc = D if t in ("dot", "simple") else 300
    torch.manual_seed(5)
    net = SimpleAttention(D) if t == "simple" else MatchingAttention(D, Dc, Da, t)
    M = torch.randn(S, B, D) * (0.2 if t in ("dot", "simple") else 1.0)     # keeps the 'dot' softmax away from one-hot
    x = torch.randn(B, Dc) * (0.2 if t == "dot" else 1.0)
    lens = torch.randint(1, S + 1, (B,))
    mask = (torch.arange(S).unsqueeze(0) < lens.unsqueeze(1)).float()
    gp, ga = torch.randn(B, D), torch.randn(B, 1, S)
    W = None
    if t == "simple":
        W = net.scalar.weight.detach().double().requires_grad_(True)
    elif t != "dot":
        W = net.transform.weight.detach().double().requires_grad_(True)
    bias = net.transform.bias.detach().double().requires_grad_(True) if t == "general2" else None
    v = net.vector_prod.weight.detach().double().requires_grad_(True) if t == "concat" else None
    Mr, xr = M.double().requires_grad_(True), x.double().requires_grad_(True)
    pr, ar = _reference_formula(t, Mr, xr, mask.double(), W, bias, v)
    ((pr * gp.double()).sum() + (ar * ga.double()).sum()).backward()
    net = net.to(DEV)
    Md, xd = M.to(DEV).requires_grad_(True), x.to(DEV).requires_grad_(True)
    pool, alpha = net(Md) if t == "simple" else net(Md, xd, mask.to(DEV))
    assert maxabs(pool, pr) < TOL and maxabs(alpha, ar) < TOL, (maxabs(pool, pr), maxabs(alpha, ar))
    ((pool * gp.to(DEV)).sum() + (alpha * ga.to(DEV)).sum()).backward()
    assert _grad_ok(Md.grad, Mr.grad), maxabs(Md.grad, Mr.grad)
    if t != "simple":
        assert _grad_ok(xd.grad, xr.grad), maxabs(xd.grad, xr.grad)
    if t == "simple":
        assert _grad_ok(net.scalar.weight.grad, W.grad)
    elif t != "dot":
        assert _grad_ok(net.transform.weight.grad, W.grad)
    if bias is not None:
        assert _grad_ok(net.transform.bias.grad, bias.grad)
    if v is not None:
        assert _grad_ok(net.vector_prod.weight.grad, v.grad)
