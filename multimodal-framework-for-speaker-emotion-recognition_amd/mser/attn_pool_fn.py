"""SimpleAttention / MatchingAttention (reference model/DialogueRNN.py:6-77) as standalone autograd nodes.

The score, softmax and pool stages and their backward are mser_attn_pool_fwd / _bwd (csrc/attnpool.hip, three launches per pass
over the whole S*B memory); the products with the modules' weights are mser_gemm calls:

  simple    q = scalar.weight (shared by every row)        d scalar.weight = sum_b dq[b]
  dot       q = x                                          dx = dq
  general   q = x W^T                                      dx = dq W, dW = dq^T x
  general2  q = x W^T + bias                               the same, d bias = sum_b dq[b]
  concat    A = M W_M^T over all S*B rows, xb = x W_x^T    (W = [W_M | W_x]: the [B, S, D_mem + D_cand] concatenation of :70-73 is
            never formed) dM += dA W_M, dW_M = dA^T M, dx = dxb W_x, dW_x = dxb^T x, d vector_prod.weight = sum_b dvb[b]

The mask reaches the kernels for 'general2' only: the reference ignores it for every other type.  An empty memory (S = 0) is
answered on the host -- a zero pool and an empty alpha, what the reference's bmm over an empty sequence returns.
"""
from __future__ import annotations

from typing import Optional

import torch

from . import _lib as L
from . import ops

TYPES = {"simple": L.MSER_ATT_SIMPLE, "dot": L.MSER_ATT_DOT, "general": L.MSER_ATT_GENERAL, "general2": L.MSER_ATT_GENERAL2,
         "concat": L.MSER_ATT_CONCAT}


def _mem_view(M: torch.Tensor) -> torch.Tensor:
    """M [S, B, D] with unit inner stride (any row and batch strides pass through without a copy)."""
    if M.dtype != torch.float32:
        raise RuntimeError(f"attention memory: expected float32, got {M.dtype}")
    return M if M.stride(2) == 1 else M.contiguous()


def _mask_rows(mask: torch.Tensor, B: int, S: int) -> torch.Tensor:
    """The 'general2' mask as a packed float32 [B, S].  The reference multiplies with mask.unsqueeze(1) against [B, 1, S]: a 2-D
    mask broadcasts there ([1, S] or [B, 1] too); any other shape raises, as the broadcast does."""
    if mask.dim() != 2:
        raise ValueError(f"MatchingAttention mask must be [batch, seq_len] = [{B}, {S}], got {tuple(mask.shape)}")
    try:
        return mask.to(torch.float32).expand(B, S).contiguous()
    except RuntimeError:
        raise ValueError(f"MatchingAttention mask must be [batch, seq_len] = [{B}, {S}], got {tuple(mask.shape)}") from None


def _desc(kind: int, M: torch.Tensor, alpha: torch.Tensor, pool: torch.Tensor, q=None, sqb=0, mask=None, A=None, xb=None, v=None):
    S, B, D = M.shape
    d = L.AttnPoolDesc()
    d.type, d.S, d.B, d.D = kind, S, B, D
    d.M, d.sMj, d.sMb = M.data_ptr(), M.stride(0), M.stride(1)
    d.q, d.sqb = (q.data_ptr() if q is not None else None), sqb
    d.mask = mask.data_ptr() if mask is not None else None
    if A is not None:
        d.Da, d.A, d.lda, d.xb, d.v = A.shape[1], A.data_ptr(), A.stride(0), xb.data_ptr(), v.data_ptr()
    d.alpha, d.pool = alpha.data_ptr(), pool.data_ptr()
    return d


class _AttnPoolFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, att_type: str, M, x, mask, W, bias, v):
        kind = TYPES[att_type]
        M = _mem_view(M)
        S, B, D = M.shape
        dev = M.device
        pool = torch.empty(B, D, device=dev)
        alpha = torch.empty(B, S, device=dev)
        q = A = xb = None
        sqb = 0
        if kind == L.MSER_ATT_SIMPLE:
            q = W.reshape(D)
        elif kind == L.MSER_ATT_DOT:
            x = x.contiguous()
            q, sqb = x, x.stride(0)
        elif kind in (L.MSER_ATT_GENERAL, L.MSER_ATT_GENERAL2):
            x = x.contiguous()
            q = torch.empty(B, D, device=dev)
            ops.linear(x, W, q, bias=bias if kind == L.MSER_ATT_GENERAL2 else None)
            sqb = D
        else:
            x = x.contiguous()
            M = M.contiguous()
            Da = W.shape[0]
            A = torch.empty(S * B, Da, device=dev)
            xb = torch.empty(B, Da, device=dev)
            if S > 0:
                ops.linear(M.view(S * B, D), W[:, :D], A)
                ops.linear(x, W[:, D:], xb)
            v = v.reshape(Da)
        mk = None
        if kind == L.MSER_ATT_GENERAL2 and mask is not None:
            mk = _mask_rows(mask, B, S)
        if S > 0:
            d = _desc(kind, M, alpha, pool, q=q, sqb=sqb, mask=mk, A=A, xb=xb, v=v)
            L.check(ops._lib().mser_attn_pool_fwd(d, ops._stream()), "mser_attn_pool_fwd")
        else:
            pool.zero_()
        ctx.kind = kind
        ctx.save_for_backward(M, x, mk, W, v, q, A, xb, alpha)
        ctx.set_materialize_grads(False)
        return pool, alpha.view(B, 1, S)

    @staticmethod
    def backward(ctx, dpool, dalpha):
        M, x, mk, W, v, q, A, xb, alpha = ctx.saved_tensors
        kind = ctx.kind
        S, B, D = M.shape
        dev = M.device
        dM = torch.zeros(S, B, D, device=dev)
        gx = torch.zeros_like(x) if x is not None and ctx.needs_input_grad[2] else None
        gW = torch.zeros_like(W) if W is not None else None
        gb = torch.zeros(D, device=dev) if kind == L.MSER_ATT_GENERAL2 else None
        gv = torch.zeros_like(v) if kind == L.MSER_ATT_CONCAT else None
        if S == 0 or (dpool is None and dalpha is None):
            return (None, dM, gx, None, gW, gb, gv.view(1, -1) if gv is not None else None)
        dpool = dpool.contiguous() if dpool is not None else torch.zeros(B, D, device=dev)
        d = _desc(kind, M, alpha, torch.empty(0, device=dev), q=q, sqb=(0 if kind == L.MSER_ATT_SIMPLE else D), mask=mk,
                  A=A, xb=xb, v=v)
        d.dpool = dpool.data_ptr()
        if dalpha is not None:
            dalpha = dalpha.reshape(B, S).contiguous()
            d.dalpha = dalpha.data_ptr()
        d.dM = dM.data_ptr()
        ds = torch.empty(B, S, device=dev)
        d.ds = ds.data_ptr()
        if kind == L.MSER_ATT_CONCAT:
            Da = A.shape[1]
            dA = torch.empty(S * B, Da, device=dev)
            dxb = torch.empty(B, Da, device=dev)
            dvb = torch.empty(B, Da, device=dev)
            d.dA, d.dxb, d.dvb = dA.data_ptr(), dxb.data_ptr(), dvb.data_ptr()
        else:
            dq = torch.empty(B, D, device=dev)
            d.dq = dq.data_ptr()
        L.check(ops._lib().mser_attn_pool_bwd(d, ops._stream()), "mser_attn_pool_bwd")
        if kind == L.MSER_ATT_SIMPLE:
            ops.colsum_acc(dq, gW.view(D))
        elif kind == L.MSER_ATT_DOT:
            gx = dq
        elif kind in (L.MSER_ATT_GENERAL, L.MSER_ATT_GENERAL2):
            if gx is not None:
                ops.matmul(dq, W, gx)
            ops.grad_weight(dq, x, gW, splitk=1)
            if gb is not None:
                ops.colsum_acc(dq, gb)
        else:
            M2 = M.view(S * B, D)
            ops.matmul(dA, W[:, :D], dM.view(S * B, D), accum=True)
            ops.grad_weight(dA, M2, gW[:, :D], splitk=1)
            if gx is not None:
                ops.matmul(dxb, W[:, D:], gx)
            ops.grad_weight(dxb, x, gW[:, D:], splitk=1)
            ops.colsum_acc(dvb, gv)
        return (None, dM, gx, None, gW, gb, gv.view(1, -1) if gv is not None else None)


def attn_pool(att_type: str, M: torch.Tensor, x: Optional[torch.Tensor], mask: Optional[torch.Tensor], W: Optional[torch.Tensor],
              bias: Optional[torch.Tensor] = None, v: Optional[torch.Tensor] = None):
    """-> (attn_pool [B, D_mem], alpha [B, 1, S]); differentiable in M, x and the weights."""
    if M.dim() != 3:
        raise ValueError(f"attention memory must be [seq_len, batch, mem_dim], got {tuple(M.shape)}")
    if M.shape[0] > L.MSER_ATTN_POOL_MAX_S:
        raise ValueError(f"attention memory longer than {L.MSER_ATTN_POOL_MAX_S} positions")
    S, B, D = M.shape
    mem = {"simple": lambda: W.shape[1], "dot": lambda: D, "general": lambda: W.shape[0], "general2": lambda: W.shape[0],
           "concat": lambda: D if W.shape[1] > D else -1}[att_type]()
    if mem != D:
        raise ValueError(f"attention memory width {D} does not match the module (mem_dim {mem})")
    if att_type != "simple":
        cand = D if att_type == "dot" else (W.shape[1] if att_type != "concat" else W.shape[1] - D)
        if x is None or x.dim() != 2 or tuple(x.shape) != (B, cand):
            raise ValueError(f"MatchingAttention({att_type}): x must be [batch, cand_dim] = [{B}, {cand}], "
                             f"got {None if x is None else tuple(x.shape)}")
    return _AttnPoolFn.apply(att_type, M, x, mask, W, bias, v)
