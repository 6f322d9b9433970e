"""Golden vectors of the standalone DialogueRNN attention modules, from the REFERENCE ITSELF (CPU, torch fp32, eval mode).

    python tests/golden/make_golden_drnn_modules.py

Uses the import shim of make_golden.py (the reference checkout's ``model/`` imported as ``models``).  Writes
``drnn_modules_attention.npz``: for each case the inputs, the module's seeded initial parameters (``torch.manual_seed(seed)``
right before the constructor), the outputs (attn_pool, alpha), a fixed random upstream gradient for both outputs and the
gradients of every tensor input and parameter.  Arrays only.

Cases: MatchingAttention 'general', 'general2', 'dot', 'concat' and SimpleAttention at S in {1, 7, 150}.  'general2' is called
with a ragged mask (padded positions); 'dot', 'general' and 'concat' are called with that mask too, which the reference ignores.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden  # noqa: E402

D_MEM, D_CAND, D_A, B = 20, 12, 16, 3
TYPES = ("general", "general2", "dot", "concat", "simple")
SIZES = (1, 7, 150)


def _mask(S, seed):
    """[B, S] ragged: row 0 full, the others padded at the end (at least one valid position)."""
    rs = np.random.RandomState(seed)
    m = np.zeros((B, S), np.float32)
    for b in range(B):
        n = S if b == 0 else int(rs.randint(1, S + 1))
        m[b, :n] = 1.0
    return torch.from_numpy(m)


def attention_cases():
    from models.DialogueRNN import MatchingAttention, SimpleAttention
    rec = {"types": np.array(TYPES), "sizes": np.array(SIZES, np.int64),
           "dims": np.array([D_MEM, D_CAND, D_A, B], np.int64)}
    for ti, t in enumerate(TYPES):
        cand = D_MEM if t in ("dot", "simple") else D_CAND
        seed = 100 + ti
        torch.manual_seed(seed)
        net = SimpleAttention(D_MEM) if t == "simple" else MatchingAttention(D_MEM, cand, D_A, t)
        net.eval()
        names = [n for n, _ in net.named_parameters()]
        rec[f"{t}/keys"] = np.array(names if names else [""])[: len(names)]
        for n, p in net.named_parameters():
            rec[f"{t}/init/{n}"] = p.detach().numpy().copy()
        for S in SIZES:
            g = torch.Generator().manual_seed(1000 * ti + S)
            M = torch.randn(S, B, D_MEM, generator=g).requires_grad_(True)
            x = torch.randn(B, cand, generator=g).requires_grad_(True)
            mask = _mask(S, 7 * S + ti)
            gp = torch.randn(B, D_MEM, generator=g)
            ga = torch.randn(B, 1, S, generator=g)
            net.zero_grad()
            if t == "simple":
                pool, alpha = net(M)
            else:
                pool, alpha = net(M, x, mask)
            ((pool * gp).sum() + (alpha * ga).sum()).backward()
            k = f"{t}/S{S}/"
            rec[k + "M"], rec[k + "x"], rec[k + "mask"] = M.detach().numpy(), x.detach().numpy(), mask.numpy()
            rec[k + "gpool"], rec[k + "galpha"] = gp.numpy(), ga.numpy()
            rec[k + "pool"], rec[k + "alpha"] = pool.detach().numpy(), alpha.detach().numpy()
            rec[k + "dM"] = M.grad.numpy()
            if t != "simple":
                rec[k + "dx"] = x.grad.numpy()
            for n, p in net.named_parameters():
                rec[k + "d/" + n] = p.grad.detach().numpy().copy()
            print(t, S, float(pool.abs().sum()), float(M.grad.abs().sum()))
    np.savez_compressed(os.path.join(HERE, "drnn_modules_attention.npz"), **rec)


if __name__ == "__main__":
    make_golden._shim()
    attention_cases()
