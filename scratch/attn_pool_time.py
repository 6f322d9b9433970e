"""Attention pool at S = 200, B = 64, D = 500 (DialogueRNN's D_g): HIP-event time of mser_attn_pool_fwd / _bwd alone and of the
modules' forward + backward including their GEMMs; one JSON line (DESIGN §4 kernel table)."""
import os, sys, json
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "multimodal-framework-for-speaker-emotion-recognition_amd")]
import torch
from models.DialogueRNN import MatchingAttention, SimpleAttention
from mser import _lib as L, ops
from mser.attn_pool_fn import _desc, TYPES

S, B, D, Dc, Da = 200, 64, 500, 300, 100
dev = "cuda:0"
torch.manual_seed(0)
res = {}


def timed(fn, n=50):
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n * 1000.0   # us


M = torch.randn(S, B, D, device=dev)
x = torch.randn(B, D, device=dev)
mask = torch.ones(B, S, device=dev)
q = torch.randn(B, D, device=dev)
alpha = torch.empty(B, S, device=dev); pool = torch.empty(B, D, device=dev)
dpool = torch.randn(B, D, device=dev); dM = torch.empty(S, B, D, device=dev); dq = torch.empty(B, D, device=dev)
ds = torch.empty(B, S, device=dev)
for t in ("general2", "dot"):
    d = _desc(TYPES[t], M, alpha, pool, q=q, sqb=D, mask=mask)
    d.dpool, d.dM, d.dq, d.ds = dpool.data_ptr(), dM.data_ptr(), dq.data_ptr(), ds.data_ptr()
    res[f"{t}_kernel_fwd_us"] = timed(lambda: L.check(ops._lib().mser_attn_pool_fwd(d, ops._stream())))
    res[f"{t}_kernel_bwd_us"] = timed(lambda: L.check(ops._lib().mser_attn_pool_bwd(d, ops._stream())))
for t in ("general2", "concat", "simple"):
    net = (SimpleAttention(D) if t == "simple" else MatchingAttention(D, Dc, Da, t)).to(dev)
    Mg = M.clone().requires_grad_(True)
    xg = torch.randn(B, Dc, device=dev, requires_grad=True)
    def step():
        p, a = net(Mg) if t == "simple" else net(Mg, xg, mask)
        p.backward(dpool)
    res[f"{t}_module_fwd_bwd_us"] = timed(step, 20)
res["bytes_M"] = M.numel() * 4
print(json.dumps({k: round(v, 2) if isinstance(v, float) else v for k, v in res.items()}))
