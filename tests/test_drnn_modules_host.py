"""CPU: the standalone DialogueRNN attention modules (models.DialogueRNN SimpleAttention / MatchingAttention) against the reference's
constructor surface as recorded in tests/golden/drnn_modules_attention.npz: signatures, parameter names and order, shapes and
the seeded initial weights; and the C-ABI descriptor of the attention pool."""
import ctypes
import inspect
import os
import subprocess
import tempfile

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def G(golden_dir):
    return np.load(os.path.join(golden_dir, "drnn_modules_attention.npz"), allow_pickle=False)


def test_constructor_signatures_match_the_reference():
    from models.DialogueRNN import MatchingAttention, SimpleAttention
    assert list(inspect.signature(SimpleAttention.__init__).parameters)[1:] == ["input_dim"]
    assert list(inspect.signature(SimpleAttention.forward).parameters)[1:] == ["M", "x"]
    sig = inspect.signature(MatchingAttention.__init__).parameters
    assert list(sig)[1:] == ["mem_dim", "cand_dim", "alpha_dim", "att_type"]
    assert sig["alpha_dim"].default is None and sig["att_type"].default == "general"
    assert list(inspect.signature(MatchingAttention.forward).parameters)[1:] == ["M", "x", "mask"]


@pytest.mark.parametrize("t", ("general", "general2", "dot", "concat", "simple"))
def test_parameters_and_seeded_init_match_the_reference(G, t):
    from models.DialogueRNN import MatchingAttention, SimpleAttention
    D_mem, D_cand, D_a, _ = (int(v) for v in G["dims"])
    cand = D_mem if t in ("dot", "simple") else D_cand
    torch.manual_seed(100 + list(G["types"]).index(t))
    net = SimpleAttention(D_mem) if t == "simple" else MatchingAttention(D_mem, cand, D_a, t)
    names = [n for n, _ in net.named_parameters()]
    assert names == [str(k) for k in G[f"{t}/keys"]]
    assert list(net.state_dict().keys()) == names
    for n, p in net.named_parameters():
        ref = G[f"{t}/init/{n}"]
        assert tuple(p.shape) == ref.shape, n
        assert np.array_equal(p.detach().numpy(), ref), n


def test_constructor_asserts_stay_as_in_the_reference():
    from models.DialogueRNN import MatchingAttention
    with pytest.raises(AssertionError):
        MatchingAttention(8, 8, att_type="concat")
    with pytest.raises(AssertionError):
        MatchingAttention(8, 6, att_type="dot")
    m = MatchingAttention(8, 6, 5, "concat")
    assert tuple(m.transform.weight.shape) == (5, 14) and m.transform.bias is None and tuple(m.vector_prod.weight.shape) == (1, 5)


def test_forward_has_no_cpu_fallback():
    from models.DialogueRNN import MatchingAttention, SimpleAttention
    with pytest.raises(RuntimeError):
        MatchingAttention(8, 6, att_type="general")(torch.zeros(3, 2, 8), torch.zeros(2, 6))
    with pytest.raises(RuntimeError):
        SimpleAttention(8)(torch.zeros(3, 2, 8))


def test_attn_pool_descriptor_matches_the_header():
    from mser import _lib
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "mser.h"\nint main(){printf("%zu %zu %zu %d %d %d\\n", '
           'sizeof(mser_attn_pool_desc), offsetof(mser_attn_pool_desc, v), offsetof(mser_attn_pool_desc, ds), MSER_ATT_CONCAT, '
           'MSER_ATT_GENERAL2, MSER_ATTN_POOL_MAX_S);return 0;}\n')
    with tempfile.TemporaryDirectory() as td:
        c = os.path.join(td, "s.c")
        open(c, "w").write(src)
        exe = os.path.join(td, "s")
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), c, "-o", exe])
        vals = [int(x) for x in subprocess.check_output([exe]).split()]
    D = _lib.AttnPoolDesc
    assert vals == [ctypes.sizeof(D), D.v.offset, D.ds.offset, _lib.MSER_ATT_CONCAT, _lib.MSER_ATT_GENERAL2, _lib.MSER_ATTN_POOL_MAX_S]
