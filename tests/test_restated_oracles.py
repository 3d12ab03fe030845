"""The restated 16-bit references the GPU tests compare the matrix modes with (oracle/gru.py:gru_restated,
oracle/rounding.py:mround, the matrix type of oracle/mlp_head.py), checked on the CPU: without rounding the GRU restatement IS torch.nn.GRU (forward and autograd
backward, float64, to ~1e-12), and its rounding is round-to-nearest-even with overflow to inf, as an independent float64
restatement of RNE says and as torch's own ``.to(dtype)`` does."""
import math

import numpy as np
import pytest
import torch

from oracle.gru import gru_restated
from oracle.rounding import mround

MT = {"bf16": torch.bfloat16, "fp16": torch.float16}


@pytest.mark.parametrize("B,T,I,reverse,with_dy", [(3, 5, 9, False, True), (2, 4, 16, True, True), (4, 1, 7, False, True),
                                                   (3, 6, 5, True, False)])
def test_unrounded_restatement_is_torch_gru(B, T, I, reverse, with_dy):
    H = 128
    torch.manual_seed(B * 100 + T * 10 + I)
    ref = torch.nn.GRU(I, H, num_layers=1, batch_first=True, bidirectional=True).double()
    sfx = "_reverse" if reverse else ""
    P = [getattr(ref, n + "_l0" + sfx) for n in ("weight_ih", "weight_hh", "bias_ih", "bias_hh")]
    x = torch.randn(B, T, I, dtype=torch.float64, requires_grad=True)
    h0 = (torch.randn(2, B, H, dtype=torch.float64) * 0.5).requires_grad_(True)
    out, hn = ref(x, h0)
    d = 1 if reverse else 0
    sl = slice(H, 2 * H) if reverse else slice(0, H)
    dy = torch.randn(B, T, H, dtype=torch.float64) if with_dy else None
    dhn = torch.randn(B, H, dtype=torch.float64)
    loss = (hn[d] * dhn).sum() + ((out[:, :, sl] * dy).sum() if with_dy else 0.0)
    loss.backward()
    o = gru_restated(x, *P, h0=h0[d], dy=dy, dh_n=dhn, mtype=None, reverse=reverse)
    err = lambda a, b: (a - b).abs().max().item()
    assert err(o["y"], out[:, :, sl].detach()) <= 1e-12
    assert err(o["h_n"], hn[d].detach()) <= 1e-12
    assert err(o["dx"], x.grad) <= 1e-12
    assert err(o["dh0"], h0.grad[d]) <= 1e-12
    for k, p in zip(("dw_ih", "dw_hh", "db_ih", "db_hh"), P):
        assert err(o[k], p.grad) <= 1e-11, k
    # forward only: the same outputs, no gradients
    f = gru_restated(x, *P, h0=h0[d], mtype=None, reverse=reverse)
    assert torch.equal(f["y"], o["y"]) and "dx" not in f


def _rne(v, mtype):
    """Independent RNE of float64 values to bf16 / fp16: quantum 2^(e - p + 1) with e = max(floor(log2|v|), emin), numpy's
    round-half-even, overflow (|rounded| > max finite) to inf."""
    p, emin, emax = {torch.bfloat16: (8, -126, 127), torch.float16: (11, -14, 15)}[mtype]
    fmax = (2.0 - 2.0 ** (1 - p)) * 2.0 ** emax
    out = np.empty_like(v)
    for i, x in enumerate(v):
        if x == 0.0 or not math.isfinite(x):
            out[i] = x
            continue
        e = max(math.floor(math.log2(abs(x))), emin)
        q = 2.0 ** (e - p + 1)
        r = float(np.round(x / q)) * q
        out[i] = math.copysign(math.inf, x) if abs(r) > fmax else r
    return out


@pytest.mark.parametrize("mt", ["bf16", "fp16"])
def test_restated_rounding_is_rne_and_torchs(mt):
    """Ties (odd and even neighbours), fp16 / bf16 subnormals and their ties, the largest finite values, the first value that
    rounds up to inf and random fp32 data: mround == the independent RNE == torch's ``.to(dtype)``."""
    mtype = MT[mt]
    p, emin, emax = {torch.bfloat16: (8, -126, 127), torch.float16: (11, -14, 15)}[mtype]
    fmax = (2.0 - 2.0 ** (1 - p)) * 2.0 ** emax
    q1, qs = 2.0 ** (1 - p), 2.0 ** (emin - p + 1)        # quantum at 1.0, subnormal quantum
    vals = [1.0 + q1 / 2, 1.0 + 3 * q1 / 2, 1.0 + q1 / 4, 1.0 + 3 * q1 / 4, -(1.0 + q1 / 2), 3.0 + 3 * q1,
            qs / 2, 3 * qs / 2, 5 * qs / 2, qs / 4, 0.75 * qs, -3 * qs / 2, 2.0 ** emin * (1 - q1 / 2),
            fmax, fmax * (1 + q1 / 8), fmax + 2.0 ** (emax - p), -(fmax + 2.0 ** (emax - p)), fmax + 2.0 ** (emax - p) * 0.99,
            0.0, -0.0]
    g = torch.Generator().manual_seed(1)
    rnd = (torch.randn(4000, generator=g) * torch.exp2(torch.randint(-30, 20, (4000,), generator=g).float())).double()
    v = torch.cat([torch.tensor(vals, dtype=torch.float64), rnd])
    v = v.float().double()                                        # the device rounds fp32 values
    a = mround(v, mtype)
    assert torch.equal(a, v.float().to(mtype).double())
    b = torch.from_numpy(_rne(v.numpy(), mtype))
    same = (a == b) | (torch.isnan(a) & torch.isnan(b))
    assert bool(same.all()), v[~same][:8]
    # the edges really are edges: ties went to even, fp16 overflow is inf, subnormals survive
    assert a[0].item() == 1.0 and a[1].item() == 1.0 + 2 * q1
    assert a[6].item() == 0.0 and a[7].item() == 2 * qs and a[8].item() == 2 * qs
    assert a[13].item() == fmax and a[15].item() == math.inf and a[16].item() == -math.inf and a[17].item() == fmax


def test_head_oracle_matrix_type():
    """oracle/mlp_head.py: ``bf16=True`` is ``mtype=torch.bfloat16``; fp16 rounds the operands of both products to fp16."""
    from oracle.mlp_head import MLPHeadOracle
    torch.manual_seed(0)
    o = MLPHeadOracle(24, 32, 3, dropout=0.0)
    x = torch.randn(5, 24, dtype=torch.float64)
    a = o(x, training=False, bf16=True)
    assert torch.equal(a, o(x, training=False, mtype=torch.bfloat16))
    l0, l3 = o.classifier[0], o.classifier[3]
    r = lambda t: t.float().half().double()
    ref = r(torch.nn.functional.hardswish(r(x) @ r(l0.weight).t() + l0.bias)) @ r(l3.weight).t() + l3.bias
    assert (o(x, training=False, mtype=torch.float16) - ref).abs().max().item() <= 1e-12
    assert not torch.equal(o(x, training=False, mtype=torch.float16), o(x, training=False))
