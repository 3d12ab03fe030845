"""GPU: ww_gemm16_nt -- the 16-bit-operand GEMM core (operands resident in HBM as bf16 / fp16, fp32 accumulation) against
float64 torch on the SAME 16-bit operand values: the products are exact in fp32, so the only error is the accumulation
order (bound 2e-6 of the row scale at K = 1024); 16-bit output = that result rounded once."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def nat():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from wakeword_trainer_home_amd import _native
    _native.load()
    return _native


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("M,N,K", [(128, 128, 64), (256, 384, 128), (1, 1, 64), (130, 70, 192), (1000, 513, 1024), (4096, 1024, 576),
                                   (127, 129, 64)])
def test_gemm16_nt_matches_float64(nat, dtype, M, N, K):
    g = torch.Generator().manual_seed(M * 7 + N * 3 + K)
    a = (torch.randn(M, K, generator=g) * 0.5).to(dtype)
    b = (torch.randn(N, K, generator=g) * 0.5).to(dtype)
    ref = a.double() @ b.double().T
    scale = ref.abs().max().item() + 1e-30
    out = nat.gemm16_nt(a.to(DEV), b.to(DEV))
    assert out.dtype == torch.float32 and out.shape == (M, N)
    assert (out.cpu().double() - ref).abs().max().item() <= 3e-6 * scale
    out16 = nat.gemm16_nt(a.to(DEV), b.to(DEV), out_dtype=dtype)
    assert out16.dtype == dtype
    assert torch.equal(out16.cpu(), out.cpu().to(dtype))          # the fp32 result rounded once (RNE)


def test_gemm16_nt_rejects_bad_input(nat):
    a = torch.zeros(64, 64, dtype=torch.bfloat16, device=DEV)
    with pytest.raises(ValueError):
        nat.gemm16_nt(a, torch.zeros(64, 64, dtype=torch.float16, device=DEV))     # mixed operand types
    with pytest.raises(ValueError):
        nat.gemm16_nt(a.float(), a.float())                                          # fp32 operands belong to ww_linear_mfma_*
    with pytest.raises(nat.NativeError):
        nat.gemm16_nt(torch.zeros(64, 96, dtype=torch.bfloat16, device=DEV), torch.zeros(8, 96, dtype=torch.bfloat16, device=DEV))  # K % 64
    with pytest.raises(ValueError):
        nat.gemm16_nt(a, a[:, :32])


def test_gemm16_fp16_output_rounding_edges(nat):
    """fp16 output of ww_gemm16_nt at the edges of the rounding contract (RNE, overflow to inf -- the signal the loss scaler
    reads).  This output is stored by the epilogue's fp32 -> _Float16 conversion, not by Act<ww_f16>::pack2 (the conv layers'
    fp16 storage: tests/test_fp16_mode.py:test_conv_fwd_fp16_rounding_edges).  Operands are small integers and powers of two,
    so every fp32 result is exact: out[i][j] = a_i b_j + c_i d_j.  The stored fp16 must equal torch's
    ``fp32_result.to(float16)`` bit for bit: RNE ties (2049 -> 2048, 2051 -> 2052), subnormal results and subnormal ties (0.5
    and 1.5 x 2^-24), 65512 -> 65504, 65520 (the tie at the top) and beyond -> inf, never 65504 or NaN.  Subnormals are
    kept, not flushed."""
    q = 2.0 ** -24                                        # fp16 subnormal quantum
    a_vals = [3.0, 7.0, 1.0, 2.0 ** -14, 2.0 ** -10, q, 255.0, 65504.0, 0.5, -3.0, 1.5, 2.0 ** -7, 65504.0, 65504.0, 3 * q, -q]
    c_vals = [0.0] * 12 + [8.0, 16.0, 0.0, 0.0]          # 65504 + 8 = 65512 -> 65504; 65504 + 16 = 65520 (tie) -> inf
    b_vals = [683.0, 293.0, 1025.0, 1023.0, 2.0 ** -5, 2.0 ** -9, 2.0 ** -12, 0.75, 2.0, 4.0, 257.0, 65504.0, -1.0, 1.0, 0.5,
              1.0 + 2.0 ** -10, 1.5 * 2.0 ** -11, 2.0 ** -11, 3.0, 0.25]
    M, N, K = len(a_vals), len(b_vals), 64
    a = torch.zeros(M, K, dtype=torch.float64)
    b = torch.zeros(N, K, dtype=torch.float64)
    a[:, 0], a[:, 1] = torch.tensor(a_vals, dtype=torch.float64), torch.tensor(c_vals, dtype=torch.float64)
    b[:, 0], b[:, 1] = torch.tensor(b_vals, dtype=torch.float64), 1.0
    b[11, 1] = 0.0                                        # (65504^2 + 8 would not be exact in fp32)
    a16, b16 = a.half(), b.half()
    assert torch.equal(a16.double(), a) and torch.equal(b16.double(), b)          # the operands are fp16 values
    ref = a @ b.T
    assert torch.equal(ref.float().double(), ref)                                # ... and every result is exact in fp32
    want = ref.float().half()
    out32 = nat.gemm16_nt(a16.to(DEV), b16.to(DEV))
    assert torch.equal(out32.cpu().double(), ref)
    out16 = nat.gemm16_nt(a16.to(DEV), b16.to(DEV), out_dtype=torch.float16).cpu()
    bad = out16.view(torch.int16) != want.view(torch.int16)
    assert not bad.any(), [(ref[i, j].item(), out16[i, j].item(), want[i, j].item()) for i, j in bad.nonzero()[:8].tolist()]
    # the edges were really there
    assert out16[0, 0].item() == 2048.0 and out16[1, 1].item() == 2052.0                    # ties to even
    assert out16[5, 14].item() == 0.0 and out16[14, 14].item() == 2 * q                       # subnormal ties: 0.5q -> 0, 1.5q -> 2q
    assert out16[5, 7].item() == q and out16[3, 4].item() == 2.0 ** -19                       # 0.75q -> q; a subnormal kept
    assert out16[12, 13].item() == 65504.0 and out16[13, 13].item() == float("inf")           # 65512 -> 65504, 65520 -> inf
    assert out16[7, 8].item() == float("inf") and out16[6, 10].item() == float("inf")         # 131008, 65535
    assert out16[9, 11].item() == float("-inf") and not torch.isnan(out16).any()
