"""Float64 restatement of ResNet18Wakeword with 16-bit ACTIVATION STORAGE (``storage="bf16" | "fp16"``), shared by
test_resnet_storage_host.py and test_resnet_storage_gpu.py.

The contract: arithmetic is wide, a value is rounded (RNE to the storage type S) exactly where the device stores a tensor and nowhere
else -- y0 = S(conv1(x)), a0 = S(relu(bn1(y0))), per block c1 = S(conv(x, S(W1))), a1 = S(relu(bn1(c1))), c2 = S(conv(a1, S(W2))),
cd = S(conv(x, S(Wd))), out = S(relu(bn2(c2) + (x | bn_d(cd)))) -- and a gradient is rounded where the device stores IT: the gradient
of each of those tensors, the downsample path's input gradient before conv1's is added to it, and S(dpooled / HW).  BatchNorm statistics
are those of the stored tensor.  The pieces are tests/resnet_cases.py's (conv2d_fwd / conv2d_bwd, the pool, ``_bn``); ``_Store`` is the
autograd shell that rounds the value forward and the gradient backward.  ``st=None`` is ResNetRestated itself, bit for bit.

Also here: the single ops in float64 (BatchNorm forward / backward as the kernels compute them, the mean, the mask) and the half-ulp
helper, for the tests that hold every stored tensor of a device run to the bound of the op that made it."""
import torch

from oracle.rounding import mround
from tests.resnet_cases import BN_EPS, LAYERS, ResNetRestated, _bn, _Conv, _Linear, _Pool

ST_NAMES = ("ww_conv2d_st_scratch_bytes", "ww_conv2d_st_fwd", "ww_conv2d_st_bwd", "ww_bn_act_st_fwd", "ww_bn_act_st_bwd",
            "ww_conv2d_stem_st_fwd", "ww_conv2d_stem_st_bwd_dw", "ww_maxpool3x3s2_st_fwd", "ww_maxpool3x3s2_st_bwd", "ww_mean_hw_st_fwd",
            "ww_mean_hw_st_bwd", "ww_relu_mask_st_bwd")
# (B, H, W, Cin, Cout, k, stride): the layer shapes of test_resnet_gpu.py with the channel counts that are no multiple of 8 widened to
# the next one (4 -> 8, 12 -> 16: a 16-byte access of a 16-bit row is 8 elements).  One pixel and one tap; only the centre tap inside
# the image; M tiles that span rows and samples, odd sizes, channel counts below a tile (both strides); the 1x1 stride-2 downsample
# whose dx is zero at odd pixels; 80-byte rows; K = 2304 and eight column tiles; K = 4608 with M = 4; M = 1360: ten dW row ranges
ST_SHAPES = [(1, 1, 1, 8, 8, 1, 1), (1, 1, 1, 8, 8, 3, 1), (2, 5, 7, 8, 16, 3, 1), (2, 5, 7, 8, 16, 3, 2), (3, 6, 4, 64, 128, 3, 2),
             (3, 6, 4, 64, 128, 1, 2), (5, 10, 9, 40, 64, 3, 1), (2, 3, 3, 256, 512, 3, 2), (1, 2, 2, 512, 512, 3, 1),
             (4, 20, 17, 64, 64, 3, 1)]
EPS32 = 2.0 ** -24                      # unit round-off of fp32
MANT = {torch.bfloat16: 8, torch.float16: 11, torch.float32: 24}      # significand bits, the hidden one included
MIN_EXP = {torch.bfloat16: -126, torch.float16: -14, torch.float32: -126}


def half_ulp(v, st):
    """Half a unit in the last place of type ``st`` at magnitude |v| (float64 tensor): the most RNE moves a value of that size
    (subnormals: the fixed spacing below 2^MIN_EXP)."""
    e = torch.floor(torch.log2(v.abs().clamp_min(2.0 ** MIN_EXP[st]))).clamp_min(MIN_EXP[st])
    return 0.5 * torch.exp2(e - (MANT[st] - 1))


# ------------------------------------------------------------------------------------------ the model
class _Store(torch.autograd.Function):
    """A storage point: the value is rounded on the way forward, its gradient on the way back."""

    @staticmethod
    def forward(ctx, x, st):
        ctx.st = st
        return mround(x, st)

    @staticmethod
    def backward(ctx, g):
        return mround(g, ctx.st), None


class _StoreGrad(torch.autograd.Function):
    """A point where only a GRADIENT is stored (the downsample path's dx, before conv1's is accumulated onto it)."""

    @staticmethod
    def forward(ctx, x, st):
        ctx.st = st
        return x.view_as(x)

    @staticmethod
    def backward(ctx, g):
        return mround(g, ctx.st), None


def store(x, st):
    return x if st is None else _Store.apply(x, st)


def basic_block_st(x, sd, pre, stride, training, st, trace=None):
    """tests/resnet_cases.basic_block with the storage points; the matrix mode is the storage type."""
    c1 = store(_Conv.apply(x, sd[pre + "conv1.weight"], stride, st), st)
    p1 = _bn(c1, sd, pre + "bn1.", training)
    a1 = store(p1.clamp_min(0.0), st)
    c2 = store(_Conv.apply(a1, sd[pre + "conv2.weight"], 1, st), st)
    o = _bn(c2, sd, pre + "bn2.", training)
    idn = x
    if pre + "downsample.0.weight" in sd:
        xd = x if st is None else _StoreGrad.apply(x, st)
        cd = store(_Conv.apply(xd, sd[pre + "downsample.0.weight"], stride, st), st)
        idn = _bn(cd, sd, pre + "downsample.1.", training)
    p2 = o + idn
    if trace is not None:
        trace += [p1, p2]
    return store(p2.clamp_min(0.0), st)


class ResNetStorageRestated(ResNetRestated):
    """ResNetRestated whose activations are stored in ``st`` (None: no storage point, the parent's arithmetic bit for bit).
    ``perturb`` = (relative size, seed): every value is multiplied by 1 + size * N(0,1) just ahead of each storage rounding -- an
    equally valid evaluation of the same contract (the device's fp32 arithmetic differs from float64 by about that much), used to
    measure how far roundings that flip move the end-to-end figures."""

    def __init__(self, sd, dropout=0.0, seed=0, st=None, perturb=None):
        super().__init__(sd, dropout=dropout, seed=seed, mtype=st)
        self.st, self.perturb = st, perturb
        self._gen = torch.Generator().manual_seed(perturb[1]) if perturb else None

    def _store(self, x):
        if self.perturb:
            x = x * (1.0 + self.perturb[0] * torch.randn(x.shape, generator=self._gen, dtype=torch.float64))
        return store(x, self.st)

    def _block(self, x, pre, stride, training):
        if not self.perturb:
            return basic_block_st(x, self.sd, pre, stride, training, self.st, self.pres)
        sd, st = self.sd, self.st
        c1 = self._store(_Conv.apply(x, sd[pre + "conv1.weight"], stride, st))
        p1 = _bn(c1, sd, pre + "bn1.", training)
        c2 = self._store(_Conv.apply(self._store(p1.clamp_min(0.0)), sd[pre + "conv2.weight"], 1, st))
        idn = x
        if pre + "downsample.0.weight" in sd:
            cd = self._store(_Conv.apply(_StoreGrad.apply(x, st), sd[pre + "downsample.0.weight"], stride, st))
            idn = _bn(cd, sd, pre + "downsample.1.", training)
        p2 = _bn(c2, sd, pre + "bn2.", training) + idn
        self.pres += [p1, p2]
        return self._store(p2.clamp_min(0.0))

    def forward(self, x, training=True, step=0, sample_offset=0):
        sd, st = self.sd, self.st
        self.pres = []
        y0 = self._store(_Conv.apply(x[:, 0, :, :, None], sd["resnet.conv1.weight"], 2, None))
        p = _bn(y0, sd, "resnet.bn1.", training)
        self.pres.append(p)
        h = _Pool.apply(self._store(p.clamp_min(0.0)))
        for i, (_, stride) in enumerate(LAYERS):
            for j in range(2):
                h = self._block(h, f"resnet.layer{i + 1}.{j}.", stride if j == 0 else 1, training)
        pooled = h.mean((1, 2))
        if training and self.p > 0:
            pooled = pooled * self.keep_mask(pooled.shape[0], pooled.shape[1], step, sample_offset)
        if training:
            for k in sd:
                if k.endswith("num_batches_tracked"):
                    sd[k] = sd[k] + 1
        return _Linear.apply(pooled, sd["resnet.fc.1.weight"], sd["resnet.fc.1.bias"], st)


# ------------------------------------------------------------------------------------------ single ops in float64
def col_sums(x):
    """x (..., C) float64 -> (sum, sum of squares, sum |x|) over the rows, each (C)."""
    r = x.reshape(-1, x.shape[-1])
    return r.sum(0), (r * r).sum(0), r.abs().sum(0)


def bn_vectors(s, q, M, gamma, beta, eps=BN_EPS):
    """scale|shift and mean|rstd from the column sums, as k_bn_finish forms them (float64)."""
    mean = s / M
    var = (q / M - mean * mean).clamp_min(0.0)
    rstd = 1.0 / torch.sqrt(var + eps)
    scale = gamma * rstd
    return torch.cat([scale, beta - mean * scale]), torch.cat([mean, rstd]), var


def bn_apply(x, ss, relu, res=None, res_ss=None):
    """act(x * scale + shift + idn) and the scale of its fp32 round-off: the sum of |terms| (float64)."""
    C = x.shape[-1]
    z, mag = x * ss[:C] + ss[C:], (x * ss[:C]).abs() + ss[C:].abs()
    if res is not None:
        idn, imag = (res, res.abs()) if res_ss is None else (res * res_ss[:C] + res_ss[C:], (res * res_ss[:C]).abs() + res_ss[C:].abs())
        z, mag = z + idn, mag + imag
    return (z.clamp_min(0.0) if relu else z), mag, z


def bn_bwd(x, da, ss, mr, relu, training):
    """The BatchNorm(+ReLU) backward as the kernels compute it (bnact_bwd_one) in float64 -> (dx, dgamma, dbeta, |terms| of dx, z)."""
    C = x.shape[-1]
    M = x.numel() // C
    sc, sf, mu, rs = ss[:C], ss[C:], mr[:C], mr[C:]
    z = x * sc + sf
    dz = da * (z > 0) if relu else da
    xh = (x - mu) * rs
    flat = lambda t: t.reshape(-1, C)
    s1, s2 = flat(dz).sum(0), flat(dz * xh).sum(0)
    a1, a2 = flat(dz).abs().sum(0), flat(dz * xh).abs().sum(0)
    if not training:
        return sc * dz, s2, s1, (sc * dz).abs(), z, (a1, a2)
    dx = sc * (dz - s1 / M - xh * s2 / M)
    mag = sc.abs() * (dz.abs() + a1 / M + xh.abs() * a2 / M)
    return dx, s2, s1, mag, z, (a1, a2)
