"""``ResNet18Wakeword`` with the constructor, ``forward`` contract and ``state_dict`` keys of the reference class
(``src/models/architectures.py:14-65``: torchvision's ``resnet18`` with ``conv1`` replaced by ``Conv2d(1, 64, 7, 2, 3, bias=False)`` and
``fc`` by ``Sequential(Dropout, Linear)`` -- ``resnet.conv1.weight`` ... ``resnet.layer4.1.bn2.num_batches_tracked``,
``resnet.fc.1.weight``, ``resnet.fc.1.bias``: 122 keys), running on ``ww_conv2d_fwd/bwd`` (dense k x k Conv2d as an implicit GEMM on the
matrix cores), ``ww_conv2d_stem_*``, ``ww_maxpool3x3s2_*``, ``ww_bn_act_*``, ``ww_add_relu_fwd``, ``ww_pool_hw_fwd`` and the MFMA
``fc``, channels-last ``(B, H, W, C)`` all the way.  Weights keep ``nn.Conv2d``'s ``(Cout, Cin, k, k)`` layout, so checkpoints interchange
with the reference.  torchvision itself is not available in this build environment: the architecture is restated from its
published definition (``tests/resnet_cases.py`` carries the same restatement in float64).

The stem (conv1 -> bn1 -> ReLU -> maxpool) is ONE autograd node and so is a ``BasicBlock`` (conv1 -> BN+ReLU -> conv2 -> BN ->
[downsample conv1x1 -> BN] -> add+ReLU); a block keeps its input, the two (three) pre-BatchNorm convolution outputs, conv2's input
and its own output for the backward.  Weight and BatchNorm gradients are born in their slots of the model's flat bucket, the sums
of the weight-gradient partials wait for the one flush at the end of the backward pass.

``storage="bf16" | "fp16"`` (opt-in; it must equal the matrix ``mode``) keeps every (B,H,W,C) activation tensor between the stem
convolution and the global mean, every gradient of one and everything autograd saves of them in that type (the ``*_st_*`` kernels):
values are rounded exactly where a tensor is stored, arithmetic, BatchNorm vectors, parameters and their gradients stay fp32, and a
block's tail relu(bn2(c2) + identity) is one pass that never stores bn2(c2) or bn_d(cd); the block BatchNorms' batch statistics come
from the convolutions' own epilogue (only the stem's takes a pass over its input).  The default, ``storage="fp32"``, is the
path described above, unchanged; state-dict keys, parameter layouts and initialisation do not depend on it."""
import torch
import torch.nn as nn

from .. import _native as nat
from .flat_buckets import FlatBuckets, grad_slot
from .heads import MFMALinear
from .mobilenet import _BN, _Conv, _PoolFn
from .recurrent import _HiddenDropout
from .storage import _storage

LAYERS = ((64, 1), (128, 2), (256, 2), (512, 2))          # (planes, stride of the stage's first block); two blocks per stage


def _no_cpu(who, x):
    if not x.is_cuda:
        raise nat.NativeError(f"{who} runs on hand-written HIP kernels only: the input is on '{x.device}', need an MI355X "
                              "('cuda') device -- there is no CPU fallback")


def _bn(c):
    """torchvision's ``nn.BatchNorm2d(c)``: eps 1e-5, momentum 0.1, weight 1, bias 0."""
    bn = _BN(c)
    bn.eps, bn.momentum = 1e-5, 0.1
    return bn


def _bn_fwd(bn, y, act, **st):
    """BatchNorm (+ activation) of a convolution output -> (a, ss, mr); counts the training forward on the host.  A 16-bit y goes
    through ww_bn_act_st_fwd, which also takes the residual of a block's tail and the statistics partials the convolution's
    epilogue left (``st``: res, res_ss, want_y, part)."""
    bnp = nat.make_bn(bn.weight, bn.bias, bn.running_mean, bn.running_var, momentum=bn.momentum, eps=bn.eps, training=bn.training)
    if y.dtype is torch.float32:
        a, ss, mr = nat.bn_act_fwd(y, bnp, act, y.shape[-1])
    else:
        a, ss, mr = nat.bn_act_st_fwd(y, bnp, act, y.shape[-1], **st)
    if bn.training:
        bn._pending_tracked += 1
    return a, ss, mr


def _defer_slots(params, dev):
    """(gradient-bucket slots of ``params``, defer) -- deferral needs every slot (a queued sum may only land in a tensor autograd
    adopts unread) and a running backward pass to flush it."""
    slots = [grad_slot(p) for p in params]
    defer = all(s is not None for s in slots) and nat.defer_begin(dev)
    return (slots if defer else [None] * len(params)), defer


class _ConvFn(torch.autograd.Function):
    """A stand-alone NativeConv2d."""

    @staticmethod
    def forward(ctx, x, weight, mod):
        ctx.save_for_backward(x, weight)
        ctx.mod = mod
        if x.dtype is not torch.float32:
            return nat.conv2d_st_fwd(x, weight, mod.stride)
        return nat.conv2d_fwd(x, weight, mod.stride, mode=mod.mode)

    @staticmethod
    def backward(ctx, dy):
        x, weight = ctx.saved_tensors
        mod = ctx.mod
        (slot,), defer = _defer_slots([mod.weight], x.device)
        if x.dtype is not torch.float32:
            dx, dw = nat.conv2d_st_bwd(x, weight, dy.contiguous(), mod.stride, need_dx=ctx.needs_input_grad[0], dw_out=slot, defer=defer)
        else:
            dx, dw = nat.conv2d_bwd(x, weight, dy.contiguous(), mod.stride, mode=mod.mode, need_dx=ctx.needs_input_grad[0], dw_out=slot,
                                    defer=defer)
        return dx, dw, None


class NativeConv2d(nn.Module):
    """``nn.Conv2d(cin, cout, k, stride, padding=k // 2, bias=False)`` on (B, H, W, C) channels-last activations.  ``weight``
    (Cout, Cin, k, k) is nn.Conv2d's, with its initialisation.  ``storage``: the type of x, y and their gradients (see the module text)."""

    def __init__(self, cin, cout, k, stride=1, mode="fp32", storage="fp32"):
        super().__init__()
        mode, storage = _storage(mode, storage)
        if cin < 4 or cout < 4 or cin % 4 or cout % 4:
            raise nat.NativeError(f"the HIP Conv2d kernels take channel counts that are positive multiples of 4, got {cin} -> {cout}")
        if storage is not torch.float32 and (cin % 8 or cout % 8):
            raise nat.NativeError(f"16-bit activation storage takes channel counts that are multiples of 8, got {cin} -> {cout}")
        if k not in (1, 3, 5, 7) or stride not in (1, 2):
            raise nat.NativeError(f"the HIP Conv2d kernels take an odd kernel_size in 1..7 and stride 1 or 2, got {k}, {stride}")
        ref = nn.Conv2d(cin, cout, k, stride, k // 2, bias=False)           # torch's own initialisation
        self.weight = nn.Parameter(ref.weight.detach().clone())
        self.in_channels, self.out_channels, self.kernel_size, self.stride = cin, cout, k, stride
        self.mode, self.storage = mode, storage

    def forward(self, x):
        _no_cpu("NativeConv2d", x)
        if x.dim() != 4 or x.shape[3] != self.in_channels:
            raise ValueError(f"expected input (B,H,W,{self.in_channels}), got {tuple(x.shape)}")
        return _ConvFn.apply(x.to(self.storage).contiguous(), self.weight, self)


class _StemFn(torch.autograd.Function):
    """x (B,H,W) -> maxpool(relu(bn1(conv1(x)))).  Saved: x, the convolution output, the activation the pool read."""

    @staticmethod
    def forward(ctx, x, w, gamma, beta, net):
        st = net.storage is not torch.float32
        y = nat.conv2d_stem_st_fwd(x, w, net.conv1.stride, net.storage) if st else nat.conv2d_stem_fwd(x, w, net.conv1.stride)
        a, ss, mr = _bn_fwd(net.bn1, y, nat.LIN_RELU)
        ctx.save_for_backward(x, y, a, ss, mr)
        ctx.net, ctx.training = net, net.bn1.training
        return nat.maxpool3x3s2_st_fwd(a) if st else nat.maxpool3x3s2_fwd(a)

    @staticmethod
    def backward(ctx, dout):
        x, y, a, ss, mr = ctx.saved_tensors
        net = ctx.net
        st = y.dtype is not torch.float32
        pool_bwd, bn_bwd, stem_dw = ((nat.maxpool3x3s2_st_bwd, nat.bn_act_st_bwd, nat.conv2d_stem_st_bwd_dw) if st else
                                     (nat.maxpool3x3s2_bwd, nat.bn_act_bwd, nat.conv2d_stem_bwd_dw))
        da = pool_bwd(a, dout.contiguous())
        dy, dgamma, dbeta = bn_bwd(y, da, ss, mr, nat.LIN_RELU, ctx.training, y.shape[-1], dgamma_out=grad_slot(net.bn1.weight),
                                   dbeta_out=grad_slot(net.bn1.bias))
        (slot,), defer = _defer_slots([net.conv1.weight], x.device)
        dw = stem_dw(x, dy, net.conv1.weight.shape, net.conv1.stride, dw_out=slot, defer=defer)
        return None, dw, dgamma, dbeta, None


class _BlockFn(torch.autograd.Function):
    """c1 = conv1(x); a1 = relu(bn1(c1)); c2 = conv2(a1); out = relu(bn2(c2) + (x | bn_d(conv_d(x)))).
    Saved: x, c1, a1, c2, [cd], out and the BatchNorms' (scale|shift, mean|rstd)."""

    @staticmethod
    def forward(ctx, x, blk, *params):
        mode, s = blk.mode, blk.stride
        if x.dtype is not torch.float32:
            return _BlockFn._forward_st(ctx, x, blk, params)
        c1 = nat.conv2d_fwd(x, params[0], s, mode=mode)
        a1, ss1, mr1 = _bn_fwd(blk.bn1, c1, nat.LIN_RELU)
        c2 = nat.conv2d_fwd(a1, params[3], 1, mode=mode)
        o2, ss2, mr2 = _bn_fwd(blk.bn2, c2, nat.LIN_NONE)
        saved = [x, c1, a1, c2, ss1, mr1, ss2, mr2]
        if blk.downsample is not None:
            cd = nat.conv2d_fwd(x, params[6], s, mode=mode)
            idn, ssd, mrd = _bn_fwd(blk.downsample[1], cd, nat.LIN_NONE)
            saved += [cd, ssd, mrd]
        else:
            idn = x
        out = nat.add_relu_fwd(o2, idn)
        ctx.save_for_backward(out, *saved, *params)
        ctx.blk, ctx.training, ctx.n_saved = blk, blk.bn1.training, len(saved)
        return out

    @staticmethod
    def _forward_st(ctx, x, blk, params):
        """The 16-bit-storage forward: the same saved list, but bn2(c2) and bn_d(cd) are never stored -- the tail is one pass."""
        s = blk.stride

        def conv(inp, w, stride, bn):
            """-> (the convolution's output, its statistics partials from the conv epilogue when bn will take batch statistics)"""
            return nat.conv2d_st_fwd(inp, w, stride, stats=True) if bn.training else (nat.conv2d_st_fwd(inp, w, stride), None)
        c1, p1 = conv(x, params[0], s, blk.bn1)
        a1, ss1, mr1 = _bn_fwd(blk.bn1, c1, nat.LIN_RELU, part=p1)
        c2, p2 = conv(a1, params[3], 1, blk.bn2)
        if blk.downsample is not None:
            cd, pd = conv(x, params[6], s, blk.downsample[1])
            _, ssd, mrd = _bn_fwd(blk.downsample[1], cd, nat.LIN_NONE, want_y=False, part=pd)
            out, ss2, mr2 = _bn_fwd(blk.bn2, c2, nat.LIN_RELU, res=cd, res_ss=ssd, part=p2)
            saved = [x, c1, a1, c2, ss1, mr1, ss2, mr2, cd, ssd, mrd]
        else:
            out, ss2, mr2 = _bn_fwd(blk.bn2, c2, nat.LIN_RELU, res=x, part=p2)
            saved = [x, c1, a1, c2, ss1, mr1, ss2, mr2]
        ctx.save_for_backward(out, *saved, *params)
        ctx.blk, ctx.training, ctx.n_saved = blk, blk.bn1.training, len(saved)
        return out

    @staticmethod
    def backward(ctx, dout):
        out, *rest = ctx.saved_tensors
        saved, params = rest[:ctx.n_saved], rest[ctx.n_saved:]
        x, c1, a1, c2, ss1, mr1, ss2, mr2 = saved[:8]
        blk, tr = ctx.blk, ctx.training
        s = blk.stride
        if x.dtype is torch.float32:
            relu_mask, bn_bwd, conv_bwd, cm = nat.relu_mask_bwd, nat.bn_act_bwd, nat.conv2d_bwd, dict(mode=blk.mode)
        else:                                       # 16-bit storage: the storage type is the matrix mode
            relu_mask, bn_bwd, conv_bwd, cm = nat.relu_mask_st_bwd, nat.bn_act_st_bwd, nat.conv2d_st_bwd, {}
        need_dx = ctx.needs_input_grad[0]
        mods = [blk.conv1, blk.bn1, blk.conv2, blk.bn2] + (list(blk.downsample) if blk.downsample is not None else [])
        # gradients born in their slots of the model's flat bucket, so the sums of the weight-gradient partials can wait for the
        # ONE flush at the end of the backward pass
        wslots, defer = _defer_slots([m.weight for m in mods[::2]], x.device)
        bns = mods[1::2]
        gslots = [(grad_slot(b.weight), grad_slot(b.bias)) for b in bns]
        grads = [None] * len(params)
        dsum = relu_mask(dout.contiguous(), out)                    # feeds bn2 and the skip path alike
        dc2, grads[4], grads[5] = bn_bwd(c2, dsum, ss2, mr2, nat.LIN_NONE, tr, c2.shape[-1], dgamma_out=gslots[1][0], dbeta_out=gslots[1][1])
        da1, grads[3] = conv_bwd(a1, params[3], dc2, 1, dw_out=wslots[1], defer=defer, **cm)
        dc1, grads[1], grads[2] = bn_bwd(c1, da1, ss1, mr1, nat.LIN_RELU, tr, c1.shape[-1], dgamma_out=gslots[0][0], dbeta_out=gslots[0][1])
        if blk.downsample is not None:
            cd, ssd, mrd = saved[8:11]
            dcd, grads[7], grads[8] = bn_bwd(cd, dsum, ssd, mrd, nat.LIN_NONE, tr, cd.shape[-1], dgamma_out=gslots[2][0],
                                             dbeta_out=gslots[2][1])
            dx, grads[6] = conv_bwd(x, params[6], dcd, s, need_dx=need_dx, dw_out=wslots[2], defer=defer, **cm)
        else:
            dx = dsum if need_dx else None
        # conv1's input gradient is added onto the skip path's
        dx, grads[0] = conv_bwd(x, params[0], dc1, s, need_dx=need_dx, dx=dx, dw_out=wslots[0], defer=defer, **cm)
        return (dx, None) + tuple(grads)


class BasicBlock(nn.Module):
    """torchvision's BasicBlock (expansion 1): children conv1, bn1, conv2, bn2 and, where the shape changes, ``downsample`` =
    Sequential(conv1x1 stride s, BatchNorm).  ``storage``: the type of its input, its output and everything between."""

    def __init__(self, inplanes, planes, stride=1, mode="fp32", storage="fp32"):
        super().__init__()
        mode, storage = _storage(mode, storage)
        if storage is not torch.float32 and (inplanes % 8 or planes % 8):
            raise nat.NativeError(f"BasicBlock: 16-bit activation storage takes channel multiples of 8, got {inplanes} -> {planes}")
        if stride not in (1, 2) or inplanes % 4 or planes % 4 or inplanes < 4 or planes < 4:
            raise nat.NativeError(f"BasicBlock: the HIP Conv2d kernels take channel multiples of 4 and stride 1 or 2, got "
                                  f"{inplanes} -> {planes}, stride {stride}")
        self.conv1, self.bn1 = _Conv(inplanes, planes, 3, stride), _bn(planes)
        self.conv2, self.bn2 = _Conv(planes, planes, 3, 1), _bn(planes)
        self.downsample = nn.Sequential(_Conv(inplanes, planes, 1, stride), _bn(planes)) if stride != 1 or inplanes != planes else None
        for conv in [self.conv1, self.conv2] + ([self.downsample[0]] if self.downsample is not None else []):
            nn.init.kaiming_normal_(conv.weight, mode="fan_out", nonlinearity="relu")       # torchvision's ResNet initialisation
        self.stride, self.inplanes = stride, inplanes
        self.mode, self.storage = mode, storage

    def forward(self, x):
        _no_cpu("BasicBlock", x)
        if x.dim() != 4 or x.shape[3] != self.inplanes:
            raise ValueError(f"expected input (B,H,W,{self.inplanes}), got {tuple(x.shape)}")
        params = [self.conv1.weight, self.bn1.weight, self.bn1.bias, self.conv2.weight, self.bn2.weight, self.bn2.bias]
        if self.downsample is not None:
            params += [self.downsample[0].weight, self.downsample[1].weight, self.downsample[1].bias]
        return _BlockFn.apply(x.to(self.storage).contiguous(), self, *params)


class _StemConv(nn.Module):
    """Parameter holder for the reference's ``nn.Conv2d(1, 64, 7, 2, 3, bias=False)``, with nn.Conv2d's own initialisation."""

    def __init__(self, cout=64, k=7, stride=2):
        super().__init__()
        self.weight = nn.Parameter(nn.Conv2d(1, cout, k, stride, k // 2, bias=False).weight.detach().clone())
        self.k, self.stride = k, stride


class _MeanFn(torch.autograd.Function):
    """(B,H,W,C) in 16-bit storage -> the (B,C) fp32 mean; its gradient is stored as S(dpooled / HW)."""

    @staticmethod
    def forward(ctx, x):
        B, H, W, Cn = x.shape
        ctx.full, ctx.dtype = x.shape, x.dtype
        return nat.mean_hw_st_fwd(x.reshape(B, H * W, Cn))

    @staticmethod
    def backward(ctx, ds):
        return nat.mean_hw_st_bwd(ds.contiguous(), ctx.full[1] * ctx.full[2], ctx.dtype).reshape(ctx.full)


class _ResNet(nn.Module):
    """torchvision's resnet18 module tree (conv1, bn1, layer1..4, fc): the children that hold no state are not registered."""

    def __init__(self, num_classes, dropout, mode, dropout_seed, storage=torch.float32):
        super().__init__()
        self.storage = storage
        self.dropout, self.dropout_seed = float(dropout), dropout_seed
        self.dropout_step, self.sample_offset, self.fc_step = 0, 0, 0
        self.conv1, self.bn1 = _StemConv(), _bn(64)
        inplanes = 64
        for i, (planes, stride) in enumerate(LAYERS):
            setattr(self, f"layer{i + 1}", nn.Sequential(BasicBlock(inplanes, planes, stride, mode, storage),
                                                         BasicBlock(planes, planes, 1, mode, storage)))
            inplanes = planes
        # indices as the reference replaces fc: Dropout(dropout), Linear(512, num_classes)
        self.fc = nn.Sequential(_HiddenDropout(dropout, self), MFMALinear(inplanes, num_classes, mode=mode))

    def forward(self, x):
        h = _StemFn.apply(x, self.conv1.weight, self.bn1.weight, self.bn1.bias, self)
        for i in range(len(LAYERS)):
            h = getattr(self, f"layer{i + 1}")(h)
        return self.fc((_PoolFn if self.storage is torch.float32 else _MeanFn).apply(h))


class ResNet18Wakeword(FlatBuckets, nn.Module):
    """The reference's ResNet18Wakeword.  Its parameters live in one flat bucket (fused clip + optimizer, one all-reduce,
    graph-capturable step).  ``forward`` takes (B,1,F,T) feature batches."""
    hip_backed = True      # every op is a HIP kernel of this build: the Trainer may run its sync-free step (no host reads)

    def __init__(self, num_classes: int = 2, pretrained: bool = False, dropout: float = 0.3, input_channels: int = 1,
                 dropout_seed: int = 0, mode: str = "fp32", storage: str = "fp32"):
        super().__init__()
        if pretrained:
            raise ValueError("pretrained ImageNet weights cannot be downloaded in this build (pass pretrained=False)")
        if input_channels != 1:
            raise ValueError(f"resnet18: the native stem takes one-channel spectrograms, got input_channels={input_channels}")
        if not 0.0 <= dropout < 1.0:
            raise ValueError(f"dropout must be in [0, 1), got {dropout}")
        m, st = _storage(mode, storage)
        self.resnet = _ResNet(num_classes, dropout, m, dropout_seed, st)

    @property
    def sample_offset(self):
        return self.resnet.sample_offset

    @sample_offset.setter
    def sample_offset(self, v):
        self.resnet.sample_offset = v

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        if x.dim() != 4 or x.shape[1] != 1:
            raise ValueError(f"resnet18 expects (B,1,F,T) features, got {tuple(x.shape)}")
        _no_cpu("ResNet18Wakeword", x)
        nat.defer_reset(x.device)              # (a previous backward pass that raised midway must not leave its queue behind)
        net = self.resnet
        net.fc_step = net.dropout_step         # one Philox step per training forward
        out = net(x.float().contiguous()[:, 0])
        if self.training and net.dropout > 0:
            net.dropout_step += 1
        return out
