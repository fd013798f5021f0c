"""DocUFCN (reference: networks/doc_ufcn/doc_ufcn.py:11-101): module tree, constructor signature and state_dict keys of the
reference, so its checkpoints load with ``strict=True``.

On a HIP device with float32 tensors the forward runs through the autograd Functions below over csrc/doc_ufcn.hip (DESIGN.md
"DocUFCN"):

* every 3x3 convolution (dilations 1 ... 16, the 3-channel input and the 3-class head included) on ``sis_dconv3x3`` -- one
  dispatch rule, ``conv_path()``; its data gradient on adjoint weights, its weight and bias gradient on ``sis_dconv3x3_wgrad`` /
  ``sis_channel_sum``;
* BatchNorm (batch statistics, ``sis_bn_stats``) + ReLU + Dropout in one pass each way (``sis_bn_drop_fwd/bwd``), dropout from the
  device counter stream (seed word advanced once per training forward, one site id per BatchNorm layer): a captured step draws
  fresh masks on every replay.  The encoder block outputs that feed a skip connection are written straight into the channel slice
  ``[C, 2C)`` of the decoder's concatenation buffer and pooled from there (``sis_max_pool2d``); the decoder's upsampled half is
  written into ``[0, C)`` -- no ``torch.cat``;
* ConvTranspose2d(k=2, s=2) = the per-pixel product on ``conv1x1_f32`` + ``sis_pixel_shuffle2`` (bias added there); nn.PixelShuffle(2)
  of the PixelShuffle variant = the same shuffle, written into the concatenation buffer.

CPU tensors and other dtypes run the reference's plain torch forward (on a HIP device through ``sis_hip.library_call``).

Differences from the reference: ``BatchNorm2d.num_batches_tracked`` is not advanced on the HIP path (it only matters for
``momentum=None``, which DocUFCN does not use).  ``min_contour_area`` keeps the reference default of 55; on a HIP
device ``BaseSegmenter.predict`` removes such contours with ``sis_hip.remove_small_contours``, which wants
square inputs up to 1024 x 1024; on CPU tensors a non-zero area raises.  Input height and width must be multiples of 8 (three poolings); on the HIP
path also (H / 8) * (W / 8) must be a multiple of 4 (the BatchNorm kernels move float4 rows of every map): any H, W that are
multiples of 16 qualify, 72 x 72 does not.
"""
from collections import OrderedDict
from typing import Type, Union

import torch
import torch.nn.functional as F
from torch import nn

from networks.base_segmenter import BaseSegmenter

_SITE_BASE = 0x0D0C0000   # dropout site ids: _SITE_BASE + index of the BatchNorm layer in module order


def conv_path(cin, cout, h, w, dilation):
    """The one dispatch rule of DocUFCN's 3x3 convolutions: every layer (any channel count, any dilation, padding = dilation) runs
    on the dilated fp32 MFMA kernel in both directions."""
    return 'dconv3x3'


def _hip_ok(x, module):
    if not x.is_cuda:
        return False
    if x.dtype == torch.float32 and all(p.dtype == torch.float32 and p.is_cuda for p in module.parameters()):
        return True
    import sis_hip
    sis_hip.library_call('doc_ufcn:dtype')
    return False


class _DConvFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, dilation):
        import sis_hip
        ctx.dilation = dilation
        ctx.has_bias = bias is not None
        ctx.save_for_backward(x, weight)
        return sis_hip.dconv3x3(x, weight, bias, dilation)

    @staticmethod
    def backward(ctx, gy):
        import sis_hip
        x, weight = ctx.saved_tensors
        dx = dw = db = None
        if ctx.needs_input_grad[0]:
            dx = sis_hip.dconv3x3(gy, sis_hip.dconv3x3_adjoint(weight), None, ctx.dilation)
        if ctx.needs_input_grad[1]:
            dw = sis_hip.dconv3x3_wgrad(gy, x, ctx.dilation)
        if ctx.has_bias and ctx.needs_input_grad[2]:
            db = sis_hip.channel_sum(gy)
        return dx, dw, db, None


class _ConvT2Fn(torch.autograd.Function):
    """ConvTranspose2d(kernel 2, stride 2, padding 0): y4 = W^T x per pixel ([Cin] -> [4 Cout], conv1x1_f32), then the shuffle."""

    @staticmethod
    def forward(ctx, x, weight, bias):
        import sis_hip
        cin, cout = weight.shape[:2]
        wm = sis_hip.transpose2d(weight.view(cin, 4 * cout)).view(4 * cout, cin, 1, 1)
        y4 = sis_hip.conv1x1_f32(x, wm)
        ctx.has_bias = bias is not None
        ctx.save_for_backward(x, wm)
        return sis_hip.pixel_shuffle2(y4, bias)

    @staticmethod
    def backward(ctx, gz):
        import sis_hip
        x, wm = ctx.saved_tensors
        cout4, cin = wm.shape[:2]
        dy4 = sis_hip.pixel_shuffle2_grad(gz)
        dx = sis_hip.conv1x1_f32(dy4, wm, data_gradient=True) if ctx.needs_input_grad[0] else None
        dw = None
        if ctx.needs_input_grad[1]:
            dwm = sis_hip.dconv3x3_wgrad(dy4, x, taps=1)
            dw = sis_hip.transpose2d(dwm.view(cout4, cin)).view(cin, cout4 // 4, 2, 2)
        db = sis_hip.channel_sum(gz) if ctx.has_bias and ctx.needs_input_grad[2] else None
        return dx, dw, db


def _bn_forward(ctx, z, gamma, beta, spec, out=None, channel_offset=0):
    """Shared forward of the BatchNorm + ReLU + Dropout Functions; spec = (bn module, dropout p, site, seed word or None)."""
    import sis_hip
    bn, p, site, seed = spec
    if bn.training:
        if bn.momentum is None:
            raise NotImplementedError("DocUFCN HIP path: BatchNorm2d(momentum=None) is not supported")
        mean, invstd = sis_hip.bn_stats(z, bn.running_mean, bn.running_var, bn.eps, bn.momentum)
        y, mask = sis_hip.bn_drop_fwd(z, mean, invstd, gamma, beta, seed=seed, site=site, drop_p=p, out=out,
                                      channel_offset=channel_offset)
    else:
        mean, invstd, mask = bn.running_mean, None, None
        y, _ = sis_hip.bn_drop_fwd(z, bn.running_mean, bn.running_var, gamma, beta, eval_mode=True, eps=bn.eps, out=out,
                                   channel_offset=channel_offset, want_mask=False)
    ctx.train_mode, ctx.p = bn.training, p
    if bn.training:
        ctx.save_for_backward(z, mean, invstd, gamma, mask)
    return y


def _bn_backward(ctx, dy, channel_offset=0, dy2=None):
    import sis_hip
    if not ctx.train_mode:
        raise NotImplementedError("DocUFCN HIP path: backward through eval-mode BatchNorm is not supported")
    z, mean, invstd, gamma, mask = ctx.saved_tensors
    return sis_hip.bn_drop_bwd(dy, z, mean, invstd, gamma, mask, ctx.p, channel_offset=channel_offset, dy2=dy2)


class _BnDropFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, z, gamma, beta, spec):
        return _bn_forward(ctx, z, gamma, beta, spec)

    @staticmethod
    def backward(ctx, dy):
        dz, dg, db = _bn_backward(ctx, dy)
        return dz, dg, db, None


class _BnDropSkipFn(torch.autograd.Function):
    """Last layer of an encoder block that feeds a skip connection -> (concatenation buffer [B, 2C, H, W] with y in channels
    [C, 2C), 2x2 max pooling of y)."""

    @staticmethod
    def forward(ctx, z, gamma, beta, spec):
        import sis_hip
        b, c, h, w = z.shape
        cat = torch.empty((b, 2 * c, h, w), dtype=z.dtype, device=z.device)
        _bn_forward(ctx, z, gamma, beta, spec, out=cat, channel_offset=c)
        pooled, ctx.argmax = sis_hip.max_pool2x2_slice(cat, c, c)
        ctx.shape = (b, c, h, w)
        return cat, pooled

    @staticmethod
    def backward(ctx, grad_cat, grad_pooled):
        import sis_hip
        b, c, h, w = ctx.shape
        dpool = None
        if grad_pooled is not None:
            dpool = sis_hip.max_pool2d_backward(grad_pooled, ctx.argmax, h, w, 2, 2, 0)
        dz, dg, db = _bn_backward(ctx, grad_cat, channel_offset=c, dy2=dpool)
        return dz, dg, db, None


class _BnDropIntoFn(torch.autograd.Function):
    """Decoder upsampling layer: y written into channels [0, C) of the concatenation buffer (modified in place, returned)."""

    @staticmethod
    def forward(ctx, z, gamma, beta, cat, spec):
        _bn_forward(ctx, z, gamma, beta, spec, out=cat, channel_offset=0)
        ctx.mark_dirty(cat)
        return cat

    @staticmethod
    def backward(ctx, grad_cat):
        dz, dg, db = _bn_backward(ctx, grad_cat, channel_offset=0)
        return dz, dg, db, grad_cat, None   # (channels [0, C) of grad_cat are not read upstream)


class _ShuffleIntoFn(torch.autograd.Function):
    """nn.PixelShuffle(2) of x [B, 4C, H, W] into channels [0, C) of the concatenation buffer (in place, returned)."""

    @staticmethod
    def forward(ctx, x, cat):
        import sis_hip
        sis_hip.pixel_shuffle2(x, None, out=cat, channel_offset=0)
        ctx.channels = x.shape[1] // 4
        ctx.mark_dirty(cat)
        return cat

    @staticmethod
    def backward(ctx, grad_cat):
        import sis_hip
        return sis_hip.pixel_shuffle2_grad(grad_cat, ctx.channels, 0), grad_cat


class DocUFCN(BaseSegmenter):

    def __init__(self, num_classes: int, input_channels: int = 3, encoder_dropout_prob: float = 0.4,
                 decoder_dropout_prob: float = 0.4, background_class_id: int = 0, min_confidence: float = 0.7,
                 min_contour_area: int = 55):
        super().__init__(background_class_id, min_confidence, min_contour_area)
        self.num_classes = num_classes
        self.num_input_channels = input_channels
        self.encoder_dropout_prob = encoder_dropout_prob
        self.decoder_dropout_prob = decoder_dropout_prob
        self.min_contour_area = min_contour_area

        self.feature_sizes = [32, 64, 128, 256]
        self.encoder_blocks = self.build_encoder(input_channels)
        self.decoder_blocks = self.build_decoder()
        self.classifier = nn.Conv2d(2 * self.feature_sizes[0], num_classes, kernel_size=3, padding=1)
        for k, bn in enumerate(m for m in self.modules() if isinstance(m, nn.BatchNorm2d)):
            bn._sis_site = _SITE_BASE + k

    def build_encoder(self, input_channels: int) -> nn.ModuleList:
        encoder_feature_sizes = [input_channels] + self.feature_sizes
        encoder_blocks = []
        for in_planes, out_planes in zip(encoder_feature_sizes, encoder_feature_sizes[1:]):
            encoder_blocks.append(self.build_encoder_conv_block(in_planes, out_planes))
        return nn.ModuleList(encoder_blocks)

    def build_decoder(self) -> nn.ModuleList:
        feature_sizes = list(reversed(self.feature_sizes))
        decoder_blocks = [self.build_decoder_conv_block(feature_sizes[0], feature_sizes[1])]
        for in_planes, out_planes in zip(feature_sizes[1:], feature_sizes[2:]):
            decoder_blocks.append(self.build_decoder_conv_block(2 * in_planes, out_planes))
        return nn.ModuleList(decoder_blocks)

    def build_conv_layer(self, in_size: int, out_size: int, dropout_prob: float, /, dilation: int = 1,
                         conv_class: Union[Type[nn.Conv2d], Type[nn.ConvTranspose2d]] = nn.Conv2d, kernel_size: int = 3,
                         stride: int = 1, padding: int = 1) -> nn.Module:
        layers = {
            "conv": conv_class(in_size, out_size, kernel_size=kernel_size, stride=stride, padding=padding, dilation=dilation),
            "bn": nn.BatchNorm2d(out_size),
            "relu": nn.ReLU(),
            "dropout": nn.Dropout(dropout_prob)
        }
        return nn.Sequential(OrderedDict(layers))

    def calc_padding(self, in_size, out_size, kernel_size, stride, dilation):
        return int(-(in_size - kernel_size - (kernel_size - 1) * (dilation - 1) - (out_size - 1) * stride) / 2)

    def build_encoder_conv_block(self, in_planes: int, out_planes: int) -> nn.Module:
        conv_layers = [self.build_conv_layer(in_planes, out_planes, self.encoder_dropout_prob, dilation=1)]
        for dilation_factor in [2, 4, 8, 16]:
            padding = self.calc_padding(out_planes, out_planes, 3, 1, dilation_factor)
            conv_layers.append(self.build_conv_layer(out_planes, out_planes, self.encoder_dropout_prob, dilation=dilation_factor,
                                                     padding=padding))
        return nn.Sequential(*conv_layers)

    def build_decoder_conv_block(self, in_planes: int, out_planes: int) -> nn.Module:
        layers = {
            "conv": self.build_conv_layer(in_planes, out_planes, self.decoder_dropout_prob),
            "upsample": self.build_conv_layer(out_planes, out_planes, self.decoder_dropout_prob, kernel_size=2, stride=2,
                                              padding=0, conv_class=nn.ConvTranspose2d)
        }
        return nn.Sequential(OrderedDict(layers))

    # ---- forward ------------------------------------------------------------------------------------------------------------
    def forward(self, x: torch.Tensor) -> torch.Tensor:
        if x.dim() != 4 or x.shape[2] % 8 or x.shape[3] % 8:
            raise ValueError(f"DocUFCN: input height and width must be multiples of 8 (three 2x2 poolings), got {tuple(x.shape)}")
        if _hip_ok(x, self):
            return self._forward_hip(x)
        return self._forward_torch(x)

    def _forward_torch(self, x):
        block_results = []
        h = self.encoder_blocks[0](x)
        for encoder_block in self.encoder_blocks[1:]:
            block_results.append(h.clone())
            h = F.max_pool2d(h, 2, stride=2)
            h = encoder_block(h)

        for decoder_block, encoder_result in zip(self.decoder_blocks, reversed(block_results)):
            h = decoder_block(h)
            h = torch.cat([h, encoder_result], dim=1)

        return self.classifier(h)

    def _spec(self, layer, seed):
        bn = layer.bn
        drop = getattr(layer, 'dropout', None)
        p = float(drop.p) if (drop is not None and self.training and drop.p > 0) else 0.0
        return bn, p, bn._sis_site, (seed if p > 0 else None)

    @staticmethod
    def _conv(conv, h):
        if conv.padding[0] != conv.dilation[0] or conv.stride[0] != 1:
            raise RuntimeError("DocUFCN HIP path: 3x3 convolutions with padding = dilation, stride 1")
        return _DConvFn.apply(h.contiguous(), conv.weight, conv.bias, conv.dilation[0])

    def _forward_hip(self, x):
        import sis_hip
        if (x.shape[2] // 8) * (x.shape[3] // 8) % 4:
            raise ValueError(f"DocUFCN on a HIP device: (H / 8) * (W / 8) must be a multiple of 4 (the BatchNorm kernels read "
                             f"float4 rows of every map), got {tuple(x.shape[2:])}; multiples of 16 qualify")
        seed = None
        if self.training and any(isinstance(m, nn.Dropout) and m.p > 0 for m in self.modules()):
            seed = sis_hip.dropout_seed(x.device)
            sis_hip.dropout_advance(seed)
        cats = []
        h = x
        n_levels = len(self.encoder_blocks)
        for level, block in enumerate(self.encoder_blocks):
            layers = list(block)
            for j, layer in enumerate(layers):
                z = self._conv(layer.conv, h)
                spec = self._spec(layer, seed)
                if j == len(layers) - 1 and level < n_levels - 1:
                    cat, h = _BnDropSkipFn.apply(z, layer.bn.weight, layer.bn.bias, spec)
                    cats.append(cat)
                else:
                    h = _BnDropFn.apply(z, layer.bn.weight, layer.bn.bias, spec)
        for decoder_block, cat in zip(self.decoder_blocks, reversed(cats)):
            layer = decoder_block.conv
            h = _BnDropFn.apply(self._conv(layer.conv, h), layer.bn.weight, layer.bn.bias, self._spec(layer, seed))
            up = decoder_block.upsample
            if isinstance(up, nn.PixelShuffle):
                h = _ShuffleIntoFn.apply(h, cat)
            else:
                z = _ConvT2Fn.apply(h, up.conv.weight, up.conv.bias)
                h = _BnDropIntoFn.apply(z, up.bn.weight, up.bn.bias, cat, self._spec(up, seed))
        return self._conv(self.classifier, h)


class DocUFCNNoDropout(DocUFCN):

    def build_conv_layer(self, in_size: int, out_size: int, dropout_prob: float, /, dilation: int = 1,
                         conv_class: Union[Type[nn.Conv2d], Type[nn.ConvTranspose2d]] = nn.Conv2d, kernel_size: int = 3,
                         stride: int = 1, padding: int = 1) -> nn.Module:
        layers = {
            "conv": conv_class(in_size, out_size, kernel_size=kernel_size, stride=stride, padding=padding, dilation=dilation),
            "bn": nn.BatchNorm2d(out_size),
            "relu": nn.ReLU()
        }
        return nn.Sequential(OrderedDict(layers))


class PixelShuffleDocUFCN(DocUFCN):

    def build_decoder_conv_block(self, in_planes: int, out_planes: int) -> nn.Module:
        layers = {
            "conv": self.build_conv_layer(in_planes, out_planes * 4, self.decoder_dropout_prob),
            "upsample": nn.PixelShuffle(2)
        }
        return nn.Sequential(OrderedDict(layers))
