"""The U-Net-like projection encoders of the reference (networks/encoder/u_net_like_encoder.py) under their names and
state_dict keys: an image goes down a ladder of residual blocks, and every block's output feeds a ``to_latent`` head (global
average pool + 1x1 convolution -> one row of the W+ latent) and / or a ``to_noise`` head (1x1 convolution to one channel ->
one of the generator's noise maps).

``BasicBlock`` restates torchvision's (torchvision is not a dependency): ``conv1, bn1, relu, conv2, bn2, downsample, stride``,
bias-free 3x3 convolutions with padding 1, so reference checkpoints load.

Two formulations, the same up to rounding:

* plain ATen (``_forward_aten``): under autograd, in training mode, on the CPU, in another dtype than float32, or with
  ``SIS_ENCODER_HIP=0``;
* the inference path on the library's kernels (``_forward_hip``: ``eval()`` + ``torch.no_grad()``, float32 on a HIP device):
  eval-mode BatchNorm folded into per-channel (scale, shift); the start block on ``sis_enc_stem``; each stride-2 block's
  conv1 + bn1 + relu and its projection shortcut on the route that measured faster (the dense Winograd convolution,
  subsampled, where its kernels take the layer; ``sis_enc_conv3x3_s2`` -- one read of the input -- elsewhere); the stride-1 3x3 layers
  on ``sis_conv3x3`` (Winograd) and ``sis_bn_act_fwd``; each block's ``relu(bn2(.) + identity)`` with its noise head and its
  pool partials on ``sis_enc_block_tail``; all latent heads of an encode in one ``sis_enc_latent_heads`` launch.  A layer
  whose shape a kernel declines runs its ATen formulation and is counted by ``sis_hip.library_call``.  Packed weights and
  folded vectors are built once and rebuilt when a parameter's or buffer's stamp (``sis_hip.weight_stamp``: storage, ``_version``,
  the counter of writes autograd cannot see) has moved.
"""
import math
import os
from typing import Dict, List, Optional

import torch
from torch import nn
from torch.nn import functional as F

import sis_hip
from latent_projecting import Latents


class BasicBlock(nn.Module):
    """torchvision.models.resnet.BasicBlock, restated: out = relu(bn2(conv2(relu(bn1(conv1(x))))) + shortcut(x))."""
    expansion = 1

    def __init__(self, inplanes: int, planes: int, stride: int = 1, downsample: Optional[nn.Module] = None):
        super().__init__()
        self.conv1 = nn.Conv2d(inplanes, planes, kernel_size=3, stride=stride, padding=1, bias=False)
        self.bn1 = nn.BatchNorm2d(planes)
        self.relu = nn.ReLU(inplace=True)
        self.conv2 = nn.Conv2d(planes, planes, kernel_size=3, stride=1, padding=1, bias=False)
        self.bn2 = nn.BatchNorm2d(planes)
        self.downsample = downsample
        self.stride = stride

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        shortcut = x if self.downsample is None else self.downsample(x)
        out = self.relu(self.bn1(self.conv1(x)))
        out = self.bn2(self.conv2(out))
        out = out + shortcut
        return self.relu(out)


def _projection(inplanes: int, planes: int, stride: int) -> nn.Sequential:
    return nn.Sequential(nn.Conv2d(inplanes, planes, kernel_size=1, stride=stride), nn.BatchNorm2d(planes))


# Which route a stride-2 layer takes: "measured" = the dispatch of DESIGN.md §13.4; "k1" = sis_enc_conv3x3_s2 wherever it takes the
# layer.  Not a switch of the product: tools/bench_encoder.py --stride2-route k1 sets it to time that kernel in the whole encoder.
STRIDE2_ROUTE = "measured"


def encoder_hip_enabled() -> bool:
    """The run-time switch of the inference path: SIS_ENCODER_HIP=0 sends the whole encoder to ATen."""
    return os.environ.get("SIS_ENCODER_HIP", "1") != "0"


class UNetLikeEncoder(nn.Module):
    """The block ladder (reference :12-68).  Subclasses choose the heads by ``build_projecting_layers`` and the class flags:
    ``latent_heads`` 'per_block' / 'last' / None, ``noise_heads``, ``sum_latents``."""
    latent_heads: Optional[str] = None
    noise_heads = False
    sum_latents = False

    def __init__(self, image_size: int, latent_size: int, num_input_channels: int, size_channel_map: dict, *,
                 target_size: int = 4, stylegan_variant: int = 2):
        super().__init__()
        self.image_size = image_size
        self.latent_size = latent_size
        self.stylegan_variant = stylegan_variant
        self.size_channel_map = size_channel_map
        self.log_input_size = int(math.log(image_size, 2))
        self.log_target_size = int(math.log(target_size, 2))
        assert image_size > target_size, "Input size must be larger than target size"
        assert 2 ** self.log_input_size == image_size, "Input size must be a power of 2"
        assert 2 ** self.log_target_size == target_size, "Target size must be a power of 2"

        top = size_channel_map[image_size]
        # registration order (and so the state_dict's) is the reference's: start_block, intermediate_block (held, never
        # called), resnet_blocks (whose entry 0 IS start_block: its tensors appear under both names), intermediate_resnet_blocks
        self.start_block = BasicBlock(num_input_channels, top, downsample=_projection(num_input_channels, top, 1))
        self.intermediate_block = BasicBlock(top, top)
        sizes = list(range(self.log_input_size, self.log_target_size - 1, -1))
        down = [BasicBlock(size_channel_map[2 ** s], size_channel_map[2 ** (s - 1)], stride=2,
                           downsample=_projection(size_channel_map[2 ** s], size_channel_map[2 ** (s - 1)], 2)) for s in sizes[:-1]]
        same = [BasicBlock(size_channel_map[2 ** s], size_channel_map[2 ** s]) for s in sizes]
        self.resnet_blocks = nn.ModuleList([self.start_block] + down)
        self.intermediate_resnet_blocks = nn.ModuleList(same)
        num_latents = (self.log_input_size - self.log_target_size) * 2 + 2
        assert len(self.resnet_blocks) + len(self.intermediate_resnet_blocks) == num_latents, \
            "The sum of all resnet blocks must be equal to the number of required latents"
        self.build_projecting_layers(self.log_input_size, self.log_target_size, size_channel_map)
        self._hip_state = self._hip_tensors = None

    def build_projecting_layers(self, log_input_size, log_target_size, size_channel_map):
        raise NotImplementedError

    def get_to_x_convs(self, input_size: int, target_size: int, target_channels: int, size_channel_map: Dict[int, int]) -> nn.ModuleList:
        return nn.ModuleList([nn.Conv2d(size_channel_map[2 ** s], target_channels, kernel_size=1, stride=1)
                              for s in range(input_size, target_size - 1, -1)])

    # ---- which head sits on which block output.  Outputs are numbered in the order they are computed: 2 i = resnet_blocks[i],
    # 2 i + 1 = intermediate_resnet_blocks[i].
    def _latent_head(self, j: int) -> Optional[nn.Conv2d]:
        if self.latent_heads == 'per_block':
            return (self.intermediate_to_latent if j % 2 else self.to_latent)[j // 2]
        if self.latent_heads == 'last' and j == 2 * len(self.resnet_blocks) - 1:
            return self.to_latent
        return None

    def _noise_head(self, j: int) -> Optional[nn.Conv2d]:
        if not self.noise_heads:
            return None
        if j % 2 == 0:
            return self.to_noise[j // 2]
        if self.stylegan_variant == 2 and j // 2 < len(self.resnet_blocks) - 1:
            return self.intermediate_to_noise[j // 2]
        return None

    def _blocks(self) -> List[BasicBlock]:
        return [blk for pair in zip(self.resnet_blocks, self.intermediate_resnet_blocks) for blk in pair]

    def _finish(self, latents: List[torch.Tensor], noises: List[torch.Tensor]) -> Latents:
        """latents: [B, latent] per head in the order computed.  The reference reverses both lists (coarse first)."""
        noise = noises[::-1] if self.noise_heads else None
        if self.latent_heads is None:
            return Latents(None, noise)
        if self.latent_heads == 'last':
            return Latents(latents[0], noise)
        stacked = torch.stack(latents[::-1], dim=1)
        return Latents(stacked.sum(dim=1) if self.sum_latents else stacked, noise)

    def forward(self, x: torch.Tensor) -> Latents:
        if self._hip_applies(x):
            return self._forward_hip(x)
        return self._forward_aten(x)

    def _forward_aten(self, x: torch.Tensor) -> Latents:
        latents, noises, h = [], [], x
        for j, block in enumerate(self._blocks()):
            h = block(h)
            head = self._latent_head(j)
            if head is not None:
                latents.append(head(F.adaptive_avg_pool2d(h, (1, 1))).flatten(1))
            head = self._noise_head(j)
            if head is not None:
                noises.append(head(h))
        return self._finish(latents, noises)

    # ------------------------------------------------------------------------------------------ the inference path
    def _hip_applies(self, x: torch.Tensor) -> bool:
        return (encoder_hip_enabled() and not self.training and not torch.is_grad_enabled() and x.is_cuda
                and x.dtype == torch.float32 and x.dim() == 4 and self.start_block.conv1.weight.dtype == torch.float32
                and self.start_block.conv1.weight.device == x.device)

    def _apply(self, fn, *args, **kwargs):
        # .to() / .float() / .double() may replace tensors: drop everything derived from them
        self._hip_state = self._hip_tensors = None
        return super()._apply(fn, *args, **kwargs)

    def _state_key(self):
        if self._hip_tensors is None:   # the module tree is walked once, not per forward
            self._hip_tensors = list(self.parameters()) + list(self.buffers())
        return tuple(sis_hip.weight_stamp(t) for t in self._hip_tensors)

    def _packs(self):
        """Per block: folded BatchNorms and the Winograd images of the stride-1 layers; rebuilt when a tensor changed.  The
        weight image of a stride-2 layer is built at the first forward that takes that route (``_stride2_image``): only
        one of the two routes ever runs on a given shape."""
        key = self._state_key()
        if self._hip_state is None or self._hip_state["key"] != key:
            packs = []
            for block in self._blocks():
                p = {"bn1": sis_hip.fold_batch_norm(block.bn1), "bn2": sis_hip.fold_batch_norm(block.bn2), "u1": None, "u2": None, "s2": None}
                p["invstd1"] = torch.rsqrt(block.bn1.running_var.detach() + block.bn1.eps)
                if block.downsample is not None:
                    p["bnd"] = sis_hip.fold_batch_norm(block.downsample[1], block.downsample[0].bias if block.stride == 2 else None)
                cin, cout = block.conv1.in_channels, block.conv1.out_channels
                if block.stride == 1 and cin % 8 == 0 and cout % 8 == 0:
                    p["u1"] = sis_hip.conv3x3_prepack(block.conv1.weight.detach())
                if block.stride == 2:
                    p["ident"] = (torch.zeros_like(p["bnd"][0]), torch.ones_like(p["bnd"][0]))
                if cout % 8 == 0:
                    p["u2"] = sis_hip.conv3x3_prepack(block.conv2.weight.detach())
                packs.append(p)
            self._hip_state = {"key": key, "packs": packs, "heads": (None, None)}   # heads: the last (batch, H, W) and its table
        return self._hip_state

    @staticmethod
    def _conv3x3(x, conv, u, site):
        if u is not None and sis_hip.conv3x3_supported(x, conv.weight):
            return sis_hip.conv3x3(x, u)
        sis_hip.library_call(site)
        return F.conv2d(x, conv.weight, None, 1, 1)

    @staticmethod
    def _stride2_image(block, p, which):
        """The Winograd image ("u1") or the sis_enc_conv3x3_s2 image ("s2") of a stride-2 block's conv1, built at first use."""
        if p[which] is None:
            p[which] = sis_hip.conv3x3_prepack(block.conv1.weight.detach()) if which == "u1" else \
                sis_hip.enc_conv3x3_s2_pack(block.conv1.weight.detach(), block.downsample[0].weight.detach())
        return p[which]

    @staticmethod
    def _conv1_stride2_dense(h, block, p):
        """Dispatch by measurement: on every stride-2 layer of Generator(256)'s map the dense stride-1 Winograd
        convolution, subsampled, with the shortcut as subsample + sis_conv1x1_f32, took less time than sis_enc_conv3x3_s2
        (1.06x at 256 x 256, B = 8; up to 10x on the small maps, where that kernel has a handful of workgroups).  So this route
        runs wherever its kernels take the layer (channels % 32 == 0 among others) and sis_enc_conv3x3_s2 takes the rest.
        -> (relu(bn1(conv1(h))), bn_d(conv_d(h))) or None."""
        if STRIDE2_ROUTE == "k1" or h.shape[2] % 2 or h.shape[3] % 2 or not sis_hip.conv3x3_supported(h, block.conv1.weight):
            return None
        hs = h[:, :, ::2, ::2].contiguous()
        wd = block.downsample[0].weight.detach()
        if not (sis_hip.conv1x1_f32_supported(hs, wd) and sis_hip.bn_supported(hs)):
            return None
        bn = block.bn1
        sub = sis_hip.conv3x3(h, UNetLikeEncoder._stride2_image(block, p, "u1"))[:, :, ::2, ::2].contiguous()
        a = sis_hip.bn_act_fwd(sub, None, bn.running_mean, p["invstd1"], bn.weight.detach(), bn.bias.detach(), True)
        zero, one = p["ident"]
        shortcut = sis_hip.bn_act_fwd(sis_hip.conv1x1_f32(hs, wd), None, zero, one, p["bnd"][0], p["bnd"][1], False)
        return a, shortcut

    @staticmethod
    def _affine_relu(c, fold, residual=None):
        scale, shift = fold
        out = c * scale.view(1, -1, 1, 1) + shift.view(1, -1, 1, 1)
        return torch.relu(out if residual is None else out + residual)

    def _forward_hip(self, x: torch.Tensor) -> Latents:
        state = self._packs()
        x = x.contiguous()
        batch = x.shape[0]
        heads_key = (batch, x.shape[2], x.shape[3])
        head_state = state["heads"][1] if state["heads"][0] == heads_key else None
        blocks = self._blocks()
        n_out = len(blocks)
        latent_js = [j for j in range(n_out) if self._latent_head(j) is not None]
        noises, fallback_latents, pool_bufs = [], {}, {}
        h = x
        for j, (block, p) in enumerate(zip(blocks, state["packs"])):
            cin, cout, (hh, ww) = block.conv1.in_channels, block.conv1.out_channels, h.shape[2:]
            # ---- conv1 + bn1 + relu, and the shortcut
            if block.stride == 2:
                dense = self._conv1_stride2_dense(h, block, p)
                if dense is not None:
                    a, shortcut = dense
                elif sis_hip.enc_conv3x3_s2_supported(cin, cout, hh, ww):
                    a, shortcut = sis_hip.enc_conv3x3_s2(h, self._stride2_image(block, p, "s2"), cout, *p["bn1"], *p["bnd"])
                else:
                    sis_hip.library_call("encoder.conv3x3_s2")
                    a = self._affine_relu(F.conv2d(h, block.conv1.weight, None, 2, 1), p["bn1"])
                    shortcut = F.conv2d(h, block.downsample[0].weight, None, 2) * p["bnd"][0].view(1, -1, 1, 1) + p["bnd"][1].view(1, -1, 1, 1)
            elif block.downsample is not None:
                if sis_hip.enc_stem_supported(cin, cout, hh, ww):
                    a, shortcut = sis_hip.enc_stem(h, block.conv1.weight.detach(), *p["bn1"], block.downsample[0].weight.detach(),
                                                   block.downsample[0].bias.detach() if block.downsample[0].bias is not None else None, *p["bnd"])
                else:
                    sis_hip.library_call("encoder.stem")
                    a = self._affine_relu(F.conv2d(h, block.conv1.weight, None, 1, 1), p["bn1"])
                    shortcut = F.conv2d(h, block.downsample[0].weight, block.downsample[0].bias) * p["bnd"][0].view(1, -1, 1, 1) \
                        + p["bnd"][1].view(1, -1, 1, 1)
            else:
                c1 = self._conv3x3(h, block.conv1, p["u1"], "encoder.conv3x3")
                if sis_hip.bn_supported(c1):
                    bn = block.bn1
                    a = sis_hip.bn_act_fwd(c1, None, bn.running_mean, p["invstd1"], bn.weight.detach(), bn.bias.detach(), True)
                else:
                    sis_hip.library_call("encoder.bn_act")
                    a = self._affine_relu(c1, p["bn1"])
                shortcut = h
            # ---- conv2, then relu(bn2(.) + shortcut) with the heads
            c2 = self._conv3x3(a, block.conv2, p["u2"], "encoder.conv3x3")
            noise_head, latent_head = self._noise_head(j), self._latent_head(j)
            hw = c2.shape[2] * c2.shape[3]
            if sis_hip.enc_block_tail_supported(cout, hw):
                pool_out = None
                if latent_head is not None:
                    pool_out = head_state["partials"][j] if head_state is not None else \
                        torch.empty((batch, cout, sis_hip.enc_block_tail_tiles(hw)), dtype=torch.float32, device=x.device)
                    pool_bufs[j] = (pool_out, hw)
                h, noise, _ = sis_hip.enc_block_tail(c2, shortcut, *p["bn2"],
                                                     noise_head.weight.detach() if noise_head is not None else None,
                                                     noise_head.bias.detach() if noise_head is not None else None,
                                                     want_pool=latent_head is not None, pool_out=pool_out)
            else:
                sis_hip.library_call("encoder.block_tail")
                h = self._affine_relu(c2, p["bn2"], shortcut)
                noise = noise_head(h) if noise_head is not None else None
                if latent_head is not None:
                    fallback_latents[j] = latent_head(F.adaptive_avg_pool2d(h, (1, 1))).flatten(1)
            if noise is not None:
                noises.append(noise)
        # ---- the latent heads: one launch through a pointer table
        latents = None
        if latent_js:
            max_c = max(blocks[j].conv1.out_channels for j in latent_js)
            if not fallback_latents and sis_hip.lib().sis_enc_latent_heads_supported(max_c, self.latent_size):
                if head_state is None:
                    n = len(latent_js)
                    # slot = position after the reference's reverse(); the summed forms add the heads in that order
                    rows = [(pool_bufs[j][0], pool_bufs[j][1], self._latent_head(j).weight.detach(), self._latent_head(j).bias.detach(), n - 1 - i)
                            for i, j in enumerate(latent_js)]
                    rows.sort(key=lambda r: r[4])
                    head_state = {"partials": {j: pool_bufs[j][0] for j in latent_js}, "table": sis_hip.enc_heads_table(rows, x.device)}
                    state["heads"] = (heads_key, head_state)   # one shape is kept: another batch or image size replaces it
                out = sis_hip.enc_latent_heads(head_state["table"], len(latent_js), sum_heads=self.sum_latents)
                noise = noises[::-1] if self.noise_heads else None
                if self.latent_heads == 'last':
                    return Latents(out.view(batch, self.latent_size), noise)
                return Latents(out, noise)
            sis_hip.library_call("encoder.latent_heads")
            latents = []
            for j in latent_js:
                if j in fallback_latents:
                    latents.append(fallback_latents[j])
                else:
                    partial, hw = pool_bufs[j]
                    pooled = (partial.sum(dim=2) / hw).view(batch, -1, 1, 1)
                    latents.append(self._latent_head(j)(pooled).flatten(1))
        return self._finish(latents or [], noises)


class WPlusEncoder(UNetLikeEncoder):
    """One latent row and (variant 2) one noise map per block output (reference :84-114)."""
    latent_heads = 'per_block'
    noise_heads = True

    def build_projecting_layers(self, log_input_size, log_target_size, size_channel_map):
        self.to_latent = self.get_to_x_convs(log_input_size, log_target_size, self.latent_size, size_channel_map)
        self.intermediate_to_latent = self.get_to_x_convs(log_input_size, log_target_size, self.latent_size, size_channel_map)
        self.to_noise = self.get_to_x_convs(log_input_size, log_target_size, 1, size_channel_map)
        if self.stylegan_variant == 2:
            self.intermediate_to_noise = self.get_to_x_convs(log_input_size, log_target_size, 1, size_channel_map)


class WWPlusEncoder(WPlusEncoder):
    """W+ rows summed into one W latent (reference :171-176)."""
    sum_latents = True


class WEncoder(UNetLikeEncoder):
    """One W latent from the last block's pooled map, plus the noise maps (reference :141-168)."""
    latent_heads = 'last'
    noise_heads = True

    def build_projecting_layers(self, log_input_size, log_target_size, size_channel_map):
        self.to_latent = nn.Conv2d(self.latent_size, self.latent_size, kernel_size=1, stride=1)
        self.to_noise = self.get_to_x_convs(log_input_size, log_target_size, 1, size_channel_map)
        if self.stylegan_variant == 2:
            self.intermediate_to_noise = self.get_to_x_convs(log_input_size, log_target_size, 1, size_channel_map)


class WPlusNoNoiseEncoder(UNetLikeEncoder):
    """W+ latents only (reference :213-233): the latent stem of the two-stem autoencoder."""
    latent_heads = 'per_block'

    def build_projecting_layers(self, log_input_size, log_target_size, size_channel_map):
        self.to_latent = self.get_to_x_convs(log_input_size, log_target_size, self.latent_size, size_channel_map)
        self.intermediate_to_latent = self.get_to_x_convs(log_input_size, log_target_size, self.latent_size, size_channel_map)


class WNoNoiseEncoder(WPlusNoNoiseEncoder):
    """The rows of WPlusNoNoiseEncoder summed (reference :236-241)."""
    sum_latents = True


class NoiseEncoder(UNetLikeEncoder):
    """Noise maps only (reference :244-264): the noise stem of the two-stem autoencoder."""
    noise_heads = True

    def build_projecting_layers(self, log_input_size, log_target_size, size_channel_map):
        self.to_noise = self.get_to_x_convs(log_input_size, log_target_size, 1, size_channel_map)
        if self.stylegan_variant == 2:
            self.intermediate_to_noise = self.get_to_x_convs(log_input_size, log_target_size, 1, size_channel_map)


class WPlusResnetNoiseEncoder(WPlusEncoder):
    """Reference :117-138 (noise heads that are residual blocks to one channel): reachable only from the StyleGAN1 factories."""

    def __init__(self, *args, **kwargs):
        raise NotImplementedError("WPlusResnetNoiseEncoder belongs to the StyleGAN1 autoencoders, which are not on the MI355X path "
                                  "(networks.get_autoencoder raises for stylegan_variant 1)")


class WCodeEncoder(WEncoder):
    """Reference :179-210 (an extra info code): reachable only with code_dim > 0, which the reference implements for StyleGAN1 alone."""

    def __init__(self, *args, **kwargs):
        raise NotImplementedError("WCodeEncoder needs the StyleGAN1 code autoencoder (the reference raises for code_dim > 0 with "
                                  "StyleGAN2); CodeLatents are not part of this port")
