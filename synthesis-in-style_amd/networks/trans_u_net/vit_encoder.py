"""ViT encoder of TransUNet: patch / position embeddings (optionally on top of the ResNetV2 stem), pre-norm
transformer blocks, final LayerNorm.  Class names, constructor signatures and parameter names follow
/root/reference/stylegan_code_finder/networks/trans_u_net/vit_seg_modeling.py:53-262 so checkpoints line up.

Product path (HIP device, bf16 autocast, ``SIS_FUSED_VIT=1``): every transformer block is ONE autograd function,
``_FusedBlockFn`` below -- own bf16 GEMMs with fused bias / GELU / dropout / residual epilogues (csrc/gemm_bf16.hip), own
fused attention (csrc/attention_bf16.hip: online softmax, no [B,12,N,N] score tensor in HBM; the reference's attention
dropout rate is 0.0, so it is the same function), own LayerNorm.  The module-by-module forward further down
(``Attention.forward`` with ``F.scaled_dot_product_attention`` / ``torch.matmul``, ``Mlp.forward``) is what runs when the
fused block declines -- fp32 (no autocast), ``vis`` attention maps, CPU tensors -- and every such use on a HIP device is
counted by ``sis_hip.library_call`` (bench.py reports the counter and fails on it for the bf16 BASELINE config).
"""
import copy
import math
import os

import torch
import torch.nn as nn
import torch.nn.functional as F
from torch.autograd import Function
from torch.nn import Dropout, Linear, Softmax

import sis_hip
from torch.nn.modules.utils import _pair

from networks.hip_conv import HipConv2d

from .vit_seg_modeling_resnet_skip import ResNetV2


def swish(x):
    return x * torch.sigmoid(x)


ACT2FN = {"gelu": F.gelu, "relu": F.relu, "swish": swish}


_HIP_LN = os.environ.get('SIS_HIP_LN', '1') != '0'


class _LayerNormFn(Function):
    @staticmethod
    def forward(ctx, x, weight, bias, eps, out_dtype):
        y, mean, rstd = sis_hip.layer_norm_fwd(x, weight, bias, eps, out_dtype)
        ctx.save_for_backward(x, mean, rstd, weight)
        return y

    @staticmethod
    def backward(ctx, grad):
        x, mean, rstd, weight = ctx.saved_tensors
        dx, dgamma, dbeta = sis_hip.layer_norm_bwd(grad, x, mean, rstd, weight)
        return dx, dgamma, dbeta, None, None


class _AmpLinearFn(Function):
    """``F.linear`` under 16-bit autocast with the backward issued explicitly: dW as one 16-bit x 16-bit -> float32 GEMM
    (autocast would round it to 16 bits and cast it back for the fp32 master weight), d(bias) by the column-sum kernel
    (csrc/column_sum.hip, float32) instead of a generic reduction + cast."""

    @staticmethod
    def forward(ctx, x, weight, bias):
        w_lp, b_lp = weight.to(x.dtype), bias.to(x.dtype)
        x2 = x.reshape(-1, x.shape[-1])
        ctx.save_for_backward(x2, w_lp)
        ctx.x_shape = x.shape
        return torch.addmm(b_lp, x2, w_lp.t()).view(*x.shape[:-1], weight.shape[0])

    @staticmethod
    def backward(ctx, grad):
        x2, w_lp = ctx.saved_tensors
        g2 = grad.reshape(-1, grad.shape[-1])
        if g2.dtype != x2.dtype:
            g2 = g2.to(x2.dtype)
        g2 = g2.contiguous()
        dx = dw = db = None
        if ctx.needs_input_grad[0]:
            dx = torch.mm(g2, w_lp).view(ctx.x_shape)
        if ctx.needs_input_grad[1]:
            dw = torch.mm(g2.t(), x2, out_dtype=torch.float32)
        if ctx.needs_input_grad[2]:
            db = sis_hip.column_sum(g2)
        return dx, dw, db


_AMP_LINEAR = os.environ.get('SIS_AMP_LINEAR', '1') != '0'
_SHADOW = os.environ.get('SIS_LINEAR_SHADOW', '1') != '0'  # 0: cast (and concatenate) the fp32 weights every forward


class _Bf16Shadow:
    """bfloat16 copy of one or several fp32 parameters concatenated along dim 0 (query | key | value of an attention
    block: ONE [3 hidden, hidden] GEMM operand without a per-forward ``torch.cat`` + cast).

    Who keeps it current: ``FusedSGD`` when the copy is registered there (``bind``): the optimizer launch that updates the
    fp32 master weights writes the rounded values into the copy as well.  Otherwise (plain ``torch.optim`` steps,
    ``load_state_dict``, a FusedSGD the copy was never registered with) the copy is refreshed here whenever a parameter's
    stamp (``sis_hip.weight_stamp``: ``_version``, or the raw-update counter the fused optimizers bump, since their kernel writes
    bypass ``_version``) has moved."""

    def __init__(self, params):
        self.params = list(params)
        self.buf = None
        self.key = None
        self.bound = None  # the buffer object FusedSGD writes into

    def _key(self):
        if self.bound is not None and self.bound is self.buf:
            return tuple(sis_hip.weight_stamp(p, raw=False) for p in self.params)  # raw optimizer updates are mirrored into the copy by the optimizer
        return tuple(sis_hip.weight_stamp(p) for p in self.params)

    def tensor(self):
        first = self.params[0]
        if self.buf is None or self.buf.device != first.device:
            rows = sum(p.shape[0] for p in self.params)
            self.buf = torch.empty((rows,) + tuple(first.shape[1:]), dtype=torch.bfloat16, device=first.device)
            self.key = None
        key = self._key()
        # While a stream is being captured into a hipGraph, a copy nobody else keeps current is ALWAYS refreshed: the cast then
        # becomes part of the graph and every replay re-derives it from the master weights (a replayed optimizer launch moves
        # the weights without touching ``_version`` or the Python-side counter, so a key match at capture time proves nothing).
        capturing = first.is_cuda and torch.cuda.is_current_stream_capturing() and not (self.bound is not None and self.bound is self.buf)
        if key != self.key or capturing:
            with torch.no_grad():
                row = 0
                for p in self.params:
                    self.buf[row:row + p.shape[0]].copy_(p)
                    row += p.shape[0]
            self.key = key
        return self.buf

    def bind(self, optimizer):
        buf = self.tensor()
        row = 0
        for p in self.params:
            optimizer.register_shadow(p, buf[row:row + p.shape[0]])
            row += p.shape[0]
        self.bound = buf
        self.key = self._key()


class _ShadowLinearFn(Function):
    """y = x W^T + b with W / b taken from bf16 shadow copies (``_Bf16Shadow``) of ``n`` fp32 weights / biases stacked
    along the output axis; the gradients go to the fp32 parameters: dW as ONE bf16 x bf16 -> float32 GEMM, split by rows
    (views, no copies), d(bias) by the column-sum kernel."""

    @staticmethod
    def forward(ctx, x, w_lp, b_lp, n, *params):
        x2 = x.reshape(-1, x.shape[-1])
        ctx.save_for_backward(x2, w_lp)
        ctx.x_shape, ctx.n = x.shape, n
        ctx.rows = [p.shape[0] for p in params[:n]]
        return torch.addmm(b_lp, x2, w_lp.t()).view(*x.shape[:-1], w_lp.shape[0])

    @staticmethod
    def backward(ctx, grad):
        x2, w_lp = ctx.saved_tensors
        g2 = grad.reshape(-1, grad.shape[-1])
        if g2.dtype != x2.dtype:
            g2 = g2.to(x2.dtype)
        g2 = g2.contiguous()
        dx = torch.mm(g2, w_lp).view(ctx.x_shape) if ctx.needs_input_grad[0] else None
        dws = dbs = [None] * ctx.n
        if any(ctx.needs_input_grad[4:4 + ctx.n]):
            dws = list(torch.mm(g2.t(), x2, out_dtype=torch.float32).split(ctx.rows, 0))
        if any(ctx.needs_input_grad[4 + ctx.n:]):
            dbs = list(sis_hip.column_sum(g2).split(ctx.rows, 0))
        return (dx, None, None, None, *dws, *dbs)


def shadow_linear(x, w_shadow, b_shadow, weights, biases):
    """``linear`` over stacked parameters through their bf16 shadows; None when the fast path does not apply."""
    if not (_SHADOW and _AMP_LINEAR and x.is_cuda and torch.is_autocast_enabled() and x.dtype == torch.bfloat16
            and torch.get_autocast_dtype('cuda') == torch.bfloat16 and x.is_contiguous()
            and all(w.dtype == torch.float32 and w.is_cuda for w in weights) and sum(w.shape[0] for w in weights) % 4 == 0):
        return None
    return _ShadowLinearFn.apply(x, w_shadow.tensor(), b_shadow.tensor(), len(weights), *weights, *biases)


def linear(x, weight, bias):
    """``F.linear``; on a HIP device under 16-bit autocast with a 16-bit input, the explicit-backward variant above."""
    if (_AMP_LINEAR and bias is not None and x.is_cuda and torch.is_autocast_enabled() and x.dtype in (torch.bfloat16, torch.float16)
            and x.dtype == torch.get_autocast_dtype('cuda') and weight.dtype == torch.float32 and weight.shape[0] % 4 == 0
            and x.is_contiguous()):
        return _AmpLinearFn.apply(x, weight, bias)
    if x.is_cuda:
        sis_hip.library_call("vit_encoder.linear")
    return F.linear(x, weight, bias)


class LayerNorm(nn.LayerNorm):
    """``nn.LayerNorm`` on one HIP launch per direction (csrc/layer_norm.hip: a wave per token, the row held in
    registers); under autocast the result is written in the autocast dtype, i.e. what the following Linear reads."""

    def forward(self, x):
        n = self.normalized_shape[-1]
        if len(self.normalized_shape) == 1 and self.elementwise_affine and self.bias is not None \
                and _HIP_LN and sis_hip.layer_norm_supported(x, n):
            out_dtype = torch.get_autocast_dtype('cuda') if torch.is_autocast_enabled() else x.dtype
            if out_dtype in (torch.float32, torch.bfloat16):
                return _LayerNormFn.apply(x, self.weight, self.bias, self.eps, out_dtype)
        if x.is_cuda:
            sis_hip.library_call("vit_encoder.LayerNorm")
        return super().forward(x)


class Attention(nn.Module):
    def __init__(self, config, vis):
        super().__init__()
        self.vis = vis
        self.num_attention_heads = config.transformer["num_heads"]
        self.attention_head_size = int(config.hidden_size / self.num_attention_heads)
        self.all_head_size = self.num_attention_heads * self.attention_head_size
        self.query = Linear(config.hidden_size, self.all_head_size)
        self.key = Linear(config.hidden_size, self.all_head_size)
        self.value = Linear(config.hidden_size, self.all_head_size)
        self.out = Linear(config.hidden_size, config.hidden_size)
        self.attn_dropout = Dropout(config.transformer["attention_dropout_rate"])
        self.proj_dropout = Dropout(config.transformer["attention_dropout_rate"])
        self.softmax = Softmax(dim=-1)
        self._lp = None  # bf16 shadows of (query | key | value) and out, built on first use (not part of the state_dict)

    def grad_fusion_groups(self):
        """Parameters whose gradients ONE kernel produces as one stacked tensor (the fused query | key | value weight-gradient
        GEMM): the data-parallel wrap lays their bucket slices out back to back in this order, so that the GEMM can write
        straight into the bucket (training/grad_exchange.py, sis_hip.grad_out_fused)."""
        return [(self.query.weight, self.key.weight, self.value.weight)]

    def _shadows(self):
        if self._lp is None or self._lp[0].params[0] is not self.query.weight:
            self._lp = (_Bf16Shadow([self.query.weight, self.key.weight, self.value.weight]),
                        _Bf16Shadow([self.query.bias, self.key.bias, self.value.bias]),
                        _Bf16Shadow([self.out.weight]), _Bf16Shadow([self.out.bias]))
        return self._lp

    def register_weight_shadows(self, optimizer):
        """Called by the train builder: the fused optimizer keeps the bf16 copies current from now on."""
        if _SHADOW and self.query.weight.is_cuda:
            for sh in self._shadows():
                sh.bind(optimizer)

    def __deepcopy__(self, memo):  # the encoder deep-copies a prototype block: copies must not share shadow objects
        lp, self._lp = self._lp, None
        try:
            cls = self.__class__
            new = cls.__new__(cls)
            memo[id(self)] = new
            for k, v in self.__dict__.items():
                setattr(new, k, copy.deepcopy(v, memo))
            return new
        finally:
            self._lp = lp

    def transpose_for_scores(self, x):
        b, n, _ = x.shape
        return x.view(b, n, self.num_attention_heads, self.attention_head_size).permute(0, 2, 1, 3)

    def forward(self, hidden_states):
        # one [hidden -> 3 * hidden] GEMM instead of three (the parameters stay separate, as in the reference's
        # checkpoints): 8192 x 768 x 768 products run the bf16 matrix cores at ~7 % of peak, the fused one is 3x larger
        lp = self._shadows()
        qkv = shadow_linear(hidden_states, lp[0], lp[1], [self.query.weight, self.key.weight, self.value.weight],
                            [self.query.bias, self.key.bias, self.value.bias])
        if qkv is None:
            qkv = linear(hidden_states, torch.cat([self.query.weight, self.key.weight, self.value.weight], 0),
                         torch.cat([self.query.bias, self.key.bias, self.value.bias], 0))
        q, k, v = (self.transpose_for_scores(t) for t in qkv.split(self.all_head_size, dim=-1))
        weights = None
        if hidden_states.is_cuda:
            sis_hip.library_call("vit_encoder.Attention (module-by-module block)")
        if self.vis or (self.training and self.attn_dropout.p > 0):
            scores = torch.matmul(q, k.transpose(-1, -2)) / math.sqrt(self.attention_head_size)
            probs = self.softmax(scores)
            weights = probs if self.vis else None
            context = torch.matmul(self.attn_dropout(probs), v)
        else:
            context = F.scaled_dot_product_attention(q, k, v)
        b, _, n, _ = context.shape
        context = context.permute(0, 2, 1, 3).reshape(b, n, self.all_head_size)
        out = shadow_linear(context, lp[2], lp[3], [self.out.weight], [self.out.bias])
        if out is None:
            out = linear(context, self.out.weight, self.out.bias)
        return self.proj_dropout(out), weights


class Mlp(nn.Module):
    def __init__(self, config):
        super().__init__()
        self.fc1 = Linear(config.hidden_size, config.transformer["mlp_dim"])
        self.fc2 = Linear(config.transformer["mlp_dim"], config.hidden_size)
        self.act_fn = ACT2FN["gelu"]
        self.dropout = Dropout(config.transformer["dropout_rate"])
        for fc in (self.fc1, self.fc2):
            nn.init.xavier_uniform_(fc.weight)
            nn.init.normal_(fc.bias, std=1e-6)
        self._lp = None

    def _shadows(self):
        if self._lp is None or self._lp[0].params[0] is not self.fc1.weight:
            self._lp = tuple(_Bf16Shadow([t]) for t in (self.fc1.weight, self.fc1.bias, self.fc2.weight, self.fc2.bias))
        return self._lp

    def register_weight_shadows(self, optimizer):
        if _SHADOW and self.fc1.weight.is_cuda:
            for sh in self._shadows():
                sh.bind(optimizer)

    __deepcopy__ = Attention.__deepcopy__

    def _fc(self, x, i, fc):
        lp = self._shadows()
        y = shadow_linear(x, lp[2 * i], lp[2 * i + 1], [fc.weight], [fc.bias])
        return y if y is not None else linear(x, fc.weight, fc.bias)

    def forward(self, x):
        hidden = self.dropout(self.act_fn(self._fc(x, 0, self.fc1)))
        return self.dropout(self._fc(hidden, 1, self.fc2))


_FUSED_BLOCK = os.environ.get('SIS_FUSED_VIT', '1') != '0'  # 0: the module-by-module path (library GEMMs / attention)
_GEMM256 = os.environ.get('SIS_GEMM256', '1') != '0'       # 0: forward / data-gradient GEMMs on the 128-wide tiles only (A/B runs)
# 1: data gradients as NT products on transposed weight shadows (one multi-tensor transpose per step) wherever a 256-row tile is
# enabled for the shape.  Off: with the shipped tile set (256 x 288 only) no data gradient would take that path -- their
# outputs are 768 / 3072 wide -- and the NN layout of csrc/gemm_bf16.hip measured faster on them (tools/bench_gemm256.py).
_GEMM256_DGRAD = os.environ.get('SIS_GEMM256_DGRAD', '0') == '1'


def _wgrad_plan(out_features, in_features):
    """(K slices, tile code) of a weight-gradient GEMM (contraction over the tokens), from tools/bench_gemm.py on MI355X at
    8 192 tokens: enough 128 x 128 tiles x slices to fill the 256 CUs about twice; the 3072-wide MLP weights run faster on the
    32-deep, 3-stage tile (three workgroups per CU) with 4 slices (68 vs 77-80 us)."""
    tiles = ((out_features + 127) // 128) * ((in_features + 127) // 128)
    if tiles >= 128:
        return 4, 4
    splits = 1
    while splits < 8 and tiles * splits * 2 <= 512:
        splits *= 2
    return splits, 0


_FUSE_BLOCK_CAST = os.environ.get('SIS_FUSE_BLOCK_CAST', '1') != '0'   # 0: every block casts its own output gradient (A/B runs)
_FUSE_BIAS_GRAD = os.environ.get('SIS_FUSE_BIAS_GRAD', '1') != '0'   # 0: bias gradients as column-sum launches of their own (A/B runs)
_WGRAD_STREAMS = {}  # device -> side stream of the weight-gradient GEMMs (process-wide, like the generator's ToRGB stream)
_WGRAD_SIDE = int(os.environ.get('SIS_WGRAD_STREAM', '0'))   # 1: weight-gradient GEMMs + column sums on a side stream (measured 273 vs 277 images/s: off); 2: column sums only


def _wgrad_stream(device):
    if not _WGRAD_SIDE:
        return None
    st = _WGRAD_STREAMS.get(device)
    if st is None:
        st = _WGRAD_STREAMS[device] = sis_hip.side_stream(device)
    return st


class _SideWgrads:
    """Weight / bias gradients of a block's Linear layers on a side stream: they depend on the backward's activations'
    gradients but nothing in the block's backward depends on them, so they fill the compute units the data-gradient GEMMs,
    the attention backward and the LayerNorm kernels leave idle (tile-count tails of 8 192-token GEMMs on 256 CUs).  The main
    stream joins once, before the gradients are handed to autograd.  Under hipGraph capture the fork / join become graph
    edges."""

    def __init__(self, device):
        self.main = torch.cuda.current_stream(device)
        self.side = _wgrad_stream(device)
        self.outputs = []

    def run(self, grad, inp, out_features, in_features, keys=None, defer=False):
        """(dW fp32 [out, in], db fp32 [out]) of y = inp W^T + b from grad = dL/dy (bf16 [tokens, out]), inp bf16 [tokens, in].
        ``keys``: storage addresses of the weight parameter(s) dW is the gradient of -- under the data-parallel wrap the GEMM
        writes into their bucket slice (``sis_hip.grad_out_fused``; several parameters: query | key | value, stacked)."""
        S = sis_hip
        splits, tile = _wgrad_plan(out_features, in_features)
        out = None
        if keys:
            rows = [out_features // len(keys)] * len(keys)
            out = S.grad_out_fused(keys, rows, in_features, grad.device)
        if self.side is None:
            if defer:   # into the batched launch at the end of the backward (sis_hip.defer_wgrad_bias): results valid after the flush
                queued = S.defer_wgrad_bias(grad, inp, dw=out)
                if queued is not None:
                    return queued
            if _FUSE_BIAS_GRAD and splits > 1 and tile in (0, 4, 5, 6) and grad.shape[0] >= 64 * splits:   # (fewer tokens: the GEMM drops its split)
                # the bias column sums ride in the weight-gradient launches (extra workgroups in the idle slots of the last round)
                return S.gemm_bf16_wgrad_bias(grad, inp, splits, tile, dw=out)
            return S.gemm_bf16(grad, inp, S.GEMM_TN, S.EPI_F32, splits=splits, tile=tile, out=out), S.column_sum(grad)
        self.side.wait_event(self.main.record_event())   # grad (and inp) are complete on the main stream
        grad.record_stream(self.side)
        if _WGRAD_SIDE == 2:   # only the small column-sum kernels leave the main stream
            dw = S.gemm_bf16(grad, inp, S.GEMM_TN, S.EPI_F32, splits=splits, tile=tile, out=out)
            with torch.cuda.stream(self.side):
                db = S.column_sum(grad)
            self.outputs += [db]
            return dw, db
        inp.record_stream(self.side)
        with torch.cuda.stream(self.side):
            dw = S.gemm_bf16(grad, inp, S.GEMM_TN, S.EPI_F32, splits=splits, tile=tile, out=out)
            db = S.column_sum(grad)
        self.outputs += [dw, db]
        return dw, db

    def join(self):
        if self.side is not None and self.outputs:
            self.main.wait_event(self.side.record_event())
            for t in self.outputs:
                t.record_stream(self.main)   # allocated on the side stream, consumed (optimizer, all-reduce) on the main one


class _FusedBlockFn(Function):
    """One pre-norm transformer block (reference: Block.forward, vit_seg_modeling.py:181-189, with Attention.forward :76-96
    and Mlp.forward :116-122) as seven launches forward and their hand-written backward:

        h1 = LN1(x)                     csrc/layer_norm.hip          (bf16 out)
        qkv = h1 Wqkv^T + b             gemm NT, bias epilogue       (query | key | value in one product)
        ctx = softmax(q k^T / 8) v      csrc/attention_bf16.hip      (reads qkv in place, writes [B, N, hidden])
        x2 = x + dropout(ctx Wo^T + b)  gemm NT, bias + dropout + residual epilogue (fp32 residual stream)
        h2 = LN2(x2)
        a = dropout(gelu(h2 W1^T + b))  gemm NT, bias + GELU + dropout epilogue (pre-activation kept for the backward)
        x3 = x2 + dropout(a W2^T + b)   gemm NT, bias + dropout + residual epilogue

    Dropout masks are functions of (step seed word, site id, element index): nothing is stored, the backward recomputes
    them in its epilogues (csrc/vit_common.h).  Weight gradients are fp32 (bf16 x bf16 products, fp32 sums, split over the
    tokens with an ordered reduction); bias gradients are column sums (csrc/column_sum.hip)."""

    @staticmethod
    def forward(ctx, x, cfg, wqkv, wo, w1, w2, ln1_w, ln1_b, q_w, k_w, v_w, q_b, k_b, v_b, o_w, o_b, ln2_w, ln2_b,
                f1_w, f1_b, f2_w, f2_b, wqkv_t=None, wo_t=None, w1_t=None, w2_t=None):
        S = sis_hip
        heads, eps, p_proj, p_mlp, site, seed = cfg
        b, n, hid = x.shape
        m = b * n
        mlp = w1.shape[0]
        x2d = x.reshape(m, hid)
        h1, mean1, rstd1 = S.layer_norm_fwd(x2d, ln1_w, ln1_b, eps, torch.bfloat16)
        # Tiles.  With >= ~200 of them (8 192 tokens) the 256-row tiles of csrc/gemm256_bf16.hip: 256 x 288 for the fused
        # projection (256 tiles = one round of the chip), 256 x 96 for the 768-wide outputs (256 tiles), 256 x 192 for fc1
        # (512).  Otherwise 128 x 96 where the output width divides by 96 (768 -> 512 tiles, 2304 -> 1536 tiles at 8 192
        # tokens = whole rounds of 2 workgroups per CU; 128 x 128 leaves the last round a quarter full).
        t96 = 8 if hid % 96 == 0 else 0
        pick = (lambda width, k, other: S.gemm_tile_256(m, width, k) or other) if _GEMM256 else (lambda width, k, other: other)
        qkv = S.gemm_bf16(h1, wqkv, S.GEMM_NT, S.EPI_BIAS, bias=(q_b, k_b, v_b), tile=pick(3 * hid, hid, t96))
        att, lse = S.attention_fwd(qkv.view(b, n, 3 * hid), heads)
        att2d = att.view(m, hid)
        x2 = S.gemm_bf16(att2d, wo, S.GEMM_NT, S.EPI_BIAS_DROP_RESID, bias=o_b, resid=x2d, seed=seed, site=site, drop_p=p_proj,
                         tile=pick(hid, hid, t96))
        h2, mean2, rstd2 = S.layer_norm_fwd(x2, ln2_w, ln2_b, eps, torch.bfloat16)
        act, pre = S.gemm_bf16(h2, w1, S.GEMM_NT, S.EPI_BIAS_GELU_DROP, bias=f1_b, seed=seed, site=site + 1, drop_p=p_mlp,
                               tile=pick(mlp, hid, 0))
        x3 = S.gemm_bf16(act, w2, S.GEMM_NT, S.EPI_BIAS_DROP_RESID, bias=f2_b, resid=x2, seed=seed, site=site + 2, drop_p=p_mlp,
                         tile=pick(hid, mlp, t96))
        ctx.save_for_backward(x2d, mean1, rstd1, h1, qkv, att, lse, x2, mean2, rstd2, h2, pre, act, wqkv, wo, w1, w2, ln1_w, ln2_w,
                              wqkv_t, wo_t, w1_t, w2_t)
        ctx.cfg, ctx.shape = cfg, (b, n, hid)
        # storage addresses of the weight parameters: the backward's weight-gradient GEMMs write into their gradient-arena slices
        ctx.weight_keys = ((q_w.data_ptr(), k_w.data_ptr(), v_w.data_ptr()), (o_w.data_ptr(),), (f1_w.data_ptr(),), (f2_w.data_ptr(),))
        ctx.norm_params = ((ln1_w, ln1_b), (ln2_w, ln2_b))   # (leaves: their .grad state decides whether a reduction may be deferred)
        ctx.linear_params = ((q_w, k_w, v_w, q_b, k_b, v_b), (o_w, o_b), (f1_w, f1_b), (f2_w, f2_b))
        return x3.view(b, n, hid)

    @staticmethod
    def backward(ctx, grad):
        S = sis_hip
        (x2d, mean1, rstd1, h1, qkv, att, lse, x2, mean2, rstd2, h2, pre, act, wqkv, wo, w1, w2, ln1_w, ln2_w,
         wqkv_t, wo_t, w1_t, w2_t) = ctx.saved_tensors
        heads, eps, p_proj, p_mlp, site, seed = ctx.cfg
        b, n, hid = ctx.shape
        m = b * n
        g3 = grad.reshape(m, hid)
        if g3.dtype != torch.float32 or not g3.is_contiguous():
            g3 = g3.float().contiguous()
        mlp = w1.shape[0]
        wg = _SideWgrads(g3.device)

        def dgrad(g, w, w_t, epilogue=S.EPI_NONE, **kw):
            """dL/dx = g W of a Linear layer y = x W^T: with the transposed weight shadow an NT product on the 256-row tiles
            (the same kernel and tiles as the forward), otherwise the NN layout of csrc/gemm_bf16.hip."""
            tile = S.gemm_tile_256(m, w.shape[1], w.shape[0]) if (w_t is not None and _GEMM256) else None
            if tile is not None:
                return S.gemm_bf16(g, w_t, S.GEMM_NT, epilogue, tile=tile, **kw)
            return S.gemm_bf16(g, w, S.GEMM_NN, epilogue, **kw)

        # ---- MLP
        # d(fc2 output), bf16: written by the NEXT block's LayerNorm backward together with the gradient it was cast from (below);
        # the last block -- or a gradient that did not come straight from there -- casts here
        gl2 = S.backward_scope.take(("block cast", site + 2), g3) if _FUSE_BLOCK_CAST else None
        if gl2 is None:
            gl2 = S.dropout_bwd_cast(g3, seed, site + 2, p_mlp)
        k_qkv, k_o, k_f1, k_f2 = ctx.weight_keys
        new_qkv, new_o, new_f1, new_f2 = (S.may_complete_late(group) for group in ctx.linear_params)
        d_w2, d_b2 = wg.run(gl2, act, hid, mlp, k_f2, defer=new_f2)
        d_pre = dgrad(gl2, w2, w2_t, S.EPI_GELU_BWD, pre=pre)   # pre = gelu'(h) * dropout factor, stored by fc1's forward epilogue
        d_w1, d_b1 = wg.run(d_pre, h2, mlp, hid, k_f1, defer=new_f1)
        d_h2 = dgrad(d_pre, w1, w1_t)
        # LN2 backward + the skip connection's gradient, and d(out-projection output) = that sum through the proj dropout
        fresh1, fresh2 = (S.may_complete_late(pair, wgrad=False) for pair in ctx.norm_params)
        g2, d_ln2_w, d_ln2_b, gl1 = S.layer_norm_bwd_fused(d_h2, x2, mean2, rstd2, ln2_w, residual_grad=g3, cast_seed=seed,
                                                           cast_site=site, cast_p=p_proj, defer=fresh2)
        # ---- attention
        d_wo, d_bo = wg.run(gl1, att.view(m, hid), hid, hid, k_o, defer=new_o)
        d_att = dgrad(gl1, wo, wo_t)
        d_qkv = S.attention_bwd(d_att.view(b, n, hid), qkv.view(b, n, 3 * hid), att, lse, heads).view(m, 3 * hid)
        d_wqkv, d_bqkv = wg.run(d_qkv, h1, 3 * hid, hid, k_qkv, defer=new_qkv)
        d_h1 = dgrad(d_qkv, wqkv, wqkv_t)
        # (block i's input gradient IS block i - 1's output gradient: its bf16 cast through that block's fc2 dropout site -- 4 (i - 1) + 2 --
        # rides in this launch instead of a launch of its own at the top of that block's backward: 11 launches per step)
        prev_site = site - 2 if (_FUSE_BLOCK_CAST and site >= 4) else None
        g1, d_ln1_w, d_ln1_b, cast_prev = S.layer_norm_bwd_fused(d_h1, x2d, mean1, rstd1, ln1_w, residual_grad=g2, cast_seed=seed,
                                                                 cast_site=prev_site, cast_p=p_mlp, defer=fresh1)
        if cast_prev is not None:   # for the block that receives g1 as it is now (kept until the end of this backward at the latest)
            S.backward_scope.hand_over(("block cast", prev_site), g1, cast_prev)
        wg.join()
        d_q, d_k, d_v = d_wqkv.split(hid, 0)
        d_qb, d_kb, d_vb = d_bqkv.split(hid, 0)
        return (g1.view(b, n, hid), None, None, None, None, None, d_ln1_w, d_ln1_b, d_q, d_k, d_v, d_qb, d_kb, d_vb, d_wo, d_bo,
                d_ln2_w, d_ln2_b, d_w1, d_b1, d_w2, d_b2, None, None, None, None)


class Embeddings(nn.Module):
    """Patch + position embeddings; in hybrid mode the "patches" are 1x1 (or p x p) cells of the ResNetV2
    stride-16 feature map and the stem's intermediate maps are returned as decoder skips."""

    def __init__(self, config, img_size, in_channels=3):
        super().__init__()
        self.config = config
        img_size = _pair(img_size)
        if config.patches.get("grid") is not None:
            grid = config.patches["grid"]
            patch_size = (img_size[0] // 16 // grid[0], img_size[1] // 16 // grid[1])
            real = (patch_size[0] * 16, patch_size[1] * 16)
            n_patches = (img_size[0] // real[0]) * (img_size[1] // real[1])
            self.hybrid = True
        else:
            patch_size = _pair(config.patches["size"])
            n_patches = (img_size[0] // patch_size[0]) * (img_size[1] // patch_size[1])
            self.hybrid = False
        if self.hybrid:
            self.hybrid_model = ResNetV2(block_units=config.resnet.num_layers, width_factor=config.resnet.width_factor)
            in_channels = self.hybrid_model.width * 16
        # nn.Conv2d subclass with the same parameters: under bf16 autocast the hybrid model's 1x1 patch embedding runs on
        # the MI355X bf16 MFMA convolution kernel (any other configuration: the library, as nn.Conv2d)
        self.patch_embeddings = HipConv2d(in_channels=in_channels, out_channels=config.hidden_size,
                                          kernel_size=patch_size, stride=patch_size)
        self.position_embeddings = nn.Parameter(torch.zeros(1, n_patches, config.hidden_size))
        self.dropout = Dropout(config.transformer["dropout_rate"])

    def forward(self, x):
        features = None
        if self.hybrid:
            x, features = self.hybrid_model(x)
        # [B, n_patches, hidden], made contiguous HERE: element-wise ops keep their first operand's strides, so a
        # transposed view would put the whole fp32 residual stream of the encoder in [B, hidden, n] memory order and
        # every LayerNorm / GEMM below (and their gradients) would start with a strided 25 MB copy
        x = self.patch_embeddings(x).flatten(2)
        if x.is_cuda and x.is_contiguous() and x.element_size() in (2, 4):
            x = sis_hip.swap_last2(x)   # one tiled transpose (and one for its gradient) instead of ATen's strided copies
        else:
            x = x.transpose(-1, -2).contiguous()
        return self.dropout(x + self.position_embeddings), features


class Block(nn.Module):
    def __init__(self, config, vis):
        super().__init__()
        self.hidden_size = config.hidden_size
        self.attention_norm = LayerNorm(config.hidden_size, eps=1e-6)
        self.ffn_norm = LayerNorm(config.hidden_size, eps=1e-6)
        self.ffn = Mlp(config)
        self.attn = Attention(config, vis)

    block_index = 0   # set by the Encoder: numbers the block's three dropout sites (4 * index + 0 / 1 / 2)
    _seed = None         # set by the Encoder per training forward: THIS forward's snapshot of the dropout seed word
    _transposed = None   # set by the Encoder per training forward: transposed bf16 shadows (Wqkv^T, Wo^T, W1^T, W2^T) for the data gradients

    def weight_shadow_tensors(self):
        """The four bf16 weight shadows of the block, current (what _FusedBlockFn multiplies with)."""
        la, lf = self.attn._shadows(), self.ffn._shadows()
        return [la[0].tensor(), la[2].tensor(), lf[0].tensor(), lf[2].tensor()]

    def _fused_ok(self, x):
        a, f = self.attn, self.ffn
        return (_FUSED_BLOCK and _SHADOW and _AMP_LINEAR and x.is_cuda and x.dtype == torch.float32 and x.dim() == 3
                and x.is_contiguous() and torch.is_autocast_enabled() and torch.get_autocast_dtype('cuda') == torch.bfloat16
                and not a.vis and a.attention_head_size == 64 and not (self.training and a.attn_dropout.p > 0)
                and a.query.weight.dtype == torch.float32 and self.hidden_size % 256 == 0 and f.fc1.out_features % 64 == 0
                and f.act_fn is F.gelu and isinstance(self.attention_norm, LayerNorm))

    def forward(self, x):
        if self._fused_ok(x):
            a, f = self.attn, self.ffn
            la, lf = a._shadows(), f._shadows()
            training = self.training
            seed = self._seed if self._seed is not None else sis_hip.dropout_seed(x.device)
            cfg = (a.num_attention_heads, self.attention_norm.eps, a.proj_dropout.p if training else 0.0,
                   f.dropout.p if training else 0.0, 4 * self.block_index, seed)
            wt = self._transposed if (self._transposed is not None and torch.is_grad_enabled()) else (None,) * 4
            y = _FusedBlockFn.apply(x, cfg, la[0].tensor(), la[2].tensor(), lf[0].tensor(), lf[2].tensor(),
                                    self.attention_norm.weight, self.attention_norm.bias, a.query.weight, a.key.weight,
                                    a.value.weight, a.query.bias, a.key.bias, a.value.bias, a.out.weight, a.out.bias,
                                    self.ffn_norm.weight, self.ffn_norm.bias, f.fc1.weight, f.fc1.bias, f.fc2.weight, f.fc2.bias, *wt)
            return y, None
        a, weights = self.attn(self.attention_norm(x))
        x = x + a
        return x + self.ffn(self.ffn_norm(x)), weights

    def load_from(self, weights, n_block):
        from .npz_import import load_encoder_block
        load_encoder_block(self, weights, n_block)


class Encoder(nn.Module):
    def __init__(self, config, vis):
        super().__init__()
        self.vis = vis
        self.layer = nn.ModuleList()
        self.encoder_norm = LayerNorm(config.hidden_size, eps=1e-6)
        prototype = Block(config, vis)
        for i in range(config.transformer["num_layers"]):
            block = copy.deepcopy(prototype)
            block.block_index = i
            self.layer.append(block)

    _bank = None   # sis_hip.TransposeBank over every block's four weight shadows

    def _refresh_transposed_shadows(self, hidden_states):
        """Data gradients as NT products (csrc/gemm256_bf16.hip) need W^T: all 4 x 12 transposes by one launch per forward that
        will be differentiated (the optimizer rewrites the shadows every step; inside a captured iteration the launch is
        replayed with them)."""
        use = (_GEMM256 and _GEMM256_DGRAD and torch.is_grad_enabled() and len(self.layer) > 0 and self.layer[0]._fused_ok(hidden_states)
               and sis_hip.gemm_tile_256(hidden_states.shape[0] * hidden_states.shape[1], self.layer[0].hidden_size,
                                         self.layer[0].hidden_size) is not None)
        if not use:
            for block in self.layer:
                block._transposed = None
            return
        sources = [t for block in self.layer for t in block.weight_shadow_tensors()]
        if self._bank is None or not self._bank.current(sources):
            self._bank = sis_hip.TransposeBank(sources)
        self._bank.refresh()
        for i, block in enumerate(self.layer):
            block._transposed = tuple(self._bank.out[4 * i:4 * i + 4])

    def forward(self, hidden_states):
        attn_weights = []
        if self.training and hidden_states.is_cuda and _FUSED_BLOCK:
            # one step of the device seed word per forward: every dropout site of the fused blocks reads it (and their
            # backward reads it again); a captured hipGraph of the iteration replays this launch too
            word = sis_hip.dropout_seed(hidden_states.device)
            sis_hip.dropout_advance(word)
            # Snapshot per forward (one 8-byte device copy, a graph node like the advance): the backward recomputes the masks
            # from the word its OWN forward read, also when another training forward ran in between (gradient accumulation,
            # two forwards then two backwards, a second TransUNet on the device) -- ADVICE r3.
            snapshot = word.clone()
            for block in self.layer:
                block._seed = snapshot
        else:
            for block in self.layer:
                block._seed = None
        if hidden_states.is_cuda:
            self._refresh_transposed_shadows(hidden_states)
        for block in self.layer:
            hidden_states, weights = block(hidden_states)
            if self.vis:
                attn_weights.append(weights)
        return self.encoder_norm(hidden_states), attn_weights


class Transformer(nn.Module):
    def __init__(self, config, img_size, vis):
        super().__init__()
        self.embeddings = Embeddings(config, img_size=img_size)
        self.encoder = Encoder(config, vis)

    def forward(self, input_ids):
        embedding_output, features = self.embeddings(input_ids)
        encoded, attn_weights = self.encoder(embedding_output)
        return encoded, attn_weights, features
