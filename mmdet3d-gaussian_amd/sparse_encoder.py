"""The top layer of the sparse stack: what is BUILT from the ops of sparse_conv.py, sparse_bn.py and sparse_pool.py on the
tensor and containers of sparse_tensor.py — mmdet3d's `SparseBasicBlock`, `make_sparse_convmodule` / `make_sparse_inverse_convmodule`,
`SparseEncoder` (CenterPoint's `pts_middle_encoder`) and `SparseUNet`, the reference's `MlvlSparseEncoder`
(models/middle_encoders/mlvl_sparse_encoder.py:11-32; PV-RCNN's `voxel_middle_encoder`), and the two rewrites of a built model:
`fuse_sparse_conv_bn` / `SparseEncoder.fuse()` (conv + eval BatchNorm + residual + ReLU in one launch) and
`convert_sparse_batchnorm` / `SparseEncoder.convert_norm()` (the live-row `SparseBatchNorm1d`).  The package namespace is
the supported import path of every name here.
"""
import torch
from torch import nn

from .sparse_bn import SparseBatchNorm1d
from .sparse_conv import (FusedSparseConv, SparseConv3d, SparseConvolution, SparseInverseConv3d, SubMConv3d, check_compute_dtype,
                          check_weight_grad)
from .sparse_tensor import SparseConvTensor, SparseModule, SparseSequential


def _norm1d(norm_cfg, channels):
    cfg = dict(norm_cfg or dict(type='BN1d'))
    kind = cfg.pop('type', 'BN1d')
    if kind not in ('BN1d', 'BN'):
        raise RuntimeError(f'norm_cfg type {kind!r}: only BN1d is built here')
    cfg.pop('requires_grad', None)
    return nn.BatchNorm1d(channels, **cfg)


class SparseBasicBlock(SparseModule):
    """mmdet3d's sparse residual block: conv -> norm -> relu -> conv -> norm -> add identity -> relu, both SubMConv3d k3 without bias.
    indice_key (an addition): one index for both layers; the result does not depend on it."""
    expansion = 1

    def __init__(self, inplanes, planes, stride=1, downsample=None, conv_cfg=None, norm_cfg=None, indice_key=None, compute_dtype=None):
        super().__init__()
        if conv_cfg is not None and conv_cfg.get('type', 'SubMConv3d') != 'SubMConv3d':
            raise RuntimeError(f'SparseBasicBlock is built from SubMConv3d, got conv_cfg {conv_cfg}')
        self.conv1 = SubMConv3d(inplanes, planes, 3, stride, padding=1, bias=False, indice_key=indice_key, compute_dtype=compute_dtype)
        self.norm1 = _norm1d(norm_cfg, planes)
        self.conv2 = SubMConv3d(planes, planes, 3, padding=1, bias=False, indice_key=indice_key, compute_dtype=compute_dtype)
        self.norm2 = _norm1d(norm_cfg, planes)
        self.relu = nn.ReLU(inplace=True)
        self.downsample = downsample

    def forward(self, x):
        identity = x.features
        out = self.conv1(x)
        out.features = self.relu(self.norm1(out.features))
        out = self.conv2(out)
        out.features = self.norm2(out.features)
        if self.downsample is not None:
            identity = self.downsample(x)
        out.features = self.relu(out.features + identity)
        return out


_CONV_TYPES = {'SubMConv3d': SubMConv3d, 'SparseConv3d': SparseConv3d, 'SparseInverseConv3d': SparseInverseConv3d}


def _convmodule(who, types, in_channels, out_channels, kernel_size, indice_key, stride, padding, conv_type, norm_cfg, order, compute_dtype):
    """the layers of `order` — conv (no bias) of one of `types`, BatchNorm1d(eps, momentum from norm_cfg), ReLU — in a `SparseSequential`"""
    if not isinstance(order, tuple) or len(order) > 3 or not set(order) <= {'conv', 'norm', 'act'}:
        raise RuntimeError(f"{who}: order must be a tuple over 'conv', 'norm', 'act', got {order!r}")
    if 'conv' in order and conv_type not in types:
        raise RuntimeError(f'{who}: conv_type {conv_type!r} is not built here ({", ".join(types)})')
    layers = []
    for layer in order:
        if layer == 'conv':
            conv = _CONV_TYPES[conv_type]
            geometry = () if conv is SparseInverseConv3d else (stride, padding)        # an inverse layer takes neither, as in mmdet3d
            layers.append(conv(in_channels, out_channels, kernel_size, *geometry, bias=False, indice_key=indice_key, compute_dtype=compute_dtype))
        elif layer == 'norm':
            layers.append(_norm1d(norm_cfg, out_channels))
        else:
            layers.append(nn.ReLU(inplace=True))
    return SparseSequential(*layers)


def make_sparse_convmodule(in_channels, out_channels, kernel_size, indice_key, stride=1, padding=0, conv_type='SubMConv3d', norm_cfg=None,
                           order=('conv', 'norm', 'act'), compute_dtype=None):
    """mmdet3d's sparse conv module: the layers of `order` — conv (no bias), BatchNorm1d(eps, momentum from norm_cfg), ReLU — in a
    `SparseSequential`.  compute_dtype (an addition) is handed to the conv.  conv_type: 'SubMConv3d' or 'SparseConv3d'; the module around a
    'SparseInverseConv3d' is built by `make_sparse_inverse_convmodule`."""
    return _convmodule('make_sparse_convmodule', ('SubMConv3d', 'SparseConv3d'), in_channels, out_channels, kernel_size, indice_key, stride, padding,
                       conv_type, norm_cfg, order, compute_dtype)


def make_sparse_inverse_convmodule(in_channels, out_channels, kernel_size, indice_key, norm_cfg=None, order=('conv', 'norm', 'act'),
                                   compute_dtype=None):
    """mmdet3d's `make_sparse_convmodule(conv_type='SparseInverseConv3d')`: a `SparseInverseConv3d` (no bias) over the index stored under
    `indice_key`, BatchNorm1d and ReLU in the order of `order`, in a `SparseSequential`.  mmdet3d ignores stride and padding for this type;
    here they are not taken."""
    return _convmodule('make_sparse_inverse_convmodule', ('SparseInverseConv3d',), in_channels, out_channels, kernel_size, indice_key, 1, 0,
                       'SparseInverseConv3d', norm_cfg, order, compute_dtype)


# ---- the live-row BatchNorm in a built model --------------------------------------------------------------------------

class SparseNormBasicBlock(SparseBasicBlock):
    """A `SparseBasicBlock` whose norms are `SparseBatchNorm1d`: norm1 carries the first ReLU, norm2 takes the identity as `residual` and
    carries the final ReLU — two convolutions and two norm calls.  Built by `convert_sparse_batchnorm`, which re-classes a block in place."""

    def forward(self, x):
        identity = x.features
        out = self.norm1(self.conv1(x))
        out = self.conv2(out)
        if self.downsample is not None:
            identity = self.downsample(x)
        return self.norm2(out, residual=identity)


def _convert_step(modules, i):
    """a step of `SparseSequential.rewrite`: a BatchNorm1d directly followed by an nn.ReLU becomes one SparseBatchNorm1d('relu') under the
    norm's name, a lone BatchNorm1d one without activation"""
    module, i = modules[i], i + 1
    if type(module) is nn.BatchNorm1d:
        act = None
        if i < len(modules) and isinstance(modules[i], nn.ReLU):
            act, i = 'relu', i + 1
        module = SparseBatchNorm1d.from_batchnorm(module, act)
    return module, i


def convert_sparse_batchnorm(module):
    """Opt-in, in place, returns the module: inside every `SparseSequential` a `BatchNorm1d` (directly followed by an `nn.ReLU` or not)
    becomes a `SparseBatchNorm1d`; every `SparseBasicBlock` becomes a `SparseNormBasicBlock`.  Parameters and buffers are shared with the
    modules they came from: `state_dict` keys and optimizer references stay valid.  Training in the static form (`max_out`,
    `hard_voxelize(static=True)`) NEEDS the converted norm; `.eval()` and `fuse_sparse_conv_bn` work on the result as before."""
    for name, child in list(module.named_children()):
        module._modules[name] = convert_sparse_batchnorm(child)
    if isinstance(module, SparseBasicBlock) and not isinstance(module, SparseNormBasicBlock):
        for name in ('norm1', 'norm2'):
            if type(getattr(module, name)) is not nn.BatchNorm1d:
                raise RuntimeError(f'convert_sparse_batchnorm: {name} of a SparseBasicBlock must be a BatchNorm1d, got {type(getattr(module, name)).__name__}')
        module.norm1 = SparseBatchNorm1d.from_batchnorm(module.norm1, 'relu')
        module.norm2 = SparseBatchNorm1d.from_batchnorm(module.norm2, 'relu')
        module.__class__ = SparseNormBasicBlock
    if isinstance(module, SparseSequential):
        module.rewrite(_convert_step)
    return module


# ---- conv + BatchNorm + residual + ReLU in one launch ----------------------------------------------------------------

class FusedSparseBasicBlock(SparseModule):
    """A `SparseBasicBlock` in two launches: conv1 + norm1 + relu, then conv2 + norm2 + identity + relu.  A `downsample` is evaluated first."""

    def __init__(self, block):
        super().__init__()
        if not isinstance(block, SparseBasicBlock):
            raise RuntimeError(f'FusedSparseBasicBlock: block must be a SparseBasicBlock, got {type(block).__name__}')
        self.conv1 = FusedSparseConv(block.conv1, block.norm1, 'relu')
        self.conv2 = FusedSparseConv(block.conv2, block.norm2, 'relu')
        self.downsample = None if block.downsample is None else fuse_sparse_conv_bn(block.downsample)

    def forward(self, x):
        identity = x.features
        if self.downsample is not None:
            identity = self.downsample(x)
        return self.conv2(self.conv1(x), residual=getattr(identity, 'features', identity))


def _fuse_step(modules, i):
    """a step of `SparseSequential.rewrite`: a conv that is followed by an eval BatchNorm1d and / or an nn.ReLU becomes one FusedSparseConv
    under the conv's name; a conv that nothing follows (a pre-activation order) stays"""
    module, i = modules[i], i + 1
    if type(module) in (SubMConv3d, SparseConv3d, SparseInverseConv3d, SparseConvolution):
        norm = act = None
        if i < len(modules) and isinstance(modules[i], nn.modules.batchnorm._BatchNorm):
            norm, i = modules[i], i + 1
            if isinstance(norm, SparseBatchNorm1d) and norm.activation == 'relu':      # a SparseBatchNorm1d carries its ReLU
                act = 'relu'
        if act is None and i < len(modules) and isinstance(modules[i], nn.ReLU):
            act, i = 'relu', i + 1
        if norm is not None or act is not None:
            module = FusedSparseConv(module, norm, act)
    return module, i


def fuse_sparse_conv_bn(module):
    """mmcv's `fuse_conv_bn` for the sparse encoder: in place, and returns the module (a `SparseBasicBlock` handed in directly comes back
    as its fused replacement).  Inside every `SparseSequential` a `SubMConv3d` / `SparseConv3d` followed by an eval-mode `BatchNorm1d` and / or
    an `nn.ReLU` becomes a `FusedSparseConv`; every `SparseBasicBlock` becomes a `FusedSparseBasicBlock`.  scale = gamma / sqrt(running_var
    + eps) and shift = beta - running_mean * scale are computed in fp64 and held as fp32 buffers (affine=False: gamma = 1, beta = 0).  A
    BatchNorm in training mode, or one without running statistics, raises.  For inference and frozen-BN fine-tuning: the fused layers stay
    differentiable w.r.t. the conv's parameters and their input.  In the static `max_out` form the rows past the count come out zero, as
    `sparse_conv` promises, where the unfused BatchNorm turned them into `shift`.  An eval `SparseBatchNorm1d` (sparse_bn.py) folds as a
    `BatchNorm1d` does and its `activation` is carried into the `FusedSparseConv`; a converted basic block fuses to the same
    `FusedSparseBasicBlock`."""
    if isinstance(module, SparseBasicBlock):
        return FusedSparseBasicBlock(module)
    for name, child in list(module.named_children()):
        module._modules[name] = fuse_sparse_conv_bn(child)
    if isinstance(module, SparseSequential):
        module.rewrite(_fuse_step)
    return module


def set_weight_grad(module, mode):
    """Sets `weight_grad` (None or 'mfma': `sparse_conv`) on every `SparseConvolution` under `module`, in place, and returns
    the module.  The switch is an attribute of the conv, read at every forward, never a buffer or a parameter: `state_dict` is unchanged, and
    it works before or after `convert_sparse_batchnorm` / `fuse_sparse_conv_bn`, whose modules share the conv itself."""
    check_weight_grad(mode, 'set_weight_grad')
    for m in module.modules():
        if isinstance(m, SparseConvolution):
            m.weight_grad = mode
    return module


class SparseEncoder(nn.Module):
    """mmdet3d 0.x's `SparseEncoder`, restated from its published sparse_encoder.py (absent from the reference tree: not pinned):
    CenterPoint's `pts_middle_encoder` (configs/_base_/models/centerpoint_01voxel_second_secfpn_nus.py:10-19).  forward returns
    `spatial_features`: conv_out's dense() viewed as (B, C * D, H, W)."""

    def __init__(self, in_channels, sparse_shape, order=('conv', 'norm', 'act'), norm_cfg=dict(type='BN1d', eps=1e-3, momentum=0.01),
                 base_channels=16, output_channels=128, encoder_channels=((16,), (32, 32, 32), (64, 64, 64), (64, 64, 64)),
                 encoder_paddings=((1,), (1, 1, 1), (1, 1, 1), ((0, 1, 1), 1, 1)), block_type='conv_module', compute_dtype=None):
        super().__init__()
        if block_type not in ('conv_module', 'basicblock'):
            raise RuntimeError(f"block_type must be 'conv_module' or 'basicblock', got {block_type!r}")
        if not isinstance(order, tuple) or len(order) != 3 or set(order) != {'conv', 'norm', 'act'}:
            raise RuntimeError(f"order must be a permutation of ('conv', 'norm', 'act'), got {order!r}")
        self.sparse_shape = list(sparse_shape)
        self.in_channels, self.order, self.base_channels, self.output_channels = in_channels, order, base_channels, output_channels
        self.encoder_channels, self.encoder_paddings = encoder_channels, encoder_paddings
        self.stage_num = len(encoder_channels)
        self.fp16_enabled = False                 # mmdet3d's attribute, inert here: compute_dtype='auto' is what follows autocast and the fp16 hook
        self.compute_dtype = check_compute_dtype(compute_dtype, type(self).__name__)    # handed to every conv built below
        self.conv_input = make_sparse_convmodule(in_channels, base_channels, 3, norm_cfg=norm_cfg, padding=1, indice_key='subm1',
                                                 conv_type='SubMConv3d', order=order if order[0] == 'conv' else ('conv',),
                                                 compute_dtype=compute_dtype)
        encoder_out_channels = self.make_encoder_layers(make_sparse_convmodule, norm_cfg, base_channels, block_type=block_type)
        self.conv_out = make_sparse_convmodule(encoder_out_channels, output_channels, kernel_size=(3, 1, 1), stride=(2, 1, 1), norm_cfg=norm_cfg,
                                               padding=0, indice_key='spconv_down2', conv_type='SparseConv3d', compute_dtype=compute_dtype)

    def make_encoder_layers(self, make_block, norm_cfg, in_channels, block_type='conv_module', conv_cfg=dict(type='SubMConv3d')):
        self.encoder_layers = SparseSequential()
        out_channels = in_channels
        for i, blocks in enumerate(self.encoder_channels):
            blocks_list = []
            for j, out_channels in enumerate(tuple(blocks)):
                padding = tuple(self.encoder_paddings[i])[j]
                if block_type == 'basicblock':                            # every stage but the last ends with the strided layer
                    strided = j == len(blocks) - 1 and i != len(self.encoder_channels) - 1
                else:                                                     # every stage but the first starts with it
                    strided = block_type == 'conv_module' and i != 0 and j == 0
                if block_type == 'basicblock' and not strided:
                    blocks_list.append(SparseBasicBlock(out_channels, out_channels, norm_cfg=norm_cfg, conv_cfg=conv_cfg,
                                                        indice_key=f'subm{i + 1}', compute_dtype=self.compute_dtype))
                else:
                    layer = (dict(stride=2, indice_key=f'spconv{i + 1}', conv_type='SparseConv3d') if strided else
                             dict(indice_key=f'subm{i + 1}', conv_type='SubMConv3d'))
                    blocks_list.append(make_block(in_channels, out_channels, 3, norm_cfg=norm_cfg, padding=padding, compute_dtype=self.compute_dtype,
                                                  **layer))
                in_channels = out_channels
            self.encoder_layers.add_module(f'encoder_layer{i + 1}', SparseSequential(*blocks_list))
        return out_channels

    def encode(self, voxel_features, coors, batch_size):
        """-> (the stages' SparseConvTensors, conv_out's dense() viewed as (B, C * D, H, W))"""
        x = self.conv_input(SparseConvTensor(voxel_features, coors.int(), self.sparse_shape, batch_size))
        encode_features = []
        for encoder_layer in self.encoder_layers:
            x = encoder_layer(x)
            encode_features.append(x)
        spatial_features = self.conv_out(encode_features[-1]).dense()
        N, C, D, H, W = spatial_features.shape
        return encode_features, spatial_features.view(N, C * D, H, W)

    def forward(self, voxel_features, coors, batch_size):
        return self.encode(voxel_features, coors, batch_size)[1]

    def fuse(self):
        """`fuse_sparse_conv_bn` on this encoder (in eval mode): every conv -> BatchNorm1d -> ReLU and every basic block in fused launches"""
        return fuse_sparse_conv_bn(self)

    def convert_norm(self):
        """`convert_sparse_batchnorm` on this encoder (opt-in, in place): every BatchNorm1d (+ ReLU) and every basic block on the live-row
        `SparseBatchNorm1d` — what training in the static form needs; `.eval().fuse()` still works afterwards"""
        return convert_sparse_batchnorm(self)

    def set_weight_grad(self, mode):
        """`set_weight_grad` on this encoder (opt-in, in place): 'mfma' takes the weight gradient of every conv on the matrix cores where it
        runs in fp16 / bf16 on the device (inert in fp32 and on CPU tensors); None is the default again"""
        return set_weight_grad(self, mode)


class MlvlSparseEncoder(SparseEncoder):
    """The reference's `MlvlSparseEncoder` (models/middle_encoders/mlvl_sparse_encoder.py:11-32), PV-RCNN's `voxel_middle_encoder`:
    forward returns dict(encode_features = every stage's SparseConvTensor, spatial_features)."""

    def forward(self, voxel_features, coors, batch_size):
        encode_features, spatial_features = self.encode(voxel_features, coors, batch_size)
        return dict(encode_features=encode_features, spatial_features=spatial_features)


class SparseUNet(SparseEncoder):
    """mmdet3d 0.x's `SparseUNet` middle encoder (Part-A2's), restated from its published sparse_unet.py (absent from the reference tree: not
    pinned): `SparseEncoder`'s conv_input, encoder_layers and conv_out, and a decoder that goes back up stage by stage.  Decoder block n
    (4 .. 1): `lateral_layer{n}` a `SparseBasicBlock` on 'subm{n}', `merge_layer{n}` a SubMConv3d module over the concatenated [bottom,
    lateral] features on 'subm{n}', `upsample_layer{n}` a `SparseInverseConv3d` module over the index the encoder stored under 'spconv{n}'
    (block 1: a SubMConv3d module on 'subm1').  The decoder builds no index of its own.
    forward returns dict(spatial_features (B, C * D, H, W), seg_features (num_voxels, decoder_channels[-1][-1])): per-voxel features on the
    input voxels, in the input's row order."""

    def __init__(self, in_channels, sparse_shape, order=('conv', 'norm', 'act'), norm_cfg=dict(type='BN1d', eps=1e-3, momentum=0.01),
                 base_channels=16, output_channels=128, encoder_channels=((16,), (32, 32, 32), (64, 64, 64), (64, 64, 64)),
                 encoder_paddings=((1,), (1, 1, 1), (1, 1, 1), ((0, 1, 1), 1, 1)),
                 decoder_channels=((64, 64, 64), (64, 64, 32), (32, 32, 16), (16, 16, 16)), decoder_paddings=((1, 0), (1, 0), (0, 0), (0, 1)),
                 compute_dtype=None):
        super().__init__(in_channels, sparse_shape, order, norm_cfg, base_channels, output_channels, encoder_channels, encoder_paddings,
                         'conv_module', compute_dtype)
        if len(decoder_channels) != len(encoder_channels) or any(len(tuple(c)) != 3 for c in decoder_channels):
            raise RuntimeError(f'SparseUNet: decoder_channels must hold one (lateral, merge, upsample) triple per encoder stage, got {decoder_channels!r}')
        self.decoder_channels, self.decoder_paddings = decoder_channels, decoder_paddings
        self.make_decoder_layers(norm_cfg, tuple(encoder_channels[-1])[-1])

    def make_decoder_layers(self, norm_cfg, in_channels):
        block_num = len(self.decoder_channels)
        for i, block_channels in enumerate(self.decoder_channels):
            n, paddings = block_num - i, self.decoder_paddings[i]
            setattr(self, f'lateral_layer{n}', SparseBasicBlock(in_channels, block_channels[0], norm_cfg=norm_cfg, indice_key=f'subm{n}',
                                                                compute_dtype=self.compute_dtype))
            setattr(self, f'merge_layer{n}', make_sparse_convmodule(in_channels * 2, block_channels[1], 3, norm_cfg=norm_cfg, padding=paddings[0],
                                                                    indice_key=f'subm{n}', conv_type='SubMConv3d', compute_dtype=self.compute_dtype))
            if n != 1:
                setattr(self, f'upsample_layer{n}', make_sparse_inverse_convmodule(in_channels, block_channels[2], 3, norm_cfg=norm_cfg,
                                                                                   indice_key=f'spconv{n}', compute_dtype=self.compute_dtype))
            else:                                                        # the last block stays on the input rows: a submanifold layer
                setattr(self, f'upsample_layer{n}', make_sparse_convmodule(in_channels, block_channels[2], 3, norm_cfg=norm_cfg, padding=paddings[1],
                                                                           indice_key='subm1', conv_type='SubMConv3d', compute_dtype=self.compute_dtype))
            in_channels = block_channels[2]

    @staticmethod
    def reduce_channel(x, out_channels):
        """x.features (n, C) -> (n, out_channels): the sum over groups of C / out_channels adjacent channels"""
        n, in_channels = x.features.shape
        if in_channels % out_channels != 0 or in_channels < out_channels:
            raise RuntimeError(f'SparseUNet.reduce_channel: {in_channels} channels cannot be reduced to {out_channels}')
        x.features = x.features.view(n, out_channels, -1).sum(dim=2)
        return x

    def decoder_layer_forward(self, x_lateral, x_bottom, lateral_layer, merge_layer, upsample_layer):
        x = lateral_layer(x_lateral)
        x.features = torch.cat((x_bottom.features, x.features), dim=1)
        x_merge = merge_layer(x)
        x = self.reduce_channel(x, x_merge.features.shape[1])
        x.features = x_merge.features + x.features
        return upsample_layer(x)

    def forward(self, voxel_features, coors, batch_size):
        encode_features, spatial_features = self.encode(voxel_features, coors, batch_size)
        x = encode_features[-1]
        for n in range(self.stage_num, 0, -1):
            x = self.decoder_layer_forward(encode_features[n - 1], x, getattr(self, f'lateral_layer{n}'), getattr(self, f'merge_layer{n}'),
                                           getattr(self, f'upsample_layer{n}'))
        return dict(spatial_features=spatial_features, seg_features=x.features)
