"""Mirror of the reference's `audiolm_pytorch/soundstream.py` for the TOKENIZE path and the DECODE path
(§8(f) item 3, incl. the LocalTransformer of the reference-default `use_local_attn=True`): `SoundStream.tokenize(audio)`, `SoundStream.forward(x, return_encoded=True |
return_codes_only=True)` -- the causal-conv encoder (soundstream.py:332-380, 519-531) and the eval-mode forward of the grouped residual VQ
(soundstream.py:592-607, :840) -- and `decode_from_codebook_indices` / `decode` (soundstream.py:691-709: code lookup, transposed-conv
decoder :347-360, 382-395, 615-627) run on the MI355X kernels of csrc/codec.hip (exact-fp32 MFMA).  The training losses (soundstream.py:868-995:
three wave MultiScaleDiscriminators, hinge / feature / reconstruction terms) are opt-in, `with_discriminators=True` (discriminators.py,
csrc/discr.hip), and so are the ComplexSTFTDiscriminator, `stft_discriminator=True` (csrc/stft_discr.hip), and the multi-spectral mel-spectrogram
reconstruction loss, `with_mel_loss=True` (mel_loss.py, csrc/mel_loss.hip), and the gradient penalty of the discriminator loss, `with_grad_penalty=True`
(a double backward through the discriminator kernels), and the FiLM conditioners of the denoising variant, `with_film=True` (`is_denoising=`;
csrc/film_se.hip, which also holds the squeeze-excite gate of `squeeze_excite=True` units); the finite scalar quantizer, `use_finite_scalar_quantizer=True` (GroupedResidualFSQ, csrc/fsq.hip); the lookup-free quantizer, `use_lookup_free_quantizer=True` together with the opt-in `with_lfq=True`
(GroupedResidualLFQ, csrc/lfq.hip: entropy and commitment losses in training mode, single process; without `with_lfq=True` it raises); the gate-loop
layers, `use_gate_loop_layers=True` together with the opt-in `with_gate_loop=True` (one GateLoopBlock after every encoder / decoder block: a linear
recurrence along time as a parallel scan, csrc/gate_loop.hip; without `with_gate_loop=True` it raises).  In training mode the quantizer takes one
training step per call (csrc/rvq_train.hip: quantize dropout, commitment loss, rotation trick, EMA codebooks with dead-code expiry, k-means
initialisation; single process only), so `forward(x, return_recons_only=True | return_encoded=True)` is differentiable end to end.  The conv encoder / decoder are
differentiable: in training mode, with grad mode on and an input or parameter that requires grad, `encode` / `decode` / `decode_from_codebook_indices`
build a graph over the backward kernels of csrc/codec_bwd.hip and, for the LocalTransformer of use_local_attn=True, csrc/local_attn_bwd.hip (codec_bwd.py;
attn_dim_head outside {32, 64} or a window outside the attention kernels' envelope raises there).
`encoder_attn` / `decoder_attn` (soundstream.py:397-440, 545, 613): local-attention's LocalMHA + FeedForward (third-party source, not vendored:
restated, parity unpinned -- oracle/local_attention_restated.py) run in the codec's [B, C, T] layout: LayerNorm / windowed causal attention with
qk-l2norm, rotary + xpos and per-head value gates / GEGLU are csrc/local_attn.hip, the Linear layers are k = 1 convs on the exact-fp32 MFMA kernel.

The module tree keeps the reference's parameter / buffer NAMES for the parts it has, so `state_dict()` entries `encoder.*` and
`rq.*` of a reference checkpoint load with `load_state_dict(..., strict=False)`:
    encoder.0.conv.{weight,bias}                        CausalConv1d(input_channels -> channels, 7)
    encoder.{b}.{r}.fn.{0,2}.conv.{weight,bias}         ResidualUnit r of EncoderBlock b (k7 dilated conv, ELU, k1 conv, ELU, + x)
    encoder.{b}.{r}.fn.4.net.{0,2}.{weight,bias}        its SqueezeExcite (squeeze_excite=True only; decoder units alike)
    {encoder,decoder}_film.to_cond.{weight,bias}        FiLM conditioners (with_film=True only)
    {encoder,decoder}.{2 b}.fn.fn.{norm.gamma, to_qkva.0.weight}   gate-loop block after block b (with_gate_loop=True only: the blocks then sit at the
                                                        odd indices 2 b - 1 and the final conv at 2 * len(strides) + 1)
    encoder.{b}.3.conv.{weight,bias}                    strided down-sampling conv (k = 2 * stride)
    encoder.{last}.conv.{weight,bias}                   CausalConv1d(-> codebook_dim, 3)
    {encoder,decoder}_attn.layers.{i}.0.{norm.{weight,bias}, to_qkv.weight, q_scale, k_scale, attn_fn.rel_pos.inv_freq, to_v_gate.0.{weight,bias},
                                         to_out.weight}   LocalMHA;   .layers.{i}.1.{0.{weight,bias}, 1.weight, 4.weight}   FeedForward
    decoder.0.conv / decoder.{b}.0.conv (ConvTranspose1d) / decoder.{b}.{1,2,3}.fn.{0,2}.conv / decoder.{last}.conv
    rq.rvqs.{g}.layers.{q}._codebook.{initted, cluster_size, embed_avg, embed (1, C, d)}
    rq.rvqs.{g}.{project_in,project_out}.{weight,bias}    GroupedResidualFSQ (use_finite_scalar_quantizer=True only; nothing in the identity case)
    rq.rvqs.{g}.{project_in,project_out}.{weight,bias}, rq.rvqs.{g}.layers.{q}.mask (int64 2^(d-1) .. 1)    GroupedResidualLFQ (with_lfq=True only)
"""
from __future__ import annotations

import functools
import os
import random
from itertools import cycle

import torch
from torch import nn

from . import codec_bwd, core, discriminators as D, mel_loss, ops
from .resample import resample

F32 = torch.float32
FUSE_RESUNIT = os.environ.get('ALM_FUSE_RESUNIT', '1') != '0'      # A/B switch: 0 = the two alm_conv1d_causal launches per ResidualUnit


class CausalConv1d(nn.Module):                                   # soundstream.py:332-345
    def __init__(self, chan_in, chan_out, kernel_size, pad_mode='reflect', **kwargs):
        super().__init__()
        if pad_mode != 'reflect':
            raise NotImplementedError('only the reference default pad_mode="reflect" is implemented')
        self.dilation = kwargs.get('dilation', 1)
        self.stride = kwargs.get('stride', 1)
        self.kernel_size = kernel_size
        self.pad_mode = pad_mode
        self.causal_padding = self.dilation * (kernel_size - 1) + (1 - self.stride)
        self.conv = nn.Conv1d(chan_in, chan_out, kernel_size, **kwargs)
        self._packed = None
        self._packed_t = codec_bwd._ImageCache()                  # transposed image for the input gradient (training mode only)

    def packed(self):
        w = self.conv.weight
        ver = (w.data_ptr(), core.tensor_version(w))
        if self._packed is None or self._packed[0] != ver:
            self._packed = (ver, ops.conv1d_pack(w.detach().to(F32)))
        return self._packed[1]

    def run(self, x, *, elu=False, residual=None):
        return ops.conv1d_causal(x, self.packed(), self.conv.bias.detach(), self.conv.out_channels, self.kernel_size, stride=self.stride,
                                 dilation=self.dilation, elu=elu, residual=residual)

    def call(self, x, *, elu=False):
        """run(), or its autograd Function in training mode with grad mode on and something that requires grad"""
        if codec_bwd.wants_grad(self, x):
            return codec_bwd.CausalConv1dFn.apply(x, self.conv.weight, self.conv.bias, self, elu)
        return self.run(x, elu=elu)

    def forward(self, x):
        return self.call(x)


class CausalConvTranspose1d(nn.Module):                          # soundstream.py:347-360
    """ConvTranspose1d(k = 2 * stride, stride) cut to n * stride outputs.  Output t = q * stride + r depends on input frames q and q - 1
    only (taps r and r + stride), so it runs as the k = 2, zero-left-padded causal conv over `stride` phase-major copies of the output
    channels (alm_conv1d_causal, exact-fp32 MFMA), followed by the phase interleave."""

    def __init__(self, chan_in, chan_out, kernel_size, stride, **kwargs):
        super().__init__()
        if kernel_size != 2 * stride or kwargs:
            raise NotImplementedError('only the reference decoder form is implemented: kernel_size = 2 * stride, default ConvTranspose1d options')
        self.upsample_factor = stride
        self.padding = kernel_size - 1
        self.conv = nn.ConvTranspose1d(chan_in, chan_out, kernel_size, stride)
        self._packed = None
        self._packed_t = codec_bwd._ImageCache()

    def packed(self):
        w, b = self.conv.weight, self.conv.bias
        ver = (w.data_ptr(), core.tensor_version(w), core.tensor_version(b))
        if self._packed is None or self._packed[0] != ver:
            s = self.upsample_factor
            cin, cout, _ = w.shape
            wd = w.detach().to(F32)                                                  # [Cin, Cout, 2 s]
            # W2[(r, co), ci, tap]: tap 0 <- x[q - 1] uses w[ci, co, r + s]; tap 1 <- x[q] uses w[ci, co, r]
            w2 = torch.stack((wd[:, :, s:], wd[:, :, :s]), dim=-1)                   # [Cin, Cout, s(r), 2(tap)]
            w2 = w2.permute(2, 1, 0, 3).reshape(s * cout, cin, 2).contiguous()
            self._packed = (ver, ops.conv1d_pack(w2), b.detach().to(F32).repeat(s).contiguous())
        return self._packed[1], self._packed[2]

    def _w2(self):
        """the weight in the k = 2 conv form W2[(r, co), ci, tap]: tap 0 <- x[q - 1] uses w[ci, co, r + s]; tap 1 <- x[q] uses w[ci, co, r]"""
        s = self.upsample_factor
        cin, cout, _ = self.conv.weight.shape
        wd = self.conv.weight.detach().to(F32)
        return torch.stack((wd[:, :, s:], wd[:, :, :s]), dim=-1).permute(2, 1, 0, 3).reshape(s * cout, cin, 2).contiguous()

    def packed_t(self):
        """transposed image of the k = 2 form for the input gradient (alm_conv1d_dgrad), per weight version"""
        return self._packed_t.get((self.conv.weight,), lambda: ops.conv1d_pack_t(self._w2()))

    def run(self, x):
        wp, b2 = self.packed()
        s, cout = self.upsample_factor, self.conv.out_channels
        y = ops.conv1d_causal(x, wp, b2, s * cout, 2, zero_pad=True)
        return ops.phase_interleave(y, cout, s)

    def forward(self, x):
        if codec_bwd.wants_grad(self, x):
            return codec_bwd.CausalConvTranspose1dFn.apply(x, self.conv.weight, self.conv.bias, self)
        return self.run(x)


class SqueezeExcite(nn.Module):                                  # soundstream.py:145-169
    """holder of the reference's parameters (`net.0` / `net.2`: the two k = 1 convs around the SiLU).  Inside a ResidualUnit its input is (b, c, n)
    and the reference takes the cumulative mean over dim -2, the CHANNEL axis: the op is pointwise in time and runs as
    alm_se_gate_fwd, fused with the unit's skip add."""

    def __init__(self, dim, reduction_factor=4, dim_minimum=8):
        super().__init__()
        dim_inner = max(dim_minimum, dim // reduction_factor)
        if not ops.se_gate_supported(dim, dim_inner):
            raise NotImplementedError(f'squeeze_excite: the squeeze-excite kernels hold the hidden layer in registers, up to 128 wide (512 channels); got '
                                      f'{dim} channels / hidden width {dim_inner}')
        self.net = nn.Sequential(nn.Conv1d(dim, dim_inner, 1), nn.SiLU(), nn.Conv1d(dim_inner, dim, 1), nn.Sigmoid())

    def forward(self, x, residual=None):
        """x fp32 [B, C, T] -> x * gate(x) (+ residual)"""
        if not x.is_cuda:
            raise RuntimeError('audiolm_pytorch_amd.SoundStream runs on the MI355X only (no CPU fallback)')
        return ops.se_gate_fwd(x.to(F32).contiguous(), *codec_bwd.se_params(self), residual=residual)


class _ResidualFn(nn.Module):
    """holder with the reference's `.fn` Sequential naming: fn.0 = dilated k7 conv, fn.2 = k1 conv (fn.1 / fn.3 are ELUs), with squeeze_excite=True
    fn.4 = SqueezeExcite."""

    def __init__(self, chan, dilation, kernel_size, pad_mode, squeeze_excite=False):
        super().__init__()
        self.fn = nn.Sequential(CausalConv1d(chan, chan, kernel_size, dilation=dilation, pad_mode=pad_mode), nn.ELU(),
                                CausalConv1d(chan, chan, 1, pad_mode=pad_mode), nn.ELU(), *((SqueezeExcite(chan),) if squeeze_excite else ()))
        self.squeeze_excite = bool(squeeze_excite)

    def forward(self, x):                                        # soundstream.py:362-369: ELU(conv1(ELU(conv7(x)))) + x
        c7, c1 = self.fn[0], self.fn[2]
        if self.squeeze_excite:                                  # SE(ELU(conv1(ELU(conv7(x))))) + x: the two convs, then the gate with the skip add
            se = self.fn[4]
            if codec_bwd.wants_grad(self, x):
                return codec_bwd.ResidualUnitSEFn.apply(x, c7.conv.weight, c7.conv.bias, c1.conv.weight, c1.conv.bias, se.net[0].weight, se.net[0].bias,
                                                        se.net[2].weight, se.net[2].bias, self)
            return se(c1.run(c7.run(x, elu=True), elu=True), residual=x)
        if codec_bwd.wants_grad(self, x):                        # two launches + the skip add, h and the pre-residual output saved (bitwise the fused result)
            return codec_bwd.ResidualUnitFn.apply(x, c7.conv.weight, c7.conv.bias, c1.conv.weight, c1.conv.bias, self)
        if FUSE_RESUNIT and ops.resunit_supported(x.shape[1]) and c7.dilation * (c7.kernel_size - 1) < x.shape[2]:
            # one launch, the intermediate in registers (alm_resunit_causal: bitwise equal to the two launches below)
            return ops.resunit_causal(x, c7.packed(), c7.conv.bias.detach(), c1.packed(), c1.conv.bias.detach(), c7.kernel_size, c7.dilation)
        h = c7.run(x, elu=True)
        return c1.run(h, elu=True, residual=x)


def ResidualUnit(chan_in, chan_out, dilation, kernel_size=7, squeeze_excite=False, pad_mode='reflect'):
    assert chan_in == chan_out
    return _ResidualFn(chan_in, dilation, kernel_size, pad_mode, squeeze_excite)


def EncoderBlock(chan_in, chan_out, stride, cycle_dilations=(1, 3, 9), squeeze_excite=False, pad_mode='reflect'):   # soundstream.py:371-380
    it = cycle(cycle_dilations)
    return nn.Sequential(ResidualUnit(chan_in, chan_in, next(it), squeeze_excite=squeeze_excite, pad_mode=pad_mode),
                         ResidualUnit(chan_in, chan_in, next(it), squeeze_excite=squeeze_excite, pad_mode=pad_mode),
                         ResidualUnit(chan_in, chan_in, next(it), squeeze_excite=squeeze_excite, pad_mode=pad_mode),
                         CausalConv1d(chan_in, chan_out, 2 * stride, stride=stride, pad_mode=pad_mode))


def DecoderBlock(chan_in, chan_out, stride, cycle_dilations=(1, 3, 9), squeeze_excite=False, pad_mode='reflect'):   # soundstream.py:382-395
    it = cycle(cycle_dilations)
    return nn.Sequential(CausalConvTranspose1d(chan_in, chan_out, 2 * stride, stride=stride),
                         ResidualUnit(chan_out, chan_out, next(it), squeeze_excite=squeeze_excite, pad_mode=pad_mode),
                         ResidualUnit(chan_out, chan_out, next(it), squeeze_excite=squeeze_excite, pad_mode=pad_mode),
                         ResidualUnit(chan_out, chan_out, next(it), squeeze_excite=squeeze_excite, pad_mode=pad_mode))


class _RMSNorm(nn.Module):                                       # gateloop_transformer's RMSNorm: holder of `gamma`
    def __init__(self, dim):
        super().__init__()
        self.gamma = nn.Parameter(torch.ones(dim))


class _Rearrange(nn.Module):                                     # `to_qkva.1` of the package ('b n (qkva d) -> qkva (b d) n'): no parameters
    def forward(self, x):
        raise NotImplementedError('runs inside the gate-loop scan (csrc/gate_loop.hip): the q | kv | a rows of z')


class SimpleGateLoopLayer(nn.Module):
    """holder of gateloop_transformer.SimpleGateLoopLayer's parameters (`norm.gamma`, `to_qkva.0.weight`) in the one configuration the reference
    builds: prenorm RMSNorm, no post_ln, forward in time.  `use_heinsen` (the log-space formulation of the same recurrence) selects no different
    arithmetic here: both of the reference's call sites run the one scan kernel.  The arithmetic is RESTATED (tests/gate_loop_restated.py; the package
    is not vendored, parity with it is unpinned, like LocalMHA, FSQ and LFQ)."""

    def __init__(self, dim, use_heinsen=False, post_ln=False, reverse=False):
        super().__init__()
        if post_ln:
            raise NotImplementedError('SimpleGateLoopLayer(post_ln=True) is not implemented (the reference builds the default False)')
        if reverse:
            raise NotImplementedError('SimpleGateLoopLayer(reverse=True) is not implemented (the reference builds the default False)')
        self.dim = dim
        self.norm = _RMSNorm(dim)
        self.to_qkva = nn.Sequential(nn.Linear(dim, dim * 3, bias=False), _Rearrange())
        self._lin = _Linear1x1()                                 # packed images of to_qkva.0.weight, per parameter version

    def forward(self, x, cache=None, return_cache=False):
        raise NotImplementedError('SimpleGateLoopLayer runs inside its GateLoopBlock in the codec layout; the streaming protocol (cache= / '
                                  'return_cache) is not implemented')


class ChannelTranspose(nn.Module):                               # soundstream.py:322-330 (holder: `fn`); its skip add is one of the block's two
    def __init__(self, fn):
        super().__init__()
        self.fn = fn

    def forward(self, x, **kwargs):
        raise NotImplementedError('runs inside its GateLoopBlock: the codec layout [B, C, T] is kept, nothing is transposed')


class Residual(nn.Module):                                       # soundstream.py:314-320
    """Residual(ChannelTranspose(GateLoop(dim))) as ONE op on x fp32 [B, dim, T]: y = q * h + 2 x (each wrapper adds x once), with
    (q | kv | a) = to_qkva(RMSNorm(x)) and h[t] = sigmoid(a[t]) h[t-1] + kv[t].  Launches: alm_gate_loop_norm_fwd, the k = 1 projection on the
    exact-fp32 MFMA conv kernel, alm_gate_loop_scan_fwd.  In training mode with a graph wanted: codec_bwd.GateLoopFn over the same launches."""

    def __init__(self, fn):
        super().__init__()
        if not (isinstance(fn, ChannelTranspose) and isinstance(fn.fn, SimpleGateLoopLayer)):
            raise NotImplementedError('Residual: only the reference\'s Residual(ChannelTranspose(GateLoop(dim))) is implemented')
        self.fn = fn

    @property
    def layer(self):
        return self.fn.fn

    def launches(self, x):
        """(z = to_qkva(RMSNorm(x)) [B, 3 dim, T], y): the forward launches, shared by the eval path and the autograd Function"""
        layer = self.layer
        xn = ops.gate_loop_norm_fwd(x, layer.norm.gamma.detach().to(F32).contiguous())
        z = layer._lin(layer.to_qkva[0], xn)
        return z, ops.gate_loop_scan_fwd(z, x)

    def forward(self, x, **kwargs):
        if kwargs:
            raise NotImplementedError(f'GateLoopBlock: the streaming protocol ({", ".join(sorted(kwargs))}) is not implemented')
        if not x.is_cuda:
            raise RuntimeError('audiolm_pytorch_amd.SoundStream runs on the MI355X only (no CPU fallback)')
        x = x.to(F32).contiguous()
        if x.dim() != 3 or x.shape[1] != self.layer.dim:
            raise ValueError(f'GateLoopBlock: expected [B, {self.layer.dim}, T], got {tuple(x.shape)}')
        if codec_bwd.wants_grad(self, x):
            return codec_bwd.GateLoopFn.apply(x, self.layer.norm.gamma, self.layer.to_qkva[0].weight, self)
        return self.launches(x)[-1]


def GateLoopBlock(dim, use_heinsen=False):
    """the reference's wrapped gate-loop layer; state_dict: fn.fn.norm.gamma (dim,), fn.fn.to_qkva.0.weight (3 dim, dim)"""
    return Residual(ChannelTranspose(SimpleGateLoopLayer(dim, use_heinsen=use_heinsen)))


class _EuclideanCodebook(nn.Module):
    def __init__(self, dim, codebook_size):
        super().__init__()
        self.register_buffer('initted', torch.tensor([False]))
        self.register_buffer('cluster_size', torch.ones(1, codebook_size))
        self.register_buffer('embed_avg', torch.zeros(1, codebook_size, dim))
        self.register_buffer('embed', torch.zeros(1, codebook_size, dim))


class _VectorQuantize(nn.Module):
    def __init__(self, dim, codebook_size):
        super().__init__()
        self._codebook = _EuclideanCodebook(dim, codebook_size)


class _ResidualVQ(nn.Module):
    def __init__(self, dim, num_quantizers, codebook_size):
        super().__init__()
        self.layers = nn.ModuleList([_VectorQuantize(dim, codebook_size) for _ in range(num_quantizers)])


class GroupedResidualVQ(nn.Module):
    """vector-quantize-pytorch's GroupedResidualVQ as the reference builds it (soundstream.py:592-607).  eval(): the tokenize forward (alm_rvq_encode).
    train(): one training step per call (csrc/rvq_train.hip; arithmetic restated in tests/rvq_train_restated.py) -- quantize dropout, per layer the
    assignment against the pre-update codebook, commitment loss, rotation trick or straight-through output, and after the layer loop the EMA codebook
    update with Laplace smoothing and dead-code expiry; layers whose `initted` is False are k-means-initialised on their residual first.  Codebooks get
    no gradient (learnable_codebook=False); the input gradient is alm_rvq_train_bwd (codec_bwd.RvqTrainFn).  Single process only: with
    torch.distributed at world size > 1 the training forward raises."""

    def __init__(self, *, dim, groups=1, num_quantizers, codebook_size, decay=0.95, commitment_weight=1., quantize_dropout=True,
                 quantize_dropout_cutoff_index=1, quantize_dropout_multiple_of=1, rotation_trick=True, threshold_ema_dead_code=2, kmeans_iters=10, eps=1e-5,
                 stochastic_sample_codes=False, **unused):
        super().__init__()
        assert dim % groups == 0
        if stochastic_sample_codes:
            raise NotImplementedError('stochastic_sample_codes is not implemented (reference default False)')
        assert kmeans_iters >= 1 and quantize_dropout_cutoff_index >= 0 and quantize_dropout_multiple_of >= 1
        self.dim, self.groups, self.num_quantizers, self.codebook_size = dim, groups, num_quantizers, codebook_size
        self.decay, self.commitment_weight, self.eps = decay, commitment_weight, eps
        self.quantize_dropout = quantize_dropout and num_quantizers > 1
        self.quantize_dropout_cutoff_index, self.quantize_dropout_multiple_of = quantize_dropout_cutoff_index, quantize_dropout_multiple_of
        self.rotation_trick, self.threshold_ema_dead_code, self.kmeans_iters = rotation_trick, threshold_ema_dead_code, kmeans_iters
        self.rvqs = nn.ModuleList([_ResidualVQ(dim // groups, num_quantizers, codebook_size) for _ in range(groups)])
        self._packed = None
        self._initted_cache = None

    def _pack(self, require_init=True):
        embeds = [[l._codebook.embed for l in r.layers] for r in self.rvqs]
        ver = tuple((e.data_ptr(), core.tensor_version(e)) for row in embeds for e in row)
        if self._packed is None or self._packed[0] != ver:
            for r in self.rvqs:
                for l in r.layers:
                    if require_init and not bool(l._codebook.initted.item()):
                        raise RuntimeError('codebooks are not initialised (`initted` is False): the k-means initialisation happens on the first '
                                           'training-mode batch (soundstream.py:600) -- load a trained codec, set them, or run a training step')
            packs = []
            for row in embeds:
                E = torch.stack([e[0].detach().to(F32) for e in row]).contiguous()       # [Q, C, d]
                packs.append((E,) + ops.rvq_pack(E))
            if not require_init:
                return packs                                     # never cached: an eval call must still meet the check above
            self._packed = (ver, packs)
        return self._packed[1]

    def _initted(self):
        """[group][layer] bools of the `initted` buffers; read from the device only when one of them changed (tensor version)"""
        bufs = [l._codebook.initted for r in self.rvqs for l in r.layers]
        key = tuple((t.data_ptr(), core.tensor_version(t)) for t in bufs)
        if self._initted_cache is None or self._initted_cache[0] != key:
            flags = [bool(v) for v in torch.cat([t.reshape(1) for t in bufs]).tolist()]
            q = self.num_quantizers
            self._initted_cache = (key, [flags[g * q:(g + 1) * q] for g in range(self.groups)])
        return self._initted_cache[1]

    def sample_rows(self, num_rows, count, device):
        """`count` random row numbers of `num_rows` (int64, on `device`): the k-means start points and the replacements of expired codes.  The one
        place randomness enters the codebooks; override it for a fixed choice."""
        if num_rows >= count:
            return torch.randperm(num_rows, device=device)[:count]
        return torch.randint(0, num_rows, (count,), device=device)

    def dropout_index(self):
        """index of the last active layer of this call: the grouped form of quantize dropout (one seed per call, shared by all groups), host only"""
        q = self.num_quantizers
        if not self.quantize_dropout:
            return q - 1
        seed = random.randint(0, int(1e7))
        k = random.Random(seed).randrange(self.quantize_dropout_cutoff_index, q)
        m = self.quantize_dropout_multiple_of
        if m != 1:
            k = -(-(k + 1) // m) * m - 1
        return min(k, q - 1)

    def _kmeans_init(self, resid, cb, E, Et, e2, q):
        """k-means initialisation of one layer on its residual [M, d]: start from sampled rows, `kmeans_iters` rounds of (assign, per-code mean; an
        empty cluster keeps its mean), then embed = means, cluster_size = the last round's counts, embed_avg = means * counts, initted = True"""
        M, C = resid.shape[0], self.codebook_size
        means = resid.index_select(0, self.sample_rows(M, C, resid.device)).unsqueeze(0).contiguous()       # [1, C, d]
        for it in range(self.kmeans_iters):
            ids = ops.rvq_encode(resid, means, *ops.rvq_pack(means))
            n, s = ops.rvq_code_stats(resid, ids[:, 0], C)
            last = it == self.kmeans_iters - 1
            ops.rvq_kmeans_update(means[0], n, s, *((cb.embed, cb.embed_avg, cb.cluster_size) if last else ()))
        cb.initted.fill_(True)
        E[q].copy_(means[0])                                     # this step's pre-update codebook of the layer, and its distance image
        Et1, e21 = ops.rvq_pack(E[q:q + 1])
        Et[q].copy_(Et1[0]), e2[q].copy_(e21[0])

    def train_step(self, x2, k):
        """x2 fp32 [M, dim], k = last active layer -> (out [M, dim], losses [g, Q], idx [g, M, Q] (-1 on dropped layers), per group the pre-update
        codebooks [Q, C, d]).  Updates the codebook buffers in place."""
        M, dim = x2.shape
        dg, Q, C = dim // self.groups, self.num_quantizers, self.codebook_size
        dev = x2.device
        for r in self.rvqs:
            cb = r.layers[0]._codebook
            if cb.embed.dtype != F32 or not cb.embed.is_cuda:
                raise RuntimeError('train-mode GroupedResidualVQ needs fp32 codebook buffers on the GPU (no CPU fallback)')
        out = torch.zeros((M, dim), dtype=F32, device=dev)
        idx = torch.full((self.groups, M, Q), -1, dtype=torch.int64, device=dev)
        losses = torch.zeros((self.groups, Q), dtype=F32, device=dev)
        initted = self._initted()
        thr = float(self.threshold_ema_dead_code)
        snaps = []
        for gi, (E, Et, e2) in enumerate(self._pack(require_init=False)):
            xg, og = x2[:, gi * dg:(gi + 1) * dg], out[:, gi * dg:(gi + 1) * dg]
            layers = self.rvqs[gi].layers
            resid = torch.empty((M, dg), dtype=F32, device=dev)
            resid.copy_(xg)
            n_all = torch.empty((k + 1, C), dtype=F32, device=dev)
            s_all = torch.empty((k + 1, C, dg), dtype=F32, device=dev)
            for q in range(k + 1):
                if not initted[gi][q]:
                    self._kmeans_init(resid, layers[q]._codebook, E, Et, e2, q)
                ops.rvq_encode(resid, E[q:q + 1], Et[q:q + 1], e2[q:q + 1], idx_out=idx[gi][:, q:q + 1])
                ops.rvq_code_stats(resid, idx[gi][:, q], C, n_all[q], s_all[q])                      # of THIS layer's input residual
                ops.rvq_train_quantize(resid, idx[gi][:, q], E[q], og, losses[gi, q:q + 1], self.commitment_weight / (M * dg), self.rotation_trick)
            # EMA updates and expiries after the layer loop (neither influences a later layer of the same step)
            dead = torch.empty((k + 1, 1 + C), dtype=torch.int32, device=dev)
            for q in range(k + 1):
                cb = layers[q]._codebook
                ops.rvq_ema_update(cb.cluster_size, cb.embed_avg, cb.embed, n_all[q], s_all[q], self.decay, self.eps, thr, dead[q])
            if thr > 0:
                counts = dead[:, 0].tolist()                     # the ONE host read per group and step: the dead-code counts size the row sampling
                for q, cnt in enumerate(counts):
                    if cnt:
                        cb = layers[q]._codebook
                        ops.rvq_expire(dead[q, 1:], cnt, self.sample_rows(M, cnt, dev).to(torch.int64).contiguous(), xg, idx[gi], E, q, self.rotation_trick, thr,
                                       cb.cluster_size, cb.embed_avg, cb.embed)
            snaps.append(E)
        self._packed = None                                      # the kernels write through raw pointers: no tensor version moved
        return out, losses, idx, snaps

    def _forward_train(self, x):
        if torch.distributed.is_available() and torch.distributed.is_initialized() and torch.distributed.get_world_size() > 1:
            raise NotImplementedError('train-mode GroupedResidualVQ is single-process: the all-reduce of the per-code statistics (cluster sizes, embedding '
                                      'sums) and the distributed k-means initialisation are not implemented')
        if not x.is_cuda:
            raise RuntimeError('audiolm_pytorch_amd.SoundStream runs on the MI355X only (no CPU fallback)')
        b, n, dim = x.shape
        x2 = x.reshape(b * n, dim).to(F32).contiguous()
        k = self.dropout_index()
        if codec_bwd.wants_grad(self, x2):
            out, losses, idx = codec_bwd.RvqTrainFn.apply(x2, self, k)
        else:
            out, losses, idx, _ = self.train_step(x2.detach(), k)
        return out.view(b, n, dim), idx.view(self.groups, b, n, self.num_quantizers), losses

    def forward(self, x):
        """x fp32 (b, n, dim) -> (quantized (b, n, dim), indices (g, b, n, q) int64, commit_loss (g, q): zeros in eval mode)."""
        if self.training:
            return self._forward_train(x)
        b, n, dim = x.shape
        x2 = x.reshape(b * n, dim).to(F32).contiguous()
        dg = dim // self.groups
        quant = torch.empty_like(x2)
        idx = torch.empty((self.groups, b * n, self.num_quantizers), dtype=torch.int64, device=x.device)
        for g, (E, Et, e2) in enumerate(self._pack()):
            ops.rvq_encode(x2[:, g * dg:(g + 1) * dg], E, Et, e2, idx_out=idx[g], quant_out=quant[:, g * dg:(g + 1) * dg])
        return quant.view(b, n, dim), idx.view(self.groups, b, n, self.num_quantizers), torch.zeros((self.groups, self.num_quantizers), device=x.device)


    @torch.no_grad()
    def get_output_from_indices(self, indices):
        """indices int (g, b, n, q) (-1 = no code) -> (b, n, dim): per group the sum of the selected code vectors (alm_rvq_decode)."""
        g, b, n, q = indices.shape
        assert g == self.groups and q <= self.num_quantizers
        dg = self.dim // self.groups
        out = torch.empty((b * n, self.dim), dtype=F32, device=indices.device)
        idx = indices.to(torch.int64).reshape(g, b * n, q).contiguous()
        for gi, (E, _, _) in enumerate(self._pack()):
            ops.rvq_decode(idx[gi], E[:q].contiguous(), out[:, gi * dg:(gi + 1) * dg])
        return out.view(b, n, self.dim)


class _GroupedProjQuant(nn.Module):
    """What GroupedResidualFSQ and GroupedResidualLFQ share (csrc/proj_quant.hpp is the kernels' side of it): per group a projection to `proj_dim`
    dimensions, Q layers of a per-dimension residual chain, a projection back.  rvqs.{g}.project_in / project_out are nn.Linear, or nn.Identity when
    dim / groups == proj_dim.  Quantize dropout (training mode only) is GroupedResidualVQ.dropout_index.  A subclass builds `rvqs` and supplies
    `run` and `decode_group`, its per-group kernel calls."""

    def __init__(self, *, dim, groups, num_quantizers, proj_dim, proj_dim_name, limits, quantize_dropout, quantize_dropout_cutoff_index,
                 quantize_dropout_multiple_of):
        super().__init__()
        assert dim % groups == 0 and num_quantizers >= 1
        assert quantize_dropout_cutoff_index >= 0 and quantize_dropout_multiple_of >= 1
        for what, v, limit in zip((proj_dim_name, 'dim / groups', 'num_quantizers'), (proj_dim, dim // groups, num_quantizers), limits):
            if v > limit:
                raise NotImplementedError(f'{type(self).__name__}: {what} = {v} exceeds the kernels\' limit of {limit}')
        self.dim, self.groups, self.num_quantizers, self.proj_dim = dim, groups, num_quantizers, proj_dim
        self.quantize_dropout = quantize_dropout and num_quantizers > 1
        self.quantize_dropout_cutoff_index, self.quantize_dropout_multiple_of = quantize_dropout_cutoff_index, quantize_dropout_multiple_of

    dropout_index = GroupedResidualVQ.dropout_index

    def group_params(self, g):
        """[project_in.weight, project_in.bias, project_out.weight, project_out.bias] of group g, or [] in the identity case"""
        r = self.rvqs[g]
        return [] if isinstance(r.project_in, nn.Identity) else [r.project_in.weight, r.project_in.bias, r.project_out.weight, r.project_out.bias]

    def all_params(self):
        return [p for g in range(self.groups) for p in self.group_params(g)]

    @staticmethod
    def kernel_weights(params):
        return tuple(p.detach().to(F32).contiguous() for p in params) if params else None

    def groups_of(self, x2):
        """x2 fp32 [M, dim] -> (out [M, dim], idx int64 [g, M, Q], per group (its columns, its kernel weights)): what `run` fills"""
        M, dim = x2.shape
        dg = dim // self.groups
        out = torch.empty((M, dim), dtype=F32, device=x2.device)
        idx = torch.empty((self.groups, M, self.num_quantizers), dtype=torch.int64, device=x2.device)
        return out, idx, [(slice(g * dg, (g + 1) * dg), self.kernel_weights(self.group_params(g))) for g in range(self.groups)]

    def flatten(self, x):
        """x (b, n, dim) -> (x2 fp32 [b n, dim], k = the last active layer of this call)"""
        if not x.is_cuda:
            raise RuntimeError('audiolm_pytorch_amd.SoundStream runs on the MI355X only (no CPU fallback)')
        b, n, dim = x.shape
        assert dim == self.dim
        return x.reshape(b * n, dim).to(F32).contiguous(), self.dropout_index() if self.training else self.num_quantizers - 1

    @torch.no_grad()
    def get_output_from_indices(self, indices):
        """indices int (g, b, n, q <= Q) (-1 = no code) -> (b, n, dim): per group project_out of the summed codes (alm_fsq_decode / alm_lfq_decode)"""
        g, b, n, q = indices.shape
        assert g == self.groups and 1 <= q <= self.num_quantizers
        if not indices.is_cuda:
            raise RuntimeError('audiolm_pytorch_amd.SoundStream runs on the MI355X only (no CPU fallback)')
        dg = self.dim // self.groups
        out = torch.empty((b * n, self.dim), dtype=F32, device=indices.device)
        idx = indices.to(torch.int64).reshape(g, b * n, q).contiguous()
        for gi in range(g):
            self.decode_group(idx[gi], self.kernel_weights(self.group_params(gi)), out[:, gi * dg:(gi + 1) * dg])
        return out.view(b, n, self.dim)


class _ResidualFSQ(nn.Module):
    def __init__(self, dim, codebook_dim):
        super().__init__()
        self.project_in = nn.Linear(dim, codebook_dim) if dim != codebook_dim else nn.Identity()
        self.project_out = nn.Linear(codebook_dim, dim) if dim != codebook_dim else nn.Identity()


class GroupedResidualFSQ(_GroupedProjQuant):
    """Residual finite scalar quantization (arXiv 2309.15505) in the grouped form of vector-quantize-pytorch's GroupedResidualFSQ, as the reference
    builds it (soundstream.py:578-586).  The arithmetic is RESTATED from the paper's Appendix A and the package's residual form (tests/fsq_restated.py;
    parity with the installed package is unpinned, like LocalMHA): per group a projection to len(levels) dimensions, Q layers of bounded rounding of
    the scaled residual, a projection back.  No codebook state, no auxiliary loss: one alm_fsq_fwd launch per group, alm_fsq_decode for
    `get_output_from_indices`, and in training mode with a graph wanted codec_bwd.FsqFn (alm_fsq_bwd)."""

    def __init__(self, *, dim, levels, num_quantizers, groups=1, quantize_dropout=True, quantize_dropout_cutoff_index=1, quantize_dropout_multiple_of=1):
        levels = [int(l) for l in levels]
        assert len(levels) >= 1 and all(l >= 2 for l in levels)
        super().__init__(dim=dim, groups=groups, num_quantizers=num_quantizers, proj_dim=len(levels), proj_dim_name='len(levels)',
                         limits=(ops.FSQ_MAX_LEVELS, ops.FSQ_MAX_DIM, ops.FSQ_MAX_QUANTIZERS), quantize_dropout=quantize_dropout,
                         quantize_dropout_cutoff_index=quantize_dropout_cutoff_index, quantize_dropout_multiple_of=quantize_dropout_multiple_of)
        self.codebook_size = functools.reduce(lambda a, b: a * b, levels)
        if self.codebook_size > 1 << 24:
            raise NotImplementedError(f'GroupedResidualFSQ: codebook_size = prod(levels) = {self.codebook_size} exceeds 2^24 (the index basis is fp32)')
        self.levels = levels
        self.rvqs = nn.ModuleList([_ResidualFSQ(dim // groups, len(levels)) for _ in range(groups)])
        self.constants = ops.fsq_constants(levels, num_quantizers)           # host table (fp32, CPU); a plain attribute: the state_dict has no entry for it
        self._constants_on = {}

    def _consts(self, device):
        if device not in self._constants_on:
            self._constants_on[device] = self.constants.to(device)
        return self._constants_on[device]

    def run(self, x2, k, save_z=False):
        """x2 fp32 [M, dim], k = last active layer -> (out [M, dim], idx int64 [g, M, Q] (-1 past k), per group z [M, d] or None)"""
        out, idx, groups = self.groups_of(x2)
        consts = self._consts(x2.device)
        zs = [ops.fsq_fwd(x2[:, sl], weights, consts, self.proj_dim, self.num_quantizers, k, idx[g], out[:, sl], save_z=save_z and weights is not None)
              for g, (sl, weights) in enumerate(groups)]
        return out, idx, zs

    def forward(self, x):
        """x fp32 (b, n, dim) -> (quantized (b, n, dim), indices (g, b, n, q) int64; -1 on the layers quantize dropout left out)"""
        x2, k = self.flatten(x)
        if codec_bwd.wants_grad(self, x2):
            out, idx = codec_bwd.FsqFn.apply(x2, self, k, *self.all_params())
        else:
            out, idx, _ = self.run(x2.detach(), k)
        return out.view(x.shape), idx.view(self.groups, *x.shape[:2], self.num_quantizers)

    def decode_group(self, idx, weights, out):
        ops.fsq_decode(idx, weights, self._consts(idx.device), self.proj_dim, self.num_quantizers, out)


class _LFQLayer(nn.Module):
    def __init__(self, codebook_bits):
        super().__init__()
        self.register_buffer('mask', 2 ** torch.arange(codebook_bits - 1, -1, -1, dtype=torch.int64))


class _ResidualLFQ(nn.Module):
    def __init__(self, dim, codebook_bits, num_quantizers):
        super().__init__()
        self.project_in = nn.Linear(dim, codebook_bits) if dim != codebook_bits else nn.Identity()
        self.project_out = nn.Linear(codebook_bits, dim) if dim != codebook_bits else nn.Identity()
        self.layers = nn.ModuleList([_LFQLayer(codebook_bits) for _ in range(num_quantizers)])


class GroupedResidualLFQ(_GroupedProjQuant):
    """Residual lookup-free quantization (arXiv 2310.05737) in the grouped form of vector-quantize-pytorch's GroupedResidualLFQ, as the reference
    builds it (soundstream.py:563-571).  The arithmetic is RESTATED from the paper and the package's residual form (tests/lfq_restated.py; parity with
    the installed package is unpinned, like FSQ and LocalMHA): per group a projection to d = log2(codebook_size) dimensions, Q layers of sign
    quantization of the residual at scale 2^-q, a projection back.  No codebook state; in training mode every active layer carries the entropy loss
    (per-sample entropy minus diversity_gamma times the entropy of the batch's mean code distribution, over all 2^d codes) and the optional
    commitment loss: alm_lfq_fwd per group, alm_lfq_decode for `get_output_from_indices`, and with a graph wanted codec_bwd.LfqFn (alm_lfq_bwd).
    rvqs.{g}.layers.{q}.mask is the package's per-layer buffer (2^(d-1) .. 1, int64)."""

    def __init__(self, *, dim, num_quantizers, codebook_size, groups=1, quantize_dropout=True, quantize_dropout_cutoff_index=1,
                 quantize_dropout_multiple_of=1, entropy_loss_weight=0.1, commitment_loss_weight=0., diversity_gamma=1.):
        codebook_size = int(codebook_size)
        assert codebook_size >= 2 and codebook_size & (codebook_size - 1) == 0, f'codebook_size = {codebook_size} must be a power of two >= 2'
        d = codebook_size.bit_length() - 1
        super().__init__(dim=dim, groups=groups, num_quantizers=num_quantizers, proj_dim=d, proj_dim_name='log2(codebook_size)',
                         limits=(ops.LFQ_MAX_CODEBOOK_BITS, ops.LFQ_MAX_DIM, ops.LFQ_MAX_QUANTIZERS), quantize_dropout=quantize_dropout,
                         quantize_dropout_cutoff_index=quantize_dropout_cutoff_index, quantize_dropout_multiple_of=quantize_dropout_multiple_of)
        self.codebook_size, self.codebook_bits = codebook_size, d
        self.entropy_loss_weight, self.commitment_loss_weight, self.diversity_gamma = float(entropy_loss_weight), float(commitment_loss_weight), float(diversity_gamma)
        self.inv_temperature = ops.LFQ_INV_TEMPERATURE
        self.rvqs = nn.ModuleList([_ResidualLFQ(dim // groups, d, num_quantizers) for _ in range(groups)])

    @property
    def loss_cfg(self):
        return (self.inv_temperature, self.entropy_loss_weight, self.commitment_loss_weight, self.diversity_gamma)

    def run(self, x2, k, with_losses=False):
        """x2 fp32 [M, dim], k = last active layer -> (out [M, dim], idx int64 [g, M, Q] (-1 past k), losses [g, Q] (zeros without with_losses),
        per group (z [M, d] float64, avg [Q, 2^d] float64) or None)"""
        out, idx, groups = self.groups_of(x2)
        losses, saved = [], []
        for g, (sl, weights) in enumerate(groups):
            z, l, avg = ops.lfq_fwd(x2[:, sl], weights, self.proj_dim, self.num_quantizers, k, idx[g], out[:, sl],
                                    loss_cfg=self.loss_cfg if with_losses else None)
            losses.append(l)
            saved.append((z, avg) if with_losses else None)
        losses = torch.stack(losses) if with_losses else torch.zeros((self.groups, self.num_quantizers), dtype=F32, device=x2.device)
        return out, idx, losses, saved

    def forward(self, x):
        """x fp32 (b, n, dim) -> (quantized (b, n, dim), indices (g, b, n, q) int64; -1 on the layers quantize dropout left out, losses (g, q):
        zeros in eval mode and on the layers left out)"""
        if x.is_cuda and self.training and torch.distributed.is_available() and torch.distributed.is_initialized() and torch.distributed.get_world_size() > 1:
            raise NotImplementedError('train-mode GroupedResidualLFQ is single-process: the all-reduce of the mean code distribution (the diversity '
                                      'term of the entropy loss) is not implemented')
        x2, k = self.flatten(x)
        if self.training and codec_bwd.wants_grad(self, x2):
            out, idx, losses = codec_bwd.LfqFn.apply(x2, self, k, *self.all_params())
        else:
            out, idx, losses, _ = self.run(x2.detach(), k, with_losses=self.training)
        return out.view(x.shape), idx.view(self.groups, *x.shape[:2], self.num_quantizers), losses

    def decode_group(self, idx, weights, out):
        ops.lfq_decode(idx, weights, self.proj_dim, self.num_quantizers, out)


# ---------------------------------------------------------------------------------------------- LocalTransformer (soundstream.py:397-440)

_NO_ATTN_BWD = ('training-mode LocalTransformer backward exists for attn_dim_head 32 and 64 with attn_window_size <= 256 (dim_head 64: <= 160) only; got '
                'dim_head {} / window {} (call eval(), or construct the SoundStream with use_local_attn=False)')


def _btc(x, grad):
    """'b c n -> b n c' (or back); grad: the caller builds a graph (codec_bwd.wants_grad)"""
    return codec_bwd.BctToBtcFn.apply(x) if grad and x.requires_grad else ops.bct_to_btc(x)


class _Linear1x1:
    """an nn.Linear applied along the channel axis of [B, C, T] = a k = 1 conv on the exact-fp32 MFMA kernel; packed weight cached per version"""

    def __init__(self):
        self._packed = None
        self._packed_t = codec_bwd._ImageCache()                  # transposed image for the input gradient (training mode only)

    def packed_t(self, lin):
        w = lin.weight
        return self._packed_t.get((w,), lambda: ops.conv1d_pack_t(w.detach().to(F32).unsqueeze(-1).contiguous()))

    def __call__(self, lin, x, residual=None):
        w, b = lin.weight, lin.bias
        ver = (w.data_ptr(), core.tensor_version(w), None if b is None else core.tensor_version(b))
        if self._packed is None or self._packed[0] != ver:
            bias = b.detach().to(F32).contiguous() if b is not None else torch.zeros(w.shape[0], dtype=F32, device=w.device)
            self._packed = (ver, ops.conv1d_pack(w.detach().to(F32).unsqueeze(-1).contiguous()), bias)
        return ops.conv1d_causal(x, self._packed[1], self._packed[2], w.shape[0], 1, residual=residual)


class _SinusoidalEmbeddings(nn.Module):                          # local-attention rotary.py (holder of the `inv_freq` buffer)
    def __init__(self, dim, scale_base, theta=10000):
        super().__init__()
        self.register_buffer('inv_freq', 1. / (theta ** (torch.arange(0, dim, 2).float() / dim)))
        self.dim, self.scale_base = dim, scale_base

    def tables(self, slots, device):
        """rotary angle cos / sin and the xpos scale for slots 0 .. slots-1 of the (look-back | own) window pair, fp32 [slots, dim] each,
        computed on the host exactly like the library does (t * inv_freq, scale ** ((t - slots // 2) / scale_base))"""
        inv = self.inv_freq.detach().float().cpu()
        t = torch.arange(slots).float()
        freqs = torch.einsum('i,j->ij', t, inv)
        freqs = torch.cat((freqs, freqs), dim=-1)
        base = (torch.arange(0, self.dim, 2) + 0.4 * self.dim) / (1.4 * self.dim)
        scale = base ** ((t - (slots // 2)) / self.scale_base)[:, None]
        scale = torch.cat((scale, scale), dim=-1)
        return tuple(x.float().contiguous().to(device) for x in (freqs.cos(), freqs.sin(), scale))


class _LocalAttention(nn.Module):
    def __init__(self, dim_head, window_size, xpos_scale_base):
        super().__init__()
        self.rel_pos = _SinusoidalEmbeddings(dim_head, scale_base=xpos_scale_base if xpos_scale_base is not None else window_size // 2)


class LocalMHA(nn.Module):
    """local-attention's LocalMHA in the one configuration the reference builds (soundstream.py:418-427): prenorm LayerNorm, causal, look-back of
    one window with the exact window size, qk_rmsnorm (attention scale 8), rotary + xpos, per-head sigmoid value gates."""

    def __init__(self, *, dim, window_size, dim_head=64, heads=8, xpos_scale_base=None, qk_scale=8):
        super().__init__()
        inner = dim_head * heads
        self.norm = nn.LayerNorm(dim)
        self.heads, self.dim_head, self.window_size, self.qk_scale = heads, dim_head, window_size, qk_scale
        self.to_qkv = nn.Linear(dim, inner * 3, bias=False)
        self.q_scale = nn.Parameter(torch.ones(dim_head))
        self.k_scale = nn.Parameter(torch.ones(dim_head))
        self.attn_fn = _LocalAttention(dim_head, window_size, xpos_scale_base)
        self.to_v_gate = nn.Sequential(nn.Linear(dim, heads))
        self.to_out = nn.Linear(inner, dim, bias=False)
        self._lin = [_Linear1x1() for _ in range(3)]
        self._tables = None

    def tables(self, device):
        inv = self.attn_fn.rel_pos.inv_freq
        key = (inv.data_ptr(), core.tensor_version(inv), device)
        if self._tables is None or self._tables[0] != key:
            self._tables = (key, self.attn_fn.rel_pos.tables(2 * self.window_size, device))
        return self._tables[1]

    def launches(self, x, add_residual=True):
        """(LN(x), qkv, gates, gated attention output, attn(x) (+ x)): the forward launches, shared by the eval path and the autograd Function"""
        cos_t, sin_t, xpos_t = self.tables(x.device)
        xn = ops.layernorm_bct(x, self.norm.weight.detach(), self.norm.bias.detach(), self.norm.eps)
        qkv = self._lin[0](self.to_qkv, xn)
        gates = self._lin[1](self.to_v_gate[0], xn)                      # from the NORMED input (LocalMHA.forward re-binds x)
        o = ops.local_attn(qkv, self.q_scale.detach(), self.k_scale.detach(), cos_t, sin_t, xpos_t, gates, self.heads, self.dim_head,
                           self.window_size, self.qk_scale)
        return xn, qkv, gates, o, self._lin[2](self.to_out, o, residual=x if add_residual else None)

    def backward_supported(self):
        return ops.local_attn_bwd_supported(self.dim_head, self.window_size)

    def run(self, x, add_residual=True):
        """x fp32 [B, dim, T] -> attn(x) (+ x), same layout"""
        return self.launches(x, add_residual)[-1]

    def call(self, x, add_residual=True):
        """run(), or its autograd Function in training mode with grad mode on and something that requires grad"""
        if codec_bwd.wants_grad(self, x):
            if not self.backward_supported():
                raise NotImplementedError(_NO_ATTN_BWD.format(self.dim_head, self.window_size))
            return codec_bwd.LocalMHAFn.apply(x, self.norm.weight, self.norm.bias, self.to_qkv.weight, self.q_scale, self.k_scale,
                                              self.to_v_gate[0].weight, self.to_v_gate[0].bias, self.to_out.weight, self, add_residual)
        return self.run(x, add_residual)

    def forward(self, x):
        """reference layout: x (b, n, dim) -> attention output WITHOUT the residual (the caller adds it, soundstream.py:437)"""
        grad = codec_bwd.wants_grad(self, x)
        return _btc(self.call(_btc(x.to(F32).contiguous(), grad), add_residual=False), grad)             # (n, c) -> (c, n) and back


class _GEGLU(nn.Module):
    def forward(self, x):
        raise NotImplementedError('runs fused inside LocalTransformer (csrc/local_attn.hip alm_geglu_bct)')


def _local_feed_forward(dim, mult=4):                                # local_attention.transformer.FeedForward: same Sequential indices
    inner = int(dim * mult * 2 / 3)
    return nn.Sequential(nn.LayerNorm(dim), nn.Linear(dim, inner * 2, bias=False), _GEGLU(), nn.Dropout(0.), nn.Linear(inner, dim, bias=False))


class LocalTransformer(nn.Module):
    def __init__(self, *, dim, depth, heads, window_size, dynamic_pos_bias=False, **kwargs):
        super().__init__()
        if dynamic_pos_bias:
            raise NotImplementedError('attn_dynamic_pos_bias=True (DynamicPositionBias instead of rotary) is not implemented (reference default False)')
        kwargs.pop('prenorm', None), kwargs.pop('causal', None)           # always True in the reference (soundstream.py:541-542)
        self.window_size = window_size
        self.pos_bias = None
        self.layers = nn.ModuleList([nn.ModuleList([LocalMHA(dim=dim, heads=heads, window_size=window_size, **kwargs), _local_feed_forward(dim)])
                                     for _ in range(depth)])
        self._ff_lin = [[_Linear1x1(), _Linear1x1()] for _ in range(depth)]

    def backward_supported(self):
        return all(attn.backward_supported() for attn, _ in self.layers)

    def check_backward(self, *tensors):
        """raises, before any launch, when a graph would be built (codec_bwd.wants_grad) for a geometry that has no backward kernel"""
        if codec_bwd.wants_grad(self, *tensors) and not self.backward_supported():
            attn = self.layers[0][0]
            raise NotImplementedError(_NO_ATTN_BWD.format(attn.dim_head, attn.window_size))

    def run_bct(self, x):
        """x fp32 [B, dim, T] (codec layout) -> same: x = attn(x) + x; x = ff(x) + x per layer (soundstream.py:436-438).  In training mode with grad
        mode on and an input or parameter that requires grad, each half is one autograd Function over the same launches (codec_bwd.py)."""
        self.check_backward(x)
        for (attn, ff), lins in zip(self.layers, self._ff_lin):
            x = attn.call(x)
            if codec_bwd.wants_grad(ff, x):
                x = codec_bwd.LocalFeedForwardFn.apply(x, ff[0].weight, ff[0].bias, ff[1].weight, ff[4].weight, ff, lins)
            else:
                x = codec_bwd.ff_launches(ff, lins, x)[-1]
        return x

    def forward(self, x):
        """x (b, n, dim) -> (b, n, dim)"""
        if not x.is_cuda:
            raise RuntimeError('audiolm_pytorch_amd.SoundStream runs on the MI355X only (no CPU fallback)')
        grad = codec_bwd.wants_grad(self, x)
        return _btc(self.run_bct(_btc(x.to(F32).contiguous(), grad)), grad)


class FiLM(nn.Module):                                           # soundstream.py:442-449
    """x * gamma + beta with (gamma | beta) = to_cond(cond), cond = [is_denoising, not is_denoising]: alm_film_fwd / alm_film_bwd (gamma and beta
    are formed in the kernel from to_cond's weight and bias)"""

    def __init__(self, dim, dim_cond=2):
        super().__init__()
        if dim_cond != 2:
            raise NotImplementedError('FiLM: only the reference\'s dim_cond=2 (the denoising switch) is implemented')
        self.to_cond = nn.Linear(dim_cond, dim * 2)

    def forward(self, x, cond):
        """x fp32 (b, n, dim), cond = a pair of floats -> same shape"""
        if not x.is_cuda:
            raise RuntimeError('audiolm_pytorch_amd.SoundStream runs on the MI355X only (no CPU fallback)')
        x = x.to(F32).contiguous()
        cond = (float(cond[0]), float(cond[1]))
        if codec_bwd.wants_grad(self, x):
            return codec_bwd.FiLMFn.apply(x, self.to_cond.weight, self.to_cond.bias, cond)
        return ops.film_fwd(x, self.to_cond.weight.detach().to(F32).contiguous(), self.to_cond.bias.detach().to(F32).contiguous(), *cond)


def curtail_to_multiple(t, mult, from_left=False):               # soundstream.py:86-90
    data_len = t.shape[-1]
    rounded = (data_len // mult) * mult
    return t[..., :rounded] if not from_left else t[..., -rounded:]


class SoundStream(nn.Module):
    """Constructor keywords and defaults follow the reference (soundstream.py:451-510); options outside the tokenize path raise.  The training losses
    are opt-in switches of this port: `with_discriminators=True` (wave discriminators and loss branches), on top of it `stft_discriminator=True`,
    `with_mel_loss=True` and `with_grad_penalty=True` (lets `forward(..., return_discr_loss=True, apply_grad_penalty=True)` add the reference's
    gradient penalties; registers no parameter, buffer or child module, so the state_dict is the same with and without it) and, independent of
    those, `with_film=True` (registers the reference's `encoder_film` / `decoder_film` and lets `forward(..., target=, is_denoising=)` apply them;
    without discriminators together with a codec-only return: the inference use of the denoiser)."""

    def __init__(self, *, channels=32, strides=(2, 4, 5, 8), channel_mults=(2, 4, 8, 16), codebook_dim=512, codebook_size=None,
                 finite_scalar_quantizer_levels=None, rq_num_quantizers=8, rq_commitment_weight=1., rq_ema_decay=0.95,
                 rq_quantize_dropout_multiple_of=1, rq_groups=1, rq_stochastic_sample_codes=False, rq_rotation_trick=True, rq_kwargs: dict = {},
                 use_lookup_free_quantizer=False, use_finite_scalar_quantizer=False, input_channels=1, discr_multi_scales=(1, 0.5, 0.25),
                 enc_cycle_dilations=(1, 3, 9), recon_loss_weight=1., multi_spectral_recon_loss_weight=1e-5, adversarial_loss_weight=1.,
                 feature_loss_weight=100, target_sample_hz=16000, use_local_attn=True, attn_window_size=128, attn_dim_head=64, attn_heads=8, attn_depth=1,
                 attn_xpos_scale_base=None, attn_dynamic_pos_bias=False, use_gate_loop_layers=False, squeeze_excite=False, pad_mode='reflect',
                 stft_discriminator=None, with_discriminators=False, stft_normalized=False, complex_stft_discr_logits_abs=True,
                 complex_stft_discr_kwargs: dict = {}, with_mel_loss=False, multi_spectral_window_powers_of_two=tuple(range(6, 12)),
                 multi_spectral_n_ffts=512, multi_spectral_n_mels=64, with_grad_penalty=False, with_film=False, with_lfq=False, with_gate_loop=False,
                 **kwargs):
        super().__init__()
        assert not (use_lookup_free_quantizer and use_finite_scalar_quantizer)                       # soundstream.py:555
        if use_lookup_free_quantizer and not with_lfq:
            raise NotImplementedError('the lookup-free quantizer (LFQ, use_lookup_free_quantizer=True) is opt-in in this port: pass with_lfq=True '
                                      '(GroupedResidualLFQ; its arithmetic is restated from the paper, parity with the installed package is unpinned)')
        if use_gate_loop_layers and not with_gate_loop:
            raise NotImplementedError('the gate-loop layers (use_gate_loop_layers=True) are opt-in in this port: pass with_gate_loop=True '
                                      '(GateLoopBlock; the layer\'s arithmetic is restated, parity with the gateloop_transformer package is unpinned)')
        if rq_stochastic_sample_codes:
            raise NotImplementedError('stochastic code sampling (rq_stochastic_sample_codes=True) is not implemented (reference default False)')
        self.use_lookup_free_quantizer = bool(use_lookup_free_quantizer)
        self.use_finite_scalar_quantizer = bool(use_finite_scalar_quantizer)
        if use_lookup_free_quantizer:                                                                # soundstream.py:561
            assert codebook_size is not None and finite_scalar_quantizer_levels is None, \
                'if use_finite_scalar_quantizer is set to False, `codebook_size` must be set (and not `finite_scalar_quantizer_levels`)'
        elif use_finite_scalar_quantizer:                                                            # soundstream.py:576
            assert codebook_size is None and finite_scalar_quantizer_levels is not None, \
                'if use_finite_scalar_quantizer is set to True, `finite_scalar_quantizer_levels` must be set (and not `codebook_size`). the effective ' \
                'codebook size is the cumulative product of all the FSQ levels'
        else:                                                                                        # soundstream.py:591
            assert codebook_size is not None and finite_scalar_quantizer_levels is None, \
                'if use_finite_scalar_quantizer is set to False, `codebook_size` must be set (and not `finite_scalar_quantizer_levels`)'
        self.target_sample_hz = target_sample_hz
        self.single_channel = input_channels == 1
        self.strides = strides
        layer_channels = (channels, *[m * channels for m in channel_mults])
        pairs = tuple(zip(layer_channels[:-1], layer_channels[1:]))
        # the gate-loop layers (soundstream.py:524-525, 620-621): one GateLoopBlock after every EncoderBlock (its chan_out) and DecoderBlock (its chan_in)
        self.use_gate_loop_layers = bool(use_gate_loop_layers)
        gate_loop = (lambda dim: (GateLoopBlock(dim),)) if self.use_gate_loop_layers else (lambda dim: ())
        blocks = [m for (ci, co), s in zip(pairs, strides)
                  for m in (EncoderBlock(ci, co, s, enc_cycle_dilations, squeeze_excite, pad_mode), *gate_loop(co))]
        self.encoder = nn.Sequential(CausalConv1d(input_channels, channels, 7, pad_mode=pad_mode), *blocks,
                                     CausalConv1d(layer_channels[-1], codebook_dim, 3, pad_mode=pad_mode))
        attn_kwargs = dict(dim=codebook_dim, dim_head=attn_dim_head, heads=attn_heads, depth=attn_depth, window_size=attn_window_size,
                           xpos_scale_base=attn_xpos_scale_base, dynamic_pos_bias=attn_dynamic_pos_bias, prenorm=True, causal=True)   # soundstream.py:533-543
        self.encoder_attn = LocalTransformer(**attn_kwargs) if use_local_attn else None
        self.decoder_attn = LocalTransformer(**attn_kwargs) if use_local_attn else None
        # the FiLM conditioners of the denoising variant (soundstream.py:547, 611) are opt-in: without `with_film=True` nothing is registered and
        # `is_denoising` raises, like before; with it a reference checkpoint's `encoder_film.*` / `decoder_film.*` load strictly
        self.with_film = bool(with_film)
        if self.with_film:
            self.encoder_film = FiLM(codebook_dim, dim_cond=2)
            self.decoder_film = FiLM(codebook_dim, dim_cond=2)
        dec_cycle_dilations = kwargs.pop('dec_cycle_dilations', (1, 3, 9))          # remaining kwargs: attention / discriminator / loss options of
                                                                                    # the parts that are not built here (ignored, like before)
        dblocks = [m for (ci, co), s in reversed(tuple(zip(pairs, strides)))
                   for m in (DecoderBlock(co, ci, s, dec_cycle_dilations, squeeze_excite, pad_mode), *gate_loop(ci))]
        self.decoder = nn.Sequential(CausalConv1d(codebook_dim, layer_channels[-1], 7, pad_mode=pad_mode), *dblocks,
                                     CausalConv1d(channels, input_channels, 7, pad_mode=pad_mode))             # soundstream.py:615-627
        self.num_quantizers = rq_num_quantizers
        self.codebook_dim = codebook_dim
        self.rq_groups = rq_groups
        if self.use_lookup_free_quantizer:                       # soundstream.py:563-573; of rq_kwargs the keys this quantizer takes, others by name
            taken = {'quantize_dropout_multiple_of', 'entropy_loss_weight', 'commitment_loss_weight', 'diversity_gamma'}
            unknown = sorted(set(rq_kwargs) - taken)
            if unknown:
                raise TypeError(f'GroupedResidualLFQ got an unexpected keyword argument {unknown[0]!r} (rq_kwargs: only '
                                f'{", ".join("`" + t + "`" for t in sorted(taken))} are implemented for the lookup-free quantizer)')
            self.rq = GroupedResidualLFQ(dim=codebook_dim, num_quantizers=rq_num_quantizers, codebook_size=codebook_size, groups=rq_groups,
                                         quantize_dropout=True, quantize_dropout_cutoff_index=kwargs.get('quantize_dropout_cutoff_index', 1), **rq_kwargs)
            self.codebook_size = codebook_size
        elif self.use_finite_scalar_quantizer:                   # soundstream.py:578-588; of rq_kwargs the one key this quantizer takes, others by name
            unknown = sorted(set(rq_kwargs) - {'quantize_dropout_multiple_of'})
            if unknown:
                raise TypeError(f'GroupedResidualFSQ got an unexpected keyword argument {unknown[0]!r} (rq_kwargs: only '
                                '`quantize_dropout_multiple_of` is implemented for the finite scalar quantizer)')
            self.rq = GroupedResidualFSQ(dim=codebook_dim, levels=finite_scalar_quantizer_levels, num_quantizers=rq_num_quantizers, groups=rq_groups,
                                         quantize_dropout=True, quantize_dropout_cutoff_index=kwargs.get('quantize_dropout_cutoff_index', 1), **rq_kwargs)
            self.codebook_size = self.rq.codebook_size
        else:
            self.codebook_size = codebook_size
            self.rq = GroupedResidualVQ(dim=codebook_dim, num_quantizers=rq_num_quantizers, codebook_size=codebook_size, groups=rq_groups,
                                        decay=rq_ema_decay, commitment_weight=rq_commitment_weight, quantize_dropout=True,
                                        quantize_dropout_cutoff_index=kwargs.get('quantize_dropout_cutoff_index', 1),
                                        quantize_dropout_multiple_of=rq_quantize_dropout_multiple_of, rotation_trick=rq_rotation_trick, kmeans_iters=10,
                                        threshold_ema_dead_code=2)                                       # soundstream.py:592-607 (rq_kwargs: ignored, like before)
        # the training losses (soundstream.py:629-679) are opt-in: without `with_discriminators=True` nothing below is registered and the loss
        # branches of forward raise, like before
        self.with_discriminators = bool(with_discriminators)
        self.discr_multi_scales = discr_multi_scales
        self.recon_loss_weight, self.multi_spectral_recon_loss_weight = recon_loss_weight, multi_spectral_recon_loss_weight
        self.adversarial_loss_weight, self.feature_loss_weight = adversarial_loss_weight, feature_loss_weight
        self._stft_discriminator_off = stft_discriminator is False
        if self.with_discriminators:
            self.discriminators = nn.ModuleList([D.MultiScaleDiscriminator() for _ in range(len(discr_multi_scales))])
            factors = [int(s1 / s2) for s1, s2 in zip(discr_multi_scales[:-1], discr_multi_scales[1:])]
            self.downsamples = nn.ModuleList([nn.Identity()] + [D.AvgPoolDownsample(f) for f in factors])
            if isinstance(stft_discriminator, nn.Module):
                self.stft_discriminator = stft_discriminator     # the caller's module, run as it is (a D.ComplexSTFTDiscriminator: on the HIP kernels)
            elif stft_discriminator is True:                     # the reference's default module (soundstream.py:638-643), native
                self.stft_discriminator = D.ComplexSTFTDiscriminator(stft_normalized=stft_normalized, logits_abs=complex_stft_discr_logits_abs,
                                                                     **complex_stft_discr_kwargs)
            elif stft_discriminator not in (None, False):
                raise TypeError('stft_discriminator: True (the native ComplexSTFTDiscriminator), an nn.Module with '
                                'forward(x, return_intermediates=False), False (train without one) or None')
        # the multi-spectral mel reconstruction loss (soundstream.py:645-672) is opt-in on top: without `with_mel_loss=True` nothing is registered,
        # the multi_spectral_* keywords are ignored and a positive weight makes the loss branches raise, like before
        self.with_mel_loss = bool(with_mel_loss)
        if self.with_mel_loss:
            if not self.with_discriminators:
                raise ValueError('with_mel_loss=True needs with_discriminators=True (the mel term is part of the generator loss)')
            powers = tuple(multi_spectral_window_powers_of_two)
            cast = lambda v: tuple(v) if isinstance(v, (tuple, list)) else (v,) * len(powers)
            n_ffts, n_mels = cast(multi_spectral_n_ffts), cast(multi_spectral_n_mels)
            if not len(n_ffts) == len(n_mels) == len(powers):
                raise ValueError('multi_spectral_n_ffts / multi_spectral_n_mels: one value, or one per entry of multi_spectral_window_powers_of_two')
            self.mel_spec_transforms = nn.ModuleList([])
            self.mel_spec_recon_alphas = []
            for power, n_fft, mels in zip(powers, n_ffts, n_mels):
                win_length = 2 ** power
                self.mel_spec_transforms.append(mel_loss.MelSpectrogram(sample_rate=target_sample_hz, n_fft=max(n_fft, win_length), win_length=win_length,
                                                                        hop_length=win_length // 4, n_mels=mels, normalized=stft_normalized))
                self.mel_spec_recon_alphas.append((win_length / 2) ** 0.5)
        # the gradient penalty (soundstream.py:883-898) is opt-in on top: a switch only, no parameter, buffer or child module; without it
        # `apply_grad_penalty=True` raises, like before
        self.with_grad_penalty = bool(with_grad_penalty)
        if self.with_grad_penalty and not self.with_discriminators:
            raise ValueError('with_grad_penalty=True needs with_discriminators=True (the penalty is part of the discriminator loss)')
        self.eval()

    @property
    def device(self):
        return next(self.parameters()).device

    def non_discr_parameters(self):                              # soundstream.py:760-769 (the FiLM conditioners: with `with_film=True` only)
        return [*self.encoder.parameters(), *self.decoder.parameters(),
                *(self.encoder_attn.parameters() if self.encoder_attn is not None else []),
                *(self.decoder_attn.parameters() if self.decoder_attn is not None else []),
                *(self.encoder_film.parameters() if self.with_film else []), *(self.decoder_film.parameters() if self.with_film else []),
                *self.rq.parameters()]

    @property
    def seq_len_multiple_of(self):                               # soundstream.py:772-774
        return functools.reduce(lambda x, y: x * y, self.strides)

    @property
    def downsample_factor(self):
        return self.seq_len_multiple_of

    def process_input(self, x, input_sample_hz=None, curtail_from_left=False):                   # soundstream.py:779-795
        lead = x.shape[:-1]
        x = x.reshape(-1, x.shape[-1])                           # pack([x], '* n')
        if input_sample_hz is not None:                          # torchaudio.functional.resample (resample.py; the same rate returns x itself)
            x = resample(x, input_sample_hz, self.target_sample_hz)
        x = curtail_to_multiple(x, self.seq_len_multiple_of, from_left=curtail_from_left)
        return x.unsqueeze(1), lead

    def encode(self, x):
        """(b, 1, n) fp32 -> (b, n / prod(strides), codebook_dim): the encoder stack + 'b c n -> b n c'."""
        if not x.is_cuda:
            raise RuntimeError('audiolm_pytorch_amd.SoundStream runs on the MI355X only (no CPU fallback)')
        h = x.to(F32).contiguous()
        if self.encoder_attn is not None:                        # a geometry without a backward kernel raises before any launch
            self.encoder_attn.check_backward(h, *self.encoder.parameters())
        for layer in self.encoder:
            if isinstance(layer, CausalConv1d):
                h = layer.call(h)
            elif isinstance(layer, Residual):                    # GateLoopBlock (use_gate_loop_layers=True)
                h = layer(h)
            else:
                for sub in layer:
                    h = sub(h) if isinstance(sub, _ResidualFn) else sub.call(h)
        if self.encoder_attn is not None:                        # :830-833 ('b c n -> b n c' first there; here the layout is kept)
            h = self.encoder_attn.run_bct(h)
        return codec_bwd.BctToBtcFn.apply(h) if h.requires_grad else ops.bct_to_btc(h)

    @torch.no_grad()
    def tokenize(self, audio):                                   # soundstream.py:797-800
        self.eval()
        return self.forward(audio, return_codes_only=True)

    def forward(self, x, target=None, is_denoising=None, return_encoded=False, return_codes_only=False, return_discr_loss=False,
                return_discr_losses_separately=False, return_loss_breakdown=False, return_recons_only=False, input_sample_hz=None,
                apply_grad_penalty=False, curtail_from_left=False):
        """The codec branches of soundstream.py:802-862 (same positional order): return_codes_only -> indices (g, b, n, q);
        return_encoded -> (quantized, indices 'b n (g q)', commit_loss (g, q)); return_recons_only -> the reconstructed wave.  In eval mode
        nothing is recorded for autograd and commit_loss is zero; in training mode the quantizer takes one training step (GroupedResidualVQ) and,
        with grad mode on, the results carry a graph through encoder, quantizer and decoder.  The loss branches (soundstream.py:868-995) need
        `with_discriminators=True` at construction and raise without it: return_discr_loss (with return_discr_losses_separately: the list of
        ('scale:{s}', loss) / ('stft', loss) pairs) works on the input and the detached reconstruction, with `apply_grad_penalty=True` (needs
        `with_grad_penalty=True` at construction) plus the reference's gradient penalties: 'stft_grad_penalty' in the total and in the package,
        'scale_grad_penalty:{s}' in the package only, labelled as the reference labels them; otherwise the generator's total loss (which ignores
        apply_grad_penalty), with
        return_loss_breakdown also (recon, multi_spectral, adversarial, feature, commitment).  `target=` replaces the input in the recon term."""
        codec_only = return_encoded or return_codes_only or return_recons_only
        denoising_args = (target is not None or is_denoising is not None) and not self.with_film        # with_film: the inference use of the denoiser
        if not self.with_discriminators and (denoising_args or return_discr_loss or return_discr_losses_separately
                                             or return_loss_breakdown or apply_grad_penalty or not codec_only):
            raise NotImplementedError('only forward(..., return_codes_only=True | return_encoded=True | return_recons_only=True) is implemented '
                                      'on a SoundStream built without with_discriminators=True (the training losses are opt-in)')
        if is_denoising is not None and not self.with_film:
            raise NotImplementedError('is_denoising (the FiLM conditioners of the denoising variant) is opt-in: construct the SoundStream with with_film=True')
        assert not (is_denoising is not None and target is None), '`is_denoising` needs `target` (soundstream.py:817)'
        denoise_input = None if is_denoising is None else (float(bool(is_denoising)), float(not is_denoising))     # [1, 0] denoise, [0, 1] not
        if not codec_only:
            self._check_loss_options(apply_grad_penalty)
        with torch.set_grad_enabled(torch.is_grad_enabled() and self.training):
            x, lead = self.process_input(x, input_sample_hz=input_sample_hz, curtail_from_left=curtail_from_left)
            if self._mel_term_on() and not codec_only and not return_discr_loss:
                for transform in self.mel_spec_transforms:       # a clip too short for a scale's reflect padding: by name, before the codec's launches
                    transform.check_length(x.shape[-1])
            feats = self.encode(x)
            if denoise_input is not None:                        # soundstream.py:835-837: after encoder_attn, before the quantizer
                feats = self.encoder_film(feats, denoise_input)
            if not self.use_finite_scalar_quantizer:
                quantized, indices, commit_loss = self.rq(feats)
            else:                                                # soundstream.py:841-845: the finite scalar quantizer has no auxiliary loss
                quantized, indices = self.rq(feats)
                commit_loss = torch.zeros((), dtype=F32, device=feats.device)
            if return_codes_only:
                return indices                                       # (g, b, n, q), soundstream.py:847-848
            b, n = indices.shape[1], indices.shape[2]
            if return_encoded:
                return quantized, indices.permute(1, 2, 0, 3).reshape(b, n, -1), commit_loss          # 'g b n q -> b n (g q)', :851
            if denoise_input is not None:                        # :854-855: after the quantizer, before decoder_attn (decode() itself never applies it)
                quantized = self.decoder_film(quantized, denoise_input)
            recon = self.decode(quantized)                           # :857-866, unpack(recon_x, ps, '* c n')
            if return_recons_only:
                return recon.reshape(*lead, recon.shape[-2], recon.shape[-1])
            orig_x = x.to(F32).contiguous()
            if return_discr_loss:
                return self._discr_loss(orig_x, recon.detach(), return_discr_losses_separately, apply_grad_penalty)
            if target is not None:
                target, _ = self.process_input(target, input_sample_hz=input_sample_hz, curtail_from_left=curtail_from_left)
            return self._generator_loss(orig_x, recon, orig_x if target is None else target.to(F32).contiguous(), commit_loss, return_loss_breakdown)

    def _check_loss_options(self, apply_grad_penalty):
        """the parts of the reference's losses that are not built, each by name, before any launch"""
        if self.multi_spectral_recon_loss_weight > 0 and not self.with_mel_loss:
            raise NotImplementedError('the multi-spectral mel-spectrogram reconstruction loss (torchaudio MelSpectrogram) is not constructed by default: '
                                      'pass with_mel_loss=True for the native one, or construct the SoundStream with multi_spectral_recon_loss_weight=0')
        if apply_grad_penalty and not self.with_grad_penalty:
            raise NotImplementedError('apply_grad_penalty=True (gradient penalty) needs a double backward through the discriminator kernels, which is '
                                      'opt-in: construct the SoundStream with with_grad_penalty=True')
        if getattr(self, 'stft_discriminator', None) is None and not self._stft_discriminator_off:
            raise NotImplementedError('the ComplexSTFTDiscriminator is not constructed by default: pass stft_discriminator=True for the native one, '
                                      'stft_discriminator=<an nn.Module with forward(x, return_intermediates=False)>, or stft_discriminator=False '
                                      'to train without one')

    def _mel_term_on(self):
        return self.with_mel_loss and self.multi_spectral_recon_loss_weight > 0

    def _scales(self, real, fake, leaves=None):
        """per wave discriminator (logits, intermediates) of real and fake run as ONE batch [real | fake] through the chain of downsamples.  With a
        list `leaves`, the wave handed to each discriminator is a fresh leaf that requires grad (appended to the list) for the gradient penalty; the
        chain of downsamples runs on the plain waves, so the pooling stays out of the penalty's graph."""
        b = real.shape[0]
        scaled = torch.cat((real, fake), dim=0)
        for discr, downsample in zip(self.discriminators, self.downsamples):
            scaled = downsample(scaled)
            wave = scaled
            if leaves is not None:
                wave = scaled.detach().requires_grad_()
                leaves.append(wave)
            logits, inter = discr(wave, return_intermediates=True)
            yield (logits[:b], logits[b:]), [(t[:b], t[b:]) for t in inter]

    @staticmethod
    def _penalty_pair(wave, loss, b):
        """(gradient_penalty(real, loss), gradient_penalty(fake, loss)) from ONE autograd.grad with respect to the batch [real | fake]: rows [:b] make
        the real penalty and rows [b:] the fake one, each a mean over its own b rows"""
        gradients = D.wave_gradients(wave, loss)
        return D.penalty_of_gradients(gradients[:b]), D.penalty_of_gradients(gradients[b:])

    def _stft(self, real, fake, return_intermediates):
        """(real, fake) outputs of the STFT discriminator: the native module takes ONE batch [real | fake] like `_scales` (every op is
        batch-independent); a caller's own module gets its two separate calls"""
        discr = self.stft_discriminator
        if not isinstance(discr, D.ComplexSTFTDiscriminator):
            if return_intermediates:
                return discr(real, return_intermediates=True), discr(fake, return_intermediates=True)
            return discr(real), discr(fake)
        b = real.shape[0]
        out = discr(torch.cat((real, fake), dim=0), return_intermediates=return_intermediates)
        if not return_intermediates:
            return out[:b], out[b:]
        logits, inter = out
        return (logits[:b], [t[:b] for t in inter]), (logits[b:], [t[b:] for t in inter])

    def _discr_loss(self, real, fake, separately, penalty=False):               # soundstream.py:870-925
        b = real.shape[0]
        stft_loss = stft_penalty = None
        if not self._stft_discriminator_off and self.single_channel:
            discr = self.stft_discriminator
            if not penalty:
                stft_real_logits, stft_fake_logits = self._stft(real, fake, False)
                stft_loss = D.hinge_discr_loss(stft_fake_logits, stft_real_logits)
            elif isinstance(discr, D.ComplexSTFTDiscriminator):
                wave = torch.cat((real, fake), dim=0).detach().requires_grad_()
                logits = discr(wave)
                stft_loss = D.hinge_discr_loss(logits[b:], logits[:b])
                penalty_real, penalty_fake = self._penalty_pair(wave, stft_loss, b)
                stft_penalty = penalty_real + penalty_fake
            else:                                                # a caller's own module: its two separate calls, torch's autograd through it
                real_leaf, fake_leaf = real.detach().clone().requires_grad_(), fake.detach().clone().requires_grad_()
                stft_loss = D.hinge_discr_loss(discr(fake_leaf), discr(real_leaf))
                stft_penalty = D.gradient_penalty(real_leaf, stft_loss) + D.gradient_penalty(fake_leaf, stft_loss)
        # the wave discriminators' penalties reach the result only in the package (the reference computes them and drops them from the total)
        leaves = [] if penalty and separately else None
        losses, penalties = [], []
        for (real_logits, fake_logits), _ in self._scales(real, fake, leaves):
            losses.append(D.hinge_discr_loss(fake_logits, real_logits))
            if leaves is not None:
                penalties.extend(self._penalty_pair(leaves[-1], losses[-1], b))           # real, then fake
        if not separately:
            total = torch.stack(losses).mean()
            if stft_loss is not None:
                total = total + stft_loss
            return total if stft_penalty is None else total + stft_penalty
        pkg = [(f'scale:{scale}', loss) for scale, loss in zip(self.discr_multi_scales, losses)]
        # The reference zips its scales with the FLAT list [real, fake] per scale (soundstream.py:917), so the labels pair the 3 scales with the first
        # 3 of 6 penalties: with the default scales 'scale_grad_penalty:1' is real at scale 1, 'scale_grad_penalty:0.5' is FAKE at scale 1 and
        # 'scale_grad_penalty:0.25' is REAL at scale 0.5.  Mirrored exactly: checkpoint and log comparisons against the reference depend on it.
        pkg.extend((f'scale_grad_penalty:{scale}', p) for scale, p in zip(self.discr_multi_scales, penalties))
        if stft_loss is not None:
            pkg.append(('stft', stft_loss))
        if stft_penalty is not None:
            pkg.append(('stft_grad_penalty', stft_penalty))
        return pkg

    def _generator_loss(self, real, fake, target, commit_loss, breakdown):      # soundstream.py:927-995
        recon_loss = D.mse_loss(target, fake)
        if self._mel_term_on():                                  # soundstream.py:937-945: from (orig_x, recon_x), never from `target`
            multi_spectral_recon_loss = mel_loss.multi_spectral_recon_loss(real, fake, self.mel_spec_transforms, self.mel_spec_recon_alphas)
        else:
            multi_spectral_recon_loss = torch.zeros((), dtype=F32, device=real.device)
        adversarial, pairs = [], []
        stft_fake_logits = None
        if not self._stft_discriminator_off:
            (_, stft_real_inter), (stft_fake_logits, stft_fake_inter) = self._stft(real, fake, True)
            pairs.extend(zip(stft_real_inter, stft_fake_inter))
        for (_, fake_logits), inter in self._scales(real, fake):
            adversarial.append(D.hinge_gen_loss(fake_logits))
            pairs.extend(inter)
        feature_loss = torch.stack([D.l1_loss(r, f) for r, f in pairs]).mean()
        if stft_fake_logits is not None:
            adversarial.append(D.hinge_gen_loss(stft_fake_logits))
        adversarial_loss = torch.stack(adversarial).mean()
        all_commitment_loss = commit_loss.sum()
        total = recon_loss * self.recon_loss_weight + multi_spectral_recon_loss * self.multi_spectral_recon_loss_weight \
            + adversarial_loss * self.adversarial_loss_weight + feature_loss * self.feature_loss_weight + all_commitment_loss
        if breakdown:
            return total, (recon_loss, multi_spectral_recon_loss, adversarial_loss, feature_loss, all_commitment_loss)
        return total

    def decode_from_codebook_indices(self, quantized_indices):               # soundstream.py:691-699
        assert quantized_indices.dtype in (torch.long, torch.int32)
        if quantized_indices.ndim == 3:
            b, n, gq = quantized_indices.shape
            quantized_indices = quantized_indices.reshape(b, n, self.rq_groups, gq // self.rq_groups).permute(2, 0, 1, 3)   # 'b n (g q) -> g b n q'
        return self.decode(self.rq.get_output_from_indices(quantized_indices))

    def decode(self, x, quantize=False):                                      # soundstream.py:701-709
        """x fp32 (b, n, codebook_dim) -> wave (b, input_channels, n * prod(strides)): 'b n c -> b c n', then the causal transposed-conv decoder.
        A graph is built only in training mode with grad mode on (the decoder's parameters, and x if it requires grad)."""
        with torch.set_grad_enabled(torch.is_grad_enabled() and self.training):
            if quantize:
                x, *_ = self.rq(x)
            if not x.is_cuda:
                raise RuntimeError('audiolm_pytorch_amd.SoundStream runs on the MI355X only (no CPU fallback)')
            x = x.to(F32).contiguous()
            grad = codec_bwd.wants_grad(self.decoder, x)
            if self.decoder_attn is not None:                                # a geometry without a backward kernel raises before any launch
                self.decoder_attn.check_backward(x)
                grad = grad or codec_bwd.wants_grad(self.decoder_attn, x)
            h = codec_bwd.BctToBtcFn.apply(x) if grad and x.requires_grad else ops.bct_to_btc(x)     # the same per-batch 2-D transpose, (n, c) -> (c, n)
            if self.decoder_attn is not None:                                # :705-706
                h = self.decoder_attn.run_bct(h)
            for layer in self.decoder:
                if isinstance(layer, CausalConv1d):
                    h = layer.call(h)
                elif isinstance(layer, Residual):                            # GateLoopBlock (use_gate_loop_layers=True)
                    h = layer(h)
                else:
                    for sub in layer:
                        h = sub(h)
            return h


# ---- the reference's two presets (soundstream.py:999-1023) ----
def AudioLMSoundStream(strides=(2, 4, 5, 8), target_sample_hz=16000, rq_num_quantizers=12, **kwargs):
    return SoundStream(strides=strides, target_sample_hz=target_sample_hz, rq_num_quantizers=rq_num_quantizers, **kwargs)


def MusicLMSoundStream(strides=(3, 4, 5, 8), target_sample_hz=24000, rq_num_quantizers=12, **kwargs):
    return SoundStream(strides=strides, target_sample_hz=target_sample_hz, rq_num_quantizers=rq_num_quantizers, **kwargs)
