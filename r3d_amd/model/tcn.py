"""Drop-in for the reference's ``model/tcn.py``: the temporal convolutional baseline (``MustafaNet1DTCN``, the alternative
model of main.py / main_proposed_50salads.py).  Same class names, constructor signatures, parameter names and order
(``conv{1,2}.bias / weight_g / weight_v``: the old-style ``weight_norm`` triple), the same 56-key ``state_dict`` (each block
registers its two convolutions a second time inside ``net``, so ``net.0.*`` / ``net.4.*`` repeat ``conv1.*`` / ``conv2.*``)
and the same initialisation stream, so the same torch seed yields the same initial weights and reference checkpoints load
with ``load_state_dict(strict=True)``.

What it computes: four residual levels (2048 -> 256 -> 512 -> 512 -> 256, kernel 3, dilation 1, 2, 4, 8, causal: output
frame t reads frames t - 2d, t - d, t of its own clip), each conv -> ReLU -> Dropout(0.2) twice plus the residual (a 1x1
convolution where the widths differ) and a ReLU; then a 1x1 regression to 8 * num_classes channels averaged over all
frames.  All arithmetic runs in libr3d_hip.so through r3d_amd.engine_tcn.TcnEngine (csrc/tconv.hip); the modules here are
parameter holders, and only ``MustafaNet1DTCN.forward`` computes.

Initialisation, as the reference leaves it: ``init_weights()`` writes N(0, 0.01) into ``conv.weight``, which under
``weight_norm`` is a derived attribute, so ``weight_v`` / ``weight_g`` keep nn.Conv1d's default initialisation -- but the
call still draws from the generator, and so does this file.  ``downsample.weight`` really is N(0, 0.01).
"""
import torch
from torch import nn

from ..engine_tcn import TcnEngine, TCN_IN, TCN_CHANNELS, TCN_DROP_P
from ._bridge import EngineOwner, arena_grads

_ONLY_WHOLE = ("r3d_amd.model.tcn: only MustafaNet1DTCN.forward computes (one fused engine on the GPU); the blocks are "
               "parameter holders")


class Chomp1d(nn.Module):
    def __init__(self, chomp_size):
        super().__init__()
        self.chomp_size = chomp_size

    def forward(self, x):
        return x.narrow(2, 0, x.size(2) - self.chomp_size).contiguous()      # drops the right-hand padding frames


class _WeightNormConv1d(nn.Module):
    """The parameters of weight_norm(nn.Conv1d(n_in, n_out, k)): bias, weight_g [n_out, 1, 1], weight_v [n_out, n_in, k],
    in that order, with nn.Conv1d's own initialisation (g = |v| per output channel)."""

    def __init__(self, n_inputs, n_outputs, kernel_size, stride, padding, dilation):
        super().__init__()
        self.in_channels, self.out_channels, self.kernel_size = n_inputs, n_outputs, (kernel_size,)
        self.stride, self.padding, self.dilation = (stride,), (padding,), (dilation,)
        init = nn.Conv1d(n_inputs, n_outputs, kernel_size)           # (initial values only; never called)
        self.bias = nn.Parameter(init.bias.detach().clone())
        v = init.weight.detach().clone()
        self.weight_g = nn.Parameter(torch.norm_except_dim(v, 2, 0))
        self.weight_v = nn.Parameter(v)

    def forward(self, x):
        raise NotImplementedError(_ONLY_WHOLE)


class TemporalBlock1D(nn.Module):
    def __init__(self, n_inputs, n_outputs, kernel_size, stride, dilation, padding, dropout=0.2):
        super().__init__()
        self.conv1 = _WeightNormConv1d(n_inputs, n_outputs, kernel_size, stride, padding, dilation)
        self.chomp1 = Chomp1d(padding)
        self.relu1 = nn.ReLU()
        self.dropout1 = nn.Dropout(dropout)
        self.conv2 = _WeightNormConv1d(n_outputs, n_outputs, kernel_size, stride, padding, dilation)
        self.chomp2 = Chomp1d(padding)
        self.relu2 = nn.ReLU()
        self.dropout2 = nn.Dropout(dropout)
        # the second registration of both convolutions: state_dict() lists them again as net.0.* and net.4.*
        self.net = nn.Sequential(*[getattr(self, f"{kind}{k}") for k in (1, 2) for kind in ("conv", "chomp", "relu", "dropout")])
        self.downsample = None                                       # the residual's 1x1 convolution, where the widths differ
        if n_inputs != n_outputs:
            self.downsample = nn.Conv1d(n_inputs, n_outputs, 1)
        self.relu = nn.ReLU()
        self.init_weights()

    def init_weights(self):
        # the two draws the reference spends on the derived conv.weight (discarded by the next forward there, here at once)
        torch.empty_like(self.conv1.weight_v).normal_(0, 0.01)
        torch.empty_like(self.conv2.weight_v).normal_(0, 0.01)
        if self.downsample is not None:
            self.downsample.weight.data.normal_(0, 0.01)

    def forward(self, x):
        raise NotImplementedError(_ONLY_WHOLE)


class TemporalConvNet1D(nn.Module):
    def __init__(self, num_inputs, num_channels, kernel_size=3, dropout=0.2):
        super().__init__()
        layers = []
        for i, out_channels in enumerate(num_channels):
            dilation = 2 ** i
            in_channels = num_inputs if i == 0 else num_channels[i - 1]
            layers.append(TemporalBlock1D(in_channels, out_channels, kernel_size, stride=1, dilation=dilation,
                                          padding=(kernel_size - 1) * dilation, dropout=dropout))
        self.network = nn.Sequential(*layers)

    def forward(self, x):
        raise NotImplementedError(_ONLY_WHOLE)


class MustafaNet1DTCN(EngineOwner, nn.Module):
    """MustafaNet1DTCN(num_classes=15, anticipated_frames=8); forward(x [B, S, 2048]) -> [B, anticipated_frames, num_classes]."""
    _engine_param, _engine_name, _engine_cls = "regression.weight", "r3d_amd.model.tcn.MustafaNet1DTCN", TcnEngine

    def __init__(self, num_classes=15, anticipated_frames=8):
        super().__init__()
        self.anticipated_frames = anticipated_frames
        self.num_classes = num_classes
        self.tcn_local = TemporalConvNet1D(num_inputs=TCN_IN, num_channels=list(TCN_CHANNELS), kernel_size=3,
                                           dropout=TCN_DROP_P)
        self.regression = nn.Conv1d(in_channels=TCN_CHANNELS[-1], out_channels=num_classes * anticipated_frames, kernel_size=1)

    def forward(self, x):
        from ..engine_tcn import check_tcn_shape
        if x.dim() != 3 or x.shape[2] != TCN_IN:
            raise ValueError(f"expected features [batch, window, {TCN_IN}], got {tuple(x.shape)}")
        check_tcn_shape(x.shape[0], x.shape[1], self.num_classes, self.anticipated_frames)    # before the engine exists
        eng = self.engine()
        x = x.to(device=eng.device, dtype=torch.float32).contiguous()
        need_grad = torch.is_grad_enabled() and any(p.requires_grad for p in self.parameters())
        if not need_grad:
            return eng.forward(x, training=self.training, need_grad=False).clone()
        names = [n for n, _ in self.named_parameters()]
        params = [p for _, p in self.named_parameters()]
        return _Forward.apply(eng, x, self.training, names, *params)


class _Forward(torch.autograd.Function):
    """Bridges the engine into autograd (a loss on the output, .backward(), any torch optimiser)."""

    @staticmethod
    def forward(ctx, eng, x, training, names, *params):
        out = eng.forward(x, training=training, need_grad=True)
        ctx.eng, ctx.names, ctx.token = eng, names, eng.last
        return out.clone()

    @staticmethod
    def backward(ctx, d_out):
        eng = ctx.eng
        if eng.last is not ctx.token:
            raise RuntimeError("r3d_amd: backward() must follow the forward() it belongs to")
        eng.backward(d_logits=d_out.to(torch.float32).contiguous())
        return (None,) * 4 + arena_grads(eng, ctx.names)
