"""Host-side sequencing of the TCN baseline (reference model/tcn.py, MustafaNet1DTCN) on one MI355X.

    four levels i = 0..3, channels 2048 -> 256 -> 512 -> 512 -> 256, dilation d = 2^i, per level
        y1  = dropout(relu(conv1(x)))                  conv = weight-normalised dilated causal Conv1d, kernel 3
        y2  = dropout(relu(conv2(y1)))
        out = relu(y2 + res),  res = x (level 2) or downsample(x) (a 1x1 convolution = nn.Linear in this layout)
    logits = regression(mean over all S frames of out_3)         [B, 8 * num_classes] viewed [B, 8, num_classes]

Activations are [B*S, C] row-major.  Every convolution product (forward, input gradient, weight gradient) is one launch
of csrc/tconv.hip, whose operand loader applies the frame shift and the clip mask: the workspaces below hold activations,
their gradients, chunk partials of column sums and (for long batches) row-range partials of the weight gradients,
never a [B*S, 3 C_in] copy.  Weight normalisation stays factored
(s = g / |v| once per step); the 1x1 convolutions, the head and their gradients are the existing fp32 GEMMs; the head is
applied to the time means (a 1x1 convolution commutes with the mean).  Nothing in a step uses atomics.
"""
import torch

from . import ops
from ._lib import GEMM_NT, GEMM_NN, GEMM_TN
from .engine_base import EngineBase

TCN_IN = 2048
TCN_CHANNELS = (256, 512, 512, 256)
TCN_DROP_P = 0.2                    # the rate model/tcn.py constructs its blocks with
TCN_MAX_HEAD = 65536                # anticipated_frames * num_classes (columns of the regression GEMM)
TCN_MAX_LOSS_ROWS = 65536           # B * anticipated_frames: the loss launch walks its rows in one workgroup (r3d_ce_rows_supported)


def check_tcn_shape(B, S, num_classes, anticipated_frames=8):
    """Raises ValueError unless the engine trains this shape.  Host arithmetic only: nothing is enqueued."""
    if B < 1 or S < 1:
        raise ValueError(f"batch {B} x {S} frames: the TCN needs at least one clip of at least one frame")
    if num_classes < 1 or anticipated_frames < 1:
        raise ValueError(f"num_classes {num_classes}, anticipated_frames {anticipated_frames}: both must be positive")
    if B * S * TCN_IN >= 2 ** 31:
        raise ValueError(f"batch {B} x {S} frames: B * S * {TCN_IN} must stay below 2^31 (the range the "
                         f"convolution kernels admit, r3d_tconv_supported)")
    assert B * S <= 64 * 65535          # (implied: the kernels' grid covers 64 frames per workgroup row, 65535 rows)
    if B * anticipated_frames > TCN_MAX_LOSS_ROWS or num_classes > TCN_MAX_LOSS_ROWS:
        raise ValueError(f"batch {B} x {anticipated_frames} anticipated frames, {num_classes} classes: the loss launch takes at "
                         f"most {TCN_MAX_LOSS_ROWS} rows and as many classes")
    if anticipated_frames * num_classes > TCN_MAX_HEAD:
        raise ValueError(f"anticipated_frames * num_classes = {anticipated_frames * num_classes}: the regression head takes "
                         f"at most {TCN_MAX_HEAD} outputs")


def is_live(name):
    return True                         # (every parameter receives a gradient)


class _Level:
    def __init__(self, i, c_in, c_out):
        self.i, self.c_in, self.c_out, self.dil = i, c_in, c_out, 2 ** i
        self.pre = f"tcn_local.network.{i}."
        self.down = c_in != c_out


class _Shape:
    def __init__(self, eng, B, S, train):
        dev = eng.device
        N = B * S
        f = lambda *s: torch.empty(*s, dtype=torch.float32, device=dev)     # noqa: E731
        self.B, self.S, self.N = B, S, N
        self.y1 = [f(N, L.c_out) for L in eng.levels]
        self.y2 = [f(N, L.c_out) for L in eng.levels]
        self.out = [f(N, L.c_out) for L in eng.levels]
        self.res = [f(N, L.c_out) if L.down else None for L in eng.levels]
        self.pooled = f(B, TCN_CHANNELS[-1])
        self.logits = f(B, eng.Q * eng.K)
        self.loss = f(4)
        self.counts = torch.zeros(4, dtype=torch.int64, device=dev)
        self.p1 = self.p2 = [None] * 4
        self.drop = None
        if train:
            self.p1 = [f(N, L.c_out) for L in eng.levels]
            self.p2 = [f(N, L.c_out) for L in eng.levels]
            sizes = [N * L.c_out for L in eng.levels for _ in (0, 1)]          # the eight dropouts, one pool
            self.drop_pool = torch.ones(sum((n + 15) // 16 * 16 for n in sizes), dtype=torch.uint8, device=dev)
            self.drop, o = [], 0
            for n in sizes:
                self.drop.append(self.drop_pool[o:o + n])
                o += (n + 15) // 16 * 16
            cmax = max(TCN_CHANNELS)
            self.d_logits = torch.zeros(B, eng.Q * eng.K, dtype=torch.float32, device=dev)
            self.d_pooled, self.d_out = f(B, TCN_CHANNELS[-1]), f(N, TCN_CHANNELS[-1])
            self.gbuf = [f(N * cmax), f(N * cmax)]
            self.dz, self.dy1, self.rds = f(N * cmax), f(N * cmax), f(N * cmax)
            self.prep_ws = f(max(1, ops.tconv_ws_floats(N, cmax)))
            # row-range partials of the weight gradients of a long batch (summed range by range; nothing for a short one)
            self.wgrad_part = f(max(4, max(ops.tconv_wgrad_ws_floats(N, ci, co) for L in eng.levels
                                           for ci, co in ((L.c_in, L.c_out), (L.c_out, L.c_out)))))


class TcnEngine(EngineBase):
    _Shape = _Shape

    def __init__(self, module, device):
        self.K, self.Q = module.num_classes, module.anticipated_frames
        check_tcn_shape(1, 1, self.K, self.Q)                        # (before anything is enqueued)
        self.levels = [_Level(i, TCN_IN if i == 0 else TCN_CHANNELS[i - 1], c) for i, c in enumerate(TCN_CHANNELS)]
        self._init_engine(module, device, is_live)
        # per convolution: s = g / |v|, 1 / |v| and the rank-one coefficient <G_o, v_o> / |v_o|^2
        tot = sum(2 * L.c_out for L in self.levels)
        self.scales = torch.zeros(3, tot, dtype=torch.float32, device=self.device)
        self.slot, o = {}, 0
        for L in self.levels:
            for c in ("conv1", "conv2"):
                self.slot[L.pre + c] = (o, L.c_out)
                o += L.c_out

    def _sc(self, name, k):
        o, n = self.slot[name]
        return self.scales[k, o:o + n]

    def workspace_shapes(self, B, S, train=True):
        """(name, shape, dtype) of every buffer a step of (B, S) uses besides the parameter arenas and the per-channel
        scales (the tests' no-im2col check)."""
        w = self._shape(B, S, train)
        out = []
        for k, v in vars(w).items():
            for t in (v if isinstance(v, (list, tuple)) else [v]):
                if torch.is_tensor(t):
                    out.append((k, tuple(t.shape), t.dtype))
        return out

    # ------------------------------------------------------------------------------------------------------
    def forward(self, feats, training=False, need_grad=True):
        """feats [B, S, 2048] f32 -> logits [B, anticipated_frames, num_classes] (a view of the workspace).
        training: dropout on (needs need_grad's workspace)."""
        a = self.arena
        assert feats.is_cuda and feats.dtype == torch.float32 and feats.dim() == 3 and feats.shape[2] == TCN_IN
        B, S = feats.shape[0], feats.shape[1]
        check_tcn_shape(B, S, self.K, self.Q)
        N = B * S
        x = feats.reshape(N, TCN_IN)
        assert x.is_contiguous()
        w = self._shape(B, S, need_grad or training)
        p_drop = float(self.module.tcn_local.network[0].dropout1.p)     # (one rate for the eight dropouts, as constructed)
        drop = bool(training) and p_drop > 0.0
        if drop:
            # the pool of THIS forward, then the offset moves on (stream-ordered, capturable): whichever route drives the
            # engine -- train_step, a torch optimiser on the arena gradients, the autograd bridge -- the next forward draws
            # fresh masks
            ops.dropout_mask(w.drop_pool, p_drop, self.drop_seed, self.drop_offset)
            ops.tick(self.drop_offset, None)
        scale = 1.0 / (1.0 - p_drop) if drop else 1.0
        for L in self.levels:
            for c in ("conv1", "conv2"):
                n = L.pre + c
                ops.tconv_wnorm(a.p(n + ".weight_v"), a.p(n + ".weight_g"), self._sc(n, 0), self._sc(n, 1))
        x_in = x
        for L in self.levels:
            i, n1, n2 = L.i, L.pre + "conv1", L.pre + "conv2"
            ops.tconv_fwd(x_in, a.p(n1 + ".weight_v"), self._sc(n1, 0), a.p(n1 + ".bias"), S, L.dil, w.y1[i], p_out=w.p1[i],
                          drop_mask=w.drop[2 * i] if drop else None, drop_scale=scale)
            if L.down:
                ops.gemm(GEMM_NT, x_in, a.p(L.pre + "downsample.weight").view(L.c_out, L.c_in), w.res[i],
                         bias=a.p(L.pre + "downsample.bias"), ws=self.ws)
            ops.tconv_fwd(w.y1[i], a.p(n2 + ".weight_v"), self._sc(n2, 0), a.p(n2 + ".bias"), S, L.dil, w.y2[i], p_out=w.p2[i],
                          drop_mask=w.drop[2 * i + 1] if drop else None, drop_scale=scale,
                          res=w.res[i] if L.down else x_in, out=w.out[i])
            x_in = w.out[i]
        ops.avgpool_rows_fwd(x_in, w.pooled, B, S, 1)                    # mean over all S frames, padded ones included
        ops.gemm(GEMM_NT, w.pooled, a.p("regression.weight").view(self.Q * self.K, TCN_CHANNELS[-1]), w.logits,
                 bias=a.p("regression.bias"), ws=self.ws)
        self.last = dict(w=w, x=x, drop=drop, scale=scale, grad=need_grad or training)
        return w.logits.view(B, self.Q, self.K)

    # ------------------------------------------------------------------------------------------------------
    def losses(self, target, pad_idx, with_grad=True):
        """cal_performance(output.view(-1, C), target.view(-1), pad_idx): loss[1] = loss[3] = the loss, counts[2:4] =
        (n_correct, n_total).  Fills d_logits."""
        w = self.last["w"]
        rows = w.B * self.Q
        assert target.numel() == rows
        ops.ce_rows_fwd_bwd(w.logits.view(rows, self.K), target.reshape(-1).contiguous(), pad_idx, w.loss, w.counts,
                            w.d_logits.view(rows, self.K) if with_grad else None)
        return w.loss, w.counts

    # ------------------------------------------------------------------------------------------------------
    def backward(self, d_logits=None):
        """Adjoint of forward(); gradients land in the grad arena (written, not accumulated)."""
        st = self.last
        assert st["grad"], "forward() ran without the backward's workspace"
        w, a, ws = st["w"], self.arena, self.ws
        B, S, N = w.B, w.S, w.N
        if d_logits is not None and d_logits.data_ptr() != w.d_logits.data_ptr():
            w.d_logits.copy_(d_logits.reshape(w.d_logits.shape))
        CL = TCN_CHANNELS[-1]
        w_reg = a.p("regression.weight").view(self.Q * self.K, CL)
        ops.gemm(GEMM_TN, w.d_logits, w.pooled, a.g("regression.weight").view(self.Q * self.K, CL),
                 bias_grad=a.g("regression.bias"), ws=ws)
        ops.gemm(GEMM_NN, w.d_logits, w_reg, w.d_pooled, ws=ws)
        ops.avgpool_rows_bwd(w.d_pooled, w.d_out, B, S, 1)
        g = w.gbuf[0][:N * CL].view(N, CL)                          # level i's gradient lives in gbuf[(i + 1) % 2]
        ops.posenc_bwd(w.d_out, g, gate=w.out[3])                      # through the last block's output ReLU
        for L in reversed(self.levels):
            i, n1, n2 = L.i, L.pre + "conv1", L.pre + "conv2"
            x_in = st["x"] if i == 0 else w.out[i - 1]
            dz = w.dz[:N * L.c_out].view(N, L.c_out)
            dy1 = w.dy1[:N * L.c_out].view(N, L.c_out)
            v1, v2 = a.p(n1 + ".weight_v"), a.p(n2 + ".weight_v")
            ops.tconv_bwd_prep(g, w.y2[i], w.p2[i], self._sc(n2, 1), dz, a.g(n2 + ".bias"), a.g(n2 + ".weight_g").view(-1),
                               self._sc(n2, 2), w.prep_ws, drop_scale=st["scale"])
            ops.tconv_wgrad(dz, w.y1[i], v2, S, L.dil, a.g(n2 + ".weight_v"), s=self._sc(n2, 0), coef=self._sc(n2, 2),
                            ws=w.wgrad_part)
            ops.tconv_dx(dz, v2, self._sc(n2, 0), S, L.dil, dy1)
            ops.tconv_bwd_prep(dy1, w.y1[i], w.p1[i], self._sc(n1, 1), dz, a.g(n1 + ".bias"), a.g(n1 + ".weight_g").view(-1),
                               self._sc(n1, 2), w.prep_ws, drop_scale=st["scale"])
            ops.tconv_wgrad(dz, x_in, v1, S, L.dil, a.g(n1 + ".weight_v"), s=self._sc(n1, 0), coef=self._sc(n1, 2),
                            ws=w.wgrad_part)
            if L.down:
                ops.gemm(GEMM_TN, g, x_in, a.g(L.pre + "downsample.weight").view(L.c_out, L.c_in),
                         bias_grad=a.g(L.pre + "downsample.bias"), ws=ws)
            if i == 0:
                break                                                   # the features carry no gradient
            res = g
            if L.down:
                res = w.rds[:N * L.c_in].view(N, L.c_in)
                ops.gemm(GEMM_NN, g, a.p(L.pre + "downsample.weight").view(L.c_out, L.c_in), res, ws=ws)
            g_prev = w.gbuf[i % 2][:N * L.c_in].view(N, L.c_in)
            ops.tconv_dx(dz, v1, self._sc(n1, 0), S, L.dil, g_prev, res=res, gate=x_in)
            g = g_prev

    # ------------------------------------------------------------------------------------------------------
    def _tick_counter(self, tick_dropout):
        return None                         # (every dropout forward moves the offset itself: see forward())

    def train_step(self, feats, target, pad_idx, lr, weight_decay, training=True, betas=(0.9, 0.999), eps=1e-8):
        """forward + loss + backward + AdamW, all enqueued, no host sync.  Returns (loss[4], counts[4]) on device."""
        self.forward(feats, training=training)
        loss, counts = self.losses(target, pad_idx)
        ops.tick(self.step_t, None)
        self.backward()
        self.adamw(lr, weight_decay, betas=betas, eps=eps, ticked=True)
        return loss, counts
