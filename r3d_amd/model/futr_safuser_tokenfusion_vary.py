"""Drop-in for the reference's ``model/futr_safuser_tokenfusion_vary.py``: the activation-magnitude token fuser.  It
differs from the token-fusion model in the fuser only (:17-87 against futr_safuser_tokenfusion.py:17-97):
  * the selection score is mean_(B,T) |x| per channel in EVERY mode, k = C // 4 smallest (:40-46);
  * a learnable scale ``alpha`` [1, 1, C] on the swapped channels: exchanged_rgb[c] = alpha[c] * depth[c] and
    exchanged_depth[c] = alpha[c] * rgb[c] on the selected channels (:32,51-56);
  * no x_res: the fuser output is norm(Block(embd_drop(x))) (:78-82).
The FUTR around the fuser is the token-fusion one (:89-220; depth_projection 224 * 224 in both).

Same class names, constructor, forward signature and state_dict keys (``fuser.alpha`` after ``fuser.fusion_conv``, as in
the reference); alpha is created with torch.ones and consumes no RNG, so a seeded init equals the token-fusion model's.
Parameters are holders only, the arithmetic runs in libr3d_hip.so (r3d_amd/csrc/varyfuse.hip + the shared kernels)."""
import torch
from torch import nn

from . import futr_safuser_tokenfusion as _base


class CMFuser(_base.CMFuser):
    def __init__(self, dim, depth=1, num_heads=4, mlp_ratio=4.0, qkv_bias=False):
        super().__init__(dim, depth, num_heads, mlp_ratio, qkv_bias)
        self.alpha = nn.Parameter(torch.ones(1, 1, dim))              # :32


class FUTR(_base.FUTR):
    _fuser_cls = CMFuser
