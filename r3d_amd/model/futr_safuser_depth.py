"""Drop-in for the reference's ``model/futr_safuser_depth.py``: the plain SA-Fuser, the baseline the token-exchanging
fusers are compared against.  It differs from the token-fusion model in the fuser only (:17-71 against
futr_safuser_tokenfusion.py:17-97):
  * no token selection or exchange: the two embeddings are stacked as they are (:43-46);
  * the learnable ``fuser.modality_token`` [1, 1, 1, C] is added to both tokens of every frame before embd_drop
    (:40,48,51) -- a trained parameter here, dead in every other fuser;
  * no x_res: the fuser output is norm(Block(embd_drop(x))), then the mean over the two tokens (:53-62);
  * the fuser has no ``fusion_conv`` (so the state_dict differs, and so does the seeded init of every parameter built
    after the fuser: Conv2d init consumes RNG);
  * depth_projection takes 160 * 120 pixels (:118);
  * outside train mode ``inputs`` is the bare feature tensor (:145); the reference's own validate() passes the
    (features, labels) tuple, so either form is accepted here;
  * the fuser's attention-weight output (:56,64) is discarded by FUTR (:173) and not built.

Same class names, constructor, forward signature, construction order and state_dict keys; parameters are holders only,
the arithmetic runs in libr3d_hip.so (r3d_amd/csrc/plainfuse.hip + the shared kernels)."""
import torch
from torch import nn

from . import futr_safuser_tokenfusion as _base


class CMFuser(nn.Module):
    """SA-Fuser parameter tree of futr_safuser_depth.py:17-29 (blocks, norm, modality_token, projection)."""

    r3d_fuser_kind = "plain"            # FusionEngine's mode selector: stack + modality token, no exchange, no x_res

    def __init__(self, dim, depth=1, num_heads=4, mlp_ratio=4.0, qkv_bias=False):
        super().__init__()
        if depth != 1:
            raise NotImplementedError("the reference builds CMFuser(depth=1) (futr_safuser_depth.py:93)")
        self.blocks = nn.ModuleList([_base._Block(dim, num_heads, mlp_ratio, qkv_bias) for _ in range(depth)])
        self.norm = nn.LayerNorm(dim)
        self.modality_token = nn.Parameter(torch.randn(1, 1, 1, dim))
        self.projection = nn.Linear(dim, dim)


class FUTR(_base.FUTR):
    _fuser_cls = CMFuser

    def __init__(self, n_class, hidden_dim, src_pad_idx, device, args, n_query=8, n_head=8, num_encoder_layers=6,
                 num_decoder_layers=6, query_num=49, depth_pixels=160 * 120):
        super().__init__(n_class, hidden_dim, src_pad_idx, device, args, n_query, n_head, num_encoder_layers,
                         num_decoder_layers, query_num, depth_pixels)

    def forward(self, inputs, depth_features, mode="train", epoch=0, idx=0):
        if mode != "train" and not isinstance(inputs, (tuple, list)):
            inputs = (inputs, None)              # the reference's bare tensor (:145)
        return super().forward(inputs, depth_features, mode, epoch, idx)
