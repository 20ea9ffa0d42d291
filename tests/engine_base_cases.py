"""One small CPU instance of every model class and the rule its engine hands to engine_base.ParamArena, for
tests/test_engine_base_cpu.py; tests/golden/engine_base_parent.json holds each instance's arena offsets and state_dict keys
as recorded (tests/golden/make_golden_engine_base.py) before the engines shared a base."""
import argparse
import importlib

import torch

H, HEADS, K, PAD, PIXELS = 16, 2, 5, 6, 12


def _args(**kw):
    return argparse.Namespace(**{**dict(input_dim=24, seg=True, anticipate=True, max_pos_len=12,
                                        input_type="i3d_transcript"), **kw})


def _futr(mod, **kw):
    cls = importlib.import_module("r3d_amd.model." + mod).FUTR
    args = kw.pop("args", None) or _args()
    return cls(K, H, PAD, torch.device("cpu"), args, n_query=8, n_head=HEADS, num_encoder_layers=1, num_decoder_layers=1,
               **kw)


def _tcn():
    from r3d_amd.model.tcn import MustafaNet1DTCN
    return MustafaNet1DTCN(num_classes=3, anticipated_frames=8)


# name -> (the model, the attribute of its engine module that is the arena's live rule -- or a callable on that module)
MODELS = {
    "tokenfusion": (lambda: _futr("futr_safuser_tokenfusion", depth_pixels=PIXELS), "engine", lambda E: E.live_rule()),
    "bn": (lambda: _futr("futr_safuser_batchnormalization", depth_pixels=PIXELS), "engine",
           lambda E: E.live_rule(E.BN_LIVE_PREFIXES)),
    "vary": (lambda: _futr("futr_safuser_tokenfusion_vary", depth_pixels=PIXELS), "engine",
             lambda E: E.live_rule(E.VARY_LIVE_PREFIXES)),
    "plain": (lambda: _futr("futr_safuser_depth", depth_pixels=PIXELS), "engine", lambda E: E.live_rule(E.PLAIN_LIVE_PREFIXES)),
    "afft": (lambda: _futr("afft", depth_pixels=PIXELS, args=_args(seg=False)), "engine_afft", lambda E: E.is_live),
    "m3": (lambda: _futr("futr_safuser_tokenfusion3", depth_pixels=PIXELS, gaze_dim=2), "engine_m3", lambda E: E.is_live),
    "cnn": (lambda: _futr("cnn"), "engine_cnn", lambda E: E.is_live),
    "rnn": (lambda: _futr("rnn"), "engine_rnn", lambda E: E.is_live),
    "tcn": (_tcn, "engine_tcn", lambda E: E.is_live),
    "unsup_depth": (lambda: _futr("futr_unsupervised_depth", depth_pixels=PIXELS), "engine_unsup", lambda E: E.is_live),
    "unsup_label": (lambda: _futr("futr_proposed"), "engine_unsup", lambda E: E.is_live),
    "l3": (lambda: _futr("futr_unsupervised_temp3"), "engine_l3", lambda E: E.is_live),
}


def named_params(name, model):
    """in the order the model's engine hands them to the arena"""
    named = list(model.named_parameters())
    if name == "rnn":
        from r3d_amd.engine_rnn import _arena_order
        named = _arena_order(named)
    return named


def arena(name, model):
    """The model's arena on the CPU, built the way its engine builds it."""
    from r3d_amd.engine_base import ParamArena
    _, mod, rule = MODELS[name]
    return ParamArena(named_params(name, model), torch.device("cpu"), rule(importlib.import_module("r3d_amd." + mod)))


def offsets(a):
    return {n: [o, k] for n, (o, k, _) in a.offsets.items()}
