"""Host side of the stepwise LSTM route (csrc/lstm_steps.hip, opts --wide_rnn): the measured bounds stay under their cap, the
admission rule with and without the flag, the route table, the flag itself, the model's state_dict at a wide hidden size and
the supervised contrastive term's refusal past its kernel's width.  Nothing here touches a GPU."""
import argparse
import json

import pytest
import torch

from tests import rnn_wide_cases as WC
from tests.helpers import load_fixture


@pytest.mark.parametrize("B,S,H", WC.ALL_CASES)
def test_float32_restatement_stays_under_the_cap(B, S, H):
    _, bounds = WC.reference(B, S, H)
    for k in WC.TENSORS:
        bound, e32, scale = bounds[k]
        print(f"B{B} S{S} H{H} {k}: e32 {e32:.3e} scale {scale:.3e} ratio {e32 / scale if scale else 0.0:.3e}")
        assert WC.MARGIN * e32 <= WC.CAP * scale, (k, e32, scale)
        assert bound <= WC.CAP * scale
    if S == 1:
        assert bounds["dw_hh"][2] == 0.0        # (h_prev is zero at a direction's first step)


@pytest.mark.parametrize("H", WC.ADMITTED_WIDE_H)
def test_check_rnn_shape_wide_admits(H):
    from r3d_amd.engine_rnn import check_rnn_shape
    check_rnn_shape(H, 8, 0.0, wide=True)


@pytest.mark.parametrize("H", WC.REFUSED_WIDE_H)
def test_check_rnn_shape_wide_refuses(H):
    from r3d_amd.engine_rnn import check_rnn_shape
    with pytest.raises(ValueError, match="hidden"):
        check_rnn_shape(H, 8, 0.0, wide=True)


def test_default_message_names_the_flag_where_it_helps():
    from r3d_amd.engine_rnn import check_rnn_shape, RNN_MAX_H, RNN_WIDE_MAX_H
    assert (RNN_MAX_H, RNN_WIDE_MAX_H) == (256, 1024)
    for H in (264, 512, 1000, 1024):
        with pytest.raises(ValueError, match=r"hidden.*held in registers.*--wide_rnn"):
            check_rnn_shape(H, 8, 0.0)
        with pytest.raises(ValueError, match=r"--wide_rnn"):
            check_rnn_shape(H, 8, 0.0, wide=False)
    for H in (0, 4, 12, 130, 260, 1028, 1032, 2048):
        with pytest.raises(ValueError, match="hidden") as e:
            check_rnn_shape(H, 8, 0.0)
        assert "wide_rnn" not in str(e.value), H
    for H in (8, 128, 256):
        check_rnn_shape(H, 8, 0.0)
    with pytest.raises(ValueError, match="n_query"):
        check_rnn_shape(512, 9, 0.0, wide=True)
    with pytest.raises(ValueError, match="erank_weight"):
        check_rnn_shape(512, 8, 0.1, wide=True)


def test_wide_range_matches_kernel_range():
    from r3d_amd import build, ops
    from r3d_amd.engine_rnn import check_rnn_shape
    build.build(verbose=False)
    for H in range(0, 1101):
        try:
            check_rnn_shape(H, 8, 0.0, wide=True)
            ok = True
        except ValueError:
            ok = False
        assert ok == ops.lstm_steps_supported(H), H
    assert ops.lstm_steps_ws_floats(8, 512) == 8 * 512 + 2 * 512 * 512
    with pytest.raises(ValueError):
        ops.lstm_steps_ws_floats(8, 1032)
    with pytest.raises(ValueError):
        ops.lstm_steps_ws_floats(0, 512)


def test_lstm_route_truth_table():
    from r3d_amd import build
    from r3d_amd.engine_rnn import lstm_route
    build.build(verbose=False)
    for wide in (False, True):
        for H in (8, 128, 136, 256):
            assert lstm_route(H, wide) == "registers", (H, wide)       # the same kernels with or without the flag
        for H in (0, 4, 12, 260, 1028, 1032, 2048):
            assert lstm_route(H, wide) is None, (H, wide)
    for H in (264, 512, 1000, 1024):
        assert lstm_route(H, True) == "steps"
        assert lstm_route(H, False) is None


def test_opts_flag():
    from r3d_amd import opts
    assert opts.parser.parse_args([]).wide_rnn is False
    assert opts.parser.parse_args(["--wide_rnn"]).wide_rnn is True


def _wide_model(H, n_class, **kw):
    from r3d_amd import opts
    from r3d_amd.model.rnn import FUTR
    args = opts.parser.parse_args(["--wide_rnn", "--hidden_dim", str(H)])
    args.n_query = 8
    for k, v in kw.items():
        setattr(args, k, v)
    model = FUTR(n_class, H, device=torch.device("cpu"), args=args, src_pad_idx=n_class + 1, n_query=8, n_head=args.n_head,
                 num_encoder_layers=args.n_encoder_layer, num_decoder_layers=args.n_decoder_layer)
    return model, args


def test_state_dict_at_hidden_264_matches_the_reference():
    from r3d_amd.model.rnn import FUTR
    fx = load_fixture("rnn_wide_264")
    model, args = _wide_model(264, fx["meta"]["n_class"])
    assert model.r3d_wide_rnn is True
    sd = model.state_dict()
    assert list(sd) == json.loads(str(fx["state_keys"]))
    assert [list(v.shape) for v in sd.values()] == json.loads(str(fx["state_shapes"]))
    bare = argparse.Namespace(**{k: v for k, v in vars(args).items() if k != "wide_rnn"})
    assert FUTR(5, 16, 6, torch.device("cpu"), bare, n_head=4, num_encoder_layers=1, num_decoder_layers=1).r3d_wide_rnn is False


def test_supcon_weight_refused_at_hidden_512(tmp_path):
    from r3d_amd import train_unimodal as TU
    from r3d_amd.engine_rnn import check_rnn_shape
    with pytest.raises(ValueError, match=r"supcon_weight.*256 columns"):
        check_rnn_shape(512, 8, 0.0, wide=True, supcon_weight=0.1)
    check_rnn_shape(256, 8, 0.0, wide=True, supcon_weight=0.1)
    check_rnn_shape(512, 8, 0.0, wide=True, supcon_weight=0.0)
    model, args = _wide_model(512, 17, supcon_weight=0.1, epochs=1)
    with pytest.raises(ValueError, match=r"supcon_weight.*256 columns"):
        TU.train(args, model, [], torch.optim.AdamW(model.parameters()), None, None, str(tmp_path), 18, torch.device("cpu"),
                 [], 1)
    assert model._engine is None
