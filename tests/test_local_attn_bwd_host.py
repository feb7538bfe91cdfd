"""CPU: the host-side queries of the LocalTransformer backward (csrc/local_attn_bwd.hip) -- workspace sizes and the support predicate.  No launches."""
import pytest

import audiolm_pytorch_amd  # noqa: F401
from audiolm_pytorch_amd import _lib, ops

# (B, H, dh, T, W) of tests/test_gpu_local_attn_bwd.py, plus the default geometry at 30 s
SHAPES = [(2, 2, 32, 129, 64), (1, 3, 32, 64, 64), (2, 2, 32, 40, 64), (2, 2, 32, 50, 16), (1, 8, 64, 300, 128), (1, 2, 64, 257, 128), (8, 8, 64, 2250, 128)]


@pytest.mark.parametrize('B,H,dh,T,W', SHAPES)
def test_attention_workspace_matches_the_documented_formula(B, H, dh, T, W):
    """lse + delta [B][H][T] each, and one q_scale and one k_scale partial [dh] per (b, h, window)"""
    windows = -(-T // W)
    assert _lib.query('alm_local_attn_bwd_ws_floats', B, H, dh, T, W) == 2 * B * H * T + 2 * B * H * windows * dh


def test_workspace_queries_refuse_what_does_not_fit():
    assert _lib.query('alm_local_attn_bwd_ws_floats', 4096, 64, 64, 1 << 20, 128) == -1          # past 2^31 floats
    assert _lib.query('alm_local_attn_bwd_ws_floats', 0, 2, 32, 10, 16) == -1
    assert _lib.query('alm_layernorm_bct_bwd_ws_floats', 2, 300) == 2 * 2 * 300                 # mean and rstd per (b, t)
    assert _lib.query('alm_layernorm_bct_bwd_ws_floats', 1 << 16, 1 << 16) == -1


def test_support_predicate():
    for dh, W in ((32, 16), (32, 64), (32, 256), (64, 128), (64, 160), (64, 1), (32, 1)):
        assert ops.local_attn_bwd_supported(dh, W), (dh, W)
    # what the forward refuses (dim_head outside {32, 64}, window > 256, K / V of the window pair past 160 KiB of LDS: dim_head 64 beyond window 160)
    # the backward refuses too, and nothing else
    for dh, W in ((8, 8), (16, 64), (128, 64), (48, 64), (32, 257), (64, 256), (64, 161), (32, 0)):
        assert not ops.local_attn_bwd_supported(dh, W), (dh, W)


def test_predicate_matches_the_lds_budget():
    """K / V (dQ pass) or rotated Q / dO_pre (dK/dV pass) of a window pair, [dh][2 W] floats each, within 160 KiB: alm_local_attn's own condition"""
    for dh in (32, 64):
        for W in range(1, 300):
            want = W <= 256 and 4 * dh * W * 4 <= 160 * 1024
            assert ops.local_attn_bwd_supported(dh, W) == want, (dh, W)
