"""CPU: the host side of audiolm_pytorch_amd.resample -- filter geometry, the sinc table against the restated torchaudio recipe
(tests/resample_restated.py), output lengths and the argument contract.  No kernel runs here."""
import importlib

import pytest
import torch

import resample_restated as R
import audiolm_pytorch_amd as A
from audiolm_pytorch_amd import _lib

RS = importlib.import_module('audiolm_pytorch_amd.resample')          # the module (the package attribute `resample` is the function)

PAIRS = {(16000, 24000): (2, 3, 7, 16), (48000, 24000): (2, 1, 13, 28), (44100, 24000): (147, 80, 12, 171),
         (22050, 32000): (441, 640, 7, 455), (32000, 22050): (640, 441, 9, 658)}


@pytest.mark.parametrize('pair', sorted(PAIRS))
def test_geometry_and_table_shape(pair):
    o, n, W, T = PAIRS[pair]
    assert RS.geometry(*pair) == (o, n, W, T)
    assert R.geometry(*pair) == (o, n, W, T)
    K = RS.sinc_table(*pair)
    assert K.shape == (n, T) and K.dtype == torch.float32


@pytest.mark.parametrize('pair', sorted(PAIRS))
def test_per_phase_dc_gain_is_one(pair):
    K = RS.sinc_table(*pair).double()
    gain = K.sum(dim=1)
    assert float((gain - 1).abs().max()) <= 1e-3, gain


@pytest.mark.parametrize('pair,kw', [((16000, 24000), {}), ((44100, 24000), {}), ((32000, 22050), {}), ((48000, 8000), {}),
                                     ((44100, 24000), dict(resampling_method='sinc_interp_kaiser')),
                                     ((16000, 22050), dict(resampling_method='sinc_interp_kaiser', beta=8.0)),
                                     ((24000, 16000), dict(lowpass_filter_width=3, rolloff=0.9)),
                                     ((8000, 44100), dict(lowpass_filter_width=10, rolloff=0.95))])
def test_table_is_bitwise_the_restated_fp32_recipe(pair, kw):
    mine = RS.sinc_table(*pair, **kw)
    ref = R.table(*pair, lw=kw.get('lowpass_filter_width', 6), rolloff=kw.get('rolloff', 0.99),
                  method=kw.get('resampling_method', 'sinc_interp_hann'), beta=kw.get('beta'))
    assert torch.equal(mine, ref)


@pytest.mark.parametrize('pair', sorted(PAIRS) + [(8000, 48000), (48000, 44100)])
def test_output_length(pair):
    o, n, W, T = RS.geometry(*pair)
    for L in sorted({0, 1, o - 1, o, T, 2 * T + 1, 1001}):
        want = -(-n * L // o)
        assert RS.output_length(L, *pair) == want == R.out_len(L, *pair)
        if 0 < L <= 2 * T + 1:                           # the recipe's own conv1d + truncation gives that many samples
            assert R.resample(torch.zeros(1, L), *pair).shape[-1] == want


def test_argument_errors_and_identity():
    x = torch.randn(2, 100)
    assert A.resample(x, 16000, 16000) is x                 # the same rate returns the input itself (even on the CPU)
    assert A.resample(x, 16000.0, 16000) is x
    with pytest.raises(TypeError):
        A.resample(torch.zeros(2, 100, dtype=torch.long), 16000, 24000)
    with pytest.raises(TypeError):
        A.resample(torch.zeros(2, 100, dtype=torch.int16), 16000, 16000)
    for bad in [(0, 16000), (16000, 0), (-8000, 16000), (16000.5, 24000), (16000, float('nan'))]:
        with pytest.raises(ValueError):
            A.resample(x, *bad)
    with pytest.raises(ValueError):
        A.resample(x, 16000, 24000, resampling_method='sinc_interp_cubic')
    with pytest.raises(ValueError):
        A.resample(x, 16000, 24000, lowpass_filter_width=0)
    with pytest.raises(_lib.AlmError):                      # no CPU path
        A.resample(x, 16000, 24000)


def test_process_input_keeps_the_same_rate_untouched():
    ss = A.SoundStream(codebook_size=16, rq_num_quantizers=2, channels=4, codebook_dim=16, use_local_attn=False, target_sample_hz=24000)
    wave = torch.randn(2, 320 * 3 + 7)
    a, lead = ss.process_input(wave, input_sample_hz=24000)
    b, _ = ss.process_input(wave)
    assert torch.equal(a, b) and a.shape == (2, 1, 320 * 3) and tuple(lead) == (2,)
    with pytest.raises(_lib.AlmError):                      # a different rate resamples: MI355X only
        ss.process_input(wave, input_sample_hz=16000)


def test_c_abi_rejects_bad_geometry():
    """argument checks run on the host before any launch (null pointers are never dereferenced)"""
    f = _lib.load().alm_resample_sinc
    g = _lib.load().alm_resample_sinc_bwd
    p = 4096                                                # fake non-null address: every call below is refused before a launch
    good = (p, 1000, p, 1500, p, 16, 2, 1000, 1500, 2, 3, 7, None)
    bad = [dict(len_out=1499), dict(taps=17), dict(rows=-1), dict(len_in=-1), dict(o=0), dict(W=-1), dict(ld_in=999)]
    names = ['x', 'ld_in', 'y', 'ld_out', 'table', 'taps', 'rows', 'len_in', 'len_out', 'o', 'n', 'W', 'stream']
    for b in bad:
        args = list(good)
        for k, v in b.items():
            args[names.index(k)] = v
        assert f(*args) == 10001, b
    assert f(p, 1000, p, 1500, p, 16, 0, 1000, 1500, 2, 3, 7, None) == 0           # no rows: nothing to do
    assert g(p, 1500, p, 1000, p, 16, 2, 1000, 1499, 2, 3, 7, None) == 10001
    assert g(p, 1500, p, 999, p, 16, 2, 1000, 1500, 2, 3, 7, None) == 10001       # ld_dx < len_in
