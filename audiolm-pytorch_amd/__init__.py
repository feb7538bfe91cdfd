"""audiolm_pytorch_amd -- MI355X (gfx950) native implementation of the audiolm-pytorch token-transformer training hot path.

The directory is called `audiolm-pytorch_amd/` (repo contract); import it as `audiolm_pytorch_amd` through the loader module
`audiolm_pytorch_amd.py` at the repo root.  `install_as_reference()` additionally registers these modules under the reference's
import paths (`audiolm_pytorch.audiolm_pytorch`, `.attend`, `.soundstream`, `.encodec`, `.t5`, `.hubert_kmeans`, `.vq_wav2vec`) so that an unmodified reference trainer.py picks
them up.
"""
from __future__ import annotations

import sys
import types

from . import _lib

_lib.load()            # no fallback path exists: fail at import, loudly, if libaudiolm_hip.so can neither be found nor built

from .attend import Attend  # noqa: E402
from .audiolm_pytorch import (AudioLM, CoarseTransformer, CoarseTransformerWrapper, FineTransformer, FineTransformerWrapper,
                              SemanticTransformer, SemanticTransformerWrapper, Transformer, get_embeds)
from .discriminators import ComplexSTFTDiscriminator, MultiScaleDiscriminator, gradient_penalty
from .encodec import EncodecWrapper
from .hubert_kmeans import HubertWithKmeans
from .mel_loss import MelSpectrogram, multi_spectral_recon_loss
from .optimizer import FusedAdam, get_optimizer
from .resample import resample
from .soundstream import AudioLMSoundStream, MusicLMSoundStream, SoundStream
from .t5 import T5Encoder, load_t5, register_t5, t5_encode_text
from .version import __version__
from .vq_wav2vec import FairseqVQWav2Vec


def install_as_reference():
    """Makes `from audiolm_pytorch.audiolm_pytorch import CoarseTransformer, ...` (reference trainer.py:36-48) resolve to this package."""
    from . import attend, audiolm_pytorch
    pkg = types.ModuleType('audiolm_pytorch')
    pkg.__path__ = []
    for name in ('SemanticTransformer', 'CoarseTransformer', 'FineTransformer', 'SemanticTransformerWrapper', 'CoarseTransformerWrapper',
                 'FineTransformerWrapper', 'AudioLM', 'get_embeds'):
        setattr(pkg, name, getattr(audiolm_pytorch, name))
    sys.modules['audiolm_pytorch'] = pkg
    sys.modules['audiolm_pytorch.audiolm_pytorch'] = audiolm_pytorch
    sys.modules['audiolm_pytorch.attend'] = attend
    from . import optimizer
    sys.modules['audiolm_pytorch.optimizer'] = optimizer          # trainer.py:32 `from audiolm_pytorch.optimizer import get_optimizer`
    try:
        from . import soundstream
        sys.modules['audiolm_pytorch.soundstream'] = soundstream
        pkg.SoundStream = soundstream.SoundStream
        pkg.AudioLMSoundStream, pkg.MusicLMSoundStream = soundstream.AudioLMSoundStream, soundstream.MusicLMSoundStream
    except ImportError:
        pass
    from . import hubert_kmeans
    sys.modules['audiolm_pytorch.hubert_kmeans'] = hubert_kmeans
    pkg.HubertWithKmeans = hubert_kmeans.HubertWithKmeans
    from . import vq_wav2vec
    sys.modules['audiolm_pytorch.vq_wav2vec'] = vq_wav2vec
    pkg.FairseqVQWav2Vec = vq_wav2vec.FairseqVQWav2Vec
    from . import encodec
    sys.modules['audiolm_pytorch.encodec'] = encodec              # trainer.py:37 `from audiolm_pytorch.encodec import EncodecWrapper`
    pkg.EncodecWrapper = encodec.EncodecWrapper
    from . import t5
    sys.modules['audiolm_pytorch.t5'] = t5                        # audiolm_pytorch.py:31 `from audiolm_pytorch.t5 import t5_encode_text, ...`
    pkg.t5 = t5
    return pkg
