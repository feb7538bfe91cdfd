"""What the frozen, inference-only fp32 models (HubertWithKmeans, FairseqVQWav2Vec, T5Encoder, EncodecWrapper) share on the host: a parameter tree registered under the
checkpoint's own key names, the key checks, and one cache of derived tensors."""
from __future__ import annotations

import os

import torch
from torch import nn

F32 = torch.float32


def load_weights(path):
    """a local checkpoint file -> what it holds, on the CPU: .safetensors through that package (ImportError where it is not installed), anything
    else through torch.load(weights_only=True)"""
    path = os.fspath(path)
    if path.endswith('.safetensors'):
        from safetensors.torch import load_file
        return load_file(path, device='cpu')
    return torch.load(path, map_location='cpu', weights_only=True)


def _reset(module, incompatible_keys):
    module._cache.clear()
    if hasattr(module, '_fold'):
        module._fold()


class _Node(nn.Module):
    """a named slot of the parameter tree (never called: the kernels read the tensors)"""


class FrozenModel(nn.Module):
    """A module whose parameters are frozen fp32 copies of checkpoint tensors, kept under the checkpoint's dotted names so that its state dict loads
    by name; the kernels read the tensors, no submodule is ever called.

    `_cache` holds whatever is derived from the parameters and the device they are on (the name -> parameter dict, the [Cout, Cin, 1] views the
    Linear layers are launched with, MFMA images, per-length tables).  It is emptied by every `_apply` (.to / .cuda / .float ...) and after
    `load_state_dict`, which then also calls `self._fold()` where the subclass defines one.  Assigning a new Parameter object by hand is not seen:
    the cache goes stale exactly as a subclass's folded buffers (`_qkv_w*`, `_pos_w`) do, until the next load_state_dict or device move."""

    def _adopt(self, names, state_dict, what, allowed_extra=lambda key: False):
        """registers state_dict[n] for every n of `names`; KeyError when one is absent (`what` names the model in the message) or when the state dict
        holds a key that is neither in `names` nor passes `allowed_extra`"""
        missing = [n for n in names if n not in state_dict]
        if missing:
            raise self._lacks(missing, what)
        known = set(names)
        extra = [k for k in state_dict if k not in known and not allowed_extra(k)]
        if extra:
            raise KeyError(f'unexpected entries in the state dict: {extra[:6]}')
        for n in names:
            self._slot(n).register_parameter(n.rsplit('.', 1)[-1], nn.Parameter(state_dict[n].detach().to(F32).clone().contiguous(), requires_grad=False))
        self._cache = {}
        self.register_load_state_dict_post_hook(_reset)

    @staticmethod
    def _lacks(missing, what):
        return KeyError(f'the state dict lacks {len(missing)} entries of {what}: {missing[:6]}' + (' ...' if len(missing) > 6 else ''))

    def _slot(self, name):
        """the node that holds the leaf of the dotted `name`, created on the way"""
        node = self
        for part in name.split('.')[:-1]:
            if part not in node._modules:
                node.add_module(part, _Node())
            node = node._modules[part]
        return node

    def _apply(self, fn, *args, **kwargs):
        self._cache.clear()
        return super()._apply(fn, *args, **kwargs)

    def _cached(self, key, make):
        if key not in self._cache:
            self._cache[key] = make()
        return self._cache[key]

    def _params(self):
        return self._cached('params', lambda: dict(self.named_parameters()))

    def _linear(self, name):
        """the Linear weight `name` in the [Cout, Cin, 1] form of ops.conv1d_valid"""
        return self._cached(('linear', name), lambda: self._params()[name].unsqueeze(-1))
