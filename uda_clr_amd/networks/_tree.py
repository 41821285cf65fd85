"""Parameter-tree helpers.

The product network keeps ``torch.nn.Conv2d`` / ``torch.nn.BatchNorm2d`` objects ONLY as named
parameter holders: they are created in the reference's construction order so that a seeded
``torch.manual_seed(s); DeepLab(...)`` yields bit-identical initial weights and identical
``state_dict`` keys; their own ``forward`` is never called - the compute runs
in ``uda_clr_amd.engine`` on the HIP kernels.
"""
import math
import os

import torch
import torch.nn as nn


class Holder(nn.Module):
    """A container whose children are addressed by state-dict path components."""

    def forward(self, *a, **k):  # pragma: no cover - never used
        raise RuntimeError("parameter holder: compute runs in uda_clr_amd.engine, not in submodules")

    def __getitem__(self, idx):
        return self._modules[str(idx)]

    def __len__(self):
        return len(self._modules)


def child(root: nn.Module, path: str, leaf: nn.Module = None) -> nn.Module:
    """Walk/create ``Holder`` containers along a dotted path and attach ``leaf`` at its end."""
    parts = path.split(".")
    node = root
    for p in parts[:-1] if leaf is not None else parts:
        if p not in node._modules:
            node.add_module(p, Holder())
        node = node._modules[p]
    if leaf is not None:
        node.add_module(parts[-1], leaf)
        return leaf
    return node


def load_known_keys(module, env):
    """The reference's key-filtered loaders (mobilenet.py:124-133, resnet.py:138-146): the entries of the state dict at the path in
    the environment variable ``env`` whose keys ``module`` has; unset means the seeded initialisation stands."""
    path = os.environ.get(env)
    if not path:
        return
    pre = torch.load(path, map_location="cpu", weights_only=True)
    own = module.state_dict()
    own.update({k: v for k, v in pre.items() if k in own})
    module.load_state_dict(own)


def conv(ci, co, k, stride=1, pad=0, dil=1, groups=1, bias=False):
    return nn.Conv2d(ci, co, k, stride, pad, dil, groups, bias)


def normal_bn_init(modules, bn_types):
    """The backbones' own pass (resnet.py:126-136, xception.py:234-245, drn.py:159-169): conv weights N(0, 2 / (k*k*out)), BN
    weight 1 / bias 0."""
    for m in modules:
        if isinstance(m, nn.Conv2d):
            n = m.kernel_size[0] * m.kernel_size[1] * m.out_channels
            m.weight.data.normal_(0, math.sqrt(2. / n))
        elif isinstance(m, bn_types):
            m.weight.data.fill_(1)
            m.bias.data.zero_()


def kaiming_bn_init(modules, bn_types):
    """The reference's ``_init_weight`` / ``_initialize_weights`` pass (aspp.py:24-33,
    decoder.py:58-72, mobilenet.py:135-151): He-normal conv weights, BN weight 1 / bias 0."""
    for m in modules:
        if isinstance(m, nn.Conv2d):
            nn.init.kaiming_normal_(m.weight)
        elif isinstance(m, bn_types):
            m.weight.data.fill_(1)
            m.bias.data.zero_()
