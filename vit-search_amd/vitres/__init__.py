"""vitres: MI355X-native ViT-Res / ViT-ResNAS (super)network hot path.

Python host side mirroring the reference's timm-style surface (create_model / network_def /
supernet_config / engine), executing through libvitres_hip.so (include/vitres_hip.h).

The model side (torch, the network factories) is imported on first use of one of the names below, not with the package: a
DataLoader worker that only decodes (`import vitres.jpeg`: numpy and libvitres_jpeg.so) loads neither torch nor the HIP runtime.
"""
import importlib

__all__ = ["create_model", "register_model", "list_models", "supernet_config"]


def __getattr__(name):
    if name in ("create_model", "register_model", "list_models"):
        importlib.import_module(".nets.vit_sr_supernet", __name__)   # registers the model factories
        return getattr(importlib.import_module(".registry", __name__), name)
    if name == "supernet_config":
        return importlib.import_module(".supernet_config", __name__)
    raise AttributeError("module %r has no attribute %r" % (__name__, name))


def __dir__():
    return sorted(list(globals()) + __all__)
