"""fmri_hip: the gfx950 engine.  The sub-modules are imported by name (``fmri_hip.steps``, ``fmri_hip.build`` ...); the
public classes below are resolved on first use, so that ``import fmri_hip.build`` needs neither torch nor the library."""

_LAZY = {"DiffAugment": "augment", "VoxelAugment": "voxaug"}


def __getattr__(name):
    mod = _LAZY.get(name)
    if mod is None:
        raise AttributeError(f"module 'fmri_hip' has no attribute {name!r}")
    import importlib
    return getattr(importlib.import_module(f"{__name__}.{mod}"), name)
