"""Host-side Python mirror of the render path (ctypes over librt_mi355x.so)."""


def __getattr__(name):
    if name == "ProbeVolume":  # rtamd.ProbeVolume, without importing numpy and the ctypes layer for `import rtamd` alone
        from .renderer import ProbeVolume
        return ProbeVolume
    if name == "ReflectionProbes":
        from .renderer import ReflectionProbes
        return ReflectionProbes
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
