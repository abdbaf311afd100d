"""MI355X-native CLIP-embedding + debiasing-adapter hot path.

Imported as `dbmm_amd` through the root shim dbmm_amd.py.
"""
__version__ = "0.1.0"

__all__ = ["analysis"]


def __getattr__(name):
    # `dbmm_amd.analysis` (group-wise embedding statistics and the representation report) without importing torch at package import
    if name == "analysis":
        import importlib
        return importlib.import_module(".analysis", __name__)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
