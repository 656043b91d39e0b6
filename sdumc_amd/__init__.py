"""sdumc_amd: import the submodule you need (engine, data, evaluate, model, ...); nothing loads the HIP library before that.
eval_epoch / EvalResult / TrainRecord / saliency_epoch / SaliencyResult are also reachable from the package itself (resolved on first
use)."""
_LAZY = {"eval_epoch": "evaluate", "EvalResult": "evaluate", "TrainRecord": "record", "saliency_epoch": "saliency",
         "SaliencyResult": "saliency"}
__all__ = sorted(_LAZY)


def __getattr__(name):
    if name in _LAZY:
        import importlib
        return getattr(importlib.import_module("." + _LAZY[name], __name__), name)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
