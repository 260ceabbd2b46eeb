"""The compiled extension (``vgate._C``), loaded on first use, and the per-device buffer key."""
from __future__ import annotations

import os

import torch

# C.gemm's integer codes (the extension binds no names for them): ``path``, the kernel family a plan asks
# for, mirrors enum GemmPath in csrc/kernels/launchers.h; the epilogue argument mirrors enum GemmEpi in
# csrc/kernels/gemm_epilogue.h (Python never passes its EPI_BF16_AR)
PATH_AUTO, PATH_PREFILL, PATH_MID, PATH_STREAMK, PATH_KX = range(5)
EPI_BF16, EPI_F32, EPI_SILU, EPI_QKV = range(4)

_C = None
_C_ERR: Exception | None = None


def _dev_key(device) -> str:
    """Key of the per-device buffers: "cuda" and "cuda:<current>" name the same device."""
    d = torch.device(device)
    if d.type == "cuda" and d.index is None:
        d = torch.device("cuda", torch.cuda.current_device())
    return str(d)


def native():
    """Return the compiled extension module, building it in-tree if needed."""
    global _C, _C_ERR
    if _C is not None:
        return _C
    try:
        from vgate import _C as mod  # type: ignore
        _C = mod
    except ImportError as e:  # pragma: no cover - depends on build state
        if os.environ.get("VGATE_AUTOBUILD", "1") == "1":
            try:
                import importlib
                import sys
                from pathlib import Path
                sys.path.insert(0, str(Path(__file__).resolve().parents[2] / "csrc"))
                import build as _build  # type: ignore
                _build.build(verbose=False)
                _C = importlib.import_module("vgate._C")
                return _C
            except Exception as e2:  # noqa: BLE001
                _C_ERR = e2
        else:
            _C_ERR = e
        raise RuntimeError(f"vgate native extension unavailable: {_C_ERR}") from _C_ERR
    return _C


def native_available() -> bool:
    try:
        native()
        return True
    except RuntimeError:
        return False
