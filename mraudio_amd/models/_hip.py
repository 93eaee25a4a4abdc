"""What the HIP encoder modules (``HipEvaViTg``, ``HipBEATs``) share: the library handle behind a ``torch.nn`` parameter container."""
from __future__ import annotations

import ctypes as C

import torch

from .. import _lib


class HipEncoder:
    """Mix-in in front of the stock module.  The subclass names the C symbol prefix (``_PREFIX``: ``mra_vit`` / ``mra_beats``), builds the
    ``cfg`` struct and calls ``_create``; ``forward`` stays with it.  Here: the device, the handle's lifetime, the dirty / ``_version``
    tracking of the parameters, their upload, the grow-only workspace and ``set_option``."""

    _PREFIX = ""

    def _fn(self, name: str):
        return getattr(_lib.lib(), f"{self._PREFIX}_{name}")

    def _call(self, name: str, *args, what: str = "") -> None:
        _lib.check(self._fn(name)(self._handle, *args), what or f"{self._PREFIX}_{name}")

    def _create(self, cfg, device) -> None:
        self._lib, self._C = _lib, C
        self._device = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        self._handle = C.c_void_p()
        with torch.cuda.device(self._device):
            _lib.check(self._fn("create")(C.byref(cfg), C.byref(self._handle)), f"{self._PREFIX}_create")
        self._dirty, self._ws = True, None
        self.to(self._device)

    def set_option(self, name: str, value: int) -> None:
        """Per-handle switch of the HIP encoder (``<prefix>_set_option``)."""
        self._call("set_option", name.encode(), int(value), what=f"{self._PREFIX}_set_option({name})")

    def _apply(self, fn, recurse=True):
        out = super()._apply(fn, recurse)
        self._dirty = True
        return out

    def load_state_dict(self, *a, **kw):
        res = super().load_state_dict(*a, **kw)
        self._dirty = True
        return res

    def __del__(self):
        try:
            if self._handle:
                self._fn("destroy")(self._handle)
                self._handle = C.c_void_p()
        except Exception:
            pass

    def _upload_tensors(self) -> dict:
        """Name -> tensor of everything ``sync_weights`` uploads (the library's parameter names)."""
        return self.state_dict()

    @torch.no_grad()
    def sync_weights(self) -> None:
        ver = sum(p._version for p in self.parameters())
        if ver != getattr(self, "_ver", None):
            self._ver, self._dirty = ver, True
        if not self._dirty:
            return
        with torch.cuda.device(self._device):
            for k, v in self._upload_tensors().items():
                t = v.detach().to(self._device)
                t = (t if t.dtype in (torch.float32, torch.float16, torch.bfloat16) else t.float()).contiguous()
                shape = (C.c_int64 * max(t.dim(), 1))(*t.shape)
                self._call("load", k.encode(), _lib.ptr(t), _lib.mra_dtype(t.dtype), shape, t.dim(), _lib.current_stream(), what=f"{self._PREFIX}_load({k})")
        self._dirty = False

    def _workspace(self, nbytes: int) -> torch.Tensor:
        """At least ``nbytes`` of scratch on the device (grow-only; call under ``torch.cuda.device(self._device)``)."""
        nbytes = (nbytes + 255) // 256 * 256
        if self._ws is None or self._ws.numel() < nbytes:
            self._ws = None
            self._ws = torch.empty(nbytes, dtype=torch.uint8, device=self._device)
        return self._ws
