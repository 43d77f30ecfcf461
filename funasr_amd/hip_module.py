"""Base class of the host-side mirrors: an nn.Module that only HOLDS parameters (same state_dict keys as the
reference module, so load_pretrained_model(strict=True) -- funasr/train_utils/load_pretrained_model.py:104 -- keeps
working) while all arithmetic is done by an opaque handle of libparaformer_hip.so.

Weights are pushed to the handle lazily before the first forward after any change (load_state_dict, .to(),
in-place edits followed by mark_dirty()). There is deliberately no CPU implementation behind forward().
"""
from __future__ import annotations

import ctypes as C

import torch
import torch.nn as nn

from . import _lib


class ParamHolder(nn.Module):
    """weight / bias container with torch-style names; never executed."""

    def __init__(self, weight_shape, bias_shape=None):
        super().__init__()
        self.weight = nn.Parameter(torch.zeros(*weight_shape), requires_grad=False)
        if bias_shape is not None:
            self.bias = nn.Parameter(torch.zeros(*bias_shape), requires_grad=False)
        else:
            self.register_parameter("bias", None)

    def forward(self, *a, **k):  # pragma: no cover
        raise RuntimeError("parameter holder: computation happens inside libparaformer_hip.so")


class Holder(nn.Module):
    """plain namespace module (children give the dotted key names)"""

    def forward(self, *a, **k):  # pragma: no cover
        raise RuntimeError("parameter holder: computation happens inside libparaformer_hip.so")


def linear(out_f, in_f, bias=True):
    return ParamHolder((out_f, in_f), (out_f,) if bias else None)


def layer_norm(dim):
    return ParamHolder((dim,), (dim,))


def depthwise(channels, k):
    return ParamHolder((channels, 1, k), None)


def _truthy(v) -> bool:
    """a yaml / omegaconf boolean in any of its spellings"""
    return v in (True, 1, "true", "True")


class HipModule(nn.Module):
    """Owns one C handle. Subclasses set _create / _destroy / _set_tensor names and _skip_keys."""

    _prefix = ""              # e.g. "pf_encoder"
    _skip_keys: tuple = ()    # state_dict keys the device does not need (training-only tensors)
    _push_buffers = False     # True: buffers (BatchNorm's running statistics) reach the handle beside the parameters

    def __init__(self):
        super().__init__()
        self._handle = None
        self._dirty = True
        self._handle_device = None

    # -- lifecycle ---------------------------------------------------------------------------------------------
    def _make_config(self):  # pragma: no cover - abstract
        raise NotImplementedError

    def _device(self) -> torch.device:
        for p in self.parameters():
            return p.device
        return torch.device("cuda", torch.cuda.current_device()) if torch.cuda.is_available() else torch.device("cpu")

    def _ensure_handle(self):
        dev = self._device()
        if dev.type != "cuda":
            raise RuntimeError(
                f"{type(self).__name__} runs only on an AMD GPU through libparaformer_hip.so; parameters are on "
                f"'{dev}'. Move the model with .to('cuda') (there is no CPU fallback by design).")
        lib = _lib.load()
        if self._handle is not None and self._handle_device != dev:
            self._free()
        if self._handle is None:
            with torch.cuda.device(dev):
                cfg = self._make_config()
                create = getattr(lib, getattr(self, "_create_name", None) or self._prefix + "_create")
                h = create(C.byref(cfg)) if cfg is not None else create(*self._create_args())
                self._handle = _lib.check_handle(h, self._prefix + "_create")
                self._after_create(lib, self._handle)
            self._handle_device = dev
            self._dirty = True
        if self._dirty:
            self._push_weights(lib)
            self._dirty = False
        return lib, self._handle

    def _create_args(self):  # for handles created from scalars instead of a config struct
        return ()

    def _after_create(self, lib, handle):  # settings that register further tensors, before the first set_tensor
        pass

    def _extra_tensors(self):  # (name, tensor) pairs built on the host that are no part of the state_dict (positional tables)
        return ()

    def _push_weights(self, lib):
        set_tensor = getattr(lib, getattr(self, "_set_tensor_name", None) or self._prefix + "_set_tensor")
        named = list(self.named_parameters())
        if self._push_buffers:
            named += [(n, b) for n, b in self.named_buffers() if not n.endswith("num_batches_tracked")]
        named += list(self._extra_tensors())
        with torch.cuda.device(self._handle_device):
            for name, p in named:
                if name in self._skip_keys or any(name.startswith(s) for s in self._skip_keys if s.endswith(".")):
                    continue
                t = p.detach().to(device=self._handle_device, dtype=torch.float32).contiguous()
                _lib.check(set_tensor(self._handle, name.encode(), t.data_ptr(), t.numel()),
                           f"{self._prefix}_set_tensor({name})")
            torch.cuda.synchronize()

    def mark_dirty(self):
        self._dirty = True

    def _free(self):
        h = self.__dict__.get("_handle")
        if h is not None:
            try:
                getattr(_lib.load(), self._prefix + "_destroy")(h)
            except Exception:
                pass
            self.__dict__["_handle"] = None      # not nn.Module.__setattr__: it is unusable at interpreter exit

    def __del__(self):
        try:
            self._free()
        except Exception:
            pass

    # -- keep the device copy coherent with nn.Module mutations ------------------------------------------------------
    def _apply(self, fn, *args, **kwargs):
        out = super()._apply(fn, *args, **kwargs)
        self._dirty = True
        return out

    def load_state_dict(self, *args, **kwargs):
        out = super().load_state_dict(*args, **kwargs)
        self._dirty = True
        return out

    def _load_from_state_dict(self, *args, **kwargs):
        super()._load_from_state_dict(*args, **kwargs)
        self._dirty = True


def stream_ptr() -> int:
    return torch.cuda.current_stream().cuda_stream


def device_lens(vals, device, dtype=torch.int32) -> torch.Tensor:
    """A lengths tensor on the device made WITHOUT waiting for the stream: `torch.tensor(list, device=cuda)` copies from pageable
    memory and synchronises behind everything already enqueued -- the kernel launch this tensor usually follows -- which turns every
    module's forward into a blocking call. Here: pinned staging, asynchronous copy, and the host values kept on the tensor
    (`_pf_host`) so that `host_i32` hands them back without a D2H copy (which would synchronise again)."""
    vals = [int(v) for v in vals]
    dev = torch.device(device)
    if dev.type != "cuda":
        t = torch.tensor(vals, dtype=dtype, device=dev)
    else:
        host = torch.empty(len(vals), dtype=dtype, pin_memory=True)
        host.copy_(torch.tensor(vals, dtype=dtype))
        t = host.to(dev, non_blocking=True)
    t._pf_host = vals
    return t


def host_i32(x, n=None):
    """lengths -> (ctypes int32 array, python list). Accepts tensors (any device), lists, numpy."""
    if isinstance(x, torch.Tensor):
        known = getattr(x, "_pf_host", None)                         # device_lens: the values never left the host
        vals = list(known) if known is not None and len(known) == x.numel() else [int(v) for v in x.detach().cpu().reshape(-1).tolist()]
    else:
        vals = [int(v) for v in list(x)]
    if n is not None and len(vals) != n:
        raise ValueError(f"expected {n} lengths, got {len(vals)}")
    return (C.c_int32 * len(vals))(*vals), vals


class HostCopyRing:
    """Device -> pinned-host copies that a later `wait()` can consume without waiting for work enqueued AFTER the copy: the copy
    and an event are put on the stream at enqueue time (a plain `.cpu()` at collect time is ordered behind everything enqueued
    since, i.e. behind the whole next batch of a pipelined serving loop). A small ring of pinned buffers per (shape, dtype).
    A slot is OUTSTANDING from `start()` until the caller has finished with the tensor `wait()` returned -- marked by the next
    `wait()` / `start()` on the same handle being impossible, i.e. by `release()` or by waiting on a LATER handle of the same
    ring position. `start()` never hands out an outstanding slot (round-3 review: a serving loop with `depth` or more
    same-shape batches in flight silently read ids a later batch had overwritten): it takes a fresh pinned buffer instead."""

    class _Slot:
        __slots__ = ("buf", "outstanding")

        def __init__(self, buf):
            self.buf, self.outstanding = buf, False

    def __init__(self, depth: int = 4):
        self.depth, self._bufs, self._next = depth, {}, {}

    def start(self, t: torch.Tensor):
        key = (tuple(t.shape), t.dtype)
        ring = self._bufs.setdefault(key, [])
        if len(self._bufs) > 64:                                    # ragged serving loops: do not grow without bound
            self._bufs = {key: ring}
            self._next = {key: self._next.get(key, 0)}
        i = self._next.get(key, 0) % max(1, len(ring)) if ring else 0
        slot = None
        for k in range(len(ring)):                                  # the next slot nobody is still reading
            cand = ring[(i + k) % len(ring)]
            if not cand.outstanding:
                slot, i = cand, (i + k) % len(ring)
                break
        if slot is None:                                            # every slot is in flight: grow (never overwrite)
            slot = HostCopyRing._Slot(torch.empty(t.shape, dtype=t.dtype, pin_memory=True))
            ring.append(slot)
            i = len(ring) - 1
        self._next[key] = i + 1
        slot.outstanding = True
        slot.buf.copy_(t, non_blocking=True)
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream(t.device))
        return slot, ev

    @staticmethod
    def wait(handle) -> torch.Tensor:
        """The host tensor of a finished copy. The slot is handed back to the ring here: the caller must be done with the tensor
        (or have copied what it needs -- `collect()` turns it into Python lists at once) before the next `start()` on this
        ring may reuse it; callers that keep the tensor call `.clone()`."""
        slot, ev = handle
        ev.synchronize()
        slot.outstanding = False
        return slot.buf


class StagedUpload:
    """Host -> device copies of padded waveform batches for PIPELINED callers (AutoModel.inference's loop over batches): the batch is
    padded straight into pinned memory and copied on an UPLOAD stream, and the caller's stream waits for that copy only. A plain
    `wav.to(device)` from pageable memory is ordered behind everything already enqueued on the caller's stream -- the previous
    batch's encoder -- and blocks the host until then, which is exactly the wait a pipelined loop exists to remove. The pinned
    buffers come from torch's caching host allocator (it keeps a block busy until the copy's event has passed)."""

    def __init__(self):
        self._streams = {}

    def __call__(self, audio, device) -> "tuple[torch.Tensor, list]":
        dev = torch.device(device)
        lens = [int(a.shape[0]) for a in audio]
        host = torch.empty(len(audio), max(lens), dtype=torch.float32, pin_memory=True)
        for j, a in enumerate(audio):                               # pad_sequence(batch_first=True) of load_utils.py:413
            host[j, : lens[j]].copy_(a)
            host[j, lens[j]:].zero_()
        up = self._streams.get(dev)
        if up is None:
            up = self._streams[dev] = torch.cuda.Stream(device=dev)
        main = torch.cuda.current_stream(dev)
        with torch.cuda.stream(up):
            wav = host.to(dev, non_blocking=True)
        main.wait_stream(up)
        wav.record_stream(main)
        return wav, lens
