"""What the binding asks of a torch tensor before it hands its address to librtmi.so: one check with one sentence, the
pointer and stream values of a foreign call, and the allocation of an output.  torch is imported when a call needs it."""
import ctypes as C

from ._abi import RtmiError


_TORCH = None


def _torch():
    """torch, imported at the first call that needs it and remembered: an import statement per call shows in a loop of steps."""
    global _TORCH
    if _TORCH is None:
        import torch
        _TORCH = torch
    return _TORCH


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _ptrs(*tensors):
    """``_ptr`` of each, for the run of pointers a foreign call takes, without a Python call per tensor."""
    vp = C.c_void_p
    return [vp(t.data_ptr()) if t is not None else None for t in tensors]


def _stream(dev):
    """torch's current stream on dev, as a foreign call takes it."""
    return C.c_void_p(_torch().cuda.current_stream(dev).cuda_stream)


def _new(dev, shape, dtype, zero=False):
    """An output tensor on dev; ``zero``: it must start as zeros (else it must not pay for that)."""
    return (_torch().zeros if zero else _torch().empty)(shape, dtype=dtype, device=dev)


def _lead(t, name, entry, dims, words, strict):
    """torch itself, once ``t``, the tensor that gives ``entry`` its extent and device, is a CUDA tensor of ``dims``
    dimensions, the last of 3 (``strict``: and contiguous float32); raises before any GPU work otherwise."""
    try:
        import torch
    except ImportError:
        raise RtmiError("%s: torch is needed for %s" % (name, entry))
    if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dim() == dims and t.shape[-1] == 3 and
            (not strict or (t.dtype == torch.float32 and t.is_contiguous()))):
        raise RtmiError("%s must be a %sCUDA float32 tensor of shape %s: %s has no CPU path"
                        % (name, "contiguous " if strict else "", words, entry))
    return torch


def _check_batch(entry, origins, directions, t_max=None):
    """(N, the rays' device, t_max made contiguous) of a batch for ``entry``; raises before any GPU work unless
    origins and directions are (N, 3) CUDA float32 tensors on one device and t_max is None or (N,) float32 there."""
    try:
        import torch
    except ImportError:
        raise RtmiError("origins: torch is needed for %s" % entry)
    for what, a in (("origins", origins), ("directions", directions)):
        if not isinstance(a, torch.Tensor):
            raise RtmiError("%s must be a torch tensor" % what)
        if not a.is_cuda:
            raise RtmiError("%s is on the CPU: %s has no CPU path (move it to the scene's GPU)" % (what, entry))
        if a.dtype != torch.float32:
            raise RtmiError("%s must be float32, not %s" % (what, a.dtype))
        if a.dim() != 2 or a.shape[1] != 3:
            raise RtmiError("%s must have shape (N, 3), not %s" % (what, tuple(a.shape)))
    n = int(origins.shape[0])
    if directions.shape[0] != n:
        raise RtmiError("origins and directions differ in length")
    if origins.device != directions.device:
        raise RtmiError("origins and directions are on different devices")
    dev = origins.device
    if t_max is not None:
        if not (isinstance(t_max, torch.Tensor) and t_max.is_cuda and t_max.dtype == torch.float32 and
                t_max.shape == (n,) and t_max.device == dev):
            raise RtmiError("t_max must be a CUDA float32 tensor of shape (N,) on the rays' device")
        t_max = t_max.contiguous()
    return n, dev, t_max


def _need(t, name, shape, dev, *dtypes, words=None, of=None, where="the rays'", optional=False):
    """``t`` itself, which must be a contiguous CUDA tensor of one of ``dtypes`` and of ``shape`` on ``dev`` (``optional``:
    or None); ``words``: the shape as the refusal spells it (``of``: what stands for "shape ..." altogether), ``where``:
    whose device it names."""
    if t is None and optional:
        return None
    if not (isinstance(t, _torch().Tensor) and t.is_cuda and t.dtype in dtypes and t.shape == shape and t.is_contiguous()
            and t.device == dev):
        raise RtmiError("%s must be a contiguous CUDA %s tensor of %s on %s device"
                        % (name, " or ".join(str(d)[len("torch."):] for d in dtypes), of or "shape %s" % (words or shape,), where))
    return t


def _out_buffer(out, words, shape, dev, *dtypes, zero=False, name="out", where="the rays'"):
    """A new tensor of the first of dtypes for out=None (``zero``: of zeros), else out itself, which must match."""
    if out is None:
        return _new(dev, shape, dtypes[0], zero)
    return _need(out, name, shape, dev, *dtypes, words=words, where=where)
