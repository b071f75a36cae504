"""The two image filters over row-major frames: the a-trous denoiser and temporal accumulation (rtmi_denoise,
rtmi_accumulate), and the state a sequence of accumulated frames carries."""
import ctypes as C

from ._abi import (ACCUMULATE_DEFAULTS, DENOISE_DEFAULTS, AccumulateOpts, DenoiseGuides, DenoiseOpts, RtmiError, _addr, _camera21,
                   _check, _fp, lib)
from ._tensors import _lead, _need, _new, _out_buffer, _ptr, _stream


def _extent(color, entry):
    """(torch, H, W, the device) of the frame whose ``color`` an ``entry`` filters."""
    torch = _lead(color, "color", entry, 3, "(H, W, 3)", False)
    return torch, int(color.shape[0]), int(color.shape[1]), color.device


def _guides(torch, h, w, dev, optional, **guides):
    """Every guide buffer by name: (H, W) for depth and alpha, (H, W, 3) for the rest, on color's device."""
    for name, t in guides.items():
        _need(t, name, (h, w) if name in ("depth", "alpha") else (h, w, 3), dev, torch.float32, where="color's", optional=optional)


def denoise(color, variance, normal, depth, alpha, albedo=None, iterations=DENOISE_DEFAULTS["iterations"],
            sigma_color=DENOISE_DEFAULTS["sigma_color"], sigma_depth=DENOISE_DEFAULTS["sigma_depth"],
            normal_squarings=DENOISE_DEFAULTS["normal_squarings"], demodulate=None, out=None, return_variance=False):
    """The variance- and feature-guided a-trous filter (rtmi_denoise; the rule is in include/rtmi.h), enqueued on torch's
    current stream.  Row-major contiguous CUDA float32 tensors on one device: ``color``, ``variance`` (of the pixel MEAN:
    ``Renderer.resolve_variance``), ``normal`` (the mean normal, not renormalised) and ``albedo`` (H, W, 3); ``depth`` and
    ``alpha`` (H, W).  Defaults: 5 iterations (steps 1, 2, 4, 8, 16 pixels), ``sigma_color`` 1 (standard errors of the two
    pixels), ``sigma_depth`` 0.05 (of the pixel's depth), 0 ``normal_squarings`` (the plain cosine of the mean normals, whose
    lengths are the pixels' coverage: a power of it lets covered neighbours outweigh a silhouette pixel itself).
    ``demodulate``: filter colour / albedo and multiply back; None means "when albedo is given".  ``out``: an optional
    (H, W, 3) tensor to write into, which may be ``color`` itself.  The call allocates its own scratch.  Returns the
    filtered image, or with ``return_variance`` (image, what is left of the variance)."""
    torch, h, w, dev = _extent(color, "rtmi_denoise")
    demodulate = (albedo is not None) if demodulate is None else bool(demodulate)
    if demodulate and albedo is None:
        raise RtmiError("demodulate needs an albedo")
    _guides(torch, h, w, dev, True, color=color, variance=variance, normal=normal, depth=depth, alpha=alpha, albedo=albedo)
    out = _out_buffer(out, "(H, W, 3)", (h, w, 3), dev, torch.float32, where="color's")
    out_var = _new(dev, (h, w, 3), torch.float32) if return_variance else None
    o = DenoiseOpts(C.sizeof(DenoiseOpts), int(iterations), int(normal_squarings), 1 if demodulate else 0,
                    float(sigma_color), float(sigma_depth))
    g = DenoiseGuides(C.sizeof(DenoiseGuides), 0, variance.data_ptr(), _addr(albedo), normal.data_ptr(), depth.data_ptr(),
                      alpha.data_ptr())
    L = lib()
    nbytes = int(L.rtmi_denoise_scratch_bytes(h, w))  # (0 for an extent the call refuses: it says why)
    # (freed on return, while the call is still queued: the caching allocator hands the block out again in this stream's order)
    scratch = _new(dev, (max(nbytes, 16),), torch.uint8)
    with torch.cuda.device(dev):
        _check(L.rtmi_denoise(h, w, C.byref(o), _ptr(color), C.byref(g), _ptr(out), _ptr(out_var), _ptr(scratch), nbytes,
                              _stream(dev)), "rtmi_denoise")
    return (out, out_var) if return_variance else out


def _known(opts):
    """opts itself, if rtmi.accumulate has every option it names."""
    unknown = set(opts) - set(ACCUMULATE_DEFAULTS)
    if unknown:
        raise RtmiError("rtmi.accumulate has no option %s" % ", ".join(sorted(unknown)))
    return opts


def accumulate(color, variance, normal, depth, alpha, camera, history=None, prev_camera=None, out_history=None, **opts):
    """Temporal accumulation (rtmi_accumulate; the rule is in include/rtmi.h), enqueued on torch's current stream.  Row-major
    contiguous CUDA float32 tensors on one device, as for ``denoise``: ``color``, ``variance`` and ``normal`` (H, W, 3),
    ``depth`` and ``alpha`` (H, W).  ``camera``: this frame's, the 21 floats of ``SceneBuilder.camera_get`` (any shape).
    ``history`` and ``prev_camera``: what the previous call returned as its history, and the camera of that frame; both None
    for the first frame.  ``out_history``: an optional uint8 tensor of ``rtmi_history_bytes(H, W)`` bytes to write the new
    history into (never ``history`` itself).  ``opts``: normal_min, depth_tolerance, min_blend (ACCUMULATE_DEFAULTS).
    Returns (color, variance, length, history): the accumulated image and its variance (H, W, 3), the number of frames
    each pixel holds (H, W), and the new history, a uint8 tensor that only the next call can read."""
    torch, h, w, dev = _extent(color, "rtmi_accumulate")
    opts = dict(ACCUMULATE_DEFAULTS, **_known(opts))
    _guides(torch, h, w, dev, False, color=color, variance=variance, normal=normal, depth=depth, alpha=alpha)
    if (history is None) != (prev_camera is None):
        raise RtmiError("history and prev_camera go together: both None (the first frame) or neither")
    L = lib()
    nbytes = int(L.rtmi_history_bytes(h, w))  # (0 for an extent the call refuses: it says why)
    for name, t in (("history", history), ("out_history", out_history)):
        _need(t, name, (nbytes,), dev, torch.uint8, of="rtmi_history_bytes(H, W) = %d bytes" % nbytes, where="color's", optional=True)
    if out_history is None:
        out_history = _new(dev, (max(nbytes, 16),), torch.uint8)[:nbytes]
    elif history is not None and out_history.data_ptr() == history.data_ptr():
        raise RtmiError("out_history must not be history: the call reads one while it writes the other")
    cur = _camera21(camera, "camera")
    prev = _camera21(prev_camera, "prev_camera") if prev_camera is not None else None
    out, out_var, length = (_new(dev, shape, torch.float32) for shape in ((h, w, 3), (h, w, 3), (h, w)))
    o = AccumulateOpts(C.sizeof(AccumulateOpts), 0, float(opts["normal_min"]), float(opts["depth_tolerance"]),
                       float(opts["min_blend"]))
    g = DenoiseGuides(C.sizeof(DenoiseGuides), 0, variance.data_ptr(), None, normal.data_ptr(), depth.data_ptr(), alpha.data_ptr())
    with torch.cuda.device(dev):
        _check(L.rtmi_accumulate(h, w, C.byref(o), _ptr(color), C.byref(g), cur.ctypes.data_as(_fp), _ptr(history),
                                 prev.ctypes.data_as(_fp) if prev is not None else None, _ptr(out_history), _ptr(out), _ptr(out_var),
                                 _ptr(length), _stream(dev)), "rtmi_accumulate")
    return out, out_var, length, out_history


class Accumulator:
    """A sequence's accumulation state: the two histories ``rtmi.accumulate`` swaps between, and the previous frame's camera.
    ``height``, ``width``: the frames' extent; ``device``: a CUDA device (default: torch's current one); ``opts``:
    rtmi.accumulate's options, for every step."""

    def __init__(self, height, width, device=None, **opts):
        import torch
        self.opts = _known(opts)
        self.height, self.width = int(height), int(width)
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        nbytes = int(lib().rtmi_history_bytes(self.height, self.width))
        if nbytes == 0:
            raise RtmiError("height and width must be within 1..65535 (RTMI_MAX_EXTENT)")
        self._histories = [_new(self.device, (nbytes,), torch.uint8) for _ in range(2)]
        self.reset()

    def reset(self):
        """Forget the history: the next step is a first frame."""
        self.frames = 0
        self._prev_camera = None
        return self

    def step(self, color, variance, normal, depth, alpha, camera):
        """Accumulate one frame seen from ``camera`` (rtmi.accumulate's arguments) and swap the histories.  Returns
        (color, variance, length)."""
        cur = _camera21(camera, "camera").copy()
        first = self._prev_camera is None
        out, var, length, _ = accumulate(color, variance, normal, depth, alpha, cur,
                                         history=None if first else self._histories[0], prev_camera=self._prev_camera,
                                         out_history=self._histories[1], **self.opts)
        self._histories.reverse()
        self._prev_camera = cur
        self.frames += 1
        return out, var, length

    @property
    def history(self):
        """The history the last step wrote (what the next one reads)."""
        return self._histories[0]
