"""Restored tensors as image files (reference: NAFNet_base/basicsr/utils/img_util.py:42-104 `tensor2img` and :147-163
`imwrite`, used at basicsr/models/image_restoration_model.py:375-414,490-506).

    img = tensor2img(out)                       # BGR uint8 HWC numpy, as the reference's
    imwrite(img, "restored.png")                # cv2.imwrite's meaning: BGR in, an RGB file out
    with ImageWriter() as w:                    # the pipelined form: nothing waits for the device
        w.write(out, "restored.png")

A device tensor is quantised by nbp_img_quantize (clamp, normalise, * 255, round half to even, CHW -> HWC and the
channel swap in one pass) and turned into PNG scanlines by nbp_png_filter, so one byte per sample crosses to the
host; nbp_png_encode deflates there on a few threads.  cv2 is not needed.  PNG is the only format, 8 bits the only
depth.
"""
from __future__ import annotations

import ctypes
import os
import queue
import threading
from typing import List, Optional, Sequence, Tuple, Union

import numpy as np
import torch
from torch import Tensor

from ._lib import NBPError, call, lib

__all__ = ["tensor2img", "imwrite", "ImageWriter", "png_encode"]


# ---------------------------------------------------------------------------------------------- shapes
def _as_chw(t: Tensor) -> Tuple[Tensor, int]:
    """tensor2img's shapes: [1,C,H,W], [C,H,W] or [H,W] -> ([C,H,W], the number of dimensions after squeeze(0))"""
    t = t.detach().squeeze(0)
    n_dim = t.dim()
    if n_dim == 4:
        raise NotImplementedError("tensor2img: a batch of more than one image (the reference's make_grid) is not "
                                  "implemented; pass the images one by one")
    if n_dim not in (2, 3):
        raise TypeError(f"Only support 4D, 3D or 2D tensor. But received with dimension: {n_dim}")
    return (t if n_dim == 3 else t.unsqueeze(0)), n_dim


def _min_max(min_max: Sequence[float]) -> Tuple[float, float]:
    lo, hi = float(np.float32(min_max[0])), float(np.float32(min_max[1]))
    if not hi > lo:
        raise ValueError(f"min_max needs max > min, got {tuple(min_max)}")
    return lo, hi


# ---------------------------------------------------------------------------------------------- device steps
def _quantize(chw: Tensor, lo: float, hi: float, reverse: bool) -> Tensor:
    """float [C,H,W] on the device -> uint8 [H,W,C] on the device (nbp_img_quantize)"""
    C, H, W = chw.shape
    if C not in (1, 3):
        raise ValueError(f"device images have 1 or 3 channels, got {C}")
    src = chw.to(torch.float32).contiguous()
    dst = torch.empty((H, W, C), dtype=torch.uint8, device=src.device)
    with torch.cuda.device(src.device):
        call("img_quantize", src, dst, C, H, W, lo, hi, int(reverse))
    return dst


def _filter(hwc: Tensor) -> Tensor:
    """uint8 [H,W,C] on the device -> PNG scanlines uint8 [H, 1 + W*C] on the device (nbp_png_filter)"""
    H, W, C = hwc.shape
    out = torch.empty((H, 1 + W * C), dtype=torch.uint8, device=hwc.device)
    with torch.cuda.device(hwc.device):
        call("png_filter", hwc, out, H, W, C)
    return out


def png_encode(scanlines: np.ndarray, H: int, W: int, C: int, level: int = 1, nthreads: int = 8,
               out: Optional[np.ndarray] = None) -> np.ndarray:
    """nbp_png_encode: host scanlines (nbp_png_filter's output) -> the bytes of a PNG file, a view of `out` (a uint8
    array, by default a new one of nbp_png_encode_bound bytes).  The bytes do not depend on nthreads."""
    L = lib().dll
    scan = np.ascontiguousarray(scanlines, dtype=np.uint8).reshape(-1)
    if scan.size != H * (1 + W * C):
        raise ValueError(f"scanlines hold {scan.size} bytes, {H} x (1 + {W} * {C}) expected")
    if out is None:
        bound = L.nbp_png_encode_bound(H, W, C)
        if bound < 0:
            raise NBPError(f"nbp_png_encode_bound failed ({bound}): {L.nbp_last_error_string().decode()}")
        out = np.empty(bound, dtype=np.uint8)
    n = ctypes.c_long(0)
    rc = L.nbp_png_encode(scan.ctypes.data, H, W, C, level, nthreads, out.ctypes.data, out.size, ctypes.byref(n))
    if rc != 0:
        raise NBPError(f"nbp_png_encode failed ({rc}): {L.nbp_last_error_string().decode()}")
    return out[:n.value]


def _write_file(path: str, data: np.ndarray, auto_mkdir: bool = True) -> None:
    """the whole file or nothing: a temporary name in the same directory, then a rename"""
    path = os.fspath(path)
    if auto_mkdir:
        os.makedirs(os.path.abspath(os.path.dirname(path)), exist_ok=True)
    tmp = f"{path}.tmp{os.getpid()}_{threading.get_ident()}"
    try:
        with open(tmp, "wb") as f:
            f.write(memoryview(data))
        os.replace(tmp, path)
    except BaseException:
        try:
            os.unlink(tmp)
        except OSError:
            pass
        raise


# ---------------------------------------------------------------------------------------------- the reference's API
def tensor2img(tensor: Union[Tensor, List[Tensor]], rgb2bgr: bool = True, out_type=np.uint8,
               min_max: Sequence[float] = (0, 1)):
    """The reference's tensor2img for out_type np.uint8: clamp to min_max, normalise to [0, 1], `(x * 255).round()`
    (half to even) as uint8; [1,C,H,W] / [C,H,W] -> HWC (BGR when rgb2bgr and C == 3, HW when C == 1), [H,W] -> HW;
    a list gives a list (a list of one its only image, as the reference).  A device tensor is quantised on the device
    (1 or 3 channels) and crosses to the host as uint8; NaN becomes 0."""
    if not (torch.is_tensor(tensor) or (isinstance(tensor, list) and all(torch.is_tensor(t) for t in tensor))):
        raise TypeError(f"tensor or list of tensors expected, got {type(tensor)}")
    if np.dtype(out_type) != np.uint8:
        raise NotImplementedError("tensor2img: only out_type=np.uint8 is implemented")
    lo, hi = _min_max(min_max)
    result = []
    for t in ([tensor] if torch.is_tensor(tensor) else tensor):
        chw, n_dim = _as_chw(t)
        C = chw.shape[0]
        reverse = bool(rgb2bgr) and n_dim == 3 and C == 3
        if chw.is_cuda:
            img = _quantize(chw, lo, hi, reverse).cpu().numpy()
        else:
            x = chw.to(torch.float32)
            x = (x.clamp(lo, hi) - lo) / float(np.float32(hi) - np.float32(lo))
            x = torch.where(torch.isnan(x), torch.zeros_like(x), (x * 255.0).round())
            x = x.permute(1, 2, 0)
            img = (x.flip(-1) if reverse else x).contiguous().numpy().astype(np.uint8)
        if n_dim == 2 or C == 1:
            img = img.reshape(img.shape[0], img.shape[1])
        result.append(img)
    return result[0] if len(result) == 1 else result


def _device_hwc(img) -> Tensor:
    if not torch.cuda.is_available():
        raise NBPError("imwrite filters the scanlines on the GPU and none is available; there is no CPU fallback")
    t = img if torch.is_tensor(img) else torch.from_numpy(np.ascontiguousarray(img))
    if t.dtype != torch.uint8:
        raise TypeError(f"imwrite expects a uint8 image, got {t.dtype}")
    if t.dim() == 2:
        t = t.unsqueeze(-1)
    if t.dim() != 3 or t.shape[2] not in (1, 3):
        raise ValueError(f"imwrite expects [H,W], [H,W,1] or [H,W,3], got {tuple(t.shape)}")
    return t if t.is_cuda else t.cuda()


def imwrite(img, file_path: str, auto_mkdir: bool = True) -> bool:
    """cv2.imwrite's meaning for a PNG path: `img` is a BGR (or gray) uint8 HWC image, a numpy array or a device
    tensor, and the file holds RGB.  Returns True; waits for the device (ImageWriter does not)."""
    t = _device_hwc(img)
    H, W, C = t.shape
    scan = _filter(t.flip(-1).contiguous() if C == 3 else t.contiguous())
    _write_file(file_path, png_encode(scan.cpu().numpy(), H, W, C), auto_mkdir)
    return True


class ImageWriter:
    """Writes restored tensors as PNG files without making the caller wait for the device.

    write() enqueues, on the current stream, the quantiser, the filter and a copy of the scanlines into one of `depth`
    pinned host buffers, records an event and returns; it blocks only while all `depth` buffers are in flight.  One
    worker thread waits for the event, deflates on `nthreads` threads at zlib `level` (nbp_png_encode; the GIL is
    released) and writes the file through a temporary name and a rename.  flush() / close() / leaving the `with`
    block wait for the worker and raise the first error it met."""

    def __init__(self, nthreads: int = 8, level: int = 1, depth: int = 2) -> None:
        if not (isinstance(nthreads, int) and 1 <= nthreads <= 256):
            raise ValueError(f"nthreads must be an int within [1, 256], got {nthreads!r}")
        if not (isinstance(level, int) and 0 <= level <= 9):
            raise ValueError(f"level must be an int within [0, 9], got {level!r}")
        if not (isinstance(depth, int) and depth >= 1):
            raise ValueError(f"depth must be a positive int, got {depth!r}")
        self.nthreads, self.level, self.depth = nthreads, level, depth
        self.frames = 0                                   # files written so far
        self._pinned: List[Optional[Tensor]] = [None] * depth
        self._free: "queue.Queue[int]" = queue.Queue()
        for i in range(depth):
            self._free.put(i)
        self._jobs: "queue.Queue" = queue.Queue()
        self._error: Optional[BaseException] = None
        self._out: Optional[np.ndarray] = None            # the worker's PNG buffer, grown on demand
        self._thread: Optional[threading.Thread] = None
        self._closed = False

    # ------------------------------------------------------------------ producer side
    def write(self, tensor: Tensor, path: str, rgb2bgr: bool = True, min_max: Sequence[float] = (0, 1)) -> None:
        """Save `tensor` ([1,C,H,W], [C,H,W] or [H,W] on the device, C 1 or 3) at `path` as tensor2img(tensor,
        rgb2bgr, min_max=min_max) followed by cv2.imwrite would: the file's channel order is the tensor's when rgb2bgr
        is true and reversed when it is false."""
        if self._closed:
            raise RuntimeError("ImageWriter.write after close()")
        if not torch.is_tensor(tensor) or not tensor.is_cuda:
            raise TypeError("ImageWriter.write expects a tensor on the GPU")
        lo, hi = _min_max(min_max)
        chw, n_dim = _as_chw(tensor)
        C, H, W = chw.shape
        scan = _filter(_quantize(chw, lo, hi, (not rgb2bgr) and n_dim == 3 and C == 3))
        n = scan.numel()
        slot = self._free.get()                           # blocks only when the ring is full
        buf = self._pinned[slot]
        if buf is None or buf.numel() < n:
            buf = self._pinned[slot] = torch.empty(n, dtype=torch.uint8, pin_memory=True)
        with torch.cuda.device(scan.device):
            buf[:n].copy_(scan.view(-1), non_blocking=True)
            done = torch.cuda.Event()
            done.record()
        if self._thread is None:
            self._thread = threading.Thread(target=self._work, name="ImageWriter", daemon=True)
            self._thread.start()
        self._jobs.put((slot, done, n, H, W, C, os.fspath(path)))

    # ------------------------------------------------------------------ worker side
    def _work(self) -> None:
        while True:
            job = self._jobs.get()
            try:
                if job is None:
                    return
                slot, done, n, H, W, C, path = job
                try:
                    done.synchronize()
                    bound = lib().dll.nbp_png_encode_bound(H, W, C)
                    if self._out is None or self._out.size < bound:
                        self._out = np.empty(bound, dtype=np.uint8)
                    png = png_encode(self._pinned[slot][:n].numpy(), H, W, C, self.level, self.nthreads, self._out)
                    _write_file(path, png)
                    self.frames += 1
                except BaseException as e:  # kept for flush(); the ring goes on turning
                    if self._error is None:
                        self._error = e
                finally:
                    self._free.put(slot)
            finally:
                self._jobs.task_done()

    def flush(self) -> None:
        """wait until every frame handed to write() is on disk; raise the first error the worker met"""
        self._jobs.join()
        err, self._error = self._error, None
        if err is not None:
            raise err

    def close(self) -> None:
        """flush() and stop the worker; the writer cannot be used afterwards"""
        if self._closed:
            return
        self._closed = True
        try:
            self.flush()
        finally:
            if self._thread is not None:
                self._jobs.put(None)
                self._thread.join()
                self._thread = None
            self._pinned = [None] * self.depth

    def __enter__(self) -> "ImageWriter":
        return self

    def __exit__(self, exc_type, exc, tb) -> None:
        if exc_type is None:
            self.close()
        else:  # the body's exception wins; still leave no thread behind
            try:
                self.close()
            except BaseException:
                pass
