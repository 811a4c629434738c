"""Sony SID dataset, HBM-resident: every distinct frame is decoded once and kept on the device as uint16; a batch
is a few RNG draws on the host, a few hundred bytes of descriptors over PCIe and one gather launch.

``SonySIDLMDBDataset`` inflates a full-resolution PNG16 (one serial DEFLATE stream) again for every crop drawn from
it, so the host decode rate bounds a training loop.  An MI355X has the memory to hold the whole Sony training split
as uint16 (about 2 000 frames of 2848 x 4256 x 3 x 2 B = 72.7 MB, about 150 GB of the 288 GB), so here:

  * plan (host, at construction): the PNG headers of the filtered entries give the distinct frames, keyed by
    ``(client, key)`` -- a long frame shared by several short exposures is stored once -- their byte sizes and the
    total, which is checked against the budget before anything is decoded or allocated;
  * build (host + device, at the first ``crop_batch`` or an explicit ``build()``, never in ``__init__`` or
    ``__getitem__``): each distinct frame is decoded whole by the native decoder on ``decode_threads`` host threads
    into a small ring of pinned staging buffers and uploaded into its own device tensor; then the pointer table and
    the frame sizes go to the device.  Host memory in flight is the ring, never the dataset;
  * ``__getitem__``: no pixels -- the reference's string / ratio fields and a descriptor (short frame, long frame,
    top, left, height, width), the crop drawn from the same ``numpy.random.default_rng(seed)`` in the same order as
    ``SonySIDLMDBDataset``;
  * ``crop_batch`` (device, sid_resident.hip, ``nbp_sid_crop_to_float``): cuts the windows out of the resident frames
    and writes the reference's float32 batch, bit-identical to ``nbp_sid_to_float`` on the host-cropped arrays.

Opt-in: ``create_dataloader`` runs this class with ``num_workers=0`` and ``CUDAPrefetcher`` / ``to_reference_batch``
call ``crop_batch`` for its batches; everything about ``SonySIDLMDBDataset`` is unchanged.
"""
from __future__ import annotations

import concurrent.futures as cf
from collections import deque
from dataclasses import dataclass
from typing import Dict, List, Mapping, Optional, Sequence, Tuple

import numpy as np
import torch

from .._lib import NBPError, call, host_call
from .sony_sid_lmdb_dataset import SonySIDLMDBDataset, _check_three_channels, png_shape

FrameKey = Tuple[str, str]  # (client key: "short" / "long", storage key)

# With max_bytes=None the plan is checked against the free device memory at build time less this reserve, kept for
# the training step (a 16 x 256^2 step of the headline configuration needs 3-10 GB) and the allocator's rounding.
RESERVE_BYTES = 16 << 30
MAX_BATCH = 65535  # grid.z of the gather launch


@dataclass(frozen=True)
class ResidentPlan:
    """What the build will put on the device."""
    frames: Tuple[FrameKey, ...]          # the distinct frames, in first-use order
    shapes: Tuple[Tuple[int, int], ...]   # rows, columns of each
    nbytes: Tuple[int, ...]               # rows * columns * 3 * 2
    total_bytes: int
    pairs: Tuple[Tuple[int, int], ...]    # per manifest entry: (short frame index, long frame index)


def distinct_frames(entries: Sequence[dict]) -> List[FrameKey]:
    """The (client, key) of every frame the entries name, each once, in first-use order."""
    seen: Dict[FrameKey, None] = {}
    for e in entries:
        seen.setdefault(("short", e["short_key"]))
        seen.setdefault(("long", e["long_key"]))
    return list(seen)


def check_budget(need: int, budget: int, what: str = "max_bytes") -> None:
    if need > budget:
        raise ValueError(f"The resident SID dataset needs {need} bytes of device memory, above the budget of "
                         f"{budget} bytes ({what}).")


def _worst_window(h: int, w: int, patch_size: Optional[int], phase: str, random_crop: bool
                  ) -> Optional[Tuple[int, int, int, int]]:
    """The window of a short frame that reaches furthest down and right (None: the patch does not fit, which
    __getitem__ reports as the base class does)."""
    if patch_size is None or phase != "train":
        return 0, 0, h, w
    if patch_size > h or patch_size > w:
        return None
    if random_crop:
        return h - patch_size, w - patch_size, patch_size, patch_size
    return (h - patch_size) // 2, (w - patch_size) // 2, patch_size, patch_size


def plan_resident(entries: Sequence[dict], shapes: Mapping[FrameKey, Tuple[int, int, int]],
                  patch_size: Optional[int] = None, phase: str = "train", random_crop: bool = True,
                  max_bytes: Optional[int] = None) -> ResidentPlan:
    """Pure host planning: `entries` are the filtered manifest records, `shapes` the (H, W, C) of each frame's PNG
    header.  Raises ValueError for a frame that is not 3-channel, a long frame smaller than a window its short
    partner can draw, or a total above `max_bytes`."""
    frames = distinct_frames(entries)
    index = {k: i for i, k in enumerate(frames)}
    hw = []
    for k in frames:
        _check_three_channels(tuple(shapes[k]))
        hw.append((int(shapes[k][0]), int(shapes[k][1])))
    pairs = []
    for e in entries:
        si, li = index[("short", e["short_key"])], index[("long", e["long_key"])]
        window = _worst_window(hw[si][0], hw[si][1], patch_size, phase, random_crop)
        if window is not None and (window[0] + window[2] > hw[li][0] or window[1] + window[3] > hw[li][1]):
            raise ValueError(f"Long-exposure image {tuple(shapes[frames[li]])} is smaller than the crop window "
                             f"{window}.")
        pairs.append((si, li))
    nbytes = tuple(h * w * 3 * 2 for h, w in hw)
    total = sum(nbytes)
    if max_bytes is not None:
        check_budget(total, int(max_bytes))
    return ResidentPlan(tuple(frames), tuple(hw), nbytes, total, tuple(pairs))


class _Resident:
    """The device state: one uint16 (int16-typed) tensor per frame, the pointer table and the frame sizes."""

    def __init__(self, frames: List[torch.Tensor], device: torch.device):
        self.frames = frames
        self.device = device
        self.ptrs = torch.tensor([t.data_ptr() for t in frames], dtype=torch.int64).to(device)
        self.hw = torch.tensor([[t.shape[0], t.shape[1]] for t in frames], dtype=torch.int32).to(device)


class SonySIDResidentDataset(SonySIDLMDBDataset):
    """SonySIDLMDBDataset whose frames live on the device (see the module docstring).  Same options, manifest
    filtering, backends and exceptions, plus ``resident: {"device": "cuda", "max_bytes": None, "decode_threads": 8}``.
    The plan is made at construction (PNG headers only); the decode + upload runs once, at the first ``crop_batch``
    or an explicit ``build()``."""

    def __init__(self, opt: dict):
        super().__init__(opt)
        res = dict(opt.get("resident") or {})
        self.resident_device = res.get("device", "cuda")
        self.max_bytes: Optional[int] = res.get("max_bytes")
        self.decode_threads = max(1, int(res.get("decode_threads", 8)))
        self._resident: Optional[_Resident] = None
        shapes = {k: self._header_shape(*k) for k in distinct_frames(self.entries)}
        self.plan = plan_resident(self.entries, shapes, self.patch_size, self.phase, self.random_crop, self.max_bytes)

    def _header_shape(self, client: str, key: str) -> Tuple[int, int, int]:
        return png_shape(self._fetch_bytes(key, client_key=client))

    def __getstate__(self):
        # a pickled copy (a worker process) carries the plan, never the device tensors or the native LMDB handles
        state = self.__dict__.copy()
        state["_resident"] = None
        state["file_client"] = None
        return state

    def __getitem__(self, index: int) -> dict:
        pair = index // self.samples_per_pair
        si, li = self.plan.pairs[pair]
        h, w = self.plan.shapes[si]
        top, left, ch, cw = self._crop_window(h, w)
        sample = self._fields(self.entries[pair])
        sample["desc"] = torch.tensor([si, li, top, left, ch, cw], dtype=torch.int32)
        return sample

    # ---------------------------------------------------------------------------------------------------- build
    def _decode_into(self, i: int, slot: torch.Tensor) -> None:
        client, key = self.plan.frames[i]
        h, w = self.plan.shapes[i]
        buf = self._fetch_bytes(key, client_key=client)
        if png_shape(buf) != (h, w, 3):
            raise ValueError(f"Frame {key!r} changed since it was planned as {(h, w, 3)}.")
        try:
            host_call("png_decode_rgb16", buf, len(buf), slot.data_ptr(), 0, 0, h, w)
        except NBPError as e:
            raise ValueError(f"Failed to decode PNG buffer into an image: {key!r}: {e}") from e

    def build(self) -> "_Resident":
        """Decode every distinct frame once and upload it (idempotent).  Ends with a device synchronise, so any
        stream may read the frames afterwards."""
        if self._resident is not None:
            return self._resident
        if not torch.cuda.is_available():
            raise RuntimeError("SonySIDResidentDataset: the frames are kept on the GPU, and none is available")
        if self.io_backend_type == "lmdb" and self.file_client is None:
            raise RuntimeError("SonySIDResidentDataset: an unpickled copy cannot build; build in the process that "
                               "constructed the dataset")
        plan = self.plan
        device = torch.device(self.resident_device)
        if self.max_bytes is None:
            free, _ = torch.cuda.mem_get_info(device)
            check_budget(plan.total_bytes, free - RESERVE_BYTES,
                         f"{free} bytes free on the device less a reserve of {RESERVE_BYTES}")
        n = len(plan.frames)
        slots = min(self.decode_threads, n)
        ring = [torch.empty(max(plan.nbytes) // 2, dtype=torch.int16, pin_memory=True) for _ in range(slots)]
        frames: List[torch.Tensor] = []
        inflight = deque()
        copied = torch.cuda.Event()
        with cf.ThreadPoolExecutor(max_workers=slots) as pool:
            for i in range(slots):
                inflight.append((i, pool.submit(self._decode_into, i, ring[i])))
            nxt = slots
            try:
                while inflight:
                    slot, fut = inflight.popleft()
                    fut.result()
                    i = len(frames)
                    h, w = plan.shapes[i]
                    dev = torch.empty((h, w, 3), dtype=torch.int16, device=device)
                    dev.view(-1).copy_(ring[slot][:h * w * 3], non_blocking=True)
                    copied.record()
                    frames.append(dev)
                    copied.synchronize()  # the staging buffer is free again
                    if nxt < n:
                        inflight.append((slot, pool.submit(self._decode_into, nxt, ring[slot])))
                        nxt += 1
            except BaseException:
                for _, fut in inflight:
                    fut.cancel()
                raise
        self._resident = _Resident(frames, device)
        torch.cuda.synchronize(device)
        return self._resident

    # ----------------------------------------------------------------------------------------------- crop_batch
    def check_descriptors(self, desc) -> np.ndarray:
        """Host validation of a [B][6] descriptor batch (short frame, long frame, top, left, height, width); returns
        it as an int64 array, or raises ValueError naming the first bad sample."""
        d = desc.detach().cpu().numpy() if torch.is_tensor(desc) else np.asarray(desc)
        if d.ndim != 2 or d.shape[1] != 6 or not 0 < d.shape[0] <= MAX_BATCH or d.dtype.kind not in "iu":
            raise ValueError(f"Expected integer descriptors [B][6] with 0 < B <= {MAX_BATCH}, got "
                             f"{d.dtype} {tuple(d.shape)}.")
        d = d.astype(np.int64)
        h, w = int(d[0, 4]), int(d[0, 5])
        if h <= 0 or w <= 0 or (d[:, 4] != h).any() or (d[:, 5] != w).any():
            raise ValueError(f"The crop windows of a batch must have one positive size, got "
                             f"{sorted(set(map(tuple, d[:, 4:6].tolist())))}.")
        hw = np.asarray(self.plan.shapes, np.int64)
        for b, (si, li, top, left, _, _) in enumerate(d.tolist()):
            if not (0 <= si < len(hw) and 0 <= li < len(hw)):
                raise ValueError(f"Sample {b}: frame indices {(si, li)} outside [0, {len(hw)}).")
            for f in (si, li):
                if top < 0 or left < 0 or top + h > hw[f, 0] or left + w > hw[f, 1]:
                    raise ValueError(f"Sample {b}: the crop window {(top, left, h, w)} is outside frame {f} of "
                                     f"shape {tuple(hw[f].tolist())}.")
        return d

    def crop_batch(self, desc, ratio, out=None):
        """(lq, short_raw, gt) float32 [B][3][h][w] for a descriptor batch [B][6] and its exposure ratios (B values),
        enqueued on the current stream.  The descriptors are validated on the host first: a bad one raises
        ValueError and nothing is launched.  out=(lq, short_raw, gt) has the batch written into caller-owned
        contiguous float32 device tensors of that shape; nothing is allocated for the outputs then."""
        d = self.check_descriptors(desc)
        B, h, w = d.shape[0], int(d[0, 4]), int(d[0, 5])
        ratio = torch.as_tensor(ratio)
        if ratio.numel() != B:
            raise ValueError(f"Expected {B} exposure ratios, got {ratio.numel()}.")
        res = self.build()
        if out is None:
            out = tuple(torch.empty(B, 3, h, w, device=res.device) for _ in range(3))
        else:
            out = tuple(out)
            if len(out) != 3 or any(not torch.is_tensor(t) or t.device != res.frames[0].device
                                    or t.dtype != torch.float32 or tuple(t.shape) != (B, 3, h, w)
                                    or not t.is_contiguous() for t in out):
                raise ValueError(f"out must be three contiguous float32 tensors of shape {(B, 3, h, w)} on "
                                 f"{res.frames[0].device}.")
        dev_desc = torch.from_numpy(np.ascontiguousarray(d[:, :4], dtype=np.int32)).to(res.device, non_blocking=True)
        dev_ratio = ratio.reshape(B).to(device=res.device, dtype=torch.float32, non_blocking=True).contiguous()
        call("sid_crop_to_float", res.ptrs, res.hw, dev_desc, dev_ratio, B, len(res.frames), h, w, *out)
        return out
