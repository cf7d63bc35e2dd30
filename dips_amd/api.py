"""Host-side mirror of the reference operator surface, over the C ABI.

Reference surface (RubenMovsesyan/DiPs, crate ``dips``):
  DiPsFilter / ChromaFilter        dips/src/lib.rs:25-61
  DiPsProperties (builder)         dips/src/lib.rs:63-170
  ComputeState::new/add_texture/dispatch   dips/src/gpu/mod.rs:59, :170, :306
  frame_callback                   dips/src/lib.rs:233-246
plus the north-star batch path (per-frame difference series), which has no
reference counterpart beyond the per-pixel math of dips_shader.wgsl:64-82.
Every call goes to libdips_hip.so; there is no Python compute path.
"""
from __future__ import annotations

import ctypes
import enum
import math
from dataclasses import dataclass
from typing import Callable, Iterable, Iterator, List, Optional, Tuple

import numpy as np

from . import _lib
from ._lib import DipsError, DipsParams, check


class DiPsFilter(enum.IntEnum):
    """dips/src/lib.rs:25-41; the value is the WGSL override id 3 code."""
    Unfiltered = 255
    Sigmoid = 0
    InverseSigmoid = 1


class ChromaFilter(enum.IntEnum):
    """dips/src/lib.rs:43-61; the value is the WGSL override id 4 code."""
    None_ = 0
    Red = 1
    Green = 2
    Blue = 3


class PixelFormat(enum.IntEnum):
    Gray8 = _lib.FMT_GRAY8
    RGB8 = _lib.FMT_RGB8
    RGBA8 = _lib.FMT_RGBA8


class Mode(enum.IntEnum):
    Overall = _lib.MODE_OVERALL     # against frame 0 (README.md:7)
    PerFrame = _lib.MODE_PER_FRAME  # against the previous frame (README.md:8-10)


class MorphOp(enum.IntEnum):
    """The operation of dips_mask_morph."""
    Erode = _lib.MORPH_ERODE
    Dilate = _lib.MORPH_DILATE
    Open = _lib.MORPH_OPEN    # erode, then dilate
    Close = _lib.MORPH_CLOSE  # dilate, then erode


class MorphShape(enum.IntEnum):
    """The structuring element of dips_mask_morph."""
    Box = _lib.MORPH_BOX          # |dx| <= rx, |dy| <= ry
    Diamond = _lib.MORPH_DIAMOND  # |dx| + |dy| <= rx (ry == rx)


class MaskLogic(enum.IntEnum):
    """The operation of dips_mask_logic."""
    And = _lib.LOGIC_AND
    Or = _lib.LOGIC_OR
    Xor = _lib.LOGIC_XOR
    AndNot = _lib.LOGIC_ANDNOT  # a & ~b
    Not = _lib.LOGIC_NOT        # ~a inside the region; takes no b


class VideoPathNotSpecifiedError(Exception):
    """dips/src/lib.rs:173-186"""


class FrameCallbackNotSpecifiedError(Exception):
    """dips/src/lib.rs:188-201"""


class DiPsProperties:
    """Builder mirroring dips/src/lib.rs:63-170 (defaults :74-86)."""

    def __init__(self) -> None:
        self._video_path: Optional[str] = None
        self._frame_callback: Optional[Callable] = None
        self._output_path: Optional[str] = None
        self.colorize_: bool = False
        self.spatial_window_size_: int = 1
        self.sensitivity_: float = 5.0
        self.filter_type_: DiPsFilter = DiPsFilter.Unfiltered
        self.chroma_filter_: ChromaFilter = ChromaFilter.None_

    @classmethod
    def new(cls) -> "DiPsProperties":
        return cls()

    def video_path(self, p: str) -> "DiPsProperties":
        self._video_path = str(p)
        return self

    def frame_callback(self, cb: Callable) -> "DiPsProperties":
        self._frame_callback = cb
        return self

    def output_path(self, p: str) -> "DiPsProperties":
        self._output_path = str(p)
        return self

    def colorize(self, v: bool) -> "DiPsProperties":
        self.colorize_ = bool(v)
        return self

    def spatial_window_size(self, v: int) -> "DiPsProperties":
        self.spatial_window_size_ = int(v)
        return self

    def sensitivity(self, v: float) -> "DiPsProperties":
        self.sensitivity_ = float(v)
        return self

    def filter_type(self, v: DiPsFilter) -> "DiPsProperties":
        self.filter_type_ = DiPsFilter(v)
        return self

    def chroma_filter(self, v: ChromaFilter) -> "DiPsProperties":
        self.chroma_filter_ = ChromaFilter(v)
        return self

    def get_video_path(self) -> Optional[str]:
        return self._video_path

    def get_output_path(self) -> Optional[str]:
        return self._output_path

    def get_frame_callback(self) -> Optional[Callable]:
        return self._frame_callback

    def build(self) -> "DiPsProperties":
        out = DiPsProperties()
        out.__dict__.update(self.__dict__)
        return out


def _params(colorize=False, spatial_window_size=1, sensitivity=5.0,
            filter_type=DiPsFilter.Unfiltered, chroma_filter=ChromaFilter.None_,
            mode=Mode.Overall, fmt=PixelFormat.RGB8, tau=0.0, flags=0) -> DipsParams:
    p = DipsParams()
    check(_lib.load().dips_params_default(ctypes.byref(p)))
    p.colorize = 1 if colorize else 0
    p.spatial_window_size = int(spatial_window_size)
    p.sensitivity = float(sensitivity)
    p.filter_type = int(filter_type)
    p.chroma_filter = int(chroma_filter)
    p.mode = int(mode)
    p.format = int(fmt)
    p.tau = float(tau)
    p.flags = int(flags)
    return p


class _Handle:
    def __init__(self, params: DipsParams, device: int = 0):
        self._lib = _lib.load()
        h = ctypes.c_void_p()
        st = self._lib.dips_create(ctypes.byref(params), int(device), ctypes.byref(h))
        check(st, None)
        self._h = h
        self.params = params
        self.device = device

    @property
    def ptr(self) -> ctypes.c_void_p:
        if self._h is None:
            raise DipsError(_lib.DIPS_ERR_STATE, "handle destroyed")
        return self._h

    def close(self) -> None:
        if getattr(self, "_h", None) is not None:
            self._lib.dips_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def check(self, st: int) -> int:
        return check(st, self._h)


def _stream_of(hd: "_Handle", tensor, stream=None) -> "_lib.on_stream":
    """`hd` bound to `stream` (default: the tensor's current stream) for one
    call, then back to its own stream (see _lib.on_stream)."""
    if stream is None:
        import torch
        stream = torch.cuda.current_stream(tensor.device).cuda_stream
    return _lib.on_stream(hd._lib.dips_set_stream, hd.ptr, hd.check, stream)


def _as_u8(frame) -> np.ndarray:
    a = np.ascontiguousarray(frame)
    if a.dtype != np.uint8:
        a = a.astype(np.uint8)
    return a


class ComputeState:
    """Drop-in for dips/src/gpu/mod.rs ComputeState on a HIP device."""

    def __init__(self, colorize: bool, spatial_window_size: int, sensitivity: float,
                 filter_type: DiPsFilter, chroma_filter: ChromaFilter, device: int = 0,
                 time_kernel: bool = False, crosscheck: bool = False):
        """crosscheck: the plain kernels and transfers (DIPS_FLAG_CROSSCHECK):
        same outputs, for tests."""
        flags = (_lib.FLAG_TIME_KERNEL if time_kernel else 0) | (_lib.FLAG_CROSSCHECK if crosscheck else 0)
        self._hd = _Handle(_params(colorize, spatial_window_size, sensitivity, filter_type,
                                   chroma_filter, fmt=PixelFormat.RGBA8, flags=flags), device)
        self._dev: Optional[_Handle] = None
        self._w = 0
        self._h = 0

    @classmethod
    def new(cls, colorize, spatial_window_size, sensitivity, filter_type, chroma_filter,
            device: int = 0) -> "ComputeState":
        return cls(colorize, spatial_window_size, sensitivity, filter_type, chroma_filter, device)

    def add_texture(self, width: int, height: int, frame_data) -> None:
        a = _as_u8(frame_data)
        self._hd.check(self._hd._lib.dips_add_texture(self._hd.ptr, width, height,
                                                      a.ctypes.data, a.nbytes))
        self._w, self._h = width, height

    def dispatch(self) -> Optional[np.ndarray]:
        """gpu/mod.rs:306-397: None only while the ring warms up (frames
        0..2); a device or argument error raises DipsError (the reference's
        wgpu path panics), so None never hides a failure."""
        out = np.empty((self._h, self._w, 4), dtype=np.uint8)
        r = self._hd.check(self._hd._lib.dips_dispatch(self._hd.ptr, out.ctypes.data, out.nbytes))
        return out if r == 1 else None

    def frame_callback_batch(self, width: int, height: int, frames) -> np.ndarray:
        """len(frames) consecutive frame_callback calls (dips/src/lib.rs:233-246)
        in one pass over HBM (dips_frame_callback_batch); frames [N, H, W, 4]."""
        a = _as_u8(frames)
        if a.size % (width * height * 4) != 0:
            raise ValueError("frames must be [N, height, width, 4] RGBA8")
        n = a.size // (width * height * 4)
        out = np.empty((n, height, width, 4), dtype=np.uint8)
        self._hd.check(self._hd._lib.dips_frame_callback_batch(self._hd.ptr, width, height, a.ctypes.data, n,
                                                               out.ctypes.data))
        self._w, self._h = width, height
        return out

    def frame_callback_batch_device(self, frames, out, stream=None) -> None:
        """Device form: uint8 HIP tensors [N, H, W, 4], asynchronous on the
        tensor's current stream.  Keeps its own ComputeState, separate from
        the host-pointer calls of this object."""
        n, h, w = int(frames.shape[0]), int(frames.shape[1]), int(frames.shape[2])
        if tuple(frames.shape) != (n, h, w, 4) or tuple(out.shape) != tuple(frames.shape):
            raise ValueError("frames/out must be [N, H, W, 4] uint8 tensors")
        for t in (frames, out):
            if not t.is_cuda or not t.is_contiguous():
                raise ValueError("device path needs contiguous HIP tensors")
        dv = self._device_handle()
        with _stream_of(dv, frames, stream):
            dv.check(dv._lib.dips_frame_callback_batch(dv.ptr, w, h, frames.data_ptr(), n, out.data_ptr()))

    def _device_handle(self) -> "_Handle":
        """The device-pointer twin handle (own ComputeState)."""
        if self._dev is None:
            p = DipsParams()
            ctypes.memmove(ctypes.byref(p), ctypes.byref(self._hd.params), ctypes.sizeof(p))
            p.flags |= _lib.FLAG_DEVICE_PTRS
            self._dev = _Handle(p, self._hd.device)
        return self._dev

    # -- frame-range sharding (3-frame halo + start texture) --
    def frame_callback_batch_sharded(self, comm, width: int, height: int, frames, n_total: int) -> np.ndarray:
        """dips_frame_callback_batch_sharded on host arrays: this rank's
        frames [n_local, H, W, 4] (its shard_range of n_total) through a
        fresh ComputeState, the outputs one ComputeState over all frames
        gives them; the library exchanges the 3-frame halo and broadcasts the
        start texture."""
        a = _as_u8(frames)
        if a.size % (width * height * 4) != 0:
            raise ValueError("frames must be [N, height, width, 4] RGBA8")
        n = a.size // (width * height * 4)
        out = np.empty((n, height, width, 4), dtype=np.uint8)
        self._hd.check(self._hd._lib.dips_frame_callback_batch_sharded(
            self._hd.ptr, comm.ptr, width, height, a.ctypes.data, n, int(n_total), out.ctypes.data))
        self._w, self._h = width, height
        return out

    def frame_callback_batch_sharded_device(self, comm, frames, out, n_total: int, stream=None) -> None:
        """The same on uint8 HIP tensors [n_local, H, W, 4] (the device
        handle, asynchronous on the tensor's current stream)."""
        n, h, w = int(frames.shape[0]), int(frames.shape[1]), int(frames.shape[2])
        if tuple(frames.shape) != (n, h, w, 4) or tuple(out.shape) != tuple(frames.shape):
            raise ValueError("frames/out must be [N, H, W, 4] uint8 tensors")
        for t in (frames, out):
            if not t.is_cuda or not t.is_contiguous():
                raise ValueError("device path needs contiguous HIP tensors")
        dv = self._device_handle()
        with _stream_of(dv, frames, stream):
            dv.check(dv._lib.dips_frame_callback_batch_sharded(dv.ptr, comm.ptr, w, h, frames.data_ptr(), n,
                                                               int(n_total), out.data_ptr()))

    def resume(self, width: int, height: int, start, halo, t0: int) -> None:
        """Continue as if frame_callback had seen global frames 0..t0-1
        (t0 >= 7, any window): `start` is the start texture of the handle that
        saw frames 0..3, `halo` the raw RGBA8 frames t0-3..t0-1 ([3, H, W, 4])."""
        s, hl = _as_u8(start), _as_u8(halo)
        if s.size != width * height * 4 or hl.size != 3 * width * height * 4:
            raise ValueError("start must be [H, W, 4] and halo [3, H, W, 4] RGBA8")
        self._hd.check(self._hd._lib.dips_compat_resume(self._hd.ptr, width, height, s.ctypes.data,
                                                        hl.ctypes.data, int(t0)))
        self._w, self._h = width, height

    def resume_device(self, start, halo, t0: int, stream=None) -> None:
        """Device form of resume (uint8 HIP tensors), for the device handle
        that frame_callback_batch_device drives."""
        h, w = int(start.shape[0]), int(start.shape[1])
        if tuple(start.shape) != (h, w, 4) or tuple(halo.shape) != (3, h, w, 4):
            raise ValueError("start must be [H, W, 4] and halo [3, H, W, 4] uint8 tensors")
        for t in (start, halo):
            if not t.is_cuda or not t.is_contiguous():
                raise ValueError("device path needs contiguous HIP tensors")
        dv = self._device_handle()
        with _stream_of(dv, start, stream):
            dv.check(dv._lib.dips_compat_resume(dv.ptr, w, h, start.data_ptr(), halo.data_ptr(), int(t0)))

    def start_texture_device(self, out, stream=None) -> bool:
        """The device handle's start texture into a uint8 HIP tensor [H, W, 4]
        (asynchronous); False while it is not built yet."""
        dv = self._device_handle()
        with _stream_of(dv, out, stream):
            return dv.check(dv._lib.dips_start_texture(dv.ptr, out.data_ptr(), out.numel())) == 1

    def kernel_time(self, reset: bool = False) -> Tuple[float, int]:
        """hipEvent time of the batch kernel on the device handle (time_kernel=True)."""
        ms, cnt = ctypes.c_double(), ctypes.c_uint64()
        hd = self._dev
        if hd is None:
            return 0.0, 0
        hd.check(hd._lib.dips_kernel_time(hd.ptr, ctypes.byref(ms), ctypes.byref(cnt)))
        if reset:
            hd.check(hd._lib.dips_kernel_time_reset(hd.ptr))
        return ms.value, cnt.value

    CALLBACK_PHASES = ("sync_us", "staged_us", "launched_us", "kernels_us", "wall_us", "pack_cpu_us",
                       "expand_cpu_us", "wait_cpu_us", "threads", "stripes", "expand_start_us")

    def callback_phases(self) -> Optional[dict]:
        """Where the last zero-copy frame_callback spent its time
        (dips_callback_phases; None before the first such call)."""
        v = (ctypes.c_double * len(self.CALLBACK_PHASES))()
        n = ctypes.c_uint32()
        st = self._hd._lib.dips_callback_phases(self._hd.ptr, v, len(v), ctypes.byref(n))
        if st == _lib.DIPS_ERR_STATE:
            return None
        self._hd.check(st)
        return dict(zip(self.CALLBACK_PHASES, list(v)[: n.value]))

    def start_texture(self) -> Optional[np.ndarray]:
        out = np.empty((self._h, self._w, 4), dtype=np.uint8)
        r = self._hd.check(self._hd._lib.dips_start_texture(self._hd.ptr, out.ctypes.data, out.nbytes))
        return out if r == 1 else None

    def close(self) -> None:
        self._hd.close()
        if self._dev is not None:
            self._dev.close()


def frame_callback(width: int, height: int, frame_data, compute: ComputeState) -> np.ndarray:
    """dips/src/lib.rs:233-246 through the C ABI's dips_frame_callback: the
    visualisation, or the input passed through while the ring warms up; an
    error raises DipsError instead of passing the input through."""
    a = _as_u8(frame_data)
    out = np.empty((height, width, 4), dtype=np.uint8)
    compute._hd.check(compute._hd._lib.dips_frame_callback(
        compute._hd.ptr, width, height, a.ctypes.data, a.nbytes, out.ctypes.data, out.nbytes))
    compute._w, compute._h = width, height
    return out


def perform_dips_frames(properties: DiPsProperties, frames: Iterable, width: int, height: int,
                        device: int = 0, batch: int = 0) -> Iterator[np.ndarray]:
    """perform_dips (dips/src/lib.rs:252-257) minus the GStreamer decode
    front-end (out of scope): runs the frame callback over an iterable of
    RGBA8 frames and yields the callback's outputs in order.  With the
    default callback and batch > 0, frames are grouped `batch` at a time
    through dips_frame_callback_batch (same outputs, one device pass each)."""
    cs = ComputeState(properties.colorize_, properties.spatial_window_size_,
                      properties.sensitivity_, properties.filter_type_,
                      properties.chroma_filter_, device)
    cb = properties.get_frame_callback()
    try:
        if cb is None and batch > 0:
            pending = []
            for f in frames:
                pending.append(np.asarray(f, dtype=np.uint8).reshape(height, width, 4))
                if len(pending) == batch:
                    yield from cs.frame_callback_batch(width, height, np.stack(pending))
                    pending = []
            if pending:
                yield from cs.frame_callback_batch(width, height, np.stack(pending))
            return
        cb = cb or frame_callback
        for f in frames:
            yield cb(width, height, f, cs)
    finally:
        cs.close()


# ---------------------------------------------------------------------------
# Batch difference series (north-star path)
# ---------------------------------------------------------------------------

@dataclass
class Series:
    """Per-frame difference series (see dips_series_entry in dips_hip.h)."""
    sad: np.ndarray       # uint64 [N]
    sj: np.ndarray        # uint64 [N]
    count: np.ndarray     # uint64 [N]
    si_fixed: np.ndarray  # uint64 [N]

    @property
    def si(self) -> np.ndarray:
        return np.ldexp(self.si_fixed.astype(np.float64), -32)

    @property
    def sj_norm(self) -> np.ndarray:
        return self.sj.astype(np.float64) / 510.0

    def as_array(self) -> np.ndarray:
        return np.stack([self.sad, self.sj, self.count, self.si_fixed], axis=1)

    @classmethod
    def from_array(cls, a: np.ndarray) -> "Series":
        a = np.asarray(a, dtype=np.uint64).reshape(-1, 4)
        return cls(a[:, 0].copy(), a[:, 1].copy(), a[:, 2].copy(), a[:, 3].copy())


@dataclass
class GridSeries:
    """The difference series per cell of a rows x cols grid
    (dips_diff_series_grid): every field uint64 [N, rows, cols]."""
    sad: np.ndarray
    sj: np.ndarray
    count: np.ndarray
    si_fixed: np.ndarray

    @property
    def si(self) -> np.ndarray:
        return np.ldexp(self.si_fixed.astype(np.float64), -32)

    def as_array(self) -> np.ndarray:
        """[N, rows, cols, 4]: sad, sj, count, si_fixed."""
        return np.stack([self.sad, self.sj, self.count, self.si_fixed], axis=-1)

    @classmethod
    def from_array(cls, a: np.ndarray) -> "GridSeries":
        a = np.asarray(a, dtype=np.uint64)
        return cls(a[..., 0].copy(), a[..., 1].copy(), a[..., 2].copy(), a[..., 3].copy())


@dataclass
class PixelSums:
    """The difference series summed over time per pixel of a region
    (dips_diff_pixel_sums): every field uint64 [h, w]."""
    sad: np.ndarray
    sj: np.ndarray
    count: np.ndarray
    si_fixed: np.ndarray

    @property
    def si(self) -> np.ndarray:
        return np.ldexp(self.si_fixed.astype(np.float64), -32)

    def as_array(self) -> np.ndarray:
        """[h, w, 4]: sad, sj, count, si_fixed."""
        return np.stack([self.sad, self.sj, self.count, self.si_fixed], axis=-1)

    @classmethod
    def from_array(cls, a: np.ndarray) -> "PixelSums":
        a = np.asarray(a, dtype=np.uint64)
        if a.ndim != 3 or a.shape[2] != 4:
            raise ValueError("pixel sums must be [h, w, 4]")
        return cls(a[..., 0].copy(), a[..., 1].copy(), a[..., 2].copy(), a[..., 3].copy())


def mask_row_bytes(width: int) -> int:
    """Bytes of one row of a change mask of a region `width` pixels wide
    (dips_mask_row_bytes): 4 * ceil(width / 32)."""
    if int(width) < 0 or int(width) > 0xFFFFFFFF:
        raise ValueError("width must be a non-negative 32-bit integer")
    return int(_lib.load().dips_mask_row_bytes(int(width)))


@dataclass
class ChangeMask:
    """The per-frame change mask of a region (dips_diff_change_mask): `bits`
    uint8 [n, h, row_bytes], one bit per pixel, bit i of a row = bit (i & 7)
    of byte (i >> 3), pad bits 0; `width` the region's width in pixels."""
    bits: np.ndarray
    width: int

    def unpack(self) -> np.ndarray:
        """bool [n, h, w]: whether pixel (i, j) changed in frame t."""
        return np.unpackbits(self.bits, axis=-1, bitorder="little")[..., :self.width].astype(bool)

    def counts(self) -> np.ndarray:
        """uint64 [n]: changed pixels per frame (the series' count)."""
        n = self.bits.shape[0]
        return np.unpackbits(self.bits.reshape(n, -1), axis=1).sum(axis=1, dtype=np.uint64)

    @classmethod
    def from_array(cls, a: np.ndarray, width: int) -> "ChangeMask":
        a = np.ascontiguousarray(a, dtype=np.uint8)
        if a.ndim != 3 or int(width) < 0 or a.shape[2] != 4 * ((int(width) + 31) // 32):
            raise ValueError("mask must be [n, h, 4 * ceil(width / 32)] bytes")
        return cls(a, int(width))


@dataclass
class PixelTimes:
    """The change times per pixel of a region (dips_diff_pixel_times): every
    field uint32 [h, w].  `first` / `last`: the global index of the first /
    last frame in which the pixel changed (NONE: it never did); `run_max`:
    the longest run of consecutive frames in which it changed; `run_cur`:
    the run that ends at the newest frame folded."""
    first: np.ndarray
    last: np.ndarray
    run_max: np.ndarray
    run_cur: np.ndarray

    NONE = _lib.TIME_NONE

    def as_array(self) -> np.ndarray:
        """[4, h, w]: first, last, run_max, run_cur (the C ABI's planes)."""
        return np.stack([self.first, self.last, self.run_max, self.run_cur], axis=0)

    @classmethod
    def from_array(cls, a: np.ndarray) -> "PixelTimes":
        a = np.asarray(a, dtype=np.uint32)
        if a.ndim != 3 or a.shape[0] != 4:
            raise ValueError("pixel times must be [4, h, w]")
        return cls(a[0].copy(), a[1].copy(), a[2].copy(), a[3].copy())


@dataclass
class Background:
    """The running-average background of a region
    (dips_diff_background_mask): `state` uint16 [C, h, w], per channel plane
    the average in 8.8 fixed point (0 .. 65280)."""
    state: np.ndarray

    def image(self) -> np.ndarray:
        """uint8 [h, w, C]: the background rounded to bytes, (state + 128) >>
        8 -- what the decision compares a frame with; a `ref` for every other
        product of the same region."""
        r = (self.state.astype(np.uint32) + 128) >> 8
        return np.ascontiguousarray(np.moveaxis(r, 0, -1).astype(np.uint8))

    @classmethod
    def from_array(cls, a: np.ndarray) -> "Background":
        a = np.ascontiguousarray(a, dtype=np.uint16)
        if a.ndim != 3 or a.shape[0] not in (1, 3, 4):
            raise ValueError("background state must be [C, h, w] with C of 1, 3 or 4")
        return cls(a)


def _background_args(rate_shift, selective) -> Tuple[int, int]:
    """rate_shift and bg_flags of dips_diff_background_mask, checked."""
    if isinstance(rate_shift, bool) or int(rate_shift) != rate_shift or not 0 <= int(rate_shift) <= _lib.BG_MAX_RATE_SHIFT:
        raise ValueError(f"rate_shift must be an integer 0 .. {_lib.BG_MAX_RATE_SHIFT}")
    return int(rate_shift), _lib.BG_SELECTIVE if selective else 0


@dataclass
class SigmaDelta:
    """The Sigma-Delta background of a region (dips_diff_sigma_delta_mask):
    `state` uint16 [2, h, w], plane 0 the running median M of the integer
    intensity J (0 .. 510), plane 1 the per-pixel threshold V."""
    state: np.ndarray

    @property
    def median(self) -> np.ndarray:
        """uint16 [h, w]: M, in units of J (twice an 8-bit intensity)."""
        return self.state[0]

    @property
    def threshold(self) -> np.ndarray:
        """uint16 [h, w]: V, the deviation of J a pixel must exceed to fire."""
        return self.state[1]

    @classmethod
    def from_array(cls, a: np.ndarray) -> "SigmaDelta":
        a = np.ascontiguousarray(a, dtype=np.uint16)
        if a.ndim != 3 or a.shape[0] != _lib.SD_PLANES:
            raise ValueError("Sigma-Delta state must be [2, h, w]")
        return cls(a)


def _sigma_delta_args(n_amp, v_min, v_max) -> Tuple[int, int, int]:
    """n_amp, v_min and v_max of dips_diff_sigma_delta_mask, checked."""
    for v in (n_amp, v_min, v_max):
        if isinstance(v, bool) or int(v) != v:
            raise ValueError("n_amp, v_min and v_max must be integers")
    n_amp, v_min, v_max = int(n_amp), int(v_min), int(v_max)
    if not 1 <= n_amp <= _lib.SD_MAX_AMP:
        raise ValueError(f"n_amp must be 1 .. {_lib.SD_MAX_AMP}")
    if not 0 <= v_min <= v_max <= _lib.SD_MAX_V:
        raise ValueError(f"0 <= v_min <= v_max <= {_lib.SD_MAX_V} is required")
    return n_amp, v_min, v_max


def _sigma_delta_option(sigma_delta) -> Tuple[int, int, int]:
    """The sigma_delta= argument of change_boxes / change_tracks: True (the
    defaults of sigma_delta_mask) or (n_amp, v_min, v_max)."""
    if sigma_delta is True:
        return _sigma_delta_args(2, 2, _lib.SD_MAX_V)
    if not isinstance(sigma_delta, (tuple, list)) or len(sigma_delta) != 3:
        raise ValueError("sigma_delta must be True or (n_amp, v_min, v_max)")
    return _sigma_delta_args(*sigma_delta)


@dataclass
class ChangeBoxes:
    """The connected components of a change mask (dips_mask_components):
    `counts` uint32 [n], the kept components per frame (not capped by K);
    `boxes` uint32 [n, K, 8], record k of frame t = its k-th kept component
    by ascending anchor (FIELDS: x0, y0, x1, y1, area, anchor, cx256, cy256;
    the box is [x0, x1) x [y0, y1), the centroid in 1/256 pixel), zeros past
    min(counts[t], K); `labels` uint32 [n, h, w] (0: clear or dropped, else
    1 + the record's index) or None."""
    counts: np.ndarray
    boxes: np.ndarray
    labels: Optional[np.ndarray] = None

    FIELDS = _lib.BOX_FIELDS

    def frame(self, t: int) -> np.ndarray:
        """uint32 [m, 8]: the m = min(counts[t], K) valid records of frame t."""
        return self.boxes[t, :min(int(self.counts[t]), self.boxes.shape[1])]

    @property
    def truncated(self) -> np.ndarray:
        """bool [n]: frames with more kept components than records."""
        return self.counts > self.boxes.shape[1]

    def as_arrays(self) -> Tuple[np.ndarray, np.ndarray, Optional[np.ndarray]]:
        return self.counts, self.boxes, self.labels

    @classmethod
    def from_arrays(cls, counts, boxes, labels=None) -> "ChangeBoxes":
        counts = np.ascontiguousarray(counts, dtype=np.uint32)
        boxes = np.ascontiguousarray(boxes, dtype=np.uint32)
        if counts.ndim != 1 or boxes.ndim != 3 or boxes.shape[0] != counts.shape[0] or boxes.shape[2] != _lib.BOX_WORDS:
            raise ValueError("counts must be [n] and boxes [n, K, 8]")
        if labels is not None:
            labels = np.ascontiguousarray(labels, dtype=np.uint32)
            if labels.ndim != 3 or labels.shape[0] != counts.shape[0]:
                raise ValueError("labels must be [n, h, w]")
        return cls(counts, boxes, labels)


def _components_args(connectivity, min_area, max_boxes, chunk_frames, n: int) -> Tuple[int, int, int, int]:
    """The scalar arguments of dips_mask_components, checked."""
    if int(connectivity) not in (4, 8):
        raise ValueError("connectivity must be 4 or 8")
    for name, v in (("min_area", min_area), ("max_boxes", max_boxes), ("chunk_frames", chunk_frames)):
        if int(v) < 0 or int(v) > 0xFFFFFFFF:
            raise ValueError(f"{name} must be a non-negative 32-bit integer")
    if n * int(max_boxes) * _lib.BOX_WORDS >= 1 << 32:
        raise ValueError("n_frames * max_boxes * 8 must stay below 2^32")
    return int(connectivity), int(min_area), int(max_boxes), int(chunk_frames)


@dataclass
class ChangeTracks:
    """The components of a change mask linked across frames
    (dips_mask_tracks): `counts` and `boxes` as in ChangeBoxes; `links`
    uint32 [n, K, 4], per record (FIELDS: prev, overlap, track, age) the
    record of the frame before it shares the most pixels with (NONE: none)
    and that overlap, the id of its track and the frames the track has lasted
    before this one; {NONE, 0, NONE, 0} past min(counts[t], K); `state`
    uint32 [1 + 2K] (the next unused id, then track and age of the last
    frame's records: what the next call of a longer clip continues from) or
    None."""
    counts: np.ndarray
    boxes: np.ndarray
    links: np.ndarray
    state: Optional[np.ndarray] = None

    FIELDS = _lib.LINK_FIELDS
    NONE = _lib.LINK_NONE

    def frame(self, t: int) -> Tuple[np.ndarray, np.ndarray]:
        """(uint32 [m, 8], uint32 [m, 4]): the m = min(counts[t], K) valid
        records of frame t and their links."""
        m = min(int(self.counts[t]), self.boxes.shape[1])
        return self.boxes[t, :m], self.links[t, :m]

    def tracks(self) -> dict:
        """id -> [(t, k), ...]: the records of every track, in frame order."""
        out: dict = {}
        track = _lib.LINK_FIELDS.index("track")
        for t in range(self.links.shape[0]):
            for k in range(min(int(self.counts[t]), self.links.shape[1])):
                out.setdefault(int(self.links[t, k, track]), []).append((t, k))
        return out

    def as_arrays(self) -> Tuple[np.ndarray, np.ndarray, np.ndarray, Optional[np.ndarray]]:
        return self.counts, self.boxes, self.links, self.state

    @classmethod
    def from_arrays(cls, counts, boxes, links, state=None) -> "ChangeTracks":
        counts = np.ascontiguousarray(counts, dtype=np.uint32)
        boxes = np.ascontiguousarray(boxes, dtype=np.uint32)
        links = np.ascontiguousarray(links, dtype=np.uint32)
        if counts.ndim != 1 or boxes.ndim != 3 or boxes.shape[0] != counts.shape[0] or boxes.shape[2] != _lib.BOX_WORDS:
            raise ValueError("counts must be [n] and boxes [n, K, 8]")
        if links.shape != boxes.shape[:2] + (_lib.LINK_WORDS,):
            raise ValueError("links must be [n, K, 4]")
        if state is not None:
            state = np.ascontiguousarray(state, dtype=np.uint32)
            if state.shape != (1 + 2 * boxes.shape[1],):
                raise ValueError("state must be [1 + 2 * K]")
        return cls(counts, boxes, links, state)


def _tracks_args(connectivity, min_area, max_boxes, chunk_frames, n: int) -> Tuple[int, int, int, int]:
    """The scalar arguments of dips_mask_tracks, checked."""
    conn, area, k, chunk = _components_args(connectivity, min_area, max_boxes, chunk_frames, n)
    if not 1 <= k <= _lib.TRACK_MAX_BOXES:
        raise ValueError(f"max_boxes must be 1 .. {_lib.TRACK_MAX_BOXES}")
    return conn, area, k, chunk


@dataclass
class ChangeShapes:
    """The shape records of the components of a change mask
    (dips_mask_shapes): `counts` and `boxes` as in ChangeBoxes; `shapes`
    uint32 [n, K, 16], record k of frame t the exact sums over the pixels
    (i, j) of the component of box record k (OFFSETS: sx, sy, sxx, syy, sxy
    and wsum as 64-bit fields of two words, wmax, cracks_v, cracks_h, euler),
    zeros past min(counts[t], K).  The integer accessors are [n, K] arrays
    over all records; the derived float64 properties are [n, K] too, NaN
    where there is no record."""
    counts: np.ndarray
    boxes: np.ndarray
    shapes: np.ndarray

    OFFSETS = _lib.SHAPE_OFFSETS

    def frame(self, t: int) -> Tuple[np.ndarray, np.ndarray]:
        """(uint32 [m, 8], uint32 [m, 16]): the m = min(counts[t], K) valid
        records of frame t and their shapes."""
        m = min(int(self.counts[t]), self.boxes.shape[1])
        return self.boxes[t, :m], self.shapes[t, :m]

    @property
    def valid(self) -> np.ndarray:
        """bool [n, K]: the records that describe a component."""
        k = self.boxes.shape[1]
        return np.arange(k, dtype=np.int64)[None, :] < np.minimum(self.counts.astype(np.int64), k)[:, None]

    def _u64(self, name: str) -> np.ndarray:
        f = self.OFFSETS[name]
        return self.shapes[..., f].astype(np.uint64) | (self.shapes[..., f + 1].astype(np.uint64) << np.uint64(32))

    @property
    def area(self) -> np.ndarray:
        return self.boxes[..., _lib.BOX_FIELDS.index("area")]

    @property
    def sx(self) -> np.ndarray:
        return self._u64("sx")

    @property
    def sy(self) -> np.ndarray:
        return self._u64("sy")

    @property
    def sxx(self) -> np.ndarray:
        return self._u64("sxx")

    @property
    def syy(self) -> np.ndarray:
        return self._u64("syy")

    @property
    def sxy(self) -> np.ndarray:
        return self._u64("sxy")

    @property
    def wsum(self) -> np.ndarray:
        return self._u64("wsum")

    @property
    def wmax(self) -> np.ndarray:
        return self.shapes[..., self.OFFSETS["wmax"]]

    @property
    def perimeter(self) -> np.ndarray:
        """uint32: the crack perimeter, cracks_v + cracks_h."""
        return self.shapes[..., self.OFFSETS["cracks_v"]] + self.shapes[..., self.OFFSETS["cracks_h"]]

    @property
    def euler(self) -> np.ndarray:
        """int32: 1 - holes."""
        return np.ascontiguousarray(self.shapes[..., self.OFFSETS["euler"]]).view(np.int32)

    @property
    def holes(self) -> np.ndarray:
        """int32: the holes of every record's component (0 where there is no record)."""
        return np.where(self.valid, 1 - self.euler, 0).astype(np.int32)

    def _central(self) -> Tuple[np.ndarray, np.ndarray, np.ndarray, np.ndarray]:
        """(A, N20, N02, N11) as object arrays of Python integers: A*SXX -
        SX^2, A*SYY - SY^2 and A*SXY - SX*SY, formed exactly."""
        a, sx, sy = self.area.astype(object), self.sx.astype(object), self.sy.astype(object)
        return (a, a * self.sxx.astype(object) - sx * sx, a * self.syy.astype(object) - sy * sy,
                a * self.sxy.astype(object) - sx * sy)

    def _ratio(self, num, den) -> np.ndarray:
        """float64 num / den of two object arrays where there is a record, NaN elsewhere."""
        out = np.full(self.valid.shape, np.nan)
        for idx in zip(*np.nonzero(self.valid)):
            out[idx] = num[idx] / den[idx]  # Python integers: correctly rounded
        return out

    @property
    def mu20(self) -> np.ndarray:
        a, n20, _, _ = self._central()
        return self._ratio(n20, a * a)

    @property
    def mu02(self) -> np.ndarray:
        a, _, n02, _ = self._central()
        return self._ratio(n02, a * a)

    @property
    def mu11(self) -> np.ndarray:
        a, _, _, n11 = self._central()
        return self._ratio(n11, a * a)

    @property
    def orientation(self) -> np.ndarray:
        """The angle of the major axis, from +x towards +y in image
        coordinates (y down), in (-pi/2, pi/2]: 0.5 * atan2(2 N11, N20 -
        N02); 0 for an isotropic component."""
        _, n20, n02, n11 = self._central()
        out = np.full(self.valid.shape, np.nan)
        for idx in zip(*np.nonzero(self.valid)):
            out[idx] = 0.5 * math.atan2(float(2 * n11[idx]), float(n20[idx] - n02[idx]))
        return out

    @property
    def axes(self) -> np.ndarray:
        """float64 [n, K, 2]: the major and the minor axis, 4 * sqrt of the
        eigenvalues of the covariance [[mu20, mu11], [mu11, mu02]] (the full
        lengths of the ellipse with the same second moments)."""
        m20, m02, m11 = self.mu20, self.mu02, self.mu11
        mean, dev = 0.5 * (m20 + m02), np.sqrt(0.25 * (m20 - m02) ** 2 + m11 ** 2)
        return np.stack([4.0 * np.sqrt(mean + dev), 4.0 * np.sqrt(np.maximum(mean - dev, 0.0))], axis=-1)

    @property
    def eccentricity(self) -> np.ndarray:
        """sqrt(1 - minor^2 / major^2) of `axes`; 0 for a single pixel."""
        ax = self.axes
        major, minor = ax[..., 0], ax[..., 1]
        with np.errstate(invalid="ignore", divide="ignore"):
            e = np.sqrt(np.maximum(1.0 - (minor / major) ** 2, 0.0))
        return np.where(major == 0.0, 0.0, e)

    @property
    def compactness(self) -> np.ndarray:
        """perimeter^2 / (4 pi area): 4 / pi for a square, larger the more ragged."""
        with np.errstate(invalid="ignore", divide="ignore"):
            c = self.perimeter.astype(np.float64) ** 2 / (4.0 * math.pi * self.area.astype(np.float64))
        return np.where(self.valid, c, np.nan)

    @property
    def mean_weight(self) -> np.ndarray:
        with np.errstate(invalid="ignore", divide="ignore"):
            m = self.wsum.astype(np.float64) / self.area.astype(np.float64)
        return np.where(self.valid, m, np.nan)

    def as_arrays(self) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        return self.counts, self.boxes, self.shapes

    @classmethod
    def from_arrays(cls, counts, boxes, shapes) -> "ChangeShapes":
        counts = np.ascontiguousarray(counts, dtype=np.uint32)
        boxes = np.ascontiguousarray(boxes, dtype=np.uint32)
        shapes = np.ascontiguousarray(shapes, dtype=np.uint32)
        if counts.ndim != 1 or boxes.ndim != 3 or boxes.shape[0] != counts.shape[0] or boxes.shape[2] != _lib.BOX_WORDS:
            raise ValueError("counts must be [n] and boxes [n, K, 8]")
        if shapes.shape != boxes.shape[:2] + (_lib.SHAPE_WORDS,):
            raise ValueError("shapes must be [n, K, 16]")
        return cls(counts, boxes, shapes)


def _shapes_args(connectivity, min_area, max_boxes, chunk_frames, n: int, w: int, h: int) -> Tuple[int, int, int, int]:
    """The scalar arguments of dips_mask_shapes over a region w x h, checked."""
    conn, area, k, chunk = _components_args(connectivity, min_area, max_boxes, chunk_frames, n)
    if w > _lib.SHAPE_MAX_SIDE or h > _lib.SHAPE_MAX_SIDE:
        raise ValueError(f"the region's width and height must be at most {_lib.SHAPE_MAX_SIDE}")
    if n * k * _lib.SHAPE_WORDS >= 1 << 32:
        raise ValueError("n_frames * max_boxes * 16 must stay below 2^32")
    return conn, area, k, chunk


def _morph_args(op, shape, rx, ry, w: int, h: int) -> Tuple[int, int, int, int]:
    """The scalar arguments of dips_mask_morph, checked; ry None means rx."""
    try:
        op, shape = int(MorphOp(op)), int(MorphShape(shape))
    except ValueError:
        raise ValueError("op must be a MorphOp (0 .. 3) and shape a MorphShape (0 or 1)") from None
    rx = int(rx)
    ry = rx if ry is None else int(ry)
    if not (0 <= rx <= _lib.MORPH_MAX_RADIUS and 0 <= ry <= _lib.MORPH_MAX_RADIUS):
        raise ValueError(f"rx and ry must be 0 .. {_lib.MORPH_MAX_RADIUS}")
    if shape == MorphShape.Diamond and ry != rx:
        raise ValueError("a diamond needs ry == rx")
    if w <= 0 or h <= 0:
        raise ValueError("the mask's width and height must not be 0")
    if w * h >= 1 << 30:
        raise ValueError("the region must stay below 2^30 pixels")
    return op, shape, rx, ry


def _morph_steps(morph, w: int, h: int) -> List[Tuple[int, int, int, int]]:
    """change_boxes' morph: a sequence of (op, shape, rx, ry) steps, checked."""
    steps = []
    for step in morph:
        if len(step) != 4:
            raise ValueError("a morph step must be (op, shape, rx, ry)")
        steps.append(_morph_args(step[0], step[1], step[2], step[3], w, h))
    return steps


def _vote_args(window, votes=None) -> Tuple[int, int]:
    """(window, votes) of dips_mask_vote, checked; votes None means the
    majority, window // 2 + 1."""
    window = int(window)
    if not 1 <= window <= _lib.VOTE_MAX_WINDOW:
        raise ValueError(f"window must be 1 .. {_lib.VOTE_MAX_WINDOW}")
    votes = window // 2 + 1 if votes is None else int(votes)
    if not 1 <= votes <= window:
        raise ValueError("votes must be 1 .. window")
    return window, votes


def _vote_option(vote) -> Tuple[int, int]:
    """change_boxes' vote: window or (window, votes), checked."""
    if isinstance(vote, (tuple, list)):
        if len(vote) != 2:
            raise ValueError("vote must be window or (window, votes)")
        return _vote_args(vote[0], vote[1])
    return _vote_args(vote)


def _select_args(connectivity, min_area, max_area, clear_border, dropped, chunk_frames) -> Tuple[int, int, int, int, int]:
    """(connectivity, min_area, max_area, select bits, chunk_frames) of
    dips_mask_select, checked."""
    if int(connectivity) not in (4, 8):
        raise ValueError("connectivity must be 4 or 8")
    for name, v in (("min_area", min_area), ("max_area", max_area), ("chunk_frames", chunk_frames)):
        if int(v) < 0 or int(v) > 0xFFFFFFFF:
            raise ValueError(f"{name} must be a non-negative 32-bit integer")
    if int(max_area) != 0 and int(max_area) < int(min_area):
        raise ValueError("max_area must be 0 (no upper bound) or at least min_area")
    bits = (_lib.SELECT_CLEAR_BORDER if clear_border else 0) | (_lib.SELECT_DROPPED if dropped else 0)
    return int(connectivity), int(min_area), int(max_area), bits, int(chunk_frames)


_SELECT_KEYS = ("min_area", "max_area", "clear_border", "connectivity", "fill_holes")


def _select_option(select) -> dict:
    """change_boxes' select: a dict with keys from min_area, max_area,
    clear_border, connectivity and fill_holes (False, True or the largest
    hole to fill), checked; the defaults select nothing away."""
    if not isinstance(select, dict) or any(k not in _SELECT_KEYS for k in select):
        raise ValueError("select must be a dict with keys from " + ", ".join(_SELECT_KEYS))
    opt = {"min_area": 1, "max_area": 0, "clear_border": False, "connectivity": 8, "fill_holes": False}
    opt.update(select)
    _select_args(opt["connectivity"], opt["min_area"], opt["max_area"], opt["clear_border"], False, 0)
    fill = opt["fill_holes"]
    if not isinstance(fill, bool) and (int(fill) < 0 or int(fill) > 0xFFFFFFFF):
        raise ValueError("fill_holes must be False, True or a non-negative 32-bit integer")
    return opt


def _logic_op(op, has_b: bool) -> int:
    """The op of dips_mask_logic, checked against whether b is given."""
    try:
        op = int(MaskLogic(op))
    except ValueError:
        raise ValueError("op must be a MaskLogic (0 .. 4)") from None
    if (op == MaskLogic.Not) == has_b:
        raise ValueError("MaskLogic.Not takes no b, every other op needs one")
    return op


def _mask_host_args(mask) -> Tuple[np.ndarray, int, int, int]:
    """(bits, region width, region height, n) of a host ChangeMask, checked
    as the mask statistics take it."""
    if not isinstance(mask, ChangeMask):
        raise ValueError("mask must be a ChangeMask")
    bits = np.ascontiguousarray(mask.bits, dtype=np.uint8)
    rw = int(mask.width)
    if bits.ndim != 3 or rw <= 0 or bits.shape[1] == 0 or bits.shape[2] != 4 * ((rw + 31) // 32):
        raise ValueError("mask.bits must be [n, h, 4 * ceil(width / 32)] bytes, h and width not 0")
    n, rh = int(bits.shape[0]), int(bits.shape[1])
    if rw * rh >= 1 << 30:
        raise ValueError("the region must stay below 2^30 pixels")
    return bits, rw, rh, n


def _mask_device_args(mask, width) -> Tuple[int, int, int]:
    """(region width, region height, n) of a device mask tensor, checked."""
    import torch
    rw = int(width)
    if mask.dim() != 3 or rw <= 0 or mask.shape[2] != 4 * ((rw + 31) // 32) or mask.dtype != torch.uint8:
        raise ValueError("mask must be a uint8 tensor of shape [N, h, 4 * ceil(width / 32)]")
    n, rh = int(mask.shape[0]), int(mask.shape[1])
    if rh == 0:
        raise ValueError("the mask's height must not be 0")
    if rw * rh >= 1 << 30:
        raise ValueError("the region must stay below 2^30 pixels")
    return rw, rh, n


def _mask_device_outputs(mask, outs) -> None:
    """The device tensors of a mask statistic: contiguous HIP tensors, 4-byte
    aligned, no output sharing a byte with the mask or another output."""
    tensors = [mask] + list(outs)
    for t in tensors:
        if not t.is_cuda or not t.is_contiguous():
            raise ValueError("device path needs contiguous HIP tensors")
        if t.numel() and (t.data_ptr() & 3) != 0:
            raise ValueError("the tensors must be 4-byte aligned")
    spans = [(t.data_ptr(), t.data_ptr() + t.numel() * t.element_size()) for t in tensors if t.numel()]
    for i, (a0, a1) in enumerate(spans):
        for b0, b1 in spans[i + 1:]:
            if a0 < b1 and b0 < a1:
                raise ValueError("an output must not overlap the mask or the other output")


def _mask_device_tensors(ins, outs) -> None:
    """The device tensors of a mask-to-mask call: contiguous HIP tensors,
    4-byte aligned, no output sharing a byte with an input or another output
    (the inputs may share theirs)."""
    for t in list(ins) + list(outs):
        if not t.is_cuda or not t.is_contiguous():
            raise ValueError("device path needs contiguous HIP tensors")
        if t.numel() and (t.data_ptr() & 3) != 0:
            raise ValueError("the tensors must be 4-byte aligned")

    def span(t):
        return t.data_ptr(), t.data_ptr() + t.numel() * t.element_size()

    outs = [t for t in outs if t.numel()]
    for i, o in enumerate(outs):
        for other in [t for t in ins if t.numel()] + outs[i + 1:]:
            (a0, a1), (b0, b1) = span(o), span(other)
            if a0 < b1 and b0 < a1:
                raise ValueError("an output must not overlap an input or the other output")


def _mask_grid_args(rows, cols, rw: int, rh: int, n: int) -> Tuple[int, int]:
    """(rows, cols) of dips_mask_counts over a region rw x rh, checked."""
    rows, cols = int(rows), int(cols)
    if rows < 1 or cols < 1:
        raise ValueError("rows and cols must be at least 1")
    if rows > rh or cols > rw:
        raise ValueError("more rows or cols than the region has pixels (a cell would be empty)")
    if n * rows * cols >= 1 << 30:
        raise ValueError("n_frames * rows * cols must stay below 2^30")
    return rows, cols


def _roi_arg(roi):
    """roi (x, y, w, h) as the uint32[4] the C ABI takes, or None."""
    if roi is None:
        return None
    if len(roi) != 4 or any(int(v) < 0 or int(v) > 0xFFFFFFFF for v in roi):
        raise ValueError("roi must be (x, y, w, h) of non-negative 32-bit integers")
    return (ctypes.c_uint32 * 4)(*[int(v) for v in roi])


def grid_cell(width: int, height: int, rows: int, cols: int, row: int, col: int,
              roi=None) -> Tuple[int, int, int, int]:
    """(x, y, w, h) of cell (row, col) of a rows x cols grid over roi (None:
    the whole frame), as dips_diff_series_grid cuts it (dips_grid_cell):
    column c covers [x + c*w//cols, x + (c+1)*w//cols), rows likewise."""
    rect = (ctypes.c_uint32 * 4)()
    check(_lib.load().dips_grid_cell(int(width), int(height), _roi_arg(roi), int(rows), int(cols), int(row),
                                     int(col), rect))
    return rect[0], rect[1], rect[2], rect[3]


def _frame_geometry(frames, fmt: PixelFormat) -> Tuple[int, int, int]:
    shape = tuple(frames.shape)
    c = int(fmt)
    if c == 1:
        if len(shape) == 4 and shape[3] == 1:
            shape = shape[:3]
        if len(shape) != 3:
            raise ValueError("gray8 frames must be [N, H, W]")
        return shape[0], shape[1], shape[2]
    if len(shape) != 4 or shape[3] != c:
        raise ValueError(f"frames must be [N, H, W, {c}]")
    return shape[0], shape[1], shape[2]


class DiffSeriesOperator:
    """The batch operator: per-frame difference series of a frame stack.

    Inputs are numpy arrays (host; the call stages them through HBM) or
    torch tensors on a HIP device (zero-copy, asynchronous on the tensor's
    current stream)."""

    def __init__(self, fmt: PixelFormat = PixelFormat.RGB8, mode: Mode = Mode.Overall,
                 tau: float = 0.0, chroma_filter: ChromaFilter = ChromaFilter.None_,
                 device: int = 0, time_kernel: bool = False, force_generic: bool = False,
                 crosscheck: bool = False, gray_table: str = "auto"):
        """force_generic: the any-shape kernel; crosscheck: the plain kernels
        (DIPS_FLAG_CROSSCHECK; GRAY8 f32 kernel, f64 intensity sums);
        gray_table: "auto" (the GRAY8 table kernel picks its layout per
        workgroup from the content), "band" or "pair" (pinned,
        DIPS_FLAG_GRAY_BAND_TABLE / _PAIR_TABLE).  All give the same series."""
        tables = {"auto": 0, "band": _lib.FLAG_GRAY_BAND_TABLE, "pair": _lib.FLAG_GRAY_PAIR_TABLE}
        if gray_table not in tables:
            raise ValueError("gray_table must be 'auto', 'band' or 'pair'")
        flags = ((_lib.FLAG_TIME_KERNEL if time_kernel else 0) | (_lib.FLAG_FORCE_GENERIC if force_generic else 0)
                 | (_lib.FLAG_CROSSCHECK if crosscheck else 0) | tables[gray_table])
        self.fmt = PixelFormat(fmt)
        self.mode = Mode(mode)
        self.tau = float(tau)
        self._host = _Handle(_params(fmt=self.fmt, mode=self.mode, tau=tau,
                                     chroma_filter=chroma_filter, flags=flags), device)
        self._dev = _Handle(_params(fmt=self.fmt, mode=self.mode, tau=tau,
                                    chroma_filter=chroma_filter,
                                    flags=flags | _lib.FLAG_DEVICE_PTRS), device)
        # hysteresis_mask's device handles at a higher tau, by that tau
        self._strong = {}
        self._strong_params = dict(fmt=self.fmt, mode=self.mode, chroma_filter=chroma_filter,
                                   flags=flags | _lib.FLAG_DEVICE_PTRS)

    def close(self) -> None:
        self._host.close()
        self._dev.close()
        for hd in self._strong.values():
            hd.close()
        self._strong = {}

    # -- host arrays -------------------------------------------------------
    def __call__(self, frames: np.ndarray, ref: Optional[np.ndarray] = None,
                 want_map: bool = False) -> Tuple[Series, Optional[np.ndarray]]:
        frames = _as_u8(frames)
        n, h, w = _frame_geometry(frames, self.fmt)
        out = np.zeros((n, 4), dtype=np.uint64)
        dmap = np.empty_like(frames) if want_map else None
        rp = None
        if ref is not None:
            ref = _as_u8(ref)
            if ref.size != h * w * int(self.fmt):
                raise ValueError("ref must have the shape of one frame")
            rp = ref.ctypes.data
        self._host.check(self._host._lib.dips_diff_series(
            self._host.ptr, w, h, frames.ctypes.data, n, rp, out.ctypes.data,
            dmap.ctypes.data if dmap is not None else None))
        return Series.from_array(out), dmap

    def streamed(self, frames: np.ndarray, ref: Optional[np.ndarray] = None,
                 chunk_frames: int = 0) -> Series:
        """Pinned-staging + side-stream DMA feed (dips_diff_series_streamed)."""
        frames = _as_u8(frames)
        n, h, w = _frame_geometry(frames, self.fmt)
        out = np.zeros((n, 4), dtype=np.uint64)
        rp = None
        if ref is not None:
            ref = _as_u8(ref)
            if ref.size != h * w * int(self.fmt):
                raise ValueError("ref must have the shape of one frame")
            rp = ref.ctypes.data
        self._host.check(self._host._lib.dips_diff_series_streamed(
            self._host.ptr, w, h, frames.ctypes.data, n, rp, out.ctypes.data, int(chunk_frames)))
        return Series.from_array(out)

    # -- device tensors (torch, HIP) ----------------------------------------
    def run_device(self, frames, series_out, ref=None, map_out=None, stream=None) -> None:
        """Asynchronous: frames / ref / map_out uint8 device tensors,
        series_out an int64 device tensor of shape [N, 4]."""
        n, h, w = _frame_geometry(frames, self.fmt)
        if tuple(series_out.shape) != (n, 4) or series_out.element_size() != 8:
            raise ValueError("series_out must be an 8-byte tensor of shape [N, 4]")
        for t in (frames, series_out, ref, map_out):
            if t is not None and (not t.is_cuda or not t.is_contiguous()):
                raise ValueError("device path needs contiguous HIP tensors")
        import torch
        for t in (frames, ref, map_out):
            if t is not None and t.dtype != torch.uint8:
                raise ValueError("frames, ref and map_out must be uint8 tensors")
        if ref is not None and ref.numel() != h * w * int(self.fmt):
            raise ValueError("ref must have the size of one frame")
        if map_out is not None and tuple(map_out.shape) != tuple(frames.shape):
            raise ValueError("map_out must have the shape of frames")
        lib = self._dev._lib
        with _stream_of(self._dev, frames, stream):
            self._dev.check(lib.dips_diff_series(
                self._dev.ptr, w, h, frames.data_ptr(), n,
                ref.data_ptr() if ref is not None else None, series_out.data_ptr(),
                map_out.data_ptr() if map_out is not None else None))

    # -- the series per cell of a spatial grid (dips_diff_series_grid) --------
    def grid(self, frames: np.ndarray, rows: int, cols: int, roi=None,
             ref: Optional[np.ndarray] = None) -> GridSeries:
        """The series of every cell of a rows x cols grid over roi = (x, y,
        w, h) (None: the whole frame): cell [t, r, c] is the entry this
        operator gives for the frames and ref cropped to grid_cell(...)."""
        frames = _as_u8(frames)
        n, h, w = _frame_geometry(frames, self.fmt)
        out = np.zeros((n, int(rows), int(cols), 4), dtype=np.uint64)
        rp = None
        if ref is not None:
            ref = _as_u8(ref)
            if ref.size != h * w * int(self.fmt):
                raise ValueError("ref must have the shape of one frame")
            rp = ref.ctypes.data
        self._host.check(self._host._lib.dips_diff_series_grid(
            self._host.ptr, w, h, frames.ctypes.data, n, rp, _roi_arg(roi), int(rows), int(cols),
            out.ctypes.data))
        return GridSeries.from_array(out)

    def run_grid_device(self, frames, cells_out, rows: int, cols: int, roi=None, ref=None, stream=None) -> None:
        """Asynchronous: frames / ref uint8 device tensors, cells_out an
        8-byte device tensor of shape [N, rows, cols, 4]."""
        n, h, w = _frame_geometry(frames, self.fmt)
        if tuple(cells_out.shape) != (n, int(rows), int(cols), 4) or cells_out.element_size() != 8:
            raise ValueError("cells_out must be an 8-byte tensor of shape [N, rows, cols, 4]")
        for t in (frames, cells_out, ref):
            if t is not None and (not t.is_cuda or not t.is_contiguous()):
                raise ValueError("device path needs contiguous HIP tensors")
        import torch
        for t in (frames, ref):
            if t is not None and t.dtype != torch.uint8:
                raise ValueError("frames and ref must be uint8 tensors")
        if ref is not None and ref.numel() != h * w * int(self.fmt):
            raise ValueError("ref must have the size of one frame")
        lib = self._dev._lib
        with _stream_of(self._dev, frames, stream):
            self._dev.check(lib.dips_diff_series_grid(
                self._dev.ptr, w, h, frames.data_ptr(), n,
                ref.data_ptr() if ref is not None else None, _roi_arg(roi), int(rows), int(cols),
                cells_out.data_ptr()))

    # -- the series summed over time per pixel (dips_diff_pixel_sums) ----------
    def _region(self, roi, h: int, w: int) -> Tuple[int, int]:
        """(rh, rw) of roi (None: the whole frame) for sizing the map; the
        library checks that the region lies in the frame."""
        if roi is None:
            return h, w
        _roi_arg(roi)
        return int(roi[3]), int(roi[2])

    def pixel_sums(self, frames: np.ndarray, roi=None, ref: Optional[np.ndarray] = None,
                   into: Optional[PixelSums] = None) -> PixelSums:
        """Per pixel of roi = (x, y, w, h) (None: the whole frame) the sum
        over the frames of the entry this operator gives for the frames and
        ref cropped to that pixel.  `into`: a PixelSums of the same region to
        add to (a clip in chunks: pass the previous chunk's last frame as ref
        in per-frame mode, the same reference in overall mode)."""
        frames = _as_u8(frames)
        n, h, w = _frame_geometry(frames, self.fmt)
        rh, rw = self._region(roi, h, w)
        if into is not None:
            out = np.ascontiguousarray(into.as_array(), dtype=np.uint64)
            if out.shape != (rh, rw, 4):
                raise ValueError("into must hold the sums of the same region")
        else:
            out = np.zeros((rh, rw, 4), dtype=np.uint64)
        rp = None
        if ref is not None:
            ref = _as_u8(ref)
            if ref.size != h * w * int(self.fmt):
                raise ValueError("ref must have the shape of one frame")
            rp = ref.ctypes.data
        self._host.check(self._host._lib.dips_diff_pixel_sums(
            self._host.ptr, w, h, frames.ctypes.data if n else None, n, rp, _roi_arg(roi),
            1 if into is not None else 0, out.ctypes.data))
        return PixelSums.from_array(out)

    def run_pixel_sums_device(self, frames, sums_out, roi=None, ref=None, accumulate: bool = False,
                              stream=None) -> None:
        """Asynchronous: frames / ref uint8 device tensors, sums_out an
        8-byte device tensor of shape [h, w, 4] of the region, overwritten or
        (accumulate) added to."""
        n, h, w = _frame_geometry(frames, self.fmt)
        rh, rw = self._region(roi, h, w)
        if tuple(sums_out.shape) != (rh, rw, 4) or sums_out.element_size() != 8:
            raise ValueError("sums_out must be an 8-byte tensor of shape [h, w, 4] of the region")
        for t in (frames, sums_out, ref):
            if t is not None and (not t.is_cuda or not t.is_contiguous()):
                raise ValueError("device path needs contiguous HIP tensors")
        import torch
        for t in (frames, ref):
            if t is not None and t.dtype != torch.uint8:
                raise ValueError("frames and ref must be uint8 tensors")
        if ref is not None and ref.numel() != h * w * int(self.fmt):
            raise ValueError("ref must have the size of one frame")
        lib = self._dev._lib
        with _stream_of(self._dev, frames, stream):
            self._dev.check(lib.dips_diff_pixel_sums(
                self._dev.ptr, w, h, frames.data_ptr() if n else None, n,
                ref.data_ptr() if ref is not None else None, _roi_arg(roi), 1 if accumulate else 0,
                sums_out.data_ptr() if sums_out.numel() else None))

    # -- the per-frame change mask (dips_diff_change_mask) -------------------
    def change_mask(self, frames: np.ndarray, roi=None, ref: Optional[np.ndarray] = None) -> ChangeMask:
        """One bit per pixel of roi = (x, y, w, h) (None: the whole frame) and
        frame: whether this operator counts the pixel as changed in that
        frame (the count of the series of the 1x1 crop).  A clip in chunks:
        pass the previous chunk's last frame as ref in per-frame mode, the
        same reference in overall mode."""
        frames = _as_u8(frames)
        n, h, w = _frame_geometry(frames, self.fmt)
        rh, rw = self._region(roi, h, w)
        out = np.zeros((n, rh, 4 * ((rw + 31) // 32)), dtype=np.uint8)
        rp = None
        if ref is not None:
            ref = _as_u8(ref)
            if ref.size != h * w * int(self.fmt):
                raise ValueError("ref must have the shape of one frame")
            rp = ref.ctypes.data
        self._host.check(self._host._lib.dips_diff_change_mask(
            self._host.ptr, w, h, frames.ctypes.data if n else None, n, rp, _roi_arg(roi),
            out.ctypes.data if out.size else None))
        return ChangeMask(out, rw)

    def run_change_mask_device(self, frames, mask_out, roi=None, ref=None, stream=None, _handle=None) -> None:
        """Asynchronous: frames / ref uint8 device tensors, mask_out a uint8
        device tensor of shape [N, h, row_bytes] of the region (4-byte
        aligned), every byte of which is written."""
        hd = self._dev if _handle is None else _handle
        n, h, w = _frame_geometry(frames, self.fmt)
        rh, rw = self._region(roi, h, w)
        if tuple(mask_out.shape) != (n, rh, 4 * ((rw + 31) // 32)):
            raise ValueError("mask_out must be a uint8 tensor of shape [N, h, 4 * ceil(w / 32)] of the region")
        for t in (frames, mask_out, ref):
            if t is not None and (not t.is_cuda or not t.is_contiguous()):
                raise ValueError("device path needs contiguous HIP tensors")
        import torch
        for t in (frames, mask_out, ref):
            if t is not None and t.dtype != torch.uint8:
                raise ValueError("frames, ref and mask_out must be uint8 tensors")
        if ref is not None and ref.numel() != h * w * int(self.fmt):
            raise ValueError("ref must have the size of one frame")
        lib = hd._lib
        with _stream_of(hd, frames, stream):
            hd.check(lib.dips_diff_change_mask(
                hd.ptr, w, h, frames.data_ptr() if n else None, n,
                ref.data_ptr() if ref is not None else None, _roi_arg(roi),
                mask_out.data_ptr() if mask_out.numel() else None))

    # -- the running-average background (dips_diff_background_mask) ----------
    def background_mask(self, frames: np.ndarray, roi=None, ref: Optional[np.ndarray] = None, rate_shift: int = 3,
                        selective: bool = False, state: Optional[Background] = None) -> Tuple[ChangeMask, Background]:
        """The change mask of every frame against a per-pixel running average
        of the frames before it (update rate 2^-rate_shift; selective: pixels
        that changed do not update), and the average after the last frame.
        The average starts at `ref` (None: frame 0) or continues `state`, the
        Background an earlier call over the same region returned -- a clip in
        chunks.  The operator's mode is not consulted."""
        frames = _as_u8(frames)
        n, h, w = _frame_geometry(frames, self.fmt)
        rh, rw = self._region(roi, h, w)
        c = int(self.fmt)
        k, flags = _background_args(rate_shift, selective)
        if state is not None:
            if ref is not None:
                raise ValueError("ref and state exclude each other")
            if not isinstance(state, Background):
                raise ValueError("state must be a Background")
            bg = np.array(state.state, dtype=np.uint16, order="C")
            if bg.shape != (c, rh, rw):
                raise ValueError("state must hold the background of the same region and format")
        else:
            if ref is None and n == 0:
                raise ValueError("the initial background needs ref or a frame")
            bg = np.zeros((c, rh, rw), dtype=np.uint16)
        out = np.zeros((n, rh, 4 * ((rw + 31) // 32)), dtype=np.uint8)
        rp = None
        if ref is not None:
            ref = _as_u8(ref)
            if ref.size != h * w * c:
                raise ValueError("ref must have the shape of one frame")
            rp = ref.ctypes.data
        self._host.check(self._host._lib.dips_diff_background_mask(
            self._host.ptr, w, h, frames.ctypes.data if n else None, n, rp, _roi_arg(roi), k, flags,
            1 if state is not None else 0, bg.ctypes.data, out.ctypes.data if out.size else None))
        return ChangeMask(out, rw), Background(bg)

    def run_background_mask_device(self, frames, background, mask_out=None, roi=None, ref=None, rate_shift: int = 3,
                                   selective: bool = False, accumulate: bool = False, stream=None) -> None:
        """Asynchronous: frames / ref uint8 device tensors, background a
        2-byte device tensor of shape [C, h, w] of the region, overwritten or
        (accumulate: ref must be None) continued; mask_out a uint8 device
        tensor of shape [N, h, row_bytes] of the region (4-byte aligned),
        every byte of which is written, or None for the background alone."""
        n, h, w = _frame_geometry(frames, self.fmt)
        rh, rw = self._region(roi, h, w)
        c = int(self.fmt)
        k, flags = _background_args(rate_shift, selective)
        if tuple(background.shape) != (c, rh, rw) or background.element_size() != 2:
            raise ValueError("background must be a 2-byte tensor of shape [C, h, w] of the region")
        if mask_out is not None and tuple(mask_out.shape) != (n, rh, 4 * ((rw + 31) // 32)):
            raise ValueError("mask_out must be a uint8 tensor of shape [N, h, 4 * ceil(w / 32)] of the region")
        for t in (frames, background, mask_out, ref):
            if t is not None and (not t.is_cuda or not t.is_contiguous()):
                raise ValueError("device path needs contiguous HIP tensors")
        import torch
        for t in (frames, mask_out, ref):
            if t is not None and t.dtype != torch.uint8:
                raise ValueError("frames, ref and mask_out must be uint8 tensors")
        if ref is not None and ref.numel() != h * w * c:
            raise ValueError("ref must have the size of one frame")
        if accumulate and ref is not None:
            raise ValueError("ref and accumulate exclude each other")
        if not accumulate and ref is None and n == 0:
            raise ValueError("the initial background needs ref or a frame")
        lib = self._dev._lib
        with _stream_of(self._dev, frames, stream):
            self._dev.check(lib.dips_diff_background_mask(
                self._dev.ptr, w, h, frames.data_ptr() if n else None, n,
                ref.data_ptr() if ref is not None else None, _roi_arg(roi), k, flags, 1 if accumulate else 0,
                background.data_ptr(), mask_out.data_ptr() if mask_out is not None and mask_out.numel() else None))

    # -- the Sigma-Delta background (dips_diff_sigma_delta_mask) --------------
    def sigma_delta_mask(self, frames: np.ndarray, roi=None, ref: Optional[np.ndarray] = None, n_amp: int = 2,
                         v_min: int = 2, v_max: int = 510,
                         state: Optional[SigmaDelta] = None) -> Tuple[ChangeMask, SigmaDelta]:
        """The change mask of every frame under a per-pixel adaptive
        threshold: each pixel keeps a running median M of its integer
        intensity J = max + min of R, G, B and an estimate V of its own
        activity (both move by at most 1 per frame, V toward n_amp times the
        deviation, inside [v_min, v_max]) and fires when |J - M| > V.  Returns
        the mask and the state after the last frame.  The state starts at M =
        J(ref) (None: frame 0), V = v_min, or continues `state`, the
        SigmaDelta an earlier call over the same region returned -- a clip in
        chunks.  The operator's mode and tau are not consulted."""
        frames = _as_u8(frames)
        n, h, w = _frame_geometry(frames, self.fmt)
        rh, rw = self._region(roi, h, w)
        c = int(self.fmt)
        n_amp, v_min, v_max = _sigma_delta_args(n_amp, v_min, v_max)
        if state is not None:
            if ref is not None:
                raise ValueError("ref and state exclude each other")
            if not isinstance(state, SigmaDelta):
                raise ValueError("state must be a SigmaDelta")
            sd = np.array(state.state, dtype=np.uint16, order="C")
            if sd.shape != (_lib.SD_PLANES, rh, rw):
                raise ValueError("state must hold the Sigma-Delta state of the same region")
        else:
            if ref is None and n == 0:
                raise ValueError("the initial state needs ref or a frame")
            sd = np.zeros((_lib.SD_PLANES, rh, rw), dtype=np.uint16)
        out = np.zeros((n, rh, 4 * ((rw + 31) // 32)), dtype=np.uint8)
        rp = None
        if ref is not None:
            ref = _as_u8(ref)
            if ref.size != h * w * c:
                raise ValueError("ref must have the shape of one frame")
            rp = ref.ctypes.data
        self._host.check(self._host._lib.dips_diff_sigma_delta_mask(
            self._host.ptr, w, h, frames.ctypes.data if n else None, n, rp, _roi_arg(roi), n_amp, v_min, v_max,
            1 if state is not None else 0, sd.ctypes.data, out.ctypes.data if out.size else None))
        return ChangeMask(out, rw), SigmaDelta(sd)

    def run_sigma_delta_mask_device(self, frames, state, mask_out=None, roi=None, ref=None, n_amp: int = 2,
                                    v_min: int = 2, v_max: int = 510, accumulate: bool = False, stream=None) -> None:
        """Asynchronous: frames / ref uint8 device tensors, state a 2-byte
        device tensor of shape [2, h, w] of the region, overwritten or
        (accumulate: ref must be None) continued; mask_out a uint8 device
        tensor of shape [N, h, row_bytes] of the region (4-byte aligned),
        every byte of which is written, or None for the state alone."""
        n, h, w = _frame_geometry(frames, self.fmt)
        rh, rw = self._region(roi, h, w)
        c = int(self.fmt)
        n_amp, v_min, v_max = _sigma_delta_args(n_amp, v_min, v_max)
        if tuple(state.shape) != (_lib.SD_PLANES, rh, rw) or state.element_size() != 2:
            raise ValueError("state must be a 2-byte tensor of shape [2, h, w] of the region")
        if mask_out is not None and tuple(mask_out.shape) != (n, rh, 4 * ((rw + 31) // 32)):
            raise ValueError("mask_out must be a uint8 tensor of shape [N, h, 4 * ceil(w / 32)] of the region")
        for t in (frames, state, mask_out, ref):
            if t is not None and (not t.is_cuda or not t.is_contiguous()):
                raise ValueError("device path needs contiguous HIP tensors")
        import torch
        for t in (frames, mask_out, ref):
            if t is not None and t.dtype != torch.uint8:
                raise ValueError("frames, ref and mask_out must be uint8 tensors")
        if ref is not None and ref.numel() != h * w * c:
            raise ValueError("ref must have the size of one frame")
        if accumulate and ref is not None:
            raise ValueError("ref and accumulate exclude each other")
        if not accumulate and ref is None and n == 0:
            raise ValueError("the initial state needs ref or a frame")
        lib = self._dev._lib
        with _stream_of(self._dev, frames, stream):
            self._dev.check(lib.dips_diff_sigma_delta_mask(
                self._dev.ptr, w, h, frames.data_ptr() if n else None, n,
                ref.data_ptr() if ref is not None else None, _roi_arg(roi), n_amp, v_min, v_max,
                1 if accumulate else 0, state.data_ptr(),
                mask_out.data_ptr() if mask_out is not None and mask_out.numel() else None))

    # -- the connected components of a change mask (dips_mask_components) ----
    def mask_components(self, mask: ChangeMask, connectivity: int = 8, min_area: int = 1, max_boxes: int = 64,
                        labels: bool = False, chunk_frames: int = 0) -> ChangeBoxes:
        """The components of every frame of `mask` (what change_mask
        returns) under 4- or 8-connectivity: those of at least min_area
        pixels, counted per frame, the first max_boxes of a frame by
        ascending anchor as records, and (labels=True) the label image.  A
        mask that lives on the device goes through
        run_mask_components_device."""
        if not isinstance(mask, ChangeMask):
            raise ValueError("mask must be a ChangeMask")
        bits = np.ascontiguousarray(mask.bits, dtype=np.uint8)
        rw = int(mask.width)
        if bits.ndim != 3 or rw < 0 or bits.shape[2] != 4 * ((rw + 31) // 32):
            raise ValueError("mask.bits must be [n, h, 4 * ceil(width / 32)] bytes")
        n, rh = int(bits.shape[0]), int(bits.shape[1])
        conn, area, k, chunk = _components_args(connectivity, min_area, max_boxes, chunk_frames, n)
        counts = np.zeros(n, dtype=np.uint32)
        boxes = np.zeros((n, k, _lib.BOX_WORDS), dtype=np.uint32)
        lab = np.zeros((n, rh, rw), dtype=np.uint32) if labels else None
        self._host.check(self._host._lib.dips_mask_components(
            self._host.ptr, bits.ctypes.data if bits.size else None, n, rw, rh, conn, area, k, chunk,
            counts.ctypes.data if n else None, boxes.ctypes.data if boxes.size else None,
            lab.ctypes.data if lab is not None and lab.size else None))
        return ChangeBoxes(counts, boxes, lab)

    def run_mask_components_device(self, mask, width: int, counts_out, boxes_out=None, labels_out=None,
                                   connectivity: int = 8, min_area: int = 1, chunk_frames: int = 0,
                                   stream=None) -> None:
        """Asynchronous: mask a uint8 device tensor [N, h, row_bytes] as
        run_change_mask_device writes it for a region `width` pixels wide;
        counts_out [N], boxes_out [N, K, 8] (None: counts only) and
        labels_out [N, h, width] (None: not produced) 4-byte device tensors,
        all 4-byte aligned; every element of them is written."""
        import torch
        rw = int(width)
        if mask.dim() != 3 or rw < 0 or mask.shape[2] != 4 * ((rw + 31) // 32) or mask.dtype != torch.uint8:
            raise ValueError("mask must be a uint8 tensor of shape [N, h, 4 * ceil(width / 32)]")
        n, rh = int(mask.shape[0]), int(mask.shape[1])
        k = 0
        if boxes_out is not None:
            if boxes_out.dim() != 3 or boxes_out.shape[0] != n or boxes_out.shape[2] != _lib.BOX_WORDS:
                raise ValueError("boxes_out must be a 4-byte tensor of shape [N, K, 8]")
            k = int(boxes_out.shape[1])
        conn, area, k, chunk = _components_args(connectivity, min_area, k, chunk_frames, n)
        if tuple(counts_out.shape) != (n,):
            raise ValueError("counts_out must be a 4-byte tensor of shape [N]")
        if labels_out is not None and tuple(labels_out.shape) != (n, rh, rw):
            raise ValueError("labels_out must be a 4-byte tensor of shape [N, h, width]")
        for t in (counts_out, boxes_out, labels_out):
            if t is not None and t.element_size() != 4:
                raise ValueError("counts_out, boxes_out and labels_out must be 4-byte tensors")
        for t in (mask, counts_out, boxes_out, labels_out):
            if t is not None and (not t.is_cuda or not t.is_contiguous()):
                raise ValueError("device path needs contiguous HIP tensors")
        lib = self._dev._lib
        with _stream_of(self._dev, mask, stream):
            self._dev.check(lib.dips_mask_components(
                self._dev.ptr, mask.data_ptr() if mask.numel() else None, n, rw, rh, conn, area, k, chunk,
                counts_out.data_ptr() if n else None,
                boxes_out.data_ptr() if boxes_out is not None and boxes_out.numel() else None,
                labels_out.data_ptr() if labels_out is not None and labels_out.numel() else None))

    # -- the shape records of the components (dips_mask_shapes) ---------------
    def mask_shapes(self, mask: ChangeMask, weights: Optional[np.ndarray] = None, connectivity: int = 8,
                    min_area: int = 1, max_boxes: int = 64, chunk_frames: int = 0) -> ChangeShapes:
        """mask_components of every frame of `mask`, and per record the exact
        moments, crack counts and Euler number of its component; with
        `weights` (uint8 [n, h, width], one value per pixel of the region)
        also their sum and peak over it.  A mask that lives on the device
        goes through run_mask_shapes_device."""
        bits, rw, rh, n = _mask_host_args(mask)
        conn, area, k, chunk = _shapes_args(connectivity, min_area, max_boxes, chunk_frames, n, rw, rh)
        if weights is not None:
            weights = np.ascontiguousarray(weights)
            if weights.dtype != np.uint8 or weights.shape != (n, rh, rw):
                raise ValueError("weights must be uint8 [n, h, width]")
        counts = np.zeros(n, dtype=np.uint32)
        boxes = np.zeros((n, k, _lib.BOX_WORDS), dtype=np.uint32)
        shapes = np.zeros((n, k, _lib.SHAPE_WORDS), dtype=np.uint32)
        self._host.check(self._host._lib.dips_mask_shapes(
            self._host.ptr, bits.ctypes.data if bits.size else None,
            weights.ctypes.data if weights is not None and weights.size else None, n, rw, rh, conn, area, k, chunk,
            counts.ctypes.data if n else None, boxes.ctypes.data if boxes.size else None,
            shapes.ctypes.data if shapes.size else None))
        return ChangeShapes(counts, boxes, shapes)

    def run_mask_shapes_device(self, mask, width: int, counts_out, boxes_out, shapes_out, weights=None,
                               connectivity: int = 8, min_area: int = 1, chunk_frames: int = 0, stream=None) -> None:
        """Asynchronous: mask a uint8 device tensor [N, h, row_bytes] as
        run_change_mask_device writes it for a region `width` pixels wide;
        counts_out [N], boxes_out [N, K, 8] and shapes_out [N, K, 16] 4-byte
        device tensors (both None: counts only), every element of them
        written; counts_out and boxes_out 4-byte aligned, shapes_out 8-byte
        aligned; weights (None: none) a uint8 device tensor [N, h, width] at
        any alignment."""
        import torch
        rw, rh, n = _mask_device_args(mask, width)
        if (boxes_out is None) != (shapes_out is None):
            raise ValueError("boxes_out and shapes_out go together")
        k = 0
        if boxes_out is not None:
            if boxes_out.dim() != 3 or boxes_out.shape[0] != n or boxes_out.shape[2] != _lib.BOX_WORDS:
                raise ValueError("boxes_out must be a 4-byte tensor of shape [N, K, 8]")
            k = int(boxes_out.shape[1])
            if tuple(shapes_out.shape) != (n, k, _lib.SHAPE_WORDS):
                raise ValueError("shapes_out must be a 4-byte tensor of shape [N, K, 16]")
        conn, area, k, chunk = _shapes_args(connectivity, min_area, k, chunk_frames, n, rw, rh)
        if tuple(counts_out.shape) != (n,):
            raise ValueError("counts_out must be a 4-byte tensor of shape [N]")
        if weights is not None and (weights.dtype != torch.uint8 or tuple(weights.shape) != (n, rh, rw)):
            raise ValueError("weights must be a uint8 tensor of shape [N, h, width]")
        for t in (counts_out, boxes_out, shapes_out):
            if t is not None and t.element_size() != 4:
                raise ValueError("counts_out, boxes_out and shapes_out must be 4-byte tensors")
        for t in (mask, weights, counts_out, boxes_out, shapes_out):
            if t is not None and (not t.is_cuda or not t.is_contiguous()):
                raise ValueError("device path needs contiguous HIP tensors")
        lib = self._dev._lib
        with _stream_of(self._dev, mask, stream):
            self._dev.check(lib.dips_mask_shapes(
                self._dev.ptr, mask.data_ptr() if mask.numel() else None,
                weights.data_ptr() if weights is not None and weights.numel() else None, n, rw, rh, conn, area, k,
                chunk, counts_out.data_ptr() if n else None,
                boxes_out.data_ptr() if boxes_out is not None and boxes_out.numel() else None,
                shapes_out.data_ptr() if shapes_out is not None and shapes_out.numel() else None))

    # -- the components linked across frames (dips_mask_tracks) ---------------
    def mask_tracks(self, mask: ChangeMask, connectivity: int = 8, min_area: int = 1, max_boxes: int = 64,
                    chunk_frames: int = 0, prev: Optional[np.ndarray] = None,
                    state: Optional[np.ndarray] = None) -> ChangeTracks:
        """mask_components of every frame of `mask`, and per record its link
        to the frame before: the record it continues or came from, their
        overlap, the id and the age of its track.  A longer clip goes call
        by call: `prev` is the last frame of the previous call's mask
        (uint8 [h, row_bytes]) and `state` its result's state, and the
        result equals the one call over the whole clip.  state without prev
        is a scene cut: the ids go on, the tracks do not.  The returned
        state is a new array (None when none was given).  A mask that lives
        on the device goes through run_mask_tracks_device."""
        if not isinstance(mask, ChangeMask):
            raise ValueError("mask must be a ChangeMask")
        bits = np.ascontiguousarray(mask.bits, dtype=np.uint8)
        rw = int(mask.width)
        if bits.ndim != 3 or rw < 0 or bits.shape[2] != 4 * ((rw + 31) // 32):
            raise ValueError("mask.bits must be [n, h, 4 * ceil(width / 32)] bytes")
        n, rh = int(bits.shape[0]), int(bits.shape[1])
        conn, area, k, chunk = _tracks_args(connectivity, min_area, max_boxes, chunk_frames, n)
        if prev is not None:
            if state is None:
                raise ValueError("prev needs state")
            prev = np.ascontiguousarray(prev, dtype=np.uint8)
            if prev.shape != bits.shape[1:]:
                raise ValueError("prev must be one frame of the mask: [h, 4 * ceil(width / 32)] bytes")
        if state is not None:
            state = np.array(state, dtype=np.uint32)  # a copy: the call writes it
            if state.shape != (1 + 2 * k,):
                raise ValueError("state must be [1 + 2 * max_boxes]")
        counts = np.zeros(n, dtype=np.uint32)
        boxes = np.zeros((n, k, _lib.BOX_WORDS), dtype=np.uint32)
        links = np.zeros((n, k, _lib.LINK_WORDS), dtype=np.uint32)
        self._host.check(self._host._lib.dips_mask_tracks(
            self._host.ptr, bits.ctypes.data if bits.size else None, n, rw, rh, conn, area, k, chunk,
            prev.ctypes.data if prev is not None and prev.size else None,
            state.ctypes.data if state is not None else None,
            counts.ctypes.data if n else None, boxes.ctypes.data if n else None, links.ctypes.data if n else None))
        return ChangeTracks(counts, boxes, links, state)

    def run_mask_tracks_device(self, mask, width: int, counts_out, boxes_out, links_out, prev=None, state=None,
                               connectivity: int = 8, min_area: int = 1, chunk_frames: int = 0, stream=None) -> None:
        """Asynchronous: mask a uint8 device tensor [N, h, row_bytes] as
        run_change_mask_device writes it for a region `width` pixels wide;
        counts_out [N], boxes_out [N, K, 8] and links_out [N, K, 4] 4-byte
        device tensors, every element of them written; prev (None: none) a
        uint8 device tensor [h, row_bytes], the frame before the mask's
        first; state (None: no carry) a 4-byte device tensor [1 + 2K], read
        and written in the stream.  All 4-byte aligned."""
        import torch
        rw = int(width)
        if mask.dim() != 3 or rw < 0 or mask.shape[2] != 4 * ((rw + 31) // 32) or mask.dtype != torch.uint8:
            raise ValueError("mask must be a uint8 tensor of shape [N, h, 4 * ceil(width / 32)]")
        n, rh = int(mask.shape[0]), int(mask.shape[1])
        if boxes_out.dim() != 3 or boxes_out.shape[0] != n or boxes_out.shape[2] != _lib.BOX_WORDS:
            raise ValueError("boxes_out must be a 4-byte tensor of shape [N, K, 8]")
        conn, area, k, chunk = _tracks_args(connectivity, min_area, int(boxes_out.shape[1]), chunk_frames, n)
        if tuple(counts_out.shape) != (n,):
            raise ValueError("counts_out must be a 4-byte tensor of shape [N]")
        if tuple(links_out.shape) != (n, k, _lib.LINK_WORDS):
            raise ValueError("links_out must be a 4-byte tensor of shape [N, K, 4]")
        if prev is not None:
            if state is None:
                raise ValueError("prev needs state")
            if tuple(prev.shape) != tuple(mask.shape[1:]) or prev.dtype != torch.uint8:
                raise ValueError("prev must be a uint8 tensor of shape [h, 4 * ceil(width / 32)]")
        if state is not None and tuple(state.shape) != (1 + 2 * k,):
            raise ValueError("state must be a 4-byte tensor of shape [1 + 2 * K]")
        for t in (counts_out, boxes_out, links_out, state):
            if t is not None and t.element_size() != 4:
                raise ValueError("counts_out, boxes_out, links_out and state must be 4-byte tensors")
        for t in (mask, prev, state, counts_out, boxes_out, links_out):
            if t is not None and (not t.is_cuda or not t.is_contiguous()):
                raise ValueError("device path needs contiguous HIP tensors")
        lib = self._dev._lib
        with _stream_of(self._dev, mask, stream):
            self._dev.check(lib.dips_mask_tracks(
                self._dev.ptr, mask.data_ptr() if mask.numel() else None, n, rw, rh, conn, area, k, chunk,
                prev.data_ptr() if prev is not None and prev.numel() else None,
                state.data_ptr() if state is not None else None,
                counts_out.data_ptr() if n else None, boxes_out.data_ptr() if n else None,
                links_out.data_ptr() if n else None))

    # -- the binary morphology of a change mask (dips_mask_morph) -------------
    def mask_morph(self, mask: ChangeMask, op, rx: int = 1, ry: Optional[int] = None,
                   shape=MorphShape.Box) -> ChangeMask:
        """Every frame of `mask` (what change_mask returns) eroded, dilated,
        opened or closed by a box of radii rx, ry (ry None: rx) or a diamond
        of radius rx; outside the region counts as clear for a dilation and
        as set for an erosion.  A mask that lives on the device goes through
        run_mask_morph_device."""
        if not isinstance(mask, ChangeMask):
            raise ValueError("mask must be a ChangeMask")
        bits = np.ascontiguousarray(mask.bits, dtype=np.uint8)
        rw = int(mask.width)
        if bits.ndim != 3 or rw < 0 or bits.shape[2] != 4 * ((rw + 31) // 32):
            raise ValueError("mask.bits must be [n, h, 4 * ceil(width / 32)] bytes")
        n, rh = int(bits.shape[0]), int(bits.shape[1])
        op, shape, rx, ry = _morph_args(op, shape, rx, ry, rw, rh)
        out = np.zeros_like(bits)
        self._host.check(self._host._lib.dips_mask_morph(
            self._host.ptr, bits.ctypes.data if n else None, n, rw, rh, op, shape, rx, ry,
            out.ctypes.data if n else None))
        return ChangeMask(out, rw)

    def run_mask_morph_device(self, mask, width: int, out, op, rx: int = 1, ry: Optional[int] = None,
                              shape=MorphShape.Box, stream=None) -> None:
        """Asynchronous: mask and out uint8 device tensors [N, h, row_bytes]
        as run_change_mask_device writes them for a region `width` pixels
        wide, 4-byte aligned and not overlapping; every byte of out is
        written."""
        import torch
        rw = int(width)
        for t in (mask, out):
            if t.dim() != 3 or rw < 0 or t.shape[2] != 4 * ((rw + 31) // 32) or t.dtype != torch.uint8:
                raise ValueError("mask and out must be uint8 tensors of shape [N, h, 4 * ceil(width / 32)]")
            if not t.is_cuda or not t.is_contiguous():
                raise ValueError("device path needs contiguous HIP tensors")
        if tuple(out.shape) != tuple(mask.shape):
            raise ValueError("out must have the shape of mask")
        n, rh = int(mask.shape[0]), int(mask.shape[1])
        op, shape, rx, ry = _morph_args(op, shape, rx, ry, rw, rh)
        nbytes = mask.numel()
        if n and mask.data_ptr() < out.data_ptr() + nbytes and out.data_ptr() < mask.data_ptr() + nbytes:
            raise ValueError("mask and out must not overlap")
        if n and ((mask.data_ptr() | out.data_ptr()) & 3) != 0:
            raise ValueError("mask and out must be 4-byte aligned")
        lib = self._dev._lib
        with _stream_of(self._dev, mask, stream):
            self._dev.check(lib.dips_mask_morph(
                self._dev.ptr, mask.data_ptr() if n else None, n, rw, rh, op, shape, rx, ry,
                out.data_ptr() if n else None))

    # -- the temporal m-of-k vote on a change mask (dips_mask_vote) ------------
    def mask_vote(self, mask: ChangeMask, window: int = 3, votes: Optional[int] = None,
                  history: Optional[ChangeMask] = None) -> Tuple[ChangeMask, ChangeMask]:
        """(voted, next_history): bit (t, y, x) of `voted` is set when at
        least `votes` of the `window` frames t - window + 1 .. t of `mask`
        have it set (votes None: the majority, window // 2 + 1; 1: the OR,
        window: the AND of the window).  The frames before the clip are the
        window - 1 frames of `history`, oldest first (None: clear).
        next_history, the last window - 1 frames of history and mask
        together, continues a clip in a later call: chunk by chunk gives
        what one call over the whole clip gives.  A mask that lives on the
        device goes through run_mask_vote_device."""
        if not isinstance(mask, ChangeMask) or (history is not None and not isinstance(history, ChangeMask)):
            raise ValueError("mask and history must be ChangeMasks")
        window, votes = _vote_args(window, votes)
        bits = np.ascontiguousarray(mask.bits, dtype=np.uint8)
        rw = int(mask.width)
        if bits.ndim != 3 or rw <= 0 or bits.shape[1] == 0 or bits.shape[2] != 4 * ((rw + 31) // 32):
            raise ValueError("mask.bits must be [n, h, 4 * ceil(width / 32)] bytes, h and width not 0")
        n, rh = int(bits.shape[0]), int(bits.shape[1])
        if rw * rh >= 1 << 30:
            raise ValueError("the region must stay below 2^30 pixels")
        hist = None
        if history is not None and window > 1:
            hist = np.ascontiguousarray(history.bits, dtype=np.uint8)
            if int(history.width) != rw or hist.shape != (window - 1, rh, bits.shape[2]):
                raise ValueError("history must hold window - 1 frames of the mask's region")
        out = np.zeros_like(bits)
        nxt = np.zeros((window - 1, rh, bits.shape[2]), dtype=np.uint8)
        self._host.check(self._host._lib.dips_mask_vote(
            self._host.ptr, bits.ctypes.data if n else None, n, rw, rh, window, votes,
            hist.ctypes.data if hist is not None else None, nxt.ctypes.data if window > 1 else None,
            out.ctypes.data if n else None))
        return ChangeMask(out, rw), ChangeMask(nxt, rw)

    def run_mask_vote_device(self, mask, width: int, out, window: int = 3, votes: Optional[int] = None,
                             history=None, history_out=None, stream=None) -> None:
        """Asynchronous: mask and out uint8 device tensors [N, h, row_bytes]
        as run_change_mask_device writes them for a region `width` pixels
        wide, history and history_out (either may be None) such tensors of
        window - 1 frames; all 4-byte aligned, no output overlapping an input
        or the other output.  Every byte of out and history_out is written."""
        import torch
        rw = int(width)
        window, votes = _vote_args(window, votes)
        if window == 1:
            history = history_out = None
        given = [t for t in (mask, out, history, history_out) if t is not None]
        for t in given:
            if t.dim() != 3 or rw <= 0 or t.shape[2] != 4 * ((rw + 31) // 32) or t.dtype != torch.uint8:
                raise ValueError("the masks must be uint8 tensors of shape [N, h, 4 * ceil(width / 32)]")
            if not t.is_cuda or not t.is_contiguous():
                raise ValueError("device path needs contiguous HIP tensors")
        if tuple(out.shape) != tuple(mask.shape):
            raise ValueError("out must have the shape of mask")
        n, rh = int(mask.shape[0]), int(mask.shape[1])
        if rh == 0:
            raise ValueError("the mask's height must not be 0")
        if rw * rh >= 1 << 30:
            raise ValueError("the region must stay below 2^30 pixels")
        for t in (history, history_out):
            if t is not None and tuple(t.shape) != (window - 1, rh, int(mask.shape[2])):
                raise ValueError("history and history_out must hold window - 1 frames of the mask's region")

        def overlap(a, b):
            return (a is not None and b is not None and a.numel() and b.numel()
                    and a.data_ptr() < b.data_ptr() + b.numel() and b.data_ptr() < a.data_ptr() + a.numel())

        if (overlap(out, mask) or overlap(out, history) or overlap(history_out, mask)
                or overlap(history_out, history) or overlap(out, history_out)):
            raise ValueError("an output must not overlap an input or the other output")
        if any(t.numel() and (t.data_ptr() & 3) != 0 for t in given):
            raise ValueError("the masks must be 4-byte aligned")
        lib = self._dev._lib
        with _stream_of(self._dev, mask, stream):
            self._dev.check(lib.dips_mask_vote(
                self._dev.ptr, mask.data_ptr() if n else None, n, rw, rh, window, votes,
                history.data_ptr() if history is not None else None,
                history_out.data_ptr() if history_out is not None else None,
                out.data_ptr() if n else None))

    # -- the selection of components and the logic of masks (dips_mask_select,
    # -- dips_mask_logic) ------------------------------------------------------
    def mask_select(self, mask: ChangeMask, marker: Optional[ChangeMask] = None, connectivity: int = 8,
                    min_area: int = 1, max_area: int = 0, clear_border: bool = False, dropped: bool = False,
                    chunk_frames: int = 0) -> Tuple[ChangeMask, np.ndarray]:
        """(selected, counts): of every frame of `mask` the union of the
        components (mask_components' under `connectivity`) that have at
        least min_area and, unless max_area is 0, at most max_area pixels,
        that hold a set bit of `marker` (None: no such condition; a marker
        of one frame serves every frame) and, with clear_border, that have
        no pixel on the region's border; dropped=True gives the mask minus
        that union.  counts uint32 [n]: the kept components per frame.  A
        mask that lives on the device goes through run_mask_select_device."""
        bits, rw, rh, n = _mask_host_args(mask)
        conn, lo, hi, sel, chunk = _select_args(connectivity, min_area, max_area, clear_border, dropped, chunk_frames)
        mk, mk_n = None, 0
        if marker is not None:
            mk, mw, mh, mk_n = _mask_host_args(marker)
            if (mw, mh) != (rw, rh) or mk_n not in (1, n):
                raise ValueError("marker must hold one frame or the mask's frames of the mask's region")
        out = np.zeros_like(bits)
        counts = np.zeros(n, dtype=np.uint32)
        self._host.check(self._host._lib.dips_mask_select(
            self._host.ptr, bits.ctypes.data if n else None, n, rw, rh, conn, lo, hi, sel,
            mk.ctypes.data if mk is not None and n else None, mk_n if n else 0, chunk,
            out.ctypes.data if n else None, counts.ctypes.data if n else None))
        return ChangeMask(out, rw), counts

    def run_mask_select_device(self, mask, width: int, out, marker=None, counts_out=None, connectivity: int = 8,
                               min_area: int = 1, max_area: int = 0, clear_border: bool = False,
                               dropped: bool = False, chunk_frames: int = 0, stream=None) -> None:
        """Asynchronous: mask and out uint8 device tensors [N, h, row_bytes]
        as run_change_mask_device writes them for a region `width` pixels
        wide, marker (None: none) such a tensor of 1 or N frames, counts_out
        (None: not produced) a 4-byte device tensor [N]; all 4-byte aligned,
        no output overlapping an input or the other output.  Every byte of
        out and every entry of counts_out is written."""
        rw, rh, n = _mask_device_args(mask, width)
        conn, lo, hi, sel, chunk = _select_args(connectivity, min_area, max_area, clear_border, dropped, chunk_frames)
        if tuple(out.shape) != tuple(mask.shape) or out.dtype != mask.dtype:
            raise ValueError("out must be a uint8 tensor of the shape of mask")
        mk_n = 0
        if marker is not None:
            mw, mh, mk_n = _mask_device_args(marker, width)
            if mh != rh or mk_n not in (1, n):
                raise ValueError("marker must hold one frame or the mask's frames of the mask's region")
        if counts_out is not None and (tuple(counts_out.shape) != (n,) or counts_out.element_size() != 4):
            raise ValueError("counts_out must be a 4-byte tensor of shape [N]")
        ins = [mask] + ([marker] if marker is not None else [])
        outs = [out] + ([counts_out] if counts_out is not None else [])
        _mask_device_tensors(ins, outs)
        lib = self._dev._lib
        with _stream_of(self._dev, mask, stream):
            self._dev.check(lib.dips_mask_select(
                self._dev.ptr, mask.data_ptr() if n else None, n, rw, rh, conn, lo, hi, sel,
                marker.data_ptr() if marker is not None and n else None, mk_n if n else 0, chunk,
                out.data_ptr() if n else None, counts_out.data_ptr() if counts_out is not None and n else None))

    def mask_logic(self, a: ChangeMask, op, b: Optional[ChangeMask] = None) -> ChangeMask:
        """`a` op `b` bit by bit inside the region (MaskLogic: And, Or, Xor,
        AndNot = a & ~b, Not = ~a with no b); a `b` of one frame, a static
        zone mask, serves every frame of `a`.  Masks that live on the device
        go through run_mask_logic_device."""
        op = _logic_op(op, b is not None)
        bits, rw, rh, n = _mask_host_args(a)
        bb, b_n = None, 0
        if b is not None:
            bb, bw, bh, b_n = _mask_host_args(b)
            if (bw, bh) != (rw, rh) or b_n not in (1, n):
                raise ValueError("b must hold one frame or a's frames of a's region")
        out = np.zeros_like(bits)
        self._host.check(self._host._lib.dips_mask_logic(
            self._host.ptr, bits.ctypes.data if n else None, n, rw, rh, op,
            bb.ctypes.data if bb is not None and n else None, b_n if n else 0, out.ctypes.data if n else None))
        return ChangeMask(out, rw)

    def run_mask_logic_device(self, a, width: int, out, op, b=None, stream=None) -> None:
        """Asynchronous: a and out uint8 device tensors [N, h, row_bytes] as
        run_change_mask_device writes them for a region `width` pixels wide,
        b (None with MaskLogic.Not) such a tensor of 1 or N frames; all
        4-byte aligned, out overlapping neither input.  Every byte of out is
        written."""
        op = _logic_op(op, b is not None)
        rw, rh, n = _mask_device_args(a, width)
        if tuple(out.shape) != tuple(a.shape) or out.dtype != a.dtype:
            raise ValueError("out must be a uint8 tensor of the shape of a")
        b_n = 0
        if b is not None:
            bw, bh, b_n = _mask_device_args(b, width)
            if bh != rh or b_n not in (1, n):
                raise ValueError("b must hold one frame or a's frames of a's region")
        _mask_device_tensors([a] + ([b] if b is not None else []), [out])
        lib = self._dev._lib
        with _stream_of(self._dev, a, stream):
            self._dev.check(lib.dips_mask_logic(
                self._dev.ptr, a.data_ptr() if n else None, n, rw, rh, op,
                b.data_ptr() if b is not None and n else None, b_n if n else 0, out.data_ptr() if n else None))

    def mask_fill_holes(self, mask: ChangeMask, connectivity: int = 8, max_hole: int = 0) -> ChangeMask:
        """`mask` with its holes filled.  The holes of a frame are the
        components of its complement inside the region that do not touch the
        region's border, taken under the dual connectivity (4 for a mask read
        under 8, 8 for 4); with max_hole != 0 only holes of at most max_hole
        pixels are filled.  The mask goes to the device once
        (run_mask_fill_holes_device)."""
        import torch
        bits, rw, rh, n = _mask_host_args(mask)
        if int(max_hole) < 0 or int(max_hole) > 0xFFFFFFFF:
            raise ValueError("max_hole must be a non-negative 32-bit integer")
        _select_args(connectivity, 1, max_hole, True, False, 0)
        dev = torch.device("cuda", self._dev.device)
        m = torch.from_numpy(bits).to(dev)
        out, scratch = torch.empty_like(m), torch.empty_like(m)
        self.run_mask_fill_holes_device(m, rw, out, scratch, connectivity, max_hole)
        return ChangeMask(out.cpu().numpy(), rw)  # the copy waits for the stream

    def run_mask_fill_holes_device(self, mask, width: int, out, scratch, connectivity: int = 8, max_hole: int = 0,
                                   stream=None) -> None:
        """Asynchronous mask_fill_holes: mask, out and scratch uint8 device
        tensors of one shape [N, h, row_bytes], none overlapping another.
        Three calls in the stream: out = NOT mask; scratch = the components
        of out under the dual connectivity that do not touch the border (of
        at most max_hole pixels unless 0); out = mask OR scratch."""
        if int(max_hole) < 0 or int(max_hole) > 0xFFFFFFFF:
            raise ValueError("max_hole must be a non-negative 32-bit integer")
        conn, _, hole, _, _ = _select_args(connectivity, 1, max_hole, True, False, 0)
        self.run_mask_logic_device(mask, width, out, MaskLogic.Not, stream=stream)
        self.run_mask_select_device(out, width, scratch, connectivity=12 - conn, max_area=hole, clear_border=True,
                                    stream=stream)
        self.run_mask_logic_device(mask, width, out, MaskLogic.Or, scratch, stream=stream)

    def hysteresis_mask(self, frames, tau_high: float, roi=None, ref=None, connectivity: int = 8) -> ChangeMask:
        """Hysteresis thresholding: the components of the operator's change
        mask (the weak mask, at the operator's tau) that hold a pixel of the
        change mask at tau_high >= tau (the strong mask): whole objects from
        the low threshold, only where the high one fires.  frames / ref:
        numpy arrays (uploaded once) or uint8 device tensors; both masks
        stay on the device.  The strong mask comes from a second device
        handle at tau_high, made on first use and closed with the operator."""
        import torch
        tau_high = float(tau_high)
        if not tau_high >= self.tau:
            raise ValueError("tau_high must be at least the operator's tau")
        if int(connectivity) not in (4, 8):
            raise ValueError("connectivity must be 4 or 8")
        dev = torch.device("cuda", self._dev.device)

        def on_device(a):
            if a is None or isinstance(a, torch.Tensor):
                return a
            return torch.from_numpy(_as_u8(a)).to(dev)

        frames, ref = on_device(frames), on_device(ref)
        n, h, w = _frame_geometry(frames, self.fmt)
        rh, rw = self._region(roi, h, w)
        if ref is not None:
            ref = ref.reshape(-1)
        strong_hd = self._strong.get(tau_high)
        if strong_hd is None:
            strong_hd = self._strong[tau_high] = _Handle(_params(tau=tau_high, **self._strong_params),
                                                         self._dev.device)
        weak = torch.empty((n, rh, 4 * ((rw + 31) // 32)), dtype=torch.uint8, device=dev)
        strong, out = torch.empty_like(weak), torch.empty_like(weak)
        self.run_change_mask_device(frames, weak, roi=roi, ref=ref)
        self.run_change_mask_device(frames, strong, roi=roi, ref=ref, _handle=strong_hd)
        if n:
            self.run_mask_select_device(weak, rw, out, marker=strong, connectivity=connectivity)
        return ChangeMask(out.cpu().numpy(), rw)  # the copy waits for the stream

    # -- the statistics of a change mask (dips_mask_counts, dips_mask_pixel_times)
    def mask_counts(self, mask: ChangeMask, rows: int = 1, cols: int = 1) -> np.ndarray:
        """uint32 [n, rows, cols]: the set bits of every frame of `mask` in
        every cell of a rows x cols grid over its region, cut as grid_cell
        cuts it (rows = cols = 1: the count series of the mask).  A mask that
        lives on the device goes through run_mask_counts_device."""
        bits, rw, rh, n = _mask_host_args(mask)
        rows, cols = _mask_grid_args(rows, cols, rw, rh, n)
        out = np.zeros((n, rows, cols), dtype=np.uint32)
        self._host.check(self._host._lib.dips_mask_counts(
            self._host.ptr, bits.ctypes.data if n else None, n, rw, rh, rows, cols, out.ctypes.data if n else None))
        return out

    def run_mask_counts_device(self, mask, width: int, counts_out, rows: int = 1, cols: int = 1, stream=None) -> None:
        """Asynchronous: mask a uint8 device tensor [N, h, row_bytes] as
        run_change_mask_device writes it for a region `width` pixels wide,
        counts_out a 4-byte device tensor [N, rows, cols]; both 4-byte
        aligned, not overlapping.  Every entry of counts_out is written."""
        rw, rh, n = _mask_device_args(mask, width)
        rows, cols = _mask_grid_args(rows, cols, rw, rh, n)
        if tuple(counts_out.shape) != (n, rows, cols) or counts_out.element_size() != 4:
            raise ValueError("counts_out must be a 4-byte tensor of shape [N, rows, cols]")
        _mask_device_outputs(mask, [counts_out])
        lib = self._dev._lib
        with _stream_of(self._dev, mask, stream):
            self._dev.check(lib.dips_mask_counts(
                self._dev.ptr, mask.data_ptr() if n else None, n, rw, rh, rows, cols,
                counts_out.data_ptr() if n else None))

    def _mask_times_host(self, mask_args, t0: int, times: Optional[np.ndarray], sums: Optional[np.ndarray],
                         accumulate: bool) -> None:
        bits, rw, rh, n = mask_args
        for out, planes in ((times, (4, rh, rw)), (sums, (rh, rw))):
            if out is not None and out.shape != planes:
                raise ValueError("into must hold the result of the same region")
        if int(t0) < 0 or int(t0) > 0xFFFFFFFF:
            raise ValueError("t0 must be a non-negative 32-bit integer")
        self._host.check(self._host._lib.dips_mask_pixel_times(
            self._host.ptr, bits.ctypes.data if n else None, n, rw, rh, int(t0), 1 if accumulate else 0,
            times.ctypes.data if times is not None else None, sums.ctypes.data if sums is not None else None))

    def mask_times(self, mask: ChangeMask, t0: int = 0, into: Optional[PixelTimes] = None) -> PixelTimes:
        """The change times of `mask` per pixel, as pixel_times gives them
        for the raw change mask: first, last, run_max, run_cur; frame t of
        the mask has the global index t0 + t.  `into`: a PixelTimes of the
        same region to fold onto (a clip in chunks: t0 = the frames folded so
        far); any chunking gives what one call gives."""
        if into is not None and not isinstance(into, PixelTimes):
            raise ValueError("into must be a PixelTimes")
        args = _mask_host_args(mask)
        if into is not None:
            out = np.ascontiguousarray(into.as_array(), dtype=np.uint32)
        else:
            out = np.zeros((4, args[2], args[1]), dtype=np.uint32)
        self._mask_times_host(args, t0, out, None, into is not None)
        return PixelTimes.from_array(out)

    def mask_sums(self, mask: ChangeMask, into: Optional[np.ndarray] = None) -> np.ndarray:
        """uint32 [h, w]: in how many frames of `mask` each pixel is set
        (pixel_sums' count for the raw change mask), modulo 2^32.  `into`:
        such an array to add onto (it is not modified)."""
        args = _mask_host_args(mask)
        if into is not None:
            out = np.array(into, dtype=np.uint32, order="C")
        else:
            out = np.zeros((args[2], args[1]), dtype=np.uint32)
        self._mask_times_host(args, 0, None, out, into is not None)
        return out

    def run_mask_times_device(self, mask, width: int, times_out=None, sums_out=None, t0: int = 0,
                              accumulate: bool = False, stream=None) -> None:
        """Asynchronous: mask a uint8 device tensor [N, h, row_bytes] as
        run_change_mask_device writes it for a region `width` pixels wide,
        times_out a 4-byte device tensor [4, h, w], sums_out one of [h, w]
        (either may be None, not both), overwritten or (accumulate) folded
        onto; all 4-byte aligned, no output overlapping the mask or the
        other output.  One read of the mask serves both outputs."""
        rw, rh, n = _mask_device_args(mask, width)
        if times_out is None and sums_out is None:
            raise ValueError("times_out and sums_out must not both be None")
        if times_out is not None and (tuple(times_out.shape) != (4, rh, rw) or times_out.element_size() != 4):
            raise ValueError("times_out must be a 4-byte tensor of shape [4, h, w] of the region")
        if sums_out is not None and (tuple(sums_out.shape) != (rh, rw) or sums_out.element_size() != 4):
            raise ValueError("sums_out must be a 4-byte tensor of shape [h, w] of the region")
        if int(t0) < 0 or int(t0) > 0xFFFFFFFF:
            raise ValueError("t0 must be a non-negative 32-bit integer")
        if times_out is not None and int(t0) + n > 0xFFFFFFFF:
            raise ValueError("t0 + n_frames must stay below 2^32")
        _mask_device_outputs(mask, [t for t in (times_out, sums_out) if t is not None])
        lib = self._dev._lib
        with _stream_of(self._dev, mask, stream):
            self._dev.check(lib.dips_mask_pixel_times(
                self._dev.ptr, mask.data_ptr() if n else None, n, rw, rh, int(t0), 1 if accumulate else 0,
                times_out.data_ptr() if times_out is not None else None,
                sums_out.data_ptr() if sums_out is not None else None))

    def change_activity(self, frames, roi=None, ref=None, rows: int = 1, cols: int = 1, morph=None, background=None,
                        sigma_delta=None, vote=None) -> Tuple[np.ndarray, PixelTimes, np.ndarray]:
        """(counts, times, sums) of the cleaned change mask, with the mask
        kept on the device: change_boxes' mask (its roi, ref, background,
        sigma_delta, vote and morph arguments), then mask_counts on a rows x
        cols grid, mask_times from t0 = 0 and mask_sums."""
        return self._activity(frames, roi, ref, rows, cols, morph, background, sigma_delta, vote, None)

    def change_activity_selected(self, frames, select, roi=None, ref=None, rows: int = 1, cols: int = 1, morph=None,
                                 background=None, sigma_delta=None,
                                 vote=None) -> Tuple[np.ndarray, PixelTimes, np.ndarray]:
        """change_activity of the mask behind change_boxes' `select` (a dict
        with keys from min_area, max_area, clear_border, connectivity and
        fill_holes): the statistics no longer hold the pixels of the
        components selected away."""
        if select is None:
            raise ValueError("select must be a dict with keys from " + ", ".join(_SELECT_KEYS))
        return self._activity(frames, roi, ref, rows, cols, morph, background, sigma_delta, vote, select)

    def _activity(self, frames, roi, ref, rows, cols, morph, background, sigma_delta, vote, select):
        import torch
        _mask_grid_args(rows, cols, 0xFFFFFFFF, 0xFFFFFFFF, 0)  # before any device work; the region is checked below
        mask, rw, rh, n = self._change_mask_on_device(frames, roi, ref, morph, background, lambda n_: None,
                                                      sigma_delta, vote, select)
        rows, cols = _mask_grid_args(rows, cols, rw, rh, n)
        dev = mask.device
        counts = torch.empty((n, rows, cols), dtype=torch.int32, device=dev)
        times = torch.empty((4, rh, rw), dtype=torch.int32, device=dev)
        sums = torch.empty((rh, rw), dtype=torch.int32, device=dev)
        self.run_mask_counts_device(mask, rw, counts, rows, cols)
        self.run_mask_times_device(mask, rw, times, sums)

        def to_u32(t):
            return t.cpu().numpy().view(np.uint32)  # the copy waits for the stream

        return to_u32(counts), PixelTimes.from_array(to_u32(times)), to_u32(sums)

    def _change_mask_on_device(self, frames, roi, ref, morph, background, check_args, sigma_delta=None, vote=None,
                               select=None):
        """(mask, region width, region height, n): the change mask of
        change_boxes / change_tracks as a device tensor, behind its vote,
        its morph steps, its selection and its hole filling; check_args(n)
        runs once the geometry is known."""
        import torch
        if sigma_delta is not None and background is not None:
            raise ValueError("sigma_delta and background exclude each other")
        sd = _sigma_delta_option(sigma_delta) if sigma_delta is not None else None
        sel = _select_option(select) if select is not None else None
        dev = torch.device("cuda", self._dev.device)

        def on_device(a):
            if a is None or isinstance(a, torch.Tensor):
                return a
            return torch.from_numpy(_as_u8(a)).to(dev)

        frames, ref = on_device(frames), on_device(ref)
        n, h, w = _frame_geometry(frames, self.fmt)
        rh, rw = self._region(roi, h, w)
        check_args(n)
        steps = _morph_steps(morph, rw, rh) if morph is not None else []
        vote = _vote_option(vote) if vote is not None else None
        if background is not None:
            bg_k, bg_sel = background if isinstance(background, (tuple, list)) else (background, False)
            _background_args(bg_k, bg_sel)
            if n == 0 and ref is None:
                raise ValueError("the initial background needs ref or a frame")
        if sd is not None and n == 0 and ref is None:
            raise ValueError("the initial state needs ref or a frame")
        if ref is not None:
            ref = ref.reshape(-1)
        mask = torch.empty((n, rh, 4 * ((rw + 31) // 32)), dtype=torch.uint8, device=dev)
        if sd is not None:
            state = torch.empty((_lib.SD_PLANES, rh, rw), dtype=torch.int16, device=dev)
            self.run_sigma_delta_mask_device(frames, state, mask, roi=roi, ref=ref, n_amp=sd[0], v_min=sd[1], v_max=sd[2])
        elif background is None:
            self.run_change_mask_device(frames, mask, roi=roi, ref=ref)
        else:
            bg = torch.empty((int(self.fmt), rh, rw), dtype=torch.int16, device=dev)
            self.run_background_mask_device(frames, bg, mask, roi=roi, ref=ref, rate_shift=bg_k, selective=bg_sel)
        other = torch.empty_like(mask) if steps or vote is not None else None
        if vote is not None:  # one-shot: clear frames before the clip, no history kept
            self.run_mask_vote_device(mask, rw, other, vote[0], vote[1])
            mask, other = other, mask
        if steps:
            for op_, shape_, rx_, ry_ in steps:  # ping-pong: the newest mask is `mask`
                self.run_mask_morph_device(mask, rw, other, op_, rx_, ry_, shape_)
                mask, other = other, mask
        if sel is not None and n:
            if int(sel["min_area"]) > 1 or int(sel["max_area"]) != 0 or sel["clear_border"]:
                other = torch.empty_like(mask) if other is None else other
                self.run_mask_select_device(mask, rw, other, connectivity=sel["connectivity"],
                                            min_area=sel["min_area"], max_area=sel["max_area"],
                                            clear_border=sel["clear_border"])
                mask, other = other, mask
            fill = sel["fill_holes"]
            if fill:  # True: every hole; a number: the holes of at most that many pixels
                other = torch.empty_like(mask) if other is None else other
                filled = torch.empty_like(mask)
                self.run_mask_fill_holes_device(mask, rw, filled, other, sel["connectivity"],
                                                0 if isinstance(fill, bool) else int(fill))
                mask = filled
        return mask, rw, rh, n

    def change_boxes(self, frames, roi=None, ref=None, connectivity: int = 8, min_area: int = 1,
                     max_boxes: int = 64, labels: bool = False, morph=None, background=None,
                     sigma_delta=None, vote=None, select=None, shapes: bool = False):
        """change_mask, then mask_components, with the mask kept on the
        device between the two: the moving objects of every frame.  frames /
        ref: numpy arrays (uploaded once) or uint8 device tensors.  morph: a
        sequence of (op, shape, rx, ry) steps of mask_morph applied in order
        to the mask before its components are taken (None: none).
        background: None, or rate_shift or (rate_shift, selective) to take
        the mask against the running-average background (background_mask)
        instead of the operator's mode.  sigma_delta: None, or True or
        (n_amp, v_min, v_max) to take the mask under the Sigma-Delta model's
        per-pixel threshold (sigma_delta_mask); it excludes background.
        vote: None, or window or (window, votes) of mask_vote, applied to
        the model's mask before the morph steps with clear frames before the
        clip (the call is one-shot: no history is carried).  select: None,
        or a dict with keys from min_area, max_area, clear_border,
        connectivity and fill_holes (True, or the largest hole to fill):
        after the morph steps the mask becomes mask_select's of it, then
        mask_fill_holes' of that, so that the pixels of the components
        dropped leave the mask and not only the records.  shapes=True
        returns (ChangeBoxes, ChangeShapes): the records come from
        mask_shapes (no weights) instead of mask_components, so the mask is
        still labelled once; it has no label image, so it excludes labels."""
        import torch
        if shapes and labels:
            raise ValueError("shapes=True produces no label image")
        mask, rw, rh, n = self._change_mask_on_device(
            frames, roi, ref, morph, background,
            lambda n_: _components_args(connectivity, min_area, max_boxes, 0, n_), sigma_delta, vote, select)
        dev, k = mask.device, int(max_boxes)
        counts = torch.empty((n,), dtype=torch.int32, device=dev)
        boxes = torch.empty((n, k, _lib.BOX_WORDS), dtype=torch.int32, device=dev)
        lab = torch.empty((n, rh, rw), dtype=torch.int32, device=dev) if labels else None

        def to_u32(t):
            return t.cpu().numpy().view(np.uint32)  # the copy waits for the stream

        if shapes:
            rec = torch.empty((n, k, _lib.SHAPE_WORDS), dtype=torch.int32, device=dev)
            self.run_mask_shapes_device(mask, rw, counts, boxes, rec, connectivity=connectivity, min_area=min_area)
            counts, boxes = to_u32(counts), to_u32(boxes)
            return ChangeBoxes(counts, boxes, None), ChangeShapes(counts, boxes, to_u32(rec))
        self.run_mask_components_device(mask, rw, counts, boxes, lab, connectivity=connectivity, min_area=min_area)
        return ChangeBoxes(to_u32(counts), to_u32(boxes), to_u32(lab) if lab is not None else None)

    def change_tracks(self, frames, roi=None, ref=None, connectivity: int = 8, min_area: int = 1,
                      max_boxes: int = 64, morph=None, background=None, sigma_delta=None,
                      vote=None, select=None, shapes: bool = False):
        """change_mask, then mask_tracks, with the mask kept on the device
        between the two: the moving objects of every frame and their
        identity from frame to frame.  The arguments are change_boxes'; the
        state of the result continues the ids in a later mask_tracks call.
        shapes=True returns (ChangeTracks, ChangeShapes), shapes record k of
        frame t describing the component of link record k; the shapes come
        from a mask_shapes call (no weights) in addition to mask_tracks, so
        the mask is labelled twice."""
        import torch
        mask, rw, rh, n = self._change_mask_on_device(
            frames, roi, ref, morph, background,
            lambda n_: _tracks_args(connectivity, min_area, max_boxes, 0, n_), sigma_delta, vote, select)
        dev, k = mask.device, int(max_boxes)
        counts = torch.empty((n,), dtype=torch.int32, device=dev)
        boxes = torch.empty((n, k, _lib.BOX_WORDS), dtype=torch.int32, device=dev)
        links = torch.empty((n, k, _lib.LINK_WORDS), dtype=torch.int32, device=dev)
        state = torch.zeros((1 + 2 * k,), dtype=torch.int32, device=dev)
        self.run_mask_tracks_device(mask, rw, counts, boxes, links, state=state, connectivity=connectivity,
                                    min_area=min_area)

        def to_u32(t):
            return t.cpu().numpy().view(np.uint32)  # the copy waits for the stream

        tracks = ChangeTracks(to_u32(counts), to_u32(boxes), to_u32(links), to_u32(state))
        if not shapes:
            return tracks
        rec = torch.empty((n, k, _lib.SHAPE_WORDS), dtype=torch.int32, device=dev)
        self.run_mask_shapes_device(mask, rw, counts, boxes, rec, connectivity=connectivity, min_area=min_area)
        return tracks, ChangeShapes(tracks.counts, tracks.boxes, to_u32(rec))

    # -- the change times per pixel (dips_diff_pixel_times) --------------------
    def pixel_times(self, frames: np.ndarray, roi=None, ref: Optional[np.ndarray] = None, t0: int = 0,
                    into: Optional[PixelTimes] = None) -> PixelTimes:
        """Per pixel of roi = (x, y, w, h) (None: the whole frame) the index
        of the first and of the last frame whose change_mask bit is set, the
        longest run of set bits and the run ending at the last frame; frame
        t of the batch has the global index t0 + t.  `into`: a PixelTimes of
        the same region to fold onto (a clip in chunks: t0 = the frames
        folded so far, and the previous chunk's last frame as ref in
        per-frame mode, the same reference in overall mode)."""
        frames = _as_u8(frames)
        n, h, w = _frame_geometry(frames, self.fmt)
        rh, rw = self._region(roi, h, w)
        if int(t0) < 0 or int(t0) > 0xFFFFFFFF:
            raise ValueError("t0 must be a non-negative 32-bit integer")
        if into is not None:
            out = np.ascontiguousarray(into.as_array(), dtype=np.uint32)
            if out.shape != (4, rh, rw):
                raise ValueError("into must hold the times of the same region")
        else:
            out = np.zeros((4, rh, rw), dtype=np.uint32)
        rp = None
        if ref is not None:
            ref = _as_u8(ref)
            if ref.size != h * w * int(self.fmt):
                raise ValueError("ref must have the shape of one frame")
            rp = ref.ctypes.data
        self._host.check(self._host._lib.dips_diff_pixel_times(
            self._host.ptr, w, h, frames.ctypes.data if n else None, n, rp, _roi_arg(roi), int(t0),
            1 if into is not None else 0, out.ctypes.data))
        return PixelTimes.from_array(out)

    def run_pixel_times_device(self, frames, times_out, roi=None, ref=None, t0: int = 0, accumulate: bool = False,
                               stream=None) -> None:
        """Asynchronous: frames / ref uint8 device tensors, times_out a
        4-byte device tensor of shape [4, h, w] of the region (4-byte
        aligned), overwritten or (accumulate) folded onto."""
        n, h, w = _frame_geometry(frames, self.fmt)
        rh, rw = self._region(roi, h, w)
        if tuple(times_out.shape) != (4, rh, rw) or times_out.element_size() != 4:
            raise ValueError("times_out must be a 4-byte tensor of shape [4, h, w] of the region")
        if int(t0) < 0 or int(t0) > 0xFFFFFFFF:
            raise ValueError("t0 must be a non-negative 32-bit integer")
        for t in (frames, times_out, ref):
            if t is not None and (not t.is_cuda or not t.is_contiguous()):
                raise ValueError("device path needs contiguous HIP tensors")
        import torch
        for t in (frames, ref):
            if t is not None and t.dtype != torch.uint8:
                raise ValueError("frames and ref must be uint8 tensors")
        if ref is not None and ref.numel() != h * w * int(self.fmt):
            raise ValueError("ref must have the size of one frame")
        lib = self._dev._lib
        with _stream_of(self._dev, frames, stream):
            self._dev.check(lib.dips_diff_pixel_times(
                self._dev.ptr, w, h, frames.data_ptr() if n else None, n,
                ref.data_ptr() if ref is not None else None, _roi_arg(roi), int(t0), 1 if accumulate else 0,
                times_out.data_ptr() if times_out.numel() else None))

    # -- frame-range sharding (native: shard_abi.hip) -------------------------
    def run_sharded(self, comm, frames, n_total: int, series_local, series_all=None, ref=None,
                    ref_resident: bool = False, stream=None) -> None:
        """dips_diff_series_sharded on device tensors, asynchronous on the
        tensor's current stream: this rank's frames [n_local, H, W(, C)]
        (its dips_shard_range of n_total), series_local int64 [n_local, 4],
        series_all int64 [n_total, 4] on rank 0 (ignored elsewhere); `ref`:
        'overall' rank 0's reference (None = its first frame) or, with
        ref_resident, every rank's copy; 'per-frame' rank 0's predecessor of
        global frame 0 (None = frame 0)."""
        n, h, w = _frame_geometry(frames, self.fmt)
        if tuple(series_local.shape) != (n, 4) or series_local.element_size() != 8:
            raise ValueError("series_local must be an 8-byte tensor of shape [n_local, 4]")
        if comm.rank == 0 and (series_all is None or tuple(series_all.shape) != (int(n_total), 4)
                               or series_all.element_size() != 8):
            raise ValueError("rank 0 needs series_all, an 8-byte tensor of shape [n_total, 4]")
        for t in (frames, series_local, series_all, ref):
            if t is not None and (not t.is_cuda or not t.is_contiguous()):
                raise ValueError("device path needs contiguous HIP tensors")
        if ref is not None and ref.numel() != h * w * int(self.fmt):
            raise ValueError("ref must have the size of one frame")
        lib = self._dev._lib
        with _stream_of(self._dev, frames, stream):
            self._dev.check(lib.dips_diff_series_sharded(
                self._dev.ptr, comm.ptr, w, h, frames.data_ptr(), n, int(n_total),
                ref.data_ptr() if ref is not None else None,
                _lib.SHARD_REF_RESIDENT if ref_resident else 0, series_local.data_ptr(),
                series_all.data_ptr() if (series_all is not None and comm.rank == 0) else None))

    def sharded(self, comm, frames: np.ndarray, n_total: int, ref: Optional[np.ndarray] = None,
                ref_resident: bool = False) -> Tuple[Series, Optional[Series]]:
        """The same on host arrays (staged through HBM, synchronous):
        returns (this rank's series, the gathered series on rank 0 / None)."""
        frames = _as_u8(frames)
        n, h, w = _frame_geometry(frames, self.fmt)
        local = np.zeros((n, 4), dtype=np.uint64)
        full = np.zeros((int(n_total), 4), dtype=np.uint64) if comm.rank == 0 else None
        rp = None
        if ref is not None:
            ref = _as_u8(ref)
            if ref.size != h * w * int(self.fmt):
                raise ValueError("ref must have the shape of one frame")
            rp = ref.ctypes.data
        self._host.check(self._host._lib.dips_diff_series_sharded(
            self._host.ptr, comm.ptr, w, h, frames.ctypes.data, n, int(n_total), rp,
            _lib.SHARD_REF_RESIDENT if ref_resident else 0, local.ctypes.data,
            full.ctypes.data if full is not None else None))
        return Series.from_array(local), (Series.from_array(full) if full is not None else None)

    def shard_broadcast_device(self, comm, frame, out, stream=None) -> None:
        """Rank 0's `frame` into `out` on every rank (dips_shard_broadcast)."""
        h, w = int(out.shape[0]), int(out.shape[1])
        lib = self._dev._lib
        with _stream_of(self._dev, out, stream):
            self._dev.check(lib.dips_shard_broadcast(self._dev.ptr, comm.ptr, w, h,
                                                     frame.data_ptr() if frame is not None else None,
                                                     out.data_ptr()))

    def shard_plan(self, comm, width: int, height: int, n_total: int) -> dict:
        """dips_shard_plan: this rank's frame range and the waves of its
        series launch beside the halo transfer (and uncapped)."""
        first, count = ctypes.c_uint64(), ctypes.c_uint32()
        waves, unc = ctypes.c_uint64(), ctypes.c_uint64()
        self._dev.check(self._dev._lib.dips_shard_plan(self._dev.ptr, comm.ptr, width, height, int(n_total),
                                                       ctypes.byref(first), ctypes.byref(count),
                                                       ctypes.byref(waves), ctypes.byref(unc)))
        return {"first": first.value, "count": count.value, "waves": waves.value, "waves_uncapped": unc.value}

    def shard_reference_device(self, out, stream=None) -> bool:
        """The reference the last run_sharded used for this rank's first
        frame, into a uint8 device tensor; False before any sharded call."""
        with _stream_of(self._dev, out, stream):
            return self._dev.check(self._dev._lib.dips_shard_reference(self._dev.ptr, out.data_ptr(),
                                                                       out.numel())) == 1

    def synth_device(self, dst, width: int, height: int, seed: int, t0: int, stream=None) -> None:
        """Fill a uint8 device tensor [N, H, W(, C)] with synthetic frames t0..t0+N-1."""
        n = dst.shape[0]
        lib = self._dev._lib
        with _stream_of(self._dev, dst, stream):
            self._dev.check(lib.dips_synth_frames(self._dev.ptr, width, height, int(seed), int(t0), n,
                                                  dst.data_ptr()))

    def read_ceiling_ms(self, tensor) -> float:
        """hipEvent time of one read-only stream over a device tensor's bytes."""
        ms = ctypes.c_double()
        self._dev.check(self._dev._lib.dips_read_ceiling(self._dev.ptr, tensor.data_ptr(),
                                                         tensor.numel() * tensor.element_size(),
                                                         ctypes.byref(ms)))
        return ms.value

    def read_ceiling_walk_ms(self, frames) -> float:
        """hipEvent time of one read-only walk over device frames [N, H, W, C]
        in the series kernel's own access shape (RGB8 / RGBA8)."""
        n, h, w = _frame_geometry(frames, self.fmt)
        ms = ctypes.c_double()
        self._dev.check(self._dev._lib.dips_read_ceiling_walk(self._dev.ptr, frames.data_ptr(), w, h, n,
                                                              ctypes.byref(ms)))
        return ms.value

    def kernel_times(self) -> List[float]:
        """Per-launch hipEvent times (ms) of the series kernel since the last reset."""
        lib, ptr = self._dev._lib, self._dev.ptr
        n = ctypes.c_uint64()
        self._dev.check(lib.dips_kernel_time_each(ptr, None, 0, ctypes.byref(n)))
        buf = (ctypes.c_double * max(1, n.value))()
        self._dev.check(lib.dips_kernel_time_each(ptr, buf, n.value, ctypes.byref(n)))
        return list(buf[: n.value])

    def kernel_time(self, reset: bool = False) -> Tuple[float, int]:
        ms = ctypes.c_double()
        cnt = ctypes.c_uint64()
        self._dev.check(self._dev._lib.dips_kernel_time(self._dev.ptr, ctypes.byref(ms), ctypes.byref(cnt)))
        out = (ms.value, cnt.value)
        if reset:
            self._dev.check(self._dev._lib.dips_kernel_time_reset(self._dev.ptr))
        return out

    def geometry(self, width: int, height: int, n_frames: int) -> Tuple[int, int, int]:
        waves, tiles, pbytes = ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_uint64()
        self._dev.check(self._dev._lib.dips_series_geometry(
            self._dev.ptr, width, height, n_frames, ctypes.byref(waves), ctypes.byref(tiles),
            ctypes.byref(pbytes)))
        return waves.value, tiles.value, pbytes.value


def diff_series(frames: np.ndarray, *, fmt: Optional[PixelFormat] = None, mode: Mode = Mode.Overall,
                tau: float = 0.0, chroma_filter: ChromaFilter = ChromaFilter.None_,
                ref: Optional[np.ndarray] = None, want_map: bool = False, device: int = 0,
                force_generic: bool = False, crosscheck: bool = False) -> Tuple[Series, Optional[np.ndarray]]:
    """One-shot helper over DiffSeriesOperator for host arrays."""
    if fmt is None:
        fmt = PixelFormat.Gray8 if frames.ndim == 3 else PixelFormat(frames.shape[-1])
    op = DiffSeriesOperator(fmt, mode, tau, chroma_filter, device, force_generic=force_generic,
                            crosscheck=crosscheck)
    try:
        return op(frames, ref=ref, want_map=want_map)
    finally:
        op.close()


def si_from_fixed(si_fixed) -> np.ndarray:
    return np.ldexp(np.asarray(si_fixed, dtype=np.float64), -32)


__all__ = [
    "DiPsFilter", "ChromaFilter", "PixelFormat", "Mode", "DiPsProperties", "ComputeState",
    "frame_callback", "perform_dips_frames", "Series", "GridSeries", "PixelSums", "PixelTimes", "ChangeMask", "ChangeBoxes", "ChangeTracks", "ChangeShapes", "Background", "SigmaDelta", "mask_row_bytes", "grid_cell",
    "DiffSeriesOperator",
    "diff_series",
    "si_from_fixed", "VideoPathNotSpecifiedError", "FrameCallbackNotSpecifiedError", "DipsError",
]
