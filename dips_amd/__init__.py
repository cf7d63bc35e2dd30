"""dips_amd -- MI355X-native (gfx950) DiPs per-pixel frame-difference path.

The compute lives in hand-written HIP kernels behind the C ABI of
include/dips_hip.h (dips_amd/lib/libdips_hip.so); this package is the host
mirror of the reference crate's operator surface (dips/src/lib.rs,
dips/src/gpu/mod.rs) plus the batch difference-series operator and the
frame-range sharding over RCCL (dips_amd.shard).
"""
from . import alt  # dips_alt crate surface (DiPsCompute, run_dips_on_file loop)
from ._lib import DipsError, DipsLibraryError, LIB_PATH, VOTE_MAX_WINDOW, load as load_library
from .api import (Background, ChangeBoxes, ChangeMask, ChangeShapes, ChangeTracks, ChromaFilter, ComputeState, DiffSeriesOperator, DiPsFilter, DiPsProperties,
                  FrameCallbackNotSpecifiedError, GridSeries, MaskLogic, Mode, MorphOp, MorphShape, PixelFormat, PixelSums, PixelTimes, Series,
                  SigmaDelta, VideoPathNotSpecifiedError, diff_series, frame_callback, grid_cell, mask_row_bytes,
                  perform_dips_frames, si_from_fixed)

__all__ = [
    "Background", "ChangeBoxes", "ChangeMask", "ChangeShapes", "ChangeTracks", "ChromaFilter", "ComputeState", "DiffSeriesOperator", "DiPsFilter", "DiPsProperties",
    "DipsError", "DipsLibraryError", "FrameCallbackNotSpecifiedError", "GridSeries", "LIB_PATH", "MaskLogic", "Mode", "MorphOp", "MorphShape",
    "PixelFormat", "PixelSums", "PixelTimes", "Series", "SigmaDelta", "VOTE_MAX_WINDOW", "VideoPathNotSpecifiedError", "diff_series", "frame_callback", "grid_cell",
    "load_library", "mask_row_bytes", "perform_dips_frames", "si_from_fixed",
]
