"""Utilities around the writer and the reader (reference: pyrecode/utils)."""
from .calibration import calibrate, make_calibration_frames  # noqa: F401
