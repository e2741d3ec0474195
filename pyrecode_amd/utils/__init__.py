"""Utilities around the writer and the reader (reference: pyrecode/utils)."""
from .calibration import calibrate, make_calibration_frames  # noqa: F401
from .converters import l1_to_l4_converter  # noqa: F401
