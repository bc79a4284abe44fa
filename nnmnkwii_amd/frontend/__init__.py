"""Linguistic frontends on the device.  ``merlin``: frame-level linguistic features from phone-level ones and durations."""
from . import merlin  # noqa: F401
