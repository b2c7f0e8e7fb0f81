"""ctypes bindings to the hand-written gfx950 calibration kernels (libvgpu_kernels.so)."""
from .calib import cu_census, decode_location, scratch_hog, scratch_reference, spin, spin_lds, stream_copy  # noqa: F401
from .calib import pattern_check, pattern_fill, pattern_poke, pattern_reference  # noqa: F401
from .calib import cu_selftest, selftest_reference  # noqa: F401
from .calib import mem_chase, mem_latency, mem_stream, ring_build, ring_jump, ring_reference  # noqa: F401
