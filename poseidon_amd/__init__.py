"""poseidon_amd — MI355X-native scOT (Poseidon) forward/backward engine.  See DESIGN.md."""
# The engine overlaps two to three HIP streams per step (dependent chain, weight gradients, DP exchange).  The ROCm runtime maps a
# process's streams onto GPU_MAX_HW_QUEUES hardware queues and multiplexes the rest; the package leaves that number to the environment
# and measures which streams really run beside each other (poseidon_amd/streams.py).

from .config import ScOTConfig, MODEL_MAP, preset  # noqa: F401
