from vq_voice_swap_amd.losses import LossTracker  # noqa: F401
