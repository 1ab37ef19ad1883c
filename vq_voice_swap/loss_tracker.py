from vq_voice_swap_amd.losses import LossTracker, classification_scores  # noqa: F401
