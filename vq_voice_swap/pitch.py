from vq_voice_swap_amd.pitch import PitchDistance  # noqa: F401
