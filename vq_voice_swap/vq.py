from vq_voice_swap_amd.vq import VQ, StandardVQLoss, VQLoss  # noqa: F401
