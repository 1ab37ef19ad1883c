#!/usr/bin/env python3
"""
Evaluate an encoder-predictor checkpoint over a data set on MI355X: the cross-entropy of the VQ-VAE's codes, the fraction of
positions predicted correctly and within the top k, on `sample_q(audio, ts)`, per quartile of t and overall -- the number the
reference only logs while it trains (`EncoderPredictorTrainLoop.compute_losses`, train_loop.py:602-613), and the one
`VQVAE.decode(enc_pred=...)` rests on.

Targets are `vq_vae.encode(audio)` (the encoder in fp32, as everywhere); the noise schedule is the VQ-VAE's.  Per batch:
`Diffusion.draw_ts`, `Diffusion.sample_q_seeded`, `EncoderPredictor.scores` (the HIP forward, then one fused scoring kernel
over the [B, num_latents, T / rate] logits).  After every batch one line, the one of eval_classifier.py:

    {n} samples: nll_q0=... nll_q3=... acc_q0=... acc_q3=... top5_q0=... top5_q3=... nll=... acc=...

nll_* is the per-position mean -- the number `EncoderPredictor.losses` returns -- and acc_* / top5_* the fraction of positions;
nll and acc are exact over every position so far.  The common flags, the seeding and the torchrun behaviour are those of the
shared pass (vq_voice_swap_amd/eval_pass.py).
"""
import os
import sys

os.environ.setdefault("HIP_FORCE_DEV_KERNARG", "1")  # kernel arguments in device memory: a process-level HIP switch, set before the runtime starts

import torch  # noqa: E402,F401

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from eval_classifier import EvalState, format_line  # noqa: E402,F401
from vq_voice_swap_amd import VQVAE, EncoderPredictor  # noqa: E402
from vq_voice_swap_amd.eval_pass import common_parser, run_pass  # noqa: E402


def arg_parser():
    p = common_parser()
    p.add_argument("--topk", default=5, type=int, help="k of the top-k accuracy (clipped to the number of codes)")
    p.add_argument("--vq-vae-path", required=True, type=str, help="the VQ-VAE whose codes the model predicts")
    return p


def main(argv=None):
    args = arg_parser().parse_args(argv)

    def build(device, num_labels):
        vq_vae = VQVAE.load(args.vq_vae_path).to(device).eval()
        model = EncoderPredictor.load(args.checkpoint_path).to(device)
        # (what the reference builds the model from: train_loop.py:633-634)
        assert model.num_latents == vq_vae.dictionary_size, f"the model predicts {model.num_latents} codes, the VQ-VAE has {vq_vae.dictionary_size}"
        rate = vq_vae.encoder.downsample_rate
        assert model.downsample_rate == rate, f"the model's downsample rate is {model.downsample_rate}, the VQ-VAE encoder's {rate}"
        model.eval().set_precision(args.precision)
        state = EvalState(model.num_latents, device, args.topk, confusion=False)
        return state, lambda audio, data_batch, first: state.add_batch(model, vq_vae.diffusion, audio, vq_vae.encode(audio), first, args.seed)

    run_pass(args, build, no_device="the guidance models have no CPU path")


if __name__ == "__main__":
    main()
