"""
Write tests/golden/f16_denoising_losses.npz: the reference's own denoising losses, speaker-search losses, tone items and
LossTracker averages on deterministic weights and seeded inputs.  Runs on the CPU where a checkout of the reference
(unixpickle/vq-voice-swap) is at hand; the reference is IMPORTED, never copied, and only data is written.

    python tools/gen_loss_golden.py --reference /path/to/vq-voice-swap        (or VQVS_REFERENCE=/path/...)

Sections of the file (T = 16384 throughout):
  a_*  unconditional unet32: ddpm_losses on 4 rows, one t per quartile; sample_q of row 0; r = |pred| / |noise - pred| per row
  b_*  VQVAE(32, num_labels 5): the reference script's evaluate_losses at 4 timesteps x 5 labels, 2 seeds, batch 8
  c_*  items 0, 4, 29 of ToneDataset (label, first 64 samples), linear and ulaw
  d_*  a sequence of (ts, mses) batches and LossTracker(avg_size=5).log_dict() after each (NaN = bucket still empty)
"""

from __future__ import annotations

import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T = 16384
FP32_REL = 1e-4  # the per-forward relative-RMS bound of the fp32 mode (tests/test_parity_gpu.py)


def bound(r, rho=FP32_REL):
    """Relative loss error allowed by a relative-RMS error rho of the prediction: 2 rho r + (rho r)^2, r = |pred| / |noise - pred|."""
    return 2 * rho * r + (rho * r) ** 2


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=os.environ.get("VQVS_REFERENCE"), help="checkout of the reference repository")
    args = ap.parse_args()
    if not args.reference or not os.path.isdir(os.path.join(args.reference, "vq_voice_swap")):
        raise SystemExit("pass --reference (or VQVS_REFERENCE): the directory that holds the reference's vq_voice_swap/ package")
    ref = os.path.abspath(args.reference)
    # the repository ships an import shim of the same name: the reference must win here
    sys.path = [ref] + [p for p in sys.path if os.path.abspath(p or ".") not in (ROOT, ref)] + [ROOT]

    import vq_voice_swap as ref_pkg
    assert os.path.abspath(ref_pkg.__file__).startswith(ref), f"not the reference: {ref_pkg.__file__}"
    import voice_search_vqvae as ref_search  # the reference's script (its evaluate_losses)
    from vq_voice_swap.dataset import ToneDataset
    from vq_voice_swap.diffusion_model import DiffusionModel
    from vq_voice_swap.loss_tracker import LossTracker
    from vq_voice_swap.vq_vae import VQVAE

    from tests.util import seeded
    from vq_voice_swap_amd.det_init import det_init_

    assert os.path.abspath(ref_search.__file__).startswith(ref), ref_search.__file__
    torch.set_num_threads(8)
    out = {}

    def det_model(m):
        det_init_(m.state_dict().items())
        m.eval()
        return m

    # ---- A: unconditional unet32
    model = det_model(DiffusionModel("unet", 32))
    a_x_seed, a_noise_seed = 101, 102
    x = 0.3 * seeded((4, 1, T), a_x_seed)
    noise = seeded((4, 1, T), a_noise_seed)
    ts = torch.tensor([0.02, 0.3, 0.6, 0.97])
    with torch.no_grad():
        losses = model.diffusion.ddpm_losses(x, model.predictor, ts, noise)
        x_t = model.diffusion.sample_q(x, ts, epsilon=noise)
        pred = model.predictor(x_t, ts)
    again = ((noise - pred) ** 2).flatten(1).mean(1)
    assert torch.allclose(losses, again, rtol=1e-6), (losses, again)
    r = pred.flatten(1).double().norm(dim=1) / (noise - pred).flatten(1).double().norm(dim=1)
    print("A: losses", losses.tolist(), "r", r.tolist())
    out.update(a_x_seed=a_x_seed, a_x_scale=0.3, a_noise_seed=a_noise_seed, a_ts=ts.numpy(), a_losses=losses.numpy(),
               a_x_t_row0=x_t[0, 0].numpy(), a_r=r.numpy())

    # ---- B: speaker search on VQVAE(32), 5 labels
    vq = det_model(VQVAE(base_channels=32, pred_name="unet", num_labels=5))
    b_dict_seed, num_ts, num_seeds, batch_size = 77, 4, 2, 8
    with torch.no_grad():
        vq.vq.dictionary.copy_(seeded(vq.vq.dictionary.shape, b_dict_seed, 0.35))
    labels = torch.tensor([i for i in range(5) for _ in range(num_ts)]).long()
    ts = torch.linspace(0.0, 1.0, steps=num_ts, dtype=torch.float32).repeat(5)
    chosen = None
    for b_x_seed in range(201, 221):
        target = (0.1 * seeded((1, 1, T), b_x_seed)).clamp(-1, 1)
        b_noise_seed = 1000 + b_x_seed
        with torch.no_grad():
            codes = vq.encode(target)
            encoded = vq.vq.embed(codes).detach()
            torch.manual_seed(b_noise_seed)
            row_losses = ref_search.evaluate_losses(vq, target, labels, ts, encoded, batch_size, num_seeds)
            torch.manual_seed(b_noise_seed)
            eps = torch.randn_like(target[None].repeat(num_seeds, 1, 1, 1))  # the draw evaluate_losses made: [num_seeds,1,1,T]
            # r per row (the larger of the two draws), from the reference's own forward
            rs, check_rows = [], []
            for e in eps:
                e_mb = e.repeat(len(ts), 1, 1)
                p = vq.predictor(vq.diffusion.sample_q(target.repeat(len(ts), 1, 1), ts, epsilon=e_mb), ts,
                                 cond=encoded.repeat(len(ts), 1, 1), labels=labels)
                rs.append(p.flatten(1).double().norm(dim=1) / (e_mb - p).flatten(1).double().norm(dim=1))
                check_rows.append(((p - e_mb) ** 2).flatten(1).mean(1))
        assert torch.allclose(torch.stack(check_rows).mean(0), row_losses, rtol=1e-4), "the re-drawn noise is not what evaluate_losses drew"
        r_rows = torch.stack(rs).max(0).values
        means = row_losses.reshape(5, num_ts).mean(-1)
        mean_bound = (bound(r_rows) * row_losses.double()).reshape(5, num_ts).mean(-1)  # absolute, per label
        order = means.argsort()
        gap = (means[order[1]] - means[order[0]]).item()
        need = 10 * max(mean_bound[order[0]].item(), mean_bound[order[1]].item())
        print(f"B: seed {b_x_seed}: label means {means.tolist()}, best-vs-runner-up gap {gap:.3e}, 10 x fp32 bound {need:.3e}")
        if gap > need:
            chosen = b_x_seed
            break
    assert chosen is not None, "no input seed separates the best label from the runner-up by 10 x the fp32 bound"
    out.update(b_x_seed=chosen, b_x_scale=0.1, b_dict_seed=b_dict_seed, b_dict_scale=0.35, b_noise_seed=b_noise_seed,
               b_codes=codes.numpy(), b_labels=labels.numpy(), b_ts=ts.numpy(), b_num_seeds=num_seeds, b_batch_size=batch_size,
               b_noise=eps[:, 0].numpy(), b_losses=row_losses.numpy(), b_label_means=means.numpy(), b_r=r_rows.numpy())

    # ---- C: tones
    for enc in ("linear", "ulaw"):
        ds = ToneDataset(encoding=enc)
        items = [ds[i] for i in (0, 4, 29)]
        out[f"c_{enc}_labels"] = np.array([it["label"] for it in items], dtype=np.int64)
        out[f"c_{enc}_head"] = np.stack([np.asarray(it["samples"][:64], dtype=np.float32) for it in items])
    out["c_items"] = np.array([0, 4, 29], dtype=np.int64)

    # ---- D: tracker with a window that slides
    g = torch.Generator().manual_seed(301)
    tracker = LossTracker(avg_size=5)
    d_ts, d_mses, d_logs = [], [], []
    for _ in range(12):
        bt, bm = torch.rand(6, generator=g), torch.rand(6, generator=g) * 2
        tracker.add(bt, bm)
        log = tracker.log_dict()
        d_ts.append(bt.numpy())
        d_mses.append(bm.numpy())
        d_logs.append([log.get(f"q{i}", float("nan")) for i in range(4)])
    out.update(d_ts=np.stack(d_ts), d_mses=np.stack(d_mses), d_logs=np.array(d_logs, dtype=np.float64), d_avg_size=5)

    path = os.path.join(ROOT, "tests", "golden", "f16_denoising_losses.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path} ({os.path.getsize(path) / 1024:.0f} KiB)")


if __name__ == "__main__":
    main()
