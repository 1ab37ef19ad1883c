#!/usr/bin/env python3
"""
Cost of the sample-quality statistics on one GPU, as one JSON line:
  - classifier features (`Classifier.features`, probabilities included) in clips/s: classifier32, B = 64, T = 64000, fp32 / fp16;
  - `vqvs_feature_moments` in microseconds per call at (B, F) = (64, 512) and (64, 4096);
  - the in-line statistics of sample_diffusion.py on the headline run (unet64, 50 steps, schedule t**2, constrain, 64 clips,
    fp16): one sampled batch alone, and the same batch followed by wav_roundtrip + features + FeatureStats.update, per
    statistics precision.
Det-init weights (vq_voice_swap_amd/det_init.py); hipEvents on the current stream for the kernels, wall time around a
synchronised batch for the sampling run.
"""
import argparse
import json
import os
import sys
import time

os.environ.setdefault("HIP_FORCE_DEV_KERNARG", "1")  # kernel arguments in device memory: a process-level HIP switch, set before the runtime starts

import torch  # noqa: E402

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from vq_voice_swap_amd import Classifier, DiffusionModel, FeatureStats, randn_clips, wav_roundtrip  # noqa: E402
from vq_voice_swap_amd import _native  # noqa: E402
from vq_voice_swap_amd.det_init import det_init_  # noqa: E402


def event_ms(fn, reps, warmup=2):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def wall_s(fn, reps):
    out = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append(time.perf_counter() - t0)
    return sorted(out)[len(out) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--num-labels", type=int, default=251, help="classifier classes (LibriSpeech train-clean-100 speakers)")
    ap.add_argument("--feature-reps", type=int, default=20)
    ap.add_argument("--moment-reps", type=int, default=50)
    ap.add_argument("--sample-reps", type=int, default=3)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    out = {"metric": "sample-quality statistics cost", "device": torch.cuda.get_device_name(dev)}

    clf = Classifier(num_labels=a.num_labels, base_channels=32)
    det_init_(clf.state_dict().items())
    clf = clf.to(dev).eval()
    B, T = 64, 64000
    x = randn_clips(B, T, dev, 5) * 0.3
    feats = {}
    for prec in ("fp32", "fp16"):
        clf.set_precision(prec)
        ms = event_ms(lambda: clf.features(x, return_probs=True), a.feature_reps)
        feats[prec] = {"ms_per_batch": round(ms, 3), "clips_per_s": round(B / (ms / 1e3), 1)}
    out["classifier32_features_B64_T64000"] = feats

    moments = {}
    for F in (512, 4096):
        f = torch.randn(64, F, device=dev)
        st = FeatureStats(F, dev)
        st.update(f)
        shift, s1, s2 = st._shift, st._s1, st._s2
        L = _native.lib()
        stream = _native._stream_ptr()

        def call():
            _native.check(L.vqvs_feature_moments(f.data_ptr(), 64, F, shift.data_ptr(), s1.data_ptr(), s2.data_ptr(), stream))

        us = event_ms(call, a.moment_reps) * 1e3
        moments[f"B64_F{F}"] = {"us_per_call": round(us, 2), "s2_bytes_rw": 2 * F * F * 8}
    out["feature_moments"] = moments

    model = DiffusionModel("unet", 64)
    det_init_(model.state_dict().items())
    model = model.to(dev).eval()
    model.set_precision("fp16")
    sq = lambda t: t ** 2  # noqa: E731
    x_T = randn_clips(64, T, dev, 3)

    def sample():
        return model.diffusion.ddpm_sample(x_T, model.predictor, 50, constrain=True, schedule=sq, seed=3)

    sample()
    base = wall_s(sample, a.sample_reps)
    inline = {"sample_only_s": round(base, 4)}
    for prec in ("fp32", "fp16"):
        clf.set_precision(prec)
        st = FeatureStats(clf.feature_dim, dev)

        def sample_and_score():
            s = sample()
            feat, probs = clf.features(wav_roundtrip(s, "linear"), return_probs=True)
            st.update(feat)
            st.add_probs(probs)

        sample_and_score()
        t = wall_s(sample_and_score, a.sample_reps)
        inline[f"with_stats_{prec}_s"] = round(t, 4)
        inline[f"overhead_{prec}_pct"] = round(100.0 * (t - base) / base, 2)
    out["inline_stats_unet64_50step_64clips_fp16"] = inline
    out["library"] = _native.lib().vqvs_version().decode()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
