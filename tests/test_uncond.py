"""Label guidance end to end, the parts that need no device: the `vqvs_guidance_mix` entry point (declared, exported, bound, its
argument refusals -- the library refuses on the host before it touches a device), the new flags of the four scripts and their
defaults with the flags absent, and `NullLabelEnroller`'s checkpoint layout and resume refusals on a CPU model."""
import ctypes as C
import os
import re
import sys

import pytest
import torch

from util import flags_of
from vq_voice_swap_amd import VQVAE, DiffusionModel, _native
from vq_voice_swap_amd.det_init import det_init_
from vq_voice_swap_amd.enroll import NullLabelEnroller, SpeakerEnroller

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


# ---------------------------------------------------------------- the entry point
def test_guidance_mix_is_declared_exported_and_bound(lib_built):
    header = " ".join(open(os.path.join(ROOT, "include", "vqvs.h")).read().split())
    decl = re.search(r"int vqvs_guidance_mix\(([^;]*)\);", header)
    assert decl, "include/vqvs.h does not declare vqvs_guidance_mix"
    args = [a.strip() for a in decl.group(1).split(",")]
    assert args == ["const float* d_outs", "float* d_eps", "int rows", "int64_t row_len", "int reps", "float s1", "float s2", "void* stream"]
    assert "vqvs_guidance_mix" in _native.EXPORTS and hasattr(lib_built, "vqvs_guidance_mix")
    assert len(lib_built.vqvs_guidance_mix.argtypes) == len(args)
    assert lib_built.vqvs_guidance_mix.argtypes[3] is C.c_int64  # row_len: 64-bit


def test_guidance_mix_refuses_bad_arguments_without_a_device(lib_built):
    L = lib_built
    buf = (C.c_float * 64)()
    base = C.addressof(buf)
    outs, eps = C.c_void_p(base), C.c_void_p(base + 48 * 4)  # 3 blocks of 4 x 4 floats, eps behind them
    ok = dict(outs=outs, eps=eps, rows=4, row_len=4, reps=3)

    def call(**kw):
        a = dict(ok, **kw)
        return L.vqvs_guidance_mix(a["outs"], a["eps"], a["rows"], a["row_len"], a["reps"], 1.0, 1.0, None)

    for bad in (dict(outs=None), dict(eps=None), dict(rows=0), dict(rows=-1), dict(row_len=0), dict(row_len=-5), dict(reps=0), dict(reps=4),
                dict(reps=-1), dict(rows=2 ** 31 - 1, row_len=2 ** 62),
                dict(eps=C.c_void_p(base + 16 * 4)),   # block 1
                dict(eps=C.c_void_p(base + 32 * 4)),   # block 2
                dict(eps=C.c_void_p(base + 4)),        # block 0 at an offset: not "in place"
                dict(eps=C.c_void_p(base + 40 * 4)),   # straddles the end of block 2
                dict(reps=2, eps=C.c_void_p(base + 16 * 4))):
        assert call(**bad) == -1 and L.vqvs_last_error(), bad
        with pytest.raises(_native.NativeArgumentError):
            _native.check(call(**bad))


# ---------------------------------------------------------------- the scripts' command lines
VQ = ["--label", "2", "--input-file", "in.wav", "ck.pt", "out.wav"]


def test_sample_vqvae_uncond_flags():
    import sample_vqvae
    import sample_vqvae_uncond

    new = ["--whole-file", "--window-seconds", "--overlap-seconds", "--window-batch", "--keep", "--strength"]
    assert set(new) <= set(flags_of(sample_vqvae_uncond.arg_parser()))
    a, b = sample_vqvae_uncond.parse_args(VQ), sample_vqvae.parse_args(VQ)
    for name in ("whole_file", "window_seconds", "overlap_seconds", "window_batch", "keep", "strength"):  # sample_vqvae.py's defaults
        assert getattr(a, name) == getattr(b, name), name
    assert (a.whole_file, a.window_seconds, a.overlap_seconds, a.window_batch, a.keep, a.strength) == (False, None, 0.4, 64, [], 1.0)
    # what the script had keeps its defaults
    assert (a.sample_rate, a.sample_steps, a.seconds, a.encoding, a.schedule, a.guide_label_scale, a.guide_vq_scale, a.no_vq, a.check_vq, a.seed,
            a.precision, a.sampler, a.eta) == (16000, 100, 4, "linear", "lambda t: t", 1.0, 0.0, False, False, None, "fp32", "ddpm", 0.0)
    a = sample_vqvae_uncond.parse_args(["--whole-file", "--window-seconds", "0.128", "--overlap-seconds", "0.032", "--window-batch", "2", "--keep", "0.1:0.2",
                                        "--keep", ":0.05", "--strength", "0.5", "--guide-label-scale", "2", "--schedule", "lambda t: t**2",
                                        "--sampler", "dpmpp"] + VQ)
    assert (a.whole_file, a.window_seconds, a.overlap_seconds, a.window_batch, a.strength, a.guide_label_scale) == (True, 0.128, 0.032, 2, 0.5, 2.0)
    assert a.keep == [(0.1, 0.2), (None, 0.05)] and a.schedule == "lambda t: t**2" and a.sampler == "dpmpp"
    for bad in (["--strength", "0"], ["--strength", "1.5"], ["--keep", "2:1"], ["--keep", "x"], ["--window-batch", "0"], ["--whole-file", "--no-vq"]):
        with pytest.raises(SystemExit):
            sample_vqvae_uncond.parse_args(bad + VQ)


def test_convert_dataset_guidance_flags():
    import convert_dataset

    base = ["m.pt", "data", "out", "--label", "7"]
    a = convert_dataset.parse_args(base)
    assert (a.guide_label_scale, a.guide_vq_scale) == (0.0, 0.0) and not convert_dataset.guided(a)
    # with the flags absent the unguided parser's namespace is what the run is made of: every other default as it was
    plain = convert_dataset.arg_parser().parse_args(base)
    assert {k: v for k, v in vars(a).items() if not k.startswith("guide_")} == vars(plain) and not convert_dataset.guided(plain)
    a = convert_dataset.parse_args(base + ["--guide-label-scale", "2"])
    assert (a.guide_label_scale, a.guide_vq_scale, a.label) == (2.0, 0.0, 7) and convert_dataset.guided(a)
    a = convert_dataset.parse_args(["m.pt", "data", "out", "--label-map", "t.tsv", "--guide-vq-scale", "-0.5"])
    assert (a.guide_label_scale, a.guide_vq_scale) == (0.0, -0.5) and convert_dataset.guided(a)
    with pytest.raises(SystemExit):
        convert_dataset.parse_args(base + ["--guide-label-scale", "much"])


def test_eval_conversion_guidance_flags():
    import eval_conversion

    a = eval_conversion.parse_args(["vqvae.pt", "tones"])
    assert (a.guide_label_scale, a.guide_vq_scale) == (0.0, 0.0) and not eval_conversion.guided(a)
    assert (a.sampler, a.eta, a.sample_steps, a.target, a.reference_steps, a.reference_sampler, a.classifier, a.pitch) == \
        ("ddpm", 0.0, 100, "other", None, "ddpm", None, False)
    a = eval_conversion.parse_args(["vqvae.pt", "tones", "--guide-label-scale", "2", "--guide-vq-scale", "0.5", "--target", "1"])
    assert (a.guide_label_scale, a.guide_vq_scale, a.target) == (2.0, 0.5, 1) and eval_conversion.guided(a)


def test_enroll_speaker_uncond_flag():
    import enroll_speaker

    base = ["speakers", "--pretrained-path", "model.pt"]
    a = enroll_speaker.parse_args(base)
    assert (a.uncond, a.output_dir, a.init, a.lr, a.save_interval, a.holdout) == (False, "ckpt_vqvae_added", "normal", 1e-4, 1000, 0)
    a = enroll_speaker.parse_args(base + ["--uncond"])
    assert (a.uncond, a.output_dir, a.init) == (True, "ckpt_vqvae_uncond", "normal")  # the directory moves, --init's default stays
    a = enroll_speaker.parse_args(base + ["--uncond", "--output-dir", "mine", "--init", "mean", "--holdout", "3", "--save-interval", "7"])
    assert (a.uncond, a.output_dir, a.init, a.holdout, a.save_interval) == (True, "mine", "mean", 3, 7)
    assert enroll_speaker.parse_args(base + ["--uncond", "--output-dir", "ckpt_vqvae_added"]).output_dir == "ckpt_vqvae_added"  # given is given
    assert enroll_speaker.parse_args(base + ["--output-dir", "x"]).output_dir == "x"


# ---------------------------------------------------------------- NullLabelEnroller on a CPU model
def cpu_model(num_labels=3):
    m = DiffusionModel("unet", 32, num_labels=num_labels)
    det_init_(("uncond.cpu." + k, v) for k, v in m.state_dict().items())
    return m.eval()


def test_checkpoint_puts_the_row_in_front(lib_built):
    model = cpu_model()
    old = model.predictor.class_embed.weight.detach().clone()
    en = NullLabelEnroller(model, init="mean", seed=3)
    assert en.num_new == 1 and en.front and tuple(en.rows.shape) == (1, old.shape[1])
    assert torch.equal(en.rows[0], old.double().mean(dim=0).float())
    en.rows += 0.25  # (a learned row)
    ck = en.checkpoint()
    w = ck["state_dict"]["predictor.class_embed.weight"]
    assert ck["kwargs"]["num_labels"] == 4 and tuple(w.shape) == (4, old.shape[1])
    assert torch.equal(w[1:], old) and torch.equal(w[0], en.rows[0])
    assert model.num_labels == 3 and torch.equal(model.predictor.class_embed.weight, old)  # the model is untouched until finish()
    for k, v in model.state_dict().items():
        if k != "predictor.class_embed.weight":
            assert torch.equal(ck["state_dict"][k], v), k
    loaded = DiffusionModel.load_dict(ck)
    assert loaded.num_labels == 4 and torch.equal(loaded.predictor.class_embed.weight.detach(), w)
    finished = en.finish()
    w = finished.predictor.class_embed.weight.detach()
    assert finished is model and model.num_labels == model.predictor.num_labels == 4
    assert torch.equal(w[1:], old) and torch.equal(w[0], en.rows[0])
    done = en.checkpoint()  # after finish(): the model's own save_dict
    assert torch.equal(done["state_dict"]["predictor.class_embed.weight"], w) and done["kwargs"]["num_labels"] == 4
    with pytest.raises(RuntimeError):
        en.finish()


def test_checkpoint_loads_as_a_vqvae(tmp_path, lib_built):
    model = VQVAE(base_channels=32, pred_name="unet", num_labels=3)
    det_init_(("uncond.vq." + k, v) for k, v in model.state_dict().items())
    model.eval()
    old = model.predictor.class_embed.weight.detach().clone()
    en = NullLabelEnroller(model, init=1)
    assert torch.equal(en.rows[0], old[1])
    path = str(tmp_path / "model.pt")
    torch.save(en.checkpoint(), path)
    grown = VQVAE.load(path)
    w = grown.predictor.class_embed.weight.detach()
    assert grown.num_labels == grown.predictor.num_labels == 4 and torch.equal(w[1:], old) and torch.equal(w[0], old[1])


def test_a_resume_of_the_other_kind_is_refused(lib_built):
    front, back = NullLabelEnroller(cpu_model(), init="mean"), SpeakerEnroller(cpu_model(), 1, init="mean")
    fs, bs = front.state_dict(), back.state_dict()
    assert fs["front"] is True and "front" not in bs  # the marker; a back state is the dict it always was
    assert sorted(bs) == ["exp_avg", "exp_avg_sq", "first_label", "rows", "steps"]
    assert tuple(fs["rows"].shape) == tuple(bs["rows"].shape)  # only the marker tells them apart
    with pytest.raises(ValueError, match="null label"):
        back.load_state_dict(fs)
    with pytest.raises(ValueError, match="new speakers"):
        front.load_state_dict(bs)
    fs["steps"], fs["rows"] = 5, fs["rows"] + 1.0
    again = NullLabelEnroller(cpu_model(), init="normal")
    again.load_state_dict(fs)
    assert again.steps == 5 and torch.equal(again.rows.cpu(), fs["rows"])
    with pytest.raises(ValueError):
        NullLabelEnroller(cpu_model(num_labels=4)).load_state_dict(fs)  # made for a model of 3 speakers
    with pytest.raises(ValueError):
        NullLabelEnroller(DiffusionModel("unet", 32).eval())  # not class-conditional
