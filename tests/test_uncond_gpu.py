"""Label guidance end to end on the device.

  * `vqvs_guidance_mix` against the tensor expressions it replaces, `torch.equal`: misaligned blocks, tails, in place, more than one
    workgroup, the grid-stride loops, magnitudes from 1e-30 to 1e30 (a contracted multiply-add would round differently);
  * the clip path: both scales 0 is `decode(codes, labels + 1)`, kept samples are the source's, bit for bit;
  * whole files: one window is the clip path; several windows with per-window labels and a ragged last slice are
    `Diffusion.<sampler>_sample_windows` driven by a guided predictor written here in tensor expressions; `window_batch` is immaterial;
  * packs: recording r is the recording alone at clip_offset + r;
  * the null label: the front row's per-clip gradient and a three-step trajectory against the float64 reference of tests/enroll_ref.py
    under its own gates (`GATES["grad"]` = 2e-4, `GATES["traj"]` = 5e-4: it is the same kernel), the loss on a fixed batch over twenty
    steps, the layout after `finish()` and through `checkpoint()` / `VQVAE.load`, the resume refusals;
  * the four scripts in a row on a tiny checkpoint.

Everything but the two float64 comparisons is bit for bit.  Their errors are printed and recorded (profiles/uncond_margins.jsonl is
one GPU run of this file) before they are held to the gates."""
import os
import sys

import numpy as np
import pytest
import torch

import enroll_ref as R
from util import record_margin, run_script, sample_lines, seeded
from vq_voice_swap_amd import VQVAE, DiffusionModel, _native
from vq_voice_swap_amd.audio import ChunkReader, ChunkWriter
from vq_voice_swap_amd.det_init import det_init_
from vq_voice_swap_amd.diffusion import guidance_mix, randn_clips
from vq_voice_swap_amd.enroll import NullLabelEnroller, SpeakerEnroller
from vq_voice_swap_amd.longform import plan_pack, plan_windows

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MARGINS = "uncond_margins.jsonl"


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    torch.set_num_threads(8)
    return torch.device("cuda:0")


# ---------------------------------------------------------------- 1. the mix kernel
SCALES = [(0.0, 7.5), (-0.3, 0.0), (7.5, -1.25), (1.5, 0.7)]


def expressions(outs, n, reps, s1, s2):
    """What `VQVAE.decode_uncond_guidance` computed before the kernel: one tensor expression per guidance term, Python-float scales."""
    base = outs[:n]
    pred = base
    for k, scale in zip(range(1, reps), (s1, s2)):
        pred = pred + scale * (base - outs[k * n:(k + 1) * n])
    return pred


def mix_inputs(reps, rows, row_len, seed, dev, offset=0):
    """[reps * rows, row_len] float32 whose elements are N(0, 1) times 1e-30, 1 or 1e30, one magnitude per element and the same for the
    reps blocks' copies of it or not, as chance has it; `offset` floats into a larger buffer (a base that is not 16-byte aligned)."""
    g = torch.Generator().manual_seed(seed)
    size = reps * rows * row_len
    vals = torch.randn(size, generator=g) * torch.tensor([1e-30, 1.0, 1e30])[torch.randint(0, 3, (size,), generator=g)]
    buf = torch.zeros(size + offset + 8)
    buf[offset:offset + size] = vals
    buf = buf.to(dev)
    return buf, buf[offset:offset + size].view(reps * rows, row_len)


def raw_mix(outs, eps, rows, row_len, reps, s1, s2):
    with torch.cuda.device(outs.device):
        return _native.lib().vqvs_guidance_mix(outs.data_ptr(), eps.data_ptr(), rows, row_len, reps, s1, s2, _native._stream_ptr())


def check_mix(rows, row_len, reps, s1, s2, dev, seed, offset=0):
    buf, outs = mix_inputs(reps, rows, row_len, seed, dev, offset)
    before = buf.clone()
    want = expressions(outs, rows, reps, s1, s2)
    assert bool(torch.isfinite(want).all())
    # out of place, into a guarded buffer
    total = rows * row_len
    guard = torch.full((total + 64,), float("nan"), device=dev)
    _native.check(raw_mix(outs, guard, rows, row_len, reps, s1, s2))
    assert torch.isnan(guard[total:]).all(), "the kernel wrote past the end of eps"
    assert torch.equal(guard[:total].view(rows, row_len), want), (rows, row_len, reps, s1, s2, offset, "out of place")
    assert torch.equal(buf, before), "an out-of-place call changed its input"
    # in place over block 0: the other blocks, and everything around the batch, stay
    _native.check(raw_mix(outs, outs, rows, row_len, reps, s1, s2))
    assert torch.equal(outs[:rows], want), (rows, row_len, reps, s1, s2, offset, "in place")
    assert torch.equal(outs[rows:], before[offset + total:offset + reps * total].view(-1, row_len))
    assert torch.equal(buf[:offset], before[:offset]) and torch.equal(buf[offset + reps * total:], before[offset + reps * total:])


@pytest.mark.parametrize("row_len", [1, 7, 1023, 4100, 4101])
@pytest.mark.parametrize("rows", [1, 3])
def test_mix_is_the_tensor_expressions(dev, rows, row_len):
    """Odd rows * row_len puts blocks 1 and 2 off the 16-byte grid (one float per access); 3 x 1023 and 4100 are aligned with a
    3-float tail (reps 1) or none; 3 x 4100 / 4 quads and 3 x 4101 floats are more than one workgroup."""
    for reps in (1, 2, 3):
        for i, (s1, s2) in enumerate(SCALES if reps > 1 else SCALES[:1]):
            check_mix(rows, row_len, reps, s1, s2, dev, seed=1000 * rows + row_len + 17 * reps + i)
    check_mix(rows, row_len, 3, 7.5, -0.3, dev, seed=5, offset=1)  # the batch itself 4 bytes off the 16-byte grid
    check_mix(rows, row_len, 1, 0.0, 0.0, dev, seed=6, offset=3)


@pytest.mark.parametrize("rows,row_len", [(4, 600000), (3, 700001)], ids=["quads", "floats"])
def test_mix_grid_stride(dev, rows, row_len):
    """More quads (600000) and more floats (2100003) than the capped grid has threads (2048 x 256): the grid-stride loops."""
    check_mix(rows, row_len, 3, 1.5, -7.5, dev, seed=rows)


def test_mix_refusals_and_wrapper(dev):
    buf, outs = mix_inputs(3, 2, 8, 1, dev)
    eps = torch.empty(2, 8, device=dev)
    for bad in (dict(reps=0), dict(reps=4), dict(rows=0), dict(row_len=0), dict(eps=outs[2:]), dict(eps=outs[4:]), dict(eps=outs[1:])):
        a = dict(dict(eps=eps, rows=2, row_len=8, reps=3), **bad)
        rc = raw_mix(outs, a["eps"], a["rows"], a["row_len"], a["reps"], 1.0, 1.0)
        assert rc == -1, bad
        with pytest.raises(_native.NativeArgumentError):
            _native.check(rc)
    want = expressions(outs, 2, 3, 1.5, 0.7)
    assert torch.equal(guidance_mix(outs, 3, 1.5, 0.7, out=eps), want) and eps.data_ptr() != outs.data_ptr()
    got = guidance_mix(outs.view(6, 1, 8), 3, 1.5, 0.7)  # no `out`: in place over block 0, returned as a view of it
    assert got.data_ptr() == outs.data_ptr() and tuple(got.shape) == (2, 1, 8) and torch.equal(got.view(2, 8), want)
    for bad_outs, reps in ((outs[:5], 3), (outs[:0], 1)):
        with pytest.raises(ValueError):
            guidance_mix(bad_outs, reps)
    with pytest.raises(_native.NativeError):
        guidance_mix(outs.cpu(), 3)


# ---------------------------------------------------------------- 2. the models
def det_model(m, prefix=""):
    det_init_((prefix + k, v) for k, v in m.state_dict().items())
    m.eval()
    return m


K = 3  # speakers; the guided model has the null label in front of them
W, H, STEPS = 2048, 1536, 3


@pytest.fixture(scope="module")
def vqvae(dev):
    """A model with the null label at 0: K + 1 labels."""
    model = det_model(VQVAE(base_channels=32, pred_name="unet", num_labels=K + 1)).to(dev)
    model.set_precision("fp32")
    return model


def ref_guided_predictor(model, cond_seq, labels, label_scale, vq_scale):
    """The guided window predictor in tensor expressions: the slice's windows as [own cond, labels + 1 | zero cond, labels + 1 | own
    cond, label 0], a block only for a non-zero scale, mixed as `decode_uncond_guidance` always has."""
    def predictor(xs, ts, first):
        n = xs.shape[0]
        cond, lab = cond_seq[first:first + n], labels[first:first + n] + 1
        conds, labs = [cond], [lab]
        if vq_scale:
            conds.append(torch.zeros_like(cond))
            labs.append(lab)
        if label_scale:
            conds.append(cond)
            labs.append(torch.zeros_like(lab))
        reps = len(conds)
        outs = model.predictor(torch.cat([xs] * reps), torch.cat([ts] * reps), cond=torch.cat(conds), labels=torch.cat(labs))
        scales = [s for s in (vq_scale, label_scale) if s] + [0.0, 0.0]
        return expressions(outs, n, reps, scales[0], scales[1])

    return predictor


# ---------------------------------------------------------------- 3. the clip path
@pytest.fixture(scope="module")
def clip(vqvae, dev):
    wave = (0.3 * seeded((2, 1, W), 31)).clamp(-1, 1).to(dev)
    return wave, vqvae.encode(wave), torch.tensor([2, 0], device=dev)


@pytest.mark.parametrize("sampler", ["ddpm", "ddim", "dpmpp"])
def test_scales_zero_is_decode_one_label_up(vqvae, clip, sampler):
    _, codes, labels = clip
    kw = dict(steps=STEPS, constrain=True, seed=9, clip_offset=4, sampler=sampler)
    got = vqvae.decode_uncond_guidance(codes, labels, label_scale=0.0, vq_scale=0.0, **kw)
    assert torch.equal(got, vqvae.decode(codes, labels + 1, **kw))
    guided = vqvae.decode_uncond_guidance(codes, labels, label_scale=2.0, **kw)
    assert not torch.equal(guided, got) and bool(torch.isfinite(guided).all())


def test_clip_path_is_the_tensor_expressions(vqvae, clip):
    """`decode_uncond_guidance` on the kernel against `ddpm_sample` driven by the predictor in tensor expressions: the move changed no bit."""
    _, codes, labels = clip
    cond = vqvae.cond_sequence(codes)
    for label_scale, vq_scale in ((2.0, 0.0), (0.0, 1.5), (0.7, 1.5)):
        ref = ref_guided_predictor(vqvae, cond, labels, label_scale, vq_scale)
        x_T = randn_clips(2, W, codes.device, 9, 4)
        want = vqvae.diffusion.ddpm_sample(x_T, lambda xs, ts: ref(xs, ts, 0), STEPS, constrain=True, seed=9, clip_offset=4)
        got = vqvae.decode_uncond_guidance(codes, labels, steps=STEPS, constrain=True, seed=9, clip_offset=4, label_scale=label_scale, vq_scale=vq_scale)
        assert torch.equal(got, want), (label_scale, vq_scale)


def test_kept_samples_are_the_source(vqvae, clip, dev):
    wave, codes, labels = clip
    keep = torch.zeros(2, 1, W, dtype=torch.bool, device=dev)
    keep[0, 0, 300:900] = True
    keep[1, 0, :128] = True
    keep[1, 0, 2000:] = True
    kw = dict(steps=STEPS, constrain=True, seed=9, label_scale=2.0, vq_scale=0.5)
    for sampler, strength in (("ddpm", 1.0), ("ddim", 1.0), ("dpmpp", 0.6)):
        got = vqvae.decode_uncond_guidance(codes, labels, source=wave, keep=keep, strength=strength, sampler=sampler, **kw)
        assert torch.equal(got[keep], wave[keep]), (sampler, strength)
        assert (got[~keep] != wave[~keep]).float().mean() > 0.9
    plain = vqvae.decode_uncond_guidance(codes, labels, **kw)
    part = vqvae.decode_uncond_guidance(codes, labels, source=wave, strength=0.6, **kw)  # starts at source_start_step, from the noised source
    assert not torch.equal(part, plain)
    with pytest.raises(ValueError):
        vqvae.decode_uncond_guidance(codes, labels, keep=keep, **kw)  # keep= needs source=
    with pytest.raises(ValueError):
        vqvae.decode_uncond_guidance(codes, labels, strength=0.5, **kw)


def test_two_byte_modes_are_promoted(vqvae, clip):
    """The clip path's rule on the long paths: a guided call in a 2-byte mode runs in fp32 (with the warning) and gives the fp32 bits."""
    _, codes, labels = clip
    kw = dict(num_samples=W, window=W, hop=H, steps=STEPS, constrain=True, seed=9, label_scale=2.0)
    want = vqvae.decode_long_uncond_guidance(codes[:1], labels[:1], **kw)
    vqvae.set_precision("fp16")
    try:
        with pytest.warns(UserWarning, match="fp32 mode"):
            got = vqvae.decode_long_uncond_guidance(codes[:1], labels[:1], **kw)
        assert vqvae.predictor.precision == "fp16" and torch.equal(got, want)
    finally:
        vqvae.set_precision("fp32")


# ---------------------------------------------------------------- 4. whole files
LENGTHS = (1500, 3000, 5000)  # 1, 2 and 3 windows of 2048 every 1536


@pytest.fixture(scope="module")
def waves(dev):
    return [(0.3 * seeded((1, 1, n), 71 + i)).clamp(-1, 1).to(dev) for i, n in enumerate(LENGTHS)]


@pytest.fixture(scope="module")
def codes(vqvae, waves):
    assert plan_pack(LENGTHS, W, H)[0] == [1, 2, 3]
    return [vqvae.encode_long(w, W, H) for w in waves]


@pytest.mark.parametrize("sampler", ["ddpm", "ddim", "dpmpp"])
def test_one_window_is_the_clip_path(vqvae, clip, sampler):
    _, codes, labels = clip
    kw = dict(steps=STEPS, constrain=True, seed=9, clip_offset=6, label_scale=2.0, vq_scale=0.5, sampler=sampler)
    want = vqvae.decode_uncond_guidance(codes[:1], labels[:1], **kw)
    got = vqvae.decode_long_uncond_guidance(codes[:1], labels[:1], num_samples=W, window=W, hop=H, **kw)
    assert tuple(got.shape) == (1, 1, W) and torch.equal(got, want[:1])


@pytest.mark.parametrize("sampler,eta", [("ddpm", 0.0), ("ddim", 0.5), ("dpmpp", 0.0)])
def test_windows_are_the_loop_with_the_expression_predictor(vqvae, codes, dev, sampler, eta):
    """Three windows, a label per window, window_batch 2 (slices of 2 and 1)."""
    n, padded = plan_windows(LENGTHS[2], W, H)
    assert n == 3
    labels = torch.tensor([2, 0, 1], device=dev)
    cond = vqvae.cond_sequence(codes[2])
    loop = getattr(vqvae.diffusion, sampler + "_sample_windows")
    extra = dict(eta=eta) if sampler == "ddim" else {}
    for label_scale, vq_scale in ((2.0, 0.0), (0.7, 1.5)):
        x_T = randn_clips(1, padded, dev, 9, 3)
        want = loop(x_T, ref_guided_predictor(vqvae, cond, labels, label_scale, vq_scale), STEPS, window=W, hop=H, window_batch=2, constrain=True,
                    seed=9, clip_offset=3, **extra)[..., :LENGTHS[2]]
        kw = dict(num_samples=LENGTHS[2], window=W, hop=H, steps=STEPS, constrain=True, seed=9, clip_offset=3, sampler=sampler, eta=eta,
                  label_scale=label_scale, vq_scale=vq_scale)
        got = vqvae.decode_long_uncond_guidance(codes[2], labels, window_batch=2, **kw)
        assert tuple(got.shape) == (1, 1, LENGTHS[2]) and torch.equal(got, want), (sampler, label_scale, vq_scale)
        for wb in (1, 64):  # the window batch is immaterial
            assert torch.equal(vqvae.decode_long_uncond_guidance(codes[2], labels, window_batch=wb, **kw), got), (sampler, wb)
    unguided = vqvae.decode_long(codes[2], labels + 1, **{k: v for k, v in kw.items() if not k.endswith("_scale")})
    assert torch.equal(vqvae.decode_long_uncond_guidance(codes[2], labels, **dict(kw, label_scale=0.0, vq_scale=0.0)), unguided)
    assert not torch.equal(got, unguided)


def test_whole_file_keeps_the_source(vqvae, codes, waves, dev):
    keep = torch.zeros(1, 1, LENGTHS[2], dtype=torch.bool, device=dev)
    keep[..., 1400:2100] = True  # across the first overlap (1536 .. 2048)
    got = vqvae.decode_long_uncond_guidance(codes[2], torch.tensor([1], device=dev), num_samples=LENGTHS[2], window=W, hop=H, steps=STEPS, constrain=True,
                                            seed=9, label_scale=2.0, source=waves[2], keep=keep, window_batch=2)
    assert torch.equal(got[keep], waves[2][keep]) and (got[~keep] != waves[2][~keep]).float().mean() > 0.9


# ---------------------------------------------------------------- 5. packs
@pytest.mark.parametrize("sampler", ["ddpm", "ddim", "dpmpp"])
def test_a_pack_is_its_recordings_alone(vqvae, codes, dev, sampler):
    counts = [1, 2, 3]
    kw = dict(window=W, hop=H, steps=STEPS, constrain=True, seed=9, sampler=sampler, label_scale=2.0, vq_scale=0.5)
    labels = [2, 0, 1]
    alone = [vqvae.decode_long_uncond_guidance(codes[r], torch.tensor([labels[r]], device=dev), num_samples=LENGTHS[r], clip_offset=5 + r, **kw)
             for r in range(3)]
    for wb in (2, 64):
        got = vqvae.decode_long_batch_uncond_guidance(torch.cat(codes), torch.tensor(labels, device=dev), counts=counts, num_samples=list(LENGTHS),
                                                      clip_offset=5, window_batch=wb, **kw)
        assert [tuple(g.shape) for g in got] == [(1, 1, n) for n in LENGTHS]
        for r in range(3):
            assert torch.equal(got[r], alone[r]), (sampler, wb, r)
    plain = vqvae.decode_long_batch(torch.cat(codes), torch.tensor(labels, device=dev) + 1, counts=counts, num_samples=list(LENGTHS), clip_offset=5,
                                    **{k: v for k, v in kw.items() if not k.endswith("_scale")})
    zero = vqvae.decode_long_batch_uncond_guidance(torch.cat(codes), torch.tensor(labels, device=dev), counts=counts, num_samples=list(LENGTHS),
                                                   clip_offset=5, **dict(kw, label_scale=0.0, vq_scale=0.0))
    assert all(torch.equal(a, b) for a, b in zip(zero, plain)) and not torch.equal(got[2], plain[2])


# ---------------------------------------------------------------- 6. the null label
def front_enroller(dev, case, lr=1e-2, init="normal"):
    """A NullLabelEnroller on a case's predictor inside a DiffusionModel (its conditioning, if any, handed in by the test)."""
    model = DiffusionModel("unet", case["base"], num_labels=case["num_labels"], cond_channels=case["cond_channels"])
    model.predictor = R.make_model(case)
    model.to(dev).eval()
    return model, NullLabelEnroller(model, lr=lr, init=init, seed=11)


def noised64(model, x0, ts, noise):
    """The x_t the enroller forms, in float64: sqrt(a) x_0 + sqrt(1 - a) eps with the model's own alpha_bar(ts)."""
    a = model.diffusion.schedule(ts).double()[:, None, None]
    return a.sqrt() * x0.double() + (1 - a).sqrt() * noise.double()


@pytest.mark.parametrize("cid", [c["id"] for c in R.CASES])
def test_front_row_gradient_against_float64(cid, dev):
    """Every clip of the batch on the one row: the per-clip gradients are those of `vqvs_unet_embed_grad` with the row as every clip's
    vector, held to float64 autograd under the gate of tests/enroll_ref.py."""
    torch.set_num_threads(8)
    case = R.CASE[cid]
    model, en = front_enroller(dev, case)
    x0, ts, noise, cond, _ = R.inputs(case)
    if cond is not None:
        en._cond = lambda inputs: cond.to(dev)
    mses, grads, _, rows = en.losses(x0.to(dev), ts=ts, noise=noise.to(dev))
    assert rows.tolist() == [0] * case["B"] and tuple(grads.shape) == (case["B"], en.rows.shape[1])
    zeros = torch.zeros(case["B"], dtype=torch.int64)
    ref = R.reference(case, R.make_model(case), table=en.rows.cpu(), labels=zeros, data=(noised64(model, x0, ts, noise), ts, noise, cond, zeros))
    got, want = grads.cpu(), ref["grads"]
    clip = R.clip_rel_rms(got, want)
    rec = dict(test="uncond.grad", case=cid, grad_err=R.rel_rms(got, want), grad_err_worst_clip=clip.max().item(), worst_clip=int(clip.argmax()),
               mse_err=R.rel_rms(mses.cpu(), ref["mses"]))
    record_margin(MARGINS, rec)
    assert bool(torch.isfinite(got).all()) and rec["grad_err"] < R.GATES["grad"] and rec["grad_err_worst_clip"] < R.GATES["grad"], rec
    assert rec["mse_err"] < 1e-3, rec


def test_three_null_label_steps_against_float64(dev):
    torch.set_num_threads(8)
    case = R.CASE["pg_ragged"]
    model, en = front_enroller(dev, case)
    x0, ts, noise, _, _ = R.inputs(case)
    rows0 = en.rows.cpu().clone()
    zeros = torch.zeros(case["B"], dtype=torch.int64)
    want, ref_losses = R.trajectory_ref(case, rows0, zeros, 3, 1e-2, data=(noised64(model, x0, ts, noise), ts, noise, None, zeros))
    losses = [en.step(x0.to(dev), ts=ts, noise=noise.to(dev))["loss"].item() for _ in range(3)]
    got = en.rows.cpu().double()
    disp = torch.from_numpy(want[-1]) - rows0.double()
    rec = dict(test="uncond.traj", case=case["id"], steps=3, lr=1e-2, traj_err=R.rel_rms(got - rows0.double(), disp),
               loss_err=max(abs(a - b) / b for a, b in zip(losses, ref_losses)))
    record_margin(MARGINS, rec)
    assert en.steps == 3 and rec["traj_err"] < R.GATES["traj"] and rec["loss_err"] < 1e-3, rec


def test_null_label_loss_falls_over_twenty_steps(dev):
    case = R.CASE["pg_ragged"]
    model, en = front_enroller(dev, case)
    x0, ts, noise, _, _ = R.inputs(case)
    x0, noise = x0.to(dev), noise.to(dev)
    before = en.losses(x0, ts=ts, noise=noise)[0].mean().item()
    for _ in range(20):
        en.step(x0, ts=ts, noise=noise)
    after = en.losses(x0, ts=ts, noise=noise)[0].mean().item()
    print(f"[margin] null-label loss on the fixed batch: {before:.6f} -> {after:.6f} after 20 steps")
    assert after < before


def test_layout_after_finish_and_through_checkpoint(dev, tmp_path):
    original = det_model(VQVAE(base_channels=32, pred_name="unet", num_labels=K), "uncond.layout.").to(dev)
    original.set_precision("fp32")
    old = original.predictor.class_embed.weight.detach().clone()
    wave = (0.3 * seeded((2, 1, W), 41)).clamp(-1, 1).to(dev)
    codes, labels = original.encode(wave), torch.tensor([2, 0], device=dev)
    kw = dict(steps=STEPS, constrain=True, seed=9)
    want = original.decode(codes, labels, **kw)

    en = NullLabelEnroller(original, lr=1e-2, init="mean")
    for i in range(2):
        en.step(wave, seed=5, clip_offset=2 * i)
    row = en.rows.detach().clone()
    assert not torch.equal(row[0], old.double().mean(dim=0).float())  # it learned something
    path = str(tmp_path / "model.pt")
    torch.save(en.checkpoint(), path)
    assert original.num_labels == K and torch.equal(original.predictor.class_embed.weight.detach(), old)
    state = en.state_dict()
    grown = [VQVAE.load(path).to(dev).eval(), en.finish()]
    for model in grown:
        model.set_precision("fp32")
        w = model.predictor.class_embed.weight.detach()
        assert model.num_labels == model.predictor.num_labels == K + 1 and tuple(w.shape) == (K + 1, old.shape[1])
        assert torch.equal(w[1:], old) and torch.equal(w[0], row[0])
        assert torch.equal(model.decode(codes, labels + 1, **kw), want)
        assert torch.equal(model.decode_uncond_guidance(codes, labels, **kw), want)  # both scales 0
        guided = model.decode_uncond_guidance(codes, labels, label_scale=2.0, **kw)
        assert bool(torch.isfinite(guided).all()) and not torch.equal(guided, want)
    with pytest.raises(RuntimeError):
        en.step(wave)  # the row is part of the model now

    fresh = det_model(VQVAE(base_channels=32, pred_name="unet", num_labels=K), "uncond.layout.").to(dev)
    with pytest.raises(ValueError, match="null label"):
        SpeakerEnroller(fresh, 1).load_state_dict(state)
    with pytest.raises(ValueError, match="new speakers"):
        NullLabelEnroller(fresh).load_state_dict(SpeakerEnroller(fresh, 1).state_dict())
    resumed = NullLabelEnroller(fresh)
    resumed.load_state_dict(state)
    assert resumed.steps == 2 and torch.equal(resumed.rows, row)


# ---------------------------------------------------------------- 7. the scripts, one after the other
def read_bytes(path):
    with open(path, "rb") as f:
        return f.read()


def read_s16(path):
    import wave

    with wave.open(str(path), "rb") as w:
        return np.frombuffer(w.readframes(w.getnframes()), dtype="<i2")


def write_wav(path, samples):
    os.makedirs(os.path.dirname(path), exist_ok=True)
    w = ChunkWriter(str(path), 16000)
    w.write(samples.astype(np.float32))
    w.close()


WINDOW_FLAGS = ["--window-seconds", "0.128", "--overlap-seconds", "0.032", "--sample-steps", "3"]


def test_scripts_end_to_end(dev, tmp_path, capsys):
    """enroll_speaker.py --uncond -> sample_vqvae_uncond.py --whole-file --keep -> convert_dataset.py --guide-label-scale ->
    eval_conversion.py --guide-label-scale, on a det-init checkpoint of three speakers.  The first and the last run as fresh child
    processes, the two in between in this one."""
    sys.path.insert(0, ROOT)
    import convert_dataset
    import enroll_speaker
    import sample_vqvae_uncond

    model = det_model(VQVAE(base_channels=32, pred_name="unet", num_labels=K), "uncond.scripts.")
    ck = str(tmp_path / "vqvae32.pt")
    model.save(ck)
    old = model.predictor.class_embed.weight.detach().clone()

    # recordings of the known speakers; the directory names are ignored
    train = tmp_path / "known"
    for k, hz in enumerate((220.0, 330.0)):
        write_wav(str(train / f"anything{k}" / "a.wav"), 0.3 * np.sin(2 * np.pi * hz * np.arange(40000) / 16000.0))
    out_dir = tmp_path / "uncond"
    text = run_script("enroll_speaker.py", [train, "--uncond", "--pretrained-path", ck, "--output-dir", out_dir, "--steps", "3", "--batch-size", "2",
                                            "--seed", "0", "--seconds", "1.024", "--lr", "1e-2", "--init", "mean", "--holdout", "2", "--save-interval", "2"])
    steps = [ln for ln in text.splitlines() if ln.startswith("step ") and "loss=" in ln]
    assert [ln.split(":")[0] for ln in steps] == ["step 1", "step 2", "step 3"], text
    assert [ln.split(":")[0] for ln in text.splitlines() if "holdout=" in ln] == ["step 2", "step 3"], text
    assert "unconditional label" in text
    grown_path = str(out_dir / "model.pt")
    grown = VQVAE.load(grown_path)
    w = grown.predictor.class_embed.weight.detach()
    assert grown.num_labels == K + 1 and torch.equal(w[1:], old) and bool(torch.isfinite(w[0]).all())
    assert not torch.equal(w[0], old.double().mean(dim=0).float())
    for k, v in model.state_dict().items():
        if k != "predictor.class_embed.weight":
            assert torch.equal(grown.state_dict()[k], v), k
    assert torch.load(str(out_dir / "enroll.pt"), map_location="cpu")["front"] is True
    # a resume of the other kind into the same directory is refused
    with pytest.raises(SystemExit, match="null label"):
        enroll_speaker.main([str(train), "--pretrained-path", ck, "--output-dir", str(out_dir), "--steps", "1", "--batch-size", "2", "--seconds", "1.024"])

    # three short files; the first is about 2.5 windows of 2048 every 1536
    data = tmp_path / "data"
    files = (("s1/a.wav", 4800), ("s1/b.wav", 3200), ("s2/a.wav", 800))
    for i, (rel, n) in enumerate(files):
        write_wav(str(data / rel), 0.3 * np.sin(np.arange(n) * (0.05 + 0.01 * i)))
    assert plan_pack([n for _, n in files], W, H)[0] == [3, 2, 1]
    first = str(data / files[0][0])
    common = ["--label", "1", "--input-file", first, "--seed", "9", "--whole-file", "--window-batch", "2", "--guide-label-scale", "2", *WINDOW_FLAGS]
    kept, plain = str(tmp_path / "kept.wav"), str(tmp_path / "plain.wav")
    sample_vqvae_uncond.main(common + ["--keep", "0.1:0.2", grown_path, kept])
    sample_vqvae_uncond.main(common + [grown_path, plain])
    r = ChunkReader(first, 16000)
    echo = str(tmp_path / "echo.wav")
    write_wav(echo, r.read(4800))  # the input on the writer's s16 grid
    r.close()
    source, a, b = read_s16(echo), 1600, 3200
    got = read_s16(kept)
    assert got.shape == source.shape == (4800,) and np.array_equal(got[a:b], source[a:b])
    assert np.concatenate([got[:a] != source[:a], got[b:] != source[b:]]).mean() > 0.5
    assert not np.array_equal(read_s16(plain)[a:b], source[a:b])

    # the corpus run writes, for the file with id 0, what the single-file script wrote
    conv = tmp_path / "converted"
    totals = convert_dataset.main([grown_path, str(data), str(conv), "--seed", "9", "--label", "1", "--guide-label-scale", "2", "--pack-windows", "4",
                                   "--window-batch", "2", *WINDOW_FLAGS])
    assert [int(t) for t in totals][:4] == [3, 0, sum(n for _, n in files), 6]
    assert read_bytes(conv / files[0][0]) == read_bytes(plain)
    unguided = tmp_path / "unguided"
    convert_dataset.main([grown_path, str(data), str(unguided), "--seed", "9", "--label", "2", *WINDOW_FLAGS])  # label 2 = speaker 1, no guidance
    assert read_bytes(unguided / files[0][0]) != read_bytes(plain)
    with pytest.raises(SystemExit, match="outside"):
        convert_dataset.main([grown_path, str(data), str(conv), "--label", "3", "--guide-label-scale", "2", *WINDOW_FLAGS])  # speakers are 0..2
    capsys.readouterr()

    lines = sample_lines(run_script("eval_conversion.py", [grown_path, "tones", "--batch-size", "2", "--seed", "1", "--max-samples", "2",
                                                           "--sample-steps", "2", "--guide-label-scale", "2"]))
    assert len(lines) == 1 and lines[0].startswith("2 samples: code_match=") and " mcd=" in lines[0] and " lsd=" in lines[0], lines
