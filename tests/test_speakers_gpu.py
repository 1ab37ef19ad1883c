"""Speaker vectors as inputs, on the device.  Everything here is bit for bit:

  * `vqvs_speaker_mix` against the numpy float32 restatement of tests/speakers_ref.py: both access paths, every slot pattern, table
    elements from 1e-30 to 1e30, a guarded output buffer, the clamp, the refusals;
  * `UNetPredictor.forward(vectors=)` against the labels call it must equal when the vectors are the table's rows (three precision
    modes, with and without cond, a padded width, a small topology at a ragged length) and against `embedding_grad`'s prediction;
  * the samplers and layouts: `decode`, `invert`, `decode_long`, `decode_long_batch` and the three uncond-guidance variants with
    vectors against the labels runs;
  * the scripts on a tiny checkpoint: a voice fitted to a recording, a morph, an anonymised corpus."""
import copy
import os
import sys

import numpy as np
import pytest
import torch

import speakers_ref as SR
from util import run_script, seeded
from vq_voice_swap_amd import VQVAE, DiffusionModel, UNetPredictor, _native
from vq_voice_swap_amd import speakers as S
from vq_voice_swap_amd.audio import ChunkReader, ChunkWriter
from vq_voice_swap_amd.det_init import det_init_
from vq_voice_swap_amd.enroll import SpeakerEnroller
from vq_voice_swap_amd.longform import plan_pack, plan_windows

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H, STEPS = 2048, 1536, 3
SAMPLERS = ["ddpm", "ddim", "dpmpp"]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    torch.set_num_threads(8)
    return torch.device("cuda:0")


def det_model(m, prefix=""):
    det_init_((prefix + k, v) for k, v in m.state_dict().items())
    m.eval()
    return m


def bits(t):
    return t.contiguous().view(torch.int32)


# ---------------------------------------------------------------- 1. the mix kernel
def raw_mix(table, idx, w, out, B=None, K=None, E=None, J=None):
    with torch.cuda.device(table.device):
        return _native.lib().vqvs_speaker_mix(table.data_ptr(), table.shape[0] if K is None else K, table.shape[1] if E is None else E, idx.data_ptr(),
                                              w.data_ptr(), idx.shape[1] if J is None else J, out.data_ptr(), idx.shape[0] if B is None else B,
                                              _native._stream_ptr())


def on_device(table, idx, w, dev, offset=0):
    """The case's arrays on the device; the table `offset` floats into a larger buffer (a base that is not 16-byte aligned)."""
    K, E = table.shape
    buf = torch.zeros(K * E + offset + 8)
    buf[offset:offset + K * E] = torch.from_numpy(table).reshape(-1)
    buf = buf.to(dev)
    return buf[offset:offset + K * E].view(K, E), torch.from_numpy(idx).to(dev), torch.from_numpy(w).to(dev)


def check_case(K, E, B, J, dev, seed, unused="some", offset=0):
    table, idx, w = SR.mix_case(K, E, B, J, seed, unused)
    want = SR.mix_ref(table, idx, w)
    assert np.isfinite(want).all()
    t, i, ww = on_device(table, idx, w, dev, offset)
    assert (t.data_ptr() % 16 == 0) == (offset % 4 == 0)
    guard = torch.full((B * E + 64 + offset,), float("nan"), device=dev)
    out = guard[offset:offset + B * E].view(B, E)  # (with the table off the 16-byte grid the output is too)
    _native.check(raw_mix(t, i, ww, out))
    assert torch.isnan(guard[:offset]).all() and torch.isnan(guard[offset + B * E:]).all(), "the kernel wrote outside its output"
    assert np.array_equal(bits(out).cpu().numpy(), want.view(np.int32)), (K, E, B, J, unused, offset)
    assert torch.equal(bits(t).cpu(), torch.from_numpy(table.view(np.int32))), "the call changed its table"
    got = S.speaker_mix(t, i, ww)  # the binding: the same bits into a buffer of its own
    assert torch.equal(bits(got), bits(out))


@pytest.mark.parametrize("E", [128, 384, 1024, 6])
def test_mix_is_the_float32_restatement(dev, E):
    """E % 4 == 0 on aligned pointers takes 16-byte accesses; E = 6, and any E through a view one float off the grid, one float at a
    time (E = 6: a last quad of two floats).  E = 1024 is exactly one workgroup of quads."""
    seed = 0
    for K in (1, 4, 251):
        for B in (1, 5, 70):
            for J in (1, 2, 16):
                seed += 1
                check_case(K, E, B, J, dev, 100 * E + seed, "some" if J > 1 else "none")
    for J in (1, 2, 16):
        check_case(4, E, 5, J, dev, 7 * E + J, "all")   # a row without a used slot: zeros
        check_case(4, E, 5, J, dev, 9 * E + J, "none")
        check_case(4, E, 5, J, dev, 11 * E + J, "some", offset=1)  # the misaligned view
        check_case(251, E, 70, J, dev, 13 * E + J, "some", offset=3)


@pytest.mark.parametrize("K,E,B,J", [(4, 1028, 3, 2), (4, 1030, 3, 2), (3, 8, 1030, 3), (3, 5, 1030, 3)],
                         ids=["two-workgroups-quads", "two-workgroups-floats", "stride-over-B-quads", "stride-over-B-floats"])
def test_mix_more_than_one_workgroup_and_the_stride_over_rows(dev, K, E, B, J):
    """E past 1024: a second workgroup of quads whose threads mostly lie past the row's end; B past the grid's 1024 rows: the stride."""
    check_case(K, E, B, J, dev, K + E + B)


def test_mix_every_position_unused_and_the_copy(dev):
    K, E, J = 4, 128, 4
    table, _, _ = SR.mix_case(K, E, 1, J, 5, "none")
    idx = np.array([[0, 1, 2, 3]] + [[-1 if j == u else j for j in range(J)] for u in range(J)] + [[-1, -1, 2, -1], [-1] * J], dtype=np.int32)
    w = np.random.RandomState(2).randn(len(idx), J).astype(np.float32)
    t, i, ww = on_device(table, idx, w, dev)
    got = S.speaker_mix(t, i, ww)
    assert np.array_equal(bits(got).cpu().numpy(), SR.mix_ref(table, idx, w).view(np.int32))
    assert not got[-1].any()
    # J = 1, w = 1: the rows themselves, bit for bit (signed zeros included)
    table[1, :4] = [-0.0, 0.0, -1e-30, 1e30]
    rows = np.array([[3], [1], [1], [0]], dtype=np.int32)
    t, i, ww = on_device(table, rows, np.ones((4, 1), dtype=np.float32), dev)
    assert torch.equal(bits(S.speaker_mix(t, i, ww)), bits(t[[3, 1, 1, 0]]))
    # ... and through one used slot among unused ones
    t, i, ww = on_device(table, np.array([[-1, 1, -1]], dtype=np.int32), np.array([[9.0, 1.0, 9.0]], dtype=np.float32), dev)
    assert torch.equal(bits(S.speaker_mix(t, i, ww)), bits(t[1:2]))


def test_mix_refusals_clamp_and_binding(dev):
    table, idx, w = SR.mix_case(4, 16, 3, 2, 1, "none")
    t, i, ww = on_device(table, idx, w, dev)
    out = torch.empty(3, 16, device=dev)
    for bad in (dict(K=0), dict(E=0), dict(B=0), dict(J=0), dict(J=17), dict(out=t), dict(out=t.view(-1)[60:]), dict(out=ww), dict(out=i)):
        a = dict(dict(out=out), **bad)
        rc = raw_mix(t, i, ww, a.pop("out"), **a)
        assert rc == -1, bad
        with pytest.raises(_native.NativeArgumentError):
            _native.check(rc)
    # an index past the table: the binding raises, the kernel itself reads the last row
    high = idx.copy()
    high[1, 0] = 4
    high[2, 1] = 1000
    hi = torch.from_numpy(high).to(dev)
    with pytest.raises(IndexError):
        S.speaker_mix(t, hi, ww)
    _native.check(raw_mix(t, hi, ww, out))
    assert np.array_equal(bits(out).cpu().numpy(), SR.mix_ref(table, high, w).view(np.int32))
    for bad_args in ((t, i.long(), ww), (t.double(), i, ww), (t, i, ww[:2]), (t[0], i, ww)):
        with pytest.raises(ValueError):
            S.speaker_mix(*bad_args)
    with pytest.raises(ValueError):
        S.speaker_mix(t, i, ww, out=torch.empty(3, 8, device=dev))
    with pytest.raises(_native.NativeError):
        S.speaker_mix(t.cpu(), i.cpu(), ww.cpu())
    assert torch.equal(S.speaker_mix(t, i, ww, out=out), S.speaker_mix(t, i, ww))


# ---------------------------------------------------------------- 2. the forward
LABELS = (1, 3, 1)  # B = 3, a repeated label


def forward_inputs(B, T, dev, cond_shape=None, seed=11):
    x = seeded((B, 1, T), seed).to(dev)
    ts = torch.tensor([0.15, 0.5, 0.85][:B], device=dev)
    cond = None if cond_shape is None else seeded((B,) + cond_shape, seed + 1).to(dev)
    return x, ts, cond


def predictor_of(kind, dev):
    if kind == "cond":  # the decoder of a VQ-VAE: conditioning sequence and labels
        return det_model(VQVAE(base_channels=32, pred_name="unet", num_labels=4), "spk.fwd.").to(dev).predictor, 2048, (512, 8)
    if kind == "nocond":
        return det_model(DiffusionModel("unet", 32, num_labels=4), "spk.fwd.").to(dev).predictor, 2048, None
    if kind == "base24":  # a padded width: 24 -> 32 channels, the vector's entries placed as class_embed's columns are
        return det_model(UNetPredictor(24, num_labels=4), "spk.fwd24.").to(dev), 2048, None
    assert kind == "small"  # a (1, 2, 2) topology at a length that is no multiple of a tile
    return det_model(UNetPredictor(32, num_labels=4, channel_mult=(1, 2, 2), depth_mult=1, middle_dilations=(4,)), "spk.fwds.").to(dev), 592, None


@pytest.mark.parametrize("kind", ["cond", "nocond", "base24", "small"])
def test_forward_with_the_tables_rows_is_the_labels_call(dev, kind):
    pred, T, cond_shape = predictor_of(kind, dev)
    x, ts, cond = forward_inputs(3, T, dev, cond_shape)
    labels = torch.tensor(LABELS, device=dev)
    rows = pred.class_embed.weight.detach()[labels]
    for precision in ("fp32", "fp16", "bf16"):
        pred.set_precision(precision)
        want = pred(x, ts, cond=cond, labels=labels)
        got = pred(x, ts, cond=cond, vectors=rows)
        assert bool(torch.isfinite(want).all()) and torch.equal(got, want), (kind, precision)
        other = pred(x, ts, cond=cond, vectors=rows[[1, 1, 2]])  # the vector does matter: clip 0 under clip 1's row
        assert not torch.equal(other[0], want[0]) and torch.equal(other[1], want[1])
        with pred.precision_override("fp32"):  # the promotion of the guided calls carries it
            assert torch.equal(pred(x, ts, cond=cond, vectors=rows), pred(x, ts, cond=cond, labels=labels)), (kind, precision)
    pred.set_precision("fp32")
    if kind != "base24":  # (the gradient handle is not built for padded widths)
        eps = seeded(tuple(x.shape), 5).to(dev)
        _, _, p = pred.embedding_grad(x, ts, eps, rows, cond=cond, return_pred=True)
        assert torch.equal(pred(x, ts, cond=cond, vectors=rows), p), kind


def test_forward_blend_is_the_labels_call_on_a_patched_table(dev):
    pred, T, _ = predictor_of("nocond", dev)
    x, ts, _ = forward_inputs(3, T, dev)
    blend = S.voice_vectors(pred, ["0:0.7,2:0.3"])
    w = pred.class_embed.weight.detach()
    assert np.array_equal(bits(blend).cpu().numpy(), SR.mix_ref(w.cpu().numpy(), np.array([[0, 2]]), np.array([[0.7, 0.3]], dtype=np.float32)).view(np.int32))
    patched = copy.deepcopy(pred)
    with torch.no_grad():
        patched.class_embed.weight[3].copy_(blend[0])
    labels = torch.tensor(LABELS, device=dev)
    vectors = torch.stack([w[1], blend[0], w[1]])
    for precision in ("fp32", "fp16"):
        pred.set_precision(precision)
        patched.set_precision(precision)
        assert torch.equal(pred(x, ts, vectors=vectors), patched(x, ts, labels=labels)), precision
    pred.set_precision("fp32")


def test_forward_refusals(dev):
    pred, T, _ = predictor_of("nocond", dev)
    x, ts, _ = forward_inputs(3, T, dev)
    labels = torch.tensor(LABELS, device=dev)
    rows = pred.class_embed.weight.detach()[labels]
    with pytest.raises(ValueError, match="not both"):
        pred(x, ts, labels=labels, vectors=rows)
    with pytest.raises(AssertionError):
        pred(x, ts)
    for bad in (rows[:, :64], rows[:2], torch.cat([rows, rows], dim=1), rows[0]):
        with pytest.raises(ValueError):
            pred(x, ts, vectors=bad)
    with pytest.raises(_native.NativeError):
        pred(x, ts, vectors=rows.cpu())
    plain = det_model(DiffusionModel("unet", 32), "spk.plain.").to(dev).predictor
    with pytest.raises(ValueError, match="class conditional"):
        plain(x, ts, vectors=rows)
    # the entry point itself: VQVS_ERR_ARG for a handle without labels, a NULL vector, a batch past the handle's
    plain(x, ts)
    out = torch.empty_like(x)
    L = _native.lib()
    with torch.cuda.device(dev):
        st = _native._stream_ptr()
        assert L.vqvs_unet_forward_vec(plain._handle.ptr, x.data_ptr(), ts.data_ptr(), None, rows.data_ptr(), out.data_ptr(), 3, T, st) == -1
        pred(x, ts, labels=labels)
        h = pred._handle.ptr
        assert L.vqvs_unet_forward_vec(h, x.data_ptr(), ts.data_ptr(), None, None, out.data_ptr(), 3, T, st) == -1
        assert L.vqvs_unet_forward_vec(h, x.data_ptr(), ts.data_ptr(), x.data_ptr(), rows.data_ptr(), out.data_ptr(), 3, T, st) == -1  # cond without cond_channels
        assert L.vqvs_unet_forward_vec(h, x.data_ptr(), ts.data_ptr(), None, rows.data_ptr(), out.data_ptr(), 4, T, st) == -1
        assert L.vqvs_unet_forward_vec(h, x.data_ptr(), ts.data_ptr(), None, rows.data_ptr(), out.data_ptr(), 3, 2 * T, st) == -1
        assert L.vqvs_unet_forward_vec(h, x.data_ptr(), ts.data_ptr(), None, rows.data_ptr(), out.data_ptr(), 3, T, st) == 0
    assert torch.equal(out, pred(x, ts, labels=labels))


# ---------------------------------------------------------------- 3. samplers and layouts
@pytest.fixture(scope="module")
def vqvae(dev):
    model = det_model(VQVAE(base_channels=32, pred_name="unet", num_labels=4)).to(dev)
    model.set_precision("fp32")
    return model


@pytest.fixture(scope="module")
def rows(vqvae):
    return vqvae.predictor.class_embed.weight.detach().clone()


@pytest.fixture(scope="module")
def clip(vqvae, dev):
    wave = (0.3 * seeded((2, 1, W), 31)).clamp(-1, 1).to(dev)
    return wave, vqvae.encode(wave), torch.tensor([2, 0], device=dev)


LENGTHS = (1500, 3000, 2 * H + W)  # 1, 2 and 3 windows of 2048 every 1536


@pytest.fixture(scope="module")
def waves(dev):
    return [(0.3 * seeded((1, 1, n), 71 + i)).clamp(-1, 1).to(dev) for i, n in enumerate(LENGTHS)]


@pytest.fixture(scope="module")
def codes(vqvae, waves):
    assert plan_pack(LENGTHS, W, H)[0] == [1, 2, 3]
    return [vqvae.encode_long(w, W, H) for w in waves]


@pytest.mark.parametrize("sampler", SAMPLERS)
def test_decode_and_invert_with_the_tables_rows(vqvae, rows, clip, sampler):
    wave, cds, labels = clip
    kw = dict(steps=STEPS, constrain=True, seed=9, clip_offset=4, sampler=sampler)
    want = vqvae.decode(cds, labels, **kw)
    assert torch.equal(vqvae.decode(cds, vectors=rows[labels], **kw), want)
    assert not torch.equal(vqvae.decode(cds, vectors=rows[labels.flip(0)], **kw), want)
    with pytest.raises(ValueError, match="not both"):
        vqvae.decode(cds, labels, vectors=rows[labels], **kw)
    if sampler == "ddim":
        assert torch.equal(vqvae.invert(wave, vectors=rows[labels], steps=STEPS), vqvae.invert(wave, labels, steps=STEPS))
        with pytest.raises(ValueError, match="not both"):
            vqvae.invert(wave, labels, vectors=rows[labels], steps=STEPS)


@pytest.mark.parametrize("sampler", SAMPLERS)
def test_decode_long_with_a_vector_per_window(vqvae, rows, codes, dev, sampler):
    """[A, a blend of A and B, B] over three windows against per-window labels on a copy whose table holds the three vectors."""
    assert plan_windows(LENGTHS[2], W, H)[0] == 3
    mix = S.voice_vectors(vqvae.predictor, ["1:0.5,2:0.5"])[0]
    vectors = torch.stack([rows[1], mix, rows[2]])
    patched = copy.deepcopy(vqvae)
    with torch.no_grad():
        patched.predictor.class_embed.weight[:3].copy_(vectors)
    kw = dict(num_samples=LENGTHS[2], window=W, hop=H, steps=STEPS, constrain=True, seed=9, clip_offset=3, sampler=sampler)
    want = patched.decode_long(codes[2], torch.tensor([0, 1, 2], device=dev), window_batch=2, **kw)
    for wb in (1, 2, 64):
        assert torch.equal(vqvae.decode_long(codes[2], vectors=vectors, window_batch=wb, **kw), want), (sampler, wb)
    assert not torch.equal(vqvae.decode_long(codes[2], vectors=torch.stack([rows[1], rows[1], rows[2]]), **kw), want)
    # one vector for every window is one label for every window
    assert torch.equal(vqvae.decode_long(codes[2], vectors=rows[2], **kw), vqvae.decode_long(codes[2], torch.tensor([2], device=dev), **kw))
    with pytest.raises(ValueError):
        vqvae.decode_long(codes[2], vectors=vectors[:2], **kw)
    with pytest.raises(ValueError, match="not both"):
        vqvae.decode_long(codes[2], torch.tensor([2], device=dev), vectors=vectors, **kw)


@pytest.mark.parametrize("sampler", SAMPLERS)
def test_a_pack_with_vectors_is_its_recordings_alone(vqvae, rows, codes, dev, sampler):
    counts = [1, 2, 3]
    kw = dict(window=W, hop=H, steps=STEPS, constrain=True, seed=9, sampler=sampler)
    voices = S.voice_vectors(vqvae.predictor, ["2", "0:0.25,3:0.75", "1"])
    alone = [vqvae.decode_long(codes[r], vectors=voices[r:r + 1], num_samples=LENGTHS[r], clip_offset=5 + r, **kw) for r in range(3)]
    per_window = voices.repeat_interleave(torch.tensor(counts, device=dev), dim=0)
    for wb, vec in ((2, voices), (64, voices), (2, per_window)):
        got = vqvae.decode_long_batch(torch.cat(codes), vectors=vec, counts=counts, num_samples=list(LENGTHS), clip_offset=5, window_batch=wb, **kw)
        for r in range(3):
            assert torch.equal(got[r], alone[r]), (sampler, wb, r)
    by_label = vqvae.decode_long_batch(torch.cat(codes), torch.tensor([2, 1], device=dev)[[0, 0, 1]], counts=counts, num_samples=list(LENGTHS), clip_offset=5, **kw)
    assert torch.equal(by_label[0], alone[0]) and torch.equal(by_label[2], alone[2]) and not torch.equal(by_label[1], alone[1])


@pytest.mark.parametrize("sampler", SAMPLERS)
def test_uncond_guidance_with_vectors_is_the_labels_run(vqvae, rows, clip, codes, dev, sampler):
    """The model's label 0 as the null label: labels name speakers 0..2, the vectors are their rows one up."""
    _, cds, labels = clip
    guide = dict(label_scale=2.0, vq_scale=0.5)
    kw = dict(steps=STEPS, constrain=True, seed=9, sampler=sampler)
    want = vqvae.decode_uncond_guidance(cds, labels, clip_offset=4, **guide, **kw)
    assert torch.equal(vqvae.decode_uncond_guidance(cds, vectors=rows[labels + 1], clip_offset=4, **guide, **kw), want)
    for g in (dict(label_scale=2.0), dict(vq_scale=0.5), dict()):
        assert torch.equal(vqvae.decode_uncond_guidance(cds, vectors=rows[labels + 1], clip_offset=4, **g, **kw),
                           vqvae.decode_uncond_guidance(cds, labels, clip_offset=4, **g, **kw)), g
    wl = torch.tensor([2, 0, 1], device=dev)
    lkw = dict(num_samples=LENGTHS[2], window=W, hop=H, clip_offset=3, window_batch=2, **guide, **kw)
    assert torch.equal(vqvae.decode_long_uncond_guidance(codes[2], vectors=rows[wl + 1], **lkw), vqvae.decode_long_uncond_guidance(codes[2], wl, **lkw))
    bkw = dict(counts=[1, 2, 3], num_samples=list(LENGTHS), window=W, hop=H, clip_offset=5, window_batch=2, **guide, **kw)
    want = vqvae.decode_long_batch_uncond_guidance(torch.cat(codes), wl, **bkw)
    got = vqvae.decode_long_batch_uncond_guidance(torch.cat(codes), vectors=rows[wl + 1], **bkw)
    assert all(torch.equal(a, b) for a, b in zip(got, want))
    with pytest.raises(ValueError, match="not both"):
        vqvae.decode_long_uncond_guidance(codes[2], wl, vectors=rows[wl + 1], **lkw)


def test_guided_calls_with_vectors_are_promoted(vqvae, rows, clip):
    _, cds, labels = clip
    kw = dict(num_samples=W, window=W, hop=H, steps=STEPS, constrain=True, seed=9, label_scale=2.0)
    want = vqvae.decode_long_uncond_guidance(cds[:1], vectors=rows[labels[:1] + 1], **kw)
    vqvae.set_precision("fp16")
    try:
        with pytest.warns(UserWarning, match="fp32 mode"):
            got = vqvae.decode_long_uncond_guidance(cds[:1], vectors=rows[labels[:1] + 1], **kw)
        assert vqvae.predictor.precision == "fp16" and torch.equal(got, want)
    finally:
        vqvae.set_precision("fp32")


# ---------------------------------------------------------------- 4. the scripts
def read_bytes(path):
    with open(path, "rb") as f:
        return f.read()


def write_wav(path, samples):
    os.makedirs(os.path.dirname(str(path)), exist_ok=True)
    w = ChunkWriter(str(path), 16000)
    w.write(np.asarray(samples, dtype=np.float32))
    w.close()


def read_wav(path):
    r = ChunkReader(str(path), 16000)
    try:
        return r.read(1 << 24)
    finally:
        r.close()


WINDOW_FLAGS = ["--window-seconds", "0.128", "--overlap-seconds", "0.032", "--sample-steps", "3"]


@pytest.fixture(scope="module")
def checkpoint(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("speakers") / "vqvae32.pt")
    det_model(VQVAE(base_channels=32, pred_name="unet", num_labels=4), "spk.scripts.").save(path)
    return path


def test_a_voice_from_a_recording(dev, checkpoint, tmp_path, capsys):
    """enroll_speaker.py --input-file -> sample_vqvae.py --voice @v.npy, against the same three steps of `SpeakerEnroller` here and
    sample_vqvae.py --label 4 on the checkpoint it writes."""
    sys.path.insert(0, ROOT)
    import enroll_speaker
    import sample_vqvae

    ref, src, voice = tmp_path / "ref.wav", tmp_path / "in.wav", tmp_path / "voices" / "v.npy"
    write_wav(ref, 0.3 * np.sin(2 * np.pi * 220.0 * np.arange(11000) / 16000.0))  # five clips of 2048 and a rest
    write_wav(src, 0.3 * np.sin(np.arange(16000) * 0.05))
    flags = ["--pretrained-path", checkpoint, "--steps", "3", "--batch-size", "2", "--seed", "0", "--seconds", "0.128", "--lr", "1e-2", "--init", "mean"]
    text = run_script("enroll_speaker.py", ["--input-file", ref, "--vector-out", voice, "--holdout", "1"] + flags)
    assert [ln.split(":")[0] for ln in text.splitlines() if ln.startswith("step ") and "loss=" in ln] == ["step 1", "step 2", "step 3"], text
    assert sorted(os.listdir(str(tmp_path / "voices"))) == ["v.json", "v.npy"]  # the voice file and its side-car: no checkpoint
    vec, meta = S.load_voice(str(voice))
    assert vec.shape == (128,) and meta["base_channels"] == 32 and meta["steps"] == 3 and meta["entries"] == 128 and meta["holdout_loss"] > 0

    model = VQVAE.load(checkpoint).to(dev).eval()
    clips = enroll_speaker.cut_clips([read_wav(ref)], 2048).to(dev)
    assert clips.shape[0] == 5
    held, train = enroll_speaker.split_holdout(5, 1, 0)
    en = SpeakerEnroller(model, 1, lr=1e-2, init="mean", seed=0)
    while en.steps < 3:
        epoch, at = divmod(en.steps, len(train) // 2)
        for batch in enroll_speaker.epoch_batches(train, 2, 0, epoch)[at:]:
            en.step(clips[batch], torch.zeros(2, dtype=torch.int64, device=dev), seed=0, clip_offset=en.steps * 2)
            if en.steps == 3:
                break
    assert np.array_equal(vec.view(np.int32), en.rows[0].cpu().numpy().view(np.int32)), "the voice file is not the enroller's row"
    grown = str(tmp_path / "grown.pt")
    torch.save(en.checkpoint(), grown)

    common = ["--input-file", str(src), "--seconds", "1", "--sample-steps", "3", "--seed", "9"]
    by_voice, by_label = tmp_path / "voice.wav", tmp_path / "label.wav"
    run_script("sample_vqvae.py", common + ["--voice", f"@{voice}", checkpoint, by_voice])
    sample_vqvae.main(common + ["--label", "4", grown, str(by_label)])  # (the other side in this process: one child fewer)
    assert read_bytes(by_voice) == read_bytes(by_label)
    capsys.readouterr()


def test_directory_mode_writes_a_voice_file_per_speaker(dev, checkpoint, tmp_path, capsys):
    """enroll_speaker.py data_dir --vectors-out DIR: the rows of the written checkpoint, bit for bit, named after the directories."""
    sys.path.insert(0, ROOT)
    import enroll_speaker

    for k, hz in enumerate((220.0, 330.0)):
        write_wav(tmp_path / "new" / f"spk{k}" / "a.wav", 0.3 * np.sin(2 * np.pi * hz * np.arange(11000) / 16000.0))
    out, voices = tmp_path / "added", tmp_path / "voices"
    enroll_speaker.main([str(tmp_path / "new"), "--pretrained-path", checkpoint, "--output-dir", str(out), "--vectors-out", str(voices), "--steps", "2",
                         "--batch-size", "2", "--seconds", "0.128", "--lr", "1e-2", "--init", "mean"])
    table = VQVAE.load(str(out / "model.pt")).predictor.class_embed.weight.detach()
    assert table.shape[0] == 6 and sorted(os.listdir(str(voices))) == ["spk0.json", "spk0.npy", "spk1.json", "spk1.npy"]
    for k in range(2):
        vec, meta = S.load_voice(str(voices / f"spk{k}.npy"))
        assert np.array_equal(vec.view(np.int32), table[4 + k].numpy().view(np.int32)) and meta["steps"] == 2 and "holdout_loss" not in meta
    capsys.readouterr()


FILES = (("s1/a.wav", 4800), ("s1/b.wav", 3200), ("s2/a.wav", 800))  # the first is about 2.5 windows of 2048 every 1536


def write_corpus(data):
    for i, (rel, n) in enumerate(FILES):
        write_wav(data / rel, 0.3 * np.sin(np.arange(n) * (0.05 + 0.01 * i)))
    return str(data / FILES[0][0])


def test_a_morph_along_a_file(dev, checkpoint, tmp_path, capsys):
    sys.path.insert(0, ROOT)
    import sample_vqvae

    first = write_corpus(tmp_path / "data")
    model = VQVAE.load(checkpoint).to(dev).eval()
    wave = torch.from_numpy(read_wav(first)[None, None]).to(dev)
    encoded = model.encode_long(wave, W, H)
    assert encoded.shape[0] == 3

    # a morph: no window centre (0.064, 0.16, 0.256 s) lies at or before 0 s or at or after 1 s, so every window is a blend
    points = [(0.0, "1"), (1.0, "2")]
    morph = tmp_path / "morph.wav"
    run_script("sample_vqvae.py", ["--input-file", first, "--seed", "9", "--whole-file", "--voice-at", "0:1", "--voice-at", "1:2", *WINDOW_FLAGS, checkpoint, morph])
    vectors = S.morph_vectors(model.predictor, points, 3, W, H, 16000)
    assert all(len(e) == 2 for e in S.morph_entries(points, 3, W, H, 16000))
    direct = model.decode_long(encoded, vectors=vectors, num_samples=4800, window=W, hop=H, steps=3, constrain=True, seed=9)
    write_wav(tmp_path / "direct.wav", direct.clamp(-1, 1).cpu().numpy().flatten())
    assert read_bytes(morph) == read_bytes(tmp_path / "direct.wav")
    one_voice = tmp_path / "label1.wav"
    sample_vqvae.main(["--input-file", first, "--seed", "9", "--whole-file", "--label", "1", *WINDOW_FLAGS, checkpoint, str(one_voice)])
    assert read_bytes(one_voice) != read_bytes(morph)
    capsys.readouterr()


def test_an_anonymised_corpus(dev, checkpoint, tmp_path, capsys):
    """Twice the same bytes, whatever the packing; file id 0 is what the single-file script writes under the tsv's spec."""
    sys.path.insert(0, ROOT)
    import convert_dataset
    import sample_vqvae

    data, files = tmp_path / "data", FILES
    first = write_corpus(data)
    a, b = tmp_path / "anon_a", tmp_path / "anon_b"
    argv = [checkpoint, str(data), "--anonymize", "2", "--seed", "9", *WINDOW_FLAGS]
    run_script("convert_dataset.py", argv[:2] + [a] + argv[2:] + ["--pack-windows", "4", "--window-batch", "2"])
    convert_dataset.main(argv[:2] + [str(b)] + argv[2:] + ["--pack-windows", "1"])
    for rel, _ in files:
        assert read_bytes(a / rel) == read_bytes(b / rel), rel
    assert read_bytes(a / "pseudo_voices.tsv") == read_bytes(b / "pseudo_voices.tsv")
    table = dict(line.split("\t") for line in (a / "pseudo_voices.tsv").read_text().splitlines())
    assert table == {d: S.pseudo_voice(9, d, 4, 2) for d in ("s1", "s2")}
    single = tmp_path / "single.wav"
    sample_vqvae.main(["--input-file", first, "--seed", "9", "--whole-file", "--voice", table["s1"], *WINDOW_FLAGS, checkpoint, str(single)])
    assert read_bytes(single) == read_bytes(a / files[0][0])
    other_seed = tmp_path / "anon_c"
    convert_dataset.main(argv[:2] + [str(other_seed)] + argv[2:4] + ["--seed", "10", *WINDOW_FLAGS])
    assert (other_seed / "pseudo_voices.tsv").read_text() != (a / "pseudo_voices.tsv").read_text()
    capsys.readouterr()
