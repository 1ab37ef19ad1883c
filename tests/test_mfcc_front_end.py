"""The MFCC front end of ConvMFCCEncoder (csrc/mfcc_kernels.hip: mfcc_logmel_kernel, mfcc_batch_max_kernel,
mfcc_features_kernel) held to a float64 reference of the whole front end (tests/mfcc_ref.py).

The reference builds the transform from torchaudio, so no fixture from the reference exists; what pins the front end is
  * CPU: the oracle (float32, torch.stft) against the float64 reference at 1e-5 of the feature range over the whole grid of
    inputs; the inputs are shown to do what they are for (the dB floor of version 2 binds on 15-70 % of the values of two
    families and never on equal-loudness noise); eight deliberately wrong references are shown to miss the GPU gate a hundredfold;
  * GPU: the feature rows of the HIP path against the float64 reference.  The gate is not a constant: per case it is
    8 * max(E_oracle, E_model) -- the oracle's own distance from float64 and the distance of a float32-rounding emulation of a
    correct kernel (mfcc_ref.Case) -- and never more than 1e-4 of the feature range.  Lengths sit on both sides of the 8-frame
    and 60-frame workgroup seams; batch coupling (dB variant: one maximum over the batch; log variant: none), handle reuse
    across batch sizes, run-to-run determinism and the lower bound of the length are checked on top.
Every GPU case prints its E_gpu, E_oracle, E_model and bound and appends them to mfcc_margins.jsonl in the directory VQVS_MARGINS_DIR
names (util.record_margin); a GPU run's file is kept as profiles/mfcc_margins.jsonl, its worst ratio in DESIGN.md section 4."""
import functools

import numpy as np
import pytest
import torch

from oracle import ref_cpu
from vq_voice_swap_amd import ConvMFCCEncoder, _native
from vq_voice_swap_amd.det_init import det_init_

from mfcc_ref import FAMILIES, FLOOR_MUTANTS, LENGTHS, MUTANTS, Case, buffers, front_end_case, make_batch
from util import record_margin, rel_rms

torch.set_num_threads(8)

# name -> (version, mu-law input); the first three are the encoders make_encoder builds, the fourth is what the constructor offers
ENCODERS = {"conv-mfcc-ulaw": (1, True), "conv-mfcc-ulaw-v2": (2, True), "conv-mfcc-linear": (1, False), "v2-linear": (2, False)}
FLOORED_FAMILIES = ("loud_quiet_tone", "tone_silence_square")
QUIET_CLIP = 1  # the 1e-3 clip of loud_quiet_tone, the silent clip of tone_silence_square


# ---------------------------------------------------------------- CPU


def test_buffers_of_module_and_oracle_agree():
    """The cases below are computed with ref_cpu.mfcc_buffers; the HIP path reads the module's buffers: the same tensors."""
    for version in (1, 2):
        sd = ConvMFCCEncoder(32, version=version).state_dict()
        for k, v in buffers(version).items():
            assert torch.equal(sd[k], v), (version, k)


@pytest.mark.parametrize("T", LENGTHS)
@pytest.mark.parametrize("enc_name", ENCODERS)
def test_oracle_vs_float64(enc_name, T):
    """All 39 rows.  Bound: the float32 FFT and float32 log of the oracle against exact arithmetic; the worst ratio measured over
    this grid is 2.6e-6 (conv-mfcc-linear, loud_quiet_tone)."""
    for family in FAMILIES:
        c = front_end_case(family, T, *ENCODERS[enc_name])
        assert c.oracle.shape == c.ref.shape == (3, 39, T // 160 + 1)
        assert bool(torch.isfinite(c.oracle).all()) and np.isfinite(c.ref).all(), (family, "not finite")  # silence included
        assert c.e_oracle <= 1e-5 * max(1.0, c.ref_max), (family, c.e_oracle, c.ref_max)
        # the condition on the GPU gate: if an input breaks it the input changes, not the cap
        assert c.gate <= c.cap, (family, c.gate, c.cap)
        assert c.e_model > 0.0  # the emulation rounds somewhere


@pytest.mark.parametrize("T", LENGTHS)
@pytest.mark.parametrize("ulaw", [True, False])
def test_inputs_make_the_db_floor_bind(ulaw, T):
    """Floored fraction of the log-mel values: 0.19 to 0.60 over the grid, with ONE exception that is recorded, not hidden:
    loud_quiet_tone without mu-law at T = 800 reaches 0.128.  Without the expansion the 1e-3 clip lies only 52 dB under the
    batch's maximum and is barely floored (0.04-0.07); the floored values are the tone's far bins, and at 6 frames two of them are edge
    frames, where the reflect padding breaks the tone's period and fills those bins.  That case (the dB variant without
    mu-law is no encoder make_encoder builds) is held to the per-clip properties only."""
    for family in FLOORED_FAMILIES:
        c = front_end_case(family, T, 2, ulaw)
        frac = c.floored_fraction()
        print(f"[floored] ulaw={ulaw} {family} T={T}: {frac:.3f}")
        if (ulaw, family, T) != (False, "loud_quiet_tone", 800):
            assert 0.15 <= frac <= 0.70, (family, frac)
        assert c.floored_fraction(QUIET_CLIP) > 0.0, family      # the quiet / silent clip is floored by the batch's maximum
        assert c.floored_fraction(0 if family == "loud_quiet_tone" else 2) < 1.0, family  # the loud clip keeps unfloored values
    # equal-loudness noise never reaches the floor: why that family alone pinned nothing about it
    assert front_end_case("noise", T, 2, ulaw).floored_fraction() == 0.0


def mutant_applies(mutant, family, version):
    if mutant in FLOOR_MUTANTS:
        return version == 2 and family in FLOORED_FAMILIES
    if mutant == "natural_log_db":
        return version == 2
    return True


@pytest.mark.parametrize("mutant", MUTANTS)
def test_gate_rejects_mutant(mutant):
    """A reference with one deliberate error must sit at least 100 gates away from the true one, else that case is no coverage
    for the property.  Required: coverage by at least three cases, at every length and for every encoder the property exists for."""
    covered, missed = [], []
    for enc_name, (version, ulaw) in ENCODERS.items():
        for family in FAMILIES:
            if not mutant_applies(mutant, family, version):
                continue
            for T in LENGTHS:
                c = front_end_case(family, T, version, ulaw)
                ratio = float(np.abs(c.mutant(mutant) - c.ref).max()) / c.gate
                (covered if ratio >= 100.0 else missed).append((enc_name, family, T, round(ratio, 1)))
    print(f"[mutant] {mutant}: {len(covered)} cases at >= 100 gates, weakest {min(covered, key=lambda r: r[3], default=None)}, not counted: {missed}")
    assert len(covered) >= 3, (mutant, covered, missed)
    assert {r[2] for r in covered} == set(LENGTHS), (mutant, "a length without coverage", missed)
    want_encoders = {n for n, (v, _) in ENCODERS.items() if any(mutant_applies(mutant, f, v) for f in FAMILIES)}
    assert {r[0] for r in covered} == want_encoders, (mutant, "an encoder without coverage", missed)


# ---------------------------------------------------------------- GPU


@functools.lru_cache(maxsize=None)
def hip_encoder(enc_name):
    """(encoder, state dict, prefix of the encoder's keys); one module and one native handle per encoder for the whole file."""
    version, ulaw = ENCODERS[enc_name]
    if enc_name == "v2-linear":
        enc = ConvMFCCEncoder(32, out_channels=512, input_ulaw=False, version=2).eval()
        det_init_((k, v) for k, v in enc.state_dict().items() if not k.startswith("mfcc."))
        sd, prefix = enc.state_dict(), ""
    else:
        from test_conv_mfcc import det_encoder

        model = det_encoder(enc_name)
        enc, sd, prefix = model.encoder, model.state_dict(), "encoder."
    assert (enc.version, enc.input_ulaw) == (version, ulaw)
    for k, v in buffers(version).items():
        assert torch.equal(sd[prefix + k], v), k
    enc.debug_taps = True
    enc.handle(torch.device("cuda:0"), 3, max(LENGTHS))  # sized once: no rebuild while the lengths grow
    return enc, {k: v.detach().clone() for k, v in sd.items()}, prefix


def run_hip(enc, wave):
    """[B, T] -> (z [B, 512, out_length], feature tap [B, 64, frames])."""
    B, T = wave.shape
    enc.debug_taps = True
    z = enc(wave[:, None, :].to("cuda:0")).cpu()
    h = enc._handle
    names = [n for n, _, _ in h.taps()]
    return z, h.read_tap(names.index("features"), B, T)


def hold(c: Case, enc, tag, record=False):
    """Run `c.wave` and hold the feature rows to the case's float64 reference.  Returns (z, tap, failure message or None)."""
    B, T = c.wave.shape
    z, tap = run_hip(enc, c.wave)
    assert z.shape == (B, 512, enc.out_length(T)) and bool(torch.isfinite(z).all()), tag
    assert tap.shape == (B, 64, T // 160 + 1), tag
    assert float(tap[:, 39:].abs().max()) == 0.0, (tag, "padding channels 39..63 are not zero")
    e_gpu, where = c.error(tap[:, :39])
    rec = {"case": tag, "B": B, "T": T, "frames": T // 160 + 1, "E_gpu": e_gpu, "E_oracle": c.e_oracle, "E_model": c.e_model,
           "bound": c.gate, "E_gpu_over_bound": e_gpu / c.gate, "max_ref": c.ref_max, "worst_at": where}
    if record:
        record_margin("mfcc_margins.jsonl", rec)
    else:
        print("[margin] " + str(rec))
    assert c.gate <= c.cap, (tag, c.gate, c.cap)
    return z, tap, (None if e_gpu <= c.gate else f"{tag}: E_gpu {e_gpu:.3e} > bound {c.gate:.3e} at {where}")


@pytest.mark.gpu
@pytest.mark.parametrize("T", LENGTHS)
@pytest.mark.parametrize("enc_name", ENCODERS)
def test_hip_features_vs_float64(enc_name, T):
    enc, sd, prefix = hip_encoder(enc_name)
    version, ulaw = ENCODERS[enc_name]
    failures = []
    for family in FAMILIES:
        c = front_end_case(family, T, version, ulaw)
        z, _, fail = hold(c, enc, f"{enc_name}/{family}/T={T}", record=True)
        if fail:
            failures.append(fail)
        if (T // 160 + 1) % 2:  # odd frame counts: the stride-2 convolution's pair view reads the zeroed padding row (blocks.1)
            want = ref_cpu.conv_mfcc_encoder(sd, c.wave[:, None, :], version=version, input_ulaw=ulaw, prefix=prefix)
            assert rel_rms(z, want) < 2e-3, (enc_name, family, T, rel_rms(z, want))
    assert not failures, failures


@pytest.mark.gpu
def test_db_floor_couples_the_batch_and_log_does_not():
    T = 9760
    batch = make_batch("loud_quiet_tone", T)
    quiet = batch[QUIET_CLIP:QUIET_CLIP + 1]
    # version 2: the floor is the maximum of the clips PRESENT minus 80 -- alone the quiet clip keeps values the batch floors
    enc, _, _ = hip_encoder("conv-mfcc-ulaw-v2")
    c_alone, c_batch = Case(quiet, 2, True), front_end_case("loud_quiet_tone", T, 2, True)
    _, f_alone, fail_a = hold(c_alone, enc, "coupling/v2/alone")
    _, f_batch, fail_b = hold(c_batch, enc, "coupling/v2/batch")
    assert not fail_a and not fail_b, (fail_a, fail_b)
    assert c_alone.floored_fraction() == 0.0 and c_batch.floored_fraction(QUIET_CLIP) > 0.5
    want = c_alone.ref[0] - c_batch.ref[QUIET_CLIP]
    got = (f_alone[0, :39] - f_batch[QUIET_CLIP, :39]).double().numpy()
    assert np.abs(want).max() >= 100.0 * (c_alone.gate + c_batch.gate)  # the coupling is far outside the gates
    assert np.abs(got - want).max() <= c_alone.gate + c_batch.gate, np.abs(got - want).max()
    # version 1 has no batch statistic: the same clip alone and inside the batch, bit for bit
    for name in ("conv-mfcc-ulaw", "conv-mfcc-linear"):
        enc, _, _ = hip_encoder(name)
        _, f_alone = run_hip(enc, quiet)
        _, f_batch = run_hip(enc, batch)
        assert torch.equal(f_alone[0], f_batch[QUIET_CLIP]), name


@pytest.mark.gpu
@pytest.mark.parametrize("enc_name", ["conv-mfcc-ulaw-v2", "conv-mfcc-ulaw"])
def test_handle_reuse_across_batch_sizes(enc_name):
    """One handle, large run first: a stale per-workgroup maximum or a leftover log-mel row of the larger run would show."""
    from test_conv_mfcc import det_encoder

    version, ulaw = ENCODERS[enc_name]
    enc = det_encoder(enc_name).encoder
    big = front_end_case("loud_quiet_tone", 19360, version, ulaw)
    runs = [("B3/T19360", big),
            ("B1/T800", Case(make_batch("loud_quiet_tone", 800)[QUIET_CLIP:QUIET_CLIP + 1], version, ulaw)),
            ("B2/T9919", Case(make_batch("loud_quiet_tone", 9919)[:2], version, ulaw))]
    handle = None
    for tag, c in runs:
        _, _, fail = hold(c, enc, f"reuse/{enc_name}/{tag}")
        assert not fail, fail
        assert handle is None or enc._handle is handle, "the handle was rebuilt: nothing was reused"
        handle = enc._handle


@pytest.mark.gpu
def test_features_are_deterministic():
    enc, _, _ = hip_encoder("conv-mfcc-ulaw-v2")
    wave = make_batch("tone_silence_square", 9760)
    z1, f1 = run_hip(enc, wave)
    z2, f2 = run_hip(enc, wave)
    assert torch.equal(f1, f2) and torch.equal(z1, z2)


@pytest.mark.gpu
def test_too_short_clip_is_rejected_and_handle_survives():
    """T = 799 is refused by vqvs_mfcc_encoder_forward on the host, before anything is enqueued (api.cpp: check_run, then the
    T < 800 test, then run_model); the handle serves the next call as if nothing had happened."""
    enc, _, _ = hip_encoder("conv-mfcc-ulaw-v2")
    c = front_end_case("tone_silence_square", 800, 2, True)
    _, before, fail = hold(c, enc, "short/before")
    assert not fail, fail
    handle = enc._handle
    with pytest.raises(_native.NativeError, match="too short"):
        enc(make_batch("tone_silence_square", 799)[:, None, :].to("cuda:0"))
    assert enc._handle is handle
    _, after, fail = hold(c, enc, "short/after")
    assert not fail, fail
    assert torch.equal(before, after)
