"""VQ-VAE evaluation, host side: the argument checks of `vqvs_vq_quantize`, the code-usage statistics, the wrong-label draw,
StandardVQLoss against its own closed form, the training-only arguments of `VQVAE.losses`, and the script's flags and line
(none of this needs a device)."""
import ctypes as C
import re

import numpy as np
import pytest
import torch

from vq_voice_swap_amd import VQVAE, StandardVQLoss, _native, code_usage


def test_quantize_entry_point_refuses_bad_arguments_without_a_device(lib_built):
    L = lib_built
    assert "vqvs_vq_quantize" in _native.EXPORTS and hasattr(L, "vqvs_vq_quantize")
    buf = (C.c_double * 16)()
    p = C.cast(buf, C.c_void_p)
    ok = dict(z=p, dict=p, idx=p, emb=p, sq=p, hist=p, B=2, Cd=8, T1=4, K=3)

    def call(**kw):
        a = dict(ok, **kw)
        return L.vqvs_vq_quantize(a["z"], a["dict"], a["idx"], a["emb"], a["sq"], a["hist"], a["B"], a["Cd"], a["T1"], a["K"], None)

    for bad in (dict(z=None), dict(dict=None), dict(idx=None), dict(B=0), dict(B=-1), dict(Cd=0), dict(Cd=-4), dict(T1=0), dict(T1=-1),
                dict(K=0), dict(K=-2), dict(Cd=6),
                # the optional outputs may be NULL: the required ones are still checked
                dict(emb=None, sq=None, hist=None, z=None), dict(emb=None, sq=None, hist=None, K=0)):
        assert call(**bad) == -1, bad
        assert L.vqvs_last_error(), bad
    assert call(K=0) == -1 and b"K=0" in L.vqvs_last_error()
    assert call(z=None) == -1 and b"non-NULL" in L.vqvs_last_error()


def test_code_usage():
    for K in (1, 7, 512):
        u = code_usage(torch.full((K,), 3, dtype=torch.int64))
        assert u["used_codes"] == K and isinstance(u["used_codes"], int)
        assert abs(u["perplexity"] - K) <= 1e-12 * K
    one_hot = torch.zeros(130, dtype=torch.int64)
    one_hot[17] = 12345
    assert code_usage(one_hot) == {"used_codes": 1, "perplexity": 1.0}
    assert code_usage(torch.zeros(9, dtype=torch.int64)) == {"used_codes": 0, "perplexity": 0.0}
    # two bins 1 : 3 -> exp(-(.25 ln .25 + .75 ln .75)), zeros between them ignored
    u = code_usage(np.array([1, 0, 0, 3]))
    assert u["used_codes"] == 2 and u["perplexity"] == pytest.approx(np.exp(-(0.25 * np.log(0.25) + 0.75 * np.log(0.75))), rel=1e-14)
    with pytest.raises(ValueError):
        code_usage([1, -1])


def test_wrong_label_draw():
    import eval_vqvae

    for num_labels in (2, 3, 5, 251):
        labels = torch.arange(400) % num_labels
        seen = set()
        for first in (0, 4, 4000):
            w = eval_vqvae.wrong_labels(labels, num_labels, 7, first)
            assert w.dtype == torch.int64 and w.shape == labels.shape
            assert int(w.min()) >= 0 and int(w.max()) < num_labels
            assert not (w == labels).any()
            assert torch.equal(w, eval_vqvae.wrong_labels(labels, num_labels, 7, first))
            seen.add(tuple(w.tolist()))
        if num_labels > 2:
            assert len(seen) == 3  # other batches, other draws
            assert not torch.equal(eval_vqvae.wrong_labels(labels, num_labels, 8, 0), eval_vqvae.wrong_labels(labels, num_labels, 7, 0))
    with pytest.raises(ValueError):
        eval_vqvae.wrong_labels(torch.zeros(3, dtype=torch.int64), 1, 0, 0)


@pytest.mark.parametrize("commitment", [0.25, 0.0, 2.0])
def test_standard_vq_loss_forms_agree(commitment):
    g = torch.Generator().manual_seed(5)
    inputs, embedded = torch.randn(3, 68, 37, generator=g), torch.randn(3, 68, 37, generator=g)
    loss = StandardVQLoss(commitment)
    direct = loss(inputs, embedded, torch.zeros(4, 68))
    sq_err = ((inputs.double() - embedded.double()) ** 2).flatten(1).sum(1)
    fused = loss.from_sq_err(sq_err, inputs.numel())
    assert not direct.requires_grad
    assert abs(direct.item() - fused.item()) <= 1e-6 * fused.item()
    assert fused.item() == pytest.approx((1 + commitment) * ((inputs.double() - embedded.double()) ** 2).mean().item(), rel=1e-14)
    # gradients are never recorded, even for inputs that ask for them
    assert not loss(inputs.clone().requires_grad_(), embedded, None).requires_grad


def test_losses_refuses_training_only_arguments_before_a_device(lib_built):
    model = VQVAE(base_channels=32, pred_name="unet", num_labels=5, dictionary_size=16).eval()
    x = torch.zeros(2, 1, 4096)  # a CPU tensor: a device would be demanded next
    for kw in (dict(jitter=0.1), dict(no_vq_prob=0.5), dict(jitter=1.0, no_vq_prob=0.1)):
        with pytest.raises(ValueError, match="training-only"):
            model.losses(StandardVQLoss(), x, torch.zeros(2, dtype=torch.int64), **kw)
    with pytest.raises(RuntimeError, match="eval"):
        model.train().losses(StandardVQLoss(), x)
    with pytest.raises(_native.NativeError):  # with nothing left to object to, the CPU tensor is what stops it
        model.eval().losses(StandardVQLoss(), x)
    with pytest.raises(_native.NativeError):
        model.vq.quantize(torch.zeros(1, model.vq.num_channels, 4))


def test_eval_vqvae_flags_and_line():
    import eval_vqvae

    flags = sorted(s for a in eval_vqvae.arg_parser()._actions for s in (a.option_strings or [a.dest]) if s not in ("-h", "--help"))
    assert flags == sorted(["--batch-size", "checkpoint_path", "data_dir", "--precision", "--seed", "--max-samples", "--dist-backend"])
    args = eval_vqvae.arg_parser().parse_args(["--batch-size", "8", "ckpt.pt", "some/dir"])  # the reference's command line
    assert (args.batch_size, args.checkpoint_path, args.data_dir, args.precision, args.seed, args.max_samples) == (8, "ckpt.pt", "some/dir", "fp32", 0, None)
    assert eval_vqvae.arg_parser().parse_args(["m.pt", "tones"]).batch_size == 4

    state = eval_vqvae.EvalState(6, "cpu")
    ts = np.array([0.1, 0.3, 0.6, 0.9])
    state.cond.add(ts, np.array([1.0, 2.0, 3.0, 4.0]))
    state.rand.add(ts, np.array([1.5, 2.5, 3.5, 4.5]))
    state.num_samples, state.sq_err, state.numel = 4, state.sq_err + 8, 20
    state.hist += torch.tensor([2, 0, 2, 0, 0, 0])
    line = eval_vqvae.format_line(state.num_samples, state.log_dict())
    assert line == ("4 samples: cond_q0=1.000000 cond_q1=2.000000 cond_q2=3.000000 cond_q3=4.000000 rand_q0=1.500000 rand_q1=2.500000 "
                    "rand_q2=3.500000 rand_q3=4.500000 vq_loss=0.500000 used_codes=2 perplexity=2.000000")
    keys = re.findall(r"(\w+)=", line)
    assert keys == [f"cond_q{i}" for i in range(4)] + [f"rand_q{i}" for i in range(4)] + ["vq_loss", "used_codes", "perplexity"]
    # fewer than two labels: no rand_ keys
    bare = eval_vqvae.EvalState(6, "cpu")
    bare.cond.add(ts[:1], np.array([1.0]))
    assert list(bare.log_dict()) == ["cond_q0", "vq_loss", "used_codes", "perplexity"]
    # merging two states adds counts, sums and histograms
    other = eval_vqvae.EvalState(6, "cpu")
    other.hist += torch.tensor([0, 1, 0, 0, 0, 0])
    other.num_samples, other.sq_err, other.numel = 1, other.sq_err + 2, 5
    state.merge(other)
    assert (state.num_samples, float(state.sq_err), state.numel, state.hist.tolist()) == (5, 10.0, 25, [2, 1, 2, 0, 0, 0])


def test_shim_exports():
    import vq_voice_swap_amd
    from vq_voice_swap.vq import VQ as ShimVQ, StandardVQLoss as ShimLoss
    from vq_voice_swap_amd.vq import VQ

    assert ShimLoss is StandardVQLoss and ShimVQ is VQ
    for name in ("StandardVQLoss", "VQLoss", "code_usage"):
        assert name in vq_voice_swap_amd.__all__ and hasattr(vq_voice_swap_amd, name)
    assert callable(VQ.quantize) and callable(VQVAE.losses)
