"""Guidance-model evaluation, host side: the export and the argument checks of `vqvs_xent_score`, the shape / dtype / device
checks of `classification_scores`, the two scripts' flags, line and state merging, the fixtures' top-two logit gaps that the
device tests rely on, and the shim's exports (none of this needs a device)."""
import ctypes as C
import itertools
import os
import re
from fractions import Fraction

import numpy as np
import pytest
import torch

import vq_voice_swap_amd
from vq_voice_swap_amd import Classifier, Diffusion, EncoderPredictor, _native, classification_scores

from util import flags_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_symbol_is_exported_and_declared(lib_built):
    assert "vqvs_xent_score" in _native.EXPORTS and hasattr(lib_built, "vqvs_xent_score")
    header = open(os.path.join(ROOT, "include", "vqvs.h")).read()
    decl = re.search(r"int vqvs_xent_score\(([^;]*)\);", header)
    assert decl, "include/vqvs.h does not declare vqvs_xent_score"
    args = [a.strip() for a in " ".join(decl.group(1).split()).split(",")]
    assert args == ["const float* d_logits", "const int64_t* d_targets", "double* d_nll", "int64_t* d_top1", "int64_t* d_topk", "int k",
                    "int64_t* d_confusion", "int B", "int K", "int L", "void* stream"]
    assert len(lib_built.vqvs_xent_score.argtypes) == len(args)


def test_entry_point_refuses_bad_arguments_without_a_device(lib_built):
    L = lib_built
    buf = (C.c_double * 16)()
    p = C.cast(buf, C.c_void_p)
    ok = dict(logits=p, targets=p, nll=p, top1=p, topk=p, k=1, conf=p, B=2, K=3, L=4)

    def call(**kw):
        a = dict(ok, **kw)
        return L.vqvs_xent_score(a["logits"], a["targets"], a["nll"], a["top1"], a["topk"], a["k"], a["conf"], a["B"], a["K"], a["L"], None)

    for bad in (dict(logits=None), dict(targets=None), dict(nll=None), dict(B=0), dict(B=-1), dict(B=65536), dict(K=0), dict(K=-3),
                dict(K=8193), dict(L=0), dict(L=-1), dict(L=2 ** 24 + 1), dict(k=0), dict(k=-1), dict(k=4), dict(k=2, K=1),
                # the optional outputs may be NULL: the required ones and the sizes are still checked
                dict(top1=None, topk=None, conf=None, nll=None), dict(top1=None, topk=None, conf=None, K=0),
                dict(top1=None, conf=None, k=4)):
        assert call(**bad) == -1, bad
        assert L.vqvs_last_error(), bad
    assert call(K=8193) == -1 and b"8192" in L.vqvs_last_error()
    assert call(k=4) == -1 and b"k=4" in L.vqvs_last_error()
    assert call(logits=None) == -1 and b"non-NULL" in L.vqvs_last_error()


def test_classification_scores_checks_raise_before_a_device():
    lg2, lg3 = torch.zeros(3, 7), torch.zeros(3, 7, 5)
    t2, t3 = torch.zeros(3, dtype=torch.int64), torch.zeros(3, 5, dtype=torch.int64)
    for logits, targets, kw in (
            (torch.zeros(3), t2, {}), (torch.zeros(3, 7, 5, 2), t3, {}),               # logits of the wrong rank
            (lg2, t3, {}), (lg3, t2, {}), (lg3, torch.zeros(3, 4, dtype=torch.int64), {}), (lg2, torch.zeros(2, dtype=torch.int64), {}),
            (lg2.double(), t2, {}), (lg2.half(), t2, {}), (lg2, t2.int(), {}), (lg2, t2.float(), {}),   # dtypes
            (lg2, t2, dict(topk=0)), (lg2, t2, dict(topk=8)), (lg3, t3, dict(topk=-1)),
            (lg2, t2, dict(confusion=torch.zeros(7, 7, dtype=torch.int32))), (lg2, t2, dict(confusion=torch.zeros(7, 6, dtype=torch.int64))),
            (lg3, t3, dict(confusion=torch.zeros(49, dtype=torch.int64))), (lg2, t2, dict(confusion=torch.zeros(7, 14, dtype=torch.int64)[:, ::2])),
            (torch.zeros(2, 8193), torch.zeros(2, dtype=torch.int64), {}), (torch.zeros(0, 7), torch.zeros(0, dtype=torch.int64), {})):
        with pytest.raises(ValueError):
            classification_scores(logits, targets, **kw)
    # nothing left to object to but the device: there is no CPU path
    for logits, targets in ((lg2, t2), (lg3, t3)):
        with pytest.raises(_native.NativeError):
            classification_scores(logits, targets, topk=5, confusion=torch.zeros(7, 7, dtype=torch.int64))
    x, ts = torch.zeros(2, 1, 512), torch.zeros(2)
    with pytest.raises(_native.NativeError):
        Classifier(num_labels=3, base_channels=32).scores(x, ts, torch.zeros(2, dtype=torch.int64))
    with pytest.raises(_native.NativeError):
        EncoderPredictor(base_channels=32, downsample_rate=256, num_latents=8).scores(x, ts, torch.zeros(2, 2, dtype=torch.int64))
    with pytest.raises(_native.NativeError):
        Diffusion(vq_voice_swap_amd.make_schedule("exp")).sample_q_seeded(x, ts, seed=0)


COMMON_FLAGS = ["--batch-size", "checkpoint_path", "data_dir", "--precision", "--seed", "--max-samples", "--dist-backend"]


def test_script_flags():
    import eval_classifier
    import eval_enc_pred
    import eval_vqvae

    assert set(COMMON_FLAGS) == set(flags_of(eval_vqvae.arg_parser()))  # the flags the two scripts share with eval_vqvae.py
    assert flags_of(eval_classifier.arg_parser()) == sorted(COMMON_FLAGS + ["--schedule", "--t", "--topk", "--confusion-path"])
    assert flags_of(eval_enc_pred.arg_parser()) == sorted(COMMON_FLAGS + ["--topk", "--vq-vae-path"])
    a = eval_classifier.arg_parser().parse_args(["clf.pt", "some/dir"])
    assert (a.batch_size, a.precision, a.seed, a.max_samples, a.dist_backend, a.schedule, a.t, a.topk, a.confusion_path) == \
        (4, "fp32", 0, None, "nccl", "exp", None, 5, None)
    a = eval_classifier.arg_parser().parse_args(["--t", "0", "--topk", "3", "--schedule", "cos", "--confusion-path", "c.npy", "clf.pt", "tones"])
    assert (a.t, a.topk, a.schedule, a.confusion_path, a.checkpoint_path, a.data_dir) == (0.0, 3, "cos", "c.npy", "clf.pt", "tones")
    a = eval_enc_pred.arg_parser().parse_args(["--vq-vae-path", "vqvae.pt", "ep.pt", "tones"])
    assert (a.vq_vae_path, a.checkpoint_path, a.data_dir, a.batch_size, a.topk, a.precision) == ("vqvae.pt", "ep.pt", "tones", 4, 5, "fp32")
    with pytest.raises(SystemExit):
        eval_enc_pred.arg_parser().parse_args(["ep.pt", "tones"])  # the VQ-VAE is required
    assert eval_enc_pred.EvalState is eval_classifier.EvalState and eval_enc_pred.format_line is eval_classifier.format_line


def scores(nll, top1, topk, L):
    return {"nll": torch.tensor(nll, dtype=torch.float64), "top1": torch.tensor(top1), "topk": torch.tensor(topk), "positions": L}


def test_format_line_and_state():
    import eval_classifier

    state = eval_classifier.EvalState(7, "cpu", topk=5)
    ts = torch.tensor([0.1, 0.3, 0.6, 0.9])
    state.add_scores(ts, scores([1.0, 2.0, 3.0, 4.0], [1, 0, 1, 0], [1, 1, 1, 0], 1))
    state.confusion[2, 3] += 4
    line = eval_classifier.format_line(state.num_samples, state.log_dict())
    assert line == ("4 samples: nll_q0=1.000000 nll_q1=2.000000 nll_q2=3.000000 nll_q3=4.000000 acc_q0=1.000000 acc_q1=0.000000 acc_q2=1.000000 "
                    "acc_q3=0.000000 top5_q0=1.000000 top5_q1=1.000000 top5_q2=1.000000 top5_q3=0.000000 nll=2.500000 acc=0.500000")
    assert re.findall(r"(\w+)=", line) == [f"{p}_q{i}" for p in ("nll", "acc", "top5") for i in range(4)] + ["nll", "acc"]
    assert (state.num_samples, state.positions, state.correct, state.topk_correct, state.nll_sum) == (4, 4, 2, 3, Fraction(10))
    # k is clipped to the class count, and names the keys
    assert eval_classifier.EvalState(3, "cpu", topk=5).topk == 3 and eval_classifier.EvalState(3, "cpu", topk=5).top.prefix == "top3_"
    # positions: the trackers hold per-position means, the overall figures are over every position
    seq = eval_classifier.EvalState(512, "cpu", topk=5, confusion=False)
    assert seq.confusion is None
    seq.add_scores(torch.tensor([0.2, 0.7]), scores([250.0, 500.0], [25, 50], [100, 250], 250))
    log = seq.log_dict()
    assert (log["nll_q0"], log["nll_q2"], log["acc_q0"], log["acc_q2"], log["top5_q0"], log["top5_q2"]) == (1.0, 2.0, 0.1, 0.2, 0.4, 1.0)
    assert (log["nll"], log["acc"], seq.positions) == (1.5, 0.15, 500)
    assert eval_classifier.EvalState(3, "cpu").log_dict() == {"nll": 0.0, "acc": 0.0}
    # a fixed t: every clip at it; t = 1 belongs to the last quartile
    d = Diffusion(vq_voice_swap_amd.make_schedule("exp"))
    assert torch.equal(state.ts_for(d, 3, 8, 1, t=0.0), torch.zeros(3)) and torch.equal(state.ts_for(d, 3, 8, 1), d.draw_ts(3, 1, 8))
    last = eval_classifier.EvalState(3, "cpu")
    last.add_scores(state.ts_for(d, 2, 0, 0, t=1.0), scores([1.0, 1.0], [1, 1], [1, 1], 1))
    assert list(last.log_dict()) == ["nll_q3", "acc_q3", "top3_q3", "nll", "acc"]


def test_merging_shards_in_any_order_is_exact():
    import eval_classifier

    g = np.random.default_rng(3)
    shards = []
    for s in range(3):
        n, L = 5, 250
        # sums whose float additions round differently in different orders: the exact total must not
        nll = (g.random(n) * 10.0 ** g.integers(-8, 8, n)).tolist()
        top1 = g.integers(0, L + 1, n).tolist()
        shards.append((torch.from_numpy(g.random(n)), scores(nll, top1, [min(L, v + 3) for v in top1], L), g.integers(0, 9, (6, 6))))

    def build(order):
        states = []
        for i in order:
            st = eval_classifier.EvalState(6, "cpu", topk=5)
            st.add_scores(shards[i][0], shards[i][1])
            st.confusion += torch.from_numpy(shards[i][2])
            states.append(st.to_host())
        merged = states[0]
        for other in states[1:]:
            merged.merge(other)
        return merged

    base = build((0, 1, 2))
    assert base.num_samples == 15 and base.positions == 15 * 250
    assert base.nll_sum == sum(Fraction(v) for sh in shards for v in sh[1]["nll"].tolist())
    for order in itertools.permutations(range(3)):
        m = build(order)
        assert m.nll_sum == base.nll_sum and isinstance(m.nll_sum, Fraction)
        assert (m.num_samples, m.positions, m.correct, m.topk_correct) == (base.num_samples, base.positions, base.correct, base.topk_correct)
        assert torch.equal(m.confusion, base.confusion)
        a, b = m.log_dict(), base.log_dict()
        assert list(a) == list(b) and a["nll"] == b["nll"] and a["acc"] == b["acc"]
        for key in a:
            assert abs(a[key] - b[key]) <= 1e-12 * abs(b[key]), key


FIXTURE_LOGITS = [("f9_classifier32", "logits"), ("f15_custom_classifiers", "c_a.logits"), ("f15_custom_classifiers", "c_b.logits"),
                  ("f10_encpred32", "logits")]


def top_two_gap(logits: np.ndarray) -> np.ndarray:
    """Gap between the largest and the second largest logit of every position of [B, K] or [B, K, L] logits."""
    s = np.sort(logits.astype(np.float64), axis=1)
    return (s[:, -1] - s[:, -2]).reshape(-1)


@pytest.mark.parametrize("name,key", FIXTURE_LOGITS)
def test_fixture_logit_gaps_leave_room_for_the_top1_comparison(golden, name, key):
    """tests/test_guidance_eval_gpu.py compares top-1 hits with the fixture wherever the reference's top-two gap exceeds twice the
    device's logit error (of the order 1e-4 in the fp32 mode): the share of positions with a gap below 2e-3 must be under 5 %."""
    gap = top_two_gap(golden(name)[key])
    assert (gap < 2e-3).mean() < 0.05, (name, key, float((gap < 2e-3).mean()))


def test_shim_and_package_exports():
    from vq_voice_swap.loss_tracker import LossTracker as ShimTracker, classification_scores as shim_scores
    from vq_voice_swap.diffusion import Diffusion as ShimDiffusion
    from vq_voice_swap.models import Classifier as ShimClassifier, EncoderPredictor as ShimEncPred

    assert shim_scores is classification_scores and ShimTracker is vq_voice_swap_amd.LossTracker
    assert "classification_scores" in vq_voice_swap_amd.__all__ and vq_voice_swap_amd.classification_scores is classification_scores
    assert callable(ShimClassifier.scores) and callable(ShimEncPred.scores) and callable(ShimDiffusion.sample_q_seeded)
    assert ShimClassifier is Classifier and ShimEncPred is EncoderPredictor and ShimDiffusion is Diffusion
